"""The chained launch's window drawn ahead of the decisions: which lanes draw again BESIDE the helper wave's flush (level 1) and which
behind it (level 2) -- csrc/gen_draw.h, gen_draw_valid.
A pick whose only fault is that its index moved with the domain's size picks again beside the flush; where its new slot or the record
it finds there is one the flush stores to (or it needs front()), the window is cut at that attempt and the second round draws it
(gen_round, movedPick).  The product takes that way where the domain holds at least GEN_MOVED_PICK_ATOMS_PER_ERASED atoms per erased
atom (10240: the cut stays rare); the domains a test on the emulator can afford are smaller, so the variant `moved` builds with that
bound at 0, and `moved_cut` adds -DGEN_TEST_MOVED_PICK_FLAG_EVERY=3, which cuts at every third moved pick whatever it read.
`moved_gate` builds with the bound at 64: the tests' domains hold a few hundred atoms and a launch erases one to a dozen, so the rule
n >= bound * m opens and closes the way from launch to launch, as 10240 does at the product's sizes.  `moved_forced` adds
-DGEN_AHEAD_BAD_EVERY=5 to the bound at 0: every fifth lane is sent to draw again whatever it read, the odd ones behind the flush (which
must keep a moved pick from taking the new way), the even ones at level 1 (a lane that moved AND carries a note).
(Births that read only what the flush leaves alone stay behind the flush: profiles/redraw_levels_cause_table.txt.)
On the fiber emulator (window 64), stepwise against the oracle; the test-only build counts the moved picks that picked again beside the
flush (GenScalars::prof[1]) and those that were cut (prof[3]).
The emulator runs fibers in turn: it checks that the lanes draw what the serial procedure draws, not the absence of a race with the
flush -- that argument stands in gen_round, and tests/test_redraw_levels_gpu.py runs the product kernels."""
import numpy as np
import pytest

import parity_util as pu

_VARIANTS = {
    "plain": ("", ""),
    "moved": ("-DGEN_MOVED_PICK_ATOMS_PER_ERASED=0", "_moved"),
    "moved_cut": ("-DGEN_MOVED_PICK_ATOMS_PER_ERASED=0 -DGEN_TEST_MOVED_PICK_FLAG_EVERY=3", "_movedcut"),
    "moved_gate": ("-DGEN_MOVED_PICK_ATOMS_PER_ERASED=64", "_movedgate"),
    "moved_forced": ("-DGEN_MOVED_PICK_ATOMS_PER_ERASED=0 -DGEN_AHEAD_BAD_EVERY=5", "_movedforced"),
}


def _lib(emul_lib, variant):
    extra, tag = _VARIANTS[variant]
    return emul_lib(64, extra=extra, tag=tag) if tag else emul_lib(64)


def _counters(lib, data, n, **kw):
    from cogaps_amd import _capi
    S = _capi.Session(data, lib=lib, nIterations=40, **kw)
    S.run_iterations(1, 0, n)
    tot = np.zeros(16, dtype=np.int64)
    chained = []
    for w in "AP":
        chained.append(bool(S.chained(w)))
        tot += np.array(S.debug_prof(w), dtype=np.int64)
    S.close()
    return chained, dict(moved_picks_beside_the_flush=int(tot[1]), moved_picks_cut=int(tot[3]),
                         held=int(tot[8]), behind_the_flush=int(tot[9]), level_1=int(tot[10]), later_rounds=int(tot[14] + tot[15]))


def _check(variant, c):
    if variant == "plain":
        assert c["moved_picks_beside_the_flush"] == 0 and c["moved_picks_cut"] == 0, c      # (small domains keep the join)
    elif variant in ("moved", "moved_gate", "moved_forced"):
        assert c["moved_picks_beside_the_flush"] > 0, c
    else:
        assert c["moved_picks_beside_the_flush"] > 0 and c["moved_picks_cut"] > 0, c
        # (every third moved pick is cut, and those the notes cut: at least a third of all of them, so at most two uncut ones per cut one)
        assert 3 * c["moved_picks_cut"] >= c["moved_picks_beside_the_flush"], c


@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_dense(emul_lib, variant):
    """1200 x 300, K = 3 (the shape of test_chained_launch_against_the_oracle: domains small enough that notes and size changes happen in
    most batches), 24 of 40 iterations."""
    lib = _lib(emul_lib, variant)
    data = pu.synthetic(1200, 300, seed=7)
    pu.run_stepwise(lib, data, 24, nPatterns=3, seed=123, total_iter=40, check_every=4)
    chained, c = _counters(lib, data, 24, nPatterns=3, seed=123)
    print(variant, c)
    assert chained == [True, True]
    assert c["held"] > 3000 and c["level_1"] >= c["moved_picks_beside_the_flush"] + c["moved_picks_cut"], c
    _check(variant, c)


@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_sparse(emul_lib, variant):
    """chain_sparse_kernel shares gen_draw_valid: the shape of test_sparse_chained_launch_two_proposals_per_evaluation_workgroup"""
    lib = _lib(emul_lib, variant)
    data = pu.synthetic_counts(600, 200, zeros=0.9, seed=5)
    pu.run_stepwise(lib, data, 30, total_iter=40, check_every=5, sparseOptimization=True, nPatterns=4, seed=11)
    chained, c = _counters(lib, data, 30, sparseOptimization=True, nPatterns=4, seed=11)
    print(variant, c)
    assert chained == [True, True]
    _check(variant, c)


@pytest.mark.parametrize("variant", ["moved"])
def test_tiny_domain(emul_lib, variant):
    """5 rows x 2 patterns (test_tiny_domain_hazards): the type depends on the count, UINT32_MAX / size moves with every erased atom.  With
    the bound at 0, the most permissive build.  (Its windows are never drawn ahead -- the counters it prints are zero in every variant --, so
    the run pins only that the build with the new way leaves such a chain as it was.)"""
    data = pu.synthetic(5, 6, rank=2, seed=3)
    lib = _lib(emul_lib, variant)
    pu.run_stepwise(lib, data, 150, nPatterns=2, seed=9, total_iter=100)
    from cogaps_amd import _capi
    S = _capi.Session(data, lib=lib, nPatterns=2, seed=9, nIterations=100)
    S.run_iterations(1, 0, 100)
    tot = sum(np.array(S.debug_prof(w), dtype=np.int64) for w in "AP")
    S.close()
    print(variant, dict(moved_picks_beside_the_flush=int(tot[1]), moved_picks_cut=int(tot[3]), held=int(tot[8]), behind_the_flush=int(tot[9]), level_1=int(tot[10])))
