"""The redraw levels of the chained launch on the hardware (csrc/gen_draw.h, gen_draw_valid; gen_round, movedPick): picks that moved with
the domain's size pick again beside the helper wave's flush where the domain holds at least 10240 atoms per erased atom
(GEN_MOVED_PICK_ATOMS_PER_ERASED).  The chained run against the same chain stepped by two launches per batch (COGAPS_NO_CHAIN=1), bit
for bit, for the dense and the sparse kernel, at the headline matrix (20000 x 2000, K = 50), 30 iterations of the bench's chain: the A
domain passes 10240 atoms at iteration ~20 and 30720 (three atoms erased per launch) at ~28 -- 37 684 atoms after iteration 30 in the
sparse model by the oracle, more than 40000 in the dense one (test_headline_shape_stepwise) --, UINT32_MAX / size is ~10^5 there and
moves with every erased atom, so every launch of those iterations that erases an atom moves its picks, and the launches that erase
one to three take the new way.  The product build has no counter for it; the tests assert the domain's size, which is what opens it."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _run(hip_lib, data, sparse):
    from cogaps_amd import _capi
    S = _capi.Session(data, lib=hip_lib, nPatterns=50, nIterations=100, seed=42, sparseOptimization=sparse)
    for it in range(30):
        S.set_annealing(min(1.0, 2.0 * it / 100))
        nA, nP = S.draw_steps()
        S.iterate(nA, nP)
    st = []
    for w in "AP":
        a = S.atoms(w)
        st += [_sha(a["pos"]), _sha(a["mass"]), _sha(a["left"]), _sha(a["right"]), _sha(S.matrix(w)), _sha(S.ap(w)), str(S.natoms(w)), str(S.check_domain(w))]
        if sparse: st.append(_sha(S.rows(w)))
    out = st, (S.chained("A"), S.chained("P")), S.natoms("A")
    S.close()
    return out


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_chained_equals_two_launches_where_moved_picks_pick_again(hip_lib, monkeypatch, sparse):
    import bench
    data = bench.synthetic_dense(20000, 2000)
    if sparse: data = (data * (np.random.Generator(np.random.MT19937(5)).random(data.shape) >= 0.9)).astype(np.float32)
    a, form_a, n_a = _run(hip_lib, data, sparse)
    assert form_a[0] == 1 and (not sparse or form_a[1] == 1), "the chained launch did not run: %r" % (form_a,)
    assert n_a > 30720, "the A domain stayed below three times GEN_MOVED_PICK_ATOMS_PER_ERASED (%d atoms): the way under test was hardly taken" % n_a
    monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    b, form_b, _ = _run(hip_lib, data, sparse)
    assert form_b == (0, 0)
    assert a == b
