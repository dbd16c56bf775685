"""The host side of the sampler update drivers (csrc/sampler_update.h, csrc/chain_batch.h) on the TEST-ONLY workgroup emulator: how many
launches an update enqueues, how many of them carry events while timing is on, how many batches they processed -- pinned per launch
form (chained, two launches per batch, split evaluation, sparse model, sequential sampler, one chain and a batch of chains) -- and how
a device error ends a chain of a batch.  The chains themselves are compared with the oracle in test_emul_parity.py; these counters
are what a change of the drivers' host code moves first.  The emulator has no graph replay: the replay arithmetic is pinned on the
hardware (test_gpu_parity.py)."""
import pytest

import parity_util as pu
from cogaps_amd import _capi

FIELDS = ("genLaunches", "evalLaunches", "batches", "genTimed", "evalTimed", "genNoopTimed", "evalNoopTimed", "proposalsQueued")


def dense():
    return pu.synthetic(1200, 300, seed=7), dict(nPatterns=3, seed=123), 20


def split():
    return pu.synthetic(6000, 8, seed=8), dict(nPatterns=3, seed=5), 3


def sparse():
    return pu.synthetic_counts(600, 200, zeros=0.9, seed=5), dict(nPatterns=4, seed=11, sparseOptimization=True), 30


def sequential():
    return pu.synthetic(60, 40, seed=9), dict(nPatterns=3, seed=4, sampler="sequential"), 10


# per sampler: FIELDS in order, then whether the last update ran as chained launches
ONE_CHAIN = {
    "dense": (dense, False, {"A": (0, 222, 163, 0, 21, 0, 7, 1108, True), "P": (0, 248, 146, 0, 18, 0, 13, 812, True)}),
    "dense_two_launches": (dense, True, {"A": (222, 222, 163, 21, 21, 7, 7, 1108, False), "P": (248, 248, 146, 18, 18, 13, 13, 812, False)}),
    "split": (split, False, {"A": (24, 24, 15, 1, 1, 2, 2, 38, False), "P": (33, 33, 24, 4, 4, 1, 1, 29, False)}),
    "sparse": (sparse, False, {"A": (0, 348, 259, 0, 34, 0, 10, 1927, True), "P": (0, 318, 212, 0, 30, 0, 10, 946, True)}),
    "sequential": (sequential, False, {"A": (0, 10, 0, 0, 10, 0, 0, 113, False), "P": (0, 10, 0, 0, 10, 0, 0, 92, False)}),
}


@pytest.mark.parametrize("case", sorted(ONE_CHAIN))
def test_one_chain_launch_counters(emul_lib, monkeypatch, case):
    """Session.perf(w) after n equilibration iterations with timing on, 64-attempt window"""
    make, no_chain, want = ONE_CHAIN[case]
    if no_chain: monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    data, kw, n = make()
    S = _capi.Session(data, lib=emul_lib(64), nIterations=40, **kw)
    S.set_timing(1)
    S.run_iterations(1, 0, n)
    got = {}
    for w in "AP":
        p = S.perf(w)
        got[w] = tuple(int(p[f]) for f in FIELDS) + (S.chained(w),)
    S.close()
    print(case, got)
    assert got == want


def dense_chain(c):
    return pu.synthetic(1200, 300, seed=7 + c), dict(nPatterns=3, seed=100 + c), 20


def sequential_chain(c):
    return pu.synthetic(60, 40, seed=9 + c), dict(nPatterns=3, seed=4 + c, sampler="sequential"), 10


# chain c's data, number of chains, COGAPS_NO_CHAIN; launches A / P, sampled A / P, per-chain [A, P] batches (None: a sequential sampler
# has none), chained
BATCH = {
    "three_chains": (dense_chain, 3, False, (278, 259), (69, 66), [[181, 141], [182, 146], [172, 140]], True),
    "three_chains_two_launches": (dense_chain, 3, True, (278, 259), (69, 66), [[181, 141], [182, 146], [172, 140]], False),
    "two_sequential_chains": (sequential_chain, 2, False, (10, 10), (10, 10), None, False),
}


@pytest.mark.parametrize("case", sorted(BATCH))
def test_batch_launch_counters(emul_lib, monkeypatch, case):
    """Batch.perf(side) and the chains' own batch counts after n iterations of the batch with timing on"""
    make, chains, no_chain, launches, sampled, batches, chained = BATCH[case]
    if no_chain: monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    lib = emul_lib(64)
    ss = []
    for c in range(chains):
        data, kw, n = make(c)
        ss.append(_capi.Session(data, lib=lib, nIterations=40, **kw))
    B = _capi.Batch(ss)
    B.set_timing(1)
    B.run_iterations(1, 0, n)
    perf = {w: B.perf(w) for w in "AP"}
    got_batches = [[int(S.perf(w)["batches"]) for w in "AP"] for S in ss]
    got_chained = [[S.chained(w) for w in "AP"] for S in ss]
    B.close()
    for S in ss: S.close()
    print(case, perf, got_batches, got_chained)
    assert tuple(perf[w]["launches"] for w in "AP") == launches
    assert tuple(perf[w]["sampled"] for w in "AP") == sampled
    if batches is not None:
        assert got_batches == batches
    assert got_chained == [[chained, chained]] * chains


def test_a_device_error_ends_one_chain_of_a_batch(emul_lib):
    """A lost hand-over inside a batch's chained launch (GAPS_ERR_SPIN, injected by the build variant of test_emul_parity's recovery test)
    is not recovered as a one-chain session's is: it ends the chain it happened in.  The update fails with the error code, the sampler
    and the chain's index; the batch is refused from then on; the chain's session is refused on its own too, the other chain's is not."""
    lib = emul_lib(64, extra="-DGEN_TEST_SPIN_FAIL_EPOCH=57", tag="_spinfail")
    data = pu.synthetic(1200, 300, seed=7)
    ss = [_capi.Session(data, lib=lib, nPatterns=3, nIterations=40, seed=123 + c) for c in range(2)]
    B = _capi.Batch(ss)
    with pytest.raises(_capi.CogapsError) as e:
        B.run_iterations(1, 0, 24)
    assert str(e.value) == "device error code 4 in sampler A of chain 1"
    with pytest.raises(_capi.CogapsError) as e:
        B.run_iterations(1, 0, 1)
    assert str(e.value) == "chain 1 of this batch was ended by a device error in an earlier update; the batch cannot be continued"
    B.close()
    with pytest.raises(_capi.CogapsError) as e:
        ss[1].update("A", 10)
    assert str(e.value) == "this session was ended by a device error in an earlier update; its chain cannot be continued"
    ss[0].update("A", 10)
    for S in ss: S.close()
