"""The sequential sampler (cogaps_params.sampler = COGAPS_SAMPLER_SEQUENTIAL, csrc/seq_kernel.h) on the test-only emulator: the reference's
SingleThreadedGibbsSampler, one workgroup per chain.

1. the reference build's recorded runs (tests/golden/refprobe_sequential_outputs.npz, tools/refprobe/record_sequential.py), digit for digit;
2. no result depends on SEQ_STEPS_PER_LAUNCH;
3. the reference's debug invariants after runs in the product arithmetic (lane-order sums);
4. a batch of chains gives every chain the bits it gives alone;
5. what is refused, and that asynchronousUpdates means what it meant."""
import numpy as np
import pytest

import sequential_cases as sc
from cogaps_amd import _capi

LANES = dict(sampler="sequential")


@pytest.fixture(scope="module")
def record():
    return sc.load_record()


@pytest.fixture(scope="module")
def all_cases(gist, modsim):
    return sc.cases(gist, modsim)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["modsim_k3", "gist_k7", "gist_rows300_k3", "gist_rows300_k3_fixedP", "tiny_5x6_k2", "gist_k4_pump_snapshots"])
def test_recorded_reference_runs(emul_lib, record, all_cases, name):
    """reductionMode seq + mathMode glibc-fma + sampler sequential against the reference build's own output: atom and chi2 histories,
    totalUpdates, meanChiSq, the statistics matrices (three rows each and a hash of every entry's bits), PUMP and snapshots."""
    data, kw = all_cases[name]
    sc.compare_with_record(record[name], _capi.run(data, lib=emul_lib(256), **sc.SEQ, **kw))


def test_the_tiny_case_reaches_the_domain_edges(emul_lib, all_cases):
    """what the 5 x 6 case is recorded for, shown on the chain itself (product arithmetic, same sizes): the domain below two atoms (a
    birth without a draw), an atom without a right neighbour (an exchange from it takes front()), and the index permutation intact"""
    data, kw = all_cases["tiny_5x6_k2"]
    s = _capi.Session(data, lib=emul_lib(256), **dict(kw, **LANES))
    try:
        few = 0
        for it in range(60):
            for w in "AP":
                few += s.natoms(w) < 2
            s.run_iterations(1, it, 1)
            for w in "AP":
                assert s.check_domain(w) == 0
                a = s.atoms(w)
                if a["pos"].size:
                    assert (a["right"] == 0xFFFFFFFF).sum() == 1 and (a["left"] == 0xFFFFFFFF).sum() == 1
        assert few >= 2
    finally:
        s.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib7(emul_lib):
    """an emulator variant whose launches end after seven steps: every update of more than seven steps takes several launches"""
    return emul_lib(256, extra="-DSEQ_STEPS_PER_LAUNCH=7", tag="_seqspl7")


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k in ("totalRunningTime", "samplerSeconds"):
            continue
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name", ["modsim_k3", "tiny_5x6_k2"])
@pytest.mark.parametrize("mode", ["seq", "lanes"])
def test_steps_per_launch_do_not_matter(emul_lib, lib7, all_cases, name, mode):
    data, kw = all_cases[name]
    kw = dict(kw, **(sc.SEQ if mode == "seq" else LANES))
    _same(_capi.run(data, lib=emul_lib(256), **kw), _capi.run(data, lib=lib7, **kw))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def _check_invariants(s, data_max, total_updates):
    """The reference's GAPS_DEBUG checks, on a session's state.
    * the domain's redundant state (links, index permutation, cached neighbour copies): cogaps_session_debug_check_domain;
    * every matrix entry against the sum of its bin's atom masses, within the reference's maximumDrift bound of 0.01;
    * the A*P cache against A * P^T recomputed in float64.  Tolerance: an update computes q = fl(p + fl(d * v)) with d = fl(new - old):
      three roundings, each of relative size u = 2^-24 on a magnitude of at most B, so an update adds at most 3 u B (1 + u) < 4 u B to
      an entry's error.  One proposal updates an entry at most twice (a move / exchange inside one row), and an entry of A*P is
      updated by the proposals of BOTH samplers (its row of A, its row of P; sync copies the cache from one sampler to the other
      without arithmetic), so after the whole run an entry has seen at most U = 2 * totalUpdates updates, and errors add linearly at
      worst: tol = 4 u B U.  B bounds |A*P| and |d * v| over the run: the chain fits A*P to the data, B = 2 * max(max data, max |A*P|
      at the end) is assumed.  float64 rounding of the recomputation (K products, relative 2^-53) is far below."""
    mats = {w: s.matrix(w).astype(np.float64) for w in "AP"}
    for w in "AP":
        assert s.check_domain(w) == 0
        m, n, k = s.dims(w)
        a = s.atoms(w)
        bin_len = (2 ** 64 - 1) // (m * k)
        bins = (a["pos"].astype(object) // bin_len).astype(np.int64) if a["pos"].size else np.zeros(0, np.int64)
        assert bins.size == 0 or (bins.min() >= 0 and bins.max() < m * k)
        sums = np.zeros(m * k)
        np.add.at(sums, bins, a["mass"].astype(np.float64))
        drift = np.abs(sums.reshape(m, k) - mats[w]).max()
        assert drift <= 0.01, (w, drift)
        assert (a["mass"] > 0).all() and mats[w].min() >= 0
    ap64 = mats["A"] @ mats["P"].T
    B = 2.0 * max(float(data_max), float(np.abs(ap64).max()))
    tol = 4.0 * 2.0 ** -24 * B * 2.0 * total_updates
    errA = np.abs(s.ap("P").astype(np.float64).T - ap64).max()      # the P sampler's cache: [samples][genes]
    errP = np.abs(s.ap("A").astype(np.float64) - ap64).max()
    print("A*P cache: max error %.3g / %.3g, tolerance %.3g (B = %.3g, %d proposals)" % (errA, errP, tol, B, total_updates))
    assert errA <= tol and errP <= tol


@pytest.mark.parametrize("name,iters", [("modsim", 60), ("gist", 12), ("synthetic_6000x8", 4)])
def test_debug_invariants_after_lane_order_runs(emul_lib, gist, modsim, name, iters):
    data = {"modsim": modsim, "gist": gist, "synthetic_6000x8": None}[name]
    if data is None:
        data = sc.synthetic_6000x8()
        assert emul_lib(256).cogaps_reduction_width(6000) == 2048      # N > 4096: two virtual lanes per thread
    s = _capi.Session(data, lib=emul_lib(256), nPatterns=3, seed=11, nIterations=iters, **LANES)
    try:
        upd = s.run_iterations(1, 0, iters)
        _check_invariants(s, data.max(), upd)
        upd += s.run_iterations(2, 0, iters)
        _check_invariants(s, data.max(), upd)
        assert s.avg_queue("A") == 0.0 and s.avg_queue("P") == 0.0
    finally:
        s.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_single_chains(emul_lib, lib7, modsim):
    """three chains in one launch per SEQ_STEPS_PER_LAUNCH steps (different seeds and pattern counts, one reduction width), and two
    chains with P fixed as a batch of their own (a batch shares its fixed matrix): every chain the bits it gives alone -- also where the
    launches end after seven steps, so that chains finish in different launches and a finished chain's workgroup leaves at once"""
    fixed = np.ascontiguousarray(0.2 + (np.arange(20 * 3).reshape(20, 3) % 5) * 0.3, dtype=np.float32)
    free = [dict(nPatterns=3, seed=1), dict(nPatterns=3, seed=2), dict(nPatterns=4, seed=3)]
    held = [dict(nPatterns=3, seed=4, whichMatrixFixed="P", fixedPatterns=fixed), dict(nPatterns=3, seed=5, whichMatrixFixed="P", fixedPatterns=fixed)]
    common = dict(nIterations=30, outputFrequency=10, **LANES)
    for lib in (emul_lib(256), lib7):
        for group in (free, held):
            together = _capi.run_batch([modsim] * len(group), lib=lib, kws=group, **common)
            for kw, r in zip(group, together):
                _same(r, _capi.run(modsim, lib=lib, **dict(common, **kw)))
                assert r["averageQueueLengthA"] == 0.0 and r["averageQueueLengthP"] == 0.0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def _refused(msg, fn):
    with pytest.raises(_capi.CogapsError) as e:
        fn()
    assert msg in str(e.value), str(e.value)


def test_refusals(emul_lib, modsim, tmp_path):
    lib = emul_lib(256)
    kw = dict(nPatterns=3, nIterations=4, seed=3)
    # a mixed batch
    _refused("cannot be mixed", lambda: _capi.run_batch([modsim, modsim], lib=lib, kws=[dict(sampler="sequential"), dict(sampler="async")], **kw))
    # the sparse model
    _refused("dense model only", lambda: _capi.Session(modsim, lib=lib, sparseOptimization=True, sampler="sequential", **kw))
    # the state file, in every way it can be asked for
    path = str(tmp_path / "chain.state")
    s = _capi.Session(modsim, lib=lib, sampler="sequential", **kw)
    try:
        s.run_iterations(1, 0, 2)
        _refused("sequential session", lambda: s.save_state(path))
        _refused("sequential session", lambda: s.load_state(path))
        _refused("sequential session", lambda: s.run_to_end(path, 1))
        assert s.position() == (1, 2)      # (refused before anything ran)
    finally:
        s.close()
    _refused("sequential session", lambda: _capi.run(modsim, lib=lib, sampler="sequential", stateFile=path, **kw))
    a = _capi.Session(modsim, lib=lib, **kw)      # (an asynchronous session's file is no way in either)
    try:
        a.save_state(path)
    finally:
        a.close()
    _refused("sequential session", lambda: _capi.run(modsim, lib=lib, sampler="sequential", stateFile=path, resume=True, **kw))
    # an unknown sampler value: the library's refusal (an integer passes the ctypes layer as it is), and the front ends' own
    _refused("sampler must be COGAPS_SAMPLER_ASYNC or COGAPS_SAMPLER_SEQUENTIAL", lambda: _capi.Session(modsim, lib=lib, sampler=2, **kw))
    with pytest.raises(ValueError, match="sampler must be"):
        _capi.make_params(lib, sampler="serial")
    from cogaps_amd import CogapsParams
    with pytest.raises(ValueError, match="sampler must be"):
        CogapsParams(sampler="serial")


def test_asynchronous_updates_mean_what_they_meant(emul_lib, modsim):
    """asynchronousUpdates = 0 stays refused outside a distributed call and stays accepted -- running the ASYNCHRONOUS sampler -- inside
    one; the default selector is the asynchronous sampler; CoGAPS(asynchronousUpdates=False) names the new selector"""
    lib = emul_lib(256)
    kw = dict(nPatterns=3, nIterations=6, seed=3, outputFrequency=3)
    p = _capi.make_params(lib)
    assert p.sampler == _capi.SAMPLER_ASYNC and p.asynchronousUpdates == 1
    _refused("asynchronousUpdates=FALSE", lambda: _capi.run(modsim, lib=lib, asynchronousUpdates=False, **kw))
    sub = dict(subsetIndices=np.arange(1, 16, dtype=np.uint32), subsetDim=1)
    worker = _capi.run(modsim, lib=lib, asynchronousUpdates=False, **kw, **sub)
    _same(worker, _capi.run(modsim, lib=lib, **kw, **sub))
    assert worker["averageQueueLengthA"] > 0.0
    seq = _capi.run(modsim, lib=lib, asynchronousUpdates=False, sampler="sequential", **kw, **sub)
    assert seq["averageQueueLengthA"] == 0.0 and seq["atomsA"].tolist() != worker["atomsA"].tolist()
    from cogaps_amd import CoGAPS
    with pytest.raises(ValueError, match='sampler="sequential"'):
        CoGAPS(modsim, nPatterns=3, nIterations=4, seed=3, asynchronousUpdates=False, messages=False)
