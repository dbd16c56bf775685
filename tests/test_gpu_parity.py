"""Parity tests proper: the HIP library (through the C ABI, on cuda:0) against the oracle on the same
seeded inputs, against the committed golden vectors, and -- at the BASELINE.json headline size -- through
size-independent invariants.  Integer results (atom counts, queue contents, bucket indices, PCG states)
and, in the matching reduction order, every float (masses, matrices, AP caches, chi2, posterior means)
must be bit-exact; the north-star tolerance for A/P posterior means is 1e-5 relative."""
import os

import numpy as np
import pytest

import parity_util as pu
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def test_library_is_the_hip_build(hip_lib):
    assert b"HIP gfx950" in hip_lib.cogaps_build_report()


def test_modsim_stepwise(hip_lib, modsim):
    pu.run_stepwise(hip_lib, modsim, 400, nPatterns=3, seed=42, total_iter=400, check_every=20)


def test_gist_stepwise(hip_lib, gist):
    a, p, props = pu.run_stepwise(hip_lib, gist, 120, nPatterns=7, seed=42, total_iter=200, check_every=10)
    assert props > 100000


@pytest.mark.parametrize("genes,samples,k", [(4100, 12, 3), (17000, 8, 3), (3000, 300, 5), (257, 129, 4), (70001, 6, 2)])
def test_wide_reductions(hip_lib, genes, samples, k):
    """evaluation workgroups of 256 / 1024 / 128 lanes and ragged vector lengths (N not a multiple of 4)"""
    pu.run_stepwise(hip_lib, pu.synthetic(genes, samples), 25, trace=(genes < 5000), nPatterns=k, seed=123, total_iter=50, check_every=5)


@pytest.mark.parametrize("genes,samples,k,iters,zeros", [(300, 50, 30, 60, 0.85), (9000, 40, 6, 25, 0.9), (2000, 3000, 50, 8, 0.95), (64, 64, 3, 200, 0.5)])
def test_sparse_model_stepwise(hip_lib, genes, samples, k, iters, zeros):
    """useSparseOptimization: bit-flag data vectors, HybridMatrix row / column copies, Z1 / Z2 tables, sparse chi2"""
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=genes + samples)
    pu.run_stepwise(hip_lib, data, iters, trace=genes * samples < 50000, nPatterns=k, seed=11, total_iter=max(iters, 40), check_every=5, sparseOptimization=True)


def _random_case(i):
    """shape, pattern count, sparsity and seeds of random case i (fixed generator: the cases are the same on every run)"""
    rng = np.random.Generator(np.random.MT19937(20260 + i))
    genes = int(rng.choice([rng.integers(20, 90), rng.integers(90, 700), rng.integers(700, 5000)]))
    samples = int(rng.choice([rng.integers(5, 40), rng.integers(40, 400), rng.integers(400, 1500)]))
    if genes * samples > 1500000:
        samples = max(5, 1500000 // genes)
    k = int(rng.integers(2, min(12, genes, samples) + 1))
    return genes, samples, k, bool(i % 3 == 2), int(rng.integers(1, 10000)), float(rng.choice([0.5, 0.8, 0.93]))


@pytest.mark.parametrize("case", range(40))
def test_random_shapes_stepwise(hip_lib, case):
    """Forty random problem shapes (ragged lengths, one- to many-wave reductions, a third of them through the sparse model),
    each stepwise against the oracle: proposal traces where the problem is small, atoms, matrices, A*P, chi2 after every check"""
    genes, samples, k, sparse, seed, zeros = _random_case(case)
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=seed) if sparse else pu.synthetic(genes, samples, seed=seed)
    iters = 80 if genes * samples < 200000 else 30
    pu.run_stepwise(hip_lib, data, iters, trace=genes * samples < 60000, nPatterns=k, seed=seed, total_iter=2 * iters, check_every=3, sparseOptimization=sparse)


def test_sparse_model_full_run(hip_lib, oracle):
    from cogaps_amd import _capi
    data = pu.synthetic_counts(400, 60, zeros=0.85, seed=33)
    kw = dict(nPatterns=5, nIterations=100, seed=42, outputFrequency=20, sparseOptimization=True)
    r = _capi.run(data, lib=hip_lib, **kw)
    o = oracle.run(data, math_mode=oracle.MATH_PORTABLE, redW_A=hip_lib.cogaps_reduction_width(60), redW_P=hip_lib.cogaps_reduction_width(400), redG=4, **kw)
    for f in ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP"):
        assert np.array_equal(r[f], o[f]), f
    assert r["totalUpdates"] == o["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"]
    # the reference's scalar order gives a statistically equivalent chain
    q = oracle.run(data, **kw)
    assert abs(q["meanChiSq"] - r["meanChiSq"]) / q["meanChiSq"] < 0.05


# ---------------------------------------------------------------------------------------------------------------------
# Verification mode (cogaps_params.reductionMode = SEQ, mathMode = GLIBC_FMA): the HIP library in the reference's own
# arithmetic.  These are the only tests that compare a GPU result with numbers the reference binary itself produced.
SEQ = dict(reductionMode="seq", mathMode="glibc-fma")


def test_device_math_modes(hip_lib):
    """logf / expf of the three math modes evaluated by a kernel: the glibc mode against the committed outputs of glibc 2.35's
    libm (tests/golden/glibc235_logf_expf.npz, tools/make_golden_r2.py), every mode against the same source run on the host"""
    from cogaps_amd import _capi
    g = np.load(os.path.join(GOLDEN, "glibc235_logf_expf.npz"))
    assert _capi.debug_math("log", g["x_log"], "glibc-fma", on_device=True).tobytes() == g["y_log"].tobytes()
    assert _capi.debug_math("exp", g["x_exp"], "glibc-fma", on_device=True).tobytes() == g["y_exp"].tobytes()
    rng = np.random.default_rng(1)
    xl = (rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.float32) / np.float32(4294967296.0))
    xe = -(rng.random(1 << 20, dtype=np.float32) * np.float32(100.0))
    for mode in ("portable", "glibc-fma", "glibc-sse2"):
        assert _capi.debug_math("log", xl, mode, on_device=True).tobytes() == _capi.debug_math("log", xl, mode).tobytes(), mode
        assert _capi.debug_math("exp", xe, mode, on_device=True).tobytes() == _capi.debug_math("exp", xe, mode).tobytes(), mode


@pytest.mark.parametrize("name", ["modsim", "gist"])
def test_reference_fingerprint_on_the_gpu(hip_lib, gist, modsim, name):
    """the atom histories, totalUpdates, meanChiSq and queue lengths the reference core printed for
    GIST.mtx K=7 / modsimdata K=3, seed 42, 1000+1000 iterations -- reproduced by cogaps_run on the GPU, plus every float of the
    committed reference-arithmetic golden run (posterior means and standard deviations, chi2 history)"""
    from cogaps_amd import _capi
    from test_oracle_pin import FINGERPRINTS
    fp = FINGERPRINTS[name]
    r = _capi.run(gist if name == "gist" else modsim, nPatterns=fp["k"], nIterations=1000, seed=42, outputFrequency=100, **SEQ)
    assert r["atomsA"].tolist() == fp["atomsA"] and r["atomsP"].tolist() == fp["atomsP"]
    assert r["totalUpdates"] == fp["totalUpdates"]
    assert abs(r["meanChiSq"] - fp["meanChiSq"]) < 6e-4
    assert abs(r["averageQueueLengthA"] - fp["qA"]) < 0.06 and abs(r["averageQueueLengthP"] - fp["qP"]) < 0.06
    g = np.load(os.path.join(GOLDEN, "%s_k%d_s42_i1000_seq.npz" % (name, fp["k"])))
    for f in ("Amean", "Pmean", "Asd", "Psd", "chisq"):
        assert np.array_equal(r[f], g[f]), f
    assert r["meanChiSq"] == float(g["meanChiSq"]) and r["averageQueueLengthA"] == float(g["avgQueueA"]) and r["averageQueueLengthP"] == float(g["avgQueueP"])
    # north-star tolerance for the posterior means: 1e-5 relative (met with zero difference)
    for f in ("Amean", "Pmean"):
        assert np.max(np.abs(r[f] - g[f]) / np.maximum(np.abs(g[f]), 1e-30)) <= 1e-5


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_reference_printed_outputs_on_the_gpu(hip_lib, gist, name):
    """the two further reference outputs of tests/test_oracle_pin.py (dense seed 123; the sparse model, seed 77): every printed
    digit, and every float of the golden run in the reference's arithmetic"""
    from cogaps_amd import _capi
    from test_oracle_pin import REFERENCE_PRINTED, check_reference_printed
    fp = REFERENCE_PRINTED[name]
    r = _capi.run(gist, **SEQ, **fp["kw"])
    check_reference_printed(r, fp)
    g = np.load(os.path.join(GOLDEN, fp["golden"]))
    for f in ("Amean", "Pmean", "Asd", "Psd", "chisq"):
        assert np.array_equal(r[f], g[f]), f
    assert r["meanChiSq"] == float(g["meanChiSq"])


def test_verification_mode_stepwise(hip_lib, gist):
    """verification mode against the oracle in the same arithmetic, batch by batch (traces, atoms, matrices, AP, chi2): dense with
    a user uncertainty matrix, wide vectors (several fold blocks, N not a multiple of 4), the sparse model with K above and
    below gaps::dot's 25-element order switch"""
    unc = np.maximum(gist * np.float32(0.15), np.float32(0.2)).astype(np.float32)
    pu.run_stepwise(hip_lib, gist, 40, nPatterns=5, seed=123, total_iter=60, check_every=10, **SEQ)
    pu.run_stepwise(hip_lib, gist, 20, trace=False, unc=unc, nPatterns=4, seed=5, total_iter=40, check_every=5, **SEQ)
    pu.run_stepwise(hip_lib, pu.synthetic(5003, 11), 8, trace=False, nPatterns=3, seed=9, total_iter=20, check_every=4, **SEQ)
    pu.run_stepwise(hip_lib, pu.synthetic_counts(300, 50, zeros=0.85, seed=350), 30, nPatterns=30, seed=11, total_iter=40, check_every=5, sparseOptimization=True, **SEQ)
    pu.run_stepwise(hip_lib, pu.synthetic_counts(900, 20, zeros=0.8, seed=9), 20, nPatterns=6, seed=12, total_iter=40, check_every=5, sparseOptimization=True, **SEQ)


def test_verification_mode_sparse_full_run(hip_lib, oracle):
    """cogaps_run in verification mode with the sparse model = the oracle's run in the same arithmetic, statistics and meanChiSq included
    (a sparse-model session holds the packed data only: the sequential meanChiSq reads the data through the flag words)"""
    from cogaps_amd import _capi
    data = pu.synthetic_counts(150, 30, zeros=0.8, seed=21)
    kw = dict(nPatterns=4, nIterations=40, seed=42, outputFrequency=10, sparseOptimization=True)
    r = _capi.run(data, lib=hip_lib, **SEQ, **kw)
    o = oracle.run(data, math_mode=oracle.MATH_GLIBC_FMA, **kw)
    for f in ("atomsA", "atomsP", "chisq", "Amean", "Pmean", "Asd", "Psd"):
        assert np.array_equal(r[f], o[f]), f
    assert r["totalUpdates"] == o["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"] and o["meanChiSq"] > 0


@pytest.mark.parametrize("case", range(40, 56))
def test_random_shapes_verification_mode(hip_lib, case):
    """sixteen more random shapes in the verification mode (the reference's scalar order, glibc's logf / expf) against the oracle
    in the same arithmetic, stepwise; the odd cases with glibc's non-fused (SSE2) variants"""
    genes, samples, k, sparse, seed, zeros = _random_case(case)
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=seed) if sparse else pu.synthetic(genes, samples, seed=seed)
    iters = 40 if genes * samples < 200000 else 12
    pu.run_stepwise(hip_lib, data, iters, trace=genes * samples < 60000, nPatterns=k, seed=seed, total_iter=2 * iters, check_every=4, sparseOptimization=sparse,
                    reductionMode="seq", mathMode="glibc-sse2" if case % 2 else "glibc-fma")


def test_user_uncertainty_stepwise(hip_lib, gist, modsim):
    """an uncertainty matrix given by the caller (DenseNormalModel.h:90-96): the kernels read S*S instead of recomputing it from D;
    fused evaluation (modsim, GIST A side) and the P side's 1363-element vectors, lane order, against the oracle"""
    unc = np.maximum(gist * np.float32(0.15), np.float32(0.2)).astype(np.float32)
    pu.run_stepwise(hip_lib, gist, 40, unc=unc, nPatterns=5, seed=8, total_iter=60, check_every=10)
    u2 = (np.maximum(modsim * 0.2, 0.05)).astype(np.float32)
    pu.run_stepwise(hip_lib, modsim, 100, unc=u2, nPatterns=3, seed=4, total_iter=100, check_every=25)
    wide = pu.synthetic(9000, 10, seed=77)      # split evaluation (alpha / apply kernels) with S*S read from memory
    pu.run_stepwise(hip_lib, wide, 12, trace=False, unc=np.maximum(wide * np.float32(0.3), np.float32(0.1)), nPatterns=3, seed=5, total_iter=20, check_every=4)


def test_pump_statistics_and_snapshots(hip_lib, modsim, oracle):
    """takePumpSamples (GapsStatistics.h:65-126) and nSnapshots / snapshotPhase (GapsStatistics.h:188-202, GapsRunner.cpp:316-322)
    through cogaps_run on the GPU against the oracle: dense and sparse model, the three snapshot phases"""
    from cogaps_amd import _capi
    for sparse, data in ((False, modsim), (True, pu.synthetic_counts(80, 24, zeros=0.7, seed=4)), (False, pu.synthetic(700, 30, seed=12))):
        kw = dict(nPatterns=3, nIterations=60, seed=42, outputFrequency=10, takePumpSamples=True, sparseOptimization=sparse)
        for phase, code in (("all", 0), ("equilibration", 1), ("sampling", 2)):
            r = _capi.run(data, lib=hip_lib, nSnapshots=4, snapshotPhase=phase, pumpThreshold="cut" if code == 1 else "unique", **kw)
            w_a, w_p = hip_lib.cogaps_reduction_width(data.shape[1]), hip_lib.cogaps_reduction_width(data.shape[0])
            o = oracle.run(data, math_mode=oracle.MATH_PORTABLE, redW_A=w_a, redW_P=w_p, redG=4, snapshotFrequency=15, snapshotPhase=code, **kw)
            for f in ("Amean", "Pmean", "Asd", "Psd", "pumpMatrix", "meanPatternAssignment", "equilibrationSnapshotsA", "equilibrationSnapshotsP",
                      "samplingSnapshotsA", "samplingSnapshotsP"):
                assert np.array_equal(r[f], o[f]), (sparse, phase, f)
            assert r["equilibrationSnapshotsA"].shape[0] == (4 if code != 2 else 0) and r["samplingSnapshotsP"].shape[0] == (4 if code != 1 else 0)
            assert np.allclose(r["pumpMatrix"].sum(axis=1), 1.0) and set(np.unique(r["meanPatternAssignment"])) <= {0.0, 1.0}


def test_headline_shape_stepwise(hip_lib):
    """BASELINE configs[2] itself -- 20000 x 2000, K = 50: the 512-thread fused evaluation (A side, 2000-element vectors) and
    the 8192-lane split evaluation (P side, 20000-element vectors) together, 30 iterations of the bench's chain against the
    lane-order oracle (OpenMP over the queue): Poisson step counts every iteration, atoms / matrices / AP / chi2 at the end"""
    import bench
    import pyoracle as po
    from cogaps_amd import _capi
    data = bench.synthetic_dense(20000, 2000)
    kw = dict(nPatterns=50, nIterations=100, seed=42)
    S = _capi.Session(data, lib=hip_lib, **kw)
    assert (hip_lib.cogaps_reduction_width(2000), hip_lib.cogaps_reduction_width(20000)) == (512, 8192)
    O = po.Session(data, omp=True, maxThreads=min(16, os.cpu_count() or 1), math_mode=po.MATH_PORTABLE, redW_A=512, redW_P=8192, redG=4, **kw)
    props = 0
    for it in range(30):
        t = min(1.0, 2.0 * it / 100)
        S.set_annealing(t), O.set_annealing(t)
        nA, nP = S.draw_steps()
        assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
        S.iterate(nA, nP), O.iterate(nA, nP)
        props += nA + nP
        assert (S.natoms("A"), S.natoms("P")) == (O.natoms("A"), O.natoms("P")), it
    assert props > 300000 and S.natoms("A") > 40000
    pu.assert_state_equal(S, O, "headline")
    # which launch form was tested: the A sampler (2000-element vectors, 512 evaluation threads) steps by chained launches
    # (csrc/chain_kernel.h), the P sampler (split evaluation) by gen_apply_kernel + eval_kernel<EVAL_DECIDE>
    assert S.chained("A") == 1 and S.chained("P") == 0
    S.close(), O.close()


def _chain_state(S):
    import hashlib
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = []
    for w in "AP":
        a = S.atoms(w)
        out += [sha(a["pos"]), sha(a["mass"]), sha(a["left"]), sha(a["right"]), sha(S.matrix(w)), sha(S.ap(w)), str(S.natoms(w)), str(S.check_domain(w))]
    return out


_CHAIN_AB = dict(genes=4000, samples=1600, nPatterns=20, nIterations=40, seed=11, iters=10)


def _chain_ab_run(lib):
    """4000 x 1600, K = 20: the A sampler's vectors have 1600 elements (512 evaluation threads: chained where the library allows it)"""
    from cogaps_amd import _capi
    c = _CHAIN_AB
    S = _capi.Session(pu.synthetic(c["genes"], c["samples"], rank=5, seed=3), lib=lib, nPatterns=c["nPatterns"], nIterations=c["nIterations"], seed=c["seed"])
    for it in range(c["iters"]):
        S.set_annealing(min(1.0, 2.0 * it / c["nIterations"]))
        nA, nP = S.draw_steps()
        S.iterate(nA, nP)
    st = _chain_state(S), S.chained("A")
    S.close()
    return st


def test_chained_equals_two_launches_on_the_gpu(hip_lib, monkeypatch):
    """The chained launch (one launch per batch: evaluation of batch b + generator of batch b + 1, csrc/chain_kernel.h) against the same
    chain stepped by two launches per batch (COGAPS_NO_CHAIN=1: gen_kernel, eval_kernel<EVAL_FUSED>) ON THE HARDWARE: atoms (positions,
    masses, links), factor matrices and A*P caches bit-equal, the domain consistent, and each session reports the form it ran."""
    chained, formA = _chain_ab_run(hip_lib)
    assert formA == 1, "the chained launch did not run: the hot path of the headline chain is untested on this device"
    monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    plain, formB = _chain_ab_run(hip_lib)
    assert formB == 0
    assert chained == plain


def test_sparse_chained_launch_with_long_queues_equals_two_launches_on_the_gpu(hip_lib, monkeypatch):
    """The sparse model's chained launch (chain_sparse_kernel) where its round-6 paths are taken ON THE HARDWARE: queues longer than the 255
    evaluation workgroups (the second group of four waves of a workgroup evaluates the proposal one grid further on, both groups passing
    through the workgroup's barriers side by side) and longer than the generator workgroup's 256 applier lanes (its attempt lanes carry
    out the slots behind theirs), and with the wide generator window such batches switch the sampler to (448 attempts).  80000 x 1200, 95 % zeros, K = 20 (a batch of the A sampler ends at the first repeated row: ~350 proposals
    once the domain is populated): stepped until the A sampler's batches average more than 256 proposals, then six iterations more; the same number of iterations with COGAPS_NO_CHAIN=1 (generator launch + eval_sparse_kernel,
    one proposal per workgroup, the decisions written by the evaluation workgroups) must leave the same bits: atoms, links, both copies of
    the HybridMatrix."""
    import bench
    from cogaps_amd import _capi
    data = bench.synthetic_dense(80000, 1200)
    data = (data * (np.random.Generator(np.random.MT19937(5)).random(data.shape) >= 0.95)).astype(np.float32)

    def run(n_fixed=None):
        S = _capi.Session(data, lib=hip_lib, nPatterns=20, nIterations=60, seed=23, sparseOptimization=True)
        it = 0; long_since = None; mean_q = 0.0
        while it < (n_fixed if n_fixed is not None else 60):
            S.set_annealing(min(1.0, 2.0 * it / 60))
            b0 = S.perf("A")
            nA, nP = S.draw_steps(); S.iterate(nA, nP); it += 1
            b1 = S.perf("A")
            mean_q = (b1["proposalsQueued"] - b0["proposalsQueued"]) / max(1, b1["batches"] - b0["batches"])
            if n_fixed is None and long_since is None and mean_q > 256.0: long_since = it
            if n_fixed is None and long_since is not None and it >= long_since + 6: break
        st = _chain_state(S) + [sha_rows(S)], (S.chained("A"), S.chained("P")), it, mean_q, long_since, S.generator_window("A")
        S.close()
        return st

    def sha_rows(S):
        import hashlib
        return hashlib.sha256(np.ascontiguousarray(S.rows("A")).tobytes() + np.ascontiguousarray(S.rows("P")).tobytes()).hexdigest()

    a, form_a, n, mean_q, long_since, win_a = run()
    assert form_a == (1, 1), "the sparse model's chained launch did not run"
    assert long_since is not None and mean_q > 256.0, "the A sampler's queues stayed short (mean %.1f after %d iterations): the paths under test were not taken" % (mean_q, n)
    monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    assert win_a == 448, win_a      # (batches beyond 230 proposals: the chained sparse launch's wide window, seven attempt waves)
    b, form_b, _, _, _, win_b = run(n)
    assert form_b == (0, 0) and win_b == 256
    assert a == b


@pytest.mark.parametrize("genes,samples,k,iters,zeros", [(3000, 700, 6, 24, 0.9), (900, 20000, 4, 8, 0.95)])
def test_sparse_wide_generator_window_stepwise(hip_lib, monkeypatch, genes, samples, k, iters, zeros):
    """chain_sparse_kernel<448, .> -- the sparse model's chained launch with seven attempt waves and the helper wave as its only applier wave, the
    attempt lanes carrying out the queue behind its 64 slots -- taken from the first update on (COGAPS_TEST_WIDE_WINDOW) and compared with the
    oracle proposal by proposal and state by state; both evaluation forms (one-round vectors with two groups per workgroup; the wide form:
    20000-element vectors for the P sampler)."""
    from cogaps_amd import _capi
    monkeypatch.setenv("COGAPS_TEST_WIDE_WINDOW", "1")
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=genes % 97)
    pu.run_stepwise(hip_lib, data, iters, trace=genes * samples < 50000, nPatterns=k, seed=19, total_iter=max(iters, 40), check_every=4, sparseOptimization=True)
    S = _capi.Session(data, lib=hip_lib, nPatterns=k, nIterations=40, seed=19, sparseOptimization=True)
    S.run_iterations(1, 0, 4)
    wins = [S.generator_window(w) for w in "AP"], [S.chained(w) for w in "AP"]
    S.close()
    assert wins == ([448, 448], [1, 1]), wins


def test_launch_clock_of_chained_launches(hip_lib):
    """cogaps_session_launch_clock: the chip-wide clock read inside EVERY chained launch since set_timing(1) (replayed graphs included) --
    as many launches as the sampler generated batches in the window (one launch per batch; the update's first launch evaluates nothing
    and is not counted), plausible durations, ordered percentiles; nothing for a sampler that does not chain."""
    from cogaps_amd import _capi
    c = _CHAIN_AB
    S = _capi.Session(pu.synthetic(c["genes"], c["samples"], rank=5, seed=3), lib=hip_lib, nPatterns=c["nPatterns"], nIterations=c["nIterations"], seed=c["seed"])
    for it in range(6):
        nA, nP = S.draw_steps(); S.iterate(nA, nP)
    S.set_timing(True)
    b0 = S.perf("A")["batches"]
    for it in range(6):
        nA, nP = S.draw_steps(); S.iterate(nA, nP)
    batches = S.perf("A")["batches"] - b0
    a, p, per = S.launch_clock("A"), S.launch_clock("P"), S.launch_period("A")
    S.close()
    assert S_chained_ok(a, batches), (a, batches)
    assert p["launches"] == 0 and p["mean_us"] == 0.0
    # the launch-to-launch period brackets the launch and what the dispatcher does around it: longer than the launch, not by much (here the
    # launches are few and sent call by call, ~5 us apart; inside a replayed graph the difference is ~1.8 us)
    assert 0.5 * a["launches"] < per["launches"] <= a["launches"] and a["mean_us"] < per["mean_us"] < a["mean_us"] + 15.0, (a, per)


def S_chained_ok(a, batches):
    return (0.9 * batches <= a["launches"] <= batches and 3.0 < a["mean_us"] < 200.0
            and 0 < a["p10_us"] <= a["p50_us"] <= a["p75_us"] <= a["p90_us"] <= a["p99_us"] < 2000.0)


def test_chained_split_evaluation_equals_two_launches_on_the_gpu(hip_lib, monkeypatch):
    """The same for the split evaluation inside the chained launch (EVAL_CHAIN_SPLIT: data vectors of more than 4096 elements -- slices,
    a deciding workgroup per proposal, the A*P updates taken up by the evaluation workgroups behind their slices): 9000 x 1500, K = 12 --
    the P sampler's vectors have 9000 elements (5 slices of 512 threads), the A sampler's 1500 (fused) -- taken with COGAPS_CHAIN_SPLIT=1 (it is
    not the default: measured slower, profiles/r05_ab_chained_split_evaluation_not_kept.txt) against the default (gen_apply_kernel +
    eval_kernel<EVAL_DECIDE>) and against COGAPS_NO_CHAIN=1, bit for bit."""
    from cogaps_amd import _capi
    def run():
        S = _capi.Session(pu.synthetic(9000, 1500, rank=4, seed=5), lib=hip_lib, nPatterns=12, nIterations=30, seed=17)
        for it in range(8):
            S.set_annealing(min(1.0, 2.0 * it / 30))
            nA, nP = S.draw_steps()
            S.iterate(nA, nP)
        st = _chain_state(S), S.chained("A"), S.chained("P")
        S.close()
        return st
    monkeypatch.setenv("COGAPS_CHAIN_SPLIT", "1")
    a = run()
    assert (a[1], a[2]) == (1, 1), "the split evaluation did not chain"
    monkeypatch.delenv("COGAPS_CHAIN_SPLIT")
    b = run()
    assert (b[1], b[2]) == (1, 0)
    monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    c = run()
    assert (c[1], c[2]) == (0, 0)
    assert a[0] == b[0] == c[0]


def test_chained_launch_with_half_the_compute_units(hip_lib):
    """`Correct and slower, never a hang` as a hardware fact.  The same chain in processes whose queues may use 120 of the 256 compute
    units (HSA_CU_MASK): (1) as the library decides; (2) with COGAPS_FORCE_CHAIN=1 the chained launch whatever the runtime reports --
    its 241 workgroups are then NOT all resident at once: the generator workgroup (the launch's first since round 6) holds one unit and waits
    while the evaluation workgroups, which never wait, run in turns on the others.  Both must finish and equal the unmasked run bit for bit."""
    import subprocess, sys, json
    ref, formA = _chain_ab_run(hip_lib)
    assert formA == 1
    here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
    code = ("import sys, json; sys.path[:0] = [%r, %r, %r]\n"
            "import test_gpu_parity as T\nfrom cogaps_amd import _capi\nimport time\nt0 = time.time()\n"
            "st, form = T._chain_ab_run(_capi.load())\nprint(json.dumps({'state': st, 'form': form, 'seconds': time.time() - t0}))\n"
            % (here, root, os.path.join(root, "oracle")))
    for force in (False, True):
        env = dict(os.environ, HSA_CU_MASK="0:0-119")
        env.pop("COGAPS_NO_CHAIN", None)
        if force: env["COGAPS_FORCE_CHAIN"] = "1"
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        print("120 compute units, force=%s: %.1f s, chained=%d" % (force, rec["seconds"], rec["form"]))
        # (whether the mask lowers the compute-unit count the runtime reports -- and so closes the library's gate -- depends on the driver:
        # unforced, either form may run; forced, the chained one must)
        assert rec["form"] == 1 or not force
        assert rec["state"] == ref


def test_chained_launch_beside_a_foreign_kernel(hip_lib):
    """The hand-over inside the chained launch while ANOTHER process keeps the GPU busy (tools/dev_soak.py: a 4 GiB tensor scaled in place,
    back to back, on its own HIP context): the chained launch's workgroups -- 136 KB of LDS and a full register file each -- are scheduled
    late, the generator's bounded wait must still hold.  The headline shape's first 36 iterations (~40 000 chained launches), first alone,
    then disturbed: no hand-over runs out (cogaps_session_chain_recoveries == 0: nothing had to be completed by chain_recover_kernel), both
    samplers stay in the chained form where they took it, and the disturbed run ends in the state of the quiet one, bit for bit.
    (The million-launch run of the same tool is profiles/r06_soak_beside_a_foreign_kernel.json.)"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dev_soak", os.path.join(root, "tools", "dev_soak.py"))
    soak = importlib.util.module_from_spec(spec); spec.loader.exec_module(soak)
    import bench
    data = bench.synthetic_dense(20000, 2000)
    params = dict(nPatterns=50, seed=42, outputFrequency=10)
    quiet = soak.run(data, 100, 36, params)
    disturbed = soak.run(data, 100, 36, params, foreign_seconds=max(30.0, 4.0 * quiet["seconds"]))
    print("quiet %.1f s, beside the foreign kernels %.1f s (%s); A launch period p99 %.1f -> %.1f us" % (
        quiet["seconds"], disturbed["seconds"], disturbed.get("foreign"), quiet["A"]["launch_period_us"]["p99_us"], disturbed["A"]["launch_period_us"]["p99_us"]))
    assert quiet["A"]["chained"] and disturbed["A"]["chained"]
    assert sum(r[w]["recoveries"] for r in (quiet, disturbed) for w in "AP") == 0
    assert disturbed["state_digest"] == quiet["state_digest"] and disturbed["proposals"] == quiet["proposals"]


def test_plain_c_client_equals_the_ctypes_path(hip_lib, gist):
    """the Rcpp-shaped C program (tests/c/rcpp_shim_test.c: allParams keys -> cogaps_params by the rules of src/Cogaps.cpp:64-139,
    then cogaps_run / cogaps_run_from_file, no Python in the process) prints the result cogaps_run gives through ctypes; a
    distributed worker call (subsetDim > 0) is accepted with R's forced asynchronousUpdates = FALSE (R/DistributedCogaps.R:28-29)"""
    import subprocess
    from cogaps_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "c", "rcpp_shim_test.bin")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "tests", "c")])

    def parse(txt):
        d = {}
        for ln in txt.splitlines():
            k, _, v = ln.partition(" ")
            d[k] = v
        return d
    mtx = os.path.join(GOLDEN, "GIST.mtx")
    for entry in ("matrix", "file"):
        out = subprocess.run([exe, mtx, "entry=" + entry, "nPatterns=4", "nIterations=60", "seed=9", "outputFrequency=20", "messages=0", "nSnapshots=3",
                              "snapshotPhase=all", "takePumpSamples=1"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        d = parse(out.stdout)
        r = _capi.run(gist, nPatterns=4, nIterations=60, seed=9, outputFrequency=20, nSnapshots=3, snapshotPhase="all", takePumpSamples=True)
        assert [int(x) for x in d["atomsA"].split()] == r["atomsA"].tolist() and [int(x) for x in d["atomsP"].split()] == r["atomsP"].tolist()
        assert int(d["totalUpdates"]) == r["totalUpdates"] and np.float32(d["meanChiSq"]) == np.float32(r["meanChiSq"])
        assert [np.float32(x) for x in d["chisq"].split()] == r["chisq"].tolist()
        seqsum = lambda m: float(np.cumsum(m.astype(np.float64).ravel())[-1])          # left to right, as the C program adds
        assert float(d["sumAmean"]) == seqsum(r["Amean"]) and float(d["sumPsd"]) == seqsum(r["Psd"]) and float(d["sumPmean"]) == seqsum(r["Pmean"])
        assert d["snapshots"] == "3 3 pump 1" and "HIP gfx950" in d["buildReport"]
    # callInternalCoGAPS: subset + asynchronousUpdates = FALSE + workerID
    out = subprocess.run([exe, mtx, "nPatterns=3", "nIterations=40", "seed=5", "outputFrequency=20", "subsetDim=1", "subsetIndices=1:300", "asynchronousUpdates=0",
                          "workerID=2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    d = parse(out.stdout)
    r = _capi.run(gist, nPatterns=3, nIterations=40, seed=5, outputFrequency=20, subsetIndices=np.arange(1, 301, dtype=np.uint32), subsetDim=1, workerID=2)
    assert d["nGenes"].split()[0] == "300" and int(d["totalUpdates"]) == r["totalUpdates"] and [int(x) for x in d["atomsA"].split()] == r["atomsA"].tolist()
    assert "worker 2 is starting!" in out.stdout and "worker 2 is finished!" in out.stdout      # GapsRunner.cpp:428-433, 494-500
    bad = subprocess.run([exe, mtx, "nPatterns=3", "nIterations=10", "asynchronousUpdates=0"], capture_output=True, text=True, timeout=600)
    assert bad.returncode == 1 and "asynchronousUpdates=FALSE" in bad.stderr
    # a worker reading its subset from the FILE (cogaps_from_file_cpp with subsetIndices): only rows 1..300 are ever read (Matrix.cpp:70-134)
    out = subprocess.run([exe, mtx, "entry=file", "nPatterns=3", "nIterations=40", "seed=5", "outputFrequency=20", "subsetDim=1", "subsetIndices=1:300", "asynchronousUpdates=0",
                          "workerID=2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    d2 = parse(out.stdout)
    assert d2["nGenes"].split()[0] == "300" and int(d2["totalUpdates"]) == r["totalUpdates"] and d2["atomsA"] == d["atomsA"] and d2["sumAmean"] == d["sumAmean"]
    # Rcpp::checkUserInterrupt() (GapsRunner.cpp:280) as the interrupt callback: raised at the 25th poll of a 40 + 40 iteration run, the
    # run ends there -- exactly 25 polls, status 1, the library's message, no result -- through both entry points; a later run in a
    # fresh process is unaffected (nothing leaks on the error path: cogaps_run destroys its session)
    for entry in ("matrix", "file"):
        out = subprocess.run([exe, mtx, "entry=" + entry, "nPatterns=3", "nIterations=40", "seed=5", "messages=0", "interruptAt=25"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 1 and "CoGAPS terminated: interrupted" in out.stderr and "interrupt polls 25" in out.stderr and "atomsA" not in out.stdout
    out = subprocess.run([exe, mtx, "nPatterns=3", "nIterations=40", "seed=5", "messages=0", "interruptAt=1000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "atomsA" in out.stdout


def test_tiny_domain(hip_lib):
    pu.run_stepwise(hip_lib, pu.synthetic(5, 6, rank=2, seed=3), 300, nPatterns=2, seed=9, total_iter=200, check_every=50)


def test_transpose_uncertainty_subset_fixed(hip_lib, gist, modsim):
    pu.run_stepwise(hip_lib, np.ascontiguousarray(modsim.T), 40, nPatterns=3, seed=4, total_iter=40, transposeData=True, check_every=10)
    idx = np.arange(1, 301, dtype=np.uint32)
    pu.run_stepwise(hip_lib, gist, 30, trace=False, nPatterns=4, seed=7, total_iter=30, subsetIndices=idx, subsetDim=1, check_every=10)
    pu.run_stepwise(hip_lib, gist, 30, trace=False, nPatterns=4, seed=7, total_iter=30, subsetIndices=np.arange(2, 9, dtype=np.uint32), subsetDim=2, check_every=10)
    fixedP = np.abs(np.random.default_rng(1).normal(size=(9, 4))).astype(np.float32)
    pu.run_stepwise(hip_lib, gist, 30, trace=False, nPatterns=4, seed=7, total_iter=30, subsetIndices=idx, subsetDim=1,
                    whichMatrixFixed="P", fixedPatterns=fixedP, check_every=10)


@pytest.mark.parametrize("sparse,transpose,fixed,subset,k,with_unc", pu.option_cases())
def test_option_combinations_stepwise(hip_lib, sparse, transpose, fixed, subset, k, with_unc):
    """all 36 combinations of {dense, sparse model} x {transposed input} x {no / A / P fixed} x {no subset, gene subset, sample subset},
    nPatterns 1..6, half of the dense ones with an uncertainty matrix: stepwise against the oracle"""
    pu.run_option_case(hip_lib, sparse, transpose, fixed, subset, k, with_unc)


@pytest.mark.parametrize("name,k", [("gist", 7), ("modsim", 3)])
def test_full_run_golden_lane_order(hip_lib, gist, modsim, name, k):
    """cogaps_run vs the committed oracle output in the kernels' reduction order: everything bit-exact"""
    from cogaps_amd import _capi
    g = np.load(os.path.join(GOLDEN, "%s_k%d_s42_i300_lane.npz" % (name, k)))
    r = _capi.run(gist if name == "gist" else modsim, nPatterns=k, nIterations=300, seed=42, outputFrequency=30)
    assert r["atomsA"].tolist() == g["atomsA"].tolist() and r["atomsP"].tolist() == g["atomsP"].tolist()
    assert r["totalUpdates"] == int(g["totalUpdates"])
    for f in ("chisq", "Amean", "Pmean", "Asd", "Psd"):
        assert np.array_equal(r[f], g[f]), f
    assert r["meanChiSq"] == float(g["meanChiSq"]) and r["averageQueueLengthA"] == float(g["avgQueueA"])
    # north-star tolerance (trivially met when bit-exact)
    for f in ("Amean", "Pmean"):
        assert np.max(np.abs(r[f] - g[f]) / np.maximum(np.abs(g[f]), 1e-30)) <= 1e-5


def test_shard_and_fixed_matrix_golden(hip_lib, gist):
    from cogaps_amd import _capi
    idx = np.arange(1, 601, dtype=np.uint32)
    g1 = np.load(os.path.join(GOLDEN, "gist_shard600_k5_s7_i200_lane.npz"))
    r1 = _capi.run(gist, nPatterns=5, nIterations=200, seed=7, outputFrequency=40, subsetIndices=idx, subsetDim=1)
    assert r1["atomsA"].tolist() == g1["atomsA"].tolist() and np.array_equal(r1["Pmean"], g1["Pmean"]) and np.array_equal(r1["Amean"], g1["Amean"])
    g2 = np.load(os.path.join(GOLDEN, "gist_shard600_k5_s7_i200_fixedP_lane.npz"))
    r2 = _capi.run(gist, nPatterns=5, nIterations=200, seed=7, outputFrequency=40, subsetIndices=idx, subsetDim=1,
                   whichMatrixFixed="P", fixedPatterns=g2["fixedP"])
    assert np.array_equal(r2["Amean"], g2["Amean"]) and not r2["Pmean"].any() and r2["meanChiSq"] == 0.0
    assert r2["totalUpdates"] == int(g2["totalUpdates"])


def test_reference_order_statistics_close(hip_lib, gist):
    """against the reference's own (sequential-order) golden run the chains differ in float rounding only:
    same regime -- atom counts within a few percent at the end of 1000+1000 iterations, chi2 within 2 %"""
    from cogaps_amd import _capi
    g = np.load(os.path.join(GOLDEN, "gist_k7_s42_i1000_seq.npz"))
    r = _capi.run(gist, nPatterns=7, nIterations=1000, seed=42, outputFrequency=100)
    assert abs(r["atomsA"][-5:].mean() - g["atomsA"][-5:].mean()) < 0.06 * g["atomsA"][-5:].mean()
    assert abs(r["chisq"][-5:].mean() - g["chisq"][-5:].mean()) < 0.02 * g["chisq"][-5:].mean()


def test_headline_size_invariants(hip_lib):
    """BASELINE configs[2] shape (20000 x 2000, K = 50): invariants that do not need the oracle --
    same seed twice gives identical bits; AP == A P^T recomputed; matrix == atoms summed per bin; atoms sorted
    and linked consistently; chi2 identity (reference tests/testthat/test_chisq.R)."""
    import bench
    from cogaps_amd import _capi
    data = bench.synthetic_dense(20000, 2000)
    runs = []
    for _ in range(2):
        S = _capi.Session(data, nPatterns=50, nIterations=20, seed=42, outputFrequency=5)
        S.run_iterations(1, 0, 12)
        runs.append((S.matrix("A"), S.matrix("P"), S.atoms("A"), S.natoms("A"), S.natoms("P"), S.chisq("P")))
        if len(runs) == 2:
            A, P, atoms = runs[1][0], runs[1][1], runs[1][2]
            ap = S.ap("A")                                           # [genes][samples]
            ref = A.astype(np.float64) @ P.astype(np.float64).T
            assert np.max(np.abs(ap - ref)) < 1e-3 * max(1.0, np.abs(ref).max())
            pos, mass = atoms["pos"], atoms["mass"]
            order = np.argsort(pos)
            assert np.all(np.diff(pos[order].astype(np.float64)) > 0)
            nxt = atoms["right"][order[:-1]]
            assert np.array_equal(nxt, order[1:].astype(np.uint32)) and atoms["right"][order[-1]] == 0xFFFFFFFF
            bin_len = (2 ** 64 - 1) // (20000 * 50)
            bins = (pos // np.uint64(bin_len)).astype(np.int64)
            acc = np.zeros(20000 * 50); np.add.at(acc, bins, mass.astype(np.float64))
            assert np.max(np.abs(acc.reshape(20000, 50) - A)) < 1e-3          # maximumDrift (AsynchronousGibbsSampler.h:235-271)
            S2 = np.maximum(data * 0.1, 0.1).astype(np.float64)
            chi = (((data - ref) / S2) ** 2).sum()
            assert abs(S.chisq("P") - chi) < 2e-3 * chi
        S.close()
    for a, b in zip(runs[0][:2], runs[1][:2]):
        assert np.array_equal(a, b)
    assert runs[0][3:] == runs[1][3:] and np.array_equal(runs[0][2]["pos"], runs[1][2]["pos"])


def test_sessions_in_flight_on_one_gpu(hip_lib, gist):
    """shards in flight (distributed.py): four sessions driven from four host threads on their own streams give the
    bits of the same runs made one after the other (graph capture, reallocation of the atom tables and the timing
    events of one session must not disturb another)"""
    import threading
    from cogaps_amd import _capi
    kw = [dict(nPatterns=3 + c, nIterations=60, seed=7 + c, outputFrequency=20) for c in range(4)]
    alone = [_capi.run(gist, **k) for k in kw]
    together, errors = [None] * 4, []

    def work(c):
        try:
            together[c] = _capi.run(gist, **kw[c])
        except Exception as e:       # noqa: BLE001 -- reported below
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(c,)) for c in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for a, b in zip(alone, together):
        for k in ("Amean", "Pmean", "Asd", "Psd", "atomsA", "atomsP", "chisq", "totalUpdates"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_batched_chains_equal_single_sessions(hip_lib, gist):
    """batched multi-chain launches (cogaps_batch_*: one generator workgroup per chain, one evaluation grid over all chains' queues,
    replayed from one captured graph): eight chains in lock-step give the bits of the eight chains run one at a time -- dense (fused
    and split evaluation), the sparse model, the fixed-matrix pass of GWCoGAPS; atom tables regrown in mid-run"""
    from cogaps_amd import _capi

    def check(datas, kws, **common):
        for d, k, r in zip(datas, kws, _capi.run_batch(datas, lib=hip_lib, kws=kws, **common)):
            o = _capi.run(d, lib=hip_lib, **dict(common, **k))
            for f in ("Amean", "Pmean", "Asd", "Psd", "atomsA", "atomsP", "chisq", "totalUpdates", "meanChiSq", "averageQueueLengthA", "averageQueueLengthP"):
                assert np.array_equal(np.asarray(r[f]), np.asarray(o[f])), f
    check([gist[170 * c:170 * (c + 1)] for c in range(8)], [dict(seed=3 + c) for c in range(8)], nPatterns=4, nIterations=120, outputFrequency=20, takePumpSamples=True)
    check([pu.synthetic(9000 + 4 * c, 24, seed=c) for c in range(4)], [dict(seed=c + 1) for c in range(4)], nPatterns=3, nIterations=40, outputFrequency=10)
    check([pu.synthetic_counts(600, 200, zeros=0.9, seed=s) for s in range(5)], [dict(seed=s + 9) for s in range(5)], nPatterns=12, nIterations=60, outputFrequency=15,
          sparseOptimization=True)
    fp = np.abs(np.random.default_rng(1).normal(size=(9, 3))).astype(np.float32)
    check([gist[:300], gist[300:600], gist[600:900]], [dict(seed=1), dict(seed=2), dict(seed=3)], nPatterns=3, nIterations=60, outputFrequency=20,
          whichMatrixFixed="P", fixedPatterns=fp)


def test_a_batch_of_chains_in_one_chained_launch_on_the_gpu(hip_lib, monkeypatch):
    """round 6, chain_kernel_multi: a batch of up to four chains whose evaluation is the fused one steps as ONE chained launch per lock-step
    (chain c's workgroups evaluate its queue, the last of them generates its next batch).  Three chains of ~3000 x 1600 (A side: 512-thread
    workgroups, the chained form; P side: 1024 threads, two launches) as one batch equal the three chains stepped alone, state for state;
    cogaps_session_chained says which form ran; with COGAPS_NO_CHAIN the batch keeps two launches per step and gives the same states."""
    from cogaps_amd import _capi
    datas = [pu.synthetic(3000 + 8 * c, 1600, seed=11 + c) for c in range(3)]
    kw = dict(nPatterns=6, nIterations=30)

    def state(S):
        return [(S.atoms(w)["pos"].copy(), S.atoms(w)["mass"].copy(), S.matrix(w).copy(), S.ap(w).copy()) for w in "AP"]
    alone = []
    for c, d in enumerate(datas):
        S = _capi.Session(d, lib=hip_lib, seed=50 + c, **kw); S.run_iterations(1, 0, 30); S.run_iterations(2, 0, 10); alone.append(state(S)); S.close()
    for no_chain in (False, True):
        if no_chain: monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
        ss = [_capi.Session(d, lib=hip_lib, seed=50 + c, **kw) for c, d in enumerate(datas)]
        B = _capi.Batch(ss)
        B.run_iterations(1, 0, 30); B.run_iterations(2, 0, 10)
        for c, S in enumerate(ss):
            assert S.chained("A") == (not no_chain) and not S.chained("P"), (c, no_chain)
            for x, y in zip(state(S), alone[c]):
                for u, v in zip(x, y): assert np.array_equal(u, v), (c, no_chain)
        B.close()
        for S in ss: S.close()


def test_batched_chains_grow_their_atom_tables(hip_lib, gist, monkeypatch):
    from cogaps_amd import _capi
    monkeypatch.setenv("COGAPS_INITIAL_ATOM_CAP", "64")
    datas, kws = [gist[:400], gist[400:800]], [dict(seed=1), dict(seed=2)]
    for d, k, r in zip(datas, kws, _capi.run_batch(datas, lib=hip_lib, kws=kws, nPatterns=5, nIterations=80, outputFrequency=20)):
        o = _capi.run(d, lib=hip_lib, nPatterns=5, nIterations=80, outputFrequency=20, **k)
        assert np.array_equal(r["Amean"], o["Amean"]) and r["atomsA"].tolist() == o["atomsA"].tolist() and r["atomsA"][-1] > 500


def test_run_from_file_equals_run_on_the_matrix(hip_lib, gist, tmp_path):
    """cogaps_run_from_file (the reference's gaps::run(path) / cogaps_from_file_cpp): the four formats of the GIST fixture give
    the bits of cogaps_run on the in-memory matrix; an uncertainty file is honoured"""
    from cogaps_amd import _capi
    kw = dict(nPatterns=4, nIterations=40, seed=9, outputFrequency=10)
    ref = _capi.run(gist, **kw)
    for ext in ("mtx", "csv", "tsv", "gct"):
        r = _capi.run_from_file(os.path.join(GOLDEN, "GIST." + ext), **kw)
        for k in ("Amean", "Pmean", "Asd", "Psd", "atomsA", "atomsP", "chisq", "totalUpdates"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(ref[k])), (ext, k)
    unc = np.maximum(gist * np.float32(0.2), np.float32(0.3)).astype(np.float32)
    upath = tmp_path / "unc.tsv"
    with open(upath, "w") as f:                       # plain decimals with 12 fractional digits read back as the same fp32
        f.write("\t".join("s%d" % j for j in range(unc.shape[1])) + "\n")
        for row in unc:
            f.write("\t".join("%.12f" % float(x) for x in row) + "\n")
    assert np.array_equal(_capi.read_matrix_file(str(upath)), unc)
    ru, rf = _capi.run(gist, unc=unc, **kw), _capi.run_from_file(os.path.join(GOLDEN, "GIST.mtx"), unc_path=str(upath), **kw)
    assert np.array_equal(ru["Amean"], rf["Amean"]) and np.array_equal(ru["chisq"], rf["chisq"]) and not np.array_equal(ru["chisq"], ref["chisq"])
    with pytest.raises(RuntimeError):
        _capi.run_from_file(os.path.join(GOLDEN, "nope.csv"), **kw)


def test_atom_tables_grow(hip_lib, gist, monkeypatch):
    """grow_atoms on the device path (reallocation invalidates the captured launch graphs): 64-atom initial capacity"""
    monkeypatch.setenv("COGAPS_INITIAL_ATOM_CAP", "64")
    a, p, props = pu.run_stepwise(hip_lib, gist, 150, trace=False, nPatterns=7, seed=42, total_iter=150, check_every=10)
    assert a > 2500


def test_bench_multi_rank_path_on_one_gpu():
    """bench.py's N > 1 path (rendezvous, barrier, all-gather of the shared factor, sum / max over ranks, one JSON line
    from rank 0) with two ranks sharing this box's GPU through the gloo test hook (the driver's runs use RCCL)"""
    import json, socket, subprocess, sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, COGAPS_BENCH_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "12", "--warmup", "4",
                          "--genes", "4000", "--samples", "400", "--patterns", "10", "--full", "--cpu-seconds", "8"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 12 and d["warmup"] == 4 and d["scaling"] == "weak" and d["unit"] == "proposals/s"
    assert d["value"] > 0 and d["roofline"]["traffic"] is None          # (not the shape the counters were collected on)
    # the N > 1 line carries the CPU comparator of BASELINE.md 3.5 -- one port run per subset, MEASURED side by side on the host (every rank its own
    # shard's window, all at once; round 5: no longer rank 0's figure times nSets) --, the spread of the ranks' timed regions and the library build
    cb = d["cpu_baseline"]
    sbs = cb["side_by_side"]
    assert cb["kind"] == "port" and cb["value"] == sbs["value"] > 0 and sbs["threads_per_shard"] >= 1 and cb["cores"] == 2 * sbs["threads_per_shard"]
    assert 0 < sbs["slowest_shard_value"] <= cb["value"] and cb["value"] < 2.5 * max(cb["value_rank0_shard"], sbs["slowest_shard_value"])
    assert "side by side" in cb["sample"] and cb["ten_x_line"] == 10 * cb["value"]
    rs = d["config"]["rank_seconds"]
    assert 0 < rs["min"] <= rs["median"] <= rs["max"] and abs(rs["max"] * 1e3 / 12 - d["ms_per_step"]) < 1e-6 * d["ms_per_step"] + 1e-9
    assert len(d["roofline"]["lib_source_hash"]) == 16
    assert d["config"]["proposals_timed"] > 0


NCCL_WORKER = r'''
import os, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import torch, torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%(port)d", rank=0, world_size=1, device_id=torch.device("cuda", 0))
from cogaps_amd import CogapsParams
from cogaps_amd.distributed import distributedCogaps
import pyoracle as po
data = po.read_mtx(os.path.join(%(root)r, "tests", "golden", "GIST.mtx"))[:360]
p = CogapsParams(nPatterns=3, seed=5, nIterations=40)
p.distributed = "genome-wide"; p.setDistributedParams(nSets=3, minNS=2)
p.explicitSets = [list(range(1, 121)), list(range(121, 241)), list(range(241, 361))]
out = distributedCogaps(data, p, outputFrequency=20)          # device = -1: resolved from torch's current device
assert dist.get_backend() == "nccl"
np.savez(sys.argv[1], Amean=out["Amean"], Asd=out["Asd"], Pmean=out["Pmean"], consensus=out["consensus"], meanChiSq=out["meanChiSq"],
         u0=out["unmatchedPatterns"][0], u2=out["unmatchedPatterns"][2])
dist.destroy_process_group()
'''


def test_rccl_path_with_one_rank(hip_lib, gist, tmp_path):
    """the `nccl` (= RCCL) branch of distributed.py and bench.py on the one GPU of this box, world size 1: rendezvous with
    device_id, device-tensor all-gathers of the shared factor and of the stitched factor, tensor placement.  The result equals
    the run without a process group; bench.py under torch.distributed.run prints its line through the same branch."""
    import json, socket, subprocess, sys
    from cogaps_amd import CogapsParams
    from cogaps_amd.distributed import distributedCogaps
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "nccl_worker.py"
    script.write_text(NCCL_WORKER % {"root": root, "port": port})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "r.npz")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    a = np.load(tmp_path / "r.npz")
    p = CogapsParams(nPatterns=3, seed=5, nIterations=40)
    p.distributed = "genome-wide"; p.setDistributedParams(nSets=3, minNS=2)
    p.explicitSets = [list(range(1, 121)), list(range(121, 241)), list(range(241, 361))]
    ref = distributedCogaps(gist[:360], p, outputFrequency=20)
    for k in ("Amean", "Asd", "Pmean", "consensus"):
        assert np.array_equal(ref[k], a[k]), k
    assert np.array_equal(ref["unmatchedPatterns"][2], a["u2"]) and abs(float(a["meanChiSq"]) - ref["meanChiSq"]) < 1e-3 * abs(ref["meanChiSq"]) + 1e-6
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2",
                          "--genes", "4000", "--samples", "400", "--patterns", "10", "--no-cpu"], cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["roofline"]["timing_consistent"]


def test_gwcogaps_driver_on_the_gpu(hip_lib, gist):
    """GWCoGAPS through the front-end on this GPU: four gene-wise shards, two in flight (BPPARAM = 2) -- the same bits as one
    shard at a time; the stitched result has the reference's structure (DistributedCogaps.R:226-278)"""
    from cogaps_amd import GWCoGAPS, CogapsParams

    def go(workers):
        p = CogapsParams(nPatterns=3, seed=5, nIterations=60)
        p.distributed = "genome-wide"
        p.setDistributedParams(nSets=4, minNS=2)
        p.explicitSets = [list(range(1 + 120 * i, 121 + 120 * i)) for i in range(4)]
        return GWCoGAPS(gist[:480], p, messages=False, outputFrequency=20, BPPARAM=workers)
    a, b = go(2), go(1)
    assert np.array_equal(a.featureLoadings, b.featureLoadings) and np.array_equal(a.loadingStdDev, b.loadingStdDev)
    assert np.array_equal(a.sampleFactors, b.sampleFactors)
    cons = a.metadata["diagnostics"]["consensus"]
    k = cons.shape[1]
    assert a.featureLoadings.shape == (480, k) and a.sampleFactors.shape == (9, k) and k >= 1
    assert np.allclose(cons.max(axis=0), 1.0) and not a.sampleFactors.any()        # the fixed side comes back zero, as in the reference
    assert len(a.metadata["diagnostics"]["unmatchedPatterns"]) == 4


def test_bench_lines_small_workload():
    """bench.py end to end on a small workload: the --full line carries roofline + cpu_baseline (the oracle port timed on
    the host), `--chains` and `--sparse` print their informational lines"""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    small = ["--genes", "3000", "--samples", "300", "--patterns", "8", "--steps", "16", "--warmup", "4"]

    def line(extra):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + small + extra, cwd=root, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1
        return json.loads(js[0])
    d = line(["--full", "--cpu-seconds", "2"])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["higher_is_better"] and d["dtype"] == "f32" and d["vs_baseline"] is None
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["traffic"] is None
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and "timed window" in c["sample"]
    assert abs(c.get("gpu_over_cpu_same_window", c.get("gpu_over_cpu_partial_window")) - d["value"] / c["value"]) < 1e-9 and (c["window_covered"] >= 1.0) == ("gpu_over_cpu_same_window" in c) and all(b["proposals"] > 0 and (b["iterations"] >= 1 or b["granularity"] != "whole iterations") for b in c["by_threads"])      # like for like: the port runs the window's own iterations
    c2 = line(["--no-cpu", "--chains", "2"])
    assert c2["value"] > 0 and c2["config"]["chains_mode"] == "batched" and c2["roofline"]["frac"] > 0
    assert line(["--no-cpu", "--chains", "2", "--chains-mode", "threads"])["value"] > 0
    s = line(["--no-cpu", "--sparse"])
    assert s["value"] > 0 and "sparse" in s["config"]["workload"]


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """a plain bench.py run prints the headline line without the CPU baseline; --dump-outputs DIR writes the run's result after the
    timed steps (float32 / float64 .npy files), and two runs with the same arguments write the same arrays"""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    small = ["--genes", "3000", "--samples", "300", "--patterns", "8", "--steps", "16", "--warmup", "4"]
    runs = []
    for k in range(2):
        d_ = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + small + ["--dump-outputs", str(d_)], cwd=root, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(js) == 1
        d = json.loads(js[0])
        assert d["steps"] == 16 and d["warmup"] == 4 and d["value"] > 0 and d["ms_per_step"] > 0 and d["cpu_baseline"] is None
        assert abs(d["ms_per_step"] - d["config"]["timed_region_ms_rank0"] / 16) < 1e-6 * d["ms_per_step"]
        runs.append({f.name: np.load(f) for f in sorted(d_.glob("*.npy"))})
    a, b = runs
    assert sorted(a) == sorted(b) and {"Amean.npy", "Asd.npy", "Pmean.npy", "Psd.npy", "A.npy", "P.npy", "chisqHistory.npy"} <= set(a)
    assert a["Amean.npy"].shape == (3000, 8) and a["Pmean.npy"].shape == (300, 8) and sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name
    assert a["Amean.npy"].any() and a["totals.npy"][0] > 0


def test_sccogaps_sparse_driver_on_the_gpu(hip_lib):
    """scCoGAPS (cell-wise shards, subsetDim = 2) with sparseOptimization through the front-end: shards in flight give the bits
    of one at a time; shard 0's first pass equals the oracle's chain on the same cell subset (SparseNormalModel)"""
    import pyoracle as po
    from cogaps_amd import scCoGAPS, CogapsParams
    data = pu.synthetic_counts(120, 90, zeros=0.8, seed=3)

    def go(workers):
        p = CogapsParams(nPatterns=3, seed=11, nIterations=50, sparseOptimization=True)
        p.distributed = "single-cell"
        p.setDistributedParams(nSets=3, minNS=2)
        p.explicitSets = [list(range(1 + 30 * i, 31 + 30 * i)) for i in range(3)]
        return scCoGAPS(data, p, messages=False, outputFrequency=10, BPPARAM=workers)
    a, b = go(3), go(1)
    assert np.array_equal(a.sampleFactors, b.sampleFactors) and np.array_equal(a.featureLoadings, b.featureLoadings)
    diag = a.metadata["diagnostics"]
    k = diag["consensus"].shape[1]
    assert a.sampleFactors.shape == (90, k) and a.featureLoadings.shape == (120, k) and not a.featureLoadings.any()
    # shard 0 = cells 1..30: the A sampler sees data vectors of 30 cells, the P sampler of 120 genes
    o = po.run(data, nPatterns=3, nIterations=50, seed=11, outputFrequency=10, math_mode=po.MATH_PORTABLE, sparseOptimization=True,
               redW_A=hip_lib.cogaps_reduction_width(30), redW_P=hip_lib.cogaps_reduction_width(120), redG=4,
               subsetIndices=np.arange(1, 31, dtype=np.uint32), subsetDim=2)
    assert np.array_equal(o["Amean"], diag["unmatchedPatterns"][0])


def test_sccogaps_every_shard_against_the_oracle(hip_lib):
    """scCoGAPS on 2000 genes x 3000 cells (95 % zeros, K = 8), three cell-wise shards of 1000: the first pass of EVERY shard equals
    the oracle's sparse-model chain on that cell subset (dataIndicesSubset on GapsParameters, as the reference's workers get it),
    and so does the second pass with the consensus fixed"""
    import pyoracle as po
    from cogaps_amd import scCoGAPS, CogapsParams
    data = pu.synthetic_counts(2000, 3000, zeros=0.95, rank=6, seed=21)
    p = CogapsParams(nPatterns=8, seed=13, nIterations=30, sparseOptimization=True)
    p.distributed = "single-cell"
    p.setDistributedParams(nSets=3, minNS=2)
    p.explicitSets = [list(range(1 + 1000 * i, 1001 + 1000 * i)) for i in range(3)]
    r = scCoGAPS(data, p, messages=False, outputFrequency=10, BPPARAM=3)
    diag = r.metadata["diagnostics"]
    wA, wP = hip_lib.cogaps_reduction_width(1000), hip_lib.cogaps_reduction_width(2000)
    okw = dict(nIterations=30, seed=13, outputFrequency=10, math_mode=po.MATH_PORTABLE, sparseOptimization=True, redW_A=wA, redW_P=wP, redG=4, subsetDim=2)
    cons = diag["consensus"]
    for i in range(3):
        idx = np.arange(1 + 1000 * i, 1001 + 1000 * i, dtype=np.uint32)
        o1 = po.run(data, nPatterns=8, subsetIndices=idx, **okw)
        assert np.array_equal(o1["Amean"], diag["unmatchedPatterns"][i]), "first pass, shard %d" % i
        assert np.array_equal(o1["Pmean"], diag["firstPass"][i]["Pmean"]) and o1["totalUpdates"] == diag["firstPass"][i]["totalUpdates"]
        o2 = po.run(data, nPatterns=cons.shape[1], subsetIndices=idx, whichMatrixFixed="A", fixedPatterns=cons, **okw)
        assert np.array_equal(o2["Pmean"], r.sampleFactors[1000 * i:1000 * (i + 1)]), "second pass, shard %d" % i
    assert r.sampleFactors.shape == (3000, cons.shape[1]) and not r.featureLoadings.any()


def test_configs4_shard_invariants(hip_lib):
    """BASELINE configs[4]'s per-GPU shard: 50000 genes x 12500 cells, 95 % zeros, sparseOptimization, K = 50 (cf. `bench.py --sparse
    --genes 50000 --samples 12500`), 16 iterations.  Size-independent properties, which hold whatever the lane order: the same seed twice
    gives the same bits; the HybridMatrix row and column copies agree within epsilon and the flag words mark exactly the column
    copy's non-zeros; the row copy equals the atoms summed per bin; atoms sorted and linked; the sparse chi2 equals the dense
    formula with the model's uncertainty (0.1 on zeros, 0.1 d elsewhere) evaluated from A, P in float64.  The same chain is compared
    with the oracle bit for bit by test_configs4_shard_shape_stepwise (proposal traces and state, up to past the A sampler's switch
    to the wide generator window) and test_benchmarked_sparse_chain_end_to_end_against_the_golden (all 200 iterations)."""
    from cogaps_amd import _capi
    data = pu.configs4_shard()
    runs = []
    for _ in range(2):
        S = _capi.Session(data, lib=hip_lib, nPatterns=50, nIterations=40, seed=42, outputFrequency=10, sparseOptimization=True)
        S.run_iterations(1, 0, 16)
        runs.append((S.rows("A"), S.rows("P"), S.matrix("A"), S.matrix("P"), S.atoms("A"), S.natoms("A"), S.natoms("P"), S.chisq("P")))
        last = S
        if len(runs) == 1:
            S.close()
    rA, rP, mA, mP, atoms, nA, nP, chi = runs[1]
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert np.array_equal(a, b)
    assert runs[0][5:] == runs[1][5:] and np.array_equal(runs[0][4]["pos"], atoms["pos"]) and nA > 1000
    for rows, mat in ((rA, mA), (rP, mP)):                                           # HybridVector::add / set epsilon rule (HybridVector.cpp:55-86)
        assert np.max(np.abs(rows - mat)) < 1e-5 + 1e-6 and np.all((mat == 0) | (mat >= 1e-5 - 1e-9))
    pos, mass = atoms["pos"], atoms["mass"]
    order = np.argsort(pos)
    assert np.all(np.diff(pos[order].astype(np.float64)) > 0) and np.array_equal(atoms["right"][order[:-1]], order[1:].astype(np.uint32))
    bins = (pos // np.uint64((2 ** 64 - 1) // (50000 * 50))).astype(np.int64)
    acc = np.zeros(50000 * 50); np.add.at(acc, bins, mass.astype(np.float64))
    assert np.max(np.abs(acc.reshape(50000, 50) - rA)) < 1e-3
    cols = np.arange(0, 12500, 50)                                                   # 250 cells
    d = data[:, cols].astype(np.float64)
    ap = rA.astype(np.float64) @ rP[cols].astype(np.float64).T
    sig = np.where(d > 0, 0.1 * d, 0.1)
    part = (((d - ap) / sig) ** 2).sum()
    # chi2 of the whole matrix from the library vs the same formula on the sampled columns scaled up: same order of magnitude only
    # (the columns differ); the exact check is per sampled column against a second, closed-form evaluation
    full = pu.sparse_chisq_f64(data, rA, rP)
    assert abs(chi - full) < 2e-3 * full and part > 0
    last.close()


C4_KW = dict(nPatterns=50, nIterations=100, seed=42, outputFrequency=10, sparseOptimization=True)


def test_configs4_shard_shape_stepwise(hip_lib):
    """BASELINE configs[4]'s per-GPU shard -- 50000 x 12500, 95 % zeros, sparseOptimization, K = 50, the chain `bench.py --sparse
    --genes 50000 --samples 12500` times -- from iteration 0 against the 16-thread lane-order oracle, so that a failure is located:
    Poisson step counts and both atom counts every iteration; the per-proposal traces (type, rows, columns, positions, PCG states, atom
    indices, batch sizes) of the first three iterations and of the iterations around the A sampler's switch from 256 to 448 attempts
    (chain_sparse_kernel<448, false>: seven attempt waves, the attempt lanes carrying the queue behind the helper wave's 64 slots); the
    full state (atoms, both HybridMatrix copies, chi2) just before the switch, three iterations after it and at the end, six iterations
    after the A sampler's window first reads 448.  The P sampler runs the wide form (chain_sparse_kernel<256, true>: 782 flag words of
    its 50000-element vectors folded onto 256 lanes) throughout.  Traced updates launch without graph capture, the others replay
    captured graphs, as the bench does.
    As measured on the MI355X (~85 s): the A window reads 448 after iteration 42 (the update of iteration 43 is the first at 448
    attempts); the P window goes 256 -> 128 after iteration 6 and back to 256 after iteration 38; 49 iterations, 4.58 M proposals, 2.46 M
    of them compared one by one by trace (iterations 0-2, 33-44), all of them through the state after iterations 42, 45 and 48."""
    import pyoracle as po
    from cogaps_amd import _capi
    data = pu.configs4_shard()
    S = _capi.Session(data, lib=hip_lib, **C4_KW)
    assert (hip_lib.cogaps_reduction_width(12500), hip_lib.cogaps_reduction_width(50000)) == (4096, 16384)
    O = po.Session(data, omp=True, maxThreads=min(16, os.cpu_count() or 1), math_mode=po.MATH_PORTABLE, redW_A=4096, redW_P=16384, redG=4, **C4_KW)
    switch, traced_its, winsP, props, traced, checked = None, [], [], 0, 0, []
    last_q = 0.0
    it = 0
    while switch is None or it <= switch + 6:
        assert it < 100, "the A sampler never switched to the wide generator window in the equilibration phase: the path under test was not taken"
        t = min(1.0, 2.0 * it / 100)
        S.set_annealing(t), O.set_annealing(t)
        nA, nP = S.draw_steps()
        assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
        # traced: the first iterations; once the A sampler's batches near the switch threshold (0.9 x 256 proposals), the narrow window's
        # last updates; the first two at 448 attempts
        trace = it < 3 or (switch is None and last_q > 0.75 * 256) or (switch is not None and it <= switch + 2)
        b0 = S.perf("A")
        if trace:
            for w, n, other in (("A", nA, "P"), ("P", nP, "A")):
                pu.assert_trace_equal(S.update(w, n, n + 256), O.update(w, n, n + 256), "iteration %d, sampler %s" % (it, w))
                S.sync(other), O.sync(other)
            traced_its.append(it)
            traced += nA + nP
        else:
            S.iterate(nA, nP), O.iterate(nA, nP)
        b1 = S.perf("A")
        last_q = (b1["proposalsQueued"] - b0["proposalsQueued"]) / max(1, b1["batches"] - b0["batches"])
        props += nA + nP
        for w in "AP":
            assert S.natoms(w) == O.natoms(w), "atom counts of sampler %s differ after iteration %d" % (w, it)
        if trace and it >= 2:
            assert S.chained("A") == 1 and S.chained("P") == 1, "iteration %d: the traced updates did not run as chained launches" % it
        winsP.append(S.generator_window("P"))
        if switch is None and S.generator_window("A") == 448:
            switch = it
        if switch is not None and it in (switch, switch + 3):
            pu.assert_state_equal(S, O, "iteration %d (A window %d)" % (it, S.generator_window("A")), ap=False)
            checked.append(it)
        it += 1
    pu.assert_state_equal(S, O, "iteration %d" % (it - 1), ap=False)
    checked.append(it - 1)
    assert S.generator_window("A") == 448 and S.chained("A") == 1 and S.chained("P") == 1
    assert switch in traced_its and switch + 1 in traced_its, "the updates on either side of the switch were not traced: %s" % traced_its
    assert set(winsP) == {128, 256}, "the P sampler's window did not move between 128 and 256 attempts: %s" % sorted(set(winsP))
    print("configs[4] shard stepwise: %d iterations, %d proposals (%d of them compared by trace, iterations %s); A window 448 from the "
          "update of iteration %d on; P windows after each iteration %s; state compared after iterations %s" % (it, props, traced, traced_its, switch + 1, winsP, checked))
    S.close(), O.close()


def test_current_device_as_the_first_runtime_call():
    """cogaps_current_device is what distributedCogaps asks before it hands a device ordinal to its shard threads -- in a process
    that has made no other HIP call yet (no torch.cuda, no session) it must still answer"""
    import subprocess, sys
    out = subprocess.run([sys.executable, "-c", "from cogaps_amd import _capi; print('device', _capi.current_device())"],
                         cwd=os.path.join(os.path.dirname(__file__), ".."), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "device 0" in out.stdout, out.stderr[-2000:]


def test_device_memory(hip_lib):
    """cogaps_device_memory: what distributed.py sizes a rank's batches by (an MI355X has 288 GB of HBM3E)"""
    from cogaps_amd import _capi
    free, total = _capi.device_memory(-1, lib=hip_lib)
    assert 0 < free <= total and total > 200e9
    assert _capi.device_memory(0, lib=hip_lib)[1] == total


def test_one_runtime_with_pytorch_in_either_import_order():
    """PyTorch's wheel bundles its own HIP / HSA runtime; the library must end up on the same one whichever is imported first
    (a process with two runtimes loses the device in the second: `no ROCm-capable device is detected`): load the library, then
    use torch.cuda, then run a session -- and the other way round"""
    import subprocess, sys
    body = ("import numpy as np\n%s\nprint(torch.ones(3, device='cuda').sum().item())\n"
            "S = _capi.Session(np.random.rand(50, 20).astype('f4'), nPatterns=3, nIterations=10, seed=1); S.run_iterations(1, 0, 5); print('session ok', _capi.current_device())\n"
            "print(sorted({l.split()[-1].split('/')[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))")
    for order in ("from cogaps_amd import _capi; _capi.load(); import torch", "import torch; torch.cuda.is_available(); from cogaps_amd import _capi"):
        out = subprocess.run([sys.executable, "-c", body % order], cwd=os.path.join(os.path.dirname(__file__), ".."), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "session ok 0" in out.stdout and "3.0" in out.stdout, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1].count("libamdhip64") == 1, out.stdout       # one HIP runtime mapped


def test_configs3_eight_shards_on_one_gpu(hip_lib):
    """BASELINE configs[3] on the one GPU a test has: synthetic dense 160000 x 2000, GWCoGAPS nSets = 8, nPatterns = 50 -- eight
    gene-wise shards of the headline shape, which a rank with eight shards runs as ONE batch of lock-stepped chains
    (cogaps_batch_*; on the 8-GPU node each rank has one).  30 + 30 iterations (the patterns need some variance for the matching step, DistributedCogaps.R:197-217); checked: a shard's chain inside the batch is
    bit-identical to the same shard run alone through cogaps_run, in the first pass and in the fixed-pattern second pass
    (callInternalCoGAPS, DistributedCogaps.R:12-35), and the stitched result has the reference's layout (:226-278)"""
    import bench
    from cogaps_amd import CogapsParams, _capi
    from cogaps_amd.distributed import distributedCogaps
    data = bench.synthetic_dense(160000, 2000)
    p = CogapsParams(nPatterns=50, seed=42, nIterations=30)
    p.distributed = "genome-wide"
    p.setDistributedParams(nSets=8, minNS=2, cut=50)
    r = distributedCogaps(data, p, outputFrequency=1000)
    sets, cons = r["subsets"], r["consensus"]
    assert len(sets) == 8 and all(len(st) == 20000 for st in sets) and np.array_equal(np.sort(np.concatenate(sets)), np.arange(1, 160001))
    k2 = cons.shape[1]
    assert cons.shape[0] == 2000 and k2 >= 1 and r["Amean"].shape == (160000, k2) and not r["Pmean"].any()
    kw = dict(nIterations=30, seed=42, outputFrequency=1000, runningDistributed=True, lib=hip_lib)
    for i in (0, 5):
        shard = np.ascontiguousarray(data[sets[i] - 1])
        one = _capi.run(shard, nPatterns=50, workerID=i + 1, **kw)
        for key in ("Amean", "Pmean", "Asd", "Psd"):
            assert np.array_equal(one[key], r["firstPass"][i][key]), "first pass, shard %d, %s" % (i, key)
        assert one["totalUpdates"] == r["firstPass"][i]["totalUpdates"] and one["meanChiSq"] == r["firstPass"][i]["meanChiSq"]
        two = _capi.run(shard, nPatterns=k2, workerID=i + 1, whichMatrixFixed="P", fixedPatterns=cons, **kw)
        assert np.array_equal(two["Amean"], r["Amean"][sets[i] - 1]), "second pass, shard %d" % i


def test_distributed_with_transposed_input(hip_lib, gist):
    """transposeData: the gene-wise shards of a samples x genes file are its column blocks (SubsetData.R:85-116); the
    result is the one of the untransposed run"""
    from cogaps_amd import GWCoGAPS, CogapsParams

    def go(data, transpose):
        p = CogapsParams(nPatterns=3, seed=5, nIterations=40)
        p.distributed = "genome-wide"
        p.setDistributedParams(nSets=3, minNS=2)
        p.explicitSets = [list(range(1 + 100 * i, 101 + 100 * i)) for i in range(3)]
        return GWCoGAPS(data, p, messages=False, outputFrequency=10, transposeData=transpose)
    a, b = go(gist[:300], False), go(np.ascontiguousarray(gist[:300].T), True)
    assert np.array_equal(a.featureLoadings, b.featureLoadings) and np.array_equal(a.loadingStdDev, b.loadingStdDev)
    assert np.array_equal(a.metadata["diagnostics"]["consensus"], b.metadata["diagnostics"]["consensus"])


def test_benchmarked_chain_end_to_end_against_the_golden(hip_lib):
    """The chain bench.py times -- BASELINE configs[2], 20000 x 2000, K = 50, seed 42, 100 + 100 iterations -- from its first iteration
    to its last against tests/golden/c3_k50_s42_i100_lane.npz (the lane-order oracle's run, tools/make_golden_c3.py; loop =
    runOnePhase, src/GapsRunner.cpp:272-327): the proposals of EVERY iteration and the domain sizes after it (so the timed window,
    iterations 181-200 of the schedule, is covered step by step), the atom / chi2 histories, totalUpdates (5.3e7), the queue
    lengths, meanChiSq, the four statistics matrices (sha256 + a 1 % sample to locate a mismatch) and the final chain state (atoms,
    factor matrices, A*P caches) -- all bit for bit."""
    import hashlib
    import bench
    from cogaps_amd import _capi
    g = np.load(os.path.join(GOLDEN, "c3_k50_s42_i100_lane.npz"))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    S = _capi.Session(bench.synthetic_dense(20000, 2000), lib=hip_lib, nPatterns=50, nIterations=100, seed=42, outputFrequency=10)
    k = 0
    for phase in (1, 2):
        for it in range(100):
            upd = S.run_iterations(phase, it, 1)
            assert upd == int(g["stepsA"][k]) + int(g["stepsP"][k]), "proposals of schedule step %d" % k
            assert (S.natoms("A"), S.natoms("P")) == (int(g["natomsA"][k]), int(g["natomsP"][k])), "atoms after schedule step %d" % k
            k += 1
    for w in "AP":
        a = S.atoms(w)
        assert sha(a["pos"]) == str(g["sha256_atoms_pos_" + w]) and sha(a["mass"]) == str(g["sha256_atoms_mass_" + w]), "final atoms " + w
        assert sha(S.matrix(w)) == str(g["sha256_matrix_" + w]), "final factor matrix " + w
        assert sha(S.ap(w)) == str(g["sha256_ap_" + w]), "final A*P cache " + w
        assert S.check_domain(w) == 0
    assert S.chained("A") == 1 and S.chained("P") == 0      # (the launch forms the bench times: chained A side, gen_apply + deciding evaluation on the P side)
    r = S.finish()
    S.close()
    assert r["totalUpdates"] == int(g["totalUpdates"]) == 52906603
    for f in ("atomsA", "atomsP", "chisq"):
        assert np.array_equal(r[f], g[f]), f
    assert r["averageQueueLengthA"] == float(g["avgQueueA"]) and r["averageQueueLengthP"] == float(g["avgQueueP"]) and r["meanChiSq"] == float(g["meanChiSq"])
    for f in ("Amean", "Pmean", "Asd", "Psd"):
        flat = r[f].ravel()
        assert np.array_equal(flat[g["sample_idx_" + f]], g["sample_" + f]), f + " (sample)"
        assert sha(r[f]) == str(g["sha256_" + f]), f


def test_benchmarked_sparse_chain_end_to_end_against_the_golden(hip_lib):
    """The sparse chain `bench.py --sparse --genes 50000 --samples 12500` times -- BASELINE configs[4]'s per-GPU shard, 95 % zeros,
    sparseOptimization, K = 50, seed 42, 100 + 100 iterations -- stepped as bench.py's run_steps does (run_iterations one schedule step
    at a time: captured graphs replayed) against tests/golden/c4shard_k50_s42_i100_sparse_lane.npz (the lane-order oracle's run,
    tools/make_golden_c3.py --sparse): the proposals of EVERY schedule step and both domain sizes after it, the atom / chi2 histories,
    totalUpdates, the queue lengths, meanChiSq, the four statistics matrices (sha256 + 4096 entries each to locate a mismatch) and the
    final chain state (atoms, both HybridMatrix copies) -- all bit for bit.  The launch forms are the bench's: chained on both sides,
    the A sampler switching from 256 to 448 attempts mid-run (graphs dropped and captured again) and the P sampler on the wide
    evaluation.  Last, chi2 of the final state in float64 over the whole matrix, through neither float32 implementation.
    As measured on the MI355X (~37 s): the A window goes 256 -> 128 after schedule step 6, -> 256 after step 22 and -> 448 after step 42,
    where it stays; the P window 256 -> 128 after step 6 and back to 256 after step 38.  The chain is 145 155 168 proposals."""
    import hashlib
    from cogaps_amd import _capi
    g = np.load(os.path.join(GOLDEN, "c4shard_k50_s42_i100_sparse_lane.npz"))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    data = pu.configs4_shard()
    assert sha(data) == str(g["sha256_input"]), "the input differs from the golden's (bench.synthetic_dense or numpy's MT19937 streams changed): not a kernel mismatch"
    assert (hip_lib.cogaps_reduction_width(12500), hip_lib.cogaps_reduction_width(50000)) == (int(g["redW_A"]), int(g["redW_P"])) == (4096, 16384)
    S = _capi.Session(data, lib=hip_lib, **C4_KW)
    win0 = S.generator_window("A")
    winsA, winsP = [], []
    k = 0
    for phase in (1, 2):
        for it in range(100):
            upd = S.run_iterations(phase, it, 1)
            assert upd == int(g["stepsA"][k]) + int(g["stepsP"][k]), "proposals of schedule step %d" % k
            for w in "AP":
                assert S.natoms(w) == int(g["natoms" + w][k]), "atoms of sampler %s after schedule step %d" % (w, k)
            winsA.append(S.generator_window("A")), winsP.append(S.generator_window("P"))
            k += 1
    for w in "AP":
        a = S.atoms(w)
        assert sha(a["pos"]) == str(g["sha256_atoms_pos_" + w]) and sha(a["mass"]) == str(g["sha256_atoms_mass_" + w]), "final atoms " + w
        assert sha(S.matrix(w)) == str(g["sha256_matrix_" + w]), "final factor matrix (HybridMatrix column copy) " + w
        assert sha(S.rows(w)) == str(g["sha256_rows_" + w]), "final factor matrix (HybridMatrix row copy) " + w
        assert S.check_domain(w) == 0
    assert S.chained("A") == 1 and S.chained("P") == 1 and winsA[-1] == 448
    switch = winsA.index(448)
    assert win0 < 448 and winsA[0] < 448 and switch > 0, "the A sampler did not begin below 448 attempts: the switch was not tested"
    moves = lambda ws: [(k, w) for k, w in enumerate(ws) if k == 0 or w != ws[k - 1]]
    print("configs[4] shard golden: window after schedule step -- A %s, P %s" % (moves(winsA), moves(winsP)))
    full = pu.sparse_chisq_f64(data, S.rows("A"), S.rows("P"))
    chi = S.chisq("P")
    assert abs(chi - full) < 2e-3 * full, (chi, full)
    r = S.finish()
    S.close()
    assert r["totalUpdates"] == int(g["totalUpdates"]) == 145155168
    for f in ("atomsA", "atomsP", "chisq"):
        assert np.array_equal(r[f], g[f]), f
    assert r["averageQueueLengthA"] == float(g["avgQueueA"]) and r["averageQueueLengthP"] == float(g["avgQueueP"]) and r["meanChiSq"] == float(g["meanChiSq"])
    for f in ("Amean", "Pmean", "Asd", "Psd"):
        flat = r[f].ravel()
        assert np.array_equal(flat[g["sample_idx_" + f]], g["sample_" + f]), f + " (sample)"
        assert sha(r[f]) == str(g["sha256_" + f]), f


@pytest.mark.parametrize("name", ["gist_tsv_k3", "modsim_sparse_k4", "gist_csv_sparse_k6", "k50_dense", "k50_sparse", "shard_round1", "shard_round2"])
def test_judge_round2_fingerprints_on_the_gpu(hip_lib, gist, modsim, name, _judge_cache={}):
    """the six further reference-printed configurations of tests/test_oracle_pin.py::JUDGE_R2 -- K = 50 dense and sparse, the two-round
    shard flow among them -- reproduced digit for digit by cogaps_run on the GPU in the verification mode"""
    from cogaps_amd import _capi
    from test_oracle_pin import JUDGE_R2, check_judge_case, run_judge_case
    r = run_judge_case(lambda d, **kw: _capi.run(d, lib=hip_lib, **SEQ, **kw), name, gist, modsim, _judge_cache)
    check_judge_case(r, JUDGE_R2[name])


@pytest.mark.parametrize("name", ["gist_gct_k9", "gist_tsv_sparse_k11_samples", "synth1500_k50_unc", "gist_csv_sparse_k4_genes", "synth2500_sparse_k50", "headline_18"])
def test_judge_round3_fingerprints_on_the_gpu(hip_lib, gist, name):
    """tests/test_oracle_pin.py::JUDGE_R3, configurations 1-6 of the round-3 verdict (a user uncertainty matrix, subsets in either dimension on
    the sparse model, K = 50 dense and sparse, the first 18 + 18 iterations of the headline matrix) reproduced by cogaps_run on the GPU in
    the verification mode: every printed digit"""
    from cogaps_amd import _capi
    from test_oracle_pin import JUDGE_R3, check_judge3_case, run_judge3_case
    r = run_judge3_case(lambda d, unc=None, **kw: _capi.run(d, unc=unc, lib=hip_lib, **SEQ, **kw), name, gist)
    check_judge3_case(r, JUDGE_R3[name])


def test_bench_starts_its_own_ranks_and_never_reports_fewer():
    """plain `python bench.py --gpus 2` (no launcher): the script starts its two ranks itself.  With the gloo test hook they share this
    box's GPU and the line says n_gpus = 2, ranks = 2; over RCCL two ranks need two GPUs -- on a one-GPU box the command fails and
    prints no line at all (never n_gpus = 1 for --gpus 2).  --sparse gathers the factor scCoGAPS shares (A), the dense line P."""
    import json, subprocess, sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    small = ["--steps", "8", "--warmup", "2", "--genes", "4000", "--samples", "400", "--patterns", "10", "--no-cpu"]
    for extra, shared in (([], "P"), (["--sparse"], "A")):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + small + extra, env=dict(base, COGAPS_BENCH_BACKEND="gloo"), cwd=root,
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["config"]["ranks"] == 2 and d["config"]["collective_backend"] == "gloo" and d["config"]["shared_factor_gathered"] == shared and d["value"] > 0
    if torch.cuda.device_count() < 2:
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + small, env=base, cwd=root, capture_output=True, text=True, timeout=900)
        assert out.returncode != 0 and not [ln for ln in out.stdout.splitlines() if ln.startswith("{")], out.stdout[-1000:]
        assert "needs 2 GPUs" in out.stderr


def test_configs4_eight_sparse_shards_on_one_gpu(hip_lib):
    """BASELINE configs[4] as a whole workload on the one GPU a test has: synthetic sparse 50000 genes x 100000 cells (95 % zeros),
    sparseOptimization, scCoGAPS nSets = 8, nPatterns = 50 -- eight cell-wise shards of 50000 x 12500, which a rank that holds all of
    them runs as batches of lock-stepped chains (on the 8-GPU node each rank has one).  The data never exist as one 20 GB matrix: a
    shard LOADER builds each 50000 x 12500 block when its turn comes (distributedCogaps(loader, shape = ...)).  Few iterations (the
    patterns need some variance for the matching step); checked: two shards' chains inside the batches are bit-identical to the same
    shards run alone through cogaps_run, in the first pass and in the fixed-pattern second pass (callInternalCoGAPS,
    DistributedCogaps.R:12-35), and the stitched result has the reference's layout (:226-278)"""
    import bench
    from cogaps_amd import CogapsParams, _capi
    from cogaps_amd.distributed import distributedCogaps
    G, CELLS, NSETS = 50000, 100000, 8
    per = CELLS // NSETS

    def block(i):
        # the bench's recipe -- rank-10 product, multiplicative noise, 95 % of the entries zeroed i.i.d. -- evaluated only where an entry
        # survives (positions from geometric gaps: the same distribution as an i.i.d. 5 % mask): a 50000 x 12500 block is built 18
        # times in this test
        rng = np.random.Generator(np.random.PCG64(12345 + i))
        a0 = (rng.gamma(2.0, 0.5, size=(G, 10)) * (rng.random((G, 10)) >= 0.7)).astype(np.float32)
        p0 = (rng.gamma(2.0, 0.5, size=(per, 10)) * (rng.random((per, 10)) >= 0.5)).astype(np.float32)
        pos = np.cumsum(rng.geometric(0.05, size=int(G * per * 0.05 * 1.02) + 4096)) - 1
        pos = pos[pos < G * per]
        rr, cc = np.divmod(pos, per)
        vals = np.einsum("ij,ij->i", a0[rr], p0[cc]) * (np.float32(0.9) + np.float32(0.2) * rng.random(pos.size, dtype=np.float32))
        d = np.zeros((G, per), dtype=np.float32)
        d.ravel()[pos] = vals
        return d
    asked = []

    def loader(i, idx):
        assert len(idx) == per and idx[0] == 1 + i * per and idx[-1] == (i + 1) * per       # contiguous explicit sets: block i
        asked.append(i)
        return block(i)
    p = CogapsParams(nPatterns=50, seed=42, nIterations=20, sparseOptimization=True)
    p.distributed = "single-cell"
    p.setDistributedParams(nSets=NSETS, minNS=2, cut=50)
    p.explicitSets = [np.arange(1 + i * per, 1 + (i + 1) * per) for i in range(NSETS)]
    r = distributedCogaps(loader, p, outputFrequency=1000, shape=(G, CELLS))
    assert sorted(asked) == sorted(list(range(NSETS)) * 2)
    cons = r["consensus"]
    k2 = cons.shape[1]
    assert cons.shape[0] == G and k2 >= 1 and r["Pmean"].shape == (CELLS, k2) and not r["Amean"].any()
    kw = dict(nIterations=20, seed=42, outputFrequency=1000, runningDistributed=True, sparseOptimization=True, lib=hip_lib)
    for i in (1, 6):
        shard = block(i)
        one = _capi.run(shard, nPatterns=50, workerID=i + 1, **kw)
        for key in ("Amean", "Pmean", "Asd", "Psd"):
            assert np.array_equal(one[key], r["firstPass"][i][key]), "first pass, shard %d, %s" % (i, key)
        assert one["totalUpdates"] == r["firstPass"][i]["totalUpdates"] and one["meanChiSq"] == r["firstPass"][i]["meanChiSq"]
        two = _capi.run(shard, nPatterns=k2, workerID=i + 1, whichMatrixFixed="A", fixedPatterns=cons, **kw)
        assert np.array_equal(two["Pmean"], r["Pmean"][i * per:(i + 1) * per]), "second pass, shard %d" % i


def test_host_launch_counters_on_the_gpu(hip_lib):
    """The update drivers' host launch counters (csrc/sampler_update.h, csrc/chain_batch.h) on the hardware, timing off, for the dense,
    sparse and three-chain cases of tests/test_update_drivers.py: launches per sampler -- replayed from a captured graph or not, a launch
    counts once -- and the batches they processed.  They follow from the chains and the chunk arithmetic alone and repeat run to run
    (profiles/update_drivers_refactor_checks.txt); on the MI355X the dense A sampler (300-element vectors: workgroups smaller than the
    generator's) keeps two launches per batch, one chain or three."""
    from cogaps_amd import _capi

    def counters(S):
        return {w: (int(S.perf(w)["genLaunches"]), int(S.perf(w)["evalLaunches"]), int(S.perf(w)["batches"]), S.chained(w)) for w in "AP"}
    S = _capi.Session(pu.synthetic(1200, 300, seed=7), lib=hip_lib, nPatterns=3, seed=123, nIterations=40)
    S.run_iterations(1, 0, 20)
    dense = counters(S)
    S.close()
    S = _capi.Session(pu.synthetic_counts(600, 200, zeros=0.9, seed=5), lib=hip_lib, nPatterns=4, seed=11, nIterations=40, sparseOptimization=True)
    S.run_iterations(1, 0, 30)
    sparse = counters(S)
    S.close()
    ss = [_capi.Session(pu.synthetic(1200, 300, seed=7 + c), lib=hip_lib, nPatterns=3, nIterations=40, seed=100 + c) for c in range(3)]
    B = _capi.Batch(ss)
    B.run_iterations(1, 0, 20)
    launches = [int(B.perf(w)["launches"]) for w in "AP"]
    batches = [[int(S.perf(w)["batches"]) for w in "AP"] for S in ss]
    chained = [[S.chained(w) for w in "AP"] for S in ss]
    B.close()
    for S in ss: S.close()
    print(dense, sparse, launches, batches, chained)
    assert dense == {"A": (222, 222, 163, False), "P": (0, 248, 146, True)}
    assert sparse == {"A": (0, 348, 259, True), "P": (0, 318, 212, True)}
    assert launches == [278, 259] and batches == [[181, 141], [182, 146], [172, 140]] and chained == [[False, True]] * 3


def test_session_build_routes_on_the_gpu(hip_lib):
    """Every input form of both models x transposeData x subsetData (csrc/session_build.h) on the hardware, "device" inputs at real
    device addresses: the table of tests/test_session_build.py and its constants -- the library before the chapter moved gives them on
    the MI355X as on the emulator (profiles/session_build_refactor_checks.txt)."""
    import test_session_build as sb
    from test_dense_device_input_gpu import dd
    got = {sb.case_id(case): sb.measure(hip_lib, case, dd) for case in sb.cases()}
    want = {sb.case_id(case): sb.expected(case) for case in sb.cases()}
    print(got)
    assert got == want
