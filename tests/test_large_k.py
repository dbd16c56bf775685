"""nPatterns above 50 on the test-only emulator build, bit for bit against the oracle.  The sparse model changes code path on K:
up to 64 patterns the other matrix's row is held in registers (SpRow, sp_row_load / sp_row_dot), above 64 every K-length dot goes
through sp_dot_row (8 float4 per trip, per-element bounds tests, a ragged last trip), and chi2 moves from chisq_sparse_tiled_kernel
to the untiled kernel (the verification mode's kernels likewise).  All dots switch their order at 25 elements (gaps::dot), the row
copies are padded to Kpad = (K + 3) & ~3, the LDS rows hold SP_KMAX = 512 entries and the Z1 / Z2 table launch has K + K (K + 1) / 2
workgroups.  The oracle has no limit on K and no branch on it besides the 25-element switch.  The cases here keep K at the value
that takes the path and shrink the matrix and the iteration count instead; tests/test_large_k_gpu.py repeats them on the hardware."""
import numpy as np
import pytest
import scipy.sparse as sp

import parity_util as pu
from cogaps_amd import _capi
from test_coo_input import coo_of

SEQ = dict(reductionMode="seq", mathMode="glibc-fma")
RUN_FIELDS = ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP")
STAT_FIELDS = RUN_FIELDS + ("pumpMatrix", "meanPatternAssignment", "equilibrationSnapshotsA", "equilibrationSnapshotsP", "samplingSnapshotsA", "samplingSnapshotsP")
BATCH_FIELDS = RUN_FIELDS + ("totalUpdates", "meanChiSq", "averageQueueLengthA", "averageQueueLengthP")

# K: what it is there for
ORDER_SWITCH = [24, 25, 26]                     # gaps::dot adds last-to-first up to 25 elements, first-to-last above; Kpad 24 / 28 / 28
REGISTER_SWITCH = [63, 64, 65, 66, 67, 68]      # SpRow and the tiled chi2 up to 64, sp_dot_row and the untiled chi2 above; every K mod 4
TRIP_COUNTS = [96, 97, 130, 256]                # sp_dot_row: exactly 3 trips of 32 elements, one element over, 5 trips with a ragged last, 8 trips


def counts_90x70():
    return pu.synthetic_counts(90, 70, zeros=0.7, seed=3)


def sparse_stepwise(lib, data, k, iters, total_iter=12, **kw):
    kw = dict(dict(trace=True, nPatterns=k, seed=9, total_iter=total_iter, check_every=2, sparseOptimization=True), **kw)
    return pu.run_stepwise(lib, data, iters, **kw)


def stepwise_proposal_types(lib, data, n_iter, total_iter, **kw):
    """pu.run_stepwise with traces, state compared after every iteration; returns per sampler the set of proposal types the ORACLE queued"""
    S, O = pu.make_pair(lib, data, nIterations=total_iter, **kw)
    types = {"A": set(), "P": set()}
    for it in range(n_iter):
        t = min(1.0, 2.0 * it / total_iter)
        S.set_annealing(t), O.set_annealing(t)
        nA, nP = S.draw_steps()
        assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
        for w, n, other in (("A", nA, "P"), ("P", nP, "A")):
            ts, to = S.update(w, n, 1 << 16), O.update(w, n, 1 << 16)
            pu.assert_trace_equal(ts, to, "it%d %s" % (it, w))
            types[w] |= {chr(c) for c in np.unique(to["rec"]["type"])}
            S.sync(other), O.sync(other)
        pu.assert_state_equal(S, O, "it%d" % it)
    S.close(), O.close()
    return types


def all_proposal_types_case(lib, iters):
    """K = 65 on 90 x 70: births, deaths, moves and exchanges all queued by both samplers, so the evaluation modes ONE, CH (a death's
    change) and SAME (a move / exchange within one row) and the two-row pair all take their K-length dots through sp_dot_row.  That the
    four types occur is a condition of the case: `iters` is the count at which the oracle's own trace shows it."""
    types = stepwise_proposal_types(lib, counts_90x70(), iters, 12, nPatterns=65, seed=9, sparseOptimization=True)
    for w in "AP":
        assert types[w] == set("BDME"), "sampler %s queued only %s" % (w, sorted(types[w]))


def dense_factors_stepwise(lib, k, iters, **kw):
    """The cases above leave the factor matrices nearly empty: a chain of a few iterations at the default alpha holds ~100 atoms in
    thousands of cells, so a K-length dot of a row of A with a row of P has almost never more than two non-zero terms -- and a sum of two
    terms from +0 does not depend on its order.  Here alphaA = alphaP = 1 (about one atom per cell expected) on a 12 x 10 matrix: on the
    oracle at K = 65, 20 iterations, every pair of rows has at least 3 common non-zeros, 9 on average, so the summation order, the
    25-element switch and the trip boundaries of sp_dot_row all show in the bits.  The condition of the case, checked on the oracle's
    matrices at the end: at least 9 of 10 pairs of rows have 3 or more common non-zeros (three terms is where the order starts to count)."""
    data = pu.synthetic_counts(12, 10, zeros=0.3, seed=3)
    S, O = pu.make_pair(lib, data, nPatterns=k, seed=9, nIterations=iters, sparseOptimization=True, alphaA=1.0, alphaP=1.0, **kw)
    for it in range(iters):
        t = min(1.0, 2.0 * it / iters)
        S.set_annealing(t), O.set_annealing(t)
        nA, nP = S.draw_steps()
        assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
        pu.assert_trace_equal(S.update("A", nA, 1 << 16), O.update("A", nA, 1 << 16), "it%d A" % it)
        S.sync("P"), O.sync("P")
        pu.assert_trace_equal(S.update("P", nP, 1 << 16), O.update("P", nP, 1 << 16), "it%d P" % it)
        S.sync("A"), O.sync("A")
        if it % 2 == 1 or it == iters - 1:
            pu.assert_state_equal(S, O, "it%d" % it)
    common = (O.matrix("A") != 0).astype(np.int64) @ (O.matrix("P") != 0).astype(np.int64).T
    S.close(), O.close()
    assert (common >= 3).mean() >= 0.9, (common >= 3).mean()


# ---- 1. the sparse model step by step, traces in lane order ----

@pytest.mark.parametrize("k", [24, 25, 26, 64, 65, 97])
def test_sparse_stepwise_dense_factors(emul_lib, k):
    dense_factors_stepwise(emul_lib(256), k, 16)


@pytest.mark.parametrize("k", ORDER_SWITCH + REGISTER_SWITCH + TRIP_COUNTS)
def test_sparse_stepwise(emul_lib, k):
    sparse_stepwise(emul_lib(256), counts_90x70(), k, 6 if k <= 130 else 4)


def test_sparse_stepwise_all_of_sp_kmax(emul_lib):
    """K = 512: the arowA / arowB / z2A / z2B rows of SP_KMAX entries filled to the last one, 16 trips of sp_dot_row, 131 840 workgroups of
    the Z1 / Z2 table launch.  One iteration: emulated, each of its four table launches (two at creation, one per sync) takes 6 - 7 s
    whatever the matrix; the hardware test steps further"""
    sparse_stepwise(emul_lib(256), pu.synthetic_counts(64, 64, zeros=0.5, seed=3), 512, 1)


@pytest.mark.parametrize("genes,samples,zeros,iters", [
    (300, 200, 0.85, 4),      # 5 and 4 flag words per vector
    (64, 64, 0.5, 6),         # N a multiple of 64: the second flag word of every vector is empty
])
def test_sparse_stepwise_flag_words(emul_lib, genes, samples, zeros, iters):
    sparse_stepwise(emul_lib(256), pu.synthetic_counts(genes, samples, zeros=zeros, seed=3), 65, iters)


def test_sparse_all_proposal_types(emul_lib):
    all_proposal_types_case(emul_lib(256), 8)


# ---- 2. verification mode ----

def test_verification_mode_stepwise(emul_lib):
    """sparse_tables_seq_kernel and the sequential chi2 kernels above 64 patterns"""
    sparse_stepwise(emul_lib(256), counts_90x70(), 70, 4, **SEQ)


def test_verification_mode_stepwise_dense_factors(emul_lib):
    dense_factors_stepwise(emul_lib(256), 70, 16, **SEQ)


def verification_full_run(lib, oracle, n_iter):
    data = pu.synthetic_counts(150, 30, zeros=0.8, seed=21)
    kw = dict(nPatterns=70, nIterations=n_iter, seed=42, outputFrequency=n_iter // 4, sparseOptimization=True)
    r = _capi.run(data, lib=lib, **SEQ, **kw)
    o = oracle.run(data, math_mode=oracle.MATH_GLIBC_FMA, **kw)
    for f in RUN_FIELDS:
        assert np.array_equal(r[f], o[f]), f
    assert r["totalUpdates"] == o["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"] and o["meanChiSq"] > 0


def test_verification_mode_full_run(emul_lib, oracle):
    """cogaps_run in the reference's own arithmetic at K = 70: statistics, and meanChiSq through mean_chisq_seq_kernel (packed_datum)"""
    verification_full_run(emul_lib(256), oracle, 8)


# ---- 3. / 5. full runs with statistics ----

def full_run_with_statistics(lib, oracle, data, n_iter, sparse):
    """cogaps_run against the oracle's run in lane order at K = 65, PUMP statistics (pump_kernel reads rows[i * Kpad + j], Kpad = 68 in
    the sparse model) and three snapshots per phase"""
    kw = dict(nPatterns=65, nIterations=n_iter, seed=42, outputFrequency=n_iter // 3, takePumpSamples=True, sparseOptimization=sparse)
    r = _capi.run(data, lib=lib, nSnapshots=3, snapshotPhase="all", **kw)
    w_a, w_p = lib.cogaps_reduction_width(data.shape[1]), lib.cogaps_reduction_width(data.shape[0])
    o = oracle.run(data, math_mode=oracle.MATH_PORTABLE, redW_A=w_a, redW_P=w_p, redG=4, snapshotFrequency=n_iter // 3, snapshotPhase=0, **kw)
    for f in STAT_FIELDS:
        assert r[f].shape == o[f].shape and np.array_equal(r[f], o[f]), f
    assert r["totalUpdates"] == o["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"] and o["meanChiSq"] > 0
    for f in ("equilibrationSnapshotsA", "equilibrationSnapshotsP", "samplingSnapshotsA", "samplingSnapshotsP"):
        assert r[f].shape[0] == 3 and r[f].shape[2] == 65, f
    assert np.allclose(r["pumpMatrix"].sum(axis=1), 1.0) and r["Amean"].any() and r["Pmean"].any()


def test_sparse_full_run_with_statistics(emul_lib, oracle):
    full_run_with_statistics(emul_lib(256), oracle, pu.synthetic_counts(60, 40, zeros=0.7, seed=21), 9, True)


def test_dense_full_run_with_statistics(emul_lib, oracle):
    """stats_kernel with 65 workgroups, the K-loop of mean_chisq_rows_kernel, pump_kernel"""
    full_run_with_statistics(emul_lib(256), oracle, pu.synthetic(83, 37), 9, False)


# ---- 4. batched chains ----

def batched_chains_equal_single_sessions(lib, genes, samples, n_iter):
    datas = [pu.synthetic_counts(genes, samples, zeros=0.8, seed=s) for s in (1, 2, 3)]
    kws = [dict(seed=s) for s in (4, 5, 6)]
    common = dict(nPatterns=65, nIterations=n_iter, outputFrequency=n_iter // 2, sparseOptimization=True)
    for c, (d, k, r) in enumerate(zip(datas, kws, _capi.run_batch(datas, lib=lib, kws=kws, **common))):
        o = _capi.run(d, lib=lib, **dict(common, **k))
        for f in BATCH_FIELDS:
            assert np.array_equal(np.asarray(r[f]), np.asarray(o[f])), (c, f)
        assert o["atomsA"][-1] > 0 and o["atomsP"][-1] > 0


def test_batched_chains_equal_single_sessions(emul_lib):
    """three sparse chains at K = 65 stepped by the *_multi kernels give the bits of the three stepped alone"""
    batched_chains_equal_single_sessions(emul_lib(256), 80, 40, 4)


# ---- 5. the dense model (no switch on K; never run above 50 before) ----

@pytest.mark.parametrize("k,iters", [(65, 6), (130, 4), (300, 3)])
def test_dense_stepwise(emul_lib, k, iters):
    pu.run_stepwise(emul_lib(256), pu.synthetic(83, 37), iters, trace=True, nPatterns=k, seed=9, total_iter=12, check_every=2)


# ---- 6. the limit ----

SPARSE_MODEL_ENTRIES = ("cogaps_session_create", "cogaps_session_create_sparse", "cogaps_session_create_coo", "cogaps_session_create_from_device_matrix")


def limit_data():
    return pu.synthetic_counts(24, 16, zeros=0.5, seed=3)


def pattern_limit(lib, entry):
    """513 patterns refused, 512 accepted by the entry `entry` (each of the four that can create a sparse-model session)"""
    data = limit_data()
    dm = None
    if entry == "cogaps_session_create_from_device_matrix":
        dm = _capi.DeviceMatrix(sp.csc_matrix(data), lib=lib)
    d = {"cogaps_session_create": data, "cogaps_session_create_sparse": sp.csr_matrix(data), "cogaps_session_create_coo": coo_of(data, 5),
         "cogaps_session_create_from_device_matrix": dm}[entry]
    with pytest.raises(_capi.CogapsError, match=entry + ": .*at most 512 patterns"):
        _capi.Session(d, lib=lib, nPatterns=513, seed=1, sparseOptimization=True)
    S = _capi.Session(d, lib=lib, nPatterns=512, seed=1, sparseOptimization=True)
    assert S.dims("A") == (24, 16, 512) and S.dims("P") == (16, 24, 512)
    assert S.chisq("A") == 100.0 * int((data > 0).sum())      # (all-zero factors: 100 per entry > 0)
    S.close()
    if dm is not None:
        dm.close()


def dense_model_takes_513_patterns(lib):
    S = _capi.Session(limit_data(), lib=lib, nPatterns=513, seed=1)
    assert S.dims("A") == (24, 16, 513) and S.dims("P") == (16, 24, 513)
    S.close()


@pytest.mark.parametrize("entry", SPARSE_MODEL_ENTRIES)
def test_pattern_limit_of_the_sparse_model(emul_lib, entry):
    pattern_limit(emul_lib(256), entry)


def test_dense_model_takes_513_patterns(emul_lib):
    dense_model_takes_513_patterns(emul_lib(256))
