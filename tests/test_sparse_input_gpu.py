"""Compressed-sparse input of the sparse model on the MI355X (product library): the build kernels of csrc/sparse_build.h and meanChiSq
from the packed data, against the oracle -- at the small shapes step by step, and at the benchmarked shape (BASELINE configs[4]'s
shard) against the lane-order oracle's recording."""
import hashlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

import parity_util as pu
from test_sparse_input import SHAPES, run_stepwise_sparse

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C4_KW = dict(nPatterns=50, nIterations=100, seed=42, outputFrequency=10, sparseOptimization=True)      # (tests/test_gpu_parity.py, C4_KW)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("genes,samples,k,iters,zeros,win", SHAPES)
def test_sparse_input_stepwise_gpu(hip_lib, oracle, genes, samples, k, iters, zeros, win, fmt):
    """(the product library has one generator window: `win` of the emulator's cases is not used)"""
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=genes + samples)
    run_stepwise_sparse(hip_lib, oracle, data, iters, fmt=fmt, trace=genes * samples < 50000, nPatterns=k, seed=11, total_iter=max(iters, 40),
                        sparseOptimization=True)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_full_run_matches_oracle_gpu(hip_lib, oracle, fmt):
    from cogaps_amd import _capi
    data = pu.synthetic_counts(150, 30, zeros=0.8, seed=21)
    kw = dict(nPatterns=4, nIterations=40, seed=42, outputFrequency=10, sparseOptimization=True)
    w_a, w_p = hip_lib.cogaps_reduction_width(30), hip_lib.cogaps_reduction_width(150)
    for capi_extra, oracle_extra, fields in ((dict(), dict(), ()), (dict(takePumpSamples=True, nSnapshots=4, snapshotPhase="all"), dict(takePumpSamples=True, snapshotFrequency=10, snapshotPhase=0),
                                             ("pumpMatrix", "meanPatternAssignment", "equilibrationSnapshotsA", "equilibrationSnapshotsP", "samplingSnapshotsA", "samplingSnapshotsP"))):
        r = _capi.run(getattr(sp, fmt + "_matrix")(data), lib=hip_lib, **kw, **capi_extra)
        o = oracle.run(data, math_mode=oracle.MATH_PORTABLE, redW_A=w_a, redW_P=w_p, redG=4, **kw, **oracle_extra)
        for f in ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP") + fields:
            assert np.array_equal(r[f], o[f]), f
        assert r["totalUpdates"] == o["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"]


def test_device_resident_input_equals_host_input(hip_lib):
    """onDevice = 1: the three arrays placed with torch, the library gets their addresses; same structures, same chain"""
    import torch
    from cogaps_amd import _capi
    data = pu.synthetic_counts(700, 260, zeros=0.85, seed=31)
    m = _capi.SparseMatrix.from_scipy(sp.csr_matrix(data))
    dev = torch.device("cuda", torch.cuda.current_device())
    # (uint64 / uint32 travel as the same bits in int64 / int32 tensors)
    t = [torch.from_numpy(a.view(v)).to(dev) for a, v in ((m.indptr, np.int64), (m.indices, np.int32), (m.values, np.float32))]
    torch.cuda.synchronize()
    md = _capi.SparseMatrix(m.shape, True, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), on_device=True)
    kw = dict(lib=hip_lib, nPatterns=5, nIterations=30, seed=3, sparseOptimization=True)
    H, D = _capi.Session(m, **kw), _capi.Session(md, **kw)
    for w in "AP":
        a, b = H.debug_sparse_data(w), D.debug_sparse_data(w)
        for f in ("flags", "prefix", "ptr", "vals", "lambda", "maxGibbsMass"):
            assert np.array_equal(a[f], b[f]), (w, f)
    assert H.device_bytes() == D.device_bytes()
    for phase in (1, 2):
        assert H.run_iterations(phase, 0, 30) == D.run_iterations(phase, 0, 30)
    rh, rd = H.finish(), D.finish()
    for f in ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP"):
        assert np.array_equal(rh[f], rd[f]), f
    assert rh["meanChiSq"] == rd["meanChiSq"]
    H.close(), D.close()
    del t


def test_structures_and_memory_against_the_dense_input_session(hip_lib):
    from cogaps_amd import _capi
    genes, samples = 3000, 2500
    data = sp.random(genes, samples, density=0.02, format="csc", dtype=np.float32, random_state=np.random.default_rng(3))
    data.data[:] = np.ceil(data.data * 9)
    kw = dict(lib=hip_lib, nPatterns=3, seed=1, sparseOptimization=True)
    S, D = _capi.Session(data, **kw), _capi.Session(data.toarray(), **kw)
    s_bytes, d_bytes = S.device_bytes(), D.device_bytes()
    print("device bytes: dense input %d, sparse input %d, one dense array %d" % (d_bytes, s_bytes, genes * samples * 4))
    assert d_bytes == s_bytes and s_bytes > 0
    assert d_bytes < genes * samples * 4
    ref = pu.packed_reference(data.toarray(), 3)
    pu.assert_structures_equal(ref, pu.structures(D), "dense input")
    pu.assert_structures_equal(ref, pu.structures(S), "csc input")
    for w in "AP":
        a, b = D.debug_sparse_data(w), S.debug_sparse_data(w)
        for f in ("flags", "prefix", "ptr", "vals", "lambda", "maxGibbsMass"):
            assert np.array_equal(a[f], b[f]), (w, f)
        assert a["vals"].size > 10000
    S.close(), D.close()


def test_two_sparse_input_sessions_in_a_batch_equal_the_two_alone(hip_lib):
    from cogaps_amd import _capi
    datas = [sp.csr_matrix(pu.synthetic_counts(300, 90, zeros=0.8, seed=40)), sp.csc_matrix(pu.synthetic_counts(300, 90, zeros=0.75, seed=41))]
    kws = [dict(seed=5), dict(seed=6)]
    common = dict(nPatterns=4, nIterations=40, outputFrequency=10, sparseOptimization=True)
    both = _capi.run_batch(datas, lib=hip_lib, kws=kws, **common)
    for d, k, b in zip(datas, kws, both):
        one = _capi.run(d, lib=hip_lib, **common, **k)
        for f in ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP"):
            assert np.array_equal(one[f], b[f]), f
        assert one["totalUpdates"] == b["totalUpdates"] and one["meanChiSq"] == b["meanChiSq"]


def test_benchmarked_sparse_chain_from_csr_against_the_golden(hip_lib):
    """tests/test_gpu_parity.py::test_benchmarked_sparse_chain_end_to_end_against_the_golden with the session created from the CSR form of
    configs[4]'s shard (50000 x 12500, 95 % zeros, K = 50, seed 42, 100 + 100 iterations): every schedule step's proposals and domain
    sizes, the histories, totalUpdates, the queue lengths, meanChiSq (the packed-data kernel at full size), the four statistics matrices,
    the final atoms and both HybridMatrix copies against tests/golden/c4shard_k50_s42_i100_sparse_lane.npz -- the lane-order oracle's
    run.  The launch forms do not depend on how the data came in (chained on both sides, 448 attempts at the end), and the session holds
    less than 2 GiB of device memory (packed values 2 x 31 M x 4 B, flag / prefix words, the atomic domains and queues of a
    50000 x 50 / 12500 x 50 problem; one dense array of the shard is 2.5 GB)."""
    from cogaps_amd import _capi
    g = np.load(os.path.join(GOLDEN, "c4shard_k50_s42_i100_sparse_lane.npz"))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    data = pu.configs4_shard()
    assert sha(data) == str(g["sha256_input"]), "the input differs from the golden's (bench.synthetic_dense or numpy's MT19937 streams changed): not a kernel mismatch"
    assert (hip_lib.cogaps_reduction_width(12500), hip_lib.cogaps_reduction_width(50000)) == (int(g["redW_A"]), int(g["redW_P"])) == (4096, 16384)
    csr = sp.csr_matrix(data)
    S = _capi.Session(csr, lib=hip_lib, **C4_KW)
    del csr
    dev_bytes = S.device_bytes()
    print("configs[4] shard from CSR: %d bytes of device memory, ordered sums %.2f ms" % (dev_bytes, S.sparse_build_ms()))
    assert dev_bytes < (2 << 30)
    win0 = S.generator_window("A")
    winsA = []
    k = 0
    for phase in (1, 2):
        for it in range(100):
            upd = S.run_iterations(phase, it, 1)
            assert upd == int(g["stepsA"][k]) + int(g["stepsP"][k]), "proposals of schedule step %d" % k
            for w in "AP":
                assert S.natoms(w) == int(g["natoms" + w][k]), "atoms of sampler %s after schedule step %d" % (w, k)
            winsA.append(S.generator_window("A"))
            k += 1
    for w in "AP":
        a = S.atoms(w)
        assert sha(a["pos"]) == str(g["sha256_atoms_pos_" + w]) and sha(a["mass"]) == str(g["sha256_atoms_mass_" + w]), "final atoms " + w
        assert sha(S.matrix(w)) == str(g["sha256_matrix_" + w]), "final factor matrix (HybridMatrix column copy) " + w
        assert sha(S.rows(w)) == str(g["sha256_rows_" + w]), "final factor matrix (HybridMatrix row copy) " + w
        assert S.check_domain(w) == 0
    assert S.chained("A") == 1 and S.chained("P") == 1 and winsA[-1] == 448
    assert win0 < 448 and winsA[0] < 448 and winsA.index(448) > 0
    assert S.device_bytes() < (2 << 30)
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
