"""Compressed-sparse input of the sparse model (cogaps_session_create_sparse, csrc/sparse_build.h) on the test-only emulator build:
a session created from the CSR / CSC form of a matrix is the session created from its dense form, bit for bit -- against the oracle
(which only knows dense matrices) step by step, structure by structure against the dense-input session and against the definition of
the structures in numpy (parity_util.packed_reference: the dense-input session goes through the same device build), and through the
front ends."""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import parity_util as pu
from cogaps_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_stepwise_sparse(lib, oracle, data, n_iter, fmt="csr", trace=True, total_iter=None, check_every=1, dense_for_oracle=None, **kw):
    """pu.run_stepwise for a session created from the compressed form (dense_for_oracle: what the oracle gets instead of `data`)"""
    total_iter = total_iter or max(n_iter, 2)
    kw.setdefault("nIterations", total_iter)
    S = _capi.Session(data if sp.issparse(data) else getattr(sp, fmt + "_matrix")(data), lib=lib, **kw)
    dense = dense_for_oracle if dense_for_oracle is not None else data
    wA, wP = lib.cogaps_reduction_width(S.dims("A")[1]), lib.cogaps_reduction_width(S.dims("P")[1])
    O = oracle.Session(dense, math_mode=oracle.MATH_PORTABLE, redW_A=wA, redW_P=wP, redG=4, **kw)
    fixed = kw.get("whichMatrixFixed", "N")
    for it in range(n_iter):
        t = min(1.0, 2.0 * it / total_iter)
        S.set_annealing(t), O.set_annealing(t)
        nA, nP = S.draw_steps()
        assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
        if trace and fixed == "N":
            pu.assert_trace_equal(S.update("A", nA, 1 << 16), O.update("A", nA, 1 << 16), "it%d A" % it)
            S.sync("P"), O.sync("P")
            pu.assert_trace_equal(S.update("P", nP, 1 << 16), O.update("P", nP, 1 << 16), "it%d P" % it)
            S.sync("A"), O.sync("A")
        else:
            S.iterate(nA, nP), O.iterate(nA, nP)
        if (it + 1) % check_every == 0 or it == n_iter - 1:
            pu.assert_state_equal(S, O, "it%d" % it)
    S.close(), O.close()


# the five shapes of test_sparse_model.py::test_sparse_stepwise
SHAPES = [
    (60, 40, 3, 120, 0.85, 256),      # one flag word per vector, K <= 25
    (300, 50, 30, 30, 0.85, 256),     # K > 25
    (9000, 12, 4, 10, 0.9, 256),      # 141 flag words
    (20, 5000, 3, 10, 0.9, 256),      # the long side on the other sampler
    (200, 70, 7, 40, 0.6, 64),        # 64-attempt windows
]


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("genes,samples,k,iters,zeros,win", SHAPES)
def test_sparse_input_stepwise(emul_lib, oracle, genes, samples, k, iters, zeros, win, fmt):
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=genes + samples)
    run_stepwise_sparse(emul_lib(win), oracle, data, iters, fmt=fmt, trace=genes * samples < 50000, nPatterns=k, seed=11, total_iter=max(iters, 40),
                        sparseOptimization=True)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_sparse_input_options(emul_lib, oracle, fmt):
    lib = emul_lib(256)
    data = pu.synthetic_counts(240, 36, zeros=0.8, seed=9)
    kw = dict(trace=False, nPatterns=4, seed=3, total_iter=40, sparseOptimization=True, fmt=fmt)
    run_stepwise_sparse(lib, oracle, np.ascontiguousarray(data.T), 20, transposeData=True, **kw)
    fixed = np.abs(np.random.default_rng(2).normal(0.5, 0.4, (36, 4))).astype(np.float32)
    fixed[fixed < 0.3] = 0.0
    run_stepwise_sparse(lib, oracle, data, 20, whichMatrixFixed="P", fixedPatterns=fixed, **kw)
    # an all-zero row, an all-zero column, and rows of exactly 128 elements (the flag word past the last element)
    d2 = pu.synthetic_counts(90, 128, zeros=0.7, seed=4)
    d2[17, :] = 0.0
    d2[:, 64] = 0.0
    run_stepwise_sparse(lib, oracle, d2, 15, **kw)
    run_stepwise_sparse(lib, oracle, np.ascontiguousarray(d2.T), 15, **kw)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_stored_zeros_negatives_and_nan_are_dropped(emul_lib, oracle, fmt):
    """explicitly stored entries that are not > 0 count as absent: the run equals the dense run of the matrix with them zeroed"""
    data = pu.synthetic_counts(70, 50, zeros=0.7, seed=8)
    m = sp.coo_matrix(data)
    rng = np.random.default_rng(1)
    empty = np.argwhere(data == 0)
    pick = empty[rng.choice(len(empty), 30, replace=False)]
    bad = np.concatenate([np.zeros(10), -np.arange(1, 11), np.full(10, np.nan)]).astype(np.float32)
    m = sp.coo_matrix((np.concatenate([m.data, bad]), (np.concatenate([m.row, pick[:, 0]]), np.concatenate([m.col, pick[:, 1]]))), shape=data.shape)
    m = m.tocsr() if fmt == "csr" else m.tocsc()
    assert m.nnz == int((data > 0).sum()) + 30
    run_stepwise_sparse(emul_lib(256), oracle, m, 25, trace=True, dense_for_oracle=data, nPatterns=3, seed=5, total_iter=40, sparseOptimization=True)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
@pytest.mark.parametrize("transpose", [False, True])
def test_structures_equal_the_dense_input_sessions(emul_lib, fmt, transpose):
    """flag words, prefix counts, pointers, packed values, lambda and maxGibbsMass of both samplers, array for array: several flag
    words per vector on both sides and > 10^4 entries, so that the ordered sums run over several chunks"""
    lib = emul_lib(256)
    data = pu.synthetic_counts(400, 330, zeros=0.85, seed=12)
    assert int((data > 0).sum()) >= 10000
    if transpose:
        data = np.ascontiguousarray(data.T)
    kw = dict(lib=lib, nPatterns=5, seed=2, sparseOptimization=True, transposeData=transpose)
    D, S = _capi.Session(data, **kw), _capi.Session(getattr(sp, fmt + "_matrix")(data), **kw)
    ref = pu.packed_reference(data, 5, transposeData=transpose)
    pu.assert_structures_equal(ref, pu.structures(D), "dense input")
    pu.assert_structures_equal(ref, pu.structures(S), fmt + " input")
    for w in "AP":
        a, b = D.debug_sparse_data(w), S.debug_sparse_data(w)
        assert a["flags"].shape[1] > 1
        for f in ("flags", "prefix", "ptr", "vals"):
            assert a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), "%s %s differs" % (w, f)
        assert a["lambda"] == b["lambda"] and a["maxGibbsMass"] == b["maxGibbsMass"], w
        assert D.chisq(w) == S.chisq(w)
    D.close(), S.close()


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_full_run_matches_oracle(emul_lib, oracle, fmt):
    data = pu.synthetic_counts(150, 30, zeros=0.8, seed=21)
    lib = emul_lib(256)
    kw = dict(nPatterns=4, nIterations=40, seed=42, outputFrequency=10, sparseOptimization=True)
    w_a, w_p = lib.cogaps_reduction_width(30), lib.cogaps_reduction_width(150)
    for extra, oracle_extra, fields in ((dict(), dict(), ()), (dict(takePumpSamples=True, nSnapshots=4, snapshotPhase="all"), dict(takePumpSamples=True, snapshotFrequency=10, snapshotPhase=0),
                                        ("pumpMatrix", "meanPatternAssignment", "equilibrationSnapshotsA", "equilibrationSnapshotsP", "samplingSnapshotsA", "samplingSnapshotsP"))):
        r = _capi.run(getattr(sp, fmt + "_matrix")(data), lib=lib, **kw, **extra)
        o = oracle.run(data, math_mode=oracle.MATH_PORTABLE, redW_A=w_a, redW_P=w_p, redG=4, **kw, **oracle_extra)
        for f in ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP") + fields:
            assert np.array_equal(r[f], o[f]), f
        assert r["totalUpdates"] == o["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"]
        if fields:
            assert r["samplingSnapshotsA"].shape[0] == 4
    # ... and the dense-input run of the library
    assert _capi.run(data, lib=lib, **kw, **extra)["meanChiSq"] == r["meanChiSq"]


def _c_matrix(shape, major_is_row, indptr, indices, values):
    return _capi.SparseMatrix(shape, major_is_row, np.asarray(indptr, dtype=np.uint64), np.asarray(indices, dtype=np.uint32), np.asarray(values, dtype=np.float32))


def test_rejections(emul_lib):
    lib = emul_lib(256)
    kw = dict(lib=lib, nPatterns=2, seed=1, sparseOptimization=True)
    good = dict(shape=(3, 4), major_is_row=True, indptr=[0, 2, 3, 5], indices=[0, 2, 1, 0, 3], values=[1, 2, 3, 4, 5])

    def refused(match, kwargs=kw, **change):
        with pytest.raises(_capi.CogapsError, match=match):
            _capi.Session(_c_matrix(**dict(good, **change)), **kwargs)
    _capi.Session(_c_matrix(**good), **kw).close()                                   # the well-formed matrix is accepted
    refused("strictly ascending", indices=[2, 0, 1, 0, 3])                           # unsorted
    refused("strictly ascending", indices=[2, 2, 1, 0, 3])                           # duplicate
    refused("outside the minor dimension", indices=[0, 4, 1, 0, 3])                  # index out of range
    refused("outside the minor dimension", major_is_row=False, shape=(3, 3), indices=[0, 2, 1, 0, 3])
    refused("indptr", indptr=[0, 3, 2, 5])                                           # decreasing
    refused("indptr", indptr=[1, 2, 3, 5])                                           # does not start at 0
    refused("indptr", indptr=[0, 2, 7, 5])                                           # runs past the stored entries
    refused("useSparseOptimization", kwargs=dict(kw, sparseOptimization=False))
    refused("subsetData", kwargs=dict(kw, subsetIndices=np.array([1, 2], dtype=np.uint32), subsetDim=1))
    refused("COGAPS_REDUCE_SEQ", kwargs=dict(kw, reductionMode="seq"))
    # null pointers, straight through the C ABI
    p = _capi.make_params(lib, nPatterns=2, sparseOptimization=True)
    assert not lib.cogaps_session_create_sparse(None, ctypes.byref(p)) and b"null" in lib.cogaps_last_error()
    m = _c_matrix(**good)
    c = m.c_struct()
    assert not lib.cogaps_session_create_sparse(ctypes.byref(c), None) and b"null" in lib.cogaps_last_error()
    for field in ("indptr", "indices", "values"):
        c = m.c_struct()
        setattr(c, field, None)
        assert not lib.cogaps_session_create_sparse(ctypes.byref(c), ctypes.byref(p)) and b"null" in lib.cogaps_last_error(), field
    r = _capi.CogapsResultC()
    assert lib.cogaps_run_sparse(None, ctypes.byref(p), ctypes.byref(r)) != 0
    assert lib.cogaps_session_device_bytes(None, None) != 0
    # an empty matrix (no stored entry) is well formed
    S = _capi.Session(_c_matrix((3, 4), True, [0, 0, 0, 0], [], []), **kw)
    assert S.debug_sparse_data("A")["vals"].size == 0
    S.close()


def test_no_dense_array_is_kept_on_the_device(emul_lib):
    """a sparse-model session holds the packed data and nothing of the size of the matrix, whatever form its input had: the session
    from the dense matrix holds what the session from its CSR form holds, less than one genes x samples array of floats"""
    lib = emul_lib(256)
    genes, samples = 3000, 2500
    rng = np.random.default_rng(3)
    data = sp.random(genes, samples, density=0.01, format="csr", dtype=np.float32, random_state=rng)
    data.data[:] = np.ceil(data.data * 9)
    kw = dict(lib=lib, nPatterns=3, seed=1, sparseOptimization=True)
    S = _capi.Session(data, **kw)
    D = _capi.Session(data.toarray(), **kw)
    s_bytes, d_bytes = S.device_bytes(), D.device_bytes()
    print("device bytes: dense input %d, sparse input %d, one dense array %d" % (d_bytes, s_bytes, genes * samples * 4))
    assert d_bytes == s_bytes
    assert d_bytes < genes * samples * 4
    assert s_bytes > 0
    ref = pu.packed_reference(data.toarray(), 3)
    pu.assert_structures_equal(ref, pu.structures(D), "dense input")
    pu.assert_structures_equal(ref, pu.structures(S), "csr input")
    for w in "AP":
        a, b = D.debug_sparse_data(w), S.debug_sparse_data(w)
        assert np.array_equal(a["vals"], b["vals"]) and np.array_equal(a["flags"], b["flags"]) and a["lambda"] == b["lambda"]
    S.close(), D.close()


def test_front_end(emul_lib, oracle, monkeypatch):
    from cogaps_amd import CoGAPS
    lib = emul_lib(256)
    monkeypatch.setattr(_capi, "load", lambda: lib)
    data = pu.synthetic_counts(120, 40, zeros=0.8, seed=6)
    kw = dict(nPatterns=3, nIterations=30, seed=7, messages=False, outputFrequency=10)
    for extra in (dict(sparseOptimization=True), dict()):
        a, b = CoGAPS(sp.csr_matrix(data), **kw, **extra), CoGAPS(data, **kw, **extra)
        assert np.array_equal(a.featureLoadings, b.featureLoadings) and np.array_equal(a.sampleFactors, b.sampleFactors)
        assert a.metadata["meanChiSq"] == b.metadata["meanChiSq"]
    c = CoGAPS(sp.csc_matrix(data), sparseOptimization=True, **kw)
    assert np.array_equal(c.featureLoadings, CoGAPS(data, sparseOptimization=True, **kw).featureLoadings)
    with pytest.raises(ValueError, match="default uncertainty"):
        CoGAPS(sp.csr_matrix(data), uncertainty=np.ones_like(data), sparseOptimization=True, **kw)
    bad = sp.csr_matrix(data)
    bad.data[3] = -1.0
    with pytest.raises(ValueError, match="negative"):
        CoGAPS(bad, sparseOptimization=True, **kw)
    bad.data[3] = np.nan
    with pytest.raises(ValueError, match="NA values"):
        CoGAPS(bad, sparseOptimization=True, **kw)
    with pytest.raises(ValueError, match="nPatterns must be less"):
        CoGAPS(sp.csr_matrix(data[:, :3]), sparseOptimization=True, **kw)


WORKER = r'''
import os, sys, ctypes, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import scipy.sparse as sp
import torch.distributed as dist
from cogaps_amd import _capi, CogapsParams
from cogaps_amd.distributed import distributedCogaps
import parity_util as pu
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
lib = _capi.bind(ctypes.CDLL(os.path.join(%(root)r, "tests", "emul", "libcogaps_emul_TESTONLY_w256.so")))
data = pu.synthetic_counts(60, 160, zeros=0.7, seed=13)
p = CogapsParams(nPatterns=3, seed=5, nIterations=12, sparseOptimization=True)
p.distributed = "single-cell"; p.setDistributedParams(nSets=2, minNS=2)
run = lambda d, unc=None, **kw: _capi.run(d, unc=unc, lib=lib, **{k: v for k, v in kw.items() if k != "device"})
out = distributedCogaps(sp.csr_matrix(data) if sys.argv[3] == "sparse" else data, p, run_fn=run, outputFrequency=6)
np.savez(sys.argv[2], Amean=out["Amean"], Pmean=out["Pmean"], Psd=out["Psd"], consensus=out["consensus"], meanChiSq=out["meanChiSq"])
dist.destroy_process_group()
'''


def test_sccogaps_world2_sparse_equals_dense(tmp_path, emul_lib):
    """scCoGAPS over a world of two gloo ranks: the shards cut from a scipy.sparse matrix (and handed on in compressed form) give the
    run the shards cut from the dense matrix give"""
    emul_lib(256)
    script = tmp_path / "worker.py"
    res = {}
    for kind in ("sparse", "dense"):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        script.write_text(WORKER % {"root": ROOT, "port": port})
        outs = [str(tmp_path / ("%s%d.npz" % (kind, r))) for r in range(2)]
        procs = [subprocess.Popen([sys.executable, str(script), str(r), outs[r], kind]) for r in range(2)]
        assert all(p.wait(timeout=600) == 0 for p in procs)
        a, b = np.load(outs[0]), np.load(outs[1])
        for k in a.files:
            assert np.array_equal(a[k], b[k]), "ranks disagree on " + k
        res[kind] = a
    for k in res["dense"].files:
        assert np.array_equal(res["sparse"][k], res["dense"][k]), k
    assert res["sparse"]["Pmean"].shape[0] == 160 and res["sparse"]["Pmean"].any()
