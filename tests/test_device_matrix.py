"""The device-resident matrix (cogaps_device_matrix, csrc/sparse_build.h's map and mapped passes) on the test-only emulator build: a
session created from a handle -- with or without subsetData, in the default or the verification mode -- is the session the dense entry
makes from the dense form of the handle's matrix with the same parameters, bit for bit: against the definition of the structures in
numpy, against the dense-input session, against the oracle step by step, and through the front ends."""
import ctypes
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import parity_util as pu
from cogaps_amd import _capi
from test_coo_input import RESULT_FIELDS, coo_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def handle_of(lib, data, kind):
    """a handle of the dense matrix `data`: from its CSR or CSC form, or from shuffled triplets with 1 % repeated positions"""
    if kind == "coo":
        return _capi.DeviceMatrix(coo_of(data, 5, repeats=0.01), lib=lib)
    return _capi.DeviceMatrix(getattr(sp, kind + "_matrix")(data), lib=lib)


def subset_of(dim, n, repeated, seed):
    """n 1-based indices of 1 .. dim in shuffled order: the first and the last index among them, `repeated` of them twice"""
    rng = np.random.default_rng(seed)
    inner = rng.choice(np.arange(2, dim), n - repeated - 2, replace=False)
    idx = np.concatenate([[1, dim], inner])
    idx = np.concatenate([idx, rng.choice(idx, repeated, replace=False)])
    rng.shuffle(idx)
    assert idx.size == n and np.unique(idx).size == n - repeated and not np.array_equal(idx, np.sort(idx))
    return idx.astype(np.uint32)


def cut(data, idx, subset_dim, transpose):
    """the dense subset by the dense entry's rule (Matrix.cpp:30-69): genes are the rows of the data unless transposeData"""
    by_rows = (subset_dim == 1) != bool(transpose)
    return np.ascontiguousarray(data[idx - 1] if by_rows else data[:, idx - 1])


@pytest.fixture(scope="module")
def big():
    data = pu.synthetic_counts(400, 330, zeros=0.85, seed=12)
    assert int((data > 0).sum()) >= 10000
    return data


@pytest.fixture(scope="module")
def big_handles(emul_lib, big):
    hs = {kind: handle_of(emul_lib(256), big, kind) for kind in ("csr", "csc", "coo")}
    yield hs
    for h in hs.values():
        h.close()


# ---- structures ----

@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("subset_dim", [1, 2])
@pytest.mark.parametrize("n,repeated", [(150, 10), (128, 0)])
def test_subset_structures(emul_lib, big, big_handles, subset_dim, transpose, n, repeated):
    """one upload per form, then a session per (subset axis, transposeData): against numpy's packing of the numpy-cut subset and,
    array for array, against the dense-input session given the same subsetIndices"""
    lib = emul_lib(256)
    dim = big.shape[0] if (subset_dim == 1) != transpose else big.shape[1]
    idx = subset_of(dim, n, repeated, seed=subset_dim * 2 + transpose)
    kw = dict(lib=lib, nPatterns=5, seed=2, sparseOptimization=True, transposeData=transpose, subsetIndices=idx, subsetDim=subset_dim)
    ref = pu.packed_reference(cut(big, idx, subset_dim, transpose), 5, transposeData=transpose)
    D = _capi.Session(big, **kw)
    d = pu.structures(D)
    pu.assert_structures_equal(ref, d, "dense input")
    for kind, dm in big_handles.items():
        S = _capi.Session(dm, **kw)
        s = pu.structures(S)
        pu.assert_structures_equal(ref, s, kind + " handle")
        pu.assert_structures_equal(d, s, kind + " handle against the dense-input session")
        for w in "AP":
            assert s[w]["flags"].shape[1] > 1
            assert np.float32(D.chisq(w)).tobytes() == np.float32(S.chisq(w)).tobytes()
        assert S.device_bytes() == D.device_bytes()
        S.close()
    D.close()


@pytest.mark.parametrize("transpose", [False, True])
def test_without_a_subset_the_session_is_the_sparse_entries(emul_lib, big, big_handles, transpose):
    lib = emul_lib(256)
    kw = dict(lib=lib, nPatterns=5, seed=2, sparseOptimization=True, transposeData=transpose)
    ref = pu.packed_reference(big, 5, transposeData=transpose)
    for kind, dm in big_handles.items():
        E = _capi.Session(coo_of(big, 5, repeats=0.01) if kind == "coo" else getattr(sp, kind + "_matrix")(big), **kw)
        S = _capi.Session(dm, **kw)
        pu.assert_structures_equal(ref, pu.structures(S), kind + " handle")
        pu.assert_structures_equal(pu.structures(E), pu.structures(S), kind)
        assert S.device_bytes() == E.device_bytes()
        E.close(), S.close()


def test_handle_info(emul_lib, big, big_handles):
    for kind, dm in big_handles.items():
        assert dm.shape == big.shape and dm.device == 0
        assert dm.nnz == int((big > 0).sum()) if kind != "coo" else dm.nnz > int((big > 0).sum())
        # the input arrays (one element of padding each) and, for triplets, one keep bit per entry
        want = (8 * (big.shape[kind == "csc"] + 2) + 8 * (dm.nnz + 1)) if kind != "coo" else 12 * (dm.nnz + 1) + 8 * (dm.nnz // 64 + 1)
        assert dm.device_bytes() == want


# ---- step by step against the oracle ----

def _stepwise_data():
    data = pu.synthetic_counts(240, 36, zeros=0.8, seed=9)
    return data


STEP_KW = dict(trace=True, nPatterns=4, seed=3, total_iter=40, sparseOptimization=True)


@pytest.mark.parametrize("kind", ["csr", "csc", "coo"])
def test_stepwise_major_and_minor_axis_subsets(emul_lib, kind):
    lib = emul_lib(256)
    data = _stepwise_data()
    with handle_of(lib, data, kind) as dm:
        idx = subset_of(240, 100, 6, seed=1)
        pu.run_stepwise(lib, dm, 20, oracle_data=data[idx - 1], subsetIndices=idx, subsetDim=1, **STEP_KW)
        idx = subset_of(36, 24, 3, seed=2)
        pu.run_stepwise(lib, dm, 20, oracle_data=data[:, idx - 1], subsetIndices=idx, subsetDim=2, **STEP_KW)


def test_stepwise_fixed_matrix_and_transposed(emul_lib):
    lib = emul_lib(256)
    data = _stepwise_data()
    idx = subset_of(240, 100, 6, seed=3)
    fixed = np.abs(np.random.default_rng(2).normal(0.5, 0.4, (36, 4))).astype(np.float32)
    fixed[fixed < 0.3] = 0.0
    with handle_of(lib, data, "csc") as dm:
        pu.run_stepwise(lib, dm, 20, oracle_data=data[idx - 1], subsetIndices=idx, subsetDim=1, whichMatrixFixed="P", fixedPatterns=fixed,
                        **dict(STEP_KW, trace=False))
    transposed = np.ascontiguousarray(data.T)          # samples x genes: subsetDim = 2 (samples) picks its rows
    idx = subset_of(36, 24, 3, seed=4)
    with handle_of(lib, transposed, "coo") as dm:
        pu.run_stepwise(lib, dm, 20, oracle_data=transposed[idx - 1], subsetIndices=idx, subsetDim=2, transposeData=True, **STEP_KW)


@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_stepwise_zero_row_selected_and_bad_entries_unselected(emul_lib, fmt):
    """a selected all-zero row; the matrix's only stored negative and NaN entries sit in a row the subset leaves out (and, stored in
    the handle all the same, are dropped wherever they are: the second run selects that row)"""
    lib = emul_lib(256)
    data = _stepwise_data()
    data[17, :] = 0.0
    stored = data.copy()
    stored[30, [2, 9]] = [-3.0, np.nan]
    data[30, [2, 9]] = 0.0
    m = sp.coo_matrix(np.where(np.isnan(stored), 1.0, stored))
    vals = stored[m.row, m.col]
    m = getattr(sp.coo_matrix((vals, (m.row, m.col)), shape=data.shape), "to" + fmt)()
    assert np.isnan(m.data).sum() == 1 and (m.data < 0).sum() == 1
    idx = np.array([k for k in subset_of(240, 100, 6, seed=5) if k != 31] + [18], dtype=np.uint32)
    with _capi.DeviceMatrix(m, lib=lib) as dm:
        assert dm.has_na and dm.has_negative
        pu.run_stepwise(lib, dm, 20, oracle_data=data[idx - 1], subsetIndices=idx, subsetDim=1, **STEP_KW)
        idx = np.concatenate([idx[:40], [31]]).astype(np.uint32)
        pu.run_stepwise(lib, dm, 10, oracle_data=data[idx - 1], subsetIndices=idx, subsetDim=1, **dict(STEP_KW, trace=False))


# ---- the verification mode ----

@pytest.mark.parametrize("subset", [False, True])
def test_verification_mode_full_run(emul_lib, oracle, subset):
    lib = emul_lib(256)
    data = pu.synthetic_counts(150, 30, zeros=0.8, seed=21)
    kw = dict(nPatterns=4, nIterations=40, seed=42, outputFrequency=10, sparseOptimization=True)
    idx = subset_of(150, 90, 5, seed=6) if subset else None
    sub = dict(subsetIndices=idx, subsetDim=1) if subset else {}
    with handle_of(lib, data, "csr") as dm:
        r = _capi.run(dm, lib=lib, reductionMode="seq", mathMode="glibc-fma", **kw, **sub)
    d = _capi.run(data, lib=lib, reductionMode="seq", mathMode="glibc-fma", **kw, **sub)
    o = oracle.run(data[idx - 1] if subset else data, math_mode=oracle.MATH_GLIBC_FMA, redW_A=1, redW_P=1, redG=1, **kw)
    for f in RESULT_FIELDS:
        assert np.array_equal(r[f], o[f]), f
        assert np.array_equal(r[f], d[f]), f
    assert r["totalUpdates"] == o["totalUpdates"] == d["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"] == d["meanChiSq"]


# ---- many sessions from one handle ----

def _same(a, b):
    for f in RESULT_FIELDS:
        assert np.array_equal(a[f], b[f]), f
    assert a["totalUpdates"] == b["totalUpdates"] and a["meanChiSq"] == b["meanChiSq"]


def test_many_sessions_from_one_handle(emul_lib):
    lib = emul_lib(256)
    data = pu.synthetic_counts(120, 40, zeros=0.8, seed=6)
    csr = sp.csr_matrix(data)
    cases = [dict(nPatterns=k, seed=s) for k in (2, 5, 9) for s in (7, 8)]
    common = dict(lib=lib, nIterations=6, outputFrequency=3, sparseOptimization=True)
    dm = _capi.DeviceMatrix(csr, lib=lib)
    sessions = [_capi.Session(dm, **common, **c) for c in cases]
    dm.close()                                        # the sessions hold nothing of the handle
    with pytest.raises(ValueError, match="closed"):
        _capi.Session(dm, **common, **cases[0])
    for S, c in zip(sessions, cases):
        for phase in (1, 2):
            S.run_iterations(phase, 0, 6)
        _same(S.finish(), _capi.run(csr, **common, **c))
        S.close()


def test_two_threads_create_sessions_from_one_handle(emul_lib, big, big_handles):
    lib = emul_lib(256)
    idx = [subset_of(400, 150, 10, seed=7), subset_of(330, 128, 0, seed=8)]
    kws = [dict(lib=lib, nPatterns=3 + t, seed=2, sparseOptimization=True, subsetIndices=idx[t], subsetDim=t + 1) for t in range(2)]
    got, errors = [None, None], []

    def work(t):
        try:
            for kind in ("csr", "csc", "coo"):
                S = _capi.Session(big_handles[kind], **kws[t])
                got[t] = pu.structures(S)
                S.close()
        except Exception as e:      # noqa: BLE001 -- handed to the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    [t.start() for t in threads], [t.join() for t in threads]
    assert not errors, errors
    for t in range(2):
        D = _capi.Session(big, **kws[t])
        pu.assert_structures_equal(pu.structures(D), got[t], "thread %d" % t)
        D.close()


def test_two_subset_sessions_in_a_batch_equal_the_two_alone(emul_lib):
    lib = emul_lib(256)
    data = pu.synthetic_counts(200, 60, zeros=0.8, seed=40)
    kws = [dict(seed=5, subsetIndices=np.arange(1, 101, dtype=np.uint32), subsetDim=1), dict(seed=6, subsetIndices=np.arange(200, 100, -1).astype(np.uint32), subsetDim=1)]
    common = dict(nPatterns=3, nIterations=12, outputFrequency=6, sparseOptimization=True)
    with handle_of(lib, data, "csr") as dm:
        both = _capi.run_batch([dm, dm], lib=lib, kws=kws, **common)
    for k, b in zip(kws, both):
        _same(_capi.run(data, lib=lib, **common, **k), b)


# ---- errors ----

GOOD = dict(shape=(3, 4), major_is_row=True, indptr=[0, 2, 3, 5], indices=[0, 2, 1, 0, 3], values=[1, 2, 3, 4, 5])
GOOD_COO = dict(shape=(3, 4), rows=[0, 2, 1, 0, 2], cols=[0, 3, 1, 2, 0], values=[1, 2, 3, 4, 5])
KW = dict(nPatterns=2, seed=1, sparseOptimization=True)


def _csr(**change):
    g = dict(GOOD, **change)
    return _capi.SparseMatrix(g["shape"], g["major_is_row"], np.asarray(g["indptr"], dtype=np.uint64), np.asarray(g["indices"], dtype=np.uint32),
                              np.asarray(g["values"], dtype=np.float32))


def _still_works(lib):
    with _capi.DeviceMatrix(_csr(), lib=lib) as dm:
        S = _capi.Session(dm, lib=lib, **KW)
        assert S.debug_sparse_data("A")["vals"].size == 5
        S.close()


@pytest.mark.parametrize("match,change", [
    ("strictly ascending", dict(indices=[2, 0, 1, 0, 3])), ("strictly ascending", dict(indices=[2, 2, 1, 0, 3])),
    ("outside the minor dimension", dict(indices=[0, 4, 1, 0, 3])), ("outside the minor dimension", dict(major_is_row=False, shape=(3, 3))),
    ("indptr", dict(indptr=[0, 3, 2, 5])), ("indptr", dict(indptr=[1, 2, 3, 5])), ("indptr", dict(indptr=[0, 2, 7, 5])),
])
def test_malformed_csr_is_refused_at_handle_creation(emul_lib, match, change):
    lib = emul_lib(256)
    with pytest.raises(_capi.CogapsError, match=match):
        _capi.DeviceMatrix(_csr(**change), lib=lib)
    _still_works(lib)


@pytest.mark.parametrize("change", [dict(rows=[0, 3, 1, 0, 2]), dict(cols=[0, 2, 1, 4, 2]), dict(rows=[0, 2, 1, 0, 0xFFFFFFFF])])
def test_malformed_triplets_are_refused_at_handle_creation(emul_lib, change):
    lib = emul_lib(256)
    g = dict(GOOD_COO, **change)
    with pytest.raises(_capi.CogapsError, match="outside the stated dimensions"):
        _capi.DeviceMatrix(_capi.CooMatrix(g["shape"], g["rows"], g["cols"], g["values"]), lib=lib)
    _still_works(lib)


def test_too_many_triplets_and_null_arguments(emul_lib):
    lib = emul_lib(256)
    p = _capi.make_params(lib, **KW)
    c = _capi.CooMatrix(GOOD_COO["shape"], GOOD_COO["rows"], GOOD_COO["cols"], GOOD_COO["values"]).c_struct()
    c.nnz = 0xFFFFFFFF
    assert not lib.cogaps_device_matrix_create_coo(ctypes.byref(c), -1) and b"2^32 - 1 entries" in lib.cogaps_last_error()
    assert not lib.cogaps_device_matrix_create_sparse(None, -1) and b"null" in lib.cogaps_last_error()
    assert not lib.cogaps_device_matrix_create_coo(None, -1) and b"null" in lib.cogaps_last_error()
    keep = _csr()
    for field in ("indptr", "indices", "values"):
        c = keep.c_struct()
        setattr(c, field, None)
        assert not lib.cogaps_device_matrix_create_sparse(ctypes.byref(c), -1) and b"null" in lib.cogaps_last_error(), field
    keep = _capi.CooMatrix(GOOD_COO["shape"], GOOD_COO["rows"], GOOD_COO["cols"], GOOD_COO["values"])
    for field in ("rows", "cols", "values"):
        c = keep.c_struct()
        setattr(c, field, None)
        assert not lib.cogaps_device_matrix_create_coo(ctypes.byref(c), -1) and b"null" in lib.cogaps_last_error(), field
    with _capi.DeviceMatrix(_csr(), lib=lib) as dm:
        assert not lib.cogaps_session_create_from_device_matrix(None, ctypes.byref(p)) and b"null" in lib.cogaps_last_error()
        assert not lib.cogaps_session_create_from_device_matrix(dm.h, None) and b"null" in lib.cogaps_last_error()
        r = _capi.CogapsResultC()
        assert lib.cogaps_run_device_matrix(None, ctypes.byref(p), ctypes.byref(r)) != 0
        assert lib.cogaps_run_device_matrix(dm.h, ctypes.byref(p), None) != 0 and b"null" in lib.cogaps_last_error()
        assert lib.cogaps_device_matrix_info(None, None, None, None, None, None) != 0
        assert lib.cogaps_device_matrix_info(dm.h, None, None, None, None, None) == 0
    lib.cogaps_device_matrix_destroy(None)
    _still_works(lib)


@pytest.mark.parametrize("match,change", [
    ("useSparseOptimization", dict(sparseOptimization=False)),
    ("outside 1 .. 3", dict(subsetIndices=np.array([0, 1], dtype=np.uint32), subsetDim=1)),
    ("outside 1 .. 3", dict(subsetIndices=np.array([1, 4], dtype=np.uint32), subsetDim=1)),
    ("outside 1 .. 4", dict(subsetIndices=np.array([5, 1], dtype=np.uint32), subsetDim=2)),
    ("outside 1 .. 4", dict(subsetIndices=np.array([5, 1], dtype=np.uint32), subsetDim=1, transposeData=True)),
    ("empty", dict(subsetIndices=np.array([], dtype=np.uint32), subsetDim=1)),
    ("device", dict(device=5)),
])
def test_refusals_at_session_creation(emul_lib, match, change):
    lib = emul_lib(256)
    with _capi.DeviceMatrix(_csr(), lib=lib) as dm:
        with pytest.raises(_capi.CogapsError, match=match):
            _capi.Session(dm, lib=lib, **dict(KW, **change))
        S = _capi.Session(dm, lib=lib, device=0, subsetIndices=np.array([3, 3, 1], dtype=np.uint32), subsetDim=1, **KW)      # a valid session can still be made
        assert np.array_equal(S.debug_sparse_data("A")["vals"], np.array([4, 5, 4, 5, 1, 2], dtype=np.float32))
        S.close()


# ---- memory ----

def test_memory(emul_lib):
    """the handle's bytes are its own; a subset session holds what the dense-input session of the same subset holds: fewer bytes than
    the whole-matrix session, less than one dense array of the subset.  (The shape: a session's state beside its data -- atom arrays with
    room for 65536 atoms more than bins, queues and decision records per data vector -- does not depend on the entries and comes to some
    15 MB at these dimensions; a dense array of the subset, 2400 x 5000 floats = 48 MB, is well above it, so the assertion fails if one
    is held and cannot pass by accident.)"""
    lib = emul_lib(256)
    genes, samples = 6000, 5000
    data = sp.random(genes, samples, density=0.01, format="csr", dtype=np.float32, random_state=np.random.default_rng(3))
    data.data[:] = np.ceil(data.data * 9)
    kw = dict(lib=lib, nPatterns=3, seed=1, sparseOptimization=True)
    idx = subset_of(genes, 2400, 200, seed=9)
    with _capi.DeviceMatrix(data, lib=lib) as dm:
        W, S = _capi.Session(dm, **kw), _capi.Session(dm, subsetIndices=idx, subsetDim=1, **kw)
        E, D = _capi.Session(data, **kw), _capi.Session(data[idx - 1].toarray(), **kw)
        print("device bytes: handle %d, whole-matrix session %d, subset session %d, one dense array of the subset %d"
              % (dm.device_bytes(), W.device_bytes(), S.device_bytes(), idx.size * samples * 4))
        assert dm.device_bytes() == 8 * (genes + 2) + 8 * (data.nnz + 1)
        assert W.device_bytes() == E.device_bytes()          # nothing of the handle is counted
        assert S.device_bytes() == D.device_bytes()
        assert 0 < S.device_bytes() < W.device_bytes()
        assert S.device_bytes() < idx.size * samples * 4
        pu.assert_structures_equal(pu.structures(D), pu.structures(S), "subset session")
        W.close(), S.close(), E.close(), D.close()


# ---- the front ends ----

def test_front_end(emul_lib, monkeypatch, tmp_path):
    from cogaps_amd import CoGAPS, DeviceMatrix
    lib = emul_lib(256)
    monkeypatch.setattr(_capi, "load", lambda: lib)
    data = pu.synthetic_counts(120, 40, zeros=0.8, seed=6)
    kw = dict(nPatterns=3, nIterations=12, seed=7, messages=False, outputFrequency=6, sparseOptimization=True)

    def same(a, b):
        assert np.array_equal(a.featureLoadings, b.featureLoadings) and np.array_equal(a.sampleFactors, b.sampleFactors)
        assert np.array_equal(a.loadingStdDev, b.loadingStdDev) and a.metadata["meanChiSq"] == b.metadata["meanChiSq"]
    with DeviceMatrix(sp.csc_matrix(data)) as dm:
        assert dm.shape == (120, 40) and dm.nnz == int((data > 0).sum()) and dm.device_bytes() > 0
        same(CoGAPS(dm, **kw), CoGAPS(data, **kw))
        idx = subset_of(120, 70, 4, seed=10)
        same(CoGAPS(dm, subsetIndices=idx, subsetDim=1, **kw), CoGAPS(data, subsetIndices=idx, subsetDim=1, **kw))
        idx = subset_of(40, 20, 2, seed=11)
        same(CoGAPS(dm, subsetIndices=idx, subsetDim=2, **kw), CoGAPS(data, subsetIndices=idx, subsetDim=2, **kw))
        with pytest.raises(ValueError, match="dense model takes a dense matrix"):
            CoGAPS(dm, **dict(kw, sparseOptimization=False))
        with pytest.raises(ValueError, match="default uncertainty"):
            CoGAPS(dm, uncertainty=np.ones_like(data), **kw)
        with pytest.raises(ValueError, match="nPatterns must be less"):
            CoGAPS(dm, **dict(kw, nPatterns=40))
    # a .mtx path goes through the triplet reader; the host values are checked where the handle is built
    r, c = np.nonzero(data)
    path = str(tmp_path / "small.mtx")
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (data.shape + (r.size,)))
        f.writelines("%d %d %g\n" % (i + 1, j + 1, data[i, j]) for i, j in zip(r, c))
    with DeviceMatrix(path) as dm:
        assert dm.shape == data.shape and dm.nnz == r.size
        same(CoGAPS(dm, **kw), CoGAPS(data, **kw))
    bad = sp.csr_matrix(data)
    bad.data[3] = -1.0
    with DeviceMatrix(bad) as dm, pytest.raises(ValueError, match="negative"):
        CoGAPS(dm, **kw)
    bad.data[3] = np.nan
    with DeviceMatrix(bad) as dm, pytest.raises(ValueError, match="NA values"):
        CoGAPS(dm, **kw)
    with pytest.raises(TypeError):
        DeviceMatrix(data)


WORKER = r'''
import os, sys, ctypes, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import scipy.sparse as sp
from cogaps_amd import _capi, CogapsParams, GWCoGAPS, scCoGAPS, DeviceMatrix
import parity_util as pu
world = int(sys.argv[4])
if world > 1:
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=world)
lib = _capi.bind(ctypes.CDLL(os.path.join(%(root)r, "tests", "emul", "libcogaps_emul_TESTONLY_w256.so")))
_capi.load = lambda: lib
_capi._lib = lib
data = sp.csr_matrix(pu.synthetic_counts(60, 160, zeros=0.7, seed=13))
out = {}
for name, driver in (("gw", GWCoGAPS), ("sc", scCoGAPS)):
    p = CogapsParams(nPatterns=3, seed=5, nIterations=12, sparseOptimization=True)
    p.setDistributedParams(nSets=2, minNS=2)
    src = DeviceMatrix(data) if sys.argv[3] == "handle" else data
    r = driver(src, p, messages=False, outputFrequency=6)
    out.update({name + "A": r.featureLoadings, name + "P": r.sampleFactors, name + "Asd": r.loadingStdDev, name + "Psd": r.factorStdDev,
                name + "chi": r.metadata["meanChiSq"]})
np.savez(sys.argv[2], **out)
if world > 1:
    dist.destroy_process_group()
'''


@pytest.mark.parametrize("world", [1, 2])
def test_distributed_drivers_from_a_handle_equal_the_scipy_input_run(tmp_path, emul_lib, world):
    """GWCoGAPS and scCoGAPS with every shard's two passes created from the handle (subsetIndices = the shard's set): the result of
    the run whose shards are cut from the scipy.sparse matrix on the host"""
    emul_lib(256)
    script = tmp_path / "worker.py"
    res = {}
    for kind in ("handle", "scipy"):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        script.write_text(WORKER % {"root": ROOT, "port": port})
        outs = [str(tmp_path / ("%s%d.npz" % (kind, r))) for r in range(world)]
        procs = [subprocess.Popen([sys.executable, str(script), str(r), outs[r], kind, str(world)]) for r in range(world)]
        assert all(p.wait(timeout=600) == 0 for p in procs)
        loaded = [np.load(o) for o in outs]
        for k in loaded[0].files:
            assert all(np.array_equal(loaded[0][k], other[k]) for other in loaded[1:]), "ranks disagree on " + k
        res[kind] = loaded[0]
    for k in res["scipy"].files:
        assert np.array_equal(res["handle"][k], res["scipy"][k]), k
    assert res["handle"]["gwA"].shape[0] == 60 and res["handle"]["gwA"].any() and res["handle"]["scP"].shape[0] == 160 and res["handle"]["scP"].any()
