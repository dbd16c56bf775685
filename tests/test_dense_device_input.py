"""Dense input resident on the "device" (csrc/dense_build.h; cogaps_session_create with data_on_device = 1, cogaps_run_device) on the
test-only emulator build, where device addresses are host addresses: a session built from _capi.DeviceDense is, byte for byte, the
session the host-pointer entry builds from the same numpy matrix -- the dense model's D / Sraw / S2 with their pads and its constants,
the sparse model's packed structures, the bytes the session owns, and every step of the chain after that.  Each of the two
dense-model sessions is also compared, as bytes, with parity_util.dense_reference: numpy's statement of what such a session holds,
which depends on neither builder."""
import numpy as np
import pytest

import parity_util as pu
from cogaps_amd import _capi

SHAPES = [(37, 70), (130, 65), (5, 260)]
# N % 4 != 0 on one sampler and == 0 on the other; dimensions on both sides of the 64-wide tile and flag word, and past several of them
assert any(sorted(n % 4 != 0 for n in sh) == [False, True] for sh in SHAPES) and {n // 64 for sh in SHAPES for n in sh} >= {0, 1, 2, 4}
# what a result holds besides the two wall-clock fields (totalRunningTime, samplerSeconds), which no two runs share
RESULT_KEYS = ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP", "totalUpdates", "meanChiSq", "seed", "averageQueueLengthA",
               "averageQueueLengthP", "equilibrationSnapshotsA", "equilibrationSnapshotsP", "samplingSnapshotsA", "samplingSnapshotsP")


def matrix(nrow, ncol, seed=0):
    """about 80 % zeros, an all-zero row and an all-zero column, the rest counts 1 .. 9 scaled by a non-dyadic factor"""
    rng = np.random.default_rng(1000 * nrow + ncol + seed)
    d = (np.ceil(rng.random((nrow, ncol)) * 9) * np.float32(1.3)).astype(np.float32) * (rng.random((nrow, ncol)) >= 0.8)
    d[nrow // 2, :] = 0
    d[:, ncol // 3] = 0
    assert 0.7 < (d == 0).mean() < 0.9 and (d > 0).any(axis=1).sum() == nrow - 1
    return np.ascontiguousarray(d, dtype=np.float32)


def uncertainty(d):
    return np.ascontiguousarray(np.maximum(d * np.float32(0.2), np.float32(0.3)) + np.float32(0.01) * (np.arange(d.size, dtype=np.float32).reshape(d.shape) % 7))


def subset(dim, seed):
    """1-based indices of 1 .. dim: unsorted (dim comes before 1), with repeated indices"""
    base = np.random.default_rng(seed).permutation(dim)[:max(3, (2 * dim) // 3)] + 1
    idx = np.concatenate([[dim, 1], base, base[:2]]).astype(np.uint32)
    assert not np.array_equal(idx, np.sort(idx)) and np.unique(idx).size < idx.size
    return idx


def device_dense(d, u=None):
    return _capi.DeviceDense(d.shape, d.ctypes.data, None if u is None else u.ctypes.data, keep=(d, u))


def bits(x):
    return np.float32(x).tobytes()


def assert_dense_equal(H, S, tag, ref):
    """H (host pointers) and S (DeviceDense) each against ref (pu.dense_reference of their input), then against each other"""
    for w in "AP":
        a, b = H.debug_dense_data(w), S.debug_dense_data(w)
        m, n, _ = H.dims(w)
        assert S.dims(w) == H.dims(w) and a["D"].shape == (m, (n + 3) & ~3) == ref[w]["D"].shape
        for name, got in (("host pointers", a), ("device pointers", b)):
            for f in ("D", "Sraw", "S2"):
                assert (got[f] is None) == (ref[w][f] is None), "%s %s, %s: %s kept, the reference says otherwise" % (tag, w, name, f)
                if got[f] is not None:
                    assert got[f].tobytes() == ref[w][f].tobytes(), "%s %s, %s: %s differs from the reference" % (tag, w, name, f)
            for f in ("lambda", "maxGibbsMass", "sparsity"):
                assert bits(got[f]) == bits(ref[w][f]), "%s %s, %s: %s is %r, the reference has %r" % (tag, w, name, f, got[f], ref[w][f])
        for f in ("D", "Sraw", "S2"):
            assert (a[f] is None) == (b[f] is None), "%s %s: %s kept by one session only" % (tag, w, f)
            if a[f] is not None:
                assert a[f].tobytes() == b[f].tobytes(), "%s %s: %s differs" % (tag, w, f)
        if n % 4:      # the pads: D = 0, Sraw = S2 = 1
            assert (b["D"][:, n:] == 0).all() and (b["Sraw"][:, n:] == 1).all() and (b["S2"] is None or (b["S2"][:, n:] == 1).all())
        for f in ("lambda", "maxGibbsMass", "sparsity"):
            assert bits(a[f]) == bits(b[f]), "%s %s: %s differs (%r, %r)" % (tag, w, f, a[f], b[f])
    assert S.device_bytes() == H.device_bytes(), tag + ": device bytes differ"


def subset_kw(shape, which, transpose):
    """which: 0 none, 1 genes, 2 samples (genes are the rows of the data unless transposeData)"""
    if not which:
        return {}
    dim = shape[0] if (which == 1) != transpose else shape[1]
    return dict(subsetIndices=subset(dim, 10 * which + transpose), subsetDim=which)


def check_structures(lib, dd, shape, transpose, which):
    d = matrix(*shape)
    u = uncertainty(d)
    sub = subset_kw(shape, which, transpose)
    kw = dict(lib=lib, nPatterns=3, seed=4, transposeData=transpose, **sub)
    for unc in (None, u):
        H, S = _capi.Session(d, unc=unc, **kw), _capi.Session(dd(d, unc), **kw)
        assert (H.debug_dense_data("A")["S2"] is None) == (unc is None)
        assert_dense_equal(H, S, "dense model, unc %s" % (unc is not None), pu.dense_reference(d, unc, 3, transpose, **sub))
        H.close(), S.close()
    H, S = _capi.Session(d, sparseOptimization=True, **kw), _capi.Session(dd(d), sparseOptimization=True, **kw)
    pu.assert_structures_equal(pu.structures(H), pu.structures(S), "sparse model")
    assert S.device_bytes() == H.device_bytes()
    H.close(), S.close()


def check_a_negative_value_and_a_negative_zero(lib, dd, shape):
    """at the C level (the front end refuses negative data): the dense model keeps the negative value in D and in lambda's sum, the
    sparse model drops it; -0.0 stays -0.0 in D and is no entry of the sparse model"""
    d = matrix(*shape)
    d[1, 2], d[2, 1] = np.float32(-2.5), np.float32(-0.0)
    plain = d.copy()
    plain[1, 2] = 0
    kw = dict(lib=lib, nPatterns=3, seed=4)
    H, S, Z = _capi.Session(d, **kw), _capi.Session(dd(d), **kw), _capi.Session(plain, **kw)
    assert_dense_equal(H, S, "dense model", pu.dense_reference(d, None, 3))
    D = S.debug_dense_data("A")
    assert D["D"][1, 2] == np.float32(-2.5) and D["D"][2, 1].tobytes() == np.float32(-0.0).tobytes()
    assert bits(D["lambda"]) != bits(Z.debug_dense_data("A")["lambda"]), "the negative value is not in the sum"
    H.close(), S.close(), Z.close()
    kw["sparseOptimization"] = True
    H, S, Z = _capi.Session(d, **kw), _capi.Session(dd(d), **kw), _capi.Session(plain, **kw)
    pu.assert_structures_equal(pu.structures(H), pu.structures(S), "sparse model")
    pu.assert_structures_equal(pu.structures(Z), pu.structures(S), "sparse model: the negative value is an entry")
    H.close(), S.close(), Z.close()


seq_sum, lam = pu.seq_sum, pu.lam


def wide_range_matrix():
    rng = np.random.default_rng(77)
    d = (10.0 ** rng.uniform(-3, 4, (130, 65))).astype(np.float32) * (rng.random((130, 65)) >= 0.5)
    return np.ascontiguousarray(d, dtype=np.float32)


def check_the_order_of_the_sum(lib, dd):
    """values over seven decades: each sampler's lambda comes from ITS one-accumulator sum, and here no other order of addition gives it"""
    d = wide_range_matrix()
    nnz = int((d > 0).sum())
    want = {}
    for w, m in (("A", d), ("P", d.T)):      # A's vectors are the rows, P's the columns
        s, pairwise = seq_sum(m), np.sum(np.ascontiguousarray(m), dtype=np.float32)
        assert bits(s) != bits(pairwise), "numpy's pairwise sum equals the ordered sum: the data does not test the order"
        assert bits(lam(s, nnz, 3)) != bits(lam(pairwise, nnz, 3))
        want[w] = lam(s, nnz, 3)
    assert bits(seq_sum(d)) != bits(seq_sum(d.T))
    H, S = _capi.Session(d, lib=lib, nPatterns=3, seed=1), _capi.Session(dd(d), lib=lib, nPatterns=3, seed=1)
    for w in "AP":
        h, s = H.debug_dense_data(w)["lambda"], S.debug_dense_data(w)["lambda"]
        print("lambda %s: host pointers %r, device pointers %r, numpy's ordered sum %r" % (w, h, s, float(want[w])))
        assert bits(s) == bits(h) and bits(s) == bits(want[w])
    assert_dense_equal(H, S, "wide range", pu.dense_reference(d, None, 3))
    H.close(), S.close()


def check_stepwise(lib, dd, sparse, fixed):
    d = matrix(37, 70)
    kw = dict(lib=lib, nPatterns=3, seed=11, nIterations=6, sparseOptimization=sparse)
    if fixed == "P":
        kw.update(whichMatrixFixed="P", fixedPatterns=np.abs(np.random.default_rng(2).normal(size=(70, 3))).astype(np.float32))
    H, S = _capi.Session(d, **kw), _capi.Session(dd(d), **kw)
    for phase in (1, 2):
        assert H.run_iterations(phase, 0, 6) == S.run_iterations(phase, 0, 6)
        for w in "AP":
            assert np.array_equal(H.matrix(w), S.matrix(w)), "factor matrix " + w
            a, b = H.atoms(w), S.atoms(w)
            for f in ("pos", "mass", "left", "right"):
                assert np.array_equal(a[f], b[f]), "atoms %s %s" % (w, f)
            assert bits(H.chisq(w)) == bits(S.chisq(w))
    H.close(), S.close()


def check_run_device_equals_run(lib, dd, sparse):
    d = matrix(37, 70)
    u = None if sparse else uncertainty(d)
    kw = dict(lib=lib, nPatterns=3, seed=5, nIterations=8, outputFrequency=4, sparseOptimization=sparse, nSnapshots=2, snapshotPhase="all",
              subsetIndices=subset(37, 3), subsetDim=1)
    a, b = _capi.run(d, unc=u, **kw), _capi.run(dd(d, u), **kw)
    assert set(a) == set(b) == set(RESULT_KEYS) | {"totalRunningTime", "samplerSeconds"}
    for f in RESULT_KEYS:
        assert np.array_equal(a[f], b[f]), f
    assert a["chisq"].size == 4


def check_refusals(lib, dd):
    d = matrix(37, 70)
    with pytest.raises(_capi.CogapsError, match="null argument: data"):
        _capi.Session(_capi.DeviceDense(d.shape, 0), lib=lib, nPatterns=3)
    for sparse in (False, True):
        with pytest.raises(_capi.CogapsError, match="dataIndicesSubset holds an index outside 1 .. 37"):
            _capi.Session(dd(d), lib=lib, nPatterns=3, sparseOptimization=sparse, subsetIndices=[1, 38, 2], subsetDim=1)
    with pytest.raises(_capi.CogapsError, match="does not run the dense model"):
        _capi.Session(dd(d), lib=lib, nPatterns=3, sparseOptimization=True).debug_dense_data("A")


# ---- the emulator build: "device" addresses are numpy's ----

@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_structures(emul_lib, shape, transpose, which):
    check_structures(emul_lib(256), device_dense, shape, transpose, which)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_negative_value_and_a_negative_zero(emul_lib, shape):
    check_a_negative_value_and_a_negative_zero(emul_lib(256), device_dense, shape)


def test_the_order_of_the_sum(emul_lib):
    check_the_order_of_the_sum(emul_lib(256), device_dense)


@pytest.mark.parametrize("sparse,fixed", [(False, "N"), (True, "N"), (False, "P")])
def test_stepwise(emul_lib, sparse, fixed):
    check_stepwise(emul_lib(256), device_dense, sparse, fixed)


@pytest.mark.parametrize("sparse", [False, True])
def test_run_device_equals_run(emul_lib, sparse):
    check_run_device_equals_run(emul_lib(256), device_dense, sparse)


def test_refusals(emul_lib):
    check_refusals(emul_lib(256), device_dense)
