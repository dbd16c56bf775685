"""The device-resident matrix on the MI355X (product library): the map and the mapped passes of csrc/sparse_build.h -- counts, fill,
flag bits and stores through the images of a subset -- against the dense-input session, numpy's packing and the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

import parity_util as pu
from test_coo_input import RESULT_FIELDS, coo_of, densify
from test_device_matrix import STEP_KW, cut, handle_of, subset_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("subset_dim,transpose", [(1, False), (2, False), (1, True), (2, True)])
def test_subset_structures_gpu(hip_lib, subset_dim, transpose):
    """400 x 330, a shuffled subset of 150 with 10 repeats and one of exactly 128, handles from CSR, CSC and triplets with repeats"""
    from cogaps_amd import _capi
    big = pu.synthetic_counts(400, 330, zeros=0.85, seed=12)
    handles = {kind: handle_of(hip_lib, big, kind) for kind in ("csr", "csc", "coo")}
    dim = big.shape[0] if (subset_dim == 1) != transpose else big.shape[1]
    for n, repeated in ((150, 10), (128, 0)):
        idx = subset_of(dim, n, repeated, seed=subset_dim * 2 + transpose)
        kw = dict(lib=hip_lib, nPatterns=5, seed=2, sparseOptimization=True, transposeData=transpose, subsetIndices=idx, subsetDim=subset_dim)
        ref = pu.packed_reference(cut(big, idx, subset_dim, transpose), 5, transposeData=transpose)
        D = _capi.Session(big, **kw)
        d = pu.structures(D)
        for kind, dm in handles.items():
            S = _capi.Session(dm, **kw)
            s = pu.structures(S)
            pu.assert_structures_equal(ref, s, kind + " handle")
            pu.assert_structures_equal(d, s, kind + " handle against the dense-input session")
            for w in "AP":
                assert np.float32(D.chisq(w)).tobytes() == np.float32(S.chisq(w)).tobytes()
            assert S.device_bytes() == D.device_bytes()
            S.close()
        D.close()
    for dm in handles.values():
        dm.close()


@pytest.mark.parametrize("kind,subset_dim", [("csr", 2), ("coo", 1)])
def test_stepwise_gpu(hip_lib, kind, subset_dim):
    """a minor-axis subset of a CSR handle, a row subset of a triplet handle: 20 iterations with traces against the oracle"""
    data = pu.synthetic_counts(240, 36, zeros=0.8, seed=9)
    idx = subset_of(240, 100, 6, seed=1) if subset_dim == 1 else subset_of(36, 24, 3, seed=2)
    with handle_of(hip_lib, data, kind) as dm:
        pu.run_stepwise(hip_lib, dm, 20, oracle_data=cut(data, idx, subset_dim, False), subsetIndices=idx, subsetDim=subset_dim, **STEP_KW)


@pytest.mark.parametrize("subset", [False, True])
def test_verification_mode_full_run_gpu(hip_lib, oracle, subset):
    from cogaps_amd import _capi
    data = pu.synthetic_counts(150, 30, zeros=0.8, seed=21)
    kw = dict(nPatterns=4, nIterations=40, seed=42, outputFrequency=10, sparseOptimization=True)
    idx = subset_of(150, 90, 5, seed=6) if subset else None
    sub = dict(subsetIndices=idx, subsetDim=1) if subset else {}
    with handle_of(hip_lib, data, "csr") as dm:
        r = _capi.run(dm, lib=hip_lib, reductionMode="seq", mathMode="glibc-fma", **kw, **sub)
    d = _capi.run(data, lib=hip_lib, reductionMode="seq", mathMode="glibc-fma", **kw, **sub)
    o = oracle.run(data[idx - 1] if subset else data, math_mode=oracle.MATH_GLIBC_FMA, redW_A=1, redW_P=1, redG=1, **kw)
    for f in RESULT_FIELDS:
        assert np.array_equal(r[f], o[f]), f
        assert np.array_equal(r[f], d[f]), f
    assert r["totalUpdates"] == o["totalUpdates"] == d["totalUpdates"] and r["meanChiSq"] == o["meanChiSq"] == d["meanChiSq"]


def test_handle_from_device_pointers_equals_the_host_pointer_handle(hip_lib):
    """onDevice = 1: the arrays placed with torch, the handle copies them device to device and they may go right after"""
    import torch
    from cogaps_amd import _capi
    data = pu.synthetic_counts(700, 260, zeros=0.85, seed=31)
    m = _capi.SparseMatrix.from_scipy(sp.csr_matrix(data))
    c = coo_of(data, 2, repeats=0.02)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = [torch.from_numpy(a.view(v)).to(dev) for a, v in ((m.indptr, np.int64), (m.indices, np.int32), (m.values, np.float32),
                                                             (c.rows, np.int32), (c.cols, np.int32), (c.values, np.float32))]
    torch.cuda.synchronize()
    on_dev = [_capi.DeviceMatrix(_capi.SparseMatrix(m.shape, True, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), on_device=True), lib=hip_lib),
              _capi.DeviceMatrix(_capi.CooMatrix(c.shape, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), on_device=True, nnz=c.nnz), lib=hip_lib)]
    del t
    torch.cuda.empty_cache()
    on_host = [_capi.DeviceMatrix(m, lib=hip_lib), _capi.DeviceMatrix(c, lib=hip_lib)]
    idx = subset_of(700, 300, 20, seed=3)
    kw = dict(lib=hip_lib, nPatterns=5, nIterations=30, seed=3, sparseOptimization=True, subsetIndices=idx, subsetDim=1)
    ref = pu.packed_reference(data[idx - 1], 5)
    for a, b in zip(on_dev, on_host):
        assert a.has_na is None and b.has_na is False and a.device_bytes() == b.device_bytes() and a.nnz == b.nnz
        A, B = _capi.Session(a, **kw), _capi.Session(b, **kw)
        pu.assert_structures_equal(ref, pu.structures(A), "device-pointer handle")
        pu.assert_structures_equal(ref, pu.structures(B), "host-pointer handle")
        assert A.device_bytes() == B.device_bytes()
        for phase in (1, 2):
            assert A.run_iterations(phase, 0, 30) == B.run_iterations(phase, 0, 30)
        ra, rb = A.finish(), B.finish()
        for f in RESULT_FIELDS:
            assert np.array_equal(ra[f], rb[f]), f
        A.close(), B.close(), a.close(), b.close()


def test_structures_and_memory(hip_lib):
    """3000 x 2500 at density 0.02, 1200 shuffled row indices of which 100 repeat, and a column subset: against the dense-input session
    given the same indices; the handle's bytes are its own"""
    from cogaps_amd import _capi
    genes, samples = 3000, 2500
    data = sp.random(genes, samples, density=0.02, format="csr", dtype=np.float32, random_state=np.random.default_rng(3))
    data.data[:] = np.ceil(data.data * 9)
    dense = data.toarray()
    kw = dict(lib=hip_lib, nPatterns=3, seed=1, sparseOptimization=True)
    handles = {"csr": _capi.DeviceMatrix(data, lib=hip_lib), "csc": _capi.DeviceMatrix(data.tocsc(), lib=hip_lib),
               "coo": _capi.DeviceMatrix(coo_of(dense, 4, repeats=0.01), lib=hip_lib)}
    assert handles["csr"].device_bytes() == 8 * (genes + 2) + 8 * (data.nnz + 1)
    W = _capi.Session(handles["csr"], **kw)
    for subset_dim, dim in ((1, genes), (2, samples)):
        idx = subset_of(dim, 1200, 100, seed=9 + subset_dim)
        D = _capi.Session(dense, subsetIndices=idx, subsetDim=subset_dim, **kw)
        d = pu.structures(D)
        assert d["A"]["vals"].size > 10000
        for kind, dm in handles.items():
            S = _capi.Session(dm, subsetIndices=idx, subsetDim=subset_dim, **kw)
            pu.assert_structures_equal(d, pu.structures(S), "%s handle, subsetDim %d" % (kind, subset_dim))
            print("device bytes: %s handle %d, whole-matrix session %d, subset session %d, dense-input subset session %d"
                  % (kind, dm.device_bytes(), W.device_bytes(), S.device_bytes(), D.device_bytes()))
            assert S.device_bytes() == D.device_bytes() and 0 < S.device_bytes() < W.device_bytes()
            S.close()
        D.close()
    ref = pu.packed_reference(cut(dense, idx, 2, False), 3)
    pu.assert_structures_equal(ref, d, "dense input")
    W.close()
    for dm in handles.values():
        dm.close()


def test_contention(hip_lib):
    """one subset index repeated 2000 times -- every entry of that row has 2000 images -- over a handle built from 200 000 triplets on 50
    positions (thousands of entries meet at one present bit and one winner word when the handle is created)"""
    from cogaps_amd import _capi
    rng = np.random.default_rng(8)
    pos = rng.choice(130 * 70, 50, replace=False)
    pick = rng.integers(0, 50, 200000)
    r, c = np.unravel_index(pos[pick], (130, 70))
    v = np.where(np.arange(200000) % 2 == 0, 1.0 + (np.arange(200000) % 7), 0.0).astype(np.float32)
    dense = densify((130, 70), r, c, v)
    assert 5 < int((dense > 0).sum()) < 45
    hot = int(np.argmax((dense > 0).sum(axis=1))) + 1
    assert (dense[hot - 1] > 0).sum() >= 1
    idx = np.concatenate([np.full(2000, hot), np.arange(1, 131)]).astype(np.uint32)
    np.random.default_rng(9).shuffle(idx)
    kw = dict(lib=hip_lib, nPatterns=3, seed=1, sparseOptimization=True)
    with _capi.DeviceMatrix(_capi.CooMatrix((130, 70), r, c, v), lib=hip_lib) as dm, _capi.DeviceMatrix(sp.csc_matrix(dense), lib=hip_lib) as dc:
        for sub in (dict(subsetIndices=idx, subsetDim=1), dict()):
            D = _capi.Session(dense, **kw, **sub)
            d = pu.structures(D)
            pu.assert_structures_equal(pu.packed_reference(dense[idx - 1] if sub else dense, 3), d, "dense input")
            for name, h in (("triplet", dm), ("csc", dc)):
                S = _capi.Session(h, **kw, **sub)
                pu.assert_structures_equal(d, pu.structures(S), name + " handle")
                S.close()
            D.close()


def test_two_subset_sessions_of_one_handle_in_a_batch_equal_the_two_alone(hip_lib):
    from cogaps_amd import _capi
    data = pu.synthetic_counts(300, 90, zeros=0.8, seed=40)
    kws = [dict(seed=5, subsetIndices=subset_of(300, 150, 8, seed=1), subsetDim=1), dict(seed=6, subsetIndices=subset_of(300, 150, 8, seed=2), subsetDim=1)]
    common = dict(nPatterns=4, nIterations=40, outputFrequency=10, sparseOptimization=True)
    with handle_of(hip_lib, data, "csr") as dm:
        both = _capi.run_batch([dm, dm], lib=hip_lib, kws=kws, **common)
        for k, b in zip(kws, both):
            one, dense = _capi.run(dm, lib=hip_lib, **common, **k), _capi.run(data, lib=hip_lib, **common, **k)
            for f in RESULT_FIELDS:
                assert np.array_equal(one[f], b[f]), f
                assert np.array_equal(dense[f], b[f]), f
            assert one["totalUpdates"] == b["totalUpdates"] == dense["totalUpdates"] and one["meanChiSq"] == b["meanChiSq"] == dense["meanChiSq"]
