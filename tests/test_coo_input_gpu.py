"""Triplet (COO) and Matrix Market input of the sparse model on the MI355X (product library): the triplet passes of csrc/sparse_build.h
-- validation, present flags, winner indices, kept entries, scatter -- against the dense-input session, the CSR-input session and the
oracle."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import parity_util as pu
from parity_util import assert_structures_equal, structures
from test_coo_input import RESULT_FIELDS, coo_of, densify, run_stepwise_coo
from test_sparse_input import SHAPES

pytestmark = pytest.mark.gpu
GIST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "GIST.mtx")


def test_structures_and_memory(hip_lib):
    from cogaps_amd import _capi
    genes, samples = 3000, 2500
    data = sp.random(genes, samples, density=0.02, format="csr", dtype=np.float32, random_state=np.random.default_rng(3))
    data.data[:] = np.ceil(data.data * 9)
    dense = data.toarray()
    m = coo_of(dense, 4, repeats=0.01)
    assert m.nnz >= data.nnz + genes * samples // 100
    chk = np.zeros_like(dense)
    chk[m.rows, m.cols] = m.values          # (numpy keeps the last of repeated indices: the loop of the definition, vectorised)
    assert np.array_equal(chk, dense)
    kw = dict(lib=hip_lib, nPatterns=3, seed=1, sparseOptimization=True)
    T, S, D = _capi.Session(m, **kw), _capi.Session(data, **kw), _capi.Session(dense, **kw)
    t_bytes, s_bytes, d_bytes = T.device_bytes(), S.device_bytes(), D.device_bytes()
    print("device bytes: dense input %d, CSR input %d, triplet input %d, one dense array %d" % (d_bytes, s_bytes, t_bytes, genes * samples * 4))
    d = structures(D)
    assert_structures_equal(d, structures(T))
    ref = pu.packed_reference(dense, 3)
    for name, sess in (("dense", D), ("CSR", S), ("triplet", T)):
        assert_structures_equal(ref, structures(sess), name + " input")
    assert d["A"]["vals"].size > 10000
    assert d_bytes == s_bytes == t_bytes and t_bytes > 0
    assert d_bytes < genes * samples * 4
    T.close(), S.close(), D.close()


def test_contention(hip_lib):
    """200 000 triplets on 50 positions of a 130 x 70 matrix, values alternating positive and zero: thousands of entries meet at one
    present bit and one winner word"""
    from cogaps_amd import _capi
    rng = np.random.default_rng(8)
    pos = rng.choice(130 * 70, 50, replace=False)
    pick = rng.integers(0, 50, 200000)
    r, c = np.unravel_index(pos[pick], (130, 70))
    v = np.where(np.arange(200000) % 2 == 0, 1.0 + (np.arange(200000) % 7), 0.0).astype(np.float32)
    dense = densify((130, 70), r, c, v)
    assert 5 < int((dense > 0).sum()) < 45
    kw = dict(lib=hip_lib, nPatterns=3, seed=1, sparseOptimization=True)
    T, D = _capi.Session(_capi.CooMatrix((130, 70), r, c, v), **kw), _capi.Session(dense, **kw)
    assert_structures_equal(structures(D), structures(T))
    ref = pu.packed_reference(dense, 3)
    assert_structures_equal(ref, structures(D), "dense input")
    assert_structures_equal(ref, structures(T), "triplet input")
    T.close(), D.close()


def test_device_resident_triplets_equal_host_triplets(hip_lib):
    import torch
    from cogaps_amd import _capi
    data = pu.synthetic_counts(700, 260, zeros=0.85, seed=31)
    m = coo_of(data, 2, repeats=0.02)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = [torch.from_numpy(a.view(v)).to(dev) for a, v in ((m.rows, np.int32), (m.cols, np.int32), (m.values, np.float32))]
    torch.cuda.synchronize()
    md = _capi.CooMatrix(m.shape, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), on_device=True, nnz=m.nnz)
    kw = dict(lib=hip_lib, nPatterns=5, nIterations=30, seed=3, sparseOptimization=True)
    H, D = _capi.Session(m, **kw), _capi.Session(md, **kw)
    assert_structures_equal(structures(H), structures(D))
    assert H.device_bytes() == D.device_bytes()
    for phase in (1, 2):
        assert H.run_iterations(phase, 0, 30) == D.run_iterations(phase, 0, 30)
    rh, rd = H.finish(), D.finish()
    for f in RESULT_FIELDS:
        assert np.array_equal(rh[f], rd[f]), f
    assert rh["meanChiSq"] == rd["meanChiSq"]
    H.close(), D.close()
    del t


def test_full_run_equals_the_csr_run_and_the_oracle(hip_lib, oracle):
    from cogaps_amd import _capi
    data = pu.synthetic_counts(700, 260, zeros=0.85, seed=21)
    kw = dict(nPatterns=5, nIterations=30, seed=42, outputFrequency=10, sparseOptimization=True)
    w_a, w_p = hip_lib.cogaps_reduction_width(260), hip_lib.cogaps_reduction_width(700)
    r = _capi.run(coo_of(data, 6, repeats=0.02), lib=hip_lib, **kw)
    s = _capi.run(sp.csr_matrix(data), lib=hip_lib, **kw)
    o = oracle.run(data, math_mode=oracle.MATH_PORTABLE, redW_A=w_a, redW_P=w_p, redG=4, **kw)
    for f in RESULT_FIELDS:
        assert np.array_equal(r[f], s[f]), f
        assert np.array_equal(r[f], o[f]), f
    assert r["totalUpdates"] == s["totalUpdates"] == o["totalUpdates"] and r["meanChiSq"] == s["meanChiSq"] == o["meanChiSq"]


@pytest.mark.parametrize("genes,samples,k,iters,zeros,win", [SHAPES[2], SHAPES[3]])
def test_coo_input_stepwise_gpu(hip_lib, oracle, genes, samples, k, iters, zeros, win):
    """(141 flag words per vector on one side, then on the other; the product library has one generator window: `win` is not used)"""
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=genes + samples)
    m = coo_of(data, 3, repeats=0.05)
    run_stepwise_coo(hip_lib, oracle, m, data, iters, trace=genes * samples < 50000, nPatterns=k, seed=11, total_iter=max(iters, 40), sparseOptimization=True)


def test_run_from_file_equals_the_run_on_the_dense_read(hip_lib):
    from cogaps_amd import _capi
    kw = dict(nPatterns=3, nIterations=30, seed=7, outputFrequency=10, sparseOptimization=True)
    want = _capi.run(_capi.read_matrix_file(GIST, lib=hip_lib), lib=hip_lib, **kw)
    got = _capi.run_from_file(GIST, lib=hip_lib, **kw)
    for f in RESULT_FIELDS:
        assert np.array_equal(got[f], want[f]), f
    assert got["meanChiSq"] == want["meanChiSq"] and got["totalUpdates"] == want["totalUpdates"]
