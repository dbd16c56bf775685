"""The projection of new data onto a result's patterns on the MI355X: the device's outputs against the numpy restatement of
tests/projection_cases.py, bit for bit (the grid of tests/test_projection.py), every input form -- a torch tensor on the GPU and a
DeviceMatrix among them -- the exact anchor, more units than the grid holds workgroups, and a single-cell-sized sparse matrix."""
import numpy as np
import pytest

import projection_cases as pc
from cogaps_amd import CogapsResult, _capi

pytestmark = pytest.mark.gpu

T = pc.TRIP


def _check(lib, L, D, want=None, what="", **kw):
    pc.check(_capi.project(L, D, lib=lib, **kw), want if want is not None else pc.restate(L, D), what)


@pytest.mark.parametrize("n,K,S", pc.GRID)
def test_bit_for_bit(hip_lib, n, K, S):
    _check(hip_lib, pc.loadings(n, K), pc.data(n, S), what="n %d K %d S %d" % (n, K, S))


def test_input_forms(hip_lib):
    import scipy.sparse as sp
    import torch
    L, pool, rows = pc.forms_case()
    want = pc.restate(L, pool, rows)
    for name, data, kw in pc.forms(pool, rows):
        _check(hip_lib, L, data, want, name, **kw)
    _check(hip_lib, L, torch.from_numpy(pool).cuda(), want, "a tensor on the GPU", rows=rows)
    _check(hip_lib, L, torch.from_numpy(np.ascontiguousarray(pool.T)).cuda(), want, "a tensor on the GPU, transposed", rows=rows, transposeData=True)
    with _capi.DeviceMatrix(sp.csr_matrix(pool), lib=hip_lib) as handle:
        _check(hip_lib, L, handle, want, "a device matrix", rows=rows)
    with _capi.DeviceMatrix(sp.csc_matrix(np.ascontiguousarray(pool.T)), lib=hip_lib) as handle:
        _check(hip_lib, L, handle, want, "a device matrix, transposed", rows=rows, transposeData=True)


def test_exact_anchor(hip_lib):
    L, D, want = pc.anchor()
    res = CogapsResult({"Amean": L, "Asd": np.ones_like(L), "Pmean": np.ones((2, 3), dtype=np.float32), "Psd": np.ones((2, 3), dtype=np.float32)})
    pc.check_anchor(res.projectR(D, full=True, lib=hip_lib), want)


def test_a_workgroup_takes_a_second_unit(hip_lib):
    """the grid is eight workgroups per compute unit: on the 256 units of a whole MI355X, 2048 T + 1 genes of one pattern and one
    sample are the fewest that give a workgroup a second unit (a partition of the device has fewer units and gets there sooner)"""
    n = 2048 * T + 1
    _check(hip_lib, pc.loadings(n, 1), pc.data(n, 1), what="n %d" % n)


def test_a_single_cell_sized_sparse_matrix(hip_lib):
    """50 000 genes x 256 samples, 50 patterns, 95 % zeros: CSR (never densified) against the dense matrix, every output"""
    import scipy.sparse as sp
    n, S, K = 50000, 256, 50
    L, D = pc.loadings(n, K), pc.data(n, S, zeros=0.95)
    assert 0.94 < (D == 0).mean() < 0.96
    dense = _capi.project(L, D, lib=hip_lib)
    sparse = _capi.project(L, sp.csr_matrix(D), lib=hip_lib)
    pc.check(sparse, dense, "CSR against dense")
    assert np.isfinite(dense["coef"]).all() and (dense["rss"] > 0).all()
    assert sparse["peakDeviceBytes"] < dense["peakDeviceBytes"]
