"""Residuals of a result on the MI355X: the shape grid, the uncertainty case and every sparse form of tests/test_residuals.py through the
product library against the numpy restatement of tests/residual_cases.py, bit for bit; the device's bytes against the emulator's; a
torch tensor on the GPU as data; the DeviceMatrix a sparse run was made from; a case whose partial array many workgroups share; the
memory a sparse call holds."""
import numpy as np
import pytest
import scipy.sparse as sp

import residual_cases as rc
from test_residuals import EDGES, PEAK_BYTES, check_memory, peak_bytes, result_of
from cogaps_amd import CoGAPS, _capi

pytestmark = pytest.mark.gpu


def dense_case(G, N, K, unc=False):
    A, P = rc.factors(G, N, K)
    D = rc.dense_data(A, P)
    return A, P, D, (rc.uncertainty_for(D) if unc else None)


def run_dense(lib, G, N, K, unc=False):
    A, P, D, S = dense_case(G, N, K, unc)
    rows = np.arange(G)
    rc.check(_capi.residuals(A, P, data=D, unc=S, rows=rows, lib=lib), rc.restate(A, P, D, S), rows=rows, what="%d x %d x %d" % (G, N, K))


@pytest.mark.parametrize("N", EDGES)
@pytest.mark.parametrize("G", EDGES)
def test_blocks_and_steps(hip_lib, G, N):
    run_dense(hip_lib, G, N, 3)


@pytest.mark.parametrize("N", [255, 256, 257])
@pytest.mark.parametrize("G", [255, 256, 257])
def test_below_at_and_above_the_fold_kernel_s_width(hip_lib, G, N):
    run_dense(hip_lib, G, N, 3)


def test_more_blocks_than_the_grid_has_workgroups(hip_lib):
    """a whole MI355X runs 2048 workgroups: 2052 blocks of genes make some of them take a second block (a partitioned device: more)"""
    G = 2048 * 64 + 200
    A, P, D, _ = dense_case(G, 3, 2)
    rows = [G - 1, 0, 2048 * 64, 64]
    want = rc.restate(A, P, D)
    for data in (D, sp.csr_matrix(D)):
        rc.check(_capi.residuals(A, P, data=data, rows=rows, lib=hip_lib), want, rows=rows, what=type(data).__name__)
    rc.check(_capi.residuals(A, P, rows=rows, lib=hip_lib), rc.restate(A, P), rows=rows)


@pytest.mark.parametrize("K", [1, 31, 32, 33, 50, 70])
def test_patterns_below_at_and_above_the_staged_chunk(hip_lib, K):
    run_dense(hip_lib, 65, 65, K)


@pytest.mark.parametrize("G", [15, 16, 17])
def test_genes_below_at_and_above_a_wave_s_share(hip_lib, G):
    run_dense(hip_lib, G, 70, 3)


@pytest.mark.parametrize("G,N,K", [(65, 129, 3), (129, 63, 50)])
def test_with_an_uncertainty_matrix(hip_lib, G, N, K):
    run_dense(hip_lib, G, N, K, unc=True)


def test_reconstruction_transposed_and_column_major(hip_lib):
    A, P, D, S = dense_case(70, 130, 5, unc=True)
    rows = [69, 0, 64, 64]
    rc.check(_capi.residuals(A, P, rows=rows, lib=hip_lib), rc.restate(A, P), rows=rows)
    want = rc.restate(A, P, D, S)
    rc.check(_capi.residuals(A, P, data=np.ascontiguousarray(D.T), unc=np.ascontiguousarray(S.T), rows=rows, transposeData=True, lib=hip_lib), want, rows=rows)
    rc.check(_capi.residuals(np.asfortranarray(A), np.asfortranarray(P), data=np.asfortranarray(D), unc=np.asfortranarray(S), rows=rows, lib=hip_lib), want, rows=rows)


@pytest.mark.parametrize("form", ["csr", "csc", "coo", "mtx", "device-csr", "device-coo", "csr-transposed"])
def test_sparse_forms_equal_the_dense_call(hip_lib, form, tmp_path):
    D = rc.sparse_matrix()
    A, P = rc.factors(D.shape[0], D.shape[1], 3)
    rows, kw = [9, 5, 0, 69, 9], {}
    dense = _capi.residuals(A, P, data=D, rows=rows, lib=hip_lib)
    rc.check(dense, rc.restate(A, P, D), rows=rows, what="dense")
    r, c, v = rc.triplets_of(D)
    if form == "csr":
        data = sp.csr_matrix(D)
    elif form == "csc":
        data = sp.csc_matrix(D)
    elif form == "coo":
        data = _capi.CooMatrix(D.shape, r, c, v)
    elif form == "mtx":
        path = str(tmp_path / "d.mtx")
        rc.write_mtx(path, r, c, v, D.shape)
        data = _capi.read_mtx_triplets(path, lib=hip_lib)
    elif form == "device-csr":
        data = _capi.DeviceMatrix(sp.csr_matrix(D), lib=hip_lib)
    elif form == "device-coo":
        data = _capi.DeviceMatrix(_capi.CooMatrix(D.shape, r, c, v), lib=hip_lib)
    else:
        data, kw = sp.csr_matrix(np.ascontiguousarray(D.T)), {"transposeData": True}
    got = _capi.residuals(A, P, data=data, rows=rows, lib=hip_lib, **kw)
    for key in ("matrix", "geneChiSq", "sampleChiSq", "chiSq"):
        rc.same_bits(got[key], dense[key], form + " " + key)


@pytest.mark.parametrize("case", ["dense", "uncertainty", "sparse", "reconstruction"])
def test_the_device_gives_the_emulator_s_bytes(hip_lib, emul_lib, case):
    A, P, D, S = dense_case(129, 129, 50, unc=True)
    rows = np.arange(129)
    kw = {"dense": dict(data=D), "uncertainty": dict(data=D, unc=S), "sparse": dict(data=sp.csr_matrix(rc.sparse_matrix(129, 129))), "reconstruction": {}}[case]
    dev, emu = _capi.residuals(A, P, rows=rows, lib=hip_lib, **kw), _capi.residuals(A, P, rows=rows, lib=emul_lib(256), **kw)
    for key in ("matrix", "geneChiSq", "sampleChiSq", "chiSq"):
        if emu[key] is None:
            assert dev[key] is None
        else:
            rc.same_bits(dev[key], emu[key], case + " " + key)


def test_a_tensor_on_the_gpu_gives_the_numpy_input_s_bytes(hip_lib):
    import torch
    A, P, D, S = dense_case(130, 70, 7, unc=True)
    rows = [0, 129, 5]
    for unc in (None, S):
        host = _capi.residuals(A, P, data=D, unc=unc, rows=rows, lib=hip_lib)
        rc.check(host, rc.restate(A, P, D, unc), rows=rows)
        dev = _capi.residuals(A, P, data=torch.from_numpy(D).cuda(), unc=None if unc is None else torch.from_numpy(unc).cuda(), rows=rows, lib=hip_lib)
        for key in ("matrix", "geneChiSq", "sampleChiSq", "chiSq"):
            rc.same_bits(dev[key], host[key], key)
    res = result_of(A, P)
    out = res.residuals(torch.from_numpy(D).cuda().double(), genes=[1, 130])      # converted on the device
    rc.same_bits(out["residuals"], rc.restate(A, P, D)[1][[0, 129]])


def test_the_device_matrix_of_a_sparse_run(hip_lib):
    D = rc.sparse_matrix(70, 130) + np.float32(0)
    D[5, 3] = 1.5; D[2, 7] = 0.5                     # (a run needs no empty gene or sample to be a run; the matrix keeps its other features)
    with _capi.DeviceMatrix(sp.csr_matrix(D), lib=hip_lib) as dm:
        res = CoGAPS(dm, nPatterns=3, nIterations=20, seed=11, sparseOptimization=True, messages=False)
        got = res.residuals(dm, genes=[10, 1])
    dense = res.residuals(D, genes=[10, 1])
    for key in ("residuals", "geneChiSq", "sampleChiSq", "chiSq"):
        rc.same_bits(got[key], dense[key], key)
    rc.same_bits(dense["geneChiSq"], rc.restate(res.featureLoadings, res.sampleFactors, D)[2])


def test_many_workgroups_share_the_partial_array(hip_lib):
    run_dense(hip_lib, 1000, 700, 7)


def test_a_sparse_call_holds_less_than_a_quarter_of_a_densification(hip_lib):
    out, dense = check_memory(hip_lib)
    for key in ("geneChiSq", "sampleChiSq", "chiSq"):
        rc.same_bits(out[key], dense[key], key)


def test_the_allocations_of_a_call_are_pinned(hip_lib):
    assert peak_bytes(hip_lib) == PEAK_BYTES
