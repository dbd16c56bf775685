"""Residuals of a result (cogaps_residuals; csrc/residual_kernel.h) on the emulator: the reconstruction, the residual
rows and the chi-square of every gene, every sample and the whole fit against the numpy restatement of tests/residual_cases.py, bit for
bit -- below, at and above every constant of the kernels (64 genes a block and 64 samples a step, 16 genes a wave, 32 patterns staged
per trip, 256 samples a workgroup and 256 genes a trip of the fold), and with a grid whose workgroups take two blocks each; dense data with and without an uncertainty, transposed and column-major; every sparse form against the dense call on the
densified matrix; a bound that does not share the restatement's order; the memory a sparse call holds; refusals; the front end."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import residual_cases as rc
from cogaps_amd import CogapsResult, _capi, binaryA, reconstructGene, residuals

EDGES = [1, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


def run_dense(lib, G, N, K, unc=False):
    A, P = rc.factors(G, N, K)
    D = rc.dense_data(A, P)
    S = rc.uncertainty_for(D) if unc else None
    rows = np.arange(G)
    rc.check(_capi.residuals(A, P, data=D, unc=S, rows=rows, lib=lib), rc.restate(A, P, D, S), rows=rows, what="%d x %d x %d" % (G, N, K))


# ---- 1. shapes ----
@pytest.mark.parametrize("N", EDGES)
@pytest.mark.parametrize("G", EDGES)
def test_blocks_and_steps(lib, G, N):
    run_dense(lib, G, N, 3)


@pytest.mark.parametrize("K", [1, 31, 32, 33, 50, 64, 65, 70])
def test_patterns_below_at_and_above_the_staged_chunk(lib, K):
    run_dense(lib, 65, 65, K)


@pytest.mark.parametrize("G", [15, 16, 17, 47, 48, 49])
def test_genes_below_at_and_above_a_wave_s_share(lib, G):
    run_dense(lib, G, 70, 3)


@pytest.mark.parametrize("N", [255, 256, 257])
@pytest.mark.parametrize("G", [255, 256, 257])
def test_below_at_and_above_the_fold_kernel_s_width(lib, G, N):
    """rs_fold_kernel: 256 samples a workgroup for sampleChiSq, 256 genes a trip through LDS for chiSq"""
    run_dense(lib, G, N, 3)


@pytest.mark.parametrize("source", ["dense", "sparse", "reconstruction"])
def test_a_grid_smaller_than_the_blocks(lib, monkeypatch, source):
    """one compute unit: eight workgroups for the 16 blocks of 1000 genes, two blocks each -- the bytes of the restatement, which knows
    no grid, and of the full grid"""
    G, N, K = 1000, 130, 3
    A, P = rc.factors(G, N, K)
    D = rc.dense_data(A, P)
    rows = [999, 0, 512, 64, 63, 999]
    kw = {"dense": dict(data=D), "sparse": dict(data=sp.csr_matrix(D)), "reconstruction": {}}[source]
    full = _capi.residuals(A, P, rows=rows, lib=lib, **kw)
    monkeypatch.setenv("COGAPS_TEST_COMPUTE_UNITS", "1")
    assert (G + 63) // 64 == 2 * 8                     # (gs_grid: eight workgroups per compute unit)
    small = _capi.residuals(A, P, rows=rows, lib=lib, **kw)
    rc.check(small, rc.restate(A, P, None if source == "reconstruction" else D), rows=rows, what=source)
    for key in ("matrix", "geneChiSq", "sampleChiSq", "chiSq"):
        if full[key] is not None:
            rc.same_bits(small[key], full[key], source + " " + key)


def test_reconstruction_alone(lib):
    A, P = rc.factors(129, 65, 50)
    rows = np.arange(129)
    out = _capi.residuals(A, P, rows=rows, lib=lib)
    rc.check(out, rc.restate(A, P), rows=rows)
    assert out["geneChiSq"] is None and out["sampleChiSq"] is None and out["chiSq"] is None


# ---- 2. uncertainty, orientation, strides ----
@pytest.mark.parametrize("G,N,K", [(65, 129, 3), (129, 63, 50)])
def test_with_an_uncertainty_matrix(lib, G, N, K):
    run_dense(lib, G, N, K, unc=True)


def test_the_default_uncertainty_is_double_precision_pmax(lib):
    """0.1 * (double)d is not (double)(0.1f * d): the two differ in the last bits of the residual"""
    A, P = rc.factors(65, 65, 3)
    D = rc.dense_data(A, P)
    M, r, *_ = rc.restate(A, P, D)
    fill32 = np.maximum(np.float32(0.1) * D, np.float32(0.1)).astype(np.float64)
    assert (rc.bits((D.astype(np.float64) - M) / fill32) != rc.bits(r)).any()
    rc.same_bits(_capi.residuals(A, P, data=D, rows=np.arange(65), lib=lib)["matrix"], r)


def test_transposed_and_column_major(lib):
    A, P = rc.factors(70, 130, 5)
    D = rc.dense_data(A, P)
    S = rc.uncertainty_for(D)
    rows = np.arange(70)
    want = rc.restate(A, P, D, S)
    rc.check(_capi.residuals(A, P, data=np.ascontiguousarray(D.T), unc=np.ascontiguousarray(S.T), rows=rows, transposeData=True, lib=lib), want, rows=rows, what="transposeData")
    fortran = [np.asfortranarray(x) for x in (A, P, D, S)]
    assert all(x.flags.f_contiguous and not x.flags.c_contiguous for x in fortran)
    rc.check(_capi.residuals(fortran[0], fortran[1], data=fortran[2], unc=fortran[3], rows=rows, lib=lib), want, rows=rows, what="column-major")
    rc.check(_capi.residuals(fortran[0], P, data=fortran[2], unc=S, rows=rows, lib=lib), want, rows=rows, what="mixed orders")
    rc.check(_capi.residuals(A, P, data=D.astype(np.float64), rows=rows, lib=lib), rc.restate(A, P, D), rows=rows, what="float64 data")


# ---- 3. selected rows ----
def test_rows_out_of_order_and_repeated(lib):
    A, P = rc.factors(130, 70, 3)
    D = rc.dense_data(A, P)
    rows = [129, 0, 64, 64, 3, 129, 63]
    rc.check(_capi.residuals(A, P, data=D, rows=rows, lib=lib), rc.restate(A, P, D), rows=rows)
    rc.check(_capi.residuals(A, P, rows=rows, lib=lib), rc.restate(A, P), rows=rows)
    none = _capi.residuals(A, P, data=D, lib=lib)
    assert none["matrix"] is None
    rc.check(none, rc.restate(A, P, D))


# ---- 4. sparse forms ----
@pytest.fixture(scope="module")
def sparse_case():
    D = rc.sparse_matrix()
    G, N = D.shape
    assert N == 130 and not D[5].any() and not D[:, 7].any() and D[0, 0] > 0 and D[G - 1, N - 1] > 0 and (np.delete(D[9], 7) > 0).all()
    A, P = rc.factors(G, N, 3)
    return A, P, D, rc.restate(A, P, D)


def test_the_triplets_denote_the_matrix():
    D = rc.sparse_matrix()
    r, c, v = rc.triplets_of(D)
    assert r.size > np.count_nonzero(D) + 20 and (v <= 0).any()
    T = _capi.CooMatrix(D.shape, r, c, v).toarray()
    assert np.array_equal(np.where(T > 0, T, 0), D) and (T < 0).any()


@pytest.mark.parametrize("form", ["csr", "csc", "coo", "mtx", "device-csr", "device-coo", "csr-transposed"])
def test_sparse_forms_equal_the_dense_call(lib, sparse_case, form, tmp_path):
    A, P, D, want = sparse_case
    rows, kw = [9, 5, 0, 69, 9], {}
    dense = _capi.residuals(A, P, data=D, rows=rows, lib=lib)
    rc.check(dense, want, rows=rows, what="dense")
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
        data = _capi.read_mtx_triplets(path, lib=lib)
        assert data.nnz == v.size
    elif form == "device-csr":
        data = _capi.DeviceMatrix(sp.csr_matrix(D), lib=lib)
    elif form == "device-coo":
        data = _capi.DeviceMatrix(_capi.CooMatrix(D.shape, r, c, v), lib=lib)
    else:
        data, kw = sp.csr_matrix(np.ascontiguousarray(D.T)), {"transposeData": True}
    got = _capi.residuals(A, P, data=data, rows=rows, lib=lib, **kw)
    for key in ("matrix", "geneChiSq", "sampleChiSq", "chiSq"):
        rc.same_bits(got[key], dense[key], form + " " + key)


# ---- 5. a check that does not share the restatement's order ----
def test_against_a_matrix_product_and_plain_sums(lib):
    G, N, K = 130, 200, 50
    A, P = rc.factors(G, N, K)
    D = rc.dense_data(A, P)
    M = _capi.residuals(A, P, rows=np.arange(G), lib=lib)["matrix"]
    A64, P64 = A.astype(np.float64), P.astype(np.float64)
    u = K * 2.0 ** -53
    gamma = u / (1 - u)
    assert (np.abs(M - A64 @ P64.T) <= 2 * gamma * (np.abs(A64) @ np.abs(P64).T)).all()
    out = _capi.residuals(A, P, data=D, lib=lib)
    tol = (G + N) * 2.0 ** -52
    assert abs(out["geneChiSq"].sum() - out["chiSq"]) <= tol * out["chiSq"]
    assert abs(out["sampleChiSq"].sum() - out["chiSq"]) <= tol * out["chiSq"]
    assert out["chiSq"] > 0


# ---- 6. the memory a sparse call holds ----
def memory_case():
    G = N = 4096
    rng = np.random.default_rng(77)
    nnz = int(0.005 * G * N)
    at = rng.choice(G * N, size=nnz, replace=False)
    m = sp.csr_matrix((rng.gamma(2.0, 2.0, size=nnz).astype(np.float32), (at // N, at % N)), shape=(G, N))
    A, P = rc.factors(G, N, 3)
    return A, P, m


def check_memory(lib):
    A, P, m = memory_case()
    out = _capi.residuals(A, P, data=m, lib=lib)
    G, N = m.shape
    assert 0 < out["peakDeviceBytes"] < G * N, out["peakDeviceBytes"]
    dense = _capi.residuals(A, P, data=m.toarray(), lib=lib)
    assert dense["peakDeviceBytes"] > 4 * G * N
    return out, dense


def test_a_sparse_call_holds_less_than_a_quarter_of_a_densification(lib):
    out, dense = check_memory(lib)
    for key in ("geneChiSq", "sampleChiSq", "chiSq"):
        rc.same_bits(out[key], dense[key], key)


# peakDeviceBytes of three calls at 70 genes x 130 samples x 3 patterns, rows = [69, 0, 64, 64]: dense host data with an uncertainty
# matrix, the CSR form of rc.sparse_matrix(), the reconstruction alone.  Taken from the build before the statistics' host code was
# rewritten around one owner of a call's temporaries (the meter counts requested sizes, so they are exact on the emulator and the device)
PEAK_BYTES = {"dense": 89620, "sparse": 29812, "reconstruction": 12140}


def peak_bytes(lib):
    A, P = rc.factors(70, 130, 3)
    D = rc.sparse_matrix()
    kw = {"dense": dict(data=D, unc=rc.uncertainty_for(D)), "sparse": dict(data=sp.csr_matrix(D)), "reconstruction": {}}
    return {case: _capi.residuals(A, P, rows=[69, 0, 64, 64], lib=lib, **kw[case])["peakDeviceBytes"] for case in kw}


def test_the_allocations_of_a_call_are_pinned(lib):
    assert peak_bytes(lib) == PEAK_BYTES


# ---- 7. refusals ----
def test_refusals_of_the_entry(lib, sparse_case):
    A, P, D, _ = sparse_case
    with pytest.raises(_capi.CogapsError, match="the data has 69 genes, featureLoadings has 70 rows"):
        _capi.residuals(A, P, data=D[:69], lib=lib)
    with pytest.raises(_capi.CogapsError, match="the data has 129 samples, sampleFactors has 130 rows"):
        _capi.residuals(A, P, data=sp.csr_matrix(D[:, :129]), lib=lib)
    with pytest.raises(_capi.CogapsError, match="the data has 130 genes, featureLoadings has 70 rows"):
        _capi.residuals(A, P, data=D, transposeData=True, lib=lib)
    with pytest.raises(ValueError, match="featureLoadings has 3 patterns, sampleFactors 2"):
        _capi.residuals(A, P[:, :2], data=D, lib=lib)
    with pytest.raises(ValueError, match="takes no uncertainty matrix"):
        _capi.residuals(A, P, data=sp.csr_matrix(D), unc=np.ones_like(D), lib=lib)
    with pytest.raises(_capi.CogapsError, match="output row 1 asks for gene 70, the result has 70"):
        _capi.residuals(A, P, data=D, rows=[0, 70], lib=lib)
    with pytest.raises(_capi.CogapsError, match="neither data nor rows"):
        _capi.residuals(A, P, lib=lib)
    # the C entry itself refuses an uncertainty beside a sparse kind
    import ctypes as C
    m = _capi.SparseMatrix.from_scipy(sp.csr_matrix(D))
    ms = m.c_struct()
    desc = _capi.CogapsResidualDataC()
    desc.kind, desc.sparse, desc.uncertainty = _capi.RESIDUAL_DATA_SPARSE, C.addressof(ms), np.ones_like(D).ctypes.data
    gene = np.zeros(70)
    rc_ = lib.cogaps_residuals(_capi._fp(A), 70, 3, 1, _capi._fp(P), 130, 3, 1, 3, C.byref(desc), None, 0, -1,
                               gene.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None)
    assert rc_ != 0 and "default uncertainty only" in lib.cogaps_last_error().decode()


def result_of(A, P, names=True):
    raw = {"Amean": A, "Asd": np.full_like(A, 0.5), "Pmean": P, "Psd": np.full_like(P, 0.5)}
    return CogapsResult(raw, geneNames=["g%d" % i for i in range(A.shape[0])] if names else None)


def test_refusals_of_the_front_end(lib, sparse_case):
    A, P, D, _ = sparse_case
    res = result_of(A, P)
    with pytest.raises(ValueError, match="unknown gene name: nobody"):
        res.residuals(D, genes=["g1", "nobody"], lib=lib)
    for bad in ([0], [71], [1, 71]):
        with pytest.raises(ValueError, match="genes holds an index outside 1 .. 70"):
            res.reconstructGene(bad, lib=lib)
    with pytest.raises(ValueError, match="takes no uncertainty matrix"):
        res.residuals(sp.csr_matrix(D), uncertainty=np.ones_like(D), lib=lib)
    na = D.copy(); na[3, 3] = np.nan
    with pytest.raises(ValueError, match="NA values in data"):
        res.residuals(na, lib=lib)
    neg = D.copy(); neg[3, 3] = -1
    with pytest.raises(ValueError, match="negative values in data and/or uncertainty matrix"):
        res.residuals(neg, lib=lib)
    with pytest.raises(ValueError, match="negative values in data and/or uncertainty matrix"):
        res.residuals(sp.csr_matrix(neg), lib=lib)
    with pytest.raises(ValueError, match="negative values in data and/or uncertainty matrix"):
        res.residuals(D, uncertainty=-np.ones_like(D), lib=lib)
    small = np.ones_like(D); small[0, 0] = 1e-6
    with pytest.warns(UserWarning, match="small values in uncertainty matrix detected"):
        res.residuals(D, uncertainty=small, matrix=False, lib=lib)


# ---- 8. the front end ----
def test_front_end_by_name_and_by_index(lib, sparse_case, tmp_path):
    A, P, D, want = sparse_case
    res = result_of(A, P)
    M, r, gene, sample, chi = want
    by_index = res.residuals(D, genes=[10, 1, 10, 70], lib=lib)
    by_name = residuals(res, D, genes=["g9", "g0", "g9", "g69"], lib=lib)
    for out in (by_index, by_name):
        rc.same_bits(out["residuals"], r[[9, 0, 9, 69]])
        rc.same_bits(out["geneChiSq"], gene); rc.same_bits(out["sampleChiSq"], sample); rc.same_bits(out["chiSq"], chi)
        assert out["genes"] == ["g9", "g0", "g9", "g69"]
    assert result_of(A, P, names=False).residuals(D, genes=[10, 1], lib=lib)["genes"] == [10, 1]
    everything = res.residuals(D, lib=lib)
    rc.same_bits(everything["residuals"], r)
    nothing = res.residuals(D, matrix=False, lib=lib)
    assert nothing["residuals"] is None and nothing["genes"] == []
    rc.same_bits(nothing["geneChiSq"], gene)
    # a .mtx path stays sparse, another format is read densely; a device matrix; a scipy matrix
    rows, cols, vals = rc.triplets_of(D)
    mtx = str(tmp_path / "d.mtx")
    rc.write_mtx(mtx, rows, cols, vals, D.shape)
    csv = str(tmp_path / "d.csv")
    with open(csv, "w") as f:
        f.write(",".join("s%d" % j for j in range(D.shape[1])) + "\n")
        for row in D:
            f.write(",".join(repr(float(x)) for x in row) + "\n")
    # (CoGAPS()'s checks see every triplet value, overwritten or not: this file has negative ones)
    with pytest.raises(ValueError, match="negative values"):
        res.residuals(mtx, lib=lib)
    keep = vals >= 0
    rc.write_mtx(mtx, rows[keep], cols[keep], vals[keep], D.shape)
    D2 = _capi.CooMatrix(D.shape, rows[keep], cols[keep], vals[keep]).toarray()
    want2 = rc.restate(A, P, D2)
    for data in (mtx, sp.csc_matrix(D2), _capi.DeviceMatrix(sp.csr_matrix(D2), lib=lib)):
        out = res.residuals(data, genes=[3], lib=lib)
        rc.same_bits(out["residuals"], want2[1][[2]]); rc.same_bits(out["sampleChiSq"], want2[3])
    rc.same_bits(res.residuals(csv, matrix=False, lib=lib)["geneChiSq"], gene)
    rc.same_bits(res.residuals(np.ascontiguousarray(D.T), transposeData=True, matrix=False, lib=lib)["geneChiSq"], gene)
    S = rc.uncertainty_for(D)
    rc.same_bits(res.residuals(D, uncertainty=S, matrix=False, lib=lib)["chiSq"], rc.restate(A, P, D, S)[4])


def test_front_end_takes_a_sparse_matrix_struct_with_and_without_entries(lib, sparse_case):
    A, P, D, want = sparse_case
    res = result_of(A, P)
    rc.same_bits(res.residuals(_capi.SparseMatrix.from_scipy(sp.csr_matrix(D)), matrix=False, lib=lib)["geneChiSq"], want[2])
    empty = np.zeros_like(D)
    out = res.residuals(_capi.SparseMatrix.from_scipy(sp.csr_matrix(empty)), genes=[70], lib=lib)
    rc.check({"matrix": out["residuals"], **out}, rc.restate(A, P, empty), rows=[69])
    neg = D.copy(); neg[3, 3] = -1
    with pytest.raises(ValueError, match="negative values"):
        res.residuals(_capi.SparseMatrix.from_scipy(sp.csr_matrix(neg)), lib=lib)


def test_front_end_on_a_real_run(lib, modsim):
    raw = _capi.run(modsim, lib=lib, nPatterns=3, nIterations=30, seed=42, messages=False)
    res = CogapsResult(raw)
    G = modsim.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (calcZ warns about zero deviations, which a short run has)
        for t in (0.5, 3.0):
            b = binaryA(res, t)
            assert b.shape == res.featureLoadings.shape and set(np.unique(b)) <= {0, 1}
            assert np.array_equal(b, (res.calcZ() > t).astype(b.dtype))
        assert 0 < binaryA(res, 0.5).sum() < b.size
    everything = reconstructGene(res, lib=lib)
    rc.same_bits(everything, res.reconstructGene(range(1, G + 1), lib=lib))
    want = rc.restate(res.featureLoadings, res.sampleFactors, modsim)
    rc.same_bits(everything, want[0])
    out = res.residuals(modsim, lib=lib)
    rc.check({"matrix": out["residuals"], **out}, want, rows=np.arange(G))
    # the fit is a fit: the mean squared residual of a 30-iteration run of this data is of the order of its meanChiSq per element
    assert np.isfinite(out["chiSq"]) and out["chiSq"] > 0
