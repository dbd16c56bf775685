"""The projection of new data onto a result's patterns (cogaps_project; csrc/project_kernel.h) on the emulator: every
output of the C entry against the numpy restatement of tests/projection_cases.py, bit for bit, over the edges of the trips, of the
pattern chunk, of the blocks of samples and of the grid; every input form with identical bits; an anchor whose sums are all exact; an
independent least-squares solver; the front end's matching of genes and patterns; the refusals, each by its message."""
import ctypes as C

import numpy as np
import pytest

import projection_cases as pc
from cogaps_amd import CogapsResult, _capi, projectR

T = pc.TRIP


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


def _check(lib, L, D, want=None, what="", **kw):
    got = _capi.project(L, D, lib=lib, **kw)
    pc.check(got, want if want is not None else pc.restate(L, D), what)
    return got


# ---- 1. the C entry against the restatement, bit for bit, every output ----
@pytest.mark.parametrize("n,K,S", pc.GRID)
def test_bit_for_bit(lib, n, K, S):
    _check(lib, pc.loadings(n, K), pc.data(n, S), what="n %d K %d S %d" % (n, K, S))


def test_the_grid_covers_every_edge():
    assert pc.CHUNK == 32                                   # (another chunk would want one pattern count either side of it)
    assert {n for n, K, S in pc.GRID if n > K + 1} == {T - 1, T, T + 1, 2 * T + 1} and any(n == K + 1 for n, K, S in pc.GRID)
    assert {K for n, K, S in pc.GRID} == {1, 2, 31, 32, 33, 64, 65, 128} and {S for n, K, S in pc.GRID} == {1, 63, 64, 65, 130}
    for axis, values in ((0, (T - 1, T, T + 1, 2 * T + 1)), (1, (1, 2, 31, 32, 33, 64, 65, 128)), (2, (1, 63, 64, 65, 130))):
        for v in values:
            assert sum(1 for case in pc.GRID if case[axis] == v) >= 2


@pytest.mark.parametrize("n,S", [(8 * T, 3), (7 * T + 1, 3), (8 * T + 1, 3), (2 * T + 1, 2 * 256 + 1), (2 * T, 4 * 256), (2 * T + 1, 2 * 256)])
def test_a_workgroup_takes_a_second_unit(lib, monkeypatch, n, S):
    """a device of one compute unit: eight workgroups, and a unit is a (trip, block of 256 samples) -- nine trips, or three trips of
    three blocks, are the fewest that give a workgroup a second unit; eight trips, or two trips of four blocks, are one fewer"""
    monkeypatch.setenv("COGAPS_TEST_COMPUTE_UNITS", "1")
    _check(lib, pc.loadings(n, 2), pc.data(n, S), what="n %d S %d" % (n, S))


def test_an_output_may_be_left_out(lib):
    n, K, S = 70, 3, 5
    L, D = np.ascontiguousarray(pc.loadings(n, K)), np.ascontiguousarray(pc.data(n, S))
    want = pc.restate(L, D)
    desc, keep, _ = _capi._residual_data(D, None, False, -1)
    coef = np.zeros((K, S))
    dp = C.POINTER(C.c_double)
    assert lib.cogaps_project(L.ctypes.data_as(C.POINTER(C.c_float)), n, K, 1, K, C.byref(desc), None, -1, coef.ctypes.data_as(dp), None, None, None, None, None) == 0
    assert np.array_equal(coef.view(np.uint64), want["coef"].view(np.uint64))


# ---- 2. every input form, identical bits ----
def test_input_forms(lib):
    import scipy.sparse as sp
    L, pool, rows = pc.forms_case()
    want = pc.restate(L, pool, rows)
    seen = []
    for name, data, kw in pc.forms(pool, rows):
        _check(lib, L, data, want, name, **kw)
        seen.append(name)
    assert len(seen) == 11
    LF = np.asfortranarray(L)
    _check(lib, LF, pool, want, "column-major loadings", rows=rows)
    wide = np.zeros((2 * L.shape[0], 2 * L.shape[1] + 1), dtype=np.float32)
    wide[::2, 1::2] = L
    _check(lib, wide[::2, 1::2], pool, want, "a slice of the loadings", rows=rows)
    with _capi.DeviceMatrix(sp.csr_matrix(pool), lib=lib) as handle:
        _check(lib, L, handle, want, "a device matrix", rows=rows)


def test_a_sparse_form_allocates_nothing_of_the_datas_size(lib):
    import scipy.sparse as sp
    n, K, S = 2 * T + 1, 3, 700
    L, D = pc.loadings(n, K), pc.data(n, S, zeros=0.97)
    dense = _capi.project(L, D, lib=lib)
    sparse = _capi.project(L, sp.csr_matrix(D), lib=lib)
    pc.check(sparse, dense)
    assert dense["peakDeviceBytes"] > 4 * n * S > sparse["peakDeviceBytes"] > 0


# ---- 3. the exact anchor, through the front end ----
def test_exact_anchor(lib):
    L, D, want = pc.anchor()
    res = CogapsResult({"Amean": L, "Asd": np.ones_like(L), "Pmean": np.ones((2, 3), dtype=np.float32), "Psd": np.ones((2, 3), dtype=np.float32)})
    out = res.projectR(D, full=True, lib=lib)
    pc.check_anchor(out, want)
    small = res.projectR(D, lib=lib)
    assert sorted(small) == ["projection", "pval"]
    import scipy.sparse as sp
    pc.check_anchor(projectR(sp.csr_matrix(D), res, full=True, lib=lib), want)


# ---- 4. an independent solver ----
def test_against_lstsq(lib, capsys):
    L, D, ref = pc.lstsq_case()
    assert (L.shape[0], D.shape[1], L.shape[1]) == pc.LSTSQ_SHAPE
    with capsys.disabled():
        print("\ncond(L) = %.4g" % np.linalg.cond(L.astype(np.float64)))
        diff = pc.relative_difference(_capi.project(L, D, lib=lib)["coef"], ref)
        print("largest |library - lstsq| / max |lstsq| = %.3g (the restatement: %.3g)" % (diff, pc.LSTSQ_RESTATEMENT_DIFFERENCE))
    assert diff <= 16 * pc.LSTSQ_RESTATEMENT_DIFFERENCE


# ---- 5. the front end ----
def _named_case():
    n, K, S = 60, 4, 9
    L, D = pc.loadings(n, K, seed=21), pc.data(n, S, seed=22)
    genes = ["g%d" % i for i in range(n)]
    res = CogapsResult({"Amean": L, "Asd": np.ones_like(L), "Pmean": np.ones((S, K), dtype=np.float32), "Psd": np.ones((S, K), dtype=np.float32)}, geneNames=genes)
    return res, L, D, genes


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def test_position_form_and_full(lib):
    from scipy.special import erfc
    res, L, D, genes = _named_case()
    want = pc.restate(L, D)
    out = res.projectR(D, full=True, lib=lib)
    assert sorted(out) == sorted(["projection", "pval", "t", "sigma", "stdevUnscaled", "df", "rss", "gram", "genesMatched", "patterns"])
    assert _same(out["projection"], want["coef"]) and _same(out["rss"], want["rss"]) and _same(out["gram"], want["gram"]) and _same(out["stdevUnscaled"], want["stdevUnscaled"])
    assert out["df"] == 56 and out["genesMatched"] == genes and out["patterns"] == ["Pattern_1", "Pattern_2", "Pattern_3", "Pattern_4"]
    sigma = np.sqrt(want["rss"] / 56)
    t = want["coef"] / want["stdevUnscaled"][:, None] / sigma[None, :]
    assert _same(out["sigma"], sigma) and _same(out["t"], t) and _same(out["pval"], erfc(np.abs(t) / np.sqrt(2.0)))
    assert out["projection"].dtype == np.float64 and out["pval"].dtype == np.float64 and ((out["pval"] >= 0) & (out["pval"] <= 1)).all()
    with pytest.raises(ValueError, match="the data has 59 genes, the loadings have 60"):
        res.projectR(D[:59], lib=lib)
    assert _same(res.projectR(np.ascontiguousarray(D.T), transposeData=True, lib=lib)["projection"], want["coef"])
    assert _same(projectR(D, L, lib=lib)["projection"], want["coef"])                      # a plain matrix


def test_genes_matched_by_name(lib):
    res, L, D, genes = _named_case()
    order = np.random.Generator(np.random.MT19937(3)).permutation(60)
    # the data: the result's genes shuffled, without g7 and g30, with two genes the result does not know, and g5 a second time
    rows = [int(i) for i in order if i not in (7, 30)]
    data = np.concatenate([D[rows[:20]], pc.data(2, 9, seed=23), D[rows[20:]], D[11:12]])
    names = [genes[i] for i in rows[:20]] + ["x1", "x2"] + [genes[i] for i in rows[20:]] + ["g5"]
    assert not np.array_equal(D[11], D[5])
    keep = [i for i in range(60) if i not in (7, 30)]
    want = pc.restate(L[keep], D[keep])
    out = res.projectR(data, dataNames=names, full=True, lib=lib)
    assert out["genesMatched"] == [genes[i] for i in keep] and out["df"] == 58 - 4
    assert _same(out["projection"], want["coef"]) and _same(out["rss"], want["rss"])
    same = projectR(data, L, dataNames=names, loadingsNames=genes, full=True, lib=lib)
    assert _same(same["projection"], want["coef"]) and _same(same["pval"], out["pval"])
    with pytest.raises(ValueError, match="4 genes matched by name, 4 patterns need at least 5"):
        res.projectR(D[:4], dataNames=genes[:4], lib=lib)
    with pytest.raises(ValueError, match="the loadings carry no gene names"):
        projectR(data, L, dataNames=names, lib=lib)
    with pytest.raises(ValueError, match="one name per gene"):
        res.projectR(data, dataNames=names[:-1], lib=lib)


def test_patterns_selected_by_NP(lib):
    res, L, D, genes = _named_case()
    want = pc.restate(L[:, [2, 0]], D)
    by_index = res.projectR(D, NP=[3, 1], full=True, lib=lib)
    by_name = res.projectR(D, NP=["Pattern_3", "Pattern_1"], full=True, lib=lib)
    for out in (by_index, by_name):
        assert out["patterns"] == ["Pattern_3", "Pattern_1"] and out["df"] == 58 and _same(out["projection"], want["coef"]) and _same(out["gram"], want["gram"])
    assert _same(res.projectR(D, NP=2, lib=lib)["projection"], pc.restate(L[:, [1]], D)["coef"])
    for bad, message in (([0], "outside 1 .. 4"), ([5], "outside 1 .. 4"), (["Pattern_9"], "unknown pattern name"), ([1, "Pattern_2"], "all indices or all names"), ([], "NP is empty")):
        with pytest.raises(ValueError, match=message):
            res.projectR(D, NP=bad, lib=lib)


def test_input_checks_are_those_of_residuals(lib):
    res, L, D, genes = _named_case()
    bad = D.copy()
    bad[3, 3] = -1.0
    with pytest.raises(ValueError):
        res.projectR(bad, lib=lib)
    bad[3, 3] = np.nan
    with pytest.raises(ValueError):
        res.projectR(bad, lib=lib)


# ---- 6. the refusals of the C entry, each by its message ----
def _call(lib, L, desc, n=None, K=None, rows=None, coef=True):
    L = np.ascontiguousarray(L, dtype=np.float32)
    n, K = L.shape[0] if n is None else n, L.shape[1] if K is None else K
    out = np.zeros((max(K, 1), 64))
    idx = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)
    rc = lib.cogaps_project(L.ctypes.data_as(C.POINTER(C.c_float)), n, L.shape[1], 1, K, None if desc is None else C.byref(desc),
                            None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)), -1,
                            out.ctypes.data_as(C.POINTER(C.c_double)) if coef else None, None, None, None, None, None)
    return rc, lib.cogaps_last_error().decode()


def test_refusals(lib):
    L, D = np.ascontiguousarray(pc.loadings(40, 3)), np.ascontiguousarray(pc.data(40, 6))
    desc, keep, _ = _capi._residual_data(D, None, False, -1)

    def refused(message, *a, **kw):
        rc, text = _call(lib, *a, **kw)
        assert rc != 0 and text.startswith("cogaps_project: ") and message in text, text

    assert _call(lib, L, desc)[0] == 0
    refused("null argument", L, desc, coef=False)
    refused("there is no data", L, None)
    none = _capi.CogapsResidualDataC()
    refused("there is no data", L, none)
    # what cogaps_residuals refuses of a descriptor
    odd, _, _ = _capi._residual_data(D, None, False, -1)
    odd.kind = 9
    refused("unknown kind of data 9", L, odd)
    odd.kind, odd.dense = _capi.RESIDUAL_DATA_DENSE, None
    refused("null argument: dense", L, odd)
    odd.kind = _capi.RESIDUAL_DATA_SPARSE
    refused("null argument: the matrix", L, odd)
    odd.kind = _capi.RESIDUAL_DATA_DEVICE_MATRIX
    refused("null argument: deviceMatrix", L, odd)
    unc, keep2, _ = _capi._residual_data(D, np.ones_like(D), False, -1)
    refused("the fit is unweighted", L, unc)
    refused("nPatterns must be at least 1", L, desc, K=0)
    refused("3 genes are not more than nPatterns = 3", L, desc, n=3, rows=[0, 1, 2])
    refused("2 genes are not more than nPatterns = 3", L, desc, n=2, rows=[0, 1])
    refused("the data has 40 genes, the loadings have 39 rows", L, desc, n=39)
    refused("gene 1 asks for row 40, the data has 40", L, desc, rows=[0, 40] + list(range(38)))
    wide = np.ascontiguousarray(pc.loadings(200, 129))
    big, keep3, _ = _capi._residual_data(np.ascontiguousarray(pc.data(200, 6)), None, False, -1)
    refused("129 patterns are more than PJ_MAX_PATTERNS = 128", wide, big)
    nan = L.copy()
    nan[7, 1] = np.inf
    refused("the loadings hold a NaN or an infinite value", nan, desc)
    zero = L.copy()
    zero[:, 1] = 0.0
    refused("loadings are rank deficient", zero, desc)
    twin = L.copy()
    twin[:, 2] = twin[:, 0]
    refused("loadings are rank deficient", twin, desc)


def test_refusals_reach_python_as_errors(lib):
    import scipy.sparse as sp
    L, D = pc.loadings(40, 3), pc.data(40, 6)
    twin = L.copy()
    twin[:, 2] = twin[:, 0]
    with pytest.raises(_capi.CogapsError, match="loadings are rank deficient"):
        _capi.project(twin, D, lib=lib)
    with pytest.raises(_capi.CogapsError, match="more than PJ_MAX_PATTERNS = 128"):
        _capi.project(pc.loadings(200, 129), pc.data(200, 6), lib=lib)
    with pytest.raises(ValueError, match="one data row per gene"):
        _capi.project(L, D, rows=[1, 2], lib=lib)
    with pytest.raises(_capi.CogapsError, match="the data has 6 genes"):
        _capi.project(L, sp.csr_matrix(D), transposeData=True, lib=lib)
    assert _capi.project(L, D, lib=lib)["coef"].shape == (3, 6)                  # (the library is as it was after a refusal)

