"""MANOVA (csrc/manova_kernel.h) on the emulator: the C entry's means and centred sums against the numpy restatement of
tests/manova_cases.py, bit for bit, over the edges of the rows, the trips, the blocks of 64 columns and the grid, through every kind of
stride; the front end against a rational anchor and against an independent regression; factor coding, na.omit and the singular cases;
the refusals; getOriginalParameters and getVersion."""
import ctypes

import numpy as np
import pytest

import manova_cases as mc
from cogaps_amd import CogapsParams, CogapsResult, MANOVA, _capi, getOriginalParameters, getVersion

R = 256                                                     # csrc/manova_kernel.h: MV_TRIP, the rows of a trip
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


def _check(lib, X, Y, want=None, what=""):
    mc.check(_capi.manova_sscp(X, Y, lib=lib), want if want is not None else mc.restate(np.asarray(X), np.asarray(Y)), what)


# ---- 1. the C entry against the restatement, bit for bit, every output ----
@pytest.mark.parametrize("p", [1, 2, 8])
@pytest.mark.parametrize("K", [1, 3, 64, 65, 130, 513])
def test_sums_bit_for_bit(lib, K, p):
    for n in mc.row_counts(p, R):
        _check(lib, mc.x_matrix(n, K), mc.y_matrix(n, p), what="n %d K %d p %d" % (n, K, p))


def test_a_workgroup_takes_a_second_trip(lib, monkeypatch):
    """a device of one compute unit: eight workgroups, so 8 R + 1 rows are the fewest that give one of them a second trip"""
    monkeypatch.setenv("COGAPS_TEST_COMPUTE_UNITS", "1")
    for n in (8 * R, 8 * R + 1):
        _check(lib, mc.x_matrix(n, 3), mc.y_matrix(n, 2), what="n %d" % n)


@pytest.mark.parametrize("n,K,p", [(65, 3, 2), (R + 1, 65, 8), (3 * R + 7, 130, 1)])
def test_strides(lib, n, K, p):
    X, Y = mc.x_matrix(n, K), mc.y_matrix(n, p)
    want = mc.restate(X, Y)
    FX, FY = np.asfortranarray(X), np.asfortranarray(Y)
    assert K == 1 or FX.strides == (4, 4 * n)
    _check(lib, FX, Y, want, "column-major X")
    _check(lib, X, FY, want, "column-major Y")
    _check(lib, FX, FY, want, "both column-major")
    wide = np.zeros((2 * n + 1, 3 * K + 2), dtype=np.float32)
    wide[1::2, 2::3][:n] = X
    view = wide[1::2, 2::3][:n]
    assert not view.flags["C_CONTIGUOUS"] and not view.flags["F_CONTIGUOUS"]
    _check(lib, view, FY, want, "a slice of X")
    back = np.ascontiguousarray(X[::-1, ::-1])[::-1, ::-1]                      # negative strides: the wrapper copies
    _check(lib, back, Y, want, "reversed X")


def test_offset_and_zero_columns(lib):
    """a column of offset 1000 and spread 1e-3 keeps its digits (two passes); an all-zero column has sxx == 0.0 exactly"""
    n = 3 * R + 7
    X, Y = mc.x_matrix(n, 3), mc.y_matrix(n, 2)
    out = _capi.manova_sscp(X, Y, lib=lib)
    mc.check(out, mc.restate(X, Y))
    assert out["sxx"][2] == 0.0 and out["xMean"][2] == 0.0 and not out["sxy"][2].any()
    x = X[:, 1].astype(np.float64)
    exact = float(np.sum((x - x.mean()) ** 2))              # ~ n * 1e-6 / 12: far below what one pass would keep of sums near n * 1e6
    assert 0 < exact < 1e-3 and abs(out["sxx"][1] - exact) <= 1e-9 * exact
    assert abs(out["xMean"][1] - 1000.0) < 1e-3


def test_syy_is_symmetric_and_shared(lib):
    X, Y = mc.x_matrix(300, 5), mc.y_matrix(300, 8)
    out = _capi.manova_sscp(X, Y, lib=lib)
    assert np.array_equal(out["syy"], out["syy"].T)
    one = _capi.manova_sscp(X[:, 3:4], Y, lib=lib)                              # a pattern does not depend on its neighbours
    assert np.array_equal(one["sxx"], out["sxx"][3:4]) and np.array_equal(one["sxy"], out["sxy"][3:4]) and np.array_equal(one["syy"], out["syy"])


# ---- 2. the front end against the anchors ----
def _anchor(lib, **kw):
    return CogapsResult(mc.raw_result(mc.ANCHOR_X[:, None])).MANOVA(mc.ANCHOR_Y, lib=lib, **kw)


def test_rational_anchor(lib, capsys):
    from scipy.stats import f
    out = _anchor(lib)
    mc.check_anchor(out)
    # one incomplete beta function, two evaluations of it: 1e-12 is a hundred times what either promises
    assert abs(out["pvalue"][0] - f.sf(out["approxF"][0], 2, 3)) <= 1e-12 * out["pvalue"][0]
    assert abs(out["pvalue"][0] - 0.0333318907608) < 1e-12
    capsys.readouterr()
    assert _anchor(lib, verbose=True)["stat"][0] == out["stat"][0]
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1 and lines[0].startswith("Pattern_1:") and "Pillai" in lines[0]
    sums = _capi.manova_sscp(mc.ANCHOR_X[:, None], mc.ANCHOR_Y, lib=lib)
    assert np.array_equal(sums["sxy"], [[9.0, 1.0]]) and np.array_equal(sums["syy"], [[4.0, 0.0], [0.0, 1.5]]) and np.array_equal(sums["yMean"], [2.0, 1.5])
    assert abs(sums["sxx"][0] - 70 / 3) <= 8 * EPS * 70 / 3


def test_the_other_statistics_follow_pillai(lib):
    P, ann = mc.planted()
    res = CogapsResult(mc.raw_result(P))
    pillai = res.MANOVA(ann, lib=lib)
    V = pillai["stat"]
    for test, want in (("Wilks", 1.0 - V), ("Hotelling-Lawley", V / (1.0 - V)), ("Roy", V / (1.0 - V))):
        out = res.MANOVA(ann, test=test, lib=lib)
        assert out["test"] == test and np.array_equal(out["stat"], want)
        assert np.array_equal(out["approxF"], pillai["approxF"]) and np.array_equal(out["pvalue"], pillai["pvalue"])
    assert np.array_equal(pillai["approxF"], (300 - 2 - 1) / 2 * (V / (1.0 - V)))


def test_planted_pattern_against_the_regression(lib):
    """Pillai's trace of manova(Y ~ x) is the R squared of x regressed on [1, Y], F the regression's F: numpy.linalg.lstsq knows nothing
    of the kernel's sums.  The tolerance is 100 x the largest relative difference between the restatement and that route on these
    cases, measured on the CPU and recorded in manova_cases.LSTSQ_MEASURED."""
    P, ann = mc.planted()
    res = CogapsResult(mc.raw_result(P), sampleNames=["s%d" % i for i in range(300)])
    out = MANOVA(ann, res, lib=lib)                                             # R's argument order
    Y = np.stack([mc.codes_of(ann[:, j])[0] for j in range(2)], axis=1)
    assert out["levels"] == [["ctrl", "dose", "high"], ["f", "m"]] and out["Df"] == (1, 298)
    sums, worst = mc.restate(P, Y), 0.0
    for k in range(5):
        r2, F = mc.lstsq_route(P[:, k], Y)
        V2, F2 = mc.pillai_f(sums, k, 300)
        worst = max(worst, abs(V2 - r2) / r2, abs(F2 - F) / F)
        assert abs(out["stat"][k] - r2) <= 100 * mc.LSTSQ_MEASURED * r2 and abs(out["approxF"][k] - F) <= 100 * mc.LSTSQ_MEASURED * F
    r2, F = mc.lstsq_route(mc.ANCHOR_X, mc.ANCHOR_Y)
    V2, F2 = mc.pillai_f(mc.restate(mc.ANCHOR_X[:, None], mc.ANCHOR_Y), 0, 6)
    worst = max(worst, abs(V2 - r2) / r2, abs(F2 - F) / F)
    print("restatement against lstsq: the largest relative difference is %.3g" % worst)
    anchor = _anchor(lib)
    assert abs(anchor["stat"][0] - r2) <= 100 * mc.LSTSQ_MEASURED * r2 and abs(anchor["approxF"][0] - F) <= 100 * mc.LSTSQ_MEASURED * F
    assert int(np.argmin(out["pvalue"])) == 3 and out["pvalue"][3] < 1e-50 and (np.delete(out["pvalue"], 3) > 1e-3).all()
    # the coefficients are the least-squares fit of every response on [1, x]
    for k in (0, 3):
        D = np.stack([np.ones(300), P[:, k].astype(np.float64)], axis=1)
        assert np.allclose(out["coefficients"][k], np.linalg.lstsq(D, Y, rcond=None)[0], rtol=1e-10, atol=1e-12)
    # featureLoadings: one row of annotations per gene
    genes = CogapsResult(mc.raw_result(np.ones((4, 5), dtype=np.float32), G=300))
    genes.featureLoadings = P
    assert np.array_equal(genes.MANOVA(ann, whichMatrix="featureLoadings", lib=lib)["stat"], out["stat"])


# ---- 3. factor coding, na.omit, the singular cases ----
def test_factor_codes(lib):
    import pandas as pd
    P, ann = mc.planted()
    res = CogapsResult(mc.raw_result(P))
    want = res.MANOVA(ann, lib=lib)
    rng = np.random.default_rng(5)
    numeric = np.stack([np.array([10.5, -3.0, 7.0])[mc.codes_of(ann[:, 0])[0].astype(int) - 1], rng.random(300), mc.codes_of(ann[:, 1])[0]], axis=1)
    out = res.MANOVA(numeric, columns=(0, 2), lib=lib)                          # -3 < 7 < 10.5: "dose" -> 1, "high" -> 2, "ctrl" -> 3
    assert out["levels"] == [[-3.0, 7.0, 10.5], [1.0, 2.0]]
    Y = np.stack([np.array([3.0, 1.0, 2.0])[mc.codes_of(ann[:, 0])[0].astype(int) - 1], mc.codes_of(ann[:, 1])[0]], axis=1)
    sums = _capi.manova_sscp(P, Y, lib=lib)
    assert np.array_equal(out["SSCP"]["hypothesis"], sums["sxy"][:, :, None] * sums["sxy"][:, None, :] / sums["sxx"][:, None, None])
    frame = pd.DataFrame({"group": ann[:, 0], "noise": rng.random(300), "sex": pd.Categorical(ann[:, 1])})
    for given in (frame.iloc[:, [0, 2]], [list(r) for r in ann], ann.astype(object)):
        got = res.MANOVA(given, lib=lib)
        assert np.array_equal(got["stat"], want["stat"]) and got["levels"] == want["levels"]
    assert np.array_equal(res.MANOVA(frame, columns=(0, 2), lib=lib)["pvalue"], want["pvalue"])
    codes, levels = mc.codes_of(["b", "a", "c", "a"])
    assert np.array_equal(codes, [2, 1, 3, 1]) and list(levels) == ["a", "b", "c"]


def test_rows_with_a_missing_value_are_dropped(lib):
    import pandas as pd
    P, ann = mc.planted()
    holes = ann.astype(object)
    holes[7, 0] = None
    holes[120, 1] = None
    keep = np.ones(300, dtype=bool)
    keep[[7, 120]] = False
    short = CogapsResult(mc.raw_result(P[keep])).MANOVA(ann[keep], lib=lib)
    res = CogapsResult(mc.raw_result(P))
    frame = pd.DataFrame(holes)
    frame.iloc[7, 0] = pd.NA
    for given in (holes, [list(r) for r in holes], frame):
        out = res.MANOVA(given, lib=lib)
        assert out["nOmitted"] == 2 and out["Df"] == (1, 296) and short["nOmitted"] == 0
        for key in ("stat", "approxF", "pvalue", "coefficients"):
            assert np.array_equal(out[key], short[key]), key
    numeric = np.stack([mc.codes_of(ann[:, j])[0] for j in range(2)], axis=1)
    numeric[7, 0] = numeric[120, 1] = np.nan
    assert np.array_equal(res.MANOVA(numeric, lib=lib)["stat"], short["stat"])
    numeric[7, 0] = 1.0                                                          # a hole in a column that is not used does not count
    assert res.MANOVA(numeric, columns=(0,), lib=lib)["nOmitted"] == 0


def test_singular_cases(lib):
    P, ann = mc.planted()
    P = P.copy()
    P[:, 1] = 0
    res = CogapsResult(mc.raw_result(P))
    out = res.MANOVA(ann, lib=lib)                                               # the zero pattern: NaN and no exception
    for key in ("stat", "approxF", "pvalue"):
        assert np.isnan(out[key][1]) and not np.isnan(np.delete(out[key], 1)).any(), key
    assert np.isnan(out["coefficients"][1, 1]).all() and np.isnan(out["SSCP"]["hypothesis"][1]).all()
    constant = ann.copy()
    constant[:, 1] = "m"
    with pytest.raises(ValueError, match="residuals have rank 1 < 2"):
        res.MANOVA(constant, lib=lib)
    with pytest.raises(ValueError, match="residuals have rank 1 < 2"):
        res.MANOVA(ann, columns=(0, 0), lib=lib)                                 # the same column twice
    collinear = np.stack([mc.codes_of(ann[:, 0])[0], mc.codes_of(ann[:, 1])[0], 10.0 - 2.0 * mc.codes_of(ann[:, 0])[0]], axis=1)
    with pytest.raises(ValueError, match="rank 2 < 3"):
        res.MANOVA(collinear, columns=(0, 1, 2), lib=lib)
    perfect = P.copy()
    perfect[:, 2] = 2.0 * mc.codes_of(ann[:, 0])[0] + 1.0
    with pytest.raises(ValueError, match="residuals have rank 1 < 2"):
        CogapsResult(mc.raw_result(perfect)).MANOVA(ann, lib=lib)
    one = res.MANOVA(ann, columns=(1,), lib=lib)                                 # p = 1
    assert one["numDf"][0] == 1 and one["denDf"][0] == 298 and one["SSCP"]["residuals"].shape == (5, 1, 1) and one["coefficients"].shape == (5, 2, 1)
    y = mc.codes_of(ann[:, 1])[0]
    for k in (0, 3):
        r = np.corrcoef(P[:, k].astype(np.float64), y)[0, 1]
        assert abs(one["stat"][k] - r * r) <= 1e-12 * max(r * r, 1e-3)           # p = 1: Pillai's trace is the squared correlation


def test_front_end_refusals(lib):
    P, ann = mc.planted()
    res = CogapsResult(mc.raw_result(P))
    for bad, msg in ((dict(interestedVariables=ann[:-1]), "299 rows"), (dict(test="pillai"), "test must be"), (dict(test="F"), "test must be"),
                     (dict(whichMatrix="A"), "whichMatrix"), (dict(columns=(0, 2)), "column 2 is outside"), (dict(columns=(-1,)), "outside"),
                     (dict(columns=()), "columns must name"), (dict(interestedVariables=ann[:, 0]), "two dimensions")):
        kw = dict(dict(interestedVariables=ann, lib=lib), **bad)
        with pytest.raises(ValueError, match=msg):
            res.MANOVA(**kw)
    few = CogapsResult(mc.raw_result(P[:3]))
    with pytest.raises(ValueError, match="complete rows"):
        few.MANOVA(ann[:3], lib=lib)


# ---- 4. the C entry's refusals ----
def test_c_entry_refusals(lib):
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    n, K, p = 20, 3, 2
    X, Y = np.ascontiguousarray(mc.x_matrix(n, K)), np.ascontiguousarray(mc.y_matrix(n, 8))
    want = mc.restate(X, Y[:, :p])
    outs = {"xMean": np.zeros(K), "yMean": np.zeros(8), "sxx": np.zeros(K), "sxy": np.zeros((K, 8)), "syy": np.zeros((8, 8))}
    good = dict(x=X, n=n, K=K, xs=(K, 1), y=Y, p=p, ys=(8, 1), **outs)

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda v, t: None if v is None else v.ctypes.data_as(t)
        rc = lib.cogaps_manova_sscp(ptr(a["x"], fp), a["n"], a["K"], a["xs"][0], a["xs"][1], ptr(a["y"], dp), a["p"], a["ys"][0], a["ys"][1], -1,
                                    *[ptr(a[k], dp) for k in ("xMean", "yMean", "sxx", "sxy", "syy")])
        return rc, lib.cogaps_last_error().decode()

    def valid():
        assert call()[0] == 0
        mc.same_bits(outs["xMean"], want["xMean"]); mc.same_bits(outs["yMean"][:p], want["yMean"]); mc.same_bits(outs["sxx"], want["sxx"])
        mc.same_bits(outs["sxy"].ravel()[:K * p].reshape(K, p), want["sxy"]); mc.same_bits(outs["syy"].ravel()[:p * p].reshape(p, p), want["syy"])

    valid()
    cases = [
        (dict(x=None), "null argument"), (dict(y=None), "null argument"),
        (dict(xMean=None, yMean=None, sxx=None, sxy=None, syy=None), "one of xMean, yMean, sxx, sxy and syy must be given"),
        (dict(p=0), "0 response columns are outside 1 .. MV_MAX_RESP = 8"), (dict(p=9), "9 response columns are outside 1 .. MV_MAX_RESP = 8"),
        (dict(n=p + 1), "3 rows are fewer than nResp + 2 = 4"), (dict(n=0), "0 rows are fewer"), (dict(K=0), "the predictor matrix has no column"),
        (dict(xs=(0, 1)), "a stride of zero"), (dict(xs=(K, 0)), "a stride of zero"), (dict(ys=(0, 1)), "a stride of zero"), (dict(ys=(8, 0)), "a stride of zero"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and err.startswith("cogaps_manova_sscp: ") and msg in err, (kw, err)
        assert lib.cogaps_last_error_code() == _capi.ERR_GENERIC
        valid()
    for name in outs:                                                            # each output is optional; the others come out the same
        assert call(**{name: None})[0] == 0
    assert call(p=8, n=10)[0] == 0 and call(p=8, n=9)[0] != 0                    # n = p + 2 is the fewest


# ---- 5. the two getters ----
def test_original_parameters_and_version():
    raw = mc.raw_result(mc.planted()[0])
    params = CogapsParams(nPatterns=5, seed=7)
    res = CogapsResult(raw, params=params)
    assert res.getOriginalParameters() is params and getOriginalParameters(res) is params
    assert res.getVersion() is None and getVersion(res) is None
    res.metadata["version"] = "3.21.5"
    assert res.getVersion() == "3.21.5" and getVersion(res) == "3.21.5"
    assert CogapsResult(raw).getOriginalParameters() is None
