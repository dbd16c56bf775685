"""MANOVA's sums restated in numpy, the host algebra on top of them, and the cases the emulator and the MI355X tests
share.  restate() is csrc/manova_kernel.h's definition, addition by addition: trips of TRIP rows, a trip's rows added in ascending order
from +0.0 with the product rounded before it is added, the trips' partials added in ascending trip order from +0.0, the means as
sum / n, the centred values rounded once.  Vectorised over the trips and the columns only -- never over what is added."""
import numpy as np

from residual_cases import bits, same_bits      # noqa: F401  (the tests take them from here)

TRIP = 256          # csrc/manova_kernel.h: MV_TRIP, the rows of a trip

# The largest relative difference between this file's route (restate() + pillai_f()) and the lstsq route (lstsq_route()) over
# test_manova.py's own front-end cases -- the planted case's five patterns and the anchor -- measured on the CPU: 2.18e-12 (the test
# prints it again).  It is the lstsq route's own error that sets it: its R squared is 1 - rss / tss, whose absolute error of a few 1e-16
# is 2e-12 of the planted case's smallest statistic, 9.9e-5.  The test asserts 100 x this value.
LSTSQ_MEASURED = 2.2e-12


def _trip_sums(terms):
    """terms [n][...] float64 -> the sum over the rows in the kernel's order"""
    n = terms.shape[0]
    nTrips = (n + TRIP - 1) // TRIP
    padded = np.zeros((nTrips * TRIP,) + terms.shape[1:])
    padded[:n] = terms
    padded = padded.reshape((nTrips, TRIP) + terms.shape[1:])
    part = np.zeros((nTrips,) + terms.shape[1:])
    for r in range(TRIP):                               # (a row past the last adds +0.0, which changes nothing: a partial is never -0.0)
        part = part + padded[:, r]
    total = np.zeros(terms.shape[1:])
    for t in range(nTrips):
        total = total + part[t]
    return total


def restate(X, Y):
    """X [n][K] float32, Y [n][p] float64 -> {"xMean", "yMean", "sxx", "sxy", "syy"}, float64, with the kernel's bits"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    Y64 = np.asarray(Y, dtype=np.float64)
    n = X64.shape[0]
    with np.errstate(all="ignore"):
        xMean, yMean = _trip_sums(X64) / np.float64(n), _trip_sums(Y64) / np.float64(n)
        dx, dy = X64 - xMean[None, :], Y64 - yMean[None, :]
        return {"xMean": xMean, "yMean": yMean, "sxx": _trip_sums(dx * dx), "sxy": _trip_sums(dx[:, :, None] * dy[:, None, :]),
                "syy": _trip_sums(dy[:, :, None] * dy[:, None, :])}


def check(out, want, what=""):
    for key in ("xMean", "yMean", "sxx", "sxy", "syy"):
        same_bits(out[key], want[key], "%s %s" % (what, key))


# ---- the C entry's cases ----
def row_counts(p, trip):
    """the row counts of the bit-for-bit grid: the fewest the entry takes, the edges of a wave and of a trip, a fourth trip that is partial"""
    return sorted({p + 2, 63, 64, 65, trip - 1, trip, trip + 1, 3 * trip + 7})


def x_matrix(n, K, seed=0):
    """float32 patterns like a run's means: non-negative, a few exact zeros; where there is room, column 1 has an offset of 1000 and a
    spread of 1e-3 and column 2 is all zero"""
    rng = np.random.default_rng([seed, n, K])
    X = rng.gamma(1.5, 0.7, size=(n, K)).astype(np.float32)
    X[rng.random((n, K)) < 0.1] = 0
    if K >= 3:
        X[:, 1] = (1000.0 + 1e-3 * rng.random(n)).astype(np.float32)
        X[:, 2] = 0
    return X


def y_matrix(n, p, seed=1):
    """factor codes as float64: column j takes the values 1 .. j + 2"""
    rng = np.random.default_rng([seed, n, p])
    return np.stack([rng.integers(1, j + 3, size=n) for j in range(p)], axis=1).astype(np.float64)


# ---- the front end's cases ----
ANCHOR_X = np.array([0, 1, 2, 3, 4, 6], dtype=np.float32)
ANCHOR_Y = np.array([[1, 1], [1, 2], [2, 2], [2, 1], [3, 1], [3, 2]], dtype=np.float64)


_EPS = 2.0 ** -52


def check_anchor(out):
    """x = (0, 1, 2, 3, 4, 6), y1 = (1, 1, 2, 2, 3, 3), y2 = (1, 2, 2, 1, 1, 2), in rationals: Sxx = 70/3, Sxy = (9, 1), Syy = diag(4, 3/2),
    slopes (27/70, 3/70), intercepts (34/35, 97/70), E = [[37/70, -27/70], [-27/70, 51/35]], Pillai 251/280, F 753/58 on 2 and 3 Df.
    The doubles nearest to 251/280 and 753/58 are what the float64 evaluation is held to, within its rounding: every sum has six
    terms and the algebra a dozen operations, so 64 eps bounds the relative error of Pillai's trace V with room to spare, and F =
    1.5 V / (1 - V) multiplies a relative error of V by 1 / (1 - V) = 280/29.  (Exact equality is out of reach of any float64
    evaluation: x's mean 8/3 is no double; this one gives V one unit in the last place below 251/280, 8.9642857142857135e-01, and
    F = 1.2982758620689644e+01, 3.7 eps below 753/58.)  E's entries are differences of numbers up to 4: 64 eps * 4 absolute."""
    V, F = 251 / 280, 753 / 58
    print("anchor: V %.17e (%.2f eps from 251/280), F %.17e (%.2f eps from 753/58)" % (
        out["stat"][0], (out["stat"][0] - V) / V / _EPS, out["approxF"][0], (out["approxF"][0] - F) / F / _EPS))
    assert abs(out["stat"][0] - V) <= 64 * _EPS * V
    assert abs(out["approxF"][0] - F) <= 64 * _EPS * F * 280 / 29
    assert out["Df"] == (1, 4) and out["numDf"][0] == 2 and out["denDf"][0] == 3 and out["nOmitted"] == 0
    assert out["patterns"] == ["Pattern_1"] and out["levels"] == [[1.0, 2.0, 3.0], [1.0, 2.0]]
    assert np.allclose(out["coefficients"][0], [[34 / 35, 97 / 70], [27 / 70, 3 / 70]], rtol=64 * _EPS, atol=0)
    H = np.array([[81.0, 9.0], [9.0, 1.0]]) * 3 / 70
    assert np.allclose(out["SSCP"]["hypothesis"][0], H, rtol=64 * _EPS, atol=0)
    assert np.allclose(out["SSCP"]["residuals"][0], [[37 / 70, -27 / 70], [-27 / 70, 51 / 35]], rtol=0, atol=64 * _EPS * 4)


def raw_result(P, G=4, seed=3):
    """a raw result dict whose sampleFactors are P"""
    rng = np.random.default_rng([seed, G])
    P = np.asarray(P, dtype=np.float32)
    A = rng.gamma(1.5, 1.0, size=(G, P.shape[1])).astype(np.float32)
    return {"Amean": A, "Asd": np.ones_like(A), "Pmean": P, "Psd": np.ones_like(P), "seed": 42, "meanChiSq": 1.0}


def planted(n=300, K=5, seed=11):
    """-> (P [n][K] float32, annotations [n][2] of str): column 0 a 3-level string factor that pattern 3 follows, column 1 a 2-level one"""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, 3, size=n)
    batch = rng.integers(0, 2, size=n)
    P = rng.gamma(2.0, 0.5, size=(n, K))
    P[:, 3] = 1.0 + 0.8 * group + 0.15 * rng.standard_normal(n)
    ann = np.stack([np.array(["ctrl", "dose", "high"])[group], np.array(["f", "m"])[batch]], axis=1)
    return np.abs(P).astype(np.float32), ann


def codes_of(column):
    """unclass(factor(column)) with numpy's sort order: the 1-based index of each value among the sorted distinct values, float64"""
    levels, inverse = np.unique(np.asarray(column), return_inverse=True)
    return (inverse + 1).astype(np.float64), levels


def pillai_f(s, k, n):
    """pattern k of restate()'s sums over n rows -> (Pillai's trace, approx F), by DESIGN.md 4.14's formulas, the p x p algebra by numpy"""
    p = s["syy"].shape[0]
    H = np.outer(s["sxy"][k], s["sxy"][k]) / s["sxx"][k]
    V = float(np.trace(H @ np.linalg.inv(s["syy"])))
    return V, (n - p - 1) / p * (V / (1.0 - V))


def lstsq_route(x, Y):
    """the independent route: regress x on [1, Y] -> (R squared, the regression's overall F)"""
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n, p = Y.shape
    D = np.concatenate([np.ones((n, 1)), Y], axis=1)
    beta = np.linalg.lstsq(D, x, rcond=None)[0]
    rss, tss = float(((x - D @ beta) ** 2).sum()), float(((x - x.mean()) ** 2).sum())
    r2 = 1.0 - rss / tss
    return r2, (r2 / p) / ((1.0 - r2) / (n - p - 1))
