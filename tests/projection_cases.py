"""The projection of new data onto a result's patterns (csrc/project_kernel.h): the inputs the emulator and the GPU tests
share, and restate(), the definition addition by addition in plain float64 numpy -- np.add and np.multiply in the written order, no
lstsq, no matrix product.  A trip's sum is taken for all trips at once, position by position: the last trip is padded with genes of
zeros, whose products are +-0.0 and leave a sum that started at +0.0 as it is, bit for bit."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "cogaps_hip.h")) as _f:
    _header = _f.read()
TRIP = int(re.search(r"#define COGAPS_PROJECT_TRIP (\d+)", _header).group(1))                    # the genes of a trip
MAX_PATTERNS = int(re.search(r"#define COGAPS_PROJECT_MAX_PATTERNS (\d+)", _header).group(1))
CHUNK = 32                                                   # csrc/project_kernel.h: PJ_KC, the patterns whose sums a lane holds
PIVOT = 1e-12

# (genes, patterns, samples): every value of each axis with two or three of the others
T = TRIP
GRID = [(2, 1, 1), (3, 2, 63), (MAX_PATTERNS + 1, MAX_PATTERNS, 65), (66, 65, 1), (33, 32, 130), (34, 33, 64),
        (T - 1, 31, 64), (T - 1, 1, 130), (T, 32, 65), (T, 2, 1), (T + 1, 33, 63), (T + 1, 64, 130),
        (2 * T + 1, 65, 64), (2 * T + 1, MAX_PATTERNS, 130), (2 * T + 1, 31, 1), (2 * T + 1, 64, 63)]


def _rng(*key):
    return np.random.Generator(np.random.MT19937(list(key)))


def loadings(n, K, seed=1):
    """non-negative float32 with a third of exact zeros, as a factor matrix has them; full column rank"""
    r = _rng(seed, n, K)
    L = (r.gamma(2.0, 0.5, size=(n, K)) * (r.random((n, K)) >= 0.33)).astype(np.float32)
    for k in range(K):
        L[k::K, k] += np.float32(1.0)                        # every pattern has genes of its own
    return L


def data(n, S, seed=2, zeros=0.6):
    """float32 >= 0 with the given share of exact zeros"""
    r = _rng(seed, n, S)
    return (r.gamma(2.0, 1.5, size=(n, S)) * (r.random((n, S)) >= zeros)).astype(np.float32)


def _trip_sums(term, n):
    """term(i) -> the terms of gene position i of every trip, [nTrips][...]; -> the sums over the trips' genes, then over the trips"""
    acc = None
    for i in range(min(TRIP, n)):
        x = term(i)
        acc = np.add(np.zeros_like(x), x) if acc is None else np.add(acc, x)
    total = np.zeros_like(acc[0])
    for t in range(acc.shape[0]):
        total = np.add(total, acc[t])
    return total


def _padded(X, n):
    nTrips = (n + TRIP - 1) // TRIP
    P = np.zeros((nTrips * TRIP,) + X.shape[1:], dtype=np.float64)
    P[:n] = X
    return P.reshape((nTrips, TRIP) + X.shape[1:])


def factor(gram):
    """gram = U diag(d) U^T column by column -> (U, d), or the index of the refused pivot"""
    K = gram.shape[0]
    U, d = np.eye(K), np.zeros(K)
    for j in range(K):
        w = np.multiply(U[j, :j], d[:j])
        s = np.zeros(K - j)
        for m in range(j):
            s = np.add(s, np.multiply(U[j:, m], w[m]))
        v = np.subtract(gram[j:, j], s)
        if not v[0] > PIVOT * gram[j, j]:
            return j
        d[j] = v[0]
        U[j + 1:, j] = np.divide(v[1:], d[j])
    return U, d


def substitute(U, d, b):
    """gram^-1 b for the columns of b [K][...]"""
    K = d.size
    x = np.array(b, dtype=np.float64)
    for i in range(K):
        s = np.zeros_like(x[0])
        for m in range(i):
            s = np.add(s, np.multiply(U[i, m], x[m]))
        x[i] = np.subtract(x[i], s)
    for i in range(K):
        x[i] = np.divide(x[i], d[i])
    for i in range(K - 1, -1, -1):
        s = np.zeros_like(x[0])
        for m in range(i + 1, K):
            s = np.add(s, np.multiply(U[m, i], x[m]))
        x[i] = np.subtract(x[i], s)
    return x


def restate(L, D, rows=None):
    """every output of cogaps_project for loadings L [n][K] and data D (its rows `rows`, if given) [n][S], float32"""
    L = np.asarray(L, dtype=np.float32)
    D = np.asarray(D, dtype=np.float32)
    if rows is not None:
        D = D[np.asarray(rows, dtype=np.int64)]
    n, K = L.shape
    S = D.shape[1]
    L64, D64 = L.astype(np.float64), D.astype(np.float64)
    Lp, Dp = _padded(L64, n), _padded(D64, n)
    gram = _trip_sums(lambda i: np.multiply(Lp[:, i, :, None], Lp[:, i, None, :]), n)
    cross = _trip_sums(lambda i: np.multiply(Lp[:, i, :, None], Dp[:, i, None, :]), n)
    f = factor(gram)
    if isinstance(f, int):
        raise ValueError("loadings are rank deficient (pattern %d)" % f)
    U, d = f
    coef = substitute(U, d, cross)
    stdev = np.sqrt(np.diagonal(substitute(U, d, np.eye(K))))
    fitted = np.zeros((n, S))
    for k in range(K):
        fitted = np.add(fitted, np.multiply(L64[:, k, None], coef[k][None, :]))
    r = np.subtract(D64, fitted)
    qp = _padded(np.multiply(r, r), n)
    rss = _trip_sums(lambda i: qp[:, i], n)
    return {"coef": coef, "cross": cross, "gram": gram, "stdevUnscaled": stdev, "rss": rss}


KEYS = ("coef", "cross", "gram", "stdevUnscaled", "rss")


def check(got, want, what=""):
    """bit for bit, NaN included"""
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k], dtype=np.float64), np.ascontiguousarray(want[k], dtype=np.float64)
        assert a.shape == b.shape, "%s %s: shape %s against %s" % (what, k, a.shape, b.shape)
        same = a.view(np.uint64) == b.view(np.uint64)
        assert same.all(), "%s %s: %d of %d differ, first at %s: %r against %r" % (
            what, k, (~same).sum(), same.size, np.argwhere(~same)[0], a[~same][0], b[~same][0])


# ---- the exact anchor: 0/1 loadings on disjoint supports of 4, 8 and 16 genes (and 4 genes of no pattern), data = L C + E ----
ANCHOR_SIZES = (4, 8, 16)
ANCHOR_C = np.array([[3, 0, 5, 2], [4, 7, 0, 2], [6, 1, 9, 2]], dtype=np.float64)      # [K][S]
ANCHOR_E = np.array([2, 0, 0, 1], dtype=np.float64)                                     # per sample: samples 1 and 2 have no noise, and each a coefficient of zero


def anchor():
    """-> (L, D, expected): every sum is one of small integers and exact"""
    n, K, S = sum(ANCHOR_SIZES) + 4, len(ANCHOR_SIZES), ANCHOR_E.size
    L, E = np.zeros((n, K), dtype=np.float32), np.zeros((n, S))
    g = 0
    for k, size in enumerate(ANCHOR_SIZES):
        L[g:g + size, k] = 1.0
        E[g:g + size] = np.where(np.arange(size)[:, None] % 2 == 0, 1.0, -1.0) * ANCHOR_E[None, :]
        g += size
    C = ANCHOR_C                                             # (C >= E wherever E is not zero: the data stay >= 0)
    D = L.astype(np.float64) @ C + E
    assert (D >= 0).all() and (D == np.rint(D)).all()
    rss = sum(ANCHOR_SIZES) * ANCHOR_E ** 2
    stdev = np.sqrt(1.0 / np.array(ANCHOR_SIZES, dtype=np.float64))
    df = n - K
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = np.sqrt(rss / df)
        t = C / stdev[:, None] / sigma[None, :]
    return L, D.astype(np.float32), {"projection": C, "rss": rss, "stdevUnscaled": stdev, "df": df, "sigma": sigma, "t": t,
                                       "gram": np.diag(np.array(ANCHOR_SIZES, dtype=np.float64))}


def check_anchor(out, want):
    from scipy.special import erfc
    for k in ("projection", "rss", "stdevUnscaled", "sigma", "t", "gram"):
        a, b = np.asarray(out[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "%s: %r against %r" % (k, a, b)
    assert out["df"] == want["df"]
    p = erfc(np.abs(want["t"]) / np.sqrt(2.0))
    assert np.array_equal(np.asarray(out["pval"]).view(np.uint64), p.view(np.uint64))
    # the sample without noise: a coefficient that is not zero is infinitely significant, one that is zero has no statistic
    quiet = np.flatnonzero(want["rss"] == 0)
    assert quiet.size == 2
    for s in quiet:
        for k in range(want["projection"].shape[0]):
            if want["projection"][k, s] != 0:
                assert np.isposinf(out["t"][k, s]) and out["pval"][k, s] == 0.0
            else:
                assert np.isnan(out["t"][k, s]) and np.isnan(out["pval"][k, s])


# ---- the independent comparator: numpy.linalg.lstsq in float64, one seeded case ----
LSTSQ_SHAPE = (300, 40, 7)
# the largest |restate - lstsq| / max |lstsq| over the coefficients of lstsq_case(), measured on a CPU; the library is
# held to 16 times that: normal equations and an SVD differ by about cond(L)^2 2^-53
LSTSQ_RESTATEMENT_DIFFERENCE = 1.1765056093484096e-14


def lstsq_case():
    n, S, K = LSTSQ_SHAPE
    r = _rng(77, n, S, K)
    L = r.random((n, K)).astype(np.float32)
    C = r.gamma(2.0, 1.0, size=(K, S))
    D = np.maximum(L.astype(np.float64) @ C + r.normal(0.0, 0.5, size=(n, S)), 0.0).astype(np.float32)
    ref = np.linalg.lstsq(L.astype(np.float64), D.astype(np.float64), rcond=None)[0]
    return L, D, ref


def relative_difference(c, ref):
    return float(np.max(np.abs(c - ref)) / np.max(np.abs(ref)))


# ---- one small case in every form the data can take: -> (name, data, keyword arguments of _capi.project); rows: a permutation with repeats ----
FORMS_SHAPE = (70, 3, 67)                                    # genes of the fit, patterns, samples


def forms_case():
    n, K, S = FORMS_SHAPE
    L = loadings(n, K, seed=5)
    pool = data(n - 10, S, seed=6)                           # the data has fewer rows than the fit has genes: some are used twice
    rows = _rng(9).permutation(np.arange(n) % (n - 10)).astype(np.uint32)
    return L, pool, rows


def forms(pool, rows):
    """the matrix D = pool[rows], and pool with `rows`, in every host form"""
    import scipy.sparse as sp
    from cogaps_amd import _capi
    D = np.ascontiguousarray(pool[rows])
    yield "row-major", D, {}
    F = np.asfortranarray(D)
    assert F.strides == (4, 4 * D.shape[0])
    yield "column-major", F, {}
    wide = np.zeros((2 * D.shape[0] + 1, 3 * D.shape[1] + 2), dtype=np.float32)
    wide[1::2, 2::3][:D.shape[0]] = D
    view = wide[1::2, 2::3][:D.shape[0]]
    assert not view.flags["C_CONTIGUOUS"] and not view.flags["F_CONTIGUOUS"]
    yield "a strided slice", view, {}
    yield "dataRows", pool, {"rows": rows}
    yield "transposeData", np.ascontiguousarray(D.T), {"transposeData": True}
    yield "CSR", sp.csr_matrix(D), {}
    yield "CSC", sp.csc_matrix(D), {}
    yield "CSR with dataRows", sp.csr_matrix(pool), {"rows": rows}
    yield "CSC, transposed, with dataRows", sp.csc_matrix(np.ascontiguousarray(pool.T)), {"rows": rows, "transposeData": True}
    r, c = np.nonzero(D)
    v = D[r, c]
    # a position given twice: the latest triplet decides
    r2, c2, v2 = np.concatenate([r[:5], r]), np.concatenate([c[:5], c]), np.concatenate([v[:5] + np.float32(3.0), v])
    yield "triplets with a repeated position", _capi.CooMatrix(D.shape, r2.astype(np.uint32), c2.astype(np.uint32), v2.astype(np.float32)), {}
    dense = sp.csr_matrix(D).toarray()
    assert np.array_equal(dense, D) and (D == 0).mean() > 0.3
    yield "a dense matrix with the same zeros", dense, {}
