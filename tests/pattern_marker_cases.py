"""Pattern markers restated in numpy from DESIGN.md 4.9 (not from the kernels): the scaling, the row normalisation, the float64 sums in
increasing k, the stable ranking with NaN last, and the two thresholds -- and the cases the CPU (emulator) and GPU tests share."""
import functools

import numpy as np


def restate(A, O, lp=None, threshold="all"):
    """-> (ranks int64 [n][L], scores float64 [n][L], markers: L int64 arrays of 0-based rows)"""
    A, O = np.asarray(A, dtype=np.float64), np.asarray(O, dtype=np.float64)
    n, K = A.shape
    pscale = O.max(axis=0)
    Am = A * pscale[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        X = Am / Am.max(axis=1)[:, None]
    lp = np.eye(K) if lp is None else np.asarray([np.asarray(v, dtype=np.float64) for v in lp])
    L = lp.shape[0]
    scores = np.zeros((n, L))
    for l in range(L):
        acc = np.zeros(n)                                   # from +0, increasing k, one multiplication and one addition each
        for k in range(K):
            d = X[:, k] - lp[l, k]
            acc = acc + d * d
        scores[:, l] = np.sqrt(acc)
    order = np.argsort(scores, axis=0, kind="stable")       # ties in row order, NaN last in row order
    ranks = np.zeros((n, L), dtype=np.int64)
    for l in range(L):
        ranks[order[:, l], l] = np.arange(1, n + 1)
    nan = np.isnan(scores[:, 0])
    assert all(np.array_equal(np.isnan(scores[:, l]), nan) for l in range(L))      # a row is NaN everywhere or nowhere
    z = int(nan.sum())
    lowest = ranks.min(axis=1)
    markers = []
    if threshold == "all":
        best = ranks.argmin(axis=1)                         # which.min: the first of equal minima
        for l in range(L):
            rows = order[:, l]                              # by increasing rank in l
            markers.append(rows[(best[rows] == l) & ~nan[rows]].astype(np.int64))
    elif threshold == "cut":
        for l in range(L):
            rows = order[:, l]
            worse = np.flatnonzero(ranks[rows, l] > lowest[rows])      # positions whose row ranks better in another column
            j = int(worse[0]) if worse.size else n
            markers.append(rows[:min(j, n - z)].astype(np.int64))
    else:
        raise ValueError(threshold)
    return ranks, scores, markers


# ---- the matrices ----
N_MAX, M_ROWS, K_MAX = 257, 41, 70
ROW_COUNTS = (1, 2, 63, 64, 65, 257)
WIDTHS = (1, 3, 64, 65, 70)
THRESHOLDS = ("all", "cut")
TIE_ROWS, TIE_K = 300, 5


@functools.lru_cache(maxsize=None)
def random_pair():
    """A (N_MAX x K_MAX) and O (M_ROWS x K_MAX): positive, skewed like factor matrices, float32 values widened"""
    rng = np.random.Generator(np.random.PCG64(31))
    A = rng.gamma(0.7, 1.0, size=(N_MAX, K_MAX)).astype(np.float32).astype(np.float64)
    O = rng.gamma(0.7, 1.0, size=(M_ROWS, K_MAX)).astype(np.float32).astype(np.float64)
    return A, O


@functools.lru_cache(maxsize=None)
def tie_pair(n=TIE_ROWS, K=TIE_K, seed=17):
    """integer-valued A (entries 0 .. 3) with three all-zero rows, one of them the last; O such that every pscale is 1: X takes few
    values, so whole groups of rows tie"""
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.integers(0, 4, size=(n, K)).astype(np.float64)
    A[A.max(axis=1) == 0, 0] = 1.0                          # the zero rows are the planted ones only
    for i in (n // 3, (2 * n) // 3, n - 1):
        A[i] = 0.0
    O = rng.random(size=(7, K))
    O[3] = 1.0
    return A, O


@functools.lru_cache(maxsize=None)
def twin_pair():
    """-> (A, O, lp): pattern vectors 0 and 2 are the same, so their columns of scores and ranks are equal, and `best` must take 0"""
    A, O = random_pair()
    lp = np.array([[1.0, 0.25, 0.0, 0.0], [0.0, 0.0, 1.0, 0.5], [1.0, 0.25, 0.0, 0.0]])
    return A[:130, :4], O[:, :4], lp


@functools.lru_cache(maxsize=None)
def lp_vectors(L, K=5):
    rng = np.random.Generator(np.random.PCG64(100 + L))
    lp = rng.random(size=(L, K))
    lp[0] = (lp[0] > 0.5).astype(np.float64)                # one vector of zeros and ones that is no unit vector
    lp[-1, 0] = 1.0
    return lp


@functools.lru_cache(maxsize=None)
def large_pair(n=200000, K=8):
    """the GPU-only case at the natural cutoffs: integer-valued, ties abound"""
    rng = np.random.Generator(np.random.PCG64(23))
    A = rng.integers(0, 6, size=(n, K)).astype(np.float64)
    A[::5003] = 0.0
    A[n - 1] = 0.0
    O = rng.integers(1, 4, size=(50, K)).astype(np.float64)
    return A, O


@functools.lru_cache(maxsize=None)
def expected(kind, n, K, threshold, L=0):
    if kind == "random":
        A, O = random_pair()
        A, O = A[:n, :K], O[:, :K]
    elif kind == "ties":
        A, O = tie_pair()
        A = A[:n]
    elif kind == "twins":
        return restate(*twin_pair(), threshold)
    elif kind == "large":
        A, O = large_pair()
    else:
        raise ValueError(kind)
    return restate(A, O, lp_vectors(L, K) if L else None, threshold)


def inputs(kind, n, K):
    if kind == "random":
        A, O = random_pair()
        return A[:n, :K], O[:, :K]
    if kind == "ties":
        A, O = tie_pair()
        return A[:n], O
    return large_pair()


def check(got, want):
    """ranks, scores, every marker list and its length, exactly; NaN equal to NaN"""
    ranks, scores, markers = got
    assert ranks.shape == want[0].shape and np.array_equal(ranks, want[0])
    scores = np.ascontiguousarray(scores)
    assert scores.dtype == np.float64 and scores.shape == want[1].shape
    assert ((scores.view(np.uint64) == np.ascontiguousarray(want[1]).view(np.uint64)) | (np.isnan(scores) & np.isnan(want[1]))).all()
    assert len(markers) == len(want[2])
    for l, (g, w) in enumerate(zip(markers, want[2])):
        assert g.size == w.size and np.array_equal(g, w), "pattern %d" % l


# ---- a result without a run ----
def raw_result(n=90, K=4, nS=23):
    rng = np.random.Generator(np.random.PCG64(9))
    raw = {"Amean": rng.gamma(0.7, 1.0, size=(n, K)).astype(np.float32), "Asd": (0.2 + rng.random((n, K))).astype(np.float32),
           "Pmean": rng.gamma(0.7, 1.0, size=(nS, K)).astype(np.float32), "Psd": (0.2 + rng.random((nS, K))).astype(np.float32), "seed": 5}
    raw["Amean"][11] = 0.0                                  # a gene no pattern uses
    return raw
