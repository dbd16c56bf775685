"""The enrichment of gene sets in every pattern restated in numpy from DESIGN.md 4.11 (not from the kernel): the stable ranking, the
running sum added in rank order, the two divisions, the first maximum, the keyed draw of gene_set_cases and the integer sums of the
permutation null -- and the cases the CPU (emulator) and GPU tests share."""
import functools

import numpy as np

from gene_set_cases import draws

SCALE = 2.0 ** 40


def ranks(stat):
    """-> (order int64 [K][n]: the rows by decreasing value, ties by ascending row; rank int64 [K][n]: its inverse)"""
    x = np.asarray(stat, dtype=np.float32).astype(np.float64)
    n, K = x.shape
    order = np.stack([np.argsort(-x[:, k], kind="stable") for k in range(K)])
    rank = np.empty_like(order)
    for k in range(K):
        rank[k, order[k]] = np.arange(n)
    return order, rank


def score(x, rank, rows):
    """the enrichment score of the row subsets `rows` (int64 [B][m], distinct in each line) in one column: x float64 [n], rank its
    ranks -> (ES float64 [B], peak int64 [B])"""
    n, (B, m) = x.shape[0], rows.shape
    r = np.sort(rank[rows], axis=1)                                     # the members in rank order ...
    inv = np.empty(n, dtype=np.int64); inv[rank] = np.arange(n)
    v = x[inv[r]]                                                       # ... and their values
    cum = np.add.accumulate(v, axis=1)                                  # sequential, one add per member, from +0 (0 + v_0 == v_0)
    NR = cum[:, -1:]
    i = np.arange(m, dtype=np.int64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        hit = np.where(NR == 0.0, (i + 1).astype(np.float64) / np.float64(m), cum / NR)
    top = hit - (r - i).astype(np.float64) / np.float64(n - m)
    return top.max(axis=1), top.argmax(axis=1)                          # argmax: the first maximum


def gsea(stat, members, numPerm, seed, set_base=0):
    """-> es float64, peak uint32, nGe uint32, permSum uint64: [nSets][K]"""
    x = np.asarray(stat, dtype=np.float32).astype(np.float64)
    n, K = x.shape
    _, rank = ranks(stat)
    T = len(members)
    es, peak = np.zeros((T, K)), np.zeros((T, K), dtype=np.uint32)
    nGe, permSum = np.zeros((T, K), dtype=np.uint32), np.zeros((T, K), dtype=np.uint64)
    for t, mem in enumerate(members):
        mem = np.asarray(mem, dtype=np.int64)
        idx = draws(n, mem.size, seed, set_base + t, np.arange(numPerm))
        for k in range(K):
            e, p = score(x[:, k], rank[k], mem[None, :])
            es[t, k], peak[t, k] = e[0], p[0]
            pe, _ = score(x[:, k], rank[k], idx)
            nGe[t, k] = (pe >= e[0]).sum()
            permSum[t, k] = np.floor(pe * SCALE).astype(np.uint64).sum(dtype=np.uint64)
    return {"es": es, "peak": peak, "nGe": nGe, "permSum": permSum}


def bh(p):
    """Benjamini-Hochberg over the entries of p that are not NaN; NaN stays"""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    ok = np.flatnonzero(~np.isnan(p))
    if ok.size:
        o = ok[np.argsort(-p[ok], kind="stable")]                       # decreasing p
        q = p[o] * ok.size / np.arange(ok.size, 0, -1)
        out[o] = np.minimum(1.0, np.minimum.accumulate(q))
    return out


# ---- item 1: ranks ----
def gamma_loadings(n, K, seed, zero_column=None):
    """gamma-distributed float32 loadings with 30 % exact zeros, optionally one all-zero column"""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.gamma(2.0, 1.0, size=(n, K))
    a[rng.random((n, K)) < 0.3] = 0.0
    if zero_column is not None:
        a[:, zero_column] = 0.0
    return a.astype(np.float32)


RANK_SHAPES = [(300, 70, 5), (4200, 3, None)]       # (rows, columns, the all-zero column)

# ---- item 2: scores, bit for bit ----
N_ROWS, K_MAX, SEED = 300, 130, 20240611
SIZES = (1, 2, 63, 64, 65, 200)
K_CASES, PERM_CASES = (1, 3, 64, 70, 130), (1, 7, 130)


@functools.lru_cache(maxsize=None)
def score_sets():
    """40 sets: sizes in turn from SIZES; every fifth set of more than one member has lost some"""
    rng = np.random.Generator(np.random.PCG64(11))
    members = []
    for t in range(40):
        s = SIZES[t % len(SIZES)]
        mem = np.sort(rng.choice(N_ROWS, size=s, replace=False))
        if t % 5 == 0 and s > 2:
            mem = mem[rng.random(s) < 0.6]
        members.append(mem.astype(np.uint32))
    return members


@functools.lru_cache(maxsize=None)
def stat_random():
    return gamma_loadings(N_ROWS, K_MAX, 5)


@functools.lru_cache(maxsize=None)
def stat_integer():
    return np.random.Generator(np.random.PCG64(6)).integers(0, 4, size=(N_ROWS, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def stat_zero_members():
    """stat_random's first three columns, with column 1 zero on the members of set 2 (63 rows): NR == 0 for the set itself"""
    a = stat_random()[:, :3].copy()
    a[score_sets()[2], 1] = 0.0
    return a


@functools.lru_cache(maxsize=None)
def expected(kind, numPerm):
    """the restatement's answer for all the columns (a column's outputs do not depend on the other columns: the tests slice it)"""
    stat = {"random": stat_random, "integer": stat_integer, "zero": stat_zero_members}[kind]()
    return gsea(stat, score_sets(), numPerm, SEED)


def integer_equalities(numPerm=130):
    """how often a permutation's score equals the set's own with the integer loadings (>= against > decides those)"""
    stat, members = stat_integer(), score_sets()
    x = stat.astype(np.float64)
    _, rank = ranks(stat)
    same = 0
    for t, mem in enumerate(members):
        idx = draws(N_ROWS, mem.size, SEED, t, np.arange(numPerm))
        for k in range(stat.shape[1]):
            e, _ = score(x[:, k], rank[k], mem.astype(np.int64)[None, :])
            same += int((score(x[:, k], rank[k], idx)[0] == e[0]).sum())
    return same


# ---- item 3: the size classes of the sort ----
BIG_ROWS, BIG_K, BIG_PERM, BIG_SIZES = 4200, 3, 3, (1024, 1025, 4095, 4096)


@functools.lru_cache(maxsize=None)
def big_case():
    stat = gamma_loadings(BIG_ROWS, BIG_K, 9)
    rng = np.random.Generator(np.random.PCG64(10))
    members = [np.sort(rng.choice(BIG_ROWS, size=s, replace=False)).astype(np.uint32) for s in BIG_SIZES]
    return stat, members, gsea(stat, members, BIG_PERM, 3)


# ---- item 4: more trips than workgroups ----
@functools.lru_cache(maxsize=None)
def many_sets_case():
    rng = np.random.Generator(np.random.PCG64(21))
    stat = stat_random()[:, :5]
    members = [np.sort(rng.choice(N_ROWS, size=(1, 2, 5)[t % 3], replace=False)).astype(np.uint32) for t in range(600)]
    return stat, members, gsea(stat, members, 130, 2)


# ---- item 7: the hypergeometric tail, exactly ----
def hypergeometric_upper_tail(N, K, n, x):
    """P(X >= x), X ~ Hypergeometric(universe N, K successes, n draws), as an exact rational"""
    from fractions import Fraction
    from math import comb
    return Fraction(sum(comb(K, i) * comb(N - K, n - i) for i in range(x, min(K, n) + 1)), comb(N, n))


# ------------------------------------------------------------------------------------------------
# The checks both test files run, each with its own library (the emulator's build, the MI355X's)
# ------------------------------------------------------------------------------------------------
def _capi():
    from cogaps_amd import _capi
    return _capi


def check_ranks(lib, n, K, zero_column):
    stat = gamma_loadings(n, K, 1, zero_column)
    got = _capi().pattern_gsea(stat, [np.array([0], dtype=np.uint32)], 1, ranks=True, lib=lib)["rank"]
    assert got.shape == (K, n) and np.array_equal(got, ranks(stat)[1])


def check_scores(lib, stat, numPerm, want, members=None):
    got = _capi().pattern_gsea(stat, score_sets() if members is None else members, numPerm, seed=SEED, lib=lib)
    K = stat.shape[1]
    for key in ("es", "peak", "nGe", "permSum"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key][:, :K]), key
    return got


def check_big(lib):
    stat, members, want = big_case()
    got = _capi().pattern_gsea(stat, members, BIG_PERM, seed=3, lib=lib)
    for key in ("es", "peak", "nGe", "permSum"):
        assert np.array_equal(got[key], want[key]), key


def raw_result_with_names(names=True):
    from cogaps_amd import CogapsResult
    from gene_set_cases import raw_result
    raw = raw_result()
    n, nS = raw["Amean"].shape[0], raw["Pmean"].shape[0]
    return CogapsResult(raw, geneNames=["g%d" % i for i in range(n)] if names else None, sampleNames=["s%d" % i for i in range(nS)] if names else None), raw


def check_planted(lib, seed=None):
    """the six top-ranked rows of pattern 0 score exactly 1 and no draw reaches them; the six bottom-ranked rows are no enrichment"""
    res, raw = raw_result_with_names()
    order, rank = ranks(raw["Amean"])
    top, bottom = order[0][:6], order[0][-6:]
    numPerm = 200
    out = res.getPatternGeneSet({"top": ["g%d" % i for i in top[::-1]], "bottom": ["g%d" % i for i in bottom]}, numPerm=numPerm, seed=seed, lib=lib)
    assert out["ES"][0, 0] == 1.0 and out["nMoreExtreme"][0, 0] == 0 and out["pval"][0, 0] == 1.0 / (numPerm + 1)
    assert out["leadingEdge"][0][0] == ["g%d" % i for i in top]              # peak == 5: all six, in rank order
    want = gsea(raw["Amean"], [np.sort(top), np.sort(bottom)], numPerm, raw["seed"] if seed is None else seed)
    assert want["peak"][0, 0] == 5 and want["es"][0, 0] == 1.0 and want["nGe"][0, 0] == 0
    assert np.array_equal(out["ES"], want["es"].T) and np.array_equal(out["nMoreExtreme"], want["nGe"].T)
    assert out["pval"][0, 1] >= 0.5
