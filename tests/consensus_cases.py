"""Consensus patterns (cogaps_pattern_match; csrc/consensus_kernel.h): the numpy restatement of the definition, which
every output of the library must equal bit for bit, the input generators and the cases shared by the emulator test
(tests/test_consensus.py) and the MI355X test (tests/test_consensus_gpu.py)."""
import numpy as np

# the constants of the definition and of the kernels (csrc/consensus_kernel.h)
KC = 4096                 # CS_KC: rows of a chunk of the row rule
TILE = 64                 # CS_TILE: columns of a tile of the cross-product kernel
LINK_THREADS = 1024       # CS_LINK_THREADS: the clustering workgroup
MAX_COLS = 4096           # CS_MAX_COLS = COGAPS_PATTERN_MATCH_MAX_COLS

NA_MESSAGE = "NA values in correlation of patterns"
EMPTY_MESSAGE = "no cluster of patterns reaches minNS members"


# ---- the restatement ----
def row_rule(L, term):
    """the one rule of every sum over the rows: term(k) for the rows of a chunk of KC in ascending order from +0.0, the chunk sums in
    ascending chunk order from +0.0"""
    total = None
    for k0 in range(0, L, KC):
        acc = None
        for k in range(k0, min(L, k0 + KC)):
            t = term(k)
            acc = (np.zeros_like(t) + t) if acc is None else acc + t
        total = (np.zeros_like(acc) + acc) if total is None else total + acc
    return total


def widen(X):
    """the float32 input, -0 as +0, exactly in float64"""
    return (np.asarray(X, dtype=np.float32) + np.float32(0)).astype(np.float64)


def correlation_distance(x):
    """-> (mean [n], c [n][n], dist [n][n]) of the float64 matrix x"""
    L = x.shape[0]
    mean = row_rule(L, lambda k: x[k]) / float(L)
    y = x - mean[None, :]
    c = row_rule(L, lambda k: y[k][:, None] * y[k][None, :])
    s = np.sqrt(np.diagonal(c))
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = 1.0 - c / (s[:, None] * s[None, :])
    return mean, c, dist


def cutree(dist, k):
    """complete linkage of dist down to k clusters: the smallest distance is merged, ties to the pair whose lower index is smallest,
    then whose higher index is smallest (the first minimum in row-major order); the merged cluster keeps the lower index and the maximum
    of the two distances; labels by first appearance.  -> (labels, number of merges)"""
    n = dist.shape[0]
    if k >= n:
        return np.arange(1, n + 1), 0
    d = np.array(dist, dtype=np.float64)
    np.fill_diagonal(d, np.inf)
    root = np.arange(n)
    for _ in range(n - k):
        a, b = divmod(int(np.argmin(d)), n)
        assert a < b and np.isfinite(d[a, b])
        merged = np.where(d[b] > d[a], d[b], d[a])
        d[a, :] = merged
        d[:, a] = merged
        d[a, a] = np.inf
        d[b, :] = np.inf
        d[:, b] = np.inf
        root[root == b] = a
    labels, seen = np.zeros(n, dtype=np.int64), {}
    for i in range(n):
        labels[i] = seen.setdefault(int(root[i]), len(seen) + 1)
    return labels, n - k


def corcut(dist, cols, k, min_ns):
    """-> (the clusters of cols with min_ns members or more, in the order of their first members; the labels; the merges)"""
    cols = np.asarray(cols)
    labels, merges = cutree(dist[np.ix_(cols, cols)], k)
    kept = [cols[labels == l] for l in range(1, int(labels.max()) + 1)]
    return [c for c in kept if c.size >= min_ns], labels, merges


def cluster_statistics(x, mean, c, members):
    """-> (r of every member, the float32 consensus column) of the cluster with the ascending columns `members`"""
    L = x.shape[0]
    total = np.zeros(L)
    for j in members:
        total = total + x[:, j]
    mean_pat = total / float(len(members))
    mm = row_rule(L, lambda k: mean_pat[k]) / float(L)
    yp = mean_pat - mm
    cpp = row_rule(L, lambda k: yp[k] * yp[k])
    y = x[:, members] - mean[members][None, :]
    cjp = row_rule(L, lambda k: y[k] * yp[k])
    with np.errstate(invalid="ignore", divide="ignore"):
        cor = cjp / (np.sqrt(np.diagonal(c)[members]) * np.sqrt(cpp))
        r = np.rint(1000.0 * cor) / 1000.0
        w = (r * r) * r
        num, den = np.zeros(L), 0.0
        for t, j in enumerate(members):
            num = num + x[:, j] * w[t]
            den = den + w[t]
        mp = num / den
        return r, (mp / np.max(mp + 0.0)).astype(np.float32)


def restate(X, cut, min_ns, max_ns):
    """what _capi.pattern_match(X, cut, min_ns, max_ns, debug=True) returns, and under "splits" / "merges" what the case went through:
    the corcut calls of the split loop and the merges of the first corcut.  ValueError with the library's message where it refuses."""
    x = widen(X)
    L, n = x.shape
    mean, c, dist = correlation_distance(x)
    if np.isnan(dist).any():
        raise ValueError(NA_MESSAGE)
    clusters, first, merges = corcut(dist, np.arange(n), cut, min_ns)
    splits = 0
    while True:
        big = [i for i, cl in enumerate(clusters) if cl.size > max_ns]
        if not big:
            break
        i = big[0]
        parts, _, _ = corcut(dist, clusters[i], 2, min_ns)
        splits += 1
        if not parts:
            clusters.pop(i)
            continue
        clusters[i] = parts[0]
        if len(parts) > 1:
            clusters.append(parts[1])
    if not clusters:
        raise ValueError(EMPTY_MESSAGE)
    cluster, corr = np.zeros(n, dtype=np.uint32), np.full(n, np.nan)
    consensus = np.zeros((L, len(clusters)), dtype=np.float32)
    for ci, members in enumerate(clusters):
        r, column = cluster_statistics(x, mean, c, members)
        if np.isnan(r).any():
            raise ValueError(NA_MESSAGE)
        cluster[members], corr[members], consensus[:, ci] = ci + 1, r, column
    return {"nClusters": len(clusters), "cluster": cluster, "corr": corr, "consensus": consensus, "dist": dist,
            "firstLabels": first.astype(np.uint32), "splits": splits, "merges": merges}


def check(got, want, what=""):
    """every output of the library against the restatement, bit for bit"""
    assert got["nClusters"] == want["nClusters"], (what, got["nClusters"], want["nClusters"])
    assert np.array_equal(got["dist"].view(np.uint64), want["dist"].view(np.uint64)), (what, "dist", int((got["dist"] != want["dist"]).sum()))
    assert np.array_equal(got["firstLabels"], want["firstLabels"]), (what, "firstLabels")
    assert np.array_equal(got["cluster"], want["cluster"]), (what, "cluster")
    assert np.array_equal(got["corr"], want["corr"], equal_nan=True), (what, "corr")
    assert got["consensus"].shape == want["consensus"].shape, (what, got["consensus"].shape)
    assert np.array_equal(got["consensus"].view(np.uint32), want["consensus"].view(np.uint32)), (what, "consensus")


# ---- inputs ----
def planted(L, sizes, seed, noise=0.4, spread=None):
    """groups of sizes[g] columns around one random non-negative pattern each, the columns of the groups interleaved (column j belongs
    to group j mod len(sizes) while that group has columns left); spread[g] (default: none) moves the halves of group g apart, so that
    the group is one cluster that splits in two.  -> float32 [L][sum(sizes)]"""
    rng = np.random.Generator(np.random.MT19937(seed))
    base = rng.gamma(2.0, 1.0, size=(L, len(sizes)))
    left, order = list(sizes), []
    while any(left):
        for g in range(len(sizes)):
            if left[g]:
                left[g] -= 1
                order.append(g)
    seen = [0] * len(sizes)
    cols = []
    for g in order:
        col = base[:, g] * (1.0 + noise * rng.random(L))
        if spread is not None and spread[g]:
            half = seen[g] % 2
            col = col + spread[g] * half * np.roll(base[:, g], 1)
        seen[g] += 1
        cols.append(col)
    return np.stack(cols, axis=1).astype(np.float32)


def random_patterns(L, n, seed):
    rng = np.random.Generator(np.random.MT19937(seed))
    return rng.gamma(2.0, 1.0, size=(L, n)).astype(np.float32)


def repeated_columns(L=9, distinct=5, copies=4, seed=21):
    """every column several times, exactly: the distances inside a group and between two groups are equal numbers"""
    return np.tile(random_patterns(L, distinct, seed), (1, copies))


def small_integers(L=6, n=40, seed=22):
    """entries 0 .. 2 in few rows: many pairs of columns are equally far apart (no column is constant)"""
    rng = np.random.Generator(np.random.MT19937(seed))
    X = rng.integers(0, 3, size=(L, n)).astype(np.float32)
    X[0, :] = 0
    X[1, :] = 2
    return X


# name -> (matrix, cut, minNS, maxNS): the shapes at which the kernels can go wrong, named by the constant they sit at
def shape_cases():
    return {
        "L=2": (random_patterns(2, 4, 1), 2, 1, 4),
        "L=3": (random_patterns(3, 5, 2), 2, 1, 5),
        "L=KC-1,n=5": (planted(KC - 1, [3, 2], 3), 2, 2, 5),
        "L=KC,n=5": (planted(KC, [3, 2], 4), 2, 2, 5),
        "L=KC+37,n=5": (planted(KC + 37, [3, 2], 5), 2, 2, 5),
        "n=2": (random_patterns(10, 2, 6), 1, 2, 2),
        "n=TILE+1": (planted(33, [22, 22, 21], 7), 3, 2, 30),
        "n=4*TILE+3,L=17": (planted(17, [90, 90, 79], 8, noise=0.5), 6, 2, 100),
        "n=7,L=10": (planted(10, [4, 3], 9), 2, 2, 7),
    }


def many_columns_case():
    """n above the clustering workgroup's threads (a thread owns two rows of the neighbour arrays), more than a thousand merges"""
    n = LINK_THREADS + 76
    return planted(24, [n // 40 + (1 if g < n % 40 else 0) for g in range(40)], 10, noise=0.3), 40, 2, n


# the split loop: name -> (matrix, cut, minNS, maxNS, corcut calls of the loop, clusters in the end)
def split_cases():
    return {
        # three groups; the first, of nine, is one cluster of the first cut, above maxNS = 4, and comes apart in two steps
        "splits twice": (planted(40, [9, 3, 3], 11, spread=[0.6, 0, 0]), 3, 2, 4, 2, 5),
        # a cluster of five above maxNS = 4 whose split leaves four columns and one: the one is below minNS = 2 and goes
        "a part is dropped": (np.concatenate([planted(40, [4, 3], 12), (planted(40, [1], 13, noise=0.8) + planted(40, [4, 3], 12)[:, :1])], axis=1), 2, 2, 4, 1, 2),
        # the first cut leaves a column on its own, below minNS
        "minNS drops a first-pass cluster": (np.concatenate([planted(40, [3, 3], 14), random_patterns(40, 1, 15)], axis=1), 3, 2, 6, 0, 2),
    }


def well_separated():
    """planted patterns far apart with little noise: where the library's rounded correlations equal the host path's"""
    return planted(50, [4, 4, 4], 16, noise=0.3), 3, 2, 6
