"""Gene-set membership (calcGeneGSStat, computeGeneGSProb) restated in numpy from DESIGN.md 4.13 (not from the kernel): the weights
from the permutation counts, the three in-order float64 sums, the two divisions, the two thresholds, the strict comparison -- and the
cases the CPU (emulator) and GPU tests share.  The permutation counts are gene_set_cases.counts'."""
import functools

import numpy as np

import gene_set_cases as gc


def weights(count, numPerm, Pw=None):
    """-> (GSUpreg floored at 1 / numPerm, g = -log of it, w = g * Pw or g), each [nSets][K]"""
    up = np.maximum(np.asarray(count), 1) / np.float64(numPerm)
    g = -np.log(up)
    return up, g, g if Pw is None else g * np.asarray(Pw, dtype=np.float64)[None, :]


def weight_sum(w):
    W = np.float64(0.0)
    for k in range(len(w)):
        W = W + w[k]
    return W


def row_stat(Z, w):
    """T of every row of Z under the K weights w"""
    Z = np.asarray(Z, dtype=np.float64)
    R, S = np.zeros(Z.shape[0]), np.zeros(Z.shape[0])
    for k in range(Z.shape[1]):
        R = R + Z[:, k]
        S = S + Z[:, k] * w[k]                              # the product is rounded, then added
    W = weight_sum(w)
    with np.errstate(invalid="ignore", divide="ignore"):
        T = (S / W) / R
    T[R < 1e-6] = 0.0                                       # (true of a negative sum, never of a NaN)
    if W < 1e-6:
        T[:] = 0.0
    return T


def membership(Z, members, wMember, wNull=None):
    """-> (per set the members' T under wMember, per set the count of rows outside the set whose T under wNull is greater, T under
    wNull of every row [nSets][N])"""
    if wNull is None:
        wNull = wMember
    N = np.asarray(Z).shape[0]
    stat, cnt, allStat = [], [], np.zeros((len(members), N))
    for t, mem in enumerate(members):
        mem = np.asarray(mem, dtype=np.int64)
        allStat[t] = row_stat(Z, wNull[t])
        stat.append(row_stat(Z, wMember[t])[mem])
        outside = np.ones(N, dtype=bool)
        outside[mem] = False
        null = allStat[t][outside]
        with np.errstate(invalid="ignore"):
            cnt.append(np.array([int((null > x).sum()) for x in stat[t]], dtype=np.int64))
    return stat, cnt, allStat


def gene_prob(Z, members, sizes, numPerm, seed, Pw=None, PwNull=False):
    """computeGeneGSProb -> (prob, stat, greaterCount per set, nullSize [nSets], GSUpreg [nSets][K])"""
    Z = np.asarray(Z, dtype=np.float64)
    up, g, w = weights(gc.counts(Z, members, sizes, numPerm, seed)[0], numPerm, Pw)
    wNull = w if PwNull or Pw is None else g
    stat, cnt, _ = membership(Z, members, w, wNull)
    nullSize = np.array([Z.shape[0] - len(m) for m in members], dtype=np.int64)
    prob = []
    for t in range(len(members)):
        with np.errstate(invalid="ignore", divide="ignore"):
            p = cnt[t] / np.float64(nullSize[t])
        p[np.isnan(stat[t])] = np.nan
        if weight_sum(w[t]) < 1e-6 or weight_sum(wNull[t]) < 1e-6 or nullSize[t] == 0:
            p[:] = np.nan
        prob.append(p)
    return prob, stat, cnt, nullSize, up


def concat(parts, dtype):
    return np.concatenate([np.asarray(p, dtype=dtype) for p in parts]) if parts else np.zeros(0, dtype=dtype)


# ---- item 1: the C entry against the restatement ----
K_LIST, PERM_LIST = (1, 3, 64, 65, 70, 130), (1, 7, 130)
K_MAX = 130


@functools.lru_cache(maxsize=None)
def z_wide():
    """gene_set_cases.z_random() (300 x 70, normal values) and 60 more columns from another stream"""
    return np.concatenate([gc.z_random(), np.random.Generator(np.random.PCG64(15)).normal(size=(gc.N_ROWS, K_MAX - gc.K_MAX))], axis=1)


@functools.lru_cache(maxsize=None)
def perm_counts(numPerm):
    """the permutation counts of the 40 sets of gene_set_cases.count_sets() in all K_MAX columns (a column's do not depend on the others)"""
    members, sizes = gc.count_sets()
    right = gc.counts(z_wide()[:, gc.K_MAX:], members, sizes, numPerm, gc.SEED)[0]
    return np.concatenate([gc.expected("random", numPerm)[0], right], axis=1)


def pattern_weights(K):
    return 0.25 + np.random.Generator(np.random.PCG64(100 + K)).random(K)


@functools.lru_cache(maxsize=None)
def entry_case(K, numPerm, mode):
    """mode "plain": no Pw; "pw": Pw on members and null (wNull NULL); "split": Pw on the members only (wNull = g)
    -> (Z, members, wMember, wNull or None, the restatement's answer)"""
    members, _ = gc.count_sets()
    Z = z_wide()[:, :K]
    _, g, w = weights(perm_counts(numPerm)[:, :K], numPerm, None if mode == "plain" else pattern_weights(K))
    wNull = g if mode == "split" else None
    return Z, members, w, wNull, membership(Z, members, w, wNull)


# ---- item 3: ties ----
def tie_case():
    """small-integer Z and power-of-two weights: every sum is exact, many statistics are equal"""
    members, _ = gc.count_sets()
    Z = gc.z_integer()
    rng = np.random.Generator(np.random.PCG64(31))
    w = 2.0 ** rng.integers(-2, 3, size=(len(members), Z.shape[1]))
    wNull = 2.0 ** rng.integers(-2, 3, size=(len(members), Z.shape[1]))
    return Z, members, w, wNull


def order_free_counts(Z, members, w, wNull):
    """the definition as one vectorised expression, the sums in whatever order numpy takes (exact for tie_case's numbers; no row sum
    of z_integer is below 1e-6 except an exact 0, which is mapped like the definition's)"""
    R = Z.sum(axis=1)
    out = []
    for t, mem in enumerate(members):
        with np.errstate(invalid="ignore", divide="ignore"):
            Tm = np.where(R < 1e-6, 0.0, (Z @ w[t] / w[t].sum()) / R)
            Tn = np.where(R < 1e-6, 0.0, (Z @ wNull[t] / wNull[t].sum()) / R)
        outside = np.setdiff1d(np.arange(Z.shape[0]), mem)
        out.append((Tn[outside][None, :] > Tm[np.asarray(mem, dtype=np.int64)][:, None]).sum(axis=1).astype(np.int64))
    return out


# ---- item 7: the front end ----
def planted_set():
    """gene_set_cases.raw_result(n=120, K=4): the eight rows with the largest Z in pattern 0 and the row with the smallest share of
    pattern 0 in its Z -> (raw, rows ascending, the intruder)"""
    raw = gc.raw_result(n=120, K=4)
    z = raw["Amean"].astype(np.float64) / raw["Asd"].astype(np.float64)
    top = np.argsort(z[:, 0])[-8:]
    intruder = int(np.argmin(z[:, 0] / z.sum(axis=1)))
    assert intruder not in top
    return raw, np.sort(np.append(top, intruder)), intruder
