"""The gene-set permutation statistic restated in numpy from DESIGN.md 4.8 (not from the kernel): the keyed draw, the in-order
float64 sums, one division, the strict comparison -- and the cases the CPU (emulator) and GPU tests share."""
import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """uint32 finaliser, on uint64 arrays holding 32-bit values (so that nothing wraps behind numpy's back)"""
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & M32
    return x ^ (x >> np.uint64(16))


def draws(n, s, seed, t, perms):
    """indices j = 0 .. s-1 of the permutations `perms` of set t: int64 [len(perms)][s]"""
    perms = np.asarray(perms, dtype=np.uint64).reshape(-1, 1)
    keys = [mix(np.uint64(seed) ^ mix(np.uint64(t) ^ mix(perms ^ np.uint64(((r + 1) * 0x9E3779B9) & 0xFFFFFFFF)))) for r in range(4)]
    h = (max(2, int(n - 1).bit_length()) + 1) // 2
    hh, mask = np.uint64(h), np.uint64((1 << h) - 1)

    def E(x, rows):
        L, R = x >> hh, x & mask
        for r in range(4):
            L, R = R, L ^ (mix(R ^ keys[r][rows, 0]) & mask)
        return (L << hh) | R

    x = np.broadcast_to(np.arange(s, dtype=np.uint64), (perms.shape[0], s)).copy()
    rows = np.broadcast_to(np.arange(perms.shape[0]).reshape(-1, 1), x.shape)
    todo = np.ones(x.shape, dtype=bool)                     # do x = E(x) while x >= n
    while todo.any():
        x[todo] = E(x[todo], rows[todo])
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def draw(n, s, seed, t, p):
    return draws(n, s, seed, t, [p])[0]


def counts(Z, members, sizes, numPerm, seed):
    """-> (lessThanCount uint32 [nSets][K], actualMean float64 [nSets][K])"""
    Z = np.asarray(Z, dtype=np.float64)
    n, K = Z.shape
    cnt, act = np.zeros((len(members), K), dtype=np.uint32), np.zeros((len(members), K), dtype=np.float64)
    for t, (mem, s) in enumerate(zip(members, sizes)):
        acc = np.zeros(K)
        for i in mem:                                       # ascending row order
            acc = acc + Z[i]
        with np.errstate(invalid="ignore", divide="ignore"):
            act[t] = acc / np.float64(len(mem))
        idx = draws(n, s, seed, t, np.arange(numPerm))
        acc = np.zeros((numPerm, K))
        for j in range(s):                                  # draws in order
            acc = acc + Z[idx[:, j]]
        cnt[t] = (act[t][None, :] < acc / np.float64(s)).sum(axis=0)
    return cnt, act


# ---- item 1: the shapes of the draw ----
DRAW_SHAPES = [(1, 1), (2, 1), (3, 3), (64, 64), (65, 64), (65, 65), (1363, 1), (1363, 63), (1363, 65), (1363, 300), (4096, 130), (4097, 130)]
DRAW_KEYS = [(0, 0, 0), (42, 3, 999), (0xFFFFFFFF, 4999, 17)]      # (seed, set, perm)

# ---- item 2: counts, bit for bit ----
N_ROWS, K_MAX, SEED = 300, 70, 20240611
SIZES = (1, 2, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def count_sets():
    """40 sets: sizes in turn from SIZES; every fifth set has lost some members (m < s), set 7 all of them (m = 0)"""
    rng = np.random.Generator(np.random.PCG64(11))
    members, sizes = [], []
    for t in range(40):
        s = SIZES[t % len(SIZES)]
        mem = np.sort(rng.choice(N_ROWS, size=s, replace=False))
        if t == 7:
            mem = mem[:0]
        elif t % 5 == 0 and s > 1:
            mem = mem[rng.random(s) < 0.6]
        members.append(mem.astype(np.uint32)); sizes.append(s)
    return members, sizes


@functools.lru_cache(maxsize=None)
def z_random():
    return np.random.Generator(np.random.PCG64(5)).normal(size=(N_ROWS, K_MAX))


@functools.lru_cache(maxsize=None)
def z_integer():
    return np.random.Generator(np.random.PCG64(6)).integers(0, 4, size=(N_ROWS, 3)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def expected(kind, numPerm):
    """the restatement's answer for all K_MAX columns (a column's counts do not depend on the other columns: the tests slice it)"""
    members, sizes = count_sets()
    return counts(z_random() if kind == "random" else z_integer(), members, sizes, numPerm, SEED)


# ---- item 3: an exact answer ----
HG_N, HG_HOT, HG_S, HG_PERM = 1363, 200, 30, 1000


def hypergeometric_case():
    """Z: the indicator of HG_HOT of HG_N rows; sets of HG_S members with h hot rows, h in (2, 4, 6, 8), three each"""
    rng = np.random.Generator(np.random.PCG64(3))
    hot = np.sort(rng.choice(HG_N, size=HG_HOT, replace=False))
    cold = np.setdiff1d(np.arange(HG_N), hot)
    Z = np.zeros((HG_N, 1)); Z[hot, 0] = 1.0
    members, hs = [], []
    for h in (2, 4, 6, 8):
        for _ in range(3):
            members.append(np.sort(np.concatenate([rng.choice(hot, size=h, replace=False), rng.choice(cold, size=HG_S - h, replace=False)])).astype(np.uint32))
            hs.append(h)
    return Z, members, hs


def hypergeometric_tail(h):
    """P(X > h), X ~ Hypergeometric(HG_N, HG_HOT, HG_S)"""
    from math import comb
    return sum(comb(HG_HOT, x) * comb(HG_N - HG_HOT, HG_S - x) for x in range(h + 1, HG_S + 1)) / comb(HG_N, HG_S)


# ---- item 4: a result without a run ----
def raw_result(n=120, K=4, nS=9, seed=77):
    rng = np.random.Generator(np.random.PCG64(8))
    return {"Amean": rng.gamma(2.0, 1.0, size=(n, K)).astype(np.float32), "Asd": (0.2 + rng.random((n, K))).astype(np.float32),
            "Pmean": rng.gamma(2.0, 1.0, size=(nS, K)).astype(np.float32), "Psd": (0.2 + rng.random((nS, K))).astype(np.float32), "seed": seed}
