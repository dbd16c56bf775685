"""The residuals of a result restated in numpy, and the cases the emulator and the MI355X tests share.  restate() is the
definition, order by order: M by a loop over k, the 64 lane sums of a gene and their xor butterfly, the blocks of 64 genes of a sample's
sum, the sequential total.  A product of two widened floats is exact in fp64, so `M + a * p` here has the bits of the kernel's FMA."""
import numpy as np

LANES = 64        # samples of a step = genes of a block


def restate(A, P, D=None, S=None):
    """A [G][K], P [N][K] float32; D [G][N] float32 or None; S [G][N] float32 or None -> (M, r, geneChiSq, sampleChiSq, chiSq), float64"""
    A64, P64 = np.asarray(A, dtype=np.float32).astype(np.float64), np.asarray(P, dtype=np.float32).astype(np.float64)
    G, K = A64.shape
    N = P64.shape[0]
    M = np.zeros((G, N))
    for k in range(K):
        M = M + A64[:, k][:, None] * P64[:, k][None, :]
    if D is None:
        return M, None, None, None, None
    D64 = np.asarray(D, dtype=np.float32).astype(np.float64)
    if S is None:
        tenth = 0.1 * D64
        s = np.where(tenth > 0.1, tenth, 0.1)
    else:
        s = np.asarray(S, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        r = (D64 - M) / s
        q = r * r
        lanes = np.zeros((G, LANES))
        for j0 in range(0, N, LANES):
            w = min(LANES, N - j0)
            lanes[:, :w] = lanes[:, :w] + q[:, j0:j0 + w]
        idx = np.arange(LANES)
        for off in (1, 2, 4, 8, 16, 32):
            lanes = lanes + lanes[:, idx ^ off]
        gene = lanes[:, 0].copy()
        sample = np.zeros(N)
        for i0 in range(0, G, LANES):
            part = np.zeros(N)
            for i in range(i0, min(i0 + LANES, G)):
                part = part + q[i]
            sample = sample + part
        chi = np.float64(0.0)
        for i in range(G):
            chi = chi + gene[i]
    return M, r, gene, sample, float(chi)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d values differ in their bits, first at %d: %r against %r" % (
        what, bad.size, want.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def factors(G, N, K, seed=0):
    """float32 factor matrices like a run's means: non-negative, a few exact zeros"""
    rng = np.random.default_rng([seed, G, N, K])
    A = rng.gamma(1.5, 1.0, size=(G, K)).astype(np.float32)
    P = rng.gamma(1.5, 0.7, size=(N, K)).astype(np.float32)
    A[rng.random((G, K)) < 0.1] = 0
    P[rng.random((N, K)) < 0.1] = 0
    return A, P


def dense_data(A, P, seed=1):
    """data near A P^T with noise, some zeros, small and large entries on both sides of the default uncertainty's knee at 1"""
    rng = np.random.default_rng([seed, A.shape[0], P.shape[0]])
    D = (A.astype(np.float64) @ P.astype(np.float64).T) * rng.uniform(0.5, 1.5, size=(A.shape[0], P.shape[0]))
    D[rng.random(D.shape) < 0.2] = 0
    return D.astype(np.float32)


def uncertainty_for(D, seed=2):
    rng = np.random.default_rng([seed, D.shape[0], D.shape[1]])
    return (0.05 + 0.2 * D * rng.uniform(0.5, 1.5, size=D.shape)).astype(np.float32)


def sparse_matrix(G=70, N=130, seed=3):
    """the dense form of the sparse cases' matrix: an empty gene (row 5), an empty sample (column 7), entries at (0, 0) and (G - 1, N - 1),
    one full row (row 9, but for the empty sample), N = 130: the last flag word is partial"""
    rng = np.random.default_rng([seed, G, N])
    D = np.where(rng.random((G, N)) < 0.08, rng.gamma(2.0, 2.0, size=(G, N)), 0.0).astype(np.float32)
    D[9, :] = rng.gamma(2.0, 2.0, size=N).astype(np.float32) + np.float32(0.01)
    D[5, :] = 0
    D[:, 7] = 0
    D[0, 0] = 3.5
    D[G - 1, N - 1] = 0.25
    return D


def triplets_of(D, seed=4):
    """(rows, cols, values) denoting D, in shuffled order, with repeated positions: earlier entries that a later one overwrites, positions
    that a later non-positive entry removes, and a removed position that comes back"""
    rng = np.random.default_rng(seed)
    r, c = np.nonzero(D)
    v = D[r, c]
    order = rng.permutation(r.size)
    r, c, v = r[order], c[order], v[order]
    zr, zc = np.nonzero(D == 0)
    pick = rng.choice(zr.size, size=12, replace=False)
    # overwritten: a wrong value first, the right one later
    early_r, early_c, early_v = r[:10], c[:10], v[:10] + np.float32(7)
    # removed: a positive entry at an absent position, then a zero (six of them) or a negative one (six)
    gone_r, gone_c = zr[pick], zc[pick]
    gone_v = np.concatenate([np.zeros(6, np.float32), -np.ones(6, np.float32)])
    rows = np.concatenate([early_r, gone_r, r, gone_r])
    cols = np.concatenate([early_c, gone_c, c, gone_c])
    vals = np.concatenate([early_v, np.full(12, 2.0, np.float32), v, gone_v])
    # a position removed in the middle and present again at the end
    back_r, back_c = r[20], c[20]
    rows = np.concatenate([rows, [back_r, back_r]]); cols = np.concatenate([cols, [back_c, back_c]])
    vals = np.concatenate([vals, [np.float32(0), v[20]]])
    return rows.astype(np.uint32), cols.astype(np.uint32), vals.astype(np.float32)


def write_mtx(path, rows, cols, vals, shape):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (shape[0], shape[1], len(vals)))
        for r, c, v in zip(rows, cols, vals):
            f.write("%d %d %s\n" % (r + 1, c + 1, repr(float(v))))


def check(out, want, rows=None, what=""):
    """a _capi.residuals() dict against restate()'s tuple, bit for bit; rows: the 0-based genes whose rows out["matrix"] holds"""
    M, r, gene, sample, chi = want
    if r is None:
        same_bits(out["matrix"], M[rows], what + " M")
        return
    same_bits(out["geneChiSq"], gene, what + " geneChiSq")
    same_bits(out["sampleChiSq"], sample, what + " sampleChiSq")
    same_bits(out["chiSq"], chi, what + " chiSq")
    if rows is not None:
        same_bits(out["matrix"], r[rows], what + " residuals")
