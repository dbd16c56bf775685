"""Shared step-wise comparison of a library session (HIP, or the test-only emulator build) with the
oracle: per-batch proposal traces (type, rows, columns, positions, PCG states, atom indices), atom
vectors (position, mass, neighbour links in vector order), factor matrices, AP caches, chi2,
average queue length -- all bit-exact."""
import numpy as np

from cogaps_amd import _capi
import pyoracle as po


def make_pair(lib, data, oracle_data=None, **kw):
    """oracle_data: the matrix of the subset, taken outside the oracle -- it then gets that matrix and no subsetIndices / subsetDim.
    sampler ("async" / "sequential") goes to both sides as it is."""
    S = _capi.Session(data, lib=lib, **kw)
    wA = lib.cogaps_reduction_width(S.dims("A")[1])
    wP = lib.cogaps_reduction_width(S.dims("P")[1])
    okw = dict(kw)
    okw.pop("device", None)
    if oracle_data is not None:
        data = oracle_data
        okw.pop("subsetIndices", None), okw.pop("subsetDim", None)
    if okw.pop("reductionMode", "lanes") == "seq":
        # verification mode: the reference's own order (one accumulator) and the session's math mode
        math = {"portable": po.MATH_PORTABLE, "glibc-fma": po.MATH_GLIBC_FMA, "glibc-sse2": po.MATH_GLIBC_SSE2}[okw.pop("mathMode", "portable")]
        O = po.Session(data, math_mode=math, redW_A=1, redW_P=1, redG=1, **okw)
    else:
        O = po.Session(data, math_mode=po.MATH_PORTABLE, redW_A=wA, redW_P=wP, redG=4, **okw)
    return S, O


def assert_trace_equal(a, b, tag):
    assert np.array_equal(a["nproc"], b["nproc"]), tag + ": batch sizes (nProcessed) differ"
    assert np.array_equal(a["qlen"], b["qlen"]), tag + ": queue lengths differ"
    assert len(a["rec"]) == len(b["rec"]), tag + ": number of queued proposals differs"
    ra, rb = a["rec"], b["rec"]
    for f in ("type", "r1", "c1", "r2", "c2", "rng_state", "atom1", "batch"):
        assert np.array_equal(ra[f], rb[f]), "%s: field %s differs first at %d" % (tag, f, int(np.nonzero(ra[f] != rb[f])[0][0]))
    m = ra["type"] == ord("M")
    assert np.array_equal(ra["pos"][m], rb["pos"][m]), tag + ": move destinations differ"
    e = ra["type"] == ord("E")
    assert np.array_equal(ra["atom2"][e], rb["atom2"][e]), tag + ": exchange partners differ"


def assert_state_equal(S, O, tag, chisq=True, ap=True):
    """ap=False: no A*P comparison -- for sparse-model sessions only, which keep no A*P cache (at configs[4]'s shard shape the getter
    would hand back 2 x 2.5 GB of zeros)"""
    for w in "AP":
        a, b = S.atoms(w), O.atoms(w)
        for f in ("pos", "mass", "left", "right"):
            assert np.array_equal(a[f], b[f]), "%s %s: atom %s differs" % (tag, w, f)
        assert np.array_equal(S.matrix(w), O.matrix(w)), "%s %s: factor matrix differs" % (tag, w)
        assert np.array_equal(S.rows(w), O.rows(w)), "%s %s: factor matrix (HybridMatrix row copy) differs" % (tag, w)
        if ap:
            assert np.array_equal(S.ap(w), O.ap(w)), "%s %s: AP cache differs" % (tag, w)
        assert S.avg_queue(w) == O.avg_queue(w), "%s %s: average queue length differs" % (tag, w)
        assert S.check_domain(w) == 0, "%s %s: the atomic domain's cached neighbour positions / masses or links are inconsistent" % (tag, w)
        if chisq:
            assert S.chisq(w) == O.chisq(w), "%s %s: chi2 differs" % (tag, w)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_seq_state_equal(S, O, tag):
    """the sequential sampler's form of assert_state_equal, bit for bit (a float as its 32 bits): both samplers' atoms in the order of
    AtomicDomain's vector (position, mass, neighbours by index), factor matrix, A*P cache and chi2; the library's domain consistent;
    no queue on either side; the oracle never drew a position past the last bin"""
    assert not O.seq_error(), tag + ": the oracle drew a position past the last bin"
    for w in "AP":
        a, b = S.atoms(w), O.atoms(w)
        assert a["pos"].size == b["pos"].size, "%s %s: %d atoms, the oracle has %d" % (tag, w, a["pos"].size, b["pos"].size)
        for f in ("pos", "mass", "left", "right"):
            assert np.array_equal(_bits(a[f]), _bits(b[f])), "%s %s: atom %s differs" % (tag, w, f)
        assert np.array_equal(_bits(S.matrix(w)), _bits(O.matrix(w))), "%s %s: factor matrix differs" % (tag, w)
        assert np.array_equal(_bits(S.ap(w)), _bits(O.ap(w))), "%s %s: AP cache differs" % (tag, w)
        assert S.check_domain(w) == 0, "%s %s: the atomic domain's cached neighbour positions / masses or links are inconsistent" % (tag, w)
        assert np.float32(S.chisq(w)).tobytes() == np.float32(O.chisq(w)).tobytes(), "%s %s: chi2 differs: %r, the oracle has %r" % (tag, w, S.chisq(w), O.chisq(w))
        assert S.avg_queue(w) == 0.0 and O.avg_queue(w) == 0.0, "%s %s: a sequential sampler has no queue" % (tag, w)


def run_stepwise_seq(lib, data, n_iter, total_iter=None, check_every=1, **kw):
    """n_iter equilibration iterations of a sequential-sampler session of `lib` and of the oracle's, side by side: the Poisson step
    counts of every update and the state after every check_every-th iteration (and the last).  -> the oracle's counts of the proposals
    that evaluated alpha parameters per sampler (pyoracle.Session.seq_counts), the atoms per sampler, and the largest update's steps"""
    total_iter = total_iter or max(n_iter, 2)
    kw.setdefault("nIterations", total_iter)
    S, O = make_pair(lib, data, sampler="sequential", **kw)
    try:
        longest = 0
        for it in range(n_iter):
            t = min(1.0, 2.0 * it / total_iter)
            S.set_annealing(t), O.set_annealing(t)
            nA, nP = S.draw_steps()
            assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
            longest = max(longest, nA, nP)
            S.iterate(nA, nP), O.iterate(nA, nP)
            if (it + 1) % check_every == 0 or it == n_iter - 1:
                assert_seq_state_equal(S, O, "it%d" % it)
        return {"counts": {w: O.seq_counts(w) for w in "AP"}, "atoms": {w: S.natoms(w) for w in "AP"}, "longest": longest}
    finally:
        S.close(), O.close()


STRUCT_FIELDS = ("flags", "prefix", "ptr", "vals")


def structures(S):
    """the sparse model's data of both samplers as the session holds it (cogaps_session_debug_sparse_data)"""
    return {w: S.debug_sparse_data(w) for w in "AP"}


def assert_structures_equal(a, b, tag=""):
    for w in "AP":
        for f in STRUCT_FIELDS:
            assert a[w][f].dtype == b[w][f].dtype and a[w][f].shape == b[w][f].shape and np.array_equal(a[w][f], b[w][f]), "%s %s %s differs" % (tag, w, f)
        for f in ("lambda", "maxGibbsMass"):      # (as bits: an empty matrix has lambda = NaN in both)
            assert np.float32(a[w][f]).tobytes() == np.float32(b[w][f]).tobytes(), "%s %s %s differs" % (tag, w, f)


def packed_reference(data, nPatterns, transposeData=False):
    """What structures() must return for a sparse-model session of the dense matrix `data`, from the definition of the four arrays
    (csrc/sparse_build.h's header) in numpy and independent of the library.  Sampler A's data vectors are the genes (elements:
    samples), sampler P's the samples; genes are the rows of `data` unless transposeData.  Per sampler, over vectors j = 0 .. M-1 of
    N elements, with Wn = N // 64 + 1 flag words per vector:
      flags[j][w]  bit b set: element 64 w + b of vector j is > 0 (NaN, zero and negative entries are absent)
      prefix[j][w] number of entries > 0 of vector j below element 64 w
      ptr[j]       number of entries > 0 of the vectors before j; ptr[M] their total
      vals         the entries > 0, vector by vector, ascending element index
    lambda and maxGibbsMass are the oracle's (default alpha and maxGibbsMass)."""
    data = np.asarray(data, dtype=np.float32)
    genes_by_samples = data.T if transposeData else data
    O = po.Session(data, nPatterns=nPatterns, seed=1, sparseOptimization=True, transposeData=transposeData)
    out = {}
    for w, mat in (("A", genes_by_samples), ("P", genes_by_samples.T)):
        M, N = mat.shape
        Wn = N // 64 + 1
        kept = np.zeros((M, Wn * 64), dtype=bool)
        kept[:, :N] = mat > 0
        flags = np.ascontiguousarray(np.packbits(kept, axis=1, bitorder="little")).view("<u8").astype(np.uint64)
        per_word = kept.reshape(M, Wn, 64).sum(axis=2, dtype=np.uint32)
        prefix = (np.cumsum(per_word, axis=1, dtype=np.uint32) - per_word).astype(np.uint32)
        ptr = np.concatenate([[0], np.cumsum(per_word.sum(axis=1, dtype=np.uint64))]).astype(np.uint32)
        out[w] = {"flags": flags, "prefix": prefix, "ptr": ptr, "vals": np.ascontiguousarray(mat)[kept[:, :N]],
                  "lambda": O.lam(w), "maxGibbsMass": O.max_gibbs_mass(w)}
    O.close()
    return out


def seq_sum(x):
    """one fp32 accumulator, left to right"""
    return np.cumsum(np.ascontiguousarray(x, dtype=np.float32).ravel(), dtype=np.float32)[-1]


def lam(total, nnz, k, alpha=0.01):
    return np.float32(alpha) * np.sqrt(np.float32(k) / (np.float32(total) / np.float32(nnz)))


def dense_reference(data, unc, nPatterns, transposeData=False, subsetIndices=None, subsetDim=0):
    """What Session.debug_dense_data() must return for a dense-model session of `data` (and the uncertainty `unc`, or None: the default
    max(0.1 v, 0.1)), in numpy and independent of the library.  Genes are the rows of `data` unless transposeData; subsetIndices are
    1-based indices of the genes (subsetDim 1) or the samples (2), applied in the order given, repeats included (Matrix.cpp:30-69).
    Sampler A's data vectors are the genes (elements: samples), sampler P's the samples.  Per sampler, over vectors j = 0 .. M-1 of N
    elements in rows of Npad = N rounded up to 4:
      D, Sraw, S2  [M][Npad]: the value, its uncertainty sd and sd * sd in fp32; the pads hold D = 0, Sraw = S2 = 1; S2 is None with
                   the default uncertainty (the session keeps no such array)
      lambda       alpha * sqrt(K / (sum / nnz)): sum = ONE fp32 accumulator over the elements in (j, i) order -- every value, a
                   negative one too -- and nnz = the entries > 0 (gaps::nonZeroMean, MatrixMath.cpp:39-55)
      maxGibbsMass 100 / lambda;  sparsity  1 - nnz / (M * N), all in fp32 (default alpha and maxGibbsMass)
    lambda and maxGibbsMass are checked here against the oracle's, which is given the cut matrix and no subset."""
    f32 = np.float32
    genes = np.asarray(data, dtype=f32).T if transposeData else np.asarray(data, dtype=f32)
    sd = None if unc is None else (np.asarray(unc, dtype=f32).T if transposeData else np.asarray(unc, dtype=f32))
    if subsetIndices is not None and subsetDim:
        idx = np.asarray(subsetIndices, dtype=np.int64) - 1
        genes = genes[idx] if subsetDim == 1 else genes[:, idx]
        if sd is not None:
            sd = sd[idx] if subsetDim == 1 else sd[:, idx]
    cut = (lambda x: None if x is None else np.ascontiguousarray(x.T if transposeData else x))
    O = po.Session(cut(genes), unc=cut(sd), nPatterns=nPatterns, seed=1, transposeData=transposeData)
    out = {}
    for w, mat, s in (("A", genes, sd), ("P", genes.T, None if sd is None else sd.T)):
        M, N = mat.shape
        D, Sraw = np.zeros((M, (N + 3) & ~3), dtype=f32), np.ones((M, (N + 3) & ~3), dtype=f32)
        D[:, :N] = mat
        Sraw[:, :N] = np.maximum(mat * f32(0.1), f32(0.1)) if s is None else s
        nnz = int((mat > 0).sum())
        lm = lam(seq_sum(mat), nnz, nPatterns)
        out[w] = {"D": D, "Sraw": Sraw, "S2": None if s is None else Sraw * Sraw, "lambda": lm, "maxGibbsMass": f32(100) / lm,
                  "sparsity": f32(1) - f32(nnz) / f32(M * N)}
        for f, o in (("lambda", O.lam(w)), ("maxGibbsMass", O.max_gibbs_mass(w))):
            assert f32(out[w][f]).tobytes() == f32(o).tobytes(), "dense_reference %s %s: %r, the oracle has %r" % (w, f, out[w][f], o)
    O.close()
    return out


def run_stepwise(lib, data, n_iter, trace=True, total_iter=None, check_every=1, **kw):
    total_iter = total_iter or max(n_iter, 2)
    kw.setdefault("nIterations", total_iter)
    S, O = make_pair(lib, data, **kw)
    fixed = kw.get("whichMatrixFixed", "N")
    props = 0
    for it in range(n_iter):
        t = min(1.0, 2.0 * it / total_iter)
        S.set_annealing(t), O.set_annealing(t)
        nA, nP = S.draw_steps()
        assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
        props += nA + nP
        if trace and fixed == "N":
            assert_trace_equal(S.update("A", nA, 1 << 16), O.update("A", nA, 1 << 16), "it%d A" % it)
            S.sync("P"), O.sync("P")
            assert_trace_equal(S.update("P", nP, 1 << 16), O.update("P", nP, 1 << 16), "it%d P" % it)
            S.sync("A"), O.sync("A")
        else:
            S.iterate(nA, nP), O.iterate(nA, nP)
        if (it + 1) % check_every == 0 or it == n_iter - 1:
            assert_state_equal(S, O, "it%d" % it)
    out = (S.natoms("A"), S.natoms("P"), props)
    S.close(), O.close()
    return out


def configs4_shard():
    """BASELINE configs[4]'s per-GPU shard as `bench.py --sparse --genes 50000 --samples 12500` builds it for rank 0 (bench.py's recipe,
    written out): bench.synthetic_dense(50000, 12500) with 95 % of the entries zeroed i.i.d. by MT19937(777)"""
    import bench
    data = bench.synthetic_dense(50000, 12500)
    data *= (np.random.Generator(np.random.MT19937(777)).random(data.shape) >= 0.95)
    return data


def sparse_chisq_f64(data, A, P, block=500):
    """chi2 of the whole matrix in float64, column block by column block, with the sparse model's uncertainty (0.1 on zeros, 0.1 d
    elsewhere; SparseNormalModel): an evaluation that goes through neither float32 implementation.  A: genes x K, P: samples x K."""
    a = A.astype(np.float64)
    full = 0.0
    for c0 in range(0, data.shape[1], block):
        d = data[:, c0:c0 + block].astype(np.float64)
        full += (((d - a @ P[c0:c0 + block].astype(np.float64).T) / np.where(d > 0, 0.1 * d, 0.1)) ** 2).sum()
    return full


def synthetic(genes, samples, rank=3, seed=7):
    rng = np.random.default_rng(seed)
    a0 = rng.gamma(2.0, 0.5, (genes, rank)) * (rng.random((genes, rank)) > 0.5)
    p0 = rng.gamma(2.0, 0.5, (samples, rank)) * (rng.random((samples, rank)) > 0.3)
    return ((a0 @ p0.T) * (0.9 + 0.2 * rng.random((genes, samples))) + 0.01).astype(np.float32)


def synthetic_counts(genes, samples, zeros=0.85, rank=4, seed=7):
    """count-like data (positive entries >= 1, `zeros` of the entries 0): the regime the sparse model's fixed
    uncertainty (0.1 on zeros, 0.1*d elsewhere) coincides with the default max(0.1*d, 0.1)"""
    rng = np.random.default_rng(seed)
    a0 = rng.gamma(2.0, 0.5, (genes, rank)) * (rng.random((genes, rank)) > 0.5)
    p0 = rng.gamma(2.0, 0.5, (samples, rank)) * (rng.random((samples, rank)) > 0.4)
    d = np.ceil((a0 @ p0.T) * (0.9 + 0.2 * rng.random((genes, samples)))) * (rng.random((genes, samples)) > zeros)
    return d.astype(np.float32)


def option_cases():
    """combinations of the run options cogaps_cpp forwards (Cogaps.cpp:64-139): transposed input, a subset in either dimension, a fixed
    factor, an uncertainty matrix, the sparse model, nPatterns from 1 up"""
    cases, i = [], 0
    for sparse in (False, True):
        for transpose in (False, True):
            for fixed in ("N", "A", "P"):
                for subset in (0, 1, 2):
                    i += 1
                    cases.append((sparse, transpose, fixed, subset, 1 + (i % 6), bool(i % 2) and not sparse))
    return cases


def run_option_case(lib, sparse, transpose, fixed, subset, k, with_unc):
    genes, samples = 83, 37
    base = synthetic_counts(genes, samples, zeros=0.6, seed=5 + k) if sparse else synthetic(genes, samples, seed=5 + k)
    data = np.ascontiguousarray(base.T) if transpose else base          # transposeData: the file holds samples x genes
    kw = dict(nPatterns=k, seed=100 + k, total_iter=40, check_every=5, transposeData=transpose, sparseOptimization=sparse)
    n_genes, n_samples = genes, samples
    if subset == 1:
        kw.update(subsetIndices=np.arange(3, 3 + 50, dtype=np.uint32), subsetDim=1); n_genes = 50
    elif subset == 2:
        kw.update(subsetIndices=np.arange(2, 2 + 20, dtype=np.uint32), subsetDim=2); n_samples = 20
    if fixed != "N":
        rows = n_genes if fixed == "A" else n_samples
        kw.update(whichMatrixFixed=fixed, fixedPatterns=np.abs(np.random.default_rng(k).normal(size=(rows, k))).astype(np.float32))
    if with_unc:
        kw.update(unc=np.maximum(data * np.float32(0.2), np.float32(0.3)).astype(np.float32))
    run_stepwise(lib, data, 40, trace=(fixed == "N"), **kw)
