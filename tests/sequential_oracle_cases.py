"""The cases in which the sequential sampler's PRODUCT arithmetic (reductionMode "lanes", portable logf / expf: csrc/seq_kernel.h's
seq_alpha_lanes) is compared step by step with the oracle's sequential sampler (oracle/gaps_oracle.c), shared by
tests/test_sequential_oracle.py (the emulator build) and tests/test_sequential_oracle_gpu.py (the HIP library).

The oracle's sequential sampler is pinned to the reference build's recorded runs by test_sequential_oracle.py itself, with one
accumulator per sum and glibc's logf / expf; here it runs in the lane order of the reduction contract (W virtual lanes, float4
chunk j to lane j mod W, ascending xor butterfly), which it shares with the asynchronous sampler's pinned comparisons."""
import numpy as np

import parity_util as pu

# ---- every reduction class ----------------------------------------------------------------------------------------------------------
# The P sampler's data vectors have `genes` elements: W = cogaps_reduction_width(genes) virtual lanes on min(W, 1024) threads, V = W / 1024
# of them per thread above that.  4097: the last float4 chunk is partial; 70001: more than one chunk per virtual lane, and a tail.
# (name, genes, samples, nPatterns, seed, iterations, W, V).  The seeds are chosen with the oracle alone, so that within the iterations
# the P sampler makes every kind of proposal that needs a reduction (test_sequential_oracle.py asserts it from the oracle's counts).
SHAPES = [
    ("200x7", 200, 7, 3, 1, 12, 64, 1),
    ("300x7", 300, 7, 3, 1, 12, 128, 1),
    ("gist_1363x9", 1363, 9, 4, 1, 8, 512, 1),
    ("4097x6", 4097, 6, 3, 1, 6, 2048, 2),
    ("8200x6", 8200, 6, 3, 1, 6, 4096, 4),
    ("16400x6", 16400, 6, 2, 1, 4, 8192, 8),
    ("33000x6", 33000, 6, 2, 1, 3, 16384, 16),
    ("70001x5", 70001, 5, 2, 1, 3, 16384, 16),
]
SHAPE_IDS = [s[0] for s in SHAPES]
KINDS = ("birth", "death", "move", "exchange", "twoRow")


def shape_data(name, genes, samples, gist=None):
    return gist if name.startswith("gist") else pu.synthetic(genes, samples, seed=genes % 97)


def check_shape(lib, gist, case):
    """one SHAPES entry, `lib` against the oracle after every iteration; what the chain must have done is asserted from the oracle's counts"""
    name, genes, samples, k, seed, iters, W, V = case
    data = shape_data(name, genes, samples, gist)
    assert data.shape == (genes, samples)
    assert lib.cogaps_reduction_width(genes) == W and W // min(W, 1024) == V, (lib.cogaps_reduction_width(genes), W, V)
    out = pu.run_stepwise_seq(lib, data, iters, nPatterns=k, seed=seed)
    assert out["atoms"]["A"] > 0 and out["atoms"]["P"] > 0, out
    for kind in KINDS:      # (the P sampler is the one whose reductions have the width W)
        assert out["counts"]["P"][kind] >= 1, "no %s proposal evaluated by the P sampler: %r" % (kind, out["counts"])
    return out


# ---- the options in the sampler's scope ---------------------------------------------------------------------------------------------
OPTIONS = ("uncertainty", "transpose", "subset_genes", "subset_samples", "fixedA", "fixedP")
# (tag, genes, samples, nPatterns, iterations, arithmetic): one narrow and one V = 2 shape in lane order; the narrow one once more in
# the verification mode, against the oracle with one accumulator per sum (redW = 1) and glibc's logf / expf
OPTION_SHAPES = [
    ("narrow_lanes", 200, 7, 3, 14, {}),
    ("v2_lanes", 4097, 6, 3, 6, {}),
    ("narrow_seq", 200, 7, 3, 14, dict(reductionMode="seq", mathMode="glibc-fma")),
]
OPTION_CASES = [(o, s[0]) for o in OPTIONS for s in OPTION_SHAPES]
OPTION_IDS = ["%s-%s" % c for c in OPTION_CASES]


def option_case(option, shape):
    """-> (data, keyword arguments of parity_util.run_stepwise_seq, the samplers that run)"""
    _, genes, samples, k, iters, arith = next(s for s in OPTION_SHAPES if s[0] == shape)
    rng = np.random.default_rng(genes + len(option))
    kw = dict(nPatterns=k, seed=3 + len(option), n_iter=iters, **arith)
    run = "AP"
    g, s = genes, samples
    if option == "subset_genes":
        g = genes + 150
    elif option == "subset_samples":
        s = samples + 4
    data = pu.synthetic(g, s, seed=11)
    if option == "uncertainty":      # an uncertainty matrix of the user's: the kernel reads S2 instead of recomputing the default one
        kw.update(unc=(np.float32(0.15) * data + np.float32(0.2) + rng.random(data.shape, dtype=np.float32) * np.float32(0.1)).astype(np.float32))
    elif option == "transpose":      # the matrix arrives as samples x genes
        data = np.ascontiguousarray(data.T)
        kw.update(transposeData=True)
    elif option == "subset_genes":   # 1-based, not ascending: the subset's order is the caller's (Matrix.cpp:55-62)
        kw.update(subsetIndices=(rng.permutation(g)[:genes] + 1).astype(np.uint32), subsetDim=1)
    elif option == "subset_samples":
        kw.update(subsetIndices=(rng.permutation(s)[:samples] + 1).astype(np.uint32), subsetDim=2)
    elif option in ("fixedA", "fixedP"):
        rows = genes if option == "fixedA" else samples
        kw.update(whichMatrixFixed=option[-1], fixedPatterns=(rng.gamma(2.0, 0.5, (rows, k)) * (rng.random((rows, k)) > 0.3)).astype(np.float32))
        run = "P" if option == "fixedA" else "A"
    if "subsetIndices" in kw:
        assert (np.diff(kw["subsetIndices"].astype(np.int64)) < 0).any()
    return data, kw, run


def check_option(lib, option, shape):
    data, kw, run = option_case(option, shape)
    out = pu.run_stepwise_seq(lib, data, kw.pop("n_iter"), **kw)
    for w in run:
        assert out["atoms"][w] > 0, (w, out)
    for kind in KINDS[:4]:
        assert sum(out["counts"][w][kind] for w in run) >= 1, "no %s proposal evaluated: %r" % (kind, out["counts"])
    return out


# ---- a batch ------------------------------------------------------------------------------------------------------------------------
BATCH_SHAPE = (4097, 6)          # V = 2
BATCH_CHAINS = [dict(nPatterns=3, seed=21), dict(nPatterns=3, seed=22), dict(nPatterns=4, seed=23)]
BATCH_ITERS = 5


def check_batch(lib):
    """three chains of one reduction width stepped by one launch per update (seq_update_kernel_multi), each against an oracle session
    of its own: the updates' step counts (as their sum per chain) and the state after the equilibration iterations"""
    from cogaps_amd import _capi
    data = pu.synthetic(*BATCH_SHAPE, seed=31)
    pairs = [pu.make_pair(lib, data, sampler="sequential", nIterations=BATCH_ITERS, **kw) for kw in BATCH_CHAINS]
    b = None
    try:
        b = _capi.Batch([S for S, _ in pairs])
        updates = b.run_iterations(1, 0, BATCH_ITERS)
        for c, (S, O) in enumerate(pairs):
            nA, nP = O.run_iterations(1, 0, BATCH_ITERS)
            assert updates[c] == int(nA.sum()) + int(nP.sum()), (c, updates[c], nA, nP)
            pu.assert_seq_state_equal(S, O, "chain %d" % c)
            assert S.natoms("A") > 0 and S.natoms("P") > 0
            assert sum(O.seq_counts("P").values()) > 0
    finally:
        if b is not None:
            b.close()
        for S, O in pairs:
            S.close(), O.close()


# ---- more than SEQ_STEPS_PER_LAUNCH = 4096 steps in one update ----------------------------------------------------------------------------
# An update's step count is Poisson(number of atoms), so a sampler needs more than 4096 atoms: the A sampler's, whose domain has
# genes x nPatterns bins.  Found with the oracle alone (seed 2, pu.synthetic(genes, 6, rank 4, seed 41); genes 3000 .. 20000, nPatterns
# 4 .. 10, nIterations 6 .. 30): the fewer iterations a run has the faster it heats up and the faster the atoms grow, so the cheapest
# complete runs that cross 4096 are short ones -- 8000 x 6, nPatterns 8, nIterations 16 takes 45908 steps in all, and two A updates of
# its sampling phase exceed 4096 (the largest: 4221 steps, two launches).  With 5000 genes the cheapest is nIterations 20 (61811 steps,
# one update of 4212); with 3000 genes only nPatterns 10 with nIterations 30 gets there (128426 steps).
LONG = dict(genes=8000, samples=6, nPatterns=8, seed=2, nIterations=16)
STEPS_PER_LAUNCH = 4096


def long_data():
    return pu.synthetic(LONG["genes"], LONG["samples"], rank=4, seed=41)


def long_kw():
    return dict(nPatterns=LONG["nPatterns"], seed=LONG["seed"], nIterations=LONG["nIterations"], outputFrequency=4)


RESULT_KEYS = ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP", "totalUpdates", "meanChiSq", "averageQueueLengthA", "averageQueueLengthP")


_long_oracle = {}


def long_oracle(lib):
    """the oracle's side of the configuration, once per process: the steps of every update of both phases, the end state, the result"""
    if not _long_oracle:
        import pyoracle as po
        n = LONG["nIterations"]
        wA, wP = lib.cogaps_reduction_width(LONG["samples"]), lib.cogaps_reduction_width(LONG["genes"])
        O = po.Session(long_data(), sampler="sequential", math_mode=po.MATH_PORTABLE, redW_A=wA, redW_P=wP, redG=4, **long_kw())
        steps = np.concatenate([np.concatenate(O.run_iterations(ph, 0, n)) for ph in (1, 2)])
        _long_oracle.update(O=O, steps=steps, result=O.finish())
    assert int(_long_oracle["steps"].max()) > STEPS_PER_LAUNCH, "no update of more than %d steps: the largest has %d" % (STEPS_PER_LAUNCH, int(_long_oracle["steps"].max()))
    return _long_oracle


def assert_results_equal(r, o):
    for k in RESULT_KEYS:
        a, b = np.asarray(r[k]), np.asarray(o[k])
        if a.dtype.kind == "f":
            a, b = a.astype(np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32)
        assert np.array_equal(a, b), "result field %s differs" % k


def check_long_state(lib):
    """both phases on a session of `lib`: the oracle's step counts show an update of more than one launch (asserted in long_oracle); the
    number of steps made, the end state and the finished result are the oracle's"""
    from cogaps_amd import _capi
    ref, n = long_oracle(lib), LONG["nIterations"]
    S = _capi.Session(long_data(), lib=lib, sampler="sequential", **long_kw())
    try:
        assert S.run_iterations(1, 0, n) + S.run_iterations(2, 0, n) == int(ref["steps"].sum())
        pu.assert_seq_state_equal(S, ref["O"], "end of the run")
        assert_results_equal(S.finish(), ref["result"])
    finally:
        S.close()


def check_long_run(lib):
    """cogaps_run of the same configuration: the oracle's result"""
    from cogaps_amd import _capi
    ref = long_oracle(lib)
    r = _capi.run(long_data(), lib=lib, sampler="sequential", **long_kw())
    assert r["totalUpdates"] == int(ref["steps"].sum())
    assert_results_equal(r, ref["result"])
