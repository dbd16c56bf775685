"""The gene sets of every pattern (getPatternGeneSet; csrc/gsea_kernel.h) on the emulator: the kernel's ranks, scores and
permutation sums against the numpy restatement of tests/pattern_gene_set_cases.py, bit for bit; an exact answer; the front end of both
methods on a CogapsResult built from a raw dict; the C entry's refusals."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import pattern_gene_set_cases as pc
from cogaps_amd import CogapsResult, _capi, getPatternGeneSet


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


# ---- 1. ranks ----
@pytest.mark.parametrize("n,K,zero", pc.RANK_SHAPES)
def test_ranks_are_the_stable_argsort(lib, n, K, zero):
    pc.check_ranks(lib, n, K, zero)


# ---- 2. scores, bit for bit ----
@pytest.mark.parametrize("numPerm", pc.PERM_CASES)
@pytest.mark.parametrize("K", pc.K_CASES)
def test_scores_bit_for_bit(lib, K, numPerm):
    pc.check_scores(lib, pc.stat_random()[:, :K], numPerm, pc.expected("random", numPerm))


def test_column_major_stat_through_the_strides(lib):
    stat = np.asfortranarray(pc.stat_random()[:, :3])
    assert stat.strides == (4, 4 * pc.N_ROWS)
    pc.check_scores(lib, stat, 7, pc.expected("random", 7))


def test_members_that_are_all_zero_in_a_column(lib):
    assert not pc.stat_zero_members()[pc.score_sets()[2], 1].any()            # NR == 0: the hits rise by 1 / m
    got = pc.check_scores(lib, pc.stat_zero_members(), 7, pc.expected("zero", 7))
    assert 0.0 < got["es"][2, 1] <= 1.0


def test_integer_stat_exercises_greater_or_equal(lib):
    assert pc.integer_equalities() > 0                                        # with > in place of >= some count would differ
    pc.check_scores(lib, pc.stat_integer(), 130, pc.expected("integer", 130))


def test_scores_do_not_depend_on_the_grid_or_on_the_chunks_of_sets(lib, monkeypatch):
    """a device of two compute units loops over the trips; seven sets per chunk of the host: a set keeps its index in the draw's key"""
    monkeypatch.setenv("COGAPS_TEST_COMPUTE_UNITS", "2")
    pc.check_scores(lib, pc.stat_random()[:, :3], 40, pc.expected("random", 40))
    monkeypatch.setenv("COGAPS_TEST_GSEA_CHUNK_SETS", "7")
    pc.check_scores(lib, pc.stat_random()[:, :3], 40, pc.expected("random", 40))


# ---- 3. the size classes of the sort ----
def test_sets_up_to_the_cap(lib):
    pc.check_big(lib)


def test_a_set_above_the_cap(lib):
    stat = pc.gamma_loadings(pc.BIG_ROWS, 2, 9)
    with pytest.raises(_capi.CogapsError, match="4097 members are more than GSEA_MAX_SET = 4096"):
        _capi.pattern_gsea(stat, [np.arange(4097, dtype=np.uint32)], 2, lib=lib)
    res = CogapsResult({"Amean": stat, "Asd": np.ones_like(stat), "Pmean": np.ones((3, 2), np.float32), "Psd": np.ones((3, 2), np.float32), "seed": 1})
    out = res.getPatternGeneSet([list(range(1, 4098)), [5, 9, 11]], numPerm=3, lib=lib)
    assert list(out["size"]) == [4097, 3]
    for key in ("ES", "NES", "pval", "padj", "negLogPadj", "nMoreExtreme"):
        assert np.isnan(out[key][:, 0]).all() and not np.isnan(out[key][:, 1]).any(), key
    assert out["leadingEdge"][0][0] == []
    want = pc.gsea(stat, [np.array([4, 8, 10])], 3, 1)                        # the one set that is tested has index 0 in the draw's key
    assert np.array_equal(out["ES"][:, 1], want["es"][0])
    with pytest.raises(ValueError, match="4096"):
        res.getPatternGeneSet([[5, 9, 11]], maxSize=4097, lib=lib)


# ---- 5. an exact answer ----
def test_planted_sets(lib):
    pc.check_planted(lib)
    pc.check_planted(lib, seed=123456)


# ---- 6. front end ----
SETS = {"alpha": ["g3", "g10", "g11", "g50"], "beta": ["g1", "nobody", "g2", "g2"], "gamma": ["unknown", "neither"], "delta": ["g7"],
        "epsilon": ["g%d" % i for i in range(20, 50)]}
MEMBERS = [[3, 10, 11, 50], [1, 2], [], [7], list(range(20, 50))]


def test_enrichment_shapes_formulas_and_names(lib):
    res, raw = pc.raw_result_with_names()
    n, K = raw["Amean"].shape
    numPerm = 50
    out = res.getPatternGeneSet(SETS, numPerm=numPerm, lib=lib)
    assert out["sets"] == list(SETS) and out["method"] == "enrichment" and list(out["size"]) == [4, 2, 0, 1, 30]
    tested = [0, 1, 3, 4]                                                     # gamma matched no row: not tested
    dev = pc.gsea(raw["Amean"], [np.array(MEMBERS[t]) for t in tested], numPerm, raw["seed"])      # seed: the result's
    for key in ("ES", "NES", "pval", "padj", "negLogPadj", "nMoreExtreme"):
        assert out[key].shape == (K, 5) and np.isnan(out[key][:, 2]).all(), key
    assert np.array_equal(out["ES"][:, tested], dev["es"].T) and np.array_equal(out["nMoreExtreme"][:, tested], dev["nGe"].T)
    assert np.array_equal(out["pval"][:, tested], (dev["nGe"].T + 1.0) / (numPerm + 1.0))
    assert (dev["permSum"] > 0).all()
    assert np.array_equal(out["NES"][:, tested], dev["es"].T / (dev["permSum"].T.astype(np.float64) / 2 ** 40 / numPerm))
    for k in range(K):                                                        # BH per pattern over the four tested sets
        assert np.array_equal(out["padj"][k], pc.bh(out["pval"][k]), equal_nan=True)
        assert np.array_equal(out["negLogPadj"][k], -10 * np.log10(pc.bh(out["pval"][k])), equal_nan=True)
    assert (out["padj"][:, tested] >= out["pval"][:, tested]).all()
    # the leading edge: the members up to the peak, in rank order
    _, rank = pc.ranks(raw["Amean"])
    for k in range(K):
        for j, t in enumerate(tested):
            mem = np.array(MEMBERS[t])
            want = mem[np.argsort(rank[k][mem])][:dev["peak"][j, k] + 1]
            assert out["leadingEdge"][k][t] == ["g%d" % i for i in want]
        assert out["leadingEdge"][k][2] == []
    # the module-level form, another seed, indices, a result without names, the other matrix
    assert np.array_equal(getPatternGeneSet(res, SETS, "enrichment", numPerm=numPerm, lib=lib)["pval"], out["pval"], equal_nan=True)
    other = res.getPatternGeneSet(SETS, numPerm=numPerm, seed=raw["seed"] + 1, lib=lib)
    assert np.array_equal(other["ES"], out["ES"], equal_nan=True) and not np.array_equal(other["nMoreExtreme"], out["nMoreExtreme"], equal_nan=True)
    bare, _ = pc.raw_result_with_names(names=False)
    byIndex = bare.getPatternGeneSet([[4, 11, 12, 51], [2, 3, 3]], numPerm=numPerm, lib=lib)
    assert byIndex["sets"] == ["1", "2"] and np.array_equal(byIndex["pval"], out["pval"][:, :2])
    assert byIndex["leadingEdge"][0][0] == [int(g[1:]) + 1 for g in out["leadingEdge"][0][0]]
    samples = res.getPatternGeneSet({"a": ["s1", "s4"], "b": ["s0", "s2", "s8"]}, whichMatrix="sampleFactors", numPerm=20, lib=lib)
    want = pc.gsea(raw["Pmean"], [np.array([1, 4]), np.array([0, 2, 8])], 20, raw["seed"])
    assert np.array_equal(samples["ES"], want["es"].T) and np.array_equal(samples["nMoreExtreme"], want["nGe"].T)


def test_size_limits_leave_nan_rows_out_of_the_adjustment(lib):
    res, raw = pc.raw_result_with_names()
    out = res.getPatternGeneSet(SETS, numPerm=30, minSize=2, maxSize=4, lib=lib)
    assert list(out["size"]) == [4, 2, 0, 1, 30]
    assert np.isnan(out["pval"][:, [2, 3, 4]]).all() and not np.isnan(out["pval"][:, [0, 1]]).any()
    dev = pc.gsea(raw["Amean"], [np.array(MEMBERS[0]), np.array(MEMBERS[1])], 30, raw["seed"])
    p = (dev["nGe"].T + 1.0) / 31.0
    assert np.array_equal(out["pval"][:, :2], p)
    for k in range(p.shape[0]):                                               # two sets count, not five
        lo, hi = sorted(p[k])
        assert sorted(out["padj"][k, :2]) == [min(2 * lo, hi), hi]
    whole = res.getPatternGeneSet({"all": ["g%d" % i for i in range(raw["Amean"].shape[0])], "a": ["g1", "g2"]}, numPerm=5, lib=lib)
    assert np.isnan(whole["ES"][:, 0]).all() and not np.isnan(whole["ES"][:, 1]).any()      # a set of every row is not tested


def test_front_end_errors(lib):
    res, raw = pc.raw_result_with_names()
    ok = {"a": ["g1", "g2"]}
    with pytest.raises(ValueError, match="method must be"):
        res.getPatternGeneSet(ok, method="gsea", lib=lib)
    with pytest.raises(ValueError, match="above the 4096 members"):
        res.getPatternGeneSet(ok, maxSize=5000, lib=lib)
    with pytest.raises(ValueError, match="whichMatrix"):
        res.getPatternGeneSet(ok, whichMatrix="A", lib=lib)
    for bad in (0, -3, 2.5, None):
        with pytest.raises(ValueError, match="numPerm"):
            res.getPatternGeneSet(ok, numPerm=bad, lib=lib)
    with pytest.raises(ValueError, match="all index sets or all name sets"):
        res.getPatternGeneSet({"a": ["g1", 2]}, lib=lib)
    for value in (np.nan, -1.0):
        broken = dict(raw, Amean=raw["Amean"].copy())
        broken["Amean"][7, 1] = value
        with pytest.raises(ValueError, match="NaN or a negative value"):
            CogapsResult(broken, geneNames=res.geneNames).getPatternGeneSet(ok, numPerm=5, lib=lib)


# ---- 7. overrepresentation ----
def _ora_result(n=1363):
    rng = np.random.Generator(np.random.PCG64(17))
    K, nS = 4, 12
    raw = {"Amean": rng.gamma(2.0, 1.0, size=(n, K)).astype(np.float32), "Asd": np.ones((n, K), np.float32),
           "Pmean": rng.gamma(2.0, 1.0, size=(nS, K)).astype(np.float32), "Psd": np.ones((nS, K), np.float32), "seed": 5}
    sets = {"set%d" % t: ["g%d" % i for i in rng.choice(n, size=30, replace=False)] for t in range(12)}
    return CogapsResult(raw, geneNames=["g%d" % i for i in range(n)]), sets, n


@pytest.mark.parametrize("threshold", ["all", "cut"])
def test_overrepresentation(lib, threshold):
    res, sets, n = _ora_result()
    out = res.getPatternGeneSet(sets, method="overrepresentation", threshold=threshold, lib=lib)
    pm = res.patternMarkers(threshold=threshold, lib=lib)                     # the argument reaches patternMarkers: the lists differ
    assert out["patterns"] == pm["patterns"] and out["sets"] == list(sets) and out["method"] == "overrepresentation" and list(out["size"]) == [30] * 12
    L = len(pm["patterns"])
    assert out["pval"].shape == (L, 12)
    worst = 0.0
    for l, label in enumerate(pm["patterns"]):
        markers = set(pm["PatternMarkers"][label])
        for t, (name, genes) in enumerate(sets.items()):
            both = markers & set(genes)
            assert out["overlap"][l, t] == len(both) and set(out["overlapGenes"][l][t]) == both and out["k/K"][l, t] == len(both) / 30
            exact = pc.hypergeometric_upper_tail(n, len(markers), 30, len(both))
            worst = max(worst, abs(Fraction(out["pval"][l, t]) - exact) / exact)
        assert np.array_equal(out["padj"][l], pc.bh(out["pval"][l])) and np.array_equal(out["negLogPadj"][l], -10 * np.log10(out["padj"][l]))
    print("largest relative error of the tail: %.3g" % float(worst))
    assert worst <= Fraction(1, 10 ** 7)
    if threshold == "cut":
        other = res.patternMarkers(threshold="all", lib=lib)["PatternMarkers"]
        assert any(len(other[k]) != len(pm["PatternMarkers"][k]) for k in other)


def test_overrepresentation_size_limits_and_errors(lib):
    res, sets, n = _ora_result(n=2100)
    sets = dict(sets, big=["g%d" % i for i in range(2039)], none=["nobody"])
    out = res.getPatternGeneSet(sets, method="overrepresentation", lib=lib)  # maxSize defaults to 2038
    assert np.isnan(out["pval"][:, -2:]).all() and not np.isnan(out["pval"][:, :-2]).any() and list(out["size"][-2:]) == [2039, 0]
    assert np.array_equal(out["padj"][0], pc.bh(out["pval"][0]), equal_nan=True)
    assert not np.isnan(res.getPatternGeneSet(sets, method="overrepresentation", maxSize=2039, lib=lib)["pval"][:, -2]).any()
    with pytest.raises(ValueError, match="axis"):
        res.getPatternGeneSet(sets, method="overrepresentation", axis=2, lib=lib)
    with pytest.raises(TypeError, match="unexpected argument"):
        res.getPatternGeneSet(sets, threshold="cut", lib=lib)


# ---- the C entry's refusals ----
def test_c_entry_refusals(lib):
    fp, u32p, u64p, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    stat = np.ascontiguousarray(pc.stat_random()[:20, :3])
    members = [np.array([1, 4], dtype=np.uint32), np.array([0, 7, 19], dtype=np.uint32)]
    good = dict(stat=stat, off=np.array([0, 2, 5], dtype=np.uint64), mem=np.concatenate(members), nSets=2, numPerm=4, es=np.zeros((2, 3)),
                peak=np.zeros((2, 3), dtype=np.uint32), nGe=np.zeros((2, 3), dtype=np.uint32), permSum=np.zeros((2, 3), dtype=np.uint64), nRows=20, nCols=3)

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        rc = lib.cogaps_pattern_gsea(ptr(a["stat"], fp), a["nRows"], a["nCols"], 3, 1, a["nSets"], ptr(a["off"], u64p), ptr(a["mem"], u32p), a["numPerm"], 5, -1,
                                     ptr(a["es"], dp), ptr(a["peak"], u32p), ptr(a["nGe"], u32p), ptr(a["permSum"], u64p), None)
        return rc, lib.cogaps_last_error().decode()

    def valid():
        rc, _ = call()
        assert rc == 0
        want = pc.gsea(stat, members, 4, 5)
        assert all(np.array_equal(good[k], want[k]) for k in ("es", "peak", "nGe", "permSum"))

    valid()
    negative, nan = stat.copy(), stat.copy()
    negative[3, 1], nan[19, 2] = -0.5, np.nan
    cases = [
        (dict(stat=None), "null argument"), (dict(off=None), "null argument"), (dict(mem=None), "null argument"), (dict(es=None), "null argument"),
        (dict(peak=None), "null argument"), (dict(nGe=None), "null argument"), (dict(permSum=None), "null argument"),
        (dict(nSets=0), "nSets must be at least 1"), (dict(numPerm=0), "numPerm must be at least 1"),
        (dict(nRows=0), "the stat matrix is empty"), (dict(nCols=0), "the stat matrix is empty"),
        (dict(stat=negative), "stat holds a NaN or a negative value (row 3, column 1)"), (dict(stat=nan), "stat holds a NaN or a negative value (row 19, column 2)"),
        (dict(off=np.array([0, 0, 5], dtype=np.uint64)), "set 0: a set without members is not tested"),
        (dict(off=np.array([0, 20, 21], dtype=np.uint64), mem=np.arange(21, dtype=np.uint32)), "set 0: 20 members are not fewer than nRows = 20"),
        (dict(mem=np.array([1, 20, 0, 7, 19], dtype=np.uint32)), "set 0: member 20 is not a row"),
        (dict(mem=np.array([1, 4, 7, 7, 19], dtype=np.uint32)), "set 1: members are not ascending"),
        (dict(mem=np.array([4, 1, 0, 7, 19], dtype=np.uint32)), "set 0: members are not ascending"),
        (dict(off=np.array([0, 6, 5], dtype=np.uint64), mem=np.arange(6, dtype=np.uint32)), "set 1: memberOffsets decrease"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
        assert lib.cogaps_last_error_code() == _capi.ERR_GENERIC
        valid()


def test_the_refusal_names_the_first_offending_element_in_row_major_order(lib):
    """a NaN at (row 3, column 1) and a negative value at (row 1, column 2): the rows are looked through in order, each by its columns"""
    stat = np.ascontiguousarray(pc.stat_random()[:20, :3])
    stat[3, 1], stat[1, 2] = np.nan, -0.5
    for s in (stat, np.asfortranarray(stat)):
        with pytest.raises(_capi.CogapsError, match=r"stat holds a NaN or a negative value \(row 1, column 2\)"):
            _capi.pattern_gsea(s, [[1, 4], [0, 7, 19]], 4, seed=5, lib=lib)
