"""The gene sets of every pattern on the MI355X: the device's ranks, scores and permutation sums against the numpy restatement of
tests/pattern_gene_set_cases.py, bit for bit (the cases of tests/test_pattern_gene_set.py), a case of more workgroup trips than the grid
holds, the planted sets and both methods through the front end."""
import numpy as np
import pytest

import pattern_gene_set_cases as pc
from cogaps_amd import CogapsResult, _capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,K,zero", pc.RANK_SHAPES)
def test_ranks_are_the_stable_argsort(hip_lib, n, K, zero):
    pc.check_ranks(hip_lib, n, K, zero)


@pytest.mark.parametrize("numPerm", pc.PERM_CASES)
@pytest.mark.parametrize("K", pc.K_CASES)
def test_scores_bit_for_bit(hip_lib, K, numPerm):
    pc.check_scores(hip_lib, pc.stat_random()[:, :K], numPerm, pc.expected("random", numPerm))


def test_column_major_stat_through_the_strides(hip_lib):
    pc.check_scores(hip_lib, np.asfortranarray(pc.stat_random()[:, :3]), 7, pc.expected("random", 7))


def test_members_that_are_all_zero_in_a_column(hip_lib):
    pc.check_scores(hip_lib, pc.stat_zero_members(), 7, pc.expected("zero", 7))


def test_integer_stat_exercises_greater_or_equal(hip_lib):
    pc.check_scores(hip_lib, pc.stat_integer(), 130, pc.expected("integer", 130))


def test_sets_up_to_the_cap(hip_lib):
    pc.check_big(hip_lib)


def test_a_set_above_the_cap(hip_lib):
    stat = pc.gamma_loadings(pc.BIG_ROWS, 2, 9)
    with pytest.raises(_capi.CogapsError, match="4097 members are more than GSEA_MAX_SET = 4096"):
        _capi.pattern_gsea(stat, [np.arange(4097, dtype=np.uint32)], 2, lib=hip_lib)
    res = CogapsResult({"Amean": stat, "Asd": np.ones_like(stat), "Pmean": np.ones((3, 2), np.float32), "Psd": np.ones((3, 2), np.float32), "seed": 1})
    out = res.getPatternGeneSet([list(range(1, 4098)), [5, 9, 11]], numPerm=3, lib=hip_lib)
    assert list(out["size"]) == [4097, 3] and np.isnan(out["ES"][:, 0]).all()
    assert np.array_equal(out["ES"][:, 1], pc.gsea(stat, [np.array([4, 8, 10])], 3, 1)["es"][0])


def test_more_trips_than_workgroups(hip_lib):
    """600 sets x 9 chunks of 16 permutations: 5400 workgroup trips, above the 8 x 256 workgroups a whole MI355X is given"""
    stat, members, want = pc.many_sets_case()
    got = _capi.pattern_gsea(stat, members, 130, seed=2, lib=hip_lib)
    for key in ("es", "peak", "nGe", "permSum"):
        assert np.array_equal(got[key], want[key]), key


def test_planted_sets(hip_lib):
    pc.check_planted(hip_lib)


def test_overrepresentation_through_the_front_end(hip_lib):
    res, raw = pc.raw_result_with_names()
    n = raw["Amean"].shape[0]
    sets = {"a": ["g%d" % i for i in range(0, 30)], "b": ["g%d" % i for i in range(50, 120, 3)]}
    out = res.getPatternGeneSet(sets, method="overrepresentation", lib=hip_lib)
    pm = res.patternMarkers(lib=hip_lib)
    for l, label in enumerate(pm["patterns"]):
        markers = set(pm["PatternMarkers"][label])
        for t, genes in enumerate(sets.values()):
            both = markers & set(genes)
            assert out["overlap"][l, t] == len(both)
            exact = pc.hypergeometric_upper_tail(n, len(markers), len(genes), len(both))
            assert abs(out["pval"][l, t] - float(exact)) <= 1e-7 * float(exact)
