"""The gene-set permutation statistic on the MI355X: the device's draws and counts against the numpy restatement of
tests/gene_set_cases.py, bit for bit (the cases of tests/test_gene_set_stat.py), a case of more workgroup trips than the grid holds, and
the planted set through the front end."""
import numpy as np
import pytest

import gene_set_cases as gc
from cogaps_amd import CogapsResult, _capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,s", gc.DRAW_SHAPES)
def test_draws_equal_the_restatement_and_are_distinct(hip_lib, n, s):
    for seed, t, p in gc.DRAW_KEYS:
        got = _capi.permutation_draw(n, s, seed, t, p, lib=hip_lib)
        assert np.array_equal(got, gc.draw(n, s, seed, t, p)), (seed, t, p)
        assert got.size == s and np.unique(got).size == s and int(got.max()) < n


def _check(lib, Z, numPerm, want):
    members, sizes = gc.count_sets()
    cnt, act = _capi.gene_set_stat(Z, members, sizes, numPerm, seed=gc.SEED, lib=lib)
    K = Z.shape[1]
    assert np.array_equal(act, want[1][:, :K], equal_nan=True)
    assert np.array_equal(cnt, want[0][:, :K])
    assert np.isnan(act[7]).all() and not cnt[7].any()


@pytest.mark.parametrize("numPerm", [1, 7, 130])
@pytest.mark.parametrize("K", [1, 3, 64, 70])
def test_counts_and_means_bit_for_bit(hip_lib, K, numPerm):
    _check(hip_lib, gc.z_random()[:, :K], numPerm, gc.expected("random", numPerm))


def test_column_major_z_through_the_strides(hip_lib):
    _check(hip_lib, np.asfortranarray(gc.z_random()[:, :3]), 7, gc.expected("random", 7))


def test_integer_z_exercises_the_strict_comparison(hip_lib):
    _check(hip_lib, gc.z_integer(), 130, gc.expected("integer", 130))


@pytest.mark.parametrize("K", [130, 300])
def test_wide_matrices(hip_lib, K):
    Z = np.random.Generator(np.random.PCG64(K)).normal(size=(50, K))
    members = [np.array([3, 9, 27], dtype=np.uint32), np.arange(0, 50, 2, dtype=np.uint32), np.array([49], dtype=np.uint32)]
    sizes = [3, 25, 2]
    cnt, act = _capi.gene_set_stat(Z, members, sizes, 9, seed=4, lib=hip_lib)
    want = gc.counts(Z, members, sizes, 9, 4)
    assert np.array_equal(cnt, want[0]) and np.array_equal(act, want[1])


def test_more_trips_than_workgroups(hip_lib):
    """600 sets x 9 chunks of 16 permutations: 5400 workgroup trips, above the 8 x 256 workgroups a whole MI355X is given"""
    rng = np.random.Generator(np.random.PCG64(21))
    Z = gc.z_random()[:, :5]
    sizes = [(1, 2, 5)[t % 3] for t in range(600)]
    members = [np.sort(rng.choice(gc.N_ROWS, size=s, replace=False)).astype(np.uint32) for s in sizes]
    cnt, act = _capi.gene_set_stat(Z, members, sizes, 130, seed=2, lib=hip_lib)
    want = gc.counts(Z, members, sizes, 130, 2)
    assert np.array_equal(cnt, want[0]) and np.array_equal(act, want[1])


def test_planted_set_through_the_front_end(hip_lib):
    raw = gc.raw_result()
    n, K = raw["Amean"].shape
    res = CogapsResult(raw, geneNames=["g%d" % i for i in range(n)])
    z = res.calcZ()
    top = np.argsort(z[:, 0])[-6:]
    out = res.calcCoGAPSStat({"top": ["g%d" % i for i in top], "other": ["g1", "g2", "g3"]}, numPerm=200, lib=hip_lib)
    assert out["GSUpreg"].shape == (K, 2) and out["sets"] == ["top", "other"]
    assert out["GSUpreg"][0, 0] == 0.0 and out["twoSidedPValue"][0, 0] == 1 / 200 and out["GSActEst"][0, 0] == 1.0
    cnt = gc.counts(z, [np.sort(top), [1, 2, 3]], [6, 3], 200, raw["seed"])[0]
    assert np.array_equal(out["GSUpreg"], cnt.T / 200.0)
