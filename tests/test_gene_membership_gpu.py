"""Gene-set membership on the MI355X: the device's statistics and counts against the numpy restatement of
tests/gene_membership_cases.py, bit for bit (the cases of tests/test_gene_membership.py), more workgroup trips than the grid holds, a
matrix of GIST's loadings' shape, and the planted set through the front end."""
import numpy as np
import pytest

import gene_membership_cases as gm
import gene_set_cases as gc
from cogaps_amd import CogapsResult, _capi

pytestmark = pytest.mark.gpu

GM_THREADS = 256                                            # csrc/genemember_kernel.h: rows of one workgroup trip


def _check(lib, Z, members, w, wNull, want=None):
    if want is None:
        want = gm.membership(np.asarray(Z), members, w, wNull)
    out = _capi.gene_set_membership(Z, members, w, wNull=wNull, allStat=True, lib=lib)
    assert np.array_equal(out["memberStat"], gm.concat(want[0], np.float64), equal_nan=True)
    assert np.array_equal(out["greaterCount"], gm.concat(want[1], np.uint32))
    assert np.array_equal(out["allStat"], want[2], equal_nan=True)
    return out


@pytest.mark.parametrize("numPerm", [7, 130])
@pytest.mark.parametrize("K", [3, 64, 70])
def test_statistics_and_counts_bit_for_bit(hip_lib, K, numPerm):
    for mode in ("plain", "pw", "split"):
        Z, members, w, wNull, want = gm.entry_case(K, numPerm, mode)
        _check(hip_lib, Z, members, w, wNull, want)


def test_ties_follow_the_strict_comparison(hip_lib):
    Z, members, w, wNull = gm.tie_case()
    out = _check(hip_lib, Z, members, w, wNull)
    assert np.array_equal(out["greaterCount"], gm.concat(gm.order_free_counts(Z, members, w, wNull), np.uint32))


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, GM_THREADS - 1, GM_THREADS, GM_THREADS + 1])
def test_row_edges(hip_lib, N):
    rng = np.random.Generator(np.random.PCG64(N))
    members = [np.arange(N), np.array([N - 1]), np.array([0])]
    if N > 2:
        members += [np.sort(rng.choice(N, size=N // 2, replace=False)), np.arange(1, N)]
    members = [m.astype(np.uint32) for m in members]
    out = _check(hip_lib, gm.z_wide()[:N, :5], members, rng.random((len(members), 5)), rng.random((len(members), 5)))
    assert not out["greaterCount"][:N].any()                # m = N: nothing is outside the set


def test_column_major_z_through_the_strides(hip_lib):
    Z, members, w, wNull, want = gm.entry_case(3, 7, "pw")
    _check(hip_lib, np.asfortranarray(Z), members, w, wNull, want)


def test_more_trips_than_workgroups(hip_lib):
    """600 sets x 2 blocks of rows, and with them the members' kernel's 150 trips of four sets"""
    rng = np.random.Generator(np.random.PCG64(21))
    Z = gc.z_random()[:, :5]
    members = [np.sort(rng.choice(gc.N_ROWS, size=(1, 2, 5)[t % 3], replace=False)).astype(np.uint32) for t in range(600)]
    _check(hip_lib, Z, members, rng.random((600, 5)), rng.random((600, 5)))


def test_loadings_of_gist_shape(hip_lib):
    """1363 x 7, twelve sets of up to 600 members (more than one chunk of them): nothing depends on the matrix being small"""
    rng = np.random.Generator(np.random.PCG64(22))
    Z = rng.gamma(2.0, 1.0, size=(1363, 7)) / (0.2 + rng.random((1363, 7)))
    members = [np.sort(rng.choice(1363, size=s, replace=False)).astype(np.uint32) for s in (1, 15, 64, 65, 100, 257, 300, 500, 512, 513, 600, 1362)]
    _check(hip_lib, Z, members, rng.random((12, 7)), rng.random((12, 7)))


def test_planted_set_through_the_front_end(hip_lib):
    raw, rows, intruder = gm.planted_set()
    res = CogapsResult(raw, geneNames=["g%d" % i for i in range(120)])
    sets = {"planted": ["g%d" % i for i in rows], "other": ["g3", "g10", "nobody", "g50"]}
    for numPerm in (200, 500):
        out = res.computeGeneGSProb(sets, numPerm=numPerm, lib=hip_lib)
        prob, stat, cnt, nullSize, up = gm.gene_prob(res.calcZ(), [rows, np.array([3, 10, 50])], [9, 4], numPerm, raw["seed"])
        for t in range(2):
            assert np.array_equal(out["prob"][t], prob[t]) and np.array_equal(out["stat"][t], stat[t]) and np.array_equal(out["greaterCount"][t], cnt[t])
        assert up[0, 0] == 1.0 / numPerm and np.array_equal(out["GSUpreg"], up) and np.array_equal(out["nullSize"], nullSize)
        p = dict(zip(out["genes"][0], out["prob"][0]))
        assert all(p["g%d" % intruder] > v for k, v in p.items() if k != "g%d" % intruder)
    T = gm.row_stat(res.calcZ(), gm.weights(gc.counts(res.calcZ(), [rows], [9], 200, raw["seed"])[0], 200)[2][0])
    assert np.array_equal(res.calcGeneGSStat({"planted": sets["planted"]}, 200, lib=hip_lib)["stat"][0], T[rows])
    assert np.array_equal(res.calcGeneGSStat({"planted": sets["planted"]}, 200, nullGenes=True, lib=hip_lib)["stat"][0], np.delete(T, rows))
