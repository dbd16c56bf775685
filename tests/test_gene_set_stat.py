"""The gene-set permutation statistic (calcCoGAPSStat; csrc/geneset_kernel.h) on the emulator: the kernel's draws and
counts against the numpy restatement of tests/gene_set_cases.py, bit for bit; the draw as a fair sample, by derived bounds; the front
end on a CogapsResult built from a raw dict; the C entry's refusals."""
import ctypes
import math
import warnings

import numpy as np
import pytest

import gene_set_cases as gc
from cogaps_amd import CogapsResult, _capi, calcCoGAPSStat, calcZ


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


# ---- 1. draws ----
@pytest.mark.parametrize("n,s", gc.DRAW_SHAPES)
def test_draws_equal_the_restatement_and_are_distinct(lib, n, s):
    for seed, t, p in gc.DRAW_KEYS:
        got = _capi.permutation_draw(n, s, seed, t, p, lib=lib)
        assert np.array_equal(got, gc.draw(n, s, seed, t, p)), (seed, t, p)
        assert got.size == s and np.unique(got).size == s and int(got.max()) < n


# ---- 2. counts, bit for bit ----
def _check(lib, Z, numPerm, want):
    members, sizes = gc.count_sets()
    cnt, act = _capi.gene_set_stat(Z, members, sizes, numPerm, seed=gc.SEED, lib=lib)
    K = Z.shape[1]
    assert np.array_equal(act, want[1][:, :K], equal_nan=True)
    assert np.array_equal(cnt, want[0][:, :K])
    assert np.isnan(act[7]).all() and not cnt[7].any() and not np.isnan(np.delete(act, 7, axis=0)).any()      # the set without members
    return cnt


@pytest.mark.parametrize("numPerm", [1, 7, 130])
@pytest.mark.parametrize("K", [1, 3, 64, 70])
def test_counts_and_means_bit_for_bit(lib, K, numPerm):
    _check(lib, gc.z_random()[:, :K], numPerm, gc.expected("random", numPerm))


def test_counts_do_not_depend_on_the_grid(lib, monkeypatch):
    """a device of two compute units: 16 workgroups loop over the 120 trips of 40 sets x 3 chunks of permutations"""
    monkeypatch.setenv("COGAPS_TEST_COMPUTE_UNITS", "2")
    _check(lib, gc.z_random()[:, :3], 40, gc.expected("random", 40))


def test_column_major_z_through_the_strides(lib):
    Z = np.asfortranarray(gc.z_random()[:, :3])
    assert Z.strides == (8, 8 * gc.N_ROWS)
    _check(lib, Z, 7, gc.expected("random", 7))


def test_integer_z_exercises_the_strict_comparison(lib):
    Z = gc.z_integer()
    members, sizes = gc.count_sets()
    cnt = _check(lib, Z, 130, gc.expected("integer", 130))
    # ties do occur: with <= in place of < some count would differ
    ties = 0
    for t in (0, 1, 6):                                     # sets of one and two rows
        act = Z[members[t]].sum(axis=0) / len(members[t])
        perm = Z[gc.draws(gc.N_ROWS, sizes[t], gc.SEED, t, np.arange(130))].sum(axis=1) / sizes[t]
        ties += int((perm == act).sum())
    assert ties > 0


@pytest.mark.parametrize("K", [130, 300])
def test_wide_matrices(lib, K):
    """more than 128 columns: four register slots per lane, and above 256 columns a second block of columns"""
    Z = np.random.Generator(np.random.PCG64(K)).normal(size=(50, K))
    members = [np.array([3, 9, 27], dtype=np.uint32), np.arange(0, 50, 2, dtype=np.uint32), np.array([49], dtype=np.uint32)]
    sizes = [3, 25, 2]
    cnt, act = _capi.gene_set_stat(Z, members, sizes, 9, seed=4, lib=lib)
    want = gc.counts(Z, members, sizes, 9, 4)
    assert np.array_equal(cnt, want[0]) and np.array_equal(act, want[1])


# ---- 3. the draw is a fair sample ----
def test_inclusion_counts_are_uniform(lib):
    """every row is in a draw with probability s / n: c_i ~ Binomial(P, s / n) with variance P (s/n) (1 - s/n); the sum of the squared
    standardised deviations is chi-square with n - 1 degrees of freedom (the counts sum to P s): mean n - 1, variance 2 (n - 1); the
    bound is the mean plus six standard deviations"""
    n, s, P = 1363, 20, 2000
    c = np.zeros(n)
    for p in range(P):
        c[_capi.permutation_draw(n, s, 9, 0, p, lib=lib)] += 1
    e = P * s / n
    x2 = float(((c - e) ** 2).sum() / (e * (1 - s / n)))
    print("X2 = %.1f, dof = %d, bound = %.1f" % (x2, n - 1, (n - 1) + 6 * math.sqrt(2 * (n - 1))))
    assert x2 <= (n - 1) + 6 * math.sqrt(2 * (n - 1))


def test_upregulation_share_against_the_hypergeometric_tail(lib):
    """Z is an indicator, so a draw's mean exceeds the set's exactly when it holds more hot rows than the set's h: GSUpreg estimates
    q = P(Hypergeometric > h) from numPerm independent draws, standard error sqrt(q (1 - q) / numPerm); six of them"""
    Z, members, hs = gc.hypergeometric_case()
    cnt, act = _capi.gene_set_stat(Z, members, [gc.HG_S] * len(members), gc.HG_PERM, seed=1, lib=lib)
    assert np.array_equal(act[:, 0], np.array(hs) / np.float64(gc.HG_S))
    for t, h in enumerate(hs):
        q = gc.hypergeometric_tail(h)
        up = cnt[t, 0] / gc.HG_PERM
        print("h = %d: GSUpreg %.4f, exact %.4f, %.2f standard errors" % (h, up, q, (up - q) / math.sqrt(q * (1 - q) / gc.HG_PERM)))
        assert abs(up - q) <= 6 * math.sqrt(q * (1 - q) / gc.HG_PERM), (t, h)


# ---- 4. front end ----
def _result(names=True, **kw):
    raw = gc.raw_result(**kw)
    n, nS = raw["Amean"].shape[0], raw["Pmean"].shape[0]
    return CogapsResult(raw, geneNames=["g%d" % i for i in range(n)] if names else None, sampleNames=["s%d" % i for i in range(nS)] if names else None), raw


def test_calcZ():
    res, raw = _result()
    assert np.array_equal(res.calcZ(), raw["Amean"].astype(np.float64) / raw["Asd"].astype(np.float64)) and res.calcZ().dtype == np.float64
    assert np.array_equal(calcZ(res, "sampleFactors"), raw["Pmean"].astype(np.float64) / raw["Psd"].astype(np.float64))
    with pytest.raises(ValueError, match="whichMatrix must be either 'featureLoadings' or 'sampleFactors'"):
        res.calcZ("Amean")
    raw["Asd"][5, 2] = 0.0
    res = CogapsResult(raw)
    with pytest.warns(UserWarning, match="zeros detected in the standard deviation matrix"):
        z = res.calcZ("featureLoadings")
    assert z[5, 2] == np.float64(raw["Amean"][5, 2]) / 1e-6 and raw["Asd"][5, 2] == 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res.calcZ("sampleFactors")


def test_calcCoGAPSStat_shapes_formulas_and_names(lib):
    res, raw = _result()
    n, K = raw["Amean"].shape
    sets = {"alpha": ["g3", "g10", "g11", "g50"], "beta": ["g1", "nobody", "g2", "g2"], "gamma": ["unknown", "neither"], "delta": ["g7"]}
    out = res.calcCoGAPSStat(sets, numPerm=50, lib=lib)
    assert out["sets"] == ["alpha", "beta", "gamma", "delta"] and set(out) == {"twoSidedPValue", "GSUpreg", "GSDownreg", "GSActEst", "sets"}
    # the counts the statistic is made of: unmatched and repeated names count towards the size of the draw, not towards the members
    members, sizes = [[3, 10, 11, 50], [1, 2], [], [7]], [4, 4, 2, 1]
    cnt, _ = _capi.gene_set_stat(res.calcZ(), members, sizes, 50, seed=raw["seed"], lib=lib)
    assert np.array_equal(cnt, gc.counts(res.calcZ(), members, sizes, 50, raw["seed"])[0])
    up = cnt.T / 50.0
    up[:, 2] = np.nan                                       # m = 0
    for k in ("twoSidedPValue", "GSUpreg", "GSDownreg", "GSActEst"):
        assert out[k].shape == (K, 4) and np.isnan(out[k][:, 2]).all() and not np.isnan(np.delete(out[k], 2, axis=1)).any()
    assert np.array_equal(out["GSUpreg"], up, equal_nan=True)
    assert np.array_equal(out["GSDownreg"], 1 - up, equal_nan=True) and np.array_equal(out["GSActEst"], 1 - 2 * up, equal_nan=True)
    assert np.array_equal(out["twoSidedPValue"], np.maximum(np.minimum(1 - up, up), 1 / 50), equal_nan=True)
    # the module-level form, the alias and another seed
    assert np.array_equal(calcCoGAPSStat(res, sets, "featureLoadings", 50, lib=lib)["GSUpreg"], up, equal_nan=True)
    assert np.array_equal(res.calcCoGAPSStat(GStoGenes=sets, numPerm=50, lib=lib)["GSUpreg"], up, equal_nan=True)
    other = res.calcCoGAPSStat(sets, numPerm=50, seed=raw["seed"] + 1, lib=lib)["GSUpreg"]
    assert not np.array_equal(other, up, equal_nan=True)
    # 1-based indices, as a list: the names are "1", "2", ...
    byIndex = res.calcCoGAPSStat([[4, 11, 12, 51], [2, 3, 3, 3], [8]], numPerm=50, lib=lib)
    assert byIndex["sets"] == ["1", "2", "3"]
    assert np.array_equal(byIndex["GSUpreg"][:, 0], up[:, 0])
    assert np.array_equal(byIndex["GSUpreg"][:, 1], up[:, 1])      # (repeats count towards the size: beta's members, size and key)
    # a result without names takes indices
    bare, _ = _result(names=False)
    assert np.array_equal(bare.calcCoGAPSStat([[4, 11, 12, 51]], numPerm=50, lib=lib)["GSUpreg"][:, 0], up[:, 0])


def test_calcCoGAPSStat_sample_factors_and_the_floor(lib):
    res, raw = _result()
    z = res.calcZ("sampleFactors")
    nS, K = z.shape
    out = res.calcCoGAPSStat({"a": ["s1", "s4"], "b": ["s0", "s2", "s8"]}, whichMatrix="sampleFactors", numPerm=20, lib=lib)
    cnt = gc.counts(z, [[1, 4], [0, 2, 8]], [2, 3], 20, raw["seed"])[0]
    assert out["GSUpreg"].shape == (K, 2) and np.array_equal(out["GSUpreg"], cnt.T / 20.0)
    # planted: the s rows with the largest Z in pattern 0 -- no subset of s rows has a larger mean and the same subset is not strictly larger
    zA = res.calcZ()
    top = np.argsort(zA[:, 0])[-6:]
    out = res.calcCoGAPSStat({"top": ["g%d" % i for i in top]}, numPerm=200, lib=lib)
    assert out["GSUpreg"][0, 0] == 0.0 and out["twoSidedPValue"][0, 0] == 1 / 200 and out["GSActEst"][0, 0] == 1.0 and out["GSDownreg"][0, 0] == 1.0


def test_calcCoGAPSStat_value_errors(lib):
    res, raw = _result()
    n = raw["Amean"].shape[0]
    ok = {"a": ["g1", "g2"]}
    for bad in ("g1", 7, None, {"a": "g1"}, [3, 4], {}, []):
        with pytest.raises(ValueError):
            res.calcCoGAPSStat(bad, numPerm=5, lib=lib)
    with pytest.raises(ValueError, match="all index sets or all name sets"):
        res.calcCoGAPSStat({"a": ["g1", 2]}, numPerm=5, lib=lib)
    with pytest.raises(ValueError, match="all index sets or all name sets"):
        res.calcCoGAPSStat({"a": ["g1"], "b": [2]}, numPerm=5, lib=lib)
    with pytest.raises(ValueError, match="empty"):                                   # s = 0
        res.calcCoGAPSStat({"a": ["g1"], "b": []}, numPerm=5, lib=lib)
    with pytest.raises(ValueError, match="without replacement"):                     # s > n
        res.calcCoGAPSStat({"a": ["g%d" % (i % n) for i in range(n + 1)]}, numPerm=5, lib=lib)
    with pytest.raises(ValueError, match="outside 1"):
        res.calcCoGAPSStat([[0, 1]], numPerm=5, lib=lib)
    with pytest.raises(ValueError, match="outside 1"):
        res.calcCoGAPSStat([[1, n + 1]], numPerm=5, lib=lib)
    for bad in (0, -3, 2.5, None):
        with pytest.raises(ValueError, match="numPerm"):
            res.calcCoGAPSStat(ok, numPerm=bad, lib=lib)
    with pytest.raises(ValueError, match="whichMatrix"):
        res.calcCoGAPSStat(ok, whichMatrix="P", numPerm=5, lib=lib)
    bare, _ = _result(names=False)
    with pytest.raises(ValueError, match="carries no geneNames"):
        bare.calcCoGAPSStat(ok, numPerm=5, lib=lib)
    assert res.calcCoGAPSStat(ok, numPerm=5, lib=lib)["GSUpreg"].shape == (raw["Amean"].shape[1], 1)


# ---- 5. the C entry's refusals ----
def test_c_entry_refusals(lib):
    u32p, u64p, dp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    Z = np.ascontiguousarray(gc.z_random()[:20, :3])
    good = dict(z=Z, off=np.array([0, 2, 2, 5], dtype=np.uint64), mem=np.array([1, 4, 0, 7, 19], dtype=np.uint32), size=np.array([2, 1, 20], dtype=np.uint32),
                nSets=3, numPerm=4, cnt=np.zeros((3, 3), dtype=np.uint32), act=np.zeros((3, 3)))

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        rc = lib.cogaps_gene_set_stat(ptr(a["z"], dp), 20, 3, 3, 1, a["nSets"], ptr(a["off"], u64p), ptr(a["mem"], u32p), ptr(a["size"], u32p), a["numPerm"], 5, -1,
                                      ptr(a["cnt"], u32p), ptr(a["act"], dp))
        return rc, lib.cogaps_last_error().decode()

    def valid():
        rc, _ = call()
        assert rc == 0
        want = gc.counts(Z, [[1, 4], [], [0, 7, 19]], [2, 1, 20], 4, 5)
        assert np.array_equal(good["cnt"], want[0]) and np.array_equal(good["act"], want[1], equal_nan=True)

    valid()
    cases = [
        (dict(z=None), "null argument"), (dict(off=None), "null argument"), (dict(mem=None), "null argument"),
        (dict(size=None), "null argument"), (dict(cnt=None), "null argument"),
        (dict(nSets=0), "nSets must be at least 1"), (dict(numPerm=0), "numPerm must be at least 1"),
        (dict(size=np.array([2, 0, 20], dtype=np.uint32)), "set 1: a draw of 0 rows is outside 1 .. nRows = 20"),
        (dict(size=np.array([2, 1, 21], dtype=np.uint32)), "set 2: a draw of 21 rows is outside 1 .. nRows = 20"),
        (dict(mem=np.array([1, 20, 0, 7, 19], dtype=np.uint32)), "set 0: member 20 is not a row"),
        (dict(mem=np.array([1, 4, 7, 7, 19], dtype=np.uint32)), "set 2: members are not ascending"),
        (dict(mem=np.array([4, 1, 0, 7, 19], dtype=np.uint32)), "set 0: members are not ascending"),
        (dict(off=np.array([0, 2, 1, 5], dtype=np.uint64)), "set 1: memberOffsets decrease"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
        assert lib.cogaps_last_error_code() == _capi.ERR_GENERIC
        valid()
    rc, _ = call(act=None)                                  # the means are optional
    assert rc == 0
    out = np.zeros(4, dtype=np.uint32)
    assert lib.cogaps_debug_permutation_draw(20, 0, 1, 0, 0, -1, out.ctypes.data_as(u32p)) != 0 and "outside 1 .. nRows" in lib.cogaps_last_error().decode()
    assert lib.cogaps_debug_permutation_draw(20, 21, 1, 0, 0, -1, out.ctypes.data_as(u32p)) != 0
    assert lib.cogaps_debug_permutation_draw(20, 4, 1, 0, 0, -1, None) != 0 and "null argument" in lib.cogaps_last_error().decode()
    assert lib.cogaps_debug_permutation_draw(20, 4, 1, 0, 0, -1, out.ctypes.data_as(u32p)) == 0 and np.array_equal(out, gc.draw(20, 4, 1, 0, 0))
