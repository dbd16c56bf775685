"""Gene-set membership (calcGeneGSStat, computeGeneGSProb; csrc/genemember_kernel.h) on the emulator: the C entry's
statistics and counts against the numpy restatement of tests/gene_membership_cases.py, bit for bit; the edges of the rows, of the
members' chunks and of the grid; ties; an answer that needs no order; the front end on a CogapsResult built from a raw dict; the C
entry's refusals; toCSV / fromCSV."""
import ctypes

import numpy as np
import pytest

import gene_membership_cases as gm
import gene_set_cases as gc
from cogaps_amd import CogapsResult, _capi, calcGeneGSStat, computeGeneGSProb, fromCSV, toCSV

GM_THREADS = 256                                            # csrc/genemember_kernel.h: rows of one workgroup trip


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


def _check(lib, Z, members, w, wNull, want=None):
    """every output of one call against the restatement, bit for bit"""
    if want is None:
        want = gm.membership(np.asarray(Z), members, w, wNull)
    out = _capi.gene_set_membership(Z, members, w, wNull=wNull, allStat=True, lib=lib)
    assert np.array_equal(out["memberStat"], gm.concat(want[0], np.float64), equal_nan=True)
    assert np.array_equal(out["greaterCount"], gm.concat(want[1], np.uint32))
    assert np.array_equal(out["allStat"], want[2], equal_nan=True)
    assert np.array_equal(out["offsets"], np.concatenate([[0], np.cumsum([len(m) for m in members])]))
    return out


# ---- 1. the C entry against the restatement ----
@pytest.mark.parametrize("numPerm", gm.PERM_LIST)
@pytest.mark.parametrize("K", gm.K_LIST)
def test_statistics_and_counts_bit_for_bit(lib, K, numPerm):
    for mode in ("plain", "pw", "split"):
        Z, members, w, wNull, want = gm.entry_case(K, numPerm, mode)
        out = _check(lib, Z, members, w, wNull, want)
        if numPerm == 1:                                    # every count is floored to numPerm: the weights vanish, every set is inactive
            assert not out["memberStat"].any() and not out["allStat"].any() and not out["greaterCount"].any()
    assert (Z.sum(axis=1) < 1e-6).any()                     # negative row sums: the statistic's second threshold is exercised


def test_the_counts_hold_the_floor_and_full_counts():
    """what the issue states of the first three columns: 130 permutations leave 3 zero counts and 3 full ones, 7 leave 22 and 16"""
    for numPerm, zeros, full in ((130, 3, 3), (7, 22, 16)):
        c = gm.perm_counts(numPerm)[:, :3]
        assert (int((c == 0).sum()), int((c == numPerm).sum())) == (zeros, full)


def test_the_outputs_are_optional_one_by_one(lib):
    Z, members, w, wNull, want = gm.entry_case(3, 7, "split")
    only = _capi.gene_set_membership(Z, members, w, wNull=wNull, stat=False, counts=True, lib=lib)
    assert only["memberStat"] is None and only["allStat"] is None and np.array_equal(only["greaterCount"], gm.concat(want[1], np.uint32))
    only = _capi.gene_set_membership(Z, members, w, wNull=wNull, stat=False, counts=False, allStat=True, lib=lib)
    assert np.array_equal(only["allStat"], want[2], equal_nan=True)
    only = _capi.gene_set_membership(Z, members, w, wNull=wNull, stat=True, counts=False, lib=lib)
    assert np.array_equal(only["memberStat"], gm.concat(want[0], np.float64), equal_nan=True)


# ---- 2. row edges, chunks of members, the grid ----
def _edge_sets(N):
    rng = np.random.Generator(np.random.PCG64(N))
    sets = [np.arange(N), np.array([N - 1]), np.array([0])]             # every row; the last row; the first
    if N > 2:
        sets += [np.sort(rng.choice(N, size=N // 2, replace=False)), np.arange(1, N)]
    return [s.astype(np.uint32) for s in sets]


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, GM_THREADS - 1, GM_THREADS, GM_THREADS + 1])
def test_row_edges(lib, N):
    members = _edge_sets(N)
    rng = np.random.Generator(np.random.PCG64(7))
    w = rng.random((len(members), 5))
    out = _check(lib, gm.z_wide()[:N, :5], members, w, rng.random((len(members), 5)))
    assert not out["greaterCount"][:N].any()                # m = N: nothing is outside the set


def test_sets_larger_than_a_chunk(emul_lib):
    """GM_CHUNK = 64: the sets of 64, 65 and 200 members take one, two and four chunks"""
    small = emul_lib(256, "-DGM_CHUNK=64", "_gmchunk64")
    Z, members, w, wNull, want = gm.entry_case(3, 130, "split")
    assert {64, 65, 200} <= {len(m) for m in members}
    _check(small, Z, members, w, wNull, want)


def test_counts_do_not_depend_on_the_grid(lib, monkeypatch):
    """a device of two compute units: 16 workgroups loop over the 80 trips of 40 sets x 2 blocks of rows"""
    monkeypatch.setenv("COGAPS_TEST_COMPUTE_UNITS", "2")
    Z, members, w, wNull, want = gm.entry_case(3, 130, "split")
    _check(lib, Z, members, w, wNull, want)


# ---- 3. ties and strictness, 4. an answer that needs no order ----
def test_ties_follow_the_strict_comparison(lib):
    Z, members, w, wNull = gm.tie_case()
    want = gm.membership(Z, members, w, wNull)
    _check(lib, Z, members, w, wNull, want)
    ties = 0
    for t, mem in enumerate(members):                       # with >= in place of > some count would differ
        null = np.delete(want[2][t], mem)
        ties += int((null[None, :] == want[0][t][:, None]).sum())
    assert ties > 0
    free = gm.order_free_counts(Z, members, w, wNull)
    assert all(np.array_equal(a, b) for a, b in zip(want[1], free))


# ---- 5. column-major Z ----
def test_column_major_z_through_the_strides(lib):
    Z, members, w, wNull, want = gm.entry_case(3, 7, "pw")
    F = np.asfortranarray(Z)
    assert F.strides == (8, 8 * gc.N_ROWS)
    _check(lib, F, members, w, wNull, want)


# ---- 6. independence of the call ----
def test_a_set_does_not_depend_on_its_call(lib):
    Z, members, w, wNull, want = gm.entry_case(3, 130, "split")
    for t in (2, 5, 7, 39):                                 # 63 and 200 members, none, 64
        _check(lib, Z, [members[t]], w[t:t + 1], wNull[t:t + 1], ([want[0][t]], [want[1][t]], want[2][t:t + 1]))
    _check(lib, Z, list(members) * 15, np.tile(w, (15, 1)), np.tile(wNull, (15, 1)), (want[0] * 15, want[1] * 15, np.tile(want[2], (15, 1))))


# ---- 7. front end ----
def _planted(names=True):
    raw, rows, intruder = gm.planted_set()
    n, nS = raw["Amean"].shape[0], raw["Pmean"].shape[0]
    res = CogapsResult(raw, geneNames=["g%d" % i for i in range(n)] if names else None, sampleNames=["s%d" % i for i in range(nS)] if names else None)
    return res, raw, rows, intruder


@pytest.mark.parametrize("numPerm", [200, 500])
def test_computeGeneGSProb_finds_the_intruder(lib, numPerm):
    res, raw, rows, intruder = _planted()
    assert intruder == 84
    sets = {"planted": ["g%d" % i for i in rows], "other": ["g3", "g10", "nobody", "g50"]}
    out = res.computeGeneGSProb(sets, numPerm=numPerm, lib=lib)
    assert set(out) == {"sets", "genes", "prob", "stat", "greaterCount", "nullSize", "GSUpreg"} and out["sets"] == ["planted", "other"]
    members, sizes = [rows, np.array([3, 10, 50])], [9, 4]
    prob, stat, cnt, nullSize, up = gm.gene_prob(res.calcZ(), members, sizes, numPerm, raw["seed"])
    assert up[0, 0] == 1.0 / numPerm                        # no permutation beats the planted set in pattern 0: the floor acts
    for t in range(2):
        assert out["genes"][t] == ["g%d" % i for i in members[t]]
        assert np.array_equal(out["prob"][t], prob[t]) and np.array_equal(out["stat"][t], stat[t]) and np.array_equal(out["greaterCount"][t], cnt[t])
        assert np.array_equal(out["prob"][t], out["greaterCount"][t] / np.float64(out["nullSize"][t])) and out["greaterCount"][t].dtype == np.int64
    assert np.array_equal(out["nullSize"], [111, 117]) and np.array_equal(out["GSUpreg"], up) and not np.isnan(out["prob"][0]).any()
    p = dict(zip(out["genes"][0], out["prob"][0]))
    print("numPerm %d: intruder %.3f, members at most %.3f" % (numPerm, p["g84"], max(v for k, v in p.items() if k != "g84")))
    assert all(p["g84"] > v for k, v in p.items() if k != "g84")
    # names and 1-based indices, the module function and the reference's argument name give the same answer
    bare = _planted(names=False)[0]
    for other in (bare.computeGeneGSProb([[int(i) + 1 for i in rows]], numPerm=numPerm, lib=lib),
                  computeGeneGSProb(res, {"planted": sets["planted"]}, numPerm, lib=lib),
                  res.computeGeneGSProb(GStoGenes={"planted": sets["planted"]}, numPerm=numPerm, lib=lib)):
        assert np.array_equal(other["prob"][0], prob[0]) and np.array_equal(other["stat"][0], stat[0])
    assert bare.computeGeneGSProb([[int(i) + 1 for i in rows]], numPerm=numPerm, lib=lib)["genes"][0] == [int(i) + 1 for i in rows]


def test_calcGeneGSStat_slices_one_statistic(lib):
    res, raw, rows, _ = _planted()
    sets = {"planted": ["g%d" % i for i in rows], "lost": ["nobody", "neither"]}
    Pw = np.array([1.0, 0.5, 2.0, 0.25])
    z = res.calcZ()
    for pw in (None, Pw):
        _, _, w = gm.weights(gc.counts(z, [rows, []], [9, 2], 200, raw["seed"])[0], 200, pw)
        T = gm.row_stat(z, w[0])
        inside, outside = res.calcGeneGSStat(sets, 200, Pw=pw, lib=lib), calcGeneGSStat(res, sets, 200, Pw=pw, nullGenes=True, lib=lib)
        assert inside["sets"] == outside["sets"] == ["planted", "lost"]
        assert np.array_equal(inside["stat"][0], T[rows]) and inside["genes"][0] == ["g%d" % i for i in rows]
        rest = np.setdiff1d(np.arange(120), rows)
        assert np.array_equal(outside["stat"][0], T[rest]) and outside["genes"][0] == ["g%d" % i for i in rest]
        # a set with no matched row: no members, every row outside it
        assert inside["stat"][1].size == 0 and inside["genes"][1] == [] and np.array_equal(outside["stat"][1], gm.row_stat(z, w[1])) and len(outside["genes"][1]) == 120
    lost = res.computeGeneGSProb(sets, numPerm=200, lib=lib)
    assert all(lost[k][1].size == 0 for k in ("prob", "stat", "greaterCount")) and lost["genes"][1] == [] and lost["nullSize"][1] == 120


def test_weighting_arguments(lib):
    res, raw, rows, _ = _planted()
    sets = {"planted": ["g%d" % i for i in rows]}
    Pw = np.array([1.0, 0.5, 2.0, 0.25])
    plain = res.computeGeneGSProb(sets, numPerm=200, lib=lib)
    for bad in ([1.0, 2.0], np.ones(5), [1.0, np.nan]):
        with pytest.raises(ValueError, match="Invalid weighting"):
            res.computeGeneGSProb(sets, numPerm=200, Pw=bad, lib=lib)
        with pytest.raises(ValueError, match="Invalid weighting"):
            res.calcGeneGSStat(sets, 200, Pw=bad, lib=lib)
    for none in (np.full(4, np.nan), [np.nan], np.full(7, np.nan)):      # all NaN, of any length: no weighting
        same = res.computeGeneGSProb(sets, numPerm=200, Pw=none, PwNull=True, lib=lib)
        assert np.array_equal(same["prob"][0], plain["prob"][0]) and np.array_equal(same["stat"][0], plain["stat"][0])
    assert np.array_equal(res.computeGeneGSProb(sets, numPerm=200, PwNull=True, lib=lib)["prob"][0], plain["prob"][0])      # PwNull without Pw: nothing to differ in
    both, split = res.computeGeneGSProb(sets, numPerm=200, Pw=Pw, PwNull=True, lib=lib), res.computeGeneGSProb(sets, numPerm=200, Pw=Pw, lib=lib)
    assert np.array_equal(both["stat"][0], split["stat"][0]) and not np.array_equal(both["greaterCount"][0], split["greaterCount"][0])
    for out, pwNull in ((both, True), (split, False)):
        want = gm.gene_prob(res.calcZ(), [rows], [9], 200, raw["seed"], Pw=Pw, PwNull=pwNull)
        assert np.array_equal(out["prob"][0], want[0][0]) and np.array_equal(out["greaterCount"][0], want[2][0])
    for bad in (0, -3, 2.5, None):
        with pytest.raises(ValueError, match="numPerm"):
            res.computeGeneGSProb(sets, numPerm=bad, lib=lib)
    # one permutation: the count is floored to 1 of 1, the weights vanish -- statistics of 0, no probability; a set of every row has none either
    dead = res.computeGeneGSProb(sets, numPerm=1, lib=lib)
    assert not dead["stat"][0].any() and np.isnan(dead["prob"][0]).all()
    whole = res.computeGeneGSProb([list(range(1, 121))], numPerm=20, lib=lib)
    assert whole["nullSize"][0] == 0 and np.isnan(whole["prob"][0]).all() and not whole["greaterCount"][0].any()


# ---- 8. the C entry's refusals ----
def test_c_entry_refusals(lib):
    u32p, u64p, dp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    Z = np.ascontiguousarray(gc.z_random()[:20, :3])
    members = [[1, 4], [], [0, 7, 19]]
    w = np.random.Generator(np.random.PCG64(2)).random((3, 3))
    good = dict(z=Z, off=np.array([0, 2, 2, 5], dtype=np.uint64), mem=np.array([1, 4, 0, 7, 19], dtype=np.uint32), w=w, wNull=None, nSets=3, nRows=20,
                stat=np.zeros(5), cnt=np.zeros(5, dtype=np.uint32), all=np.zeros((3, 20)))
    want = gm.membership(Z, members, w)

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        rc = lib.cogaps_gene_set_membership(ptr(a["z"], dp), a["nRows"], 3, 3, 1, a["nSets"], ptr(a["off"], u64p), ptr(a["mem"], u32p), ptr(a["w"], dp), ptr(a["wNull"], dp), -1,
                                            ptr(a["stat"], dp), ptr(a["cnt"], u32p), ptr(a["all"], dp))
        return rc, lib.cogaps_last_error().decode()

    def valid():
        rc, _ = call()
        assert rc == 0
        assert np.array_equal(good["stat"], gm.concat(want[0], np.float64), equal_nan=True) and np.array_equal(good["cnt"], gm.concat(want[1], np.uint32))
        assert np.array_equal(good["all"], want[2], equal_nan=True)

    valid()
    cases = [
        (dict(z=None), "null argument"), (dict(off=None), "null argument"), (dict(mem=None), "null argument"), (dict(w=None), "null argument"),
        (dict(stat=None, cnt=None, all=None), "one of memberStat, greaterCount and allStat must be given"),
        (dict(nSets=0), "nSets must be at least 1"), (dict(nRows=0), "the Z matrix is empty"),
        (dict(mem=np.array([1, 20, 0, 7, 19], dtype=np.uint32)), "set 0: member 20 is not a row"),
        (dict(mem=np.array([1, 4, 7, 7, 19], dtype=np.uint32)), "set 2: members are not ascending"),
        (dict(mem=np.array([4, 1, 0, 7, 19], dtype=np.uint32)), "set 0: members are not ascending"),
        (dict(off=np.array([0, 2, 1, 5], dtype=np.uint64)), "set 1: memberOffsets decrease"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and err.startswith("cogaps_gene_set_membership: ") and msg in err, (kw, err)
        assert lib.cogaps_last_error_code() == _capi.ERR_GENERIC
        valid()
    for kw in (dict(stat=None), dict(cnt=None), dict(all=None), dict(stat=None, cnt=None), dict(cnt=None, all=None)):      # each output is optional
        assert call(**kw)[0] == 0


# ---- 9. toCSV / fromCSV ----
def test_csv_round_trip(tmp_path):
    raw = gc.raw_result(n=30, K=3)
    raw.update(meanChiSq=1234.5678901234567, chisq=np.array([3.5, 0.1, 1e-30], dtype=np.float32), atomsA=np.array([5, 7, 11], dtype=np.uint32), atomsP=np.array([2, 3, 4], dtype=np.uint32))
    raw["Amean"][3, 1] = np.float32(1e-38)
    raw["Psd"][2, 0] = np.float32(3.4028235e38)
    genes = ["g%d" % i for i in range(29)] + ['odd, "quoted" name']
    res = CogapsResult(raw, geneNames=genes, sampleNames=["s%d" % i for i in range(9)])
    res.metadata["version"] = "3.21.5"
    toCSV(res, str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(n + ".csv" for n in (
        "featureLoadings", "sampleFactors", "loadingStdDev", "factorStdDev", "geneNames", "sampleNames", "meanChiSq", "chisqHistory", "version", "atomsA", "atomsP"))
    back = fromCSV(str(tmp_path))
    for name in ("featureLoadings", "sampleFactors", "loadingStdDev", "factorStdDev"):
        assert getattr(back, name).dtype == np.float32 and np.array_equal(getattr(back, name), getattr(res, name)), name
    assert back.geneNames == genes and back.sampleNames == res.sampleNames
    assert back.metadata["meanChiSq"] == raw["meanChiSq"] and back.metadata["version"] == "3.21.5"
    for key in ("chisq", "atomsA", "atomsP"):
        assert np.array_equal(back.metadata["diagnostics"][key], raw[key]), key
    assert back.metadata["diagnostics"]["atomsA"].dtype == np.int64 and back.metadata["diagnostics"]["chisq"].dtype == np.float64
    assert np.array_equal(back.calcZ(), res.calcZ())
    # a result without names, history or version
    bare = CogapsResult(gc.raw_result(n=5, K=2))
    bare.toCSV(str(tmp_path))
    back = fromCSV(str(tmp_path))
    assert back.geneNames is None and back.sampleNames is None and back.metadata["meanChiSq"] is None and back.metadata["version"] is None
    assert "chisq" not in back.metadata["diagnostics"] and np.array_equal(back.featureLoadings, bare.featureLoadings)
