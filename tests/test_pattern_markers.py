"""Pattern markers (patternMarkers; csrc/markers_kernel.h) on the emulator: ranks, scores, every marker list and its
length against the numpy restatement of tests/pattern_marker_cases.py, exactly, for both thresholds and through every form of the
ranking -- the one-workgroup count in LDS and the radix sort through global memory, below, at and above the cutoff between them; the
front end on a CogapsResult built from a raw dict; the C entry's refusals."""
import ctypes

import numpy as np
import pytest

import pattern_marker_cases as pc
from cogaps_amd import CogapsResult, _capi, patternMarkers

SMALL_ROWS = 1024        # PM_SMALL_ROWS of csrc/markers_kernel.h: the natural cutoff between the two forms
TILE = 256               # the smallest tile of the radix sort (COGAPS_TEST_MARKERS_TILE_ROWS), one workgroup's share of a column


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


@pytest.fixture(params=["lds", "global"])
def form(request, monkeypatch):
    """both forms of the ranking at any row count: the natural cutoff (every case here has at most 1024 rows), or no LDS form at all and
    tiles of 256 rows"""
    if request.param == "global":
        monkeypatch.setenv("COGAPS_TEST_MARKERS_SMALL_ROWS", "0")
        monkeypatch.setenv("COGAPS_TEST_MARKERS_TILE_ROWS", str(TILE))
    return request.param


def run(lib, kind, n, K, threshold, L=0):
    A, O = pc.inputs(kind, n, K)
    return _capi.pattern_markers(A, O, lp=pc.lp_vectors(L, K) if L else None, threshold=threshold, lib=lib)


# ---- 1. row counts and widths ----
@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("n", pc.ROW_COUNTS)
def test_row_counts(lib, form, n, threshold):
    pc.check(run(lib, "random", n, 3, threshold), pc.expected("random", n, 3, threshold))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("K", pc.WIDTHS)
def test_widths(lib, form, K, threshold):
    got = run(lib, "random", 65, K, threshold)
    pc.check(got, pc.expected("random", 65, K, threshold))
    if K == 1 and threshold == "cut":                       # one column: nothing is ever worse elsewhere, every row is a marker
        assert got[2][0].size == 65 and np.array_equal(got[0][:, 0][got[2][0]], np.arange(1, 66))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("L", [2, 70])
def test_pattern_vectors_that_are_no_unit_vectors(lib, form, L, threshold):
    got = run(lib, "random", 130, 5, threshold, L=L)
    assert got[0].shape == (130, L) and len(got[2]) == L
    pc.check(got, pc.expected("random", 130, 5, threshold, L=L))


# ---- 2. the cutoff between the forms ----
@pytest.mark.parametrize("n", [SMALL_ROWS - 1, SMALL_ROWS, SMALL_ROWS + 1])
def test_the_natural_cutoff(lib, n):
    A, O = pc.tie_pair(n=SMALL_ROWS + 1, K=3, seed=19)
    for threshold in pc.THRESHOLDS:
        pc.check(_capi.pattern_markers(A[:n], O, threshold=threshold, lib=lib), pc.restate(A[:n], O, None, threshold))


@pytest.mark.parametrize("n", [99, 100, 101, 300])
def test_a_cutoff_moved_to_a_hundred_rows(lib, monkeypatch, n):
    """99 and 100 rows are ranked in LDS, 101 and 300 by the radix sort, 300 of them in two tiles"""
    monkeypatch.setenv("COGAPS_TEST_MARKERS_SMALL_ROWS", "100")
    monkeypatch.setenv("COGAPS_TEST_MARKERS_TILE_ROWS", str(TILE))
    for threshold in pc.THRESHOLDS:
        pc.check(run(lib, "ties", n, pc.TIE_K, threshold), pc.expected("ties", n, pc.TIE_K, threshold))


# ---- 3. ties ----
def test_the_tie_case_has_ties_that_span_workgroups():
    """what makes section 3 a test of stability: groups of equal scores whose rows lie in more than one tile of 256 rows"""
    ranks, scores, cut = pc.expected("ties", pc.TIE_ROWS, pc.TIE_K, "cut")
    assert int(np.isnan(scores[:, 0]).sum()) == 3 and np.isnan(scores[pc.TIE_ROWS - 1]).all()
    for l in range(pc.TIE_K):
        col = scores[~np.isnan(scores[:, l]), l]
        values, counts = np.unique(col, return_counts=True)
        assert int((counts > 1).sum()) > 0 and int(counts[counts > 1].sum()) > 100      # well over a hundred tied scores
        spanning = [v for v in values[counts > 1] if np.flatnonzero(scores[:, l] == v).min() < TILE <= np.flatnonzero(scores[:, l] == v).max()]
        assert spanning, "no tie group of column %d spans two tiles" % l
    assert all(0 < m.size < pc.TIE_ROWS - 3 for m in cut)   # prefixes, neither empty nor everything
    assert ranks[-3:, 0].max() == pc.TIE_ROWS and set(ranks[np.isnan(scores[:, 0]), 0]) == {298, 299, 300}


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_heavy_ties_through_every_form(lib, form, threshold):
    got = run(lib, "ties", pc.TIE_ROWS, pc.TIE_K, threshold)
    pc.check(got, pc.expected("ties", pc.TIE_ROWS, pc.TIE_K, threshold))
    nan = np.isnan(got[1][:, 0])
    assert np.array_equal(np.flatnonzero(nan), [100, 200, 299])
    assert np.array_equal(got[0][nan], np.repeat([[298], [299], [300]], pc.TIE_K, axis=1))      # last, in row order, in every column
    assert not any(np.isin([100, 200, 299], m).any() for m in got[2])                              # and markers of nothing


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_equal_ranks_across_columns_take_the_lower_column(lib, form, threshold):
    A, O, lp = pc.twin_pair()
    got = _capi.pattern_markers(A, O, lp=lp, threshold=threshold, lib=lib)
    pc.check(got, pc.expected("twins", 0, 0, threshold))
    assert np.array_equal(got[0][:, 0], got[0][:, 2])
    if threshold == "all":
        assert got[2][0].size > 0 and got[2][2].size == 0
    else:
        assert np.array_equal(got[2][0], got[2][2])


# ---- 4. layouts, axes, the grid ----
@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_column_major_matrices_through_the_strides(lib, form, threshold):
    A, O = pc.inputs("random", 257, 3)
    A, O = np.asfortranarray(A), np.asfortranarray(O)
    assert A.strides == (8, 8 * 257) and O.strides == (8, 8 * pc.M_ROWS)
    pc.check(_capi.pattern_markers(A, O, threshold=threshold, lib=lib), pc.expected("random", 257, 3, threshold))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_the_other_axis(lib, form, threshold):
    """axis = 2 ranks the rows of the other matrix: the two inputs change places"""
    A, O = pc.inputs("random", 257, 3)
    pc.check(_capi.pattern_markers(O, A, threshold=threshold, lib=lib), pc.restate(O, A, None, threshold))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_outputs_do_not_depend_on_the_grid(lib, form, monkeypatch, threshold):
    """a device of two compute units: 16 workgroups loop over the tiles, columns and row blocks of the tie case"""
    want = run(lib, "ties", pc.TIE_ROWS, pc.TIE_K, threshold)
    monkeypatch.setenv("COGAPS_TEST_COMPUTE_UNITS", "2")
    A, O = pc.inputs("ties", pc.TIE_ROWS, pc.TIE_K)
    lp = pc.lp_vectors(70, pc.TIE_K)
    got = run(lib, "ties", pc.TIE_ROWS, pc.TIE_K, threshold)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert [m.tobytes() for m in got[2]] == [m.tobytes() for m in want[2]]
    pc.check(_capi.pattern_markers(A, O, lp=lp, threshold=threshold, lib=lib), pc.restate(A, O, lp, threshold))      # 70 columns on 16 workgroups


# ---- 5. front end ----
def _result(names=True):
    raw = pc.raw_result()
    n, nS = raw["Amean"].shape[0], raw["Pmean"].shape[0]
    return CogapsResult(raw, geneNames=["g%d" % i for i in range(n)] if names else None, sampleNames=["s%d" % i for i in range(nS)] if names else None), raw


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_patternMarkers_names_indices_and_axes(lib, threshold):
    res, raw = _result()
    n, K = raw["Amean"].shape
    nS = raw["Pmean"].shape[0]
    want = pc.restate(raw["Amean"], raw["Pmean"], None, threshold)
    out = res.patternMarkers(threshold=threshold, lib=lib)
    assert set(out) == {"PatternMarkers", "PatternRanks", "PatternScores", "patterns"}
    assert out["patterns"] == ["Pattern_%d" % (k + 1) for k in range(K)] == list(out["PatternMarkers"])
    assert out["PatternRanks"].shape == (n, K) and out["PatternRanks"].dtype.kind == "i" and out["PatternScores"].dtype == np.float64
    pc.check((out["PatternRanks"], out["PatternScores"], [np.array([int(g[1:]) for g in out["PatternMarkers"][p]], dtype=np.int64) for p in out["patterns"]]), want)
    assert np.isnan(out["PatternScores"][11]).all() and not any("g11" in v for v in out["PatternMarkers"].values())
    # a result without names: 1-based indices
    bare, _ = _result(names=False)
    byIndex = bare.patternMarkers(threshold=threshold, lib=lib)["PatternMarkers"]
    assert all(byIndex[p] == [int(i) + 1 for i in w] for p, w in zip(out["patterns"], want[2]))
    # the module-level form; the samples (axis = 2): the matrices change places
    assert patternMarkers(res, threshold, lib=lib)["PatternMarkers"] == out["PatternMarkers"]
    want2 = pc.restate(raw["Pmean"], raw["Amean"], None, threshold)
    out2 = patternMarkers(res, threshold, axis=2, lib=lib)
    assert out2["PatternRanks"].shape == (nS, K)
    pc.check((out2["PatternRanks"], out2["PatternScores"], [np.array([int(s[1:]) for s in out2["PatternMarkers"][p]], dtype=np.int64) for p in out2["patterns"]]), want2)


def test_patternMarkers_lp_forms_and_labels(lib):
    res, raw = _result()
    K = raw["Amean"].shape[1]
    vecs = {"early": [1, 1, 0, 0], "late": [0, 0, 0.5, 1], "flat": [1, 1, 1, 1]}
    want = pc.restate(raw["Amean"], raw["Pmean"], list(vecs.values()), "all")
    byName = res.patternMarkers(lp=vecs, lib=lib)
    assert byName["patterns"] == ["early", "late", "flat"] and list(byName["PatternMarkers"]) == ["early", "late", "flat"]
    assert byName["PatternRanks"].shape == (raw["Amean"].shape[0], 3)
    pc.check((byName["PatternRanks"], byName["PatternScores"], [np.array([int(g[1:]) for g in byName["PatternMarkers"][p]], dtype=np.int64) for p in vecs]), want)
    byList = res.patternMarkers(lp=[np.array(v) for v in vecs.values()], lib=lib)
    assert byList["patterns"] == ["1", "2", "3"]
    assert [byList["PatternMarkers"][p] for p in ("1", "2", "3")] == [byName["PatternMarkers"][p] for p in vecs]
    # the unit vectors given by hand are the default
    eye = res.patternMarkers(lp=[list(r) for r in np.eye(K)], lib=lib)
    dflt = res.patternMarkers(lib=lib)
    assert np.array_equal(eye["PatternRanks"], dflt["PatternRanks"]) and list(eye["PatternMarkers"].values()) == list(dflt["PatternMarkers"].values())


def test_patternMarkers_value_errors(lib):
    res, raw = _result()
    with pytest.raises(ValueError, match="axis must be 1 or 2"):
        res.patternMarkers(axis=0, lib=lib)
    with pytest.raises(ValueError, match="axis must be 1 or 2"):
        patternMarkers(res, axis=3, lib=lib)
    for bad in ("some", "ALL", None, 1):
        with pytest.raises(ValueError, match="threshold"):
            res.patternMarkers(threshold=bad, lib=lib)
    for bad in ([[1, 0, 0]], {"a": [1, 0, 0, 0], "b": [1, 0, 0, 0, 0]}, [[]]):
        with pytest.raises(ValueError, match="lp length must equal the number of columns"):
            res.patternMarkers(lp=bad, lib=lib)
    for bad in ([[1, 0, 0, 1.5]], {"a": [0, 0, float("nan"), 1]}):
        with pytest.raises(ValueError, match="lp should be a list of vectors with max value of 1"):
            res.patternMarkers(lp=bad, lib=lib)
    for bad in ([], {}, 3, "ab"):
        with pytest.raises(ValueError):
            res.patternMarkers(lp=bad, lib=lib)
    with pytest.raises(ValueError, match="threshold"):
        _capi.pattern_markers(raw["Amean"], raw["Pmean"], threshold="most", lib=lib)
    with pytest.raises(ValueError, match="same number of columns"):
        _capi.pattern_markers(raw["Amean"], raw["Pmean"][:, :3], lib=lib)


# ---- 6. the C entry's refusals ----
def test_c_entry_refusals(lib):
    u32p, dp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    A, O = (np.ascontiguousarray(x) for x in pc.inputs("random", 20, 3))
    lp = np.ascontiguousarray(pc.lp_vectors(2, 3))
    good = dict(a=A, n=20, K=3, o=O, m=pc.M_ROWS, lp=lp, L=2, threshold=_capi.MARKERS_CUT, ranks=np.zeros((20, 2), dtype=np.uint32), scores=np.zeros((20, 2)),
                markers=np.zeros((2, 20), dtype=np.uint32), count=np.zeros(2, dtype=np.uint32))
    want = pc.restate(A, O, lp, "cut")

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        rc = lib.cogaps_pattern_markers(ptr(a["a"], dp), a["n"], a["K"], 3, 1, ptr(a["o"], dp), a["m"], 3, 1, ptr(a["lp"], dp), a["L"], a["threshold"], -1,
                                        ptr(a["ranks"], u32p), ptr(a["scores"], dp), ptr(a["markers"], u32p), ptr(a["count"], u32p))
        return rc, lib.cogaps_last_error().decode()

    def valid():
        for k in ("ranks", "scores", "markers", "count"):
            good[k][...] = 0
        rc, _ = call()
        assert rc == 0
        lists = [good["markers"][l, :good["count"][l]] for l in range(2)]
        pc.check((good["ranks"], good["scores"], lists), want)
        assert all((good["markers"][l, good["count"][l]:] == 0xFFFFFFFF).all() for l in range(2))      # the rest of a row is padding

    valid()
    cases = [
        (dict(a=None), "null argument"), (dict(o=None), "null argument"),
        (dict(n=0), "a matrix is empty"), (dict(K=0), "a matrix is empty"), (dict(m=0), "a matrix is empty"),
        (dict(lp=None), "lp and its length must be given together"), (dict(L=0), "lp and its length must be given together"),
        (dict(lp=np.array([[0.5, 1.0, 0.0], [0.0, 1.0000001, 0.0]])), "lp should be a list of vectors with max value of 1"),
        (dict(lp=np.array([[0.5, 1.0, 0.0], [np.nan, 1.0, 0.0]])), "lp should be a list of vectors with max value of 1"),
        (dict(threshold=2), "unknown threshold 2"), (dict(threshold=-1), "unknown threshold -1"),
        (dict(n=1 << 32), "more than 32-bit ranks hold"),
    ]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, err)
        assert lib.cogaps_last_error_code() == _capi.ERR_GENERIC
        valid()
    for out in ("ranks", "scores", "markers", "count"):     # every output is optional
        rc, _ = call(**{out: None})
        assert rc == 0
    rc, _ = call(ranks=None, scores=None, markers=None, count=None)
    assert rc == 0
    # NULL and 0 are the unit vectors
    ranks = np.zeros((20, 3), dtype=np.uint32)
    rc, _ = call(lp=None, L=0, ranks=ranks, scores=None, markers=None, count=None)
    assert rc == 0 and np.array_equal(ranks, pc.restate(A, O, None, "cut")[0])
