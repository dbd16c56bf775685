"""Pattern markers on the MI355X: ranks, scores, every marker list and its length against the numpy restatement of
tests/pattern_marker_cases.py, exactly (the cases of tests/test_pattern_markers.py, through both forms of the ranking), the device's
bytes against the emulator's, one case at the natural cutoffs -- 200 000 rows, 49 tiles a column, integer-valued so that ties abound --
and the front end."""
import numpy as np
import pytest

import pattern_marker_cases as pc
from cogaps_amd import CogapsResult, _capi

pytestmark = pytest.mark.gpu

TILE = 256


@pytest.fixture(params=["lds", "global"])
def form(request, monkeypatch):
    if request.param == "global":
        monkeypatch.setenv("COGAPS_TEST_MARKERS_SMALL_ROWS", "0")
        monkeypatch.setenv("COGAPS_TEST_MARKERS_TILE_ROWS", str(TILE))
    return request.param


def run(lib, kind, n, K, threshold, L=0):
    A, O = pc.inputs(kind, n, K)
    return _capi.pattern_markers(A, O, lp=pc.lp_vectors(L, K) if L else None, threshold=threshold, lib=lib)


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("n", pc.ROW_COUNTS)
def test_row_counts(hip_lib, form, n, threshold):
    pc.check(run(hip_lib, "random", n, 3, threshold), pc.expected("random", n, 3, threshold))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("K", pc.WIDTHS)
def test_widths(hip_lib, form, K, threshold):
    pc.check(run(hip_lib, "random", 65, K, threshold), pc.expected("random", 65, K, threshold))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
@pytest.mark.parametrize("L", [2, 70])
def test_pattern_vectors_that_are_no_unit_vectors(hip_lib, form, L, threshold):
    pc.check(run(hip_lib, "random", 130, 5, threshold, L=L), pc.expected("random", 130, 5, threshold, L=L))


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_the_natural_cutoff(hip_lib, n):
    A, O = pc.tie_pair(n=1025, K=3, seed=19)
    for threshold in pc.THRESHOLDS:
        pc.check(_capi.pattern_markers(A[:n], O, threshold=threshold, lib=hip_lib), pc.restate(A[:n], O, None, threshold))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_heavy_ties_through_every_form(hip_lib, form, threshold):
    got = run(hip_lib, "ties", pc.TIE_ROWS, pc.TIE_K, threshold)
    pc.check(got, pc.expected("ties", pc.TIE_ROWS, pc.TIE_K, threshold))
    assert np.array_equal(np.flatnonzero(np.isnan(got[1][:, 0])), [100, 200, 299])


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_equal_ranks_across_columns_take_the_lower_column(hip_lib, form, threshold):
    A, O, lp = pc.twin_pair()
    got = _capi.pattern_markers(A, O, lp=lp, threshold=threshold, lib=hip_lib)
    pc.check(got, pc.expected("twins", 0, 0, threshold))
    assert np.array_equal(got[0][:, 0], got[0][:, 2])


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_column_major_matrices_and_the_other_axis(hip_lib, form, threshold):
    A, O = pc.inputs("random", 257, 3)
    pc.check(_capi.pattern_markers(np.asfortranarray(A), np.asfortranarray(O), threshold=threshold, lib=hip_lib), pc.expected("random", 257, 3, threshold))
    pc.check(_capi.pattern_markers(O, A, threshold=threshold, lib=hip_lib), pc.restate(O, A, None, threshold))


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_device_bytes_equal_the_emulators(hip_lib, emul_lib, form, threshold):
    emul = emul_lib(256)
    for kind, n, K, L in (("random", 257, 3, 0), ("random", 65, 70, 0), ("random", 130, 5, 70), ("ties", pc.TIE_ROWS, pc.TIE_K, 0)):
        dev, emu = run(hip_lib, kind, n, K, threshold, L), run(emul, kind, n, K, threshold, L)
        assert dev[0].tobytes() == emu[0].tobytes(), (kind, n, K, L)
        same = (dev[1].view(np.uint64) == emu[1].view(np.uint64)) | (np.isnan(dev[1]) & np.isnan(emu[1]))
        assert same.all(), (kind, n, K, L)
        assert [m.tobytes() for m in dev[2]] == [m.tobytes() for m in emu[2]], (kind, n, K, L)


@pytest.mark.parametrize("threshold", pc.THRESHOLDS)
def test_two_hundred_thousand_rows_at_the_natural_cutoffs(hip_lib, threshold):
    A, O = pc.large_pair()
    want = pc.expected("large", 0, 0, threshold)
    z = int(np.isnan(want[1][:, 0]).sum())
    col = want[1][~np.isnan(want[1][:, 0]), 0]
    assert z == 41 and np.unique(col).size < col.size // 10          # NaN rows, and at least ten rows to a score on average
    pc.check(_capi.pattern_markers(A, O, threshold=threshold, lib=hip_lib), want)


def test_front_end(hip_lib):
    raw = pc.raw_result()
    n = raw["Amean"].shape[0]
    res = CogapsResult(raw, geneNames=["g%d" % i for i in range(n)])
    for threshold in pc.THRESHOLDS:
        out = res.patternMarkers(threshold=threshold, lib=hip_lib)
        want = pc.restate(raw["Amean"], raw["Pmean"], None, threshold)
        pc.check((out["PatternRanks"], out["PatternScores"], [np.array([int(g[1:]) for g in out["PatternMarkers"][p]], dtype=np.int64) for p in out["patterns"]]), want)
        out2 = res.patternMarkers(threshold=threshold, axis=2, lib=hip_lib)
        assert np.array_equal(out2["PatternRanks"], pc.restate(raw["Pmean"], raw["Amean"], None, threshold)[0])
