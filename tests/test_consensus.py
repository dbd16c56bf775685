"""Consensus patterns (cogaps_pattern_match; csrc/consensus_kernel.h) on the emulator: the correlation distance, the
labels of the first cut, the cluster and the rounded correlation of every column, the consensus matrix and the number of clusters
against the numpy restatement of tests/consensus_cases.py, bit for bit -- at two and three rows, below, at and above a chunk of the row
rule, at two columns, one column above a tile, column and row counts that are no multiple of four, and more columns than the clustering
workgroup has threads with more than a thousand merges; ties; the split loop; layouts; refusals; the host path; the front end.  The
bodies take the library, so that tests/test_consensus_gpu.py runs them on the MI355X."""
import ctypes as C

import numpy as np
import pytest

import consensus_cases as cc
from cogaps_amd import CogapsParams, CogapsResult, GWCoGAPS, _capi, findConsensusMatrix, patternMatch
from cogaps_amd import distributed as dd

SHAPES = cc.shape_cases()
SPLITS = cc.split_cases()


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


def run_case(lib, X, cut, min_ns, max_ns, what=""):
    got = _capi.pattern_match(X, cut, min_ns, max_ns, lib=lib, debug=True)
    want = cc.restate(X, cut, min_ns, max_ns)
    cc.check(got, want, what)
    return got, want


# ---- 0. the restatement's clustering is the host path's ----
def test_the_restatement_clusters_like_the_host_path():
    rng = np.random.Generator(np.random.MT19937(31))
    for n in (2, 3, 7, 20, 60):
        for kind in ("random", "ties"):
            d = rng.random((n, n)) if kind == "random" else rng.integers(1, 4, size=(n, n)).astype(np.float64)
            d = np.maximum(d, d.T)
            np.fill_diagonal(d, 0.0)
            for k in sorted({1, 2, n // 2 + 1, n - 1, n, n + 3}):
                assert np.array_equal(cc.cutree(d, k)[0], dd._complete_linkage_cutree(d, k)), (n, kind, k)


# ---- 1. shapes ----
def check_shape(lib, name):
    X, cut, min_ns, max_ns = SHAPES[name]
    run_case(lib, X, cut, min_ns, max_ns, name)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(lib, name):
    check_shape(lib, name)


def test_the_named_shapes_sit_at_the_kernels_constants():
    dims = {name: SHAPES[name][0].shape for name in SHAPES}
    assert dims["L=2"][0] == 2 and dims["L=3"][0] == 3 and dims["n=2"][1] == 2
    assert [dims[k] for k in ("L=KC-1,n=5", "L=KC,n=5", "L=KC+37,n=5")] == [(4095, 5), (4096, 5), (4133, 5)] and cc.KC == 4096
    assert dims["n=TILE+1"][1] == 65 == cc.TILE + 1 and dims["n=4*TILE+3,L=17"] == (17, 259)
    assert dims["n=7,L=10"][1] % 4 and dims["n=7,L=10"][0] % 4


def check_many_columns(lib):
    X, cut, min_ns, max_ns = cc.many_columns_case()
    assert X.shape[1] > cc.LINK_THREADS
    got, want = run_case(lib, X, cut, min_ns, max_ns, "many columns")
    assert want["merges"] > 1000 and got["nClusters"] == cut


def test_more_columns_than_the_clustering_workgroup_has_threads(lib):
    check_many_columns(lib)


# ---- 2. ties ----
def check_ties(lib, X, cut):
    got, want = run_case(lib, X, cut, 1, X.shape[1], "ties")
    d = got["dist"]
    off = d[~np.eye(d.shape[0], dtype=bool)]
    assert np.unique(off).size < off.size // 4                   # (many pairs are equally far apart: the tie rule decides)
    assert np.array_equal(got["firstLabels"], dd._complete_linkage_cutree(d, cut))


@pytest.mark.parametrize("cut", [2, 3, 5, 7])
def test_columns_repeated_exactly(lib, cut):
    check_ties(lib, cc.repeated_columns(), cut)


@pytest.mark.parametrize("cut", [2, 5, 11])
def test_small_integers_with_many_equal_distances(lib, cut):
    check_ties(lib, cc.small_integers(), cut)


# ---- 3. the split loop ----
def check_split(lib, name):
    X, cut, min_ns, max_ns, splits, clusters = SPLITS[name]
    got, want = run_case(lib, X, cut, min_ns, max_ns, name)
    assert (want["splits"], want["nClusters"]) == (splits, clusters)
    sizes = np.bincount(got["cluster"], minlength=clusters + 1)
    assert (sizes[1:] >= min_ns).all() and (sizes[1:] <= max_ns).all()
    if name != "splits twice":
        assert sizes[0] == 1 and np.isnan(got["corr"][got["cluster"] == 0]).all()
    if name == "a part is dropped":
        assert np.bincount(want["firstLabels"]).max() == 5         # (the first cut kept the five together)
    if name == "minNS drops a first-pass cluster":
        assert np.bincount(want["firstLabels"])[1:].min() == 1


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_the_split_loop(lib, name):
    check_split(lib, name)


def check_no_cluster_reaches_minns(lib):
    X = cc.random_patterns(12, 4, 41)
    with pytest.raises(ValueError, match=cc.EMPTY_MESSAGE):
        cc.restate(X, 4, 2, 4)
    with pytest.raises(_capi.CogapsError, match=cc.EMPTY_MESSAGE):
        _capi.pattern_match(X, 4, 2, 4, lib=lib)


def test_no_cluster_reaches_minns(lib):
    check_no_cluster_reaches_minns(lib)


# ---- 4. layouts ----
def check_layouts(lib):
    X, cut, min_ns, max_ns = SHAPES["n=TILE+1"]
    want = cc.restate(X, cut, min_ns, max_ns)
    wide = np.zeros((X.shape[0] * 2 + 1, X.shape[1] * 3 + 2), dtype=np.float32) - 1      # (what a wrong stride would read is refused: negative)
    wide[1::2, 2::3] = X
    view = wide[1::2, 2::3]
    fortran = np.asfortranarray(X)
    assert fortran.flags.f_contiguous and not fortran.flags.c_contiguous and not view.flags.c_contiguous and not view.flags.f_contiguous
    for what, m in (("row-major", np.ascontiguousarray(X)), ("column-major", fortran), ("strided", view), ("float64", X.astype(np.float64))):
        cc.check(_capi.pattern_match(m, cut, min_ns, max_ns, lib=lib, debug=True), want, what)


def test_row_major_column_major_and_strided(lib):
    check_layouts(lib)


# ---- 5. refusals ----
def check_refusals(lib):
    X = cc.planted(12, [3, 3], 42)
    for bad, message in ((dict(X=np.zeros((0, 6), dtype=np.float32)), "the pattern matrix is empty"),
                         (dict(X=np.zeros((6, 0), dtype=np.float32)), "the pattern matrix is empty"),
                         (dict(X=X[:, :1]), "nCols must be at least 2"),
                         (dict(cut=0), "cut must be at least 1"),
                         (dict(minNS=0), "minNS must be at least 1"),
                         (dict(minNS=3, maxNS=2), "maxNS = 2 is below minNS = 3"),
                         (dict(X=np.ones((2, cc.MAX_COLS + 1), dtype=np.float32)), "4097 patterns are more than COGAPS_PATTERN_MATCH_MAX_COLS = 4096")):
        kw = dict(X=X, cut=2, minNS=2, maxNS=6)
        kw.update(bad)
        with pytest.raises(_capi.CogapsError, match=message):
            _capi.pattern_match(kw["X"], kw["cut"], kw["minNS"], kw["maxNS"], lib=lib)
    for value in (np.nan, -1.0):
        poisoned = X.copy()
        poisoned[7, 4] = value
        with pytest.raises(_capi.CogapsError, match="a NaN or a negative value"):
            _capi.pattern_match(poisoned, 2, 2, 6, lib=lib)
    constant = X.copy()
    constant[:, 2] = 1.5
    with pytest.raises(ValueError, match=cc.NA_MESSAGE):
        cc.restate(constant, 2, 2, 6)
    with pytest.raises(_capi.CogapsError, match=cc.NA_MESSAGE):
        _capi.pattern_match(constant, 2, 2, 6, lib=lib)
    # null arguments, at the C entry itself
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    count, cluster, consensus = C.c_uint32(0), np.zeros(6, dtype=np.uint32), np.zeros(X.size, dtype=np.float32)
    good = [X.ctypes.data, 12, 6, 6, 1, 0, 2, 2, 6, -1, C.byref(count), cluster.ctypes.data_as(u32p), None, _capi._fp(consensus), None, None]
    assert lib.cogaps_pattern_match(*good) == 0 and count.value == 2
    for slot in (0, 10, 11, 13):
        args = list(good)
        args[slot] = None
        assert lib.cogaps_pattern_match(*args) != 0 and "null argument" in lib.cogaps_last_error().decode()


def test_refusals(lib):
    check_refusals(lib)


# ---- 6. against the host path ----
def ulps_apart(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_against_the_host_path(lib):
    X, cut, min_ns, max_ns = cc.well_separated()
    p = CogapsParams(nPatterns=3)
    p.setDistributedParams(nSets=4, cut=cut, minNS=min_ns, maxNS=max_ns)
    host = dd.pattern_match(X, p)
    got, want = run_case(lib, X, cut, min_ns, max_ns, "well separated")
    assert got["nClusters"] == len(host["clusteredPatterns"]) == 3
    for ci, members in enumerate(host["clusteredPatterns"]):
        mine = np.nonzero(got["cluster"] == ci + 1)[0]
        assert np.array_equal(X[:, mine], members)
        assert np.array_equal(want["corr"][mine], dd.corr_to_mean_pattern(members))      # (the case's premise: no correlation sits at a rounding boundary)
    assert ulps_apart(got["consensus"], host["consensus"]).max() <= 1


def test_against_the_host_path(lib):
    check_against_the_host_path(lib)


# ---- 7. the front end ----
def check_exported_functions(lib):
    X, cut, min_ns, max_ns = cc.well_separated()
    p = CogapsParams(nPatterns=3)
    p.setDistributedParams(nSets=4, cut=cut, minNS=min_ns, maxNS=max_ns)
    want = cc.restate(X, cut, min_ns, max_ns)
    for out in (patternMatch(X, p, lib=lib), findConsensusMatrix([X[:, :5], X[:, 5:7], X[:, 7:]], p, lib=lib)):
        assert sorted(out) == ["CorrToMeanPattern", "clusteredPatterns", "consensus"]
        assert out["consensus"].dtype == np.float32 and np.array_equal(out["consensus"], want["consensus"])
        assert len(out["clusteredPatterns"]) == len(out["CorrToMeanPattern"]) == want["nClusters"]
        for ci in range(want["nClusters"]):
            members = want["cluster"] == ci + 1
            assert np.array_equal(out["clusteredPatterns"][ci], X[:, members]) and np.array_equal(out["CorrToMeanPattern"][ci], want["corr"][members])


def test_find_consensus_matrix_and_pattern_match(lib):
    check_exported_functions(lib)
    import cogaps_amd
    assert {"findConsensusMatrix", "patternMatch"} <= set(cogaps_amd.__all__)


def gw_params():
    p = CogapsParams(nPatterns=3, seed=5, nIterations=20)
    p.distributed = "genome-wide"
    p.setDistributedParams(nSets=3, minNS=2)
    p.explicitSets = [list(range(1, 101)), list(range(101, 181)), list(range(181, 301))]
    return p


def check_gwcogaps(lib, gist):
    """(the library is the one _capi.load() gives: the caller sees to that)"""
    runs = {c: GWCoGAPS(gist[:300], gw_params(), messages=False, outputFrequency=10, **({} if c is None else {"consensus": c}))
            for c in ("device", "host", None)}
    diag = {c: r.metadata["diagnostics"] for c, r in runs.items()}
    for key in ("Amean", "Asd", "Pmean", "Psd"):
        for i in range(3):
            assert np.array_equal(diag["device"]["firstPass"][i][key], diag["host"]["firstPass"][i][key]), (key, i)
    for a, b in zip(diag["device"]["unmatchedPatterns"], diag["host"]["unmatchedPatterns"]):
        assert np.array_equal(a, b)
    p = gw_params()
    again = _capi.pattern_match(np.concatenate(diag["device"]["unmatchedPatterns"], axis=1), p.cut, p.minNS, p.maxNS, lib=lib)
    assert np.array_equal(diag["device"]["consensus"], again["consensus"])
    assert runs["device"].featureLoadings.shape == (300, again["nClusters"])
    corr = runs["device"].getCorrelationToMeanPattern()
    assert len(corr) == len(runs["device"].getClusteredPatterns()) == again["nClusters"]
    for ci, r in enumerate(corr):
        assert np.array_equal(r, again["corr"][again["cluster"] == ci + 1])
    assert len(runs["host"].getCorrelationToMeanPattern()) == len(runs["host"].getClusteredPatterns())
    # "host" is the default, and the default is what it was
    for key in ("featureLoadings", "loadingStdDev", "sampleFactors", "factorStdDev"):
        assert np.array_equal(getattr(runs["host"], key), getattr(runs[None], key)), key
    assert np.array_equal(diag["host"]["consensus"], diag[None]["consensus"])
    host = dd.find_consensus_matrix(diag["host"]["unmatchedPatterns"], p)
    assert np.array_equal(diag["host"]["consensus"], host["consensus"])


def test_gwcogaps_with_the_device_consensus(lib, gist, monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: lib)
    check_gwcogaps(lib, gist)


def test_an_unknown_consensus_is_refused(gist):
    with pytest.raises(ValueError, match="consensus must be 'host' or 'device'"):
        GWCoGAPS(gist[:300], gw_params(), messages=False, consensus="gpu")
    with pytest.raises(ValueError, match="consensus must be 'host' or 'device'"):
        dd.distributedCogaps(gist[:300], gw_params(), consensus="gpu")


def test_the_gather_hands_back_the_stacked_tensor():
    """what the device consensus reads with an NCCL group: the gathered matrices side by side, in subset order"""
    import torch

    class OneRank:
        get_world_size = staticmethod(lambda: 1)
        get_rank = staticmethod(lambda: 0)

        @staticmethod
        def all_gather(out, buf):
            out[0].copy_(buf)
    local = {i: cc.random_patterns(9, 3, 50 + i) for i in range(3)}
    listed, stacked = dd._all_gather_arrays(local, [(9, 3)] * 3, OneRank, "cpu", stacked=True)
    assert isinstance(stacked, torch.Tensor) and np.array_equal(stacked.numpy(), np.concatenate([local[i] for i in range(3)], axis=1))
    again = dd._all_gather_arrays(local, [(9, 3)] * 3, OneRank, "cpu")
    assert all(np.array_equal(a, b) and np.array_equal(a, local[i]) for i, (a, b) in enumerate(zip(listed, again)))


def test_a_standard_result_has_no_correlation_to_a_mean_pattern():
    A, P = np.ones((4, 2), dtype=np.float32), np.ones((3, 2), dtype=np.float32)
    assert CogapsResult({"Amean": A, "Asd": A, "Pmean": P, "Psd": P}).getCorrelationToMeanPattern() is None
