"""Consensus patterns on the MI355X: the cases of tests/test_consensus.py through the product library against the numpy restatement of
tests/consensus_cases.py, bit for bit -- shapes, ties, the split loop, layouts, refusals, the host path, the front end -- and a torch
tensor on the device, contiguous and as a strided view, against the same numpy array."""
import numpy as np
import pytest

import consensus_cases as cc
import test_consensus as tc
from cogaps_amd import CogapsParams, _capi, findConsensusMatrix, patternMatch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(tc.SHAPES))
def test_shapes(hip_lib, name):
    tc.check_shape(hip_lib, name)


def test_more_columns_than_the_clustering_workgroup_has_threads(hip_lib):
    tc.check_many_columns(hip_lib)


@pytest.mark.parametrize("cut", [2, 3, 5, 7])
def test_columns_repeated_exactly(hip_lib, cut):
    tc.check_ties(hip_lib, cc.repeated_columns(), cut)


@pytest.mark.parametrize("cut", [2, 5, 11])
def test_small_integers_with_many_equal_distances(hip_lib, cut):
    tc.check_ties(hip_lib, cc.small_integers(), cut)


@pytest.mark.parametrize("name", sorted(tc.SPLITS))
def test_the_split_loop(hip_lib, name):
    tc.check_split(hip_lib, name)


def test_no_cluster_reaches_minns(hip_lib):
    tc.check_no_cluster_reaches_minns(hip_lib)


def test_row_major_column_major_and_strided(hip_lib):
    tc.check_layouts(hip_lib)


def test_refusals(hip_lib):
    tc.check_refusals(hip_lib)


def test_against_the_host_path(hip_lib):
    tc.check_against_the_host_path(hip_lib)


def test_find_consensus_matrix_and_pattern_match(hip_lib):
    tc.check_exported_functions(hip_lib)


def test_a_tensor_on_the_gpu_gives_the_numpy_input_s_bytes(hip_lib):
    import torch
    X, cut, min_ns, max_ns = tc.SHAPES["n=TILE+1"]
    want = cc.restate(X, cut, min_ns, max_ns)
    cc.check(_capi.pattern_match(X, cut, min_ns, max_ns, lib=hip_lib, debug=True), want, "numpy")
    t = torch.from_numpy(X).cuda()
    cc.check(_capi.pattern_match(t, cut, min_ns, max_ns, lib=hip_lib, debug=True), want, "tensor")
    transposed = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()          # (a view: column-major on the device, read where it lies)
    assert not transposed.is_contiguous()
    cc.check(_capi.pattern_match(transposed, cut, min_ns, max_ns, lib=hip_lib, debug=True), want, "strided tensor")
    cc.check(_capi.pattern_match(t.double(), cut, min_ns, max_ns, lib=hip_lib, debug=True), want, "float64 tensor")      # (converted on the device)
    p = CogapsParams(nPatterns=3)
    p.distributed = "genome-wide"
    p.setDistributedParams(nSets=4, cut=cut, minNS=min_ns, maxNS=max_ns)
    for out in (patternMatch(t, p), findConsensusMatrix([t[:, :30], t[:, 30:]], p)):
        assert np.array_equal(out["consensus"], want["consensus"])
        assert [m.shape[1] for m in out["clusteredPatterns"]] == np.bincount(want["cluster"])[1:].tolist()
    with pytest.raises(ValueError, match="resides on device 0"):
        _capi.pattern_match(t, cut, min_ns, max_ns, device=1, lib=hip_lib)


def test_gwcogaps_with_the_device_consensus(hip_lib, gist):
    tc.check_gwcogaps(hip_lib, gist)
