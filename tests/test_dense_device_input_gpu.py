"""Dense input resident on the MI355X (product library): the kernels of csrc/dense_build.h from device pointers and from host pointers,
each against parity_util.dense_reference and against each other -- the checks of test_dense_device_input.py with real device addresses
-- and torch tensors on the GPU through CoGAPS / GWCoGAPS / scCoGAPS."""
import numpy as np
import pytest

import test_dense_device_input as t
from cogaps_amd import CoGAPS, CogapsParams, GWCoGAPS, scCoGAPS

pytestmark = pytest.mark.gpu


def dd(d, u=None):
    """the arrays placed on the GPU with torch, as raw addresses"""
    import torch
    from cogaps_amd import _capi
    dev = torch.device("cuda", torch.cuda.current_device())
    td, tu = torch.from_numpy(d).to(dev), None if u is None else torch.from_numpy(u).to(dev)
    torch.cuda.synchronize()
    return _capi.DeviceDense(d.shape, td.data_ptr(), None if tu is None else tu.data_ptr(), keep=(td, tu))


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("shape", t.SHAPES)
def test_structures_gpu(hip_lib, shape, transpose, which):
    t.check_structures(hip_lib, dd, shape, transpose, which)


@pytest.mark.parametrize("shape", t.SHAPES)
def test_a_negative_value_and_a_negative_zero_gpu(hip_lib, shape):
    t.check_a_negative_value_and_a_negative_zero(hip_lib, dd, shape)


def test_the_order_of_the_sum_gpu(hip_lib):
    t.check_the_order_of_the_sum(hip_lib, dd)


@pytest.mark.parametrize("sparse,fixed", [(False, "N"), (True, "N"), (False, "P")])
def test_stepwise_gpu(hip_lib, sparse, fixed):
    t.check_stepwise(hip_lib, dd, sparse, fixed)


@pytest.mark.parametrize("sparse", [False, True])
def test_run_device_equals_run_gpu(hip_lib, sparse):
    t.check_run_device_equals_run(hip_lib, dd, sparse)


def test_refusals_gpu(hip_lib):
    t.check_refusals(hip_lib, dd)


# ---- torch tensors through the front end ----

def assert_results_equal(a, b):
    for f in ("featureLoadings", "loadingStdDev", "sampleFactors", "factorStdDev"):
        assert getattr(a, f).size and np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.getMeanChiSq() == b.getMeanChiSq()


@pytest.fixture(scope="module")
def data():
    return t.matrix(130, 65)


def gpu(x, dtype=None):
    import torch
    return torch.from_numpy(x).to(device=torch.device("cuda", torch.cuda.current_device()), dtype=dtype)


KW = dict(nPatterns=3, nIterations=20, seed=9, messages=False, outputFrequency=10)


@pytest.mark.parametrize("sparse", [False, True])
def test_cogaps_from_a_gpu_tensor(hip_lib, data, sparse):
    import torch
    kw = dict(KW, sparseOptimization=sparse)
    ref = CoGAPS(data, **kw)
    assert_results_equal(ref, CoGAPS(gpu(data), **kw))
    assert_results_equal(ref, CoGAPS(gpu(data, torch.float64), **kw))                                       # converted on the device
    view = gpu(np.ascontiguousarray(data.T)).t()
    assert not view.is_contiguous() and tuple(view.shape) == data.shape
    assert_results_equal(ref, CoGAPS(view, **kw))
    sub = dict(subsetIndices=t.subset(130, 5), subsetDim=1)
    assert_results_equal(CoGAPS(data, **kw, **sub), CoGAPS(gpu(data), **kw, **sub))
    assert_results_equal(CoGAPS(np.ascontiguousarray(data.T), transposeData=True, **kw), CoGAPS(gpu(data).t(), transposeData=True, **kw))


def test_cogaps_with_an_uncertainty_tensor(hip_lib, data):
    u = t.uncertainty(data)
    ref = CoGAPS(data, uncertainty=u, **KW)
    assert_results_equal(ref, CoGAPS(gpu(data), uncertainty=gpu(u), **KW))
    assert_results_equal(ref, CoGAPS(gpu(data), uncertainty=u, **KW))          # follows the data to the device
    assert_results_equal(ref, CoGAPS(data, uncertainty=gpu(u), **KW))          # ... or to the host
    assert not np.array_equal(ref.featureLoadings, CoGAPS(data, **KW).featureLoadings)


def test_a_cpu_tensor_is_its_numpy_view(hip_lib, data):
    import torch
    assert_results_equal(CoGAPS(data, **KW), CoGAPS(torch.from_numpy(data), **KW))


def test_front_end_errors(hip_lib, data):
    bad = data.copy()
    bad[3, 4] = -1
    with pytest.raises(ValueError, match="negative values"):
        CoGAPS(gpu(bad), **KW)
    with pytest.raises(ValueError, match="negative values"):
        CoGAPS(gpu(data), uncertainty=gpu(-t.uncertainty(data)), **KW)
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="NA values"):
        CoGAPS(gpu(bad), **KW)
    with pytest.raises(ValueError, match="device"):
        CoGAPS(gpu(data), device=5, **KW)
    with pytest.raises(ValueError, match="nPatterns must be less"):
        CoGAPS(gpu(data), **dict(KW, nPatterns=65))


@pytest.mark.parametrize("entry,sparse", [(GWCoGAPS, False), (scCoGAPS, False), (scCoGAPS, True)])
def test_distributed_from_a_gpu_tensor(hip_lib, entry, sparse):
    """world 1, two sets: every shard's session is created from the one resident array with subsetIndices"""
    d = t.matrix(60, 160)
    p = CogapsParams(nPatterns=3, nIterations=30, seed=4, sparseOptimization=sparse)
    p.setDistributedParams(nSets=2, minNS=2)
    ref, got = entry(d, p, messages=False), entry(gpu(d), p, messages=False)
    assert_results_equal(ref, got)
