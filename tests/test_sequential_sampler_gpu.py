"""The sequential sampler (csrc/seq_kernel.h) on the MI355X: the reference's recorded runs in the verification mode, the device against
the emulator bit for bit in the product arithmetic, a batch against its single chains, and GWCoGAPS with sampler="sequential"."""
import numpy as np
import pytest

import sequential_cases as sc
from cogaps_amd import _capi

pytestmark = pytest.mark.gpu
LANES = dict(sampler="sequential")


@pytest.mark.parametrize("name", ["modsim_k3", "gist_rows300_k3", "tiny_5x6_k2"])
def test_reference_fingerprints_on_the_gpu(hip_lib, gist, modsim, name):
    """cases 1, 3 and 5 of the recording (tests/golden/refprobe_sequential_outputs.npz), digit for digit"""
    data, kw = sc.cases(gist, modsim)[name]
    sc.compare_with_record(sc.load_record()[name], _capi.run(data, lib=hip_lib, **sc.SEQ, **kw))


def _state(lib, data, iters):
    s = _capi.Session(data, lib=lib, nPatterns=3, seed=11, nIterations=iters, outputFrequency=max(1, iters // 4), **LANES)
    try:
        s.run_iterations(1, 0, iters)
        out = {}
        for w in "AP":
            assert s.check_domain(w) == 0
            a = s.atoms(w)
            out.update({w + "pos": a["pos"], w + "mass": a["mass"], w + "left": a["left"], w + "right": a["right"], w + "mat": s.matrix(w), w + "ap": s.ap(w),
                        w + "chisq": np.float32(s.chisq(w))})
        return out
    finally:
        s.close()


@pytest.mark.parametrize("name,iters", [("modsim", 40), ("gist", 10), ("synthetic_6000x8", 4)])
def test_device_equals_emulator_in_lane_order(hip_lib, emul_lib, gist, modsim, name, iters):
    """product arithmetic: atoms (positions, masses, neighbours by index), both factor matrices, both A*P caches and chi2 after `iters`
    equilibration iterations -- one wave (modsim), 512 lanes (GIST's P sampler), two virtual lanes per thread (6000 elements)"""
    data = {"modsim": modsim, "gist": gist}.get(name)
    if data is None:
        data = sc.synthetic_6000x8()
    dev, emu = _state(hip_lib, data, iters), _state(emul_lib(256), data, iters)
    assert dev["Apos"].size > 0 and dev["Ppos"].size > 0
    for k in emu:
        assert np.array_equal(dev[k].view(np.uint32) if dev[k].dtype == np.float32 else dev[k], emu[k].view(np.uint32) if emu[k].dtype == np.float32 else emu[k]), k


def test_batch_equals_single_chains_on_the_gpu(hip_lib, modsim):
    """three chains, one workgroup each in one launch: every chain the bits it gives alone"""
    group = [dict(nPatterns=3, seed=1), dict(nPatterns=3, seed=2), dict(nPatterns=4, seed=3)]
    common = dict(nIterations=30, outputFrequency=10, **LANES)
    together = _capi.run_batch([modsim] * 3, lib=hip_lib, kws=group, **common)
    for kw, r in zip(group, together):
        alone = _capi.run(modsim, lib=hip_lib, **dict(common, **kw))
        for k in alone:
            if k not in ("totalRunningTime", "samplerSeconds"):
                assert np.array_equal(np.asarray(r[k]), np.asarray(alone[k])), k
        assert r["averageQueueLengthA"] == 0.0 and r["averageQueueLengthP"] == 0.0 and r["totalUpdates"] > 0


def test_gwcogaps_with_the_sequential_sampler(hip_lib, gist):
    """GWCoGAPS over three explicit sets on one rank: both passes run the sequential sampler (a rank's shards as one batch); every
    shard's first pass equals _capi.run of that shard alone.  (Seed 5, the seed of the other GWCoGAPS tests: the consensus step needs
    every shard's patterns to vary over the samples -- with seed 9 the third shard's chain leaves one pattern constant after 40
    iterations and the pattern matching stops with the reference's own "NA values in correlation of patterns".)"""
    from cogaps_amd import GWCoGAPS, CogapsParams
    sets = [np.arange(1, 455), np.arange(455, 909), np.arange(909, 1364)]
    p = CogapsParams(nPatterns=3, nIterations=40, seed=5, distributed="genome-wide", explicitSets=sets)
    p.setDistributedParams(nSets=3)
    res = GWCoGAPS(gist, p, sampler="sequential", messages=False, outputFrequency=20)
    first = res.metadata["diagnostics"]["firstPass"]
    assert res.featureLoadings.shape == (1363, 3) and len(first) == 3
    for i, st in enumerate(sets):
        alone = _capi.run(np.ascontiguousarray(gist[st - 1]), lib=hip_lib, nPatterns=3, nIterations=40, seed=5, outputFrequency=20, runningDistributed=True,
                          workerID=i + 1, sampler="sequential")
        for k in ("Amean", "Asd", "Pmean", "Psd", "atomsA", "atomsP", "chisq"):
            assert np.array_equal(first[i][k], alone[k]), (i, k)
        assert first[i]["totalUpdates"] == alone["totalUpdates"] and first[i]["meanChiSq"] == alone["meanChiSq"]
        assert first[i]["averageQueueLengthA"] == 0.0 and first[i]["averageQueueLengthP"] == 0.0
