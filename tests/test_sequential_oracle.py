"""The sequential sampler against an INDEPENDENT restatement: the oracle's SingleThreadedGibbsSampler (oracle/gaps_oracle.c), on the CPU.

1. the oracle's sequential sampler reproduces the reference build's six recorded runs -- neither the emulator nor the library takes part;
2. the emulator build of csrc/seq_kernel.h equals that oracle step by step in the PRODUCT arithmetic (lane-order sums, portable logf /
   expf) at every reduction class, with the options of the sampler's scope, and as a batch (cases: sequential_oracle_cases.py; the
   same cases run on the MI355X in test_sequential_oracle_gpu.py);
3. gm_udiv64 and pcg_uniform64 (csrc/gaps_math.h), compiled for the host, against exact integers (cases: udiv64_cases.py)."""
import pytest

import sequential_cases as sc
import sequential_oracle_cases as oc
import udiv64_cases as uc
from cogaps_amd import _capi


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["modsim_k3", "gist_k7", "gist_rows300_k3", "gist_rows300_k3_fixedP", "tiny_5x6_k2", "gist_k4_pump_snapshots"])
def test_oracle_reproduces_the_recorded_reference_runs(oracle, gist, modsim, name):
    """one accumulator per sum (redW = 1, redG = 1) and glibc's logf / expf (MATH_GLIBC_FMA): atom and chi2 histories, totalUpdates,
    meanChiSq, the statistics matrices, PUMP and snapshots of tests/golden/refprobe_sequential_outputs.npz, digit for digit.  A case
    that fails here is a fault of the oracle, not of the recording."""
    data, kw = sc.cases(gist, modsim)[name]
    kw = dict(kw)
    n_snap, phase = kw.pop("nSnapshots", 0), kw.pop("snapshotPhase", "sampling")
    if n_snap:      # Cogaps.cpp:104-123
        kw.update(snapshotFrequency=kw["nIterations"] // n_snap, snapshotPhase={"all": 0, "equilibration": 1, "sampling": 2}[phase])
    o = oracle.run(data, sampler="sequential", math_mode=oracle.MATH_GLIBC_FMA, redW_A=1, redW_P=1, redG=1, **kw)
    sc.compare_with_record(sc.load_record()[name], o)


def test_oracle_scope(oracle, modsim):
    """the dense model only; the asynchronous sampler stays the default, and the selector changes the chain"""
    with pytest.raises(RuntimeError, match="dense model only"):
        oracle.Session(modsim, nPatterns=3, seed=1, sampler="sequential", sparseOptimization=True)
    kw = dict(nPatterns=3, seed=42, nIterations=20, outputFrequency=5, math_mode=oracle.MATH_PORTABLE)
    a, d, s = oracle.run(modsim, sampler="async", **kw), oracle.run(modsim, **kw), oracle.run(modsim, sampler="sequential", **kw)
    assert a["atomsA"].tolist() == d["atomsA"].tolist() and a["averageQueueLengthA"] == d["averageQueueLengthA"] > 0.0
    assert s["averageQueueLengthA"] == 0.0 and s["averageQueueLengthP"] == 0.0 and s["atomsA"].tolist() != a["atomsA"].tolist()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.SHAPES, ids=oc.SHAPE_IDS)
def test_every_reduction_class_stepwise(emul_lib, gist, case):
    oc.check_shape(emul_lib(256), gist, case)


@pytest.mark.parametrize("option,shape", oc.OPTION_CASES, ids=oc.OPTION_IDS)
def test_options_stepwise(emul_lib, option, shape):
    oc.check_option(emul_lib(256), option, shape)


def test_batch_against_one_oracle_session_per_chain(emul_lib):
    oc.check_batch(emul_lib(256))


def test_update_across_a_launch_boundary_on_the_emulator(emul_lib):
    """sequential_oracle_cases.LONG with the real SEQ_STEPS_PER_LAUNCH = 4096 (the variant with 7 of test_sequential_sampler.py shows
    independence of the constant; this one parks and resumes where the device does): 45908 steps, the largest update 4221"""
    oc.check_long_state(emul_lib(256))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_udiv64_host_edges(emul_lib):
    a, b = uc.edge_pairs()
    uc.check_udiv64(lambda x, y: _capi.debug_udiv64(x, y, lib=emul_lib(256)), a, b)


def test_udiv64_host_exact_multiples(emul_lib):
    a, b = uc.multiple_pairs()
    uc.check_udiv64(lambda x, y: _capi.debug_udiv64(x, y, lib=emul_lib(256)), a, b)


def test_udiv64_host_random_pairs(emul_lib):
    a, b = uc.random_pairs()
    uc.check_udiv64(lambda x, y: _capi.debug_udiv64(x, y, lib=emul_lib(256)), a, b)


def test_uniform64_host(emul_lib):
    uc.check_uniform64(lambda s, lo, hi: _capi.debug_uniform64(s, lo, hi, lib=emul_lib(256)))


def test_refused_inputs_host(emul_lib):
    uc.check_refusals(emul_lib(256), on_device=False)
