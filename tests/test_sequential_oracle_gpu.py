"""The sequential sampler on the MI355X against the oracle's own sequential sampler (oracle/gaps_oracle.c, pinned to the reference's
recorded runs by test_sequential_oracle.py): the HIP kernel's PRODUCT arithmetic bit for bit at every reduction class (V = 1, 2, 4, 8,
16 virtual lanes per thread), with the options of the sampler's scope, as a batch, and across a real launch boundary; the device's
gm_udiv64 / pcg_uniform64 against exact integers.  The cases are those of the emulator's tests (sequential_oracle_cases.py, udiv64_cases.py)."""
import pytest

import sequential_oracle_cases as oc
import udiv64_cases as uc
from cogaps_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", oc.SHAPES, ids=oc.SHAPE_IDS)
def test_every_reduction_class_stepwise_on_the_gpu(hip_lib, gist, case):
    oc.check_shape(hip_lib, gist, case)


@pytest.mark.parametrize("option,shape", oc.OPTION_CASES, ids=oc.OPTION_IDS)
def test_options_stepwise_on_the_gpu(hip_lib, option, shape):
    oc.check_option(hip_lib, option, shape)


def test_batch_against_one_oracle_session_per_chain_on_the_gpu(hip_lib):
    oc.check_batch(hip_lib)


def test_update_across_a_launch_boundary_state(hip_lib):
    """8000 x 6, nPatterns 8, seed 2, nIterations 16 (sequential_oracle_cases.LONG): 45908 steps over both phases, and two updates of
    the A sampler in the sampling phase take more than SEQ_STEPS_PER_LAUNCH = 4096 steps -- the largest 4221, so the launch parks in
    GenScalars after 4096 steps and a second queued launch resumes it.  The oracle's step counts assert the crossing; the state at the
    end of the run (atoms, matrices, A*P, chi2) and the finished result are the oracle's."""
    oc.check_long_state(hip_lib)


def test_update_across_a_launch_boundary_run(hip_lib):
    """the same configuration through cogaps_run (_capi.run): the oracle's result"""
    oc.check_long_run(hip_lib)


def test_udiv64_device_edges(hip_lib):
    a, b = uc.edge_pairs()
    uc.check_udiv64(lambda x, y: _capi.debug_udiv64(x, y, on_device=True, lib=hip_lib), a, b)


def test_udiv64_device_exact_multiples(hip_lib):
    a, b = uc.multiple_pairs()
    uc.check_udiv64(lambda x, y: _capi.debug_udiv64(x, y, on_device=True, lib=hip_lib), a, b)


def test_udiv64_device_random_pairs(hip_lib):
    a, b = uc.random_pairs()
    uc.check_udiv64(lambda x, y: _capi.debug_udiv64(x, y, on_device=True, lib=hip_lib), a, b)


def test_uniform64_device(hip_lib):
    uc.check_uniform64(lambda s, lo, hi: _capi.debug_uniform64(s, lo, hi, on_device=True, lib=hip_lib))


def test_refused_inputs_device(hip_lib):
    """(refused on the host, before any launch)"""
    uc.check_refusals(hip_lib, on_device=True)
