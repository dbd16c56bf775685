"""nPatterns above 50 on the MI355X, bit for bit against the oracle: the cases of tests/test_large_k.py (see there for what each K is
for) on the hardware, and what is too slow on the emulator -- the wide evaluation form, the balancing list's overflow, the chained
launch against two launches per batch."""
import numpy as np
import pytest

import parity_util as pu
import test_large_k as lk
from cogaps_amd import _capi

pytestmark = pytest.mark.gpu


# ---- 1. the sparse model step by step ----

@pytest.mark.parametrize("k", lk.ORDER_SWITCH + lk.REGISTER_SWITCH + lk.TRIP_COUNTS)
def test_sparse_stepwise(hip_lib, k):
    lk.sparse_stepwise(hip_lib, lk.counts_90x70(), k, 20, total_iter=20)


def test_sparse_stepwise_all_of_sp_kmax(hip_lib):
    lk.sparse_stepwise(hip_lib, pu.synthetic_counts(64, 64, zeros=0.5, seed=3), 512, 10, total_iter=20)


@pytest.mark.parametrize("k", [24, 25, 26, 64, 65, 97, 130, 512])
def test_sparse_stepwise_dense_factors(hip_lib, k):
    lk.dense_factors_stepwise(hip_lib, k, 20)


@pytest.mark.parametrize("genes,samples,zeros", [(300, 200, 0.85), (64, 64, 0.5)])
def test_sparse_stepwise_flag_words(hip_lib, genes, samples, zeros):
    lk.sparse_stepwise(hip_lib, pu.synthetic_counts(genes, samples, zeros=zeros, seed=3), 65, 20, total_iter=20)


def test_sparse_all_proposal_types(hip_lib):
    lk.all_proposal_types_case(hip_lib, 8)


def test_sparse_wide_form(hip_lib):
    """eval_sparse_kernel_wide above 64 patterns: the P sampler's data vectors have 20000 elements (more than 16384)"""
    lk.sparse_stepwise(hip_lib, pu.synthetic_counts(20000, 6, zeros=0.85, seed=3), 65, 8, trace=False)


def test_sparse_balancing_list_overflow(hip_lib):
    """8000 genes, 70 % non-zero: a round of flag words lists more common non-zeros than the lane-balancing list holds -- the owners'
    fallback loop with sp_dot_row"""
    lk.sparse_stepwise(hip_lib, pu.synthetic_counts(8000, 10, zeros=0.3, seed=2), 65, 6, trace=False)


# ---- 2. verification mode ----

def test_verification_mode_stepwise(hip_lib):
    lk.sparse_stepwise(hip_lib, lk.counts_90x70(), 70, 12, **lk.SEQ)


def test_verification_mode_stepwise_dense_factors(hip_lib):
    lk.dense_factors_stepwise(hip_lib, 70, 20, **lk.SEQ)


def test_verification_mode_full_run(hip_lib, oracle):
    lk.verification_full_run(hip_lib, oracle, 20)


# ---- 3. / 5. full runs with statistics ----

def test_sparse_full_run_with_statistics(hip_lib, oracle):
    lk.full_run_with_statistics(hip_lib, oracle, pu.synthetic_counts(60, 40, zeros=0.7, seed=21), 30, True)


def test_dense_full_run_with_statistics(hip_lib, oracle):
    lk.full_run_with_statistics(hip_lib, oracle, pu.synthetic(83, 37), 30, False)


# ---- 4. launch forms above 64 patterns ----

def _state(S):
    out = []
    for w in "AP":
        a = S.atoms(w)
        out += [a["pos"], a["mass"], a["left"], a["right"], S.matrix(w), S.rows(w), np.float32(S.chisq(w)), np.uint32(S.check_domain(w))]
    return [np.ascontiguousarray(x).tobytes() for x in out]


def test_chained_launch_equals_two_launches_and_the_oracle(hip_lib, monkeypatch):
    """chain_sparse_kernel (two proposal groups per workgroup) at K = 65: a session that runs alone steps both samplers by chained
    launches and ends in the oracle's state; with COGAPS_NO_CHAIN the same chain, stepped by two launches per batch, leaves the same bits"""
    data = pu.synthetic_counts(300, 200, zeros=0.85, seed=3)
    kw = dict(nPatterns=65, seed=9, nIterations=20, sparseOptimization=True)

    def run(with_oracle):
        S, O = pu.make_pair(hip_lib, data, **kw)
        for it in range(10):
            t = min(1.0, 2.0 * it / 20)
            S.set_annealing(t), O.set_annealing(t)
            nA, nP = S.draw_steps()
            S.iterate(nA, nP)
            if with_oracle:
                assert (nA, nP) == O.draw_steps(), it
                O.iterate(nA, nP)
        if with_oracle:
            pu.assert_state_equal(S, O, "chained")
        out = _state(S), (S.chained("A"), S.chained("P")), S.natoms("A")
        S.close(), O.close()
        return out

    chained, form, n_atoms = run(True)
    assert form == (1, 1), "the sparse model's chained launch did not run"
    assert n_atoms > 100
    monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    plain, form, _ = run(False)
    assert form == (0, 0)
    assert chained == plain


def test_batched_chains_equal_single_sessions(hip_lib):
    lk.batched_chains_equal_single_sessions(hip_lib, 600, 200, 20)


# ---- 5. the dense model ----

@pytest.mark.parametrize("k", [65, 130, 300])
def test_dense_stepwise(hip_lib, k):
    pu.run_stepwise(hip_lib, pu.synthetic(83, 37), 20, trace=True, nPatterns=k, seed=9, total_iter=20, check_every=2)


# ---- 6. the limit ----

@pytest.mark.parametrize("entry", lk.SPARSE_MODEL_ENTRIES)
def test_pattern_limit_of_the_sparse_model(hip_lib, entry):
    lk.pattern_limit(hip_lib, entry)


def test_dense_model_takes_513_patterns(hip_lib):
    lk.dense_model_takes_513_patterns(hip_lib)
