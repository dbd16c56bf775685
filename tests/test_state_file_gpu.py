"""The state file on the MI355X (the product library): what tests/test_state_file.py checks on the emulator build, and what only the
hardware has -- launch forms (chained launch, two launches, batches), device-resident tensors, the verification-mode golden, the
file-size rule at a shape with a real A*P cache."""
import os

import numpy as np
import pytest

import state_file_cases as sc
from conftest import GOLDEN
from cogaps_amd import _capi
from cogaps_amd._capi import CogapsError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def datas():
    return {"dense": (sc.dense_data(), dict(sc.KW)), "sparse": (sc.sparse_data(), dict(sc.KW, sparseOptimization=True))}


@pytest.fixture(scope="module")
def references(hip_lib, datas):
    return {m: sc.uninterrupted(hip_lib, d, **kw) for m, (d, kw) in datas.items()}


@pytest.mark.parametrize("point", list(sc.SAVE_POINTS))
@pytest.mark.parametrize("model", ["dense", "sparse"])
def test_a_resumed_chain_is_the_uninterrupted_chain_on_the_gpu(hip_lib, datas, references, tmp_path, model, point):
    data, kw = datas[model]
    path = str(tmp_path / "chain.state")
    S = _capi.Session(data, lib=hip_lib, **kw)
    sc.run_to(S, sc.SAVE_POINTS[point])
    pos = S.position()
    S.save_state(path)
    want_traces, want_state = sc.traced_iterations(S), sc.stepped_state(S)
    S.close()
    T = _capi.Session(data, lib=hip_lib, **kw)
    T.load_state(path)
    assert T.position() == pos
    sc.assert_traces_equal(sc.traced_iterations(T), want_traces, model + " " + point)
    sc.assert_states_equal(sc.stepped_state(T), want_state, model + " " + point)
    T.close()
    sc.assert_results_equal(sc.resume(hip_lib, data, path, **kw), references[model], model + " " + point)


@pytest.mark.parametrize("model,what", [("dense", "uncertainty"), ("dense", "pump"), ("sparse", "snapshots"), ("dense", "fixed-P"), ("sparse", "fixed-A")])
def test_everything_that_accumulates_is_resumed_on_the_gpu(hip_lib, datas, tmp_path, model, what):
    data, kw = datas[model]
    kw = dict(kw, **{"uncertainty": {}, "pump": dict(takePumpSamples=True), "snapshots": dict(nSnapshots=4, snapshotPhase="all"),
                     "fixed-P": dict(whichMatrixFixed="P"), "fixed-A": dict(whichMatrixFixed="A")}[what])
    unc = (0.1 * data + 0.05 + 0.01 * np.random.default_rng(4).random(data.shape)).astype(np.float32) if what == "uncertainty" else None
    if what.startswith("fixed"):
        kw["fixedPatterns"] = np.random.default_rng(6).gamma(2.0, 0.5, (data.shape[1] if what == "fixed-P" else data.shape[0], 3)).astype(np.float32)
    want = sc.uninterrupted(hip_lib, data, unc=unc, **kw)
    path = str(tmp_path / "acc.state")
    sc.save_at(hip_lib, data, sc.SAVE_POINTS["mid-sampling"], path, unc=unc, **kw)
    sc.assert_results_equal(sc.resume(hip_lib, data, path, unc=unc, **kw), want, model + " " + what)


def test_verification_mode_resumed_once_in_each_phase_equals_the_golden(hip_lib, gist, tmp_path):
    """reductionMode seq + mathMode glibc-fma on GIST with the parameters of tests/golden/gist_k5_s123_i300_seq.npz: ONE chain of 300 + 300
    iterations, saved, destroyed and resumed at iteration 140 of the equilibration and again at iteration 120 of the sampling phase, gives
    the golden's arrays.  On the GPU only: 600 verification-mode iterations of GIST take the emulator minutes."""
    kw = dict(nPatterns=5, nIterations=300, seed=123, outputFrequency=30, reductionMode="seq", mathMode="glibc-fma")
    path = str(tmp_path / "seq.state")
    S = _capi.Session(gist, lib=hip_lib, **kw)
    S.run_iterations(1, 0, 140); S.save_state(path); S.close()
    S = _capi.Session(gist, lib=hip_lib, **kw)
    S.load_state(path)
    assert S.position() == (1, 140)
    S.run_iterations(1, 140, 160); S.run_iterations(2, 0, 120); S.save_state(path); S.close()
    S = _capi.Session(gist, lib=hip_lib, **kw)
    S.load_state(path)
    assert S.position() == (2, 120)
    r = S.run_to_end()
    S.close()
    g = np.load(os.path.join(GOLDEN, "gist_k5_s123_i300_seq.npz"))
    for f in ("Amean", "Pmean", "Asd", "Psd", "chisq"):
        assert np.array_equal(r[f], g[f]), f


def test_the_input_form_does_not_matter_on_the_gpu(hip_lib, datas, references, tmp_path):
    import scipy.sparse as sp
    import torch
    data, kw = datas["sparse"]
    path = str(tmp_path / "form.state")
    sc.save_at(hip_lib, data, sc.SAVE_POINTS["mid-sampling"], path, **kw)
    dm = _capi.DeviceMatrix(sp.csr_matrix(data), lib=hip_lib)
    for name, form in {"csr": sp.csr_matrix(data), "coo": sc.shuffled_triplets(data), "device matrix": dm, "device tensor": torch.from_numpy(data).cuda()}.items():
        sc.assert_results_equal(sc.resume(hip_lib, form, path, **kw), references["sparse"], name)
    idx = np.array([5, 9, 2, 64, 65, 130, 17, 33, 34, 35, 77, 1], dtype=np.uint32)
    skw = dict(kw, subsetIndices=idx, subsetDim=1)
    want = sc.uninterrupted(hip_lib, data, **skw)
    sc.save_at(hip_lib, data, sc.SAVE_POINTS["mid-equilibration"], path, **skw)
    sc.assert_results_equal(sc.resume(hip_lib, dm, path, **skw), want, "subset, device matrix")
    dm.close()
    data, kw = datas["dense"]
    sc.save_at(hip_lib, data, sc.SAVE_POINTS["mid-equilibration"], path, **kw)
    sc.assert_results_equal(sc.resume(hip_lib, torch.from_numpy(data).cuda(), path, **kw), references["dense"], "dense model, device tensor")
    sc.save_at(hip_lib, torch.from_numpy(data).cuda(), sc.SAVE_POINTS["mid-sampling"], path, **kw)
    sc.assert_results_equal(sc.resume(hip_lib, data, path, **kw), references["dense"], "dense model, saved from a device tensor")


@pytest.fixture(scope="module")
def chained_case(hip_lib):
    """a shape whose A sampler takes the chained launch (512-thread evaluation workgroups): 300 x 1600"""
    import parity_util as pu
    data = pu.synthetic(300, 1600, seed=11)
    kw = dict(nPatterns=4, nIterations=12, outputFrequency=4, seed=50)
    return data, kw, sc.uninterrupted(hip_lib, data, **kw)


@pytest.mark.parametrize("saver_chained", [True, False])
def test_the_launch_form_is_not_state(hip_lib, chained_case, tmp_path, monkeypatch, saver_chained):
    data, kw, want = chained_case
    path = str(tmp_path / "form.state")
    if not saver_chained: monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    S = _capi.Session(data, lib=hip_lib, **kw)
    sc.run_to(S, (1, 5))
    assert S.chained("A") == saver_chained
    S.save_state(path); S.close()
    if saver_chained: monkeypatch.setenv("COGAPS_NO_CHAIN", "1")
    else: monkeypatch.delenv("COGAPS_NO_CHAIN")
    T = _capi.Session(data, lib=hip_lib, **kw)
    T.load_state(path)
    T.run_iterations(1, 5, 1)
    assert T.chained("A") == (not saver_chained)
    sc.assert_results_equal(T.run_to_end(), want, "chained -> two launches" if saver_chained else "two launches -> chained")
    T.close()


def test_a_batch_member_and_a_one_chain_session_continue_each_other_on_the_gpu(hip_lib, datas, references, tmp_path):
    data, kw = datas["dense"]
    other = sc.dense_data()[::-1].copy()
    path = str(tmp_path / "b.state")
    sc.save_at(hip_lib, data, sc.SAVE_POINTS["mid-equilibration"], path, **kw)
    a, b = _capi.Session(data, lib=hip_lib, **kw), _capi.Session(other, lib=hip_lib, **dict(kw, seed=77))
    a.load_state(path)
    B = _capi.Batch([a, b])
    with pytest.raises(CogapsError, match="batch"):
        a.load_state(path)
    B.run_iterations(1, 7, sc.N_ITER - 7)
    a.save_state(path)      # a batch member, between two batch calls
    B.run_iterations(2, 0, sc.N_ITER)
    assert a.position() == (3, 0)
    sc.assert_results_equal(a.finish(), references["dense"], "one chain -> batch")
    B.close(); a.close(); b.close()
    sc.assert_results_equal(sc.resume(hip_lib, data, path, **kw), references["dense"], "batch member -> one chain")


def test_capacity_is_not_state_on_the_gpu(hip_lib, datas, tmp_path, monkeypatch):
    data, kw = datas["dense"]
    kw = dict(kw, alphaA=0.05, alphaP=0.05)      # (107 atoms in A at the save point)
    want = sc.uninterrupted(hip_lib, data, **kw)
    path = str(tmp_path / "cap.state")
    for small_saver in (True, False):
        if small_saver: monkeypatch.setenv("COGAPS_INITIAL_ATOM_CAP", "64")
        else: monkeypatch.delenv("COGAPS_INITIAL_ATOM_CAP", raising=False)
        S = _capi.Session(data, lib=hip_lib, **kw)
        sc.run_to(S, sc.SAVE_POINTS["mid-sampling"])
        assert S.natoms("A") > 64
        S.save_state(path); S.close()
        if small_saver: monkeypatch.delenv("COGAPS_INITIAL_ATOM_CAP")
        else: monkeypatch.setenv("COGAPS_INITIAL_ATOM_CAP", "64")
        sc.assert_results_equal(sc.resume(hip_lib, data, path, **kw), want, "small saver" if small_saver else "small loader")


def test_refused_loads_leave_the_session_untouched_on_the_gpu(hip_lib, datas, references, tmp_path):
    data, kw = datas["dense"]
    good = str(tmp_path / "good.state")
    sc.save_at(hip_lib, data, sc.SAVE_POINTS["mid-sampling"], good, **kw)
    T = _capi.Session(data, lib=hip_lib, **kw)
    T.run_iterations(1, 0, 4)
    for name, (path, says) in sc.corrupt_copies(good, str(tmp_path)).items():
        with pytest.raises(CogapsError, match=says):
            T.load_state(path)
    ulp = data.copy(); ulp[17, 5] = np.nextafter(ulp[17, 5], np.float32(np.inf))
    assert T.position() == (1, 4)
    sc.assert_results_equal(T.run_to_end(), references["dense"], "after four refused files")
    T.close()
    for name, (d, k) in {"seed": (data, dict(kw, seed=6)), "nPatterns": (data, dict(kw, nPatterns=4)), "nIterations": (data, dict(kw, nIterations=sc.N_ITER + 1)),
                         "data digest": (ulp, kw), "model": (data, dict(kw, sparseOptimization=True))}.items():
        T = _capi.Session(d, lib=hip_lib, **k)
        with pytest.raises(CogapsError, match=name + ".* differs"):
            T.load_state(good)
        T.close()


def test_file_size(hip_lib, tmp_path):
    """dense 1024 x 768, K = 3, after 10 iterations: one A*P array and everything else fit where two arrays would; the sparse model at
    90 % zeros holds no array of the matrix's size at all"""
    d = sc.sparse_data(1024, 768, zeros=0.9, seed=8)
    for sparse, limit in ((False, 2 * 4 * 1024 * 768), (True, 4 * 1024 * 768)):
        path = str(tmp_path / ("size%d.state" % sparse))
        S = _capi.Session(d + (0 if sparse else 0.5), lib=hip_lib, nPatterns=3, nIterations=10, seed=3, sparseOptimization=sparse)
        S.run_iterations(1, 0, 10)
        S.save_state(path)
        S.close()
        size = os.path.getsize(path)
        print("state file, %s model, 1024 x 768: %d bytes (limit %d)" % ("sparse" if sparse else "dense", size, limit))
        assert size < limit


def test_data_digest_on_the_gpu(hip_lib):
    import scipy.sparse as sp
    import torch
    for genes, samples in ((40, 1), (40, 5), (3000, 700)):      # (3000 x 700: 2048 workgroups, every thread goes round four times)
        d = sc.sparse_data(genes, samples, zeros=0.7, seed=genes + samples)
        d[0, 0] = 3.0
        kw = dict(nPatterns=1 if samples == 1 else 2, nIterations=4, seed=1)
        for model in ("dense", "sparse"):
            k = dict(kw, sparseOptimization=(model == "sparse"))
            S = _capi.Session(d, lib=hip_lib, **k)
            want = S.data_digest()
            assert S.data_digest() == want and want != 0
            S.close()
            changed = d.copy(); changed[0, 0] = np.nextafter(np.float32(3.0), np.float32(4.0))
            forms = [changed, torch.from_numpy(d).cuda()] + ([sp.csr_matrix(d), sc.shuffled_triplets(d)] if model == "sparse" else [])
            for i, form in enumerate(forms):
                S = _capi.Session(form, lib=hip_lib, **k)
                assert (S.data_digest() == want) == (i > 0), (model, genes, samples, i)
                S.close()
