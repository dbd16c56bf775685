"""The library's own state file (cogaps_session_save_state / _load_state / _run_to_end, include/cogaps_hip.h): a chain saved between two
iterations and loaded into a fresh session made from the same data is the uninterrupted chain, bit for bit.  The emulator build compiles
the library's own host file and kernels, so the whole feature -- file format, fingerprint, digest kernel, front end -- runs here without
a GPU; tests/test_state_file_gpu.py repeats it on the product library and adds what only the hardware has (launch forms, device tensors,
the verification-mode golden, the file-size shapes)."""
import os
import stat

import numpy as np
import pytest

import state_file_cases as sc
from cogaps_amd import _capi
from cogaps_amd._capi import CogapsError


@pytest.fixture(scope="module")
def lib(emul_lib):
    return emul_lib(256)


@pytest.fixture(scope="module")
def datas():
    return {"dense": (sc.dense_data(), dict(sc.KW)), "sparse": (sc.sparse_data(), dict(sc.KW, sparseOptimization=True))}


@pytest.fixture(scope="module")
def references(lib, datas):
    """the uninterrupted runs, computed once"""
    return {m: sc.uninterrupted(lib, d, **kw) for m, (d, kw) in datas.items()}


@pytest.mark.parametrize("point", list(sc.SAVE_POINTS))
@pytest.mark.parametrize("model", ["dense", "sparse"])
def test_a_resumed_chain_is_the_uninterrupted_chain(lib, datas, references, tmp_path, model, point):
    data, kw = datas[model]
    path = str(tmp_path / "chain.state")
    S = _capi.Session(data, lib=lib, **kw)
    sc.run_to(S, sc.SAVE_POINTS[point])
    pos = S.position()
    if point == "mid-equilibration":
        assert pos == (1, 7) and 2.0 * 7 / sc.N_ITER < 1.0      # the annealing temperature is still below 1
    assert pos == {"mid-equilibration": (1, 7), "phase-boundary": (2, 0), "mid-sampling": (2, 9)}[point]
    S.save_state(path)
    # the saving session goes on by hand: it is the uninterrupted chain of the next two iterations
    want_traces = sc.traced_iterations(S)
    want_state = sc.stepped_state(S)
    S.close()
    T = _capi.Session(data, lib=lib, **kw)
    T.load_state(path)
    assert T.position() == pos
    sc.assert_traces_equal(sc.traced_iterations(T), want_traces, model + " " + point)
    sc.assert_states_equal(sc.stepped_state(T), want_state, model + " " + point)
    T.close()
    sc.assert_results_equal(sc.resume(lib, data, path, **kw), references[model], model + " " + point)


ACCUMULATING = {
    "uncertainty": dict(), "pump": dict(takePumpSamples=True), "snapshots": dict(nSnapshots=4, snapshotPhase="all"),
    "fixed-P": dict(whichMatrixFixed="P"), "fixed-A": dict(whichMatrixFixed="A"),
}


@pytest.mark.parametrize("model,what", [("dense", w) for w in ACCUMULATING] + [("sparse", w) for w in ACCUMULATING if w != "uncertainty"])      # (the sparse model takes no uncertainty matrix)
def test_everything_that_accumulates_is_resumed(lib, datas, tmp_path, model, what):
    data, kw = datas[model]
    kw = dict(kw, **ACCUMULATING[what])
    unc = None
    if what == "uncertainty":
        unc = (0.1 * data + 0.05 + 0.01 * np.random.default_rng(4).random(data.shape)).astype(np.float32)
    if what.startswith("fixed"):
        rows = data.shape[1] if what == "fixed-P" else data.shape[0]
        kw["fixedPatterns"] = np.random.default_rng(6).gamma(2.0, 0.5, (rows, 3)).astype(np.float32)
    want = sc.uninterrupted(lib, data, unc=unc, **kw)
    path = str(tmp_path / "acc.state")
    assert sc.save_at(lib, data, sc.SAVE_POINTS["mid-sampling"], path, unc=unc, **kw) == (2, 9)
    got = sc.resume(lib, data, path, unc=unc, **kw)
    sc.assert_results_equal(got, want, model + " " + what)
    if what == "pump":
        assert got["pumpMatrix"].any()
    if what == "snapshots":
        assert got["equilibrationSnapshotsA"].shape[0] == 4 and got["samplingSnapshotsP"].shape[0] == 4


def test_the_input_form_does_not_matter(lib, datas, references, tmp_path):
    import scipy.sparse as sp
    data, kw = datas["sparse"]
    path = str(tmp_path / "form.state")
    sc.save_at(lib, data, sc.SAVE_POINTS["mid-sampling"], path, **kw)
    dm = _capi.DeviceMatrix(sp.csr_matrix(data), lib=lib)
    forms = {"csr": sp.csr_matrix(data), "coo": sc.shuffled_triplets(data), "device matrix": dm}
    assert np.array_equal(forms["coo"].toarray(), data)
    for name, form in forms.items():
        sc.assert_results_equal(sc.resume(lib, form, path, **kw), references["sparse"], name)
    # a subset session (a distributed worker's call), saved from the dense input, loaded from the device-resident matrix and back
    idx = np.array([5, 9, 2, 64, 65, 130, 17, 33, 34, 35, 77, 1], dtype=np.uint32)
    skw = dict(kw, subsetIndices=idx, subsetDim=1)
    want = sc.uninterrupted(lib, data, **skw)
    sc.save_at(lib, data, sc.SAVE_POINTS["mid-equilibration"], path, **skw)
    sc.assert_results_equal(sc.resume(lib, dm, path, **skw), want, "subset, device matrix")
    sc.save_at(lib, dm, sc.SAVE_POINTS["mid-sampling"], path, **skw)
    sc.assert_results_equal(sc.resume(lib, data, path, **skw), want, "subset, numpy")
    dm.close()
    # ... and the dense model's subset
    data, kw = datas["dense"]
    skw = dict(kw, subsetIndices=np.array([3, 1, 30, 31, 12, 8, 22], dtype=np.uint32), subsetDim=2)
    want = sc.uninterrupted(lib, data, **skw)
    sc.save_at(lib, data, sc.SAVE_POINTS["mid-sampling"], path, **skw)
    sc.assert_results_equal(sc.resume(lib, data, path, **skw), want, "dense subset")


def test_capacity_is_not_state(lib, datas, tmp_path, monkeypatch):
    """the chain holds more than 64 atoms at the save point: saved from a session that started with room for 64 and grew, loaded into
    a default session -- and the other way round, where the load has to grow first"""
    data, kw = datas["dense"]
    kw = dict(kw, alphaA=0.05, alphaP=0.05)      # (107 atoms in A, 58 in P at the save point)
    want = sc.uninterrupted(lib, data, **kw)
    path = str(tmp_path / "cap.state")
    for small_saver in (True, False):
        if small_saver: monkeypatch.setenv("COGAPS_INITIAL_ATOM_CAP", "64")
        else: monkeypatch.delenv("COGAPS_INITIAL_ATOM_CAP", raising=False)
        S = _capi.Session(data, lib=lib, **kw)
        sc.run_to(S, sc.SAVE_POINTS["mid-sampling"])
        assert S.natoms("A") > 64
        S.save_state(path); S.close()
        if small_saver: monkeypatch.delenv("COGAPS_INITIAL_ATOM_CAP")
        else: monkeypatch.setenv("COGAPS_INITIAL_ATOM_CAP", "64")
        sc.assert_results_equal(sc.resume(lib, data, path, **kw), want, "small saver" if small_saver else "small loader")


def test_a_batch_member_and_a_one_chain_session_continue_each_other(lib, datas, references, tmp_path):
    data, kw = datas["dense"]
    other = sc.dense_data()[::-1].copy()
    path = str(tmp_path / "b.state")
    # one chain alone -> two sessions of a batch (the second chain is another one)
    sc.save_at(lib, data, sc.SAVE_POINTS["mid-equilibration"], path, **kw)
    a, b = _capi.Session(data, lib=lib, **kw), _capi.Session(other, lib=lib, **dict(kw, seed=77))
    a.load_state(path)
    B = _capi.Batch([a, b])
    with pytest.raises(CogapsError, match="batch"):
        a.load_state(path)
    B.run_iterations(1, 7, sc.N_ITER - 7)
    assert a.position() == (2, 0)
    # ... saved as a batch member between two batch calls, resumed as a one-chain session
    a.save_state(path)
    B.run_iterations(2, 0, sc.N_ITER)
    assert a.position() == (3, 0)
    sc.assert_results_equal(a.finish(), references["dense"], "one chain -> batch")
    B.close(); a.close(); b.close()
    sc.assert_results_equal(sc.resume(lib, data, path, **kw), references["dense"], "batch member -> one chain")


def test_refused_loads_leave_the_session_untouched(lib, datas, references, tmp_path):
    data, kw = datas["dense"]
    good = str(tmp_path / "good.state")
    sc.save_at(lib, data, sc.SAVE_POINTS["mid-sampling"], good, **kw)
    T = _capi.Session(data, lib=lib, **kw)
    T.run_iterations(1, 0, 4)
    for name, (path, says) in sc.corrupt_copies(good, str(tmp_path)).items():
        with pytest.raises(CogapsError, match=says):
            T.load_state(path)
    with pytest.raises(CogapsError, match="cannot read"):
        T.load_state(str(tmp_path / "missing.state"))
    assert T.position() == (1, 4)
    sc.assert_results_equal(T.run_to_end(), references["dense"], "after four refused files")
    T.close()
    # sessions that differ from the file's in exactly one fingerprint item
    ulp = data.copy(); ulp[17, 5] = np.nextafter(ulp[17, 5], np.float32(np.inf))
    others = {
        "seed": (data, dict(kw, seed=6)), "nPatterns": (data, dict(kw, nPatterns=4)), "nIterations": (data, dict(kw, nIterations=sc.N_ITER + 1)),
        "data digest": (ulp, kw), "model": (data, dict(kw, sparseOptimization=True)),
    }
    for name, (d, k) in others.items():
        U = _capi.Session(d, lib=lib, **k)
        U.run_iterations(1, 0, 6)
        T = _capi.Session(d, lib=lib, **k)
        T.run_iterations(1, 0, 3)
        with pytest.raises(CogapsError, match=name + ".* differs"):
            T.load_state(good)
        assert T.position() == (1, 3)
        T.run_iterations(1, 3, 3)
        sc.assert_states_equal(sc.stepped_state(T), sc.stepped_state(U), "after a refused load: " + name)
        T.close(); U.close()


def test_a_failed_save_leaves_the_previous_file_loadable(lib, datas, references, tmp_path):
    if os.geteuid() == 0:
        pytest.skip("root writes into a read-only directory")
    data, kw = datas["dense"]
    d = tmp_path / "ro"
    d.mkdir()
    good = str(d / "run.state")
    sc.save_at(lib, data, sc.SAVE_POINTS["mid-equilibration"], good, **kw)
    before = open(good, "rb").read()
    S = _capi.Session(data, lib=lib, **kw)
    S.run_iterations(1, 0, 3)
    os.chmod(str(d), stat.S_IRUSR | stat.S_IXUSR)
    try:
        with pytest.raises(CogapsError, match="cannot write"):
            S.save_state(good)
    finally:
        os.chmod(str(d), stat.S_IRWXU)
    S.close()
    assert open(good, "rb").read() == before and os.listdir(str(d)) == ["run.state"]
    sc.assert_results_equal(sc.resume(lib, data, good, **kw), references["dense"], "the old file")


def assert_front_end_equal(got, want, tag):
    for f in ("featureLoadings", "loadingStdDev", "sampleFactors", "factorStdDev"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), tag + ": " + f
    assert got.metadata["meanChiSq"] == want.metadata["meanChiSq"], tag
    for k, v in want.metadata["diagnostics"].items():
        if k != "totalRunningTime":
            assert np.array_equal(np.asarray(got.metadata["diagnostics"][k]), np.asarray(v)), tag + ": " + k


def test_front_end(lib, datas, references, tmp_path, monkeypatch):
    from cogaps_amd import CoGAPS, CogapsParams, checkpointsEnabled
    from cogaps_amd.api import check_inputs
    monkeypatch.setattr(_capi, "load", lambda: lib)
    data, kw = datas["dense"]
    params = CogapsParams(nPatterns=3, nIterations=sc.N_ITER, seed=5)
    plain = CoGAPS(data, params, messages=False, outputFrequency=5)
    path = str(tmp_path / "fe.state")
    with_file = CoGAPS(data, params, messages=False, outputFrequency=5, stateFile=path, stateInterval=7)
    assert_front_end_equal(with_file, plain, "with a state file")
    T = _capi.Session(data, lib=lib, **kw)
    T.load_state(path)
    assert T.position() == (3, 0)      # complete
    sc.assert_results_equal(T.run_to_end(), references["dense"], "a complete state finishes at once")
    T.close()
    # the interrupt hook raised at iteration 13: the 14th poll (equilibration)
    polls = [0]

    def hook():
        polls[0] += 1
        return polls[0] == 14
    S = _capi.Session(data, lib=lib, interrupt=hook, **kw)
    with pytest.raises(CogapsError, match="interrupted"):
        S.run_to_end(path, 0)
    assert S.position() == (1, 13)
    S.close()
    T = _capi.Session(data, lib=lib, **kw)
    T.load_state(path)
    assert T.position() == (1, 13)
    T.close()
    resumed = CoGAPS(data, params, messages=False, outputFrequency=5, stateFile=path, resume=True)
    assert_front_end_equal(resumed, plain, "resumed behind the interrupt")
    # resume without a file: from the start
    fresh = str(tmp_path / "none.state")
    again = CoGAPS(data, params, messages=False, outputFrequency=5, stateFile=fresh, resume=True)
    assert_front_end_equal(again, plain, "resume without a file")
    assert os.path.exists(fresh)
    # _capi.run without a state file is the one C call it was
    sc.assert_results_equal(_capi.run(data, lib=lib, **kw), references["dense"], "cogaps_run")
    sc.assert_results_equal(_capi.run(data, lib=lib, stateFile=fresh, resume=True, **kw), references["dense"], "a complete file, resumed")
    # the distributed drivers take no state file yet
    dist = CogapsParams(nPatterns=3, nIterations=sc.N_ITER, seed=5, distributed="genome-wide")
    for extra in (dict(stateFile=path), dict(stateFile=path, stateInterval=5), dict(stateFile=path, resume=True)):
        with pytest.raises(ValueError, match="distributed drivers do not take a state file"):
            CoGAPS(data, dist, messages=False, **extra)
    # the reference's checkpoints stay what they were: another notion
    assert lib.cogaps_checkpoints_enabled() == 0 and checkpointsEnabled() is False
    with pytest.raises(ValueError, match="checkpoints"):
        check_inputs(data, None, params, checkpointInFile="x")
    with pytest.raises(ValueError, match="checkpoints"):
        CoGAPS(data, params, messages=False, checkpointInFile=path)


def test_data_digest(lib):
    """equal for every input form of a matrix and for repeated calls, different when one element changes; N = 1 and N = 5 samples, and a
    shape whose threads go round their grid-stride loop more than once (a workgroup per 1024 elements: four rounds at 300 x 70)"""
    import scipy.sparse as sp
    for genes, samples in ((40, 1), (40, 5), (300, 70)):
        d = sc.sparse_data(genes, samples, zeros=0.7, seed=genes + samples)
        d[0, 0] = 3.0
        kw = dict(nPatterns=1 if samples == 1 else 2, nIterations=4, seed=1)
        digests = {}
        for model in ("dense", "sparse"):
            k = dict(kw, sparseOptimization=(model == "sparse"))
            S = _capi.Session(d, lib=lib, **k)
            digests[model] = S.data_digest()
            assert S.data_digest() == digests[model] and digests[model] != 0
            S.close()
            changed = d.copy(); changed[0, 0] = np.nextafter(np.float32(3.0), np.float32(4.0))
            S = _capi.Session(changed, lib=lib, **k)
            assert S.data_digest() != digests[model], (model, genes, samples)
            S.close()
        for form in (sp.csr_matrix(d), sp.csc_matrix(d), sc.shuffled_triplets(d)):
            S = _capi.Session(form, lib=lib, **dict(kw, sparseOptimization=True))
            assert S.data_digest() == digests["sparse"]
            S.close()
        dm = _capi.DeviceMatrix(sp.csr_matrix(d), lib=lib)
        S = _capi.Session(dm, lib=lib, **dict(kw, sparseOptimization=True))
        assert S.data_digest() == digests["sparse"]
        S.close(); dm.close()
