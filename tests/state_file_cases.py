"""Shared by tests/test_state_file.py (the emulator build, no GPU) and tests/test_state_file_gpu.py (the product library): data,
comparisons and the save / destroy / create / load / continue cycle of the state-file tests.  "Equal" is np.array_equal / == throughout."""
import os

import numpy as np

from cogaps_amd import _capi
import parity_util as pu

TIME_FIELDS = ("totalRunningTime", "samplerSeconds")      # the only result fields a resumed run may differ in
N_ITER = 20
KW = dict(nPatterns=3, nIterations=N_ITER, outputFrequency=5, seed=5)
# (phase, iterations of that phase done): mid-equilibration (annealing temperature 0.7), the phase boundary, mid-sampling
SAVE_POINTS = {"mid-equilibration": (1, 7), "phase-boundary": (1, N_ITER), "mid-sampling": (2, 9)}


def dense_data():
    """61 x 37: neither a multiple of 4 (live pads) nor of 64"""
    return np.random.default_rng(1).gamma(2.0, 1.0, (61, 37)).astype(np.float32)


def sparse_data(genes=130, samples=70, zeros=0.8, seed=2):
    """count-like, 80 % zeros, 130 x 70: the flag words' tails are live"""
    rng = np.random.default_rng(seed)
    return (np.ceil(rng.gamma(2.0, 1.5, (genes, samples))) * (rng.random((genes, samples)) >= zeros)).astype(np.float32)


def assert_results_equal(got, want, tag=""):
    assert set(got) == set(want), tag
    for k in want:
        if k not in TIME_FIELDS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), "%s: result field %s differs" % (tag, k)


def stepped_state(S):
    out = {}
    for w in "AP":
        a = S.atoms(w)
        out[w] = dict(matrix=S.matrix(w), rows=S.rows(w), ap=S.ap(w), pos=a["pos"], mass=a["mass"], left=a["left"], right=a["right"],
                      natoms=S.natoms(w), chisq=S.chisq(w), avg_queue=S.avg_queue(w), violations=S.check_domain(w))
    return out


def assert_states_equal(a, b, tag=""):
    for w in "AP":
        assert a[w]["violations"] == 0 and b[w]["violations"] == 0, "%s %s: check_domain" % (tag, w)
        for k in a[w]:
            assert np.array_equal(np.asarray(a[w][k]), np.asarray(b[w][k])), "%s: %s of sampler %s differs" % (tag, k, w)


def run_to(S, point):
    """a fresh session up to a save point"""
    phase, done = point
    n = int(S.p.nIterations)
    S.run_iterations(1, 0, n if phase == 2 else done)
    if phase == 2:
        S.run_iterations(2, 0, done)


def traced_iterations(S, count=2, cap=4096):
    """the next `count` iterations from the session's position, stepped by hand with proposal traces (no fixed matrix); the position
    itself is the caller's book from here on"""
    phase, it = S.position()
    n = int(S.p.nIterations)
    out = []
    for _ in range(count):
        if phase > 2:
            break
        if phase == 1:
            S.set_annealing(float(min(np.float32(1.0), np.float32(2 * it) / np.float32(n))))
        nA, nP = S.draw_steps()
        ta = S.update("A", nA, trace_cap=cap); S.sync("P")
        tp = S.update("P", nP, trace_cap=cap); S.sync("A")
        out.append((nA, nP, ta, tp))
        it += 1
        if it == n:
            phase, it = phase + 1, 0
    return out


def assert_traces_equal(a, b, tag=""):
    assert len(a) == len(b), tag
    for k, ((nA, nP, ta, tp), (mA, mP, ua, up)) in enumerate(zip(a, b)):
        assert (nA, nP) == (mA, mP), "%s: step counts of iteration +%d differ" % (tag, k)
        for w, t, u in (("A", ta, ua), ("P", tp, up)):
            pu.assert_trace_equal(t, u, "%s: iteration +%d, sampler %s" % (tag, k, w))


def save_at(lib, data, point, path, unc=None, **kw):
    """a session run to the save point, saved, destroyed; returns the saved position"""
    S = _capi.Session(data, unc=unc, lib=lib, **kw)
    run_to(S, point)
    pos = S.position()
    S.save_state(path)
    S.close()
    return pos


def resume(lib, data, path, unc=None, **kw):
    """a fresh session from `data`, the state loaded, run to its end"""
    T = _capi.Session(data, unc=unc, lib=lib, **kw)
    try:
        T.load_state(path)
        return T.run_to_end()
    finally:
        T.close()


def uninterrupted(lib, data, unc=None, **kw):
    S = _capi.Session(data, unc=unc, lib=lib, **kw)
    try:
        return S.run_to_end()
    finally:
        S.close()


def shuffled_triplets(d, seed=3):
    """the matrix as unordered triplets with repeated positions: stale earlier entries (other values, some not > 0) before the deciding ones"""
    rng = np.random.default_rng(seed)
    r, c = np.nonzero(d)
    v = d[r, c]
    order = rng.permutation(r.size)
    r, c, v = r[order], c[order], v[order]
    k = r.size // 5
    stale_v = np.where(rng.random(k) < 0.5, v[:k] + 1.0, 0.0).astype(np.float32)
    return _capi.CooMatrix(d.shape, np.concatenate([r[:k], r]), np.concatenate([c[:k], c]), np.concatenate([stale_v, v]))


def corrupt_copies(good, tmp):
    """four bad files from one good one: {name: (path, what the message must say)}"""
    raw = open(good, "rb").read()
    out = {}

    def put(name, data, says):
        p = os.path.join(tmp, name + ".state")
        open(p, "wb").write(data)
        out[name] = (p, says)
    put("truncated", raw[:len(raw) // 2], "truncated")
    flipped = bytearray(raw); flipped[len(raw) - 100] ^= 0x10
    put("flipped", bytes(flipped), "checksum")
    put("magic", b"XXXXXXXX" + raw[8:], "magic")
    newer = bytearray(raw); newer[8:12] = (int.from_bytes(raw[8:12], "little") + 1).to_bytes(4, "little")
    put("newer", bytes(newer), "newer")
    return out
