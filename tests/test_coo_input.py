"""Triplet (COO) and Matrix Market input of the sparse model (cogaps_session_create_coo, cogaps_read_mtx_triplets, the second half of
csrc/sparse_build.h) on the test-only emulator build.  Triplets denote D = 0; D[rows[k], cols[k]] = values[k] in input order -- the
latest entry of a position decides it -- and a session created from them is the session created from that dense D, bit for bit:
structure by structure against the dense-input session and against the definition of the structures in numpy
(parity_util.packed_reference: the dense-input session goes through the same device build as the compressed one), step by step
against the oracle, and through the file route and the front ends."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

import parity_util as pu
from cogaps_amd import _capi
from parity_util import assert_structures_equal, structures
from test_sparse_input import SHAPES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GIST = os.path.join(GOLDEN, "GIST.mtx")
RESULT_FIELDS = ("Amean", "Asd", "Pmean", "Psd", "chisq", "atomsA", "atomsP")


def densify(shape, rows, cols, values):
    """the matrix the triplets denote, by the definition: an explicit loop in input order"""
    d = np.zeros(shape, dtype=np.float32)
    for r, c, v in zip(rows, cols, values):
        d[r, c] = v
    return d


def shuffled_triplets(data, seed, repeats=0.0):
    """the entries > 0 of `data` as triplets in a shuffled order.  repeats: that fraction of ALL positions (present or not) also gets one
    or two earlier entries of other values, and the absent ones among them a closing explicit zero -- the triplets still denote `data`"""
    rng = np.random.default_rng(seed)
    r, c = np.nonzero(data)
    v = data[r, c]
    key = rng.random(r.size)
    if repeats:
        n = int(round(repeats * data.size))
        pos = rng.choice(data.size, n, replace=False)
        pr, pc = np.unravel_index(pos, data.shape)
        # the deciding entry of each picked position: its own if it is present, an explicit zero otherwise
        final_key = np.empty(n)
        present = data[pr, pc] > 0
        lookup = {(a, b): k for a, b, k in zip(r.tolist(), c.tolist(), key.tolist())}
        for i in range(n):
            final_key[i] = lookup[(int(pr[i]), int(pc[i]))] if present[i] else rng.random()
        zr, zc, zk = pr[~present], pc[~present], final_key[~present]
        # decoys: before the deciding entry in input order (a smaller key), positive, zero or negative
        twice = rng.random(n) < 0.3
        dr, dc = np.concatenate([pr, pr[twice]]), np.concatenate([pc, pc[twice]])
        dk = np.concatenate([final_key, final_key[twice]]) * rng.random(dr.size)
        dv = rng.choice(np.array([0.0, -2.0, 1.0, 3.0, 7.5], dtype=np.float32), dr.size)
        r, c = np.concatenate([r, zr, dr]), np.concatenate([c, zc, dc])
        v = np.concatenate([v, np.zeros(zr.size, dtype=np.float32), dv])
        key = np.concatenate([key, zk, dk])
    order = np.argsort(key, kind="stable")
    return r[order].astype(np.uint32), c[order].astype(np.uint32), v[order].astype(np.float32)


def coo_of(data, seed, repeats=0.0):
    r, c, v = shuffled_triplets(data, seed, repeats)
    return _capi.CooMatrix(data.shape, r, c, v)


def assert_same_session_as_dense(lib, shape, rows, cols, values, **kw):
    """the session from the triplets against the dense-input session of the loop-built matrix, and both against the numpy packer's
    structures of that matrix; returns the dense-input session's structures"""
    kw = dict(dict(lib=lib, nPatterns=2, seed=3, sparseOptimization=True), **kw)
    dense = densify(shape, rows, cols, values)
    D, S = _capi.Session(dense, **kw), _capi.Session(_capi.CooMatrix(shape, rows, cols, values), **kw)
    d = structures(D)
    assert_structures_equal(d, structures(S))
    ref = pu.packed_reference(dense, kw["nPatterns"], transposeData=kw.get("transposeData", False))
    assert_structures_equal(ref, d, "dense input")
    assert_structures_equal(ref, structures(S), "triplet input")
    for w in "AP":
        assert np.float32(D.chisq(w)).tobytes() == np.float32(S.chisq(w)).tobytes()
    D.close(), S.close()
    return d, dense


def run_stepwise_coo(lib, oracle, coo, dense, n_iter, trace=True, total_iter=None, **kw):
    """the loop of test_sparse_input.run_stepwise_sparse for a session created from triplets (the oracle gets the dense matrix)"""
    total_iter = total_iter or max(n_iter, 2)
    kw.setdefault("nIterations", total_iter)
    S = _capi.Session(coo, lib=lib, **kw)
    wA, wP = lib.cogaps_reduction_width(S.dims("A")[1]), lib.cogaps_reduction_width(S.dims("P")[1])
    O = oracle.Session(dense, math_mode=oracle.MATH_PORTABLE, redW_A=wA, redW_P=wP, redG=4, **kw)
    for it in range(n_iter):
        t = min(1.0, 2.0 * it / total_iter)
        S.set_annealing(t), O.set_annealing(t)
        nA, nP = S.draw_steps()
        assert (nA, nP) == O.draw_steps(), "Poisson step counts differ at iteration %d" % it
        if trace:
            pu.assert_trace_equal(S.update("A", nA, 1 << 16), O.update("A", nA, 1 << 16), "it%d A" % it)
            S.sync("P"), O.sync("P")
            pu.assert_trace_equal(S.update("P", nP, 1 << 16), O.update("P", nP, 1 << 16), "it%d P" % it)
            S.sync("A"), O.sync("A")
        else:
            S.iterate(nA, nP), O.iterate(nA, nP)
        pu.assert_state_equal(S, O, "it%d" % it)
    S.close(), O.close()


# ---- 1. structures equal the dense-input session ----

@pytest.mark.parametrize("transpose", [False, True])
def test_structures_equal_the_dense_input_session(emul_lib, transpose):
    lib = emul_lib(256)
    data = pu.synthetic_counts(400, 330, zeros=0.85, seed=12)
    if transpose:
        data = np.ascontiguousarray(data.T)
    kw = dict(lib=lib, nPatterns=5, seed=2, sparseOptimization=True, transposeData=transpose)
    D, C = _capi.Session(data, **kw), _capi.Session(sp.csr_matrix(data), **kw)
    d = structures(D)
    ref = pu.packed_reference(data, 5, transposeData=transpose)
    assert_structures_equal(ref, d, "dense input")
    assert_structures_equal(ref, structures(C), "CSR input")
    assert d["A"]["flags"].shape[1] > 1 and d["P"]["flags"].shape[1] > 1 and d["A"]["vals"].size >= 10000
    orders = []
    for seed in (1, 2):
        m = coo_of(data, seed)
        orders.append(m.rows.copy())
        assert np.array_equal(densify(data.shape, m.rows, m.cols, m.values), data)
        S = _capi.Session(m, **kw)
        assert_structures_equal(d, structures(S), "shuffle %d" % seed)
        assert_structures_equal(ref, structures(S), "triplet input, shuffle %d" % seed)
        for w in "AP":
            assert D.chisq(w) == S.chisq(w)
        assert S.device_bytes() == C.device_bytes() == D.device_bytes()
        S.close()
    assert not np.array_equal(orders[0], orders[1])
    D.close(), C.close()


# ---- 2. repeated positions ----

def _base(shape, seed, zeros=0.7):
    data = pu.synthetic_counts(shape[0], shape[1], zeros=zeros, seed=seed)
    r, c, v = shuffled_triplets(data, seed)
    return data, list(r), list(c), list(v)


def _case_last_not_positive(bad):
    data, r, c, v = _base((70, 130), 5)
    taken = np.argwhere(data > 0)[:3]
    free = np.argwhere(data == 0)[:3]
    for (i, j) in list(taken) + list(free):      # a position the base holds, and one it does not: positive first, then the bad value
        r += [i, i]; c += [j, j]; v += [5.0, bad]
    return (70, 130), r, c, v


def _case_last_positive(bad):
    data, r, c, v = _base((70, 130), 6)
    free = np.argwhere(data == 0)[:4]
    for (i, j) in free:
        r += [i, i]; c += [j, j]; v += [bad, 4.0]
    return (70, 130), r, c, v


def _case_three_and_five_times():
    data, r, c, v = _base((70, 130), 7)
    i, j = np.argwhere(data == 0)[0]
    k, l = np.argwhere(data > 0)[10]
    # spread through the input; (i, j) ends at 2.0, (k, l) ends at 0: absent although the base holds it
    for n, val in enumerate((9.0, 0.0, 2.0)):
        at = 50 + 400 * n
        r.insert(at, i); c.insert(at, j); v.insert(at, val)
    r += [k] * 5; c += [l] * 5; v += [1.0, 6.0, -1.0, 3.0, 0.0]
    return (70, 130), r, c, v


def _case_far_apart():
    data, r, c, v = _base((70, 130), 8, zeros=0.4)
    assert len(r) > 2400
    free = np.argwhere(data == 0)
    for n, gap in enumerate((70, 300, 1100)):      # another wave, another workgroup, another round of the grid
        i, j = free[n]
        first = 10 + n
        r.insert(first, i); c.insert(first, j); v.insert(first, 8.0)
        r.insert(first + gap, i); c.insert(first + gap, j); v.insert(first + gap, 2.0 + n)
        i, j = free[10 + n]                         # ... and with the earlier entry the larger value and the later one zero
        r.insert(first + 1200, i); c.insert(first + 1200, j); v.insert(first + 1200, 8.0)
        r.insert(first + 1200 + gap, i); c.insert(first + 1200 + gap, j); v.insert(first + 1200 + gap, 0.0)
    return (70, 130), r, c, v


def _case_every_entry_at_one_position(last):
    n = 700
    v = list(np.random.default_rng(9).integers(0, 9, n).astype(np.float32))
    v[-1] = last
    return (40, 70), [3] * n, [66] * n, v


def _case_sixty_four_in_one_flag_word():
    data, r, c, v = _base((70, 130), 10)
    rng = np.random.default_rng(10)
    er, ec, ev = [], [], []
    for j in range(64, 128):                        # row 5, columns 64 .. 127: one flag word of sampler A's vector 5
        er += [5, 5]; ec += [j, j]; ev += [float(rng.integers(0, 5)), float(rng.integers(0, 5))]
    for j in range(64):                             # column 7, rows 0 .. 63: one flag word of sampler P's vector 7
        er += [j, j]; ec += [7, 7]; ev += [float(rng.integers(0, 5)), float(rng.integers(0, 5))]
    order = rng.permutation(len(er))
    at = rng.integers(0, len(r), len(er))
    for o, a in zip(order, at):
        r.insert(a, er[o]); c.insert(a, ec[o]); v.insert(a, ev[o])
    return (70, 130), r, c, v


def _case_last_element_of_128(shape):
    data, r, c, v = _base(shape, 11)
    lr, lc = shape[0] - 1, shape[1] - 1
    for i in range(0, shape[0], 7):
        r += [i, i]; c += [lc, lc]; v += [0.0, 3.0]
    for j in range(0, shape[1], 5):
        r += [lr, lr]; c += [j, j]; v += [6.0, 0.0 if j % 2 else 2.0]
    return shape, r, c, v


def _case_zero_row_and_column():
    data, r, c, v = _base((90, 128), 4)
    # row 17 and column 64: every entry the base holds there is followed by a zero, and a few positions get a zero only
    for k in range(len(r)):
        if r[k] == 17 or c[k] == 64:
            r.append(r[k]); c.append(c[k]); v.append(0.0)
    r += [17, 17, 3]; c += [0, 127, 64]; v += [0.0, -1.0, 0.0]
    return (90, 128), r, c, v


REPEAT_CASES = {
    "positive_then_zero": lambda: _case_last_not_positive(0.0),
    "positive_then_negative": lambda: _case_last_not_positive(-3.0),
    "positive_then_nan": lambda: _case_last_not_positive(np.nan),
    "zero_then_positive": lambda: _case_last_positive(0.0),
    "negative_then_positive": lambda: _case_last_positive(-3.0),
    "nan_then_positive": lambda: _case_last_positive(np.nan),
    "three_and_five_times": _case_three_and_five_times,
    "far_apart": _case_far_apart,
    "all_at_one_position_present": lambda: _case_every_entry_at_one_position(4.0),
    "all_at_one_position_absent": lambda: _case_every_entry_at_one_position(0.0),
    "sixty_four_in_one_flag_word": _case_sixty_four_in_one_flag_word,
    "last_element_of_128_columns": lambda: _case_last_element_of_128((90, 128)),
    "last_element_of_128_rows": lambda: _case_last_element_of_128((128, 90)),
    "zero_row_and_column": _case_zero_row_and_column,
}


@pytest.mark.parametrize("case", sorted(REPEAT_CASES))
def test_repeated_positions(emul_lib, case):
    shape, r, c, v = REPEAT_CASES[case]()
    r, c, v = np.asarray(r, dtype=np.uint32), np.asarray(c, dtype=np.uint32), np.asarray(v, dtype=np.float32)
    d, dense = assert_same_session_as_dense(emul_lib(256), shape, r, c, v)
    kept = int((dense > 0).sum())
    assert d["A"]["vals"].size == kept == d["P"]["vals"].size
    if case == "zero_row_and_column":
        assert not (dense[17] > 0).any() and not (dense[:, 64] > 0).any() and kept > 100
    if case == "all_at_one_position_present":
        assert kept == 1 and d["A"]["vals"][0] == 4.0
    if case == "all_at_one_position_absent":
        assert kept == 0
    if case.startswith("positive_then"):
        assert kept == int((pu.synthetic_counts(70, 130, zeros=0.7, seed=5) > 0).sum()) - 3


# ---- 3. step by step against the oracle ----

@pytest.mark.parametrize("genes,samples,k,iters,zeros,win", [SHAPES[0], SHAPES[4]])
def test_coo_input_stepwise(emul_lib, oracle, genes, samples, k, iters, zeros, win):
    data = pu.synthetic_counts(genes, samples, zeros=zeros, seed=genes + samples)
    m = coo_of(data, 3, repeats=0.05)
    assert m.nnz > int((data > 0).sum()) + int(0.04 * data.size)
    assert np.array_equal(densify(data.shape, m.rows, m.cols, m.values), data)
    run_stepwise_coo(emul_lib(win), oracle, m, data, iters, trace=True, nPatterns=k, seed=11, total_iter=max(iters, 40), sparseOptimization=True)


# ---- 4. errors ----

GOOD = dict(shape=(3, 4), rows=[0, 2, 1, 0, 2], cols=[0, 2, 1, 3, 2], values=[1, 2, 3, 4, 5])
KW = dict(nPatterns=2, seed=1, sparseOptimization=True)


def _refused(lib, match, kwargs=KW, **change):
    with pytest.raises(_capi.CogapsError, match=match):
        _capi.Session(_capi.CooMatrix(**dict(GOOD, **change)), lib=lib, **kwargs)
    S = _capi.Session(_capi.CooMatrix(**GOOD), lib=lib, **KW)      # the process goes on: a valid session afterwards
    assert S.debug_sparse_data("A")["vals"].size == 4
    S.close()


def test_error_dense_model(emul_lib):
    _refused(emul_lib(256), "needs useSparseOptimization", kwargs=dict(KW, sparseOptimization=False))


def test_error_subset_data(emul_lib):
    _refused(emul_lib(256), "subsetData is not supported with a triplet matrix", kwargs=dict(KW, subsetIndices=np.array([1, 2], dtype=np.uint32), subsetDim=1))


def test_error_reduce_seq(emul_lib):
    _refused(emul_lib(256), "COGAPS_REDUCE_SEQ is not supported with a triplet matrix", kwargs=dict(KW, reductionMode="seq"))


@pytest.mark.parametrize("field", ["rows", "cols", "values"])
def test_error_null_array(emul_lib, field):
    lib = emul_lib(256)
    p = _capi.make_params(lib, **KW)
    m = _capi.CooMatrix(**GOOD)
    c = m.c_struct()
    setattr(c, field, None)
    assert not lib.cogaps_session_create_coo(ctypes.byref(c), ctypes.byref(p))
    assert b"null argument: rows / cols / values" in lib.cogaps_last_error()
    r = _capi.CogapsResultC()
    assert lib.cogaps_run_coo(ctypes.byref(c), ctypes.byref(p), ctypes.byref(r)) == 1
    assert not lib.cogaps_session_create_coo(None, ctypes.byref(p)) and b"null" in lib.cogaps_last_error()
    assert not lib.cogaps_session_create_coo(ctypes.byref(m.c_struct()), None) and b"null" in lib.cogaps_last_error()
    c.nnz = 0                                     # no entries: the arrays are not looked at, the matrix is empty and well formed
    h = lib.cogaps_session_create_coo(ctypes.byref(c), ctypes.byref(p))
    assert h
    lib.cogaps_session_destroy(h)
    _capi.Session(m, lib=lib, **KW).close()


@pytest.mark.parametrize("change", [dict(rows=[0, 3, 1, 0, 2]), dict(cols=[0, 2, 1, 4, 2]), dict(rows=[0, 2, 1, 0, 0xFFFFFFFF]),
                                    dict(shape=(3, 3))])
def test_error_index_out_of_range(emul_lib, change):
    _refused(emul_lib(256), "index is outside the stated dimensions", **change)


def test_error_too_many_entries(emul_lib):
    """nnz >= 2^32 - 1 is refused before any of the arrays is read (they hold five entries here)"""
    lib = emul_lib(256)
    p = _capi.make_params(lib, **KW)
    m = _capi.CooMatrix(**GOOD)
    for nnz in (0xFFFFFFFF, 1 << 40):
        c = m.c_struct()
        c.nnz = nnz
        assert not lib.cogaps_session_create_coo(ctypes.byref(c), ctypes.byref(p))
        assert b"2^32 - 1 entries or more" in lib.cogaps_last_error()
    _capi.Session(m, lib=lib, **KW).close()


# ---- 5. files ----

MESSY = """%%MatrixMarket matrix coordinate real general
% a comment
%another
7 5 14
1 1 1.5
2 3 2e2

3 3 4.25e-1
7 5 9
\t
2 3 1.25
5 2 0
6 4 3.5e0
6 4 0
1 1 7
4 1 -2e-3
3 5 12
  4   4    6.5
7 1 1e1
2 2 0.0
"""


def _same_as_dense_read(lib, path, **sub):
    t = _capi.read_mtx_triplets(path, lib=lib, **sub)
    d = _capi.read_matrix_file(path, lib=lib, **sub)
    assert t.shape == d.shape and t.rows.dtype == np.uint32 and t.values.dtype == np.float32
    assert densify(t.shape, t.rows, t.cols, t.values).tobytes() == d.tobytes()
    assert t.toarray().tobytes() == d.tobytes()
    return t, d


def test_triplet_reader_equals_the_dense_reader(emul_lib, tmp_path):
    lib = emul_lib(256)
    t, d = _same_as_dense_read(lib, GIST)
    assert t.shape == (1363, 9) and t.nnz == 12267
    path = str(tmp_path / "messy.mtx")
    with open(path, "w") as f:
        f.write(MESSY)
    t, d = _same_as_dense_read(lib, path)
    assert t.nnz == 14 and d[1, 2] == np.float32(1.25) and d[5, 3] == 0 and d[0, 0] == 7 and d[1, 1] == 0
    assert abs(float(d[2, 2]) - 0.425) < 1e-6 and d[1, 2] != 200 and abs(float(d[3, 0]) + 0.002) < 1e-8
    # file order, 0-based
    assert list(t.rows[:4]) == [0, 1, 2, 6] and list(t.cols[:4]) == [0, 2, 2, 4]
    # subsets: unsorted and duplicated 1-based indices (sorted by the reader; a duplicate fills its first position only)
    for sub in (dict(rows=[6, 2, 2, 1]), dict(cols=[5, 3, 3, 1]), dict(rows=[7]), dict(cols=[4, 2])):
        ts, ds = _same_as_dense_read(lib, path, **sub)
        assert ds.shape == ((len(sub["rows"]), 5) if "rows" in sub else (7, len(sub["cols"])))
    for sub in (dict(rows=[900, 3, 3, 1363, 1]), dict(cols=[9, 2, 2])):
        _same_as_dense_read(lib, GIST, **sub)
    # the messages of the dense reader
    for text, msg in (("% only comments\n", "Invalid MTX file"), ("2 2 1\n3 1 5\n", "MTX entry outside the stated dimensions"),
                      ("2 2 1\n1 1 abc\n", "Invalid entry found in input data: abc")):
        with open(path, "w") as f:
            f.write(text)
        for read in (_capi.read_mtx_triplets, _capi.read_matrix_file):
            with pytest.raises(_capi.CogapsError, match=msg):
                read(path, lib=lib)
    with open(path, "w") as f:
        f.write(MESSY)
    for read in (_capi.read_mtx_triplets, _capi.read_matrix_file):
        with pytest.raises(_capi.CogapsError, match="subset index outside the file's dimensions"):
            read(path, lib=lib, rows=[1, 8])
    with pytest.raises(_capi.CogapsError, match="Matrix Market"):
        _capi.read_mtx_triplets(os.path.join(GOLDEN, "GIST.csv"), lib=lib)


def test_file_route_equals_the_run_on_the_dense_read(emul_lib, tmp_path, monkeypatch):
    from cogaps_amd import CoGAPS, api, io
    lib = emul_lib(256)
    kw = dict(nPatterns=3, nIterations=6, seed=7, outputFrequency=2, sparseOptimization=True)
    dense = _capi.read_matrix_file(GIST, lib=lib)
    want = _capi.run(dense, lib=lib, **kw)
    got = _capi.run_from_file(GIST, lib=lib, **kw)
    for f in RESULT_FIELDS:
        assert np.array_equal(got[f], want[f]), f
    assert got["meanChiSq"] == want["meanChiSq"] and got["totalUpdates"] == want["totalUpdates"]
    # a subset (a distributed worker's call): taken by the triplet reader, as the dense reader takes it
    idx = np.array([9, 2, 5, 7, 1], dtype=np.uint32)
    sub = _capi.run(_capi.read_matrix_file(GIST, lib=lib, cols=idx), lib=lib, **kw)
    got = _capi.run_from_file(GIST, lib=lib, subsetIndices=idx, subsetDim=2, **kw)
    for f in RESULT_FIELDS:
        assert np.array_equal(got[f], sub[f]), f
    assert got["meanChiSq"] == sub["meanChiSq"]
    # a file with repeated positions and explicit zeros
    path = str(tmp_path / "messy.mtx")
    with open(path, "w") as f:
        f.write(MESSY)
    small = dict(kw, nPatterns=2)
    a, b = _capi.run_from_file(path, lib=lib, **small), _capi.run(_capi.read_matrix_file(path, lib=lib), lib=lib, **small)
    for f in RESULT_FIELDS:
        assert np.array_equal(a[f], b[f]), f
    assert a["meanChiSq"] == b["meanChiSq"]
    # the front end: through the library's triplet reader, never io.read_matrix
    monkeypatch.setattr(_capi, "load", lambda: lib)

    def no_dense_read(*a, **k):
        raise AssertionError("the .mtx + sparseOptimization route must not read the file densely")
    monkeypatch.setattr(api, "read_matrix", no_dense_read)
    monkeypatch.setattr(io, "read_matrix", no_dense_read)
    r = CoGAPS(GIST, messages=False, **kw)
    for mine, f in ((r.featureLoadings, "Amean"), (r.loadingStdDev, "Asd"), (r.sampleFactors, "Pmean"), (r.factorStdDev, "Psd"),
                    (r.metadata["diagnostics"]["chisq"], "chisq"), (r.metadata["diagnostics"]["atomsA"], "atomsA"), (r.metadata["diagnostics"]["atomsP"], "atomsP")):
        assert np.array_equal(mine, want[f]), f
    assert r.metadata["meanChiSq"] == want["meanChiSq"]
    with pytest.raises(ValueError, match="nPatterns must be less"):
        CoGAPS(GIST, messages=False, **dict(kw, nPatterns=9))
    with pytest.raises(AssertionError, match="must not read the file densely"):      # every other call keeps its path
        CoGAPS(GIST, messages=False, **dict(kw, sparseOptimization=False))


def test_tocsr_resolves_repeats_as_the_library_does(emul_lib):
    """CooMatrix.tocsr (what a distributed run from an .mtx path hands to the shard code): the CSR form of the loop-built matrix"""
    shape, r, c, v = _case_three_and_five_times()
    m = _capi.CooMatrix(shape, r, c, v)
    dense = densify(shape, m.rows, m.cols, m.values)
    csr = m.tocsr()
    assert csr.has_canonical_format and np.array_equal(csr.toarray(), np.where(dense > 0, dense, 0)) and csr.nnz == int((dense > 0).sum())
    kw = dict(lib=emul_lib(256), nPatterns=2, seed=3, sparseOptimization=True)
    A, B = _capi.Session(m, **kw), _capi.Session(csr, **kw)
    assert_structures_equal(structures(A), structures(B))
    assert A.device_bytes() == B.device_bytes()
    A.close(), B.close()


# ---- 6. a batch ----

def test_a_triplet_and_a_csr_session_in_a_batch_equal_the_two_alone(emul_lib):
    lib = emul_lib(256)
    d0, d1 = pu.synthetic_counts(120, 40, zeros=0.8, seed=40), pu.synthetic_counts(120, 40, zeros=0.75, seed=41)
    datas = [coo_of(d0, 1, repeats=0.03), sp.csr_matrix(d1)]
    kws = [dict(seed=5), dict(seed=6)]
    common = dict(nPatterns=3, nIterations=20, outputFrequency=5, sparseOptimization=True)
    both = _capi.run_batch(datas, lib=lib, kws=kws, **common)
    for d, k, b in zip((d0, d1), kws, both):
        one = _capi.run(d, lib=lib, **common, **k)
        for f in RESULT_FIELDS:
            assert np.array_equal(one[f], b[f]), f
        assert one["totalUpdates"] == b["totalUpdates"] and one["meanChiSq"] == b["meanChiSq"]
    alone = _capi.run(datas[0], lib=lib, **common, **kws[0])
    assert np.array_equal(alone["Amean"], both[0]["Amean"]) and alone["meanChiSq"] == both[0]["meanChiSq"]


# ---- the front end: a worker's subset, and the distributed drivers, from an .mtx path ----

def _assert_same_result(a, b):
    for f in ("featureLoadings", "loadingStdDev", "sampleFactors", "factorStdDev"):
        assert getattr(a, f).shape == getattr(b, f).shape and np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("chisq", "atomsA", "atomsP"):
        assert np.array_equal(a.metadata["diagnostics"][f], b.metadata["diagnostics"][f]), f
    assert a.metadata["meanChiSq"] == b.metadata["meanChiSq"]


@pytest.mark.parametrize("dim,indices", [(1, np.arange(2, 62)), (2, np.array([1, 3, 4, 6, 7, 9]))])
def test_front_end_subset_from_an_mtx_path(emul_lib, monkeypatch, dim, indices):
    """CoGAPS(path, subsetIndices=..., subsetDim=...) -- a distributed worker's call -- with the sparse model: the run on the dense read
    with the same subset.  Ascending indices are taken by the triplet reader (no dense read); indices in another order keep the dense
    route, whose subset keeps the order given"""
    from cogaps_amd import CoGAPS, api, io
    lib = emul_lib(256)
    monkeypatch.setattr(_capi, "load", lambda: lib)
    dense = io.read_matrix(GIST)
    kw = dict(nPatterns=3, nIterations=6, seed=7, outputFrequency=2, sparseOptimization=True, messages=False, subsetDim=dim)
    want = CoGAPS(dense, subsetIndices=indices, **kw)
    assert want.featureLoadings.shape[0] == (60 if dim == 1 else 1363) and want.sampleFactors.shape[0] == (9 if dim == 1 else 6)
    shuffled = indices[::-1].copy()
    want_shuffled = CoGAPS(dense, subsetIndices=shuffled, **kw)
    _assert_same_result(CoGAPS(GIST, subsetIndices=shuffled, **kw), want_shuffled)
    reads = []
    monkeypatch.setattr(api, "read_matrix", lambda *a, **k: reads.append(a) or io.read_matrix(*a, **k))
    _assert_same_result(CoGAPS(GIST, subsetIndices=indices, **kw), want)
    assert not reads
    with pytest.raises(_capi.CogapsError, match="outside 1"):      # the dense route's message for an index outside the matrix
        CoGAPS(GIST, subsetIndices=np.array([1, 2, 3, 4, 5000]), **kw)
    assert len(reads) == 1


@pytest.mark.parametrize("driver", ["genome-wide", "single-cell"])
def test_distributed_run_from_an_mtx_path(emul_lib, monkeypatch, tmp_path, driver):
    """GWCoGAPS / scCoGAPS from an .mtx path with the sparse model: triplets, repeats resolved on the host, a scipy CSR to the shard code
    -- the run from the scipy CSR of the dense read"""
    from cogaps_amd import CoGAPS, CogapsParams, api
    lib = emul_lib(256)
    monkeypatch.setattr(_capi, "load", lambda: lib)
    data = pu.synthetic_counts(90, 48, zeros=0.6, seed=17)
    r, c, v = shuffled_triplets(data, 5, repeats=0.05)
    v = np.where(v < 0, 0, v)                     # (the front end checks every triplet value: no negative one, overwritten or not)
    path = str(tmp_path / "d.mtx")
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (data.shape + (r.size,)))
        f.write("".join("%d %d %g\n" % (i + 1, j + 1, x) for i, j, x in zip(r, c, v)))
    assert np.array_equal(_capi.read_matrix_file(path, lib=lib), data)
    p = CogapsParams(nPatterns=3, seed=5, nIterations=12, sparseOptimization=True)
    p.distributed = driver
    p.setDistributedParams(nSets=2, minNS=2)

    def no_dense_read(*a, **k):
        raise AssertionError("the .mtx + sparseOptimization route must not read the file densely")
    monkeypatch.setattr(api, "read_matrix", no_dense_read)
    a, b = CoGAPS(path, p, messages=False, outputFrequency=4), CoGAPS(sp.csr_matrix(data), p, messages=False, outputFrequency=4)
    for f in ("featureLoadings", "loadingStdDev", "sampleFactors", "factorStdDev"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.featureLoadings.shape == (90, 3) and (a.featureLoadings.any() or a.sampleFactors.any())
    assert np.array_equal(a.metadata["meanChiSq"], b.metadata["meanChiSq"])
