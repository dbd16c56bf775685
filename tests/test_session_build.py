"""Session building (csrc/session_build.h) on the TEST-ONLY workgroup emulator: every input form of both models -- dense host, dense
"device" pointer, CSR, CSC, triplets with a repeated position, a device-matrix handle -- with and without transposeData and subsetData,
each pinned to constants (the data digest, the session's device bytes, the samplers' dimensions, the factor matrices after two
iterations), and every refusal of session_create's argument checks as a whole string.  Routes that denote the same matrix share one
constant, so they agree with each other.  A wrong copy of the rule "which axis does the subset pick, which axis are the vectors"
(Matrix.cpp:30-69, GapsRunner.cpp:402-406) builds a valid session of the wrong matrix: these constants are what it moves.
test_gpu_parity.py runs the same table on the hardware."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from cogaps_amd import _capi

K = 3
SHAPES = [(70, 9), (9, 70)]      # a 70-element vector has two 64-bit flag words, a 9-element vector one
TILED = (70, 66)                 # the dense device build's column-tile kernel (DNB_TILE = 64): two tiles each way
SUBSET_ROUTES = ("dense_host", "dense_device", "sparse_host", "sparse_device", "device_matrix")
PLAIN_ROUTES = ("csr", "csc", "coo")      # these take no subsetData
SUBSETS = ("none", "genes", "samples")


def matrix(shape):
    """about 60 % zeros, the rest counts 1 .. 9 scaled by a non-dyadic factor"""
    rng = np.random.default_rng(100 * shape[0] + shape[1])
    d = (np.ceil(rng.random(shape) * 9) * np.float32(1.3)).astype(np.float32) * (rng.random(shape) >= 0.6)
    assert 0.5 < (d == 0).mean() < 0.7
    return np.ascontiguousarray(d, dtype=np.float32)


def subset_indices(dim):
    """five 1-based indices, out of order, one of them repeated"""
    return np.array([dim // 2, 2, dim, 2, dim // 4 + 1], dtype=np.uint32)


def subset_kw(shape, transpose, subset):
    """genes are the rows of the data unless transposeData"""
    if subset == "none":
        return {}
    dim = shape[0] if (subset == "genes") != bool(transpose) else shape[1]
    return dict(subsetIndices=subset_indices(dim), subsetDim=1 if subset == "genes" else 2)


def triplets(d):
    """the entries > 0 in a shuffled order; the first position once more in front with another value (the later entry decides)"""
    r, c = np.nonzero(d > 0)
    order = np.random.default_rng(5).permutation(r.size)
    r, c = r[order], c[order]
    return _capi.CooMatrix(d.shape, np.concatenate([r[:1], r]), np.concatenate([c[:1], c]), np.concatenate([[np.float32(77.5)], d[r, c]]))


def compressed(d, major_is_row):
    m = d if major_is_row else d.T
    counts = (m > 0).sum(axis=1)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    r, c = np.nonzero(m > 0)
    return _capi.SparseMatrix(d.shape, major_is_row, indptr, c.astype(np.uint32), np.ascontiguousarray(m[r, c], dtype=np.float32))


def host_pointers(d):
    """a "device" array on the emulator, where device addresses are host addresses"""
    return _capi.DeviceDense(d.shape, d.ctypes.data, keep=(d,))


def cases():
    out = []
    for shape in SHAPES:
        for transpose in (0, 1):
            for route in SUBSET_ROUTES:
                out += [(route, shape, transpose, sub) for sub in SUBSETS]
            out += [(route, shape, transpose, "none") for route in PLAIN_ROUTES]
    return out + [("dense_device", TILED, 0, "none")]


def case_id(case):
    return "%s-%dx%d-t%d-%s" % (case[0], case[1][0], case[1][1], case[2], case[3])


def measure(lib, case, dd=host_pointers):
    """(data digest, device bytes, dims of A, dims of P, digest of the factor matrices after two iterations) of the case's session"""
    route, shape, transpose, subset = case
    d = matrix(shape)
    kw = dict(lib=lib, nPatterns=K, seed=11, nIterations=10, transposeData=bool(transpose), sparseOptimization=not route.startswith("dense"),
              **subset_kw(shape, transpose, subset))
    dm = None
    if route in ("dense_host", "sparse_host"): src = d
    elif route in ("dense_device", "sparse_device"): src = dd(d)
    elif route == "csr": src = compressed(d, True)
    elif route == "csc": src = compressed(d, False)
    elif route == "coo": src = triplets(d)
    else: src = dm = _capi.DeviceMatrix(compressed(d, True), lib=lib)
    S = _capi.Session(src, **kw)
    got = [S.data_digest(), S.device_bytes(), S.dims("A"), S.dims("P")]
    S.run_iterations(1, 0, 2)
    got.append(hashlib.sha256(S.matrix("A").tobytes() + S.matrix("P").tobytes()).hexdigest()[:16])
    S.close()
    if dm is not None: dm.close()
    return tuple(got)


def expected(case):
    route, shape, transpose, subset = case
    return EXPECTED[("dense" if route.startswith("dense") else "sparse", shape, transpose, subset)]


# (model, shape, transposeData, subsetData) -> what measure() gives for every route of that model: taken on the emulator from the
# sources before csrc/session_build.h existed, at the product's generator window (the device bytes hold the generator's jump tables, whose
# length follows the window); the MI355X gives the same (test_gpu_parity.py)
EXPECTED = {
    ('dense', (70, 9), 0, 'none'): (0xd8f4f762d3901fee, 12538428, (70, 9, 3), (9, 70, 3), '3edbf9de49d2840e'),
    ('dense', (70, 9), 0, 'genes'): (0x1b6abb9454295238, 12433248, (5, 9, 3), (9, 5, 3), '026c220f0a041936'),
    ('dense', (70, 9), 0, 'samples'): (0x2f4067abda3b1bf6, 12526188, (70, 5, 3), (5, 70, 3), '0acf877d3ce4a47c'),
    ('sparse', (70, 9), 0, 'none'): (0x76277f99d7b8c7ab, 12525448, (70, 9, 3), (9, 70, 3), '9ed39b258a443c7e'),
    ('sparse', (70, 9), 0, 'genes'): (0x6090bdbfdbcc4dcc, 12432392, (5, 9, 3), (9, 5, 3), '026c220f0a041936'),
    ('sparse', (70, 9), 0, 'samples'): (0x1cd501f4e6768e73, 12518808, (70, 5, 3), (5, 70, 3), 'cb43a8f90df8cf07'),
    ('dense', (70, 9), 1, 'none'): (0xb104883d11030228, 12537696, (9, 70, 3), (70, 9, 3), '3f1e3b2c2bfa6860'),
    ('dense', (70, 9), 1, 'genes'): (0x7bc05fc5ac8b761e, 12525408, (5, 70, 3), (70, 5, 3), '01cf548d82ed8a54'),
    ('dense', (70, 9), 1, 'samples'): (0x15668b51d34bfc12, 12433296, (9, 5, 3), (5, 9, 3), 'cc7506b977cd07c8'),
    ('sparse', (70, 9), 1, 'none'): (0x0a00f792a17287c1, 12524716, (9, 70, 3), (70, 9, 3), '6bc1f993ee297058'),
    ('sparse', (70, 9), 1, 'genes'): (0x64fbfcc048ad7a45, 12518028, (5, 70, 3), (70, 5, 3), '7ecef8c3c26a122e'),
    ('sparse', (70, 9), 1, 'samples'): (0x408a1a67b2a9ea2a, 12432440, (9, 5, 3), (5, 9, 3), 'cc7506b977cd07c8'),
    ('dense', (9, 70), 0, 'none'): (0xf79ed2492cf88dec, 12537696, (9, 70, 3), (70, 9, 3), 'c31b7aec74cc248f'),
    ('dense', (9, 70), 0, 'genes'): (0xfd8154783d1163ad, 12525408, (5, 70, 3), (70, 5, 3), '7532e6cf0e4701d1'),
    ('dense', (9, 70), 0, 'samples'): (0x5066c270c0685074, 12433296, (9, 5, 3), (5, 9, 3), '84e1efac0bc70302'),
    ('sparse', (9, 70), 0, 'none'): (0xc57c5c731360883c, 12524612, (9, 70, 3), (70, 9, 3), 'c31b7aec74cc248f'),
    ('sparse', (9, 70), 0, 'genes'): (0x55fb449cdf9cfff4, 12518092, (5, 70, 3), (70, 5, 3), 'e72828402d5aa942'),
    ('sparse', (9, 70), 0, 'samples'): (0x0ce3220b0accbbeb, 12432440, (9, 5, 3), (5, 9, 3), '84e1efac0bc70302'),
    ('dense', (9, 70), 1, 'none'): (0x6e1628ed28ce80f9, 12538428, (70, 9, 3), (9, 70, 3), 'e677639194f8e6fb'),
    ('dense', (9, 70), 1, 'genes'): (0x301bfc1f9db097ad, 12433248, (5, 9, 3), (9, 5, 3), 'aadbbbfb6a51c1f8'),
    ('dense', (9, 70), 1, 'samples'): (0x7dd4b4daf56855a3, 12526188, (70, 5, 3), (5, 70, 3), '0fc763d7c79bb88a'),
    ('sparse', (9, 70), 1, 'none'): (0xc68ad3d94803baf0, 12525344, (70, 9, 3), (9, 70, 3), '7f73cfb157d41a2a'),
    ('sparse', (9, 70), 1, 'genes'): (0xe7e3af01ff8432e4, 12432392, (5, 9, 3), (9, 5, 3), 'aadbbbfb6a51c1f8'),
    ('sparse', (9, 70), 1, 'samples'): (0x2f2a791f0d91f2da, 12518872, (70, 5, 3), (5, 70, 3), '89686eac7396b6d6'),
    ('dense', (70, 66), 0, 'none'): (0x4dc3dfbf07a3a32a, 12711996, (70, 66, 3), (66, 70, 3), '4680b8cae855a409'),
}


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_route(emul_lib, case):
    got = measure(emul_lib(), case)
    print(case_id(case), got)
    assert got == expected(case)


def test_routes_that_denote_the_same_matrix_share_a_constant():
    """every route of a model is held to one entry of EXPECTED, and every entry is used"""
    used = {}
    for case in cases():
        used.setdefault(("dense" if case[0].startswith("dense") else "sparse",) + case[1:], []).append(case[0])
    assert set(used) == set(EXPECTED)
    for key, routes in used.items():
        if key[1] == TILED: continue
        assert len(routes) == (2 if key[0] == "dense" else 3 + (3 if key[3] == "none" else 0)), key
    # the same matrix under the two models: one shape of samplers
    for (model, shape, transpose, subset), v in EXPECTED.items():
        if model == "dense" and shape != TILED:
            assert v[2:4] == EXPECTED[("sparse", shape, transpose, subset)][2:4]


# ---- session_create's refusals ----

def refusal(lib, src, tweak=None, params=True, **kw):
    """the library's message for a creation that must fail: src a dense array, a DeviceDense, a SparseMatrix, a CooMatrix or a DeviceMatrix"""
    p = _capi.make_params(lib, **dict(dict(nPatterns=K, seed=1), **kw))
    if tweak: tweak(p)
    pp = C.byref(p) if params else None
    if isinstance(src, np.ndarray): h = lib.cogaps_session_create(src.ctypes.data, src.shape[0], src.shape[1], pp, None, 0)
    elif isinstance(src, _capi.DeviceDense): h = lib.cogaps_session_create(src.data_addr, src.shape[0], src.shape[1], pp, None, 1)
    elif isinstance(src, _capi.DeviceMatrix): h = lib.cogaps_session_create_from_device_matrix(src._handle(), pp)
    else:
        m = src.c_struct()
        h = getattr(lib, "cogaps_session_create_coo" if isinstance(src, _capi.CooMatrix) else "cogaps_session_create_sparse")(C.byref(m), pp)
    assert not h
    return lib.cogaps_last_error().decode()


D = matrix((70, 9))
SP = dict(sparseOptimization=True)
SUB = dict(subsetIndices=subset_indices(9), subsetDim=2)


def set_field(name, value):
    return lambda p: setattr(p, name, value)


def index_case(transpose, dim_is_genes, index, bound):
    idx = np.array([1, index], dtype=np.uint32)
    return (lambda lib: D, dict(transposeData=transpose, subsetIndices=idx, subsetDim=1 if dim_is_genes else 2), None,
            "dataIndicesSubset holds an index outside 1 .. %d" % bound)


# name -> (source, keywords, tweak of the parameters, the message): each fails one check alone
REFUSALS = {
    "sparse_needs_the_sparse_model": (lambda lib: compressed(D, True), {}, None,
                                      "a compressed-sparse matrix needs useSparseOptimization = 1 (the dense model takes a dense matrix)"),
    "sparse_with_subset": (lambda lib: compressed(D, True), dict(SP, **SUB), None,
                           "subsetData is not supported with a compressed-sparse matrix: pass the rows / columns of the subset"),
    "sparse_with_seq": (lambda lib: compressed(D, True), dict(SP, reductionMode="seq"), None,
                        "reductionMode COGAPS_REDUCE_SEQ is not supported with a compressed-sparse matrix"),
    "coo_needs_the_sparse_model": (lambda lib: triplets(D), {}, None, "a triplet matrix needs useSparseOptimization = 1 (the dense model takes a dense matrix)"),
    "coo_with_subset": (lambda lib: triplets(D), dict(SP, **SUB), None, "subsetData is not supported with a triplet matrix: pass the entries of the subset"),
    "coo_with_seq": (lambda lib: triplets(D), dict(SP, reductionMode="seq"), None, "reductionMode COGAPS_REDUCE_SEQ is not supported with a triplet matrix"),
    "device_matrix_needs_the_sparse_model": (lambda lib: _capi.DeviceMatrix(compressed(D, True), lib=lib), {}, None,
                                             "a device-resident matrix needs useSparseOptimization = 1 (the dense model takes a dense matrix)"),
    "device_matrix_on_another_device": (lambda lib: _capi.DeviceMatrix(compressed(D, True), lib=lib), dict(SP, device=5), None,
                                        "params->device must be -1 or the device the matrix resides on (0)"),
    "null_data": (lambda lib: _capi.DeviceDense(D.shape, 0), {}, None, "null argument: data"),
    "null_indptr": (lambda lib: _capi.SparseMatrix(D.shape, True, 0, 0, 0, on_device=True), SP, None, "null argument: indptr"),
    "coo_too_many_entries": (lambda lib: _capi.CooMatrix(D.shape, 0, 0, 0, on_device=True, nnz=2 ** 32 - 1), SP, None,
                             "triplet matrix: 2^32 - 1 entries or more (entries and packed values are indexed by 32 bits)"),
    "coo_null_arrays": (lambda lib: _capi.CooMatrix(D.shape, 0, 0, 0, on_device=True, nnz=3), SP, None, "null argument: rows / cols / values"),
    "synchronous_updates": (lambda lib: D, dict(asynchronousUpdates=False), None,
                            "asynchronousUpdates=FALSE (SingleThreadedGibbsSampler) is not part of this library"),
    "unknown_sampler": (lambda lib: D, dict(sampler=7), None, "sampler must be COGAPS_SAMPLER_ASYNC or COGAPS_SAMPLER_SEQUENTIAL"),
    "sequential_sparse": (lambda lib: D, dict(SP, sampler="sequential"), None,
                          "sampler = COGAPS_SAMPLER_SEQUENTIAL supports the dense model only: the SparseNormalModel evaluation of the sequential kernel is missing "
                          "(useSparseOptimization must be 0)"),
    "no_patterns": (lambda lib: D, dict(nPatterns=0), None, "empty problem"),
    "no_rows": (lambda lib: D[:0], {}, None, "empty problem"),
    "no_columns": (lambda lib: np.zeros((4, 0), dtype=np.float32), {}, None, "empty problem"),
    "fixed_matrix_letter": (lambda lib: D, dict(whichMatrixFixed="X"), None, "whichMatrixFixed must be 'N', 'A' or 'P'"),
    "reduction_mode": (lambda lib: D, dict(reductionMode=5), None, "reductionMode must be COGAPS_REDUCE_LANES or COGAPS_REDUCE_SEQ"),
    "math_mode": (lambda lib: D, dict(mathMode=9, reductionMode="seq"), None, "mathMode must be COGAPS_MATH_PORTABLE, _GLIBC_FMA or _GLIBC_SSE2"),
    "math_mode_without_seq": (lambda lib: D, dict(mathMode="glibc-fma"), None,
                              "mathMode other than COGAPS_MATH_PORTABLE needs reductionMode COGAPS_REDUCE_SEQ (the verification mode)"),
    "pump_threshold": (lambda lib: D, dict(pumpThreshold=2), None, "pumpThreshold must be 0 (PUMP_UNIQUE) or 1 (PUMP_CUT)"),
    "fixed_patterns_columns": (lambda lib: D, dict(whichMatrixFixed="P", fixedPatterns=np.ones((9, K), dtype=np.float32)), set_field("fixedCols", K + 1),
                               "fixedPatterns must have nPatterns columns"),
    "empty_subset": (lambda lib: D, SUB, set_field("nSubset", 0), "dataIndicesSubset is empty"),
    # the bound of the index check is the subset's input axis: 70 x 9, genes are the rows unless transposeData
    "index_genes": index_case(False, True, 71, 70),
    "index_samples": index_case(False, False, 10, 9),
    "index_genes_transposed": index_case(True, True, 10, 9),
    "index_samples_transposed": index_case(True, False, 71, 70),
    "index_zero": index_case(False, True, 0, 70),
}
# arguments that fail two checks: the first in the order of the checks is reported
TWO_REFUSALS = {
    "sparse_model_before_subset": (lambda lib: compressed(D, True), SUB, None,
                                   "a compressed-sparse matrix needs useSparseOptimization = 1 (the dense model takes a dense matrix)"),
    "synchronous_before_empty": (lambda lib: D, dict(asynchronousUpdates=False, nPatterns=0), None,
                                 "asynchronousUpdates=FALSE (SingleThreadedGibbsSampler) is not part of this library"),
    "math_mode_range_before_its_reduction": (lambda lib: D, dict(mathMode=9), None, "mathMode must be COGAPS_MATH_PORTABLE, _GLIBC_FMA or _GLIBC_SSE2"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS) + sorted(TWO_REFUSALS))
def test_refusal(emul_lib, name):
    lib = emul_lib()
    make, kw, tweak, message = (REFUSALS.get(name) or TWO_REFUSALS[name])
    src = make(lib)
    got = refusal(lib, src, tweak, **kw)
    if isinstance(src, _capi.DeviceMatrix): src.close()
    assert got == message


def test_null_params(emul_lib):
    lib = emul_lib()
    assert refusal(lib, D, params=False) == "null argument"
    assert refusal(lib, compressed(D, True), params=False) == "null argument"
