"""ctypes view of include/cogaps_hip.h.

`load()` returns the product library (libcogaps_hip.so, HIP/gfx950).  It fails loudly when the
library has not been built: there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libcogaps_hip.so")

INTERRUPT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)


class CogapsParamsC(C.Structure):
    _fields_ = [
        ("seed", C.c_uint32), ("nPatterns", C.c_uint32), ("nIterations", C.c_uint32),
        ("maxThreads", C.c_uint32), ("outputFrequency", C.c_uint32),
        ("checkpointInterval", C.c_uint32), ("snapshotFrequency", C.c_uint32),
        ("alphaA", C.c_float), ("alphaP", C.c_float),
        ("maxGibbsMassA", C.c_float), ("maxGibbsMassP", C.c_float),
        ("transposeData", C.c_int32), ("printMessages", C.c_int32),
        ("subsetData", C.c_int32), ("subsetGenes", C.c_int32),
        ("dataIndicesSubset", C.POINTER(C.c_uint32)), ("nSubset", C.c_uint32),
        ("useSparseOptimization", C.c_int32), ("takePumpSamples", C.c_int32),
        ("asynchronousUpdates", C.c_int32),
        ("whichMatrixFixed", C.c_char), ("fixedPatterns", C.POINTER(C.c_float)),
        ("fixedRows", C.c_uint32), ("workerID", C.c_uint32), ("runningDistributed", C.c_int32),
        ("device", C.c_int32), ("interrupt", INTERRUPT_FN), ("interruptArg", C.c_void_p),
        ("snapshotPhase", C.c_int32), ("pumpThreshold", C.c_int32), ("fixedCols", C.c_int32),
        ("reductionMode", C.c_int32), ("mathMode", C.c_int32), ("sampler", C.c_int32),
    ]


class CogapsResultC(C.Structure):
    _fields_ = [
        ("nGenes", C.c_uint32), ("nSamples", C.c_uint32), ("nPatterns", C.c_uint32),
        ("Amean", C.POINTER(C.c_float)), ("Asd", C.POINTER(C.c_float)),
        ("Pmean", C.POINTER(C.c_float)), ("Psd", C.POINTER(C.c_float)),
        ("nHistory", C.c_uint32), ("chisqHistory", C.POINTER(C.c_float)),
        ("atomHistoryA", C.POINTER(C.c_uint32)), ("atomHistoryP", C.POINTER(C.c_uint32)),
        ("totalUpdates", C.c_uint64), ("seed", C.c_uint32), ("totalRunningTime", C.c_uint32),
        ("meanChiSq", C.c_float), ("averageQueueLengthA", C.c_float), ("averageQueueLengthP", C.c_float),
        ("samplerSeconds", C.c_double),
        ("pumpMatrix", C.POINTER(C.c_float)), ("meanPatternAssignment", C.POINTER(C.c_float)),
        ("nEquilibrationSnapshots", C.c_uint32), ("nSamplingSnapshots", C.c_uint32),
        ("equilibrationSnapshotsA", C.POINTER(C.c_float)), ("equilibrationSnapshotsP", C.POINTER(C.c_float)),
        ("samplingSnapshotsA", C.POINTER(C.c_float)), ("samplingSnapshotsP", C.POINTER(C.c_float)),
    ]


class CogapsPerfC(C.Structure):
    _fields_ = [
        ("evalBytes", C.c_uint64), ("evalLaunches", C.c_uint64), ("genLaunches", C.c_uint64),
        ("batches", C.c_uint64), ("proposalsQueued", C.c_uint64),
        ("evalMs", C.c_double), ("genMs", C.c_double), ("syncMs", C.c_double),
        ("evalNoopMs", C.c_double), ("genNoopMs", C.c_double), ("evalNoopTimed", C.c_uint64), ("genNoopTimed", C.c_uint64),
        ("timedBatches", C.c_uint64), ("evalTimed", C.c_uint64), ("genTimed", C.c_uint64), ("syncTimed", C.c_uint64), ("syncBytes", C.c_uint64),
    ]


class CogapsSparseMatrixC(C.Structure):
    _fields_ = [
        ("nrow", C.c_uint32), ("ncol", C.c_uint32), ("majorIsRow", C.c_int32),
        ("indptr", C.c_void_p), ("indices", C.c_void_p), ("values", C.c_void_p), ("onDevice", C.c_int32),
    ]


class CogapsCooMatrixC(C.Structure):
    _fields_ = [
        ("nrow", C.c_uint32), ("ncol", C.c_uint32), ("nnz", C.c_uint64),
        ("rows", C.c_void_p), ("cols", C.c_void_p), ("values", C.c_void_p), ("onDevice", C.c_int32),
    ]


class CogapsResidualDataC(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("transposeData", C.c_int32), ("nrow", C.c_uint32), ("ncol", C.c_uint32),
        ("dense", C.c_void_p), ("uncertainty", C.c_void_p), ("rowStride", C.c_size_t), ("colStride", C.c_size_t), ("onDevice", C.c_int32),
        ("sparse", C.c_void_p), ("coo", C.c_void_p), ("deviceMatrix", C.c_void_p),
    ]


TRACE_DTYPE = np.dtype([
    ("pos", "<u8"), ("rng_state", "<u8"), ("atom1", "<u4"), ("atom2", "<u4"),
    ("r1", "<u4"), ("c1", "<u4"), ("r2", "<u4"), ("c2", "<u4"), ("type", "<u4"), ("batch", "<u4"),
])

# every symbol include/cogaps_hip.h declares
EXPORTS = [
    "cogaps_default_params", "cogaps_run", "cogaps_result_free", "cogaps_last_error", "cogaps_last_error_code",
    "cogaps_build_report", "cogaps_source_hash", "cogaps_checkpoints_enabled", "cogaps_compiled_with_openmp",
    "cogaps_session_create", "cogaps_session_destroy", "cogaps_session_set_annealing",
    "cogaps_session_draw_steps", "cogaps_session_update", "cogaps_session_sync",
    "cogaps_session_iterate", "cogaps_session_run_iterations", "cogaps_session_natoms",
    "cogaps_session_chisq", "cogaps_session_get_matrix", "cogaps_session_get_ap",
    "cogaps_session_get_atoms", "cogaps_session_dims", "cogaps_session_avg_queue",
    "cogaps_session_finish", "cogaps_session_set_timing", "cogaps_session_perf",
    "cogaps_session_perf_sampler", "cogaps_session_chained", "cogaps_session_chain_recoveries", "cogaps_session_generator_window", "cogaps_session_launch_clock", "cogaps_session_launch_period", "cogaps_session_get_rows", "cogaps_sparse_width", "cogaps_reduction_width", "cogaps_session_debug_prof", "cogaps_session_debug_replay",
    "cogaps_run_from_file", "cogaps_read_matrix_file", "cogaps_read_matrix_file_subset", "cogaps_matrix_free", "cogaps_file_info", "cogaps_debug_math", "cogaps_debug_udiv64", "cogaps_debug_uniform64", "cogaps_current_device", "cogaps_device_memory",
    "cogaps_session_create_sparse", "cogaps_run_sparse", "cogaps_session_device_bytes", "cogaps_session_sparse_build_ms", "cogaps_session_debug_sparse_data",
    "cogaps_session_create_coo", "cogaps_run_coo", "cogaps_read_mtx_triplets", "cogaps_triplets_free",
    "cogaps_device_matrix_create_sparse", "cogaps_device_matrix_create_coo", "cogaps_device_matrix_destroy", "cogaps_device_matrix_info",
    "cogaps_session_create_from_device_matrix", "cogaps_run_device_matrix",
    "cogaps_run_device", "cogaps_session_debug_dense_data",
    "cogaps_session_position", "cogaps_session_save_state", "cogaps_session_load_state", "cogaps_session_run_to_end", "cogaps_session_debug_data_digest",
    "cogaps_gene_set_stat", "cogaps_debug_permutation_draw", "cogaps_gene_set_membership", "cogaps_pattern_markers", "cogaps_residuals", "cogaps_pattern_gsea", "cogaps_pattern_match", "cogaps_manova_sscp", "cogaps_project",
    "cogaps_session_debug_check_domain", "cogaps_batch_create", "cogaps_batch_destroy", "cogaps_batch_run_iterations", "cogaps_batch_set_timing", "cogaps_batch_perf",
]

REDUCE_LANES, REDUCE_SEQ = 0, 1                              # cogaps_params.reductionMode
MATH_PORTABLE, MATH_GLIBC_FMA, MATH_GLIBC_SSE2 = 0, 1, 2     # cogaps_params.mathMode
_REDUCE = {"lanes": REDUCE_LANES, "seq": REDUCE_SEQ}
_MATH = {"portable": MATH_PORTABLE, "glibc-fma": MATH_GLIBC_FMA, "glibc-sse2": MATH_GLIBC_SSE2}
_PUMP = {"unique": 0, "cut": 1}
SAMPLER_ASYNC, SAMPLER_SEQUENTIAL = 0, 1                     # cogaps_params.sampler
_SAMPLER = {"async": SAMPLER_ASYNC, "sequential": SAMPLER_SEQUENTIAL}

ERR_GENERIC, ERR_OUT_OF_DEVICE_MEMORY, ERR_OUT_OF_HOST_MEMORY = 1, 2, 3      # cogaps_last_error_code()


class CogapsError(RuntimeError):
    """a failing call of the C ABI: the library's message, and its kind as a code (include/cogaps_hip.h, cogaps_last_error_code)"""

    def __init__(self, message, code=ERR_GENERIC):
        super().__init__(message)
        self.code = code


class OutOfDeviceMemory(CogapsError):
    """hipErrorOutOfMemory inside the library (COGAPS_ERR_OUT_OF_DEVICE_MEMORY)"""


def _error(L, prefix=""):
    """the exception for the calling thread's last failing call"""
    code = int(L.cogaps_last_error_code())
    msg = prefix + L.cogaps_last_error().decode()
    return OutOfDeviceMemory(msg, code) if code == ERR_OUT_OF_DEVICE_MEMORY else CogapsError(msg, code)


def bind(L):
    """Attach prototypes to an opened library implementing include/cogaps_hip.h."""
    fp, u32p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p
    L.cogaps_default_params.argtypes = [C.POINTER(CogapsParamsC)]
    L.cogaps_default_params.restype = None
    L.cogaps_run.argtypes = [fp, C.c_uint32, C.c_uint32, C.POINTER(CogapsParamsC), fp, C.POINTER(CogapsResultC)]
    if hasattr(L, "cogaps_run_device"):      # (an A/B build of an older source tree lacks the two: tools/measure_dense_device_session_create.py)
        L.cogaps_run_device.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(CogapsParamsC), vp, C.POINTER(CogapsResultC)]
        L.cogaps_session_debug_dense_data.argtypes = [vp, C.c_char, vp, vp, vp, fp, fp, fp, C.POINTER(C.c_int)]
    L.cogaps_result_free.argtypes = [C.POINTER(CogapsResultC)]
    L.cogaps_result_free.restype = None
    L.cogaps_last_error.restype = C.c_char_p
    L.cogaps_last_error_code.restype = C.c_int
    L.cogaps_build_report.restype = C.c_char_p
    L.cogaps_source_hash.restype = C.c_char_p
    L.cogaps_session_create.restype = vp
    L.cogaps_session_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(CogapsParamsC), vp, C.c_int]
    L.cogaps_session_create_sparse.restype = vp
    L.cogaps_session_create_sparse.argtypes = [C.POINTER(CogapsSparseMatrixC), C.POINTER(CogapsParamsC)]
    L.cogaps_run_sparse.argtypes = [C.POINTER(CogapsSparseMatrixC), C.POINTER(CogapsParamsC), C.POINTER(CogapsResultC)]
    L.cogaps_session_create_coo.restype = vp
    L.cogaps_session_create_coo.argtypes = [C.POINTER(CogapsCooMatrixC), C.POINTER(CogapsParamsC)]
    L.cogaps_run_coo.argtypes = [C.POINTER(CogapsCooMatrixC), C.POINTER(CogapsParamsC), C.POINTER(CogapsResultC)]
    L.cogaps_device_matrix_create_sparse.restype = vp
    L.cogaps_device_matrix_create_sparse.argtypes = [C.POINTER(CogapsSparseMatrixC), C.c_int]
    L.cogaps_device_matrix_create_coo.restype = vp
    L.cogaps_device_matrix_create_coo.argtypes = [C.POINTER(CogapsCooMatrixC), C.c_int]
    L.cogaps_device_matrix_destroy.argtypes = [vp]
    L.cogaps_device_matrix_destroy.restype = None
    L.cogaps_device_matrix_info.argtypes = [vp, u32p, u32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.cogaps_session_create_from_device_matrix.restype = vp
    L.cogaps_session_create_from_device_matrix.argtypes = [vp, C.POINTER(CogapsParamsC)]
    L.cogaps_run_device_matrix.argtypes = [vp, C.POINTER(CogapsParamsC), C.POINTER(CogapsResultC)]
    L.cogaps_read_mtx_triplets.argtypes = [C.c_char_p, C.c_int, u32p, C.c_uint32, u32p, u32p, C.POINTER(C.c_uint64), C.POINTER(u32p), C.POINTER(u32p), C.POINTER(fp)]
    L.cogaps_triplets_free.argtypes = [u32p, u32p, fp]
    L.cogaps_triplets_free.restype = None
    L.cogaps_session_device_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.cogaps_session_sparse_build_ms.argtypes = [vp, fp]
    L.cogaps_session_debug_sparse_data.argtypes = [vp, C.c_char, u32p, u32p, fp, fp, vp, vp, vp, vp]
    L.cogaps_session_destroy.argtypes = [vp]
    L.cogaps_session_destroy.restype = None
    L.cogaps_session_set_annealing.argtypes = [vp, C.c_float]
    L.cogaps_session_draw_steps.argtypes = [vp, u32p, u32p]
    L.cogaps_session_update.argtypes = [vp, C.c_char, C.c_uint32, vp, C.c_uint32, u32p, u32p, u32p, C.c_uint32, u32p]
    L.cogaps_session_sync.argtypes = [vp, C.c_char]
    L.cogaps_session_iterate.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int]
    L.cogaps_session_run_iterations.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.cogaps_session_natoms.argtypes = [vp, C.c_char, u32p]
    L.cogaps_session_chisq.argtypes = [vp, C.c_char, fp]
    L.cogaps_session_get_matrix.argtypes = [vp, C.c_char, fp]
    L.cogaps_session_get_ap.argtypes = [vp, C.c_char, fp]
    L.cogaps_session_get_atoms.argtypes = [vp, C.c_char, C.POINTER(C.c_uint64), fp, u32p, u32p]
    L.cogaps_session_dims.argtypes = [vp, C.c_char, u32p, u32p, u32p]
    L.cogaps_session_avg_queue.argtypes = [vp, C.c_char, fp]
    L.cogaps_session_finish.argtypes = [vp, C.POINTER(CogapsResultC)]
    L.cogaps_session_set_timing.argtypes = [vp, C.c_int]
    L.cogaps_session_perf.argtypes = [vp, C.POINTER(CogapsPerfC)]
    L.cogaps_session_perf_sampler.argtypes = [vp, C.c_char, C.POINTER(CogapsPerfC)]
    L.cogaps_session_chained.argtypes = [vp, C.c_char, C.POINTER(C.c_int)]
    L.cogaps_session_chain_recoveries.argtypes = [vp, C.c_char, C.POINTER(C.c_uint32)]
    L.cogaps_session_generator_window.argtypes = [vp, C.c_char, C.POINTER(C.c_uint32)]
    if hasattr(L, "cogaps_session_launch_period"):
        L.cogaps_session_launch_period.argtypes = [vp, C.c_char, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    if hasattr(L, "cogaps_session_launch_clock"):      # (an A/B build of an older source tree may lack it: launch_clock() then reports no launches)
        L.cogaps_session_launch_clock.argtypes = [vp, C.c_char, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.cogaps_session_debug_prof.argtypes = [vp, C.c_char, C.POINTER(C.c_uint64)]
    L.cogaps_session_debug_replay.argtypes = [vp, C.c_char, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.cogaps_reduction_width.restype = C.c_uint32
    L.cogaps_sparse_width.restype = C.c_uint32
    L.cogaps_sparse_width.argtypes = [C.c_uint32]
    L.cogaps_session_get_rows.argtypes = [vp, C.c_char, fp]
    L.cogaps_reduction_width.argtypes = [C.c_uint32]
    L.cogaps_run_from_file.argtypes = [C.c_char_p, C.POINTER(CogapsParamsC), C.c_char_p, C.POINTER(CogapsResultC)]
    L.cogaps_read_matrix_file.argtypes = [C.c_char_p, u32p, u32p, C.POINTER(fp)]
    L.cogaps_read_matrix_file_subset.argtypes = [C.c_char_p, C.c_int, u32p, C.c_uint32, u32p, u32p, C.POINTER(fp)]
    L.cogaps_matrix_free.argtypes = [fp]
    L.cogaps_matrix_free.restype = None
    L.cogaps_file_info.argtypes = [C.c_char_p, u32p, u32p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cogaps_debug_math.argtypes = [C.c_int, C.c_int, fp, fp, C.c_uint32, C.c_int]
    if hasattr(L, "cogaps_debug_udiv64"):      # (an A/B build of an older source tree lacks the two)
        L.cogaps_debug_udiv64.argtypes = [C.POINTER(C.c_uint64)] * 3 + [C.c_uint32, C.c_int]
        L.cogaps_debug_uniform64.argtypes = [C.POINTER(C.c_uint64)] * 5 + [C.c_uint32, C.c_int]
    L.cogaps_current_device.argtypes = [C.POINTER(C.c_int)]
    L.cogaps_device_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.cogaps_session_debug_check_domain.argtypes = [vp, C.c_char, u32p]
    L.cogaps_session_position.argtypes = [vp, C.POINTER(C.c_int), u32p]
    L.cogaps_session_save_state.argtypes = [vp, C.c_char_p]
    L.cogaps_session_load_state.argtypes = [vp, C.c_char_p]
    L.cogaps_session_run_to_end.argtypes = [vp, C.c_char_p, C.c_uint32, C.POINTER(CogapsResultC)]
    L.cogaps_session_debug_data_digest.argtypes = [vp, C.POINTER(C.c_uint64)]
    u64p, dp = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    L.cogaps_gene_set_stat.argtypes = [dp, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, u64p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_int, u32p, dp]
    L.cogaps_debug_permutation_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, u32p]
    L.cogaps_gene_set_membership.argtypes = [dp, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, u64p, u32p, dp, dp, C.c_int, dp, u32p, dp]
    L.cogaps_pattern_markers.argtypes = [dp, C.c_uint64, C.c_uint32, C.c_size_t, C.c_size_t, dp, C.c_uint64, C.c_size_t, C.c_size_t, dp, C.c_uint32, C.c_int, C.c_int, u32p, dp, u32p, u32p]
    L.cogaps_pattern_gsea.argtypes = [fp, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, u64p, u32p, C.c_uint32, C.c_uint32, C.c_int, dp, u32p, u32p, u64p, u32p]
    L.cogaps_residuals.argtypes = [fp, C.c_uint32, C.c_size_t, C.c_size_t, fp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(CogapsResidualDataC),
                                   u32p, C.c_uint32, C.c_int, dp, dp, dp, dp, u64p]
    L.cogaps_pattern_match.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                       u32p, u32p, dp, fp, dp, u32p]
    L.cogaps_manova_sscp.argtypes = [fp, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, dp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int, dp, dp, dp, dp, dp]
    if hasattr(L, "cogaps_project"):      # (an A/B build of an older source tree lacks it)
        L.cogaps_project.argtypes = [fp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(CogapsResidualDataC), u32p, C.c_int, dp, dp, dp, dp, dp, u64p]
    L.cogaps_batch_create.restype = vp
    L.cogaps_batch_create.argtypes = [C.POINTER(vp), C.c_uint32]
    L.cogaps_batch_destroy.argtypes = [vp]
    L.cogaps_batch_destroy.restype = None
    L.cogaps_batch_run_iterations.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.cogaps_batch_set_timing.argtypes = [vp, C.c_int]
    L.cogaps_batch_perf.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


_lib = None


def load():
    """The HIP library, or RuntimeError.  No fallback of any kind."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "cogaps_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        # One HIP / HSA runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64; when the library
        # is loaded first it brings /opt/rocm's copies in, a later `import torch` adds the bundled ones, and whichever runtime touches
        # the device second finds it taken ("no ROCm-capable device is detected" -- in torch.cuda / RCCL, or here).  With torch
        # imported first the loader resolves this library's dependencies to the copies torch uses, so the front-end (device
        # tensors, torch.distributed over RCCL) and the sampler share one runtime.  Without PyTorch (a plain C / R client) the
        # library runs on the ROCm installation's runtime alone.
        # COGAPS_NO_TORCH=1 skips this (a Python client that never uses torch saves the import and stays on the ROCm installation's
        # runtime; it must then not import torch later in the same process).  A PyTorch that is not a ROCm build (CPU-only, CUDA)
        # bundles no HIP runtime: nothing to share, the library resolves against /opt/rocm as it would without PyTorch.
        import sys
        if "torch" in sys.modules or os.environ.get("COGAPS_NO_TORCH", "") in ("", "0"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def make_params(L, nPatterns=3, nIterations=1000, seed=0, outputFrequency=500, nThreads=1,
                alphaA=0.01, alphaP=0.01, maxGibbsMassA=100.0, maxGibbsMassP=100.0,
                transposeData=False, subsetIndices=None, subsetDim=0, whichMatrixFixed="N",
                fixedPatterns=None, sparseOptimization=False, asynchronousUpdates=True,
                messages=False, workerID=1, device=-1, takePumpSamples=False,
                checkpointInterval=0, nSnapshots=0, snapshotPhase="sampling", snapshotFrequency=None,
                pumpThreshold="unique", reductionMode="lanes", mathMode="portable", runningDistributed=False, interrupt=None,
                sampler="async"):
    p = CogapsParamsC()
    L.cogaps_default_params(C.byref(p))
    p.nPatterns, p.nIterations, p.seed = int(nPatterns), int(nIterations), int(seed)
    p.outputFrequency, p.maxThreads = int(outputFrequency), int(nThreads)
    p.alphaA, p.alphaP = float(alphaA), float(alphaP)
    p.maxGibbsMassA, p.maxGibbsMassP = float(maxGibbsMassA), float(maxGibbsMassP)
    p.transposeData = int(bool(transposeData))
    p.printMessages = int(bool(messages)) if workerID == 1 else 0       # Cogaps.cpp:85
    p.useSparseOptimization = int(bool(sparseOptimization))
    p.asynchronousUpdates = int(bool(asynchronousUpdates))
    p.takePumpSamples = int(bool(takePumpSamples))
    p.checkpointInterval = int(checkpointInterval)
    # Cogaps.cpp:104-123: nSnapshots -> snapshotFrequency = nIterations / nSnapshots; phase names
    p.snapshotFrequency = int(snapshotFrequency) if snapshotFrequency is not None else (int(nIterations) // int(nSnapshots) if nSnapshots else 0)
    p.snapshotPhase = {"all": 0, "equilibration": 1, "sampling": 2}[snapshotPhase] if isinstance(snapshotPhase, str) else int(snapshotPhase)
    p.workerID = int(workerID)
    p.device = int(device)
    p.runningDistributed = int(bool(runningDistributed))
    p.pumpThreshold = _PUMP[pumpThreshold] if isinstance(pumpThreshold, str) else int(pumpThreshold)
    p.reductionMode = _REDUCE[reductionMode] if isinstance(reductionMode, str) else int(reductionMode)
    p.mathMode = _MATH[mathMode] if isinstance(mathMode, str) else int(mathMode)
    if isinstance(sampler, str) and sampler not in _SAMPLER:
        raise ValueError('sampler must be "async" or "sequential", not %r' % (sampler,))
    p.sampler = _SAMPLER[sampler] if isinstance(sampler, str) else int(sampler)      # (an integer reaches the library as it is: it refuses what it does not know)
    keep = []
    if interrupt is not None:
        # cogaps_params.interrupt: a callable without arguments, polled at the head of every iteration; a true value ends the run
        fn = INTERRUPT_FN(lambda _arg: int(bool(interrupt())))
        keep.append(fn)
        p.interrupt = fn
    if subsetIndices is not None and subsetDim > 0:
        idx = np.ascontiguousarray(subsetIndices, dtype=np.uint32)
        keep.append(idx)
        p.subsetData = 1
        p.subsetGenes = 1 if subsetDim == 1 else 0
        p.dataIndicesSubset = idx.ctypes.data_as(C.POINTER(C.c_uint32))
        p.nSubset = idx.size
        p.runningDistributed = 1
    p.whichMatrixFixed = str(whichMatrixFixed).encode()[:1]
    if fixedPatterns is not None and whichMatrixFixed != "N":
        fx = np.ascontiguousarray(fixedPatterns, dtype=np.float32)
        keep.append(fx)
        if fx.ndim != 2 or fx.shape[1] != int(nPatterns):
            raise ValueError("fixedPatterns must have nPatterns = %d columns" % int(nPatterns))
        p.fixedPatterns = _fp(fx)
        p.fixedRows = fx.shape[0]
        p.fixedCols = fx.shape[1]
    p._keep = keep
    return p


def result_to_dict(L, r):
    g, s, k, h = r.nGenes, r.nSamples, r.nPatterns, r.nHistory
    out = {
        "Amean": np.ctypeslib.as_array(r.Amean, shape=(g, k)).copy(),
        "Asd": np.ctypeslib.as_array(r.Asd, shape=(g, k)).copy(),
        "Pmean": np.ctypeslib.as_array(r.Pmean, shape=(s, k)).copy(),
        "Psd": np.ctypeslib.as_array(r.Psd, shape=(s, k)).copy(),
        "chisq": np.ctypeslib.as_array(r.chisqHistory, shape=(max(h, 1),))[:h].copy(),
        "atomsA": np.ctypeslib.as_array(r.atomHistoryA, shape=(max(h, 1),))[:h].copy(),
        "atomsP": np.ctypeslib.as_array(r.atomHistoryP, shape=(max(h, 1),))[:h].copy(),
        "totalUpdates": int(r.totalUpdates), "meanChiSq": float(r.meanChiSq), "seed": int(r.seed),
        "averageQueueLengthA": float(r.averageQueueLengthA),
        "averageQueueLengthP": float(r.averageQueueLengthP),
        "totalRunningTime": int(r.totalRunningTime), "samplerSeconds": float(r.samplerSeconds),
    }

    def _arr(ptr, shape):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].reshape(shape).copy() if ptr else np.zeros(shape, dtype=np.float32)
    if r.pumpMatrix:
        out["pumpMatrix"] = _arr(r.pumpMatrix, (g, k)); out["meanPatternAssignment"] = _arr(r.meanPatternAssignment, (g, k))
    ne, ns = int(r.nEquilibrationSnapshots), int(r.nSamplingSnapshots)
    out["equilibrationSnapshotsA"] = _arr(r.equilibrationSnapshotsA, (ne, g, k)); out["equilibrationSnapshotsP"] = _arr(r.equilibrationSnapshotsP, (ne, s, k))
    out["samplingSnapshotsA"] = _arr(r.samplingSnapshotsA, (ns, g, k)); out["samplingSnapshotsP"] = _arr(r.samplingSnapshotsP, (ns, s, k))
    L.cogaps_result_free(C.byref(r))
    return out


def is_sparse(data):
    """whether `data` is a scipy.sparse matrix (scipy is imported only if the process can import it; without it nothing is sparse)"""
    try:
        import scipy.sparse as sp
    except ImportError:
        return False
    return sp.issparse(data)


class SparseMatrix:
    """A matrix in compressed-sparse form as cogaps_sparse_matrix takes it (include/cogaps_hip.h): CSR or CSC, indptr uint64,
    indices uint32, values float32 -- from a scipy.sparse matrix (canonicalised: duplicates summed, indices sorted; anything but CSC
    becomes CSR), or from three device-resident arrays (on_device=True: the integers are addresses, e.g. torch's data_ptr())."""

    def __init__(self, shape, major_is_row, indptr, indices, values, on_device=False):
        self.shape = (int(shape[0]), int(shape[1]))
        self.major_is_row, self.on_device = bool(major_is_row), bool(on_device)
        self.indptr, self.indices, self.values = indptr, indices, values

    @classmethod
    def from_scipy(cls, m):
        m = m.copy() if m.format == "csc" else m.tocsr(copy=True)
        m.sum_duplicates()
        m.sort_indices()
        return cls(m.shape, m.format == "csr", np.ascontiguousarray(m.indptr, dtype=np.uint64), np.ascontiguousarray(m.indices, dtype=np.uint32),
                   np.ascontiguousarray(m.data, dtype=np.float32))

    def c_struct(self):
        addr = (lambda a: int(a)) if self.on_device else (lambda a: a.ctypes.data)
        return CogapsSparseMatrixC(self.shape[0], self.shape[1], int(self.major_is_row), addr(self.indptr), addr(self.indices), addr(self.values), int(self.on_device))


class CooMatrix:
    """A matrix as unordered triplets as cogaps_coo_matrix takes it (include/cogaps_hip.h): rows / cols uint32 (0-based), values float32,
    any order, repeats allowed -- the LATEST entry of a position decides it (a Matrix Market file read in file order; not scipy's
    meaning of COO, which sums repeats: a scipy.sparse matrix goes through SparseMatrix.from_scipy).  on_device=True: the three are
    addresses of device-resident arrays and `nnz` their length.  CoGAPS() applies its input checks (NA, negative values) to every
    triplet value of a file, overwritten or not: a file whose earlier entry of a repeated position is negative is refused there,
    while the dense read of the same file -- and cogaps_run_from_file -- never see that entry."""

    def __init__(self, shape, rows, cols, values, on_device=False, nnz=None):
        self.shape = (int(shape[0]), int(shape[1]))
        self.on_device = bool(on_device)
        if not self.on_device:
            rows, cols = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(cols, dtype=np.uint32)
            values = np.ascontiguousarray(values, dtype=np.float32)
            if not (rows.ndim == cols.ndim == values.ndim == 1 and rows.size == cols.size == values.size):
                raise ValueError("rows, cols and values must be one-dimensional and of one length")
            nnz = values.size
        elif nnz is None:
            raise ValueError("device-resident triplets need nnz")
        self.rows, self.cols, self.values, self.nnz = rows, cols, values, int(nnz)

    def c_struct(self):
        addr = (lambda a: int(a)) if self.on_device else (lambda a: a.ctypes.data)
        return CogapsCooMatrixC(self.shape[0], self.shape[1], self.nnz, addr(self.rows), addr(self.cols), addr(self.values), int(self.on_device))

    def toarray(self):
        """the dense matrix the triplets denote (host-resident triplets; the last entry of a position decides)"""
        d = np.zeros(self.shape, dtype=np.float32)
        d[self.rows, self.cols] = self.values        # (numpy assigns repeated indices in order: the last one stays)
        return d

    def tocsr(self):
        """scipy CSR of the matrix the triplets denote: repeats resolved (the last entry decides), entries not > 0 dropped"""
        import scipy.sparse as sp
        key = self.rows.astype(np.int64) * self.shape[1] + self.cols
        order = np.argsort(key, kind="stable")
        last = np.ones(order.size, dtype=bool)
        last[:-1] = key[order][1:] != key[order][:-1]
        keep = order[last]
        keep = keep[self.values[keep] > 0]
        return sp.csr_matrix((self.values[keep], (self.rows[keep], self.cols[keep])), shape=self.shape, dtype=np.float32)


class DeviceMatrix:
    """A matrix resident on one GPU (cogaps_device_matrix of include/cogaps_hip.h): uploaded, validated and -- for triplets -- resolved
    for repeated positions once; Session / run / run_batch / CoGAPS then make any number of sparse-model sessions from it, each with its
    own nPatterns, seed, transposeData and subsetIndices / subsetDim (the subset is taken on the device, by the dense entry's rule: the
    1-based indices in the order given, a repeated index repeats the row / column).  `data`: a scipy.sparse matrix, a SparseMatrix, a
    CooMatrix (host or device arrays) or the path of a .mtx file (read as triplets, never densified).  device = -1: the calling
    thread's current one.  May be closed while sessions made from it live on."""

    def __init__(self, data, device=-1, lib=None):
        self.L = lib if lib is not None else load()
        self.h = None
        if isinstance(data, (str, bytes, os.PathLike)):
            data = read_mtx_triplets(data, lib=self.L)
        elif is_sparse(data):
            data = SparseMatrix.from_scipy(data)
        if not isinstance(data, (SparseMatrix, CooMatrix)):
            raise TypeError("DeviceMatrix takes a scipy.sparse matrix, a SparseMatrix, a CooMatrix or the path of a .mtx file")
        # what the front end's input checks (api.check_inputs) need to know of the host values; None: device arrays, never seen here
        self.has_na = None if data.on_device else bool(np.isnan(data.values).any())
        self.has_negative = None if data.on_device else bool((data.values < 0).any())
        m = data.c_struct()
        name = "cogaps_device_matrix_create_coo" if isinstance(data, CooMatrix) else "cogaps_device_matrix_create_sparse"
        self.h = getattr(self.L, name)(C.byref(m), int(device))
        if not self.h:
            raise _error(self.L, name + ": ")
        nr, nc, nnz, dev = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_int()
        if self.L.cogaps_device_matrix_info(self.h, C.byref(nr), C.byref(nc), C.byref(nnz), None, C.byref(dev)):
            raise _error(self.L)
        self.shape, self.nnz, self.device = (nr.value, nc.value), int(nnz.value), dev.value

    def _handle(self):
        if not self.h:
            raise ValueError("the DeviceMatrix is closed")
        return self.h

    def device_bytes(self):
        """bytes of device memory the handle holds (never part of a session's device_bytes())"""
        v = C.c_uint64(0)
        if self.L.cogaps_device_matrix_info(self._handle(), None, None, None, C.byref(v), None):
            raise _error(self.L)
        return int(v.value)

    def close(self):
        if getattr(self, "h", None):
            self.L.cogaps_device_matrix_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceDense:
    """A dense matrix resident on one GPU as cogaps_session_create takes it with data_on_device = 1 (include/cogaps_hip.h): `data_addr`
    -- and `unc_addr`, unless None -- are the addresses of row-major fp32 arrays of `shape` in the memory of the run's device (e.g.
    torch's data_ptr()), in the manner of SparseMatrix(..., on_device=True).  Session / run / run_batch build from them on the device,
    for both models; nothing of the matrix goes through the host.  The arrays must be complete before the call and stay alive until it
    returns (`keep`: objects that own them, held as long as this object lives).  A torch tensor given to Session / run / run_batch /
    CoGAPS becomes one of these by itself (device_input)."""

    def __init__(self, shape, data_addr, unc_addr=None, keep=None):
        self.shape = (int(shape[0]), int(shape[1]))
        self.data_addr, self.unc_addr, self.keep = int(data_addr), (None if unc_addr is None else int(unc_addr)), keep


def is_tensor(x):
    """whether x is a torch tensor, without importing torch: by the module of its type (a process that holds a tensor has torch loaded)"""
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def on_gpu(x):
    return is_tensor(x) and x.is_cuda


def device_input(data, unc, kw):
    """Torch tensors among (data, unc) resolved: -> (data, unc, kw) for the dense entry.  A CPU tensor is its numpy view.  A GPU tensor
    becomes a DeviceDense of contiguous fp32 copies made on its device (none where it is contiguous fp32 already); the uncertainty
    follows the data to the device, or to the host.  kw's device = -1 resolves to the tensor's device, any other device is a
    ValueError; the tensor's current stream is synchronised, so that the library -- which reads on a stream of its own -- finds the
    arrays complete."""
    if isinstance(data, DeviceDense) and unc is not None:
        raise ValueError("a DeviceDense carries its uncertainty itself (unc_addr)")
    if not (is_tensor(data) or is_tensor(unc)):
        return data, unc, kw
    if not on_gpu(data):
        cpu = lambda t: t.detach().cpu().numpy() if is_tensor(t) else t
        return cpu(data), cpu(unc), kw
    import torch      # (loaded already: the caller holds a tensor.  load() imports it first in any case: one HIP runtime per process)
    dev = data.device.index if data.device.index is not None else torch.cuda.current_device()
    want = int(kw.get("device", -1))
    if want not in (-1, dev):
        raise ValueError("the data tensor resides on device %d, the run was given device=%d" % (dev, want))
    if data.dim() != 2:
        raise ValueError("data must be a 2-D tensor")
    d = data.detach().to(dtype=torch.float32).contiguous()
    u = None
    if unc is not None:
        u = (unc.detach() if is_tensor(unc) else torch.from_numpy(np.ascontiguousarray(unc))).to(device=data.device, dtype=torch.float32).contiguous()
        if tuple(u.shape) != tuple(d.shape):
            raise ValueError("the uncertainty matrix must have the shape of the data")
    torch.cuda.current_stream(data.device).synchronize()
    return DeviceDense(d.shape, d.data_ptr(), None if u is None else u.data_ptr(), keep=(d, u)), None, dict(kw, device=dev)


def _sparse_input(data, unc, kw):
    """the SparseMatrix / CooMatrix / DeviceMatrix to hand to the library's compressed-sparse / triplet / device-matrix entry, or None
    for the dense entry.  A scipy.sparse matrix goes in compressed form when the run uses the sparse model; the dense model takes it
    densified (the caller does: toarray())."""
    if isinstance(data, (SparseMatrix, CooMatrix, DeviceMatrix)):
        if unc is not None:
            raise ValueError("the sparse model takes no uncertainty matrix")
        return data
    if is_sparse(data) and kw.get("sparseOptimization", False):
        if unc is not None:
            raise ValueError("the sparse model takes no uncertainty matrix")
        return SparseMatrix.from_scipy(data)
    return None


def _dense(a):
    return np.ascontiguousarray(a.toarray() if is_sparse(a) else a, dtype=np.float32)


class Session:
    """One sampler run, one step at a time (cogaps_session_* of include/cogaps_hip.h).  `data`: a dense matrix (a numpy array, a torch
    tensor -- on the GPU it is consumed there -- or a DeviceDense of raw device addresses, with `unc` alike), a scipy.sparse matrix
    (with sparseOptimization=True it reaches the library in compressed form, cogaps_session_create_sparse; otherwise densified), a
    SparseMatrix, a CooMatrix (cogaps_session_create_coo) or a DeviceMatrix (cogaps_session_create_from_device_matrix)."""

    def __init__(self, data, unc=None, lib=None, **kw):
        self.L = lib if lib is not None else load()
        data, unc, kw = device_input(data, unc, kw)
        self.p = make_params(self.L, **kw)
        if isinstance(data, DeviceDense):
            # device pointers: built on the device (csrc/dense_build.h); the call synchronises, the arrays are not referenced afterwards
            self.sp = self.d = self.u = None
            self.h = self.L.cogaps_session_create(data.data_addr, data.shape[0], data.shape[1], C.byref(self.p), data.unc_addr, 1)
            if not self.h:
                raise _error(self.L, "cogaps_session_create: ")
            return
        self.sp = _sparse_input(data, unc, kw)
        if isinstance(self.sp, DeviceMatrix):
            self.d = self.u = None
            self.h = self.L.cogaps_session_create_from_device_matrix(self.sp._handle(), C.byref(self.p))
            if not self.h:
                raise _error(self.L, "cogaps_session_create_from_device_matrix: ")
            self.sp = None      # the session holds nothing of the handle
            return
        if self.sp is not None:
            self.d = self.u = None
            m = self.sp.c_struct()
            name = "cogaps_session_create_coo" if isinstance(self.sp, CooMatrix) else "cogaps_session_create_sparse"
            self.h = getattr(self.L, name)(C.byref(m), C.byref(self.p))
            if not self.h:
                raise _error(self.L, name + ": ")
            self.sp = None      # the library copied what it needs
            return
        self.d = _dense(data)
        self.u = None if unc is None else _dense(unc)
        self.h = self.L.cogaps_session_create(self.d.ctypes.data, self.d.shape[0], self.d.shape[1], C.byref(self.p),
                                              None if self.u is None else self.u.ctypes.data, 0)
        if not self.h:
            raise _error(self.L, "cogaps_session_create: ")

    def device_bytes(self):
        """bytes of device memory the session holds (its own allocations)"""
        v = C.c_uint64(0)
        self._ck(self.L.cogaps_session_device_bytes(self.h, C.byref(v)))
        return int(v.value)

    def sparse_build_ms(self):
        """HIP-event time of the ordered sums at the creation of a sparse-model session (0 for the dense model)"""
        v = C.c_float(0)
        self._ck(self.L.cogaps_session_sparse_build_ms(self.h, C.byref(v)))
        return float(v.value)

    def debug_dense_data(self, which):
        """the dense model's data of sampler `which` as the device holds it: D, Sraw, S2 [M][Npad] with their pads (S2: None when the
        session keeps none), lambda, maxGibbsMass, sparsity"""
        m, n, _ = self.dims(which)
        shape = (m, (n + 3) & ~3)
        D, SR, S2 = (np.full(shape, np.nan, dtype=np.float32) for _ in range(3))
        lam, mg, spa, has = C.c_float(), C.c_float(), C.c_float(), C.c_int()
        self._ck(self.L.cogaps_session_debug_dense_data(self.h, which.encode(), D.ctypes.data, SR.ctypes.data, S2.ctypes.data,
                                                        C.byref(lam), C.byref(mg), C.byref(spa), C.byref(has)))
        return {"D": D, "Sraw": SR, "S2": S2 if has.value else None, "lambda": lam.value, "maxGibbsMass": mg.value, "sparsity": spa.value}

    def debug_sparse_data(self, which):
        """the sparse model's data structures of sampler `which`: flags / prefix [M][Wn], ptr [M + 1], vals, lambda, maxGibbsMass"""
        wn, nv, lam, mg = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float()
        self._ck(self.L.cogaps_session_debug_sparse_data(self.h, which.encode(), C.byref(wn), C.byref(nv), C.byref(lam), C.byref(mg), None, None, None, None))
        m = self.dims(which)[0]
        fl, pre = np.zeros((m, wn.value), dtype=np.uint64), np.zeros((m, wn.value), dtype=np.uint32)
        ptr, vals = np.zeros(m + 1, dtype=np.uint32), np.zeros(nv.value, dtype=np.float32)
        self._ck(self.L.cogaps_session_debug_sparse_data(self.h, which.encode(), None, None, None, None, fl.ctypes.data, pre.ctypes.data, ptr.ctypes.data, vals.ctypes.data))
        return {"flags": fl, "prefix": pre, "ptr": ptr, "vals": vals, "lambda": lam.value, "maxGibbsMass": mg.value}

    def _ck(self, rc):
        if rc:
            raise _error(self.L)

    def close(self):
        if getattr(self, "h", None):
            self.L.cogaps_session_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_annealing(self, t):
        self._ck(self.L.cogaps_session_set_annealing(self.h, t))

    def draw_steps(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._ck(self.L.cogaps_session_draw_steps(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def update(self, which, nsteps, trace_cap=0):
        if not trace_cap:
            self._ck(self.L.cogaps_session_update(self.h, which.encode(), nsteps, None, 0, None, None, None, 0, None))
            return None
        rec = np.zeros(trace_cap, dtype=TRACE_DTYPE)
        bn = np.zeros(trace_cap, dtype=np.uint32)
        bq = np.zeros(trace_cap, dtype=np.uint32)
        nt, nb = C.c_uint32(), C.c_uint32()
        u32p = C.POINTER(C.c_uint32)
        self._ck(self.L.cogaps_session_update(self.h, which.encode(), nsteps, rec.ctypes.data, trace_cap, C.byref(nt),
                                              bn.ctypes.data_as(u32p), bq.ctypes.data_as(u32p), trace_cap, C.byref(nb)))
        assert nt.value <= trace_cap and nb.value <= trace_cap, "trace overflow"
        return {"rec": rec[:nt.value], "nproc": bn[:nb.value], "qlen": bq[:nb.value]}

    def sync(self, which):
        self._ck(self.L.cogaps_session_sync(self.h, which.encode()))

    def iterate(self, nA, nP, sampling=False):
        self._ck(self.L.cogaps_session_iterate(self.h, nA, nP, int(sampling)))

    def run_iterations(self, phase, first, n):
        upd = C.c_uint64(0)
        self._ck(self.L.cogaps_session_run_iterations(self.h, phase, first, n, C.byref(upd)))
        return upd.value

    def natoms(self, which):
        n = C.c_uint32()
        self._ck(self.L.cogaps_session_natoms(self.h, which.encode(), C.byref(n)))
        return n.value

    def chisq(self, which):
        c = C.c_float()
        self._ck(self.L.cogaps_session_chisq(self.h, which.encode(), C.byref(c)))
        return c.value

    def dims(self, which):
        m, n, k = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.L.cogaps_session_dims(self.h, which.encode(), C.byref(m), C.byref(n), C.byref(k)))
        return m.value, n.value, k.value

    def matrix(self, which):
        m, n, k = self.dims(which)
        out = np.zeros((m, k), dtype=np.float32)
        self._ck(self.L.cogaps_session_get_matrix(self.h, which.encode(), _fp(out)))
        return out

    def rows(self, which):
        m, n, k = self.dims(which)
        out = np.zeros((m, k), dtype=np.float32)
        self._ck(self.L.cogaps_session_get_rows(self.h, which.encode(), _fp(out)))
        return out

    def ap(self, which):
        m, n, k = self.dims(which)
        out = np.zeros((m, n), dtype=np.float32)
        self._ck(self.L.cogaps_session_get_ap(self.h, which.encode(), _fp(out)))
        return out

    def atoms(self, which, n=None):
        # size query: the library reports the current count through natoms after an update;
        # before any update it is 0
        cap = self.dims(which)[0] * self.dims(which)[2] + (1 << 17)
        pos = np.zeros(cap, dtype=np.uint64)
        mass = np.zeros(cap, dtype=np.float32)
        left = np.zeros(cap, dtype=np.uint32)
        right = np.zeros(cap, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._ck(self.L.cogaps_session_get_atoms(self.h, which.encode(), pos.ctypes.data_as(C.POINTER(C.c_uint64)), _fp(mass),
                                                 left.ctypes.data_as(u32p), right.ctypes.data_as(u32p)))
        n = self.natoms(which) if n is None else n
        return {"pos": pos[:n].copy(), "mass": mass[:n].copy(), "left": left[:n].copy(), "right": right[:n].copy()}

    def avg_queue(self, which):
        a = C.c_float()
        self._ck(self.L.cogaps_session_avg_queue(self.h, which.encode(), C.byref(a)))
        return a.value

    def set_timing(self, on):
        self._ck(self.L.cogaps_session_set_timing(self.h, int(on)))

    def launch_period(self, which):
        """the same launches by their period (entry to the next launch's entry: dispatcher start-up and end-of-kernel write-back included)"""
        m, n = C.c_double(0), C.c_uint64(0)
        pc = (C.c_double * 5)()
        if not hasattr(self.L, "cogaps_session_launch_period"):
            return {"mean_us": 0.0, "p10_us": 0.0, "p50_us": 0.0, "p75_us": 0.0, "p90_us": 0.0, "p99_us": 0.0, "launches": 0}
        self._ck(self.L.cogaps_session_launch_period(self.h, which.encode(), C.byref(m), pc, C.byref(n)))
        return {"mean_us": m.value, "p10_us": pc[0], "p50_us": pc[1], "p75_us": pc[2], "p90_us": pc[3], "p99_us": pc[4], "launches": int(n.value)}

    def launch_clock(self, which):
        """durations of the sampler's chained launches since set_timing(1), every launch (device clock): mean, percentiles, count"""
        m, n = C.c_double(0), C.c_uint64(0)
        pc = (C.c_double * 5)()
        if not hasattr(self.L, "cogaps_session_launch_clock"):
            return {"mean_us": 0.0, "p10_us": 0.0, "p50_us": 0.0, "p75_us": 0.0, "p90_us": 0.0, "p99_us": 0.0, "launches": 0}
        self._ck(self.L.cogaps_session_launch_clock(self.h, which.encode(), C.byref(m), pc, C.byref(n)))
        return {"mean_us": m.value, "p10_us": pc[0], "p50_us": pc[1], "p75_us": pc[2], "p90_us": pc[3], "p99_us": pc[4], "launches": int(n.value)}

    def chained(self, which):
        """whether the sampler's last update ran as chained launches (one launch per batch: csrc/chain_kernel.h)"""
        v = C.c_int()
        self._ck(self.L.cogaps_session_chained(self.h, which.encode(), C.byref(v)))
        return bool(v.value)

    def generator_window(self, which):
        """attempts per round of the sampler's generator launches as of its last update"""
        v = C.c_uint32()
        self._ck(self.L.cogaps_session_generator_window(self.h, which.encode(), C.byref(v)))
        return v.value

    def chain_recoveries(self, which):
        """how often a hand-over inside a chained launch of this sampler never arrived and the batch was completed by the recovery (the sampler
        keeps two launches per batch from the first such event on)"""
        v = C.c_uint32()
        self._ck(self.L.cogaps_session_chain_recoveries(self.h, which.encode(), C.byref(v)))
        return int(v.value)

    def perf(self, which=None):
        p = CogapsPerfC()
        if which is None:
            self._ck(self.L.cogaps_session_perf(self.h, C.byref(p)))
        else:
            self._ck(self.L.cogaps_session_perf_sampler(self.h, which.encode(), C.byref(p)))
        return {f[0]: getattr(p, f[0]) for f in CogapsPerfC._fields_}

    def debug_replay(self, which, kind, n, flags=0):
        us = C.c_double()
        self._ck(self.L.cogaps_session_debug_replay(self.h, which.encode(), kind, n, flags, C.byref(us)))
        return us.value

    def check_domain(self, which):
        """number of broken invariants of the atomic domain's redundant state (0 = consistent)"""
        v = C.c_uint32()
        self._ck(self.L.cogaps_session_debug_check_domain(self.h, which.encode(), C.byref(v)))
        return v.value

    def debug_prof(self, which):
        out = (C.c_uint64 * 16)()
        self._ck(self.L.cogaps_session_debug_prof(self.h, which.encode(), out))
        return list(out)

    def finish(self):
        r = CogapsResultC()
        self._ck(self.L.cogaps_session_finish(self.h, C.byref(r)))
        return result_to_dict(self.L, r)

    def position(self):
        """(phase, next iteration of that phase) as run_iterations / Batch.run_iterations left it; phase 3: both phases complete"""
        ph, it = C.c_int(), C.c_uint32()
        self._ck(self.L.cogaps_session_position(self.h, C.byref(ph), C.byref(it)))
        return ph.value, it.value

    def save_state(self, path):
        """the chain's state into the library's state file (include/cogaps_hip.h): between two iterations; written beside `path`, then renamed"""
        self._ck(self.L.cogaps_session_save_state(self.h, os.fsencode(path)))

    def load_state(self, path):
        """continue the chain a state file holds: this session must be made from the same data and parameters (any input form); a
        refused file leaves it untouched"""
        self._ck(self.L.cogaps_session_load_state(self.h, os.fsencode(path)))

    def run_to_end(self, state_file=None, interval=0):
        """what remains of the two phases from position(), then finish(); with a state file: saved every `interval` iterations (0: not on
        the way), when the run is complete, and before an interrupt ends the call"""
        r = CogapsResultC()
        self._ck(self.L.cogaps_session_run_to_end(self.h, None if state_file is None else os.fsencode(state_file), int(interval), C.byref(r)))
        return result_to_dict(self.L, r)

    def data_digest(self):
        """test hook: the 64-bit digest of the session's data as the state file's fingerprint holds it"""
        v = C.c_uint64(0)
        self._ck(self.L.cogaps_session_debug_data_digest(self.h, C.byref(v)))
        return int(v.value)


def read_matrix_file(path, lib=None, rows=None, cols=None):
    """The library's own reader (csrc/file_reader.h): the file as a dense fp32 matrix.  Host only.  rows / cols (one of them): 1-based
    indices of the rows / columns to keep -- only that part of the file is materialised, in SORTED index order, as the reference's
    workers read their subset of a file (Matrix.cpp:70-134)."""
    L = lib or load()
    nr, nc, ptr = C.c_uint32(), C.c_uint32(), C.POINTER(C.c_float)()
    if rows is not None and cols is not None:
        raise ValueError("rows or cols, not both")
    if rows is None and cols is None:
        rc = L.cogaps_read_matrix_file(os.fsencode(path), C.byref(nr), C.byref(nc), C.byref(ptr))
    else:
        idx = np.ascontiguousarray(rows if rows is not None else cols, dtype=np.uint32)
        rc = L.cogaps_read_matrix_file_subset(os.fsencode(path), int(rows is not None), idx.ctypes.data_as(C.POINTER(C.c_uint32)), idx.size, C.byref(nr), C.byref(nc), C.byref(ptr))
    if rc:
        raise _error(L)
    try:
        return np.ctypeslib.as_array(ptr, shape=(nr.value, nc.value)).copy() if nr.value * nc.value else np.zeros((nr.value, nc.value), np.float32)
    finally:
        L.cogaps_matrix_free(ptr)


def read_mtx_triplets(path, lib=None, rows=None, cols=None):
    """The library's triplet reader (csrc/file_reader.h): the .mtx file as a CooMatrix, its entries in file order, never densified.
    Host only.  rows / cols (one of them): 1-based indices as for read_matrix_file -- the entries of that part of the file, renumbered.
    CooMatrix.toarray() of the result is read_matrix_file of the same arguments."""
    L = lib or load()
    u32p, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    nr, nc, nnz, pr, pc, pv = C.c_uint32(), C.c_uint32(), C.c_uint64(), u32p(), u32p(), fp()
    if rows is not None and cols is not None:
        raise ValueError("rows or cols, not both")
    idx = None if rows is None and cols is None else np.ascontiguousarray(rows if rows is not None else cols, dtype=np.uint32)
    if idx is not None and idx.size == 0:
        raise ValueError("empty subset")
    if L.cogaps_read_mtx_triplets(os.fsencode(path), int(rows is not None), None if idx is None else idx.ctypes.data_as(u32p), 0 if idx is None else idx.size,
                                  C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(pr), C.byref(pc), C.byref(pv)):
        raise _error(L)
    try:
        n = int(nnz.value)
        take = lambda p, dt: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=dt)
        return CooMatrix((nr.value, nc.value), take(pr, np.uint32), take(pc, np.uint32), take(pv, np.float32))
    finally:
        L.cogaps_triplets_free(pr, pc, pv)


def file_info(path, lib=None):
    """getFileInfo_cpp: (nrow, ncol, rowNames, colNames)"""
    L = lib or load()
    nr, nc, rn, cn = C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t()
    if L.cogaps_file_info(os.fsencode(path), C.byref(nr), C.byref(nc), None, 0, C.byref(rn), None, 0, C.byref(cn)):
        raise _error(L)
    rb, cb = C.create_string_buffer(rn.value), C.create_string_buffer(cn.value)
    if L.cogaps_file_info(os.fsencode(path), C.byref(nr), C.byref(nc), rb, rn.value, None, cb, cn.value, None):
        raise _error(L)
    names = lambda b: b.value.decode().split("\n") if b.value else []
    return nr.value, nc.value, names(rb), names(cb)


def run_from_file(path, unc_path=None, lib=None, **kw):
    """cogaps_run_from_file: the reference's file entry point, parsed natively."""
    L = lib if lib is not None else load()
    params = make_params(L, **kw)
    res = CogapsResultC()
    if L.cogaps_run_from_file(os.fsencode(path), C.byref(params), os.fsencode(unc_path) if unc_path else None, C.byref(res)):
        raise _error(L, "cogaps_run_from_file: ")
    return result_to_dict(L, res)


def run(data, unc=None, lib=None, stateFile=None, stateInterval=0, resume=False, **kw):
    """cogaps_run: one full equilibration + sampling run.  With stateFile the run goes through a Session of whatever input form was
    given and cogaps_session_run_to_end: the state is saved every stateInterval iterations (0: not on the way), at the end, and when an
    interrupt ends the run; resume=True continues from the file if it exists (a job that restarts itself) and starts from the
    beginning if it does not."""
    L = lib if lib is not None else load()
    if stateFile is None:
        if resume or stateInterval:
            raise ValueError("resume / stateInterval need a stateFile")
    else:
        s = Session(data, unc=unc, lib=L, **kw)
        try:
            if resume and os.path.exists(stateFile):
                s.load_state(stateFile)
            return s.run_to_end(stateFile, stateInterval)
        finally:
            s.close()
    data, unc, kw = device_input(data, unc, kw)
    p = make_params(L, **kw)
    r = CogapsResultC()
    if isinstance(data, DeviceDense):
        if L.cogaps_run_device(data.data_addr, data.shape[0], data.shape[1], C.byref(p), data.unc_addr, C.byref(r)):
            raise _error(L, "cogaps_run_device: ")
        return result_to_dict(L, r)
    sp = _sparse_input(data, unc, kw)
    if isinstance(sp, DeviceMatrix):
        if L.cogaps_run_device_matrix(sp._handle(), C.byref(p), C.byref(r)):
            raise _error(L, "cogaps_run_device_matrix: ")
        return result_to_dict(L, r)
    if sp is not None:
        m = sp.c_struct()
        name = "cogaps_run_coo" if isinstance(sp, CooMatrix) else "cogaps_run_sparse"
        if getattr(L, name)(C.byref(m), C.byref(p), C.byref(r)):
            raise _error(L, name + ": ")
        return result_to_dict(L, r)
    d = _dense(data)
    u = None if unc is None else _dense(unc)
    rc = L.cogaps_run(_fp(d), d.shape[0], d.shape[1], C.byref(p), None if u is None else _fp(u), C.byref(r))
    if rc:
        raise _error(L, "cogaps_run: ")
    return result_to_dict(L, r)


def debug_math(fn, x, mathMode="portable", on_device=False, lib=None):
    """logf (fn = "log") / expf ("exp") in a math mode of the library, on the device or from the same source on the host"""
    L = lib if lib is not None else load()
    xs = np.ascontiguousarray(x, dtype=np.float32)
    ys = np.zeros_like(xs)
    if L.cogaps_debug_math({"log": 0, "exp": 1}[fn], _MATH[mathMode] if isinstance(mathMode, str) else int(mathMode), _fp(xs), _fp(ys), xs.size, int(on_device)):
        raise _error(L)
    return ys


def debug_udiv64(a, b, on_device=False, lib=None):
    """gm_udiv64(a[i], b[i]) (csrc/gaps_math.h; every b >= 1), on the device or from the same source on the host -> uint64 array"""
    L = lib if lib is not None else load()
    u64p = C.POINTER(C.c_uint64)
    a, b = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1), np.ascontiguousarray(b, dtype=np.uint64).reshape(-1)
    if a.size != b.size:
        raise ValueError("one divisor per dividend")
    q = np.zeros_like(a)
    if L.cogaps_debug_udiv64(a.ctypes.data_as(u64p), b.ctypes.data_as(u64p), q.ctypes.data_as(u64p), a.size, int(on_device)):
        raise _error(L)
    return q


def debug_uniform64(state, lo, hi, on_device=False, lib=None):
    """pcg_uniform64(state[i], lo[i], hi[i]) (csrc/gaps_math.h) -> (values, generator states after the draw), uint64 arrays"""
    L = lib if lib is not None else load()
    u64p = C.POINTER(C.c_uint64)
    s, lo, hi = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in (state, lo, hi))
    if not (s.size == lo.size == hi.size):
        raise ValueError("one state per range")
    v, after = np.zeros_like(s), np.zeros_like(s)
    if L.cogaps_debug_uniform64(s.ctypes.data_as(u64p), lo.ctypes.data_as(u64p), hi.ctypes.data_as(u64p), v.ctypes.data_as(u64p), after.ctypes.data_as(u64p), s.size, int(on_device)):
        raise _error(L)
    return v, after


def _strided(x, dtype, what="a matrix is expected"):
    """x as a matrix of dtype whose strides are whole, non-negative numbers of elements: as it lies where it is one, a contiguous copy otherwise"""
    x = np.asarray(x, dtype=dtype)
    if x.ndim != 2:
        raise ValueError(what)
    if any(st % x.itemsize or st < 0 for st in x.strides):
        x = np.ascontiguousarray(x)
    return x


def _pack_sets(members):
    """per set the member rows -> (off uint64 [nSets + 1], mem uint32: the sets one after the other)"""
    members = [np.asarray(m, dtype=np.uint32).reshape(-1) for m in members]
    off = np.zeros(len(members) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([m.size for m in members], dtype=np.uint64)
    mem = np.ascontiguousarray(np.concatenate(members) if members else np.zeros(0), dtype=np.uint32)
    if mem.size == 0:
        mem = np.zeros(1, dtype=np.uint32)      # (an address to hand over; nothing of it is read)
    return off, mem


def gene_set_stat(z, members, sizes, numPerm, seed=0, device=-1, lib=None):
    """cogaps_gene_set_stat: the permutation counts of the gene-set statistic.  z: the Z matrix (n x K; float64, any strides: a
    column-major array goes in as it is), members: per set the 0-based member rows, ascending; sizes: per set the rows to draw.
    -> (lessThanCount uint32 [nSets][K], actualMean float64 [nSets][K])"""
    L = lib if lib is not None else load()
    z = _strided(z, np.float64, "z must be a matrix")
    off, mem = _pack_sets(members)
    sz = np.ascontiguousarray(sizes, dtype=np.uint32).reshape(-1)
    if sz.size != off.size - 1:
        raise ValueError("one draw size per set")
    cnt = np.zeros((off.size - 1, z.shape[1]), dtype=np.uint32)
    act = np.zeros((off.size - 1, z.shape[1]), dtype=np.float64)
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    if L.cogaps_gene_set_stat(z.ctypes.data_as(dp), z.shape[0], z.shape[1], z.strides[0] // 8, z.strides[1] // 8, off.size - 1,
                              off.ctypes.data_as(C.POINTER(C.c_uint64)), mem.ctypes.data_as(u32p), sz.ctypes.data_as(u32p),
                              int(numPerm), int(seed) & 0xFFFFFFFF, int(device), cnt.ctypes.data_as(u32p), act.ctypes.data_as(dp)):
        raise _error(L)
    return cnt, act


def gene_set_membership(z, members, wMember, wNull=None, device=-1, stat=True, counts=True, allStat=False, lib=None):
    """cogaps_gene_set_membership: the statistic of every member of every set under the set's pattern weights, and the rows outside the
    set that exceed it.  z, members: as for gene_set_stat; wMember, wNull: float64 [nSets][K] (wNull None: = wMember).
    -> {"memberStat": float64 and "greaterCount": uint32, the sets one after the other (members' order); "offsets": where each set
    begins in them; "allStat": float64 [nSets][n]} -- each None unless asked for (stat, counts, allStat)"""
    L = lib if lib is not None else load()
    z = _strided(z, np.float64, "z must be a matrix")
    off, mem = _pack_sets(members)
    nSets, (n, K) = off.size - 1, z.shape
    w = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (wMember, wNull)]
    if any(x is not None and x.shape != (nSets, K) for x in w):
        raise ValueError("one weight per set and column")
    nMem = max(int(off[-1]), 1)
    out = {"memberStat": np.zeros(nMem) if stat else None, "greaterCount": np.zeros(nMem, dtype=np.uint32) if counts else None,
           "allStat": np.zeros((nSets, n)) if allStat else None}
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
    if L.cogaps_gene_set_membership(z.ctypes.data_as(dp), n, K, z.strides[0] // 8, z.strides[1] // 8, nSets,
                                    off.ctypes.data_as(C.POINTER(C.c_uint64)), mem.ctypes.data_as(u32p), ptr(w[0], dp), ptr(w[1], dp), int(device),
                                    ptr(out["memberStat"], dp), ptr(out["greaterCount"], u32p), ptr(out["allStat"], dp)):
        raise _error(L)
    for k in ("memberStat", "greaterCount"):
        if out[k] is not None:
            out[k] = out[k][:int(off[-1])]
    out["offsets"] = off.astype(np.int64)
    return out


def manova_sscp(x, y, device=-1, lib=None):
    """cogaps_manova_sscp: the column means and the centred sums of squares and cross-products of x (n x K, float32) and y (n x p,
    float64, p <= 8), any strides: a column-major array or a slice goes in as it is.
    -> {"xMean" [K], "yMean" [p], "sxx" [K], "sxy" [K][p], "syy" [p][p]}, float64"""
    L = lib if lib is not None else load()
    x, y = _strided(x, np.float32, "x must be a matrix"), _strided(y, np.float64, "y must be a matrix")
    x, y = [np.array(m, order="C") if any(st == 0 and d > 1 for st, d in zip(m.strides, m.shape)) else m for m in (x, y)]      # (a broadcast view)
    sx, sy = [[st // m.itemsize if d > 1 else 1 for st, d in zip(m.strides, m.shape)] for m in (x, y)]      # (numpy's stride of an axis of one element means nothing)
    if x.shape[0] != y.shape[0]:
        raise ValueError("x has %d rows, y %d" % (x.shape[0], y.shape[0]))
    (n, K), p = x.shape, y.shape[1]
    out = {"xMean": np.zeros(K), "yMean": np.zeros(p), "sxx": np.zeros(K), "sxy": np.zeros((K, p)), "syy": np.zeros((p, p))}
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    if L.cogaps_manova_sscp(x.ctypes.data_as(fp), n, K, sx[0], sx[1], y.ctypes.data_as(dp), p, sy[0], sy[1],
                            int(device), *[out[k].ctypes.data_as(dp) for k in ("xMean", "yMean", "sxx", "sxy", "syy")]):
        raise _error(L)
    return out


def permutation_draw(nRows, size, seed, set_index, perm, device=-1, lib=None):
    """cogaps_debug_permutation_draw: the `size` rows of draw (seed, set_index, perm) from nRows rows, by the statistic's kernel code"""
    L = lib if lib is not None else load()
    out = np.zeros(max(int(size), 1), dtype=np.uint32)
    if L.cogaps_debug_permutation_draw(int(nRows), int(size), int(seed) & 0xFFFFFFFF, int(set_index), int(perm), int(device), out.ctypes.data_as(C.POINTER(C.c_uint32))):
        raise _error(L)
    return out[:int(size)]


MARKERS_ALL, MARKERS_CUT = 0, 1       # COGAPS_MARKERS_*


def pattern_markers(A, O, lp=None, threshold="all", device=-1, lib=None):
    """cogaps_pattern_markers: ranks, scores and marker lists of the rows of A (n x K) against the pattern vectors lp (L x K; None: the
    K unit vectors), O (m x K) being the other factor matrix.  A, O: float64, any strides (a column-major array goes in as it is).
    -> (ranks uint32 [n][L], scores float64 [n][L], markers: a list of L uint32 arrays of 0-based rows, best rank first)"""
    L = lib if lib is not None else load()
    if threshold not in ("all", "cut"):
        raise ValueError("threshold must be 'all' or 'cut'")
    A, O = (_strided(x, np.float64, "A and O must be matrices") for x in (A, O))
    if A.shape[1] != O.shape[1]:
        raise ValueError("A and O must have the same number of columns")
    K = A.shape[1]
    if lp is not None:
        lp = [np.asarray(v, dtype=np.float64).reshape(-1) for v in lp]
        if not lp or any(v.size != K for v in lp):
            raise ValueError("lp length must equal the number of columns of the Amatrix")
        lp = np.ascontiguousarray(np.stack(lp))
    nL = K if lp is None else lp.shape[0]
    n = A.shape[0]
    ranks, scores = np.zeros((n, nL), dtype=np.uint32), np.zeros((n, nL), dtype=np.float64)
    markers, count = np.zeros((nL, n), dtype=np.uint32), np.zeros(nL, dtype=np.uint32)
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    if L.cogaps_pattern_markers(A.ctypes.data_as(dp), n, K, A.strides[0] // 8, A.strides[1] // 8,
                                O.ctypes.data_as(dp), O.shape[0], O.strides[0] // 8, O.strides[1] // 8,
                                None if lp is None else lp.ctypes.data_as(dp), 0 if lp is None else nL,
                                MARKERS_ALL if threshold == "all" else MARKERS_CUT, int(device),
                                ranks.ctypes.data_as(u32p), scores.ctypes.data_as(dp), markers.ctypes.data_as(u32p), count.ctypes.data_as(u32p)):
        raise _error(L)
    return ranks, scores, [markers[l, :int(count[l])].copy() for l in range(nL)]


GSEA_MAX_SET = 4096                   # COGAPS_GSEA_MAX_SET


def pattern_gsea(stat, members, numPerm, seed=0, device=-1, ranks=False, lib=None):
    """cogaps_pattern_gsea: the enrichment score of every set in every column of stat (n x K; float32, any strides: a column-major
    array goes in as it is), and its permutation null.  members: per set the 0-based member rows, ascending.
    -> {"es" float64, "peak" uint32, "nGe" uint32, "permSum" uint64: [nSets][K]; with ranks=True "rank": uint32 [K][n], 0-based}"""
    L = lib if lib is not None else load()
    stat = _strided(stat, np.float32)
    off, mem = _pack_sets(members)
    n, K = stat.shape
    shape = (off.size - 1, K)
    out = {"es": np.zeros(shape, dtype=np.float64), "peak": np.zeros(shape, dtype=np.uint32), "nGe": np.zeros(shape, dtype=np.uint32),
           "permSum": np.zeros(shape, dtype=np.uint64)}
    if ranks:
        out["rank"] = np.zeros((K, n), dtype=np.uint32)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    if L.cogaps_pattern_gsea(stat.ctypes.data_as(C.POINTER(C.c_float)), n, K, stat.strides[0] // 4, stat.strides[1] // 4, off.size - 1,
                             off.ctypes.data_as(u64p), mem.ctypes.data_as(u32p), int(numPerm), int(seed) & 0xFFFFFFFF, int(device),
                             out["es"].ctypes.data_as(C.POINTER(C.c_double)), out["peak"].ctypes.data_as(u32p), out["nGe"].ctypes.data_as(u32p),
                             out["permSum"].ctypes.data_as(u64p), out["rank"].ctypes.data_as(u32p) if ranks else None):
        raise _error(L)
    return out


RESIDUAL_DATA_NONE, RESIDUAL_DATA_DENSE, RESIDUAL_DATA_SPARSE, RESIDUAL_DATA_COO, RESIDUAL_DATA_DEVICE_MATRIX = 0, 1, 2, 3, 4      # COGAPS_RESIDUAL_DATA_*


def _residual_data(data, unc, transposeData, device):
    """the cogaps_residual_data descriptor of any kind of input (None: kind _NONE) -> (descriptor, what must stay alive while it is used, device)"""
    desc, keep = CogapsResidualDataC(), []
    desc.kind, desc.transposeData = RESIDUAL_DATA_NONE, int(bool(transposeData))
    if data is not None:
        data, unc, kw = device_input(data, unc, {"device": device})
        device = kw["device"]
        if is_sparse(data):
            data = SparseMatrix.from_scipy(data)
        if isinstance(data, (SparseMatrix, CooMatrix, DeviceMatrix)):
            if unc is not None:
                raise ValueError("a sparse matrix takes no uncertainty matrix: the default uncertainty only")
            if isinstance(data, DeviceMatrix):
                desc.kind, desc.deviceMatrix = RESIDUAL_DATA_DEVICE_MATRIX, data._handle()
            else:
                m = data.c_struct()
                keep.append(m)
                if isinstance(data, CooMatrix):
                    desc.kind, desc.coo = RESIDUAL_DATA_COO, C.addressof(m)
                else:
                    desc.kind, desc.sparse = RESIDUAL_DATA_SPARSE, C.addressof(m)
        elif isinstance(data, DeviceDense):
            desc.kind, desc.onDevice = RESIDUAL_DATA_DENSE, 1
            desc.nrow, desc.ncol = data.shape
            desc.dense, desc.uncertainty = data.data_addr, data.unc_addr
            desc.rowStride, desc.colStride = data.shape[1], 1
        else:
            d = _strided(data, np.float32)
            u = None if unc is None else _strided(unc, np.float32)
            if u is not None:
                if u.shape != d.shape:
                    raise ValueError("the uncertainty matrix must have the shape of the data")
                if u.strides != d.strides:      # one pair of strides serves both
                    d, u = np.ascontiguousarray(d), np.ascontiguousarray(u)
            keep += [d, u]
            desc.kind, desc.onDevice = RESIDUAL_DATA_DENSE, 0
            desc.nrow, desc.ncol = d.shape
            desc.dense, desc.uncertainty = d.ctypes.data, None if u is None else u.ctypes.data
            desc.rowStride, desc.colStride = d.strides[0] // 4, d.strides[1] // 4
        keep.append(data)
    elif unc is not None:
        raise ValueError("an uncertainty matrix without data")
    return desc, keep, device


def residuals(A, P, data=None, unc=None, rows=None, transposeData=False, device=-1, lib=None):
    """cogaps_residuals: how well A (genes x K) and P (samples x K), float32 with any strides, fit `data`.  data: None (the
    reconstruction A P^T alone), a dense matrix (numpy, any strides -- a column-major array goes in as it is; a torch tensor or a
    DeviceDense on the GPU is read where it lies) with an optional `unc` of its shape, or a scipy.sparse matrix, SparseMatrix, CooMatrix
    or DeviceMatrix (never densified; the default uncertainty only).  rows: 0-based genes whose rows of the residual matrix (of the
    reconstruction without data) are wanted, any order, repeats allowed.  -> {"matrix": float64 [len(rows)][samples] or None,
    "geneChiSq", "sampleChiSq": float64 vectors, "chiSq": float (the three are None without data), "peakDeviceBytes": int}"""
    L = lib if lib is not None else load()
    A, P = _strided(A, np.float32), _strided(P, np.float32)
    if A.shape[1] != P.shape[1]:
        raise ValueError("featureLoadings has %d patterns, sampleFactors %d" % (A.shape[1], P.shape[1]))
    G, N, K = A.shape[0], P.shape[0], A.shape[1]
    desc, keep, device = _residual_data(data, unc, transposeData, device)
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    idx = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    n_out = 0 if idx is None else idx.size
    out = np.zeros((n_out, N), dtype=np.float64) if n_out else None
    have = desc.kind != RESIDUAL_DATA_NONE
    gene, sample, chi = np.zeros(G if have else 0), np.zeros(N if have else 0), C.c_double(0.0)
    peak = C.c_uint64(0)
    if L.cogaps_residuals(_fp(A), G, A.strides[0] // 4, A.strides[1] // 4, _fp(P), N, P.strides[0] // 4, P.strides[1] // 4, K,
                          C.byref(desc) if have else None, idx.ctypes.data_as(u32p) if n_out else None, n_out, int(device),
                          gene.ctypes.data_as(dp) if have else None, sample.ctypes.data_as(dp) if have else None, C.byref(chi) if have else None,
                          out.ctypes.data_as(dp) if n_out else None, C.byref(peak)):
        raise _error(L)
    return {"matrix": out, "geneChiSq": gene if have else None, "sampleChiSq": sample if have else None,
            "chiSq": float(chi.value) if have else None, "peakDeviceBytes": int(peak.value)}


PROJECT_TRIP, PROJECT_MAX_PATTERNS = 1024, 128       # COGAPS_PROJECT_TRIP, COGAPS_PROJECT_MAX_PATTERNS


def project(L, data, rows=None, transposeData=False, device=-1, lib=None):
    """cogaps_project: every sample of `data` regressed on the loadings L (genes x K, float32, any strides) by least squares
    (DESIGN.md 4.15).  data: what residuals() takes, without an uncertainty; rows: None (gene i is row i of the data) or, per gene of L,
    its 0-based row of the data, any order, repeats allowed.  -> {"coef", "cross": float64 [K][samples], "gram": [K][K],
    "stdevUnscaled": [K], "rss": [samples], "peakDeviceBytes": int}"""
    lib_ = lib if lib is not None else load()
    L = _strided(L, np.float32, "the loadings must be a matrix")
    if any(st == 0 and d > 1 for st, d in zip(L.strides, L.shape)):      # (a broadcast view)
        L = np.array(L, order="C")
    n, K = L.shape
    sl = [st // 4 if d > 1 else 1 for st, d in zip(L.strides, L.shape)]      # (numpy's stride of an axis of one element means nothing)
    if data is None:
        raise ValueError("there is no data to project")
    desc, keep, device = _residual_data(data, None, transposeData, device)
    if desc.kind == RESIDUAL_DATA_DENSE:
        S = desc.nrow if transposeData else desc.ncol
    elif desc.kind == RESIDUAL_DATA_DEVICE_MATRIX:
        S = data.shape[0 if transposeData else 1]
    else:
        S = keep[0].nrow if transposeData else keep[0].ncol
    idx = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
    if idx is not None and idx.size != n:
        raise ValueError("one data row per gene of the loadings: %d rows for %d genes" % (idx.size, n))
    out = {"coef": np.zeros((K, S)), "rss": np.zeros(S), "gram": np.zeros((K, K)), "stdevUnscaled": np.zeros(K), "cross": np.zeros((K, S))}
    peak = C.c_uint64(0)
    dp = C.POINTER(C.c_double)
    if lib_.cogaps_project(_fp(L), n, sl[0], sl[1], K, C.byref(desc), None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)), int(device),
                           *[out[k].ctypes.data_as(dp) for k in ("coef", "rss", "gram", "stdevUnscaled", "cross")], C.byref(peak)):
        raise _error(lib_)
    out["peakDeviceBytes"] = int(peak.value)
    return out


PATTERN_MATCH_MAX_COLS = 4096         # COGAPS_PATTERN_MATCH_MAX_COLS


def pattern_match(patterns, cut, minNS, maxNS, device=-1, lib=None, debug=False):
    """cogaps_pattern_match: the consensus of the gathered patterns (L x n, one pattern per column).  patterns: a numpy
    array (float32, any strides: a column-major array goes in as it is) or a torch tensor -- on the GPU it goes by address, like a
    DeviceDense, after its stream is synchronised, and `device` follows it.
    -> {"nClusters": int, "cluster": uint32 [n] (1-based, in the order of clusteredPatterns; 0: dropped), "corr": float64 [n] (the rounded
    correlation with the cluster's mean pattern; NaN: dropped), "consensus": float32 [L][nClusters]; with debug=True "dist": float64
    [n][n] and "firstLabels": uint32 [n], the labels of the first corcut before its minNS filter}"""
    L = lib if lib is not None else load()
    keep, on_device = None, 0
    if on_gpu(patterns):
        import torch
        if patterns.dim() != 2:
            raise ValueError("patterns must be a matrix")
        dev = patterns.device.index if patterns.device.index is not None else torch.cuda.current_device()
        if int(device) not in (-1, dev):
            raise ValueError("the pattern tensor resides on device %d, the call was given device=%d" % (dev, int(device)))
        keep = patterns.detach()
        if keep.dtype != torch.float32 or any(st < 0 for st in keep.stride()):
            keep = keep.to(dtype=torch.float32).contiguous()
        torch.cuda.current_stream(keep.device).synchronize()
        addr, shape, strides, device, on_device = keep.data_ptr(), tuple(keep.shape), tuple(keep.stride()), dev, 1
    else:
        if is_tensor(patterns):
            patterns = patterns.detach().cpu().numpy()
        keep = _strided(patterns, np.float32, "patterns must be a matrix")
        addr, shape, strides = keep.ctypes.data, keep.shape, tuple(st // 4 for st in keep.strides)
    rows, n = int(shape[0]), int(shape[1])
    count = C.c_uint32(0)
    cluster, corr = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.float64)
    consensus = np.empty(max(rows * n, 1), dtype=np.float32)
    dist = np.zeros((n, n), dtype=np.float64) if debug else None
    first = np.zeros(max(n, 1), dtype=np.uint32) if debug else None
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    if L.cogaps_pattern_match(addr, rows, n, strides[0], strides[1], on_device, int(cut), int(minNS), int(maxNS), int(device),
                              C.byref(count), cluster.ctypes.data_as(u32p), corr.ctypes.data_as(dp), _fp(consensus),
                              dist.ctypes.data_as(dp) if debug else None, first.ctypes.data_as(u32p) if debug else None):
        raise _error(L)
    k = int(count.value)
    out = {"nClusters": k, "cluster": cluster[:n], "corr": corr[:n], "consensus": consensus[:rows * k].reshape(rows, k).copy()}
    if debug:
        out["dist"], out["firstLabels"] = dist, first[:n]
    return out


def device_memory(device=-1, lib=None):
    """(free, total) bytes of HBM on `device` (-1: the calling thread's current one)"""
    L = lib if lib is not None else load()
    f, t = C.c_uint64(0), C.c_uint64(0)
    if L.cogaps_device_memory(int(device), C.byref(f), C.byref(t)):
        raise _error(L)
    return int(f.value), int(t.value)


def current_device(lib=None):
    """hipGetDevice for the calling host thread"""
    L = lib if lib is not None else load()
    d = C.c_int(0)
    if L.cogaps_current_device(C.byref(d)):
        raise _error(L)
    return d.value


class Batch:
    """Batched multi-chain launches (cogaps_batch_* of include/cogaps_hip.h): the given sessions stepped in lock-step by one stream,
    one generator / evaluation launch for all of them.  Every chain gives the bits it gives on its own."""

    def __init__(self, sessions):
        self.sessions = list(sessions)
        self.L = self.sessions[0].L
        arr = (C.c_void_p * len(self.sessions))(*[s.h for s in self.sessions])
        self.h = self.L.cogaps_batch_create(arr, len(self.sessions))
        if not self.h:
            raise _error(self.L, "cogaps_batch_create: ")

    def _ck(self, rc):
        if rc:
            raise _error(self.L)

    def run_iterations(self, phase, first, n):
        upd = (C.c_uint64 * len(self.sessions))()
        self._ck(self.L.cogaps_batch_run_iterations(self.h, phase, first, n, upd))
        return [int(u) for u in upd]

    def set_timing(self, on):
        self._ck(self.L.cogaps_batch_set_timing(self.h, int(on)))

    def perf(self, side):
        g, e, n, l = C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()
        self._ck(self.L.cogaps_batch_perf(self.h, {"A": 0, "P": 1}[side], C.byref(g), C.byref(e), C.byref(n), C.byref(l)))
        return {"gen_us": g.value, "eval_us": e.value, "sampled": n.value, "launches": l.value}

    def close(self):
        if getattr(self, "h", None):
            self.L.cogaps_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_batch(datas, uncs=None, lib=None, kws=None, **common):
    """cogaps_run for several chains at once through the batched launches: datas[i] with the keyword arguments kws[i] (merged over
    `common`) -- or ONE iterable of (data, uncertainty, keyword arguments) triples, consumed one at a time: a chain's host matrices
    are released as soon as its session holds them in HBM.  All chains need the same nIterations.  Returns the result dicts in order."""
    L = lib if lib is not None else load()
    if uncs is None and kws is None and not isinstance(datas, (list, tuple)):
        triples = datas
    else:
        kws = kws or [{} for _ in datas]
        uncs = uncs or [None] * len(datas)
        triples = zip(datas, uncs, kws)
    ss, b = [], None
    try:
        for d, u, k in triples:
            s_ = Session(d, unc=u, lib=L, **dict(common, **k))
            s_.d = s_.u = None                # the library copied them at creation (cogaps_session_create)
            ss.append(s_)
            del d, u
        n_iter = {int(s.p.nIterations) for s in ss}
        if len(n_iter) != 1:
            raise ValueError("the chains of a batch need the same nIterations")
        n_iter = n_iter.pop()
        b = Batch(ss)
        b.run_iterations(1, 0, n_iter)
        b.run_iterations(2, 0, n_iter)
        return [s.finish() for s in ss]
    finally:
        if b is not None:
            b.close()
        for s in ss:
            s.close()
