"""CoGAPS() -- the reference's user entry point (R/CoGAPS.R:90-155) over the HIP library.

Same arguments and defaults; `data` is a 2-D array (genes x samples unless transposeData; a numpy array or a torch tensor -- a tensor
on the GPU is checked and consumed there, with its uncertainty, and never copied to the host; results stay numpy), a scipy.sparse matrix
(with sparseOptimization=True it is never densified), a DeviceMatrix (a matrix uploaded to the GPU once: any number of runs, subsets
and distributed shards are then taken from it on the device; sparseOptimization=True only) or a path to a .mtx/.csv/.tsv file (a .mtx file with sparseOptimization=True
is read as triplets by the library and never densified either).  The standard run dispatches to cogaps_run (the C-ABI replacement of gaps::run);
`distributed` = "genome-wide" / "single-cell" dispatches to cogaps_amd.distributed (GWCoGAPS / scCoGAPS).

stateFile / stateInterval / resume (a standard run only): the library's own state file (include/cogaps_hip.h, cogaps_session_run_to_end) --
the run saves its chain every stateInterval iterations, at its end and when it is interrupted, and resume=True continues the chain the file
holds, bit for bit (from the beginning if there is no file).  Not the reference's checkpoints: checkpointInFile stays refused.
"""
import warnings

import numpy as np

from . import _capi
from .io import read_matrix
from .params import CogapsParams
from .result import CogapsResult


def check_values(data, uncertainty):
    """checkDataMatrix's rules for the values (R/HelperFunctions.R:194-207): no NA, nothing negative in the data or the uncertainty"""
    # a scipy.sparse matrix: its stored entries (the rest are zeros); triplets read from a file: their values
    if isinstance(data, _capi.DeviceMatrix):
        # a device-resident matrix: what its host values showed when it was built (nothing is known of arrays that were on the device already)
        has_na, has_negative = bool(data.has_na), bool(data.has_negative)
    else:
        values = data.values if isinstance(data, (_capi.CooMatrix, _capi.SparseMatrix)) else data.data if _capi.is_sparse(data) else data
        if getattr(data, "on_device", False):
            values = np.zeros(0, np.float32)                     # (device arrays given by address: never seen here)
        # (a tensor on the GPU: torch evaluates the same tests there, one flag each comes to the host)
        has_na = bool(values.isnan().any()) if _capi.is_tensor(values) else np.isnan(values).any()
        has_negative = bool((values < 0).any())
    if has_na:
        raise ValueError("NA values in data")
    if has_negative or (uncertainty is not None and bool((uncertainty < 0).any())):
        raise ValueError("negative values in data and/or uncertainty matrix")


def warn_small_uncertainty(uncertainty):
    if uncertainty is not None and bool((uncertainty < 1e-5).any()):
        warnings.warn("small values in uncertainty matrix detected")


def check_inputs(data, uncertainty, params, snapshotPhase="sampling", nSnapshots=0, checkpointInFile=None, nThreads=1):
    """R/HelperFunctions.R:194-249 (checkDataMatrix + checkInputs)"""
    if uncertainty is not None and params.sparseOptimization:
        raise ValueError("must use default uncertainty when enabling sparseOptimization")
    if checkpointInFile is not None:
        raise ValueError("CoGAPS was built with checkpoints disabled")
    if snapshotPhase not in ("equilibration", "sampling", "all"):
        raise ValueError("snapshotPhase must be either equilibration, sampling, or all")
    if params.distributed is not None and nThreads > 1:
        warnings.warn("can't run multi-threaded and distributed CoGAPS at the same time, ignoring nThreads")
    check_values(data, uncertainty)
    if data.shape[0] <= params.nPatterns or data.shape[1] <= params.nPatterns:
        raise ValueError("nPatterns must be less than dimensions of data")
    warn_small_uncertainty(uncertainty)


def CoGAPS(data, params=None, nPatterns=None, nThreads=1, messages=True, outputFrequency=1000, uncertainty=None,
           checkpointOutFile="gaps_checkpoint.out", checkpointInterval=0, checkpointInFile=None, transposeData=False,
           BPPARAM=None, workerID=1, asynchronousUpdates=True, nSnapshots=0, snapshotPhase="sampling", device=-1,
           stateFile=None, stateInterval=0, resume=False, sampler=None, consensus="host", **extra):
    if params is None:
        params = CogapsParams(**({} if nPatterns is None else {"nPatterns": nPatterns}))
    else:
        params = params.copy()                                   # value semantics of the S4 object: the caller's params stay as they are
        if nPatterns is not None:
            params.setParam("nPatterns", nPatterns)
    for k, v in extra.items():                                   # parseExtraParams: named CogapsParams slots in ...
        params.setParam(k, v)
    if sampler is not None:                                      # "async" | "sequential" (CogapsParams.sampler; include/cogaps_hip.h)
        params.setParam("sampler", sampler)
    params.validate()
    if consensus not in ("host", "device"):                      # where a distributed run matches its patterns (distributed.py)
        raise ValueError("consensus must be 'host' or 'device', not %r" % (consensus,))
    path = data if isinstance(data, str) else None
    subset = params.subsetIndices is not None and params.subsetDim > 0     # a distributed worker's call: the run takes these rows / columns only
    subset_by_rows = (params.subsetDim == 1) != bool(transposeData)         # genes are the data's rows unless transposeData
    if path is not None and params.sparseOptimization and path.lower().endswith(".mtx"):
        # a Matrix Market file reaches the sparse model as triplets (the library's reader, cogaps_run_coo): never densified
        # The reader takes a subset the way the reference's workers read theirs: sorted, a repeated index once.  The dense entry takes
        # the indices in the order given.  The two agree for strictly ascending indices inside the matrix -- what a distributed caller
        # sends; anything else keeps the dense read, its results and its messages.  The order of the indices is tested first, so that
        # such a call parses the file once, densely; only an index past the matrix, an error in the end, costs both reads.
        idx = np.asarray(params.subsetIndices, dtype=np.int64).ravel() if subset else None
        if subset and not (idx.size and idx[0] >= 1 and (np.diff(idx) > 0).all()):
            data = read_matrix(path)
        else:
            data = _capi.read_mtx_triplets(path)
            if subset and idx[-1] > data.shape[0 if subset_by_rows else 1]:
                data = read_matrix(path)
    elif path is not None:
        data = read_matrix(path)
    if isinstance(uncertainty, str):
        uncertainty = read_matrix(uncertainty)
    unc = uncertainty
    if _capi.is_tensor(data) or _capi.is_tensor(unc):
        # a CPU tensor is its numpy view; a GPU tensor stays where it is, as contiguous fp32 (converted on its device), and so does its
        # uncertainty: the checks below run there, the library builds its session from the two arrays on the device
        if _capi.on_gpu(data):
            import torch
            if device not in (-1, None) and device != data.device.index:
                raise ValueError("the data tensor resides on device %d, the run was given device=%d" % (data.device.index, device))
            device = data.device.index
            data = data.detach().to(dtype=torch.float32).contiguous()
            if unc is not None:
                unc = (unc.detach() if _capi.is_tensor(unc) else torch.from_numpy(np.ascontiguousarray(unc))).to(device=data.device, dtype=torch.float32).contiguous()
        else:
            data, unc, _ = _capi.device_input(data, unc, {})
    if _capi.on_gpu(data):
        pass
    elif isinstance(data, _capi.DeviceMatrix):
        # uploaded and validated once by the caller; every run from it is a sparse-model session (the subset, if any, is taken on the device)
        if not params.sparseOptimization:
            raise ValueError("a DeviceMatrix needs sparseOptimization=True: the dense model takes a dense matrix")
    elif isinstance(data, _capi.CooMatrix):
        pass
    elif _capi.is_sparse(data):
        # a scipy.sparse matrix reaches the sparse model in compressed form (never densified: cogaps_session_create_sparse); the dense
        # model takes a dense matrix
        data = data.astype(np.float32) if params.sparseOptimization else np.ascontiguousarray(data.toarray(), dtype=np.float32)
    else:
        data = np.ascontiguousarray(data, dtype=np.float32)
    if unc is not None and not _capi.on_gpu(unc):
        unc = np.ascontiguousarray(unc, dtype=np.float32)
    check_inputs(data, unc, params, snapshotPhase, nSnapshots, checkpointInFile, nThreads)
    if not asynchronousUpdates:
        raise ValueError("asynchronousUpdates=FALSE is not taken here: the reference's sequential sampler is selected with sampler=\"sequential\"")
    if stateFile is None and (resume or stateInterval):
        raise ValueError("resume / stateInterval need a stateFile")
    if params.distributed is not None:
        if stateFile is not None:
            raise ValueError("the distributed drivers do not take a state file yet (stateFile / stateInterval / resume serve a standard run)")
        from .distributed import distributedCogaps
        if isinstance(data, _capi.CooMatrix):
            data = data.tocsr()                                  # the shard code cuts a scipy.sparse matrix (repeats resolved on the host: the last entry decides)
        # BPPARAM: the reference hands the subsets to that many BiocParallel workers (R/DistributedCogaps.R:60-63); here: shards in
        # flight per GPU, run as batches of lock-stepped chains (an int, or an object with a `workers` attribute; default 16 = two batches of eight)
        in_flight = 16 if BPPARAM is None else int(getattr(BPPARAM, "workers", BPPARAM))
        raw = distributedCogaps(data, params, unc, messages=messages, outputFrequency=outputFrequency, transposeData=transposeData, device=device,
                                shardsInFlight=in_flight, nSnapshots=nSnapshots, snapshotPhase=snapshotPhase, consensus=consensus)
    else:
        subset_kw = dict(subsetIndices=params.subsetIndices, subsetDim=params.subsetDim)
        if subset and isinstance(data, _capi.CooMatrix):
            # the whole file's triplets were checked above, as the whole matrix is for every other input; the run gets the subset's, taken
            # by the reader (as cogaps_run_from_file does), and has no subset left to take.  That is a second parse of the file: a worker
            # pays it for checks that see the whole matrix, as they do on every other route, and holds the subset's triplets only
            data = _capi.read_mtx_triplets(path, **{"rows" if subset_by_rows else "cols": params.subsetIndices})
            subset_kw = dict(runningDistributed=True)
        raw = _capi.run(data, unc=unc, nPatterns=params.nPatterns, nIterations=params.nIterations, seed=params.seed,
                        outputFrequency=outputFrequency, nThreads=nThreads, alphaA=params.alphaA, alphaP=params.alphaP,
                        maxGibbsMassA=params.maxGibbsMassA, maxGibbsMassP=params.maxGibbsMassP, transposeData=transposeData,
                        whichMatrixFixed=params.whichMatrixFixed, **subset_kw,
                        fixedPatterns=params.fixedPatterns, sparseOptimization=params.sparseOptimization, messages=messages,
                        workerID=workerID, device=device, takePumpSamples=params.takePumpSamples,
                        nSnapshots=nSnapshots, snapshotPhase=snapshotPhase, sampler=params.sampler,
                        **({} if stateFile is None else dict(stateFile=stateFile, stateInterval=stateInterval, resume=resume)))
    return CogapsResult(raw, params=params, geneNames=params.geneNames, sampleNames=params.sampleNames)


def GWCoGAPS(data, params=None, nPatterns=None, **kw):
    """R/CoGAPS.R:213-224"""
    params = params.copy() if params is not None else CogapsParams(**({} if nPatterns is None else {"nPatterns": nPatterns}))
    params.distributed = "genome-wide"
    return CoGAPS(data, params, nPatterns, **kw)


def scCoGAPS(data, params=None, nPatterns=None, **kw):
    """R/CoGAPS.R:173-184"""
    params = params.copy() if params is not None else CogapsParams(**({} if nPatterns is None else {"nPatterns": nPatterns}))
    params.distributed = "single-cell"
    params.sparseOptimization = kw.pop("sparseOptimization", params.sparseOptimization)
    return CoGAPS(data, params, nPatterns, **kw)
