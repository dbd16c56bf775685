/*
 * cogaps_hip.h -- C ABI of libcogaps_hip.so, the MI355X (gfx950) implementation of the CoGAPS
 * asynchronous Gibbs sampler hot path.
 *
 * The boundary it replaces is the reference's language-neutral core entry
 *     GapsResult gaps::run(const Matrix &data, GapsParameters &params,
 *                          const Matrix &uncertainty, GapsRandomState *randState)
 * (reference src/GapsRunner.h:17-22, src/GapsRunner.cpp:113-123), which Rcpp's cogaps_cpp
 * (src/Cogaps.cpp:205-215, R/RcppExports.R:8-10) reaches through cogapsRun (src/Cogaps.cpp:148-186).
 * INTEGRATION.md shows the Rcpp stub that binds these entry points in place of gaps::run.
 *
 * Plain pointers and sizes only; the callee copies its inputs; results are callee-allocated and
 * released with cogaps_result_free.  All functions return 0 on success and a non-zero code plus a
 * message (cogaps_last_error) on failure; nothing calls exit() (reference: utils/GapsAssert.h:19-25).
 * Threading: a session (or a cogaps_run call) is driven by one host thread at a time; different sessions may run
 * concurrently from different host threads, on the same GPU or on different ones (each owns one non-blocking
 * stream and the library creates no other; no legacy-stream operation is issued; graph capture is thread-local).
 * Up to four sessions per process and GPU run truly side by side (HIP's four hardware queues per process).  The library keeps no global
 * mutable state besides the per-thread last error and, per device, a count of the updates in flight on it (a chained launch, which wants
 * the whole chip, is taken only by an update -- a session's or a batch's -- that runs alone on its GPU).
 * Environment, all optional, none changes a result; each is read when a session is created and has its test (tests/test_gpu_parity.py):
 *   COGAPS_NO_GRAPH (any value)  every kernel as a plain launch instead of replaying captured graphs -- for counter-collection tools
 *                                (tools/pmc_pass.sh); the whole -m gpu suite passes with it
 *   COGAPS_NO_CHAIN              two launches per batch instead of the chained launch: A/B runs, test_chained_equals_two_launches_on_the_gpu
 *   COGAPS_FORCE_CHAIN           the fused evaluation's chained launch also where the device shows fewer compute units than the launch has
 *                                workgroups, or another update is in flight: test_chained_launch_with_half_the_compute_units.  (Not the split
 *                                evaluation's: its update items wait for deciding workgroups of higher index, every workgroup must be resident.)
 *   COGAPS_CHAIN_SPLIT           the split evaluation (data vectors of more than 4096 elements) inside the chained launch -- built, measured
 *                                6 % slower on the headline chain (profiles/r05_ab_chained_split_evaluation_not_kept.txt), not the default:
 *                                test_chained_split_evaluation_equals_two_launches_on_the_gpu
 *   COGAPS_TEST_WIDE_WINDOW      the sparse model's chained launch with its widest generator window (448 attempts) from the first update on; the
 *                                library takes it by itself once a sampler's batches exceed 230 proposals:
 *                                test_sparse_chained_launch_with_long_queues_equals_two_launches_on_the_gpu
 * Development builds (-DCOGAPS_DEV, never shipped) read further switches that only change what is measured.
 */
#ifndef COGAPS_HIP_H
#define COGAPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* POD mirror of GapsParameters (reference src/GapsParameters.h:35-66; defaults :79-111) */
typedef struct cogaps_params {
    uint32_t seed;
    uint32_t nPatterns;          /* default 3 */
    uint32_t nIterations;        /* default 1000, per phase */
    uint32_t maxThreads;         /* accepted for API parity; the GPU path ignores it */
    uint32_t outputFrequency;    /* default 500 */
    uint32_t checkpointInterval; /* accepted, must be 0 (checkpoints are disabled, Cogaps.cpp:224-231) */
    uint32_t snapshotFrequency;  /* GapsRunner.cpp:316-322: a copy of A and P every so many iterations of the snapshot phase(s); 0 = none.
                                    cogaps_cpp derives it as nIterations / nSnapshots (Cogaps.cpp:104-109) */
    float alphaA, alphaP;        /* default 0.01 */
    float maxGibbsMassA, maxGibbsMassP; /* default 100 */
    int32_t transposeData;
    int32_t printMessages;
    int32_t subsetData;          /* dataIndicesSubset in use */
    int32_t subsetGenes;         /* subsetDim == 1 (rows of A) else samples */
    const uint32_t *dataIndicesSubset; /* 1-based indices, as R passes them (Matrix.cpp:55-62) */
    uint32_t nSubset;
    int32_t useSparseOptimization; /* SparseNormalModel (default uncertainty only) instead of DenseNormalModel.  The sparse model takes at
                                      most 512 patterns: a larger nPatterns is refused at session creation, whatever the input form */
    int32_t takePumpSamples;       /* GapsStatistics::updatePump per sampling iteration (GapsRunner.cpp:310-313) */
    int32_t asynchronousUpdates;   /* must be 1: this library IS the asynchronous sampler.  One exception: 0 is accepted, and ignored, when
                                      runningDistributed is set -- R's distributed caller forces FALSE on its workers (R/DistributedCogaps.R:28-29) */
    char whichMatrixFixed;         /* 'N', 'A' or 'P' */
    const float *fixedPatterns;    /* row-major [fixedRows][nPatterns] when whichMatrixFixed != 'N' */
    uint32_t fixedRows;
    uint32_t workerID;
    int32_t runningDistributed;
    int32_t device;                /* HIP device ordinal, -1 = the creating thread's current one (resolved at session creation; every later call on the session selects that GPU for its calling thread) */
    int (*interrupt)(void *);      /* polled once per iteration (GapsRunner.cpp:280); non-zero aborts */
    void *interruptArg;
    int32_t snapshotPhase;         /* 0 = all phases (GAPS_ALL_PHASES, the default of GapsParameters.h:98), 1 = equilibration, 2 = sampling */
    int32_t pumpThreshold;         /* PumpThreshold (GapsParameters.h:52; GapsStatistics.h:58-63): 0 = PUMP_UNIQUE (default), 1 = PUMP_CUT.
                                      The reference's two rules are the same code (GapsStatistics.h:65-126) and so are they here */
    int32_t fixedCols;             /* columns of fixedPatterns; 0 = nPatterns.  Anything else is rejected (GapsRunner.cpp:329-350 copies
                                      nPatterns columns) */
    /* ---- verification mode: no counterpart in GapsParameters -------------------------------------------------------------
     * reductionMode COGAPS_REDUCE_LANES (default): the kernels' lane order (cogaps_reduction_width).  COGAPS_REDUCE_SEQ: every
     * floating-point sum runs in the order of the reference's default scalar build (src/math/SIMD.h:36-47: one accumulator,
     * i = 0 .. N-1; chiSq DenseNormalModel.cpp:56-68; gaps::dot VectorMath.h:41-134) -- slow, and bit-identical to that build.
     * mathMode (honoured with COGAPS_REDUCE_SEQ): the logf / expf of the accept tests and draws.  COGAPS_MATH_PORTABLE
     * (default): the kernels' own correctly rounded algorithm.  COGAPS_MATH_GLIBC_FMA / _SSE2: GNU libc 2.35's logf / expf
     * restated (its -mfma ifunc variant, which x86-64 glibc selects on FMA-capable hosts / its generic variant) -- what the
     * reference binary computes when it is linked against that C library.  With SEQ + GLIBC the HIP library reproduces the
     * reference's atom histories, totalUpdates and statistics digit for digit (tests/test_gpu_parity.py). */
    int32_t reductionMode;
    int32_t mathMode;
    /* ---- which of the reference's two samplers runs (GapsRunner.cpp:69-77) ------------------------------------------------
     * COGAPS_SAMPLER_ASYNC (default): AsynchronousGibbsSampler.  COGAPS_SAMPLER_SEQUENTIAL: SingleThreadedGibbsSampler -- one
     * generator per sampler, no queue; what every worker of the reference's GWCoGAPS / scCoGAPS runs (R/DistributedCogaps.R:28-29).
     * One workgroup runs a whole update (csrc/seq_kernel.h); a cogaps_batch of sequential sessions is one launch with a workgroup
     * per chain.  Dense model only (useSparseOptimization is refused); no state file (cogaps_session_save_state / _load_state and
     * cogaps_session_run_to_end with a path are refused); averageQueueLengthA / P are 0; a batch cannot mix samplers.
     * asynchronousUpdates keeps its meaning above and does NOT select this sampler.  Any other value is refused. */
    int32_t sampler;
} cogaps_params;
#define COGAPS_SAMPLER_ASYNC 0
#define COGAPS_SAMPLER_SEQUENTIAL 1
#define COGAPS_REDUCE_LANES 0
#define COGAPS_REDUCE_SEQ 1
#define COGAPS_MATH_PORTABLE 0
#define COGAPS_MATH_GLIBC_FMA 1
#define COGAPS_MATH_GLIBC_SSE2 2

/* POD mirror of GapsResult (reference src/GapsResult.h:17-36) + the names cogapsRun returns */
typedef struct cogaps_result {
    uint32_t nGenes, nSamples, nPatterns;
    float *Amean, *Asd;          /* row-major [nGenes][nPatterns] */
    float *Pmean, *Psd;          /* row-major [nSamples][nPatterns] */
    uint32_t nHistory;
    float *chisqHistory;         /* diagnostics$chisq */
    uint32_t *atomHistoryA;      /* diagnostics$atomsA */
    uint32_t *atomHistoryP;      /* diagnostics$atomsP */
    uint64_t totalUpdates;
    uint32_t seed;
    uint32_t totalRunningTime;   /* seconds */
    float meanChiSq;
    float averageQueueLengthA, averageQueueLengthP;
    double samplerSeconds;       /* wall time of the two phases, for proposals/s */
    float *pumpMatrix;           /* diagnostics$pumpStat, row-major [nGenes][nPatterns]; NULL unless takePumpSamples */
    float *meanPatternAssignment;/* diagnostics$meanPatternAssignment, same shape */
    uint32_t nEquilibrationSnapshots, nSamplingSnapshots;
    float *equilibrationSnapshotsA, *equilibrationSnapshotsP;   /* [n][rows][nPatterns] row-major */
    float *samplingSnapshotsA, *samplingSnapshotsP;
} cogaps_result;

void cogaps_default_params(cogaps_params *p);

/* gaps::run for an in-memory matrix: data row-major [nrow][ncol] fp32 (genes x samples unless
 * transposeData), uncertainty the same shape or NULL.  Host pointers. */
int cogaps_run(const float *data, uint32_t nrow, uint32_t ncol, const cogaps_params *params,
               const float *uncertainty, cogaps_result *out);
/* cogaps_run for DEVICE pointers: `data` -- and `uncertainty`, unless NULL -- are row-major [nrow][ncol] fp32 arrays in the memory of
 * params->device (-1: the calling thread's current device).  cogaps_session_create with data_on_device = 1 + phases + finish: see there
 * for the contract.  Every field of the result is what cogaps_run gives for host copies of the same arrays. */
int cogaps_run_device(const float *data, uint32_t nrow, uint32_t ncol, const cogaps_params *params,
                      const float *uncertainty, cogaps_result *out);
/* gaps::run for a matrix file (src/GapsRunner.h:24-29; Rcpp cogaps_from_file_cpp, src/Cogaps.cpp:217-227): .mtx, .csv, .tsv
 * or .gct, read as the reference's parsers read them (src/file_parser/, incl. the text -> fp32 rule of
 * MatrixElement.cpp:10-47); uncertaintyPath NULL or "" for the default uncertainty. */
int cogaps_run_from_file(const char *dataPath, const cogaps_params *params, const char *uncertaintyPath, cogaps_result *out);
/* the file as a dense row-major fp32 matrix (callee-allocated; release with cogaps_matrix_free).  Host only: no GPU needed. */
int cogaps_read_matrix_file(const char *path, uint32_t *nrow, uint32_t *ncol, float **data);
/* ... of a SUBSET of the file: the rows (byRows != 0) or columns named by the 1-based `indices`, read the way the reference's workers
 * read their subset of a file (Matrix(path, genesInCols, subsetGenes, indices), src/data_structures/Matrix.cpp:70-134: the indices
 * are sorted first, a duplicated index fills its first position only); the rest of the matrix is never materialised.
 * cogaps_run_from_file does the same when params->subsetData is set. */
int cogaps_read_matrix_file_subset(const char *path, int byRows, const uint32_t *indices, uint32_t nIndices,
                                   uint32_t *nrow, uint32_t *ncol, float **data);
void cogaps_matrix_free(float *data);
/* the .mtx file as triplets in file order (0-based), values by the reader's text -> fp32 rule; with indices != NULL only the entries of
 * the named rows (byRows) / columns, renumbered as cogaps_read_matrix_file_subset places them; *nrow, *ncol: of the (subset) matrix.
 * A position may repeat: D = 0, then D[rows[k]][cols[k]] = values[k] for k = 0, 1, ... is the matrix cogaps_read_matrix_file[_subset]
 * returns, byte for byte -- the meaning cogaps_coo_matrix gives the same arrays.  Same messages as the dense reader.  Host only: no GPU
 * needed.  The three arrays are callee-allocated; release them with cogaps_triplets_free. */
int cogaps_read_mtx_triplets(const char *path, int byRows, const uint32_t *indices, uint32_t nIndices,
                             uint32_t *nrow, uint32_t *ncol, uint64_t *nnz, uint32_t **rows, uint32_t **cols, float **values);
void cogaps_triplets_free(uint32_t *rows, uint32_t *cols, float *values);
/* getFileInfo_cpp (src/Cogaps.cpp:229-246): dimensions and the row / column names the file carries, '\n'-joined into the
 * caller's buffers (NULL / 0 to skip; *needed = bytes of a complete copy incl. the terminator).  Host only. */
int cogaps_file_info(const char *path, uint32_t *nrow, uint32_t *ncol, char *rowNames, size_t rowCap, size_t *rowNeeded,
                     char *colNames, size_t colCap, size_t *colNeeded);
void cogaps_result_free(cogaps_result *r);
const char *cogaps_last_error(void);
/* What kind of failure the calling thread's last failing call was -- so that a caller can react to device memory running out (fewer
 * sessions in flight) without reading message texts.  The reference has one failure path (GAPS_ERROR, utils/GapsAssert.h:19-25). */
enum { COGAPS_OK = 0, COGAPS_ERR_GENERIC = 1, COGAPS_ERR_OUT_OF_DEVICE_MEMORY = 2, COGAPS_ERR_OUT_OF_HOST_MEMORY = 3 };
int cogaps_last_error_code(void);

/* the HIP device ordinal that is current for the calling host thread (what cogaps_params.device = -1 resolves to) */
int cogaps_current_device(int *device);
/* free and total bytes of HBM on `device` (-1: the calling thread's current one); what a caller that keeps several sessions per GPU
 * sizes its batches by (cogaps_amd/distributed.py) */
int cogaps_device_memory(int device, uint64_t *freeBytes, uint64_t *totalBytes);

/* the three trivial exports next to cogaps_cpp (src/Cogaps.cpp:217-246) */
const char *cogaps_build_report(void);
/* sha256 (first 16 hex digits) over the sources the library was built from, "unknown" for a build outside csrc/Makefile.  bench.py compares it
 * with the hash recorded beside a committed counter measurement (profiles/r*_pmc_traffic.json) and marks the measurement stale when they differ. */
const char *cogaps_source_hash(void);
int cogaps_checkpoints_enabled(void);
int cogaps_compiled_with_openmp(void);

/* ------------------------------------------------------------------------------------------------
 * Session interface: the same run, one step at a time.  Used by bench.py (inputs resident in HBM
 * before the timed region; `data_on_device` accepts a device pointer) and by the parity tests
 * (per-batch proposal traces).  cogaps_run is cogaps_session_create + phases + finish.
 * ---------------------------------------------------------------------------------------------- */
typedef struct cogaps_session cogaps_session;

typedef struct cogaps_trace_rec {   /* one queued proposal, ProposalQueue.h:15-28 */
    uint64_t pos, rng_state;
    uint32_t atom1, atom2;          /* indices in the unsorted atom vector, 0xFFFFFFFF = none */
    uint32_t r1, c1, r2, c2;
    uint32_t type;                  /* 'B','D','M','E' */
    uint32_t batch;
} cogaps_trace_rec;

/* With useSparseOptimization = 1 the session holds the sparse model's packed data only -- per sampler the flag words, prefix counts,
 * pointers and values of the entries > 0, built on the device (csrc/sparse_build.h) -- and no nrow x ncol array, whichever of the
 * three entries created it: this one compacts the dense matrix to CSR on the host (applying subsetData; `uncertainty` is ignored,
 * the model knows the default only) and goes through the builder of cogaps_session_create_sparse.  A dense matrix with 2^32 - 1
 * or more entries > 0 is refused with that builder's message.
 *
 * data_on_device = 1: `data` AND `uncertainty` (unless NULL) are device pointers of params->device, row-major [nrow][ncol] fp32, and
 * are consumed where they lie (csrc/dense_build.h): nothing of size nrow x ncol is allocated on the host or copied to it.  The dense
 * model's D, Sraw and S2 of both samplers are written by one kernel pass per sampler (a copy or gather for the sampler whose vectors
 * are input rows, a transpose through LDS tiles for the other; subsetData's indices gather on either axis), lambda's sum by an ordered
 * one-accumulator pass on the device; the sparse model's CSR matrix is compacted on the device (count, scan, fill) and handed to the
 * builder of cogaps_session_create_sparse.  THE SESSION IS, BIT FOR BIT, THE SESSION THE SAME CALL MAKES WITH data_on_device = 0 FROM
 * HOST COPIES OF THE ARRAYS: data arrays with their pads, lambda, maxGibbsMass, dataSparsity, the seeder's state, every proposal, and
 * cogaps_session_device_bytes (the build's temporaries -- the subset's indices, for the sparse model the CSR arrays -- are released
 * before the call returns and never counted).  Completion contract: the caller's arrays must be complete before the call (work queued
 * on the caller's own streams is not waited for); the library reads them on its own stream, synchronises that stream before it
 * returns, and does not reference them afterwards.  Errors and their texts are those of the host-pointer call. */
cogaps_session *cogaps_session_create(const float *data, uint32_t nrow, uint32_t ncol,
                                      const cogaps_params *params, const float *uncertainty,
                                      int data_on_device);
void cogaps_session_destroy(cogaps_session *s);

/* A matrix in compressed-sparse form -- CSR (majorIsRow = 1) or CSC (0) -- as the input of the sparse model (useSparseOptimization = 1,
 * the reference's SparseNormalModel).  A scipy.sparse csr_matrix / csc_matrix maps onto it directly, and so does R's dgCMatrix with
 * majorIsRow = 0: @p -> indptr (widened to 64 bits), @i -> indices, @x -> values (as fp32), @Dim -> nrow, ncol.
 *
 * A session created from it is the session cogaps_session_create makes from the dense form of the same matrix, bit for bit: the flag
 * words, prefix counts, pointers and packed values of both samplers and lambda / maxGibbsMass are built on the device
 * (csrc/sparse_build.h) and no nrow x ncol array is allocated on the host or on the device.  With host pointers the three arrays are
 * uploaded once; with onDevice = 1 nothing is copied to the host but indptr[nMajor].  The caller's arrays are not referenced after the
 * call returns.  Stored entries that are not > 0 (zeros, negatives, NaN) are dropped, as the sparse model drops them from a dense matrix.
 * Errors (NULL / 1, cogaps_last_error): useSparseOptimization = 0; subsetData (pass the subset's rows / columns instead); reductionMode
 * COGAPS_REDUCE_SEQ (the verification mode takes dense input); indptr that does not start at 0, decreases or does
 * not end at the number of stored entries; an index >= the minor dimension; indices not strictly ascending inside a row / column
 * (duplicates included); 2^32 - 1 stored entries or more.  The input is validated on the device before anything is built from it.
 * transposeData, whichMatrixFixed / fixedPatterns and everything else in cogaps_params work as for the dense entry points; such a session
 * is an ordinary session (batches, traces, copy-outs, snapshots, PUMP). */
typedef struct cogaps_sparse_matrix {
    uint32_t nrow, ncol;        /* of the data as the caller sees it (genes x samples unless transposeData) */
    int32_t  majorIsRow;        /* 1 = CSR, 0 = CSC */
    const uint64_t *indptr;     /* [nMajor + 1] */
    const uint32_t *indices;    /* [nnz] minor indices, strictly ascending inside each major slice */
    const float    *values;     /* [nnz] */
    int32_t  onDevice;          /* 0: host pointers, 1: device pointers of params->device */
} cogaps_sparse_matrix;
cogaps_session *cogaps_session_create_sparse(const cogaps_sparse_matrix *m, const cogaps_params *params);
/* cogaps_run for such a matrix (host or device pointers) */
int cogaps_run_sparse(const cogaps_sparse_matrix *m, const cogaps_params *params, cogaps_result *out);

/* A matrix as unordered triplets (COO) -- what a Matrix Market file holds, or R's dgTMatrix (@i -> rows, @j -> cols, @x -> values as
 * fp32, @Dim -> nrow, ncol) -- as the input of the sparse model.  The triplets denote the matrix
 *
 *     D = zeros(nrow, ncol);  for k in 0 .. nnz-1, in that order:  D[rows[k], cols[k]] = values[k]
 *
 * THE ENTRY LATEST IN INPUT ORDER DECIDES A POSITION, also when its value is not > 0: the position is then absent whatever came before.
 * (This is what the .mtx reader does with a repeated position.  It is NOT what R's Matrix package or scipy mean by repeated triplets --
 * they sum them: a caller who wants sums canonicalises first.)  After that rule a value that is not > 0 (zero, negative, NaN) is absent,
 * as for the compressed entry.
 *
 * A session created from the triplets is the session cogaps_session_create makes from D, bit for bit (flag words, prefix counts,
 * pointers, packed values, lambda, maxGibbsMass, meanChiSq, every proposal), and holds the bytes of device memory the session created
 * from the CSR form of D holds.  No nrow x ncol array is allocated on the host or on the device: the build (csrc/sparse_build.h) resolves
 * repeated positions on the device by the entry index alone, so the result does not depend on how the device schedules the work; its
 * temporaries -- the uploaded arrays, one present bit per position in one sampler's flag layout with prefix counts, one 32-bit index per
 * present position, one bit per entry -- are released before the call returns.  The caller's arrays are not referenced afterwards.
 * Errors (NULL / 1, cogaps_last_error): useSparseOptimization = 0; subsetData; reductionMode COGAPS_REDUCE_SEQ; a NULL array with
 * nnz > 0; a row or column index outside the stated dimensions (checked on the device before anything is built); nnz >= 2^32 - 1.
 * Everything else as for cogaps_sparse_matrix: transposeData, whichMatrixFixed / fixedPatterns, batches, traces, copy-outs, snapshots,
 * PUMP.  cogaps_run_from_file takes this route for a .mtx path with useSparseOptimization = 1, the default reductionMode and no
 * uncertainty file (a subset is taken by the reader); its results are those of the dense read of the file. */
typedef struct cogaps_coo_matrix {
    uint32_t nrow, ncol;          /* of the data as the caller sees it (genes x samples unless transposeData) */
    uint64_t nnz;
    const uint32_t *rows, *cols;  /* [nnz], 0-based, any order, repeats allowed: the latest entry of a position decides */
    const float    *values;       /* [nnz] */
    int32_t  onDevice;            /* 0: host pointers, 1: device pointers of params->device */
} cogaps_coo_matrix;
cogaps_session *cogaps_session_create_coo(const cogaps_coo_matrix *m, const cogaps_params *params);
int cogaps_run_coo(const cogaps_coo_matrix *m, const cogaps_params *params, cogaps_result *out);
/* A matrix resident on one GPU: uploaded, validated and -- for triplets -- resolved for repeated positions ONCE, then the source of any
 * number of sparse-model sessions (a K sweep, replicate seeds, both passes of every shard of a distributed run), each with its own
 * nPatterns, seed, fixed matrix, transposeData and subsetData.  `device` = -1: the calling thread's current device.
 *
 * The handle holds device copies of the input arrays (with onDevice = 1: a device-to-device copy) -- for triplets also one keep bit per
 * entry (the latest entry > 0 of its position) -- and nothing else; the caller's arrays are not referenced after the call, which
 * synchronises before it returns.  The handle never changes afterwards: sessions may be created from it by several host threads at once.
 * A session copies nothing from it but what its own packed structures hold, so the handle may be destroyed while sessions made from it
 * live on.  Its bytes are reported by cogaps_device_matrix_info and never appear in a session's cogaps_session_device_bytes.
 * Errors of the creating calls (NULL, cogaps_last_error) are those of cogaps_session_create_sparse / _coo for the same arrays, with the
 * same texts, checked on the device over the whole input before anything is kept: indptr that does not start at 0, decreases or does not
 * end at the number of stored entries; an index >= the minor dimension; indices not strictly ascending; a triplet index outside the
 * dimensions; 2^32 - 1 entries or more; NULL arrays.
 *
 * cogaps_session_create_from_device_matrix: THE SESSION IS, BIT FOR BIT, THE SESSION cogaps_session_create MAKES FROM THE DENSE FORM OF
 * THE HANDLE'S MATRIX WITH THE SAME cogaps_params (flag words, prefix counts, pointers, packed values, lambda, maxGibbsMass, meanChiSq,
 * every proposal, cogaps_session_device_bytes) -- without subsetData therefore also the session cogaps_session_create_sparse / _coo makes.
 * Everything in cogaps_params is honoured, unlike those two entries including
 *   - subsetData / subsetGenes (with transposeData) by the dense entry's rule (Matrix.cpp:30-69): the 1-based dataIndicesSubset name rows
 *     or columns of the genes / samples axis IN THE ORDER GIVEN; output row / column i is input dataIndicesSubset[i] - 1; AN INDEX MAY
 *     REPEAT, and the row / column then appears that often.  The subset is taken on the device (csrc/sparse_build.h, the map): the build
 *     reads the whole handle once, O(stored entries), uploads nothing but the indices, and allocates nothing of the size of the whole
 *     matrix -- its temporaries are O(dimension of the subset axis + nSubset);
 *   - reductionMode COGAPS_REDUCE_SEQ with any mathMode (the verification mode).
 * Errors (NULL, cogaps_last_error): useSparseOptimization = 0 (the dense model takes a dense matrix); params->device other than -1 or the
 * handle's device; an index of dataIndicesSubset outside 1 .. dimension or an empty subset (the dense entry's messages); a subset whose
 * repeated indices bring it to 2^32 - 1 kept entries or more. */
typedef struct cogaps_device_matrix cogaps_device_matrix;
cogaps_device_matrix *cogaps_device_matrix_create_sparse(const cogaps_sparse_matrix *m, int device);   /* CSR / CSC, host or device pointers */
cogaps_device_matrix *cogaps_device_matrix_create_coo(const cogaps_coo_matrix *m, int device);         /* triplets, the latest entry decides */
void cogaps_device_matrix_destroy(cogaps_device_matrix *m);
/* dimensions, stored entries (triplets: all of them, overwritten ones included), bytes of device memory held, device; any pointer may be NULL */
int  cogaps_device_matrix_info(const cogaps_device_matrix *m, uint32_t *nrow, uint32_t *ncol, uint64_t *storedEntries,
                               uint64_t *deviceBytes, int *device);
cogaps_session *cogaps_session_create_from_device_matrix(const cogaps_device_matrix *m, const cogaps_params *params);
int cogaps_run_device_matrix(const cogaps_device_matrix *m, const cogaps_params *params, cogaps_result *out);
/* Bytes of device memory the session holds: the sum of its own allocations (as requested), counted as they are made and released -- not
 * hipMemGetInfo, which is device-wide.  For every session, however it was created. */
int cogaps_session_device_bytes(cogaps_session *s, uint64_t *bytes);
/* HIP-event time of the two ordered fp32 sums over the packed values at the creation of a sparse-model session, whatever its input
 * (the one serial pass of the build), or of the two ordered sums over D of a dense-model session built from device pointers; 0 for a
 * dense-model session built from host pointers (its sums run on the host) */
int cogaps_session_sparse_build_ms(cogaps_session *s, float *orderedSumMs);
/* test hook: the sparse model's data structures of sampler `which` -- flags / prefix [M][Wn], ptr [M + 1], vals [nVals] -- and the
 * constants derived from the data; NULL skips an output (sizes first, then the arrays) */
int cogaps_session_debug_sparse_data(cogaps_session *s, char which, uint32_t *Wn, uint32_t *nVals, float *lambda, float *maxGibbsMass,
                                     uint64_t *flags, uint32_t *prefix, uint32_t *ptr, float *vals);
/* test hook, the dense model's counterpart: the raw [M][Npad] arrays of sampler `which` as the device holds them, pads included -- D,
 * Sraw (the un-squared uncertainty) and S2 -- and the constants derived from the data (lambda, maxGibbsMass, DenseNormalModel's
 * dataSparsity).  NULL skips an output.  *hasS2 = 0 and S2 left untouched when the session keeps no S2 array (the default uncertainty:
 * the evaluation recomputes it from D); M, N from cogaps_session_dims, Npad = (N + 3) & ~3. */
int cogaps_session_debug_dense_data(cogaps_session *s, char which, float *D, float *Sraw, float *S2, float *lambda, float *maxGibbsMass,
                                    float *sparsity, int *hasS2);
/* annealing temperature of both samplers (runOnePhase sets min(1, 2*iter/nIter) while equilibrating) */
int cogaps_session_set_annealing(cogaps_session *s, float temp);
/* nA, nP ~ Poisson(max(nAtoms,10)) from the runner's generator (GapsRunner.cpp:294-295) */
int cogaps_session_draw_steps(cogaps_session *s, uint32_t *nA, uint32_t *nP);
/* AsynchronousGibbsSampler::update for sampler `which` ('A' or 'P'); optional proposal trace */
int cogaps_session_update(cogaps_session *s, char which, uint32_t nSteps,
                          cogaps_trace_rec *trace, uint32_t traceCap, uint32_t *nTrace,
                          uint32_t *batchNproc, uint32_t *batchQlen, uint32_t batchCap, uint32_t *nBatches);
/* DenseNormalModel::sync for sampler `which` (copies the transposed AP of the other sampler) */
int cogaps_session_sync(cogaps_session *s, char which);
/* one iteration of runOnePhase: updateSampler(nA, nP) (+ statistics when sampling != 0) */
int cogaps_session_iterate(cogaps_session *s, uint32_t nA, uint32_t nP, int sampling);
/* `n` complete iterations of a phase starting at iteration `firstIter` (anneal, draw, update, stats,
 * history); phase 1 = equilibration, 2 = sampling.  Adds to *updates the proposals processed. */
int cogaps_session_run_iterations(cogaps_session *s, int phase, uint32_t firstIter, uint32_t n, uint64_t *updates);
int cogaps_session_natoms(cogaps_session *s, char which, uint32_t *n);
int cogaps_session_chisq(cogaps_session *s, char which, float *chisq);
/* copy-outs (host buffers): matrix row-major [M][K]; AP [M][N]; atoms in vector order */
int cogaps_session_get_matrix(cogaps_session *s, char which, float *out);
int cogaps_session_get_rows(cogaps_session *s, char which, float *out);   /* sparse model: the HybridMatrix row copy, row-major [rows][nPatterns]; dense model: = get_matrix */
int cogaps_session_get_ap(cogaps_session *s, char which, float *out);
int cogaps_session_get_atoms(cogaps_session *s, char which, uint64_t *pos, float *mass,
                             uint32_t *left, uint32_t *right);
int cogaps_session_dims(cogaps_session *s, char which, uint32_t *M, uint32_t *N, uint32_t *K);
int cogaps_session_avg_queue(cogaps_session *s, char which, float *avg);
int cogaps_session_finish(cogaps_session *s, cogaps_result *out);
/* ------------------------------------------------------------------------------------------------
 * State file: stop a run and go on later -- in another process, another GPU allocation -- with THE SAME CHAIN, BIT FOR BIT.  This is the
 * library's own file, not the reference's Archive checkpoint: cogaps_checkpoints_enabled() stays 0 and checkpointInFile stays refused.
 *
 * Position: the session records where it stands -- phase 1 (equilibration) or 2 (sampling) and the next iteration of that phase; phase 3:
 * both phases complete.  cogaps_session_run_iterations and cogaps_batch_run_iterations advance it; a caller that steps with
 * cogaps_session_iterate / _update keeps its own book, and the position stays where the last run_iterations left it.
 *
 * save_state writes what changes while a chain runs -- per sampler the factor matrix (the sparse model's row copy, flags and lookup
 * tables), the atomic domain and the generator's scalars, ONE sampler's A*P cache (the other's is its transpose); per session the host
 * generators with the seeder's look-ahead, statistics accumulators, PUMP, snapshots, histories, counters, times, the position -- and
 * nothing of the data, the lookup tables or a capacity: a sparse-model file holds no array of size genes x samples, a dense-model file
 * one.  It is taken BETWEEN TWO ITERATIONS (after run_iterations / iterate; between two cogaps_batch_run_iterations calls for a batch
 * member), where the queue and the erase cache are empty and the two A*P caches agree.  The file is little-endian: magic, format
 * version, section table, payload, a 64-bit checksum; it is written to path + ".tmp", flushed and renamed, so a save that fails leaves
 * the previous file intact.  Device arrays pass through one 4 MiB pinned buffer.
 *
 * load_state: create a session the ordinary way -- any creation entry, the caller's data and parameters -- then load.  The file is
 * validated completely before anything is overwritten: magic, version, length, checksum, the fingerprint, every section's size.  The
 * fingerprint names what file and session must share: model, nGenes, nSamples, nPatterns, seed, nIterations, alphaA/P, maxGibbsMassA/P,
 * outputFrequency, snapshotFrequency / snapshotPhase, takePumpSamples, pumpThreshold, whichMatrixFixed and a hash of fixedPatterns,
 * reductionMode / mathMode, the data-derived lambda, maxGibbsMass, dataSparsity / number of packed values, and a 64-bit digest of the
 * data computed on the device (csrc/state_digest.h) at the session's first save or load.  A refused load names the first differing item
 * and leaves the session untouched.  The loading session's capacity (grown if the file's atoms need it), launch form (chained or two
 * launches, graphs, generator window) and later membership of a batch are its own: none is state.  A session that already belongs to a
 * batch refuses to load (load first, then create the batch); a session ended by a device error refuses both calls.  Both synchronise the
 * session's stream (a batch member's is the batch's).  After a load, samplerSeconds continues from the saved value and
 * totalRunningTime is the saved elapsed time plus the time since the load; every other result field is the uninterrupted run's.
 *
 * run_to_end: everything that remains of the two phases from the session's position, then cogaps_session_finish.  With statePath != NULL
 * the state is saved after every `interval` iterations (0: not on the way), once more when both phases are complete (position 3), and
 * -- the interrupt hook is polled at the head of an iteration, before anything of it is drawn -- before the call fails with
 * "interrupted": a later load continues at exactly that iteration.
 * ---------------------------------------------------------------------------------------------- */
int cogaps_session_position(cogaps_session *s, int *phase, uint32_t *nextIter);
int cogaps_session_save_state(cogaps_session *s, const char *path);
int cogaps_session_load_state(cogaps_session *s, const char *path);
int cogaps_session_run_to_end(cogaps_session *s, const char *statePath, uint32_t interval, cogaps_result *out);
/* test hook: the fingerprint's data digest, computed anew by every call (the same for every input form of a matrix) */
int cogaps_session_debug_data_digest(cogaps_session *s, uint64_t *digest);
/* counters for the roofline report: algorithmic bytes moved by the evaluation kernel so far, number
 * of evaluation launches, batches generated, and the accumulated HIP-event time of each kernel */
typedef struct cogaps_perf {
    uint64_t evalBytes;       /* sum over evaluated proposals of 16N/20N/32N + 12N per AP update */
    uint64_t evalLaunches, genLaunches, batches, proposalsQueued;
    double evalMs, genMs, syncMs;   /* HIP-event time (dispatch begin to end) of the launches that processed a batch since timing was switched on
                                       (a sample of them carries events; scaled to `timedBatches`) */
    double evalNoopMs, genNoopMs;   /* summed HIP-event time of sampled launches past the end of an update (empty queue) */
    uint64_t evalNoopTimed, genNoopTimed; /* ... and how many were sampled */
    uint64_t timedBatches;    /* batches processed since cogaps_session_set_timing(1): what evalMs / genMs are scaled to */
    uint64_t evalTimed, genTimed;   /* launches that carried events and processed a batch */
    uint64_t syncTimed, syncBytes;  /* sync launches timed since then (all of them; their summed time is syncMs) and their algorithmic bytes (8 M N each) */
} cogaps_perf;
int cogaps_session_set_timing(cogaps_session *s, int on);
int cogaps_session_perf(cogaps_session *s, cogaps_perf *out);                      /* both samplers */
int cogaps_session_perf_sampler(cogaps_session *s, char which, cogaps_perf *out);   /* the 'A' or the 'P' sampler alone */
/* 1 when the sampler's last update ran as chained launches (csrc/chain_kernel.h: ONE launch evaluates batch n and generates batch n + 1;
 * its time is reported as evalMs, genMs stays 0), 0 for a generator launch and an evaluation launch per batch.  The chained form serves
 * the one-chain fused evaluation (AsynchronousGibbsSampler.h:88-122, same results); environment COGAPS_NO_CHAIN=1 switches it off.  It is taken
 * only where the device shows a compute unit per workgroup of the launch (241; hipDeviceAttributeMultiprocessorCount, which honours
 * HSA_CU_MASK): the evaluation workgroups never wait for anything, so with fewer units the launch is still correct -- the workgroups run in
 * turns beside the generator's -- but slower than two launches; COGAPS_FORCE_CHAIN=1 (tests) takes it there anyway.  The hand-over inside the
 * launch assumes nothing about the order in which the dispatcher starts workgroups: only the generator workgroup waits, and only for
 * evaluation workgroups, which never wait, so every workgroup ends; the wait is bounded all the same (two seconds at least, for a workgroup
 * the GPU does not schedule at all) -- never a hang.  A wait that runs out applies nothing
 * of the decision it waited for and makes the launches already enqueued behind it no-ops; the host then completes the batch from the
 * decisions the evaluation workgroups have left by then (chain_recover_kernel), and the sampler goes on -- same chain, same bits -- with
 * two launches per batch for the rest of the session.  cogaps_session_chain_recoveries counts such events (0 in every run so far).  Only if
 * a decision is still missing then (the split evaluation's chained form, COGAPS_CHAIN_SPLIT: its deciding workgroups wait as well) does the
 * update end with an error (GAPS_ERR_SPIN) and the session refuse further steps.  All of this -- the completed batch, "same chain, same
 * bits" -- holds for ONE-CHAIN sessions only.  A batch (cogaps_batch_*, whose chained launch is chain_kernel_multi) has no recovery: there
 * the same event ENDS the chain it happens in.  cogaps_batch_run_iterations fails with "device error code 4 in sampler X of chain C"
 * (4 = GAPS_ERR_SPIN), that chain's session is poisoned -- it refuses further updates, on its own too, and holds no result -- and the batch
 * refuses every later call.  The other chains' sessions are not poisoned and take calls of their own once the batch is destroyed, but
 * the failing call left them wherever their own update stood: they are no longer the chains an undisturbed run gives. */
int cogaps_session_chained(cogaps_session *s, char which, int *chained);
int cogaps_session_chain_recoveries(cogaps_session *s, char which, uint32_t *n);
/* Attempts per round of the sampler's generator launches as of its last update (the library's instantiations: 128, 256, and 448 for the sparse
 * model's chained launch once batches are long; no result depends on it). */
int cogaps_session_generator_window(cogaps_session *s, char which, uint32_t *attempts);
/* Durations of the sampler's chained launches since cogaps_session_set_timing(1), EVERY launch -- replayed graphs included, where HIP
 * events cannot ride --, from the chip-wide 100 MHz clock read inside the launch (entry of its first workgroup to the end of its generator
 * workgroup, the last to finish: what rocprofv3 --kernel-trace reports as the dispatch's duration, minus the dispatcher's fill / drain).
 * meanUs; percentilesUs[5] = 10th, 50th, 75th, 90th, 99th (0.1 us bins); launches = how many were measured (0: the sampler does not chain). */
int cogaps_session_launch_clock(cogaps_session *s, char which, double *meanUs, double *percentilesUs, uint64_t *launches);
/* The same launches by their PERIOD: entry of a launch's first workgroup to the entry of the next launch's -- the launch with the dispatcher's
 * start-up and the end-of-kernel write-back around it (what rocprofv3 reports as the dispatch's duration, plus the idle gap to the next
 * dispatch); seams where the host read progress back (> 100 us) are left out.  The sum of the periods cannot exceed the wall time. */
int cogaps_session_launch_period(cogaps_session *s, char which, double *meanUs, double *percentilesUs, uint64_t *launches);

/* ------------------------------------------------------------------------------------------------
 * Batched multi-chain launches: the sessions of a batch -- the subsets of a GWCoGAPS / scCoGAPS job that share one GPU
 * (R/DistributedCogaps.R:60-68 hands them to BiocParallel workers), or replicas -- are stepped in lock-step by one stream: one
 * generator launch with a workgroup per chain, one evaluation launch over all chains' queues.  Every chain produces exactly the
 * bits it produces on its own.  The sessions must share the model (dense / sparse), whichMatrixFixed, the device and the
 * evaluation launch shape (equal cogaps_reduction_width of their vector lengths); create them first, then the batch; drive the
 * batch with cogaps_batch_run_iterations (phase 1, then phase 2), then cogaps_session_finish each session; destroy the batch
 * before the sessions.  While a session belongs to a batch only the batch may step it.
 * ---------------------------------------------------------------------------------------------- */
typedef struct cogaps_batch cogaps_batch;
cogaps_batch *cogaps_batch_create(cogaps_session **sessions, uint32_t n);
void cogaps_batch_destroy(cogaps_batch *b);
/* iterations [firstIter, firstIter + n) of `phase` for every chain; updates (may be NULL): [n chains], += proposals per chain */
int cogaps_batch_run_iterations(cogaps_batch *b, int phase, uint32_t firstIter, uint32_t n, uint64_t *updates);
int cogaps_batch_set_timing(cogaps_batch *b, int on);
/* mean HIP-event time (us) of the sampled generator / evaluation launches of sampler side 0 (A) or 1 (P) since set_timing(1) */
int cogaps_batch_perf(cogaps_batch *b, int side, double *genUs, double *evalUs, uint64_t *sampled, uint64_t *launches);

/* development aid: per-phase cycle counters of the generator kernel (all zero unless built with -DGEN_PROFILE) */
int cogaps_session_debug_prof(cogaps_session *s, char which, uint64_t *out16);
int cogaps_session_debug_replay(cogaps_session *s, char which, int kind, uint32_t n, uint32_t dbgFlags, double *usPerLaunch);
/* test hook: counts broken invariants of the atomic domain's redundant state (links, index vector, cached neighbour positions / masses) */
int cogaps_session_debug_check_domain(cogaps_session *s, char which, uint32_t *violations);

/* test hook for the math modes: y[i] = fn(x[i]) with fn 0 = logf, 1 = expf in math mode `mathMode`, evaluated by a kernel on
 * the current device (on_device != 0) or by the same source compiled for the host */
int cogaps_debug_math(int fn, int mathMode, const float *x, float *y, uint32_t n, int on_device);
/* test hooks for the 64-bit integer draws (csrc/gaps_math.h), evaluated like cogaps_debug_math: q[i] = gm_udiv64(a[i], b[i]) (every
 * b[i] >= 1), and value[i] = pcg_uniform64(s, lo[i], hi[i]) from the generator state s = state[i], with stateAfter[i] = s after the
 * draw.  A range lo .. hi needs hi >= lo and fewer than 2^64 values: hi + 1 - lo wraps to 0 for the whole 64-bit range, by which the
 * reference's GapsRng::uniform64 divides (Random.cpp:112-114) -- no caller asks for it, and the hook refuses it. */
int cogaps_debug_udiv64(const uint64_t *a, const uint64_t *b, uint64_t *q, uint32_t n, int on_device);
int cogaps_debug_uniform64(const uint64_t *state, const uint64_t *lo, const uint64_t *hi, uint64_t *value, uint64_t *stateAfter, uint32_t n, int on_device);

/* ------------------------------------------------------------------------------------------------
 * Result statistics: the gene-set permutation test of the reference's calcCoGAPSStat (R/methods-CogapsResult.R:499-531).
 *
 * z: the Z-score matrix (calcZ: mean / standard deviation of a factor matrix), nRows x nCols doubles in host memory, element (i, k)
 * at z[i * rowStride + k * colStride] -- rowStride = nCols, colStride = 1 for a row-major matrix, rowStride = 1, colStride = nRows
 * for R's column-major one.  It is uploaded (and repacked) per call.  Set t has the member rows members[memberOffsets[t] ..
 * memberOffsets[t + 1]), 0-based and ascending, and the draw size drawSizes[t] (the reference draws length(thisSet) rows, whether or
 * not every name matched a row).  For every set and column k:
 *   actualMean[t][k]    = the fp64 sum of z over the members, in ascending row order, divided once by their number
 *   lessThanCount[t][k] = the number of permutations p < numPerm with actualMean[t][k] < the mean of z over the drawSizes[t]
 *                         distinct rows of draw (seed, t, p), summed in the order of the draw and divided once
 * The draw is the keyed permutation DESIGN.md 4.8 writes down (not R's sample() stream); a count does not depend on the device or
 * on how the work was divided.  A set without members has NaN means and counts of 0.  device: -1 for the calling thread's current
 * one (it is restored before the call returns).  Refused, with a message: null arguments (actualMean may be NULL), nSets == 0,
 * numPerm == 0, an empty matrix, a draw size of 0 or above nRows, a member that is no row or not above its predecessor,
 * memberOffsets that decrease.
 * ---------------------------------------------------------------------------------------------- */
int cogaps_gene_set_stat(const double *z, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride,
                         uint32_t nSets, const uint64_t *memberOffsets, const uint32_t *members, const uint32_t *drawSizes,
                         uint32_t numPerm, uint32_t seed, int device, uint32_t *lessThanCount, double *actualMean);
/* test hook: out[j], j < size: the rows of draw (seed, set, perm) from nRows rows, computed on the device by the statistic's own code */
int cogaps_debug_permutation_draw(uint32_t nRows, uint32_t size, uint32_t seed, uint32_t set, uint32_t perm, int device, uint32_t *out);

/* ------------------------------------------------------------------------------------------------
 * Result statistics: which genes of a set behave like the set -- the arithmetic of the reference's calcGeneGSStat and
 * computeGeneGSProb (R/methods-CogapsResult.R:535-594).
 *
 * z: the Z-score matrix, addressed through its strides as cogaps_gene_set_stat addresses it (R's column-major matrix passes as it is);
 * it is uploaded (and repacked) per call.  Set t has the member rows members[memberOffsets[t] .. memberOffsets[t + 1]), 0-based and
 * ascending, and the pattern weights wMember[t][k] and wNull[t][k], k < nCols, row-major doubles (wNull NULL: wNull = wMember).  The
 * weights are the caller's: the front end makes them from cogaps_gene_set_stat's counts with the host's logarithm.  Under the weights
 * w of a set, the statistic of row i is, every sum in fp64 over ascending k from +0, the product rounded before it is added,
 *   W = sum w[k],  R = sum z[i][k],  S = sum z[i][k] * w[k],  T = (S / W) / R,  but T = 0 where W < 1e-6 or R < 1e-6
 * (a negative sum is below 1e-6, a NaN sum never is).  Outputs, each of which may be NULL but not all three:
 *   memberStat[x]   = T under wMember of row members[x]                                  (laid out like members)
 *   greaterCount[x] = the number of rows i outside set t with T under wNull of row i > memberStat[x], the comparison strict and
 *                     false for a NaN on either side                                      (laid out like members)
 *   allStat[t][i]   = T under wNull of every row, members included                        ([nSets][nRows])
 * Nothing of size nSets x nRows is allocated, on the host or on the device, unless allStat is given.  No output depends on the device,
 * on the grid, on scheduling or on how many sets a call holds.  device: -1 for the calling thread's current one (it is restored
 * before the call returns).  Refused, with a message: z, memberOffsets, members or wMember NULL, all three outputs NULL, nSets == 0,
 * an empty matrix, a member that is no row or not above its predecessor, memberOffsets that decrease.
 * ---------------------------------------------------------------------------------------------- */
int cogaps_gene_set_membership(const double *z, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride,
                               uint32_t nSets, const uint64_t *memberOffsets, const uint32_t *members,
                               const double *wMember, const double *wNull, int device,
                               double *memberStat, uint32_t *greaterCount, double *allStat);

/* ------------------------------------------------------------------------------------------------
 * Result statistics: the pattern markers of the reference's patternMarkers (R/methods-CogapsResult.R:397-494).
 *
 * a: the matrix whose rows are ranked (featureLoadings for the reference's axis = 1, sampleFactors for axis = 2), nRows x nCols doubles
 * in host memory, element (i, k) at a[i * aRowStride + k * aColStride]; o: the other factor matrix, oRows x nCols, addressed the same
 * way through its own strides (rowStride = nCols, colStride = 1 for a row-major matrix; rowStride = 1, colStride = rows for R's
 * column-major one).  Both are uploaded per call.  lp: nLp pattern vectors of nCols entries each, row-major; NULL with nLp = 0 stands
 * for the nCols unit vectors.  With L = nLp, or nCols for the unit vectors:
 *   X[i][k]     = a[i][k] * max_j o[j][k], divided by the largest such product of row i
 *   score[i][l] = sqrt(sum over k, ascending, of (X[i][k] - lp[l][k])^2)            (fp64, no contraction)
 *   rank[i][l]  = 1 + the rows with a smaller score in column l + the rows before i with the same score; NaN scores (a row whose
 *                 largest product is 0) are above every number and equal to each other
 *   COGAPS_MARKERS_ALL: the markers of l are the rows whose smallest rank over the columns is first reached in column l, NaN rows
 *                 left out, by ascending rank in l
 *   COGAPS_MARKERS_CUT: the markers of l are the rows of column l by ascending rank, up to the first row that ranks better in another
 *                 column (all rows with a number for a score if there is none); a row may be a marker of several patterns
 * Outputs, each of which may be NULL: ranks [nRows][L] (1-based), scores [nRows][L], markers [L][nRows] (row l: its markerCount[l]
 * marker rows, 0-based, best rank first, then 0xFFFFFFFF), markerCount [L].  No output depends on the device, on the grid or on
 * scheduling.  device: -1 for the calling thread's current one (it is restored before the call returns).  Refused, with a message:
 * a or o NULL, a matrix without rows or columns, lp without nLp or nLp without lp, an lp entry above 1 or NaN, an unknown
 * threshold, more rows than 32-bit ranks hold.
 * ---------------------------------------------------------------------------------------------- */
#define COGAPS_MARKERS_ALL 0
#define COGAPS_MARKERS_CUT 1
int cogaps_pattern_markers(const double *a, uint64_t nRows, uint32_t nCols, size_t aRowStride, size_t aColStride,
                           const double *o, uint64_t oRows, size_t oRowStride, size_t oColStride,
                           const double *lp, uint32_t nLp, int threshold, int device,
                           uint32_t *ranks, double *scores, uint32_t *markers, uint32_t *markerCount);

/* ------------------------------------------------------------------------------------------------
 * Result statistics: the enrichment of gene sets in every pattern -- the "enrichment" method of the reference's getPatternGeneSet
 * (R/methods-CogapsResult.R:300-344), a pre-ranked gene-set enrichment analysis with scoreType = "pos" (DESIGN.md 4.11).
 *
 * stat: a factor matrix (featureLoadings or sampleFactors), nRows x nCols floats in host memory, element (i, k) at
 * stat[i * rowStride + k * colStride] -- rowStride = nCols, colStride = 1 for a row-major matrix, rowStride = 1, colStride = nRows
 * for R's column-major one.  It is uploaded once per call.  Column k ranks the rows by decreasing value, equal values in row order;
 * rankOut[k][i] (may be NULL) is the 0-based rank of row i.  Set t has the member rows members[memberOffsets[t] ..
 * memberOffsets[t + 1]), 0-based and ascending, m_t of them.  All outputs are laid out [nSets][nCols]; for set t and column k:
 *   es[t][k]      = max over the members in rank order, i = 0 .. m-1, of cum_i / cum_(m-1) - (rank_i - i) / (nRows - m), cum_i the
 *                   fp64 sum of the first i + 1 members' values in that order ((i + 1) / m where cum_(m-1) is 0)
 *   peak[t][k]    = the first i that attains it
 *   nGe[t][k]     = the number of permutations p < numPerm whose score is >= es[t][k], the score of permutation p being that of the
 *                   first m_t rows of draw (seed, t, p) -- cogaps_gene_set_stat's keyed draw; one subset serves every column
 *   permSum[t][k] = the sum over the permutations of floor(score * 2^40)
 * None of them depends on the device, on how the work was divided or on how many sets a call holds.  device: -1 for the calling
 * thread's current one (it is restored before the call returns).  Refused, with a message: null arguments (rankOut may be NULL),
 * nSets == 0, numPerm == 0, an empty matrix, a NaN or negative value in stat, a set without members, with nRows or more members or
 * with more than COGAPS_GSEA_MAX_SET of them, a member that is no row or not above its predecessor, memberOffsets that decrease.
 * ---------------------------------------------------------------------------------------------- */
#define COGAPS_GSEA_MAX_SET 4096
int cogaps_pattern_gsea(const float *stat, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride,
                        uint32_t nSets, const uint64_t *memberOffsets, const uint32_t *members,
                        uint32_t numPerm, uint32_t seed, int device,
                        double *es, uint32_t *peak, uint32_t *nGe, uint64_t *permSum, uint32_t *rankOut);

/* ------------------------------------------------------------------------------------------------
 * Result statistics: residuals -- the reference's reconstructGene and the matrix of its plotResiduals (R/methods-CogapsResult.R:233-286;
 * DESIGN.md 4.10) -- and the chi-square of every gene, of every sample and of the whole fit.
 *
 * a: featureLoadings, nGenes x nPatterns floats in host memory, element (i, k) at a[i * aRowStride + k * aColStride]; p: sampleFactors,
 * nSamples x nPatterns, through its own strides (rowStride = nPatterns, colStride = 1 for a row-major matrix; rowStride = 1, colStride
 * = rows for R's column-major one).  All arithmetic is fp64 on the exactly widened floats, D the data, S the uncertainty:
 *   M[i][j] = sum over k, ascending from +0.0, of A[i][k] * P[j][k], one fused multiply-add each (the product of two widened floats
 *             is exact in fp64, so a multiply followed by an add gives the same bits)
 *   s[i][j] = S[i][j], or max(0.1 * D[i][j], 0.1) in double without an uncertainty (R's pmax; not the sampler's fp32 fill)
 *   r[i][j] = (D[i][j] - M[i][j]) / s[i][j]                 q = r * r
 *   geneChiSq[i]   = the 64 sums t[L] = q[i][L] + q[i][L + 64] + ... (ascending j, from +0.0), folded by the ascending xor butterfly:
 *                    t[L] += t[L ^ 1], then ^ 2, ^ 4, ^ 8, ^ 16, ^ 32
 *   sampleChiSq[j] = the sums of q[i][j] over the genes of block b = i / 64 (ascending i, from +0.0), added in ascending b from +0.0
 *   chiSq          = geneChiSq[0] + geneChiSq[1] + ... from +0.0
 * No output depends on the device, on the grid or on scheduling; each can be recomputed bit for bit.
 *
 * data: what the fit is compared with, or NULL / kind COGAPS_RESIDUAL_DATA_NONE for M alone (the three chi-square outputs are then
 * left untouched).  transposeData: the data's rows are samples.  The data's dimensions must be those of a and p: a message names both
 * numbers otherwise.
 *   _DENSE          dense (and uncertainty, or NULL for the default): element (row, col) at [row * rowStride + col * colStride], both
 *                   through the same strides, nrow x ncol; onDevice = 1: device pointers of `device`, read where they lie
 *   _SPARSE / _COO  sparse / coo (host or device pointers, as their own onDevice says): the entries > 0, absent positions are 0, the
 *                   latest triplet of a position decides; validated as for a session
 *   _DEVICE_MATRIX  deviceMatrix: a handle's matrix, on the handle's device (device: -1 or that one)
 * The three sparse kinds take the default uncertainty only (a given one is refused).  They go through the sparse model's one builder
 * (csrc/sparse_build.h) for the gene side of its packed form -- flag words, prefix counts, pointers, packed values -- which the kernel
 * reads: without output rows such a call allocates nothing of the size nGenes x nSamples.
 *
 * rows: nRowsOut 0-based genes, any order, repeats allowed; matrixOut [nRowsOut][nSamples] doubles receives their rows of r (of M
 * without data).  NULL with 0: no rows.  geneChiSq [nGenes], sampleChiSq [nSamples], chiSq [1]: each may be NULL.  peakDeviceBytes
 * (may be NULL): the most device memory the call held at once beyond the caller's own device arrays and handle.  device: -1 for the
 * calling thread's current one (it is restored before the call returns).  Refused, with a message: a or p NULL, an empty matrix, rows
 * without matrixOut, a row that is no gene, neither data nor rows, an unknown kind, a NULL matrix of the stated kind, dimensions
 * that disagree, an uncertainty beside a sparse kind, a device other than the handle's, and what the sparse entries refuse.
 * ---------------------------------------------------------------------------------------------- */
#define COGAPS_RESIDUAL_DATA_NONE 0
#define COGAPS_RESIDUAL_DATA_DENSE 1
#define COGAPS_RESIDUAL_DATA_SPARSE 2
#define COGAPS_RESIDUAL_DATA_COO 3
#define COGAPS_RESIDUAL_DATA_DEVICE_MATRIX 4
typedef struct cogaps_residual_data {
    int32_t  kind;                        /* COGAPS_RESIDUAL_DATA_* */
    int32_t  transposeData;               /* 0: genes x samples, 1: samples x genes */
    uint32_t nrow, ncol;                  /* dense: of the data as the caller holds it */
    const float *dense, *uncertainty;     /* dense: the data; its uncertainty or NULL */
    size_t   rowStride, colStride;        /* dense: of both, in elements */
    int32_t  onDevice;                    /* dense: 0 host pointers, 1 device pointers */
    const cogaps_sparse_matrix *sparse;
    const cogaps_coo_matrix *coo;
    const cogaps_device_matrix *deviceMatrix;
} cogaps_residual_data;
int cogaps_residuals(const float *a, uint32_t nGenes, size_t aRowStride, size_t aColStride,
                     const float *p, uint32_t nSamples, size_t pRowStride, size_t pColStride, uint32_t nPatterns,
                     const cogaps_residual_data *data, const uint32_t *rows, uint32_t nRowsOut, int device,
                     double *geneChiSq, double *sampleChiSq, double *chiSq, double *matrixOut, uint64_t *peakDeviceBytes);

/* ------------------------------------------------------------------------------------------------
 * Consensus patterns: the step between the two passes of a distributed run -- the reference's findConsensusMatrix / patternMatch
 * (R/DistributedCogaps.R:129-217).
 *
 * patterns: the gathered patterns, one per column: nRows x nCols floats, element (k, j) at patterns[k * rowStride + j * colStride]
 * (rowStride = nCols, colStride = 1 for a row-major matrix; rowStride = 1, colStride = nRows for R's column-major one).  onDevice = 0:
 * host memory, uploaded once per call; onDevice = 1: a device pointer of `device`, read where it lies (complete before the call).
 * All arithmetic is fp64 on the exactly widened floats, every product rounded before it is added, and every sum over the rows follows
 * one rule: chunks of 4096 consecutive rows, a chunk's terms added in ascending row order from +0.0, the chunk sums in ascending chunk
 * order from +0.0.  With mean[j] = (sum of column j) / nRows and y[k][j] = x[k][j] - mean[j]:
 *   c[i][j]    = sum over k of y[k][i] * y[k][j]               dist[i][j] = 1 - c[i][j] / (sqrt(c[i][i]) * sqrt(c[j][j]))
 *   corcut(columns, k, minNS): complete linkage of the columns' sub-block of dist down to k clusters -- the smallest distance is
 *                merged, ties go to the pair whose lower index is smallest, then whose higher index is smallest; the merged cluster
 *                keeps the lower index and the maximum of the two distances to every other; clusters are numbered by first
 *                appearance, k >= the number of columns gives singletons -- of which those with minNS columns or more are kept
 *   patternMatch: corcut(all, cut, minNS); while a cluster has more than maxNS columns the first such is split by corcut(cluster, 2,
 *                minNS): its first part replaces it, a second part is appended, a cluster that leaves no part is dropped
 *   per cluster with the columns m_1 < ... < m_q:  meanPat[k] = (x[k][m_1] + ... + x[k][m_q]) / q;  cor_j = the correlation of column
 *                m_j with meanPat by the formulas above;  r_j = rint(1000 * cor_j) / 1000;  w_j = (r_j * r_j) * r_j;
 *                mp[k] = (x[k][m_1] * w_1 + ... + x[k][m_q] * w_q) / (w_1 + ... + w_q), both sums ascending from +0.0;
 *                consensus[k] = (float)(mp[k] / max over k of mp[k])
 * Outputs: nClusters [1]; cluster [nCols]: the 1-based cluster of every column in the order of the reference's clusteredPatterns, 0 for
 * a dropped one; corr [nCols] (may be NULL): r_j of every column, NaN for a dropped one; consensus: room for nRows x nCols floats, of
 * which the first nRows x nClusters are written, row-major [nRows][nClusters]; dist [nCols][nCols] and firstLabels [nCols] (the labels
 * of the first corcut before its minNS filter), both for tests, may be NULL.  No output depends on the device, on the grid or on
 * scheduling; each can be recomputed bit for bit.  device: -1 for the calling thread's current one (it is restored before the call
 * returns).  Refused, with a message: patterns, nClusters, cluster or consensus NULL, an empty matrix, nCols < 2, cut == 0, minNS == 0,
 * maxNS < minNS, nCols > COGAPS_PATTERN_MATCH_MAX_COLS (what the clustering workgroup keeps in LDS), a NaN or negative value in
 * patterns, a NaN in dist or among the r_j ("NA values in correlation of patterns": a constant column), no cluster with minNS columns.
 * ---------------------------------------------------------------------------------------------- */
#define COGAPS_PATTERN_MATCH_MAX_COLS 4096
int cogaps_pattern_match(const float *patterns, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride, int onDevice,
                         uint32_t cut, uint32_t minNS, uint32_t maxNS, int device,
                         uint32_t *nClusters, uint32_t *cluster, double *corr, float *consensus, double *dist, uint32_t *firstLabels);

/* ------------------------------------------------------------------------------------------------
 * Result statistics: the sums that the reference's MANOVA stands on (R/methods-CogapsResult.R:596-619) -- the column
 * means and the centred sums of squares and cross-products of a predictor matrix X (a result's patterns) and a response matrix Y (the
 * factor codes of the sample annotations).  With one numeric predictor per fit, manova(Y ~ x_k) follows from them for every k.
 *
 * x: nRows x nCols floats, element (i, k) at x[i * xRowStride + k * xColStride]; y: nRows x nResp doubles, element (i, j) at
 * y[i * yRowStride + j * yColStride] (strides in elements: R's column-major matrix and a row-major array both pass as they are).
 * Both are host pointers, uploaded per call (repacked row-major unless they lie so already).  All arithmetic is fp64 on the exactly
 * widened floats, in two passes, every product rounded before it is added, and every sum over the rows follows one rule: trips of 256
 * consecutive rows, a trip's terms added in ascending row order from +0.0, the trips' sums in ascending trip order from +0.0:
 *   xMean[k] = (sum of column k of x) / nRows          yMean[j] = (sum of column j of y) / nRows
 *   sxx[k]    = sum over i of dx * dx,    dx = x[i][k] - xMean[k]                        ([nCols])
 *   sxy[k][j] = sum over i of dx * dy_j,  dy_j = y[i][j] - yMean[j]                      ([nCols][nResp], row-major)
 *   syy[a][b] = sum over i of dy_a * dy_b                                                ([nResp][nResp], row-major; symmetric bit for bit)
 * Each output may be NULL, but not all five.  Nothing of size nRows x nCols is allocated on the device beyond the upload of x.  No
 * output depends on the device, on the grid, on scheduling or on how the columns are shared among waves; each can be recomputed bit for
 * bit.  device: -1 for the calling thread's current one (it is restored before the call returns).  Refused, with a message: x or y NULL,
 * all five outputs NULL, nResp outside 1 .. 8, nCols == 0, nRows < nResp + 2 (no residual degree of freedom), a stride of zero,
 * nCols * (1 + nResp) + nResp * nResp of 2^31 or more.  nCols has no other limit.
 * ---------------------------------------------------------------------------------------------- */
int cogaps_manova_sscp(const float *x, uint32_t nRows, uint32_t nCols, size_t xRowStride, size_t xColStride,
                       const double *y, uint32_t nResp, size_t yRowStride, size_t yColStride, int device,
                       double *xMean, double *yMean, double *sxx, double *sxy, double *syy);

/* ------------------------------------------------------------------------------------------------
 * New data projected onto a result's patterns: how strongly each pattern shows in each sample of a second data set -- the lmFit route of
 * projectR(data, loadings = cogapsResult), the companion package of the reference.  Every sample s of the data is
 * regressed on the loadings by least squares, D[:, s] ~ L c[:, s].
 *
 * loadings: L, nGenes x nPatterns floats in host memory, element (i, k) at loadings[i * lRowStride + k * lColStride].  data: D, a
 * descriptor as cogaps_residuals takes it (every kind but _NONE; no uncertainty: the fit is unweighted), genes x samples unless
 * transposeData.  dataRows: NULL -- the data has nGenes genes, matched by position -- or nGenes 0-based rows of the data: gene i of the
 * fit is data row dataRows[i], any order, repeats allowed (another gene set, or the same genes in another order, without a copy).
 * All arithmetic is fp64 on the exactly widened floats.  Every sum over the genes follows one rule: trips of COGAPS_PROJECT_TRIP
 * consecutive genes of the fit, a trip's terms added in ascending gene order from +0.0, the trips' sums in ascending trip order from +0.0:
 *   gram[a][b]  = sum over g of L[g][a] * L[g][b]            cross[k][s] = sum over g of L[g][k] * D[g][s]
 *                 (products of two widened floats: exact, so fused or not they give the same bits; a zero that a sparse kind never
 *                 stores adds +-0.0 to a sum that started at +0.0 and changes no bit: the sparse kinds give the dense kind's bits)
 *   gram = U diag(d) U^T, U unit lower triangular, column by column: w[m] = U[j][m] * d[m]; s = sum over m < j, ascending from +0.0, of
 *                 U[i][m] * w[m]; d[j] = gram[j][j] - s (i = j); U[i][j] = (gram[i][j] - s) / d[j] (i > j).  d[j] <= 1e-12 * gram[j][j]:
 *                 "loadings are rank deficient" (an all-zero pattern, collinear patterns)
 *   x = gram^-1 b: z[i] = b[i] - sum over m < i of U[i][m] * z[m]; y[i] = z[i] / d[i]; x[i] = y[i] - sum over m > i of U[m][i] * x[m], i
 *                 descending; both sums ascending in m from +0.0
 *   coef[:, s] = gram^-1 cross[:, s]                         stdevUnscaled[k] = sqrt(x[k]) for b = the unit vector e_k
 *   rss[s]      = sum over g of r * r, r = D[g][s] - fitted, fitted = sum over k, ascending from +0.0, of L[g][k] * coef[k][s] -- over every
 *                 position, the zeros of sparse data included
 * Every product of the factorisation, the substitutions and the fitted value is rounded before it is added (no fused multiply-add).
 * No output depends on the device, on the grid or on scheduling; each can be recomputed bit for bit.
 *
 * Outputs: coef and cross [nPatterns][nSamples], gram [nPatterns][nPatterns] (symmetric bit for bit), stdevUnscaled [nPatterns], rss
 * [nSamples]; all but coef may be NULL (without rss its pass is not run).  peakDeviceBytes (may be NULL): as for cogaps_residuals; a
 * sparse kind allocates nothing of the size genes x samples.  device: -1 for the calling thread's current one (it is restored before
 * the call returns).  Refused, with a message: loadings or coef NULL, no data, what cogaps_residuals refuses of a descriptor, an
 * uncertainty, empty data, nPatterns == 0 or above COGAPS_PROJECT_MAX_PATTERNS (the factor's packed triangle lives in LDS), nGenes <=
 * nPatterns, without dataRows a data set of another number of genes, a dataRows entry that is no row of the data, a loading that is not
 * finite, rank deficiency.
 * ---------------------------------------------------------------------------------------------- */
#define COGAPS_PROJECT_TRIP 1024
#define COGAPS_PROJECT_MAX_PATTERNS 128
int cogaps_project(const float *loadings, uint32_t nGenes, size_t lRowStride, size_t lColStride, uint32_t nPatterns,
                   const cogaps_residual_data *data, const uint32_t *dataRows, int device,
                   double *coef, double *rss, double *gram, double *stdevUnscaled, double *cross, uint64_t *peakDeviceBytes);

/* lanes of the evaluation workgroup for data vectors of length N (the reduction-order contract) */
uint32_t cogaps_reduction_width(uint32_t N);
/* threads (= virtual lanes) of the sparse model's evaluation workgroup: one per 64-bit flag word of a data vector, 64..256 */
uint32_t cogaps_sparse_width(uint32_t N);

#ifdef __cplusplus
}
#endif
#endif
