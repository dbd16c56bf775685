// session_build.h -- building a session's two samplers from every form of input (dense host, dense device, CSR / CSC, triplets, a
// device-matrix handle; both models; with or without subsetData and transposeData): host code only, a chapter of cogaps_hip.cpp, which
// includes it once, where the chapter used to stand -- after the kernel headers, HostSampler, cogaps_session, fail, dalloc and dev_env,
// which it takes from there.  Not a stand-alone header.  Kernels are instantiated, and laid out in the code object, in the order of their
// first use: the launch sites stay in the order they have here.  session_create and device_matrix_create (cogaps_hip.cpp) call the
// build_samplers_* / device_matrix_from_* entries and session_args_refusal; sampler_update.h takes build_death_prob_table; result_stats.h
// takes SpbTemps, SpbMatrix, sparse_args_refusal, spb_compressed, spb_triplets and spb_build_sides.  Steps written here once: the
// orientation rule (Orientation), a sampler's model and domain behind its data (finish_sampler), the timed ordered sum
// (timed_ordered_sum), the 64-bit total before the 32-bit scan (spb_checked_total), the grid of one wave per vector
// (SPB_LAUNCH_VECTORS), the kernels' view of an SpbMatrix (spb_in, coo_in), the dense model's data arrays (dense_data_alloc).
#pragma once

// SamplerDev::deathProb for the atom arrays' current capacity (the sampler's creation, grow_atoms)
static void build_death_prob_table(cogaps_session *s, SamplerDev &d)
{
    const uint32_t n = d.atomCap + GAPS_DEATH_PROB_PAD;
    float *tab = dalloc<float>(n);
    RT_LAUNCH(death_prob_table_kernel, (n + 255u) / 256u, 256, s->stream, tab, n, d.domainLenD, d.alphaD, d.numBins);
    rt_sync(s->stream);
    d.deathProb = tab;
}

static void free_sampler(HostSampler &h)
{
    SamplerDev &d = h.d;
    rt_free(d.seqScratch); rt_free((void *)d.deathProb); rt_free(d.launchClock);
    rt_free((void *)d.D); rt_free((void *)d.S2); rt_free(d.AP); rt_free(d.mat); rt_free(d.colPos);
    rt_free(d.atoms); rt_free(d.vec); rt_free(d.freeHandles); rt_free(d.binHead);
    rt_free(d.bits0); rt_free(d.bits1); rt_free(d.bits2); rt_free(d.eraseList); rt_free(d.queue); rt_free(d.queueUnits); rt_free(d.chainSlots); rt_free(h.chainGrans); rt_free(d.partials); rt_free(d.grans); rt_free(d.dec);
    rt_free(d.rowStamp); rt_free(d.atomStamp); rt_free(d.gapStamp); rt_free(d.inlineStamp); rt_free(d.atomDest);
    rt_free(d.gs); rt_free(d.trace); rt_free(d.traceBatchNproc); rt_free(d.traceBatchQlen);
    rt_free(h.Sraw); rt_free(h.seeds); rt_free_host(h.hSeeds); rt_free(h.partial); rt_free(h.dRecord);
    rt_free((void *)d.dflags); rt_free((void *)d.dprefix); rt_free((void *)d.dptr); rt_free((void *)d.dvals); rt_free(d.rows); rt_free(d.mflags); rt_free(d.Z1); rt_free(d.Z2);
}

// THE rule "which axis does the subset pick, which axis are the vectors" (Matrix.cpp:30-69, GapsRunner.cpp:402-406), for every builder
// and for the index check of session_create.  Genes are the input's rows unless transposeData; subsetData's indices pick genes or samples
// (subsetGenes), hence input rows or input columns.  Sampler A (side 0) is made from the transposed data with the subset flag flipped:
// its vectors are genes, its elements samples; sampler P (side 1) the other way round.
struct Orientation {
    bool subset, subsetRows;      // there is a subset; it picks input rows (a subset that does not picks input columns)
    uint32_t dim;                 // extent of the input axis the indices point into: their upper bound
    uint32_t nrow, ncol;          // the session's matrix in the input's orientation, after the subset
    // per sampler: Matrix(mat, genesInCols, subsetGenes, indices) -- its vectors are input rows (genesInCols) or input columns, the
    // subset picks its elements (subsetGenes) or its vectors; nS vectors of nG elements
    struct Side { bool genesInCols, subsetGenes; uint32_t nG, nS; } side[2];
    bool subsetCols() const { return subset && !subsetRows; }
    // the subset's indices as the map of input rows / of input columns (null: that axis is taken as it is)
    const uint32_t *rowMap(const uint32_t *indices) const { return subsetRows ? indices : nullptr; }
    const uint32_t *colMap(const uint32_t *indices) const { return subsetCols() ? indices : nullptr; }
};
// nSubset: the number of subset indices the session holds, 0 without subsetData; nrow x ncol: the input
static Orientation orientation(const cogaps_params &p, size_t nSubset, uint32_t nrow, uint32_t ncol)
{
    Orientation o;
    const bool picksRows = (p.subsetGenes != 0) == (p.transposeData == 0);
    o.subset = p.subsetData && nSubset != 0; o.subsetRows = o.subset && picksRows;
    o.dim = picksRows ? nrow : ncol;
    o.nrow = o.subsetRows ? (uint32_t)nSubset : nrow; o.ncol = o.subsetCols() ? (uint32_t)nSubset : ncol;
    for (int w = 0; w < 2; ++w) {
        Orientation::Side &sd = o.side[w];
        sd.genesInCols = (w == 0) == (p.transposeData == 0); sd.subsetGenes = (w == 0) == (p.subsetGenes == 0);
        sd.nG = sd.genesInCols ? o.ncol : o.nrow; sd.nS = sd.genesInCols ? o.nrow : o.ncol;
    }
    return o;
}
static HostSampler &sampler_of(cogaps_session *s, int w) { return w == 0 ? s->A : s->P; }

static void sampler_domain(cogaps_session *s, HostSampler &h, float alpha);
// dimensions of sampler w (0: A, 1: P) over nS data vectors of nG elements
static void sampler_dims(cogaps_session *s, int w, const Orientation &o)
{
    const cogaps_params &p = s->p;
    HostSampler &h = sampler_of(s, w);
    SamplerDev &d = h.d; memset(&d, 0, sizeof(d)); h.name = "AP"[w];
    d.N = o.side[w].nG; d.M = o.side[w].nS; d.K = p.nPatterns;
    d.seq = p.reductionMode == COGAPS_REDUCE_SEQ ? 1u : 0u; d.mathMode = (uint32_t)p.mathMode;
    d.Npad = (d.N + 3u) & ~3u; d.Mpad = (d.M + 3u) & ~3u;
    d.redW = cogaps_reduction_width(d.N);
    if (p.useSparseOptimization) {
        if (d.K > SP_KMAX) throw std::runtime_error("useSparseOptimization supports at most 512 patterns");
        d.Wn = d.N / 64u + 1u;
    }
}
// the DenseNormalModel constructor's constants (DenseNormalModel.h:66-88) from the data's ordered sum and its count of entries > 0
static void sampler_model(HostSampler &h, float alpha, float maxGibbsMass, float sum, unsigned nnz)
{
    SamplerDev &d = h.d;
    const float meanD = sum / (float)nnz;
    h.dataSparsity = 1.f - (float)(uint32_t)nnz / (float)(d.M * d.N);       // gaps::sparsity, MatrixMath.cpp:6-21 (unsigned count, float product of the dimensions)
    d.alpha = alpha;
    d.lambda = alpha * sqrtf((float)(uint64_t)d.K / meanD);
    d.maxGibbsMass = maxGibbsMass / d.lambda;
    d.unitBytes = 4u * d.N;
}
// the sparse model beside its packed data (dflags, dprefix, dptr, dvals: sparse_build.h, whatever form the input had -- the only data a
// sparse-model session holds: d.D, d.S2 and h.Sraw stay null): the HybridMatrix copies and the lookup tables
static void sampler_sparse_model(HostSampler &h)
{
    SamplerDev &d = h.d;
    d.sparse = 1; d.beta = 100.f; d.unitBytes = 1u;
    d.Mw = d.M / 64u + 1u; d.Kpad = (d.K + 3u) & ~3u; d.spW = cogaps_sparse_width(d.N);
    d.rows = dalloc<float>((size_t)d.M * d.Kpad);
    d.mflags = dalloc<unsigned long long>((size_t)d.K * d.Mw);
    d.Z1 = dalloc<float>(d.K); d.Z2 = dalloc<float>((size_t)d.K * d.K);
    if (d.seq) {
        if (d.Wn > (uint32_t)SP_SEQ_WORDS) throw std::runtime_error("reductionMode SEQ with the sparse model supports data vectors of up to 262080 elements");
        d.seqScratch = dalloc<float>((size_t)SEQ_SPARSE_GRID * 3u * d.Npad);
    }
}
// Sampler w's data are in place: its model from their ordered sum and count of entries > 0, what the model keeps beside the data (the
// sparse model's copies and tables, the dense model's A*P cache), then its matrix, atomic domain and queue.  Every builder ends with this,
// for A before P: sampler_domain takes the seeder's next output (A's queue, then P's, then the runner: part of the chain).
static void finish_sampler(cogaps_session *s, int w, float sum, unsigned nnz)
{
    const cogaps_params &p = s->p;
    HostSampler &h = sampler_of(s, w);
    const float alpha = w == 0 ? p.alphaA : p.alphaP;
    sampler_model(h, alpha, w == 0 ? p.maxGibbsMassA : p.maxGibbsMassP, sum, nnz);
    if (p.useSparseOptimization) sampler_sparse_model(h); else h.d.AP = dalloc<float>((size_t)h.d.M * h.d.Npad);
    sampler_domain(s, h, alpha);
}
// Runs launch() -- the ordered sums of both samplers' data -- between two events on the session's stream, reads its `bytes` of results
// back from dev and waits; what the launch took is the session's to report (cogaps_session_sparse_build_ms)
template <class Launch> static void timed_ordered_sum(cogaps_session *s, void *host, const void *dev, size_t bytes, Launch &&launch)
{
    rt_event_pair ev; rt_event_create(ev); rt_event_start(ev, s->stream);
    launch();
    rt_event_stop(ev, s->stream);
    rt_d2h(host, dev, bytes, s->stream); rt_sync(s->stream);
    s->orderedSumMs = rt_event_ms(ev); rt_event_destroy(ev);
}

// The dense model's data arrays of a sampler whose dimensions are set -- D, S2, Sraw [M][Npad], the session's from here on -- and their
// length.  With the default uncertainty the evaluation kernel recomputes S*S = max(0.1 D, 0.1)^2 from the D value it loads anyway
// (bit-identical: the same three fp32 operations as the builders' fill): no S2 array, one row less per proposal from HBM.
// (COGAPS_READ_S: diagnostics, keeps the array and the loads.)
struct DenseData { float *D, *S2, *Sraw; size_t tot; };
static DenseData dense_data_alloc(HostSampler &h, const float *unc)
{
    SamplerDev &d = h.d;
    const bool defaultS = unc == nullptr && !dev_env("COGAPS_READ_S");
    DenseData a; a.tot = (size_t)d.M * d.Npad;
    a.D = dalloc<float>(a.tot); a.S2 = defaultS ? nullptr : dalloc<float>(a.tot); a.Sraw = dalloc<float>(a.tot);
    d.D = a.D; d.S2 = a.S2; h.Sraw = a.Sraw; d.defaultS = defaultS ? 1u : 0u;
    return a;
}

// The dense model's sampler w from host input: Matrix(mat, genesInCols, subsetGenes, indices) (data_structures/Matrix.cpp:30-69) laid
// out as [vector j][element i] + the DenseNormalModel constructor (DenseNormalModel.h:66-88)
static void build_sampler(cogaps_session *s, int w, const Orientation &o, const float *data, uint32_t ncol, const float *unc)
{
    const uint32_t *indices = s->subset.data();
    const bool genesInCols = o.side[w].genesInCols;
    HostSampler &h = sampler_of(s, w); SamplerDev &d = h.d;
    sampler_dims(s, w, o);
    const DenseData a = dense_data_alloc(h, unc);
    // The vectors are staged through the host in blocks of at most 16 M elements (pad: D = 0, S = S2 = 1) -- never three dense
    // host copies of the matrix (BASELINE configs[4]'s shard is 2.5 GB per copy).  The sums run over the vectors in order, as
    // gaps::nonZeroMean does (MatrixMath.cpp:39-55).
    const uint32_t rowsPerBlock = (uint32_t)std::max<size_t>(1, std::min<size_t>(d.M, ((size_t)1 << 24) / std::max<uint32_t>(1u, d.Npad)));
    std::vector<float> D((size_t)rowsPerBlock * d.Npad), S2(a.S2 ? D.size() : 0), SR(D.size());
    float sum = 0.f; unsigned nnz = 0;
    for (uint32_t j0 = 0; j0 < d.M; j0 += rowsPerBlock) {
        const uint32_t j1 = std::min(d.M, j0 + rowsPerBlock);
        std::fill(D.begin(), D.end(), 0.f); std::fill(SR.begin(), SR.end(), 1.f); if (a.S2) std::fill(S2.begin(), S2.end(), 1.f);
        for (uint32_t j = j0; j < j1; ++j) {
            for (uint32_t i = 0; i < d.N; ++i) {
                const uint32_t row = genesInCols ? j : i, col = genesInCols ? i : j;      // of the session's matrix: through the subset to the input's
                const uint32_t dataRow = o.subsetRows ? indices[row] - 1 : row, dataCol = o.subsetCols() ? indices[col] - 1 : col;
                const float v = data[(size_t)dataRow * ncol + dataCol];
                const size_t at = (size_t)(j - j0) * d.Npad + i;
                D[at] = v;
                const float sd = unc ? unc[(size_t)dataRow * ncol + dataCol] : gm_max(v * 0.1f, 0.1f);   // gaps::pmax, MatrixMath.cpp:74-84
                SR[at] = sd; if (a.S2) S2[at] = sd * sd;
                sum += v; if (v > 0.f) ++nnz;                                    // gaps::nonZeroMean, MatrixMath.cpp:39-55
            }
        }
        const size_t off = (size_t)j0 * d.Npad, cnt = (size_t)(j1 - j0) * d.Npad;
        rt_h2d(a.D + off, D.data(), cnt * 4, s->stream); if (a.S2) rt_h2d(a.S2 + off, S2.data(), cnt * 4, s->stream);
        rt_h2d(a.Sraw + off, SR.data(), cnt * 4, s->stream);
        rt_sync(s->stream);                                                     // the staging buffers are reused by the next block
    }
    finish_sampler(s, w, sum, nnz);
}

// the sampler's own state behind its data: the matrix, the atomic domain, the proposal queue (the seed of the queue's generator is
// the session seeder's next output: A's sampler first, then P's)
static void sampler_domain(cogaps_session *s, HostSampler &h, float alpha)
{
    SamplerDev &d = h.d;
    d.mat = dalloc<float>((size_t)d.K * d.Mpad);
    d.colPos = dalloc<uint32_t>(d.K);
    d.luts.erf = s->dErf; d.luts.erfinv = s->dErfinv; d.luts.qgamma = s->dQgamma;
    // atomic domain
    const uint64_t nBins = (uint64_t)d.M * d.K;
    d.atomCap = (uint32_t)std::min<uint64_t>(nBins + 65536ull, 0x7FFFFFF0ull);
    if (const char *e = getenv("COGAPS_INITIAL_ATOM_CAP")) d.atomCap = (uint32_t)std::max(64l, atol(e));      // tests: exercises grow_atoms
    d.atoms = dalloc<AtomRec>(d.atomCap); d.vec = dalloc<uint32_t>(d.atomCap); d.freeHandles = dalloc<uint32_t>(d.atomCap);
    d.binHead = dalloc<uint32_t>(nBins); rt_memset(d.binHead, 0xFF, nBins * 4, s->stream);
    d.nWords0 = (uint32_t)((nBins + 63) / 64); d.nWords1 = (d.nWords0 + 63) / 64; d.nWords2 = (d.nWords1 + 63) / 64;
    d.bits0 = dalloc<unsigned long long>(d.nWords0); d.bits1 = dalloc<unsigned long long>(d.nWords1); d.bits2 = dalloc<unsigned long long>(d.nWords2);
    d.queueCap = d.M + 8; d.eraseCap = d.queueCap;
    d.eraseList = dalloc<unsigned long long>(d.eraseCap); d.queue = dalloc<PropRec>((size_t)2 * d.queueCap); d.chainSlots = dalloc<ChainSlot>(2); d.launchClock = dalloc<unsigned long long>(2u * GAPS_CLOCK_RING); h.chainGrans = dalloc<unsigned long long>((size_t)d.queueCap * CHAIN_GRAN_STRIDE); d.queueUnits = dalloc<uint32_t>(d.queueCap); d.partials = dalloc<float>((size_t)d.queueCap * 64); d.grans = dalloc<unsigned long long>((size_t)d.queueCap * 64); d.dec = dalloc<DecRec>(d.queueCap);
    d.rowStamp = dalloc<unsigned long long>(d.M);
    d.atomStamp = dalloc<unsigned long long>(d.atomCap); d.gapStamp = dalloc<unsigned long long>((size_t)d.atomCap + 1);
    d.inlineStamp = dalloc<unsigned long long>(d.atomCap); d.atomDest = dalloc<uint64_t>(d.atomCap);
    d.lcgMul = s->dLcgMul; d.lcgInc = s->dLcgInc;
    d.binLength = 0xFFFFFFFFFFFFFFFFull / nBins;               // ProposalQueue.cpp:27
    d.domainLenU = d.binLength * nBins;                         // ConcurrentAtomicDomain.cpp:16-18
    d.domainLenD = (double)d.domainLenU;                        // ProposalQueue.cpp:30
    d.numBins = (double)nBins; d.alphaD = (double)alpha;
    d.invBinLen = 1.0 / (double)d.binLength;
    d.invK = 1.0 / (double)d.K;
    if (nBins >= 0xFFFFFFF0ull) throw std::runtime_error("rows x nPatterns must stay below 2^32");
    d.rboundNone = gm_u64_from_double_x86(d.domainLenD);
    d.iPartL = 0xFFFFFFFFFFFFFFFFull / d.domainLenU; d.limitL = d.domainLenU * d.iPartL;   // uniform64(1, L)
    build_death_prob_table(s, d);
    d.gs = dalloc<GenScalars>(1);
    GenScalars g; memset(&g, 0, sizeof(g));
    g.front = CG_NONE;
    g.qrng = pcg_from_seed(s->seeder.next());                   // ProposalQueue::mRng(randState), ProposalQueue.cpp:24
    rt_h2d(d.gs, &g, sizeof(g), s->stream); rt_sync(s->stream);
    h.partial = dalloc<float>(d.M);
}

// a kernel that gives one wave to each of n vectors (or major slices), SPB_WAVES of them per workgroup
#define SPB_LAUNCH_VECTORS(KERNEL, n, stream, ...) \
    RT_LAUNCH(KERNEL, ((uint32_t)(n) + (uint32_t)SPB_WAVES - 1u) / (uint32_t)SPB_WAVES, 64 * SPB_WAVES, stream, __VA_ARGS__)

static void spb_check_entries(uint64_t n)
{
    if (n >= 0xFFFFFFFFull) throw std::runtime_error("compressed-sparse matrix: 2^32 - 1 stored entries or more (the packed values are indexed by 32 bits)");
}
// The total of n per-vector counts in device memory, taken in 64 bits before the 32-bit scan runs over them: refused where the packed
// values could not be indexed
static uint64_t spb_checked_total(const uint32_t *dCounts, uint32_t n, rt_stream_t stream)
{
    std::vector<uint32_t> counts(n); rt_d2h(counts.data(), dCounts, (size_t)n * 4, stream); rt_sync(stream);
    uint64_t total = 0; for (uint32_t c : counts) total += c;
    spb_check_entries(total);
    return total;
}

// side[w].ptr holds the kept entries per vector: their exclusive scan, the packed values' allocation (allocVals(w, count): the side's
// owner makes it), the prefix counts; returns the number of kept entries
template <class AllocVals>
static uint32_t spb_scan_and_allocate(rt_stream_t stream, SpbSide *side, int nSides, AllocVals &&allocVals)
{
    uint32_t kept[2] = {0, 0};
    for (int w = 0; w < nSides; ++w) { RT_LAUNCH(spb_scan_kernel, 1, SPB_SCAN_BS, stream, side[w].ptr, side[w].M); rt_d2h(&kept[w], side[w].ptr + side[w].M, 4, stream); }
    rt_sync(stream);
    if (nSides == 2 && kept[0] != kept[1]) throw std::runtime_error("internal: the two samplers count different numbers of entries");
    for (int w = 0; w < nSides; ++w) {
        side[w].vals = allocVals(w, (size_t)kept[w] + 1);
        SPB_LAUNCH_VECTORS(spb_prefix_kernel, side[w].M, stream, side[w]);
    }
    return kept[0];
}
// the packed values are in place: each sampler's ordered sum (sums: two floats of device scratch), then the model and the atomic domain
static void spb_models(cogaps_session *s, SpbSide *side, uint32_t kept, float *sums)
{
    // gaps::nonZeroMean (MatrixMath.cpp:39-55): each sampler's sum in the order of its own vectors
    float sum[2] = {0.f, 0.f};
    timed_ordered_sum(s, sum, sums, sizeof(sum), [&] {
        RT_LAUNCH(spb_ordered_sum_kernel, 2, 256, s->stream, (const float *)side[0].vals, (const float *)side[1].vals, kept, sums); });
    for (int w = 0; w < 2; ++w) finish_sampler(s, w, sum[w], kept);
}
// The two samplers' dimensions and their flag / prefix / pointer arrays (the session's from here on: free_sampler releases them if anything
// later throws).  The sampler whose vector axis is the input's minor axis takes its entries transposed (SpbSide::swap)
static void spb_sides(cogaps_session *s, const Orientation &o, bool majorIsRow, SpbSide *side)
{
    for (int w = 0; w < 2; ++w) {
        sampler_dims(s, w, o);
        SamplerDev &d = sampler_of(s, w).d; SpbSide &sd = side[w];
        const bool vectorsAreRows = o.side[w].genesInCols;
        sd.M = d.M; sd.Wn = d.Wn; sd.swap = vectorsAreRows == majorIsRow ? 0u : 1u; sd.vals = nullptr;
        sd.flags = dalloc<unsigned long long>((size_t)d.M * d.Wn); sd.prefix = dalloc<uint32_t>((size_t)d.M * d.Wn); sd.ptr = dalloc<uint32_t>((size_t)d.M + 1);
        d.dflags = sd.flags; d.dprefix = sd.prefix; d.dptr = sd.ptr;
    }
}

// Device temporaries of a call -- a build's, a result statistic's (result_stats.h): not a session's (allocated under a null owner scope),
// released when their owner goes, however the call ends
struct SpbTemps {
    std::vector<void *> p;
    ~SpbTemps() { for (void *q : p) rt_free(q); }
    template <class T> T *alloc(size_t count)
    {
        p.push_back(nullptr);      // (the slot first: nothing is ever allocated that has no place here)
        rt_owner_scope notTheSessions(nullptr); p.back() = dalloc<T>(count); return (T *)p.back();
    }
    // one of the caller's arrays where the kernels read it: uploaded, or used where it is
    template <class T> const T *stage(const T *src, size_t count, bool onDevice, rt_stream_t stream)
    {
        if (onDevice) return src;
        T *q = alloc<T>(count + 1);
        if (count) rt_h2d(q, src, count * sizeof(T), stream);
        return q;
    }
    uint32_t *err() { return alloc<uint32_t>(4); }      // the error word, the two ordered sums
};

// A sparse-model matrix in device memory as the one builder reads it: a plain description that owns nothing.  The arrays are a
// caller's, staged for one session (build_samplers_sparse_input / _coo_input), or a cogaps_device_matrix's; either way they have been
// through spb_compressed or spb_triplets -- checked, triplets resolved into keep[] -- before anything is built from them.
struct SpbMatrix {
    uint32_t nrow = 0, ncol = 0; uint64_t nnz = 0;
    bool coo = false, majorIsRow = true;
    const uint64_t *indptr = nullptr; const uint32_t *indices = nullptr;      // compressed: [nMajor + 1], [nnz]
    const uint32_t *rows = nullptr, *cols = nullptr;                          // triplets: [nnz]
    const unsigned long long *keep = nullptr;                                 // triplets: bit k = entry k is the latest of its position and > 0
    const float *values = nullptr;
    uint32_t nMajor() const { return majorIsRow ? nrow : ncol; }
    uint32_t nMinor() const { return majorIsRow ? ncol : nrow; }
};
// the matrix as the kernels of sparse_build.h take it: its compressed form, its triplets
static SpbIn spb_in(const SpbMatrix &d)
{
    SpbIn in; in.nMajor = d.nMajor(); in.nMinor = d.nMinor(); in.nnz = d.nnz; in.indptr = d.indptr; in.indices = d.indices; in.values = d.values;
    return in;
}
static CooIn coo_in(const SpbMatrix &d)
{
    CooIn in; in.nrow = d.nrow; in.ncol = d.ncol; in.nnz = d.nnz; in.rows = d.rows; in.cols = d.cols; in.values = d.values;
    return in;
}
static uint32_t entry_grid(uint64_t n, unsigned computeUnits, uint32_t bs)
{
    // grid-stride over the entries: enough workgroups to fill the device, never more than the entries need (at least one)
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + bs - 1) / bs, (uint64_t)computeUnits * 8u));
}
// What a caller's sparse matrix is refused for before anything else is looked at (null: nothing)
static const char *sparse_args_refusal(const cogaps_sparse_matrix *sp, const cogaps_coo_matrix *coo)
{
    if (sp) return sp->indptr ? nullptr : "null argument: indptr";
    if (!coo) return nullptr;
    if (coo->nnz >= 0xFFFFFFFFull) return "triplet matrix: 2^32 - 1 entries or more (entries and packed values are indexed by 32 bits)";
    if (coo->nnz && (!coo->rows || !coo->cols || !coo->values)) return "null argument: rows / cols / values";
    return nullptr;
}

// The caller's compressed matrix, checked (sparse_build.h, spb_validate_kernel), as d.  place(array, count) puts one of the caller's
// arrays where the kernels read it and says where that is: staged for the call, or copied into a handle's own memory.
template <class Place> static void spb_compressed(SpbMatrix &d, const cogaps_sparse_matrix &m, rt_stream_t stream, Place &&place)
{
    d.nrow = m.nrow; d.ncol = m.ncol; d.coo = false; d.majorIsRow = m.majorIsRow != 0;
    const uint32_t nMajor = d.nMajor();
    if (m.onDevice) { rt_d2h(&d.nnz, m.indptr + nMajor, 8, stream); rt_sync(stream); } else d.nnz = m.indptr[nMajor];
    spb_check_entries(d.nnz);
    if (d.nnz && (!m.indices || !m.values)) throw std::runtime_error("null argument: indices / values");
    d.indptr = place(m.indptr, (size_t)nMajor + 1); d.indices = place(m.indices, (size_t)d.nnz); d.values = place(m.values, (size_t)d.nnz);
    SpbTemps tmp; uint32_t *err = tmp.err();
    const SpbIn in = spb_in(d);
    SPB_LAUNCH_VECTORS(spb_validate_kernel, nMajor, stream, in, err);
    uint32_t code = 0; rt_d2h(&code, err, 4, stream); rt_sync(stream);
    if (code == SPB_ERR_INDPTR) throw std::runtime_error("compressed-sparse matrix: indptr must start at 0, never decrease and end at the number of stored entries");
    if (code == SPB_ERR_RANGE) throw std::runtime_error("compressed-sparse matrix: an index is outside the minor dimension");
    if (code != 0) throw std::runtime_error("compressed-sparse matrix: the indices of a row / column must be strictly ascending (sorted, no duplicates)");
}

// The caller's triplets, checked and resolved (sparse_build.h, passes 1 to 4 of its second half), as d: keep -- nnz / 64 + 1 words, the
// caller's to own -- gets one bit per entry.  The present flags with their prefix counts and pointers and the winner indices are
// temporaries of this call: O(nnz + nrow x ncol / 64 bits).
template <class Place>
static void spb_triplets(SpbMatrix &d, const cogaps_coo_matrix &m, unsigned long long *keep, unsigned computeUnits, rt_stream_t stream, Place &&place)
{
    d.keep = keep;
    d.nrow = m.nrow; d.ncol = m.ncol; d.coo = true; d.majorIsRow = true; d.nnz = m.nnz;
    d.rows = place(m.rows, (size_t)d.nnz); d.cols = place(m.cols, (size_t)d.nnz); d.values = place(m.values, (size_t)d.nnz);
    SpbTemps tmp; uint32_t *err = tmp.err();
    const CooIn in = coo_in(d);
    SpbSide pres; pres.M = d.nrow; pres.Wn = d.ncol / 64u + 1u; pres.swap = 0u; pres.vals = nullptr;
    pres.flags = tmp.alloc<unsigned long long>((size_t)pres.M * pres.Wn); pres.prefix = tmp.alloc<uint32_t>((size_t)pres.M * pres.Wn);
    pres.ptr = tmp.alloc<uint32_t>((size_t)pres.M + 1);
    const uint32_t grid = entry_grid(d.nnz, computeUnits, COO_BS);
    RT_LAUNCH(coo_present_kernel, grid, COO_BS, stream, in, pres, err);
    uint32_t code = 0; rt_d2h(&code, err, 4, stream); rt_sync(stream);
    if (code != 0) throw std::runtime_error("triplet matrix: a row or column index is outside the stated dimensions");
    SPB_LAUNCH_VECTORS(spb_count_kernel, pres.M, stream, pres);
    RT_LAUNCH(spb_scan_kernel, 1, SPB_SCAN_BS, stream, pres.ptr, pres.M);
    SPB_LAUNCH_VECTORS(spb_prefix_kernel, pres.M, stream, pres);
    uint32_t nPresent = 0; rt_d2h(&nPresent, pres.ptr + pres.M, 4, stream); rt_sync(stream);
    uint32_t *winner = tmp.alloc<uint32_t>((size_t)nPresent + 1);
    RT_LAUNCH(coo_winner_kernel, grid, COO_BS, stream, in, pres, winner);
    RT_LAUNCH(coo_keep_bits_kernel, grid, COO_BS, stream, in, pres, (const uint32_t *)winner, keep);
    rt_sync(stream);
}

// The builder's passes over a checked matrix in device memory (sparse_build.h, passes 3 to 5 of the mapped route): the flag bits, the
// counts, their scan, the prefix counts and the packed values of the sides given, whose flags / prefix / ptr arrays are allocated and
// zero.  Two sides: a session's samplers.  One side: the gene side alone, which is all the residuals of a result read
// (cogaps_residuals) -- the mapped kernels then get that side for both of theirs, see that the two are one (spb_mapped_entry) and
// set every bit, and store every value, once.  mapped: the map repeats indices, so the kept entries are counted in 64 bits before the
// 32-bit scan (without a map they cannot exceed nnz).  Returns the number of kept entries.
template <class AllocVals>
static uint32_t spb_build_sides(const SpbMatrix &dm, const SpbMap &mp, bool mapped, SpbSide *side, int nSides, unsigned computeUnits, rt_stream_t stream,
                                AllocVals &&allocVals)
{
    const SpbSide &a = side[0], &b = side[nSides - 1];
    const SpbIn in = spb_in(dm); const CooIn cin = coo_in(dm);
    const uint32_t grid = entry_grid(dm.nnz, computeUnits, COO_BS);
    if (dm.coo) RT_LAUNCH(coo_mapped_kernel<false>, grid, COO_BS, stream, cin, dm.keep, mp, a, b);
    else SPB_LAUNCH_VECTORS(spb_mapped_kernel<false>, in.nMajor, stream, in, mp, a, b);
    for (int w = 0; w < nSides; ++w) SPB_LAUNCH_VECTORS(spb_count_kernel, side[w].M, stream, side[w]);
    if (mapped) spb_checked_total(side[0].ptr, side[0].M, stream);
    const uint32_t kept = spb_scan_and_allocate(stream, side, nSides, allocVals);
    // (the sides now carry their vals: the references above see them)
    if (dm.coo) RT_LAUNCH(coo_mapped_kernel<true>, grid, COO_BS, stream, cin, dm.keep, mp, a, b);
    else SPB_LAUNCH_VECTORS(spb_mapped_kernel<true>, in.nMajor, stream, in, mp, a, b);
    return kept;
}

// Both samplers of a sparse-model session from a checked matrix in device memory, with or without a subset of its rows or columns
// (sparse_build.h, the map and the mapped passes): THE builder of the sparse model, whatever form the input had.  subset: subsetData's
// 1-based indices, or null -- also for a caller that has applied them already.  One read of the entries per mapped pass; the session's
// allocations are those of any sparse-model session, the temporaries (the subset's indices, counts, cursors, list) O(dim + n).  Nothing
// is uploaded but the subset's indices.
static void build_samplers_device_matrix(cogaps_session *s, const SpbMatrix &dm, const std::vector<uint32_t> *subset)
{
    const uint32_t nIdx = subset ? (uint32_t)subset->size() : 0u;
    const Orientation o = orientation(s->p, nIdx, dm.nrow, dm.ncol);
    SpbTemps tmp;
    SpbSide side[2];
    spb_sides(s, o, dm.majorIsRow, side);
    SpbMap mp; mp.start = mp.list = nullptr; mp.onMajor = o.subsetRows == dm.majorIsRow ? 1u : 0u;
    if (o.subset) {
        const uint32_t *indices = tmp.stage(subset->data(), nIdx, false, s->stream);
        uint32_t *start = tmp.alloc<uint32_t>((size_t)o.dim + 1), *cursor = tmp.alloc<uint32_t>(o.dim), *list = tmp.alloc<uint32_t>(nIdx);
        const uint32_t mapGrid = entry_grid(nIdx, s->computeUnits, SPB_MAP_BS);
        RT_LAUNCH(spb_map_count_kernel, mapGrid, SPB_MAP_BS, s->stream, indices, nIdx, start);
        RT_LAUNCH(spb_scan_kernel, 1, SPB_SCAN_BS, s->stream, start, o.dim);
        RT_LAUNCH(spb_map_fill_kernel, mapGrid, SPB_MAP_BS, s->stream, indices, nIdx, (const uint32_t *)start, cursor, list);
        mp.start = start; mp.list = list;
    }
    const uint32_t kept = spb_build_sides(dm, mp, o.subset, side, 2, s->computeUnits, s->stream,
                                          [&](int w, size_t n) { float *v = dalloc<float>(n); sampler_of(s, w).d.dvals = v; return v; });
    spb_models(s, side, kept, (float *)(tmp.err() + 1));
}

// The one-shot entries: the caller's arrays staged for this call (SpbTemps::stage: uploaded from host pointers, read in place from
// device pointers), checked, then the builder with no subset.  A compressed-sparse matrix is the caller's (cogaps_session_create_sparse)
// or a dense input's entries > 0 (build_samplers_dense_input, build_samplers_dense_device_sparse); triplets (cogaps_session_create_coo)
// make the session cogaps_session_create makes from the matrix they denote -- the latest entry of a position decides it.  No nrow x ncol
// array exists on either side.
static void build_samplers_sparse_input(cogaps_session *s, const cogaps_sparse_matrix &m)
{
    SpbTemps tmp; SpbMatrix d;
    spb_compressed(d, m, s->stream, [&](auto *src, size_t n) { return tmp.stage(src, n, m.onDevice != 0, s->stream); });
    build_samplers_device_matrix(s, d, nullptr);
}
static void build_samplers_coo_input(cogaps_session *s, const cogaps_coo_matrix &m)
{
    SpbTemps tmp; SpbMatrix d;
    spb_triplets(d, m, tmp.alloc<unsigned long long>((size_t)(m.nnz / 64 + 1)), s->computeUnits, s->stream,
                 [&](auto *src, size_t n) { return tmp.stage(src, n, m.onDevice != 0, s->stream); });
    build_samplers_device_matrix(s, d, nullptr);
}

// The sparse model from a dense matrix: its entries > 0 (SparseVector.cpp:20-33: NaN, zero and negative values are absent), row by row
// in the data's own orientation, as the CSR matrix build_samplers_sparse_input takes.  subsetData picks rows or columns here, by
// Matrix.cpp:30-69's rule (Orientation): 1-based indices in the order given; output row / column i is input indices[i] - 1, so the column
// indices ascend whatever the order of the subset.
static void build_samplers_dense_input(cogaps_session *s, const float *data, uint32_t nrow, uint32_t ncol)
{
    const Orientation o = orientation(s->p, s->subset.size(), nrow, ncol);
    const uint32_t *indices = s->subset.data();
    cogaps_sparse_matrix m; memset(&m, 0, sizeof(m));
    m.nrow = o.nrow; m.ncol = o.ncol; m.majorIsRow = 1;
    std::vector<uint64_t> indptr((size_t)m.nrow + 1, 0); std::vector<uint32_t> cols; std::vector<float> vals;
    for (uint32_t r = 0; r < m.nrow; ++r) {
        const float *row = data + (size_t)(o.subsetRows ? indices[r] - 1 : r) * ncol;
        for (uint32_t c = 0; c < m.ncol; ++c) {
            const float v = row[o.subsetCols() ? indices[c] - 1 : c];
            if (v > 0.f) { cols.push_back(c); vals.push_back(v); }
        }
        indptr[(size_t)r + 1] = vals.size();
    }
    m.indptr = indptr.data(); m.indices = cols.data(); m.values = vals.data();
    build_samplers_sparse_input(s, m);
}

// A matrix resident on one device: the description with device copies of the caller's arrays, which it owns -- checked and, for
// triplets, resolved once, at its creation.  Immutable from then on: any number of sessions, on any host threads, are built from it
// (build_samplers_device_matrix) and copy nothing of it but what their packed structures hold.
struct cogaps_device_matrix {
    SpbMatrix m;
    int device = 0; unsigned computeUnits = 0;
    std::atomic<uint64_t> deviceBytes{0};
    ~cogaps_device_matrix() { rt_free((void *)m.indptr); rt_free((void *)m.indices); rt_free((void *)m.rows); rt_free((void *)m.cols); rt_free((void *)m.keep); rt_free((void *)m.values); }
};
// one of the caller's arrays into the handle's own memory (count + 1 elements: never an empty allocation)
template <class T> static T *dm_copy(const T *src, size_t count, bool onDevice, rt_stream_t stream)
{
    T *q = dalloc<T>(count + 1);
    if (count) { if (onDevice) rt_d2d(q, src, count * sizeof(T), stream); else rt_h2d(q, src, count * sizeof(T), stream); }
    return q;
}
static void device_matrix_from_sparse(cogaps_device_matrix *dm, const cogaps_sparse_matrix &m, rt_stream_t stream)
{
    spb_compressed(dm->m, m, stream, [&](auto *src, size_t n) { return dm_copy(src, n, m.onDevice != 0, stream); });
}
static void device_matrix_from_coo(cogaps_device_matrix *dm, const cogaps_coo_matrix &m, rt_stream_t stream)
{
    spb_triplets(dm->m, m, dalloc<unsigned long long>((size_t)(m.nnz / 64 + 1)), dm->computeUnits, stream,
                 [&](auto *src, size_t n) { return dm_copy(src, n, m.onDevice != 0, stream); });
}

// ---- dense input resident on the device (cogaps_session_create with data_on_device = 1; dense_build.h) ----
// subsetData's indices in device memory (a temporary), or null without a subset
static const uint32_t *dnb_subset(cogaps_session *s, const Orientation &o, SpbTemps &tmp)
{
    return o.subset ? tmp.stage(s->subset.data(), s->subset.size(), false, s->stream) : nullptr;
}
static uint32_t dnb_grid(uint64_t workgroups)
{
    if (workgroups == 0 || workgroups > 0x7FFFFFFFull) throw std::runtime_error("the matrix has more tiles than one launch has workgroups");
    return (uint32_t)workgroups;
}

// Both samplers of the dense model from the device-resident matrix: build_sampler's arrays and constants, bit for bit, with nothing of
// the matrix on the host.  Per sampler one fill launch (D, Sraw, S2 if kept, the pads, the count of entries > 0), then both ordered sums
// in one launch (its time: cogaps_session_sparse_build_ms), then the models and the atomic domains in build_sampler's order -- the
// seeder's outputs go to A's queue, then P's.  The session owns what build_sampler's session owns; the indices, the sums and the
// counts are temporaries.
static void build_samplers_dense_device(cogaps_session *s, const float *data, uint32_t nrow, uint32_t ncol, const float *unc)
{
    const Orientation o = orientation(s->p, s->subset.size(), nrow, ncol);
    SpbTemps tmp;
    const uint32_t *dIdx = dnb_subset(s, o, tmp);
    uint32_t *scratch = tmp.err();      // [0], [1]: the counts of entries > 0, [2], [3]: the ordered sums (as floats)
    size_t tot[2];
    for (int w = 0; w < 2; ++w) {
        HostSampler &h = sampler_of(s, w); SamplerDev &d = h.d;
        sampler_dims(s, w, o);
        const DenseData a = dense_data_alloc(h, unc); tot[w] = a.tot;
        DnbIn in; in.data = data; in.unc = unc; in.nrow = nrow; in.ncol = ncol;
        DnbOut out; out.D = a.D; out.Sraw = a.Sraw; out.S2 = a.S2; out.M = d.M; out.N = d.N; out.Npad = d.Npad;
        if (o.side[w].genesInCols) {      // the vectors are input rows
            in.vecMap = o.rowMap(dIdx); in.elMap = o.colMap(dIdx);
            const uint32_t chunks = (d.Npad + (uint32_t)DNB_BS - 1u) / (uint32_t)DNB_BS;
            RT_LAUNCH(dnb_rows_kernel, dnb_grid((uint64_t)d.M * chunks), DNB_BS, s->stream, in, out, chunks, scratch + w);
        } else {                          // the vectors are input columns
            in.vecMap = o.colMap(dIdx); in.elMap = o.rowMap(dIdx);
            const uint32_t tilesI = (d.Npad + (uint32_t)DNB_TILE - 1u) / (uint32_t)DNB_TILE, tilesJ = (d.M + (uint32_t)DNB_TILE - 1u) / (uint32_t)DNB_TILE;
            RT_LAUNCH(dnb_cols_kernel, dnb_grid((uint64_t)tilesI * tilesJ), DNB_BS, s->stream, in, out, tilesI, scratch + w);
        }
    }
    uint32_t host[4];
    timed_ordered_sum(s, host, scratch, sizeof(host), [&] {
        RT_LAUNCH(dnb_ordered_sum_kernel, 2, DNB_SUM_BS, s->stream, s->A.d.D, (uint64_t)tot[0], s->P.d.D, (uint64_t)tot[1], (float *)(scratch + 2)); });
    for (int w = 0; w < 2; ++w) {
        float sum; memcpy(&sum, &host[2 + w], 4);
        finish_sampler(s, w, sum, host[w]);
    }
}

// The sparse model from the device-resident matrix: build_samplers_dense_input's CSR matrix -- the entries > 0 of the subset's rows and
// columns, ascending column indices -- compacted on the device, then the one builder.  The CSR arrays are temporaries of this call.
static void build_samplers_dense_device_sparse(cogaps_session *s, const float *data, uint32_t nrow, uint32_t ncol)
{
    const Orientation o = orientation(s->p, s->subset.size(), nrow, ncol);
    SpbTemps tmp;
    const uint32_t *dIdx = dnb_subset(s, o, tmp);
    cogaps_sparse_matrix m; memset(&m, 0, sizeof(m));
    m.nrow = o.nrow; m.ncol = o.ncol; m.majorIsRow = 1; m.onDevice = 1;
    DnbIn in; in.data = data; in.unc = nullptr; in.nrow = nrow; in.ncol = ncol; in.vecMap = o.rowMap(dIdx); in.elMap = o.colMap(dIdx);
    uint32_t *ptr = tmp.alloc<uint32_t>((size_t)m.nrow + 1);
    SPB_LAUNCH_VECTORS(dnb_csr_count_kernel, m.nrow, s->stream, in, m.nrow, m.ncol, ptr);
    const uint64_t total = spb_checked_total(ptr, m.nrow, s->stream);
    RT_LAUNCH(spb_scan_kernel, 1, SPB_SCAN_BS, s->stream, ptr, m.nrow);
    uint64_t *indptr = tmp.alloc<uint64_t>((size_t)m.nrow + 1); uint32_t *indices = tmp.alloc<uint32_t>((size_t)total + 1);
    float *values = tmp.alloc<float>((size_t)total + 1);
    SPB_LAUNCH_VECTORS(dnb_csr_fill_kernel, m.nrow, s->stream, in, m.nrow, m.ncol, (const uint32_t *)ptr, indptr, indices, values);
    m.indptr = indptr; m.indices = indices; m.values = values;
    build_samplers_sparse_input(s, m);
}

// What session_create refuses its arguments for before the GPU is touched (empty: nothing), the checks in their order: the first that
// fails is reported.  nrow x ncol: the input's shape, whatever form it has.
static std::string session_args_refusal(const float *data, uint32_t nrow, uint32_t ncol, const cogaps_params *params, const cogaps_sparse_matrix *sp,
                                        const cogaps_coo_matrix *coo, const cogaps_device_matrix *dm)
{
    if (!params) return "null argument";
    const cogaps_params &p = *params;
    if (sp) {
        if (!p.useSparseOptimization) return "a compressed-sparse matrix needs useSparseOptimization = 1 (the dense model takes a dense matrix)";
        if (p.subsetData) return "subsetData is not supported with a compressed-sparse matrix: pass the rows / columns of the subset";
        if (p.reductionMode == COGAPS_REDUCE_SEQ) return "reductionMode COGAPS_REDUCE_SEQ is not supported with a compressed-sparse matrix";
    } else if (coo) {
        if (!p.useSparseOptimization) return "a triplet matrix needs useSparseOptimization = 1 (the dense model takes a dense matrix)";
        if (p.subsetData) return "subsetData is not supported with a triplet matrix: pass the entries of the subset";
        if (p.reductionMode == COGAPS_REDUCE_SEQ) return "reductionMode COGAPS_REDUCE_SEQ is not supported with a triplet matrix";
    } else if (dm) {
        if (!p.useSparseOptimization) return "a device-resident matrix needs useSparseOptimization = 1 (the dense model takes a dense matrix)";
        if (p.device != dm->device) return "params->device must be -1 or the device the matrix resides on (" + std::to_string(dm->device) + ")";
    } else if (!data) return "null argument: data";
    if (const char *refusal = sparse_args_refusal(sp, coo)) return refusal;
    // The reference's distributed caller forces asynchronousUpdates = FALSE on its workers (R/DistributedCogaps.R:28-29) -- there to keep
    // BiocParallel workers single-threaded, not for the sampler's sake.  Documented deviation: a
    // distributed worker call (runningDistributed, i.e. subsetDim > 0 in cogaps_cpp, Cogaps.cpp:82) runs the asynchronous sampler anyway,
    // so that GWCoGAPS / scCoGAPS through the real R package reach this library.  Everywhere else FALSE is refused.
    if (!p.asynchronousUpdates && !p.runningDistributed) return "asynchronousUpdates=FALSE (SingleThreadedGibbsSampler) is not part of this library";
    // The sequential sampler (seq_kernel.h) is chosen by `sampler` alone: asynchronousUpdates keeps the meaning above.
    if (p.sampler != COGAPS_SAMPLER_ASYNC && p.sampler != COGAPS_SAMPLER_SEQUENTIAL) return "sampler must be COGAPS_SAMPLER_ASYNC or COGAPS_SAMPLER_SEQUENTIAL";
    if (p.sampler == COGAPS_SAMPLER_SEQUENTIAL && p.useSparseOptimization)
        return "sampler = COGAPS_SAMPLER_SEQUENTIAL supports the dense model only: the SparseNormalModel evaluation of the sequential kernel is missing "
               "(useSparseOptimization must be 0)";
    if (p.nPatterns == 0 || nrow == 0 || ncol == 0) return "empty problem";
    if (p.whichMatrixFixed != 'N' && p.whichMatrixFixed != 'A' && p.whichMatrixFixed != 'P') return "whichMatrixFixed must be 'N', 'A' or 'P'";
    if (p.reductionMode != COGAPS_REDUCE_LANES && p.reductionMode != COGAPS_REDUCE_SEQ) return "reductionMode must be COGAPS_REDUCE_LANES or COGAPS_REDUCE_SEQ";
    if (p.mathMode < COGAPS_MATH_PORTABLE || p.mathMode > COGAPS_MATH_GLIBC_SSE2) return "mathMode must be COGAPS_MATH_PORTABLE, _GLIBC_FMA or _GLIBC_SSE2";
    if (p.mathMode != COGAPS_MATH_PORTABLE && p.reductionMode != COGAPS_REDUCE_SEQ)
        return "mathMode other than COGAPS_MATH_PORTABLE needs reductionMode COGAPS_REDUCE_SEQ (the verification mode)";
    if (p.pumpThreshold != 0 && p.pumpThreshold != 1) return "pumpThreshold must be 0 (PUMP_UNIQUE) or 1 (PUMP_CUT)";
    if (p.whichMatrixFixed != 'N' && p.fixedCols != 0 && (uint32_t)p.fixedCols != p.nPatterns) return "fixedPatterns must have nPatterns columns";
    if (p.subsetData && p.dataIndicesSubset) {
        if (p.nSubset == 0) return "dataIndicesSubset is empty";
        const uint32_t dim = orientation(p, p.nSubset, nrow, ncol).dim;      // 1-based indices into the subset's input axis (Matrix.cpp:55-62)
        for (uint32_t i = 0; i < p.nSubset; ++i)
            if (p.dataIndicesSubset[i] < 1u || p.dataIndicesSubset[i] > dim) return "dataIndicesSubset holds an index outside 1 .. " + std::to_string(dim);
    }
    return std::string();
}
