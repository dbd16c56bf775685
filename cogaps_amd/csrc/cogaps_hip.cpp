// cogaps_hip.cpp -- host side of libcogaps_hip.so: the runner around the HIP kernels and the C ABI
// of include/cogaps_hip.h.  Restates runCoGAPSAlgorithm / runOnePhase / updateSampler
// (reference src/GapsRunner.cpp:382-499, :272-327, :201-222), GapsStatistics (GapsStatistics.h/.cpp)
// and the DenseNormalModel constructor (gibbs_sampler/DenseNormalModel.h:66-88) with every matrix,
// the atomic domains and the proposal queues resident in HBM.  The host only draws the per-iteration
// Poisson step counts (GapsRunner.cpp:294-295), streams the Xoroshiro seed sequence the proposal
// generator consumes (math/Random.cpp:221-248) and enqueues kernels.
#include <atomic>
#include "../../include/cogaps_hip.h"
#include "rt.h"
#include "gaps_state.h"
#include "gen_kernel.h"
#include "file_reader.h"
#include "eval_kernel.h"
#include "chain_kernel.h"
#include "seq_kernel.h"
#include "aux_kernels.h"
#include "sparse_kernels.h"
#include "sparse_build.h"
#include "dense_build.h"
#include "state_digest.h"
#include "state_file.h"
#include "geneset_kernel.h"
#include "genemember_kernel.h"
#include "markers_kernel.h"
#include "gsea_kernel.h"
#include "residual_kernel.h"
#include "consensus_kernel.h"
#include "manova_kernel.h"
#include "project_kernel.h"

#include <math.h>
#include <cmath>
#include <stdio.h>
#include <time.h>
#include <algorithm>
#include <type_traits>
#include <vector>

#ifndef GEN_WIN
#define GEN_WIN 256
#endif
// A sampler whose batches are short takes half the window: every wave with live lanes costs a generator launch 0.4-0.9 us, a second
// round of a batch that outgrows the window ~3.5 us (profiles/r02_ab_generator_window.txt: the headline shape's P sampler, ~94 attempts
// per batch, is 0.75 us per launch faster with 128 lanes; its A sampler, ~157, needs the 256).  Any window gives the same batches.
#ifndef GEN_WIN_HALF
#define GEN_WIN_HALF (GEN_WIN / 2 >= 64 ? GEN_WIN / 2 : GEN_WIN)      // the narrower instantiation, for a sampler with short batches
#endif
// A third, WIDER window for the sparse model's chained launch (round 6): there the generator workgroup's window drawn ahead and its hand-over
// disappear behind the evaluation, which is long, and a second round of the batch costs ~12 us -- with the widest window the launch's workgroup
// holds (seven attempt waves + the helper wave: 448 attempts; the attempt lanes carry out the queue behind the helper wave's 64 slots) a batch of
// ~250 proposals (BASELINE configs[4]'s shard shape: 34 % of the A sampler's launches took two rounds) nearly always ends in its first round:
// A 33.9 -> 31.5 us per launch at 384 attempts, 30.9 at 448: 6.24 -> 6.55 -> 6.65 M proposals/s (profiles/r06_ab_sparse_chained_launch.txt).
// The dense chain pays for every further attempt wave in every launch (profiles/r06_ab_windows_320_384.txt) and keeps two windows.  Only the
// chained sparse launch is instantiated at this window: a sampler that steps by two launches per batch goes back to GEN_WIN first (the window
// is free to change between batches: results do not depend on it).
#ifndef GEN_WIN_WIDE
#define GEN_WIN_WIDE (GEN_WIN == 256 ? GEN_CHAIN_THREADS - 64 : GEN_WIN)
#endif
static uint32_t gen_window_for(uint32_t current, float stepsPerBatch, bool wideOk = false)
{
    if (GEN_WIN_WIDE != GEN_WIN) {
        if (current == (uint32_t)GEN_WIN_WIDE) return (wideOk && (stepsPerBatch <= 1.f || stepsPerBatch > 0.75f * (float)GEN_WIN)) ? current : (uint32_t)GEN_WIN;
        if (wideOk && current == (uint32_t)GEN_WIN && stepsPerBatch > 0.9f * (float)GEN_WIN) return (uint32_t)GEN_WIN_WIDE;
    }
    if (GEN_WIN_HALF == GEN_WIN || stepsPerBatch <= 1.f) return current;
    if (current == (uint32_t)GEN_WIN && stepsPerBatch < 0.85f * (float)GEN_WIN_HALF) return (uint32_t)GEN_WIN_HALF;
    if (current == (uint32_t)GEN_WIN_HALF && stepsPerBatch > 0.95f * (float)GEN_WIN_HALF) return (uint32_t)GEN_WIN;
    return current;
}


static thread_local std::string g_last_error;
static thread_local int g_last_code = COGAPS_OK;
static int fail(const std::string &m, int code = COGAPS_ERR_GENERIC) { g_last_error = m; g_last_code = code; return 1; }
// a caught exception: device memory exhausted and host memory exhausted keep their own codes (cogaps_last_error_code)
static int fail_exc(const std::exception &e)
{
    if (dynamic_cast<const rt_out_of_memory *>(&e)) return fail(e.what(), COGAPS_ERR_OUT_OF_DEVICE_MEMORY);
    if (dynamic_cast<const std::bad_alloc *>(&e)) return fail(e.what(), COGAPS_ERR_OUT_OF_HOST_MEMORY);
    return fail(e.what());
}

// ------------------------------------------------------------------------------------------------
// host RNG pieces: Xoroshiro128+ seeder (Random.cpp:221-248) and the runner's PCG (GapsRunner.cpp:437)
// ------------------------------------------------------------------------------------------------
struct HostSeeder {
    uint64_t s0, s1;
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    uint64_t next()
    {
        const uint64_t a = s0; uint64_t b = s1; const uint64_t r = a + b;
        b ^= a; s0 = rotl(a, 24) ^ b ^ (b << 16); s1 = rotl(b, 37);
        return r;
    }
    void init(uint64_t seed) { s0 = seed | 1; s1 = seed | 1; for (int i = 0; i < 5000; ++i) next(); }
};

// Random.cpp:125-170 (host double math, as in the reference; gaps::lgamma = libm lgamma here)
static int host_poisson(uint64_t &st, double lambda)
{
    auto unifd = [&]() { return (double)pcg_u32(st) / 4294967295.0; };
    if (lambda <= 5.0) {
        int x = 0; double p = unifd(); const double cutoff = exp(-lambda);
        while (p >= cutoff) { p *= unifd(); ++x; }
        return x;
    }
    const double c = 0.767 - 3.36 / lambda;
    const double beta = 3.1415926535897932384626433832795 / sqrt(3.0 * lambda);
    const double alpha = beta * lambda;
    const double k = log(c) - lambda - log(beta);
    for (;;) {
        const double u = unifd();
        const double x = (alpha - log((1.0 - u) / u)) / beta;
        const double n = floor(x + 0.5);
        if (n < 0.0) continue;
        const double v = unifd();
        const double y = alpha - beta * x;
        const double w = 1.0 + exp(y);
        const double lhs = y + log(v / (w * w));
        const double rhs = k + n * log(lambda) - lgamma(n + 1);
        if (lhs <= rhs) return (int)n;
    }
}

// ------------------------------------------------------------------------------------------------
// lookup tables (Random.cpp:269-295 over Math.cpp:43-81): float argument, double-precision normal /
// gamma(2,1) cdf and quantile, rounded to float.  Boost.Math in the reference; libm + Newton here.
// ------------------------------------------------------------------------------------------------
static double lut_erfc_inv(double y)
{
    if (y == 1.0) return 0.0;
    double lo = -6.0, hi = 6.0;
    for (int i = 0; i < 60; ++i) { const double mid = 0.5 * (lo + hi); if (erfc(mid) > y) lo = mid; else hi = mid; }
    double x = 0.5 * (lo + hi);
    for (int i = 0; i < 4; ++i) {
        const double f = erfc(x) - y, fp = -2.0 / sqrt(3.1415926535897932384626433832795) * exp(-x * x), fpp = -2.0 * x * fp;
        const double dx = f / fp;
        x -= dx / (1.0 - 0.5 * dx * fpp / fp);
    }
    return x;
}
static double lut_gamma2_cdf(double x)
{
    if (x < 0.5) { double sum = 0.0, xk = x * x, fact = 2.0; for (int k = 2; k < 40; ++k) { const double t = xk * (double)(k - 1) / fact; sum += (k & 1) ? -t : t; xk *= x; fact *= (double)(k + 1); } return sum; }
    return 1.0 - exp(-x) * (1.0 + x);
}
static double lut_gamma2_quantile(double p)
{
    double lo = 0.0, hi = 60.0;
    for (int i = 0; i < 80; ++i) { const double mid = 0.5 * (lo + hi); if (lut_gamma2_cdf(mid) < p) lo = mid; else hi = mid; }
    double x = 0.5 * (lo + hi);
    for (int i = 0; i < 3; ++i) { const double f = lut_gamma2_cdf(x) - p, fp = x * exp(-x); if (fp > 0) x -= f / fp; }
    return x;
}
static void build_luts(std::vector<float> &e, std::vector<float> &ei, std::vector<float> &qg)
{
    e.resize(GAPS_ERF_N); ei.resize(GAPS_ERFINV_N); qg.resize(GAPS_QGAMMA_N);
    auto pnorm = [](float p) { return (float)(0.5 * erfc(-(double)p / 1.41421356237309504880)); };
    auto qnorm = [](float q) { double r = lut_erfc_inv(2.0 * (double)q); r = -r; r *= 1.41421356237309504880; return (float)(r + 0.0); };
    auto qgam = [](float q) { if (q < 0.000001f) return 0.f; return (float)lut_gamma2_quantile((double)q); };
    for (unsigned i = 0; i < GAPS_ERF_N; ++i) { const float x = (float)i / 1000.f; e[i] = 2.f * pnorm(x * GAPS_SQRT2F) - 1.f; }
    for (unsigned i = 0; i < GAPS_ERFINV_N - 1; ++i) { const float x = (float)i / (float)(GAPS_ERFINV_N - 1); ei[i] = qnorm((1.f + x) / 2.f) / GAPS_SQRT2F; }
    ei[GAPS_ERFINV_N - 1] = qnorm(1.9998f / 2.f) / GAPS_SQRT2F;
    qg[0] = 0.f;
    for (unsigned i = 1; i < GAPS_QGAMMA_N - 1; ++i) { const float x = (float)i / (float)(GAPS_QGAMMA_N - 1); qg[i] = qgam(x); }
    qg[GAPS_QGAMMA_N - 1] = qgam(0.9998f);
}

// Virtual lanes of the row reductions: one float4 chunk per lane while the vector has at most 16384 chunks
// (eval_kernel.h).  Workgroups have min(W, 1024) threads.
extern "C" uint32_t cogaps_reduction_width(uint32_t N)
{
    uint32_t need = (N + 3u) / 4u, w = 64;
    while (w < need && w < 16384u) w <<= 1;
    return w;
}
// threads (= virtual lanes) of the sparse evaluation: one per 64-bit flag word of a data vector, 64..256 (sparse_kernels.h)
extern "C" uint32_t cogaps_sparse_width(uint32_t N)
{
    uint32_t need = N / 64u + 1u, w = 64;
    while (w < need && w < 256u) w <<= 1;
    return w;
}
// launch a kernel template<int V> with V = W / threads virtual lanes per thread
#define LAUNCH_V(KERNEL, W, grid, stream, ...) do { const uint32_t bs_ = (W) < 1024u ? (W) : 1024u; \
    switch ((W) / bs_) { case 1: RT_LAUNCH(KERNEL<1>, grid, bs_, stream, __VA_ARGS__); break; case 2: RT_LAUNCH(KERNEL<2>, grid, bs_, stream, __VA_ARGS__); break; \
                         case 4: RT_LAUNCH(KERNEL<4>, grid, bs_, stream, __VA_ARGS__); break; case 8: RT_LAUNCH(KERNEL<8>, grid, bs_, stream, __VA_ARGS__); break; \
                         default: RT_LAUNCH(KERNEL<16>, grid, bs_, stream, __VA_ARGS__); break; } } while (0)

// Switches that change what is MEASURED and never a result (launch sizes, the two-launch split form, reading S instead of recomputing it)
// exist in development builds only (-DCOGAPS_DEV, -DGEN_PROFILE): the product library does not look at them.  What the product library
// does read from the environment, on purpose, is documented in include/cogaps_hip.h: COGAPS_NO_GRAPH (every launch as a plain call --
// counter collection hangs on replayed graphs), COGAPS_NO_CHAIN (two launches per batch: the A/B and the equality test of the chained launch) and
// COGAPS_FORCE_CHAIN (tests: the chained launch on a device with fewer compute units than the launch has workgroups), COGAPS_CHAIN_SPLIT (the
// split evaluation inside the chained launch: measured, not the default).
static const char *dev_env(const char *name)
{
#if defined(COGAPS_DEV) || defined(GEN_PROFILE) || defined(COGAPS_EMUL)
    return getenv(name);
#else
    (void)name; return nullptr;
#endif
}
static const uint32_t SEQ_SPARSE_GRID = 256;      // workgroups of the sparse model's verification-mode evaluation (one scratch region each)

// Calls f(std::integral_constant<int, WIN>()) for the generator window `win`: the library's instantiations are GEN_WIN, GEN_WIN_HALF and,
// for the sparse model's chained launch only (Wide), GEN_WIN_WIDE.
template <bool Wide = false, class F> static void by_window(uint32_t win, F &&f)
{
    if constexpr (Wide && GEN_WIN_WIDE != GEN_WIN) if (win == (uint32_t)GEN_WIN_WIDE) return f(std::integral_constant<int, GEN_WIN_WIDE>());
    if (win == (uint32_t)GEN_WIN) f(std::integral_constant<int, GEN_WIN>()); else f(std::integral_constant<int, GEN_WIN_HALF>());
}

// HIP-event timing of a sample of the launches: the start / stop events are attached to the kernel's own dispatch packet
// (hipExtLaunchKernelGGL), so their difference is the dispatch's begin-to-end time, the figure rocprofv3 --kernel-trace reports; no extra
// packets enter the stream.  Events are resolved after the chunk's synchronisation so that timing never stalls the queue.
struct HostSampler;
enum EvKind { EV_GEN, EV_EVAL, EV_EVAL2, EV_SYNC };      // generator launch, evaluation launch, second kernel of a split evaluation (the first's sample), sync launch
struct EvSample { int kind; HostSampler *owner; uint64_t ord; };      // (owner, ord: a one-chain session's sampler and the batch step the launch belongs to)
struct EventPool {
    std::vector<rt_event_pair> ev; std::vector<EvSample> rec; size_t used = 0;
    void create(size_t n) { if (ev.empty()) { ev.resize(n); rec.resize(n); for (auto &e : ev) rt_event_create(e); } }
    ~EventPool() { for (auto &e : ev) rt_event_destroy(e); }
    bool room(size_t n) const { return used + n <= ev.size(); }
    int take(int kind, HostSampler *owner = nullptr, uint64_t ord = 0) { if (!room(1)) return -1; rec[used] = {kind, owner, ord}; return (int)used++; }
    template <class F> void drain(F f) { for (size_t i = 0; i < used; ++i) f(rec[i], rt_event_ms(ev[i])); used = 0; }
};
#define LAUNCH_MAYBE_TIMED(stream, pool, slot, KERNEL, grid, block, ...) do { if ((slot) >= 0) RT_LAUNCH_TIMED(KERNEL, grid, block, stream, (pool).ev[slot], __VA_ARGS__); \
    else RT_LAUNCH(KERNEL, grid, block, stream, __VA_ARGS__); } while (0)

// A dependent kernel pair costs ~3.5 us per launch on the host and leaves a ~5 us bubble on the GPU when it is
// launched call by call; replayed from a captured graph the same pair leaves ~1.6 us per kernel boundary.
static const uint32_t GRAPH_PAIRS = 64;
static_assert(GRAPH_PAIRS % 2u == 0u, "a replay must leave the chained launch's parity as it found it");
// The captured runs of GRAPH_PAIRS batch steps of a one-chain sampler or of one side of a batch: the two-launch form, and the chained form
// once per starting parity (consecutive chained launches alternate the parity they carry as a kernel argument).  A one-chain sampler's
// kernels take their state through SamplerDev, so its graphs serve while the record they were captured with (`key`, rekey) stays the
// sampler's; a batch's kernels take the address of its records' array, and its graphs are not keyed.
struct GraphCache {
    rt_graph pair, chain[2]; bool pairValid = false, chainValid[2] = {false, false};
    SamplerDev key{};
    void drop() { rt_graph_destroy(pair); rt_graph_destroy(chain[0]); rt_graph_destroy(chain[1]); pairValid = chainValid[0] = chainValid[1] = false; }
    void rekey(const SamplerDev &d) { if (memcmp(&key, &d, sizeof(SamplerDev)) != 0) { drop(); memcpy(&key, &d, sizeof(SamplerDev)); } }
    // replays the run of the given form (chained: the one starting at `parity`), captured first from GRAPH_PAIRS calls of `step` if it is
    // missing (the caller undoes what the captured calls did to its launch counters)
    template <class Step> void replay(rt_stream_t stream, bool chained, uint32_t parity, Step step)
    {
        rt_graph &g = chained ? chain[parity] : pair; bool &valid = chained ? chainValid[parity] : pairValid;
        if (!valid) { rt_capture_begin(stream); for (uint32_t b = 0; b < GRAPH_PAIRS; ++b) step(); rt_capture_end(stream, g); valid = true; }
        rt_graph_launch(g, stream);
    }
};

// ------------------------------------------------------------------------------------------------
struct HostSampler {
    SamplerDev d;                 // device pointers + constants (passed by value to the kernels)
    float *Sraw = nullptr;        // un-squared uncertainty [M][Npad] (chiSq); the dense model only
    uint64_t *seeds = nullptr; size_t seedCap = 0;
    uint64_t *hSeeds = nullptr; size_t hSeedCap = 0;
    float *partial = nullptr;     // [M] chi2 partials
    uint32_t nAtoms = 0;          // host copy after the last update
    float avgQueue = 0.f;
    float dataSparsity = 0.f;     // DenseNormalModel::dataSparsity
    SamplerDev *dRecord = nullptr; SamplerDev recordHeld;   // `d` in device memory (the generator reads it through a pointer) and what that copy holds
    bool recordValid = false;
    float stepsPerBatch = 0.f;    // proposals per batch in the last update (chunk-size predictor)
    uint32_t genWin = GEN_WIN;    // lanes of the generator launch (gen_window_for)
    float anneal = 1.f;           // annealing temperature of the next update
    GraphCache graphs;
    // chained launch (chain_kernel.h): one launch per batch; consecutive launches alternate the parity they carry as a kernel argument
    bool chain = false; uint32_t chainParity = 0;
    uint32_t chainParityStart = 0;      // parity of the current update's first chained launch (which copy a given launch of the update evaluated)
    bool chainOff = false; uint32_t chainRecoveries = 0;      // a hand-over inside a chained launch never arrived: the batch was completed by chain_recover, the sampler keeps two launches per batch from then on
    unsigned long long *chainGrans = nullptr;      // [queueCap][CHAIN_GRAN_STRIDE] the decisions' granules (the split form's per-slice totals keep SamplerDev::grans)
    size_t traceCap = 0;
    char name = 'A';
    // perf accounting
    uint64_t evalLaunches = 0, genLaunches = 0, batches = 0;
    // HIP-event samples, split into launches that processed a batch and launches past the end of an update
    double evalMs = 0, genMs = 0, evalNoopMs = 0, genNoopMs = 0; uint64_t evalTimed = 0, genTimed = 0, evalNoopTimed = 0, genNoopTimed = 0;
    uint64_t updLaunches = 0;    // (generator, evaluation) pairs enqueued in the current update
    uint64_t batchesAtTimingOn = 0;   // `batches` when event timing was switched on: the sampled times are scaled to the batches since then
    uint64_t plainRotor = 0;     // which graph replay of a chunk runs as plain, event-carrying launches while timing is on
    // launch clock of the chained launches (gaps_state.h): durations in 0.1 us bins since timing was switched on, their sum and count
    std::vector<unsigned long long> clockHost; uint64_t clockSeen = 0; std::vector<uint64_t> clockHist; double clockSumUs = 0; uint64_t clockN = 0;
    // ... and the launch-to-launch PERIOD (entry of one launch's first workgroup to the next launch's): the launch with everything the
    // dispatcher does around it -- what rocprofv3's dispatch duration plus the idle gap adds up to
    std::vector<uint64_t> periodHist; double periodSumUs = 0; uint64_t periodN = 0;
};

struct cogaps_session {
    double startTime = 0.0;                                          // gaps::run's startTime (GapsRunner.cpp:383): status lines, totalRunningTime
    float *pump = nullptr; uint32_t pumpUpdates = 0;                 // mPumpMatrix [nGenes][K] row-major (device), mPumpUpdates
    std::vector<float> snapA[2], snapP[2]; uint32_t nSnap[2] = {0, 0};   // [0] equilibration, [1] sampling snapshots, row-major

    cogaps_params p;
    std::vector<uint32_t> subset; std::vector<float> fixed;
    uint32_t nGenes = 0, nSamples = 0, K = 0;
    HostSampler A, P;
    HostSeeder seeder; uint64_t runnerRng = 0;
    // The seeder's output sequence does not depend on how it is consumed (update k takes the next nSteps values, Random.cpp:221-248), so it
    // is produced AHEAD of its use while the host waits for the GPU: seed_take() pops, seed_top_up() refills between launch and sync.
    std::vector<uint64_t> seedFifo; size_t seedHead = 0;
    rt_stream_t stream; bool ownsStream = true;      // a session that joined a cogaps_batch runs on the batch's stream
    float *dErf = nullptr, *dErfinv = nullptr, *dQgamma = nullptr; uint64_t *dLcgMul = nullptr, *dLcgInc = nullptr;
    float *Asum = nullptr, *Asq = nullptr, *Psum = nullptr, *Psq = nullptr;
    unsigned statUpdates = 0;
    std::vector<float> chisqHist; std::vector<uint32_t> atomHistA, atomHistP;
    uint64_t totalUpdates = 0; double samplerSeconds = 0; double syncMs = 0; uint64_t syncTimed = 0, syncBytes = 0;
    bool timing = false;
    bool noGraph = getenv("COGAPS_NO_GRAPH") != nullptr;     // diagnostics: every launch as a plain call (counter collection tools)
    bool noChain = getenv("COGAPS_NO_CHAIN") != nullptr;     // A/B and tests: two launches per batch (gen_kernel, eval_kernel<EVAL_FUSED>) where the chained launch would serve
    // The split evaluation inside the chained launch (EVAL_CHAIN_SPLIT) is built, tested on the hardware and NOT the default: measured on the
    // headline chain it loses 6 % (profiles/r05_ab_chained_split_evaluation_not_kept.txt -- the launch's workgroups carry the generator's 142 KB
    // of LDS, so one evaluation workgroup fits a compute unit and each takes 3-4 slices one after the other, where the two-launch form has
    // two per unit and all slices resident).  COGAPS_CHAIN_SPLIT=1 takes it (the A/B, the equality test).
    bool noChainSplit = getenv("COGAPS_CHAIN_SPLIT") == nullptr;
    bool testWideWindow = getenv("COGAPS_TEST_WIDE_WINDOW") != nullptr;      // tests: the sparse model's chained launch at GEN_WIN_WIDE from the first update on (otherwise once batches exceed 0.9 * GEN_WIN)
    bool forceChain = getenv("COGAPS_FORCE_CHAIN") != nullptr;      // tests: the chained launch also where the device shows fewer compute units than the launch has workgroups (they then run in turns, the generator last)
    unsigned computeUnits = 0;      // of the session's device: the chained launch wants all its workgroups resident at once, one per compute unit
    EventPool ev;
    GenScalars *hGs = nullptr;    // pinned staging
    std::atomic<uint64_t> deviceBytes{0};      // device memory the session holds (rt_owner_scope; cogaps_session_device_bytes)
    float orderedSumMs = 0.f;     // ... and what the ordered sums of the packed values took at its creation (HIP events)
    bool poisoned = false;        // a device error ended an update half way (capacity, a hand-over inside a launch that never arrived): the chain's state is not a state of the chain
    // where the run stands (cogaps_session_position): the phase and its next iteration, advanced by cogaps_session_run_iterations and
    // cogaps_batch_run_iterations; phase 3 = both phases complete
    int posPhase = 1; uint32_t posNext = 0;
    // state-file fingerprint (session_state.h): a hash of fixedPatterns, taken at creation (the caller's array is not kept), and
    // the data digest, computed on the device at the first save or load
    uint64_t fixedHash = 0, dataDigest = 0; bool digestValid = false;
};

static double now_s() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

template <class T> static T *dalloc(size_t n) { return (T *)rt_malloc(n * sizeof(T)); }

// building a session's samplers from every form of input, at its place among the chapters: the kernels keep their order of first use
#include "session_build.h"

#include "sampler_update.h"

static void do_sync(cogaps_session *s, HostSampler &dst, HostSampler &src)
{
    if (dst.d.sparse) {     // SparseNormalModel::sync = generateLookupTables (SparseNormalModel.cpp:27-31, 294-311)
        const uint32_t K = dst.d.K;
        if (dst.d.seq) RT_LAUNCH(sparse_tables_seq_kernel, K + K * (K + 1u) / 2u, 256, s->stream, dst.d);
        else LAUNCH_V(sparse_tables_kernel, dst.d.redW, K + K * (K + 1u) / 2u, s->stream, dst.d);
        return;
    }
    const uint32_t tilesX = (src.d.N + TR_TILE - 1) / TR_TILE, tilesY = (src.d.M + TR_TILE - 1) / TR_TILE;
    const int slot = timing_slot(s, dst, EV_SYNC, 0);
    if (slot >= 0) s->syncBytes += 8ull * src.d.M * src.d.N;         // algorithmic traffic of a sync: M x N floats read and written
    LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, transpose_kernel, tilesX * tilesY, 256, (const float *)src.d.AP, dst.d.AP, src.d.M, src.d.N, src.d.Npad, dst.d.Npad, tilesX);
}

// the M per-vector partial sums a chi-square launch left, added on the host: one float accumulator, ascending j
static float sum_partials(cogaps_session *s, const float *partial, uint32_t M)
{
    std::vector<float> part(M);
    rt_d2h(part.data(), partial, (size_t)M * 4, s->stream); rt_sync(s->stream);
    float c = 0.f; for (uint32_t j = 0; j < M; ++j) c += part[j];
    return c;
}

static float chisq_of(cogaps_session *s, HostSampler &h)
{
    if (h.d.seq) {      // the reference's order: one accumulator over the whole matrix, on the device
        if (h.d.sparse) RT_LAUNCH(chisq_sparse_seq_kernel, 1, 256, s->stream, h.d, h.partial);
        else RT_LAUNCH(chisq_seq_kernel, 1, 256, s->stream, h.d, (const float *)h.Sraw, h.partial);
        float c = 0.f;
        rt_d2h(&c, h.partial, 4, s->stream); rt_sync(s->stream);
        return h.d.sparse ? c * h.d.beta : c;
    }
    if (h.d.sparse && h.d.K <= 64u) LAUNCH_V(chisq_sparse_tiled_kernel, h.d.redW, (h.d.M + (uint32_t)SP_CHI_ROWS - 1u) / (uint32_t)SP_CHI_ROWS, s->stream, h.d, h.partial);      // SP_CHI_ROWS vectors per workgroup share the other matrix's rows
    else if (h.d.sparse) LAUNCH_V(chisq_sparse_kernel, h.d.redW, h.d.M, s->stream, h.d, h.partial);
    else LAUNCH_V(chisq_rows_kernel_s, h.d.redW, h.d.M, s->stream, h.d, (const float *)h.Sraw, h.partial);
    const float c = sum_partials(s, h.partial, h.d.M);
    return h.d.sparse ? c * h.d.beta : c;
}

CG_KERNEL void debug_math_kernel(int fn, uint32_t mode, const float *x, float *y, uint32_t n)
{
    const uint32_t i = cg_bid() * cg_bdim() + cg_tid();
    if (i < n) y[i] = fn ? gm_expf_m(x[i], mode) : gm_logf_m(x[i], mode);
}

CG_KERNEL void debug_udiv64_kernel(const uint64_t *a, const uint64_t *b, uint64_t *q, uint32_t n)
{
    const uint32_t i = cg_bid() * cg_bdim() + cg_tid();
    if (i < n) q[i] = gm_udiv64(a[i], b[i]);
}

CG_KERNEL void debug_uniform64_kernel(const uint64_t *state, const uint64_t *lo, const uint64_t *hi, uint64_t *value, uint64_t *stateAfter, uint32_t n)
{
    const uint32_t i = cg_bid() * cg_bdim() + cg_tid();
    if (i < n) { uint64_t s = state[i]; value[i] = pcg_uniform64(s, lo[i], hi[i]); stateAfter[i] = s; }
}

extern "C" {

int cogaps_debug_math(int fn, int mathMode, const float *x, float *y, uint32_t n, int on_device)
{
    try {
        if (mathMode < COGAPS_MATH_PORTABLE || mathMode > COGAPS_MATH_GLIBC_SSE2 || (fn != 0 && fn != 1)) return fail("bad function or math mode");
        if (!on_device) { for (uint32_t i = 0; i < n; ++i) y[i] = fn ? gm_expf_m(x[i], (uint32_t)mathMode) : gm_logf_m(x[i], (uint32_t)mathMode); return 0; }
        rt_stream_t st = rt_stream_create();
        rt_alloc_scope allocOn(st);
        float *dx = dalloc<float>(n), *dy = dalloc<float>(n);
        rt_h2d(dx, x, (size_t)n * 4, st);
        RT_LAUNCH(debug_math_kernel, (n + 255u) / 256u, 256, st, fn, (uint32_t)mathMode, (const float *)dx, dy, n);
        rt_d2h(y, dy, (size_t)n * 4, st); rt_sync(st);
        rt_free(dx); rt_free(dy); rt_stream_destroy(st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

int cogaps_debug_udiv64(const uint64_t *a, const uint64_t *b, uint64_t *q, uint32_t n, int on_device)
{
    try {
        if (!a || !b || !q) return fail("null argument");
        for (uint32_t i = 0; i < n; ++i) if (b[i] == 0ull) return fail("gm_udiv64 needs a divisor >= 1");
        if (!on_device) { for (uint32_t i = 0; i < n; ++i) q[i] = gm_udiv64(a[i], b[i]); return 0; }
        if (n == 0u) return 0;
        rt_stream_t st = rt_stream_create();
        rt_alloc_scope allocOn(st);
        uint64_t *da = dalloc<uint64_t>(n), *db = dalloc<uint64_t>(n), *dq = dalloc<uint64_t>(n);
        rt_h2d(da, a, (size_t)n * 8, st); rt_h2d(db, b, (size_t)n * 8, st);
        RT_LAUNCH(debug_udiv64_kernel, (n + 255u) / 256u, 256, st, (const uint64_t *)da, (const uint64_t *)db, dq, n);
        rt_d2h(q, dq, (size_t)n * 8, st); rt_sync(st);
        rt_free(da); rt_free(db); rt_free(dq); rt_stream_destroy(st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

int cogaps_debug_uniform64(const uint64_t *state, const uint64_t *lo, const uint64_t *hi, uint64_t *value, uint64_t *stateAfter, uint32_t n, int on_device)
{
    try {
        if (!state || !lo || !hi || !value || !stateAfter) return fail("null argument");
        // (a range of 0 values after the wrap would be divided by, and its rejection loop would never end)
        for (uint32_t i = 0; i < n; ++i) if (hi[i] < lo[i] || hi[i] + 1ull - lo[i] == 0ull) return fail("pcg_uniform64 needs lo <= hi and fewer than 2^64 values");
        if (!on_device) { for (uint32_t i = 0; i < n; ++i) { uint64_t s = state[i]; value[i] = pcg_uniform64(s, lo[i], hi[i]); stateAfter[i] = s; } return 0; }
        if (n == 0u) return 0;
        rt_stream_t st = rt_stream_create();
        rt_alloc_scope allocOn(st);
        uint64_t *ds = dalloc<uint64_t>(n), *dl = dalloc<uint64_t>(n), *dh = dalloc<uint64_t>(n), *dv = dalloc<uint64_t>(n), *dso = dalloc<uint64_t>(n);
        rt_h2d(ds, state, (size_t)n * 8, st); rt_h2d(dl, lo, (size_t)n * 8, st); rt_h2d(dh, hi, (size_t)n * 8, st);
        RT_LAUNCH(debug_uniform64_kernel, (n + 255u) / 256u, 256, st, (const uint64_t *)ds, (const uint64_t *)dl, (const uint64_t *)dh, dv, dso, n);
        rt_d2h(value, dv, (size_t)n * 8, st); rt_d2h(stateAfter, dso, (size_t)n * 8, st); rt_sync(st);
        rt_free(ds); rt_free(dl); rt_free(dh); rt_free(dv); rt_free(dso); rt_stream_destroy(st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

int cogaps_current_device(int *device)
{
    try { if (!device) return fail("null argument"); *device = rt_get_device(); return 0; } catch (const std::exception &e) { return fail_exc(e); }
}

int cogaps_device_memory(int device, uint64_t *freeBytes, uint64_t *totalBytes)
{
    try {
        if (!freeBytes || !totalBytes) return fail("null argument");
        const int before = rt_get_device();
        if (device >= 0) rt_set_device(device);
        size_t f = 0, t = 0; rt_mem_info(&f, &t);
        if (device >= 0) rt_set_device(before);
        *freeBytes = (uint64_t)f; *totalBytes = (uint64_t)t;
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

} // extern "C"

// the statistics of a finished run, at their place among the chapters: the kernels keep their order of first use
#include "result_stats.h"

extern "C" {

void cogaps_default_params(cogaps_params *p)
{
    memset(p, 0, sizeof(*p));
    p->nPatterns = 3; p->nIterations = 1000; p->maxThreads = 1; p->outputFrequency = 500;   // GapsParameters.h:79-111
    p->alphaA = 0.01f; p->alphaP = 0.01f; p->maxGibbsMassA = 100.f; p->maxGibbsMassP = 100.f;
    p->printMessages = 0; p->asynchronousUpdates = 1; p->whichMatrixFixed = 'N'; p->workerID = 1; p->device = -1;
    p->sampler = COGAPS_SAMPLER_ASYNC;
}
const char *cogaps_last_error(void) { return g_last_error.c_str(); }
int cogaps_last_error_code(void) { return g_last_code; }
#ifndef COGAPS_SOURCE_HASH
#define COGAPS_SOURCE_HASH "unknown"      // (builds that do not go through csrc/Makefile: the test-only emulator)
#endif
const char *cogaps_source_hash(void) { return COGAPS_SOURCE_HASH; }
const char *cogaps_build_report(void)
{
    static const std::string rep = std::string("cogaps-amd 0.2 | ") + CG_PLATFORM_NAME + " | asynchronous Gibbs sampler, dense and sparse normal model | checkpoints: no | sources " + COGAPS_SOURCE_HASH;
    return rep.c_str();
}
int cogaps_checkpoints_enabled(void) { return 0; }
int cogaps_compiled_with_openmp(void) { return 0; }

} // extern "C"

// cogaps_session_create (sp == coo == dm == nullptr: the dense matrix `data`), cogaps_session_create_sparse (sp: the compressed one),
// cogaps_session_create_coo (coo: unordered triplets) and cogaps_session_create_from_device_matrix (dm: a device-resident matrix)
static cogaps_session *session_create(const float *data, uint32_t nrow, uint32_t ncol, const cogaps_params *params, const float *unc, int data_on_device,
                                      const cogaps_sparse_matrix *sp, const cogaps_coo_matrix *coo = nullptr, const cogaps_device_matrix *dm = nullptr)
{
    cogaps_session *s = nullptr;
    try {
        if (sp) { nrow = sp->nrow; ncol = sp->ncol; } else if (coo) { nrow = coo->nrow; ncol = coo->ncol; } else if (dm) { nrow = dm->m.nrow; ncol = dm->m.ncol; }
        const std::string refusal = session_args_refusal(data, nrow, ncol, params, sp, coo, dm);      // (before the GPU is touched)
        if (!refusal.empty()) { fail(refusal); return nullptr; }
        const cogaps_params &p = *params;
        rt_set_device(p.device);
        s = new cogaps_session(); s->computeUnits = rt_compute_units();
        s->p = p;
        s->p.device = rt_get_device();            // (-1 resolved: later calls from other host threads select the same GPU)
        g_updatesRunning(s->p.device);            // (the counters exist before any session steps)
        s->startTime = now_s();
        if (p.printMessages) { printf("Loading Data..."); fflush(stdout); }                  // GapsRunner.cpp:399
        if (p.subsetData && p.dataIndicesSubset) s->subset.assign(p.dataIndicesSubset, p.dataIndicesSubset + p.nSubset);
        s->stream = rt_stream_create();
        rt_alloc_scope allocOn(s->stream); rt_owner_scope owner(&s->deviceBytes);
        s->hGs = (GenScalars *)rt_malloc_host(sizeof(GenScalars));
        // GapsRandomState(seed): seeder + lookup tables (Cogaps.cpp:158, Random.cpp:264-267)
        s->seeder.init(p.seed);
        std::vector<float> e, ei, qg; build_luts(e, ei, qg);
        s->dErf = dalloc<float>(e.size() + 8); s->dErfinv = dalloc<float>(ei.size() + 8); s->dQgamma = dalloc<float>(qg.size() + 8);      // (read as whole float4 chunks by the evaluation kernel's LDS staging)
        rt_h2d(s->dErf, e.data(), e.size() * 4, s->stream); rt_h2d(s->dErfinv, ei.data(), ei.size() * 4, s->stream); rt_h2d(s->dQgamma, qg.data(), qg.size() * 4, s->stream);
        std::vector<uint64_t> lm(2 * GEN_WIN_WIDE + 2), li(2 * GEN_WIN_WIDE + 2);      // (jumps of up to 2 * window steps; GEN_WIN_WIDE >= GEN_WIN)
        for (uint32_t k = 0; k < lm.size(); ++k) pcg_jump_coeffs(k, lm[k], li[k]);
        s->dLcgMul = dalloc<uint64_t>(lm.size()); s->dLcgInc = dalloc<uint64_t>(li.size());
        rt_h2d(s->dLcgMul, lm.data(), lm.size() * 8, s->stream); rt_h2d(s->dLcgInc, li.data(), li.size() * 8, s->stream);
        rt_sync(s->stream);
        // samplers: A on the transposed data with the subset flag flipped (GapsRunner.cpp:402-406);
        // seed order: A queue, P queue, runner (AsynchronousGibbsSampler.h:68, GapsRunner.cpp:437)
        if (sp) build_samplers_sparse_input(s, *sp);
        else if (coo) build_samplers_coo_input(s, *coo);
        else if (dm) build_samplers_device_matrix(s, dm->m, &s->subset);
        else if (data_on_device) {      // device-resident dense input (and uncertainty): built where it lies (dense_build.h)
            if (p.useSparseOptimization) build_samplers_dense_device_sparse(s, data, nrow, ncol); else build_samplers_dense_device(s, data, nrow, ncol, unc);
        } else if (p.useSparseOptimization) build_samplers_dense_input(s, data, nrow, ncol);      // (unc: the sparse model always assumes the default, SparseNormalModel.h:90-96)
        else {
            const Orientation o = orientation(s->p, s->subset.size(), nrow, ncol);
            for (int w = 0; w < 2; ++w) build_sampler(s, w, o, data, ncol, unc);
        }
        s->nGenes = s->A.d.M; s->nSamples = s->P.d.M; s->K = p.nPatterns;
        if (s->A.d.N != s->P.d.M || s->P.d.N != s->A.d.M) throw std::runtime_error("internal: sampler dimensions do not mirror");
        s->A.d.other = s->P.d.mat; s->A.d.otherColPos = s->P.d.colPos;
        s->P.d.other = s->A.d.mat; s->P.d.otherColPos = s->A.d.colPos;
        if (p.useSparseOptimization) {
            s->A.d.orows = s->P.d.rows; s->A.d.oflags = s->P.d.mflags; s->A.d.oMw = s->P.d.Mw; s->A.d.oKpad = s->P.d.Kpad;
            s->P.d.orows = s->A.d.rows; s->P.d.oflags = s->A.d.mflags; s->P.d.oMw = s->A.d.Mw; s->P.d.oKpad = s->A.d.Kpad;
        }
        // processFixedMatrix (GapsRunner.cpp:329-350)
        if (p.whichMatrixFixed != 'N') {
            HostSampler &f = (p.whichMatrixFixed == 'A') ? s->A : s->P;
            if (!p.fixedPatterns || p.fixedRows != f.d.M) throw std::runtime_error("fixedPatterns must have one row per row of the fixed matrix");
            s->fixedHash = cgstate::hash_bytes(p.fixedPatterns, (size_t)f.d.M * f.d.K * sizeof(float));
            std::vector<float> m((size_t)f.d.K * f.d.Mpad, 0.f);
            for (uint32_t r = 0; r < f.d.M; ++r) for (uint32_t k = 0; k < f.d.K; ++k) m[(size_t)k * f.d.Mpad + r] = p.fixedPatterns[(size_t)r * f.d.K + k];
            if (f.d.sparse) {
                // HybridMatrix::operator=(Matrix) (HybridMatrix.cpp:70-84): the row copy takes the value, the column copy
                // takes it through add(): entries below epsilon are held at zero and unflagged
                std::vector<float> rw((size_t)f.d.M * f.d.Kpad, 0.f); std::vector<unsigned long long> fl((size_t)f.d.K * f.d.Mw, 0ull); std::vector<uint32_t> cnt(f.d.K, 0u);
                for (uint32_t r = 0; r < f.d.M; ++r) for (uint32_t k = 0; k < f.d.K; ++k) {
                    const float v = p.fixedPatterns[(size_t)r * f.d.K + k];
                    rw[(size_t)r * f.d.Kpad + k] = v;
                    if (0.f + v < GAPS_EPSILON) m[(size_t)k * f.d.Mpad + r] = 0.f;
                    else { fl[(size_t)k * f.d.Mw + (r >> 6)] |= 1ull << (r & 63u); ++cnt[k]; }
                }
                rt_h2d(f.d.rows, rw.data(), rw.size() * 4, s->stream); rt_h2d(f.d.mflags, fl.data(), fl.size() * 8, s->stream); rt_h2d(f.d.colPos, cnt.data(), cnt.size() * 4, s->stream);
            }
            rt_h2d(f.d.mat, m.data(), m.size() * 4, s->stream); rt_sync(s->stream);
            if (!f.d.sparse) RT_LAUNCH(count_pos_kernel, f.d.K, 256, s->stream, f.d);
        }
        s->Asum = dalloc<float>((size_t)s->K * s->A.d.Mpad); s->Asq = dalloc<float>((size_t)s->K * s->A.d.Mpad);
        s->Psum = dalloc<float>((size_t)s->K * s->P.d.Mpad); s->Psq = dalloc<float>((size_t)s->K * s->P.d.Mpad);
        s->pump = dalloc<float>((size_t)s->nGenes * s->K);
        s->runnerRng = pcg_from_seed(s->seeder.next());
        // ASampler.sync(PSampler); PSampler.sync(ASampler); extraInitialization x2 (GapsRunner.cpp:444-447)
        if (p.useSparseOptimization) { do_sync(s, s->A, s->P); do_sync(s, s->P, s->A); }     // the lookup tables; extraInitialization is a no-op (SparseNormalModel.cpp:34-37)
        else if (p.whichMatrixFixed != 'N') {
            // (no fixed matrix: both factors are all zero and AP = 0 is what the allocation holds -- 0.11 s of multiplying zeros per
            // session at the headline shape otherwise)
            for (HostSampler *h : {&s->A, &s->P}) {
                const uint32_t tilesI = (h->d.N + 255u) / 256u, tilesJ = (h->d.M + (uint32_t)INIT_JT - 1u) / (uint32_t)INIT_JT;
                RT_LAUNCH(init_ap_kernel, tilesI * tilesJ, 256, s->stream, h->d, tilesI);
            }
        }
        rt_sync(s->stream);
        if (p.printMessages) {                                                   // GapsRunner.cpp:412-426
            const unsigned el = (unsigned)(now_s() - s->startTime);
            printf("Done! (%02u:%02u:%02u)\n", el / 3600u, (el % 3600u) / 60u, el % 60u);
            if (!p.useSparseOptimization && s->A.dataSparsity > 0.80f) printf("\nWarning: data is more than 80%% sparse and sparseOptimization is not enabled\n");
        }
        if (p.runningDistributed) printf("    worker %u is starting!\n", p.workerID);         // :428-433
        fflush(stdout);
        return s;
    } catch (const std::exception &e) {
        fail_exc(e);
        if (s) cogaps_session_destroy(s);
        return nullptr;
    }
}

extern "C" {

cogaps_session *cogaps_session_create(const float *data, uint32_t nrow, uint32_t ncol, const cogaps_params *params, const float *unc, int data_on_device)
{
    return session_create(data, nrow, ncol, params, unc, data_on_device, nullptr);
}
cogaps_session *cogaps_session_create_sparse(const cogaps_sparse_matrix *m, const cogaps_params *params)
{
    if (!m) { fail("null argument"); return nullptr; }
    return session_create(nullptr, 0, 0, params, nullptr, 0, m);
}
cogaps_session *cogaps_session_create_coo(const cogaps_coo_matrix *m, const cogaps_params *params)
{
    if (!m) { fail("null argument"); return nullptr; }
    return session_create(nullptr, 0, 0, params, nullptr, 0, nullptr, m);
}

static cogaps_device_matrix *device_matrix_create(const cogaps_sparse_matrix *sp, const cogaps_coo_matrix *coo, int device)
{
    cogaps_device_matrix *dm = nullptr;
    rt_stream_t stream; bool haveStream = false;
    try {
        if (const char *refusal = sparse_args_refusal(sp, coo)) { fail(refusal); return nullptr; }
        if ((sp ? sp->nrow : coo->nrow) == 0 || (sp ? sp->ncol : coo->ncol) == 0) { fail("empty problem"); return nullptr; }
        rt_set_device(device);
        dm = new cogaps_device_matrix();
        dm->device = rt_get_device(); dm->computeUnits = rt_compute_units();
        stream = rt_stream_create(); haveStream = true;
        {
            rt_alloc_scope allocOn(stream); rt_owner_scope owner(&dm->deviceBytes);
            if (sp) device_matrix_from_sparse(dm, *sp, stream); else device_matrix_from_coo(dm, *coo, stream);
            rt_sync(stream);
        }
        rt_stream_destroy(stream);
        return dm;
    } catch (const std::exception &e) {
        fail_exc(e);
        if (haveStream) rt_stream_destroy(stream);
        delete dm;
        return nullptr;
    }
}
cogaps_device_matrix *cogaps_device_matrix_create_sparse(const cogaps_sparse_matrix *m, int device)
{
    if (!m) { fail("null argument"); return nullptr; }
    return device_matrix_create(m, nullptr, device);
}
cogaps_device_matrix *cogaps_device_matrix_create_coo(const cogaps_coo_matrix *m, int device)
{
    if (!m) { fail("null argument"); return nullptr; }
    return device_matrix_create(nullptr, m, device);
}
void cogaps_device_matrix_destroy(cogaps_device_matrix *m)
{
    if (!m) return;
    try { rt_set_device(m->device); } catch (const std::exception &) { }
    delete m;
}
int cogaps_device_matrix_info(const cogaps_device_matrix *m, uint32_t *nrow, uint32_t *ncol, uint64_t *storedEntries, uint64_t *deviceBytes, int *device)
{
    if (!m) return fail("null argument");
    if (nrow) *nrow = m->m.nrow;
    if (ncol) *ncol = m->m.ncol;
    if (storedEntries) *storedEntries = m->m.nnz;
    if (deviceBytes) *deviceBytes = m->deviceBytes.load();
    if (device) *device = m->device;
    return 0;
}
cogaps_session *cogaps_session_create_from_device_matrix(const cogaps_device_matrix *m, const cogaps_params *params)
{
    if (!m || !params) { fail("null argument"); return nullptr; }
    cogaps_params p = *params;
    if (p.device == -1) p.device = m->device;
    return session_create(nullptr, 0, 0, &p, nullptr, 0, nullptr, nullptr, m);
}
int cogaps_session_device_bytes(cogaps_session *s, uint64_t *bytes)
{
    if (!s || !bytes) return fail("null argument");
    *bytes = s->deviceBytes.load();
    return 0;
}

int cogaps_session_sparse_build_ms(cogaps_session *s, float *orderedSumMs)
{
    if (!s || !orderedSumMs) return fail("null argument");
    *orderedSumMs = s->orderedSumMs;
    return 0;
}

void cogaps_session_destroy(cogaps_session *s)
{
    if (!s) return;
    s->A.graphs.drop(); s->P.graphs.drop();
    free_sampler(s->A); free_sampler(s->P);
    rt_free(s->dErf); rt_free(s->dErfinv); rt_free(s->dQgamma); rt_free(s->dLcgMul); rt_free(s->dLcgInc);
    rt_free(s->Asum); rt_free(s->Asq); rt_free(s->Psum); rt_free(s->Psq); rt_free(s->pump);
    rt_free_host(s->hGs);
    if (s->ownsStream) rt_stream_destroy(s->stream);
    delete s;
}

// (the HIP current device belongs to the calling host thread: a session used from another thread than its creator's selects its GPU again)
#define SESSION_TRY try { rt_set_device(s->p.device); rt_alloc_scope allocOn_(s->stream); rt_owner_scope owner_(&s->deviceBytes);      // allocations made on behalf of a session fill on its stream
#define SESSION_END } catch (const std::exception &e) { return fail_exc(e); } return 0;

static HostSampler &pick(cogaps_session *s, char w) { return w == 'A' ? s->A : s->P; }

int cogaps_session_set_annealing(cogaps_session *s, float temp) { s->A.anneal = temp; s->P.anneal = temp; return 0; }

int cogaps_session_draw_steps(cogaps_session *s, uint32_t *nA, uint32_t *nP)
{
    const unsigned a = std::max(s->A.nAtoms, 10u), b = std::max(s->P.nAtoms, 10u);
    *nA = (uint32_t)host_poisson(s->runnerRng, (double)a);
    *nP = (uint32_t)host_poisson(s->runnerRng, (double)b);
    return 0;
}

int cogaps_session_update(cogaps_session *s, char which, uint32_t nSteps, cogaps_trace_rec *trace, uint32_t traceCap, uint32_t *nTrace,
                          uint32_t *batchNproc, uint32_t *batchQlen, uint32_t batchCap, uint32_t *nBatches)
{
    SESSION_TRY
    HostSampler &h = pick(s, which);
    const bool tr = trace != nullptr && traceCap > 0;
    const uint32_t cap = tr ? std::max(traceCap, batchCap) : 0;
    if (run_update(s, h, nSteps, cap)) return 1;
    if (tr) {
        const uint32_t n = std::min(s->hGs->traceCount, cap), nb = std::min(s->hGs->traceBatchCount, cap);
        std::vector<PropRec> rec(n);
        if (n) rt_d2h(rec.data(), h.d.trace, (size_t)n * sizeof(PropRec), s->stream);
        std::vector<uint32_t> bn(nb), bq(nb);
        if (nb) { rt_d2h(bn.data(), h.d.traceBatchNproc, (size_t)nb * 4, s->stream); rt_d2h(bq.data(), h.d.traceBatchQlen, (size_t)nb * 4, s->stream); }
        rt_sync(s->stream);
        for (uint32_t i = 0; i < n && i < traceCap; ++i) {
            cogaps_trace_rec &o = trace[i]; const PropRec &r = rec[i];
            o.pos = r.pos; o.rng_state = r.rng; o.atom1 = r.i1; o.atom2 = r.i2; o.r1 = r.r1; o.c1 = r.c1; o.r2 = r.r2; o.c2 = r.c2; o.type = r.type; o.batch = r.batch;
        }
        for (uint32_t i = 0; i < nb && i < batchCap; ++i) { if (batchNproc) batchNproc[i] = bn[i]; if (batchQlen) batchQlen[i] = bq[i]; }
        if (nTrace) *nTrace = s->hGs->traceCount;
        if (nBatches) *nBatches = s->hGs->traceBatchCount;
    }
    SESSION_END
}

int cogaps_session_sync(cogaps_session *s, char which)
{
    SESSION_TRY
    if (which == 'A') do_sync(s, s->A, s->P); else do_sync(s, s->P, s->A);
    SESSION_END
}

// the part of an iteration after the two updates: the proposal counter and GapsStatistics::update* (GapsRunner.cpp:297-313)
static void iterate_tail(cogaps_session *s, uint32_t nA, uint32_t nP, int sampling)
{
    const char f = s->p.whichMatrixFixed;
    s->totalUpdates += (uint64_t)nA + nP;
    if (sampling) {
        const uint32_t mode = (f == 'N') ? 0u : (f == 'P' ? 1u : 2u);   // P fixed -> updateA ; A fixed -> updateP
        RT_LAUNCH(stats_kernel, s->K, 256, s->stream, s->A.d, s->P.d, s->Asum, s->Asq, s->Psum, s->Psq, mode);
        s->statUpdates++;
        if (f == 'N' && s->p.takePumpSamples) { RT_LAUNCH(pump_kernel, (s->A.d.M + 255u) / 256u, 256, s->stream, s->A.d, s->pump); s->pumpUpdates++; }   // GapsRunner.cpp:308-313
    }
}

// updateSampler (GapsRunner.cpp:201-222) + GapsStatistics::update* (GapsRunner.cpp:299-312)
int cogaps_session_iterate(cogaps_session *s, uint32_t nA, uint32_t nP, int sampling)
{
    SESSION_TRY
    const char f = s->p.whichMatrixFixed;
    if (f != 'A') { if (run_update(s, s->A, nA, 0)) return 1; if (f != 'P') do_sync(s, s->P, s->A); }
    if (f != 'P') { if (run_update(s, s->P, nP, 0)) return 1; if (f != 'A') do_sync(s, s->A, s->P); }
    iterate_tail(s, nA, nP, sampling);
    SESSION_END
}

// the head of one iteration of runOnePhase (GapsRunner.cpp:280-295): interrupt poll, annealing temperature, Poisson step counts
static int iteration_head(cogaps_session *s, int phase, uint32_t it, uint32_t *nA, uint32_t *nP)
{
    if (s->p.interrupt && s->p.interrupt(s->p.interruptArg)) return fail("interrupted");
    if (phase == 1) {
        const float temp = (float)(2 * it) / (float)s->p.nIterations;
        cogaps_session_set_annealing(s, gm_min(1.f, temp));
    }
    const int rc = cogaps_session_draw_steps(s, nA, nP);
#if defined(COGAPS_EMUL)
    // TEST-ONLY emulator build (never in the product library: a stray environment variable must not be able to change a chain):
    // COGAPS_TEST_ZERO_STEPS="<workerID>:<iteration>" turns that worker's A update of that equilibration iteration into update(0) -- what a
    // Poisson draw of 0 (probability e^-10 per draw while a chain holds at most ten atoms) does -- after the draw, so the generators'
    // sequences are unchanged
    if (phase == 1) if (const char *z = getenv("COGAPS_TEST_ZERO_STEPS")) { unsigned wk = 0, zi = 0; if (sscanf(z, "%u:%u", &wk, &zi) == 2 && wk == s->p.workerID && zi == it) *nA = 0; }
#endif
    return rc;
}
// ... and its tail (:314-325): snapshots, status line / histories
static int iteration_tail(cogaps_session *s, int phase, uint32_t it)
{
    if ((s->p.snapshotPhase == 0 || s->p.snapshotPhase == phase) && s->p.snapshotFrequency > 0 && ((it + 1) % s->p.snapshotFrequency) == 0) {
        // GapsStatistics::takeSnapshot (GapsStatistics.h:188-202): getMatrix() of both samplers
        const int w = phase - 1;
        const size_t na = (size_t)s->nGenes * s->K, np_ = (size_t)s->nSamples * s->K;
        s->snapA[w].resize((size_t)(s->nSnap[w] + 1) * na); s->snapP[w].resize((size_t)(s->nSnap[w] + 1) * np_);
        if (cogaps_session_get_rows(s, 'A', s->snapA[w].data() + (size_t)s->nSnap[w] * na)) return 1;
        if (cogaps_session_get_rows(s, 'P', s->snapP[w].data() + (size_t)s->nSnap[w] * np_)) return 1;
        s->nSnap[w]++;
    }
    if (s->p.outputFrequency > 0 && ((it + 1) % s->p.outputFrequency) == 0) {        // displayStatus, :162-199
        const float cs = (s->p.whichMatrixFixed == 'P') ? chisq_of(s, s->A) : chisq_of(s, s->P);
        s->chisqHist.push_back(cs); s->atomHistA.push_back(s->A.nAtoms); s->atomHistP.push_back(s->P.nAtoms);
        if (s->p.printMessages) {
            // elapsed / estimated total time (estimatedPercentComplete, GapsRunner.cpp:127-159)
            const double nIter = (double)it + (phase == 2 ? (double)s->p.nIterations : 0.0), totalIter = 2.0 * (double)s->p.nIterations;
            auto est = [](double current, double total, double nAtoms) {
                const double coef = nAtoms / std::log(current);
                return coef * std::log(std::sqrt(2.0 * total * 3.14159265358979323846)) + total * coef * std::log(total) - total * coef; };
            const double done = est(nIter, nIter, s->A.nAtoms) + est(nIter, nIter, s->P.nAtoms), all = est(nIter, totalIter, s->A.nAtoms) + est(nIter, totalIter, s->P.nAtoms);
            const unsigned el = (unsigned)(now_s() - s->startTime);
            const double frac = done / all;
            const unsigned tt = (frac > 0.0 && std::isfinite((double)el / frac)) ? (unsigned)((double)el / frac) : 0u;
            printf("%u of %u, Atoms: %u(A), %u(P), ChiSq: %.0f, Time: %02u:%02u:%02u / %02u:%02u:%02u\n", it + 1, s->p.nIterations, s->A.nAtoms, s->P.nAtoms, cs,
                   el / 3600u, (el % 3600u) / 60u, el % 60u, tt / 3600u, (tt % 3600u) / 60u, tt % 60u);
            fflush(stdout);
        }
    }
    return 0;
}

// the session's position behind iteration `done` - 1 of `phase`: the last iteration of a phase hands over to the next phase
static void set_position(cogaps_session *s, int phase, uint32_t done)
{
    if (done == s->p.nIterations) { s->posPhase = phase + 1; s->posNext = 0; } else { s->posPhase = phase; s->posNext = done; }
}

// runOnePhase (GapsRunner.cpp:272-327) for iterations [firstIter, firstIter+n)
int cogaps_session_run_iterations(cogaps_session *s, int phase, uint32_t firstIter, uint32_t n, uint64_t *updates)
{
    SESSION_TRY
    const double t0 = now_s();
    if (s->p.printMessages && firstIter == 0 && n > 0) { printf(phase == 1 ? "-- Equilibration Phase --\n" : "-- Sampling Phase --\n"); fflush(stdout); }   // GapsRunner.cpp:446-457
    for (uint32_t it = firstIter; it < firstIter + n; ++it) {
        uint32_t nA, nP;
        if (iteration_head(s, phase, it, &nA, &nP)) return 1;
        if (cogaps_session_iterate(s, nA, nP, phase == 2)) return 1;
        if (updates) *updates += (uint64_t)nA + nP;
        if (iteration_tail(s, phase, it)) return 1;
        set_position(s, phase, it + 1u);
    }
    rt_sync(s->stream);
    s->samplerSeconds += now_s() - t0;
    SESSION_END
}

#include "chain_batch.h"

int cogaps_session_natoms(cogaps_session *s, char which, uint32_t *n) { *n = pick(s, which).nAtoms; return 0; }
int cogaps_session_chisq(cogaps_session *s, char which, float *c) { SESSION_TRY *c = chisq_of(s, pick(s, which)); SESSION_END }
int cogaps_session_dims(cogaps_session *s, char which, uint32_t *M, uint32_t *N, uint32_t *K) { HostSampler &h = pick(s, which); *M = h.d.M; *N = h.d.N; *K = h.d.K; return 0; }
int cogaps_session_avg_queue(cogaps_session *s, char which, float *a) { *a = pick(s, which).avgQueue; return 0; }

int cogaps_session_get_matrix(cogaps_session *s, char which, float *out)
{
    SESSION_TRY
    HostSampler &h = pick(s, which);
    std::vector<float> m((size_t)h.d.K * h.d.Mpad);
    rt_d2h(m.data(), h.d.mat, m.size() * 4, s->stream); rt_sync(s->stream);
    for (uint32_t r = 0; r < h.d.M; ++r) for (uint32_t k = 0; k < h.d.K; ++k) out[(size_t)r * h.d.K + k] = m[(size_t)k * h.d.Mpad + r];
    SESSION_END
}
int cogaps_session_get_rows(cogaps_session *s, char which, float *out)
{
    SESSION_TRY
    HostSampler &h = pick(s, which);
    if (!h.d.sparse) return cogaps_session_get_matrix(s, which, out);
    std::vector<float> m((size_t)h.d.M * h.d.Kpad);
    rt_d2h(m.data(), h.d.rows, m.size() * 4, s->stream); rt_sync(s->stream);
    for (uint32_t r = 0; r < h.d.M; ++r) memcpy(out + (size_t)r * h.d.K, m.data() + (size_t)r * h.d.Kpad, (size_t)h.d.K * 4);
    SESSION_END
}
int cogaps_session_get_ap(cogaps_session *s, char which, float *out)
{
    SESSION_TRY
    HostSampler &h = pick(s, which);
    if (h.d.sparse) { memset(out, 0, (size_t)h.d.M * h.d.N * 4); return 0; }     // the sparse model keeps no A*P cache
    std::vector<float> m((size_t)h.d.M * h.d.Npad);
    rt_d2h(m.data(), h.d.AP, m.size() * 4, s->stream); rt_sync(s->stream);
    for (uint32_t r = 0; r < h.d.M; ++r) memcpy(out + (size_t)r * h.d.N, m.data() + (size_t)r * h.d.Npad, (size_t)h.d.N * 4);
    SESSION_END
}
// a sampler's atomic domain as the device holds it: its scalars (in s->hGs), the handles of its atoms in vector order, every atom record;
// returns the number of atoms
static uint32_t fetch_domain(cogaps_session *s, HostSampler &h, std::vector<uint32_t> &vec, std::vector<AtomRec> &atoms)
{
    read_gs(s, h);
    vec.resize(s->hGs->nAtoms); atoms.resize(h.d.atomCap);
    if (!vec.empty()) rt_d2h(vec.data(), h.d.vec, vec.size() * 4, s->stream);
    rt_d2h(atoms.data(), h.d.atoms, atoms.size() * sizeof(AtomRec), s->stream); rt_sync(s->stream);
    return s->hGs->nAtoms;
}
int cogaps_session_get_atoms(cogaps_session *s, char which, uint64_t *pos, float *mass, uint32_t *left, uint32_t *right)
{
    SESSION_TRY
    HostSampler &h = pick(s, which);
    std::vector<uint32_t> vec; std::vector<AtomRec> atoms;
    const uint32_t n = fetch_domain(s, h, vec, atoms);
    for (uint32_t i = 0; i < n; ++i) {
        const AtomRec &a = atoms[vec[i]];
        if (pos) pos[i] = a.pos;
        if (mass) mass[i] = a.mass;
        if (left) left[i] = a.left != CG_NONE ? atoms[a.left].idx : CG_NONE;
        if (right) right[i] = a.right != CG_NONE ? atoms[a.right].idx : CG_NONE;
    }
    SESSION_END
}

// test hook: the atomic domain's redundant state -- links symmetric, vec / idx inverse of each other, every record's cached neighbour
// positions and right-neighbour mass equal to the neighbours' own -- *violations = number of broken invariants
int cogaps_session_debug_check_domain(cogaps_session *s, char which, uint32_t *violations)
{
    SESSION_TRY
    HostSampler &h = pick(s, which);
    std::vector<uint32_t> vec; std::vector<AtomRec> atoms;
    const uint32_t n = fetch_domain(s, h, vec, atoms);
    uint32_t bad = 0, fronts = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t hd = vec[i];
        if (hd >= h.d.atomCap) { ++bad; continue; }
        const AtomRec &a = atoms[hd];
        if (a.idx != i) ++bad;
        if (a.left != CG_NONE) { const AtomRec &l = atoms[a.left]; if (l.right != hd || a.lpos != l.pos || !(l.pos < a.pos)) ++bad; } else { ++fronts; if (s->hGs->front != hd) ++bad; }
        if (a.right != CG_NONE) { const AtomRec &r = atoms[a.right]; if (r.left != hd || a.rpos != r.pos || gm_f2u(a.rmass) != gm_f2u(r.mass)) ++bad; }
    }
    if (n && fronts != 1) ++bad;
    *violations = bad;
    SESSION_END
}

int cogaps_session_finish(cogaps_session *s, cogaps_result *out)
{
    SESSION_TRY
    memset(out, 0, sizeof(*out));
    if (s->poisoned) return fail("this session was ended by a device error; it holds no result (the state getters still read the half-applied state, for diagnosis)");
    out->nGenes = s->nGenes; out->nSamples = s->nSamples; out->nPatterns = s->K;
    const uint32_t K = s->K;
    auto fetch = [&](float *dptr, size_t n) { std::vector<float> v(n); rt_d2h(v.data(), dptr, n * 4, s->stream); rt_sync(s->stream); return v; };
    std::vector<float> As = fetch(s->Asum, (size_t)K * s->A.d.Mpad), Aq = fetch(s->Asq, (size_t)K * s->A.d.Mpad);
    std::vector<float> Ps = fetch(s->Psum, (size_t)K * s->P.d.Mpad), Pq = fetch(s->Psq, (size_t)K * s->P.d.Mpad);
    const float n = (float)s->statUpdates;
    auto fill = [&](uint32_t rows, uint32_t Mpad, const std::vector<float> &sum, const std::vector<float> &sq, float *&mean, float *&sd) {
        mean = (float *)malloc((size_t)rows * K * 4 + 4); sd = (float *)malloc((size_t)rows * K * 4 + 4);
        for (uint32_t i = 0; i < rows; ++i) for (uint32_t k = 0; k < K; ++k) {       // GapsStatistics.cpp:13-59
            const float a = sum[(size_t)k * Mpad + i], q = sq[(size_t)k * Mpad + i];
            mean[(size_t)i * K + k] = a / n;
            const float meanTerm = (a * a) / n, numer = gm_max(0.f, q - meanTerm);
            sd[(size_t)i * K + k] = sqrtf(numer / (n - 1.f));
        }
    };
    fill(s->nGenes, s->A.d.Mpad, As, Aq, out->Amean, out->Asd);
    fill(s->nSamples, s->P.d.Mpad, Ps, Pq, out->Pmean, out->Psd);
    out->nHistory = (uint32_t)s->chisqHist.size();
    out->chisqHistory = (float *)malloc(out->nHistory * 4 + 4); out->atomHistoryA = (uint32_t *)malloc(out->nHistory * 4 + 4); out->atomHistoryP = (uint32_t *)malloc(out->nHistory * 4 + 4);
    memcpy(out->chisqHistory, s->chisqHist.data(), out->nHistory * 4); memcpy(out->atomHistoryA, s->atomHistA.data(), out->nHistory * 4); memcpy(out->atomHistoryP, s->atomHistP.data(), out->nHistory * 4);
    out->totalUpdates = s->totalUpdates; out->seed = s->p.seed;
    out->averageQueueLengthA = s->A.avgQueue; out->averageQueueLengthP = s->P.avgQueue;
    out->samplerSeconds = s->samplerSeconds; out->totalRunningTime = (uint32_t)(now_s() - s->startTime);   // GapsRunner.cpp:463
    out->meanChiSq = 0.f;                                                             // GapsRunner.cpp:478-484
    if (s->p.whichMatrixFixed == 'N' && s->statUpdates > 0) {
        const float n2 = (float)s->statUpdates * (float)s->statUpdates;
        if (s->P.d.seq) {
            RT_LAUNCH(mean_chisq_seq_kernel, 1, 256, s->stream, s->P.d, (const float *)s->P.Sraw, (const float *)s->Asum, (const float *)s->Psum, s->A.d.Mpad, n2, s->P.partial);
            rt_d2h(&out->meanChiSq, s->P.partial, 4, s->stream); rt_sync(s->stream);
        } else {
        if (s->P.d.sparse) LAUNCH_V(mean_chisq_rows_packed_kernel, s->P.d.redW, s->P.d.M, s->stream, s->P.d, (const float *)s->Asum, (const float *)s->Psum, s->A.d.Mpad, n2, s->P.partial);      // (no dense D / Sraw: sparse_build.h)
        else LAUNCH_V(mean_chisq_rows_kernel, s->P.d.redW, s->P.d.M, s->stream, s->P.d, (const float *)s->P.Sraw, (const float *)s->Asum, (const float *)s->Psum, s->A.d.Mpad, n2, s->P.partial);
        out->meanChiSq = sum_partials(s, s->P.partial, s->P.d.M);
        }
    }
    if (s->p.takePumpSamples) {                                                       // GapsRunner.cpp:487-492, GapsStatistics.cpp:113-131
        const size_t na = (size_t)s->nGenes * K;
        std::vector<float> pm = fetch(s->pump, na);
        const float denom = s->pumpUpdates != 0 ? (float)s->pumpUpdates : 1.f;
        out->pumpMatrix = (float *)malloc(na * 4 + 4); out->meanPatternAssignment = (float *)calloc(na + 1, 4);
        for (size_t t = 0; t < na; ++t) out->pumpMatrix[t] = pm[t] / denom;
        for (uint32_t i = 0; i < s->nGenes; ++i) {                                    // meanPattern(): the same rule on Amean
            float maxV = 0.f; uint32_t maxI = 0;
            for (uint32_t j = 0; j < K; ++j) { const float v = out->Amean[(size_t)i * K + j]; if (maxV < v) { maxV = v; maxI = j; } }
            out->meanPatternAssignment[(size_t)i * K + maxI] += 1.f;
        }
    }
    out->nEquilibrationSnapshots = s->nSnap[0]; out->nSamplingSnapshots = s->nSnap[1];
    auto dup = [](const std::vector<float> &v) { float *p = (float *)malloc(v.size() * 4 + 4); if (!v.empty()) memcpy(p, v.data(), v.size() * 4); return p; };
    out->equilibrationSnapshotsA = dup(s->snapA[0]); out->equilibrationSnapshotsP = dup(s->snapP[0]);
    out->samplingSnapshotsA = dup(s->snapA[1]); out->samplingSnapshotsP = dup(s->snapP[1]);
        if (s->p.runningDistributed) {                                                     // GapsRunner.cpp:494-500
        const unsigned el = (unsigned)(now_s() - s->startTime);
        printf("    worker %u is finished! Time: %02u:%02u:%02u\n", s->p.workerID, el / 3600u, (el % 3600u) / 60u, el % 60u); fflush(stdout);
    }
    SESSION_END
}

// development aid: relaunch the evaluation (kind 1) or generator (kind 0) kernel `n` times on the current
// device state and return the mean wall time per launch in microseconds (the chain state is garbage afterwards)
int cogaps_session_debug_replay(cogaps_session *s, char which, int kind, uint32_t n, uint32_t dbgFlags, double *usPerLaunch)
{
    SESSION_TRY
    HostSampler &h = pick(s, which);
    {   // arm a fresh update of 4096 steps and generate one batch so that the queue is populated
        read_gs(s, h);
        GenScalars g = *s->hGs;
        const uint32_t steps = kind >= 2 ? 65536u : 4096u;       // kinds 2 (generator alone) / 3 (pairs) run many real batches
        if (h.seedCap < steps) { rt_free(h.seeds); h.seedCap = 2u * steps; h.seeds = dalloc<uint64_t>(h.seedCap); }
        std::vector<uint64_t> sd(steps); seed_take(s, sd.data(), sd.size());
        rt_h2d(h.seeds, sd.data(), sd.size() * 8, s->stream); h.d.seeds = h.seeds;
        g.nSteps = steps; g.nDone = 0; g.updateFlushed = 0; g.qlen = 0; g.traceOn = 0;
        *s->hGs = g; rt_h2d(h.d.gs, s->hGs, sizeof(GenScalars), s->stream);
        sync_record(s, h);
        launch_gen(s, h);
        if (kind == 0 || kind == 3) launch_eval(s, h);
    }
    rt_sync(s->stream);
    h.d.dbg = dbgFlags;
    sync_record(s, h);
    const double t0 = now_s();
    for (uint32_t i = 0; i < n; ++i) { if (kind == 0 || kind == 3) { launch_gen(s, h); launch_eval(s, h); } else if (kind == 2) launch_gen(s, h); else launch_eval(s, h); }
    rt_sync(s->stream);
    *usPerLaunch = 1e6 * (now_s() - t0) / (double)n;
    h.d.dbg = 0;
    SESSION_END
}
int cogaps_session_debug_prof(cogaps_session *s, char which, uint64_t *out16)
{
    SESSION_TRY
    read_gs(s, pick(s, which));
    for (int i = 0; i < 16; ++i) out16[i] = s->hGs->prof[i];
    SESSION_END
}
#if defined(GEN_TIMELINE)
extern "C" int cogaps_debug_timeline(unsigned long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), sizeof(unsigned long long) * (size_t)n);
}
extern "C" int cogaps_debug_chain_timeline(unsigned long long *wgs, unsigned long long *gen)
{
    if (hipMemcpyFromSymbol(wgs, HIP_SYMBOL(g_chain_rt), sizeof(unsigned long long) * 1024) != hipSuccess) return 1;
    return (int)hipMemcpyFromSymbol(gen, HIP_SYMBOL(g_chain_gen), sizeof(unsigned long long) * 8);
}
extern "C" int cogaps_debug_ahead_why(unsigned long long *out8) { return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ahead_why), sizeof(unsigned long long) * 8); }
extern "C" int cogaps_debug_chain_log(unsigned long long *out, unsigned int *n)
{
    if (hipMemcpyFromSymbol(n, HIP_SYMBOL(g_chain_log_n), sizeof(unsigned int)) != hipSuccess) return 1;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chain_log), sizeof(unsigned long long) * (size_t)GEN_LOG_N * 8);
}
extern "C" int cogaps_debug_eval_timeline(unsigned long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_eval_timeline), sizeof(unsigned long long) * (size_t)n);
}
#endif
int cogaps_session_set_timing(cogaps_session *s, int on)
{
    SESSION_TRY
    if (on) s->ev.create(2048);
    if (on && !s->timing) {      // a new window: the sampled times are scaled to the batches processed from here on
        for (HostSampler *h : {&s->A, &s->P}) {
            h->batchesAtTimingOn = h->batches;
            h->evalMs = h->genMs = h->evalNoopMs = h->genNoopMs = 0; h->evalTimed = h->genTimed = h->evalNoopTimed = h->genNoopTimed = 0;
            h->clockHist.assign(2048, 0); h->clockSumUs = 0; h->clockN = 0;
            h->periodHist.assign(2048, 0); h->periodSumUs = 0; h->periodN = 0;
        }
        s->syncMs = 0; s->syncTimed = 0; s->syncBytes = 0;
    }
    s->timing = on != 0;
    SESSION_END
}
static void add_perf(cogaps_session *s, HostSampler *h, cogaps_perf *out)
{
    read_gs(s, *h);
    out->evalBytes += s->hGs->evalBytes; out->proposalsQueued += s->hGs->evalProps;
    out->evalLaunches += h->evalLaunches; out->genLaunches += h->genLaunches; out->batches += h->batches;
    // sampled event timing scaled to the batches processed since timing was switched on
    const double win = (double)(h->batches - h->batchesAtTimingOn);
    out->timedBatches += h->batches - h->batchesAtTimingOn; out->evalTimed += h->evalTimed; out->genTimed += h->genTimed;
    if (h->evalTimed) out->evalMs += h->evalMs * win / (double)h->evalTimed;
    if (h->genTimed) out->genMs += h->genMs * win / (double)h->genTimed;
    out->evalNoopMs += h->evalNoopMs; out->evalNoopTimed += h->evalNoopTimed;
    out->genNoopMs += h->genNoopMs; out->genNoopTimed += h->genNoopTimed;
}
int cogaps_session_perf(cogaps_session *s, cogaps_perf *out)
{
    SESSION_TRY
    memset(out, 0, sizeof(*out));
    rt_sync(s->stream); timing_resolve(s, 0);        // sync launches timed since the last update (generator / evaluation events are resolved per chunk)
    for (HostSampler *h : {&s->A, &s->P}) add_perf(s, h, out);
    out->syncMs = s->syncMs; out->syncTimed = s->syncTimed; out->syncBytes = s->syncBytes;
    SESSION_END
}
int cogaps_session_perf_sampler(cogaps_session *s, char which, cogaps_perf *out)
{
    SESSION_TRY
    memset(out, 0, sizeof(*out));
    add_perf(s, &pick(s, which), out);
    SESSION_END
}

// the mean and the 10 / 50 / 75 / 90 / 99th percentiles of n launch times kept as a histogram of 0.1 us bins
static int report_hist(const std::vector<uint64_t> &hist, double sumUs, uint64_t n, double *meanUs, double *percentilesUs, uint64_t *launches)
{
    if (!meanUs || !percentilesUs || !launches) return fail("null argument");
    *launches = n; *meanUs = n ? sumUs / (double)n : 0.0;
    static const double q[5] = {0.10, 0.50, 0.75, 0.90, 0.99};
    for (int k = 0; k < 5; ++k) {
        percentilesUs[k] = 0.0;
        if (!n) continue;
        const uint64_t want = (uint64_t)(q[k] * (double)n); uint64_t acc = 0;
        for (size_t b = 0; b < hist.size(); ++b) { acc += hist[b]; if (acc > want) { percentilesUs[k] = 0.1 * ((double)b + 0.5); break; } }
    }
    return 0;
}
int cogaps_session_launch_clock(cogaps_session *s, char which, double *meanUs, double *percentilesUs, uint64_t *launches)
{
    SESSION_TRY
    const HostSampler &h = pick(s, which);
    return report_hist(h.clockHist, h.clockSumUs, h.clockN, meanUs, percentilesUs, launches);
    SESSION_END
}
int cogaps_session_launch_period(cogaps_session *s, char which, double *meanUs, double *percentilesUs, uint64_t *launches)
{
    SESSION_TRY
    const HostSampler &h = pick(s, which);
    return report_hist(h.periodHist, h.periodSumUs, h.periodN, meanUs, percentilesUs, launches);
    SESSION_END
}
int cogaps_session_chain_recoveries(cogaps_session *s, char which, uint32_t *n)
{
    SESSION_TRY
    if (!n) return fail("null argument");
    *n = pick(s, which).chainRecoveries;
    SESSION_END
}
int cogaps_session_generator_window(cogaps_session *s, char which, uint32_t *attempts)
{
    SESSION_TRY
    if (!attempts) return fail("null argument");
    *attempts = pick(s, which).genWin;
    SESSION_END
}
int cogaps_session_chained(cogaps_session *s, char which, int *chained)
{
    SESSION_TRY
    if (!chained) return fail("null argument");
    *chained = pick(s, which).chain ? 1 : 0;
    SESSION_END
}

// the library's own state file, at its place among the chapters
#include "session_state.h"

int cogaps_session_run_to_end(cogaps_session *s, const char *statePath, uint32_t interval, cogaps_result *out)
{
    if (!s || !out) return fail("null argument");
    if (statePath && state_refusal(s, statePath, "saved")) return 1;      // (before anything runs: a sequential session keeps no state file)
    const uint32_t nIter = s->p.nIterations;
    uint32_t sinceSave = 0;
    while (s->posPhase < 3) {
        const int phase = s->posPhase; const uint32_t next = s->posNext;
        if (next >= nIter) { set_position(s, phase, nIter); continue; }      // (nothing left of this phase)
        uint32_t n = nIter - next;
        if (statePath && interval) n = std::min(n, interval - sinceSave);
        if (cogaps_session_run_iterations(s, phase, next, n, nullptr)) {
            // the interrupt hook is polled at the head of an iteration, before anything of it is drawn: the state is that of the position
            if (statePath && g_last_error == "interrupted" && cogaps_session_save_state(s, statePath)) return fail("interrupted, and the state could not be saved: " + g_last_error);
            return 1;
        }
        sinceSave += n;
        if (statePath && interval && sinceSave >= interval) { if (cogaps_session_save_state(s, statePath)) return 1; sinceSave = 0; }
    }
    if (statePath && cogaps_session_save_state(s, statePath)) return 1;      // the complete run: position 3
    return cogaps_session_finish(s, out);
}

// The one-shot entries' run of the session they have just created: both phases, the result, and the session's end whatever came of
// them.  s null: the creation has said why (cogaps_last_error).  The iterations are the session's copy of the caller's parameters.
static int run_once(cogaps_session *s, cogaps_result *out)
{
    if (!s) return 1;
    int rc = cogaps_session_run_iterations(s, 1, 0, s->p.nIterations, nullptr);
    if (!rc) rc = cogaps_session_run_iterations(s, 2, 0, s->p.nIterations, nullptr);
    if (!rc) rc = cogaps_session_finish(s, out);
    cogaps_session_destroy(s);
    return rc;
}

int cogaps_run(const float *data, uint32_t nrow, uint32_t ncol, const cogaps_params *params, const float *unc, cogaps_result *out)
{
    if (!out) return fail("null argument");
    return run_once(cogaps_session_create(data, nrow, ncol, params, unc, 0), out);
}

int cogaps_run_device(const float *data, uint32_t nrow, uint32_t ncol, const cogaps_params *params, const float *unc, cogaps_result *out)
{
    if (!out) return fail("null argument");
    return run_once(cogaps_session_create(data, nrow, ncol, params, unc, 1), out);
}

int cogaps_session_debug_dense_data(cogaps_session *s, char which, float *D, float *Sraw, float *S2, float *lambda, float *maxGibbsMass, float *sparsity, int *hasS2)
{
    if (!s) return fail("null argument");
    SESSION_TRY
    const HostSampler &h = pick(s, which); const SamplerDev &d = h.d;
    if (d.sparse) return fail("the session does not run the dense model");
    const size_t bytes = (size_t)d.M * d.Npad * 4;
    if (lambda) *lambda = d.lambda;
    if (maxGibbsMass) *maxGibbsMass = d.maxGibbsMass;
    if (sparsity) *sparsity = h.dataSparsity;
    if (hasS2) *hasS2 = d.S2 != nullptr;
    if (D) rt_d2h(D, d.D, bytes, s->stream);
    if (Sraw) rt_d2h(Sraw, h.Sraw, bytes, s->stream);
    if (S2 && d.S2) rt_d2h(S2, d.S2, bytes, s->stream);
    rt_sync(s->stream);
    SESSION_END
}

int cogaps_session_debug_sparse_data(cogaps_session *s, char which, uint32_t *Wn, uint32_t *nVals, float *lambda, float *maxGibbsMass,
                                     uint64_t *flags, uint32_t *prefix, uint32_t *ptr, float *vals)
{
    if (!s) return fail("null argument");
    SESSION_TRY
    const SamplerDev &d = pick(s, which).d;
    if (!d.sparse) return fail("the session does not run the sparse model");
    uint32_t n = 0; rt_d2h(&n, d.dptr + d.M, 4, s->stream); rt_sync(s->stream);
    if (Wn) *Wn = d.Wn;
    if (nVals) *nVals = n;
    if (lambda) *lambda = d.lambda;
    if (maxGibbsMass) *maxGibbsMass = d.maxGibbsMass;
    if (flags) rt_d2h(flags, d.dflags, (size_t)d.M * d.Wn * 8, s->stream);
    if (prefix) rt_d2h(prefix, d.dprefix, (size_t)d.M * d.Wn * 4, s->stream);
    if (ptr) rt_d2h(ptr, d.dptr, ((size_t)d.M + 1) * 4, s->stream);
    if (vals && n) rt_d2h(vals, d.dvals, (size_t)n * 4, s->stream);
    rt_sync(s->stream);
    SESSION_END
}

int cogaps_run_sparse(const cogaps_sparse_matrix *m, const cogaps_params *params, cogaps_result *out)
{
    if (!out) return fail("null argument");
    return run_once(cogaps_session_create_sparse(m, params), out);
}

int cogaps_run_coo(const cogaps_coo_matrix *m, const cogaps_params *params, cogaps_result *out)
{
    if (!out) return fail("null argument");
    return run_once(cogaps_session_create_coo(m, params), out);
}

int cogaps_run_device_matrix(const cogaps_device_matrix *m, const cogaps_params *params, cogaps_result *out)
{
    if (!out) return fail("null argument");
    return run_once(cogaps_session_create_from_device_matrix(m, params), out);
}

// ---- the file entry point (gaps::run(const std::string&...), GapsRunner.h:24-29; cogaps_from_file_cpp, Cogaps.cpp:217-227) ----
static int table_out(const cgio::Table &t, uint32_t *nrow, uint32_t *ncol, float **data)
{
    float *v = (float *)malloc(std::max<size_t>(1, t.v.size()) * sizeof(float));
    if (!v) return fail("out of memory");
    memcpy(v, t.v.data(), t.v.size() * sizeof(float));
    *nrow = t.nrow; *ncol = t.ncol; *data = v;
    return 0;
}
int cogaps_read_matrix_file(const char *path, uint32_t *nrow, uint32_t *ncol, float **data)
{
    try {
        if (!path || !nrow || !ncol || !data) return fail("null argument");
        return table_out(cgio::read_matrix_file(path), nrow, ncol, data);
    } catch (const std::exception &e) { return fail_exc(e); }
}
// the rows (byRows != 0) or columns of the file named by the 1-based `indices`, as the reference's workers read their subset of a
// file (Matrix(path, genesInCols, subsetGenes, indices), data_structures/Matrix.cpp:70-134: sorted indices, lower_bound placement);
// the rest of the matrix is never materialised
int cogaps_read_matrix_file_subset(const char *path, int byRows, const uint32_t *indices, uint32_t nIndices, uint32_t *nrow, uint32_t *ncol, float **data)
{
    try {
        if (!path || !nrow || !ncol || !data || !indices || nIndices == 0) return fail("null argument or empty subset");
        cgio::ReadOpts o; o.sub = cgio::Subset(byRows != 0, indices, nIndices);
        return table_out(cgio::read_matrix_file(path, o), nrow, ncol, data);
    } catch (const std::exception &e) { return fail_exc(e); }
}

void cogaps_matrix_free(float *data) { free(data); }

// The .mtx file as triplets in file order (file_reader.h, read_mtx_triplets): what cogaps_read_matrix_file[_subset] gives, entry by
// entry instead of densified -- D = 0; D[rows[k]][cols[k]] = values[k] in order reproduces it byte for byte.
int cogaps_read_mtx_triplets(const char *path, int byRows, const uint32_t *indices, uint32_t nIndices,
                             uint32_t *nrow, uint32_t *ncol, uint64_t *nnz, uint32_t **rows, uint32_t **cols, float **values)
{
    try {
        if (!path || !nrow || !ncol || !nnz || !rows || !cols || !values) return fail("null argument");
        if (indices && nIndices == 0) return fail("null argument or empty subset");
        cgio::ReadOpts o; if (indices) o.sub = cgio::Subset(byRows != 0, indices, nIndices);
        const cgio::Triplets t = cgio::read_mtx_triplets_file(path, o);
        const size_t n = t.v.size(), bytes = std::max<size_t>(1, n) * 4;
        uint32_t *r = (uint32_t *)malloc(bytes), *c = (uint32_t *)malloc(bytes); float *v = (float *)malloc(bytes);
        if (!r || !c || !v) { free(r); free(c); free(v); return fail("out of memory"); }
        memcpy(r, t.r.data(), n * 4); memcpy(c, t.c.data(), n * 4); memcpy(v, t.v.data(), n * 4);
        *nrow = t.nrow; *ncol = t.ncol; *nnz = n; *rows = r; *cols = c; *values = v;
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}
void cogaps_triplets_free(uint32_t *rows, uint32_t *cols, float *values) { free(rows); free(cols); free(values); }

// getFileInfo_cpp (Cogaps.cpp:229-246): dimensions and the names the file carries, '\n'-joined into caller buffers
// (a NULL buffer or zero capacity skips the names; *needed reports the bytes a complete copy takes, terminator included)
int cogaps_file_info(const char *path, uint32_t *nrow, uint32_t *ncol, char *rowNames, size_t rowCap, size_t *rowNeeded,
                     char *colNames, size_t colCap, size_t *colNeeded)
{
    try {
        if (!path || !nrow || !ncol) return fail("null argument");
        cgio::ReadOpts o; o.values = false;                      // dimensions and names: no value is parsed, no matrix is built
        cgio::Table t = cgio::read_matrix_file(path, o);
        *nrow = t.nrow; *ncol = t.ncol;
        auto join = [](const std::vector<std::string> &v, char *out, size_t cap, size_t *needed) {
            std::string s; for (size_t i = 0; i < v.size(); ++i) { if (i) s += '\n'; s += v[i]; }
            if (needed) *needed = s.size() + 1;
            if (out && cap) { const size_t n = std::min(cap - 1, s.size()); memcpy(out, s.data(), n); out[n] = 0; }
        };
        join(t.rowNames, rowNames, rowCap, rowNeeded); join(t.colNames, colNames, colCap, colNeeded);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

int cogaps_run_from_file(const char *dataPath, const cogaps_params *params, const char *uncertaintyPath, cogaps_result *out)
{
    try {
        if (!dataPath || !params || !out) return fail("null argument");
        // A worker of a distributed run reads ITS subset of the file (Matrix.cpp:70-134): the rows or columns the indices name, in
        // sorted order -- never the whole matrix.  The run then sees an ordinary matrix with no subset left to take.
        cgio::ReadOpts o; cogaps_params p = *params;
        if (p.subsetData && p.dataIndicesSubset && p.nSubset) {
            const bool byRows = (p.subsetGenes != 0) == (p.transposeData == 0);      // genes are the file's rows unless transposeData
            o.sub = cgio::Subset(byRows, p.dataIndicesSubset, p.nSubset);
            p.subsetData = 0; p.dataIndicesSubset = nullptr; p.nSubset = 0;
        }
        const bool haveUnc = uncertaintyPath && uncertaintyPath[0];
        // A Matrix Market file for the sparse model (default reduction order, default uncertainty) goes in as triplets: the run of the
        // dense read, bit for bit, without the nrow x ncol array on the host or the device.  (An empty matrix keeps the dense route's
        // message.)
        if (cgio::is_mtx_path(dataPath) && p.useSparseOptimization && p.reductionMode == COGAPS_REDUCE_LANES && !haveUnc && !p.subsetData) {
            const cgio::Triplets t = cgio::read_mtx_triplets_file(dataPath, o);
            if (t.nrow && t.ncol && t.v.size() < 0xFFFFFFFFull) {
                cogaps_coo_matrix m; m.nrow = t.nrow; m.ncol = t.ncol; m.nnz = t.v.size(); m.rows = t.r.data(); m.cols = t.c.data(); m.values = t.v.data(); m.onDevice = 0;
                return cogaps_run_coo(&m, &p, out);
            }
        }
        cgio::Table d = cgio::read_matrix_file(dataPath, o), u;
        if (haveUnc) {
            u = cgio::read_matrix_file(uncertaintyPath, o);
            if (u.nrow != d.nrow || u.ncol != d.ncol || u.fileRows != d.fileRows || u.fileCols != d.fileCols) return fail("uncertainty matrix has different dimensions than the data");
        }
        return cogaps_run(d.v.data(), d.nrow, d.ncol, &p, haveUnc ? u.v.data() : nullptr, out);
    } catch (const std::exception &e) { return fail_exc(e); }
}

void cogaps_result_free(cogaps_result *r)
{
    if (!r) return;
    free(r->Amean); free(r->Asd); free(r->Pmean); free(r->Psd); free(r->chisqHistory); free(r->atomHistoryA); free(r->atomHistoryP);
    free(r->pumpMatrix); free(r->meanPatternAssignment);
    free(r->equilibrationSnapshotsA); free(r->equilibrationSnapshotsP); free(r->samplingSnapshotsA); free(r->samplingSnapshotsP);
    memset(r, 0, sizeof(*r));
}

} // extern "C"
