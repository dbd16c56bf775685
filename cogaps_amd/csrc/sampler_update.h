// sampler_update.h -- the update of one sampler of a one-chain session (AsynchronousGibbsSampler::update, SingleThreadedGibbsSampler::update):
// host code only, a chapter of cogaps_hip.cpp, which includes it once, where the chapter used to stand -- after the kernel headers, by_window,
// EventPool, GraphCache, HostSampler, cogaps_session, fail, dalloc, dev_env and session_build.h's build_death_prob_table, which it takes from there.  Not a
// stand-alone header.  Kernels are instantiated, and laid out in the code object, in the order of their first use: one kernel per by_window
// call, and the LAUNCH_* sites stay in the order they have here.  What chain_batch.h, the second chapter of the drivers, shares with this
// one is written here once: begin_update / end_update, chunk_size, steps_per_batch, split_geometry / split_per_wave, set_window,
// clear_chain_slots, fail_device_error, begin_update_seq / end_update_seq.
#pragma once

static void read_gs(cogaps_session *s, HostSampler &h)
{
    rt_d2h(s->hGs, h.d.gs, sizeof(GenScalars), s->stream);
    rt_sync(s->stream);
}

// the next n outputs of the session's seeder into dst, from the look-ahead buffer as far as it reaches
static void seed_take(cogaps_session *s, uint64_t *dst, size_t n)
{
    const size_t avail = s->seedFifo.size() - s->seedHead, k = std::min(avail, n);
    if (k) { memcpy(dst, s->seedFifo.data() + s->seedHead, k * 8); s->seedHead += k; }
    for (size_t i = k; i < n; ++i) dst[i] = s->seeder.next();
    if (s->seedHead == s->seedFifo.size()) { s->seedFifo.clear(); s->seedHead = 0; }
}
// look ahead while the GPU works through a chunk of launches: the seeds of the next update, the other sampler's (about one per atom it
// holds; Poisson spread + margin)
static void seed_top_up(cogaps_session *s, const HostSampler &next)
{
    const uint32_t na = std::max(next.nAtoms, 10u);
    const size_t target = (size_t)na + (size_t)(6.0 * sqrt((double)na)) + 64u;
    size_t avail = s->seedFifo.size() - s->seedHead;
    if (avail >= target) return;
    if (s->seedHead) { s->seedFifo.erase(s->seedFifo.begin(), s->seedFifo.begin() + (ptrdiff_t)s->seedHead); s->seedHead = 0; }
    s->seedFifo.reserve(target);
    for (; avail < target; ++avail) s->seedFifo.push_back(s->seeder.next());
}

static void grow_atoms(cogaps_session *s, HostSampler &h, uint32_t need)
{
    SamplerDev &d = h.d;
    if (need <= d.atomCap) return;
    rt_alloc_scope allocOn(s->stream); rt_owner_scope owner(&s->deviceBytes);
    uint32_t cap = d.atomCap;
    while (cap < need) cap = (uint32_t)std::min<uint64_t>((uint64_t)cap * 2, 0x7FFFFFF0ull);
    auto regrow = [&](auto *&ptr, size_t elt) {
        void *n = rt_malloc((size_t)cap * elt);
        rt_d2d(n, ptr, (size_t)d.atomCap * elt, s->stream); rt_sync(s->stream);
        rt_free(ptr); ptr = (decltype(ptr))n;
    };
    regrow(d.atoms, sizeof(AtomRec)); regrow(d.vec, 4); regrow(d.freeHandles, 4);
    regrow(d.atomStamp, 8); regrow(d.inlineStamp, 8); regrow(d.atomDest, 8);
    { void *n = rt_malloc(((size_t)cap + 1) * 8); rt_d2d(n, d.gapStamp, ((size_t)d.atomCap + 1) * 8, s->stream); rt_sync(s->stream); rt_free(d.gapStamp); d.gapStamp = (unsigned long long *)n; }
    d.atomCap = cap;
    rt_free((void *)d.deathProb); d.deathProb = nullptr;
    build_death_prob_table(s, d);
}

// A one-chain session times every 8th generator / evaluation launch (and every sync launch) of its plain launches
static int timing_slot(cogaps_session *s, HostSampler &h, int kind, uint64_t ordinal)
{
    if (!s->timing || (kind != EV_SYNC && (ordinal % 8) != 0)) return -1;
    return s->ev.take(kind, &h, h.updLaunches);
}
// `realBatches` = batches the current update has generated so far: pair number k processed a batch iff k < realBatches
static void timing_resolve(cogaps_session *s, uint64_t realBatches)
{
    s->ev.drain([&](const EvSample &e, float ms) {
        HostSampler *h = e.owner;
        const bool real = e.ord < realBatches;
        if (e.kind == EV_GEN) { if (real) { h->genMs += ms; h->genTimed++; } else { h->genNoopMs += ms; h->genNoopTimed++; } }
        else if (e.kind == EV_EVAL) { if (real) { h->evalMs += ms; h->evalTimed++; } else { h->evalNoopMs += ms; h->evalNoopTimed++; } }
        else if (e.kind == EV_SYNC) { s->syncMs += ms; s->syncTimed++; }     // sync (AP transpose / lookup tables): every launch is timed
        else { if (real) h->evalMs += ms; else h->evalNoopMs += ms; }
    });
}
// The generator reads the sampler's record from device memory (gen_populate.h: a by-value SamplerDev made the compiler open the kernel
// with seven serial scalar-cache misses).  The copy is refreshed, on the session's stream, whenever the host's record changed.
static void sync_record(cogaps_session *s, HostSampler &h)
{
    if (!h.dRecord) h.dRecord = dalloc<SamplerDev>(1);
    if (h.recordValid && memcmp(&h.recordHeld, &h.d, sizeof(SamplerDev)) == 0) return;
    h.recordHeld = h.d;
    rt_h2d(h.dRecord, &h.recordHeld, sizeof(SamplerDev), s->stream);
    rt_sync(s->stream);
    h.recordValid = true;
}
// The one-chain split evaluation (data vectors of more than 4096 elements, dense model, product arithmetic) is ONE launch that decides
// (eval_kernel<EVAL_DECIDE>); the A*P updates it owes are carried out by the further workgroups of the NEXT generator launch
// (gen_apply_kernel) -- see eval_kernel.h.  The batched multi-chain launches keep the two-launch form (alpha, apply).
static bool split_one_launch(const HostSampler &h)
{
    static const bool twoLaunches = dev_env("COGAPS_SPLIT_TWO_LAUNCHES") != nullptr;      // dev builds: A/B against the two-launch form (alpha kernel, apply kernel)
    return !twoLaunches && !h.d.seq && !h.d.sparse && h.d.redW > 1024u;
}
static uint32_t apply_grid()
{
#if defined(COGAPS_EMUL)
    static const uint32_t g = 5u;        // (test-only emulator: a workgroup is a set of fibers, few of them keep the tests quick; 5 does not divide the items evenly)
#else
    static const uint32_t g = dev_env("COGAPS_APPLY_GRID") ? (uint32_t)atoi(dev_env("COGAPS_APPLY_GRID")) : 127u;      // dev builds: A/B of the update workgroups' number
#endif
    return g < 1u ? 1u : g;
}
// Updates in flight in this process (sessions stepped from several host threads: shards in flight, bench --chains-mode threads).  A chained
// launch wants every workgroup of its launch resident at once -- one per compute unit: its kernel's LDS -- so two chains' chained launches
// take turns on the chip and the hand-over inside each waits for the other's workgroups to leave (correct, and slower than two launches
// per batch each).  The chained form is therefore taken only by an update that runs alone ON ITS GPU: one count per device ordinal (sessions
// on different GPUs of one process do not switch each other's chained launch off), taken by the one-chain update and by the batched update
// alike; the count is looked at when an update begins.
static const int MAX_DEVICES = 64;
static std::atomic<int> &g_updatesRunning(int device) { static std::atomic<int> n[MAX_DEVICES]; return n[device >= 0 && device < MAX_DEVICES ? device : 0]; }
struct UpdateInFlight { int dev; explicit UpdateInFlight(int device) : dev(device) { g_updatesRunning(dev).fetch_add(1); } ~UpdateInFlight() { g_updatesRunning(dev).fetch_sub(1); } };
// launch geometry of the split evaluation (data vectors of more than 4096 elements): `slices` workgroups of `bs` threads per proposal
// (512 threads fill the machine a little better than 1024; at most 16 slices fit the partials record)
static void split_geometry(const HostSampler &h, uint32_t &bs, uint32_t &slices)
{
    bs = std::max<uint32_t>(512u, h.d.redW / 16u);
    slices = std::min<uint32_t>(h.d.redW / bs, ((h.d.Npad >> 2) + bs - 1u) / bs);
}
// ... and the proposals one wave of its workgroups takes: two resident 1024-thread workgroups per compute unit
static uint32_t split_per_wave(uint32_t bs, uint32_t slices) { return std::max<uint32_t>(1u, (512u * (1024u / bs)) / slices); }
static void launch_chain(cogaps_session *s, HostSampler &h)
{
    const int slot = timing_slot(s, h, EV_EVAL, h.evalLaunches);
    const SamplerDev CG_CONSTANT *rec = (const SamplerDev CG_CONSTANT *)h.dRecord;
    const uint32_t parity = h.chainParity; h.chainParity ^= 1u;
    if (h.d.sparse) {
        // sparse model (sparse_kernels.h, chain_sparse_kernel): the launch has 512 threads per workgroup whatever the model's width
        // (255 evaluation workgroups + the generator = the chip's 256 compute units; a workgroup evaluates two proposals side by side where the
        // model's vectors take one round of flag words -- sparse_kernels.h, sp_grp -- so queues of up to 510 fit one pass; the dense launch keeps
        // 240 workgroups, profiles/r04_ab_chained_launch_not_kept.txt)
#if defined(COGAPS_EMUL)
        const uint32_t grid = std::min<uint32_t>(h.d.queueCap, CHAIN_EVAL_GRID) + 1u;      // (test-only emulator: few workgroups, so that both groups of an evaluation workgroup get proposals)
#else
        const uint32_t grid = std::min<uint32_t>(h.d.queueCap, s->computeUnits >= 256u ? 255u : CHAIN_EVAL_GRID) + 1u;
#endif
        const bool wide = h.d.Wn > cogaps_sparse_width(h.d.N);
        by_window<true>(h.genWin, [&](auto W) {
            constexpr int WIN = decltype(W)::value;
            if (wide) LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, (chain_sparse_kernel<WIN, true>), grid, CHAIN_MAX_THREADS, h.d.lcgMul, h.d.lcgInc, h.d.gs, h.d.queue, h.chainGrans, h.d.chainSlots, h.d.queueCap, parity, rec);
            else LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, (chain_sparse_kernel<WIN, false>), grid, CHAIN_MAX_THREADS, h.d.lcgMul, h.d.lcgInc, h.d.gs, h.d.queue, h.chainGrans, h.d.chainSlots, h.d.queueCap, parity, rec);
        });
    } else {
        // the fused evaluation, or the split one (data vectors of more than 4096 elements): then the evaluation workgroups are a multiple of
        // the slices per proposal (chain_kernel.h)
        const bool split = h.d.redW > 1024u;
        uint32_t bs = h.d.redW, slices = 1u;
        if (split) split_geometry(h, bs, slices);
        const uint32_t groups = split ? std::max<uint32_t>(1u, std::min<uint32_t>(h.d.queueCap, CHAIN_EVAL_GRID / slices)) : std::min<uint32_t>(h.d.queueCap, CHAIN_EVAL_GRID);
        const uint32_t grid = groups * slices + 1u;
        // (one kernel per window dispatch: the kernels are instantiated, and laid out in the code object, in the order they appear here)
        if (split) by_window(h.genWin, [&](auto W) {
            constexpr int WIN = decltype(W)::value;
            LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, (chain_kernel<WIN, true>), grid, bs, h.d.lcgMul, h.d.lcgInc, h.d.gs, h.d.queue, h.chainGrans, h.d.chainSlots, h.d.queueCap, parity, slices, rec);
        });
        else by_window(h.genWin, [&](auto W) {
            constexpr int WIN = decltype(W)::value;
            LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, (chain_kernel<WIN, false>), grid, bs, h.d.lcgMul, h.d.lcgInc, h.d.gs, h.d.queue, h.chainGrans, h.d.chainSlots, h.d.queueCap, parity, slices, rec);
        });
#if defined(COGAPS_EMUL)
        if (split) RT_LAUNCH(chain_updates_kernel, 5, bs, s->stream, h.d.queue, h.chainGrans, h.d.chainSlots, h.d.queueCap, parity, rec);      // (test-only emulator: the updates behind the launch)
#endif
    }
    h.evalLaunches++;      // (one launch per batch: counted with the evaluation launches, as its time is)
}
static void launch_gen(cogaps_session *s, HostSampler &h)
{
    const int slot = timing_slot(s, h, EV_GEN, h.genLaunches);
    const SamplerDev CG_CONSTANT *rec = (const SamplerDev CG_CONSTANT *)h.dRecord;
    if (split_one_launch(h)) by_window(h.genWin, [&](auto W) {      // (the one-launch split evaluation's A*P updates: further workgroups of this launch)
        constexpr int WIN = decltype(W)::value;
        LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, gen_apply_kernel<WIN>, 1u + apply_grid(), WIN + 64, h.d.lcgMul, h.d.lcgInc, h.d.gs, (const unsigned long long *)h.d.eraseList, (const uint32_t *)h.d.queueUnits, h.d.eraseCap, h.d.queueCap, rec);
    });
    else by_window(h.genWin, [&](auto W) {
        constexpr int WIN = decltype(W)::value;
        LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, gen_kernel<WIN>, 1, WIN + 64, h.d.lcgMul, h.d.lcgInc, h.d.gs, (const unsigned long long *)h.d.eraseList, (const uint32_t *)h.d.queueUnits, h.d.eraseCap, h.d.queueCap, rec);
    });
    h.genLaunches++;
}
static void launch_eval(cogaps_session *s, HostSampler &h)
{
    const int slot = timing_slot(s, h, EV_EVAL, h.evalLaunches);
    const SamplerDev CG_CONSTANT *rec = (const SamplerDev CG_CONSTANT *)h.dRecord;      // (kept current by sync_record, as for the generator)
    if (h.d.seq) {
        // verification mode: one workgroup per proposal whatever the vector length, sums in the reference's order
        if (h.d.sparse) LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, eval_sparse_seq_kernel, std::min<uint32_t>(h.d.queueCap, SEQ_SPARSE_GRID), cogaps_sparse_width(h.d.N), h.d);
        else LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, eval_kernel<EVAL_SEQ>, std::min<uint32_t>(h.d.queueCap, 512u), EVAL_SEQ_BS, (const PropRec *)h.d.queue, (const GenScalars *)h.d.gs, h.d.queueCap, 1u, rec);
    } else if (h.d.sparse) {
        const uint32_t grid = std::min<uint32_t>(h.d.queueCap, 1024u);
        const uint32_t W = cogaps_sparse_width(h.d.N);
        if (h.d.Wn > W) LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, eval_sparse_kernel_wide, grid, W, (const PropRec *)h.d.queue, (const GenScalars *)h.d.gs, h.d.queueCap, rec);      // several rounds of flag words per vector
        else LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, eval_sparse_kernel, grid, W, (const PropRec *)h.d.queue, (const GenScalars *)h.d.gs, h.d.queueCap, rec);
    } else if (h.d.redW <= 1024u) {
        // one workgroup of W threads per proposal
        static const uint32_t fusedGrid = dev_env("COGAPS_FUSED_GRID") ? (uint32_t)atoi(dev_env("COGAPS_FUSED_GRID")) : 512u;      // dev builds: A/B of the launch size
        const uint32_t grid = std::min<uint32_t>(h.d.queueCap, fusedGrid);
        LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, eval_kernel<EVAL_FUSED>, grid, h.d.redW, (const PropRec *)h.d.queue, (const GenScalars *)h.d.gs, h.d.queueCap, 1u, rec);
    } else {
        // long data vectors: `slices` workgroups of `bs` threads per proposal, alpha kernel then apply kernel
        // (512 threads fill the machine a little better than 1024; at most 16 slices fit the partials record)
        uint32_t bs, slices; split_geometry(h, bs, slices);
        const uint32_t grid = std::min<uint32_t>(h.d.queueCap, split_per_wave(bs, slices)) * slices;
        if (split_one_launch(h)) {
            // one launch: the slices' totals reach the proposal's last slice workgroup inside it (eval_kernel.h, EVAL_DECIDE); the A*P updates
            // follow beside the next generator launch (launch_gen)
            LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, eval_kernel<EVAL_DECIDE>, grid, bs, (const PropRec *)h.d.queue, (const GenScalars *)h.d.gs, h.d.queueCap, slices, rec);
        } else {
            const int slot2 = slot >= 0 ? s->ev.take(EV_EVAL2, &h, h.updLaunches) : -1;
            LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, eval_kernel<EVAL_ALPHA>, grid, bs, (const PropRec *)h.d.queue, (const GenScalars *)h.d.gs, h.d.queueCap, slices, rec);
            LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot2, eval_kernel<EVAL_APPLY>, grid, bs, (const PropRec *)h.d.queue, (const GenScalars *)h.d.gs, h.d.queueCap, slices, rec);
        }
    }
    h.evalLaunches++;
}

// The chained launch serves the one-chain fused evaluation (dense model, product arithmetic) whose workgroups are at least as large as
// the generator's and small enough for the generator's register budget (chain_kernel.h); everything else keeps two launches per batch.
static bool chain_eligible(const cogaps_session *s, const HostSampler &h)
{
    // (a device with fewer compute units than the launch has workgroups -- a partitioned GPU -- would run them in turns, the generator
    // workgroup last: correct, and slower than two launches)
    if (s->noChain || h.d.seq || h.chainOff) return false;
    if (g_updatesRunning(s->p.device).load() > 1 && !s->forceChain) return false;      // (another update -- a session's or a batch's -- is in flight on this session's GPU: see g_updatesRunning)
    if (h.d.sparse)      // sparse model (round 5): a launch of 512-thread workgroups, the evaluation keeps the model's width inside it
        return CHAIN_MAX_THREADS >= h.genWin + 64u && (s->forceChain || s->computeUnits >= std::min<uint32_t>(h.d.queueCap, CHAIN_EVAL_GRID) + 1u);
    uint32_t block = h.d.redW;
    if (h.d.redW > 1024u) {      // split evaluation (round 5): workgroups of 512 threads, at most as many slices per proposal as the launch has evaluation workgroups
        uint32_t slices; split_geometry(h, block, slices);
        if (!split_one_launch(h) || slices > 16u || s->noChainSplit) return false;
    }
    // (the split form's update items wait for deciding workgroups of HIGHER index -- eval_chain_updates --: every workgroup must be resident,
    // so COGAPS_FORCE_CHAIN does not take it on a device with fewer compute units than the launch has workgroups; the fused form, whose
    // evaluation workgroups never wait, runs in turns there)
    const bool forced = s->forceChain && h.d.redW <= 1024u;
    return block <= (uint32_t)CHAIN_MAX_THREADS && block >= h.genWin + 64u
           && (forced || s->computeUnits >= std::min<uint32_t>(h.d.queueCap, CHAIN_EVAL_GRID) + 1u);
}
// one batch step: the chained launch, or a generator launch and an evaluation launch
static void launch_pair(cogaps_session *s, HostSampler &h)
{
    if (h.chain) launch_chain(s, h); else { launch_gen(s, h); launch_eval(s, h); }
}
// a sampler's (or a batch side's) generator window becomes `win`; the captured launches carry the window
static void set_window(uint32_t &genWin, GraphCache &graphs, uint32_t win) { if (win != genWin) { genWin = win; graphs.drop(); } }
// the generator window for the coming update (stepsPerBatch = 0: none measured yet) or the next one
static void retune_window(cogaps_session *s, HostSampler &h, float stepsPerBatch)
{
    const bool wideOk = h.chain && h.d.sparse != 0u;      // (the wide window: the chained sparse launch only; tests take it from the first update on)
    const uint32_t win = wideOk && s->testWideWindow ? (uint32_t)GEN_WIN_WIDE : gen_window_for(h.genWin, stepsPerBatch, wideOk);
    set_window(h.genWin, h.graphs, win);
}

// Launch clock of the chained launches (gaps_state.h): the ring holds {entry of the first workgroup, end of the generator workgroup} of
// every chained launch, slot = tag of the batch it evaluated.  Read back with the progress word of a chunk (at most 4096 launches, the ring
// holds 8192): the launches that evaluated batches (clockSeen, upTo] are complete -- the batch generated last is evaluated by the next
// launch, unless the update is over.
static void clock_collect(cogaps_session *s, HostSampler &h, uint64_t epoch, bool flushed)
{
    const uint64_t upTo = flushed ? epoch : (epoch ? epoch - 1u : 0u);
    if (!s->timing || !h.d.launchClock) { h.clockSeen = upTo; return; }
    if (upTo <= h.clockSeen) return;
    h.clockHost.resize(2u * GAPS_CLOCK_RING);
    rt_d2h(h.clockHost.data(), h.d.launchClock, sizeof(unsigned long long) * 2u * GAPS_CLOCK_RING, s->stream); rt_sync(s->stream);
    if (h.clockHist.empty()) h.clockHist.assign(2048, 0);
    if (h.periodHist.empty()) h.periodHist.assign(2048, 0);
    const uint64_t from = upTo - h.clockSeen > GAPS_CLOCK_RING ? upTo - GAPS_CLOCK_RING : h.clockSeen;
    for (uint64_t e = from + 1u; e <= upTo; ++e) {
        const unsigned long long b = h.clockHost[2u * (uint32_t)(e % GAPS_CLOCK_RING)], en = h.clockHost[2u * (uint32_t)(e % GAPS_CLOCK_RING) + 1u];
        if (!b || en <= b || en - b > 100000000ull) continue;      // (an entry whose halves belong to different launches: a stale slot)
        const double us = 0.01 * (double)(en - b);
        h.clockSumUs += us; h.clockN++;
        h.clockHist[std::min<size_t>(h.clockHist.size() - 1u, (size_t)(us * 10.0))]++;
        // the period to the next launch (the batch behind this one is evaluated by the very next launch on the stream; a chunk's last launch is
        // followed by the host's progress read-back: periods beyond 100 us are such seams and left out)
        if (e + 1u <= upTo) {
            const unsigned long long nb = h.clockHost[2u * (uint32_t)((e + 1u) % GAPS_CLOCK_RING)];
            if (nb > b && nb - b < 10000ull) {
                const double pu = 0.01 * (double)(nb - b);
                h.periodSumUs += pu; h.periodN++;
                h.periodHist[std::min<size_t>(h.periodHist.size() - 1u, (size_t)(pu * 10.0))]++;
            }
        }
    }
    h.clockSeen = upTo;
}

// A chained launch's generator gave up waiting for a decision (GAPS_ERR_SPIN; chain_kernel.h, chain_recover_kernel): the stream is idle
// (the error word was read behind a synchronisation), the evaluation workgroups of the failed launch have all ended.  The batch is
// completed on the device, the scalars are put back, and the sampler goes on with two launches per batch -- for the rest of the session:
// what kept a workgroup from being scheduled for two seconds (a foreign kernel holding compute units, a debugger) may well still be there.
// The split evaluation's chained form (not the default) is not recovered: its deciding workgroups wait as well.
static bool chain_recover(cogaps_session *s, HostSampler &h, uint32_t nSteps)
{
    if (!h.chain || h.d.seq || (!h.d.sparse && h.d.redW > 1024u)) return false;
    // launch k of the update (k = 0, 1, ...) has parity start ^ (k & 1), evaluates batch k and generates batch k + 1: the launch that gave up
    // had generated nothing, so it is launch number nBatches and the batch it was carrying out lies in the queue copy of its parity
    const uint32_t parityFail = (h.chainParityStart + s->hGs->nBatches) & 1u;
    const SamplerDev CG_CONSTANT *rec = (const SamplerDev CG_CONSTANT *)h.dRecord;
    RT_LAUNCH(chain_recover_kernel, 1, 256, s->stream, h.d.gs, (const PropRec *)(h.d.queue + (size_t)parityFail * h.d.queueCap), (const unsigned long long *)h.chainGrans, nSteps, rec);
    read_gs(s, h);
    if (s->hGs->error) return false;      // (a decision is still missing: the update cannot be completed)
    h.chain = false; h.chainOff = true; h.chainRecoveries++;
    retune_window(s, h, 0.f);      // (the wide window exists for the chained sparse launch only)
    return true;
}

// Arms sampler h for an update of n proposals: room for the atoms it can add, exactly n seeder outputs in the seed buffer
// (ProposalQueue.cpp:12-15; a failed attempt rolls the seeder back, Random.cpp:244-248) and its scalars `g` (as read back) reset for the
// update; the caller uploads them.  Returns the predicted proposals per batch: the previous update of this sampler is the best predictor.
static float begin_update(cogaps_session *s, HostSampler &h, GenScalars &g, uint32_t n, uint32_t traceCap)
{
    rt_owner_scope owner(&s->deviceBytes);      // (a batch steps its sessions from its own scope)
    grow_atoms(s, h, g.nAtoms + n + 1024u);
    if (h.seedCap < (size_t)n + 1) { rt_free(h.seeds); h.seedCap = (size_t)n * 5 / 4 + 1024; h.seeds = dalloc<uint64_t>(h.seedCap); }
    if (h.hSeedCap < (size_t)n + 1) { rt_free_host(h.hSeeds); h.hSeedCap = (size_t)n * 5 / 4 + 1024; h.hSeeds = (uint64_t *)rt_malloc_host(h.hSeedCap * 8); }
    seed_take(s, h.hSeeds, n);
    rt_h2d(h.seeds, h.hSeeds, (size_t)n * 8, s->stream);
    h.d.seeds = h.seeds;
    g.annealTemp = h.anneal;
    g.nSteps = n; g.nDone = 0; g.nBatches = 0; g.updateFlushed = 0; g.qlen = 0;
    g.traceOn = traceCap ? 1u : 0u; g.traceCount = 0; g.traceCap = traceCap; g.traceBatchCount = 0;
    h.updLaunches = 0;
    return h.stepsPerBatch > 1.f ? h.stepsPerBatch : (g.avgQueue > 1.f ? g.avgQueue : 1.f);
}
// the outcome of an update of n proposals, as the statistics and the sampler's next update read it
static void end_update(HostSampler &h, const GenScalars &g, uint32_t n)
{
    h.nAtoms = g.nAtoms; h.avgQueue = g.avgQueue; h.batches += g.nBatches;
    if (g.nBatches >= 8u) h.stepsPerBatch = (float)n / (float)g.nBatches;
}
// proposals per batch of the update so far, from its scalars as read back: the predictor of its next chunk (`avgq` while no batch is complete)
static float steps_per_batch(const GenScalars &g, float avgq) { return g.nBatches > 0 ? std::max(1.f, (float)g.nDone / (float)g.nBatches) : avgq; }
// chained launch: both parities of sampler h start an update from an empty queue (enqueued on `stream`; the caller waits for it)
static const ChainSlot g_emptySlots[2] = {{0u, 0u}, {0u, 0u}};
static void clear_chain_slots(const HostSampler &h, rt_stream_t stream) { rt_h2d(h.d.chainSlots, g_emptySlots, sizeof(g_emptySlots), stream); }
// A device error ends the update and with it the chain of session s: its state is not a state of the chain any more.  `chain`: the
// chain's index in its batch, or -1 for a one-chain session.
static int fail_device_error(cogaps_session *s, uint32_t code, char sampler, int chain, bool sequential)
{
    s->poisoned = true;
    return fail(std::string("device error code ") + std::to_string(code) + " in sampler " + sampler + (chain >= 0 ? " of chain " + std::to_string(chain) : std::string()) + (sequential ? " (sequential sampler)" : ""));
}
// Batch steps to enqueue before the next progress read-back, for C chains stepped together (g, nSteps, avgq: one per chain; done: the
// chains whose update is over, or null): what the slowest unfinished chain still needs.  A step enqueued past the end of an update is a
// wasted launch (two), a read-back one short pipeline bubble: the first chunk takes slightly fewer steps than the estimate says, the
// later ones converge on the tail.
static uint32_t chunk_size(uint32_t C, const GenScalars *g, const uint32_t *nSteps, const float *avgq, const char *done, bool first)
{
    uint32_t chunk = 0;
    for (uint32_t c = 0; c < C; ++c)
        if (!done || !done[c]) chunk = std::max(chunk, (uint32_t)((double)(nSteps[c] - g[c].nDone) / avgq[c] * (first ? 0.97 : 1.0)) + (first ? 0u : 2u));
    return std::min(std::max(chunk, 6u), 4096u);
}

// AsynchronousGibbsSampler::update (AsynchronousGibbsSampler.h:88-122): batches of generate + evaluate
// until nSteps proposals have been processed.  The number of batches is data dependent, so (generate,
// evaluate) pairs are enqueued in chunks and the generator's progress word is read back per chunk;
// pairs enqueued past the end are no-ops (the generator flushes the last erase cache and reports
// qlen = 0).
static int run_update_seq(cogaps_session *s, HostSampler &h, uint32_t nSteps);
static int run_update(cogaps_session *s, HostSampler &h, uint32_t nSteps, uint32_t traceCap)
{
    SamplerDev &d = h.d;
    if (s->poisoned) return fail("this session was ended by a device error in an earlier update; its chain cannot be continued");
    if (s->p.sampler == COGAPS_SAMPLER_SEQUENTIAL) {
        if (traceCap) return fail("proposal traces belong to the asynchronous sampler's queue: a sequential session has none");
        return run_update_seq(s, h, nSteps);
    }
    UpdateInFlight inFlight(s->p.device);
    read_gs(s, h);
    if (h.traceCap < traceCap) {
        rt_free(d.trace); rt_free(d.traceBatchNproc); rt_free(d.traceBatchQlen);
        d.trace = dalloc<PropRec>(traceCap); d.traceBatchNproc = dalloc<uint32_t>(traceCap); d.traceBatchQlen = dalloc<uint32_t>(traceCap);
        h.traceCap = traceCap;
    }
    float avgq = begin_update(s, h, *s->hGs, nSteps, traceCap);
    rt_h2d(d.gs, s->hGs, sizeof(GenScalars), s->stream);
    clear_chain_slots(h, s->stream);
    rt_sync(s->stream);
    if (nSteps == 0) return 0;
    sync_record(s, h);
    h.chain = chain_eligible(s, h);
    retune_window(s, h, 0.f);
    h.chainParityStart = h.chainParity;
    h.clockSeen = s->hGs->batchEpoch;      // (launch clock: the batches of this update carry the tags behind this one)
    bool firstChunk = true, topped = false;
    for (;;) {
        uint32_t plain = chunk_size(1, s->hGs, &nSteps, &avgq, nullptr, firstChunk);
        firstChunk = false;
        if (rt_graphs_supported() && !s->noGraph && !traceCap && plain >= GRAPH_PAIRS) {
            h.graphs.rekey(h.d);
            // HIP events cannot ride on replayed launches.  While timing is on, one replay of every chunk -- its position moves
            // through the chunk from update to update -- is issued as plain launches that carry events, so that the sample covers
            // the whole population of batches and not only the tail of each chunk (the remainder below).
            const uint32_t nRep = plain / GRAPH_PAIRS;
            const uint64_t rot = s->timing ? h.plainRotor++ : 0;                       // (every fourth chunk: the plain launches leave longer gaps than a replay)
            const uint32_t timedRep = (s->timing && (rot & 3u) == 0u) ? (uint32_t)(((rot >> 2) * 7u) % nRep) : 0xFFFFFFFFu;
            for (uint32_t r = 0; plain >= GRAPH_PAIRS; plain -= GRAPH_PAIRS, ++r) {
                if (r == timedRep) { for (uint32_t b = 0; b < GRAPH_PAIRS; ++b) { launch_pair(s, h); h.updLaunches++; } continue; }
                const bool timing = s->timing; s->timing = false;      // (a capture's launches are neither timed nor counted)
                const uint64_t g0 = h.genLaunches, e0 = h.evalLaunches;
                h.graphs.replay(s->stream, h.chain, h.chainParity, [&] { launch_pair(s, h); });
                s->timing = timing; h.genLaunches = g0 + (h.chain ? 0u : GRAPH_PAIRS); h.evalLaunches = e0 + GRAPH_PAIRS; h.updLaunches += GRAPH_PAIRS;
            }
        }
        for (uint32_t b = 0; b < plain; ++b) { launch_pair(s, h); h.updLaunches++; }
        if (!topped) { seed_top_up(s, &h == &s->A ? s->P : s->A); topped = true; }
        read_gs(s, h);
        timing_resolve(s, s->hGs->nBatches);
        if (h.chain) clock_collect(s, h, s->hGs->batchEpoch, s->hGs->updateFlushed != 0);
        if (s->hGs->error == GAPS_ERR_SPIN && chain_recover(s, h, nSteps)) continue;      // (the batch completed, the update goes on with two launches per batch)
        if (s->hGs->error) return fail_device_error(s, s->hGs->error, h.name, -1, false);
        if (s->hGs->updateFlushed) break;
        avgq = steps_per_batch(*s->hGs, avgq);
    }
    end_update(h, *s->hGs, nSteps);
    retune_window(s, h, h.stepsPerBatch);
    return 0;
}

// ---- the sequential sampler (seq_kernel.h): SingleThreadedGibbsSampler::update ------------------------------------------------------
// Arms sampler h for update(n): room for the atoms n births can add, progress and temperature in its scalars `g` (as read back; the
// caller uploads them).  No seeder output is taken: the sampler's one generator lives in g.qrng since the session's creation.
static void begin_update_seq(cogaps_session *s, HostSampler &h, GenScalars &g, uint32_t n)
{
    rt_owner_scope owner(&s->deviceBytes);
    grow_atoms(s, h, g.nAtoms + n + 1024u);
    g.annealTemp = h.anneal;
    g.nSteps = n; g.nDone = 0; g.nBatches = 0; g.updateFlushed = n == 0 ? 1u : 0u; g.qlen = 0;
    g.traceOn = 0; g.traceCount = 0; g.traceBatchCount = 0;
    h.updLaunches = 0;
}
// ... and its end, scalars `g` as read back behind the launches: an error, or an update the launches did not complete, ends the chain
// (`chain`: as for fail_device_error)
static int end_update_seq(cogaps_session *s, HostSampler &h, const GenScalars &g, int chain)
{
    h.chain = false;
    if (g.error || !g.updateFlushed) return fail_device_error(s, g.error, h.name, chain, true);
    h.nAtoms = g.nAtoms;      // (avgQueue stays 0: SingleThreadedGibbsSampler::getAverageQueueLength)
    return 0;
}
static uint32_t seq_launches(uint32_t nSteps) { return (nSteps + (uint32_t)SEQ_STEPS_PER_LAUNCH - 1u) / (uint32_t)SEQ_STEPS_PER_LAUNCH; }
// workgroup size of a sampler's sequential launch: the reduction's width up to 1024 threads; the verification mode's term scratch holds 256
static uint32_t seq_block(const SamplerDev &d) { return std::min<uint32_t>(d.redW, d.seq ? (uint32_t)EVAL_SEQ_BS : 1024u); }
// One workgroup runs the whole update, SEQ_STEPS_PER_LAUNCH steps per launch; the number of launches is known beforehand, so they are
// enqueued at once and the scalars are read back once.
static int run_update_seq(cogaps_session *s, HostSampler &h, uint32_t nSteps)
{
    SamplerDev &d = h.d;
    read_gs(s, h);
    begin_update_seq(s, h, *s->hGs, nSteps);
    rt_h2d(d.gs, s->hGs, sizeof(GenScalars), s->stream);
    rt_sync(s->stream);
    if (nSteps == 0) return 0;
    sync_record(s, h);
    const SamplerDev CG_CONSTANT *rec = (const SamplerDev CG_CONSTANT *)h.dRecord;
    const uint32_t bs = seq_block(d);
    for (uint32_t k = seq_launches(nSteps); k; --k) {
        const int slot = timing_slot(s, h, EV_EVAL, 0);
        if (d.seq) LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, seq_update_kernel<true>, 1, bs, rec);
        else LAUNCH_MAYBE_TIMED(s->stream, s->ev, slot, seq_update_kernel<false>, 1, bs, rec);
        h.evalLaunches++; h.updLaunches++;
    }
    read_gs(s, h);
    timing_resolve(s, ~0ull);
    return end_update_seq(s, h, *s->hGs, -1);
}
