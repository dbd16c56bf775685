// chain_batch.h -- the chain batch (cogaps_batch_*): host code only, a chapter of cogaps_hip.cpp, which includes it once, where the chapter
// used to stand -- inside its extern "C" block, after sampler_update.h (whose shared steps the batch's updates take), do_sync,
// iteration_head / iterate_tail / iteration_tail and set_position.  Not a stand-alone header.  As in sampler_update.h, the LAUNCH_* sites keep
// their order: the kernels are laid out in the code object in the order of their first use.
#pragma once

// ================================================================================================================================
// Batched multi-chain launches: C independent chains -- the subsets of a GWCoGAPS / scCoGAPS job that share one GPU (nSets > #GPUs),
// or replicas -- stepped in lock-step by ONE stream.  One chain alone alternates between a one-workgroup generator launch and an
// evaluation launch of a few hundred workgroups, both latency-bound; with C chains the generator grid is C workgroups and the
// evaluation grid C times as many, so a step of the batch costs about what a step of one chain costs and the evaluation kernels
// finally move enough rows per launch to approach the HBM roofline.  Every chain is the same chain it would be on its own, bit for
// bit (tests/test_gpu_parity.py::test_batched_chains_equal_single_sessions): the kernels are the one-chain kernels' bodies, fed from
// a device array of SamplerDev records instead of a by-value argument.
// ================================================================================================================================
struct cogaps_batch {
    std::vector<cogaps_session *> ss;
    rt_stream_t stream = rt_stream_t();
    SamplerDev *dev[2] = {nullptr, nullptr};            // [0] the A samplers' records, [1] the P samplers'
    std::vector<SamplerDev> host[2];                    // what the device arrays hold
    GraphCache graphs[2];
    // round 6: a side whose evaluation is the fused one steps as ONE chained launch for all chains (chain_kernel_multi) where every workgroup
    // of it is resident at once
    bool chain[2] = {false, false}; uint32_t chainParity[2] = {0, 0}; uint32_t chainWg[2] = {0, 0};
    GenScalars *hGs = nullptr;                          // pinned, [C]
    bool sparse = false; char fixed = 'N';
    uint64_t launches[2] = {0, 0};
    // HIP-event samples of the plain-launch remainder of each chunk
    bool timing = false; EventPool ev;
    double genMs[2] = {0, 0}, evalMs[2] = {0, 0}; uint64_t genTimed[2] = {0, 0}, evalTimed[2] = {0, 0};
    uint64_t ord = 0;
    uint32_t genWin[2] = {GEN_WIN, GEN_WIN};           // per side, from the chain with the longest batches
};

static HostSampler &bpick(cogaps_batch *b, uint32_t c, int w) { return w == 0 ? b->ss[c]->A : b->ss[c]->P; }

// the scalars of sampler w of every chain, read back behind everything the stream holds
static void batch_read_gs(cogaps_batch *b, int w)
{
    for (uint32_t c = 0; c < (uint32_t)b->ss.size(); ++c) rt_d2h(&b->hGs[c], bpick(b, c, w).d.gs, sizeof(GenScalars), b->stream);
    rt_sync(b->stream);
}
// the records the kernels read: re-uploaded when a pointer in one of them changed (atom tables regrown, seed buffer moved);
// the captured graph stays valid -- its kernels' arguments are the array's address and the launch geometry.  Waits for the stream: the
// scalars the caller uploaded before are in place too.
static void batch_sync_records(cogaps_batch *b, int w)
{
    bool changed = false;
    for (uint32_t c = 0; c < (uint32_t)b->ss.size(); ++c) if (memcmp(&b->host[w][c], &bpick(b, c, w).d, sizeof(SamplerDev)) != 0) { b->host[w][c] = bpick(b, c, w).d; changed = true; }
    if (changed) rt_h2d(b->dev[w], b->host[w].data(), b->ss.size() * sizeof(SamplerDev), b->stream);
    rt_sync(b->stream);
}

// launch geometry shared by the chains of a batch (checked at creation: equal reduction widths and slice counts)
struct MultiGeom { uint32_t block, slices, wgPerChain; bool fused; };
static MultiGeom multi_geom(cogaps_batch *b, int w)
{
    const SamplerDev &d = bpick(b, 0, w).d;
    const uint32_t C = (uint32_t)b->ss.size();
    uint32_t minCap = 0xFFFFFFFFu; for (uint32_t c = 0; c < C; ++c) minCap = std::min(minCap, bpick(b, c, w).d.queueCap);
    MultiGeom g;
    if (b->sparse) { g.block = cogaps_sparse_width(d.N); g.slices = 1; g.fused = true; g.wgPerChain = std::min<uint32_t>(minCap, std::max<uint32_t>(64u, 1024u / C)); return g; }
    if (d.redW <= 1024u) { g.block = d.redW; g.slices = 1; g.fused = true; g.wgPerChain = std::min<uint32_t>(minCap, std::max<uint32_t>(64u, 2048u / C)); return g; }
    g.fused = false;
    split_geometry(bpick(b, 0, w), g.block, g.slices);
    g.wgPerChain = std::min<uint32_t>(minCap, std::max<uint32_t>(4u, (2u * split_per_wave(g.block, g.slices)) / C + 1u)) * g.slices;
    return g;
}
// The chained form for a batch (chain_kernel.h, chain_kernel_multi): the dense model's fused evaluation (workgroups as large as the generator's),
// every workgroup of the launch resident at once -- compute units / chains per chain -- and no other update in flight on the GPU.  Taken
// for up to FOUR chains (64 workgroups each on the MI355X): measured +9 % at two chains, +2 % at four, -7 % at eight, -20 % at sixteen
// (profiles/r06_ab_chained_batch.txt) -- a chain's evaluation workgroups are alone on their compute units (the generator's LDS), where the
// batched evaluation launch packs three per unit.  COGAPS_NO_CHAIN switches it off (A/B, equality tests).
static uint32_t multi_chain_wg(cogaps_batch *b, int w, const MultiGeom &g)
{
    const cogaps_session *s0 = b->ss[0];
    const uint32_t C = (uint32_t)b->ss.size();
    if (s0->noChain || b->sparse || !g.fused || g.block > (uint32_t)CHAIN_MAX_THREADS || g.block < b->genWin[w] + 64u) return 0u;
    if (g_updatesRunning(s0->p.device).load() > 1) return 0u;
    for (cogaps_session *s : b->ss) if ((w == 0 ? s->A : s->P).d.seq) return 0u;
    const uint32_t perChain = std::min<uint32_t>(s0->computeUnits / C, CHAIN_EVAL_GRID + 1u);
    return perChain >= (CHAIN_EVAL_GRID >= 16u ? 64u : 3u) ? perChain : 0u;      // (the test-only emulator's launches have seven evaluation workgroups)
}
static void multi_launch_pair(cogaps_batch *b, int w, const MultiGeom &g, int slotGen, int slotEval, int slotEval2)
{
    const uint32_t C = (uint32_t)b->ss.size();
    const SamplerDev CG_CONSTANT *arr = (const SamplerDev CG_CONSTANT *)b->dev[w];
    if (b->chain[w]) {
        const uint32_t parity = b->chainParity[w]; b->chainParity[w] ^= 1u;
        by_window(b->genWin[w], [&](auto W) {
            constexpr int WIN = decltype(W)::value;
            LAUNCH_MAYBE_TIMED(b->stream, b->ev, slotEval, chain_kernel_multi<WIN>, C * b->chainWg[w], g.block, arr, parity, b->chainWg[w]);
        });
        b->launches[w]++;
        return;
    }
    by_window(b->genWin[w], [&](auto W) {
        constexpr int WIN = decltype(W)::value;
        LAUNCH_MAYBE_TIMED(b->stream, b->ev, slotGen, gen_kernel_multi<WIN>, C, WIN + 64, arr);
    });
    if (b->sparse) LAUNCH_MAYBE_TIMED(b->stream, b->ev, slotEval, eval_sparse_kernel_multi, C * g.wgPerChain, g.block, arr, g.wgPerChain);
    else if (g.fused) LAUNCH_MAYBE_TIMED(b->stream, b->ev, slotEval, eval_kernel_multi<EVAL_FUSED>, C * g.wgPerChain, g.block, arr, 1u, g.wgPerChain);
    else {
        LAUNCH_MAYBE_TIMED(b->stream, b->ev, slotEval, eval_kernel_multi<EVAL_ALPHA>, C * g.wgPerChain, g.block, arr, g.slices, g.wgPerChain);
        LAUNCH_MAYBE_TIMED(b->stream, b->ev, slotEval2, eval_kernel_multi<EVAL_APPLY>, C * g.wgPerChain, g.block, arr, g.slices, g.wgPerChain);
    }
    b->launches[w]++;
}

// AsynchronousGibbsSampler::update of sampler `w` (0 = A, 1 = P) of every chain, nSteps[c] proposals each
static int run_update_multi_seq(cogaps_batch *b, int w, const std::vector<uint32_t> &nSteps);
static int run_update_multi(cogaps_batch *b, int w, const std::vector<uint32_t> &nSteps)
{
    const uint32_t C = (uint32_t)b->ss.size();
    if (b->ss[0]->p.sampler == COGAPS_SAMPLER_SEQUENTIAL) return run_update_multi_seq(b, w, nSteps);
    UpdateInFlight inFlight(b->ss[0]->p.device);      // (a one-chain session stepped beside the batch on the same GPU keeps two launches per batch meanwhile)
    rt_alloc_scope allocOn(b->stream);
    batch_read_gs(b, w);
    std::vector<float> avgq(C); std::vector<char> done(C, 0);
    for (uint32_t c = 0; c < C; ++c) {
        HostSampler &h = bpick(b, c, w); GenScalars &g = b->hGs[c];
        avgq[c] = begin_update(b->ss[c], h, g, nSteps[c], 0);
        // update(0) -- a Poisson draw of 0 has probability e^-10 while a chain holds at most 10 atoms -- is a no-op in the reference
        // (AsynchronousGibbsSampler.h:94: the loop body never runs): the chain is done before the first launch and the lock-stepped
        // batch never waits for it (its generator workgroup sees nDone >= nSteps and leaves at once)
        if (nSteps[c] == 0) { g.updateFlushed = 1; done[c] = 1; }
        rt_h2d(h.d.gs, &g, sizeof(GenScalars), b->stream);
    }
    if (std::all_of(done.begin(), done.end(), [](char d) { return d != 0; })) { rt_sync(b->stream); return 0; }
    batch_sync_records(b, w);
    const MultiGeom geo = multi_geom(b, w);
    b->chainWg[w] = multi_chain_wg(b, w, geo);
    b->chain[w] = b->chainWg[w] != 0u;
    for (uint32_t c = 0; c < C; ++c) bpick(b, c, w).chain = b->chain[w];      // (cogaps_session_chained reports what runs)
    if (b->chain[w]) {      // both parities of every chain start from an empty queue
        for (uint32_t c = 0; c < C; ++c) clear_chain_slots(bpick(b, c, w), b->stream);
        rt_sync(b->stream);
    }
    bool first = true, topped = false;
    for (;;) {
        uint32_t plain = chunk_size(C, b->hGs, nSteps.data(), avgq.data(), done.data(), first);
        first = false;
        if (rt_graphs_supported() && !b->ss[0]->noGraph)
            for (; plain >= GRAPH_PAIRS; plain -= GRAPH_PAIRS) {
                const uint64_t l0 = b->launches[w];      // (the captured launches are not counted)
                b->graphs[w].replay(b->stream, b->chain[w], b->chainParity[w], [&] { multi_launch_pair(b, w, geo, -1, -1, -1); });
                b->launches[w] = l0 + GRAPH_PAIRS; b->ord += GRAPH_PAIRS;
            }
        for (uint32_t k = 0; k < plain; ++k) {
            int sg = -1, se = -1, se2 = -1;
            if (b->timing && (b->ord % 4u) == 0u && b->ev.room(3)) {
                if (b->chain[w]) se = b->ev.take(EV_EVAL);      // (one launch per step: timed as the evaluation launch, as the one-chain form's is)
                else { sg = b->ev.take(EV_GEN); se = b->ev.take(EV_EVAL); if (!geo.fused) se2 = b->ev.take(EV_EVAL2); }
            }
            multi_launch_pair(b, w, geo, sg, se, se2);
            b->ord++;
        }
        if (!topped) { for (uint32_t c = 0; c < C; ++c) seed_top_up(b->ss[c], bpick(b, c, 1 - w)); topped = true; }
        batch_read_gs(b, w);
        b->ev.drain([&](const EvSample &e, float ms) {          // (sampled launches near the end of a chunk: most chains still have work there)
            if (e.kind == EV_GEN) { b->genMs[w] += ms; b->genTimed[w]++; } else { b->evalMs[w] += ms; if (e.kind == EV_EVAL) b->evalTimed[w]++; }
        });
        bool all = true;
        for (uint32_t c = 0; c < C; ++c) {
            const GenScalars &g = b->hGs[c];
            if (g.error) return fail_device_error(b->ss[c], g.error, w ? 'P' : 'A', (int)c, false);
            if (g.updateFlushed) done[c] = 1; else all = false;
            avgq[c] = steps_per_batch(g, avgq[c]);
        }
        if (all) break;
    }
    float spb = 0.f;
    for (uint32_t c = 0; c < C; ++c) { end_update(bpick(b, c, w), b->hGs[c], nSteps[c]); spb = std::max(spb, bpick(b, c, w).stepsPerBatch); }
    set_window(b->genWin[w], b->graphs[w], gen_window_for(b->genWin[w], spb));
    return 0;
}

// The sequential sampler's update of sampler `w` of every chain: ONE launch of a workgroup per chain per SEQ_STEPS_PER_LAUNCH steps of the
// longest update; a chain whose update is over leaves at once and nobody waits for anybody.
static int run_update_multi_seq(cogaps_batch *b, int w, const std::vector<uint32_t> &nSteps)
{
    const uint32_t C = (uint32_t)b->ss.size();
    rt_alloc_scope allocOn(b->stream);
    batch_read_gs(b, w);
    uint32_t longest = 0;
    for (uint32_t c = 0; c < C; ++c) {
        HostSampler &h = bpick(b, c, w);
        begin_update_seq(b->ss[c], h, b->hGs[c], nSteps[c]);
        rt_h2d(h.d.gs, &b->hGs[c], sizeof(GenScalars), b->stream);
        longest = std::max(longest, nSteps[c]);
    }
    batch_sync_records(b, w);
    if (longest == 0) return 0;
    const SamplerDev CG_CONSTANT *arr = (const SamplerDev CG_CONSTANT *)b->dev[w];
    const uint32_t bs = seq_block(bpick(b, 0, w).d);      // (equal reduction widths: checked at the batch's creation)
    for (uint32_t k = seq_launches(longest); k; --k) {
        const int slot = (b->timing && b->ev.room(1)) ? b->ev.take(EV_EVAL) : -1;
        LAUNCH_MAYBE_TIMED(b->stream, b->ev, slot, seq_update_kernel_multi, C, bs, arr);
        b->launches[w]++; b->ord++;
    }
    batch_read_gs(b, w);
    b->ev.drain([&](const EvSample &, float ms) { b->evalMs[w] += ms; b->evalTimed[w]++; });
    for (uint32_t c = 0; c < C; ++c)
        if (end_update_seq(b->ss[c], bpick(b, c, w), b->hGs[c], (int)c)) return 1;
    return 0;
}

cogaps_batch *cogaps_batch_create(cogaps_session **sessions, uint32_t n)
{
    cogaps_batch *b = nullptr;
    try {
        if (!sessions || n == 0) { fail("no sessions"); return nullptr; }
        const cogaps_session *s0 = sessions[0];
        for (uint32_t c = 0; c < n; ++c) {
            const cogaps_session *s = sessions[c];
            if (!s) { fail("null session"); return nullptr; }
            if (!s->ownsStream) { fail("a session can be in one batch only"); return nullptr; }
            if (s->A.d.seq || s0->A.d.seq) { fail("the verification mode runs one chain at a time"); return nullptr; }
            if (s->p.sampler != s0->p.sampler) { fail("the sessions of a batch must share the sampler: sequential and asynchronous chains cannot be mixed"); return nullptr; }
            // one launch geometry for all chains: the same model, reduction widths and slice counts (subsets of one job have them)
            if (s->p.useSparseOptimization != s0->p.useSparseOptimization || s->p.whichMatrixFixed != s0->p.whichMatrixFixed || s->p.device != s0->p.device
                || s->A.d.redW != s0->A.d.redW || s->P.d.redW != s0->P.d.redW || ((s->A.d.Npad >> 2) + 511u) / 512u != ((s0->A.d.Npad >> 2) + 511u) / 512u
                || ((s->P.d.Npad >> 2) + 511u) / 512u != ((s0->P.d.Npad >> 2) + 511u) / 512u
                || (s->p.useSparseOptimization && (cogaps_sparse_width(s->A.d.N) != cogaps_sparse_width(s0->A.d.N) || cogaps_sparse_width(s->P.d.N) != cogaps_sparse_width(s0->P.d.N))))      // (the dense kernels never see the sparse model's workgroup width: subsets of 4095 and 4096 rows share a batch)
            { fail("the sessions of a batch must share the model, the fixed matrix, the device and the evaluation launch shape (equal reduction widths)"); return nullptr; }
        }
        rt_set_device(s0->p.device);
        b = new cogaps_batch();
        b->ss.assign(sessions, sessions + n);
        b->sparse = s0->p.useSparseOptimization != 0; b->fixed = s0->p.whichMatrixFixed;
        b->stream = rt_stream_create();
        rt_alloc_scope allocOn(b->stream);
        // everything that can fail is done BEFORE a session is touched: a failed creation leaves every session as it was
        b->hGs = (GenScalars *)rt_malloc_host(sizeof(GenScalars) * n);
        for (int w = 0; w < 2; ++w) { b->dev[w] = dalloc<SamplerDev>(n); b->host[w].resize(n); memset(b->host[w].data(), 0, sizeof(SamplerDev) * n); }
        for (cogaps_session *s : b->ss) rt_sync(s->stream);
        for (cogaps_session *s : b->ss) {      // from here on the sessions run on the batch's stream, one after the other (nothing below throws)
            s->A.graphs.drop(); s->P.graphs.drop();
            rt_stream_destroy(s->stream); s->stream = b->stream; s->ownsStream = false; s->A.chain = false; s->P.chain = false;      // (the batched launches keep two launches per step: cogaps_session_chained reports what runs)
        }
        return b;
    } catch (const std::exception &e) {
        fail_exc(e);
        if (b) {
            for (int w = 0; w < 2; ++w) rt_free(b->dev[w]);
            rt_free_host(b->hGs);
            if (b->stream) rt_stream_destroy(b->stream);
            delete b;
        }
        return nullptr;
    }
}

void cogaps_batch_destroy(cogaps_batch *b)
{
    if (!b) return;
    try { rt_sync(b->stream); } catch (...) { }
    for (cogaps_session *s : b->ss) { try { s->stream = rt_stream_create(); s->ownsStream = true; } catch (...) { } }      // the sessions outlive the batch
    for (int w = 0; w < 2; ++w) { b->graphs[w].drop(); rt_free(b->dev[w]); }
    rt_free_host(b->hGs);
    rt_stream_destroy(b->stream);
    delete b;
}

// runOnePhase for every chain of the batch: iterations [firstIter, firstIter + n) of `phase`; updates[c] += proposals of chain c
int cogaps_batch_run_iterations(cogaps_batch *b, int phase, uint32_t firstIter, uint32_t n, uint64_t *updates)
{
    try {
        rt_set_device(b->ss[0]->p.device);
        rt_alloc_scope allocOn(b->stream);
        const uint32_t C = (uint32_t)b->ss.size();
        for (uint32_t c = 0; c < C; ++c)
            if (b->ss[c]->poisoned) return fail("chain " + std::to_string(c) + " of this batch was ended by a device error in an earlier update; the batch cannot be continued");
        const double t0 = now_s();
        for (cogaps_session *s : b->ss)
            if (s->p.printMessages && firstIter == 0 && n > 0) { printf(phase == 1 ? "-- Equilibration Phase --\n" : "-- Sampling Phase --\n"); fflush(stdout); }
        std::vector<uint32_t> nA(C), nP(C);
        const char f = b->fixed;
        for (uint32_t it = firstIter; it < firstIter + n; ++it) {
            for (uint32_t c = 0; c < C; ++c)
                if (iteration_head(b->ss[c], phase, it, &nA[c], &nP[c])) return 1;
            // updateSampler (GapsRunner.cpp:201-222), every chain at once
            if (f != 'A') { if (run_update_multi(b, 0, nA)) return 1; if (f != 'P') for (cogaps_session *s : b->ss) do_sync(s, s->P, s->A); }
            if (f != 'P') { if (run_update_multi(b, 1, nP)) return 1; if (f != 'A') for (cogaps_session *s : b->ss) do_sync(s, s->A, s->P); }
            for (uint32_t c = 0; c < C; ++c) {
                iterate_tail(b->ss[c], nA[c], nP[c], phase == 2);
                if (updates) updates[c] += (uint64_t)nA[c] + nP[c];
                if (iteration_tail(b->ss[c], phase, it)) return 1;
            }
            for (cogaps_session *s : b->ss) set_position(s, phase, it + 1u);
        }
        rt_sync(b->stream);
        const double dt = now_s() - t0;
        for (cogaps_session *s : b->ss) s->samplerSeconds += dt;
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

int cogaps_batch_set_timing(cogaps_batch *b, int on)
{
    try {
        if (on) b->ev.create(1536);
        if (on && !b->timing) for (int w = 0; w < 2; ++w) { b->genMs[w] = b->evalMs[w] = 0; b->genTimed[w] = b->evalTimed[w] = 0; }
        b->timing = on != 0;
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// mean HIP-event time of the sampled batched launches since cogaps_batch_set_timing(1), per sampler side (0 = A, 1 = P); the
// algorithmic bytes and proposal counts are the sessions' own (cogaps_session_perf_sampler)
int cogaps_batch_perf(cogaps_batch *b, int side, double *genUs, double *evalUs, uint64_t *sampled, uint64_t *launches)
{
    if (side < 0 || side > 1) return fail("side must be 0 (A) or 1 (P)");
    if (genUs) *genUs = b->genTimed[side] ? 1e3 * b->genMs[side] / (double)b->genTimed[side] : 0.0;
    if (evalUs) *evalUs = b->evalTimed[side] ? 1e3 * b->evalMs[side] / (double)b->evalTimed[side] : 0.0;
    if (sampled) *sampled = b->evalTimed[side];
    if (launches) *launches = b->launches[side];
    return 0;
}
