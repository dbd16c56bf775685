// session_state.h -- the library's own state file (cogaps_session_save_state / _load_state, cogaps_session_position, the data digest):
// host code only, a chapter of cogaps_hip.cpp, which includes it once, where the chapter used to stand -- inside its extern "C" block,
// after cogaps_session, fail, dalloc, now_s, SESSION_TRY / SESSION_END, read_gs and grow_atoms (sampler_update.h) and do_sync, which it
// takes from there; cogaps_session_run_to_end, beside the other run loops, takes state_refusal.  Not a stand-alone header.  Steps written
// here once, because a save and a load must agree exactly: which samplers take part (state_samplers), the host arrays of a state
// (StateHostArrays), every section with its size (state_sections), a piece of a device section through the staging buffer (state_piece;
// the pieces themselves: state_file.h), the packed-value count (packed_value_count), how a fingerprint word reads (FP_WORDS).
#pragma once

// ================================================================================================================================
// The library's own STATE FILE: what changes while a chain runs, saved between two iterations and loaded into a session created the
// ordinary way from the same data and parameters -- the resumed chain is the uninterrupted chain, bit for bit.  (Not the reference's
// Archive checkpoints: cogaps_checkpoints_enabled stays 0.)  Container: state_file.h.  Sections:
//   fingerprint  what a file and a session must agree on, as 64-bit words in the order of FP_WORDS
//   meta         StateMeta: position, host generators, counters, times, the lengths of the variable sections
//   per session  the seeder's look-ahead, the four statistics accumulators, the PUMP matrix, snapshots, the three histories
//   per sampler that runs (a fixed matrix's sampler keeps what creation gave it): GenScalars, the factor matrix, colPos, the atomic
//                domain -- atom records up to the handle high-water mark, the index vector up to the atom count, the free-handle stack up
//                to its depth, bin heads, occupancy bitmaps --, for the sparse model the row copy, its flags and the lookup tables
//   A*P          the dense model's cache of ONE sampler: P's, or A's when P is fixed; without a fixed matrix A's is its transpose (do_sync)
// Not in the file, because the next batch cannot see them: the conflict stamps and queued-move destinations (valid for their own batch
// epoch only; a load clears them), the queue, the erase cache (empty between updates), hand-over granules; and nothing of the data, the
// lookup tables or a capacity.  Launch form -- chained or not, graphs, generator window, a batch -- is the loading session's own.
// ================================================================================================================================
// The fingerprint's words, in order: what a message calls each and how its value reads there -- a number, the bits of a float, a
// letter, a hash
enum FpKind { FP_NUMBER, FP_FLOAT, FP_LETTER, FP_HASH };
static const struct { const char *name; FpKind kind; } FP_WORDS[] = {
    {"model (useSparseOptimization)", FP_NUMBER}, {"nGenes", FP_NUMBER}, {"nSamples", FP_NUMBER}, {"nPatterns", FP_NUMBER}, {"seed", FP_NUMBER},
    {"nIterations", FP_NUMBER}, {"alphaA", FP_FLOAT}, {"alphaP", FP_FLOAT}, {"maxGibbsMassA", FP_FLOAT}, {"maxGibbsMassP", FP_FLOAT},
    {"outputFrequency", FP_NUMBER}, {"snapshotFrequency", FP_NUMBER}, {"snapshotPhase", FP_NUMBER}, {"takePumpSamples", FP_NUMBER},
    {"pumpThreshold", FP_NUMBER}, {"whichMatrixFixed", FP_LETTER}, {"fixedPatterns", FP_HASH}, {"reductionMode", FP_NUMBER}, {"mathMode", FP_NUMBER},
    {"lambda of A (data)", FP_FLOAT}, {"lambda of P (data)", FP_FLOAT}, {"maxGibbsMass / lambda of A (data)", FP_FLOAT},
    {"maxGibbsMass / lambda of P (data)", FP_FLOAT}, {"dataSparsity of A (data)", FP_FLOAT}, {"dataSparsity of P (data)", FP_FLOAT},
    {"number of packed values (data)", FP_NUMBER}, {"data digest (the data differ)", FP_HASH} };
static const int FP_N = (int)(sizeof(FP_WORDS) / sizeof(FP_WORDS[0]));
struct StateMeta {
    uint32_t phase, nextIter;
    uint64_t seeder0, seeder1, runnerRng, totalUpdates;
    double samplerSeconds, elapsedSeconds;
    uint32_t statUpdates, pumpUpdates, nSnap[2], nHistory, genScalarsBytes;
    uint64_t nSeedFifo;
    struct { uint32_t present, nAtoms; float avgQueue, anneal; } samp[2];
};
enum { SEC_FINGERPRINT = 1, SEC_META, SEC_SEEDFIFO, SEC_ASUM, SEC_ASQ, SEC_PSUM, SEC_PSQ, SEC_PUMP, SEC_SNAP_A_EQ, SEC_SNAP_P_EQ, SEC_SNAP_A_SA, SEC_SNAP_P_SA,
       SEC_CHISQ_HIST, SEC_ATOM_HIST_A, SEC_ATOM_HIST_P,
       SEC_SAMPLER = 0x100,      // + 0x100 * (0: A, 1: P) + one of:
       SS_GS = 0, SS_MAT, SS_COLPOS, SS_ATOMS, SS_VEC, SS_FREE, SS_BINHEAD, SS_BITS0, SS_BITS1, SS_BITS2, SS_AP, SS_ROWS, SS_MFLAGS, SS_Z1, SS_Z2 };
static const size_t STATE_STAGING_BYTES = (size_t)4 << 20;      // device arrays pass through one pinned buffer of this size

static float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
// the number of packed values of the sparse model's data, read back from the end of A's pointers (the dense model: 0)
static uint32_t packed_value_count(cogaps_session *s)
{
    const SamplerDev &d = s->A.d;
    uint32_t nVals = 0;
    if (d.sparse) { rt_d2h(&nVals, d.dptr + d.M, 4, s->stream); rt_sync(s->stream); }
    return nVals;
}
// the data digest (state_digest.h), computed once per session, at its first save or load; its scratch word is not the session's
static uint64_t data_digest(cogaps_session *s)
{
    if (s->digestValid) return s->dataDigest;
    const SamplerDev &d = s->A.d;
    rt_owner_scope notTheSessions(nullptr);
    unsigned long long *out = dalloc<unsigned long long>(1);
    try {
        const uint32_t nVals = packed_value_count(s);
        const unsigned long long rows = d.sparse ? 1ull : d.M, nFlags = d.sparse ? (unsigned long long)d.M * d.Wn : 0ull;
        const uint32_t N = d.sparse ? nVals : d.N, stride = d.sparse ? nVals : d.Npad;
        const unsigned long long items = std::max<unsigned long long>(rows * N, nFlags);
        const uint32_t grid = (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>((items + 4u * DIGEST_BS - 1u) / (4u * DIGEST_BS), 2048u));
        RT_LAUNCH(state_digest_kernel, grid, DIGEST_BS, s->stream, (const uint32_t *)(d.sparse ? (const void *)d.dvals : (const void *)d.D), rows, N, stride,
                  (const unsigned long long *)d.dflags, nFlags, out);
        unsigned long long v = 0; rt_d2h(&v, out, 8, s->stream); rt_sync(s->stream);
        s->dataDigest = v; s->digestValid = true;
    } catch (...) { rt_free(out); throw; }
    rt_free(out);
    return s->dataDigest;
}
static void state_fingerprint(cogaps_session *s, uint64_t *fp)
{
    const cogaps_params &p = s->p;
    const bool dense = !p.useSparseOptimization;
    const uint64_t v[] = {
        (uint64_t)!dense, s->nGenes, s->nSamples, s->K, p.seed,
        p.nIterations, gm_f2u(p.alphaA), gm_f2u(p.alphaP), gm_f2u(p.maxGibbsMassA), gm_f2u(p.maxGibbsMassP),
        p.outputFrequency, p.snapshotFrequency, (uint64_t)(uint32_t)p.snapshotPhase, (uint64_t)(p.takePumpSamples != 0),
        (uint64_t)(uint32_t)p.pumpThreshold, (uint64_t)(unsigned char)p.whichMatrixFixed, s->fixedHash, (uint64_t)(uint32_t)p.reductionMode, (uint64_t)(uint32_t)p.mathMode,
        gm_f2u(s->A.d.lambda), gm_f2u(s->P.d.lambda), gm_f2u(s->A.d.maxGibbsMass),
        gm_f2u(s->P.d.maxGibbsMass), dense ? gm_f2u(s->A.dataSparsity) : 0u, dense ? gm_f2u(s->P.dataSparsity) : 0u,
        packed_value_count(s), data_digest(s) };
    static_assert(sizeof(v) / sizeof(v[0]) == (size_t)FP_N, "one value per word of FP_WORDS, line for line");
    memcpy(fp, v, sizeof(v));
}
// how a differing fingerprint word reads in a message
static std::string fp_text(int i, uint64_t v)
{
    char b[64];
    switch (FP_WORDS[i].kind) {
    case FP_FLOAT: snprintf(b, sizeof(b), "%.9g", (double)f_of((uint32_t)v)); return b;
    case FP_LETTER: return std::string(1, (char)v);
    case FP_HASH: snprintf(b, sizeof(b), "%016llx", (unsigned long long)v); return b;
    default: return std::to_string(v);
    }
}
// Which samplers take part in a state -- a fixed matrix's sampler keeps what creation gave it -- and which ONE of them owns the A*P cache
// the dense model's state holds: P, or A when P is fixed
struct StateSamplers { HostSampler *hs[2]; uint32_t present[2]; int apOwner; };
static StateSamplers state_samplers(cogaps_session *s)
{
    const char fixed = s->p.whichMatrixFixed;
    return {{&s->A, &s->P}, {fixed == 'A' ? 0u : 1u, fixed == 'P' ? 0u : 1u}, fixed == 'P' ? 0 : 1};
}
// host arrays of a state: a save points at the session's own vectors (the seeder's look-ahead from its head on), a load at temporaries of
// the lengths the file's meta section states
struct StateHostArrays {
    uint64_t *fifo; float *snapA[2], *snapP[2], *chisq; uint32_t *histA, *histP;
    StateHostArrays(std::vector<uint64_t> &fifo_, size_t fifoHead, std::vector<float> *snapA_, std::vector<float> *snapP_, std::vector<float> &chisq_,
                    std::vector<uint32_t> &histA_, std::vector<uint32_t> &histP_)
        : fifo(fifo_.data() + fifoHead), snapA{snapA_[0].data(), snapA_[1].data()}, snapP{snapP_[0].data(), snapP_[1].data()}, chisq(chisq_.data()),
          histA(histA_.data()), histP(histP_.data()) {}
};
// Every section of the session's state with its size, in file order: the one list a save writes and a load expects.  gs: the samplers'
// scalars (a save's: just read back; a load's: the file's), which size the atomic domain's sections.
static std::vector<cgstate::Section> state_sections(cogaps_session *s, uint64_t *fp, StateMeta *meta, GenScalars *gs, const StateHostArrays &ha)
{
    std::vector<cgstate::Section> v;
    auto host = [&](uint32_t id, void *p, uint64_t bytes) { static char none; v.push_back({id, bytes ? p : (void *)&none, nullptr, bytes}); };
    auto dev = [&](uint32_t id, void *p, uint64_t bytes) { v.push_back({id, nullptr, p, bytes}); };
    const uint64_t K = s->K, na = (uint64_t)s->nGenes * K, np_ = (uint64_t)s->nSamples * K, nh = (uint64_t)meta->nHistory * 4;
    host(SEC_FINGERPRINT, fp, (uint64_t)FP_N * 8); host(SEC_META, meta, sizeof(StateMeta));
    host(SEC_SEEDFIFO, ha.fifo, meta->nSeedFifo * 8);
    dev(SEC_ASUM, s->Asum, K * s->A.d.Mpad * 4); dev(SEC_ASQ, s->Asq, K * s->A.d.Mpad * 4);
    dev(SEC_PSUM, s->Psum, K * s->P.d.Mpad * 4); dev(SEC_PSQ, s->Psq, K * s->P.d.Mpad * 4);
    dev(SEC_PUMP, s->pump, na * 4);
    host(SEC_SNAP_A_EQ, ha.snapA[0], meta->nSnap[0] * na * 4); host(SEC_SNAP_P_EQ, ha.snapP[0], meta->nSnap[0] * np_ * 4);
    host(SEC_SNAP_A_SA, ha.snapA[1], meta->nSnap[1] * na * 4); host(SEC_SNAP_P_SA, ha.snapP[1], meta->nSnap[1] * np_ * 4);
    host(SEC_CHISQ_HIST, ha.chisq, nh); host(SEC_ATOM_HIST_A, ha.histA, nh); host(SEC_ATOM_HIST_P, ha.histP, nh);
    const StateSamplers st = state_samplers(s);
    for (int w = 0; w < 2; ++w) {
        if (!st.present[w]) continue;
        const SamplerDev &d = st.hs[w]->d; const GenScalars &g = gs[w];
        const uint32_t base = SEC_SAMPLER + 0x100u * (uint32_t)w;
        host(base + SS_GS, &gs[w], sizeof(GenScalars));
        dev(base + SS_MAT, d.mat, (uint64_t)d.K * d.Mpad * 4); dev(base + SS_COLPOS, d.colPos, (uint64_t)d.K * 4);
        dev(base + SS_ATOMS, d.atoms, (uint64_t)g.handleHi * sizeof(AtomRec)); dev(base + SS_VEC, d.vec, (uint64_t)g.nAtoms * 4);
        dev(base + SS_FREE, d.freeHandles, (uint64_t)g.freeCount * 4);
        dev(base + SS_BINHEAD, d.binHead, (uint64_t)d.M * d.K * 4);
        dev(base + SS_BITS0, d.bits0, (uint64_t)d.nWords0 * 8); dev(base + SS_BITS1, d.bits1, (uint64_t)d.nWords1 * 8); dev(base + SS_BITS2, d.bits2, (uint64_t)d.nWords2 * 8);
        if (d.sparse) {
            dev(base + SS_ROWS, d.rows, (uint64_t)d.M * d.Kpad * 4); dev(base + SS_MFLAGS, d.mflags, (uint64_t)d.K * d.Mw * 8);
            dev(base + SS_Z1, d.Z1, (uint64_t)d.K * 4); dev(base + SS_Z2, d.Z2, (uint64_t)d.K * d.K * 4);
        } else if (w == st.apOwner) dev(base + SS_AP, d.AP, (uint64_t)d.M * d.Npad * 4);
    }
    return v;
}
// pinned staging buffer of a save or load (not the session's: released before the call returns)
struct StateStaging { void *p; StateStaging() : p(rt_malloc_host(STATE_STAGING_BYTES)) {} ~StateStaging() { rt_free_host(p); } };
// one piece of a device section between the device and the staging buffer, complete before the buffer is used again (the pieces are
// cgstate's: Writer::write, Reader::read_pieces)
static void state_piece(cogaps_session *s, bool toDevice, const cgstate::Section &sec, uint64_t off, size_t n, void *buf)
{
    if (toDevice) rt_h2d((char *)sec.dev + off, buf, n, s->stream); else rt_d2h(buf, (const char *)sec.dev + off, n, s->stream);
    rt_sync(s->stream);
}

static int state_refusal(cogaps_session *s, const char *path, const char *what)
{
    if (!s || !path) return fail("null argument");
    if (s->poisoned) return fail(std::string("this session was ended by a device error; its state cannot be ") + what);
    if (s->p.sampler == COGAPS_SAMPLER_SEQUENTIAL) return fail(std::string("a state file holds the asynchronous sampler's chain: the state of a sequential session (sampler = COGAPS_SAMPLER_SEQUENTIAL) cannot be ") + what);
    return 0;
}

int cogaps_session_position(cogaps_session *s, int *phase, uint32_t *nextIter)
{
    if (!s) return fail("null argument");
    if (phase) *phase = s->posPhase;
    if (nextIter) *nextIter = s->posNext;
    return 0;
}

int cogaps_session_debug_data_digest(cogaps_session *s, uint64_t *digest)
{
    if (!s || !digest) return fail("null argument");
    SESSION_TRY
    s->digestValid = false;      // (the hook computes it anew every time)
    *digest = data_digest(s);
    SESSION_END
}

int cogaps_session_save_state(cogaps_session *s, const char *path)
{
    if (state_refusal(s, path, "saved")) return 1;
    SESSION_TRY
    rt_sync(s->stream);
    StateMeta meta; memset(&meta, 0, sizeof(meta));
    GenScalars gs[2]; memset(gs, 0, sizeof(gs));
    const StateSamplers st = state_samplers(s);
    for (int w = 0; w < 2; ++w) {
        if (!st.present[w]) continue;
        const HostSampler &h = *st.hs[w];
        read_gs(s, *st.hs[w]); gs[w] = *s->hGs;
        if (gs[w].error) return fail("this session's device state carries an error code; its state cannot be saved");
        meta.samp[w].present = 1; meta.samp[w].nAtoms = h.nAtoms; meta.samp[w].avgQueue = h.avgQueue; meta.samp[w].anneal = h.anneal;
    }
    meta.phase = (uint32_t)s->posPhase; meta.nextIter = s->posNext;
    meta.seeder0 = s->seeder.s0; meta.seeder1 = s->seeder.s1; meta.runnerRng = s->runnerRng; meta.totalUpdates = s->totalUpdates;
    meta.samplerSeconds = s->samplerSeconds; meta.elapsedSeconds = now_s() - s->startTime;
    meta.statUpdates = s->statUpdates; meta.pumpUpdates = s->pumpUpdates; meta.nSnap[0] = s->nSnap[0]; meta.nSnap[1] = s->nSnap[1];
    meta.nHistory = (uint32_t)s->chisqHist.size(); meta.genScalarsBytes = (uint32_t)sizeof(GenScalars);
    meta.nSeedFifo = s->seedFifo.size() - s->seedHead;
    uint64_t fp[FP_N]; state_fingerprint(s, fp);
    const StateHostArrays ha(s->seedFifo, s->seedHead, s->snapA, s->snapP, s->chisqHist, s->atomHistA, s->atomHistP);
    const std::vector<cgstate::Section> secs = state_sections(s, fp, &meta, gs, ha);
    StateStaging staging;
    cgstate::Writer out(path);
    out.write(secs, staging.p, STATE_STAGING_BYTES, [&](const cgstate::Section &sec, uint64_t off, size_t n, void *buf) { state_piece(s, false, sec, off, n, buf); });
    SESSION_END
}

int cogaps_session_load_state(cogaps_session *s, const char *path)
{
    if (state_refusal(s, path, "replaced")) return 1;
    if (!s->ownsStream) return fail("this session belongs to a batch: load the state first, then create the batch");
    SESSION_TRY
    rt_sync(s->stream);
    // ---- everything is validated before anything of the session is overwritten ----
    StateStaging staging;
    cgstate::Reader in(path, staging.p, STATE_STAGING_BYTES);
    const std::string name = std::string("state file: ") + path;
    uint64_t fpFile[FP_N], fpMine[FP_N];
    const cgstate::TableEntry *e = in.find(SEC_FINGERPRINT);
    if (!e || e->bytes != sizeof(fpFile)) return fail(name + " is corrupt: it has no fingerprint section of this version's size");
    in.read(*e, 0, fpFile, sizeof(fpFile));
    state_fingerprint(s, fpMine);
    for (int i = 0; i < FP_N; ++i)
        if (fpFile[i] != fpMine[i])
            return fail(name + " does not belong to this session: " + FP_WORDS[i].name + " differs (file " + fp_text(i, fpFile[i]) + ", session " + fp_text(i, fpMine[i]) + ")");
    StateMeta meta;
    e = in.find(SEC_META);
    if (!e || e->bytes != sizeof(meta)) return fail(name + " is corrupt: it has no meta section of this version's size");
    in.read(*e, 0, &meta, sizeof(meta));
    const StateSamplers st = state_samplers(s);
    GenScalars gs[2]; memset(gs, 0, sizeof(gs));
    const uint64_t na = (uint64_t)s->nGenes * s->K;
    bool sane = meta.phase >= 1 && meta.phase <= 3 && meta.genScalarsBytes == sizeof(GenScalars) && meta.nSeedFifo < ((uint64_t)1 << 32)
                && (na == 0 || (meta.nSnap[0] < ((uint64_t)1 << 40) / na && meta.nSnap[1] < ((uint64_t)1 << 40) / na));
    for (int w = 0; w < 2 && sane; ++w) {
        if (meta.samp[w].present != st.present[w]) { sane = false; break; }
        if (!st.present[w]) continue;
        e = in.find(SEC_SAMPLER + 0x100u * (uint32_t)w + SS_GS);
        if (!e || e->bytes != sizeof(GenScalars)) { sane = false; break; }
        in.read(*e, 0, &gs[w], sizeof(GenScalars));
        const GenScalars &g = gs[w];
        sane = g.error == 0 && g.handleHi < 0x7FFFFFF0u && g.nAtoms <= g.handleHi && g.freeCount <= g.handleHi && g.eraseCount == 0;
    }
    if (!sane) return fail(name + " is corrupt: its counters contradict each other or this session");
    std::vector<uint64_t> fifo(meta.nSeedFifo); std::vector<float> snapA[2], snapP[2], chisq(meta.nHistory); std::vector<uint32_t> histA(meta.nHistory), histP(meta.nHistory);
    for (int w = 0; w < 2; ++w) { snapA[w].resize((size_t)meta.nSnap[w] * na); snapP[w].resize((size_t)meta.nSnap[w] * s->nSamples * s->K); }
    const StateHostArrays ha(fifo, 0, snapA, snapP, chisq, histA, histP);
    std::vector<cgstate::Section> secs = state_sections(s, fpFile, &meta, gs, ha);
    if (secs.size() != in.tab.size())
        return fail(name + " holds " + std::to_string(in.tab.size()) + " sections where this session's state has " + std::to_string(secs.size()));
    for (const cgstate::Section &sec : secs) {
        e = in.find(sec.id);
        if (!e || e->bytes != sec.bytes)
            return fail(name + ": section " + std::to_string(sec.id) + (e ? " has " + std::to_string(e->bytes) + " bytes" : std::string(" is missing"))
                        + " where this session's state has " + std::to_string(sec.bytes) + " bytes");
    }
    // capacities are not state: room for the file's atoms first (the session's own atoms move with the arrays)
    for (int w = 0; w < 2; ++w) if (st.present[w]) grow_atoms(s, *st.hs[w], gs[w].handleHi);
    secs = state_sections(s, fpFile, &meta, gs, ha);      // (the same sizes; the arrays may have moved)
    // ---- from here on the session is overwritten; a failure leaves a state that is no state of any chain ----
    try {
        for (const cgstate::Section &sec : secs) {
            e = in.find(sec.id);
            if (sec.id == SEC_FINGERPRINT || sec.id == SEC_META || (sec.id >= SEC_SAMPLER && ((sec.id & 0xFFu) == SS_GS))) continue;      // read above
            if (sec.host) { if (sec.bytes) in.read(*e, 0, sec.host, (size_t)sec.bytes); continue; }
            in.read_pieces(*e, sec, staging.p, STATE_STAGING_BYTES, [&](const cgstate::Section &to, uint64_t off, size_t n, void *buf) { state_piece(s, true, to, off, n, buf); });
        }
        for (int w = 0; w < 2; ++w) {
            if (!st.present[w]) continue;
            HostSampler &h = *st.hs[w]; SamplerDev &d = h.d;
            gs[w].traceOn = gs[w].traceCount = gs[w].traceCap = gs[w].traceBatchCount = 0;
            *s->hGs = gs[w];
            rt_h2d(d.gs, s->hGs, sizeof(GenScalars), s->stream); rt_sync(s->stream);
            // what a batch of this session left for its own epoch only: cleared, as a fresh session has it
            rt_memset(d.rowStamp, 0, (size_t)d.M * 8, s->stream); rt_memset(d.atomStamp, 0, (size_t)d.atomCap * 8, s->stream);
            rt_memset(d.gapStamp, 0, ((size_t)d.atomCap + 1) * 8, s->stream); rt_memset(d.inlineStamp, 0, (size_t)d.atomCap * 8, s->stream);
            rt_memset(d.atomDest, 0, (size_t)d.atomCap * 8, s->stream);
            rt_memset(h.chainGrans, 0, (size_t)d.queueCap * CHAIN_GRAN_STRIDE * 8, s->stream); rt_memset(d.grans, 0, (size_t)d.queueCap * 64 * 8, s->stream);
            h.nAtoms = meta.samp[w].nAtoms; h.avgQueue = meta.samp[w].avgQueue; h.anneal = meta.samp[w].anneal;
            h.stepsPerBatch = 0.f;      // (the chunk predictor starts over; no result depends on it)
        }
        if (!s->p.useSparseOptimization && st.present[0] && st.present[1]) do_sync(s, s->A, s->P);      // no fixed matrix: A's A*P cache is the transpose of P's
        rt_sync(s->stream);
    } catch (...) { s->poisoned = true; throw; }
    s->seedFifo.swap(fifo); s->seedHead = 0;
    s->seeder.s0 = meta.seeder0; s->seeder.s1 = meta.seeder1; s->runnerRng = meta.runnerRng; s->totalUpdates = meta.totalUpdates;
    s->samplerSeconds = meta.samplerSeconds; s->startTime = now_s() - meta.elapsedSeconds;
    s->statUpdates = meta.statUpdates; s->pumpUpdates = meta.pumpUpdates;
    for (int w = 0; w < 2; ++w) { s->nSnap[w] = meta.nSnap[w]; s->snapA[w].swap(snapA[w]); s->snapP[w].swap(snapP[w]); }
    s->chisqHist.swap(chisq); s->atomHistA.swap(histA); s->atomHistP.swap(histP);
    s->posPhase = (int)meta.phase; s->posNext = meta.nextIter;
    SESSION_END
}
