// seq_kernel.h -- the reference's OTHER sampler: SingleThreadedGibbsSampler<DenseNormalModel>::update
// (gibbs_sampler/SingleThreadedGibbsSampler.h:95-257) over AtomicDomain (atomic/AtomicDomain.cpp:18-119), one chain per workgroup.
//
// The sampler draws ALL its randomness from one generator (mRng: update type, site, masses, accept tests) and changes the domain at
// once: no queue, no conflict sets, no erase cache, no speculation.  A step is therefore serial by definition; what a workgroup adds
// is the width of the row reductions and of the A*P update:
//   lane 0            draws the update type and the site from the sampler's PCG state and publishes the proposal through LDS (a
//                     PropRec, as the asynchronous generator queues them; a birth carries the gap it found)
//   the workgroup     computes alphaParameters / alphaParametersWithChange / the two-site forms (DenseNormalModel.cpp:161-240)
//   lane 0            makes the scalar step with the evaluation's functions (gm_gibbs_mass, gm_logf_m), changes the domain and the matrix
//                     and publishes the A*P update(s) the step owes (a DecRec)
//   the workgroup     carries them out (DenseNormalModel.cpp:243-258) -- the next step's draw by lane 0 follows its own share, the
//                     barrier behind the draw orders every store before the next reduction's loads.
// Three workgroup barriers per step; nothing outside the workgroup is waited for, so a batch of chains is one launch with a workgroup
// each (seq_update_kernel_multi) and none of them ever waits for another.
//
// State between launches (GenScalars): qrng = the sampler's PCG state (seeded as GapsRng(randState): A's sampler, P's, then the runner's,
// GapsRunner.cpp:402-437), nAtoms / front / freeCount / handleHi = the domain, nSteps / nDone = update(nSteps)'s progress.  A launch runs at
// most SEQ_STEPS_PER_LAUNCH steps and parks; the host enqueues ceil(nSteps / SEQ_STEPS_PER_LAUNCH) launches per update.  No result depends
// on that constant: a launch ends between two steps, where registers hold nothing the scalars do not.
//
// The domain is the asynchronous sampler's device structure (gaps_state.h: AtomRec by handle, vec[idx] -> handle, binHead, occupancy
// bitmaps) with AtomicDomain's index permutation: push_back on insert, swap-with-last at once on erase (gen_erase_one).
//
// Reductions.  Product arithmetic (SEQ = false): the reduction contract of eval_kernel.h -- W = cogaps_reduction_width(N) virtual lanes,
// chunk j to lane j mod W in increasing j, ascending xor butterfly -- with BS = min(W, 1024) threads carrying V = W / BS virtual lanes
// each, folded by the asynchronous evaluation's eval_vfinish.  Verification mode (SEQ = true): eval_alpha_seq, one accumulator per sum,
// and the session's math mode.
#pragma once
#include "gaps_state.h"
#include "gen_kernel.h"
#include "eval_kernel.h"

#ifndef SEQ_STEPS_PER_LAUNCH
#define SEQ_STEPS_PER_LAUNCH 4096
#endif
#define SEQ_T_STOP 0xFFu      // published instead of a proposal: the launch is over (update complete, launch budget spent, or an error)
#define SEQ_T_NONE 0u         // a step that needs no evaluation: a same-bin move (applied at once), an exchange that is ignored

// lane 0's registers during a launch
struct SeqState { uint64_t rng; uint32_t nAtoms, front, freeCount, handleHi, error; };

// bin of a drawn position; a position past the last bin (uniform64's upper bound is inclusive; static_cast<uint64_t>(mDomainLength) may
// round up) would index past the matrix in the reference: here it ends the update with an error
CG_DEVICE bool seq_bin(const SamplerDev &S, SeqState &st, uint64_t pos, uint32_t &bin)
{
    bin = gen_bin_of(S, pos);
    if ((double)bin >= S.numBins) { st.error = GAPS_ERR_DOMAIN; return false; }
    return true;
}

// getUpdateType (:95-111) and the site of birth / death / move / exchange (:134-136, :157-159, :195-206, :231-239), lane 0 only.
// Births carry the gap (h1 = predecessor, h2 = successor, i1 = becomes its bin's head, i2 = bin).
CG_DEVICE PropRec seq_draw(const SamplerDev &S, SeqState &st)
{
    PropRec p; p.pos = 0; p.rng = 0; p.h1 = CG_NONE; p.h2 = CG_NONE; p.i1 = 0; p.i2 = 0; p.r1 = 0; p.c1 = 0; p.r2 = 0; p.c2 = 0; p.type = SEQ_T_NONE; p.gibbs = 0;
    p.m1 = 0.f; p.m2 = 0.f; p.old1 = 0.f; p.old2 = 0.f; p.curPos = 0; p.batch = 0; p.pad[0] = 0; p.pad[1] = 0; p.pad[2] = 0;
    uint32_t type = 'B';
    if (st.nAtoms >= 2u) {
        const float u1 = pcg_uniform(st.rng);
        if (u1 < 0.5f) type = pcg_uniform(st.rng) < gm_death_prob((double)st.nAtoms, S.domainLenD, S.alphaD, S.numBins) ? 'D' : 'B';
        else type = u1 < 0.75f ? 'M' : 'E';
    }
    const uint32_t K = S.K;
    if (type == 'B') {
        // AtomicDomain::randomFreePosition (AtomicDomain.cpp:41-49)
        uint64_t pos; uint32_t bin, pred = CG_NONE, succ = CG_NONE; bool occupied = false, newHead = false;
        do {
            pos = pcg_uniform64(st.rng, 1ull, S.domainLenU);
            if (!seq_bin(S, st, pos, bin)) return p;
            gen_find_gap(S, pos, bin, &pred, &succ, &occupied, &newHead);
        } while (occupied);
        p.pos = pos; p.h1 = pred; p.h2 = succ; p.i1 = newHead ? 1u : 0u; p.i2 = bin;
        p.r1 = gen_div_k(S, bin); p.c1 = bin - p.r1 * K;
        p.gibbs = S.otherColPos[p.c1] ? 1u : 0u;
        p.old1 = S.mat[(size_t)p.c1 * S.Mpad + p.r1];
        p.type = 'B';
        return p;
    }
    // randomAtom / randomAtomWithNeighbors (:24-39)
    const uint32_t idx = pcg_uniform32(st.rng, 0u, st.nAtoms - 1u);
    const uint32_t h = S.vec[idx];
    const AtomRec a = S.atoms[h];
    uint32_t bin1;
    if (!seq_bin(S, st, a.pos, bin1)) return p;
    p.h1 = h; p.i1 = idx; p.m1 = a.mass; p.curPos = a.pos;
    p.r1 = gen_div_k(S, bin1); p.c1 = bin1 - p.r1 * K;
    p.old1 = S.mat[(size_t)p.c1 * S.Mpad + p.r1];
    p.gibbs = S.otherColPos[p.c1] ? 1u : 0u;
    if (type == 'D') { p.type = 'D'; return p; }
    uint32_t bin2;
    if (type == 'M') {
        const uint64_t lbound = a.left != CG_NONE ? a.lpos : 0ull, rbound = a.right != CG_NONE ? a.rpos : S.rboundNone;
        const uint64_t pos = pcg_uniform64(st.rng, lbound + 1ull, rbound - 1ull);
        if (!seq_bin(S, st, pos, bin2)) return p;
        p.pos = pos;
        if (bin2 == bin1) { atom_set_pos(S, h, a.left, a.right, pos); return p; }      // same matrix element: accepted without a test (:209-213)
        p.type = 'M';
    } else {
        const uint32_t h2 = a.right != CG_NONE ? a.right : st.front;      // the right neighbour, or front() (:233)
        const AtomRec b = S.atoms[h2];
        if (!seq_bin(S, st, b.pos, bin2)) return p;
        if (bin2 == bin1) return p;                                        // exchanges in the same bin are ignored (:242)
        p.h2 = h2; p.m2 = b.mass;
        p.type = 'E';
    }
    p.r2 = gen_div_k(S, bin2); p.c2 = bin2 - p.r2 * K;
    p.old2 = S.mat[(size_t)p.c2 * S.Mpad + p.r2];
    p.gibbs |= S.otherColPos[p.c2] ? 2u : 0u;
    if (type == 'E' && p.gibbs == 0u) p.type = SEQ_T_NONE;                 // canUseGibbs(c1, c2) (:242)
    return p;
}

// which reduction a published proposal needs
CG_DEVICE bool seq_needs_alpha(const PropRec &p) { return p.type == 'B' ? (p.gibbs & 1u) != 0u : (p.type == 'D' || p.type == 'M' || p.type == 'E'); }

// AtomicDomain::insert (AtomicDomain.cpp:56-78): the atom takes index size(); links and the neighbours' cached copies spliced
CG_DEVICE void seq_insert(const SamplerDev &S, SeqState &st, const PropRec &p, float mass)
{
    uint32_t h;
    if (st.freeCount) h = S.freeHandles[--st.freeCount];
    else { if (st.handleHi >= S.atomCap) { st.error = GAPS_ERR_ATOM_CAP; return; } h = st.handleHi++; }
    if (st.nAtoms >= S.atomCap) { st.error = GAPS_ERR_ATOM_CAP; return; }
    const uint32_t pred = p.h1, succ = p.h2;
    AtomRec a; a.pos = p.pos; a.lpos = 0; a.rpos = 0; a.left = pred; a.right = succ; a.mass = mass; a.rmass = 0.f; a.idx = st.nAtoms; a.pad0 = 0;
    if (pred != CG_NONE) { a.lpos = S.atoms[pred].pos; S.atoms[pred].right = h; S.atoms[pred].rpos = p.pos; S.atoms[pred].rmass = mass; } else st.front = h;
    if (succ != CG_NONE) { a.rpos = S.atoms[succ].pos; a.rmass = S.atoms[succ].mass; S.atoms[succ].left = h; S.atoms[succ].lpos = p.pos; }
    S.atoms[h] = a;
    S.vec[st.nAtoms++] = h;
    if (p.i1) { S.binHead[p.i2] = h; bm_set(S, p.i2); }
}

// The scalar step of a published proposal, lane 0 only: (s, smu) = the un-annealed alpha parameters.  Returns the A*P update(s) owed.
CG_DEVICE DecRec seq_decide(const SamplerDev &S, SeqState &st, const PropRec &p, float s, float smu, float T, uint32_t mm)
{
    DecRec u; u.n = 0; u.r1 = 0; u.c1 = 0; u.d1 = 0.f; u.r2 = 0; u.c2 = 0; u.d2 = 0.f; u.pad = 0;
    s = s * T; smu = smu * T;
    const float m1 = p.m1, m2 = p.m2, old1 = p.old1, old2 = p.old2;
    if (p.type == 'B') {
        // birth (:131-149): sampleBirth where canUseGibbs(col), else an exponential draw; kept if > epsilon
        OptF g;
        if (p.gibbs & 1u) g = gm_gibbs_mass(s, smu, 0.f, S.maxGibbsMass, st.rng, S.luts, true, S.lambda);
        else { g.v = pcg_exponential(st.rng, S.lambda, mm); g.has = true; }
        if (g.has && g.v > GAPS_EPSILON) {
            seq_insert(S, st, p, g.v);
            if (st.error) return u;
            eval_store_matrix(S, p.r1, p.c1, old1, old1 + g.v);          // changeMatrix
            u.n = 1u; u.r1 = p.r1; u.c1 = p.c1; u.d1 = g.v;
        }
    } else if (p.type == 'D') {
        // death (:154-188): a rebirth mass, the accept test, on reject safelyChangeMatrix(-mass) and the erase at once
        float rebirth = m1;
        if (p.gibbs & 1u) { const OptF g = gm_gibbs_mass(s, smu, 0.f, S.maxGibbsMass, st.rng, S.luts, true, S.lambda); if (g.has) rebirth = g.v; }
        const float deltaLL = rebirth * (smu - s * rebirth / 2.f);
        if (gm_logf_m(pcg_uniform(st.rng), mm) < deltaLL) {
            if (rebirth != m1) {
                const float nv = gm_max(old1 + (rebirth - m1), 0.f);     // safelyChangeMatrix
                eval_store_matrix(S, p.r1, p.c1, old1, nv);
                atom_set_mass(S, p.h1, S.atoms[p.h1].left, rebirth);
                u.n = 1u; u.r1 = p.r1; u.c1 = p.c1; u.d1 = nv - old1;
            }
        } else {
            const float nv = gm_max(old1 + (-1.f * m1), 0.f);
            eval_store_matrix(S, p.r1, p.c1, old1, nv);
            gen_erase_one(S, p.h1, st.nAtoms, st.freeCount, st.front);
            u.n = 1u; u.r1 = p.r1; u.c1 = p.c1; u.d1 = nv - old1;
        }
    } else if (p.type == 'M') {
        // move across matrix elements (:215-222)
        const float deltaLL = -1.f * m1 * (smu + s * m1 / 2.f);
        if (gm_logf_m(pcg_uniform(st.rng), mm) < deltaLL) {
            const float nv1 = gm_max(old1 + (-m1), 0.f);
            eval_domain_move(S, p, S.atoms[p.h1]);
            eval_store_matrix(S, p.r1, p.c1, old1, nv1);                 // safelyChangeMatrix(r1, c1, -mass)
            eval_store_matrix(S, p.r2, p.c2, old2, old2 + m1);           // changeMatrix(r2, c2, mass)
            u.n = 2u; u.r1 = p.r1; u.c1 = p.c1; u.d1 = nv1 - old1; u.r2 = p.r2; u.c2 = p.c2; u.d2 = m1;
        }
    } else if (p.type == 'E') {
        // exchange (:242-256): sampleExchange with bounds (-m1, m2), applied if both new masses stay above epsilon
        const OptF g = gm_gibbs_mass(s, smu, -m1, m2, st.rng, S.luts, false, 0.f);
        const float n1 = m1 + g.v, n2 = m2 - g.v;
        if (g.has && n1 > GAPS_EPSILON && n2 > GAPS_EPSILON) {
            const float nv1 = gm_max(old1 + (n1 - m1), 0.f), nv2 = gm_max(old2 + (n2 - m2), 0.f);
            eval_store_matrix(S, p.r1, p.c1, old1, nv1);
            eval_store_matrix(S, p.r2, p.c2, old2, nv2);
            atom_set_mass(S, p.h1, S.atoms[p.h1].left, n1); atom_set_mass(S, p.h2, S.atoms[p.h2].left, n2);
            u.n = 2u; u.r1 = p.r1; u.c1 = p.c1; u.d1 = nv1 - old1; u.r2 = p.r2; u.c2 = p.c2; u.d2 = nv2 - old2;
        }
    }
    return u;
}

// Alpha parameters of NR rows in the lane order: thread t carries the virtual lanes t, t + BS, ... (V = W / BS of them); virtual lane L
// accumulates the chunks L, L + W, ... in increasing order from +0, its wave folds bits 0-5 of the lane index, eval_vfinish the waves
// (bits 6 ..) and the thread's slots (the top bits).  tot = {s, s_mu} per row, valid in wave 0.  lds: [16][4][V].
template <int NR, int MODE>
CG_DEVICE void seq_alpha_lanes(const SamplerDev &S, const uint32_t (&row)[NR], const uint32_t (&col)[NR], uint32_t col2, float ch, float *lds, float (&tot)[4])
{
    const uint32_t nq = S.Npad >> 2, BS = cg_bdim(), t = cg_tid(), W = S.redW, V = W / BS, NV = 4u * V;
    for (uint32_t v = 0; v < V; ++v) {
        float ps[NR], pm[NR];
        for (int r = 0; r < NR; ++r) { ps[r] = 0.f; pm[r] = 0.f; }
        for (uint32_t j = t + v * BS; j < nq; j += W) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float *Dr = S.D + (size_t)row[r] * S.Npad, *Ar = S.AP + (size_t)row[r] * S.Npad, *Vr = S.other + (size_t)col[r] * S.Npad;
                const cg_f4 x = ld4(Vr, j), d = ld4_stream(Dr, j), q = ld4(Ar, j);
                cg_f4 w2 = f4_zero(), s2;
                if (MODE == EVAL_MODE_SAME) w2 = ld4(S.other + (size_t)col2 * S.Npad, j);
                if (S.defaultS) {      // S * S of the default uncertainty max(0.1 D, 0.1), the host fill's three operations (eval_alpha)
                    const float sx = gm_max(d.x * 0.1f, 0.1f), sy = gm_max(d.y * 0.1f, 0.1f), sz = gm_max(d.z * 0.1f, 0.1f), sw = gm_max(d.w * 0.1f, 0.1f);
                    s2.x = sx * sx; s2.y = sy * sy; s2.z = sz * sz; s2.w = sw * sw;
                } else s2 = ld4_stream(S.S2 + (size_t)row[r] * S.Npad, j);
                EvalAcc a; a.s = ps[r]; a.m = pm[r];
                if (MODE == EVAL_MODE_CH) { EVAL_ELEM_CH(x.x, d.x, s2.x, q.x) EVAL_ELEM_CH(x.y, d.y, s2.y, q.y) EVAL_ELEM_CH(x.z, d.z, s2.z, q.z) EVAL_ELEM_CH(x.w, d.w, s2.w, q.w) }
                else if (MODE == EVAL_MODE_SAME) {
                    { const float y = x.x - w2.x; EVAL_ELEM(y, d.x, s2.x, q.x) }
                    { const float y = x.y - w2.y; EVAL_ELEM(y, d.y, s2.y, q.y) }
                    { const float y = x.z - w2.z; EVAL_ELEM(y, d.z, s2.z, q.z) }
                    { const float y = x.w - w2.w; EVAL_ELEM(y, d.w, s2.w, q.w) }
                } else { EVAL_ELEM(x.x, d.x, s2.x, q.x) EVAL_ELEM(x.y, d.y, s2.y, q.y) EVAL_ELEM(x.z, d.z, s2.z, q.z) EVAL_ELEM(x.w, d.w, s2.w, q.w) }
                ps[r] = a.s; pm[r] = a.m;
            }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float fs = cg_wave_allsum_f32(ps[r]), fm = cg_wave_allsum_f32(pm[r]);
            if ((t & 63u) == 0u) { lds[(t >> 6) * NV + (2u * r) * V + v] = fs; lds[(t >> 6) * NV + (2u * r + 1u) * V + v] = fm; }
        }
        if (NR == 1 && (t & 63u) == 0u) { lds[(t >> 6) * NV + 2u * V + v] = 0.f; lds[(t >> 6) * NV + 3u * V + v] = 0.f; }
    }
    cg_sync();
    switch (V) {
    case 1: eval_vfinish<4, 1>(lds, tot); break;
    case 2: eval_vfinish<4, 2>(lds, tot); break;
    case 4: eval_vfinish<4, 4>(lds, tot); break;
    case 8: eval_vfinish<4, 8>(lds, tot); break;
    default: eval_vfinish<4, 16>(lds, tot); break;
    }
}

// update(nSteps) of one chain, by the workgroup that calls it: at most SEQ_STEPS_PER_LAUNCH steps from where the last launch parked
template <bool SEQ>
CG_DEVICE void seq_body(const SamplerDev &S)
{
    CG_SHARED PropRec shP;
    CG_SHARED DecRec shU;
    CG_SHARED float lds[SEQ ? 16 : 16 * 4 * 16];
    CG_SHARED float seqTerm[SEQ ? 4 * 4 * EVAL_SEQ_BS : 1];
    const uint32_t t = cg_tid(), BS = cg_bdim();
    GenScalars *gs = S.gs;
    const uint32_t nSteps = gs->nSteps, nDone0 = gs->nDone;
    if (nDone0 >= nSteps || gs->error) return;      // (uniform: a chain whose update is over leaves at once)
    const float T = gs->annealTemp;
    const uint32_t mm = SEQ ? S.mathMode : GM_MATH_PORTABLE;
    const uint32_t budget = nSteps - nDone0 < (uint32_t)SEQ_STEPS_PER_LAUNCH ? nSteps - nDone0 : (uint32_t)SEQ_STEPS_PER_LAUNCH;
    SeqState st; st.rng = 0; st.nAtoms = 0; st.front = CG_NONE; st.freeCount = 0; st.handleHi = 0; st.error = 0;
    if (t == 0u) { st.rng = gs->qrng; st.nAtoms = gs->nAtoms; st.front = gs->front; st.freeCount = gs->freeCount; st.handleHi = gs->handleHi; }
    uint32_t done = 0;
    for (;;) {
        if (t == 0u) {
            if (done < budget && !st.error) { shP = seq_draw(S, st); if (st.error) shP.type = SEQ_T_STOP; }
            else shP.type = SEQ_T_STOP;
        }
        cg_sync();      // the proposal is published; every A*P store of the step before is complete
        const PropRec p = shP;
        if (p.type == SEQ_T_STOP) break;
        const bool need = seq_needs_alpha(p);
        float s = 0.f, smu = 0.f;
        if (need) {
            const bool two = p.type == 'M' || p.type == 'E', diff = two && p.r1 != p.r2;
            float tot[4] = {0.f, 0.f, 0.f, 0.f};
            const uint32_t rowA[1] = {p.r1}, colA[1] = {p.c1}, rowAB[2] = {p.r1, p.r2}, colAB[2] = {p.c1, p.c2};
            if (SEQ) {
                if (diff) eval_alpha_seq<2, EVAL_MODE_ONE>(S, rowAB, colAB, 0u, 0.f, seqTerm, lds, tot);
                else {
                    float t2[2] = {0.f, 0.f};
                    if (p.type == 'D') eval_alpha_seq<1, EVAL_MODE_CH>(S, rowA, colA, 0u, -1.f * p.m1, seqTerm, lds, t2);
                    else if (two) eval_alpha_seq<1, EVAL_MODE_SAME>(S, rowA, colA, p.c2, 0.f, seqTerm, lds, t2);
                    else eval_alpha_seq<1, EVAL_MODE_ONE>(S, rowA, colA, 0u, 0.f, seqTerm, lds, t2);
                    tot[0] = t2[0]; tot[1] = t2[1];
                }
            } else {
                if (diff) seq_alpha_lanes<2, EVAL_MODE_ONE>(S, rowAB, colAB, 0u, 0.f, lds, tot);
                else if (p.type == 'D') seq_alpha_lanes<1, EVAL_MODE_CH>(S, rowA, colA, 0u, -1.f * p.m1, lds, tot);
                else if (two) seq_alpha_lanes<1, EVAL_MODE_SAME>(S, rowA, colA, p.c2, 0.f, lds, tot);
                else seq_alpha_lanes<1, EVAL_MODE_ONE>(S, rowA, colA, 0u, 0.f, lds, tot);
            }
            s = diff ? tot[0] + tot[2] : tot[0]; smu = diff ? tot[1] - tot[3] : tot[1];      // AlphaParameters.cpp:11-14
        }
        if (t == 0u) shU = seq_decide(S, st, p, s, smu, T, mm);
        ++done;
        cg_sync();      // the decision is published
        const DecRec u = shU;
        if (u.n == 1u) eval_update_ap(S, u.r1, u.c1, u.d1, 0u, BS);
        else if (u.n == 2u) eval_update_ap2(S, u.r1, u.c1, u.d1, u.r2, u.c2, u.d2, 0u, BS);
    }
    if (t == 0u) {
        // (an error keeps the count of whole steps made before it; the host ends the update and poisons the session)
        const uint32_t nDone = nDone0 + done;
        gs->qrng = st.rng; gs->nAtoms = st.nAtoms; gs->front = st.front; gs->freeCount = st.freeCount; gs->handleHi = st.handleHi;
        gs->nDone = nDone; gs->evalProps += done;
        if (st.error) gs->error = st.error;
        if (nDone >= nSteps) gs->updateFlushed = 1u;
    }
}

template <bool SEQ>
CG_KERNEL void CG_LAUNCH_BOUNDS(1024) seq_update_kernel(const SamplerDev CG_CONSTANT *sp)
{
    cg_const_warm<sizeof(SamplerDev)>(sp);
    seq_body<SEQ>(*(const SamplerDev *)sp);
}

// one workgroup per chain: blockIdx.x = chain
CG_KERNEL void CG_LAUNCH_BOUNDS(1024) seq_update_kernel_multi(const SamplerDev CG_CONSTANT *arr)
{
    const SamplerDev CG_CONSTANT *sp = arr + cg_bid();
    cg_const_warm<sizeof(SamplerDev)>(sp);
    seq_body<false>(*(const SamplerDev *)sp);
}
