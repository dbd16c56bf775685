// genemember_kernel.h -- which genes of a set behave like the set (calcGeneGSStat and computeGeneGSProb,
// R/methods-CogapsResult.R:535-594): the statistic T of a row under one set's pattern weights, and for every member of
// the set the number of rows outside the set whose T is greater.  Lane = row over the transposed Z, so a column is one coalesced read;
// fp64 adds in ascending column order, the product rounded before it is added, two divisions: numbers anyone can recompute.  The
// counts are integers that meet in LDS and leave as atomics, so nothing depends on how the work is cut.  Nothing here waits for
// another workgroup.
#pragma once
#include "platform.h"

#define GM_THREADS 256                  // rows of one workgroup trip of the count kernel: thread = row
#define GM_WAVES (GM_THREADS / 64)
#ifndef GM_CHUNK
#define GM_CHUNK 512                    // members of a set whose statistics a trip holds in LDS at a time (6 KiB with their counts)
#endif
static_assert(GM_CHUNK >= 64 && GM_CHUNK % 64 == 0, "a chunk is whole groups of 64 members: one count per lane");
#define GM_UNROLL 8u                    // members compared per LDS round trip; a chunk's last eight are filled up with NaN, greater than which nothing is

struct GmArgs {
    const double *zt; size_t ldn;                   // Z transposed: column k is the run zt[k * ldn ..] of nRows rows
    uint32_t nRows, K, nSets;
    const unsigned long long *memberOffsets;        // [nSets + 1], from 0
    const uint32_t *members;                        // rows of every set, ascending
    const double *wMember, *wNull;                  // [nSets][K]: the pattern weights of the members' statistic and of the null's
    double *memberStat;                             // laid out like members: T under wMember
    uint32_t *greaterCount;                         // laid out like members: rows outside the set with T under wNull above the member's (null: not counted)
    double *allStat;                                // [nSets][nRows]: T under wNull of every row (null: not kept)
};

// T of one row under the K weights w: W = sum w, R = sum z, S = sum z * w in ascending k from +0; 0 where W or R is below 1e-6
// (never true of a NaN), else (S / W) / R
CG_DEVICE double gm_row_stat(const double *zt, size_t ldn, uint32_t K, uint32_t row, const double *w)
{
    double W = 0.0, R = 0.0, S = 0.0;
    for (uint32_t k = 0; k < K; ++k) {
        const double z = zt[(size_t)k * ldn + row], wk = w[k];
        W = W + wk; R = R + z; S = S + z * wk;
    }
    if (W < 1e-6 || R < 1e-6) return 0.0;
    return (S / W) / R;
}

// memberStat: one wave per set, lane = member; the grid loops
CG_KERNEL void CG_LAUNCH_BOUNDS(GM_THREADS) gm_member_kernel(GmArgs a)
{
    const uint32_t lane = cg_tid() & 63u, wave = cg_tid() >> 6;
    for (unsigned long long t = (unsigned long long)cg_bid() * GM_WAVES + wave; t < a.nSets; t += (unsigned long long)cg_gdim() * GM_WAVES) {
        const unsigned long long end = a.memberOffsets[t + 1u];
        for (unsigned long long x = a.memberOffsets[t] + lane; x < end; x += 64u)
            a.memberStat[x] = gm_row_stat(a.zt, a.ldn, a.K, a.members[x], a.wMember + (size_t)t * a.K);
    }
}

// allStat[t][i] and greaterCount[x] += #{rows i of the block outside set t : T[i] > memberStat[x]}: a workgroup trip takes one set and
// GM_THREADS rows, neighbouring trips the same rows of the next sets (the block of Z stays in the cache).  A thread computes its row's
// T in registers; a row that is a member (binary search) or past the last becomes NaN, which is greater than nothing.  The members'
// statistics are staged GM_CHUNK at a time, filled up with NaN to whole GM_UNROLLs; of each group of 64, lane j keeps the wave's count
// for member j -- the comparison's lane mask, counted -- and adds it to the chunk's counts in LDS, which leave as one atomic per member.
CG_KERNEL void CG_LAUNCH_BOUNDS(GM_THREADS) gm_count_kernel(GmArgs a)
{
    CG_SHARED double tm[GM_CHUNK];
    CG_SHARED uint32_t cnt[GM_CHUNK];
    const uint32_t tid = cg_tid(), lane = tid & 63u;
    const unsigned long long units = (unsigned long long)a.nSets * (((unsigned long long)a.nRows + GM_THREADS - 1ull) / GM_THREADS);
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t t = (uint32_t)(u % a.nSets);
        const unsigned long long row = u / a.nSets * GM_THREADS + tid, first = a.memberOffsets[t];
        const uint32_t m = (uint32_t)(a.memberOffsets[t + 1u] - first);
        const uint32_t *mem = a.members + first;
        double tn = __builtin_nan("");
        if (row < a.nRows) {
            tn = gm_row_stat(a.zt, a.ldn, a.K, (uint32_t)row, a.wNull + (size_t)t * a.K);
            if (a.allStat) a.allStat[(size_t)t * a.nRows + row] = tn;
            uint32_t lo = 0u, hi = m;
            while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (mem[mid] < row) lo = mid + 1u; else hi = mid; }
            if (lo < m && mem[lo] == row) tn = __builtin_nan("");
        }
        if (!a.greaterCount) continue;
        for (uint32_t c0 = 0; c0 < m; c0 += GM_CHUNK) {
            const uint32_t len = m - c0 < (uint32_t)GM_CHUNK ? m - c0 : (uint32_t)GM_CHUNK;
            for (uint32_t x = tid; x < ((len + GM_UNROLL - 1u) & ~(GM_UNROLL - 1u)); x += GM_THREADS) {
                tm[x] = x < len ? a.memberStat[first + c0 + x] : __builtin_nan("");
                cnt[x] = 0u;
            }
            cg_sync();
            for (uint32_t base = 0; base < len; base += 64u) {
                const uint32_t here = len - base < 64u ? len - base : 64u;
                uint32_t mine = 0u;
                for (uint32_t j = 0; j < here; j += GM_UNROLL) {
                    double v[GM_UNROLL];
                    for (uint32_t b = 0; b < GM_UNROLL; ++b) v[b] = tm[base + j + b];
                    for (uint32_t b = 0; b < GM_UNROLL; ++b) {
                        const uint32_t c = (uint32_t)cg_popc64(cg_ballot(tn > v[b]));
                        if (lane == j + b) mine = c;
                    }
                }
                if (mine) cg_atomic_add_u32(&cnt[base + lane], mine);
            }
            cg_sync();
            for (uint32_t x = tid; x < len; x += GM_THREADS)
                if (cnt[x]) cg_atomic_add_u32(a.greaterCount + first + c0 + x, cnt[x]);
            cg_sync();
        }
    }
}
