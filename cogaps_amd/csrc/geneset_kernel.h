// geneset_kernel.h -- the gene-set permutation statistic of the result side (calcCoGAPSStat, R/methods-CogapsResult.R:499-531):
// for every set, numPerm draws of `size` distinct rows of the Z matrix, the column means over them, and the count of draws whose
// mean exceeds the set's own.  A gather-and-reduce: one wave per (set, permutation), lane = column, every drawn
// row one coalesced read; fp64 adds in the order of the draws and one division, so that the counts are integers anyone can
// recompute.  Nothing here waits for another workgroup.
#pragma once
#include "platform.h"

#define GS_THREADS 256                  // four waves per workgroup
#define GS_WAVES (GS_THREADS / 64)
#define GS_PERMS 16                     // permutations of one set per workgroup trip: four per wave, one atomic per column for all sixteen
#define GS_BATCH 8                      // rows a wave has in flight before it adds them, in order

// ------------------------------------------------------------------------------------------------
// The draw: a keyed permutation of [0, n) evaluated per index -- a four-round balanced Feistel network on 2h bits, 2^(2h) >= n,
// walked until it lands below n (cycle walking).  Index j of permutation p of set t depends on (seed, t, p, n, j) alone, and
// j = 0 .. s-1 are distinct because a permutation is.
// ------------------------------------------------------------------------------------------------
CG_HD uint32_t gs_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
struct GsPerm { uint32_t key[4]; uint32_t n, h, mask; };
CG_HD GsPerm gs_perm_make(uint32_t seed, uint32_t t, uint32_t p, uint32_t n)
{
    GsPerm q;
    for (uint32_t r = 0; r < 4u; ++r) q.key[r] = gs_mix(seed ^ gs_mix(t ^ gs_mix(p ^ ((r + 1u) * 0x9E3779B9u))));
    const uint32_t top = n - 1u;
    uint32_t bits = top ? 32u - (uint32_t)__builtin_clz(top) : 0u;      // bit_length(n - 1)
    if (bits < 2u) bits = 2u;
    q.n = n; q.h = (bits + 1u) / 2u; q.mask = (1u << q.h) - 1u;          // (h <= 16)
    return q;
}
CG_HD uint32_t gs_perm_index(const GsPerm &q, uint32_t j)
{
    uint32_t x = j;
    do {
        uint32_t L = x >> q.h, R = x & q.mask;
        for (uint32_t r = 0; r < 4u; ++r) { const uint32_t f = L ^ (gs_mix(R ^ q.key[r]) & q.mask); L = R; R = f; }
        x = (L << q.h) | R;
    } while (x >= q.n);
    return x;
}

// ------------------------------------------------------------------------------------------------
// Sum of `count` rows of z (row-major, ld doubles per row) over the columns c0 + 64 * slot + lane, slot < SLOTS, in the order
// i = 0 .. count-1 of index(i): the lanes compute 64 indices at a time, every index is then broadcast in turn and lane = column
// adds the row.  GS_BATCH rows are loaded before they are added (still in order) to keep that many reads in flight per wave.  A lane
// whose column does not exist reads column 0 of the row -- an address inside the row, no branch -- and its sum is never used.
// Every lane of the wave calls it with the same count.
// ------------------------------------------------------------------------------------------------
template <int SLOTS, class IndexFn>
CG_DEVICE void gs_sum_rows(const double *z, size_t ld, uint32_t K, uint32_t c0, uint32_t count, IndexFn index, double (&acc)[SLOTS])
{
    const uint32_t lane = cg_tid() & 63u;
    uint32_t col[SLOTS];
    for (int s = 0; s < SLOTS; ++s) { const uint32_t c = c0 + 64u * (uint32_t)s + lane; col[s] = c < K ? c : 0u; acc[s] = 0.0; }
    for (uint32_t base = 0; base < count; base += 64u) {
        const uint32_t here = count - base < 64u ? count - base : 64u;
        const uint32_t mine = lane < here ? index(base + lane) : 0u;
        uint32_t i = 0;
        for (; i + GS_BATCH <= here; i += GS_BATCH) {
            double v[GS_BATCH][SLOTS];
            for (int b = 0; b < GS_BATCH; ++b) {
                const double *row = z + (size_t)cg_wave_bcast_u32(mine, (int)i + b) * ld;
                for (int s = 0; s < SLOTS; ++s) v[b][s] = row[col[s]];
            }
            for (int b = 0; b < GS_BATCH; ++b)
                for (int s = 0; s < SLOTS; ++s) acc[s] = acc[s] + v[b][s];
        }
        for (; i < here; ++i) {
            const double *row = z + (size_t)cg_wave_bcast_u32(mine, (int)i) * ld;
            for (int s = 0; s < SLOTS; ++s) acc[s] = acc[s] + row[col[s]];
        }
    }
}

struct GsArgs {
    const double *z; size_t ld;                     // Z, row-major, ld >= K doubles per row
    uint32_t nRows, K, nSets, numPerm, seed;
    const unsigned long long *memberOffsets;        // [nSets + 1]
    const uint32_t *members;                        // rows of every set, ascending
    const uint32_t *drawSizes;                      // [nSets]
    double *actual;                                 // [nSets][K]: mean over the set's members (NaN for a set without one)
    uint32_t *counts;                               // [nSets][K]: permutations with actual < permuted mean
};

// actual[t][k]: one wave per (set, block of 64 * SLOTS columns), the grid loops
template <int SLOTS>
CG_KERNEL void CG_LAUNCH_BOUNDS(GS_THREADS) gs_actual_kernel(GsArgs a)
{
    const uint32_t lane = cg_tid() & 63u, wave = cg_tid() >> 6;
    const uint32_t colBlocks = (a.K + 64u * SLOTS - 1u) / (64u * SLOTS);
    const unsigned long long units = (unsigned long long)a.nSets * colBlocks;
    for (unsigned long long u = (unsigned long long)cg_bid() * GS_WAVES + wave; u < units; u += (unsigned long long)cg_gdim() * GS_WAVES) {
        const uint32_t t = (uint32_t)(u / colBlocks), c0 = (uint32_t)(u % colBlocks) * 64u * SLOTS;
        const unsigned long long first = a.memberOffsets[t];
        const uint32_t m = (uint32_t)(a.memberOffsets[t + 1u] - first);
        const uint32_t *mem = a.members + first;
        double acc[SLOTS];
        gs_sum_rows<SLOTS>(a.z, a.ld, a.K, c0, m, [&](uint32_t j) { return mem[j]; }, acc);
        for (int s = 0; s < SLOTS; ++s) {
            const uint32_t c = c0 + 64u * (uint32_t)s + lane;
            if (c < a.K) a.actual[(size_t)t * a.K + c] = acc[s] / (double)m;
        }
    }
}

// counts[t][k] += #{p : actual[t][k] < mean of permutation p}: a workgroup trip takes GS_PERMS permutations of one set (and one
// block of 64 * SLOTS columns), a wave one permutation at a time; the waves' counts meet in LDS and leave as one atomic per column.
// Integer sums: the result does not depend on how the work is cut.
template <int SLOTS>
CG_KERNEL void CG_LAUNCH_BOUNDS(GS_THREADS) gs_count_kernel(GsArgs a)
{
    CG_SHARED uint32_t part[GS_WAVES][64 * SLOTS];
    const uint32_t lane = cg_tid() & 63u, wave = cg_tid() >> 6;
    const uint32_t colBlocks = (a.K + 64u * SLOTS - 1u) / (64u * SLOTS);
    const uint32_t chunks = (a.numPerm + GS_PERMS - 1u) / GS_PERMS;
    const unsigned long long units = (unsigned long long)a.nSets * chunks * colBlocks;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t c0 = (uint32_t)(u % colBlocks) * 64u * SLOTS;
        const unsigned long long rest = u / colBlocks;
        const uint32_t t = (uint32_t)(rest / chunks), p0 = (uint32_t)(rest % chunks) * GS_PERMS;
        const uint32_t pEnd = a.numPerm - p0 < (uint32_t)GS_PERMS ? a.numPerm : p0 + GS_PERMS;
        const uint32_t size = a.drawSizes[t];
        double act[SLOTS]; uint32_t cnt[SLOTS];
        for (int s = 0; s < SLOTS; ++s) {
            const uint32_t c = c0 + 64u * (uint32_t)s + lane;
            act[s] = a.actual[(size_t)t * a.K + (c < a.K ? c : 0u)]; cnt[s] = 0u;
        }
        for (uint32_t p = p0 + wave; p < pEnd; p += GS_WAVES) {
            const GsPerm q = gs_perm_make(a.seed, t, p, a.nRows);
            double acc[SLOTS];
            gs_sum_rows<SLOTS>(a.z, a.ld, a.K, c0, size, [&](uint32_t j) { return gs_perm_index(q, j); }, acc);
            for (int s = 0; s < SLOTS; ++s) cnt[s] += act[s] < acc[s] / (double)size ? 1u : 0u;
        }
        for (int s = 0; s < SLOTS; ++s) part[wave][64 * s + lane] = cnt[s];
        cg_sync();
        if (wave == 0u)
            for (int s = 0; s < SLOTS; ++s) {
                const uint32_t c = c0 + 64u * (uint32_t)s + lane;
                uint32_t sum = 0u;
                for (int w = 0; w < GS_WAVES; ++w) sum += part[w][64 * s + lane];
                if (c < a.K && sum) cg_atomic_add_u32(a.counts + (size_t)t * a.K + c, sum);
            }
        cg_sync();
    }
}

// test hook: indices 0 .. size-1 of permutation `perm` of set `set`, by the code the count kernel draws with (one wave)
CG_KERNEL void CG_LAUNCH_BOUNDS(64) gs_draw_kernel(uint32_t nRows, uint32_t size, uint32_t seed, uint32_t set, uint32_t perm, uint32_t *out)
{
    const GsPerm q = gs_perm_make(seed, set, perm, nRows);
    for (uint32_t j = cg_tid(); j < size; j += 64u) out[j] = gs_perm_index(q, j);
}
