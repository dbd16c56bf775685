// gsea_kernel.h -- the pre-ranked gene-set enrichment of the result side (getPatternGeneSet, method "enrichment",
// R/methods-CogapsResult.R:300-344: fgsea with scoreType = "pos"): every column of a factor matrix ranks the rows, and
// every set -- and numPerm keyed draws of its size -- is scored in every column by the running-sum statistic.  A gather-sort-scan:
//   ranks   the stable sort of markers_kernel.h on the keys gsea_key_kernel writes (descending value, ties in row order); gsea_pack_kernel
//           then lays (rank, value) of a row's columns side by side, one 8-byte word each, so that a drawn row is ONE contiguous read
//           for all the columns a workgroup scores at a time and the word is its own sort key (ranks are distinct);
//   scores  a workgroup trip takes one set, GSEA_PERMS subsets of it (slot 0: the set's own members, slot s: permutation s - 1 -- one
//           code path) and a block of up to GSEA_BLOCK columns.  The subset's rows are computed once into LDS; P columns at a time are
//           gathered, sorted side by side by one bitonic network over the whole workgroup (list p, entry i at buf[i * P + p]: the lanes
//           of a step touch consecutive words), and scanned with lane = column: the dependent fp64 add chains of P columns run side
//           by side.  The divisions of the definition are done with lane = entry in between, every thread keeping the first maximum of
//           its own entries; a list's 256 / P candidates meet with lane = column again.  nGe and permSum of a trip meet in LDS and
//           leave as one atomic per (set, column): integer sums, so the result does not depend on how the work is cut.
// LDS of a workgroup: buf 4096 x 8 B = 32 KB (the sort; then the running sums, in place), rk 4096 x 4 B = 16 KB (the ranks the running
// sums displaced), idx 4096 x 4 B = 16 KB (the subset), 3 KB of candidates, 1.25 KB of per-column cells: 68.25 KB of the compute
// unit's 160 KB -- two workgroups (eight waves) per compute unit.  GSEA_MAX_SET = 4096 members is what buf holds of one column.
// fp64 in the order the definition gives; the build contracts nothing (-ffp-contract=off).  Every loop is a grid-stride loop over a
// unit count the host computed, or has uniform bounds read from the set's size; the one data-dependent loop is the draw's cycle
// walk (geneset_kernel.h).  Nothing here waits for another workgroup: the permutations read the sets' own scores from the launch before.
#pragma once
#include "platform.h"
#include "geneset_kernel.h"
#include "markers_kernel.h"

#define GSEA_THREADS 256
#define GSEA_MAX_SET 4096               // members of a set: entries of one column's list in LDS
#define GSEA_PERMS 16                   // subsets of one set per workgroup trip
#define GSEA_BLOCK 64                   // columns per workgroup trip (and the most that are sorted side by side)
#define GSEA_CELLS (GSEA_MAX_SET / GSEA_THREADS)      // words of the sort buffer per thread
#define GSEA_BATCH 8                    // entries a lane of the running sum has in flight before it adds them, in order
#define GSEA_SCALE 1099511627776.0      // 2^40: the quantum of permSum

CG_HD float gsea_value(unsigned long long word) { const uint32_t bits = (uint32_t)word; float v; memcpy(&v, &bits, 4); return v; }
CG_HD uint32_t gsea_pow2_ceil(uint32_t x) { return x <= 1u ? 1u : 1u << (32u - (uint32_t)__builtin_clz(x - 1u)); }

// ---- ranks: the sort key of value v >= +0 in the markers' ascending sort -- descending value; equal values stay in row order ----
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) gsea_key_kernel(const float *vt, PmArgs a)
{
    const unsigned long long rowBlocks = ((unsigned long long)a.n + PM_THREADS - 1ull) / PM_THREADS, units = rowBlocks * a.L;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const size_t col = (size_t)(u / rowBlocks) * a.ldn;
        const unsigned long long i = (u % rowBlocks) * PM_THREADS + cg_tid();
        if (i >= a.n) continue;
        a.keys[0][col + (size_t)i] = ~pm_bits((double)vt[col + (size_t)i]);
        a.order[0][col + (size_t)i] = (uint32_t)i;
    }
}

// pk[g][k] = (0-based rank of row g in column k) << 32 | the bits of its fp32 value; rankT is the sort's 1-based [K][ldn]
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) gsea_pack_kernel(const float *vt, const uint32_t *rankT, size_t ldn, uint32_t n, uint32_t K, unsigned long long *pk, size_t ldk)
{
    const unsigned long long units = ((unsigned long long)n * K + PM_THREADS - 1ull) / PM_THREADS;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const unsigned long long e = u * PM_THREADS + cg_tid();
        if (e >= (unsigned long long)n * K) continue;
        const size_t g = (size_t)(e / K), k = (size_t)(e % K);
        uint32_t bits; const float v = vt[k * ldn + g]; memcpy(&bits, &v, 4);
        pk[g * ldk + k] = ((unsigned long long)(rankT[k * ldn + g] - 1u) << 32) | bits;
    }
}

struct GseaArgs {
    const unsigned long long *pk; size_t ldk;       // [nRows][ldk >= K]
    uint32_t nRows, K, nSets, setBase;              // the sets of this launch are setBase .. setBase + nSets - 1 of the caller's: the draw's key
    uint32_t seed, slot0, nSlots;                   // the subsets of this launch: slot 0 is the set itself, slot s permutation s - 1
    const unsigned long long *memberOffsets;        // [nSets + 1]
    const uint32_t *members;                        // rows of every set, ascending; 1 .. GSEA_MAX_SET of them, fewer than nRows
    double *es; uint32_t *peak;                     // [nSets][K]: written by slot 0, read by the others
    uint32_t *nGe; unsigned long long *permSum;     // [nSets][K]: zero before the launch
};

CG_KERNEL void CG_LAUNCH_BOUNDS(GSEA_THREADS) gsea_score_kernel(GseaArgs a)
{
    CG_SHARED unsigned long long buf[GSEA_MAX_SET];
    CG_SHARED uint32_t rk[GSEA_MAX_SET];
    CG_SHARED uint32_t idx[GSEA_MAX_SET];
    CG_SHARED double nr[GSEA_BLOCK];
    CG_SHARED double candTop[GSEA_THREADS];
    CG_SHARED uint32_t candAt[GSEA_THREADS];
    CG_SHARED uint32_t accGe[GSEA_BLOCK];
    CG_SHARED unsigned long long accSum[GSEA_BLOCK];
    const uint32_t tid = cg_tid();
    const uint32_t kBlocks = (a.K + GSEA_BLOCK - 1u) / GSEA_BLOCK, chunks = (a.nSlots + GSEA_PERMS - 1u) / GSEA_PERMS;
    const unsigned long long units = (unsigned long long)a.nSets * chunks * kBlocks;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t kb0 = (uint32_t)(u % kBlocks) * GSEA_BLOCK, kb = a.K - kb0 < (uint32_t)GSEA_BLOCK ? a.K - kb0 : (uint32_t)GSEA_BLOCK;
        const unsigned long long rest = u / kBlocks;
        const uint32_t t = (uint32_t)(rest / chunks), s0 = a.slot0 + (uint32_t)(rest % chunks) * GSEA_PERMS;
        const uint32_t sEnd = a.slot0 + a.nSlots - s0 < (uint32_t)GSEA_PERMS ? a.slot0 + a.nSlots : s0 + GSEA_PERMS;
        const unsigned long long first = a.memberOffsets[t];
        const uint32_t m = (uint32_t)(a.memberOffsets[t + 1u] - first);                  // (1 .. GSEA_MAX_SET: the host refuses others)
        const uint32_t n2 = gsea_pow2_ceil(m);
        const uint32_t room = (uint32_t)GSEA_MAX_SET / n2 < (uint32_t)GSEA_BLOCK ? (uint32_t)GSEA_MAX_SET / n2 : (uint32_t)GSEA_BLOCK;
        const uint32_t P = gsea_pow2_ceil(kb) < room ? gsea_pow2_ceil(kb) : room;          // lists side by side: n2 * P <= GSEA_MAX_SET
        const uint32_t logP = (uint32_t)__builtin_ctz(P), cells = n2 * P, pairs = (n2 >> 1) * P;
        const double span = (double)(a.nRows - m);
        if (tid < (uint32_t)GSEA_BLOCK) { accGe[tid] = 0u; accSum[tid] = 0ull; }
        for (uint32_t s = s0; s < sEnd; ++s) {
            if (s == 0u) for (uint32_t j = tid; j < m; j += GSEA_THREADS) idx[j] = a.members[first + j];
            else {
                const GsPerm q = gs_perm_make(a.seed, a.setBase + t, s - 1u, a.nRows);
                for (uint32_t j = tid; j < m; j += GSEA_THREADS) idx[j] = gs_perm_index(q, j);
            }
            cg_sync();
            for (uint32_t sub0 = 0; sub0 < kb; sub0 += P) {
                const uint32_t live = kb - sub0 < P ? kb - sub0 : P;
                // gather: entry i of list p is row idx[i] in column kb0 + sub0 + p; the lists are padded to n2 entries with the key above all
                // (a thread's up to GSEA_CELLS words are all requested before the first is stored: that many reads in flight; a cell
                // that is padding reads word 0 of the matrix -- an address that exists, no branch -- and stores the padding key)
                const uint32_t mine = tid & (P - 1u);                    // a thread's cells and pairs belong to one list: P divides the workgroup
                {
                    unsigned long long w[GSEA_CELLS];
#pragma unroll
                    for (int b = 0; b < GSEA_CELLS; ++b) {
                        const uint32_t x = tid + (uint32_t)b * GSEA_THREADS, i = x >> logP;
                        const bool real = x < cells && i < m && mine < live;
                        const size_t at = real ? (size_t)idx[i] * a.ldk + kb0 + sub0 + mine : (size_t)0;
                        w[b] = a.pk[at];
                        if (!real) w[b] = ~0ull;
                    }
#pragma unroll
                    for (int b = 0; b < GSEA_CELLS; ++b) {
                        const uint32_t x = tid + (uint32_t)b * GSEA_THREADS;
                        if (x < cells) buf[x] = w[b];
                    }
                }
                cg_sync();
                // the bitonic network, ascending: every step one compare-exchange per pair and list; a thread reads its up to
                // GSEA_CELLS / 2 pairs (they are disjoint) before it writes any of them back
                for (uint32_t k2 = 2u; k2 <= n2; k2 <<= 1)
                    for (uint32_t j = k2 >> 1; j > 0u; j >>= 1) {
                        unsigned long long A[GSEA_CELLS / 2], B[GSEA_CELLS / 2];
                        uint32_t lo[GSEA_CELLS / 2];
#pragma unroll
                        for (int b = 0; b < GSEA_CELLS / 2; ++b) {
                            const uint32_t x = tid + (uint32_t)b * GSEA_THREADS, c = x >> logP;
                            lo[b] = x < pairs && mine < live ? 2u * c - (c & (j - 1u)) : CG_NONE;
                            const uint32_t la = (lo[b] << logP) + mine;
                            A[b] = lo[b] != CG_NONE ? buf[la] : 0ull; B[b] = lo[b] != CG_NONE ? buf[la + (j << logP)] : 0ull;
                        }
#pragma unroll
                        for (int b = 0; b < GSEA_CELLS / 2; ++b)
                            if (lo[b] != CG_NONE && (A[b] > B[b]) == ((lo[b] & k2) == 0u)) {
                                buf[(lo[b] << logP) + mine] = B[b]; buf[((lo[b] + j) << logP) + mine] = A[b];
                            }
                        cg_sync_lds();
                    }
                // lane = list: cum_i = v_0 + ... + v_i from +0 in rank order, left in place of the entry; the rank moves to rk
                // (GSEA_BATCH entries are read before they are added, still in order: that many LDS reads in flight per lane)
                if (tid < live) {
                    double cum = 0.0;
                    uint32_t i = 0;
                    for (; i + GSEA_BATCH <= m; i += GSEA_BATCH) {
                        unsigned long long e[GSEA_BATCH];
                        for (int b = 0; b < GSEA_BATCH; ++b) e[b] = buf[((i + (uint32_t)b) << logP) + tid];
                        for (int b = 0; b < GSEA_BATCH; ++b) {
                            cum = cum + (double)gsea_value(e[b]);
                            rk[((i + (uint32_t)b) << logP) + tid] = (uint32_t)(e[b] >> 32);
                            buf[((i + (uint32_t)b) << logP) + tid] = pm_bits(cum);
                        }
                    }
                    for (; i < m; ++i) {
                        const unsigned long long e = buf[(i << logP) + tid];
                        cum = cum + (double)gsea_value(e);
                        rk[(i << logP) + tid] = (uint32_t)(e >> 32);
                        buf[(i << logP) + tid] = pm_bits(cum);
                    }
                    nr[tid] = cum;
                }
                cg_sync();
                // lane = entry: top_i = cum_i / NR - (r_i - i) / (N - m).  A thread's entries belong to one list (P divides the
                // workgroup) and ascend, so it keeps the first maximum of its own; the 256 / P candidates of a list meet below
                {
                    const uint32_t p = tid & (P - 1u);
                    double best = 0.0; uint32_t at = CG_NONE;
                    if (p < live) {
                        const double NR = nr[p];
                        for (uint32_t x = tid; x < (m << logP); x += GSEA_THREADS) {
                            const uint32_t i = x >> logP;
                            const double hit = NR == 0.0 ? (double)(i + 1u) / (double)m : pm_from_bits(buf[x]) / NR;
                            const double top = hit - (double)(rk[x] - i) / span;
                            if (at == CG_NONE || top > best) { best = top; at = i; }
                        }
                    }
                    candTop[tid] = best; candAt[tid] = at;
                }
                cg_sync();
                // lane = list: the maximum and the first entry that attains it
                if (tid < live) {
                    double best = candTop[tid]; uint32_t at = candAt[tid];                   // (entry 0: there is one)
                    for (uint32_t c = tid + P; c < (uint32_t)GSEA_THREADS; c += P) {
                        const double top = candTop[c]; const uint32_t i = candAt[c];
                        if (i != CG_NONE && (top > best || (top == best && i < at))) { best = top; at = i; }
                    }
                    const size_t out = (size_t)t * a.K + kb0 + sub0 + tid;
                    if (s == 0u) { a.es[out] = best; a.peak[out] = at; }
                    else {
                        accGe[sub0 + tid] += best >= a.es[out] ? 1u : 0u;
                        accSum[sub0 + tid] += (unsigned long long)(best * GSEA_SCALE);      // floor: ES in [0, 1], the product exact
                    }
                }
                cg_sync();
            }
        }
        if (tid < kb && sEnd > 1u) {
            const size_t out = (size_t)t * a.K + kb0 + tid;
            if (accGe[tid]) cg_atomic_add_u32(a.nGe + out, accGe[tid]);
            if (accSum[tid]) cg_atomic_add_u64(a.permSum + out, accSum[tid]);
        }
        cg_sync();
    }
}
