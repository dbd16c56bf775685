// residual_kernel.h -- how well a result fits its data (reconstructGene and plotResiduals' matrix, R/methods-CogapsResult.R:233-286;
// DESIGN.md 4.10): M = A P^T, the residual r = (D - M) / s, and the sums of r^2 per gene, per sample and over everything.  fp64 on
// exactly widened fp32 values, in the order the definition fixes, so that every output can be recomputed bit for bit:
//   M[i][j]        adds A[i][k] * P[j][k] from +0.0 in ascending k, one FMA each (the product of two widened floats is exact)
//   geneChiSq[i]   lane L adds q[i][j] for j = L (mod 64) in ascending j; the 64 lanes meet in the ascending xor butterfly
//   partial[b][j]  adds q[i][j] over the genes of block b (64 of them) in ascending i; sampleChiSq[j] adds the partials in ascending b
//   chiSq          adds geneChiSq[i] in ascending i
// A workgroup of four waves owns a block of 64 genes and walks its 64-column steps; lane = sample.  A wave owns 16 of the block's
// genes: their M values and their lane sums are its registers, the gene's row of A is wave-uniform (scalar loads), and the step's 64
// rows of P -- RS_KC patterns at a time, for any K -- are staged once per workgroup in LDS ([k][lane]: consecutive lanes read
// consecutive 8-byte words) and used by all 64 genes.  The q values of a step cross the waves through LDS, where wave 0 adds each
// column's 64 in gene order.  No floating-point atomics; no workgroup waits for another; the grid only decides which workgroup takes
// which block.
#pragma once
#include "platform.h"
#include "sparse_build.h"

#define RS_THREADS 256
#define RS_WAVES (RS_THREADS / 64)
#define RS_BLOCK 64                         // genes of a block (sampleChiSq's partials) = samples of a step = lanes
#define RS_GT (RS_BLOCK / RS_WAVES)         // genes a wave holds in registers
#define RS_KC 32                            // patterns staged per trip: 16 KB of LDS

#define RS_DATA_NONE 0                      // no data: M alone (reconstructGene)
#define RS_DATA_DENSE 1
#define RS_DATA_PACKED 2                    // the gene side of the sparse model's packed form (sparse_build.h)

struct RsArgs {
    const double *a64;                      // [ceil(G / 64) * 64][K]: A widened, rows of zeros past the last gene
    const double *pt64;                     // [K][ldp]: P widened and transposed, zeros from column N on
    size_t ldp;                             // nSteps * 64
    uint32_t G, N, K, nSteps;
    int source;
    const float *data, *unc; size_t rowStride, colStride;      // dense: (gene i, sample j) at [i * rowStride + j * colStride]; unc may be null
    SpbSide side;                           // packed: vector = gene, element = sample
    double *geneChiSq;                      // [G]
    double *partial;                        // [ceil(G / 64)][ldp]
    const uint32_t *outStart, *outList;     // the output rows that want gene i: outList[outStart[i] .. outStart[i + 1]); null: none
    double *matrixOut;                      // [nRowsOut][N]: r, or M without data
};

// the 64 lanes' values added in the order of the ascending xor butterfly; the same bits in every lane (a + b == b + a)
CG_DEVICE double rs_wave_allsum(double x)
{
    for (int off = 1; off < 64; off <<= 1) x = x + cg_shfl_xor_f64(x, off);
    return x;
}

CG_KERNEL void CG_LAUNCH_BOUNDS(RS_THREADS) rs_main_kernel(RsArgs a)
{
    CG_SHARED double pt[RS_KC * 64];
    CG_SHARED double qx[RS_BLOCK * 64];
    const uint32_t lane = cg_tid() & 63u, wave = cg_uniform_u32(cg_tid() >> 6);
    const uint32_t nBlocks = (a.G + (uint32_t)RS_BLOCK - 1u) / (uint32_t)RS_BLOCK;
    for (uint32_t b = cg_bid(); b < nBlocks; b += cg_gdim()) {
        const uint32_t g0 = b * (uint32_t)RS_BLOCK + wave * (uint32_t)RS_GT;      // (g0 + 15 < G + 64 < 2^32: the host refuses more than 2^32 - 256 genes)
        const uint32_t blockGenes = a.G - b * (uint32_t)RS_BLOCK < (uint32_t)RS_BLOCK ? a.G - b * (uint32_t)RS_BLOCK : (uint32_t)RS_BLOCK;
        const double *arows = a.a64 + (size_t)g0 * a.K;                         // (a gene past the last reads a row of zeros and writes nothing)
        double gacc[RS_GT];
#pragma unroll
        for (int t = 0; t < RS_GT; ++t) gacc[t] = 0.0;
        for (uint32_t s = 0; s < a.nSteps; ++s) {
            const size_t j = (size_t)s * 64u + lane;
            const bool liveJ = j < a.N;
            double m[RS_GT];
#pragma unroll
            for (int t = 0; t < RS_GT; ++t) m[t] = 0.0;
            for (uint32_t k0 = 0; k0 < a.K; k0 += (uint32_t)RS_KC) {
                const uint32_t kn = a.K - k0 < (uint32_t)RS_KC ? a.K - k0 : (uint32_t)RS_KC;
                cg_sync();                                                      // the chunk before, and the step before's qx, have been read
                for (uint32_t e = cg_tid(); e < kn * 64u; e += (uint32_t)RS_THREADS) pt[e] = a.pt64[(size_t)(k0 + (e >> 6)) * a.ldp + (size_t)s * 64u + (e & 63u)];
                cg_sync();
                for (uint32_t k = 0; k < kn; ++k) {
                    const double p = pt[k * 64u + lane];
#pragma unroll
                    for (int t = 0; t < RS_GT; ++t) m[t] = cg_fma_f64(arows[(size_t)t * a.K + k0 + k], p, m[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < RS_GT; ++t) {
                const uint32_t i = g0 + (uint32_t)t;
                double q = 0.0;
                if (i < a.G) {                                                  // (the same in every lane of the wave)
                    double out = m[t];
                    if (a.source != RS_DATA_NONE) {
                        float d = 0.f, given = 1.f;                             // (a lane past the last sample computes on 0 and 1 and keeps nothing)
                        if (a.source == RS_DATA_DENSE) {
                            const size_t at = (size_t)i * a.rowStride + j * a.colStride;
                            if (liveJ) d = a.data[at];
                            if (liveJ && a.unc) given = a.unc[at];
                        } else {
                            const size_t w = (size_t)i * a.side.Wn + s;
                            const unsigned long long word = a.side.flags[w];
                            if ((word >> lane) & 1ull) d = a.side.vals[a.side.ptr[i] + a.side.prefix[w] + (uint32_t)cg_popc64(word & ((1ull << lane) - 1ull))];
                        }
                        const double tenth = 0.1 * (double)d;                   // R's pmax(0.1 * data, 0.1), in double
                        const double sd = a.unc ? (double)given : (tenth > 0.1 ? tenth : 0.1);
                        const double r = ((double)d - m[t]) / sd;
                        q = r * r;
                        out = r;
                        if (liveJ) gacc[t] = gacc[t] + q;
                    }
                    if (a.outStart && liveJ)
                        for (uint32_t x = a.outStart[i]; x < a.outStart[i + 1u]; ++x) a.matrixOut[(size_t)a.outList[x] * a.N + j] = out;
                }
                qx[(wave * (uint32_t)RS_GT + (uint32_t)t) * 64u + lane] = liveJ ? q : 0.0;
            }
            cg_sync();
            if (wave == 0u && a.source != RS_DATA_NONE) {
                double col = 0.0;
                for (uint32_t g = 0; g < blockGenes; ++g) col = col + qx[g * 64u + lane];
                a.partial[(size_t)b * a.ldp + j] = col;                         // (j < ldp: the row is padded to whole steps)
            }
        }
        if (a.source != RS_DATA_NONE) {
#pragma unroll
            for (int t = 0; t < RS_GT; ++t) {
                const double sum = rs_wave_allsum(gacc[t]);
                if (lane == 0u && g0 + (uint32_t)t < a.G) a.geneChiSq[g0 + (uint32_t)t] = sum;
            }
        }
    }
}

// sampleChiSq[j] = the partials of column j in ascending block order (workgroups 0 .. ceil(N / 256) - 1, lane = sample); chiSq = the
// gene sums in ascending gene order (the last workgroup: 256 at a time through LDS, one lane adds)
CG_KERNEL void CG_LAUNCH_BOUNDS(RS_THREADS) rs_fold_kernel(RsArgs a, double *sampleChiSq, double *chiSq)
{
    CG_SHARED double chunk[RS_THREADS];
    const uint32_t nBlocks = (a.G + (uint32_t)RS_BLOCK - 1u) / (uint32_t)RS_BLOCK;
    if (cg_bid() + 1u < cg_gdim()) {
        const size_t j = (size_t)cg_bid() * RS_THREADS + cg_tid();
        if (j >= a.N) return;
        double sum = 0.0;
        for (uint32_t b = 0; b < nBlocks; ++b) sum = sum + a.partial[(size_t)b * a.ldp + j];
        sampleChiSq[j] = sum;
        return;
    }
    double total = 0.0;
    for (uint32_t i0 = 0; i0 < a.G; i0 += (uint32_t)RS_THREADS) {
        const uint32_t n = a.G - i0 < (uint32_t)RS_THREADS ? a.G - i0 : (uint32_t)RS_THREADS;
        if (cg_tid() < n) chunk[cg_tid()] = a.geneChiSq[i0 + cg_tid()];
        cg_sync();
        if (cg_tid() == 0u) for (uint32_t e = 0; e < n; ++e) total = total + chunk[e];
        cg_sync();
    }
    if (cg_tid() == 0u) *chiSq = total;
}
