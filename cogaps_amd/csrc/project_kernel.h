// project_kernel.h -- new data projected onto a result's patterns (projectR's lmFit route): for loadings L (n x K, fp32)
// and data D (n x S, fp32 >= 0, the same genes) every sample s is regressed on the loadings by least squares, D[:, s] ~ L c[:, s]:
//   gram[a][b] = sum_g L[g][a] L[g][b]      cross[k][s] = sum_g L[g][k] D[g][s]      gram c = cross      rss[s] = sum_g (D[g][s] - sum_k L[g][k] c[k][s])^2
// in fp64 on exactly widened floats, in an order anyone can repeat:
//   the genes are cut into trips of PJ_TRIP genes, trip t = genes [t * PJ_TRIP, (t + 1) * PJ_TRIP);
//   a trip's partial of a sum adds the trip's genes in ascending order from +0.0; a sum adds the trips' partials in ascending trip order from +0.0;
//   gram, cross   every product is one of two widened floats: exact in fp64, so the FMA used here and a rounded product give the same bits,
//                 and a skipped zero of sparse data changes no bit (a sum that started at +0.0 is never -0.0, and x + (+-0.0) == x);
//   factor        gram = U D U^T, U unit lower triangular, column by column:  w[m] = U[j][m] * D[m];  s = sum_{m < j} U[i][m] * w[m] ascending
//                 from +0.0;  D[j] = gram[j][j] - s (i = j);  U[i][j] = (gram[i][j] - s) / D[j] (i > j);  D[j] <= 1e-12 gram[j][j] is refused;
//   substitute    x = gram^-1 b in place:  z[i] = b[i] - sum_{m < i} U[i][m] * z[m];  y[i] = z[i] / D[i];  c[i] = y[i] - sum_{m > i} U[m][i] * c[m],
//                 i descending; both sums ascending in m from +0.0;  stdevUnscaled[k] = sqrt(x[k]) of the unit right-hand side e_k;
//   fitted        sum_k L[g][k] * c[k][s] ascending in k from +0.0;  r = D - fitted;  rss adds r * r.
// Every product of factor, substitute and fitted is rounded before it is added (no FMA: the build contracts nothing).
// Geometry: lane = sample.  pj_cross_kernel -- the hot one, K n S multiply-adds -- gives a workgroup a (trip, block of 256 samples): a
// wave owns 64 samples, a lane keeps the sums of PJ_KC patterns in registers, and the loadings of PJ_GB genes x PJ_KC patterns are staged
// in LDS widened to fp64, where all 64 lanes read the same word (a broadcast) while each loads its own datum.  The data are read K / PJ_KC
// times, the loadings once per block of samples.  pj_rss_kernel has the same units; a wave holds the fitted values of PJ_RG genes.
// The gene of the fit i is row rows[i] of the data (null: i) -- dense through its strides, or the gene side of the sparse model's packed
// form (sparse_build.h) read as rs_main_kernel reads it.  No floating-point atomics; no workgroup waits for another; the grid only decides
// which workgroup takes which unit.
#pragma once
#include "platform.h"
#include "sparse_build.h"
#include "residual_kernel.h"                // RS_DATA_DENSE, RS_DATA_PACKED

#define PJ_TRIP 1024u                       // genes of a trip: the partials [nTrips][K][S] are 245 MB at 50 000 x 12 500 x 50
#define PJ_MAX_PATTERNS 128u                // the packed triangle of the factor is 66 KB of LDS
#define PJ_TRI(i) ((uint32_t)(i) * ((uint32_t)(i) + 1u) / 2u)      // where row i of a packed lower triangle begins
#define PJ_THREADS 256
#define PJ_KC 32                            // patterns whose sums a lane holds (64 VGPRs)
#define PJ_GB 32u                           // genes staged per tile of the cross-product: 8 KB of LDS
#define PJ_UNROLL 8u                        // genes whose data are loaded before the first is used
#define PJ_RG 16u                           // genes whose fitted values a lane holds in the rss pass: the tile [16][K] is 16 KB of LDS

struct PjArgs {
    const double *l64;                      // [n][K]: the loadings widened
    const uint32_t *rows;                   // [n]: the data row of every gene of the fit, or null
    uint32_t n, K, S, nTrips, nSBlocks;     // nSBlocks = ceil(S / 256)
    int source;                             // RS_DATA_DENSE or RS_DATA_PACKED
    const float *data; size_t rowStride, colStride;      // dense: (data row r, sample j) at [r * rowStride + j * colStride]
    SpbSide side;                           // packed: vector = data row, element = sample
    double *gramPart;                       // [nTrips][K (K + 1) / 2]: the lower triangle, packed
    double *gramTri, *gram;                 // [K (K + 1) / 2]; [K][K]
    double *factor;                         // [K (K + 1) / 2]: U[i][m] at PJ_TRI(i) + m, D[i] at PJ_TRI(i) + i
    double *unit;                           // [K][K]: the unit right-hand sides, column k at unit[i * K + k]
    double *stdev;                          // [K]
    uint32_t *bad;                          // [1]: the first refused pivot, or CG_NONE
    double *crossPart;                      // [nTrips][K][S]
    double *cross, *coef;                   // [K][S]
    double *rssPart, *rss;                  // [nTrips][S]; [S]
};

CG_DEVICE uint32_t pj_rows_of(const PjArgs &a, uint32_t t) { return a.n - t * PJ_TRIP < PJ_TRIP ? a.n - t * PJ_TRIP : PJ_TRIP; }      // (t * PJ_TRIP < n <= 2^32 - 1)

// D[gene][j], j = step * 64 + lane.  The caller's wave has step * 64 < S: the packed form has a flag word for it, whose bits past the last sample are 0
CG_DEVICE float pj_datum(const PjArgs &a, uint32_t gene, size_t j, uint32_t step, uint32_t lane, bool live)
{
    const uint32_t r = a.rows ? a.rows[gene] : gene;
    if (a.source == RS_DATA_DENSE) return live ? a.data[(size_t)r * a.rowStride + j * a.colStride] : 0.f;
    const size_t w = (size_t)r * a.side.Wn + step;
    const unsigned long long word = a.side.flags[w];
    if (!((word >> lane) & 1ull)) return 0.f;
    return a.side.vals[a.side.ptr[r] + a.side.prefix[w] + (uint32_t)cg_popc64(word & ((1ull << lane) - 1ull))];
}

// gramPart[t][PJ_TRI(i) + m] = the trip's sum of L[g][i] L[g][m], m <= i: a workgroup takes a trip, a thread an entry of the triangle
CG_KERNEL void CG_LAUNCH_BOUNDS(PJ_THREADS) pj_gram_kernel(PjArgs a)
{
    const uint32_t K = a.K, tri = PJ_TRI(K);
    for (uint32_t t = cg_bid(); t < a.nTrips; t += cg_gdim()) {
        const uint32_t rows = pj_rows_of(a, t);
        const double *l = a.l64 + (size_t)t * PJ_TRIP * K;
        for (uint32_t e = cg_tid(); e < tri; e += (uint32_t)PJ_THREADS) {
            uint32_t i = 0;
            while (PJ_TRI(i + 1u) <= e) ++i;
            const uint32_t m = e - PJ_TRI(i);
            double s = 0.0;
            for (uint32_t g = 0; g < rows; ++g) s = cg_fma_f64(l[(size_t)g * K + i], l[(size_t)g * K + m], s);
            a.gramPart[(size_t)t * tri + e] = s;
        }
    }
}

// the trips' partials of the triangle in ascending trip order: one thread per entry; gram leaves packed and as the full symmetric matrix
CG_KERNEL void CG_LAUNCH_BOUNDS(PJ_THREADS) pj_gram_fold_kernel(PjArgs a)
{
    const uint32_t K = a.K, tri = PJ_TRI(K);
    const uint32_t e = cg_bid() * (uint32_t)PJ_THREADS + cg_tid();
    if (e >= tri) return;
    double s = 0.0;
    for (uint32_t t = 0; t < a.nTrips; ++t) s = s + a.gramPart[(size_t)t * tri + e];
    uint32_t i = 0;
    while (PJ_TRI(i + 1u) <= e) ++i;
    const uint32_t m = e - PJ_TRI(i);
    a.gramTri[e] = s;
    a.gram[(size_t)i * K + m] = s;
    a.gram[(size_t)m * K + i] = s;
}

// x = gram^-1 x in place, x[i] at x[i * stride], f the packed factor (see the head of the file for the order)
CG_DEVICE void pj_substitute(const double *f, uint32_t K, double *x, size_t stride)
{
    for (uint32_t i = 0; i < K; ++i) {
        const double *row = f + PJ_TRI(i);
        double s = 0.0;
        for (uint32_t m = 0; m < i; ++m) s = s + row[m] * x[(size_t)m * stride];
        x[(size_t)i * stride] = x[(size_t)i * stride] - s;
    }
    for (uint32_t i = 0; i < K; ++i) x[(size_t)i * stride] = x[(size_t)i * stride] / f[PJ_TRI(i) + i];
    for (uint32_t i = K; i-- > 0u;) {
        double s = 0.0;
        for (uint32_t m = i + 1u; m < K; ++m) s = s + f[PJ_TRI(m) + i] * x[(size_t)m * stride];
        x[(size_t)i * stride] = x[(size_t)i * stride] - s;
    }
}

// One workgroup: the factor of gram in LDS, column by column (thread x has row j + x of column j), the rank decision, and the K unit
// right-hand sides (thread k has e_k) for stdevUnscaled.  K <= PJ_MAX_PATTERNS (the host refuses more).
CG_KERNEL void CG_LAUNCH_BOUNDS(PJ_THREADS) pj_factor_kernel(PjArgs a)
{
    CG_SHARED double f[PJ_TRI(PJ_MAX_PATTERNS)];
    CG_SHARED double w[PJ_MAX_PATTERNS];
    CG_SHARED uint32_t bad;
    const uint32_t K = a.K, tri = PJ_TRI(K), tid = cg_tid();
    for (uint32_t e = tid; e < tri; e += (uint32_t)PJ_THREADS) f[e] = a.gramTri[e];
    if (tid == 0u) bad = CG_NONE;
    cg_sync();
    for (uint32_t j = 0; j < K; ++j) {
        if (tid < j) w[tid] = f[PJ_TRI(j) + tid] * f[PJ_TRI(tid) + tid];
        cg_sync();
        const uint32_t i = j + tid;
        double v = 0.0;
        if (i < K) {
            const double *row = f + PJ_TRI(i);
            double s = 0.0;
            for (uint32_t m = 0; m < j; ++m) s = s + row[m] * w[m];
            v = row[j] - s;
            if (i == j) {
                if (!(v > 1e-12 * row[j])) bad = j;
                f[PJ_TRI(j) + j] = v;
            }
        }
        cg_sync();
        if (bad != CG_NONE) break;                                              // (the same in every thread)
        if (i > j && i < K) f[PJ_TRI(i) + j] = v / f[PJ_TRI(j) + j];
        cg_sync();
    }
    if (tid == 0u) *a.bad = bad;
    if (bad != CG_NONE) return;
    for (uint32_t e = tid; e < tri; e += (uint32_t)PJ_THREADS) a.factor[e] = f[e];
    if (tid < K) {
        a.unit[(size_t)tid * K + tid] = 1.0;                                    // (the rest of the column is the allocation's zeros)
        pj_substitute(f, K, a.unit + tid, K);
        a.stdev[tid] = sqrt(a.unit[(size_t)tid * K + tid]);
    }
}

// crossPart[t][k][j] = the trip's sum of L[g][k] D[g][j]: a workgroup takes a (trip, block of 256 samples), wave w its samples
// [(4 sb + w) 64, + 64)
CG_KERNEL void CG_LAUNCH_BOUNDS(PJ_THREADS) pj_cross_kernel(PjArgs a)
{
    CG_SHARED double lt[PJ_GB * PJ_KC];                                         // [gene of the tile][pattern of the chunk], zeros past either end
    const uint32_t lane = cg_tid() & 63u, wave = cg_uniform_u32(cg_tid() >> 6), K = a.K;
    const unsigned long long units = (unsigned long long)a.nTrips * a.nSBlocks;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t t = (uint32_t)(u / a.nSBlocks), sb = (uint32_t)(u % a.nSBlocks);
        const uint32_t g0 = t * PJ_TRIP, rows = pj_rows_of(a, t);
        const uint32_t step = sb * 4u + wave;                                   // (< 2^26)
        const size_t j = (size_t)step * 64u + lane;
        const bool waveLive = (size_t)step * 64u < a.S, live = j < a.S;
        for (uint32_t k0 = 0; k0 < K; k0 += (uint32_t)PJ_KC) {
            const uint32_t kn = K - k0 < (uint32_t)PJ_KC ? K - k0 : (uint32_t)PJ_KC;
            double acc[PJ_KC];
#pragma unroll
            for (int k = 0; k < PJ_KC; ++k) acc[k] = 0.0;
            for (uint32_t gb = 0; gb < rows; gb += PJ_GB) {
                const uint32_t gn = rows - gb < PJ_GB ? rows - gb : PJ_GB;
                cg_sync();                                                      // the tile before has been read
                for (uint32_t e = cg_tid(); e < PJ_GB * (uint32_t)PJ_KC; e += (uint32_t)PJ_THREADS) {
                    const uint32_t g = e / (uint32_t)PJ_KC, k = e % (uint32_t)PJ_KC;
                    lt[e] = g < gn && k < kn ? a.l64[(size_t)(g0 + gb + g) * K + k0 + k] : 0.0;
                }
                cg_sync();
                if (!waveLive) continue;
                for (uint32_t x0 = 0; x0 < gn; x0 += PJ_UNROLL) {
                    float v[PJ_UNROLL];
#pragma unroll
                    for (uint32_t x = 0; x < PJ_UNROLL; ++x) v[x] = x0 + x < gn ? pj_datum(a, g0 + gb + x0 + x, j, step, lane, live) : 0.f;
#pragma unroll
                    for (uint32_t x = 0; x < PJ_UNROLL; ++x) {                  // (a gene past the tile's last adds 0 * 0 to sums that are never -0)
                        const double d = (double)v[x];
                        const double *lr = lt + (x0 + x) * (uint32_t)PJ_KC;
#pragma unroll
                        for (int k = 0; k < PJ_KC; ++k) acc[k] = cg_fma_f64(lr[k], d, acc[k]);
                    }
                }
            }
            if (live) {
#pragma unroll
                for (int k = 0; k < PJ_KC; ++k)
                    if ((uint32_t)k < kn) a.crossPart[((size_t)t * K + k0 + (uint32_t)k) * a.S + j] = acc[k];
            }
        }
    }
}

// out[e] (and copy[e], if given) = part[0][e] + part[1][e] + ... in ascending trip order from +0.0: one thread per sum
CG_KERNEL void CG_LAUNCH_BOUNDS(PJ_THREADS) pj_fold_kernel(const double *part, size_t count, uint32_t nTrips, double *out, double *copy)
{
    const size_t e = (size_t)cg_bid() * PJ_THREADS + cg_tid();
    if (e >= count) return;
    double s = 0.0;
    for (uint32_t t = 0; t < nTrips; ++t) s = s + part[(size_t)t * count + e];
    out[e] = s;
    if (copy) copy[e] = s;
}

// coef[:, j] = gram^-1 coef[:, j] in place, lane = sample, the factor read from LDS (every lane the same word)
CG_KERNEL void CG_LAUNCH_BOUNDS(PJ_THREADS) pj_solve_kernel(PjArgs a)
{
    CG_SHARED double f[PJ_TRI(PJ_MAX_PATTERNS)];
    const uint32_t tri = PJ_TRI(a.K);
    for (uint32_t e = cg_tid(); e < tri; e += (uint32_t)PJ_THREADS) f[e] = a.factor[e];
    cg_sync();
    const size_t j = (size_t)cg_bid() * PJ_THREADS + cg_tid();
    if (j < a.S) pj_substitute(f, a.K, a.coef + j, a.S);
}

// rssPart[t][j] = the trip's sum of (D[g][j] - fitted)^2: the units of pj_cross_kernel; a tile of PJ_RG genes' loadings in LDS
CG_KERNEL void CG_LAUNCH_BOUNDS(PJ_THREADS) pj_rss_kernel(PjArgs a)
{
    CG_SHARED double lt[PJ_RG * PJ_MAX_PATTERNS];                               // [gene of the tile][K], zeros past the last gene
    const uint32_t lane = cg_tid() & 63u, wave = cg_uniform_u32(cg_tid() >> 6), K = a.K;
    const unsigned long long units = (unsigned long long)a.nTrips * a.nSBlocks;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t t = (uint32_t)(u / a.nSBlocks), sb = (uint32_t)(u % a.nSBlocks);
        const uint32_t g0 = t * PJ_TRIP, rows = pj_rows_of(a, t);
        const uint32_t step = sb * 4u + wave;
        const size_t j = (size_t)step * 64u + lane;
        const bool waveLive = (size_t)step * 64u < a.S, live = j < a.S;
        double acc = 0.0;
        for (uint32_t gb = 0; gb < rows; gb += PJ_RG) {
            const uint32_t gn = rows - gb < PJ_RG ? rows - gb : PJ_RG;
            cg_sync();
            for (uint32_t e = cg_tid(); e < PJ_RG * K; e += (uint32_t)PJ_THREADS) lt[e] = e / K < gn ? a.l64[(size_t)(g0 + gb) * K + e] : 0.0;
            cg_sync();
            if (!waveLive) continue;
            float v[PJ_RG];
            double m[PJ_RG];
#pragma unroll
            for (uint32_t x = 0; x < PJ_RG; ++x) { v[x] = x < gn ? pj_datum(a, g0 + gb + x, j, step, lane, live) : 0.f; m[x] = 0.0; }
            for (uint32_t k = 0; k < K; ++k) {
                const double c = live ? a.coef[(size_t)k * a.S + j] : 0.0;
#pragma unroll
                for (uint32_t x = 0; x < PJ_RG; ++x) m[x] = m[x] + lt[x * K + k] * c;
            }
#pragma unroll
            for (uint32_t x = 0; x < PJ_RG; ++x)
                if (x < gn) { const double r = (double)v[x] - m[x]; acc = acc + r * r; }
        }
        if (live) a.rssPart[(size_t)t * a.S + j] = acc;
    }
}
