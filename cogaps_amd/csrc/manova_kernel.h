// manova_kernel.h -- the sums MANOVA stands on (R/methods-CogapsResult.R:596-619): for a predictor matrix X (n x K, fp32:
// a result's patterns) and a response matrix Y (n x p, fp64: the factor codes, p <= MV_MAX_RESP) the column means and the centred sums of
// squares and cross-products
//   xMean[k], yMean[j],  sxx[k] = sum (x_ik - xMean[k])^2,  sxy[k][j] = sum (x_ik - xMean[k]) (y_ij - yMean[j]),
//   syy[a][b] = sum (y_ia - yMean[a]) (y_ib - yMean[b])
// in two passes -- the means first, then the centred products: a pattern with a large offset and a small spread keeps its digits -- and
// in fp64 throughout (a widened float is exact), in an order anyone can repeat:
//   the rows are cut into trips of MV_TRIP rows, trip t = rows [t * MV_TRIP, (t + 1) * MV_TRIP);
//   a trip's partial of a sum adds the trip's rows in ascending row order from +0.0, the product rounded before it is added (no FMA);
//   a sum adds the trips' partials in ascending trip order from +0.0;  a mean is its sum / (double)n;
//   a centred value is value - mean, rounded once.
// Layout: lane = column.  X lies row-major without padding ([n][K], the repacked -- or, row-major already, the caller's own -- upload), so
// the 64 lanes of a wave read 64 consecutive floats of one row and the rows of a trip follow one another in memory: every byte of every
// line fetched is used, once per pass.  Y lies row-major as well ([n][p]).  A workgroup takes a trip; its waves share the blocks of 64
// columns among them (wave w: blocks w, w + waves, ...), and a lane walks its column down the trip's rows with its sums in registers: no
// value crosses a lane, so there is no butterfly to specify, and K's split over waves and workgroups decides nothing.  Pass 1 treats Y's
// columns as columns K .. K + p - 1 of the same walk.  Pass 2 stages the trip's centred Y rows in LDS once per workgroup ([row][p], 16 KB
// at p = 8), where every lane reads the same word (a broadcast); one further block of lanes, a < p, b < p on lane a * p + b, adds syy from
// LDS alone.  X is read from memory exactly twice and Y twice.  The grid only decides which workgroup takes which trip; the fold kernels
// add the trips' partials, one thread per sum.  No floating-point atomics, no workgroup waits for another.
#pragma once
#include "platform.h"

#define MV_TRIP 256u                    // rows of a trip
#define MV_MAX_RESP 8u                  // columns of Y
#define MV_THREADS 256                  // at most; a launch has as many waves as there are blocks of 64 columns, up to four
#define MV_UNROLL 8u                    // rows whose loads are issued before the first is added

struct MvArgs {
    const float *x;                     // [n][K]
    const double *y;                    // [n][p]
    uint32_t n, K, p, nTrips;
    double *part1;                      // [nTrips][K + p]: the trips' sums of X's columns, then of Y's
    double *mean;                       // [K + p]: xMean, yMean
    double *part2;                      // [nTrips][K + K * p + p * p]: sxx[k] at k, sxy[k][j] at K + j * K + k, syy[a][b] at K + K * p + a * p + b
    double *out2;                       // [K + K * p + p * p]: sxx, sxy ([k][j] at K + k * p + j), syy
};

CG_DEVICE uint32_t mv_rows_of(const MvArgs &a, uint32_t t) { return a.n - t * MV_TRIP < MV_TRIP ? a.n - t * MV_TRIP : MV_TRIP; }      // (t * MV_TRIP < n <= 2^32 - 1)

// pass 1: part1[t][q] = the sum of column q of [X | Y] over trip t
CG_KERNEL void CG_LAUNCH_BOUNDS(MV_THREADS) mv_sum_kernel(MvArgs a)
{
    const uint32_t lane = cg_tid() & 63u, wave = cg_uniform_u32(cg_tid() >> 6), waves = cg_bdim() >> 6;
    const uint32_t cols = a.K + a.p, nBlocks = (cols + 63u) / 64u;
    for (uint32_t t = cg_bid(); t < a.nTrips; t += cg_gdim()) {
        const uint32_t rows = mv_rows_of(a, t);
        const size_t row0 = (size_t)t * MV_TRIP;
        for (uint32_t c = wave; c < nBlocks; c += waves) {
            const uint32_t q = c * 64u + lane;
            if (q >= cols) continue;
            double s = 0.0;
            if (q < a.K) {
                const float *col = a.x + row0 * a.K + q;
                uint32_t r = 0;
                for (; r + MV_UNROLL <= rows; r += MV_UNROLL) {
                    float v[MV_UNROLL];
#pragma unroll
                    for (uint32_t u = 0; u < MV_UNROLL; ++u) v[u] = col[(size_t)(r + u) * a.K];
#pragma unroll
                    for (uint32_t u = 0; u < MV_UNROLL; ++u) s = s + (double)v[u];
                }
                for (; r < rows; ++r) s = s + (double)col[(size_t)r * a.K];
            } else {
                const double *col = a.y + row0 * a.p + (q - a.K);
                for (uint32_t r = 0; r < rows; ++r) s = s + col[(size_t)r * a.p];
            }
            a.part1[(size_t)t * cols + q] = s;
        }
    }
}

// mean[q] = (the trips' sums of column q in ascending trip order) / n: one thread per column
CG_KERNEL void CG_LAUNCH_BOUNDS(MV_THREADS) mv_mean_kernel(MvArgs a)
{
    const uint32_t cols = a.K + a.p;
    const size_t q = (size_t)cg_bid() * cg_bdim() + cg_tid();
    if (q >= cols) return;
    double s = 0.0;
    for (uint32_t t = 0; t < a.nTrips; ++t) s = s + a.part1[(size_t)t * cols + q];
    a.mean[q] = s / (double)a.n;
}

// pass 2: part2[t][..] = the centred squares and products of trip t
CG_KERNEL void CG_LAUNCH_BOUNDS(MV_THREADS) mv_sscp_kernel(MvArgs a)
{
    CG_SHARED double dy[MV_TRIP * MV_MAX_RESP];                                     // [row of the trip][p]: y - yMean
    const uint32_t lane = cg_tid() & 63u, wave = cg_uniform_u32(cg_tid() >> 6), waves = cg_bdim() >> 6;
    const uint32_t K = a.K, p = a.p, xBlocks = (K + 63u) / 64u, outs = K + K * p + p * p;
    for (uint32_t t = cg_bid(); t < a.nTrips; t += cg_gdim()) {
        const uint32_t rows = mv_rows_of(a, t);
        const size_t row0 = (size_t)t * MV_TRIP;
        cg_sync();                                                                  // the trip before has been read
        for (uint32_t e = cg_tid(); e < rows * p; e += cg_bdim()) dy[e] = a.y[row0 * p + e] - a.mean[K + e % p];
        cg_sync();
        double *part = a.part2 + (size_t)t * outs;
        for (uint32_t c = wave; c <= xBlocks; c += waves) {
            if (c == xBlocks) {                                                     // syy: lane = (a, b)
                if (lane >= p * p) continue;
                const uint32_t ya = lane / p, yb = lane % p;
                double s = 0.0;
                for (uint32_t r = 0; r < rows; ++r) s = s + dy[r * p + ya] * dy[r * p + yb];
                part[K + K * p + lane] = s;
                continue;
            }
            const uint32_t k = c * 64u + lane;
            if (k >= K) continue;
            const float *col = a.x + row0 * K + k;
            const double xm = a.mean[k];
            double sxx = 0.0, sxy[MV_MAX_RESP];
#pragma unroll
            for (uint32_t j = 0; j < MV_MAX_RESP; ++j) sxy[j] = 0.0;
            for (uint32_t r0 = 0; r0 < rows; r0 += MV_UNROLL) {
                const uint32_t here = rows - r0 < MV_UNROLL ? rows - r0 : MV_UNROLL;
                float v[MV_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < MV_UNROLL; ++u) v[u] = u < here ? col[(size_t)(r0 + u) * K] : 0.f;
#pragma unroll
                for (uint32_t u = 0; u < MV_UNROLL; ++u) {
                    if (u < here) {                                                 // (the same in every lane)
                        const double dx = (double)v[u] - xm;
                        sxx = sxx + dx * dx;
#pragma unroll
                        for (uint32_t j = 0; j < MV_MAX_RESP; ++j)
                            if (j < p) sxy[j] = sxy[j] + dx * dy[(r0 + u) * p + j];
                    }
                }
            }
            part[k] = sxx;
#pragma unroll
            for (uint32_t j = 0; j < MV_MAX_RESP; ++j)
                if (j < p) part[K + j * K + k] = sxy[j];
        }
    }
}

// out2[..] = the trips' partials in ascending trip order: one thread per sum; sxy leaves as [k][j]
CG_KERNEL void CG_LAUNCH_BOUNDS(MV_THREADS) mv_fold_kernel(MvArgs a)
{
    const uint32_t K = a.K, p = a.p, outs = K + K * p + p * p;
    const size_t e = (size_t)cg_bid() * cg_bdim() + cg_tid();
    if (e >= outs) return;
    double s = 0.0;
    for (uint32_t t = 0; t < a.nTrips; ++t) s = s + a.part2[(size_t)t * outs + e];
    size_t to = e;
    if (e >= K && e < (size_t)K + (size_t)K * p) { const size_t j = (e - K) / K, k = (e - K) % K; to = K + k * p + j; }
    a.out2[to] = s;
}
