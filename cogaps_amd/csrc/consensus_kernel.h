// consensus_kernel.h -- the step between the two passes of a distributed run (findConsensusMatrix / patternMatch,
// R/DistributedCogaps.R:129-217): the correlation distance of the gathered patterns, complete-linkage clustering of
// it, and the weighted mean pattern of every cluster.  fp64 on exactly widened fp32 values, every product rounded before it is added
// (the build contracts nothing), no floating-point atomics, and one rule for every sum over the L rows:
//   rows are cut into chunks of CS_KC consecutive rows; a chunk's terms are added in ascending row order from +0.0, the chunk sums in
//   ascending chunk order from +0.0
// so that every output can be recomputed bit for bit (tests/consensus_cases.py) and none depends on grid, scheduling or device.
//   cs_stage_kernel        X, any strides, into row-major rows of whole 64-column tiles (LDS transpose: reads and writes are both
//                          coalesced, whichever axis of X is contiguous); -0 becomes +0; a NaN or negative value raises a flag
//   cs_colsum_kernel, cs_mean_kernel   the column sums of a chunk, then the means (sum / L)
//   cs_cross_kernel        c[i][j] = sum over k of (x[k][i] - mean[i]) * (x[k][j] - mean[j]): a workgroup per 64 x 64 tile of the upper
//                          triangle, a thread per 4 x 4 outputs, the rows walked in ascending order through LDS, the chunk sums folded
//                          in registers; each pair is computed on its own, so a subset's matrix is the sub-block of the full one
//   cs_dist_kernel         dist[i][j] = 1 - c[i][j] / (sqrt(c[i][i]) * sqrt(c[j][j]))
//   cs_gather_kernel       the sub-block of dist of a list of columns: the matrix one clustering works on (and destroys)
//   cs_link_kernel         complete linkage down to k clusters by ONE persistent workgroup: per active row its nearest neighbour among
//                          the active columns above it (smallest distance, ties to the lowest column) in LDS; per merge the global
//                          minimum (ties to the lowest row), row / column lo = max(row lo, row hi), hi retired, and the neighbour of lo
//                          and of every row whose neighbour was lo or hi found again -- complete-linkage distances never decrease, so
//                          no other row's minimum changes.  The merge list goes to the host, which numbers the labels
//   cs_meanpat_kernel .. cs_consensus_kernel   per cluster: the mean pattern, each member's rounded correlation with it, the mean
//                          weighted by the cubed correlations, its maximum, the float32 consensus column
#pragma once
#include "platform.h"
#include <math.h>

#define CS_KC 4096u                          // rows of a chunk of the row rule: part of the definition, not a launch parameter
#define CS_THREADS 256
#define CS_TILE 64u                          // columns (and staged rows) of a tile
#define CS_KB 16u                            // rows of both tiles' columns staged per trip: 16 KB of LDS (divides CS_KC)
#define CS_LINK_THREADS 1024
#define CS_LINK_WAVES (CS_LINK_THREADS / 64)
#define CS_MAX_COLS 4096u                    // what the clustering workgroup keeps in LDS: 8 + 4 + 1 + 2 bytes per column = 60 KB of the 64 KB a kernel declares statically

#define CS_FLAG_INPUT 0                      // a NaN or negative value in X
#define CS_FLAG_DIST 1                       // a NaN in dist
#define CS_FLAG_CORR 2                       // a NaN correlation with a mean pattern

struct CsArgs {
    const float *x; size_t rowStride, colStride;      // the caller's matrix: (k, j) at x[k * rowStride + j * colStride]
    uint32_t L, n, nChunks;                            // rows, columns, ceil(L / CS_KC)
    float *xr; size_t ldx;                             // [L][ldx]: staged, ldx = n rounded up to whole tiles, zeros past column n
    double *partial;                                   // [nChunks][ldx]: column sums of a chunk
    double *mean;                                      // [ldx]
    double *c, *dist;                                  // [n][ldx]
    uint32_t *flags;                                   // [3]: CS_FLAG_*
};

// the statistics of the clusters: S = T member slots (cluster by cluster, ascending columns), then one slot per cluster
struct CsClusterArgs {
    const float *xr; size_t ldx;
    const double *mean, *c;
    uint32_t L, nChunks, nC, T;
    const uint32_t *start;                             // [nC + 1]: slots of cluster c
    const uint32_t *slotCol, *slotCluster;             // [T]
    size_t ldc;                                        // nC rounded up to whole 128-byte lines
    double *mp, *mpw;                                  // [L][ldc]: mean pattern, weighted mean pattern
    double *partial, *mpMean;                          // [nChunks][ldc], [ldc]
    double *cpart;                                     // [nChunks][T + nC]: chunk sums of the slots' centred cross-products
    double *r, *w;                                     // [T]
    double *maxPart;                                   // [nChunks][ldc]
    float *consensus;                                  // [L][nC]
    uint32_t *flags;
};

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_stage_kernel(CsArgs a)
{
    CG_SHARED float tile[CS_TILE * (CS_TILE + 1u)];
    const unsigned long long tilesC = a.ldx / CS_TILE, tilesR = ((unsigned long long)a.L + CS_TILE - 1u) / CS_TILE;
    const bool colsAdjacent = a.colStride <= a.rowStride;
    for (unsigned long long t = cg_bid(); t < tilesR * tilesC; t += cg_gdim()) {
        const size_t r0 = (size_t)(t / tilesC) * CS_TILE, c0 = (size_t)(t % tilesC) * CS_TILE;
        for (uint32_t e = cg_tid(); e < CS_TILE * CS_TILE; e += (uint32_t)CS_THREADS) {
            const uint32_t lr = colsAdjacent ? e >> 6 : e & 63u, lc = colsAdjacent ? e & 63u : e >> 6;
            float v = 0.f;
            if (r0 + lr < a.L && c0 + lc < a.n) {
                v = a.x[(r0 + lr) * a.rowStride + (c0 + lc) * a.colStride];
                if (!(v >= 0.f)) cg_atomic_or_u32(a.flags + CS_FLAG_INPUT, 1u);
                v = v + 0.f;
            }
            tile[lr * (CS_TILE + 1u) + lc] = v;
        }
        cg_sync();
        for (uint32_t e = cg_tid(); e < CS_TILE * CS_TILE; e += (uint32_t)CS_THREADS) {
            const uint32_t lr = e >> 6, lc = e & 63u;
            if (r0 + lr < a.L) a.xr[(r0 + lr) * a.ldx + c0 + lc] = tile[lr * (CS_TILE + 1u) + lc];
        }
        cg_sync();
    }
}

// partial[chunk][j] = the sum of rows [chunk * CS_KC, ...) of column j of m ([L][ld], nc columns), ascending from +0.0
template <class T>
CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_colsum_kernel(const T *m, size_t ld, uint32_t L, uint32_t nc, uint32_t nChunks, double *partial, size_t ldp)
{
    const unsigned long long colBlocks = ((unsigned long long)nc + CS_THREADS - 1u) / CS_THREADS;
    for (unsigned long long u = cg_bid(); u < colBlocks * nChunks; u += cg_gdim()) {
        const uint32_t chunk = (uint32_t)(u / colBlocks), j = (uint32_t)(u % colBlocks) * (uint32_t)CS_THREADS + cg_tid();
        if (j >= nc) continue;
        const uint32_t k0 = chunk * CS_KC, k1 = L - k0 < CS_KC ? L : k0 + CS_KC;
        double acc = 0.0;
        for (uint32_t k = k0; k < k1; ++k) acc = acc + (double)m[(size_t)k * ld + j];
        partial[(size_t)chunk * ldp + j] = acc;
    }
}

// the chunk sums of a slot in ascending chunk order from +0.0
CG_DEVICE double cs_fold(const double *partial, size_t ld, uint32_t nChunks, size_t j)
{
    double total = 0.0;
    for (uint32_t ch = 0; ch < nChunks; ++ch) total = total + partial[(size_t)ch * ld + j];
    return total;
}

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_mean_kernel(const double *partial, size_t ldp, uint32_t L, uint32_t nc, uint32_t nChunks, double *mean)
{
    for (unsigned long long j = (unsigned long long)cg_bid() * CS_THREADS + cg_tid(); j < nc; j += (unsigned long long)cg_gdim() * CS_THREADS)
        mean[j] = cs_fold(partial, ldp, nChunks, (size_t)j) / (double)L;
}

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_cross_kernel(CsArgs a)
{
    CG_SHARED double yi[CS_KB * CS_TILE];
    CG_SHARED double yj[CS_KB * CS_TILE];
    const uint32_t tiles = (uint32_t)(a.ldx / CS_TILE), pairs = tiles * (tiles + 1u) / 2u;
    const uint32_t ty = cg_tid() >> 4, tx = cg_tid() & 15u, lc = cg_tid() & 63u, lr0 = cg_tid() >> 6;
    for (uint32_t p = cg_bid(); p < pairs; p += cg_gdim()) {
        uint32_t tj = 0;                                                       // pair p of the upper triangle: ti <= tj, column by column
        while ((tj + 1u) * (tj + 2u) / 2u <= p) ++tj;
        const uint32_t ti = p - tj * (tj + 1u) / 2u;
        const size_t i0 = (size_t)ti * CS_TILE, j0 = (size_t)tj * CS_TILE;
        const double mi = a.mean[i0 + lc], mj = a.mean[j0 + lc];               // (the means' array is padded with zeros like the rows)
        double total[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) total[u][v] = 0.0;
        for (uint32_t c0 = 0; c0 < a.L; c0 += CS_KC) {
            const uint32_t cn = a.L - c0 < CS_KC ? a.L - c0 : CS_KC;
            double acc[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
            for (uint32_t k0 = 0; k0 < cn; k0 += CS_KB) {
                const uint32_t kn = cn - k0 < CS_KB ? cn - k0 : CS_KB;
                cg_sync();                                                     // the trip before has been read
                for (uint32_t lr = lr0; lr < kn; lr += (uint32_t)CS_THREADS / 64u) {
                    const float *row = a.xr + (size_t)(c0 + k0 + lr) * a.ldx;
                    yi[lr * CS_TILE + lc] = (double)row[i0 + lc] - mi;
                    yj[lr * CS_TILE + lc] = (double)row[j0 + lc] - mj;
                }
                cg_sync();
                for (uint32_t kk = 0; kk < kn; ++kk) {
                    double vi[4], vj[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { vi[u] = yi[kk * CS_TILE + ty * 4u + (uint32_t)u]; vj[u] = yj[kk * CS_TILE + tx + 16u * (uint32_t)u]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v) acc[u][v] = acc[u][v] + vi[u] * vj[v];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) total[u][v] = total[u][v] + acc[u][v];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const size_t i = i0 + ty * 4u + (uint32_t)u, j = j0 + tx + 16u * (uint32_t)v;
                if (i < a.n && j < a.n) { a.c[i * a.ldx + j] = total[u][v]; a.c[j * a.ldx + i] = total[u][v]; }      // (y_i * y_j == y_j * y_i: a diagonal tile writes the same bits twice)
            }
    }
}

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_dist_kernel(CsArgs a)
{
    const unsigned long long all = (unsigned long long)a.n * a.n;
    for (unsigned long long e = (unsigned long long)cg_bid() * CS_THREADS + cg_tid(); e < all; e += (unsigned long long)cg_gdim() * CS_THREADS) {
        const size_t i = (size_t)(e / a.n), j = (size_t)(e % a.n);
        const double si = sqrt(a.c[i * a.ldx + i]), sj = sqrt(a.c[j * a.ldx + j]);
        const double d = 1.0 - a.c[i * a.ldx + j] / (si * sj);
        if (d != d) cg_atomic_or_u32(a.flags + CS_FLAG_DIST, 1u);
        a.dist[i * a.ldx + j] = d;
    }
}

// w[a][b] = dist[cols[a]][cols[b]] (cols null: the whole matrix)
CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_gather_kernel(const double *dist, size_t ld, const uint32_t *cols, uint32_t m, double *w, size_t ldw)
{
    const unsigned long long all = (unsigned long long)m * m;
    for (unsigned long long e = (unsigned long long)cg_bid() * CS_THREADS + cg_tid(); e < all; e += (unsigned long long)cg_gdim() * CS_THREADS) {
        const uint32_t ra = (uint32_t)(e / m), rb = (uint32_t)(e % m);
        const size_t i = cols ? cols[ra] : ra, j = cols ? cols[rb] : rb;
        w[(size_t)ra * ldw + rb] = dist[i * ld + j];
    }
}

// the smaller of (d, i) and the other lanes' by (distance, then index), in every lane of the wave
CG_DEVICE void cs_wave_min(double &d, uint32_t &i)
{
    for (int off = 1; off < 64; off <<= 1) {
        const double od = cg_shfl_xor_f64(d, off);
        const uint32_t oi = cg_shfl_xor_u32(i, off);
        if (od < d || (od == d && oi < i)) { d = od; i = oi; }
    }
}

// the nearest neighbour of row a among the active columns above it (all 64 lanes of a wave call it)
CG_DEVICE void cs_row_nn(const double *w, size_t ldw, uint32_t m, uint32_t a, const unsigned char *alive, double *nnD, uint32_t *nnI)
{
    double best = INFINITY; uint32_t at = CG_NONE;
    for (uint32_t b = a + 1u + (cg_tid() & 63u); b < m; b += 64u) {
        if (!alive[b]) continue;
        const double v = w[(size_t)a * ldw + b];
        if (v < best) { best = v; at = b; }
    }
    cs_wave_min(best, at);
    if ((cg_tid() & 63u) == 0u) { nnD[a] = best; nnI[a] = at; }
}

// complete linkage of the m x m matrix w (symmetric; destroyed) down to k clusters, 2 <= m <= CS_MAX_COLS, 1 <= k < m: merge s joins
// cluster merges[2 s + 1] into merges[2 s] (the lower index, which the joined cluster keeps).  One workgroup.
CG_KERNEL void CG_LAUNCH_BOUNDS(CS_LINK_THREADS) cs_link_kernel(double *w, size_t ldw, uint32_t m, uint32_t k, uint32_t *merges)
{
    CG_SHARED double nnD[CS_MAX_COLS];
    CG_SHARED uint32_t nnI[CS_MAX_COLS];
    CG_SHARED unsigned short todo[CS_MAX_COLS];
    CG_SHARED unsigned char alive[CS_MAX_COLS];
    CG_SHARED double redD[CS_LINK_WAVES];
    CG_SHARED uint32_t redI[CS_LINK_WAVES];
    CG_SHARED uint32_t nTodo;
    const uint32_t tid = cg_tid(), lane = tid & 63u, wave = cg_uniform_u32(tid >> 6);
    for (uint32_t a = tid; a < m; a += (uint32_t)CS_LINK_THREADS) alive[a] = 1;
    cg_sync();
    for (uint32_t a = wave; a < m; a += (uint32_t)CS_LINK_WAVES) cs_row_nn(w, ldw, m, a, alive, nnD, nnI);
    cg_sync();
    for (uint32_t step = 0; step + k < m; ++step) {
        // 1. the closest pair: the smallest neighbour distance, ties to the lowest row (its neighbour is its lowest closest column)
        double best = INFINITY; uint32_t at = CG_NONE;
        for (uint32_t a = tid; a < m; a += (uint32_t)CS_LINK_THREADS)
            if (alive[a] && nnD[a] < best) { best = nnD[a]; at = a; }
        cs_wave_min(best, at);
        if (lane == 0u) { redD[wave] = best; redI[wave] = at; }
        if (tid == 0u) nTodo = 0u;
        cg_sync();
        best = redD[0]; at = redI[0];
        for (uint32_t v = 1; v < (uint32_t)CS_LINK_WAVES; ++v)
            if (redD[v] < best || (redD[v] == best && redI[v] < at)) { best = redD[v]; at = redI[v]; }
        const uint32_t lo = at, hi = nnI[lo < m ? lo : 0u];
        if (lo >= m || hi >= m) return;                                         // (no pair is left: not reached with k >= 1 and distances that are numbers; the same in every thread)
        // 2. row and column lo become the element-wise maximum of lo's and hi's; who has to look for a neighbour again
        for (uint32_t o = tid; o < m; o += (uint32_t)CS_LINK_THREADS) {
            if (!alive[o] || o == hi) continue;
            if (o != lo) {
                const double x = w[(size_t)lo * ldw + o], y = w[(size_t)hi * ldw + o], v = y > x ? y : x;
                w[(size_t)lo * ldw + o] = v; w[(size_t)o * ldw + lo] = v;
            }
            if (o == lo || nnI[o] == lo || nnI[o] == hi) todo[cg_atomic_add_u32(&nTodo, 1u)] = (unsigned short)o;
        }
        if (tid == 0u) { merges[2u * step] = lo; merges[2u * step + 1u] = hi; alive[hi] = 0; }
        cg_sync();
        // 3. their neighbours, a wave per row
        const uint32_t nt = nTodo;
        for (uint32_t t = wave; t < nt; t += (uint32_t)CS_LINK_WAVES) cs_row_nn(w, ldw, m, todo[t], alive, nnD, nnI);
        cg_sync();
    }
}

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_meanpat_kernel(CsClusterArgs a)
{
    const unsigned long long all = (unsigned long long)a.L * a.nC;
    for (unsigned long long e = (unsigned long long)cg_bid() * CS_THREADS + cg_tid(); e < all; e += (unsigned long long)cg_gdim() * CS_THREADS) {
        const size_t k = (size_t)(e / a.nC); const uint32_t c = (uint32_t)(e % a.nC);
        double sum = 0.0;
        for (uint32_t t = a.start[c]; t < a.start[c + 1u]; ++t) sum = sum + (double)a.xr[k * a.ldx + a.slotCol[t]];
        a.mp[k * a.ldc + c] = sum / (double)(a.start[c + 1u] - a.start[c]);
    }
}

// cpart[chunk][s]: slot s < T: the chunk's sum of (x[k][col] - mean[col]) * (mp[k][cluster] - mpMean[cluster]); slot T + c: of (mp[k][c] - mpMean[c])^2
CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_cluster_cross_kernel(CsClusterArgs a)
{
    const uint32_t S = a.T + a.nC;
    const unsigned long long slotBlocks = ((unsigned long long)S + CS_THREADS - 1u) / CS_THREADS;
    for (unsigned long long u = cg_bid(); u < slotBlocks * a.nChunks; u += cg_gdim()) {
        const uint32_t chunk = (uint32_t)(u / slotBlocks), s = (uint32_t)(u % slotBlocks) * (uint32_t)CS_THREADS + cg_tid();
        if (s >= S) continue;
        const uint32_t k0 = chunk * CS_KC, k1 = a.L - k0 < CS_KC ? a.L : k0 + CS_KC;
        const bool member = s < a.T;
        const uint32_t c = member ? a.slotCluster[s] : s - a.T, col = member ? a.slotCol[s] : 0u;
        const double mc = member ? a.mean[col] : 0.0, mm = a.mpMean[c];
        double acc = 0.0;
        for (uint32_t k = k0; k < k1; ++k) {
            const double yp = a.mp[(size_t)k * a.ldc + c] - mm;
            const double y = member ? (double)a.xr[(size_t)k * a.ldx + col] - mc : yp;
            acc = acc + y * yp;
        }
        a.cpart[(size_t)chunk * S + s] = acc;
    }
}

// r = rint(1000 * cor) / 1000 (numpy's round(cor, 3)), w = r^3
CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_corr_kernel(CsClusterArgs a)
{
    const uint32_t S = a.T + a.nC;
    for (uint32_t s = cg_bid() * (uint32_t)CS_THREADS + cg_tid(); s < a.T; s += cg_gdim() * (uint32_t)CS_THREADS) {
        const size_t col = a.slotCol[s];
        const double cjp = cs_fold(a.cpart, S, a.nChunks, s), cpp = cs_fold(a.cpart, S, a.nChunks, (size_t)a.T + a.slotCluster[s]);
        const double cor = cjp / (sqrt(a.c[col * a.ldx + col]) * sqrt(cpp));
        const double r = rint(1000.0 * cor) / 1000.0;
        if (r != r) cg_atomic_or_u32(a.flags + CS_FLAG_CORR, 1u);
        a.r[s] = r; a.w[s] = (r * r) * r;
    }
}

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_wmean_kernel(CsClusterArgs a)
{
    const unsigned long long all = (unsigned long long)a.L * a.nC;
    for (unsigned long long e = (unsigned long long)cg_bid() * CS_THREADS + cg_tid(); e < all; e += (unsigned long long)cg_gdim() * CS_THREADS) {
        const size_t k = (size_t)(e / a.nC); const uint32_t c = (uint32_t)(e % a.nC);
        double num = 0.0, den = 0.0;
        for (uint32_t t = a.start[c]; t < a.start[c + 1u]; ++t) {
            num = num + (double)a.xr[k * a.ldx + a.slotCol[t]] * a.w[t];
            den = den + a.w[t];
        }
        a.mpw[k * a.ldc + c] = num / den;
    }
}

// the larger of m and v + 0.0 (so that no zero is negative and the order of the comparisons decides nothing); a NaN stays
CG_DEVICE double cs_max(double m, double v)
{
    v = v + 0.0;
    return (v > m || v != v) ? v : m;
}

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_colmax_kernel(CsClusterArgs a)
{
    const unsigned long long colBlocks = ((unsigned long long)a.nC + CS_THREADS - 1u) / CS_THREADS;
    for (unsigned long long u = cg_bid(); u < colBlocks * a.nChunks; u += cg_gdim()) {
        const uint32_t chunk = (uint32_t)(u / colBlocks), c = (uint32_t)(u % colBlocks) * (uint32_t)CS_THREADS + cg_tid();
        if (c >= a.nC) continue;
        const uint32_t k0 = chunk * CS_KC, k1 = a.L - k0 < CS_KC ? a.L : k0 + CS_KC;
        double m = -INFINITY;
        for (uint32_t k = k0; k < k1; ++k) m = cs_max(m, a.mpw[(size_t)k * a.ldc + c]);
        a.maxPart[(size_t)chunk * a.ldc + c] = m;
    }
}

CG_KERNEL void CG_LAUNCH_BOUNDS(CS_THREADS) cs_consensus_kernel(CsClusterArgs a)
{
    const unsigned long long all = (unsigned long long)a.L * a.nC;
    for (unsigned long long e = (unsigned long long)cg_bid() * CS_THREADS + cg_tid(); e < all; e += (unsigned long long)cg_gdim() * CS_THREADS) {
        const size_t k = (size_t)(e / a.nC); const uint32_t c = (uint32_t)(e % a.nC);
        double m = -INFINITY;
        for (uint32_t ch = 0; ch < a.nChunks; ++ch) m = cs_max(m, a.maxPart[(size_t)ch * a.ldc + c]);
        a.consensus[k * a.nC + c] = (float)(a.mpw[k * a.ldc + c] / m);
    }
}
