// markers_kernel.h -- the pattern markers of the result side (patternMarkers, R/methods-CogapsResult.R:397-494): every
// row of a factor matrix is scaled, normalised by its own maximum and scored by its distance to each pattern vector; every column of
// scores is ranked (ties in row order, NaN last), and the marker lists are read off the ranks.  The matrices live on the device
// transposed (one column = one contiguous run of rows), so that lane = row reads and writes whole lines both while scoring and while
// sorting.  fp64 in the order the definition gives, no contraction; everything after the scores is integer work whose result does not
// depend on the grid, on scheduling or on the order in which atomics arrive.  Nothing here waits for another workgroup: a phase that
// needs every workgroup's result is the next launch.
#pragma once
#include "platform.h"
#include <string.h>
#include <math.h>

#define PM_THREADS 256                  // four waves per workgroup; also the number of values of a radix digit
#define PM_WAVES (PM_THREADS / 64)
#define PM_SMALL_ROWS 1024              // at most this many rows: one workgroup ranks a column in LDS by counting (pm_rank_small_kernel)
#define PM_TILE_ROWS 4096               // above: rows of a column one workgroup histograms / scatters per trip of the radix sort
#define PM_DIGIT_BITS 8
#define PM_PASSES (64 / PM_DIGIT_BITS)  // (even: the sorted column ends in the buffer it started in)
#define PM_LBLOCK 8                     // patterns a lane scores per read of its row
#define PM_NAN_KEY 0xFFFFFFFFFFFFFFFFull

#define PM_THRESHOLD_ALL 0
#define PM_THRESHOLD_CUT 1

CG_HD unsigned long long pm_bits(double v) { unsigned long long b; memcpy(&b, &v, 8); return b; }
CG_HD double pm_from_bits(unsigned long long b) { double v; memcpy(&v, &b, 8); return v; }
// a score -- +0 and above, or NaN -- as an integer that orders the same way, every NaN as the one key above all numbers
CG_HD unsigned long long pm_score_key(double s) { return s != s ? PM_NAN_KEY : pm_bits(s); }
// any double as such an integer (for the column maxima, which meet in an integer atomic max); never 0, which is the empty maximum
CG_HD unsigned long long pm_ordered_key(double v)
{
    if (v != v) return PM_NAN_KEY;
    const unsigned long long b = pm_bits(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
CG_HD double pm_ordered_value(unsigned long long key)
{
    if (key == PM_NAN_KEY) return pm_from_bits(0x7FF8000000000000ull);
    return pm_from_bits((key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key);
}

struct PmArgs {
    double *at; const double *ot;                   // A and O transposed: element (i, k) at at[k * ldn + i], ot[k * ldm + j]; at becomes X in place
    size_t ldn, ldm;                                // (multiples of 16)
    uint32_t n, m, K, L;
    const double *lp;                               // [L][K], or null: the K one-hot vectors (then L == K)
    unsigned long long *colMax;                     // [K] ordered keys of the column maxima of O (zero-filled before the launch)
    unsigned long long *keys[2];                    // [L][ldn] each: the score keys of a column, and the radix sort's other buffer
    uint32_t *order[2];                             // [L][ldn] each: the rows in the keys' order
    uint32_t *rankT;                                // [L][ldn]: 1-based rank of row i in column l
    uint32_t *rowMin, *best;                        // [n]: the row's smallest rank over the columns, and the lowest column that has it
    uint32_t *nanRows;                              // [1]: z, the rows whose scores are NaN
    uint32_t *cutPos;                               // [L]: first 0-based position of a column whose row ranks better elsewhere (n before the launch)
    uint32_t *hist;                                 // [L][256][nTiles]: rows of tile t with digit d -> after the scan, those of the tiles before t
    uint32_t *digitBase;                            // [L][256]: rows of the column with a smaller digit
    uint32_t *tileCount;                            // [L][nTiles]: markers among a tile's positions -> after the scan, among the tiles before
    uint32_t tileRows, nTiles, shift;               // (tileRows: a multiple of PM_THREADS)
    int threshold;
    double *scores; uint32_t *ranks;                // outputs [n][L], either may be null
    uint32_t *markers, *markerCount;                // outputs [L][n] (0xFF-filled before the launch) and [L]
};

// the first element a tile holds and how many trips of PM_THREADS elements cover it (the same in every lane of the workgroup)
CG_DEVICE uint32_t pm_tile_trips(const PmArgs &a, uint32_t tile, uint32_t &first)
{
    first = tile * a.tileRows;                      // (< n <= 2^32 - 1: nTiles = ceil(n / tileRows))
    const uint32_t len = a.n - first < a.tileRows ? a.n - first : a.tileRows;
    return (len + PM_THREADS - 1u) / PM_THREADS;
}

// ---- column maxima of O: a workgroup takes PM_TILE_ROWS rows of one column, the maxima meet as ordered keys in one integer atomic ----
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_colmax_kernel(PmArgs a)
{
    CG_SHARED unsigned long long part[PM_THREADS];
    const uint32_t chunks = (a.m + PM_TILE_ROWS - 1u) / PM_TILE_ROWS;
    const unsigned long long units = (unsigned long long)a.K * chunks;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t k = (uint32_t)(u / chunks), j0 = (uint32_t)(u % chunks) * PM_TILE_ROWS;
        const uint32_t jEnd = a.m - j0 < (uint32_t)PM_TILE_ROWS ? a.m : j0 + PM_TILE_ROWS;
        unsigned long long best = 0ull;
        for (uint32_t j = j0 + cg_tid(); j < jEnd; j += PM_THREADS) {
            const unsigned long long key = pm_ordered_key(a.ot[(size_t)k * a.ldm + j]);
            best = key > best ? key : best;
        }
        part[cg_tid()] = best;
        cg_sync();
        for (uint32_t half = PM_THREADS / 2u; half > 0u; half >>= 1) {
            if (cg_tid() < half) { const unsigned long long o = part[cg_tid() + half]; if (o > part[cg_tid()]) part[cg_tid()] = o; }
            cg_sync();
        }
        if (cg_tid() == 0u) cg_atomic_max_u64(a.colMax + k, part[0]);
        cg_sync();
    }
}

// ---- X[i][k] = A[i][k] * pscale[k] / max_k (A[i][k] * pscale[k]), in place; lane = row.  The maximum keeps a NaN it meets. ----
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_normalise_kernel(PmArgs a)
{
    const unsigned long long blocks = ((unsigned long long)a.n + PM_THREADS - 1ull) / PM_THREADS;
    for (unsigned long long b = cg_bid(); b < blocks; b += cg_gdim()) {
        const unsigned long long i = b * PM_THREADS + cg_tid();
        if (i >= a.n) continue;
        double top = a.at[i] * pm_ordered_value(a.colMax[0]);
        for (uint32_t k = 1; k < a.K; ++k) {
            const double v = a.at[(size_t)k * a.ldn + i] * pm_ordered_value(a.colMax[k]);
            if (v > top || v != v) top = v;
        }
        for (uint32_t k = 0; k < a.K; ++k) {
            const double v = a.at[(size_t)k * a.ldn + i] * pm_ordered_value(a.colMax[k]);
            a.at[(size_t)k * a.ldn + i] = v / top;
        }
    }
}

// ---- score[i][l] = sqrt(sum over k, ascending from +0, of (X[i][k] - lp[l][k])^2): lane = row, PM_LBLOCK patterns per read of the
// row; the pattern vector's entry is the same in every lane.  Writes the sort key and the row as the sort's payload. ----
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_score_kernel(PmArgs a)
{
    const uint32_t lBlocks = (a.L + PM_LBLOCK - 1u) / PM_LBLOCK;
    const unsigned long long rowBlocks = ((unsigned long long)a.n + PM_THREADS - 1ull) / PM_THREADS, units = rowBlocks * lBlocks;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t l0 = (uint32_t)(u % lBlocks) * PM_LBLOCK;
        const unsigned long long row = (u / lBlocks) * PM_THREADS + cg_tid();
        const bool live = row < a.n;
        const size_t i = live ? (size_t)row : (size_t)a.n - 1u;
        uint32_t col[PM_LBLOCK]; double acc[PM_LBLOCK];
        for (int t = 0; t < PM_LBLOCK; ++t) { col[t] = l0 + (uint32_t)t < a.L ? l0 + (uint32_t)t : a.L - 1u; acc[t] = 0.0; }
        for (uint32_t k = 0; k < a.K; ++k) {
            const double x = a.at[(size_t)k * a.ldn + i];
            for (int t = 0; t < PM_LBLOCK; ++t) {
                const double p = a.lp ? a.lp[(size_t)col[t] * a.K + k] : (col[t] == k ? 1.0 : 0.0);
                const double d = x - p;
                acc[t] = acc[t] + d * d;
            }
        }
        bool nan0 = false;
        for (int t = 0; t < PM_LBLOCK; ++t) {
            const double s = sqrt(acc[t]);
            if (t == 0) nan0 = live && l0 == 0u && s != s;
            if (live && l0 + (uint32_t)t < a.L) {
                a.keys[0][(size_t)col[t] * a.ldn + i] = pm_score_key(s);
                a.order[0][(size_t)col[t] * a.ldn + i] = (uint32_t)i;
                if (a.scores) a.scores[i * a.L + col[t]] = s;
            }
        }
        const unsigned long long nanLanes = cg_ballot(nan0);      // a row is NaN in every column or in none: column 0 counts them
        if ((cg_tid() & 63u) == 0u && nanLanes) cg_atomic_add_u32(a.nanRows, (uint32_t)cg_popc64(nanLanes));
    }
}

// ---- ranking, n <= PM_SMALL_ROWS: a workgroup holds a column's keys in LDS and counts, for every row, the rows before it ----
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_rank_small_kernel(PmArgs a)
{
    CG_SHARED unsigned long long key[PM_SMALL_ROWS];
    for (uint32_t l = cg_bid(); l < a.L; l += cg_gdim()) {
        for (uint32_t i = cg_tid(); i < a.n; i += PM_THREADS) key[i] = a.keys[0][(size_t)l * a.ldn + i];
        cg_sync();
        for (uint32_t i = cg_tid(); i < a.n; i += PM_THREADS) {
            const unsigned long long mine = key[i];
            uint32_t before = 0u;
            for (uint32_t j = 0; j < a.n; ++j) before += (key[j] < mine || (key[j] == mine && j < i)) ? 1u : 0u;
            a.rankT[(size_t)l * a.ldn + i] = before + 1u;
            a.order[0][(size_t)l * a.ldn + before] = i;
        }
        cg_sync();
    }
}

// ---- ranking, any n: least-significant-digit radix sort of (key, row), PM_PASSES passes of three launches.  The lanes of a wave
// that hold the same digit find each other by ballots -- one per bit of the digit -- so that a tile's rows are counted and placed in
// their order without an atomic: the sort is stable, and the row index that makes equal keys distinct never has to be compared. ----
CG_DEVICE unsigned long long pm_same_digit(uint32_t digit, bool live)
{
    unsigned long long peers = cg_ballot(live);
    for (uint32_t b = 0; b < PM_DIGIT_BITS; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long set = cg_ballot(live && bit);
        peers &= bit ? set : ~set;
    }
    return peers;
}

CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_hist_kernel(PmArgs a, int from)
{
    CG_SHARED uint32_t inWave[PM_WAVES][PM_THREADS];
    const uint32_t lane = cg_tid() & 63u, wave = cg_tid() >> 6;
    const unsigned long long units = (unsigned long long)a.L * a.nTiles;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t l = (uint32_t)(u / a.nTiles), tile = (uint32_t)(u % a.nTiles);
        uint32_t first;
        const uint32_t trips = pm_tile_trips(a, tile, first);
        for (uint32_t w = 0; w < PM_WAVES; ++w) inWave[w][cg_tid()] = 0u;
        cg_sync();
        for (uint32_t c = 0; c < trips; ++c) {
            const unsigned long long e = (unsigned long long)first + c * PM_THREADS + cg_tid();
            const bool live = e < a.n;
            const uint32_t digit = live ? (uint32_t)(a.keys[from][(size_t)l * a.ldn + (size_t)e] >> a.shift) & 255u : 0u;
            const unsigned long long peers = pm_same_digit(digit, live);
            if (live && (uint32_t)cg_ctz64(peers) == lane) inWave[wave][digit] += (uint32_t)cg_popc64(peers);
            cg_wave_sync();
        }
        cg_sync();
        uint32_t sum = 0u;
        for (uint32_t w = 0; w < PM_WAVES; ++w) sum += inWave[w][cg_tid()];
        a.hist[((size_t)l * PM_THREADS + cg_tid()) * a.nTiles + tile] = sum;
        cg_sync();
    }
}

// per column: hist[d][t] becomes the rows with digit d in the tiles before t, digitBase[d] the rows with a digit below d
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_hist_scan_kernel(PmArgs a)
{
    CG_SHARED uint32_t total[PM_THREADS];
    for (uint32_t l = cg_bid(); l < a.L; l += cg_gdim()) {
        uint32_t *mine = a.hist + ((size_t)l * PM_THREADS + cg_tid()) * a.nTiles;
        uint32_t run = 0u;
        for (uint32_t t = 0; t < a.nTiles; ++t) { const uint32_t v = mine[t]; mine[t] = run; run += v; }
        total[cg_tid()] = run;
        cg_sync();
        uint32_t below = 0u;
        for (uint32_t d = 0; d < cg_tid(); ++d) below += total[d];
        a.digitBase[(size_t)l * PM_THREADS + cg_tid()] = below;
        cg_sync();
    }
}

CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_scatter_kernel(PmArgs a, int from)
{
    CG_SHARED uint32_t inWave[PM_WAVES][PM_THREADS];
    CG_SHARED uint32_t base[PM_THREADS];
    const uint32_t lane = cg_tid() & 63u, wave = cg_tid() >> 6;
    const unsigned long long units = (unsigned long long)a.L * a.nTiles;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t l = (uint32_t)(u / a.nTiles), tile = (uint32_t)(u % a.nTiles);
        uint32_t first;
        const uint32_t trips = pm_tile_trips(a, tile, first);
        const size_t col = (size_t)l * a.ldn;
        base[cg_tid()] = a.digitBase[(size_t)l * PM_THREADS + cg_tid()] + a.hist[((size_t)l * PM_THREADS + cg_tid()) * a.nTiles + tile];
        for (uint32_t w = 0; w < PM_WAVES; ++w) inWave[w][cg_tid()] = 0u;
        cg_sync();
        for (uint32_t c = 0; c < trips; ++c) {
            const unsigned long long e = (unsigned long long)first + c * PM_THREADS + cg_tid();
            const bool live = e < a.n;
            const unsigned long long key = live ? a.keys[from][col + (size_t)e] : 0ull;
            const uint32_t row = live ? a.order[from][col + (size_t)e] : 0u;
            const uint32_t digit = (uint32_t)(key >> a.shift) & 255u;
            const unsigned long long peers = pm_same_digit(digit, live);
            if (live && (uint32_t)cg_ctz64(peers) == lane) inWave[wave][digit] = (uint32_t)cg_popc64(peers);
            cg_sync();
            if (live) {
                uint32_t at = base[digit] + (uint32_t)cg_popc64(peers & ((1ull << lane) - 1ull));
                for (uint32_t w = 0; w < wave; ++w) at += inWave[w][digit];
                if (at < a.n) { a.keys[from ^ 1][col + at] = key; a.order[from ^ 1][col + at] = row; }
            }
            cg_sync();
            uint32_t sum = 0u;
            for (uint32_t w = 0; w < PM_WAVES; ++w) { sum += inWave[w][cg_tid()]; inWave[w][cg_tid()] = 0u; }
            base[cg_tid()] += sum;
            cg_sync();
        }
    }
}

// rank[order[l][p]][l] = p + 1
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_rank_scatter_kernel(PmArgs a)
{
    const unsigned long long rowBlocks = ((unsigned long long)a.n + PM_THREADS - 1ull) / PM_THREADS, units = rowBlocks * a.L;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const size_t col = (size_t)(u / rowBlocks) * a.ldn;
        const unsigned long long p = (u % rowBlocks) * PM_THREADS + cg_tid();
        if (p >= a.n) continue;
        const uint32_t row = a.order[0][col + (size_t)p];
        if (row < a.n) a.rankT[col + row] = (uint32_t)p + 1u;
    }
}

// per row: the smallest rank over the columns and the lowest column that has it; the ranks leave row-major
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_rowmin_kernel(PmArgs a)
{
    const unsigned long long blocks = ((unsigned long long)a.n + PM_THREADS - 1ull) / PM_THREADS;
    for (unsigned long long b = cg_bid(); b < blocks; b += cg_gdim()) {
        const unsigned long long i = b * PM_THREADS + cg_tid();
        if (i >= a.n) continue;
        uint32_t low = 0xFFFFFFFFu, at = 0u;
        for (uint32_t l = 0; l < a.L; ++l) {
            const uint32_t r = a.rankT[(size_t)l * a.ldn + (size_t)i];
            if (r < low) { low = r; at = l; }
            if (a.ranks) a.ranks[(size_t)i * a.L + l] = r;
        }
        a.rowMin[i] = low; a.best[i] = at;
    }
}

// cutPos[l] = the first position of column l whose row has a better rank in another column: a minimum over positions
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_cutpos_kernel(PmArgs a)
{
    const uint32_t lane = cg_tid() & 63u;
    const unsigned long long rowBlocks = ((unsigned long long)a.n + PM_THREADS - 1ull) / PM_THREADS, units = rowBlocks * a.L;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t l = (uint32_t)(u / rowBlocks);
        const unsigned long long p = (u % rowBlocks) * PM_THREADS + cg_tid();
        bool worse = false;
        if (p < a.n) {
            const uint32_t row = a.order[0][(size_t)l * a.ldn + (size_t)p];
            worse = row < a.n && (uint32_t)p + 1u > a.rowMin[row];
        }
        const unsigned long long any = cg_ballot(worse);       // positions ascend with the lane: the wave's first is its minimum
        if (worse && (uint32_t)cg_ctz64(any) == lane) cg_atomic_min_u32(a.cutPos + l, (uint32_t)p);
    }
}

// is position p of column l a marker of l?  Positions from n - z on hold the NaN rows.
CG_DEVICE bool pm_is_marker(const PmArgs &a, uint32_t l, unsigned long long p, uint32_t numbers, uint32_t cut)
{
    if (p >= numbers) return false;
    if (a.threshold == PM_THRESHOLD_CUT) return p < cut;
    const uint32_t row = a.order[0][(size_t)l * a.ldn + (size_t)p];
    return row < a.n && a.best[row] == l;
}

// markers among a tile's positions
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_marker_count_kernel(PmArgs a)
{
    CG_SHARED uint32_t inWave[PM_WAVES];
    const uint32_t lane = cg_tid() & 63u, wave = cg_tid() >> 6;
    const unsigned long long units = (unsigned long long)a.L * a.nTiles;
    const uint32_t numbers = a.n - *a.nanRows;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t l = (uint32_t)(u / a.nTiles), tile = (uint32_t)(u % a.nTiles);
        uint32_t first;
        const uint32_t trips = pm_tile_trips(a, tile, first), cut = a.cutPos[l];
        uint32_t mine = 0u;
        for (uint32_t c = 0; c < trips; ++c) {
            const unsigned long long p = (unsigned long long)first + c * PM_THREADS + cg_tid();
            mine += (uint32_t)cg_popc64(cg_ballot(pm_is_marker(a, l, p, numbers, cut)));
        }
        if (lane == 0u) inWave[wave] = mine;
        cg_sync();
        if (cg_tid() == 0u) {
            uint32_t sum = 0u;
            for (uint32_t w = 0; w < PM_WAVES; ++w) sum += inWave[w];
            a.tileCount[(size_t)l * a.nTiles + tile] = sum;
        }
        cg_sync();
    }
}

// per column: tileCount[t] becomes the markers of the tiles before t, markerCount the column's total
CG_KERNEL void CG_LAUNCH_BOUNDS(64) pm_marker_scan_kernel(PmArgs a)
{
    for (unsigned long long l = (unsigned long long)cg_bid() * 64ull + cg_tid(); l < a.L; l += (unsigned long long)cg_gdim() * 64ull) {
        uint32_t *mine = a.tileCount + (size_t)l * a.nTiles;
        uint32_t run = 0u;
        for (uint32_t t = 0; t < a.nTiles; ++t) { const uint32_t v = mine[t]; mine[t] = run; run += v; }
        a.markerCount[l] = run;
    }
}

// the markers of column l, in the order of their positions, to the front of markers[l]
CG_KERNEL void CG_LAUNCH_BOUNDS(PM_THREADS) pm_marker_write_kernel(PmArgs a)
{
    CG_SHARED uint32_t inWave[PM_WAVES];
    const uint32_t lane = cg_tid() & 63u, wave = cg_tid() >> 6;
    const unsigned long long units = (unsigned long long)a.L * a.nTiles;
    const uint32_t numbers = a.n - *a.nanRows;
    for (unsigned long long u = cg_bid(); u < units; u += cg_gdim()) {
        const uint32_t l = (uint32_t)(u / a.nTiles), tile = (uint32_t)(u % a.nTiles);
        uint32_t first;
        const uint32_t trips = pm_tile_trips(a, tile, first), cut = a.cutPos[l];
        uint32_t run = a.tileCount[(size_t)l * a.nTiles + tile];
        for (uint32_t c = 0; c < trips; ++c) {
            const unsigned long long p = (unsigned long long)first + c * PM_THREADS + cg_tid();
            const bool is = pm_is_marker(a, l, p, numbers, cut);
            const unsigned long long set = cg_ballot(is);
            if (lane == 0u) inWave[wave] = (uint32_t)cg_popc64(set);
            cg_sync();
            uint32_t at = run + (uint32_t)cg_popc64(set & ((1ull << lane) - 1ull)), all = 0u;
            for (uint32_t w = 0; w < PM_WAVES; ++w) { if (w < wave) at += inWave[w]; all += inWave[w]; }
            if (is && at < a.n) a.markers[(size_t)l * a.n + at] = a.order[0][(size_t)l * a.ldn + (size_t)p];
            run += all;
            cg_sync();
        }
    }
}
