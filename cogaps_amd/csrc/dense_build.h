// dense_build.h -- a session's data from a dense matrix that is resident on the device: a row-major [nrow][ncol] fp32 array, an optional
// uncertainty array of the same shape (cogaps_session_create with data_on_device = 1, cogaps_run_device).  Nothing of the matrix goes
// through the host.  Element offsets into the input are 64-bit throughout: nrow * ncol may exceed 2^32.
//
// The dense model (build_sampler's layout, cogaps_hip.cpp): per sampler D, Sraw and -- when the session keeps it -- S2 as
// [vector j][element i] with rows of Npad floats, the pad elements N .. Npad-1 written too (D = 0, Sraw = S2 = 1).  Input position of
// (j, i): Matrix(mat, genesInCols, subsetGenes, indices) (Matrix.cpp:30-69) -- for one sampler the vectors are input rows
// (dnb_rows_kernel: a copy, or a gather where subsetData names rows or columns), for the other input columns (dnb_cols_kernel: a
// transpose through LDS tiles, so that both the reads of the input and the writes of the vectors are along consecutive addresses).
// subsetData's 1-based indices apply in the order given and may repeat, on either axis of either sampler (DnbIn::vecMap / elMap).
// The constants: the entries > 0 are counted by the fill kernels (an integer count: any order); the sum that feeds lambda is
// gaps::nonZeroMean's (MatrixMath.cpp:39-55) -- ONE fp32 accumulator over the sampler's elements in (j, i) order, each sampler in its
// own order (dnb_ordered_sum_kernel).
//
// The sparse model: the entries > 0 of the matrix -- with subsetData applied -- compacted to CSR on the device (dnb_csr_count_kernel,
// sparse_build.h's spb_scan_kernel, dnb_csr_fill_kernel: ascending column indices), then sparse_build.h's builder as for any CSR input.
#pragma once
#include "gaps_state.h"
#include "aux_kernels.h"
#include "sparse_build.h"

struct DnbIn {
    const float *data, *unc;              // [nrow][ncol]; unc may be null (the default uncertainty max(0.1 v, 0.1))
    uint32_t nrow, ncol;
    const uint32_t *vecMap, *elMap;       // subsetData's 1-based indices where they pick the vectors / the elements of this sampler, else null
};
struct DnbOut {
    float *D, *Sraw, *S2;                 // [M][Npad]; S2 may be null (the session keeps none)
    uint32_t M, N, Npad;
};
#define DNB_BS 256
#define DNB_TILE 64

// sd = the uncertainty of a value: the caller's, or gaps::pmax(v * 0.1, 0.1) (MatrixMath.cpp:74-84) -- build_sampler's fp32 operations
CG_DEVICE float dnb_sd(const DnbIn &in, size_t src, float v) { return in.unc ? in.unc[src] : gm_max(v * 0.1f, 0.1f); }
CG_DEVICE void dnb_store(const DnbOut &o, size_t at, float v, float sd)
{
    o.D[at] = v; o.Sraw[at] = sd;
    if (o.S2) o.S2[at] = sd * sd;
}

// The sampler whose vectors are input rows.  Workgroup = DNB_BS consecutive elements of one vector (chunks workgroups per vector):
// consecutive lanes read consecutive input columns (unless elMap gathers them) and write consecutive elements.  Bounds: j < M by the
// grid (M * chunks workgroups), i < Npad tested; the maps hold indices the host has checked against the input's dimensions.
CG_KERNEL void CG_LAUNCH_BOUNDS(DNB_BS) dnb_rows_kernel(DnbIn in, DnbOut o, uint32_t chunks, uint32_t *count)
{
    const uint32_t j = cg_bid() / chunks, i = (cg_bid() % chunks) * (uint32_t)DNB_BS + cg_tid();
    bool positive = false;
    if (i < o.Npad) {
        const size_t at = (size_t)j * o.Npad + i;
        if (i < o.N) {
            const uint32_t r = in.vecMap ? in.vecMap[j] - 1u : j, c = in.elMap ? in.elMap[i] - 1u : i;
            const size_t src = (size_t)r * in.ncol + c;
            const float v = in.data[src];
            dnb_store(o, at, v, dnb_sd(in, src, v));
            positive = v > 0.f;
        } else dnb_store(o, at, 0.f, 1.f);
    }
    const unsigned long long m = cg_ballot(positive);
    if ((cg_tid() & 63u) == 0u && m != 0ull) cg_atomic_add_u32(count, (uint32_t)cg_popc64(m));
}

// The sampler whose vectors are input columns.  Workgroup = one tile of DNB_TILE elements (input rows) x DNB_TILE vectors (input columns),
// four waves.  In: a wave reads one input row of the tile per round, lane = column, into LDS row [element][vector]; out: a wave writes
// one vector of the tile per round, lane = element, reading the LDS column.  The LDS rows are DNB_TILE + 1 floats long: the column read
// (ds_read_b32: 32 banks per half wave) then has stride 65 and touches every bank once; the row write is conflict-free anyway.
// Positions outside the matrix are loaded as the pad's values (D = 0, Sraw = 1), so the pad elements N .. Npad-1 -- always inside the
// last tile of a vector, Npad - N < 4 -- come out of the same store loop.  Nothing is read at i >= N or j >= M, nothing written at
// i >= Npad or j >= M.
CG_KERNEL void CG_LAUNCH_BOUNDS(DNB_BS) dnb_cols_kernel(DnbIn in, DnbOut o, uint32_t tilesI, uint32_t *count)
{
    CG_SHARED float tv[DNB_TILE][DNB_TILE + 1];
    CG_SHARED float ts[DNB_TILE][DNB_TILE + 1];
    const uint32_t lane = cg_tid() & 63u, w = cg_tid() >> 6, waves = (uint32_t)DNB_BS / 64u;
    const uint32_t i0 = (cg_bid() % tilesI) * (uint32_t)DNB_TILE, j0 = (cg_bid() / tilesI) * (uint32_t)DNB_TILE;
    const uint32_t jIn = j0 + lane;
    const bool jLive = jIn < o.M;
    const uint32_t c = !jLive ? 0u : in.vecMap ? in.vecMap[jIn] - 1u : jIn;
    uint32_t positive = 0;
    for (uint32_t il = w; il < (uint32_t)DNB_TILE; il += waves) {
        const uint32_t i = i0 + il;
        float v = 0.f, sd = 1.f;
        if (jLive && i < o.N) {
            const uint32_t r = in.elMap ? in.elMap[i] - 1u : i;
            const size_t src = (size_t)r * in.ncol + c;
            v = in.data[src]; sd = dnb_sd(in, src, v);
            if (v > 0.f) ++positive;
        }
        tv[il][lane] = v; ts[il][lane] = sd;
    }
    cg_sync();
    const uint32_t iOut = i0 + lane;
    for (uint32_t jl = w; jl < (uint32_t)DNB_TILE; jl += waves) {
        const uint32_t j = j0 + jl;
        if (j < o.M && iOut < o.Npad) dnb_store(o, (size_t)j * o.Npad + iOut, tv[lane][jl], ts[lane][jl]);
    }
    positive = cg_wave_sum_u32(positive);
    if (lane == 0u && positive != 0u) cg_atomic_add_u32(count, positive);
}

// out[0], out[1] = 0 + D[0][0] + D[0][1] + ... + D[M-1][N-1] of sampler a and of sampler b, ONE fp32 accumulator each: workgroup 0 and
// workgroup 1.  The order of the additions is the result (sparse_build.h, spb_ordered_sum_kernel: a tree or an atomic sum gives other
// bits), so one thread adds.  What is spread over the workgroup is everything else: the array is read as it lies, [M][Npad] with its
// pads, a float4 per thread and round (n: a multiple of 4), and the values that are not +-0 are packed, in order, into LDS (a wave scan
// of the threads' counts, the waves' totals through LDS); thread 0 adds the packed values only.  Leaving +-0 out is exact: the
// accumulator starts at +0, never becomes -0, and x + (+-0) = x for every other x -- so the pads (D = 0) and a sparse matrix's zeros
// cost no serial step.  Negative and NaN values are added: the dense model keeps them in D.  The next round's float4 is requested
// before the serial loop so that its latency passes under it.
#define DNB_SUM_BS 1024
CG_KERNEL void CG_LAUNCH_BOUNDS(DNB_SUM_BS) dnb_ordered_sum_kernel(const float *Da, uint64_t na, const float *Db, uint64_t nb, float *out)
{
    CG_SHARED float packed[4 * DNB_SUM_BS];
    CG_SHARED uint32_t waveTotal[DNB_SUM_BS / 64];
    const cg_f4 *D = reinterpret_cast<const cg_f4 *>(cg_bid() == 0u ? Da : Db);
    const uint64_t n4 = (cg_bid() == 0u ? na : nb) >> 2;
    const uint32_t t = cg_tid(), lane = t & 63u, w = t >> 6;
    cg_f4 zero; zero.x = zero.y = zero.z = zero.w = 0.f;
    cg_f4 cur = t < n4 ? D[t] : zero;
    float acc = 0.f;
    for (uint64_t base = 0; base < n4; base += DNB_SUM_BS) {
        const uint64_t ahead = base + DNB_SUM_BS + t;
        const cg_f4 next = ahead < n4 ? D[ahead] : zero;
        const bool k0 = cur.x != 0.f, k1 = cur.y != 0.f, k2 = cur.z != 0.f, k3 = cur.w != 0.f;      // (NaN != 0: kept)
        uint32_t total;
        uint32_t at = cg_wave_excl_scan_u32((uint32_t)k0 + (uint32_t)k1 + (uint32_t)k2 + (uint32_t)k3, total);
        if (lane == 0u) waveTotal[w] = total;
        cg_sync();
        uint32_t all = 0;
        for (uint32_t q = 0; q < (uint32_t)DNB_SUM_BS / 64u; ++q) { const uint32_t x = waveTotal[q]; if (q < w) at += x; all += x; }
        if (k0) packed[at++] = cur.x;
        if (k1) packed[at++] = cur.y;
        if (k2) packed[at++] = cur.z;
        if (k3) packed[at++] = cur.w;
        cg_sync();
        if (t == 0u) for (uint32_t e = 0; e < all; ++e) acc = acc + packed[e];
        cg_sync();                                                              // packed and waveTotal are the next round's
        cur = next;
    }
    if (t == 0u) out[cg_bid()] = acc;
}

// ---- the sparse model: the entries > 0 to CSR ----
// The matrix compacted is the subset's: rows x cols, row r = input row vecMap[r] - 1, column c = input column elMap[c] - 1 (a null map:
// the identity).  One wave per row, 64 consecutive columns per round.
// cnt[r] = entries > 0 of row r (SparseVector keeps v > 0 only, SparseVector.cpp:20-33: NaN, zeros and negatives are absent)
CG_KERNEL void CG_LAUNCH_BOUNDS(64 * SPB_WAVES) dnb_csr_count_kernel(DnbIn in, uint32_t rows, uint32_t cols, uint32_t *cnt)
{
    const uint32_t lane = cg_tid() & 63u, r = cg_bid() * (uint32_t)SPB_WAVES + (cg_tid() >> 6);
    const bool live = r < rows;
    const size_t row = live ? (size_t)(in.vecMap ? in.vecMap[r] - 1u : r) * in.ncol : 0;
    uint32_t n = 0;
    for (uint32_t c0 = 0; c0 < cols; c0 += 64u) {
        const uint32_t c = c0 + lane;
        if (live && c < cols && in.data[row + (in.elMap ? in.elMap[c] - 1u : c)] > 0.f) ++n;
    }
    n = cg_wave_sum_u32(n);
    if (lane == 0u && live) cnt[r] = n;
}
// ptr = the exclusive scan of cnt, ptr[rows] the total (below 2^32 - 1: checked by the host).  Row r's entries > 0 go to ptr[r] on in
// ascending column order: a round's kept lanes take consecutive slots by the wave's ballot.  indptr = ptr widened to 64 bits.
CG_KERNEL void CG_LAUNCH_BOUNDS(64 * SPB_WAVES) dnb_csr_fill_kernel(DnbIn in, uint32_t rows, uint32_t cols, const uint32_t *ptr,
                                                                     uint64_t *indptr, uint32_t *indices, float *values)
{
    const uint32_t lane = cg_tid() & 63u, r = cg_bid() * (uint32_t)SPB_WAVES + (cg_tid() >> 6);
    const bool live = r < rows;
    const size_t row = live ? (size_t)(in.vecMap ? in.vecMap[r] - 1u : r) * in.ncol : 0;
    uint32_t at = live ? ptr[r] : 0u;
    const uint32_t end = live ? ptr[r + 1u] : 0u;      // (a slot is tested against it: no store leaves the row's run even if the caller broke the contract and changed the input between the two passes)
    if (lane == 0u && live) { indptr[r] = at; if (r == rows - 1u) indptr[rows] = ptr[rows]; }
    for (uint32_t c0 = 0; c0 < cols; c0 += 64u) {
        const uint32_t c = c0 + lane;
        float v = 0.f;
        if (live && c < cols) v = in.data[row + (in.elMap ? in.elMap[c] - 1u : c)];
        const bool keep = v > 0.f;
        const unsigned long long m = cg_ballot(keep);
        if (keep) { const uint32_t slot = at + (uint32_t)cg_popc64(m & ((1ull << lane) - 1ull)); if (slot < end) { indices[slot] = c; values[slot] = v; } }
        at += (uint32_t)cg_popc64(m);
    }
}
