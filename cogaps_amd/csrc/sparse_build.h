// sparse_build.h -- the sparse model's data structures, built on the device from a compressed-sparse matrix (CSR or CSC) or from unordered
// triplets (COO: further down), and meanChiSq from them.  Every sparse-model session is built here, whatever its input: a dense matrix
// is compacted to CSR first -- on the host (cogaps_hip.cpp, build_samplers_dense_input), or on the device when it resides there (dense_build.h).  These four arrays per sampler are all the data
// such a session holds: no genes x samples array exists on the device.
//
// A sampler holds its data as [vector j][element i]: dflags [M][Wn] (bit i of vector j: the entry is > 0), dprefix [M][Wn] (packed
// values of the vector before each flag word), dptr [M + 1] (first packed value of each vector), dvals (the values > 0, vector by
// vector, ascending element index).  For one sampler the input's major axis is the vector axis, for the other the element axis
// (SpbSide::swap).  The input is validated first (spb_validate_kernel; triplets: resolved into one keep bit per entry, further down);
// both samplers are then built by ONE route, the mapped passes at the end of this file (cogaps_hip.cpp, build_samplers_device_matrix),
// whether the arrays are a caller's of one session or a cogaps_device_matrix's of many.  None of its passes depends on the order in
// which the entries arrive, and spb_ordered_sum_kernel adds each sampler's packed values with one fp32 accumulator in their order --
// gaps::nonZeroMean's sum over the dense elements in (j, i) order (zeros add nothing), which feeds lambda.
#pragma once
#include "gaps_state.h"
#include "eval_kernel.h"
#include "aux_kernels.h"

// what the validation found (the largest code wins; 0 = well formed)
#define SPB_ERR_ORDER 1u        // indices not strictly ascending inside a major slice (a duplicate included)
#define SPB_ERR_RANGE 2u        // an index >= nMinor
#define SPB_ERR_INDPTR 3u       // indptr does not start at 0, decreases, or runs past indptr[nMajor]

struct SpbIn {
    const uint64_t *indptr; const uint32_t *indices; const float *values;
    uint32_t nMajor, nMinor; uint64_t nnz;
};
struct SpbSide {
    unsigned long long *flags; uint32_t *prefix, *ptr; float *vals;
    uint32_t M, Wn, swap;      // swap: the vector index is the entry's minor index (0: its major index)
};
#define SPB_WAVES 4      // major slices (or vectors) per workgroup: one wave each

CG_DEVICE void spb_slice(const SpbIn &in, uint32_t m, uint64_t &b, uint64_t &e)
{
    b = e = 0;
    if (m < in.nMajor) { b = in.indptr[m]; e = in.indptr[m + 1]; }
}
CG_DEVICE void spb_place(const SpbSide &s, uint32_t major, uint32_t minor, uint32_t &vec, uint32_t &el)
{
    vec = s.swap ? minor : major; el = s.swap ? major : minor;
}

// The checks of a compressed matrix, one wave per major slice: the slice's bounds, every index against nMinor and against its
// predecessor.  Nothing is read outside [0, nnz) whatever the input holds, nothing written but *err; the host reads *err before
// anything is built from the arrays.
CG_KERNEL void CG_LAUNCH_BOUNDS(64 * SPB_WAVES) spb_validate_kernel(SpbIn in, uint32_t *err)
{
    const uint32_t lane = cg_tid() & 63u, m = cg_bid() * (uint32_t)SPB_WAVES + (cg_tid() >> 6);
    uint64_t lo, hi; spb_slice(in, m, lo, hi);
    if (m == 0u && m < in.nMajor && lo != 0ull) { if (lane == 0u) cg_atomic_max_u32(err, SPB_ERR_INDPTR); }
    if (lo > hi || hi > in.nnz) { if (lane == 0u) cg_atomic_max_u32(err, SPB_ERR_INDPTR); hi = lo = 0; }
    for (uint64_t k = lo + lane; k < hi; k += 64u) {
        const uint32_t idx = in.indices[k];
        if (idx >= in.nMinor) { cg_atomic_max_u32(err, SPB_ERR_RANGE); continue; }
        if (k > lo && in.indices[k - 1] >= idx) cg_atomic_max_u32(err, SPB_ERR_ORDER);
    }
}

// cnt[0 .. n) -> their exclusive prefix sums, cnt[n] = the total.  One workgroup of 1024 threads: a contiguous run of the array per
// thread, the runs' sums scanned through LDS (n is a matrix dimension: at most a few 10^5).
#define SPB_SCAN_BS 1024
CG_KERNEL void CG_LAUNCH_BOUNDS(SPB_SCAN_BS) spb_scan_kernel(uint32_t *cnt, uint32_t n)
{
    CG_SHARED uint32_t run[SPB_SCAN_BS];
    const uint32_t t = cg_tid(), per = (n + (uint32_t)SPB_SCAN_BS - 1u) / (uint32_t)SPB_SCAN_BS;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += cnt[i];
    run[t] = sum; cg_sync();
    for (uint32_t off = 1; off < (uint32_t)SPB_SCAN_BS; off <<= 1) {      // inclusive scan of the runs' sums
        const uint32_t o = t >= off ? run[t - off] : 0u;
        cg_sync();
        run[t] += o; cg_sync();
    }
    uint32_t acc = run[t] - sum;
    for (uint32_t i = lo; i < hi; ++i) { const uint32_t c = cnt[i]; cnt[i] = acc; acc += c; }
    if (t == (uint32_t)SPB_SCAN_BS - 1u) cnt[n] = run[t];
}

// dprefix[j][w] = entries of vector j below flag word w -- all Wn words, the word past the last element (Wn = N/64 + 1) included.
// One wave per vector, 64 words per round.
CG_KERNEL void CG_LAUNCH_BOUNDS(64 * SPB_WAVES) spb_prefix_kernel(SpbSide s)
{
    const uint32_t lane = cg_tid() & 63u, j = cg_bid() * (uint32_t)SPB_WAVES + (cg_tid() >> 6);
    const bool live = j < s.M;
    uint32_t carry = 0;
    for (uint32_t w0 = 0; w0 < s.Wn; w0 += 64u) {
        const uint32_t w = w0 + lane; const bool on = live && w < s.Wn;
        const uint32_t pc = on ? (uint32_t)cg_popc64(s.flags[(size_t)j * s.Wn + w]) : 0u;
        uint32_t total; const uint32_t before = cg_wave_excl_scan_u32(pc, total);
        if (on) s.prefix[(size_t)j * s.Wn + w] = carry + before;
        carry += total;
    }
}

// the packed slot of a flagged position: entries of the vectors before it, of its vector's words before its own, of its word below its bit
CG_DEVICE uint32_t spb_slot(const SpbSide &s, uint32_t major, uint32_t minor)
{
    uint32_t vec, el; spb_place(s, major, minor, vec, el);
    const size_t w = (size_t)vec * s.Wn + (el >> 6);
    return s.ptr[vec] + s.prefix[w] + (uint32_t)cg_popc64(s.flags[w] & ((1ull << (el & 63u)) - 1ull));
}
CG_DEVICE void spb_store(const SpbSide &s, uint32_t major, uint32_t minor, float v) { s.vals[spb_slot(s, major, minor)] = v; }
// out[0], out[1] = 0 + v[0] + v[1] + ... of sampler a's and sampler b's packed values, one accumulator each (seq_sum): workgroup 0
// and workgroup 1.  The order of the additions is the result; a tree or an atomic sum would give other bits.
CG_KERNEL void CG_LAUNCH_BOUNDS(256) spb_ordered_sum_kernel(const float *va, const float *vb, uint32_t n, float *out)
{
    CG_SHARED float lds[SEQ_CHUNK];
    const float *v = cg_bid() == 0u ? va : vb;
    const float c = seq_sum(0.f, (uint64_t)n, lds, [&](uint64_t e) { return v[e]; });
    if (cg_tid() == 0) out[cg_bid()] = c;
}

// ---- unordered triplets (COO): rows[k], cols[k], values[k], k = 0 .. nnz-1, repeats allowed ----
// The matrix they denote is D = 0; for k in input order: D[rows[k]][cols[k]] = values[k] -- the LATEST entry of a position decides it,
// also when its value is not > 0 (the position is then absent).  Which entry is the latest depends on k alone, never on which wave ran
// first:
//   1. coo_present_kernel: checks every index, sets a PRESENT bit per entry -- whatever its value -- in a temporary flag array laid out
//      [nrow][ncol / 64 + 1] (64-bit atomic OR: idempotent)
//   2. spb_count_kernel, spb_scan_kernel, spb_prefix_kernel on that array: every present position gets a slot
//   3. coo_winner_kernel: winner[slot] = max k over the position's entries (32-bit atomic max: commutative, so the order of arrival is
//      immaterial)
//   4. coo_keep_bits_kernel: entry k is KEPT when winner[slot] == k and its value is > 0; the kept entries are distinct positions, one
//      bit each in keep[] (a wave's ballot: one 64-bit store per 64 entries)
// The present flags with their prefix counts and pointers and the winner indices are temporaries; the
// rows, columns, values and keep[] then go through the mapped passes below, which read the kept entries only.
// Hot positions (many entries of one position, or of one flag word) meet at one address in passes 1 and 3; an entry first reads the word
// (a relaxed device-scope atomic load: served where the atomics are carried out, no cache line of this compute unit involved) and leaves
// the atomic out when it would change nothing (both words only ever grow, so an old value costs an atomic, never the result).
struct CooIn {
    const uint32_t *rows, *cols; const float *values;
    uint32_t nrow, ncol; uint64_t nnz;
};
#define COO_BS 256       // entries per workgroup and round (grid-stride loops: the grid is sized to the device, not to nnz)

// Every index against the dimensions; the present bit of every entry in range.  Nothing is read outside [0, nnz), nothing written outside
// the temporary flag array whatever the input holds; the host reads *err before anything is built from it.
CG_KERNEL void CG_LAUNCH_BOUNDS(COO_BS) coo_present_kernel(CooIn in, SpbSide t, uint32_t *err)
{
    for (uint64_t k = (uint64_t)cg_bid() * COO_BS + cg_tid(); k < in.nnz; k += (uint64_t)cg_gdim() * COO_BS) {
        const uint32_t r = in.rows[k], c = in.cols[k];
        if (r >= in.nrow || c >= in.ncol) { cg_atomic_max_u32(err, SPB_ERR_RANGE); continue; }
        uint32_t vec, el; spb_place(t, r, c, vec, el);
        unsigned long long *w = t.flags + (size_t)vec * t.Wn + (el >> 6); const unsigned long long bit = 1ull << (el & 63u);
        if (!(cg_load_l2_u64(w) & bit)) cg_atomic_or_u64(w, bit);
    }
}

// ptr[j] = set flag bits of vector j (a popcount, not a count of entries: a triplet position or an image of a subset may repeat).  One wave per vector.
CG_KERNEL void CG_LAUNCH_BOUNDS(64 * SPB_WAVES) spb_count_kernel(SpbSide s)
{
    const uint32_t lane = cg_tid() & 63u, j = cg_bid() * (uint32_t)SPB_WAVES + (cg_tid() >> 6);
    const bool live = j < s.M;
    uint32_t n = 0;
    for (uint32_t w0 = 0; w0 < s.Wn; w0 += 64u) {
        const uint32_t w = w0 + lane;
        if (live && w < s.Wn) n += (uint32_t)cg_popc64(s.flags[(size_t)j * s.Wn + w]);
    }
    n = cg_wave_sum_u32(n);
    if (lane == 0u && live) s.ptr[j] = n;
}

// winner[slot of the entry's position] = the largest k among the position's entries (winner starts at 0; validated input only)
CG_KERNEL void CG_LAUNCH_BOUNDS(COO_BS) coo_winner_kernel(CooIn in, SpbSide t, uint32_t *winner)
{
    for (uint64_t k = (uint64_t)cg_bid() * COO_BS + cg_tid(); k < in.nnz; k += (uint64_t)cg_gdim() * COO_BS) {
        uint32_t *w = winner + spb_slot(t, in.rows[k], in.cols[k]);
        if (cg_load_l2_u32(w) < (uint32_t)k) cg_atomic_max_u32(w, (uint32_t)k);
    }
}

// keep[k >> 6] bit k & 63: entry k is the latest of its position and its value is > 0 (SparseVector keeps v > 0 only,
// SparseVector.cpp:20-33).  A wave takes 64 consecutive entries from a multiple of 64 on, so a keep word has one writer.
CG_KERNEL void CG_LAUNCH_BOUNDS(COO_BS) coo_keep_bits_kernel(CooIn in, SpbSide t, const uint32_t *winner, unsigned long long *keep)
{
    const uint32_t lane = cg_tid() & 63u;
    for (uint64_t base = (uint64_t)cg_bid() * COO_BS + (cg_tid() - lane); base < in.nnz; base += (uint64_t)cg_gdim() * COO_BS) {
        const uint64_t k = base + lane;
        const bool kept = k < in.nnz && in.values[k] > 0.f && winner[spb_slot(t, in.rows[k], in.cols[k])] == (uint32_t)k;
        const unsigned long long mask = cg_ballot(kept);
        if (lane == 0u) keep[base >> 6] = mask;
    }
}

// ---- the one route from validated arrays to both samplers, with or without a subset of the rows or columns ----
// The arrays are a caller's (one session: staged for the call) or a cogaps_device_matrix's (kept as they came, validated -- triplets:
// resolved -- once at its creation, any number of sessions).  A session visits every stored entry once (triplets: every kept entry)
// and places it through a MAP of the subset axis:
// subsetData names n 1-based indices of that axis (dimension dim), output row / column i is input indices[i] - 1 (Matrix.cpp:30-69: in
// the order given, an index may repeat), so input index c has the IMAGES { i : indices[i] - 1 == c } -- none when c is not in the subset.
//   1. spb_map_count_kernel: cnt[c] = number of images of c (32-bit atomic add); spb_scan_kernel: start = exclusive scan, start[dim] = n
//   2. spb_map_fill_kernel: list[start[c] + q] = i, q from a per-index cursor (32-bit atomic add)
//   3. spb_mapped_kernel<false> / coo_mapped_kernel<false>: every entry ORs its bit into both samplers' flag words once per image
//   4. spb_count_kernel (popcount: an entry may have several images), spb_scan_kernel, spb_prefix_kernel per sampler
//   5. spb_mapped_kernel<true> / coo_mapped_kernel<true>: every entry stores its value at spb_slot of each image
// The order of a list (which image of c got which q) depends on how the device schedules pass 2.  No bit of the session depends on it:
// the passes that read a list treat it as a SET -- pass 3 ORs one bit per image (commutative, idempotent), pass 5 stores the same value
// at the slot of each image, and the images of distinct stored positions are distinct positions of the subset, so no slot has two
// writers.  Without a subset the map is the identity (SpbMap::start == nullptr): the entry is its own only image.  The temporaries are
// the indices, cnt / start [dim + 1], the cursors [dim] and the list [n]: O(dim + n); the other axis is not mapped at all.
struct SpbMap {
    const uint32_t *start, *list;      // images of index c of the subset axis: list[start[c] .. start[c + 1]); start == nullptr: the identity
    uint32_t onMajor;                  // the subset axis is the entries' major axis (their minor axis otherwise)
};
#define SPB_MAP_BS 256

// cnt[indices[i] - 1] += 1 (the host has checked 1 <= indices[i] <= dim)
CG_KERNEL void CG_LAUNCH_BOUNDS(SPB_MAP_BS) spb_map_count_kernel(const uint32_t *indices, uint32_t n, uint32_t *cnt)
{
    for (uint32_t i = cg_bid() * (uint32_t)SPB_MAP_BS + cg_tid(); i < n; i += cg_gdim() * (uint32_t)SPB_MAP_BS) cg_atomic_add_u32(cnt + (indices[i] - 1u), 1u);
}
// list[start[c] + (the next free place of c)] = i: each output position once, inside its input index's run of the list
CG_KERNEL void CG_LAUNCH_BOUNDS(SPB_MAP_BS) spb_map_fill_kernel(const uint32_t *indices, uint32_t n, const uint32_t *start, uint32_t *cursor, uint32_t *list)
{
    for (uint32_t i = cg_bid() * (uint32_t)SPB_MAP_BS + cg_tid(); i < n; i += cg_gdim() * (uint32_t)SPB_MAP_BS) {
        const uint32_t c = indices[i] - 1u;
        list[start[c] + cg_atomic_add_u32(cursor + c, 1u)] = i;
    }
}

// One stored entry > 0 at (major, minor) of the handle's matrix, once per image under the map: its flag bit in both samplers (STORE =
// false) or its value at its slot in both (STORE = true).  Shared by the compressed and the triplet form.
template <bool STORE>
CG_DEVICE void spb_mapped_entry(const SpbMap &mp, const SpbSide &a, const SpbSide &b, uint32_t major, uint32_t minor, float v)
{
    const bool mapped = mp.start != nullptr;
    const bool two = b.flags != a.flags;      // (one side alone is given as both: cogaps_residuals' gene side)
    const uint32_t c = mp.onMajor ? major : minor;
    const uint32_t lo = mapped ? mp.start[c] : 0u, hi = mapped ? mp.start[c + 1u] : 1u;
    for (uint32_t q = lo; q < hi; ++q) {
        const uint32_t img = mapped ? mp.list[q] : c;
        const uint32_t mj = mp.onMajor ? img : major, mn = mp.onMajor ? minor : img;
        if (STORE) { spb_store(a, mj, mn, v); if (two) spb_store(b, mj, mn, v); }
        else {
            uint32_t vec, el;
            spb_place(a, mj, mn, vec, el); cg_atomic_or_u64(a.flags + (size_t)vec * a.Wn + (el >> 6), 1ull << (el & 63u));
            if (two) { spb_place(b, mj, mn, vec, el); cg_atomic_or_u64(b.flags + (size_t)vec * b.Wn + (el >> 6), 1ull << (el & 63u)); }
        }
    }
}

// A validated compressed matrix through the map: one wave per major slice.  A slice whose major index has no image is left unread.
template <bool STORE>
CG_KERNEL void CG_LAUNCH_BOUNDS(64 * SPB_WAVES) spb_mapped_kernel(SpbIn in, SpbMap mp, SpbSide a, SpbSide b)
{
    const uint32_t lane = cg_tid() & 63u, m = cg_bid() * (uint32_t)SPB_WAVES + (cg_tid() >> 6);
    uint64_t lo, hi; spb_slice(in, m, lo, hi);
    if (m < in.nMajor && mp.start != nullptr && mp.onMajor && mp.start[m] == mp.start[m + 1u]) return;
    for (uint64_t k = lo + lane; k < hi; k += 64u) {
        const float v = in.values[k];
        if (!(v > 0.f)) continue;                                             // SparseVector keeps v > 0 only (SparseVector.cpp:20-33)
        spb_mapped_entry<STORE>(mp, a, b, m, in.indices[k], v);
    }
}

// The kept triplets through the map (rows are the major axis): grid-stride over the entries
template <bool STORE>
CG_KERNEL void CG_LAUNCH_BOUNDS(COO_BS) coo_mapped_kernel(CooIn in, const unsigned long long *keep, SpbMap mp, SpbSide a, SpbSide b)
{
    for (uint64_t k = (uint64_t)cg_bid() * COO_BS + cg_tid(); k < in.nnz; k += (uint64_t)cg_gdim() * COO_BS) {
        if (!((keep[k >> 6] >> (k & 63u)) & 1ull)) continue;
        spb_mapped_entry<STORE>(mp, a, b, in.rows[k], in.cols[k], in.values[k]);
    }
}

// GapsStatistics::meanChiSq per-vector partials (aux_kernels.h, mean_chisq_rows_kernel) with the data taken from the P sampler's packed
// form: d = the packed value where the flag bit is set, 0 elsewhere, sd = max(0.1 d, 0.1) -- the default uncertainty, as the dense
// model's dnb_sd (dense_build.h) fills Sraw.  Same lanes, chunks, slots and finish as the dense model's kernel.
template <int V>
CG_KERNEL void CG_LAUNCH_BOUNDS(1024) mean_chisq_rows_packed_kernel(SamplerDev P, const float *Asum, const float *Psum, uint32_t AMpad, float n2, float *partial)
{
    CG_SHARED float lds[16 * V];
    const uint32_t j = cg_bid(), t = cg_tid(), BS = cg_bdim(), W = (uint32_t)V * BS, nq = P.Npad >> 2;
    const unsigned long long *fl = P.dflags + (size_t)j * P.Wn; const uint32_t *pre = P.dprefix + (size_t)j * P.Wn;
    const float *vals = P.dvals + P.dptr[j];
    float tot[1] = {0.f};
    for (int slot = 0; slot < V; ++slot) {
        float acc = 0.f;
        for (uint32_t c = (uint32_t)slot * BS + t; c < nq; c += W) {
            const unsigned long long word = fl[c >> 4]; const uint32_t base = pre[c >> 4];      // (the chunk's four elements share a flag word)
            for (uint32_t e = 0; e < 4; ++e) {
                const uint32_t i = 4 * c + e;
                if (i < P.N) {
                    const unsigned long long bit = 1ull << (i & 63u);
                    const float d = (word & bit) ? vals[base + (uint32_t)cg_popc64(word & (bit - 1ull))] : 0.f;
                    const float sd = gm_max(d * 0.1f, 0.1f);
                    float m = 0.f;
                    for (uint32_t k = 0; k < P.K; ++k) m = m + Asum[(size_t)k * AMpad + i] * Psum[(size_t)k * P.Mpad + j];
                    m = m / n2;
                    acc = acc + ((d - m) * (d - m)) / (sd * sd);
                }
            }
        }
        eval_vpark<V>(acc, slot, lds, tot);
    }
    if (BS > 64u) { cg_sync(); eval_vfinish<1, V>(lds, tot); }
    if (t == 0) partial[j] = tot[0];
}
