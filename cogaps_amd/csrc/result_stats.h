// result_stats.h -- the statistics of a finished run: host code only, a chapter of cogaps_hip.cpp, which includes
// it once, after everything it takes from there:
//   fail, fail_exc                    the one home of the library's error message
//   SpbTemps, SpbMatrix, SpbSide, SpbMap, sparse_args_refusal, spb_compressed, spb_triplets, spb_build_sides
//                                     the sparse builder's helpers, of session_build.h (cogaps_residuals reads the gene side of its packed form)
//   cogaps_device_matrix              the handle cogaps_residuals takes as data, of session_build.h too
// and after the kernel headers geneset_kernel.h, genemember_kernel.h, markers_kernel.h, gsea_kernel.h, residual_kernel.h, consensus_kernel.h, manova_kernel.h, project_kernel.h.
// The entries here: cogaps_gene_set_stat, cogaps_debug_permutation_draw, cogaps_gene_set_membership, cogaps_pattern_markers, cogaps_pattern_gsea, cogaps_residuals, cogaps_pattern_match, cogaps_manova_sscp, cogaps_project.
#pragma once

// One call's device and stream, its device memory, and the stream announced for its allocations' fills.  However the call ends they go
// in this order: the temporaries, then the stream, then the switch back to the caller's device
struct GsScratch {
    struct OnDevice {
        int before; bool moved;
        explicit OnDevice(int device) : before(rt_get_device()), moved(device >= 0 && device != before) { if (moved) rt_set_device(device); }
        ~OnDevice() { if (moved) { try { rt_set_device(before); } catch (const std::exception &) {} } }
    } dev;
    struct Stream { rt_stream_t h; Stream() : h(rt_stream_create()) {} ~Stream() { rt_stream_destroy(h); } } own;
    rt_stream_t st;
    SpbTemps mem;
    rt_alloc_scope allocOn;
    explicit GsScratch(int device) : dev(device), st(own.h), allocOn(st) {}
    template <class T> T *get(size_t n) { return mem.alloc<T>(n); }      // (zero-filled)
    // a host vector in device memory: allocated, the upload enqueued (v must live until the stream is waited for)
    template <class T> T *up(const std::vector<T> &v)
    {
        T *d = get<T>(v.size());
        if (!v.empty()) rt_h2d(d, v.data(), v.size() * sizeof(T), st);
        return d;
    }
};
// rows of whole 128-byte lines of doubles (and of 64-byte lines of floats)
static size_t pad16(size_t n) { return (n + 15u) & ~(size_t)15u; }
// workgroups of a looping grid: eight of 256 threads fill a compute unit
static uint32_t gs_grid(unsigned long long units)
{
    const unsigned long long room = (unsigned long long)rt_compute_units() * 8ull;
    const unsigned long long g = units < room ? units : room;
    return (uint32_t)(g < 1ull ? 1ull : (g > 0x7FFFFFFFull ? 0x7FFFFFFFull : g));
}

// A host matrix (element (i, k) at src[i * rowStride + k * colStride]) into dst, which has its size and the zeros of its padding: row i
// is the run dst[i * ld ..], or, transposed, column k is the run dst[k * ld ..] -- the rows are then taken a block at a time so that a
// row-major source is read from the cache, not once per column.  The element is converted to dst's type (double from float: exact).
// each(v, i, k), if given, sees every element once, in no promised order, and returns what is stored for it.
template <class D, class S, class Each = std::nullptr_t>
static void stage_matrix(std::vector<D> &dst, size_t ld, bool transpose, const S *src, size_t rows, size_t cols, size_t rowStride, size_t colStride, Each each = nullptr)
{
    const size_t di = transpose ? 1u : ld, dk = transpose ? ld : 1u;
    auto put = [&](size_t i, size_t k) {
        const S v = src[i * rowStride + k * colStride];
        if constexpr (std::is_same<Each, std::nullptr_t>::value) dst[i * di + k * dk] = v; else dst[i * di + k * dk] = each(v, i, k);
    };
    if (!transpose) {
        for (size_t i = 0; i < rows; ++i)
            for (size_t k = 0; k < cols; ++k) put(i, k);
        return;
    }
    for (size_t i0 = 0; i0 < rows; i0 += 1024u) {
        const size_t i1 = rows - i0 < 1024u ? rows : i0 + 1024u;
        for (size_t k = 0; k < cols; ++k)
            for (size_t i = i0; i < i1; ++i) put(i, k);
    }
}

// What a CSR list of sets over the rows of `matrix` is refused for (empty: nothing), in `me`'s name.  Per set, in this order: its draw
// size (drawSizes, if given: 1 .. nRows), offsets that decrease, members without a members array, then -- maxSet != 0: the sets are
// tested one by one -- no member or more than maxSet, then each member (a row of the matrix, above its predecessor), then -- maxSet != 0
// -- as many members as rows.
static std::string set_list_refusal(const std::string &me, const char *matrix, uint32_t nRows, uint32_t nSets, const uint64_t *memberOffsets, const uint32_t *members,
                                    const uint32_t *drawSizes, uint64_t maxSet)
{
    for (uint32_t t = 0; t < nSets; ++t) {
        const std::string set = me + "set " + std::to_string(t);
        if (drawSizes && (drawSizes[t] == 0u || drawSizes[t] > nRows)) return set + ": a draw of " + std::to_string(drawSizes[t]) + " rows is outside 1 .. nRows = " + std::to_string(nRows);
        if (memberOffsets[t + 1u] < memberOffsets[t]) return set + ": memberOffsets decrease";
        const uint64_t m = memberOffsets[t + 1u] - memberOffsets[t];
        if (m && !members) return me + "null argument";
        if (maxSet && m == 0u) return set + ": a set without members is not tested";
        if (maxSet && m > maxSet) return set + ": " + std::to_string(m) + " members are more than GSEA_MAX_SET = " + std::to_string(maxSet);
        for (uint64_t i = memberOffsets[t]; i < memberOffsets[t + 1u]; ++i) {
            if (members[i] >= nRows) return set + ": member " + std::to_string(members[i]) + " is not a row of " + matrix + " (nRows = " + std::to_string(nRows) + ")";
            if (i > memberOffsets[t] && members[i] <= members[i - 1u]) return set + ": members are not ascending";
        }
        if (maxSet && m >= (uint64_t)nRows) return set + ": " + std::to_string(m) + " members are not fewer than nRows = " + std::to_string(nRows);
    }
    return std::string();
}
// The sets [t0, t0 + here) where the kernels read them: their offsets, rebased to the first's, through off (here + 1 words or more, the
// caller's until the stream is waited for) into dOff, their members into dMem
static void upload_sets(const uint64_t *memberOffsets, const uint32_t *members, uint64_t t0, uint32_t here, std::vector<unsigned long long> &off,
                        unsigned long long *dOff, uint32_t *dMem, rt_stream_t st)
{
    const uint64_t first = memberOffsets[t0], nMem = memberOffsets[t0 + here] - first;
    for (uint32_t t = 0; t <= here; ++t) off[t] = memberOffsets[t0 + t] - first;
    rt_h2d(dOff, off.data(), ((size_t)here + 1u) * 8, st);
    if (nMem) rt_h2d(dMem, members + first, (size_t)nMem * 4, st);
}

// ------------------------------------------------------------------------------------------------
// The gene-set permutation statistic (geneset_kernel.h)
// ------------------------------------------------------------------------------------------------
template <int SLOTS>
static void gs_launch(const GsArgs &a, rt_stream_t st)
{
    const unsigned long long colBlocks = (a.K + 64u * SLOTS - 1u) / (64u * SLOTS), chunks = (a.numPerm + GS_PERMS - 1u) / GS_PERMS;
    RT_LAUNCH(gs_actual_kernel<SLOTS>, gs_grid(((unsigned long long)a.nSets * colBlocks + GS_WAVES - 1ull) / GS_WAVES), GS_THREADS, st, a);
    RT_LAUNCH(gs_count_kernel<SLOTS>, gs_grid((unsigned long long)a.nSets * chunks * colBlocks), GS_THREADS, st, a);
}

extern "C" {

int cogaps_gene_set_stat(const double *z, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride,
                         uint32_t nSets, const uint64_t *memberOffsets, const uint32_t *members, const uint32_t *drawSizes,
                         uint32_t numPerm, uint32_t seed, int device, uint32_t *lessThanCount, double *actualMean)
{
    try {
        if (!z || !memberOffsets || !drawSizes || !lessThanCount) return fail("cogaps_gene_set_stat: null argument");
        if (nRows == 0u || nCols == 0u) return fail("cogaps_gene_set_stat: the Z matrix is empty");
        if (nSets == 0u) return fail("cogaps_gene_set_stat: nSets must be at least 1");
        if (numPerm == 0u) return fail("cogaps_gene_set_stat: numPerm must be at least 1");
        const std::string refusal = set_list_refusal("cogaps_gene_set_stat: ", "Z", nRows, nSets, memberOffsets, members, drawSizes, 0u);
        if (!refusal.empty()) return fail(refusal);
        // Z repacked row-major, rows of whole 128-byte lines
        const size_t ld = pad16(nCols);
        std::vector<double> zp((size_t)nRows * ld, 0.0);
        stage_matrix(zp, ld, false, z, nRows, nCols, rowStride, colStride);
        std::vector<unsigned long long> off(nSets + 1u);
        const size_t nOut = (size_t)nSets * nCols;

        GsScratch g(device);
        GsArgs a;
        a.z = g.up(zp); a.ld = ld; a.nRows = nRows; a.K = nCols; a.nSets = nSets; a.numPerm = numPerm; a.seed = seed;
        unsigned long long *dOff = g.get<unsigned long long>(off.size());
        uint32_t *dMem = g.get<uint32_t>(memberOffsets[nSets] - memberOffsets[0]), *dSize = g.get<uint32_t>(nSets);
        upload_sets(memberOffsets, members, 0, nSets, off, dOff, dMem, g.st);
        rt_h2d(dSize, drawSizes, (size_t)nSets * 4, g.st);
        a.memberOffsets = dOff; a.members = dMem; a.drawSizes = dSize; a.actual = g.get<double>(nOut); a.counts = g.get<uint32_t>(nOut);
        if (nCols <= 64u) gs_launch<1>(a, g.st);
        else if (nCols <= 128u) gs_launch<2>(a, g.st);
        else gs_launch<4>(a, g.st);
        rt_d2h(lessThanCount, a.counts, nOut * 4, g.st);
        if (actualMean) rt_d2h(actualMean, a.actual, nOut * 8, g.st);
        rt_sync(g.st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

int cogaps_debug_permutation_draw(uint32_t nRows, uint32_t size, uint32_t seed, uint32_t set, uint32_t perm, int device, uint32_t *out)
{
    try {
        if (!out) return fail("cogaps_debug_permutation_draw: null argument");
        if (size == 0u || size > nRows) return fail("cogaps_debug_permutation_draw: a draw of " + std::to_string(size) + " rows is outside 1 .. nRows = " + std::to_string(nRows));
        GsScratch g(device);
        uint32_t *d = g.get<uint32_t>(size);
        RT_LAUNCH(gs_draw_kernel, 1, 64, g.st, nRows, size, seed, set, perm, d);
        rt_d2h(out, d, (size_t)size * 4, g.st); rt_sync(g.st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// ------------------------------------------------------------------------------------------------
// The genes of a set that behave like the set (genemember_kernel.h)
// ------------------------------------------------------------------------------------------------
int cogaps_gene_set_membership(const double *z, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride,
                               uint32_t nSets, const uint64_t *memberOffsets, const uint32_t *members,
                               const double *wMember, const double *wNull, int device,
                               double *memberStat, uint32_t *greaterCount, double *allStat)
{
    try {
        const std::string me = "cogaps_gene_set_membership: ";
        if (!z || !memberOffsets || !members || !wMember) return fail(me + "null argument");
        if (!memberStat && !greaterCount && !allStat) return fail(me + "null argument: one of memberStat, greaterCount and allStat must be given");
        if (nRows == 0u || nCols == 0u) return fail(me + "the Z matrix is empty");
        if (nSets == 0u) return fail(me + "nSets must be at least 1");
        const std::string refusal = set_list_refusal(me, "Z", nRows, nSets, memberOffsets, members, nullptr, 0u);
        if (!refusal.empty()) return fail(refusal);
        // Z transposed: one column = one run of rows, read lane = row
        const size_t ldn = pad16(nRows);
        std::vector<double> zt(ldn * nCols, 0.0);
        stage_matrix(zt, ldn, true, z, nRows, nCols, rowStride, colStride);
        std::vector<unsigned long long> off(nSets + 1u);
        const size_t nMem = (size_t)(memberOffsets[nSets] - memberOffsets[0]), nW = (size_t)nSets * nCols, nAll = (size_t)nSets * nRows;

        GsScratch g(device);
        GmArgs a;
        memset(&a, 0, sizeof(a));
        a.zt = g.up(zt); a.ldn = ldn; a.nRows = nRows; a.K = nCols; a.nSets = nSets;
        unsigned long long *dOff = g.get<unsigned long long>(off.size());
        uint32_t *dMem = g.get<uint32_t>(nMem);
        upload_sets(memberOffsets, members, 0, nSets, off, dOff, dMem, g.st);
        a.memberOffsets = dOff; a.members = dMem;
        a.wMember = a.wNull = g.mem.stage(wMember, nW, false, g.st);
        if (wNull) a.wNull = g.mem.stage(wNull, nW, false, g.st);
        a.memberStat = g.get<double>(nMem);                                  // (zero-filled, as the counts are)
        if (greaterCount) a.greaterCount = g.get<uint32_t>(nMem);
        if (allStat) a.allStat = g.get<double>(nAll);                        // the one thing of size nSets x nRows, and only on request
        if (memberStat || greaterCount) RT_LAUNCH(gm_member_kernel, gs_grid(((unsigned long long)nSets + GM_WAVES - 1ull) / GM_WAVES), GM_THREADS, g.st, a);
        if (greaterCount || allStat)
            RT_LAUNCH(gm_count_kernel, gs_grid((unsigned long long)nSets * (((unsigned long long)nRows + GM_THREADS - 1ull) / GM_THREADS)), GM_THREADS, g.st, a);
        double *const statOut = memberStat ? memberStat + memberOffsets[0] : nullptr;
        uint32_t *const countOut = greaterCount ? greaterCount + memberOffsets[0] : nullptr;
        if (statOut && nMem) rt_d2h(statOut, a.memberStat, nMem * 8, g.st);
        if (countOut && nMem) rt_d2h(countOut, a.greaterCount, nMem * 4, g.st);
        if (allStat) rt_d2h(allStat, a.allStat, nAll * 8, g.st);
        rt_sync(g.st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// ------------------------------------------------------------------------------------------------
// Pattern markers (markers_kernel.h)
// ------------------------------------------------------------------------------------------------
} // extern "C"

static_assert(COGAPS_MARKERS_ALL == PM_THRESHOLD_ALL && COGAPS_MARKERS_CUT == PM_THRESHOLD_CUT, "the header's thresholds are the kernels'");

// test-only: COGAPS_TEST_MARKERS_SMALL_ROWS / COGAPS_TEST_MARKERS_TILE_ROWS move the ranking's cutoff and the radix sort's tile, so
// that a test reaches every form, and more than one tile, at a few hundred rows
static uint64_t pm_test_override(const char *name, uint64_t natural)
{
    const char *e = getenv(name);
    return e && *e ? (uint64_t)strtoull(e, nullptr, 10) : natural;
}

// the ranking's form for p.n rows: true for the one-workgroup form, else the radix sort's tile is set (p.tileRows, p.nTiles)
static bool pm_sort_plan(PmArgs &p)
{
    uint64_t smallRows = pm_test_override("COGAPS_TEST_MARKERS_SMALL_ROWS", PM_SMALL_ROWS);
    if (smallRows > (uint64_t)PM_SMALL_ROWS) smallRows = PM_SMALL_ROWS;      // (what the kernel's LDS holds)
    uint64_t tileRows = pm_test_override("COGAPS_TEST_MARKERS_TILE_ROWS", PM_TILE_ROWS);
    tileRows = (tileRows + PM_THREADS - 1u) / PM_THREADS * PM_THREADS;
    if (tileRows < (uint64_t)PM_THREADS) tileRows = PM_THREADS;
    if (tileRows > (uint64_t)PM_TILE_ROWS) tileRows = PM_TILE_ROWS;
    p.tileRows = (uint32_t)tileRows; p.nTiles = (uint32_t)(((uint64_t)p.n + tileRows - 1u) / tileRows);
    return (uint64_t)p.n <= smallRows;
}
// the ranking's buffers for the p.L columns of p.ldn rows (pm_sort_plan has been): the second keys / order and the histograms are the radix sort's alone
static void pm_rank_scratch(PmArgs &p, bool small, GsScratch &g)
{
    const size_t nCol = p.ldn * p.L;
    p.keys[0] = g.get<unsigned long long>(nCol); p.order[0] = g.get<uint32_t>(nCol); p.rankT = g.get<uint32_t>(nCol);
    if (small) return;
    p.keys[1] = g.get<unsigned long long>(nCol); p.order[1] = g.get<uint32_t>(nCol);
    p.hist = g.get<uint32_t>((size_t)p.L * PM_THREADS * p.nTiles); p.digitBase = g.get<uint32_t>((size_t)p.L * PM_THREADS);
}
// ranks the L columns of keys[0] / order[0] (stable, ascending): rankT, and order[0] the rows in rank order
static void pm_rank_launch(PmArgs &p, bool small, rt_stream_t st)
{
    const unsigned long long rowBlocks = ((unsigned long long)p.n + PM_THREADS - 1ull) / PM_THREADS, tiles = (unsigned long long)p.L * p.nTiles;
    if (small) { RT_LAUNCH(pm_rank_small_kernel, gs_grid(p.L), PM_THREADS, st, p); return; }
    for (int pass = 0; pass < PM_PASSES; ++pass) {
        p.shift = (uint32_t)pass * PM_DIGIT_BITS;
        RT_LAUNCH(pm_hist_kernel, gs_grid(tiles), PM_THREADS, st, p, pass & 1);
        RT_LAUNCH(pm_hist_scan_kernel, gs_grid(p.L), PM_THREADS, st, p);
        RT_LAUNCH(pm_scatter_kernel, gs_grid(tiles), PM_THREADS, st, p, pass & 1);
    }
    RT_LAUNCH(pm_rank_scatter_kernel, gs_grid(rowBlocks * p.L), PM_THREADS, st, p);
}

extern "C" {

int cogaps_pattern_markers(const double *a, uint64_t nRows, uint32_t nCols, size_t aRowStride, size_t aColStride,
                           const double *o, uint64_t oRows, size_t oRowStride, size_t oColStride,
                           const double *lp, uint32_t nLp, int threshold, int device,
                           uint32_t *ranks, double *scores, uint32_t *markers, uint32_t *markerCount)
{
    try {
        if (!a || !o) return fail("cogaps_pattern_markers: null argument");
        if (nRows == 0u || nCols == 0u || oRows == 0u) return fail("cogaps_pattern_markers: a matrix is empty");
        if (nRows > 0xFFFFFFFFull) return fail("cogaps_pattern_markers: " + std::to_string(nRows) + " rows are more than 32-bit ranks hold");
        if (oRows > 0xFFFFFFFFull) return fail("cogaps_pattern_markers: " + std::to_string(oRows) + " rows of the other matrix are more than 32 bits hold");
        if ((lp == nullptr) != (nLp == 0u)) return fail("cogaps_pattern_markers: lp and its length must be given together (NULL and 0: the unit vectors)");
        for (size_t x = 0; lp && x < (size_t)nLp * nCols; ++x)
            if (!(lp[x] <= 1.0)) return fail("cogaps_pattern_markers: lp should be a list of vectors with max value of 1");
        if (threshold != COGAPS_MARKERS_ALL && threshold != COGAPS_MARKERS_CUT) return fail("cogaps_pattern_markers: unknown threshold " + std::to_string(threshold));
        const uint32_t n = (uint32_t)nRows, m = (uint32_t)oRows, K = nCols, L = lp ? nLp : nCols;
        const size_t ldn = pad16(n), ldm = pad16(m);
        std::vector<double> at(ldn * K, 0.0), ot(ldm * K, 0.0);      // transposed: one column = one run of rows
        stage_matrix(at, ldn, true, a, n, K, aRowStride, aColStride);
        stage_matrix(ot, ldm, true, o, m, K, oRowStride, oColStride);
        const size_t nOut = (size_t)n * L;

        GsScratch g(device);
        PmArgs p;
        memset(&p, 0, sizeof(p));
        p.ldn = ldn; p.ldm = ldm; p.n = n; p.m = m; p.K = K; p.L = L; p.threshold = threshold;
        const bool small = pm_sort_plan(p);
        p.at = g.up(at); p.ot = g.up(ot);                                    // (everything below is zero-filled)
        if (lp) { double *dlp = g.get<double>((size_t)L * K); rt_h2d(dlp, lp, (size_t)L * K * 8, g.st); p.lp = dlp; }
        p.colMax = g.get<unsigned long long>(K);
        pm_rank_scratch(p, small, g);
        p.rowMin = g.get<uint32_t>(n); p.best = g.get<uint32_t>(n);
        p.nanRows = g.get<uint32_t>(1); p.tileCount = g.get<uint32_t>((size_t)L * p.nTiles);
        p.markerCount = g.get<uint32_t>(L);
        if (scores) p.scores = g.get<double>(nOut);
        if (ranks) p.ranks = g.get<uint32_t>(nOut);
        const std::vector<uint32_t> noCut(L, n);
        p.cutPos = g.up(noCut);
        if (markers) { p.markers = g.get<uint32_t>(nOut); rt_memset(p.markers, 0xFF, nOut * 4, g.st); }

        const unsigned long long rowBlocks = ((unsigned long long)n + PM_THREADS - 1ull) / PM_THREADS, tiles = (unsigned long long)L * p.nTiles;
        RT_LAUNCH(pm_colmax_kernel, gs_grid((unsigned long long)K * ((m + PM_TILE_ROWS - 1ull) / PM_TILE_ROWS)), PM_THREADS, g.st, p);
        RT_LAUNCH(pm_normalise_kernel, gs_grid(rowBlocks), PM_THREADS, g.st, p);
        RT_LAUNCH(pm_score_kernel, gs_grid(rowBlocks * ((L + PM_LBLOCK - 1u) / PM_LBLOCK)), PM_THREADS, g.st, p);
        pm_rank_launch(p, small, g.st);
        RT_LAUNCH(pm_rowmin_kernel, gs_grid(rowBlocks), PM_THREADS, g.st, p);
        if (markers || markerCount) {
            if (threshold == COGAPS_MARKERS_CUT) RT_LAUNCH(pm_cutpos_kernel, gs_grid(rowBlocks * L), PM_THREADS, g.st, p);
            RT_LAUNCH(pm_marker_count_kernel, gs_grid(tiles), PM_THREADS, g.st, p);
            RT_LAUNCH(pm_marker_scan_kernel, gs_grid((L + 63u) / 64u), 64, g.st, p);
            if (markers) RT_LAUNCH(pm_marker_write_kernel, gs_grid(tiles), PM_THREADS, g.st, p);
        }
        if (ranks) rt_d2h(ranks, p.ranks, nOut * 4, g.st);
        if (scores) rt_d2h(scores, p.scores, nOut * 8, g.st);
        if (markers) rt_d2h(markers, p.markers, nOut * 4, g.st);
        if (markerCount) rt_d2h(markerCount, p.markerCount, (size_t)L * 4, g.st);
        rt_sync(g.st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// ------------------------------------------------------------------------------------------------
// The enrichment of gene sets in every pattern (gsea_kernel.h)
// ------------------------------------------------------------------------------------------------
int cogaps_pattern_gsea(const float *stat, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride,
                        uint32_t nSets, const uint64_t *memberOffsets, const uint32_t *members,
                        uint32_t numPerm, uint32_t seed, int device,
                        double *es, uint32_t *peak, uint32_t *nGe, uint64_t *permSum, uint32_t *rankOut)
{
    static_assert(COGAPS_GSEA_MAX_SET == GSEA_MAX_SET, "the header's cap is the kernel's");
    try {
        const std::string me = "cogaps_pattern_gsea: ";
        if (!stat || !memberOffsets || !members || !es || !peak || !nGe || !permSum) return fail(me + "null argument");
        if (nRows == 0u || nCols == 0u) return fail(me + "the stat matrix is empty");
        if (nSets == 0u) return fail(me + "nSets must be at least 1");
        if (numPerm == 0u) return fail(me + "numPerm must be at least 1");
        if (numPerm == 0xFFFFFFFFu) return fail(me + "numPerm must be below 2^32 - 1");
        const uint32_t n = nRows, K = nCols;
        // the values transposed (one column = one run of rows, as the sort wants them); -0 becomes +0, which is the same number.  A value
        // that is no factor matrix's: the first in row-major order is named (the staging visits them in another)
        const size_t ldn = pad16(n), ldk = pad16(K);
        std::vector<float> vt(ldn * K, 0.f);
        size_t badRow = n, badCol = 0;
        stage_matrix(vt, ldn, true, stat, n, K, rowStride, colStride, [&](float v, size_t i, size_t k) {
            if (!(v >= 0.f) && (i < badRow || (i == badRow && k < badCol))) { badRow = i; badCol = k; }
            return v + 0.f;
        });
        if (badRow < n) return fail(me + "stat holds a NaN or a negative value (row " + std::to_string(badRow) + ", column " + std::to_string(badCol) + "): factor matrices are non-negative");
        const std::string refusal = set_list_refusal(me, "stat", nRows, nSets, memberOffsets, members, nullptr, GSEA_MAX_SET);
        if (!refusal.empty()) return fail(refusal);

        GsScratch g(device);
        // ranks: the markers' stable sort on the descending keys, then (rank, value) of a row's columns side by side
        const float *dvt = g.up(vt);
        PmArgs p;
        memset(&p, 0, sizeof(p));
        p.ldn = ldn; p.n = n; p.K = K; p.L = K;
        const bool small = pm_sort_plan(p);
        const size_t nCol = ldn * K;
        pm_rank_scratch(p, small, g);
        const unsigned long long rowBlocks = ((unsigned long long)n + PM_THREADS - 1ull) / PM_THREADS;
        RT_LAUNCH(gsea_key_kernel, gs_grid(rowBlocks * K), PM_THREADS, g.st, dvt, p);
        pm_rank_launch(p, small, g.st);
        unsigned long long *pk = g.get<unsigned long long>((size_t)n * ldk);
        RT_LAUNCH(gsea_pack_kernel, gs_grid(((unsigned long long)n * K + PM_THREADS - 1ull) / PM_THREADS), PM_THREADS, g.st,
                  dvt, (const uint32_t *)p.rankT, ldn, n, K, pk, ldk);
        if (rankOut) {
            std::vector<uint32_t> r(nCol);
            rt_d2h(r.data(), p.rankT, nCol * 4, g.st); rt_sync(g.st);
            for (uint32_t k = 0; k < K; ++k)
                for (uint32_t i = 0; i < n; ++i) rankOut[(size_t)k * n + i] = r[(size_t)k * ldn + i] - 1u;
        }

        // scores: the sets in chunks whose outputs and members stay within a fixed amount of device memory
        uint64_t chunkSets = pm_test_override("COGAPS_TEST_GSEA_CHUNK_SETS", ((uint64_t)1 << 22) / K);
        if (chunkSets < 1u) chunkSets = 1u;
        if (chunkSets > nSets) chunkSets = nSets;
        const size_t nOut = (size_t)chunkSets * K, maxMem = (size_t)chunkSets * GSEA_MAX_SET < (size_t)(memberOffsets[nSets] - memberOffsets[0]) ? (size_t)chunkSets * GSEA_MAX_SET : (size_t)(memberOffsets[nSets] - memberOffsets[0]);
        GseaArgs a;
        memset(&a, 0, sizeof(a));
        a.pk = pk; a.ldk = ldk; a.nRows = n; a.K = K; a.seed = seed;
        unsigned long long *dOff = g.get<unsigned long long>(chunkSets + 1u);
        uint32_t *dMem = g.get<uint32_t>(maxMem);
        a.memberOffsets = dOff; a.members = dMem;
        a.es = g.get<double>(nOut); a.peak = g.get<uint32_t>(nOut); a.nGe = g.get<uint32_t>(nOut); a.permSum = g.get<unsigned long long>(nOut);
        std::vector<unsigned long long> off(chunkSets + 1u);
        const unsigned long long kBlocks = (K + GSEA_BLOCK - 1u) / GSEA_BLOCK;
        for (uint64_t t0 = 0; t0 < nSets; t0 += chunkSets) {
            const uint32_t here = (uint32_t)(nSets - t0 < chunkSets ? nSets - t0 : chunkSets);
            const size_t nHere = (size_t)here * K;
            upload_sets(memberOffsets, members, t0, here, off, dOff, dMem, g.st);
            rt_memset(a.nGe, 0, nHere * 4, g.st); rt_memset(a.permSum, 0, nHere * 8, g.st);
            a.nSets = here; a.setBase = (uint32_t)t0;
            a.slot0 = 0u; a.nSlots = 1u;                                         // the sets themselves ...
            RT_LAUNCH(gsea_score_kernel, gs_grid((unsigned long long)here * kBlocks), GSEA_THREADS, g.st, a);
            a.slot0 = 1u; a.nSlots = numPerm;                                    // ... then their permutations, which compare with them
            RT_LAUNCH(gsea_score_kernel, gs_grid((unsigned long long)here * ((numPerm + GSEA_PERMS - 1ull) / GSEA_PERMS) * kBlocks), GSEA_THREADS, g.st, a);
            rt_d2h(es + (size_t)t0 * K, a.es, nHere * 8, g.st); rt_d2h(peak + (size_t)t0 * K, a.peak, nHere * 4, g.st);
            rt_d2h(nGe + (size_t)t0 * K, a.nGe, nHere * 4, g.st); rt_d2h(permSum + (size_t)t0 * K, a.permSum, nHere * 8, g.st);
            rt_sync(g.st);                                                       // (off is rewritten for the next chunk)
        }
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// ------------------------------------------------------------------------------------------------
// Residuals and the chi-square of every gene and sample (residual_kernel.h)
// ------------------------------------------------------------------------------------------------
} // extern "C"

static std::string rs_dims(const char *what, uint64_t has, const char *of, uint64_t wants)
{
    return std::string("cogaps_residuals: the data has ") + std::to_string(has) + " " + what + ", " + of + " has " + std::to_string(wants) + " rows";
}

// A data descriptor's matrix as a call sees it: the handle of a device matrix, and its genes and samples (transposeData applied)
struct RsData { const cogaps_device_matrix *handle = nullptr; uint32_t G = 0, N = 0; };
// What a descriptor with data (its kind is not _NONE) is refused for, in `me`'s name (empty: nothing); a device matrix decides the device
static std::string rs_data_refusal(const std::string &me, const cogaps_residual_data *data, int &device, RsData &d)
{
    const int kind = data->kind;
    uint32_t dr = 0, dc = 0;
    if (kind == COGAPS_RESIDUAL_DATA_DENSE) {
        if (!data->dense) return me + "null argument: dense";
        dr = data->nrow; dc = data->ncol;
    } else if (kind == COGAPS_RESIDUAL_DATA_SPARSE || kind == COGAPS_RESIDUAL_DATA_COO) {
        const cogaps_sparse_matrix *sp = kind == COGAPS_RESIDUAL_DATA_SPARSE ? data->sparse : nullptr;
        const cogaps_coo_matrix *coo = kind == COGAPS_RESIDUAL_DATA_COO ? data->coo : nullptr;
        if (!sp && !coo) return me + "null argument: the matrix";
        if (const char *refusal = sparse_args_refusal(sp, coo)) return refusal;
        dr = sp ? sp->nrow : coo->nrow; dc = sp ? sp->ncol : coo->ncol;
    } else if (kind == COGAPS_RESIDUAL_DATA_DEVICE_MATRIX) {
        d.handle = data->deviceMatrix;
        if (!d.handle) return me + "null argument: deviceMatrix";
        if (device != -1 && device != d.handle->device)
            return me + "the matrix resides on device " + std::to_string(d.handle->device) + ", the call was given device " + std::to_string(device);
        device = d.handle->device;
        dr = d.handle->m.nrow; dc = d.handle->m.ncol;
    } else return me + "unknown kind of data " + std::to_string(kind);
    d.G = data->transposeData ? dc : dr; d.N = data->transposeData ? dr : dc;
    return std::string();
}
// The data where the kernels read them.  Dense: the caller's arrays as they lie, from the first element to the last the strides reach
// (uploaded unless they are on the device), (gene i, sample j) at [i * rowStride + j * colStride].  The sparse kinds: the gene side of
// the sparse model's packed form, by the one builder; nothing of size genes x samples exists.
static void rs_stage_data(GsScratch &g, const cogaps_residual_data *data, const RsData &d, int &source, const float *&dense, const float *&unc,
                          size_t &rowStride, size_t &colStride, SpbSide &sideOut)
{
    const int kind = data->kind;
    const uint32_t G = d.G, N = d.N;
    if (kind == COGAPS_RESIDUAL_DATA_DENSE) {
        source = RS_DATA_DENSE;
        rowStride = data->transposeData ? data->colStride : data->rowStride;
        colStride = data->transposeData ? data->rowStride : data->colStride;
        dense = data->dense; unc = data->uncertainty;
        if (!data->onDevice) {
            const size_t span = (size_t)(G - 1u) * rowStride + (size_t)(N - 1u) * colStride + 1u;
            float *dd = g.get<float>(span); rt_h2d(dd, data->dense, span * 4, g.st); dense = dd;
            if (data->uncertainty) { float *du = g.get<float>(span); rt_h2d(du, data->uncertainty, span * 4, g.st); unc = du; }
        }
        return;
    }
    SpbMatrix staged; const SpbMatrix *src = &staged;
    const unsigned cu = rt_compute_units();
    if (kind == COGAPS_RESIDUAL_DATA_SPARSE) {
        const cogaps_sparse_matrix &m = *data->sparse;
        spb_compressed(staged, m, g.st, [&](auto *from, size_t n) { return g.mem.stage(from, n, m.onDevice != 0, g.st); });
    } else if (kind == COGAPS_RESIDUAL_DATA_COO) {
        const cogaps_coo_matrix &m = *data->coo;
        spb_triplets(staged, m, g.get<unsigned long long>((size_t)(m.nnz / 64 + 1)), cu, g.st,
                     [&](auto *from, size_t n) { return g.mem.stage(from, n, m.onDevice != 0, g.st); });
    } else src = &d.handle->m;
    SpbSide side;
    side.M = G; side.Wn = N / 64u + 1u; side.vals = nullptr;
    side.swap = (data->transposeData == 0) == src->majorIsRow ? 0u : 1u;      // genes are the data's rows unless transposeData
    side.flags = g.get<unsigned long long>((size_t)G * side.Wn); side.prefix = g.get<uint32_t>((size_t)G * side.Wn); side.ptr = g.get<uint32_t>((size_t)G + 1u);
    SpbMap identity; identity.start = identity.list = nullptr; identity.onMajor = 0u;
    spb_build_sides(*src, identity, false, &side, 1, cu, g.st, [&](int, size_t n) { return g.get<float>(n); });
    source = RS_DATA_PACKED; sideOut = side;
}

extern "C" {

int cogaps_residuals(const float *a, uint32_t nGenes, size_t aRowStride, size_t aColStride,
                     const float *p, uint32_t nSamples, size_t pRowStride, size_t pColStride, uint32_t nPatterns,
                     const cogaps_residual_data *data, const uint32_t *rows, uint32_t nRowsOut, int device,
                     double *geneChiSq, double *sampleChiSq, double *chiSq, double *matrixOut, uint64_t *peakDeviceBytes)
{
    try {
        const uint32_t G = nGenes, N = nSamples, K = nPatterns;
        if (!a || !p) return fail("cogaps_residuals: null argument");
        if (G == 0u || N == 0u || K == 0u) return fail("cogaps_residuals: a matrix is empty");
        if (G > 0xFFFFFF00u) return fail("cogaps_residuals: " + std::to_string(G) + " genes are more than the blocks of 64 count in 32 bits");
        if ((rows == nullptr) != (nRowsOut == 0u) || (nRowsOut != 0u && !matrixOut)) return fail("cogaps_residuals: rows, their number and matrixOut must be given together");
        for (uint32_t x = 0; x < nRowsOut; ++x)
            if (rows[x] >= G) return fail("cogaps_residuals: output row " + std::to_string(x) + " asks for gene " + std::to_string(rows[x]) + ", the result has " + std::to_string(G));
        const int kind = data ? data->kind : COGAPS_RESIDUAL_DATA_NONE;
        if (kind == COGAPS_RESIDUAL_DATA_NONE && nRowsOut == 0u) return fail("cogaps_residuals: neither data nor rows: nothing to compute");
        RsData d;
        if (kind != COGAPS_RESIDUAL_DATA_NONE) {
            const std::string refusal = rs_data_refusal("cogaps_residuals: ", data, device, d);
            if (!refusal.empty()) return fail(refusal);
            if (kind != COGAPS_RESIDUAL_DATA_DENSE && data->uncertainty)
                return fail("cogaps_residuals: a sparse matrix takes the default uncertainty only (no uncertainty matrix)");
            if (d.G != G) return fail(rs_dims("genes", d.G, "featureLoadings", G));
            if (d.N != N) return fail(rs_dims("samples", d.N, "sampleFactors", N));
        }
        const uint32_t nSteps = (uint32_t)(((uint64_t)N + 63u) / 64u), nBlocks = (G + (uint32_t)RS_BLOCK - 1u) / (uint32_t)RS_BLOCK;
        const size_t ldp = (size_t)nSteps * 64u;
        // A widened row by row (rows of zeros up to whole blocks), P widened and transposed (zeros past the last sample); the output rows that want each gene
        std::vector<double> a64((size_t)nBlocks * RS_BLOCK * K, 0.0), pt64((size_t)K * ldp, 0.0);
        stage_matrix(a64, K, false, a, G, K, aRowStride, aColStride);
        stage_matrix(pt64, ldp, true, p, N, K, pRowStride, pColStride);
        std::vector<uint32_t> outStart, outList(nRowsOut);
        if (nRowsOut) {
            outStart.assign((size_t)G + 1u, 0u);
            for (uint32_t x = 0; x < nRowsOut; ++x) ++outStart[(size_t)rows[x] + 1u];
            for (size_t i = 0; i < G; ++i) outStart[i + 1u] += outStart[i];
            std::vector<uint32_t> cursor(outStart.begin(), outStart.end() - 1);
            for (uint32_t x = 0; x < nRowsOut; ++x) outList[cursor[rows[x]]++] = x;
        }

        rt_alloc_meter meter;                                                // (outlives everything the call allocates)
        rt_meter_scope metered(&meter);
        GsScratch g(device);
        RsArgs r;
        memset(&r, 0, sizeof(r));
        r.G = G; r.N = N; r.K = K; r.nSteps = nSteps; r.ldp = ldp; r.source = RS_DATA_NONE;
        r.a64 = g.up(a64); r.pt64 = g.up(pt64);
        if (kind != COGAPS_RESIDUAL_DATA_NONE) rs_stage_data(g, data, d, r.source, r.data, r.unc, r.rowStride, r.colStride, r.side);
        double *dSample = nullptr, *dChi = nullptr;
        if (kind != COGAPS_RESIDUAL_DATA_NONE) {
            r.geneChiSq = g.get<double>(G); r.partial = g.get<double>((size_t)nBlocks * ldp);
            dSample = g.get<double>(N); dChi = g.get<double>(1);
        }
        if (nRowsOut) { r.outStart = g.up(outStart); r.outList = g.up(outList); r.matrixOut = g.get<double>((size_t)nRowsOut * N); }
        RT_LAUNCH(rs_main_kernel, gs_grid(nBlocks), RS_THREADS, g.st, r);
        if (kind != COGAPS_RESIDUAL_DATA_NONE) {
            RT_LAUNCH(rs_fold_kernel, (uint32_t)(((uint64_t)N + RS_THREADS - 1u) / RS_THREADS) + 1u, RS_THREADS, g.st, r, dSample, dChi);
            if (geneChiSq) rt_d2h(geneChiSq, r.geneChiSq, (size_t)G * 8, g.st);
            if (sampleChiSq) rt_d2h(sampleChiSq, dSample, (size_t)N * 8, g.st);
            if (chiSq) rt_d2h(chiSq, dChi, 8, g.st);
        }
        if (nRowsOut) rt_d2h(matrixOut, r.matrixOut, (size_t)nRowsOut * N * 8, g.st);
        rt_sync(g.st);
        if (peakDeviceBytes) *peakDeviceBytes = meter.peak.load();
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// ------------------------------------------------------------------------------------------------
// Consensus patterns: the step between the passes of a distributed run (consensus_kernel.h)
// ------------------------------------------------------------------------------------------------
} // extern "C"

static_assert(COGAPS_PATTERN_MATCH_MAX_COLS == CS_MAX_COLS, "the header's limit is the clustering kernel's");

// What one clustering works with: the distances, the matrix it destroys, the list of its columns and of its merges on the device
struct CsCutree {
    GsScratch &g;
    const double *dist; size_t ld;
    double *w; uint32_t *dCols, *dMerges;
    // cutree(agnes(complete), k) of the sub-block of dist of `cols` (null: all m columns): the label of every one, 1-based, numbered
    // by first appearance.  k >= m: singletons, nothing is launched.
    std::vector<uint32_t> labels(const std::vector<uint32_t> *cols, uint32_t m, uint32_t k)
    {
        std::vector<uint32_t> root(m), label(m, 0u), ofRoot(m, 0u);
        for (uint32_t i = 0; i < m; ++i) root[i] = i;
        if (k < m) {
            if (cols) rt_h2d(dCols, cols->data(), (size_t)m * 4, g.st);
            RT_LAUNCH(cs_gather_kernel, gs_grid(((unsigned long long)m * m + CS_THREADS - 1ull) / CS_THREADS), CS_THREADS, g.st,
                      dist, ld, cols ? (const uint32_t *)dCols : (const uint32_t *)nullptr, m, w, (size_t)m);
            RT_LAUNCH(cs_link_kernel, 1, CS_LINK_THREADS, g.st, w, (size_t)m, m, k, dMerges);
            std::vector<uint32_t> merges(2u * (size_t)(m - k));
            rt_d2h(merges.data(), dMerges, merges.size() * 4, g.st); rt_sync(g.st);
            for (size_t s = 0; s < merges.size(); s += 2) {
                const uint32_t lo = merges[s], hi = merges[s + 1u];
                if (lo >= hi || hi >= m || root[hi] != hi) throw std::runtime_error("cogaps_pattern_match: the clustering left no pair to merge");
                root[hi] = lo;
            }
            for (uint32_t i = 0; i < m; ++i) root[i] = root[root[i]];      // (a cluster keeps its lowest index: root[i] <= i, resolved before i)
        }
        uint32_t next = 0;
        for (uint32_t i = 0; i < m; ++i) {
            if (!ofRoot[root[i]]) ofRoot[root[i]] = ++next;
            label[i] = ofRoot[root[i]];
        }
        return label;
    }
    // corcut: the clusters of `cols` (null: all m columns) with minNS members or more, in the order of their first members, as columns of X
    std::vector<std::vector<uint32_t>> cut(const std::vector<uint32_t> *cols, uint32_t m, uint32_t k, uint32_t minNS, std::vector<uint32_t> *labelsOut = nullptr)
    {
        const std::vector<uint32_t> label = labels(cols, m, k);
        uint32_t most = 0;
        for (uint32_t l : label) most = l > most ? l : most;
        std::vector<std::vector<uint32_t>> all(most), kept;
        for (uint32_t i = 0; i < m; ++i) all[label[i] - 1u].push_back(cols ? (*cols)[i] : i);
        for (auto &c : all) if (c.size() >= (size_t)minNS) kept.push_back(std::move(c));
        if (labelsOut) *labelsOut = label;
        return kept;
    }
};

extern "C" {

int cogaps_pattern_match(const float *patterns, uint32_t nRows, uint32_t nCols, size_t rowStride, size_t colStride, int onDevice,
                         uint32_t cut, uint32_t minNS, uint32_t maxNS, int device,
                         uint32_t *nClusters, uint32_t *cluster, double *corr, float *consensus, double *dist, uint32_t *firstLabels)
{
    try {
        const std::string me = "cogaps_pattern_match: ";
        if (!patterns || !nClusters || !cluster || !consensus) return fail(me + "null argument");
        if (nRows == 0u || nCols == 0u) return fail(me + "the pattern matrix is empty");
        if (nCols < 2u) return fail(me + "nCols must be at least 2: one pattern has nothing to be matched with");
        if (cut == 0u) return fail(me + "cut must be at least 1");
        if (minNS == 0u) return fail(me + "minNS must be at least 1");
        if (maxNS < minNS) return fail(me + "maxNS = " + std::to_string(maxNS) + " is below minNS = " + std::to_string(minNS));
        if (nCols > CS_MAX_COLS) return fail(me + std::to_string(nCols) + " patterns are more than COGAPS_PATTERN_MATCH_MAX_COLS = " + std::to_string(CS_MAX_COLS));
        const uint32_t L = nRows, n = nCols;

        GsScratch g(device);
        CsArgs a;
        memset(&a, 0, sizeof(a));
        a.L = L; a.n = n; a.nChunks = (uint32_t)(((uint64_t)L + CS_KC - 1u) / CS_KC); a.ldx = ((size_t)n + CS_TILE - 1u) / CS_TILE * CS_TILE;
        a.rowStride = rowStride; a.colStride = colStride;
        // the caller's array as it lies, from the first element to the last the strides reach -- or where it lies on the device
        a.x = g.mem.stage(patterns, (size_t)(L - 1u) * rowStride + (size_t)(n - 1u) * colStride + 1u, onDevice != 0, g.st);
        a.xr = g.get<float>((size_t)L * a.ldx); a.partial = g.get<double>((size_t)a.nChunks * a.ldx); a.mean = g.get<double>(a.ldx);
        a.c = g.get<double>((size_t)n * a.ldx); a.dist = g.get<double>((size_t)n * a.ldx); a.flags = g.get<uint32_t>(4);
        const unsigned long long colBlocks = ((unsigned long long)n + CS_THREADS - 1ull) / CS_THREADS, tiles = a.ldx / CS_TILE;
        uint32_t flags[4] = {0u, 0u, 0u, 0u};
        RT_LAUNCH(cs_stage_kernel, gs_grid(tiles * (((unsigned long long)L + CS_TILE - 1ull) / CS_TILE)), CS_THREADS, g.st, a);
        RT_LAUNCH(cs_colsum_kernel<float>, gs_grid(colBlocks * a.nChunks), CS_THREADS, g.st, (const float *)a.xr, a.ldx, L, n, a.nChunks, a.partial, a.ldx);
        RT_LAUNCH(cs_mean_kernel, gs_grid(colBlocks), CS_THREADS, g.st, (const double *)a.partial, a.ldx, L, n, a.nChunks, a.mean);
        rt_d2h(flags, a.flags, sizeof(flags), g.st); rt_sync(g.st);
        if (flags[CS_FLAG_INPUT]) return fail(me + "the patterns hold a NaN or a negative value: factor matrices are non-negative");
        RT_LAUNCH(cs_cross_kernel, gs_grid(tiles * (tiles + 1ull) / 2ull), CS_THREADS, g.st, a);
        RT_LAUNCH(cs_dist_kernel, gs_grid(((unsigned long long)n * n + CS_THREADS - 1ull) / CS_THREADS), CS_THREADS, g.st, a);
        rt_d2h(flags, a.flags, sizeof(flags), g.st); rt_sync(g.st);
        if (flags[CS_FLAG_DIST]) return fail(me + "NA values in correlation of patterns");
        if (dist) {
            std::vector<double> padded((size_t)n * a.ldx);
            rt_d2h(padded.data(), a.dist, padded.size() * 8, g.st); rt_sync(g.st);
            for (size_t i = 0; i < n; ++i) memcpy(dist + i * n, padded.data() + i * a.ldx, (size_t)n * 8);
        }

        // patternMatch: corcut of everything, then the first cluster above maxNS is split in two until none is left (a handful of integers: host)
        CsCutree tree{g, a.dist, a.ldx, g.get<double>((size_t)n * n), g.get<uint32_t>(n), g.get<uint32_t>(2u * (size_t)n)};
        std::vector<uint32_t> first;
        std::vector<std::vector<uint32_t>> clusters = tree.cut(nullptr, n, cut, minNS, &first);
        if (firstLabels) memcpy(firstLabels, first.data(), (size_t)n * 4);
        for (;;) {
            size_t big = 0;
            while (big < clusters.size() && clusters[big].size() <= (size_t)maxNS) ++big;
            if (big == clusters.size()) break;
            std::vector<std::vector<uint32_t>> parts = tree.cut(&clusters[big], (uint32_t)clusters[big].size(), 2u, minNS);
            if (parts.empty()) { clusters.erase(clusters.begin() + (ptrdiff_t)big); continue; }
            clusters[big] = std::move(parts[0]);
            if (parts.size() > 1u) clusters.push_back(std::move(parts[1]));
        }
        if (clusters.empty()) return fail(me + "no cluster of patterns reaches minNS members");

        // the clusters' statistics: their members one after the other
        const uint32_t nC = (uint32_t)clusters.size();
        std::vector<uint32_t> start(nC + 1u, 0u), slotCol, slotCluster;
        for (uint32_t c = 0; c < nC; ++c) {
            for (uint32_t col : clusters[c]) { slotCol.push_back(col); slotCluster.push_back(c); }
            start[c + 1u] = (uint32_t)slotCol.size();
        }
        CsClusterArgs s;
        memset(&s, 0, sizeof(s));
        s.xr = a.xr; s.ldx = a.ldx; s.mean = a.mean; s.c = a.c; s.L = L; s.nChunks = a.nChunks; s.nC = nC; s.T = (uint32_t)slotCol.size();
        s.start = g.up(start); s.slotCol = g.up(slotCol); s.slotCluster = g.up(slotCluster);
        s.ldc = pad16(nC);
        s.mp = g.get<double>((size_t)L * s.ldc); s.mpw = g.get<double>((size_t)L * s.ldc);
        s.partial = g.get<double>((size_t)a.nChunks * s.ldc); s.mpMean = g.get<double>(s.ldc); s.maxPart = g.get<double>((size_t)a.nChunks * s.ldc);
        s.cpart = g.get<double>((size_t)a.nChunks * (s.T + nC)); s.r = g.get<double>(s.T); s.w = g.get<double>(s.T);
        s.consensus = g.get<float>((size_t)L * nC); s.flags = a.flags;
        const unsigned long long cells = ((unsigned long long)L * nC + CS_THREADS - 1ull) / CS_THREADS, cBlocks = ((unsigned long long)nC + CS_THREADS - 1ull) / CS_THREADS;
        RT_LAUNCH(cs_meanpat_kernel, gs_grid(cells), CS_THREADS, g.st, s);
        RT_LAUNCH(cs_colsum_kernel<double>, gs_grid(cBlocks * a.nChunks), CS_THREADS, g.st, (const double *)s.mp, s.ldc, L, nC, a.nChunks, s.partial, s.ldc);
        RT_LAUNCH(cs_mean_kernel, gs_grid(cBlocks), CS_THREADS, g.st, (const double *)s.partial, s.ldc, L, nC, a.nChunks, s.mpMean);
        RT_LAUNCH(cs_cluster_cross_kernel, gs_grid((((unsigned long long)s.T + nC + CS_THREADS - 1ull) / CS_THREADS) * a.nChunks), CS_THREADS, g.st, s);
        RT_LAUNCH(cs_corr_kernel, gs_grid(((unsigned long long)s.T + CS_THREADS - 1ull) / CS_THREADS), CS_THREADS, g.st, s);
        RT_LAUNCH(cs_wmean_kernel, gs_grid(cells), CS_THREADS, g.st, s);
        RT_LAUNCH(cs_colmax_kernel, gs_grid(cBlocks * a.nChunks), CS_THREADS, g.st, s);
        RT_LAUNCH(cs_consensus_kernel, gs_grid(cells), CS_THREADS, g.st, s);
        std::vector<double> r(s.T);
        rt_d2h(r.data(), s.r, (size_t)s.T * 8, g.st); rt_d2h(flags, a.flags, sizeof(flags), g.st); rt_sync(g.st);
        if (flags[CS_FLAG_CORR]) return fail(me + "NA values in correlation of patterns");
        rt_d2h(consensus, s.consensus, (size_t)L * nC * 4, g.st); rt_sync(g.st);
        for (uint32_t j = 0; j < n; ++j) { cluster[j] = 0u; if (corr) corr[j] = (double)NAN; }
        for (uint32_t t = 0; t < s.T; ++t) { cluster[slotCol[t]] = slotCluster[t] + 1u; if (corr) corr[slotCol[t]] = r[t]; }
        *nClusters = nC;
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// ------------------------------------------------------------------------------------------------
// MANOVA's sums of squares and cross-products (manova_kernel.h)
// ------------------------------------------------------------------------------------------------
int cogaps_manova_sscp(const float *x, uint32_t nRows, uint32_t nCols, size_t xRowStride, size_t xColStride,
                       const double *y, uint32_t nResp, size_t yRowStride, size_t yColStride, int device,
                       double *xMean, double *yMean, double *sxx, double *sxy, double *syy)
{
    try {
        const std::string me = "cogaps_manova_sscp: ";
        if (!x || !y) return fail(me + "null argument");
        if (!xMean && !yMean && !sxx && !sxy && !syy) return fail(me + "null argument: one of xMean, yMean, sxx, sxy and syy must be given");
        if (nResp < 1u || nResp > MV_MAX_RESP) return fail(me + std::to_string(nResp) + " response columns are outside 1 .. MV_MAX_RESP = " + std::to_string(MV_MAX_RESP));
        if (nCols < 1u) return fail(me + "the predictor matrix has no column");
        if ((uint64_t)nRows < (uint64_t)nResp + 2u) return fail(me + std::to_string(nRows) + " rows are fewer than nResp + 2 = " + std::to_string(nResp + 2u) + ": no residual degree of freedom is left");
        if (!xRowStride || !xColStride || !yRowStride || !yColStride) return fail(me + "a stride of zero");
        const uint64_t outs64 = (uint64_t)nCols * (1u + nResp) + (uint64_t)nResp * nResp;
        if (outs64 >= 0x80000000ull) return fail(me + std::to_string(nCols) + " predictor columns with " + std::to_string(nResp) + " responses are 2^31 sums or more");
        const uint32_t K = nCols, p = nResp, cols = K + p, outs = (uint32_t)outs64;
        // X and Y row-major without padding: the caller's own array where it lies so already, else repacked
        const size_t nx = (size_t)nRows * K, ny = (size_t)nRows * p;
        std::vector<float> xp;
        std::vector<double> yp;
        if (!(xColStride == 1u && xRowStride == K)) { xp.resize(nx); stage_matrix(xp, K, false, x, nRows, K, xRowStride, xColStride); }
        if (!(yColStride == 1u && yRowStride == p)) { yp.resize(ny); stage_matrix(yp, p, false, y, nRows, p, yRowStride, yColStride); }

        GsScratch g(device);
        MvArgs a;
        memset(&a, 0, sizeof(a));
        a.x = g.mem.stage(xp.empty() ? x : xp.data(), nx, false, g.st);
        a.y = g.mem.stage(yp.empty() ? y : yp.data(), ny, false, g.st);
        a.n = nRows; a.K = K; a.p = p; a.nTrips = (uint32_t)(((uint64_t)nRows + MV_TRIP - 1u) / MV_TRIP);
        a.part1 = g.get<double>((size_t)a.nTrips * cols); a.mean = g.get<double>(cols);
        a.part2 = g.get<double>((size_t)a.nTrips * outs); a.out2 = g.get<double>(outs);
        const uint32_t blocks1 = (cols + 63u) / 64u, blocks2 = (K + 63u) / 64u + 1u;      // blocks of 64 columns; pass 2: X's, and one for syy
        RT_LAUNCH(mv_sum_kernel, gs_grid(a.nTrips), 64u * (blocks1 < 4u ? blocks1 : 4u), g.st, a);
        RT_LAUNCH(mv_mean_kernel, (cols + MV_THREADS - 1u) / MV_THREADS, MV_THREADS, g.st, a);
        RT_LAUNCH(mv_sscp_kernel, gs_grid(a.nTrips), 64u * (blocks2 < 4u ? blocks2 : 4u), g.st, a);
        RT_LAUNCH(mv_fold_kernel, (outs + MV_THREADS - 1u) / MV_THREADS, MV_THREADS, g.st, a);
        if (xMean) rt_d2h(xMean, a.mean, (size_t)K * 8, g.st);
        if (yMean) rt_d2h(yMean, a.mean + K, (size_t)p * 8, g.st);
        if (sxx) rt_d2h(sxx, a.out2, (size_t)K * 8, g.st);
        if (sxy) rt_d2h(sxy, a.out2 + K, (size_t)K * p * 8, g.st);
        if (syy) rt_d2h(syy, a.out2 + K + (size_t)K * p, (size_t)p * p * 8, g.st);
        rt_sync(g.st);
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

// ------------------------------------------------------------------------------------------------
// New data projected onto a result's patterns (project_kernel.h)
// ------------------------------------------------------------------------------------------------
int cogaps_project(const float *loadings, uint32_t nGenes, size_t lRowStride, size_t lColStride, uint32_t nPatterns,
                   const cogaps_residual_data *data, const uint32_t *dataRows, int device,
                   double *coef, double *rss, double *gram, double *stdevUnscaled, double *cross, uint64_t *peakDeviceBytes)
{
    static_assert(COGAPS_PROJECT_TRIP == PJ_TRIP && COGAPS_PROJECT_MAX_PATTERNS == PJ_MAX_PATTERNS, "the header's constants are the kernels'");
    try {
        const std::string me = "cogaps_project: ";
        const uint32_t n = nGenes, K = nPatterns;
        if (!loadings || !coef) return fail(me + "null argument");
        if (!data || data->kind == COGAPS_RESIDUAL_DATA_NONE) return fail(me + "null argument: there is no data to project");
        RsData d;
        const std::string refusal = rs_data_refusal(me, data, device, d);
        if (!refusal.empty()) return fail(refusal);
        if (data->uncertainty) return fail(me + "an uncertainty matrix is not taken: the fit is unweighted");
        if (d.G == 0u || d.N == 0u) return fail(me + "the data is empty");
        if (K == 0u) return fail(me + "nPatterns must be at least 1");
        if (K > PJ_MAX_PATTERNS) return fail(me + std::to_string(K) + " patterns are more than PJ_MAX_PATTERNS = " + std::to_string(PJ_MAX_PATTERNS));
        if (n <= K) return fail(me + std::to_string(n) + " genes are not more than nPatterns = " + std::to_string(K) + ": no residual degree of freedom is left");
        if (!dataRows && n != d.G) return fail(me + "the data has " + std::to_string(d.G) + " genes, the loadings have " + std::to_string(n) + " rows (and no dataRows match them)");
        for (uint32_t i = 0; dataRows && i < n; ++i)
            if (dataRows[i] >= d.G) return fail(me + "gene " + std::to_string(i) + " asks for row " + std::to_string(dataRows[i]) + ", the data has " + std::to_string(d.G));
        const uint32_t S = d.N, tri = PJ_TRI(K);
        // the loadings widened, row-major without padding
        std::vector<double> l64((size_t)n * K);
        bool finite = true;
        stage_matrix(l64, K, false, loadings, n, K, lRowStride, lColStride, [&](float v, size_t, size_t) { if (!std::isfinite(v)) finite = false; return (double)v; });
        if (!finite) return fail(me + "the loadings hold a NaN or an infinite value");

        rt_alloc_meter meter;                                                // (outlives everything the call allocates)
        rt_meter_scope metered(&meter);
        GsScratch g(device);
        PjArgs a;
        memset(&a, 0, sizeof(a));
        a.n = n; a.K = K; a.S = S; a.nTrips = (uint32_t)(((uint64_t)n + PJ_TRIP - 1u) / PJ_TRIP); a.nSBlocks = (uint32_t)(((uint64_t)S + PJ_THREADS - 1u) / PJ_THREADS);
        a.l64 = g.up(l64);
        if (dataRows) { uint32_t *dr = g.get<uint32_t>(n); rt_h2d(dr, dataRows, (size_t)n * 4, g.st); a.rows = dr; }
        const float *noUnc = nullptr;
        rs_stage_data(g, data, d, a.source, a.data, noUnc, a.rowStride, a.colStride, a.side);
        const size_t nKS = (size_t)K * S;
        a.gramPart = g.get<double>((size_t)a.nTrips * tri); a.gramTri = g.get<double>(tri); a.gram = g.get<double>((size_t)K * K);
        a.factor = g.get<double>(tri); a.unit = g.get<double>((size_t)K * K); a.stdev = g.get<double>(K); a.bad = g.get<uint32_t>(1);
        a.crossPart = g.get<double>((size_t)a.nTrips * nKS); a.cross = g.get<double>(nKS); a.coef = g.get<double>(nKS);
        if (rss) { a.rssPart = g.get<double>((size_t)a.nTrips * S); a.rss = g.get<double>(S); }

        RT_LAUNCH(pj_gram_kernel, gs_grid(a.nTrips), PJ_THREADS, g.st, a);
        RT_LAUNCH(pj_gram_fold_kernel, (tri + PJ_THREADS - 1u) / PJ_THREADS, PJ_THREADS, g.st, a);
        RT_LAUNCH(pj_factor_kernel, 1, PJ_THREADS, g.st, a);
        uint32_t bad = CG_NONE;
        rt_d2h(&bad, a.bad, 4, g.st); rt_sync(g.st);
        if (bad != CG_NONE) return fail(me + "loadings are rank deficient (pattern " + std::to_string(bad) + " adds nothing to the patterns before it)");
        const unsigned long long units = (unsigned long long)a.nTrips * a.nSBlocks;
        RT_LAUNCH(pj_cross_kernel, gs_grid(units), PJ_THREADS, g.st, a);
        RT_LAUNCH(pj_fold_kernel, (uint32_t)((nKS + PJ_THREADS - 1u) / PJ_THREADS), PJ_THREADS, g.st, (const double *)a.crossPart, nKS, a.nTrips, a.cross, a.coef);
        RT_LAUNCH(pj_solve_kernel, a.nSBlocks, PJ_THREADS, g.st, a);
        if (rss) {
            RT_LAUNCH(pj_rss_kernel, gs_grid(units), PJ_THREADS, g.st, a);
            RT_LAUNCH(pj_fold_kernel, a.nSBlocks, PJ_THREADS, g.st, (const double *)a.rssPart, (size_t)S, a.nTrips, a.rss, (double *)nullptr);
            rt_d2h(rss, a.rss, (size_t)S * 8, g.st);
        }
        rt_d2h(coef, a.coef, nKS * 8, g.st);
        if (cross) rt_d2h(cross, a.cross, nKS * 8, g.st);
        if (gram) rt_d2h(gram, a.gram, (size_t)K * K * 8, g.st);
        if (stdevUnscaled) rt_d2h(stdevUnscaled, a.stdev, (size_t)K * 8, g.st);
        rt_sync(g.st);
        if (peakDeviceBytes) *peakDeviceBytes = meter.peak.load();
        return 0;
    } catch (const std::exception &e) { return fail_exc(e); }
}

} // extern "C"
