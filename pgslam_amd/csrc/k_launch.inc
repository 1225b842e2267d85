// k_launch.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): host-side launchers and explicit instantiations.

// ---------------------------------------------------------------------------
// launchers (host side, called from pgicp_api.cpp)
// ---------------------------------------------------------------------------
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int round8(int x) { return (x + 7) & ~7; }

template <typename T>
void launch_centroid_bbox_batch(hipStream_t st, const BuildDesc<T> *descs, int n, int max_m, unsigned long long *stats)
{
    int nb = cdiv(max_m, 256 * 8);
    if (nb < 1) nb = 1;
    if (nb > 512) nb = 512;
    hipLaunchKernelGGL(k_centroid_bbox_b<T>, dim3(nb, n), dim3(256), 0, st, descs, stats);
}

// descs: device array; totals over the batch: points, fine cells (incl. one sentinel slot per cloud), super-cells, bins
// scratch: fkey / skey [tot_m], arrival [tot_m], words [tot_m] (64 bit), bins_a / bins_b [max(tot_b + 1, tot_c)] (bin counts
// and starts, then the sweeps' scratch), block_sums
template <typename T>
void launch_grid_build_batch(hipStream_t st, const BuildDesc<T> *descs, int n, long long tot_m, long long tot_b, long long tot_s,
                             int max_m, int max_cells, int max_bins, int max_nsc, int max_blocks, int kx_all4, int *fkey, int *bins_a, int *block_sums,
                             int *cell_start, int *cell_start_f, int *bins_b, int *arrival, unsigned long long *words,
                             typename Vec4<T>::type *cpts, typename Vec4<T>::type *cnrm,
                             typename Vec4<T>::type *pts, typename Vec4<T>::type *nrm_out,
                             int *slot_of, int *sc_count, int *near, int *sc_dist, int *sc_wit, unsigned *occ, long long tot_o, float *sc_ext, float *ptsf,
                             uint4 *sw, int *ostart, int *flag_scratch, int *rank_scratch)
{
    // sw != null: the maps of this build carry the succinct table (MapDev::sw / ostart) instead of the dense ones;
    // flag_scratch / rank_scratch: tot_m + 1 ints each
    (void)hipMemsetAsync(bins_a, 0, sizeof(int) * (tot_b + 1), st);
    (void)hipMemsetAsync(occ, 0, sizeof(unsigned) * tot_o, st);
    (void)hipMemsetAsync(sc_count, 0, sizeof(int) * tot_s, st);
    hipLaunchKernelGGL(k_mbin<T>, dim3(cdiv(max_m, kBinBlock), n), dim3(kBinBlock), 0, st, descs, fkey, bins_a, arrival, cpts, cnrm);
    launch_exclusive_scan(st, bins_a, (int)(tot_b + 1), bins_b, block_sums);
    const dim3 per_point(cdiv(max_m, 256), n);
    hipLaunchKernelGGL(k_mscatter<T>, per_point, dim3(256), 0, st, descs, (const int *)fkey, (const int *)bins_b, (const int *)arrival, words);
    hipLaunchKernelGGL(k_mchunk_sort<T>, kChunk == 1024 ? dim3(cdiv(max_m, 1024), n) : per_point, dim3(256), 0, st, descs, words);
    // (`fkey` is dead once the words are scattered: it becomes the sorted keys)
    hipLaunchKernelGGL(k_mplace<T>, dim3(cdiv(max_m, kPlaceSpan), n), dim3(256), 0, st, descs, (const int *)bins_b, (const unsigned long long *)words,
                       (const typename Vec4<T>::type *)cpts, (const typename Vec4<T>::type *)cnrm, pts, nrm_out, fkey, reinterpret_cast<float4 *>(ptsf));
    (void)slot_of;
    if (sw) {
        hipLaunchKernelGGL(k_mflags<T>, per_point, dim3(256), 0, st, descs, (const int *)fkey, flag_scratch, tot_m);
        launch_exclusive_scan(st, flag_scratch, (int)(tot_m + 1), rank_scratch, block_sums);     // (block_sums: the bins' scan is done with it)
        hipLaunchKernelGGL(k_mostart, dim3(cdiv(tot_m + 1, 256)), dim3(256), 0, st, (const int *)flag_scratch, (const int *)rank_scratch, tot_m, ostart);
        hipLaunchKernelGGL((k_mfill<T, true>), dim3(cdiv(max_bins, kFillGroup), n), dim3(256), 0, st, descs, (const int *)bins_b, (const int *)fkey, cell_start_f,
                           cell_start, occ, sc_count, sw, (const int *)rank_scratch);
    } else
        hipLaunchKernelGGL((k_mfill<T, false>), dim3(cdiv(max_bins, kFillGroup), n), dim3(256), 0, st, descs, (const int *)bins_b, (const int *)fkey, cell_start_f,
                           cell_start, occ, sc_count, (uint4 *)nullptr, (const int *)nullptr);
    // (the bin tables are scratch from here on: the sweeps of the near / super-cell tables)
    int *counts = bins_a, *cursor = bins_b;
    for (int pass = -1; pass < 3; pass++)
        hipLaunchKernelGGL(k_near_b<T>, dim3(cdiv(max_blocks, 256), n), dim3(256), 0, st, descs, pass, (const unsigned *)occ, counts,
                           cursor, near);
    if (max_nsc <= 4096) {
        hipLaunchKernelGGL(k_scdist_b<T>, dim3(n), dim3(1024), 0, st, descs, (const int *)sc_count, counts, cursor, sc_dist);
    } else {
        for (int pass = 0; pass < 3; pass++)
            hipLaunchKernelGGL(k_scdist_pass_b<T>, dim3(cdiv(max_nsc, 256), n), dim3(256), 0, st, descs, pass, (const int *)sc_count,
                               counts, cursor, sc_dist);
    }
    // (`counts` is scratch by now: the first point of every occupied super-cell, then the witness table)
    hipLaunchKernelGGL(k_sc_first_b<T>, dim3(cdiv(max_nsc, 256), n), dim3(256), 0, st, descs, (const int *)sc_count, (const int *)cell_start, counts,
                       (const uint4 *)sw, (const int *)ostart);
    hipLaunchKernelGGL(k_sc_wit_b<T>, dim3(cdiv(max_nsc, 256), n), dim3(256), 0, st, descs, (const int *)sc_dist, (const int *)counts, sc_wit);
    hipLaunchKernelGGL(k_sc_extent_b<T>, dim3(cdiv(max_nsc, 256), n), dim3(256), 0, st, descs, (const int *)sc_count, (const unsigned *)occ, sc_ext);
}

// once per scan: move every problem's reading into its map's centred frame and order it by (block of map cells, cell, index)
template <typename T>
void launch_query_sort(hipStream_t st, const ProblemDev *probs, const SrcDesc *src, const MapDev<T> *maps, typename Vec4<T>::type *rd_pre, T *rd_sorted,
                       int *qkey, unsigned long long *qtmp, int *order, int *counts, int *block_sums, int *qstart, int P,
                       int max_n, int max_rows, int bin_shift, typename Vec4<T>::type *nrm_pre, T *nrm_sorted)
{
    const long long nbins = (long long)P * max_rows;
    // (`counts` arrives cleared: launch_batch_setup, the call's one set-up kernel)
    const dim3 grid(cdiv(max_n, 256), P);
    // `order` carries the arrival positions until k_qplace overwrites it with the final permutation
    hipLaunchKernelGGL(k_qbin<T>, dim3(cdiv(max_n, kBinBlock), P), dim3(kBinBlock), 0, st, probs, src, maps, rd_pre, max_rows, bin_shift, qkey, counts, order, nrm_pre);
    launch_exclusive_scan(st, counts, (int)nbins, qstart, block_sums);
    hipLaunchKernelGGL(k_qscatter, grid, dim3(256), 0, st, probs, max_rows, 3 * bin_shift, (const int *)qkey, (const int *)qstart, (const int *)order, qtmp);
    hipLaunchKernelGGL(k_qchunk_sort, kChunk == 1024 ? dim3(cdiv(max_n, 1024), P) : grid, dim3(256), 0, st, probs, qtmp);
    hipLaunchKernelGGL(k_qplace<T>, dim3(cdiv(max_n, kPlaceSpan), P), dim3(256), 0, st, probs, max_rows, 3 * bin_shift, (const int *)qstart,
                       (const unsigned long long *)qtmp, (const typename Vec4<T>::type *)rd_pre, rd_sorted, order,
                       (const typename Vec4<T>::type *)nrm_pre, nrm_sorted);
}

size_t knn_queue_counter_words(int n_problems) { return (size_t)n_problems * 8 * kQueueCounterStride; }

void launch_batch_setup(hipStream_t st, int *active, int P, int *z0, long long n0, int *z1, long long n1, int *z2, long long n2, int *z3, long long n3)
{
    const long long words = n0 + n1 + n2 + n3;
    const int blocks = (int)std::min<long long>(4096, std::max<long long>(1, cdiv(std::max<long long>(words, P), 256 * 4)));
    hipLaunchKernelGGL(k_batch_setup, dim3(blocks), dim3(256), 0, st, active, P, z0, n0, z1, n1, z2, n2, z3, n3);
}

void launch_invert_order(hipStream_t st, const ProblemDev *probs, const int *order, int *scan_pos, int P, int max_n)
{
    hipLaunchKernelGGL(k_invert_order, dim3(cdiv(max_n, 256), P), dim3(256), 0, st, probs, order, scan_pos);
}

template <typename T>
void launch_transform(hipStream_t st, const T *in, int in_stride, T *out, int out_stride, int n, const double *T16,
                      int rotate_only)
{
    Mat34 M;
    for (int i = 0; i < 12; i++) M.v[i] = T16[i];
    if (n > 0)
        hipLaunchKernelGGL(k_transform<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, in, in_stride, out, out_stride, n, M,
                           rotate_only);
}

// queries of one XCD's span of tiles (+ one tile: with fewer than 64 queries per wave the spans are cut elsewhere)
// (The capacity does not depend on WHICH tiles an XCD runs, only on how many: the fast matcher's grid is a multiple of 8
// blocks, and tile_of_block (tile_map.hpp) hands every class b & 7 exactly nb / 8 = ceil(nb / 8) of a problem's tiles for
// every group size, as the spans did -- at most that many times `lanes` queries can reach the segment of (problem, XCD).)
static inline int knn_q_cap(int max_n) { return (round8(cdiv(max_n, kFastBlock)) / 8) * kFastBlock + kFastBlock; }

size_t knn_queue_bytes(int n_problems, int max_n, size_t elem)
{
    const size_t nseg = (size_t)n_problems * 8, q_cap = (size_t)knn_q_cap(max_n);
    return nseg * kQueueCounterStride * sizeof(int) + nseg * sizeof(int) + nseg * q_cap * (sizeof(int2) + elem + sizeof(int)) + 1024;
}

// experiment knobs (integer environment variables, read once)
static inline int env_knob(const char *name, int dflt)
{
    const char *v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}
// the fast matcher's tile groups (tile_map.hpp, DESIGN §4): what an unset PGICP_TILE_GROUP means
constexpr int kTileGroupUnset = -0x7fffffff;
constexpr int kTileGroupDefault = 4;

template <typename T>
void launch_knn(hipStream_t st, int matcher, const ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot,
                T *d2, const ChainDev<T> &ch, int P, int max_n, int use_seed, int *slow_count, int2 *slow_list, T *slow_lb,
                int *slow_ring, int fast_rings, const int *active, T *none_r, int n_problems, void *queue_buf, int clear_queue_counters,
                int table_kinds)
{
    if (matcher == 1) {
        (void)hipMemsetAsync(slow_count, 0, 4 * sizeof(int), st);
        hipLaunchKernelGGL(k_knn_brute<T>, dim3(cdiv(max_n, kKnnBlock), P), dim3(kKnnBlock), 0, st, probs, maps, rd, slot, d2,
                           ch, active);
        return;
    }
    // segmented queue of this pass (see finish_query): [counters | starts | list | lb | ring]
    const int nseg = n_problems * 8, q_cap = knn_q_cap(max_n);
    char *qb = (char *)queue_buf;
    int *seg_count = (int *)qb;                 qb += sizeof(int) * (size_t)nseg * kQueueCounterStride;
    int *seg_start = (int *)qb;                 qb += (sizeof(int) * (size_t)nseg + 255) & ~(size_t)255;
    int2 *seg_list = (int2 *)qb;                qb += sizeof(int2) * (size_t)nseg * q_cap;
    T *seg_lb = (T *)qb;                        qb += sizeof(T) * (size_t)nseg * q_cap;
    int *seg_ring = (int *)qb;
    // (inside an ICP run the first selection of the previous iteration has cleared them: sel_finish)
    if (clear_queue_counters) (void)hipMemsetAsync(seg_count, 0, sizeof(int) * (size_t)nseg * kQueueCounterStride, st);
    {
        // R = 1 in both cases: measured, a 5x5x5 collected block on the unseeded first iteration costs
        // 2.5x the ring-by-ring continuation (nothing prunes it until the own row has a hit)
        // queries per wave: all 64 lanes when that still gives the chip a wave per slot (8 per SIMD), fewer for a small launch
        static const int forced_lanes = env_knob("PGICP_FAST_LANES", 0);
        // (measured: 16 per wave for one 100 k-pt scan, fast kernel -10 %; a 10 k-pt scan is quicker left at 64 -- 550 vs
        // 516 scans/s through the SLAM facade -- so small launches are not spread further than 16 per wave, tiny ones not at all)
        int lanes = kFastBlock;
        if ((long long)P * max_n >= 50000)
            while (lanes > 16 && (long long)P * cdiv(max_n, lanes >> 1) <= 8192) lanes >>= 1;
        if (forced_lanes > 0) lanes = std::min(forced_lanes, kFastBlock);
        // tiles per group dealt round the XCDs (tile_of_block, tile_map.hpp): PGICP_TILE_GROUP; <= 0 one contiguous span per XCD
        static const int forced_group = env_knob("PGICP_TILE_GROUP", kTileGroupUnset);
        const int tile_group = forced_group != kTileGroupUnset ? forced_group : kTileGroupDefault;
        // (table_kinds: bit 0 -- some map of the batch carries the dense tables, bit 1 -- some map the succinct one)
        if (table_kinds & 1)
            hipLaunchKernelGGL((k_knn_grid<T, 1, 0>), dim3(round8(cdiv(max_n, lanes)), P), dim3(kFastBlock), 0, st, probs, maps, rd, slot, d2, ch,
                               use_seed, fast_rings, seg_count, seg_list, seg_lb, seg_ring, active, none_r, q_cap, lanes, tile_group);
        if (table_kinds & 2)
            hipLaunchKernelGGL((k_knn_grid<T, 1, 1>), dim3(round8(cdiv(max_n, lanes)), P), dim3(kFastBlock), 0, st, probs, maps, rd, slot, d2, ch,
                               use_seed, fast_rings, seg_count, seg_list, seg_lb, seg_ring, active, none_r, q_cap, lanes, tile_group);
    }
    if (P <= 8) {                                     // up to eight ACTIVE problems -- a small batch, or the last iterations of a large one
                                                      // (a finished problem's counters are zero: its last first selection cleared them): see k_queue_small
        hipLaunchKernelGGL(k_queue_small<T>, dim3(P * 8, cdiv(q_cap, 256)), dim3(256), 0, st, (const int *)seg_count, nseg, q_cap,
                           (const int2 *)seg_list, (const T *)seg_lb, (const int *)seg_ring, slow_list, slow_lb, slow_ring, active, slow_count);
        return;
    }
    hipLaunchKernelGGL(k_queue_offsets, dim3(1), dim3(1024), 0, st, (const int *)seg_count, nseg, seg_start, slow_count);
    hipLaunchKernelGGL(k_queue_compact<T>, dim3(P * 8, cdiv(q_cap, 256)), dim3(256), 0, st, (const int *)seg_count, (const int *)seg_start,
                       q_cap, (const int2 *)seg_list, (const T *)seg_lb, (const int *)seg_ring, slow_list, slow_lb, slow_ring, active);
}

template <typename T>
void launch_borrow_order(hipStream_t st, const ProblemDev *probs, const SrcDesc *src, const int *order_a, const int *slot_a, const typename Vec4<T>::type *pts_a,
                         int first_a, int m_a, int n, const SeedSegs &sg, const int *slot_of_b, int m_b, T *rd_sorted, int *order_b, int *slot_b)
{
    hipLaunchKernelGGL(k_borrow_order<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, probs, src, order_a, slot_a, pts_a, first_a, m_a, n, sg, slot_of_b, m_b, rd_sorted, order_b, slot_b);
}

template <typename T>
void launch_knn_med(hipStream_t st, ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot, T *d2,
                    const ChainDev<T> &ch, int *slow_count, const int2 *slow_list, T *slow_lb, int *slow_ring, int *slow2_idx,
                    int med_rings, int use_seed, T *none_r)
{
    static const int short_rings = env_knob("PGICP_MED_SHORT_RINGS", 1);
    hipLaunchKernelGGL(k_knn_med<T>, dim3(8192), dim3(64), 0, st, probs, maps, rd, slot, d2, ch, slow_count, slow_list, slow_lb,
                       slow_ring, slow2_idx, med_rings, use_seed, none_r, short_rings);
}

// KDTreeMatcher.knn > 1: the top-K matcher (k_normals.inc); returns -1 when knn exceeds its register lists
template <typename T>
int launch_knn_topk(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot, T *d2,
                    const ChainDev<T> &ch, int P, int max_n, const int *active)
{
    const dim3 grid(cdiv(max_n, 128), P), block(128);
    if (ch.knn <= 2) hipLaunchKernelGGL((k_knn_topk<T, 2>), grid, block, 0, st, probs, maps, rd, slot, d2, ch, active);
    else if (ch.knn <= 4) hipLaunchKernelGGL((k_knn_topk<T, 4>), grid, block, 0, st, probs, maps, rd, slot, d2, ch, active);
    else if (ch.knn <= 8) hipLaunchKernelGGL((k_knn_topk<T, 8>), grid, block, 0, st, probs, maps, rd, slot, d2, ch, active);
    else if (ch.knn <= 16) hipLaunchKernelGGL((k_knn_topk<T, 16>), grid, block, 0, st, probs, maps, rd, slot, d2, ch, active);
    else return -1;
    return 0;
}

// resolves the queries the fast path queued: all of them (exact_all, public matcher
// output) or only those that can still matter for the trimmed filter (lazy)
constexpr int kSlowBlocks = 2048;

template <typename T>
void launch_knn_slow(hipStream_t st, ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot, T *d2,
                     const ChainDev<T> &ch, const int *slow_count, const int2 *slow_list, const T *slow_lb,
                     const int *slow2_idx, int exact_all, T *none_r)
{
    static const int square_rows = env_knob("PGICP_SLOW_SQUARE_ROWS", kSlowSquareRows);
    static const int slow_blocks = env_knob("PGICP_SLOW_BLOCKS", kSlowBlocks);
    static const int prune_pct = env_knob("PGICP_PRUNE_PCT", 3);       // the walk prunes this far beyond maxDist (see k_knn_slow)
    hipLaunchKernelGGL(k_knn_slow<T>, dim3(slow_blocks), dim3(256), 0, st, probs, maps, rd, slot, d2, ch, slow_count, slow_list,
                       slow_lb, slow2_idx, exact_all, none_r, square_rows, (T)(1.0 + 0.01 * prune_pct));
}

// (guess: 0 none -- the three-launch selection; 1 the last selection's result: k_sel_band + k_sel_final2)
constexpr int kSelBandMinProblems = 4;
static inline int sel_small_n() { static const int v = env_knob("PGICP_SEL_SMALL_N", 32768); return v; }
template <typename T>
void launch_trim_select(hipStream_t st, ProblemDev *probs, const T *d2, const ChainDev<T> &ch, int P, int max_n, int second,
                        const int *active, int *tables, void *keys, int *seg_count, int guess)
{
    using U = typename Bits<T>::U;
    const int small_n = sel_small_n();
    // PGICP_SEL_BAND: 1 the band path whenever there is a guess, 0 never, unset: only for batches -- for one problem (a scan of the
    // SLAM facade, a streamed scan) the band path's final stage is ONE block that selects inside a compacted list, a serial tail of
    // 7-12 us (57 when the guess was off) where the three-launch selection's stages are each wide and short: measured on the
    // single-thread facade at sensor size, six interleaved pairs, +2 ... +10 % scans/s (profiles/r06_experiments/facade_knobs.txt)
    static const int band_knob = env_knob("PGICP_SEL_BAND", -1);
    const int use_band = band_knob >= 0 ? band_knob : (P >= kSelBandMinProblems ? 1 : 0);
    if (max_n <= small_n) {
        hipLaunchKernelGGL(k_sel_small<T>, dim3(P), dim3(kSelectBlock), 0, st, probs, d2, ch, second, active, seg_count);
        return;
    }
    // about 2048 blocks in all: every block costs one table merge (global atomics on the problem's bins)
    const int tiles = cdiv(max_n, kSelTile);
    const int per_problem = std::min(tiles, std::max(1, 2048 / P));
    const int span = cdiv(tiles, per_problem) * kSelTile;
    const dim3 wide(cdiv(max_n, span), P);
    if (guess && use_band) {
        // the last selection's result as a guess (ProblemDev::qraw): one pass, two launches
        hipLaunchKernelGGL(k_sel_band<T>, wide, dim3(256), 0, st, (const ProblemDev *)probs, d2, second, active, tables, (U *)keys, span);
        hipLaunchKernelGGL(k_sel_final2<T>, dim3(P), dim3(kSelectBlock), 0, st, probs, d2, ch, second, active, tables, (const U *)keys, seg_count);
        return;
    }
    hipLaunchKernelGGL(k_sel_hist<T>, wide, dim3(256), 0, st, (const ProblemDev *)probs, d2, second, active, tables, span);
    hipLaunchKernelGGL(k_sel_filter<T>, wide, dim3(256), 0, st, (const ProblemDev *)probs, d2, ch, second, active, tables, (U *)keys, span);
    // (filter and final stage merged through a last-block ticket -- two launches per selection -- measured slower: the
    // final stage is a serial tail, and 256 threads run it four times as long as 1 024: the history of tools/experiments/, r03_e14)
    hipLaunchKernelGGL(k_sel_final<T>, dim3(P), dim3(kSelectBlock), 0, st, probs, ch, second, active, tables, (const U *)keys, seg_count);
}

size_t trim_select_table_bytes(int P) { return sizeof(int) * (size_t)P * kSelStride; }

// diagnostics: selections of this process (current device) whose guess was off since the last call with reset != 0
int sel_fallbacks_read(int reset)
{
    int v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_sel_fallbacks), sizeof v) != hipSuccess) return -1;
    if (reset) { const int z = 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_sel_fallbacks), &z, sizeof z); }
    return v;
}

template <typename T>
int launch_surface_normals(hipStream_t st, const MapDev<T> *maps, int map, int m, int knn, T max_dist, T eps_rank, T *out_nrm,
                           int out_stride, T *out_eig, int *out_ids, T *out_d2)
{
    const dim3 grid(cdiv(m, 128)), block(128);
    if (knn <= 8) hipLaunchKernelGGL((k_surface_normals<T, 8>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, out_ids, out_d2);
    else if (knn <= 16) hipLaunchKernelGGL((k_surface_normals<T, 16>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, out_ids, out_d2);
    else if (knn <= 32) hipLaunchKernelGGL((k_surface_normals<T, 32>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, out_ids, out_d2);
    else return -1;
    return 0;
}

// pgicp_normals_ext.h: the instantiation with both epilogues (any output may be null; x's rows as NormalsExtOut says)
template <typename T>
int launch_surface_normals_ext(hipStream_t st, const MapDev<T> *maps, int map, int m, int knn, T max_dist, T eps_rank, T *out_nrm,
                               int out_stride, T *out_eig, int *out_ids, T *out_d2, T *out_dens, const NormalsExtOut<T> &x)
{
    const dim3 grid(cdiv(m, 128)), block(128);
    if (knn <= 8) hipLaunchKernelGGL((k_surface_normals<T, 8, true, true>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, out_ids, out_d2, out_dens, x);
    else if (knn <= 16) hipLaunchKernelGGL((k_surface_normals<T, 16, true, true>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, out_ids, out_d2, out_dens, x);
    else if (knn <= 32) hipLaunchKernelGGL((k_surface_normals<T, 32, true, true>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, out_ids, out_d2, out_dens, x);
    else return -1;
    return 0;
}

template <typename T>
void launch_smooth_normals(hipStream_t st, const T *nrm, int ns, const int *nb, long long rs, long long cs, int knn, int n, const int *out_of,
                           T *out, int os, int *bad)
{
    if (bad) (void)hipMemsetAsync(bad, 0, sizeof(int), st);
    hipLaunchKernelGGL(k_smooth_normals<T>, dim3(cdiv(n, 128)), dim3(128), 0, st, nrm, ns, nb, rs, cs, knn, n, out_of, out, os, bad);
}

int reduce_blocks(int max_n) { return round8(cdiv(max_n, kReduceSpan)); }

// (max_n: the largest number of PAIRS of a problem = points x knn; rd_nrm: the sorted reading normals when a
// SurfaceNormalOutlierFilter is in the chain, else null)
template <typename T>
void launch_reduce(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd_pre, const T *rd_nrm, const int *slot,
                   const T *d2, double *partials, int P, int max_n, const int *active, const ChainDev<T> &ch)
{
    const int nb = reduce_blocks(max_n);
    const dim3 grid(nb, P), block(kReduceBlock);
    const bool gen = ch.knn > 1 || rd_nrm != nullptr || ch.robust.fct != 0 || ch.gd_mode != PGICP_DESC_FILTER_OFF;
#define PGICP_REDUCE_LAUNCH(MIN, GEN) \
    hipLaunchKernelGGL((k_p2plane_reduce<T, MIN, GEN>), grid, block, 0, st, probs, maps, rd_pre, rd_nrm, slot, d2, partials, nb, active, ch.normal_cos, ch.robust, ch.scan_pos, \
                       ch.gd_mode, ch.gd_thr)
    if (ch.minimizer == 1) { if (gen) PGICP_REDUCE_LAUNCH(1, true); else PGICP_REDUCE_LAUNCH(1, false); }
    else { if (gen) PGICP_REDUCE_LAUNCH(0, true); else PGICP_REDUCE_LAUNCH(0, false); }
#undef PGICP_REDUCE_LAUNCH
}

template <typename T>
void launch_solve(hipStream_t st, ProblemDev *probs, const double *partials, const ChainDev<T> &ch, int *n_done, int P,
                  int max_n, const int *active, int *single_host_flag, int *single_stamp, int *single_queue_counters)
{
    // (the three `single_` pointers: non-null for a batch of one problem, whose solve kernel does k_compact_active's work too)
    hipLaunchKernelGGL(k_solve_update<T>, dim3(P), dim3(256), 0, st, probs, partials, reduce_blocks(max_n), ch, n_done, active,
                       single_host_flag, single_stamp, single_queue_counters);
}

template <typename T>
void launch_cov(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd_pre, const T *rd_nrm, const int *slot,
                const T *d2, double *partials, double *out, int P, int max_n, const ChainDev<T> &ch)
{
    const int nb = reduce_blocks(max_n);
    if (ch.gd_mode != PGICP_DESC_FILTER_OFF)
        hipLaunchKernelGGL((k_cov_reduce<T, true>), dim3(nb, P), dim3(kReduceBlock), 0, st, probs, maps, rd_pre, rd_nrm, slot, d2, partials, nb, ch.normal_cos,
                           ch.robust, ch.scan_pos, ch.gd_mode, ch.gd_thr);
    else
        hipLaunchKernelGGL((k_cov_reduce<T, false>), dim3(nb, P), dim3(kReduceBlock), 0, st, probs, maps, rd_pre, rd_nrm, slot, d2, partials, nb, ch.normal_cos,
                           ch.robust, ch.scan_pos, ch.gd_mode, ch.gd_thr);
    hipLaunchKernelGGL(k_sum_partials, dim3(P), dim3(256), 0, st, (const double *)partials, nb, kCovTerms, probs, 0, out);
}

// RobustOutlierFilter (k_minimise.inc): lift the lazy matcher's threshold; the scale of this iteration
void launch_robust_open(hipStream_t st, ProblemDev *probs, const int *active, int n_active)
{
    hipLaunchKernelGGL(k_robust_open, dim3(cdiv(n_active, 64)), dim3(64), 0, st, probs, active, n_active);
}
// GenericDescriptorOutlierFilter (k_minimise.inc): soft mode's uncapped matcher; the soft maximum of this iteration; the values
void launch_gd_open(hipStream_t st, ProblemDev *probs, const int *active, int n_active)
{
    hipLaunchKernelGGL(k_gd_open, dim3(cdiv(n_active, 64)), dim3(64), 0, st, probs, active, n_active);
}
template <typename T>
void launch_gd_max(hipStream_t st, ProblemDev *probs, const MapDev<T> *maps, const int *slot, int n_active, int max_pairs, const int *active)
{
    hipLaunchKernelGGL(k_gd_max<T>, dim3(cdiv(max_pairs, 256 * kGdMaxItems), n_active), dim3(256), 0, st, probs, maps, slot, active);
}
template <typename T>
void launch_map_values(hipStream_t st, const typename Vec4<T>::type *pts, int first, int m, const T *values, int stride, T *out, int *flags)
{
    hipLaunchKernelGGL(k_map_values<T>, dim3(cdiv(m, 256)), dim3(256), 0, st, pts, first, m, values, stride, out, flags);
}

template <typename T>
void launch_robust_scale(hipStream_t st, ProblemDev *probs, const T *d2, T *dev, const ChainDev<T> &ch, int n_active, int max_pairs,
                         const int *active, int *tables, void *keys, int phase, int part)
{
    // phase: a RobustPhase; part: -1 everything, or (the caller profiles them apart) 0 the first selection, 1 the deviations and
    // their median, 2 the finish
    const bool all = part < 0;
    const bool mad = phase == kRobustMad || (phase == kRobustLegacy && ch.robust.mad);
    ChainDev<T> half = ch;
    half.trim_ratio = (T)0.5; half.trim_scale = (T)1;
    // (no guesses: the two medians alternate -- each would start from the other's value)
    if (all || part == 0) {
        if (mad || phase == kRobustMedian) launch_trim_select<T>(st, probs, d2, half, n_active, max_pairs, 0, active, tables, keys, nullptr, 0);
        // scaleEstimator none: one selection over the resolved distances all the same, for the count of finite pairs
        else if (phase == kRobustLegacy) launch_trim_select<T>(st, probs, d2, ch, n_active, max_pairs, 0, active, tables, keys, nullptr, 0);
    }
    if ((all || part == 1) && mad) {
        hipLaunchKernelGGL(k_robust_absdev<T>, dim3(cdiv(max_pairs, 256), n_active), dim3(256), 0, st, (const ProblemDev *)probs, d2, dev, active);
        launch_trim_select<T>(st, probs, (const T *)dev, half, n_active, max_pairs, 0, active, tables, keys, nullptr, 0);
    }
    if (all || part == 2) {
        // a held iteration ran no selection: the pairs with a neighbour are counted behind the finish, which clears the count
        const int count = phase == kRobustHold ? 1 : 0;
        hipLaunchKernelGGL(k_robust_finish<T>, dim3(cdiv(n_active, 64)), dim3(64), 0, st, probs, active, n_active, ch.robust, ch.outlier_max_d2, count);
        if (count) hipLaunchKernelGGL(k_robust_count<T>, dim3(cdiv(max_pairs, 256 * kRobustCountItems), n_active), dim3(256), 0, st, probs, d2, active);
    }
}

void launch_sum_partials(hipStream_t st, const double *partials, int max_blocks, int nt, const ProblemDev *probs,
                         int nb_uniform, double *out, int P)
{
    hipLaunchKernelGGL(k_sum_partials, dim3(P), dim3(256), 0, st, partials, max_blocks, nt, probs, nb_uniform, out);
}

template <typename T>
void launch_trim_raw(hipStream_t st, const T *d2, int n, T ratio, T scale, T *limit_nf, T *w)
{
    hipLaunchKernelGGL(k_trim_select_raw<T>, dim3(1), dim3(kSelectBlock), 0, st, d2, n, ratio, scale, limit_nf);
    if (w) hipLaunchKernelGGL(k_weights<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, d2, n, (const T *)limit_nf, w);
}

template <typename T>
void launch_robust_raw(hipStream_t st, const T *d2, int n, const RobustDev<T> &rb, T *dev, T *stat, T *w)
{
    if (rb.mad) {
        hipLaunchKernelGGL(k_trim_select_raw<T>, dim3(1), dim3(kSelectBlock), 0, st, d2, n, (T)0.5, (T)1, stat);
        hipLaunchKernelGGL(k_robust_absdev_raw<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, d2, n, (const T *)stat, dev);
        hipLaunchKernelGGL(k_trim_select_raw<T>, dim3(1), dim3(kSelectBlock), 0, st, (const T *)dev, n, (T)0.5, (T)1, stat + 2);
    } else if (rb.est == 2)
        hipLaunchKernelGGL(k_trim_select_raw<T>, dim3(1), dim3(kSelectBlock), 0, st, d2, n, (T)0.5, (T)1, stat);   // (berg, iteration 1: the median)
    else
        hipLaunchKernelGGL(k_trim_select_raw<T>, dim3(1), dim3(kSelectBlock), 0, st, d2, n, (T)1, (T)1, stat);     // (the finite count)
    if (w) hipLaunchKernelGGL(k_robust_weights_raw<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, d2, n, rb, (const T *)stat, w);
}

template <typename T>
void launch_slot_of(hipStream_t st, const typename Vec4<T>::type *pts, int first, int m, int *slot_of)
{
    hipLaunchKernelGGL(k_slot_of<T>, dim3(cdiv(m, 256)), dim3(256), 0, st, pts, first, m, slot_of);
}

template <typename T>
void launch_error_stats(hipStream_t st, const MapDev<T> *maps, int map, const int *slot_of, const T *rd, int stride,
                        const int *ids, const T *w, int n, int knn, const T mean[3], double *partials, double *out, int minimizer)
{
    const int nb = cdiv((long long)n * knn, kReduceSpan);
    if (minimizer == 1)
        hipLaunchKernelGGL((k_error_stats<T, 1>), dim3(nb), dim3(kReduceBlock), 0, st, maps, map, slot_of, rd, stride, ids, w, n, knn,
                           mean[0], mean[1], mean[2], partials);
    else
        hipLaunchKernelGGL((k_error_stats<T, 0>), dim3(nb), dim3(kReduceBlock), 0, st, maps, map, slot_of, rd, stride, ids, w, n, knn,
                           mean[0], mean[1], mean[2], partials);
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, (const double *)partials, nb, kSys,
                       (const ProblemDev *)nullptr, nb, out);
}

template <typename T>
void launch_unpermute(hipStream_t st, const MapDev<T> *maps, int map, const int *order, const int *slot, const T *d2, int n, int knn,
                      int *ids_out, T *d2_out)
{
    hipLaunchKernelGGL(k_unpermute<T>, dim3(cdiv((long long)n * knn, 256)), dim3(256), 0, st, maps, map, order, slot, d2, n, knn, ids_out, d2_out);
}

// MaxQuantileOnAxis (k_axisquantile.inc): the scratch of one selection, and the selection -- the table's memset and three launches
constexpr int kAqTableInts = kSelBins + 8;     // k_aq_hist's bins, then the candidate list's cursor
template <typename T>
static AqScratch aq_scratch(Carve &cv, int n)
{
    AqScratch w;
    w.table = cv.take<int>(kAqTableInts);
    w.result = cv.take<AqResult>(1);
    w.keys = cv.take<typename Bits<T>::U>((size_t)std::max(n, 1));      // worst case: every point in the rank's bin
    return w;
}
size_t axis_quantile_scratch_bytes(int n, size_t elem)
{
    Carve cv;
    if (elem == 4) (void)aq_scratch<float>(cv, n); else (void)aq_scratch<double>(cv, n);
    return cv.used;
}
AqScratch axis_quantile_scratch(void *base, int n, size_t elem)
{
    Carve cv(base);
    return elem == 4 ? aq_scratch<float>(cv, n) : aq_scratch<double>(cv, n);
}

template <typename T>
void launch_axis_quantile(hipStream_t st, const T *feat, int stride, int dim, int n, const int *keep, T ratio, const AqScratch &w)
{
    using U = typename Bits<T>::U;
    (void)hipMemsetAsync(w.table, 0, sizeof(int) * kAqTableInts, st);
    // about 2048 blocks at the most: every block costs one table merge
    const int tiles = cdiv(n, kSelTile);
    const int blocks = std::min(tiles, 2048);
    const int span = cdiv(tiles, blocks) * kSelTile;
    const dim3 wide(cdiv(n, span));
    hipLaunchKernelGGL(k_aq_hist<T>, wide, dim3(256), 0, st, feat, stride, dim, n, keep, w.table, span);
    hipLaunchKernelGGL(k_aq_filter<T>, wide, dim3(256), 0, st, feat, stride, dim, n, keep, ratio, w.table, (U *)w.keys, span);
    hipLaunchKernelGGL(k_aq_final<T>, dim3(1), dim3(kSelectBlock), 0, st, ratio, (const int *)w.table, (const U *)w.keys, w.result);
}

// The localizer's input filters + sensor transform on the device (k_filter.inc).  `filters`: n entries of (type, p[8]) as
// pgicp.h's pgicp_filter.  keep / pos: n + 1 ints each; block_sums: scan scratch.  pos[n] ends up holding the number kept.
template <typename T>
void launch_filter_cloud(hipStream_t st, const T *feat, int fstride, int frows, const T *desc, int drows, int n, int n_filters,
                         const int *types, const double *params, const double *T16, int rot0, int rot1, int *keep, int *pos,
                         int *block_sums, T *out_feat, T *out_desc, int *kept_idx, int *dropped, int dropped_cap, const AqScratch *aq)
{
    FilterList fl;
    std::memset(&fl, 0, sizeof fl);
    fl.n = std::min(n_filters, 8);
    for (int k = 0; k < fl.n; ++k) { fl.f[k].type = types[k]; for (int j = 0; j < 8; ++j) fl.f[k].p[j] = params[8 * k + j]; }
    const dim3 grid(cdiv(n, 256)), block(256);
    hipLaunchKernelGGL(k_fill_int, dim3(cdiv(n + 1, 256)), block, 0, st, keep, n + 1, 1);
    int k = 0;
    while (k < fl.n) {
        int e = k;
        while (e < fl.n && fl.f[e].type != PGICP_F_FIX_STEP && fl.f[e].type != PGICP_F_RANDOM_SAMPLING && fl.f[e].type != PGICP_F_MAX_POINT_COUNT &&
               fl.f[e].type != PGICP_F_MAX_QUANTILE_ON_AXIS) ++e;
        if (e > k) hipLaunchKernelGGL(k_filter_points<T>, grid, block, 0, st, feat, fstride, frows, desc, drows, n, fl, k, e, keep);
        if (e < fl.n && fl.f[e].type == PGICP_F_MAX_QUANTILE_ON_AXIS) {
            // the third kind of entry: it looks at all the survivors before it decides -- the selection over the flags as they
            // stand, then the cut; the limit stays on the device (aq: the caller's scratch, required with such an entry)
            const int dim = (int)fl.f[e].p[0];
            launch_axis_quantile<T>(st, feat, fstride, dim, n, keep, (T)fl.f[e].p[1], *aq);
            hipLaunchKernelGGL(k_aq_apply<T>, grid, block, 0, st, feat, fstride, dim, n, (const AqResult *)aq->result, keep);
            ++e;
        } else if (e < fl.n) {
            launch_exclusive_scan(st, keep, n, pos, block_sums);
            hipLaunchKernelGGL(k_filter_index, grid, block, 0, st, n, fl.f[e], (const int *)pos, keep);
            ++e;
        }
        k = e;
    }
    launch_exclusive_scan(st, keep, n, pos, block_sums);
    Mat34 M;
    for (int i = 0; i < 12; i++) M.v[i] = T16 ? T16[i] : (i % 5 == 0 ? 1.0 : 0.0);
    // (descriptors handed in for a CutAtDescriptor entry alone -- no out_desc -- stay behind)
    hipLaunchKernelGGL(k_filter_compact<T>, grid, block, 0, st, feat, fstride, frows, out_desc ? desc : (const T *)nullptr, drows, n, (const int *)keep, (const int *)pos, M,
                       T16 ? 1 : 0, rot0, rot1, out_feat, out_desc, kept_idx, dropped, dropped_cap);
}

#define INSTANTIATE(T)                                                                                                   \
    template void launch_centroid_bbox_batch<T>(hipStream_t, const BuildDesc<T> *, int, int, unsigned long long *);       \
    template void launch_grid_build_batch<T>(hipStream_t, const BuildDesc<T> *, int, long long, long long, long long, int, \
                                             int, int, int, int, int, int *, int *, int *, int *, int *, int *, int *, unsigned long long *, typename Vec4<T>::type *, \
                                             typename Vec4<T>::type *, typename Vec4<T>::type *,                                                  \
                                             typename Vec4<T>::type *, int *, int *, int *, int *, int *, unsigned *, long long, float *, float *, \
                                             uint4 *, int *, int *, int *); \
    template void launch_query_sort<T>(hipStream_t, const ProblemDev *, const SrcDesc *, const MapDev<T> *, typename Vec4<T>::type *, T *, int *,  \
                                       unsigned long long *, int *, int *, int *, int *, int, int, int, int, typename Vec4<T>::type *, T *); \
    template void launch_transform<T>(hipStream_t, const T *, int, T *, int, int, const double *, int);                   \
    template void launch_knn<T>(hipStream_t, int, const ProblemDev *, const MapDev<T> *, const T *, int *, T *,           \
                                const ChainDev<T> &, int, int, int, int *, int2 *, T *, int *, int, const int *, T *, int, void *, int, int); \
    template void launch_knn_med<T>(hipStream_t, ProblemDev *, const MapDev<T> *, const T *, int *, T *,                  \
                                    const ChainDev<T> &, int *, const int2 *, T *, int *, int *, int, int, T *);          \
    template void launch_knn_slow<T>(hipStream_t, ProblemDev *, const MapDev<T> *, const T *, int *, T *,                 \
                                     const ChainDev<T> &, const int *, const int2 *, const T *, const int *, int, T *);   \
    template void launch_trim_select<T>(hipStream_t, ProblemDev *, const T *, const ChainDev<T> &, int, int, int, const int *, int *, void *, int *, int); \
    template void launch_reduce<T>(hipStream_t, const ProblemDev *, const MapDev<T> *, const T *, const T *, const int *, const T *, \
                                   double *, int, int, const int *, const ChainDev<T> &);                                 \
    template int launch_knn_topk<T>(hipStream_t, const ProblemDev *, const MapDev<T> *, const T *, int *, T *, const ChainDev<T> &, int, int, const int *); \
    template void launch_solve<T>(hipStream_t, ProblemDev *, const double *, const ChainDev<T> &, int *, int, int,        \
                                  const int *, int *, int *, int *);                                                      \
    template void launch_cov<T>(hipStream_t, const ProblemDev *, const MapDev<T> *, const T *, const T *, const int *, const T *, \
                                double *, double *, int, int, const ChainDev<T> &);                                       \
    template void launch_trim_raw<T>(hipStream_t, const T *, int, T, T, T *, T *);                                           \
    template void launch_robust_raw<T>(hipStream_t, const T *, int, const RobustDev<T> &, T *, T *, T *);                 \
    template void launch_robust_scale<T>(hipStream_t, ProblemDev *, const T *, T *, const ChainDev<T> &, int, int, const int *, int *, void *, int, int); \
    template void launch_error_stats<T>(hipStream_t, const MapDev<T> *, int, const int *, const T *, int, const int *,    \
                                        const T *, int, int, const T[3], double *, double *, int);                        \
    template void launch_filter_cloud<T>(hipStream_t, const T *, int, int, const T *, int, int, int, const int *, const double *,   \
                                         const double *, int, int, int *, int *, int *, T *, T *, int *, int *, int, const AqScratch *); \
    template void launch_axis_quantile<T>(hipStream_t, const T *, int, int, int, const int *, T, const AqScratch &);         \
    template void launch_slot_of<T>(hipStream_t, const typename Vec4<T>::type *, int, int, int *);                       \
    template void launch_gd_max<T>(hipStream_t, ProblemDev *, const MapDev<T> *, const int *, int, int, const int *);     \
    template void launch_map_values<T>(hipStream_t, const typename Vec4<T>::type *, int, int, const T *, int, T *, int *); \
    template void launch_borrow_order<T>(hipStream_t, const ProblemDev *, const SrcDesc *, const int *, const int *, const typename Vec4<T>::type *, int, int, int, const SeedSegs &, \
                                         const int *, int, T *, int *, int *);                                            \
    template int launch_surface_normals<T>(hipStream_t, const MapDev<T> *, int, int, int, T, T, T *, int, T *, int *, T *); \
    template int launch_surface_normals_ext<T>(hipStream_t, const MapDev<T> *, int, int, int, T, T, T *, int, T *, int *, T *, T *, const NormalsExtOut<T> &); \
    template void launch_smooth_normals<T>(hipStream_t, const T *, int, const int *, long long, long long, int, int, const int *, T *, int, int *); \
    template void launch_unpermute<T>(hipStream_t, const MapDev<T> *, int, const int *, const int *, const T *, int, int, \
                                      int *, T *);

INSTANTIATE(float)
INSTANTIATE(double)
