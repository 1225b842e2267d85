// kernels.hpp -- launch entry points of kernels.hip (host callable).
#pragma once
#include "device_types.hpp"
#include "pgslam_amd/octree_host.hpp"
#ifdef __HIPCC__
#define PGSLAM_ELIP_HD __host__ __device__
#endif
#include "pgslam_amd/elipsoids_host.hpp"
#ifdef __HIPCC__
#define PGSLAM_CHAIN_HD __host__ __device__
#endif
#include "pgicp_sensor_chain.h"
#include "pgslam_amd/sensor_chain_host.hpp"
#include "pgicp_descriptor_filters.h"
#include "pgslam_amd/descriptor_filters_host.hpp"

namespace pgicp {

template <typename T>
void launch_centroid_bbox_batch(hipStream_t st, const BuildDesc<T> *descs, int n, int max_m, unsigned long long *stats);
template <typename T>
void launch_grid_build_batch(hipStream_t st, const BuildDesc<T> *descs, int n, long long tot_m, long long tot_b, long long tot_s,
                             int max_m, int max_cells, int max_bins, int max_nsc, int max_blocks, int kx_all4, int *fkey, int *bins_a, int *block_sums,
                             int *cell_start, int *cell_start_f, int *bins_b, int *arrival, unsigned long long *words,
                             typename Vec4<T>::type *cpts, typename Vec4<T>::type *cnrm,
                             typename Vec4<T>::type *pts, typename Vec4<T>::type *nrm_out,
                             int *slot_of, int *sc_count, int *near, int *sc_dist, int *sc_wit, unsigned *occ, long long tot_o, float *sc_ext, float *ptsf,
                             uint4 *sw, int *ostart, int *flag_scratch, int *rank_scratch);
template <typename T>
void launch_query_sort(hipStream_t st, const ProblemDev *probs, const SrcDesc *src, const MapDev<T> *maps, typename Vec4<T>::type *rd_pre, T *rd_sorted,
                       int *qkey, unsigned long long *qtmp, int *order, int *counts, int *block_sums, int *qstart, int P,
                       int max_n, int max_rows, int bin_shift, typename Vec4<T>::type *nrm_pre, T *nrm_sorted);
template <typename T>
int launch_knn_topk(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot, T *d2,
                    const ChainDev<T> &ch, int P, int max_n, const int *active);
template <typename T>
void launch_transform(hipStream_t st, const T *in, int in_stride, T *out, int out_stride, int n, const double *T16,
                      int rotate_only);
template <typename T>
void launch_knn(hipStream_t st, int matcher, const ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot,
                T *d2, const ChainDev<T> &ch, int P, int max_n, int use_seed, int *slow_count, int2 *slow_list, T *slow_lb,
                int *slow_ring, int fast_rings, const int *active, T *none_r, int n_problems, void *queue_buf, int clear_queue_counters,
                int table_kinds);
size_t knn_queue_bytes(int n_problems, int max_n, size_t elem);
template <typename T>
void launch_knn_med(hipStream_t st, ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot, T *d2,
                    const ChainDev<T> &ch, int *slow_count, const int2 *slow_list, T *slow_lb, int *slow_ring, int *slow2_idx,
                    int med_rings, int use_seed, T *none_r);
template <typename T>
void launch_knn_slow(hipStream_t st, ProblemDev *probs, const MapDev<T> *maps, const T *rd, int *slot, T *d2,
                     const ChainDev<T> &ch, const int *slow_count, const int2 *slow_list, const T *slow_lb,
                     const int *slow2_idx, int exact_all, T *none_r);
template <typename T>
void launch_trim_select(hipStream_t st, ProblemDev *probs, const T *d2, const ChainDev<T> &ch, int P, int max_n, int second,
                        const int *active, int *tables, void *keys, int *seg_count, int guess);
size_t trim_select_table_bytes(int P);
int sel_fallbacks_read(int reset);
int knn_stats_read(unsigned long long out[56], int reset);
int knn_phase_read(unsigned long long out[48], int reset);   // diagnostics build only: wave cycles per phase of the fast kernel
int knn_xcc_report(int use_seed, int reset);                 // diagnostics build (-DPGICP_XCC_STATS) only: the fast kernel's launches per XCC
int knn_dump_setup(long long total, int passes);              // diagnostics build only: per-query candidate dump
int knn_dump_read(unsigned *cnt, float *d2, long long n);
int knn_trace_set(int sorted_index);                       // diagnostics build only   // diagnostics build (-DPGICP_KNN_STATS) only
void launch_reopen(hipStream_t st, ProblemDev *probs, int P);
void launch_compact_active(hipStream_t st, const ProblemDev *probs, int P, int *active, int *host_flag, int *stamp_counter,
                           int *queue_counters);
template <typename T>
int launch_surface_normals(hipStream_t st, const MapDev<T> *maps, int map, int m, int knn, T max_dist, T eps_rank, T *out_nrm,
                           int out_stride, T *out_eig, int *out_ids, T *out_d2);
int reduce_blocks(int max_n);
struct SeedSegs { int n; int src[17]; int dst[16]; };      // pgicp_partial_chain_seeded: the two maps as concatenations of keyframe clouds
template <typename T>
void launch_borrow_order(hipStream_t st, const ProblemDev *probs, const SrcDesc *src, const int *order_a, const int *slot_a, const typename Vec4<T>::type *pts_a,
                         int first_a, int m_a, int n, const SeedSegs &sg, const int *slot_of_b, int m_b, T *rd_sorted, int *order_b, int *slot_b);
void launch_batch_setup(hipStream_t st, int *active, int P, int *z0, long long n0, int *z1, long long n1, int *z2, long long n2, int *z3, long long n3);
size_t knn_queue_counter_words(int n_problems);      // the segmented queue counters at the head of the matcher's queue buffer
void launch_invert_order(hipStream_t st, const ProblemDev *probs, const int *order, int *scan_pos, int P, int max_n);
template <typename T>
void launch_reduce(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd_pre, const T *rd_nrm, const int *slot,
                   const T *d2, double *partials, int P, int max_n, const int *active, const ChainDev<T> &ch);
template <typename T>
void launch_solve(hipStream_t st, ProblemDev *probs, const double *partials, const ChainDev<T> &ch, int *n_done, int P,
                  int max_n, const int *active, int *single_host_flag, int *single_stamp, int *single_queue_counters);
template <typename T>
void launch_cov(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd_pre, const T *rd_nrm, const int *slot,
                const T *d2, double *partials, double *out, int P, int max_n, const ChainDev<T> &ch);
void launch_sum_partials(hipStream_t st, const double *partials, int max_blocks, int nt, const ProblemDev *probs,
                         int nb_uniform, double *out, int P);
// SimpleSensorNoise descriptor and the sensor-noise getOverlap() over the last error elements (k_noise.inc, include/pgicp_noise.h)
template <typename T>
void launch_simple_sensor_noise(hipStream_t st, const T *xyz, int stride, int n, int sensor_type, T min_r, T angle, T cst, T gain, T *out);
template <typename T>
void launch_noise_stage(hipStream_t st, const T *src, int stride, int n, T *dst, int *flag);
template <typename T>
void launch_noise_overlap(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd_pre, const T *rd_nrm, const int *slot, const T *d2,
                          const int *order, const T *noise, const long long *noise_off, T *dist, double *partials, double *out, int *count,
                          int P, int max_pairs, const ChainDev<T> &ch);
// KDTreeVarDistMatcher's per-point radii (k_vardist.inc, include/pgicp_vardist.h): staging a device row; the cut of the matcher's
// exact pairs into a second pair of arrays; the uncapped next pass after a quantile selection over cut distances
template <typename T>
void launch_vardist_stage(hipStream_t st, const T *src, int stride, int n, T *dst, int *flag);
template <typename T>
void launch_vardist_cut(hipStream_t st, const ProblemDev *probs, const int *active, int n_active, int max_pairs, const int *slot, const T *d2,
                        const int *order, const T *radii, const long long *radii_off, int *slot_cut, T *d2_cut);
void launch_vardist_reset(hipStream_t st, ProblemDev *probs, const int *active, int n_active);
void launch_robust_open(hipStream_t st, ProblemDev *probs, const int *active, int n_active);
void launch_gd_open(hipStream_t st, ProblemDev *probs, const int *active, int n_active);
template <typename T>
void launch_gd_max(hipStream_t st, ProblemDev *probs, const MapDev<T> *maps, const int *slot, int n_active, int max_pairs, const int *active);
template <typename T>
void launch_map_values(hipStream_t st, const typename Vec4<T>::type *pts, int first, int m, const T *values, int stride, T *out, int *flags);
template <typename T>
void launch_robust_raw(hipStream_t st, const T *d2, int n, const RobustDev<T> &rb, T *dev, T *stat, T *w);
template <typename T>
void launch_robust_scale(hipStream_t st, ProblemDev *probs, const T *d2, T *dev, const ChainDev<T> &ch, int n_active, int max_pairs,
                         const int *active, int *tables, void *keys, int phase, int part);
template <typename T>
void launch_var_trim(hipStream_t st, ProblemDev *probs, const T *d2, const int *active, int n_active, void *keys_a, void *keys_b,
                     double min_ratio, double max_ratio, double lambda);
template <typename T>
void launch_trim_raw(hipStream_t st, const T *d2, int n, T ratio, T scale, T *limit_nf, T *w);
// MaxQuantileOnAxis (k_axisquantile.inc): what a selection leaves on the device (limit: T's bits; count: the points it ranked), and
// its scratch -- the bin table with the candidate list's cursor, the result, one key (T's width) per point
struct AqResult { unsigned long long limit_bits; int k, below, count, pad_; };
struct AqScratch { int *table; AqResult *result; void *keys; };
size_t axis_quantile_scratch_bytes(int n, size_t elem);
AqScratch axis_quantile_scratch(void *base, int n, size_t elem);
// the selection over the points of [0, n) with keep[i] != 0 (keep == null: all of them); n >= 1; no host step inside
template <typename T>
void launch_axis_quantile(hipStream_t st, const T *feat, int stride, int dim, int n, const int *keep, T ratio, const AqScratch &w);
template <typename T>
void launch_filter_cloud(hipStream_t st, const T *feat, int fstride, int frows, const T *desc, int drows, int n, int n_filters,
                         const int *types, const double *params, const double *T16, int rot0, int rot1, int *keep, int *pos,
                         int *block_sums, T *out_feat, T *out_desc, int *kept_idx, int *dropped = nullptr, int dropped_cap = 0,
                         const AqScratch *aq = nullptr);
template <typename T>
void launch_slot_of(hipStream_t st, const typename Vec4<T>::type *pts, int first, int m, int *slot_of);
template <typename T>
void launch_error_stats(hipStream_t st, const MapDev<T> *maps, int map, const int *slot_of, const T *rd, int stride,
                        const int *ids, const T *w, int n, int knn, const T mean[3], double *partials, double *out, int minimizer);
template <typename T>
void launch_unpermute(hipStream_t st, const MapDev<T> *maps, int map, const int *order, const int *slot, const T *d2, int n, int knn,
                      int *ids_out, T *d2_out);

// The exclusive scan (launch_exclusive_scan, k_build.inc): elements per block (1024 threads x 4), and the ints of block sums a
// scan of `len` elements needs -- one per block
constexpr int kScanChunk = 4096;
inline size_t scan_scratch_ints(size_t len) { return (len + kScanChunk - 1) / kScanChunk; }

// Carves a buffer into arrays aligned to 256 bytes.  With a null base it only measures: a layout names every array once and is
// run twice, to size the buffer and then to point into it.  (!want: the space is kept, the caller gets no pointer to it)
struct Carve {
    char *p;
    size_t used = 0;
    explicit Carve(void *base = nullptr) : p((char *)base) {}
    template <class U> U *take(size_t count, bool want = true)
    {
        U *r = p && want ? (U *)(p + used) : nullptr;
        used += (sizeof(U) * count + 255) & ~(size_t)255;
        return r;
    }
};

// pgicp_sampling_surface_normal_*: the device scratch of one call; counters (4 ints, device): [0] boxes made, [1] boxes fused,
// [2] a coordinate is not finite, [3] points kept
constexpr int kSsnMaxKnn = 1024;        // (one thread fuses a box: its loops are sequential, nothing is sized by knn)
template <typename T>
struct SsnSeg {
    int first, count, cut, pad;
    T lo[3], hi[3];
};
struct SsnBox { int first, count, axis; };   // axis 3: the identity order (a root of at most knn points)
struct SsnScratch {
    void *keys[2];
    int *lst[2], *flag[2], *scan, *bsum, *seg_of[2], *side;
    void *seg[2], *boxes;
    int *keep, *box_of;
    void *bnrm, *bmean;
    int *pos;
};
template <typename T>
SsnScratch ssn_scratch(Carve &cv, int n)
{
    const size_t n1 = (size_t)n + 1, n3 = 3 * (size_t)n + 1;
    SsnScratch w;
    for (auto &k : w.keys) k = cv.take<T>(n3);
    for (auto &l : w.lst) l = cv.take<int>(n3);
    for (auto &f : w.flag) f = cv.take<int>(n3);
    w.scan = cv.take<int>(n3);
    w.bsum = cv.take<int>(scan_scratch_ints(n3));
    for (auto &s : w.seg_of) s = cv.take<int>(n1);
    w.side = cv.take<int>(n1);
    for (auto &s : w.seg) s = cv.take<SsnSeg<T>>(n1 + 2);
    w.boxes = cv.take<SsnBox>(n1);
    w.keep = cv.take<int>(n1);
    w.box_of = cv.take<int>(n1);
    w.bnrm = cv.take<T>(3 * n1);
    w.bmean = cv.take<T>(3 * n1);
    w.pos = cv.take<int>(n1);
    return w;
}
// The per-box rows beside SsnScratch's bnrm / bmean that the three entries of the box filters offer (pgicp_sampling_surface_normal_*
// none, include/pgicp_ssn_ext.h the first three, include/pgicp_elipsoids.h all), as a set of bits.  (kBoxMean is an output only: it
// is gathered from bmean and has no scratch of its own.)
enum : unsigned { kBoxEig = 1, kBoxVec = 2, kBoxDens = 4, kBoxCov = 8, kBoxWeight = 16, kBoxShape = 32, kBoxMean = 64, kBoxRowsExt = 7, kBoxRowsAll = 127 };
// BoxRows: what k_box_fuse<T, true> writes per box slot -- 3, 9, 1, 9, 1 and 3 values; a null pointer is a row nobody asked for, and
// is not written.  BoxOut: what k_box_compact<T, true> copies to each kept point (every output may be null; `means` is gathered
// from bmean).
template <typename T>
struct BoxRows { T *beig, *bvec, *bdens, *bcov, *bweight, *bshape; };
template <typename T>
struct BoxOut {
    T *eig, *eigvec, *dens, *cov, *weights, *means, *shapes;
    BoxRows<T> box;
    bool any() const { return eig || eigvec || dens || cov || weights || means || shapes; }
};
// carved after the call's SsnScratch from the same buffer: room for every row the entry offers, whether asked for or not, so the
// buffer's size depends on the entry and n alone; a pointer only for a row that is asked for
template <typename T>
BoxRows<T> box_scratch(Carve &cv, int n, unsigned offered, const BoxOut<T> &want)
{
    const size_t n1 = (size_t)n + 1;
    auto row = [&](unsigned bit, size_t width, const T *asked) { return offered & bit ? cv.take<T>(width * n1, asked != nullptr) : nullptr; };
    BoxRows<T> b;
    b.beig = row(kBoxEig, 3, want.eig);
    b.bvec = row(kBoxVec, 9, want.eigvec);
    b.bdens = row(kBoxDens, 1, want.dens);
    b.bcov = row(kBoxCov, 9, want.cov);
    b.bweight = row(kBoxWeight, 1, want.weights);
    b.bshape = row(kBoxShape, 3, want.shapes);
    return b;
}
// The one schedule of the three entries (k_ssn.inc): the tree, then the boxes fused and the kept points compacted.  With no row
// asked for in x the lean instantiations run.  min_planarity 0: no planarity drop (the SamplingSurfaceNormal entries).
template <typename T>
int launch_box_filter(hipStream_t st, const T *X, int xs, int n, int knn, int method, T ratio, T max_box, T min_planarity, unsigned long long seed,
                      const T *desc, int drows, int average, const SsnScratch &w, T *out_xyz, int os, T *out_nrm, int ns, T *out_desc,
                      int *kept_idx, int *counters, const BoxOut<T> &x);

// The stable LSD radix sort of (64-bit key, index) pairs (k_pairsort.inc), 8 bits a pass, that VoxelGrid, OctreeGrid and NormalSpace
// share: the two ping-pong buffers, the [digit][tile] counts and their scan, and the scan's block sums.  `other_scan`: the longest
// scan the caller itself runs through bsum (0: none) -- bsum is sized for the longer of that and the sort's own
constexpr int kPairTile = 4096;      // pairs per block of the radix passes: 256 threads x 16 rounds
struct PairSort {
    unsigned long long *key[2];
    int *idx[2], *hist, *hoff, *bsum;
};
inline PairSort pair_sort_scratch(Carve &cv, int n, size_t other_scan)
{
    const size_t n1 = (size_t)n + 1, tiles = ((size_t)n + kPairTile - 1) / kPairTile + 1, hist = 256 * tiles + 1;
    PairSort w;
    for (auto &k : w.key) k = cv.take<unsigned long long>(n1);
    for (auto &i : w.idx) i = cv.take<int>(n1);
    w.hist = cv.take<int>(hist);
    w.hoff = cv.take<int>(hist);
    w.bsum = cv.take<int>(scan_scratch_ints(hist > other_scan ? hist : other_scan));
    return w;
}
// sorts the pairs in key[cur] / idx[cur] over the low `bits` bits of the key; returns which of key[] / idx[] holds the result
int launch_pair_sort(hipStream_t st, const PairSort &w, int n, int bits, int cur);

// pgicp_voxel_grid_*: the bounds and counters of a call (device), the grid the host derives from the bounds, and the scratch
struct VoxStat {
    unsigned long long lo[3], hi[3];    // order-preserving keys of each axis's min / max (-0.0 as +0.0)
    int bad, kept, nheavy, pad;         // a coordinate is not finite; voxels (points out); voxels summed by k_vox_heavy
};
template <typename T>
struct VoxGrid {
    T v[3], minB[3];
    unsigned long long nd[3];           // numDiv of each axis (< 2^31)
};
struct VoxScratch {
    PairSort sort;
    int *head, *hs, *start, *first, *vox_of, *pos;
    int2 *heavy;
};
inline VoxScratch vox_scratch(Carve &cv, int n)
{
    const size_t n1 = (size_t)n + 1;
    VoxScratch w;
    w.sort = pair_sort_scratch(cv, n, n1);           // bsum also serves the scans of head and first: n + 1 elements
    w.head = cv.take<int>(n1);
    w.hs = cv.take<int>(n1);
    w.start = cv.take<int>(n1 + 1);
    w.first = cv.take<int>(n1);
    w.vox_of = cv.take<int>(n1);
    w.pos = cv.take<int>(n1);
    w.heavy = cv.take<int2>(n1);
    return w;
}
template <typename T>
void launch_voxel_bounds(hipStream_t st, const T *X, int xs, int n, VoxStat *stat);
template <typename T>
void launch_voxel_grid(hipStream_t st, const T *X, int xs, int n, const VoxGrid<T> &g, int bits, int centroid, const T *desc, int drows, int average,
                       const VoxScratch &w, T *out_xyz, int os, T *out_desc, int *kept_idx, int *out_count, VoxStat *stat);

// include/pgicp_octree.h (k_octree.inc): OctreeGridDataPointsFilter.  The root the host derives from the bounds (VoxStat, from
// launch_voxel_bounds) and the levels of a path code: octree_host.hpp's Root<T>, as make_root returns it; the scratch of a call: the
// pair sort's, then per sorted position the leaf depth, the head flag and its scan, per leaf the start and depth, and the heavy
// leaves' list
template <typename T>
using OctRoot = pgslam_amd::octree::Root<T>;
struct OctScratch {
    PairSort sort;
    int *depth, *head, *hs, *start, *ldepth, *heavy;
};
inline OctScratch oct_scratch(Carve &cv, int n)
{
    const size_t n1 = (size_t)n + 1;
    OctScratch w;
    w.sort = pair_sort_scratch(cv, n, n1);           // bsum also serves the scan of head: n + 1 elements
    w.depth = cv.take<int>(n1);
    w.head = cv.take<int>(n1);
    w.hs = cv.take<int>(n1);
    w.start = cv.take<int>(n1 + 1);
    w.ldepth = cv.take<int>(n1);
    w.heavy = cv.take<int>(n1);
    return w;
}
template <typename T>
void launch_octree_grid(hipStream_t st, const T *X, int xs, int n, const OctRoot<T> &R, int max_pts, int method, unsigned long long seed, const T *desc,
                        int drows, const OctScratch &w, T *out_xyz, int os, T *out_desc, int *kept_idx, int *out_count, int *out_depth, VoxStat *stat);

// include/pgicp_density.h (k_density.inc): the densities as an epilogue of the normals kernel, and MaxDensityDataPointsFilter
struct DensStat {
    unsigned long long key;         // the largest order-preserving key of a non-NaN density (0: none seen)
    int saturated;                  // #{dens[i] == last}
    int first_nan;                  // dens[0] is a NaN: `last` is a NaN, nothing equals it
};
// the scratch of the filter -- keep (n + 1), pos (n + 1), the scan's block sums -- then, for a call that runs the normals kernel
// first (`rows`), that kernel's rows in input order
template <typename T>
struct DensWork { int *keep, *pos, *bsum; T *nrm, *eig, *dens; };
template <typename T>
DensWork<T> dens_scratch(Carve &cv, int n, bool rows)
{
    DensWork<T> w{};
    w.keep = cv.take<int>((size_t)n + 1);
    w.pos = cv.take<int>((size_t)n + 1);
    w.bsum = cv.take<int>(scan_scratch_ints(n));
    if (rows) {
        w.nrm = cv.take<T>(3 * (size_t)n);
        w.eig = cv.take<T>(3 * (size_t)n);
        w.dens = cv.take<T>((size_t)n);
    }
    return w;
}
template <typename T>
int launch_surface_densities(hipStream_t st, const MapDev<T> *maps, int map, int m, int knn, T max_dist, T eps_rank, T *out_nrm,
                             int out_stride, T *out_eig, T *out_dens);

// include/pgicp_normals_ext.h (k_normals.inc): what k_surface_normals<.., EXT> writes besides; every pointer may be null.  eigvec
// (9 a point), mean_dist (1) and matched (knn, the ids as values of T) go to the point's original index.  raw, self and nb are
// for the smoothing pass and travel together (raw null: none of them): in SLOT order the raw normal (3), the original index, and
// the neighbours' slots relative to the map's first, transposed -- entry j of slot s at nb[j * m + s], -1 = none
template <typename T>
struct NormalsExtOut { T *eigvec, *mean_dist, *matched, *raw; int *self, *nb; };
template <typename T>
int launch_surface_normals_ext(hipStream_t st, const MapDev<T> *maps, int map, int m, int knn, T max_dist, T eps_rank, T *out_nrm,
                               int out_stride, T *out_eig, int *out_ids, T *out_d2, T *out_dens, const NormalsExtOut<T> &x);
// out[out_of ? out_of[i] : i] = the smoothed normal of row i; entry j of row i at nb[i * rs + j * cs]; *bad (zeroed here; may be
// null) is raised by an id outside [-1, n)
template <typename T>
void launch_smooth_normals(hipStream_t st, const T *nrm, int ns, const int *nb, long long rs, long long cs, int knn, int n, const int *out_of,
                           T *out, int os, int *bad);
template <typename T>
void launch_max_density(hipStream_t st, const T *dens, int n, T max_density, unsigned long long seed, DensStat *stat, int *keep, int *pos,
                        int *block_sums);
template <typename T>
void launch_density_compact(hipStream_t st, int n, const int *keep, const int *pos, const T *xyz, int stride, const T *desc, int drows,
                            const T *nrm, const T *eig, const T *dens, T *out_xyz, T *out_desc, T *out_nrm, int out_nstride, T *out_eig,
                            T *out_dens, int *kept_idx);

// include/pgicp_sensor_chain.h, include/pgicp_descriptor_filters.h (k_sensor_chain.inc): the stages behind the normals kernel.
// ChainSeg: the parameters of every stage type that appears at most once, and the stages of ONE segment, in list order; a
// CutAtDescriptor stage drops, so it ends its segment and `cut` is that one's.  ChainCut: the row a cut reads (PGICP_CHAIN_ROW_*;
// desc_row with ROW_DESC), its direction and threshold.  ChainRows: the scratch of a call -- the rows at the points' input indices
// (null: not made), the survivors' densities by rank, and per dropping stage (kChainMaxDrops: Shadow, MaxDensity, four cuts) the
// flags, their scan (n + 1 each; pos[n] = the number kept) and the survivor list.  ChainOut: where the kept points' rows go (null:
// not asked for)
constexpr int kChainMaxDrops = 2 + PGICP_CHAIN_EXT_MAX_CUTS;
template <typename T>
struct ChainCut { int row, desc_row, larger; T thr; };
template <typename T>
struct ChainSeg {
    int n_ops, op[PGICP_CHAIN_EXT_MAX_STAGES];
    T c[3]; int toward; T sin_eps; T max_density; unsigned long long seed;
    pgslam_amd::sensor_chain::NoiseModel<T> noise;
    int keep_uns, keep_str;
    ChainCut<T> cut;
};
template <typename T>
struct ChainRows {
    T *nrm, *eig, *dens, *obs, *noise, *inc, *sph, *uns, *str, *dens_rank;
    int *keep[kChainMaxDrops], *pos[kChainMaxDrops], *idx[kChainMaxDrops], *bsum;
};
template <typename T>
struct ChainOut { T *xyz, *desc, *nrm; int nstride; T *eig, *dens, *obs, *noise, *inc, *sph, *uns, *str; int *kept_idx; };
// which rows a call makes
struct ChainHas { bool nrm, eig, dens, obs, noise, inc, sph, uns, str, max_density; };
template <typename T>
ChainRows<T> chain_scratch(Carve &cv, int n, const ChainHas &h, int drops)
{
    ChainRows<T> w{};
    w.nrm = cv.take<T>(3 * (size_t)n, h.nrm);
    w.eig = cv.take<T>(3 * (size_t)n, h.eig);
    w.dens = cv.take<T>((size_t)n, h.dens);
    w.obs = cv.take<T>(3 * (size_t)n, h.obs);
    w.noise = cv.take<T>((size_t)n, h.noise);
    // (placed only when made: a list of the older stages carves what it always carved)
    if (h.inc) w.inc = cv.take<T>((size_t)n);
    if (h.sph) w.sph = cv.take<T>((size_t)n);
    if (h.uns) w.uns = cv.take<T>((size_t)n);
    if (h.str) w.str = cv.take<T>((size_t)n);
    w.dens_rank = cv.take<T>((size_t)n, h.max_density);
    for (int k = 0; k < drops; k++) {
        w.keep[k] = cv.take<int>((size_t)n + 1);
        w.pos[k] = cv.take<int>((size_t)n + 1);
        w.idx[k] = cv.take<int>((size_t)n);
    }
    w.bsum = cv.take<int>(scan_scratch_ints(n));
    return w;
}
// cuts[k]: the cut of stage k (read only where types[k] is CUT_AT_DESCRIPTOR)
template <typename T>
void launch_sensor_chain(hipStream_t st, const T *xyz, int stride, int n, const T *desc, int drows, int n_stages, const int *types,
                         const ChainSeg<T> &params, const ChainCut<T> *cuts, const ChainRows<T> &w, DensStat *stat, const ChainOut<T> &out,
                         const int **last_pos);

// include/pgicp_covsample.h (k_covsample.inc): CovarianceSamplingDataPointsFilter
constexpr int kCovBlocks = 1024;        // the most blocks of a frame reduction: one row of partials each
constexpr int kCovSums = 21;            // the distinct sums of C; no reduction carries more values
struct CovStat {
    double r1[10];                      // pass 1 folded: coordinate sums, #non-finite points, -min and max of each axis
    double nsum;                        // pass 2 folded: the sum of the norms
    double sums[kCovSums];              // pass 3 folded: C's upper triangle, row-major
    double c[3], L, inv;                // the centre, L and T(1) / L: values of T
    unsigned long long prefix[6];       // the selection: each list's key prefix so far, in the end the threshold key
    int rank[6];                        // ... and the rank sought among the keys under the prefix, in the end the ties to take
    int cursor[6];                      // candidates emitted into each list
    int bad, pad;                       // an input of the values pass is not finite
};
template <typename T>
struct CovFrameDev { T c[3], inv, X[36]; };     // X column-major
struct CovScratch {
    double *part;                       // kCovBlocks rows of at most kCovSums doubles
    void *v;                            // n x 6 values of T
    int *hist, *eq, *pos, *bsum;        // passes x 6 x 256 counts; the tie flags [list][point], their scan, its block sums
    int *cand_idx; void *cand_v;        // [list][m] indices, [list][m][6] values of T
    int *picks;                         // m
};
// n points, m = min(n, nbSample) candidates a list
template <typename T>
CovScratch cov_scratch(Carve &cv, int n, int m)
{
    const size_t n6 = 6 * (size_t)n;
    CovScratch w;
    w.part = cv.take<double>((size_t)kCovBlocks * kCovSums);
    w.v = cv.take<T>(n6);
    w.hist = cv.take<int>(sizeof(T) * 6 * 256);
    w.eq = cv.take<int>(n6 + 1);
    w.pos = cv.take<int>(n6 + 2);
    w.bsum = cv.take<int>(scan_scratch_ints(n6));
    w.cand_idx = cv.take<int>(6 * (size_t)m);
    w.cand_v = cv.take<T>(36 * (size_t)m);
    w.picks = cv.take<int>((size_t)m);
    return w;
}
// passes 1-3 and their folds: CovStat's r1, nsum, sums, c, L, inv (stat zeroed by the caller)
template <typename T>
void launch_cov_frame(hipStream_t st, const T *X, int xs, const T *N, int ns, int n, int torque_norm, const CovScratch &w, CovStat *stat);
// pass 4: the values, each list's first m entries (unordered) into cand_idx / cand_v
template <typename T>
void launch_cov_select(hipStream_t st, const T *X, int xs, const T *N, int ns, int n, const CovFrameDev<T> &F, int m, const CovScratch &w, CovStat *stat);
// the gather of CovarianceSampling (pass 5) and NormalSpace: out[j] = in[i] with i = pos[j], or -- sidx and skey set, both or
// neither -- i = sidx[pos[j]] and bucket_out[j] = skey[pos[j]] >> 24; pos == null: the identity, bucket -1.  Any output may be null
template <typename T>
void launch_gather_rows(hipStream_t st, const int *pos, const unsigned long long *skey, const int *sidx, int m, int n, const T *X, int xs, const T *N,
                        int ns, const T *desc, int drows, T *out_xyz, int os, T *out_nrm, int ons, T *out_desc, int *kept_idx, int *bucket_out);

// include/pgicp_normalspace.h (k_normalspace.inc): NormalSpaceDataPointsFilter.  The scratch of a call: the pair sort's, the
// buckets' counts with the not-finite flag behind them (counts[nb_bucket]), and the picks' sorted positions
constexpr int kNsLdsBuckets = 8192;     // a grid of at most this many buckets is counted in LDS, block by block
struct NsGrid { double epsilon; int n_phi, n_theta, nb_bucket; };
struct NsScratch {
    PairSort sort;
    int *counts, *pos;
};
// n points, m = min(n, nbSample) picks
inline NsScratch ns_scratch(Carve &cv, int n, int m, int nb_bucket)
{
    NsScratch w;
    w.sort = pair_sort_scratch(cv, n, 0);            // nothing of length n is scanned: bsum serves the sort alone
    w.counts = cv.take<int>((size_t)nb_bucket + 1);
    w.pos = cv.take<int>((size_t)m);
    return w;
}
// the keys, the counts (zeroed here) and the stable sort of (key, index); returns which of key[] / idx[] holds the sorted order
template <typename T>
int launch_ns_sort(hipStream_t st, const T *N, int ns, int n, const NsGrid &g, unsigned long long seed, const NsScratch &w);

}  // namespace pgicp
