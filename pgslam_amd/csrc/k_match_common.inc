// k_match_common.inc -- part of kernels.hip through k_match.inc (one translation unit, inside namespace pgicp): the matcher's candidate record, diagnostics macros, distance / slab / row helpers, the per-lane ring walk (grid_nn)

// ---------------------------------------------------------------------------
// matcher: exact nearest neighbour on the cell-sorted map
// ---------------------------------------------------------------------------
template <typename T>
struct Best {
    T d2;
    int idx;
    int slot;
#ifdef PGICP_KNN_STATS
    int cnt = 0;      // diagnostics build only: candidates evaluated
#endif
};

#ifdef PGICP_KNN_STATS
__device__ int g_trace_i = -1;          // diagnostics: sorted index of one query of problem 0 to narrate
#define KNN_TRACE(prob_, i_, ...) do { if ((prob_) == 0 && (i_) == g_trace_i) printf(__VA_ARGS__); } while (0)
__device__ unsigned long long g_knn_stats[56];   // [16..31] histogram of own-row, [32..47] of flat-walk candidates per lane (log2 bins)
// per-query dump (tools/studies/balance_study.py): candidates by phase of every pass, and the distance a pass started with
__device__ unsigned *g_cnt_dump = nullptr;
__device__ float *g_d2_dump = nullptr;
__device__ long long g_dump_total = 0;
__device__ int g_dump_passes = 0;
#define KNN_STAT_WAVE_ADD(slot_, v_)                                                              \
    do {                                                                                          \
        long long s_ = (v_);                                                                      \
        for (int o_ = 32; o_ > 0; o_ >>= 1) s_ += __shfl_xor(s_, o_, 64);                          \
        if ((threadIdx.x & 63) == 0) atomicAdd(&g_knn_stats[slot_], (unsigned long long)s_);      \
    } while (0)
#define KNN_STAT_WAVE_MAX(slot_, v_)                                                              \
    do {                                                                                          \
        int s_ = (v_);                                                                            \
        for (int o_ = 32; o_ > 0; o_ >>= 1) s_ = max(s_, __shfl_xor(s_, o_, 64));                  \
        if ((threadIdx.x & 63) == 0) atomicAdd(&g_knn_stats[slot_], (unsigned long long)s_);      \
    } while (0)
#else
#define KNN_TRACE(prob_, i_, ...) do { } while (0)
#endif

#ifdef PGICP_PHASE_STATS
// Diagnostics build of its own (-DPGICP_PHASE_STATS, without the candidate counters: their contended atomics distort
// every timing): wave time per phase of the fast kernel ([0] unseeded pass, [1] seeded passes).  Shader cycles between
// marks are kept in registers and added once, when the wave leaves the kernel, by its first active lane, into one of 64
// copies of the table; slot 15 counts the waves.
__device__ unsigned long long g_phase[64][3][16];
__device__ unsigned long long g_ball[16];       // grid_nn_ball: waves, open lanes, trips, rows with a range, items, evaluations, on-the-spot scans, lanes' rows   // [2]: the wave-per-query kernel
__device__ unsigned long long g_slow_worst[16];      // the slowest entry of the wave-per-query kernel: [0] cycles, [1..6] by phase, [8..] counts
#define PHASE_BEGIN() long long ph_t = (long long)__builtin_amdgcn_s_memtime(); unsigned ph_d[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define PHASE_MARK(k_) do { const long long t_ = (long long)__builtin_amdgcn_s_memtime(); ph_d[k_] += (unsigned)(t_ - ph_t); ph_t = t_; } while (0)
#define PHASE_FLUSH() do {                                                                                                  \
        if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) {                                              \
            unsigned long long *dst_ = g_phase[blockIdx.x & 63][use_seed ? 1 : 0];                                          \
            for (int k_ = 0; k_ < 8; ++k_) atomicAdd(dst_ + k_, (unsigned long long)ph_d[k_]);                              \
            atomicAdd(dst_ + 15, 1ULL);                                                                                     \
        } } while (0)
#define SPH_BEGIN() long long sph_t = (long long)__builtin_amdgcn_s_memtime(); const long long sph_t0 = sph_t; long long sph_e0 = sph_t; unsigned sph_emax = 0; unsigned sph_d[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned sph_n = 0
#define SPH_MARK(k_) do { const long long t_ = (long long)__builtin_amdgcn_s_memtime(); sph_d[k_] += (unsigned)(t_ - sph_t); sph_t = t_; } while (0)
// a timer mark means something only once the loads before it have ARRIVED: a never-true test on their values makes the wave wait
#define SPH_ARRIVED(cond_) do { if (cond_) printf("x"); } while (0)
#define SPH_FLUSH() do {                                                                                                    \
        if ((threadIdx.x & 63) == 0) {                                                                                      \
            unsigned long long *dst_ = g_phase[blockIdx.x & 63][2];                                                         \
            for (int k_ = 0; k_ < 8; ++k_) atomicAdd(dst_ + k_, (unsigned long long)sph_d[k_]);                              \
            atomicAdd(dst_ + 14, (unsigned long long)sph_n); atomicAdd(dst_ + 15, 1ULL);                                    \
            atomicMax(dst_ + 12, (unsigned long long)(sph_t - sph_t0)); atomicMax(dst_ + 13, (unsigned long long)sph_emax);  \
        } } while (0)
#else
#define PHASE_BEGIN() do { } while (0)
#define PHASE_MARK(k_) do { } while (0)
#define PHASE_FLUSH() do { } while (0)
#define SPH_BEGIN() do { } while (0)
#define SPH_ARRIVED(cond_) do { } while (0)
#define SPH_MARK(k_) do { } while (0)
#define SPH_FLUSH() do { } while (0)
#endif

#ifdef PGICP_XCC_STATS
// Diagnostics build of its own (-DPGICP_XCC_STATS alone: the phase marks above make a wave wait for its loads at every mark
// and triple the kernel's time): how a launch of the fast kernel spreads over the XCDs.  Per hardware XCC (the XCC_ID
// register) and launch: [0] ~(first start of a wave), [1] last end, [2] wave time summed, [3] waves, [8 + c] waves of the
// blocks with blockIdx.x & 7 == c -- on the constant 100 MHz clock all XCDs share.  Two clock reads and six atomics without
// a return value per wave, into one of kXccCopies 128-byte lines of the wave's XCC (each touched by that XCD's L2 only; with
// ONE line per XCC the 150 000 atomics of a seeded launch's short waves queued on it for 1.2 ms and levelled the XCDs' end
// times); zero means "nothing yet" everywhere (hence the complement in [0]).  Read with PGICP_PHASE_EACH_PASS=1
// (knn_xcc_report), digested by tools/xcd_balance.py.
constexpr int kXccCopies = 32;
__device__ unsigned long long g_xcc[8][kXccCopies][16];
#define XCC_BEGIN() const unsigned long long xc_t0 = wall_clock64()
#define XCC_END() do {                                                                                                      \
        if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) {                                              \
            const unsigned long long xc_t1 = wall_clock64();                                                                \
            unsigned long long *xc_ = g_xcc[__builtin_amdgcn_s_getreg(20 | (3 << 11)) & 7u][(blockIdx.x >> 3) % kXccCopies];   /* hwreg(HW_REG_XCC_ID, 0, 4) */ \
            atomicMax(xc_ + 0, ~xc_t0); atomicMax(xc_ + 1, xc_t1); atomicAdd(xc_ + 2, xc_t1 - xc_t0); atomicAdd(xc_ + 3, 1ULL); \
            atomicAdd(xc_ + 8 + (blockIdx.x & 7u), 1ULL);                                                                   \
        } } while (0)
#else
#define XCC_BEGIN() do { } while (0)
#define XCC_END() do { } while (0)
#endif

// (squared distance, index) as one 64-bit key: distances are >= +0, so the order of the keys is the matcher's order --
// smaller distance first, then smaller index
__device__ __forceinline__ unsigned long long item_key(float d2, int idx)
{
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)idx;
}
#ifndef PGICP_KEY_CMP
#define PGICP_KEY_CMP 1          // measured: fast matcher 8.58 -> 8.31 ms per step
#endif
template <typename T>
__device__ __forceinline__ bool cand_better(T d, int idx, const Best<T> &best)
{
#if PGICP_KEY_CMP
    if constexpr (sizeof(T) == 4) return item_key(d, idx) < item_key(best.d2, best.idx);     // one 64-bit compare for three
#endif
    return (d < best.d2) | ((d == best.d2) & (idx < best.idx));
}

// Squared distance of a record to the query, (dx dx + dy dy) + dz dz in that order, every operation rounded by itself (no
// fused multiply-add: the arithmetic contract of kernels.hip).  T = float: dx, dy and their squares as ONE two-wide
// subtraction and ONE two-wide multiplication (v_pk_add_f32 with the negate modifier, v_pk_mul_f32) on the record's own
// (x, y) register pair -- the same operations on the same values, bit for bit, six instructions for eight.  (Left to itself
// the compiler's SLP pass pairs x with z, which costs a register move per record to bring them together.)  Round 6,
// profiles/r06_experiments/fast_matcher_variants.txt: SQ_INSTS_VALU of the fast matcher -4.1 %, its launches -1.2 %.
#ifndef PGICP_PK_XY
#define PGICP_PK_XY 1
#endif
typedef float pk2f __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ T dist2_rec(const typename Vec4<T>::type v, T qx, T qy, T qz)
{
#if PGICP_PK_XY
    if constexpr (sizeof(T) == 4) {
        const pk2f q = {qx, qy}, c = {v.x, v.y};
        const pk2f e = q - c;
        const pk2f s = e * e;
        const float dz = qz - v.z;
        return (s.x + s.y) + dz * dz;
    }
#endif
    const T dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
    return (dx * dx + dy * dy) + dz * dz;
}

template <typename T>
__device__ __forceinline__ void eval_point(const typename Vec4<T>::type v, int s, T qx, T qy, T qz, Best<T> &best)
{
    const T d = dist2_rec<T>(v, qx, qy, qz);
    const int idx = Bits<T>::unpack_idx(v.w);
    // selects, not branches: the update is rare and the loop bodies must stay straight-line
    const bool better = cand_better<T>(d, idx, best);
    best.d2 = better ? d : best.d2;
    best.idx = better ? idx : best.idx;
    best.slot = better ? s : best.slot;
#ifdef PGICP_KNN_STATS
    best.cnt++;
#endif
}

// predicated form for straight-line loops (field-wise selects: a struct-typed ?: goes through scratch)
template <typename T>
__device__ __forceinline__ void eval_point_if(bool on, const typename Vec4<T>::type v, int s, T qx, T qy, T qz, Best<T> &best)
{
    const T d = dist2_rec<T>(v, qx, qy, qz);
    const int idx = Bits<T>::unpack_idx(v.w);
    const bool better = on & cand_better<T>(d, idx, best);
    best.d2 = better ? d : best.d2;
    best.idx = better ? idx : best.idx;
    best.slot = better ? s : best.slot;
#ifdef PGICP_KNN_STATS
    best.cnt += on ? 1 : 0;
#endif
}

template <typename T>
__device__ __forceinline__ void scan_range(const typename Vec4<T>::type *__restrict__ pts_generic, int a, int b, T qx, T qy,
                                           T qz, Best<T> &best)
{
    const auto *pts = pts_generic;
    int s = a;
    for (; s + 4 <= b; s += 4) {                 // four independent loads in flight
        const auto v0 = load_rec<T, 0>(pts, s), v1 = load_rec<T, 1>(pts, s), v2 = load_rec<T, 2>(pts, s), v3 = load_rec<T, 3>(pts, s);
        eval_point<T>(v0, s, qx, qy, qz, best);
        eval_point<T>(v1, s + 1, qx, qy, qz, best);
        eval_point<T>(v2, s + 2, qx, qy, qz, best);
        eval_point<T>(v3, s + 3, qx, qy, qz, best);
    }
    if (s < b) {                                 // the 1..3 left over: one round trip, not one each
        // (the two records after the range's last are read, not used: no index arithmetic, and the point array is never
        // the last thing in its block -- the cell tables follow it, pgicp_api.cpp map_create_batch)
        const auto v0 = load_rec<T, 0>(pts, s), v1 = load_rec<T, 1>(pts, s), v2 = load_rec<T, 2>(pts, s);
        eval_point<T>(v0, s, qx, qy, qz, best);
        eval_point_if<T>(s + 1 < b, v1, s + 1, qx, qy, qz, best);
        eval_point_if<T>(s + 2 < b, v2, s + 2, qx, qy, qz, best);
    }
}

// distance from coordinate offset u (= x - origin) to the slab of cell c
template <typename T>
__device__ __forceinline__ T slab_dist(T u, int c, T h)
{
    const T lo = (T)c * h - u;          // > 0 when the query is below the slab
    const T hi = u - (T)(c + 1) * h;    // > 0 when above
    return fmax((T)0, fmax(lo, hi));
}

// BOOKKEEPING IN FLOAT (round 5, the double fast matcher).  Which rows, cells and x-windows a query looks at is decided from
// slab distances, radii and floors; none of that has to be exact, only CONSERVATIVE: every such test already carries the
// grid's margin (0.02 h, ~2 mm) on the safe side against the rounding of its own arithmetic.  With double clouds the same
// tests in float stay inside a margin widened per query by the float rounding at its offsets (bk_margin, below: at hundreds of
// metres ~1e-4 m on top of the grid's ~2e-3), bounds taken from a double best are rounded UP (bk_up) -- so the
// double instantiation keeps its candidates, its bests and every value it hands on (queue bounds, empty radii) in double and
// does the walking in float: half of its 2 641 VALU instructions were double bookkeeping (square roots of ~15 instructions,
// floors, conversions, 64-bit compares) and its 118 registers allowed 4 waves per SIMD.  The query's OWN cell numbers stay
// computed in T: the medium and the wave-per-query path continue a queued query ring by ring from that cell.
typedef float BK;
__device__ __forceinline__ float bk_up(float v) { return v; }
__device__ __forceinline__ float bk_up(double v)
{
    const float f = (float)v;                                   // (>= +0; +inf stays +inf, a double beyond FLT_MAX becomes +inf)
    return ((double)f < v) ? __uint_as_float(__float_as_uint(f) + 1u) : f;
}
__device__ __forceinline__ float bk_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
// The margin the float walk of a DOUBLE cloud works with, per query: the grid's margin plus what float rounding can cost at
// this query's offsets -- 2^-24 of max(|u|, the grid's extent) per operation, a handful of operations per test, so 2^-21 of it.
// Nothing assumes "hundreds of metres" any more: a reading kilometres from the map (a bad initial pose with maxDist = inf), or a
// map kilometres wide, only widens its own tests (tests/test_gpu_edge_cases.py: test_double_query_far_from_the_map...).
// A larger margin is the safe side of every test that uses it (smaller slab bounds, wider x-windows, smaller ring guarantees).
// Float clouds: the walk's values ARE the cloud's type, the margin is the grid's, as it always was.
template <typename T>
__device__ __forceinline__ BK bk_margin(const GridDesc<T> &g, T ux, T uy, T uz)
{
    if constexpr (sizeof(T) == 4) return g.margin;
    else {
        const T ext = g.h * (T)max(g.nx, max(g.ny, g.nz));
        const T u = fmax(fmax(fabs(ux), fabs(uy)), fmax(fabs(uz), ext));
        return bk_up(g.margin + u * (T)4.76837158203125e-07);       // 2^-21
    }
}

// Is any cell of [xa, xb] in row `row_id` occupied?  One or two words of MapDev::occ (a bit per cell; ranges here span a
// few cells), which is small enough to stay cached while the cell tables of a large sparse map are not.
template <typename T>
__device__ __forceinline__ bool row_any(const MapDev<T> &M, int row_id, int xa, int xb)
{
    const int c_lo = row_id * M.g.nx + xa, c_hi = row_id * M.g.nx + xb;
    const auto *occ = as_global(M.occ);
    const int w_lo = c_lo >> 5, w_hi = c_hi >> 5;
    unsigned first = occ[w_lo] & (0xFFFFFFFFu << (c_lo & 31));
    if (w_lo == w_hi) return (first & (0xFFFFFFFFu >> (31 - (c_hi & 31)))) != 0u;
    unsigned any = first | (occ[w_hi] & (0xFFFFFFFFu >> (31 - (c_hi & 31))));
    for (int w = w_lo + 1; w < w_hi; ++w) any |= occ[w];
    return any != 0u;
}

// One (y,z) row of cells, restricted to cells [xa,xb]: the cells of a row are contiguous in memory, and only those within
// sqrt(best - rowdist^2) of the query in x can hold a better point.  [xa, xb] are cells of the search structure; the range actually
// read is cut down on the kx-times finer x grid the points are ordered by (every candidate is a 16-byte gather: fewer is faster);
// the hardware square root, pushed outward (the rounded one costs some eighteen instructions more, and a range a hair too wide only
// reads candidates that cannot win).  The range arithmetic is float for double clouds too (BK, above).
template <typename T, int TK = 2>
__device__ __forceinline__ void scan_row_bk(const MapDev<T> &M, int row_id, int xa, int xb, BK ux, BK lb2, BK inv_hx, BK margin, T qx, T qy,
                                            T qz, Best<T> &best)
{
    const int kx = M.kx, nxf = M.g.nx * kx;
    int fa = xa * kx, fb = xb * kx + kx - 1;
    int a = 0, b = 0;
    const BK bound = bk_up(best.d2);
    bool any = true;
    if (bound < Bits<BK>::inf()) {
        const BK rad = bk_sqrt(fmax(bound - lb2, (BK)0)) * (BK)1.000001 + margin;
        fa = max(fa, clamp_cell<BK>(ux - rad, inv_hx, nxf));
        fb = min(fb, clamp_cell<BK>(ux + rad, inv_hx, nxf));
        any = fa <= fb;
    }
    if (any) { const int row = nxf * row_id; tab_range_k<TK, T>(M, row + fa, row + fb + 1, a, b); }
    scan_range<T>(M.pts, a, b, qx, qy, qz, best);
}

// guaranteed radius after ring r: every cell outside Chebyshev ring r around c0 is at
// least this far from the query (+inf when the grid is exhausted); margin NOT yet removed
template <typename T>
__device__ __forceinline__ T ring_guarantee(const GridDesc<T> &g, T ux, T uy, T uz, int c0x, int c0y, int c0z, int r)
{
    T gr = Bits<T>::inf();
    if (c0x - r - 1 >= 0) gr = fmin(gr, slab_dist(ux, c0x - r - 1, g.h));
    if (c0x + r + 1 <= g.nx - 1) gr = fmin(gr, slab_dist(ux, c0x + r + 1, g.h));
    if (c0y - r - 1 >= 0) gr = fmin(gr, slab_dist(uy, c0y - r - 1, g.h));
    if (c0y + r + 1 <= g.ny - 1) gr = fmin(gr, slab_dist(uy, c0y + r + 1, g.h));
    if (c0z - r - 1 >= 0) gr = fmin(gr, slab_dist(uz, c0z - r - 1, g.h));
    if (c0z + r + 1 <= g.nz - 1) gr = fmin(gr, slab_dist(uz, c0z + r + 1, g.h));
    return gr;
}

// Exact NN by expanding Chebyshev rings of cells around the query's (clamped)
// cell, starting at ring r_start (rings below it were already examined).  A row
// is skipped when its slab distance already exceeds the best candidate; the
// search is RESOLVED when every unexamined cell is provably farther than the
// best candidate or than maxDist.  At most ring max_rings is walked here (the
// per-lane path); returns false if unresolved, with the last guaranteed radius.
template <typename T>
__device__ __forceinline__ bool grid_nn(const MapDev<T> &M, T qx, T qy, T qz, T max_dist, int r_start, int max_rings,
                                        T stop_d2, Best<T> &best, T &gr_out, int &r_next)
{
    r_next = r_start;
    const GridDesc<T> g = M.g;
    const int c0x = clamp_cell<T>(qx - g.ox, g.inv_h, g.nx), c0y = clamp_cell<T>(qy - g.oy, g.inv_h, g.ny),
              c0z = clamp_cell<T>(qz - g.oz, g.inv_h, g.nz);
    // (the walk's arithmetic in float -- BK, above: conservative tests inside the grid's margin, double or float clouds alike)
    GridDesc<BK> gb;
    gb.h = (BK)g.h; gb.inv_h = (BK)g.inv_h; gb.margin = bk_margin<T>(g, qx - g.ox, qy - g.oy, qz - g.oz); gb.nx = g.nx; gb.ny = g.ny; gb.nz = g.nz;
    const BK ux = (BK)(qx - g.ox), uy = (BK)(qy - g.oy), uz = (BK)(qz - g.oz);
    const BK bmax = (BK)max_dist, bstop = (BK)stop_d2, inv_hx = gb.inv_h * (BK)M.kx;
    gr_out = (T)0;
    if (r_start > 0) {
        BK gr = ring_guarantee<BK>(gb, ux, uy, uz, c0x, c0y, c0z, r_start - 1);
        if (!(gr < Bits<BK>::inf())) return true;
        gr = gr - gb.margin;
        gr_out = (T)gr;
        if (gr > (BK)0 && (bk_up(best.d2) < gr * gr || gr > bmax)) return true;
        if (gr > (BK)0 && gr * gr > bstop) return false;               // far enough for the caller: leave it unresolved
    }
    for (int r = r_start; r <= max_rings; ++r) {
        const int z0 = max(c0z - r, 0), z1 = min(c0z + r, g.nz - 1);
        const int y0 = max(c0y - r, 0), y1 = min(c0y + r, g.ny - 1);
        const int xa = max(c0x - r, 0), xb = min(c0x + r, g.nx - 1);
        for (int z = z0; z <= z1; ++z) {
            const BK lz = fmax(slab_dist<BK>(uz, z, gb.h) - gb.margin, (BK)0);
            const bool zo = (z - c0z == r) || (c0z - z == r);
            for (int y = y0; y <= y1; ++y) {
                const BK ly = fmax(slab_dist<BK>(uy, y, gb.h) - gb.margin, (BK)0);
                const BK lb2 = ly * ly + lz * lz;
                if (lb2 > bk_up(best.d2)) continue;
                const int row = y + g.ny * z;
                if (zo || (y - c0y == r) || (c0y - y == r)) {
                    scan_row_bk<T>(M, row, xa, xb, ux, lb2, inv_hx, gb.margin, qx, qy, qz, best);
                } else {                         // inner row of the shell: only its two end cells are new
                    if (c0x - r >= 0) scan_row_bk<T>(M, row, c0x - r, c0x - r, ux, lb2, inv_hx, gb.margin, qx, qy, qz, best);
                    if (c0x + r <= g.nx - 1) scan_row_bk<T>(M, row, c0x + r, c0x + r, ux, lb2, inv_hx, gb.margin, qx, qy, qz, best);
                }
            }
        }
        BK gr = ring_guarantee<BK>(gb, ux, uy, uz, c0x, c0y, c0z, r);
        if (!(gr < Bits<BK>::inf())) return true;                       // grid exhausted
        gr = gr - gb.margin;
        gr_out = (T)gr;
        if (gr > (BK)0 && (bk_up(best.d2) < gr * gr || gr > bmax)) return true;
        r_next = r + 1;
        if (gr > (BK)0 && gr * gr > bstop) return false;
    }
    return false;
}

