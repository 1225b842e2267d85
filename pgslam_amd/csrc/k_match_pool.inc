// k_match_pool.inc -- part of kernels.hip through k_match.inc (one translation unit, inside namespace pgicp): the item pool -- neighbour rows and the ball walk of a whole wave through LDS items (float, double, double with a float prefilter)
// ---- item walk (T = float): one lane per RANGE ---------------------------------------------------------------
// A wave's candidate ranges are short (four to a dozen records) and unevenly spread over its queries; walked by their
// owners, lane by lane, the wave makes as many trips as its busiest lane while most lanes idle -- and a wave's VALU time is
// what the fast kernel is made of (94 % VALU-busy in the unseeded pass, 68-83 % later; DESIGN.md section 4).  So ranges
// are cut into ITEMS of at most kItemChunk records, pooled in LDS, and lane L evaluates item L, L + 64, ...: every lane is
// busy and a round is kItemChunk / 4 quad-loads deep.  An owner's best travels as a 64-bit key (distance bits, index) --
// the order of the keys IS the matcher's order (smaller distance, then smaller index) -- folded with an LDS atomic
// minimum; the lane whose key won a round also leaves its slot.  Same candidates, same rule: bit-identical results.
#ifndef PGICP_ITEMS_MAX
#define PGICP_ITEMS_MAX 512
#endif
#ifndef PGICP_ITEM_CHUNK
#define PGICP_ITEM_CHUNK 8
#endif
constexpr int kItemsMax = PGICP_ITEMS_MAX;
// records per item, by scalar type.  Float: 4 since round 5 (one quad-load deep; with the ball walk's two rows per trip: headline 11 240-11 294 ->
// 11 472-11 488 scans/s, loop closing unchanged; round 3 had measured 8 as the optimum of the kernel as it was then).  Double: 8 (4: 7 650 -> 7 419).
#ifndef PGICP_ITEM_CHUNK_F
#define PGICP_ITEM_CHUNK_F 4
#endif
#ifndef PGICP_ITEM_CHUNK_D
#define PGICP_ITEM_CHUNK_D PGICP_ITEM_CHUNK
#endif
template <typename T> struct ItemChunk { static constexpr int n = sizeof(T) == 4 ? PGICP_ITEM_CHUNK_F : PGICP_ITEM_CHUNK_D;
                                         static constexpr int shift = n == 4 ? 2 : n == 8 ? 3 : n == 16 ? 4 : n == 32 ? 5 : -1; };
constexpr int kItemShift = ItemChunk<float>::shift;
static_assert(ItemChunk<float>::shift > 0 && ItemChunk<double>::shift > 0, "the item size is a power of two (items are counted with shifts: a division by a run-time size costs ~30 VALU instructions)");

// Evaluates items [0, total) of the wave's pool and folds the results into the owners' keys; ends with the LDS in order.
// (A workgroup is one wave: the barriers only order its own LDS traffic.)
__device__ __forceinline__ void item_rounds(const float4 *__restrict__ pts, const int2 *items, int total, const float *sq,
                                            unsigned long long *skey, int *sslot, int lane, int chunk)
{
    __syncthreads();
    for (int b0 = 0; b0 < total; b0 += 64) {
        const int it = b0 + lane;
        const int2 I = it < total ? items[it] : make_int2(0, 0);
        const int owner = I.y & 63, len = I.y >> 6;          // (an item of up to 2^25 records: whatever a range holds)
        const float ox = sq[owner], oy = sq[64 + owner], oz = sq[128 + owner];
        // lb.slot counts from the item's first record here (the offsets of an unrolled trip are then constants)
        Best<float> lb;
        lb.d2 = Bits<float>::inf(); lb.idx = 0x7FFFFFFF; lb.slot = -1;
        const float4 *rp = pts + I.x;
        auto trip = [&](const int t4) {
            const bool p0 = t4 < len, p1 = t4 + 1 < len, p2 = t4 + 2 < len, p3 = t4 + 3 < len;
            // Loads under the execution mask: a lane without a record issues no request at all.  (Measured against it, same
            // box: redirecting such a lane to record 0 of the array 8.09 ms per step, to record 0 of its item 8.31, reading
            // on past the item's end -- fewest instructions -- 8.12-8.25; masked 7.95.  Requests of idle lanes cost
            // address-path time; LLVM does not speculate loads, so the nest below stays a nest.)
            float4 c0, c1, c2, c3;
            if (p0) {
                c0 = load_rec<float, 0>(rp, t4);
                if (p1) {
                    c1 = load_rec<float, 1>(rp, t4);
                    if (p2) {
                        c2 = load_rec<float, 2>(rp, t4);
                        if (p3) c3 = load_rec<float, 3>(rp, t4);
                    }
                }
            }
            eval_point_if<float>(p0, c0, t4, ox, oy, oz, lb);
            eval_point_if<float>(p1, c1, t4 + 1, ox, oy, oz, lb);
            eval_point_if<float>(p2, c2, t4 + 2, ox, oy, oz, lb);
            eval_point_if<float>(p3, c3, t4 + 3, ox, oy, oz, lb);
        };
        trip(0);                                             // (unrolled: the slot offsets of a trip are constants)
        if (__any(4 < len)) trip(4);
#pragma unroll 1
        for (int t4 = 8; t4 < chunk; t4 += 4) {              // larger items: a crowded wave only
            if (!__any(t4 < len)) break;
            trip(t4);
        }
        lb.slot = lb.slot < 0 ? -1 : I.x + lb.slot;
        const unsigned long long key = item_key(lb.d2, lb.idx);
        const bool cand = lb.slot >= 0 && key < skey[owner];
        if (cand) atomicMin(&skey[owner], key);
        __syncthreads();
        if (cand && skey[owner] == key) sslot[owner] = lb.slot;     // the round's winner (a key belongs to one point)
        __syncthreads();
    }
}

// Inclusive wave scan of a small count (items per lane) and its total.
__device__ __forceinline__ int wave_incl_scan(int v, int lane, int &total)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
    total = __shfl(v, 63, 64);
    return v;
}

// N ranges per lane (registers), through the wave's pool: items of kItemChunk records -- larger ones when the wave's
// ranges would overflow the pool (one item per range always fits: N x 64 <= kItemsMax) -- evaluated by item_rounds and
// folded into `best`.  Every lane of the wave calls this together.
template <int N>
__device__ __forceinline__ void walk_ranges(const float4 *__restrict__ pts, const int (&ra)[N], const int (&rb)[N], int lane, float qx, float qy,
                                            float qz, Best<float> &best, int2 *items, float *sq, unsigned long long *skey, int *sslot)
{
    static_assert(N * 64 <= kItemsMax, "one item per range must fit");
    int sh = kItemShift, mine, total, incl;
    for (;;) {
        mine = 0;
#pragma unroll
        for (int t = 0; t < N; ++t) mine += (max(rb[t] - ra[t], 0) + (1 << sh) - 1) >> sh;
        incl = wave_incl_scan(mine, lane, total);
        if (total <= kItemsMax) break;                      // (wave-uniform)
        ++sh;
    }
    if (total == 0) return;
    const int chunk = 1 << sh;
    int w = incl - mine;
    // (a range's first item straight-line, the rest -- rare after the first passes -- behind a wave-uniform branch: the
    // plain loop came back from the compiler vectorised, with a pre-header, an epilogue and a remainder per range)
#pragma unroll
    for (int t = 0; t < N; ++t) {
        const int len = rb[t] - ra[t];
        if (len > 0) { items[w] = make_int2(ra[t], (min(len, chunk) << 6) | lane); ++w; }
        if (__any(len > chunk)) {
#pragma clang loop vectorize(disable) unroll(disable)
            for (int a = ra[t] + chunk; a < rb[t]; a += chunk) { items[w] = make_int2(a, (min(rb[t] - a, chunk) << 6) | lane); ++w; }
        }
    }
    const unsigned long long key0 = item_key(best.d2, best.idx);
    sq[lane] = qx; sq[64 + lane] = qy; sq[128 + lane] = qz;
    skey[lane] = key0;
    sslot[lane] = best.slot;
    item_rounds(pts, items, total, sq, skey, sslot, lane, chunk);
    const unsigned long long kf = skey[lane];
    if (kf != key0) { best.d2 = __uint_as_float((unsigned)(kf >> 32)); best.idx = (int)(unsigned)kf; best.slot = sslot[lane]; }
}

// ---- the same item walk for T = double (round 4) -------------------------------------------------------------------
// A double's (squared distance, index) does not fit one 64-bit key: the owners' bests travel as TWO words -- the distance's
// bit pattern (>= +0: its order is the value's) and the index -- and a round folds its results in two steps: atomicMin on
// the distance words; the owners whose distance got smaller reset their index word; atomicMin on the index words among the
// items that hold the round's smallest distance; the item that holds both writes its slot.  Same candidates, same order
// (smaller distance, then smaller index) as the per-lane walk: bit-identical results.
__device__ __forceinline__ void item_rounds_d(const double4 *__restrict__ pts, const int2 *items, int total, const double *sq,
                                              unsigned long long *skey, int *sidx, int *sslot, int lane, int chunk)
{
    __syncthreads();
    for (int b0 = 0; b0 < total; b0 += 64) {
        const int it = b0 + lane;
        const int2 I = it < total ? items[it] : make_int2(0, 0);
        const int owner = I.y & 63, len = I.y >> 6;
        const double ox = sq[owner], oy = sq[64 + owner], oz = sq[128 + owner];
        const unsigned long long key_before = skey[owner];
        const int idx_before = sidx[owner];
        Best<double> lb;
        lb.d2 = Bits<double>::inf(); lb.idx = 0x7FFFFFFF; lb.slot = -1;
        const double4 *rp = pts + I.x;
        auto trip = [&](const int t4) {
            const bool p0 = t4 < len, p1 = t4 + 1 < len, p2 = t4 + 2 < len, p3 = t4 + 3 < len;
            double4 c0, c1, c2, c3;
            if (p0) {
                c0 = load_rec<double, 0>(rp, t4);
                if (p1) {
                    c1 = load_rec<double, 1>(rp, t4);
                    if (p2) {
                        c2 = load_rec<double, 2>(rp, t4);
                        if (p3) c3 = load_rec<double, 3>(rp, t4);
                    }
                }
            }
            eval_point_if<double>(p0, c0, t4, ox, oy, oz, lb);
            eval_point_if<double>(p1, c1, t4 + 1, ox, oy, oz, lb);
            eval_point_if<double>(p2, c2, t4 + 2, ox, oy, oz, lb);
            eval_point_if<double>(p3, c3, t4 + 3, ox, oy, oz, lb);
        };
        trip(0);
        if (__any(4 < len)) trip(4);
#pragma unroll 1
        for (int t4 = 8; t4 < chunk; t4 += 4) {
            if (!__any(t4 < len)) break;
            trip(t4);
        }
        lb.slot = lb.slot < 0 ? -1 : I.x + lb.slot;
        const unsigned long long key = (unsigned long long)__double_as_longlong(lb.d2);
        const bool cand = lb.slot >= 0 && (key < key_before || (key == key_before && lb.idx < idx_before));
        if (cand) atomicMin(&skey[owner], key);
        __syncthreads();
        const bool tied = cand && skey[owner] == key;                // holds the round's smallest distance of its owner
        if (tied && key < key_before) sidx[owner] = 0x7FFFFFFF;      // (the old index belonged to a larger distance)
        __syncthreads();
        if (tied) atomicMin(&sidx[owner], lb.idx);
        __syncthreads();
        if (tied && sidx[owner] == lb.idx) sslot[owner] = lb.slot;   // (distance, index) belongs to one point
        __syncthreads();
    }
}

// ---- the same with a FLOAT PREFILTER (round 5) -------------------------------------------------------------------
// A double record is two load instructions, a float one is one, and the fast matcher's time follows its load instructions
// (223 M wave loads per step against float's 130 M, 1.78 x the time).  Double maps carry a float mirror of their points
// (MapDev::ptsf); an item's records are read THERE first: float distances d_f, the owner's smallest folded with one 32-bit LDS
// atomic (fb: it starts from the owner's best so far, rounded up), and only a candidate that may still be the double minimum
// is read again as a double record and evaluated exactly -- with the same (distance, index) order as ever.
//   |d_f - d| <= E(d_f) = 4 sqrt(d_f) U + 16 U^2 + 2^-20 d_f,   U = 2^-22 max(|q|_inf, the map's largest |coordinate|):
// both points are rounded to float (2^-24 of their magnitude each), the differences and the three-term sum are rounded
// again.  The true minimum d* is at most d(c) for the candidate c that set fb, so d* <= fb + E(fb); a candidate with
// d_f - E(d_f) > fb + E(fb) cannot reach it.  The test used is weaker (d_f - 2.5 E(d_f) <= fb, E increasing, d_f >= fb), as one
// threshold per item: a superset survives, typically one or two records per owner and round.  Items longer than eight records (a pool that
// overflowed its slots: rare) take item_rounds_d.
// (What holds the threshold: tests/test_gpu_tie_scenes.py::test_double_pairs_against_the_float_prefilter -- pairs that float32 orders wrongly half the time, on both branches.)
__device__ __forceinline__ void item_rounds_dp(const double4 *__restrict__ pts, const float4 *__restrict__ ptsf, const int2 *items, int total,
                                               const double *sq, unsigned long long *skey, int *sidx, int *sslot, unsigned *fb, const float *su,
                                               int lane, int chunk)
{
    if (chunk > 8) { item_rounds_d(pts, items, total, sq, skey, sidx, sslot, lane, chunk); return; }
    __syncthreads();
    for (int b0 = 0; b0 < total; b0 += 64) {
        const int it = b0 + lane;
        const int2 I = it < total ? items[it] : make_int2(0, 0);
        const int owner = I.y & 63, len = I.y >> 6;
        const double ox = sq[owner], oy = sq[64 + owner], oz = sq[128 + owner];
        const float fx = (float)ox, fy = (float)oy, fz = (float)oz;
        const unsigned long long key_before = skey[owner];
        const int idx_before = sidx[owner];
        const float4 *rf = ptsf + I.x;
        float df[8];
        float lmin = Bits<float>::inf();
        auto ftrip = [&](const int t4) {
            const bool p0 = t4 < len, p1 = t4 + 1 < len, p2 = t4 + 2 < len, p3 = t4 + 3 < len;
            float4 c0, c1, c2, c3;                                 // (loads under the execution mask, nested as in item_rounds)
            if (p0) {
                c0 = load_rec<float, 0>(rf, t4);
                if (p1) {
                    c1 = load_rec<float, 1>(rf, t4);
                    if (p2) {
                        c2 = load_rec<float, 2>(rf, t4);
                        if (p3) c3 = load_rec<float, 3>(rf, t4);
                    }
                }
            }
            auto dist = [&](const bool on, const float4 c) {
                const float dx = fx - c.x, dy = fy - c.y, dz = fz - c.z;
                return on ? (dx * dx + dy * dy) + dz * dz : Bits<float>::inf();
            };
            df[t4] = dist(p0, c0); df[t4 + 1] = dist(p1, c1); df[t4 + 2] = dist(p2, c2); df[t4 + 3] = dist(p3, c3);
            lmin = fmin(fmin(lmin, fmin(df[t4], df[t4 + 1])), fmin(df[t4 + 2], df[t4 + 3]));
        };
        ftrip(0);
        if (__any(4 < len)) ftrip(4);
        else { df[4] = df[5] = df[6] = df[7] = Bits<float>::inf(); }
        if (len > 0) atomicMin(&fb[owner], __float_as_uint(lmin));           // (distances are >= +0: the bits order as the values)
        __syncthreads();
        // who may still be the double minimum: d_f - 2.5 E(d_f) <= fb.  With h = 2.5 E (increasing, slope below 1/2 from
        // 100 U^2 on) the largest such d_f is below fb + 2 h(fb), or below 400 U^2 when fb is that small: ONE threshold per item
        const float fmin_o = __uint_as_float(fb[owner]), U = su[owner];
        const float h = ((10.0f * __builtin_amdgcn_sqrtf(fmin_o)) * U + (40.0f * U) * U) + fmin_o * 2.384185791015625e-06f;
        const float thr = fmax(fmin_o + 2.001f * h, (400.0f * U) * U) * 1.000001f;
        unsigned mask = 0u;
#pragma unroll
        for (int t = 0; t < 8; ++t) mask |= (df[t] <= thr) ? 1u << t : 0u;
        mask &= (1u << len) - 1u;           // (a slot past the item's end holds +inf -- and the threshold is +inf while the owner has no bound: maxDist inf)
        Best<double> lb;
        lb.d2 = Bits<double>::inf(); lb.idx = 0x7FFFFFFF; lb.slot = -1;
        const double4 *rp = pts + I.x;
        while (__any(mask != 0u)) {
            const bool on = mask != 0u;
            const int t = on ? __ffs((int)mask) - 1 : 0;
            double4 c;
            if (on) c = load_rec<double>(rp, t);
            eval_point_if<double>(on, c, t, ox, oy, oz, lb);
            mask &= mask - 1u;
        }
        lb.slot = lb.slot < 0 ? -1 : I.x + lb.slot;
        const unsigned long long key = (unsigned long long)__double_as_longlong(lb.d2);
        const bool cand = lb.slot >= 0 && (key < key_before || (key == key_before && lb.idx < idx_before));
        if (cand) atomicMin(&skey[owner], key);
        __syncthreads();
        const bool tied = cand && skey[owner] == key;                // holds the round's smallest distance of its owner
        if (tied && key < key_before) sidx[owner] = 0x7FFFFFFF;      // (the old index belonged to a larger distance)
        __syncthreads();
        if (tied) atomicMin(&sidx[owner], lb.idx);
        __syncthreads();
        if (tied && sidx[owner] == lb.idx) sslot[owner] = lb.slot;   // (distance, index) belongs to one point
        __syncthreads();
    }
}

template <int N>
__device__ __forceinline__ void walk_ranges_d(const double4 *__restrict__ pts, const float4 *__restrict__ ptsf, const int (&ra)[N], const int (&rb)[N], int lane, double qx,
                                              double qy, double qz, Best<double> &best, int2 *items, double *sq, unsigned long long *skey,
                                              int *sidx, int *sslot, unsigned *fb, const float *su)
{
    static_assert(N * 64 <= kItemsMax, "one item per range must fit");
    int sh = ItemChunk<double>::shift, mine, total, incl;
    for (;;) {
        mine = 0;
#pragma unroll
        for (int t = 0; t < N; ++t) mine += (max(rb[t] - ra[t], 0) + (1 << sh) - 1) >> sh;
        incl = wave_incl_scan(mine, lane, total);
        if (total <= kItemsMax) break;
        ++sh;
    }
    if (total == 0) return;
    const int chunk = 1 << sh;
    int w = incl - mine;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        const int len = rb[t] - ra[t];
        if (len > 0) { items[w] = make_int2(ra[t], (min(len, chunk) << 6) | lane); ++w; }
        if (__any(len > chunk)) {
#pragma clang loop vectorize(disable) unroll(disable)
            for (int a = ra[t] + chunk; a < rb[t]; a += chunk) { items[w] = make_int2(a, (min(rb[t] - a, chunk) << 6) | lane); ++w; }
        }
    }
    const unsigned long long key0 = (unsigned long long)__double_as_longlong(best.d2);
    const int idx0 = best.idx;
    sq[lane] = qx; sq[64 + lane] = qy; sq[128 + lane] = qz;
    skey[lane] = key0;
    sidx[lane] = idx0;
    sslot[lane] = best.slot;
    if (ptsf) { fb[lane] = __float_as_uint(bk_up(best.d2)); item_rounds_dp(pts, ptsf, items, total, sq, skey, sidx, sslot, fb, su, lane, chunk); }
    else item_rounds_d(pts, items, total, sq, skey, sidx, sslot, lane, chunk);
    const unsigned long long kf = skey[lane];
    const int xf = sidx[lane];
    if (kf != key0 || xf != idx0) { best.d2 = __longlong_as_double((long long)kf); best.idx = xf; best.slot = sslot[lane]; }
}

// ---- beyond the 27 cells, through the item pool (T = float) ------------------------------------------------------
// What grid_nn does ring by ring and lane by lane, done by the WHOLE WAVE and ball by ball.  A lane that the 27 cells did
// not settle holds a bound (its best candidate, or the search cap): only cells that meet the ball of that radius can
// matter.  So the lane walks the (y, z) rows of the ball's box -- clipped to `max_rings` cells around its own, which is as
// far as the fast kernel goes -- one row per trip of a loop whose trips all lanes make together: the row's x-extent is cut
// with the bound as everywhere else, the part the 27 cells already covered is left out (a row inside their footprint
// brings two side windows), and the point range goes into the wave's item pool; the pool slots come from an LDS counter
// (one ds_add_rtn per range: no wave scan, so it works inside divergent code).  The wave evaluates the pool (item_rounds)
// whenever it is nearly full and at the end; a range that no longer fits is scanned by its owner on the spot.  Walked ring
// by ring (2r + 1)^2 rows per ring and lane were tested -- 74 for rings 2 and 3, most of them pruned at once, which was
// 73 % of a wave's time in the unseeded pass; a ball of 1.5-2 cells touches 16-30 rows.  The bound a row prunes with is
// the lane's best of the last evaluation (grid_nn tightens it row by row): a superset of grid_nn's candidates within the
// same window, the same minimum under the same order -- bit-identical results.  Afterwards everything within `max_rings`
// cells that could matter has been examined: resolved if the bound lies within the guaranteed radius of that ring,
// otherwise the query is left for the queue with that radius as lower bound, like grid_nn's.
// `active`: the lanes that still search; every lane of the wave calls this together.
#ifndef PGICP_RING_POOL
#define PGICP_RING_POOL 1
#endif
#ifndef PGICP_FREE_SKIP
#define PGICP_FREE_SKIP 1
#endif
constexpr int kPoolCap = kItemsMax - 1;           // the ball walk's pool: the last item slot holds its counter (5 632 bytes of LDS per
                                                  // wave: 28 waves fit a CU's 160 KB, 5 648 did not)
#ifndef PGICP_BALL_ROWS
#define PGICP_BALL_ROWS 2          // measured (headline / loop closing / f64): 1 -> 11 094-11 179 / 8 786-8 933 / 7 540-7 561; 2 -> 11 270-11 280 / 8 881-9 006 / 7 682;
#endif                            // 3 -> 11 317 / 9 010 / 7 616; 4 -> 10 994 / 8 890
constexpr int kBallRows = PGICP_BALL_ROWS;        // rows of its box a lane looks up per trip of the ball walk
constexpr int kPoolFlushAt = kPoolCap - 128 * kBallRows;
// (T = double, round 4: the owners' bests as two words -- distance bits in skey, index in sidx -- folded by item_rounds_d)
template <typename T, int TK = 2>
__device__ __forceinline__ bool grid_nn_ball(const MapDev<T> &M, int lane, bool active, T qx, T qy, T qz, T max_dist,
                                             int r_done, int max_rings, T stop_d2, Best<T> &best, T &gr_out, int &r_next,
                                             int2 *items, T *sq, unsigned long long *skey, int *sidx, int *sslot, int *pool_n,
                                             unsigned *fb = nullptr, const float *su = nullptr)
{
    r_next = r_done + 1;
    const GridDesc<T> g = M.g;
    const int c0x = clamp_cell<T>(qx - g.ox, g.inv_h, g.nx), c0y = clamp_cell<T>(qy - g.oy, g.inv_h, g.ny), c0z = clamp_cell<T>(qz - g.oz, g.inv_h, g.nz);
    // the walk's arithmetic in float (BK, this file's head): conservative tests, double or float clouds alike
    GridDesc<BK> gb;
    gb.h = (BK)g.h; gb.inv_h = (BK)g.inv_h; gb.margin = bk_margin<T>(g, qx - g.ox, qy - g.oy, qz - g.oz); gb.nx = g.nx; gb.ny = g.ny; gb.nz = g.nz;
    const BK ux = (BK)(qx - g.ox), uy = (BK)(qy - g.oy), uz = (BK)(qz - g.oz);
    const BK bmax = (BK)max_dist, bstop = (BK)stop_d2;
    BK bbest = bk_up(best.d2);                                               // the best candidate's distance, rounded up
    gr_out = (T)0;
    bool resolved = false, open = active;
    if (open) {                                                              // what the cells examined so far guarantee
        BK gr = ring_guarantee<BK>(gb, ux, uy, uz, c0x, c0y, c0z, r_done);
        if (!(gr < Bits<BK>::inf())) { resolved = true; open = false; }
        else {
            gr = gr - gb.margin;
            gr_out = (T)gr;
            if (gr > (BK)0 && (bbest < gr * gr || gr > bmax)) { resolved = true; open = false; }
            else if (gr > (BK)0 && gr * gr > bstop) open = false;           // far enough for the caller: left unresolved
        }
    }
    if (max_rings <= r_done || !__any(open)) return resolved;
    const typename Vec4<T>::type *pts = M.pts;
    const int kx = M.kx, nxf = g.nx * kx;
    const BK inv_hx = gb.inv_h * (BK)kx;
    const int sy = __builtin_amdgcn_readfirstlane(nxf), sz = __builtin_amdgcn_readfirstlane(nxf * g.ny);
    sq[lane] = qx; sq[64 + lane] = qy; sq[128 + lane] = qz;
    if constexpr (sizeof(T) == 4) skey[lane] = item_key(best.d2, best.idx);
    else { skey[lane] = (unsigned long long)__double_as_longlong(best.d2); sidx[lane] = best.idx; if (fb) fb[lane] = __float_as_uint(bk_up(best.d2)); }
    sslot[lane] = best.slot;
    if (lane == 0) *pool_n = 0;
    __syncthreads();
#ifdef PGICP_PHASE_STATS
    int st_trips = 0, st_items = 0, st_flush = 0;
#endif
    auto push = [&](int a, int b) {
        constexpr int kItemChunk = ItemChunk<T>::n;
        const int n = (b - a + kItemChunk - 1) >> ItemChunk<T>::shift;
        const int w = atomicAdd(pool_n, n);
        if (w + n <= kPoolCap) {
            items[w] = make_int2(a, (min(b - a, kItemChunk) << 6) | lane);
#pragma clang loop vectorize(disable) unroll(disable)
            for (int k = 1; k < n; ++k) items[w + k] = make_int2(a + k * kItemChunk, (min(b - a - k * kItemChunk, kItemChunk) << 6) | lane);
        } else {
            // the pool is full: the slots this lane was given stay empty, and it reads the range itself
#pragma clang loop vectorize(disable) unroll(disable)
            for (int k = w; k < kPoolCap; ++k) items[k] = make_int2(0, lane);
            scan_range<T>(pts, a, b, qx, qy, qz, best);
        }
    };
    auto flush = [&]() {
        __syncthreads();
        const int total = min(__builtin_amdgcn_readfirstlane(*pool_n), kPoolCap);
        if (total > 0) {
#ifdef PGICP_PHASE_STATS
            st_items += total; ++st_flush;
#endif
            if constexpr (sizeof(T) == 4) {
                item_rounds(pts, items, total, sq, skey, sslot, lane, ItemChunk<T>::n);
                const unsigned long long kf = skey[lane];
                if (kf < item_key(best.d2, best.idx)) { best.d2 = __uint_as_float((unsigned)(kf >> 32)); best.idx = (int)(unsigned)kf; best.slot = sslot[lane]; }
            } else {
                // (a range its owner scanned itself -- pool full -- may have improved `best` past what the words hold: the words
                // are folded into `best`, then written back, so that the next flush compares against the owner's true best)
                if (fb && M.ptsf) item_rounds_dp(pts, reinterpret_cast<const float4 *>(M.ptsf), items, total, sq, skey, sidx, sslot, fb, su, lane, ItemChunk<T>::n);
                else item_rounds_d(pts, items, total, sq, skey, sidx, sslot, lane, ItemChunk<T>::n);
                const unsigned long long kf = skey[lane], kb = (unsigned long long)__double_as_longlong(best.d2);
                const int xf = sidx[lane];
                if (kf < kb || (kf == kb && xf < best.idx)) { best.d2 = __longlong_as_double((long long)kf); best.idx = xf; best.slot = sslot[lane]; }
                skey[lane] = (unsigned long long)__double_as_longlong(best.d2); sidx[lane] = best.idx; sslot[lane] = best.slot;
                if (fb) fb[lane] = __float_as_uint(bk_up(best.d2));
            }
            bbest = bk_up(best.d2);
            if (lane == 0) *pool_n = 0;
            __syncthreads();
        }
    };
    // the lane's box of rows, and its windows on the fine x grid (as floats): all of [c0x - max_rings, c0x + max_rings] for
    // a row outside the footprint of the cells already examined, the two parts beside them for a row inside
    const BK rho = bk_sqrt(bbest) * (BK)1.000001 + gb.margin;
    const int ylo = max(c0y - max_rings, clamp_cell<BK>(uy - rho, gb.inv_h, g.ny)), yhi = min(c0y + max_rings, clamp_cell<BK>(uy + rho, gb.inv_h, g.ny));
    const int zlo = max(c0z - max_rings, clamp_cell<BK>(uz - rho, gb.inv_h, g.nz)), zhi = min(c0z + max_rings, clamp_cell<BK>(uz + rho, gb.inv_h, g.nz));
    const BK wl_all = (BK)(max(c0x - max_rings, 0) * kx), wh_all = (BK)(min(c0x + max_rings, g.nx - 1) * kx + kx - 1);
    const BK wh_left = (BK)((c0x - r_done) * kx - 1), wl_right = (BK)((c0x + r_done) * kx + kx);
#ifdef PGICP_PHASE_STATS
    const int st_open = __popcll(__ballot(open));
    int st_rows = open ? (yhi - ylo + 1) * (zhi - zlo + 1) : 0;
    for (int o_ = 32; o_ > 0; o_ >>= 1) st_rows += __shfl_xor(st_rows, o_, 64);
#endif
    int y = ylo, z = zlo;
    int rowb = nxf * (ylo + g.ny * zlo);
    const int wrap = sz - (yhi - ylo + 1) * sy;
    bool walking = open;
#if PGICP_BALL_ROWS > 1
    // several rows per trip: the table look-ups of both (up to eight) are in flight together -- a trip is a dependent round trip to
    // the cell table, and where every problem reads its own map (loop closing) neither pipe is busy while the wave waits for it
    while (__any(walking)) {
        constexpr int NW = 2 * kBallRows;
        int ia[NW], ib[NW];
        bool need[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) { ia[w] = 0; ib[w] = 0; need[w] = false; }
#pragma unroll
        for (int r = 0; r < kBallRows; ++r) {
            if (walking) {
                const BK ly = fmax(slab_dist<BK>(uy, y, gb.h) - gb.margin, (BK)0), lz = fmax(slab_dist<BK>(uz, z, gb.h) - gb.margin, (BK)0);
                const BK lb2 = ly * ly + lz * lz;
                if (!(lb2 > bbest)) {
                    const BK rad = bk_sqrt(fmax(bbest - lb2, (BK)0)) * (BK)1.000001 + gb.margin;
                    const BK flo = floor((ux - rad) * inv_hx), fhi = floor((ux + rad) * inv_hx);
                    const bool inside = abs(y - c0y) <= r_done && abs(z - c0z) <= r_done;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const BK wl = (inside && k == 1) ? wl_right : wl_all, wh = (inside && k == 0) ? wh_left : wh_all;
                        const bool on = (k == 0 || inside) && !(wl > wh || fhi < wl || flo > wh);
                        need[2 * r + k] = on;
                        ia[2 * r + k] = rowb + (int)fmax(flo, wl); ib[2 * r + k] = rowb + (int)fmin(fhi, wh) + 1;
                    }
                }
                ++y; rowb += sy;
                if (y > yhi) { y = ylo; ++z; rowb += wrap; walking = z <= zhi; }
            }
        }
        int va[NW], vb[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) { va[w] = 0; vb[w] = 0; if (need[w]) tab_range_k<TK, T>(M, ia[w], ib[w], va[w], vb[w]); }
#pragma unroll
        for (int w = 0; w < NW; ++w) if (va[w] < vb[w]) push(va[w], vb[w]);
#ifdef PGICP_PHASE_STATS
        ++st_trips;
#endif
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(*pool_n) >= kPoolFlushAt) flush();
    }
#else
    while (__any(walking)) {
        if (walking) {
            const BK ly = fmax(slab_dist<BK>(uy, y, gb.h) - gb.margin, (BK)0), lz = fmax(slab_dist<BK>(uz, z, gb.h) - gb.margin, (BK)0);
            const BK lb2 = ly * ly + lz * lz;
            // (a range its owner scanned itself -- pool full -- improves best.d2 between flushes: bbest then lags on the safe side)
            if (!(lb2 > bbest)) {
                const BK rad = bk_sqrt(fmax(bbest - lb2, (BK)0)) * (BK)1.000001 + gb.margin;
                const BK flo = floor((ux - rad) * inv_hx), fhi = floor((ux + rad) * inv_hx);
                const bool inside = abs(y - c0y) <= r_done && abs(z - c0z) <= r_done;
#pragma unroll 1
                for (int k = 0; k < (inside ? 2 : 1); ++k) {
                    const BK wl = (inside && k == 1) ? wl_right : wl_all, wh = (inside && k == 0) ? wh_left : wh_all;
                    if (wl > wh || fhi < wl || flo > wh) continue;           // nothing new there, or the ball misses the window
                    const int fa = (int)fmax(flo, wl), fb = (int)fmin(fhi, wh);
                    int a, b;
                    tab_range_k<TK, T>(M, rowb + fa, rowb + fb + 1, a, b);
                    if (a < b) push(a, b);
                }
            }
            ++y; rowb += sy;
            if (y > yhi) { y = ylo; ++z; rowb += wrap; walking = z <= zhi; }
        }
#ifdef PGICP_PHASE_STATS
        ++st_trips;
#endif
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane(*pool_n) >= kPoolFlushAt) flush();
    }
#endif
    flush();
#ifdef PGICP_PHASE_STATS
    if (lane == 0) {
        atomicAdd(&g_ball[0], 1ULL); atomicAdd(&g_ball[1], (unsigned long long)st_open); atomicAdd(&g_ball[2], (unsigned long long)st_trips);
        atomicAdd(&g_ball[4], (unsigned long long)st_items); atomicAdd(&g_ball[5], (unsigned long long)st_flush);
        atomicAdd(&g_ball[7], (unsigned long long)st_rows);
    }
#endif
    if (open) {
        BK gr = ring_guarantee<BK>(gb, ux, uy, uz, c0x, c0y, c0z, max_rings);
        if (!(gr < Bits<BK>::inf())) resolved = true;                        // grid exhausted
        else {
            gr = gr - gb.margin;
            gr_out = (T)gr;
            bbest = bk_up(best.d2);
            if (gr > (BK)0 && (bbest < gr * gr || gr > bmax)) resolved = true;
            else r_next = max_rings + 1;
        }
    }
    return resolved;
}
