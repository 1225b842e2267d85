// k_minimise.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): point-to-plane sums, solve + update + convergence check, Censi covariance sums.

// ---------------------------------------------------------------------------
// error minimiser: per-pair 6-DoF Jacobian, 30 sums, register fold of the wave's sums (wave_fold)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void accumulate_pair(double *acc, double w, double px, double py, double pz, double qx,
                                                double qy, double qz, double nx, double ny, double nz)
{
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    const double e = (nx * dx + ny * dy) + nz * dz;
    double J[6];
    J[0] = py * nz - pz * ny;
    J[1] = pz * nx - px * nz;
    J[2] = px * ny - py * nx;
    J[3] = nx; J[4] = ny; J[5] = nz;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) acc[k++] += w * (J[a] * J[b]);
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] -= w * (J[a] * e);
    acc[27] += w;
    acc[28] += 1.0;
    acc[29] += w * (e * e);
}

// ---------------------------------------------------------------------------
// T3 of the reduction tree for NT sums at once, in registers.  wave_sum(v) gives lane 0 the tree whose level o (32, 16, 8, 4, 2,
// 1, in that order) replaces v[l] by v[l] + v[l + o] for l < o.  wave_fold adds exactly those pairs at exactly those levels for
// each of the NT sums (IEEE addition is commutative: which lane of a pair holds the sum does not matter; nothing is
// re-associated), but TRANSPOSES while it folds: at level o two registers (a, b) are first exchanged so that the lanes with bit o
// clear hold both halves of a and the lanes with bit o set both halves of b, and ONE add forms the level of both.  n registers
// become (n + 1) / 2 (an odd one out is paired with itself), and after the six levels one register holds every sum: sum k in the
// lane whose bits are k's reversed (fold_lane).  Levels 32 / 16 are v_permlane32_swap / v_permlane16_swap per dword, levels 8 / 4
// DPP row moves under a bank mask, levels 2 / 1 quad_perm (a bank is four lanes, so level 2 selects by lane bit instead).  No LDS
// traffic, ~1/6 of the instructions of NT x wave_sum.
// The swaps and DPP moves read the registers of inactive lanes as they are: ALL 64 LANES OF THE WAVE MUST BE ACTIVE here.  Every
// return before block_reduce_store in the reduce kernels is block-uniform (a whole problem done, a whole block past the end);
// the per-pair conditions only skip arithmetic.
// ---------------------------------------------------------------------------
constexpr int kDppShl4 = 0x104, kDppShr4 = 0x114, kDppRor8 = 0x128, kDppQuadXor2 = 0x4E, kDppQuadXor1 = 0xB1;

__host__ __device__ constexpr int fold_lane(int k)
{
    return ((k & 1) << 5) | ((k & 2) << 3) | ((k & 4) << 1) | ((k & 8) >> 1) | ((k & 16) >> 3) | ((k & 32) >> 5);
}

__device__ __forceinline__ double fold_pack(unsigned lo, unsigned hi) { return __hiloint2double((int)hi, (int)lo); }
__device__ __forceinline__ unsigned fold_lo(double v) { return (unsigned)__double2loint(v); }
__device__ __forceinline__ unsigned fold_hi(double v) { return (unsigned)__double2hiint(v); }

// levels 32 and 16: lanes [32, 64) (odd rows of 16) of a change places with lanes [0, 32) (even rows) of b
template <int O>
__device__ __forceinline__ double fold_swap_add(double a, double b)
{
    static_assert(O == 32 || O == 16, "swap levels");
    unsigned al = fold_lo(a), ah = fold_hi(a), bl = fold_lo(b), bh = fold_hi(b);
    if constexpr (O == 32) {
        const auto l = __builtin_amdgcn_permlane32_swap(al, bl, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(ah, bh, false, false);
        al = l[0]; bl = l[1]; ah = h[0]; bh = h[1];
    } else {
        const auto l = __builtin_amdgcn_permlane16_swap(al, bl, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(ah, bh, false, false);
        al = l[0]; bl = l[1]; ah = h[0]; bh = h[1];
    }
    return fold_pack(al, ah) + fold_pack(bl, bh);
}

// x = `keep` with the lanes of the banks in BANKS replaced by src moved as CTRL says
template <int CTRL, int BANKS>
__device__ __forceinline__ double fold_dpp(double keep, double src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)fold_lo(keep), (int)fold_lo(src), CTRL, 0xF, BANKS, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)fold_hi(keep), (int)fold_hi(src), CTRL, 0xF, BANKS, false);
    return fold_pack(lo, hi);
}

// levels 8 .. 1 of a pair: lanes with bit O clear get a[l] + a[l + O], lanes with bit O set b[l - O] + b[l]
template <int O>
__device__ __forceinline__ double fold_row_add(double a, double b, int lane)
{
    if constexpr (O == 8)           // banks 2, 3 = lanes 8 .. 15 of a row take b's lanes 0 .. 7; banks 0, 1 take a's lanes 8 .. 15
        return fold_dpp<kDppRor8, 0xC>(a, b) + fold_dpp<kDppRor8, 0x3>(b, a);
    else if constexpr (O == 4)      // banks 1, 3 = lanes 4 .. 7, 12 .. 15 take b[l - 4]; banks 0, 2 take a[l + 4]
        return fold_dpp<kDppShr4, 0xA>(a, b) + fold_dpp<kDppShl4, 0x5>(b, a);
    else {
        const bool up = (lane & O) != 0;
        const double own = up ? b : a, sent = up ? a : b;
        return own + fold_dpp<O == 2 ? kDppQuadXor2 : kDppQuadXor1, 0xF>(sent, sent);
    }
}

template <int O>
__device__ __forceinline__ double fold_pair(double a, double b, int lane)
{
    if constexpr (O >= 16) return fold_swap_add<O>(a, b); else return fold_row_add<O>(a, b, lane);
}

// one level: v[0 .. N) -> v[0 .. (N + 1) / 2)
template <int O, int N>
__device__ __forceinline__ void fold_level(double *v, int lane)
{
#pragma unroll
    for (int j = 0; j < (N + 1) / 2; j++) v[j] = fold_pair<O>(v[2 * j], 2 * j + 1 < N ? v[2 * j + 1] : v[2 * j], lane);
}

// sum k of the wave ends in lane fold_lane(k) of the value returned (v is used up)
template <int NT>
__device__ __forceinline__ double wave_fold(double *v, int lane)
{
    static_assert(NT >= 1 && NT <= 64, "one lane per sum");
    constexpr int n1 = (NT + 1) / 2, n2 = (n1 + 1) / 2, n3 = (n2 + 1) / 2, n4 = (n3 + 1) / 2, n5 = (n4 + 1) / 2;
    fold_level<32, NT>(v, lane);
    fold_level<16, n1>(v, lane);
    fold_level<8, n2>(v, lane);
    fold_level<4, n3>(v, lane);
    fold_level<2, n4>(v, lane);
    fold_level<1, n5>(v, lane);
    return v[0];
}

template <int NT>
__device__ __forceinline__ void block_reduce_store(double *acc, double *__restrict__ out)
{
    __shared__ double red[kReduceBlock / 64][NT];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const double v = wave_fold<NT>(acc, lane);
    const int k = fold_lane(lane);              // (the bit reversal is its own inverse)
    if (k < NT) red[wid][k] = v;
    __syncthreads();
    if (threadIdx.x < NT) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kReduceBlock / 64; w++) s += red[w][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// PointToPointErrorMinimizer's sums for one kept pair (icp_math.hpp solve_p2point): sum w p, sum w q, sum w q p^T, the
// residual is the sum of the pairs' distances |p - q| (difference in T, as libpointmatcher takes it)
template <typename T>
__device__ __forceinline__ void accumulate_pair_p2p(double *acc, double w, T px, T py, T pz, T qx, T qy, T qz)
{
    const double p[3] = {(double)px, (double)py, (double)pz}, q[3] = {(double)qx, (double)qy, (double)qz};
#pragma unroll
    for (int a = 0; a < 3; a++) { acc[a] += w * p[a]; acc[3 + a] += w * q[a]; }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) acc[6 + 3 * a + b] += w * (q[a] * p[b]);
    const double dx = (double)(T)(px - qx), dy = (double)(T)(py - qy), dz = (double)(T)(pz - qz);
    acc[27] += w;
    acc[28] += 1.0;
    acc[29] += sqrt((dx * dx + dy * dy) + dz * dz);
}

// v / sqrt(v.v) in T (left alone when v.v == 0): Eigen's normalized()
template <typename T>
__device__ __forceinline__ void normalized3(T &x, T &y, T &z)
{
    const T zz = (x * x + y * y) + z * z;
    if (zz > (T)0) { const T s = sqrt(zz); x = x / s; y = y / s; z = z / s; }
}

// The error elements of one iteration -> block partials.  A PAIR e = (reading point e / knn, its (e % knn)-th neighbour) is
// kept when it has a neighbour, its distance is within the quantile filter's limit and -- with a SurfaceNormalOutlierFilter
// in the chain -- the reading's normal (rotated with the reading) and the reference's lie within maxAngle of each other.
// MIN: 0 point-to-plane (30 sums of J J^T, J e, ...), 1 point-to-point (Kabsch sums).  GEN: false is the usual chain -- one
// neighbour per point, no normal filter -- with nothing of the general case compiled in (measured: the general kernel costs
// the headline's reduce 15 %).
// [EXT] RobustOutlierFilter's weight of a pair (oracle: orc_robust_weights; the same expressions in T)
template <typename T>
__device__ __forceinline__ T robust_weight(const RobustDev<T> &rb, T dd, T s2)
{
    const T e2 = dd / s2;
    T w = (T)0;
    switch (rb.fct) {
    case 1: w = (T)1 / ((T)1 + e2 / rb.k2); break;
    case 2: w = exp(-(e2 / rb.k2)); break;
    case 3: { const T t = rb.k + e2; w = e2 >= rb.k ? ((T)4 * rb.k2) / (t * t) : (T)1; break; }
    case 4: { const T t = rb.k + e2; w = rb.k2 / (t * t); break; }
    case 5: { const T t = (T)1 - e2 / rb.k2; w = e2 >= rb.k2 ? (T)0 : t * t; break; }
    case 6: w = e2 >= rb.k2 ? rb.k / sqrt_rn_t(e2) : (T)1; break;
    default: w = (T)1 / sqrt_rn_t(e2); break;
    }
    if (sizeof(T) == 8 && w <= (T)1e-50) w = (T)1e-50;       // (upstream's floor is a double: zero in float)
    if (rb.cut && e2 >= rb.a2) w = (T)0;
    return w;
}

// [EXT] The distance RobustOutlierFilter weighs a pair by (pgicp_robust.h): the matcher's d2, or -- distanceType point2plane -- the
// squared distance of the step reading p' = Tc (rx, ry, rz) from the plane through the matched map point q with normal n, in T.
// One statement for k_p2plane_reduce, k_cov_reduce and k_noise_sum (Tc: as for pair_filter_weight).
template <typename T, typename S>
__device__ __forceinline__ T robust_pair_dd(const RobustDev<T> &rb, T d2, const S *Tc, T rx, T ry, T rz, T qx, T qy, T qz, T nx, T ny, T nz)
{
    if (rb.dist == 0) return d2;
    T px, py, pz;
    apply_T<T>(Tc, rx, ry, rz, px, py, pz);
    const T dx = px - qx, dy = py - qy, dz = pz - qz;
    const T v = (nx * dx + ny * dy) + nz * dz;
    return v * v;
}

// [EXT] GenericDescriptorOutlierFilter's weight of a pair whose neighbour's value is v (pgicp.h, pgicp_set_descriptor_filter; in
// T): hard modes 1 / 0 by the strict comparison, soft v / gmax -- and 0 when the soft maximum is 0 (deviation b)
template <typename T>
__device__ __forceinline__ T gd_weight(int mode, T thr, T v, T gmax)
{
    if (mode == PGICP_DESC_FILTER_LARGER) return v > thr ? (T)1 : (T)0;
    if (mode == PGICP_DESC_FILTER_SMALLER) return v < thr ? (T)1 : (T)0;
    return gmax > (T)0 ? v / gmax : (T)0;
}

// The combined outlier weight of a pair that has a neighbour within the quantile / MaxDist limit (`keep` in k_p2plane_reduce):
// the SurfaceNormalOutlierFilter's 0 / 1 (the step reading's normal is R (R_pre n) with R the rotation of Tc, in T like the
// points), times the Robust weight, times the GenericDescriptor weight -- the real-valued factors multiply in T.  0: the pair is
// no error element.  One statement for every kernel that must agree on the last error elements: k_p2plane_reduce (Tc the
// iteration's transform) and k_noise_sum (k_noise.inc; Tc = T_prev, gmax = gd_last: what the last iteration ran with).
template <typename T, typename S>
__device__ __forceinline__ T pair_filter_weight(const S *Tc, bool use_nrm, const T *qn, T bx, T by, T bz, T normal_cos, bool robust,
                                                const RobustDev<T> &rb, T dd, T rs2, bool gd, int gd_mode, T gd_thr, T gv, T gmax)
{
    if (use_nrm) {
        T ax = ((T)Tc[0] * qn[0] + (T)Tc[1] * qn[1]) + (T)Tc[2] * qn[2];
        T ay = ((T)Tc[4] * qn[0] + (T)Tc[5] * qn[1]) + (T)Tc[6] * qn[2];
        T az = ((T)Tc[8] * qn[0] + (T)Tc[9] * qn[1]) + (T)Tc[10] * qn[2];
        normalized3<T>(ax, ay, az);
        normalized3<T>(bx, by, bz);
        if (((ax * bx + ay * by) + az * bz) < normal_cos) return (T)0;
    }
    T w = (T)1;
    if (robust) w = robust_weight<T>(rb, dd, rs2);
    if (gd) w = w * gd_weight<T>(gd_mode, gd_thr, gv, gmax);
    return w;
}

template <typename T, int MIN, bool GEN>
__global__ __launch_bounds__(kReduceBlock) void k_p2plane_reduce(const ProblemDev *__restrict__ probs,
                                                                  const MapDev<T> *__restrict__ maps,
                                                                  const T *__restrict__ rd_pre, const T *__restrict__ rd_nrm,
                                                                  const int *__restrict__ slot,
                                                                  const T *__restrict__ d2, double *__restrict__ partials,
                                                                  int max_blocks, const int *__restrict__ active, T normal_cos, RobustDev<T> rb,
                                                                  const int *__restrict__ scan_pos, int gd_mode, T gd_thr)
{
    // The reduction tree RT-1 (oracle/icp_oracle.c, DESIGN.md section 2): this block is tree block `tile`, thread t adds the pairs
    // at tree positions tile * kReduceSpan + u * 256 + t, u = 0 .. 7, in that order (T2); block_reduce_store is T3 + T4, the solve
    // kernel / k_sum_partials T5.  A tree position IS a sorted position (PGICP_SUM_ORDER_SORTED, scan_pos null: everything below
    // reads coalesced) or a position in the caller's reading (PGICP_SUM_ORDER_SCAN): then pair `e` below is where the sort put it.
    const int prob = active[blockIdx.y];
    const ProblemDev &P = probs[prob];
    if (P.done) return;
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const bool robust = GEN && rb.fct != 0;
    const T rs2 = (T)P.robust_s2;
    const int knn = GEN ? P.knn : 1;
    const int np = GEN ? pairs_n(P) : P.n;
    const long long poff = GEN ? pairs_off(P) : P.off;
    if (tile * kReduceSpan >= np) return;       // whole block past the end: partial stays unused
    const MapDev<T> M = maps[P.map];
    const T limit = (T)P.limit;
    const bool use_nrm = GEN && rd_nrm != nullptr;
    const bool plane_dd = GEN && robust && rb.dist != 0;        // (pgicp_robust.h: the robust weights see plane distances)
    const bool need_nrm = MIN == 0 || use_nrm || plane_dd;
    const bool gd = GEN && gd_mode != PGICP_DESC_FILTER_OFF;
    const T gmax = GEN ? Bits<T>::val((typename Bits<T>::U)P.gd_key) : (T)0;
    double acc[kSys];
#pragma unroll
    for (int k = 0; k < kSys; k++) acc[k] = 0.0;
    // three load stages, each with kReduceItems independent loads in flight per lane:
    // (slot, d2) -> gathered (point, normal, reading) -> arithmetic
    using V4 = typename Vec4<T>::type;
    for (int rnd = 0; rnd < kReduceRounds; ++rnd) {
    const int base = tile * kReduceSpan + rnd * (kReduceBlock * kReduceItems);
    if (base >= np) break;
    int ss[kReduceItems];
    bool keep[kReduceItems];
    T dds[GEN ? kReduceItems : 1];
    int es[kReduceItems];                       // the pair's position in the SORTED per-pair arrays
#pragma unroll
    for (int it = 0; it < kReduceItems; it++) {
        const int pos = base + it * kReduceBlock + threadIdx.x;
        int e = pos;
        if (scan_pos && pos < np) e = knn == 1 ? scan_pos[P.off + pos] : scan_pos[P.off + pos / knn] * knn + pos % knn;
        es[it] = e;
        ss[it] = -1;
        T dd = Bits<T>::inf();
        if (pos < np) { dd = d2[poff + e]; ss[it] = slot[poff + e]; }
        keep[it] = ss[it] >= 0 && dd <= limit;
        if constexpr (GEN) dds[it] = dd;
    }
    V4 mp[kReduceItems], mn[kReduceItems];
    T qv[kReduceItems][3], qn[kReduceItems][3];
    T gv[GEN ? kReduceItems : 1];
#pragma unroll
    for (int it = 0; it < kReduceItems; it++) {
        const int e = es[it];
        const int s = keep[it] ? ss[it] : 0;
        const int i = keep[it] ? (knn == 1 ? e : e / knn) : 0;
        if (need_nrm) { mp[it] = map_rec<T>(M.nrm, 2 * (long long)s); mn[it] = map_rec<T>(M.nrm, 2 * (long long)s + 1); }     // one 32-byte record
        else mp[it] = map_rec<T>(M.pts, s);
        const T *q = rd_pre + 3 * (P.off + i);
        qv[it][0] = q[0]; qv[it][1] = q[1]; qv[it][2] = q[2];
        if constexpr (GEN) {
            if (use_nrm) { const T *n = rd_nrm + 3 * (P.off + i); qn[it][0] = n[0]; qn[it][1] = n[1]; qn[it][2] = n[2]; }
            if (gd) gv[it] = as_global(M.val)[s - (keep[it] ? M.first : 0)];       // (s = 0 for a pair not kept: a valid index, unused)
        }
    }
#pragma unroll
    for (int it = 0; it < kReduceItems; it++) {
        if (keep[it]) {
            double wgt = 1.0;
            if constexpr (GEN) {
                // SurfaceNormal x Robust x GenericDescriptor (pair_filter_weight; the quantile / MaxDist filters are `keep`)
                const T w = pair_filter_weight<T>(tcur_of<T>(P), use_nrm, qn[it], use_nrm ? mn[it].x : (T)0, use_nrm ? mn[it].y : (T)0,
                                                  use_nrm ? mn[it].z : (T)0, normal_cos, robust, rb,
                                                  plane_dd ? robust_pair_dd<T>(rb, dds[it], tcur_of<T>(P), qv[it][0], qv[it][1], qv[it][2], mp[it].x, mp[it].y,
                                                                               mp[it].z, mn[it].x, mn[it].y, mn[it].z) : dds[it],
                                                  rs2, gd, gd_mode, gd_thr, gd ? gv[it] : (T)0, gmax);
                if (w == (T)0) continue;
                wgt = (double)w;
            }
            T px, py, pz;
            apply_T<T>(tcur_of<T>(P), qv[it][0], qv[it][1], qv[it][2], px, py, pz);
            if (MIN == 0)
                accumulate_pair(acc, wgt, (double)px, (double)py, (double)pz, (double)mp[it].x, (double)mp[it].y, (double)mp[it].z,
                                (double)mn[it].x, (double)mn[it].y, (double)mn[it].z);
            else
                accumulate_pair_p2p<T>(acc, wgt, px, py, pz, mp[it].x, mp[it].y, mp[it].z);
        }
    }
    }
    block_reduce_store<kSys>(acc, partials + ((long long)prob * max_blocks + tile) * kSys);
}

// stage-level ErrorElements/residual with caller-provided ids (original
// indices) and weights; reading is already in the map frame.
template <typename T, int MIN>
__global__ __launch_bounds__(kReduceBlock) void k_error_stats(const MapDev<T> *__restrict__ maps, int map,
                                                               const int *__restrict__ slot_of, const T *__restrict__ rd,
                                                               int stride, const int *__restrict__ ids,
                                                               const T *__restrict__ w, int n, int knn, T mx, T my, T mz,
                                                               double *__restrict__ partials)
{
    // (ids / w: knn entries per reading point, [point][neighbour]; n = points)
    const MapDev<T> M = maps[map];
    double acc[kSys];
#pragma unroll
    for (int k = 0; k < kSys; k++) acc[k] = 0.0;
    for (int it = 0; it < kReduceItems * kReduceRounds; it++) {
        const int e = blockIdx.x * kReduceSpan + it * kReduceBlock + threadIdx.x;
        if (e < n * knn) {
            const int i = knn == 1 ? e : e / knn;
            const T wi = w[e];
            const int id = ids[e];
            if (id >= 0 && wi != (T)0) {
                // the map is stored centred; express the reading in the same frame
                const T px = rd[(long long)i * stride] - mx, py = rd[(long long)i * stride + 1] - my,
                        pz = rd[(long long)i * stride + 2] - mz;
                const int s = slot_of[id];
                const auto mp = map_rec<T>(M.pts, s);
                if (MIN == 0) {
                    const auto mn = map_rec<T>(M.nrm, 2 * (long long)s + 1);
                    accumulate_pair(acc, (double)wi, (double)px, (double)py, (double)pz, (double)mp.x, (double)mp.y,
                                    (double)mp.z, (double)mn.x, (double)mn.y, (double)mn.z);
                } else
                    accumulate_pair_p2p<T>(acc, (double)wi, px, py, pz, mp.x, mp.y, mp.z);
            }
        }
    }
    block_reduce_store<kSys>(acc, partials + (long long)blockIdx.x * kSys);
}

// Blocks -> problem, step T5 of the reduction tree (oracle/icp_oracle.c "RT-1", DESIGN.md section 2): eight chains, chain c
// adds blocks c, c + 8, c + 16 ... in order, then the eight chain values are added in chain order -- a fixed shape whatever
// the launch, ~8x shorter than one serial chain.  256 threads: 8 chains x 32 values; valid for threadIdx.x < nt (nt <= 32).
__device__ __forceinline__ double sum_partials_256(const double *__restrict__ part, int nb, int nt, double (*lds)[32])
{
    const int v = threadIdx.x & 31, grp = threadIdx.x >> 5;
    double s = 0.0;
    if (v < nt)
        for (int b = grp; b < nb; b += 8) s += part[(long long)b * nt + v];
    lds[grp][v] = s;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x < 32) {
#pragma unroll
        for (int k = 0; k < 8; k++) tot += lds[k][threadIdx.x];
    }
    return tot;
}

// the same for every problem of a batch and up to 64 values per block partial (the covariance sums have 42): per problem one
// block of 256 threads, values 32 at a time.  Everything that leaves the device as a sum over pairs passes through T5 here or
// in k_solve_update.
__global__ __launch_bounds__(256) void k_sum_partials(const double *__restrict__ partials, int max_blocks, int nt,
                                                       const ProblemDev *__restrict__ probs /* or null */,
                                                       int nb_uniform, double *__restrict__ out)
{
    const int p = blockIdx.x;
    int nb = nb_uniform;
    if (probs) {
        nb = (pairs_n(probs[p]) + kReduceSpan - 1) / kReduceSpan;
        if (probs[p].status != PGICP_ST_OK) nb = 0;       // partials were never written
    }
    __shared__ double red[8][32];
    const double *src = partials + (long long)p * max_blocks * nt;
    for (int v0 = 0; v0 < nt; v0 += 32) {
        const int v = threadIdx.x & 31, grp = threadIdx.x >> 5;
        double s = 0.0;
        if (v0 + v < nt)
            for (int b = grp; b < nb; b += 8) s += src[(long long)b * nt + v0 + v];
        __syncthreads();                                  // (the previous chunk's read of `red`)
        red[grp][v] = s;
        __syncthreads();
        if (threadIdx.x < 32 && v0 + threadIdx.x < nt) {
            double tot = 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) tot += red[k][threadIdx.x];
            out[(long long)p * nt + v0 + threadIdx.x] = tot;
        }
    }
}

// ---------------------------------------------------------------------------
// solve + update + convergence check: one wave per problem, lane 0 does the
// (tiny, serial) double-precision algebra; no host round trip per iteration
// ---------------------------------------------------------------------------
// What k_compact_active does for a batch, done by the solve kernel itself for a batch of ONE problem: the iteration stamp,
// the matcher's queue counters, {problems done, stamp} for the polling host.  No-op when single_stamp is null.
__device__ __forceinline__ void single_bookkeeping(int *single_host_flag, int *__restrict__ single_stamp,
                                                   int *__restrict__ single_queue_counters, int done)
{
    if (!single_stamp) return;
    const int stamp = *single_stamp + 1;
    *single_stamp = stamp;
    if (single_queue_counters)
        for (int t = 0; t < 4; ++t) { single_queue_counters[8 + t] = single_queue_counters[t]; single_queue_counters[t] = 0; }
    if (single_host_flag) {
        __hip_atomic_store(single_host_flag, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(single_host_flag + 1, stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_solve_update(ProblemDev *__restrict__ probs, const double *__restrict__ partials,
                                                       int max_blocks, ChainDev<T> ch, int *__restrict__ n_done,
                                                       const int *__restrict__ active, int *single_host_flag,
                                                       int *__restrict__ single_stamp, int *__restrict__ single_queue_counters)
{
    const int prob = active[blockIdx.x];
    ProblemDev &P = probs[prob];
    if (P.done) {
        // (a batch of one problem whose host looks at the flag every few iterations keeps enqueueing iterations past the
        // converged one: each of them must still advance the stamp the host counts, or the host's wait never ends)
        if (threadIdx.x == 0) single_bookkeeping(single_host_flag, single_stamp, single_queue_counters, 1);
        return;
    }
    __shared__ double sys[kSys];
    __shared__ double red[8][32];
    const int nb = (pairs_n(P) + kReduceSpan - 1) / kReduceSpan;
    const double tot = sum_partials_256(partials + (long long)prob * max_blocks * kSys, nb, kSys, red);
    if (threadIdx.x < kSys) {
        sys[threadIdx.x] = tot;
        P.sys[threadIdx.x] = tot;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    P.gd_last = P.gd_key;            // (GenericDescriptor soft maximum: this iteration's, kept for the covariance; the next starts from 0)
    P.gd_key = 0;
    int status = PGICP_ST_OK;
    if (P.n_finite == 0 || !(sys[28] > 0.0)) status = PGICP_ST_NO_MATCH;
    if (status == PGICP_ST_OK) {
        double x[6], dT[16], Tn[16];
        if (ch.minimizer == 1) P.rank = solve_p2point(sys, dT);
        else if (ch.force4dof) {
            double s4[27];
            for (int i = 0; i < 27; i++) s4[i] = sys[i];
            constrain_4dof(s4);
            P.rank = solve6(s4, ch.rank_rel_tol, x) - 2;          // (the two cleared directions are not degrees of freedom)
            delta_T(x, dT);
        }
        else {
            P.rank = solve6(sys, ch.rank_rel_tol, x);
            delta_T(x, dT);
        }
        for (int i = 0; i < 16; i++) { P.T_prev[i] = P.T_iter[i]; P.dT[i] = dT[i]; }
        mat4_mul(dT, P.T_iter, Tn);
        for (int i = 0; i < 16; i++) P.T_iter[i] = Tn[i];
        for (int i = 0; i < 12; i++) { P.Tcur_prev[i] = P.Tcur[i]; P.Tcur[i] = Tn[i]; P.Tcur_prev_f[i] = P.Tcur_f[i]; P.Tcur_f[i] = (float)Tn[i]; }
        P.n_kept = (int)sys[28];
        P.iters += 1;
        const int f = checker_check(P.chk, Tn, ch.max_iters, ch.min_rot, ch.min_trans, ch.smooth, ch.bound_rot, ch.bound_trans);
        if (f & 8) status = PGICP_ST_NAN;
        else if (f & 16) status = PGICP_ST_BOUND;
        else {
            if (f & 2) P.converged = 1;
            if (f & 4) P.max_iter_reached = 1;
            if (!(f & 1)) { P.done = 1; atomicAdd(n_done, 1); }
        }
    }
    if (status != PGICP_ST_OK) {
        P.status = status;
        P.done = 1;
        atomicAdd(n_done, 1);
    }
    // A batch of ONE problem (a streamed scan, the SLAM front end): what k_compact_active would do in a launch of its own --
    // the iteration stamp, the matcher's queue counters, {problems done, stamp} for the polling host -- is done here
    // (active[] = {0} needs no update).
    single_bookkeeping(single_host_flag, single_stamp, single_queue_counters, P.done ? 1 : 0);
}

// active[] = ids of the problems still iterating, followed by the finished ones (so a stale, larger
// launch count only adds blocks that exit at once).  One block; P is at most a few thousand.
__global__ __launch_bounds__(1024) void k_compact_active(const ProblemDev *__restrict__ probs, int P, int *__restrict__ active,
                                                         int *host_flag, int *__restrict__ stamp_counter, int *__restrict__ queue_counters)
{
    // The stamp is a counter in device memory that this kernel advances (the host counts its launches alongside): a
    // kernel argument would differ from launch to launch, and the iteration is replayed from a captured graph.
    int stamp = 0;
    if (threadIdx.x == 0) { stamp = *stamp_counter + 1; *stamp_counter = stamp; }
    // the matcher's queue counters are cleared here for the next iteration (their last values stay readable 8 ints on)
    if (queue_counters && threadIdx.x < 4) { queue_counters[8 + threadIdx.x] = queue_counters[threadIdx.x]; queue_counters[threadIdx.x] = 0; }
    __shared__ int lds[32];
    __shared__ int base_live, base_done;
    if (threadIdx.x == 0) { base_live = 0; base_done = 0; }
    __syncthreads();
    // pass 1: count live
    int live_cnt = 0;
    for (int p = threadIdx.x; p < P; p += 1024) live_cnt += probs[p].done ? 0 : 1;
    int tot;
    block_exclusive_scan_1024(live_cnt, lds, tot);
    const int n_live = tot;
    // pass 2: stable placement chunk by chunk
    for (int b = 0; b < P; b += 1024) {
        const int p = b + threadIdx.x;
        const int is_live = (p < P && !probs[p].done) ? 1 : 0;
        const int is_done = (p < P && probs[p].done) ? 1 : 0;
        int tl, td;
        const int el = block_exclusive_scan_1024(is_live, lds, tl);
        const int ed = block_exclusive_scan_1024(is_done, lds, td);
        if (is_live) active[base_live + el] = p;
        if (is_done) active[n_live + base_done + ed] = p;
        __syncthreads();
        if (threadIdx.x == 0) { base_live += tl; base_done += td; }
        __syncthreads();
    }
    // the host polls this pair in pinned memory instead of waiting for a copy: {problems done, iteration stamp}
    if (host_flag && threadIdx.x == 0) {
        __hip_atomic_store(host_flag, P - n_live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_flag + 1, stamp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// after an ICP run: its problems take part in one more pass of the chain (the residual check of the result)
__global__ __launch_bounds__(256) void k_reopen(ProblemDev *__restrict__ probs, int P)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P && probs[p].status == PGICP_ST_OK) probs[p].done = 0;
}
void launch_reopen(hipStream_t st, ProblemDev *probs, int P)
{
    hipLaunchKernelGGL(k_reopen, dim3((P + 255) / 256), dim3(256), 0, st, probs, P);
}

int knn_trace_set(int sorted_index)
{
#ifdef PGICP_KNN_STATS
    return hipMemcpyToSymbol(HIP_SYMBOL(g_trace_i), &sorted_index, sizeof(int)) == hipSuccess ? 0 : -1;
#else
    (void)sorted_index;
    return -1;
#endif
}

int knn_phase_read(unsigned long long out[48], int reset)
{
#ifdef PGICP_PHASE_STATS
    static unsigned long long h[64 * 48];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof h) != hipSuccess) return -1;
    for (int k = 0; k < 48; k++) {
        out[k] = 0;
        const bool is_max = k == 32 + 12 || k == 32 + 13;
        for (int c = 0; c < 64; c++) out[k] = is_max ? std::max(out[k], h[c * 48 + k]) : out[k] + h[c * 48 + k];
    }
    if (reset) { std::memset(h, 0, sizeof h); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase), h, sizeof h); }
    {
        unsigned long long b[16];
        if (hipMemcpyFromSymbol(b, HIP_SYMBOL(g_ball), sizeof b) == hipSuccess && b[0])
            std::fprintf(stderr, "      ball walk: %llu waves; per wave: %.1f open lanes, %.1f trips, %.1f items in %.2f evaluations; %.1f rows per open lane\n",
                         b[0], (double)b[1] / b[0], (double)b[2] / b[0], (double)b[4] / b[0], (double)b[5] / b[0], b[1] ? (double)b[7] / b[1] : 0.0);
        if (reset) { std::memset(b, 0, sizeof b); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_ball), b, sizeof b); }
    }
    {
        unsigned long long w[16];
        if (hipMemcpyFromSymbol(w, HIP_SYMBOL(g_slow_worst), sizeof w) == hipSuccess && w[0])
            std::fprintf(stderr, "      slowest entry: %llu cycles [fetch %llu seed %llu look-ups %llu points %llu walk %llu finish %llu]; square of %llu rows, %llu with points, %llu long, %llu candidates; bounded %llu capped %llu, result at %llu mm\n",
                         w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[8], w[9], w[10], w[11], w[12], w[13], w[14]);
        if (reset) { std::memset(w, 0, sizeof w); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_slow_worst), w, sizeof w); }
    }
    return 0;
#else
    (void)out; (void)reset;
    return -1;
#endif
}

// diagnostics build (-DPGICP_XCC_STATS) only: the fast matcher's launches since the last reset, per hardware XCC, to stderr
int knn_xcc_report(int use_seed, int reset)
{
#ifdef PGICP_XCC_STATS
    static unsigned long long h[8][kXccCopies][16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_xcc), sizeof h) != hipSuccess) return -1;
    unsigned long long x[8][16] = {};
    for (int c = 0; c < 8; c++)
        for (int k = 0; k < kXccCopies; k++)
            for (int s = 0; s < 16; s++) x[c][s] = s < 2 ? std::max(x[c][s], h[c][k][s]) : x[c][s] + h[c][k][s];
    unsigned long long first = ~0ULL;
    for (int c = 0; c < 8; c++) if (x[c][3]) first = std::min(first, ~x[c][0]);
    std::fprintf(stderr, "    fast kernel per XCC (seeded %d) [last end after the launch's first start | wave time summed | waves | waves by blockIdx.x & 7], ticks of 10 ns:", use_seed);
    for (int c = 0; c < 8; c++) {
        std::fprintf(stderr, " %llu|%llu|%llu|", x[c][3] ? x[c][1] - first : 0ULL, x[c][2], x[c][3]);
        for (int k = 0; k < 8; k++) std::fprintf(stderr, "%s%llu", k ? "," : "", x[c][8 + k]);
    }
    std::fprintf(stderr, "\n");
    if (reset) { std::memset(h, 0, sizeof h); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_xcc), h, sizeof h); }
    return 0;
#else
    (void)use_seed; (void)reset;
    return -1;
#endif
}

int knn_stats_read(unsigned long long out[56], int reset)
{
#ifdef PGICP_KNN_STATS
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_knn_stats), 56 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[56] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_knn_stats), z, sizeof z); }
    return 0;
#else
    (void)out; (void)reset;
    return -1;
#endif
}

// diagnostics build only: per-query dump buffers of the fast matcher (see g_cnt_dump)
int knn_dump_setup(long long total, int passes)
{
#ifdef PGICP_KNN_STATS
    unsigned *c = nullptr; float *d = nullptr;
    if (hipMalloc((void **)&c, sizeof(unsigned) * total * passes) != hipSuccess || hipMalloc((void **)&d, sizeof(float) * total * passes) != hipSuccess) return -1;
    (void)hipMemset(c, 0, sizeof(unsigned) * total * passes);
    (void)hipMemset(d, 0, sizeof(float) * total * passes);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_cnt_dump), &c, sizeof c);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_d2_dump), &d, sizeof d);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dump_total), &total, sizeof total);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dump_passes), &passes, sizeof passes);
    return 0;
#else
    (void)total; (void)passes;
    return -1;
#endif
}
int knn_dump_read(unsigned *cnt, float *d2, long long n)
{
#ifdef PGICP_KNN_STATS
    unsigned *c = nullptr; float *d = nullptr;
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(&c, HIP_SYMBOL(g_cnt_dump), sizeof c);
    (void)hipMemcpyFromSymbol(&d, HIP_SYMBOL(g_d2_dump), sizeof d);
    if (!c || !d) return -1;
    if (hipMemcpy(cnt, c, sizeof(unsigned) * n, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(d2, d, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
#else
    (void)cnt; (void)d2; (void)n;
    return -1;
#endif
}

void launch_compact_active(hipStream_t st, const ProblemDev *probs, int P, int *active, int *host_flag, int *stamp_counter,
                           int *queue_counters)
{
    hipLaunchKernelGGL(k_compact_active, dim3(1), dim3(1024), 0, st, probs, P, active, host_flag, stamp_counter, queue_counters);
}

// ---------------------------------------------------------------------------
// Censi covariance sums (SURVEY.md A.8) over the last iteration's kept pairs:
// 21 terms of H (upper) + 21 terms of G (upper); the host inverts H.
// ---------------------------------------------------------------------------
// GD: a GenericDescriptorOutlierFilter is in the chain (false: the chain's kernel as it was without it)
template <typename T, bool GD>
__global__ __launch_bounds__(kReduceBlock) void k_cov_reduce(const ProblemDev *__restrict__ probs,
                                                              const MapDev<T> *__restrict__ maps,
                                                              const T *__restrict__ rd_pre, const T *__restrict__ rd_nrm,
                                                              const int *__restrict__ slot,
                                                              const T *__restrict__ d2, double *__restrict__ partials,
                                                              int max_blocks, T normal_cos, RobustDev<T> rb, const int *__restrict__ scan_pos,
                                                              int gd_mode, T gd_thr)
{
    // (tree positions -> pairs as in k_p2plane_reduce)
    const ProblemDev &P = probs[blockIdx.y];
    if (P.status != PGICP_ST_OK) return;
    const int np = pairs_n(P), knn = P.knn;
    const long long poff = pairs_off(P);
    if (blockIdx.x * kReduceSpan >= np) return;
    const MapDev<T> M = maps[P.map];
    const T limit = (T)P.limit;
    // small-angle parameters of the last increment
    // (small_angles: arctangents in IEEE operations only -- the math library's asin / atan2 / cos are not the host's to the bit)
    double alpha, beta, gamma;
    small_angles(P.dT, alpha, beta, gamma);
    const double t_x = P.dT[3], t_y = P.dT[7], t_z = P.dT[11];
    double Tp[12];
#pragma unroll
    for (int k = 0; k < 12; k++) Tp[k] = P.T_prev[k];
    double acc[kCovTerms];
#pragma unroll
    for (int k = 0; k < kCovTerms; k++) acc[k] = 0.0;
    // the stages of k_p2plane_reduce, each with kReduceItems independent loads in flight per lane:
    // (slot, d2) -> gathered (record, reading, value) -> arithmetic; a thread adds its items u = 0 .. 7 in that order
    using V4 = typename Vec4<T>::type;
    const bool use_nrm = rd_nrm != nullptr;
    for (int rnd = 0; rnd < kReduceRounds; ++rnd) {
    const int base = blockIdx.x * kReduceSpan + rnd * (kReduceBlock * kReduceItems);
    if (base >= np) break;
    int ss[kReduceItems], es[kReduceItems];
    bool keep[kReduceItems];
    T dds[kReduceItems];
#pragma unroll
    for (int it = 0; it < kReduceItems; it++) {
        const int pos = base + it * kReduceBlock + threadIdx.x;
        int e = pos;
        if (scan_pos && pos < np) e = knn == 1 ? scan_pos[P.off + pos] : scan_pos[P.off + pos / knn] * knn + pos % knn;
        es[it] = e;
        ss[it] = -1;
        T dd = Bits<T>::inf();
        if (pos < np) { dd = d2[poff + e]; ss[it] = slot[poff + e]; }
        keep[it] = ss[it] >= 0 && dd <= limit;
        dds[it] = dd;
    }
    V4 mps[kReduceItems], mns[kReduceItems];
    T qv[kReduceItems][3], qn[kReduceItems][3];
    T gv[GD ? kReduceItems : 1];
#pragma unroll
    for (int it = 0; it < kReduceItems; it++) {
        const int e = es[it];
        const int s = keep[it] ? ss[it] : 0;            // (a pair not kept: valid indices, the values unused)
        const int i = keep[it] ? (knn == 1 ? e : e / knn) : 0;
        mps[it] = map_rec<T>(M.nrm, 2 * (long long)s);
        mns[it] = map_rec<T>(M.nrm, 2 * (long long)s + 1);
        const T *q = rd_pre + 3 * (P.off + i);
        qv[it][0] = q[0]; qv[it][1] = q[1]; qv[it][2] = q[2];
        if (use_nrm) { const T *n = rd_nrm + 3 * (P.off + i); qn[it][0] = n[0]; qn[it][1] = n[1]; qn[it][2] = n[2]; }
        if constexpr (GD) gv[it] = as_global(M.val)[s - (keep[it] ? M.first : 0)];
    }
#pragma unroll
    for (int it = 0; it < kReduceItems; it++) {
        if (!keep[it]) continue;
        // (the distance the robust weight saw in the last iteration: robust_pair_dd with the transform that iteration ran with)
        const T dd = rb.fct != 0 ? robust_pair_dd<T>(rb, dds[it], Tp, qv[it][0], qv[it][1], qv[it][2], mps[it].x, mps[it].y, mps[it].z,
                                                     mns[it].x, mns[it].y, mns[it].z) : dds[it];
        if constexpr (GD) {
            // the pair's Robust x GenericDescriptor weight in T, as k_p2plane_reduce forms it (the GenericDescriptor soft maximum:
            // the last iteration's); a pair of weight 0 is not an error element
            T w = rb.fct != 0 ? robust_weight<T>(rb, dd, (T)P.robust_s2) : (T)1;
            w = w * gd_weight<T>(gd_mode, gd_thr, gv[it], Bits<T>::val((typename Bits<T>::U)P.gd_last));
            if (w == (T)0) continue;
        } else {
            if (rb.fct != 0 && robust_weight<T>(rb, dd, (T)P.robust_s2) == (T)0) continue;      // (not an error element)
        }
        T pxt, pyt, pzt;
        apply_T<T>(Tp, qv[it][0], qv[it][1], qv[it][2], pxt, pyt, pzt);
        const V4 mp = mps[it], mn = mns[it];
        if (use_nrm) {                                  // (the SurfaceNormalOutlierFilter's weight of the pair: as in k_p2plane_reduce)
            const T *n = qn[it];
            T ax = ((T)Tp[0] * n[0] + (T)Tp[1] * n[1]) + (T)Tp[2] * n[2];
            T ay = ((T)Tp[4] * n[0] + (T)Tp[5] * n[1]) + (T)Tp[6] * n[2];
            T az = ((T)Tp[8] * n[0] + (T)Tp[9] * n[1]) + (T)Tp[10] * n[2];
            T bx = mn.x, by = mn.y, bz = mn.z;
            normalized3<T>(ax, ay, az);
            normalized3<T>(bx, by, bz);
            if (((ax * bx + ay * by) + az * bz) < normal_cos) continue;
        }
        const double px = pxt, py = pyt, pz = pzt, qx = mp.x, qy = mp.y, qz = mp.z, nx = mn.x, ny = mn.y, nz = mn.z;
        const double rr = sqrt((px * px + py * py) + pz * pz);
        const double rdx = px / rr, rdy = py / rr, rdz = pz / rr;
        const double qr = sqrt((qx * qx + qy * qy) + qz * qz);
        const double qdx = qx / qr, qdy = qy / qr, qdz = qz / qr;
        const double n_alpha = nz * rdy - ny * rdz;
        const double n_beta = nx * rdz - nz * rdx;
        const double n_gamma = ny * rdx - nx * rdy;
        double E = nx * (px - gamma * py + beta * pz + t_x - qx);
        E += ny * (gamma * px + py - alpha * pz + t_y - qy);
        E += nz * (-beta * px + alpha * py + pz + t_z - qz);
        double Nr = nx * (rdx - gamma * rdy + beta * rdz);
        Nr += ny * (gamma * rdx + rdy - alpha * rdz);
        Nr += nz * (-beta * rdx + alpha * rdy + rdz);
        const double Nq = -((nx * qdx + ny * qdy) + nz * qdz);
        const double er = E + rr * Nr;
        const double h[6] = {nx, ny, nz, rr * n_alpha, rr * n_beta, rr * n_gamma};
        const double gr[6] = {nx * Nr, ny * Nr, nz * Nr, n_alpha * er, n_beta * er, n_gamma * er};
        const double gq[6] = {nx * Nq, ny * Nq, nz * Nq, qr * n_alpha * Nq, qr * n_beta * Nq, qr * n_gamma * Nq};
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) {
                acc[k] += h[a] * h[b];
                acc[21 + k] += gr[a] * gr[b] + gq[a] * gq[b];
                k++;
            }
    }
    }
    block_reduce_store<kCovTerms>(acc, partials + ((long long)blockIdx.y * max_blocks + blockIdx.x) * kCovTerms);
}


// ---------------------------------------------------------------------------
// RobustOutlierFilter's scale (round 5).  The chain's distance filter is the robust one: nothing is trimmed, so the matcher's
// lazy path must resolve every queued query -- k_robust_open lifts the threshold the lazy path works up to to +inf right after
// the iteration's first selection.  With scaleEstimator "mad": the median of the finite squared distances (the selection at
// ratio 0.5: element size / 2), the absolute deviations from it (k_robust_absdev), their median the same way; k_robust_finish
// turns it into the squared scale upstream divides by: the rounded root, squared, in T.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_robust_open(ProblemDev *__restrict__ probs, const int *__restrict__ active, int n_active)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_active) return;
    ProblemDev &P = probs[active[a]];
    if (P.done) return;
    P.limit = __longlong_as_double(0x7FF0000000000000LL);
    P.rlimit = P.limit;
}
// [EXT] GenericDescriptorOutlierFilter, soft mode.  k_gd_open: as k_robust_open (the maximum covers every pair with a neighbour:
// the lazy path must resolve every queued query) and the second selection must run whatever the lazy path refined -- it restores
// the iteration's threshold.  k_gd_max: the maximum value over the pairs with a neighbour -> ProblemDev::gd_key (values >= 0:
// their bits order as the values do; -0 counts as 0).
__global__ __launch_bounds__(64) void k_gd_open(ProblemDev *__restrict__ probs, const int *__restrict__ active, int n_active)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_active) return;
    ProblemDev &P = probs[active[a]];
    if (P.done) return;
    P.limit = __longlong_as_double(0x7FF0000000000000LL);
    P.rlimit = P.limit;
    P.n_refined = 1;
}
constexpr int kGdMaxItems = 16;       // pairs per thread of k_gd_max
template <typename T>
__global__ __launch_bounds__(256) void k_gd_max(ProblemDev *__restrict__ probs, const MapDev<T> *__restrict__ maps,
                                                const int *__restrict__ slot, const int *__restrict__ active)
{
    using U = typename Bits<T>::U;
    ProblemDev &P = probs[active[blockIdx.y]];
    if (P.done) return;
    const int np = pairs_n(P);
    const int base = blockIdx.x * (256 * kGdMaxItems);
    if (base >= np) return;
    const MapDev<T> M = maps[P.map];
    const long long poff = pairs_off(P);
    int ss[kGdMaxItems];
#pragma unroll
    for (int it = 0; it < kGdMaxItems; it++) {
        const int e = base + it * 256 + threadIdx.x;
        ss[it] = e < np ? slot[poff + e] : -1;
    }
    U k = 0;
#pragma unroll
    for (int it = 0; it < kGdMaxItems; it++)
        if (ss[it] >= 0) { const T v = M.val[ss[it] - M.first]; if (v > (T)0) k = max(k, Bits<T>::key(v)); }
    __shared__ U red[4];
    for (int o = 32; o > 0; o >>= 1) { const U t = __shfl_xor(k, o); k = t > k ? t : k; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) k = red[w] > k ? red[w] : k;
        if (k) atomicMax(&P.gd_key, (unsigned long long)k);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_robust_absdev(const ProblemDev *__restrict__ probs, const T *__restrict__ d2, T *__restrict__ dev,
                                                       const int *__restrict__ active)
{
    const ProblemDev &P = probs[active[blockIdx.y]];
    if (P.done) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= pairs_n(P)) return;
    const T med = (T)P.qraw, v = d2[pairs_off(P) + e];
    dev[pairs_off(P) + e] = v > med ? v - med : med - v;               // (+inf stays +inf: not a value of the selection)
}
// The scale of an iteration, problem by problem (pgicp_robust.h): it = iters + 1 is the problem's iteration, estimated while
// nb == 0 || it <= nb and held afterwards (ProblemDev::robust_s carries it from iteration to iteration, in T).  mad: the rounded
// root of the second median (P.qraw, launch_robust_scale); berg: T(1.9) times the rounded root of the median in the first
// iteration, then the recurrence towards the target.  `count`: no selection ran in this iteration -- k_robust_count follows and
// adds the pairs with a neighbour up in n_finite, which is cleared here.
template <typename T>
__global__ __launch_bounds__(64) void k_robust_finish(ProblemDev *__restrict__ probs, const int *__restrict__ active, int n_active, RobustDev<T> rb, T outlier_max_d2,
                                                      int count)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_active) return;
    ProblemDev &P = probs[active[a]];
    if (P.done) return;
    const int it = P.iters + 1;
    const bool estimate = rb.nb == 0 || it <= rb.nb;
    T s = (T)P.robust_s;
    if (rb.est == 0) s = (T)1;
    else if (estimate) {
        if (rb.est == 1) s = sqrt_rn_t((T)P.qraw);
        else if (it == 1) s = (T)1.9 * sqrt_rn_t((T)P.qraw);
        else s = (T)0.85 * (s - rb.target) + rb.target;
    }
    P.robust_s = (double)s;
    P.robust_s2 = (double)(s * s);
    if (count) P.n_finite = 0;
    // a MaxDistOutlierFilter beside the robust one still cuts (the weights multiply): the minimiser's `dist <= limit`; the NEXT
    // pass of the matcher must again find every pair exactly (the medians are over all finite distances): no search cap
    P.limit = (double)outlier_max_d2;
    P.rlimit = __longlong_as_double(0x7FF0000000000000LL);
    P.n_refined = 0;
}
// a held iteration's count of the pairs with a neighbour (what a selection leaves in n_finite): an integer sum, no order in it
constexpr int kRobustCountItems = 16;       // pairs per thread of k_robust_count
template <typename T>
__global__ __launch_bounds__(256) void k_robust_count(ProblemDev *__restrict__ probs, const T *__restrict__ d2, const int *__restrict__ active)
{
    ProblemDev &P = probs[active[blockIdx.y]];
    if (P.done) return;
    const int np = pairs_n(P);
    const int base = blockIdx.x * (256 * kRobustCountItems);
    if (base >= np) return;
    const long long poff = pairs_off(P);
    // wave ballot and popcount, one integer add a wave (as k_noise_count counts): no LDS
    int cnt = 0;
#pragma unroll
    for (int it = 0; it < kRobustCountItems; it++) {
        const int e = base + it * 256 + threadIdx.x;
        cnt += __popcll(__ballot(e < np && d2[poff + e] != Bits<T>::inf()));
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&P.n_finite, cnt);
}

// stage-level RobustOutlierFilter::compute over one raw array of squared distances (pgicp_outlier_weights): stat[0] the median,
// stat[1] the finite count, stat[2] the median absolute deviation (k_trim_select_raw at ratio 0.5, twice)
template <typename T>
__global__ __launch_bounds__(256) void k_robust_absdev_raw(const T *__restrict__ d2, int n, const T *__restrict__ stat, T *__restrict__ dev)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T med = stat[0], v = d2[i];
    dev[i] = v > med ? v - med : med - v;
}
template <typename T>
__global__ __launch_bounds__(256) void k_robust_weights_raw(const T *__restrict__ d2, int n, RobustDev<T> rb, const T *__restrict__ stat,
                                                             T *__restrict__ w)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T s2 = (T)1;
    if (rb.est == 2) { const T sc = (T)1.9 * sqrt_rn_t(stat[0]); s2 = sc * sc; }        // (berg, iteration 1: pgicp_robust.h)
    else if (rb.mad) { const T sc = sqrt_rn_t(stat[2]); s2 = sc * sc; }
    const T v = d2[i];
    w[i] = v == __builtin_huge_val() ? (T)0 : robust_weight<T>(rb, v, s2);      // (no neighbour: never an error element)
}


// pgicp_map_set_values: the caller's values (original point order, values[i * stride]) into the map's slot order; flags[0]: a
// non-finite value was met, flags[1]: a negative one
template <typename T>
__global__ __launch_bounds__(256) void k_map_values(const typename Vec4<T>::type *__restrict__ pts, int first, int m,
                                                    const T *__restrict__ values, int stride, T *__restrict__ out, int *__restrict__ flags)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    const T v = values[(long long)Bits<T>::unpack_idx(pts[first + s].w) * stride];
    out[s] = v;
    if (!isfinite(v)) atomicOr(flags, 1);
    else if (v < (T)0) atomicOr(flags + 1, 1);
}
