// k_noise.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): SimpleSensorNoiseDataPointsFilter's
// descriptor and the sensor-noise branch of getOverlap() over the last error elements (include/pgicp_noise.h).

// noise(i) of orc_simple_sensor_noise (oracle/icp_oracle.c), the same expressions in T, no contraction: r2 = (x x + y y) + z z,
// the rounded root, max(minRadius, angle r + cst) -- type 3: (r r) * T(0.5 * 0.00285) -- times gain
template <typename T>
__global__ __launch_bounds__(256) void k_simple_sensor_noise(const T *__restrict__ xyz, int stride, int n, int sensor_type, T min_r, T angle,
                                                             T cst, T gain, T *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T *p = xyz + (long long)i * stride;
    const T x = p[0], y = p[1], z = p[2];
    const T r2 = (x * x + y * y) + z * z;
    T v;
    if (sensor_type == 3) { const T r = sqrt_rn_t(r2); v = (r * r) * (T)(0.5 * 0.00285); }
    else { v = angle * sqrt_rn_t(r2) + cst; if (v < min_r) v = min_r; }
    out[i] = gain * v;
}

// pgicp_arm_reading_noise, device input: one problem's values (src[i * stride]) into the context's packed copy; flag: a value
// that is negative or not finite was met
template <typename T>
__global__ __launch_bounds__(256) void k_noise_stage(const T *__restrict__ src, int stride, int n, T *__restrict__ dst, int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T v = src[(long long)i * stride];
    dst[i] = v;
    if (!(v >= (T)0) || !isfinite(v)) atomicOr(flag, 1);
}

// Pass 1 over the LAST iteration's error elements of every armed problem: a pair is kept as k_p2plane_reduce kept it in that
// iteration (has a neighbour, d2 <= limit, pair_filter_weight != 0 with the transform and the soft maximum that iteration ran
// with: T_prev, gd_last -- what k_cov_reduce reads too).  dist_out[pair] = sqrt(d2) in T for a kept pair, -1 otherwise; block
// partials {sum of dist, number kept} in double at the pair's position of the reduction tree RT-1 (thread t of tree block
// `tile` adds positions tile * kReduceSpan + u * 256 + t, u = 0 .. 7, in that order; block_reduce_store is T3 + T4,
// k_sum_partials T5), the tree position being a sorted position or -- scan_pos -- a position in the caller's reading.
template <typename T>
__global__ __launch_bounds__(kReduceBlock) void k_noise_sum(const ProblemDev *__restrict__ probs, const MapDev<T> *__restrict__ maps,
                                                             const T *__restrict__ rd_pre, const T *__restrict__ rd_nrm, const int *__restrict__ slot,
                                                             const T *__restrict__ d2, const long long *__restrict__ noise_off,
                                                             T *__restrict__ dist_out, double *__restrict__ partials, int max_blocks,
                                                             T normal_cos, RobustDev<T> rb, const int *__restrict__ scan_pos, int gd_mode,
                                                             T gd_thr)
{
    const int prob = blockIdx.y;
    const ProblemDev &P = probs[prob];
    if (P.status != PGICP_ST_OK || noise_off[prob] < 0) return;
    const int np = pairs_n(P), knn = P.knn;
    const long long poff = pairs_off(P);
    const int tile = blockIdx.x;
    if (tile * kReduceSpan >= np) return;
    const MapDev<T> M = maps[P.map];
    const T limit = (T)P.limit;
    const bool use_nrm = rd_nrm != nullptr;
    const bool robust = rb.fct != 0;
    const bool plane_dd = robust && rb.dist != 0;      // (pgicp_robust.h: the robust weights saw plane distances)
    const bool gd = gd_mode != PGICP_DESC_FILTER_OFF;
    const T rs2 = (T)P.robust_s2;
    const T gmax = Bits<T>::val((typename Bits<T>::U)P.gd_last);
    double Tp[12];
#pragma unroll
    for (int k = 0; k < 12; k++) Tp[k] = P.T_prev[k];
    double acc[2] = {0.0, 0.0};
    for (int u = 0; u < kReduceItems * kReduceRounds; u++) {
        const int pos = tile * kReduceSpan + u * kReduceBlock + threadIdx.x;
        if (pos >= np) continue;
        const int e = !scan_pos ? pos : knn == 1 ? scan_pos[P.off + pos] : scan_pos[P.off + pos / knn] * knn + pos % knn;
        const T dd = d2[poff + e];
        const int s = slot[poff + e];
        T dist = (T)-1;
        if (s >= 0 && dd <= limit) {
            const int i = knn == 1 ? e : e / knn;
            T bx = (T)0, by = (T)0, bz = (T)0;
            if (use_nrm || plane_dd) { const auto mn = M.nrm[2 * (long long)s + 1]; bx = mn.x; by = mn.y; bz = mn.z; }
            T rdd = dd;
            if (plane_dd) {
                const auto mp = M.nrm[2 * (long long)s];
                const T *q = rd_pre + 3 * (P.off + i);
                rdd = robust_pair_dd<T>(rb, dd, Tp, q[0], q[1], q[2], mp.x, mp.y, mp.z, bx, by, bz);
            }
            const T w = pair_filter_weight<T>(Tp, use_nrm, use_nrm ? rd_nrm + 3 * (P.off + i) : nullptr, bx, by, bz, normal_cos, robust, rb, rdd, rs2, gd, gd_mode,
                                              gd_thr, gd ? M.val[s - M.first] : (T)0, gmax);
            if (w != (T)0) {
                dist = sqrt_rn_t(dd);
                acc[0] += (double)dist;
                acc[1] += 1.0;
            }
        }
        dist_out[poff + e] = dist;
    }
    block_reduce_store<2>(acc, partials + ((long long)prob * max_blocks + tile) * 2);
}

// Pass 2: mean = T(S / nb); the kept pairs with dist < mean + noise(point), comparison and addition in T.  An integer count:
// wave ballot and popcount, one integer add a block -- no order to depend on.  sums: {S, nb} per problem (k_sum_partials).
template <typename T>
__global__ __launch_bounds__(256) void k_noise_count(const ProblemDev *__restrict__ probs, const T *__restrict__ dist,
                                                     const int *__restrict__ order, const T *__restrict__ noise,
                                                     const long long *__restrict__ noise_off, const double *__restrict__ sums,
                                                     int *__restrict__ count)
{
    const int prob = blockIdx.y;
    const ProblemDev &P = probs[prob];
    const long long noff = noise_off[prob];
    if (P.status != PGICP_ST_OK || noff < 0) return;
    const int np = pairs_n(P), knn = P.knn;
    if ((int)blockIdx.x * 256 >= np) return;
    const T mean = (T)(sums[2 * prob] / sums[2 * prob + 1]);
    const int e = blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (e < np) {
        const T d = dist[pairs_off(P) + e];
        if (d >= (T)0) {
            const int i = knn == 1 ? e : e / knn;
            in = d < mean + noise[noff + order[P.off + i]];
        }
    }
    const unsigned long long b = __ballot(in);
    __shared__ int wc[4];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = (wc[0] + wc[1]) + (wc[2] + wc[3]);
        if (c) atomicAdd(count + prob, c);
    }
}

template <typename T>
void launch_simple_sensor_noise(hipStream_t st, const T *xyz, int stride, int n, int sensor_type, T min_r, T angle, T cst, T gain, T *out)
{
    hipLaunchKernelGGL(k_simple_sensor_noise<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, xyz, stride, n, sensor_type, min_r, angle, cst, gain, out);
}
template <typename T>
void launch_noise_stage(hipStream_t st, const T *src, int stride, int n, T *dst, int *flag)
{
    hipLaunchKernelGGL(k_noise_stage<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, src, stride, n, dst, flag);
}
// out: {S, nb} per problem (2 P doubles); count: P ints, zero on entry (the caller clears them on the same stream)
template <typename T>
void launch_noise_overlap(hipStream_t st, const ProblemDev *probs, const MapDev<T> *maps, const T *rd_pre, const T *rd_nrm, const int *slot, const T *d2,
                          const int *order, const T *noise, const long long *noise_off, T *dist, double *partials, double *out, int *count,
                          int P, int max_pairs, const ChainDev<T> &ch)
{
    const int nb = reduce_blocks(max_pairs);
    hipLaunchKernelGGL(k_noise_sum<T>, dim3(nb, P), dim3(kReduceBlock), 0, st, probs, maps, rd_pre, rd_nrm, slot, d2, noise_off, dist, partials, nb,
                       ch.normal_cos, ch.robust, ch.scan_pos, ch.gd_mode, ch.gd_thr);
    hipLaunchKernelGGL(k_sum_partials, dim3(P), dim3(256), 0, st, (const double *)partials, nb, 2, probs, 0, out);
    hipLaunchKernelGGL(k_noise_count<T>, dim3(cdiv(max_pairs, 256), P), dim3(256), 0, st, probs, (const T *)dist, order, noise, noise_off,
                       (const double *)out, count);
}

#define INSTANTIATE_NOISE(T)                                                                                                           \
    template void launch_simple_sensor_noise<T>(hipStream_t, const T *, int, int, int, T, T, T, T, T *);                               \
    template void launch_noise_stage<T>(hipStream_t, const T *, int, int, T *, int *);                                                 \
    template void launch_noise_overlap<T>(hipStream_t, const ProblemDev *, const MapDev<T> *, const T *, const T *, const int *, const T *, \
                                          const int *, const T *, const long long *, T *, double *, double *, int *, int, int,         \
                                          const ChainDev<T> &);
INSTANTIATE_NOISE(float)
INSTANTIATE_NOISE(double)
#undef INSTANTIATE_NOISE
