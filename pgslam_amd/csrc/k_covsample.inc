// k_covsample.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp):
// CovarianceSamplingDataPointsFilter (statement: include/pgicp_covsample.h).
//
//   pass 1  k_cov_reduce<1>: coordinate sums, the count of points with a non-finite input, -min / max of each axis;
//   pass 2  k_cov_reduce<2>: the sum of |x - c| (torqueNorm 1 only);
//   pass 3  k_cov_reduce<3>: the 21 distinct sums of C = sum f f^T.
//           Each is a grid-stride pass of at most kCovBlocks blocks: lane -> wave (shuffles) -> block (LDS) -> one row of partials,
//           then k_cov_fold sums the rows in a fixed tree (one block a value), as k_p2plane_reduce / sum_partials_256 do: no atomics
//           on doubles, the same bits from run to run.  The sums behind c and L are cascaded (cov_dd_add).  k_cov_finish (one
//           thread) turns the folded sums into c, L and 1 / L, which the next pass reads from device memory, so the host waits
//           once for the whole frame.
//   pass 4  k_cov_values: v (n x 6) and the histogram of each list's top key byte.  The keys are the values' bit patterns (v >= 0:
//           their unsigned order is the values').  Per further byte k_cov_hist counts the keys under the prefix found so far and
//           k_cov_pick (one wave a list) walks the 256 counts from the top: after the last byte prefix = the nbSample-th largest
//           key and rank = how many of its ties belong to the list.  k_cov_flag marks the ties, ONE scan ranks them (any number:
//           a planar cloud makes a whole list equal), k_cov_emit writes each list's entries through a cursor -- in no order: the
//           host sorts them by (value, index), a total order.
//   pass 5  k_gather_rows: the picks' coordinates, normals and descriptor rows (NormalSpace's gather too, through its sort).

template <int MODE> struct CovMode;
// nv values a row of partials, the first nsum of them sums (the rest maxima), the first ndd of those carried as (sum, error):
// a row holds nv + ndd doubles, the error terms last
template <> struct CovMode<1> { static constexpr int nv = 10, nsum = 4, ndd = 3; };
template <> struct CovMode<2> { static constexpr int nv = 1, nsum = 1, ndd = 1; };
template <> struct CovMode<3> { static constexpr int nv = kCovSums, nsum = kCovSums, ndd = 0; };

// The sums behind c and L are cascaded (Knuth's two-sum, the rounding errors summed apart): c and L then are the exact sums'
// roundings for every order of summation, which a plain double sum is not once T is double (its n 2^-53 is n/2 eps of T).
__device__ __forceinline__ void cov_dd_add(double &hi, double &lo, double v, double vlo)
{
    const double s = hi + v, bb = s - hi;
    lo += ((hi - (s - bb)) + (v - bb)) + vlo;
    hi = s;
}

template <typename T>
__device__ __forceinline__ bool cov_finite(T v) { return fabs(v) <= std::numeric_limits<T>::max(); }

// f of a point (the statement's "per point", in T)
template <typename T>
__device__ __forceinline__ void cov_f(const T *__restrict__ x, const T *__restrict__ nr, T c0, T c1, T c2, T inv, T f[6])
{
    const T px = x[0] - c0, py = x[1] - c1, pz = x[2] - c2;
    const T nx = nr[0], ny = nr[1], nz = nr[2];
    const T cx = py * nz - pz * ny, cy = pz * nx - px * nz, cz = px * ny - py * nx;
    f[0] = inv * cx; f[1] = inv * cy; f[2] = inv * cz; f[3] = nx; f[4] = ny; f[5] = nz;
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_cov_reduce(const T *__restrict__ X, int xs, const T *__restrict__ N, int ns, int n,
                                                    const CovStat *__restrict__ stat, double *__restrict__ part)
{
    constexpr int NV = CovMode<MODE>::nv, NSUM = CovMode<MODE>::nsum, NDD = CovMode<MODE>::ndd;
    double a[NV], lo[NDD + 1];
#pragma unroll
    for (int k = 0; k < NV; k++) a[k] = k < NSUM ? 0.0 : -HUGE_VAL;
#pragma unroll
    for (int k = 0; k <= NDD; k++) lo[k] = 0.0;
    T c0 = 0, c1 = 0, c2 = 0, inv = 0;
    if constexpr (MODE != 1) { c0 = (T)stat->c[0]; c1 = (T)stat->c[1]; c2 = (T)stat->c[2]; inv = (T)stat->inv; }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const T *x = X + i * xs;
        if constexpr (MODE == 1) {
            const T *nr = N + i * ns;
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double v = (double)x[k];
                ok = ok && cov_finite(x[k]) && cov_finite(nr[k]);
                cov_dd_add(a[k], lo[k], v, 0.0);
                a[4 + k] = -v > a[4 + k] ? -v : a[4 + k];
                a[7 + k] = v > a[7 + k] ? v : a[7 + k];
            }
            if (!ok) a[3] += 1.0;
        } else if constexpr (MODE == 2) {
            const T dx = x[0] - c0, dy = x[1] - c1, dz = x[2] - c2;
            cov_dd_add(a[0], lo[0], (double)sqrt((dx * dx + dy * dy) + dz * dz), 0.0);
        } else {
            T f[6];
            cov_f<T>(x, N + i * ns, c0, c1, c2, inv, f);
            int q = 0;
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int s = r; s < 6; s++) a[q++] += (double)f[r] * (double)f[s];
        }
    }
    __shared__ double red[4][NV + NDD];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        double v = a[k];
        if (k < NDD) {
            double e = lo[k];
            for (int o = 32; o > 0; o >>= 1) { const double tv = __shfl_down(v, o, 64), te = __shfl_down(e, o, 64); cov_dd_add(v, e, tv, te); }
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][NV + k] = e;
        } else if (k < NSUM) v = wave_sum(v);
        else
            for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_down(v, o, 64); v = t > v ? t : v; }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int k = threadIdx.x;
        double *row = part + (long long)blockIdx.x * (NV + NDD);
        double v;
        if (k < NDD) {
            double e = red[0][NV + k];
            v = red[0][k];
            for (int w = 1; w < 4; w++) cov_dd_add(v, e, red[w][k], red[w][NV + k]);
            row[NV + k] = e;
        } else if (k < NSUM) v = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        else { v = red[0][k]; for (int w = 1; w < 4; w++) v = red[w][k] > v ? red[w][k] : v; }
        row[k] = v;
    }
}

// out[k] = the sum (k < nsum; cascaded for k < ndd) or the maximum of part[b][k] over the nb rows: one block a value, a fixed tree
__global__ __launch_bounds__(256) void k_cov_fold(const double *__restrict__ part, int nb, int nv, int nsum, int ndd, double *__restrict__ out)
{
    const int k = blockIdx.x, stride = nv + ndd;
    const bool sum = k < nsum, dd = k < ndd;
    double v = sum ? 0.0 : -HUGE_VAL, e = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) {
        const double t = part[(long long)b * stride + k];
        if (dd) cov_dd_add(v, e, t, part[(long long)b * stride + nv + k]);
        else v = sum ? v + t : (t > v ? t : v);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_down(v, o, 64), te = __shfl_down(e, o, 64);
        if (dd) cov_dd_add(v, e, t, te);
        else v = sum ? v + t : (t > v ? t : v);
    }
    __shared__ double red[4], rede[4];
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = v; rede[threadIdx.x >> 6] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (dd) { for (int w = 1; w < 4; w++) cov_dd_add(v, e, red[w], rede[w]); v = v + e; }
        else if (sum) v = (red[0] + red[1]) + (red[2] + red[3]);
        else for (int w = 1; w < 4; w++) v = red[w] > v ? red[w] : v;
        out[k] = v;
    }
}

// stage 1 (after pass 1): c, and L of torqueNorm 0 / 2; stage 2 (after pass 2): L of torqueNorm 1.  One thread.
template <typename T>
__global__ void k_cov_finish(CovStat *__restrict__ stat, int n, int torque_norm, int stage)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    T L = (T)1;
    if (stage == 1) {
        for (int a = 0; a < 3; a++) stat->c[a] = (double)(T)(stat->r1[a] / (double)n);
        if (torque_norm == 2) {
            T e = (T)stat->r1[7] - (T)(-stat->r1[4]);
            for (int a = 1; a < 3; a++) { const T ea = (T)stat->r1[7 + a] - (T)(-stat->r1[4 + a]); if (ea > e) e = ea; }
            L = (T)0.5 * e;
        }
    } else
        L = (T)(stat->nsum / (double)n);
    stat->L = (double)L;
    stat->inv = (double)((T)1 / L);
}

// one count into an LDS histogram of 256 bins; every lane of the wave calls it (`on`: this lane has a key).  A wave whose keys
// share the bin -- a plane's zeros, a sorted run -- adds once
__device__ __forceinline__ void cov_count(int *__restrict__ h, bool on, int d)
{
    const unsigned long long act = __ballot(on);
    if (act == 0) return;
    const int first = __ffsll((long long)act) - 1;
    const int d0 = __shfl(d, first, 64);
    if (__ballot(on && d == d0) == act) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[d0], __popcll(act));
    } else if (on)
        atomicAdd(&h[d], 1);
}
__device__ __forceinline__ void cov_hist_flush(const int *__restrict__ h, int *__restrict__ hist)
{
    __syncthreads();
    for (int j = threadIdx.x; j < 6 * 256; j += 256)
        if (h[j]) atomicAdd(&hist[j], h[j]);
}

constexpr int kCovHistBlocks = 512;
template <typename T>
__global__ __launch_bounds__(256) void k_cov_values(const T *__restrict__ X, int xs, const T *__restrict__ N, int ns, int n, const CovFrameDev<T> F,
                                                    T *__restrict__ v, int *__restrict__ hist, CovStat *__restrict__ stat)
{
    __shared__ int h[6 * 256];
    for (int j = threadIdx.x; j < 6 * 256; j += 256) h[j] = 0;
    __syncthreads();
    bool bad = false;
    // (every lane of a wave makes the same number of rounds: cov_count is a wave operation)
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        const bool on = i < n;
        T f[6] = {0, 0, 0, 0, 0, 0};
        if (on) {
            const T *x = X + i * xs, *nr = N + i * ns;
            bad = bad || !(cov_finite(x[0]) && cov_finite(x[1]) && cov_finite(x[2]) && cov_finite(nr[0]) && cov_finite(nr[1]) && cov_finite(nr[2]));
            cov_f<T>(x, nr, F.c[0], F.c[1], F.c[2], F.inv, f);
        }
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const T *Xk = F.X + 6 * k;
            const T vk = fabs(((((f[0] * Xk[0] + f[1] * Xk[1]) + f[2] * Xk[2]) + f[3] * Xk[3]) + f[4] * Xk[4]) + f[5] * Xk[5]);
            if (on) v[i * 6 + k] = vk;
            cov_count(h + 256 * k, on, (int)(Bits<T>::key(vk) >> (Bits<T>::kBits - 8)));
        }
    }
    if (bad) stat->bad = 1;
    cov_hist_flush(h, hist);
}

// byte `pass` (1 .. sizeof(T) - 1, from the top) of the keys that carry their list's prefix
template <typename T>
__global__ __launch_bounds__(256) void k_cov_hist(const T *__restrict__ v, int n, int pass, const CovStat *__restrict__ stat, int *__restrict__ hist)
{
    using U = typename Bits<T>::U;
    __shared__ int h[6 * 256];
    for (int j = threadIdx.x; j < 6 * 256; j += 256) h[j] = 0;
    __syncthreads();
    const int shift = Bits<T>::kBits - 8 * (pass + 1);
    U pre[6];
#pragma unroll
    for (int k = 0; k < 6; k++) pre[k] = (U)stat->prefix[k] >> (shift + 8);
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        const bool on = i < n;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const U key = on ? Bits<T>::key(v[i * 6 + k]) : (U)0;
            cov_count(h + 256 * k, on && (key >> (shift + 8)) == pre[k], (int)((key >> shift) & 255));
        }
    }
    cov_hist_flush(h, hist);
}

// one wave a list: the byte of the rank-th largest key under the prefix.  Lane l holds bins 4 l .. 4 l + 3; a suffix sum over the
// lanes finds the one lane whose bins hold the rank
template <typename T>
__global__ __launch_bounds__(384) void k_cov_pick(const int *__restrict__ hist, int pass, int m, CovStat *__restrict__ stat)
{
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int *h = hist + 256 * k + 4 * lane;
    const int c[4] = {h[0], h[1], h[2], h[3]};
    const int own = (c[0] + c[1]) + (c[2] + c[3]);
    int incl = own;                                     // the counts of this lane's bins and every bin above them
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(incl, o, 64); if (lane + o < 64) incl += t; }
    const int rank = pass == 0 ? m : stat->rank[k];
    const int above = incl - own;
    if (above < rank && rank <= incl) {
        int r = rank - above, d = 3;
        for (; d > 0; d--) { if (c[d] >= r) break; r -= c[d]; }
        const int shift = Bits<T>::kBits - 8 * (pass + 1);
        const unsigned long long pre = pass == 0 ? 0ULL : stat->prefix[k];
        stat->prefix[k] = pre | ((unsigned long long)(4 * lane + d) << shift);
        stat->rank[k] = r;
    }
}

// eq[k n + i] = v_ik is a tie of list k's threshold
template <typename T>
__global__ __launch_bounds__(256) void k_cov_flag(const T *__restrict__ v, int n, const CovStat *__restrict__ stat, int *__restrict__ eq)
{
    using U = typename Bits<T>::U;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int k = 0; k < 6; k++) eq[(long long)k * n + i] = Bits<T>::key(v[i * 6 + k]) == (U)stat->prefix[k] ? 1 : 0;
}

// list k takes the keys above its threshold and the rank[k] lowest-index ties: m entries in all
template <typename T>
__global__ __launch_bounds__(256) void k_cov_emit(const T *__restrict__ v, int n, int m, CovStat *__restrict__ stat, const int *__restrict__ pos,
                                                  int *__restrict__ cand_idx, T *__restrict__ cand_v)
{
    using U = typename Bits<T>::U;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n;
    const int lane = threadIdx.x & 63;
    T vi[6] = {0, 0, 0, 0, 0, 0};
    if (on)
#pragma unroll
        for (int k = 0; k < 6; k++) vi[k] = v[i * 6 + k];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const U key = Bits<T>::key(vi[k]), thr = (U)stat->prefix[k];
        bool take = on && key > thr;
        if (on && key == thr) take = pos[(long long)k * n + i] - pos[(long long)k * n] < stat->rank[k];
        const unsigned long long mask = __ballot(take);
        if (mask == 0) continue;
        const int first = __ffsll((long long)mask) - 1;
        int slot = 0;
        if (lane == first) slot = atomicAdd(&stat->cursor[k], __popcll(mask));
        slot = __shfl(slot, first, 64) + __popcll(mask & ((1ULL << lane) - 1ULL));
        if (take && slot < m) {
            const long long o = (long long)k * m + slot;
            cand_idx[o] = (int)i;
#pragma unroll
            for (int q = 0; q < 6; q++) cand_v[o * 6 + q] = vi[q];
        }
    }
}

// out[j] = in[i]: i = pos[j], or -- through a pair sort's result -- i = sidx[pos[j]] with the bucket skey[pos[j]] >> 24
template <typename T>
__global__ __launch_bounds__(256) void k_gather_rows(const int *__restrict__ pos, const unsigned long long *__restrict__ skey, const int *__restrict__ sidx,
                                                     int m, int n, const T *__restrict__ X, int xs, const T *__restrict__ N, int ns,
                                                     const T *__restrict__ desc, int drows, T *__restrict__ out_xyz, int os, T *__restrict__ out_nrm,
                                                     int ons, T *__restrict__ out_desc, int *__restrict__ kept_idx, int *__restrict__ bucket_out)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    long long i = pos ? pos[j] : j;
    int b = -1;
    if (pos && sidx) {
        if (i < 0 || i >= n) return;
        b = (int)(skey[i] >> 24);
        i = sidx[i];
    }
    if (i < 0 || i >= n) return;
    if (out_xyz) { const T *x = X + i * xs; T *o = out_xyz + j * os; o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; }
    if (out_nrm) { const T *x = N + i * ns; T *o = out_nrm + j * ons; o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; }
    if (out_desc)
        for (int r = 0; r < drows; r++) out_desc[j * drows + r] = desc[i * drows + r];
    if (kept_idx) kept_idx[j] = (int)i;
    if (bucket_out) bucket_out[j] = b;
}

// ---- launchers ----
template <typename T, int MODE>
static void cov_reduce(hipStream_t st, const T *X, int xs, const T *N, int ns, int n, const CovScratch &w, CovStat *stat, double *out)
{
    const int nb = std::min(cdiv(n, 256), kCovBlocks);
    hipLaunchKernelGGL((k_cov_reduce<T, MODE>), dim3(nb), dim3(256), 0, st, X, xs, N, ns, n, (const CovStat *)stat, w.part);
    hipLaunchKernelGGL(k_cov_fold, dim3(CovMode<MODE>::nv), dim3(256), 0, st, (const double *)w.part, nb, CovMode<MODE>::nv, CovMode<MODE>::nsum,
                       CovMode<MODE>::ndd, out);
}

template <typename T>
void launch_cov_frame(hipStream_t st, const T *X, int xs, const T *N, int ns, int n, int torque_norm, const CovScratch &w, CovStat *stat)
{
    cov_reduce<T, 1>(st, X, xs, N, ns, n, w, stat, stat->r1);
    hipLaunchKernelGGL(k_cov_finish<T>, dim3(1), dim3(64), 0, st, stat, n, torque_norm, 1);
    if (torque_norm == 1) {
        cov_reduce<T, 2>(st, X, xs, N, ns, n, w, stat, &stat->nsum);
        hipLaunchKernelGGL(k_cov_finish<T>, dim3(1), dim3(64), 0, st, stat, n, torque_norm, 2);
    }
    cov_reduce<T, 3>(st, X, xs, N, ns, n, w, stat, stat->sums);
}

template <typename T>
void launch_cov_select(hipStream_t st, const T *X, int xs, const T *N, int ns, int n, const CovFrameDev<T> &F, int m, const CovScratch &w, CovStat *stat)
{
    constexpr int passes = (int)sizeof(T);
    const int nb = std::min(cdiv(n, 256), kCovHistBlocks);
    T *v = (T *)w.v;
    (void)hipMemsetAsync(w.hist, 0, sizeof(int) * passes * 6 * 256, st);
    hipLaunchKernelGGL(k_cov_values<T>, dim3(nb), dim3(256), 0, st, X, xs, N, ns, n, F, v, w.hist, stat);
    hipLaunchKernelGGL(k_cov_pick<T>, dim3(1), dim3(384), 0, st, (const int *)w.hist, 0, m, stat);
    for (int p = 1; p < passes; p++) {
        int *h = w.hist + p * 6 * 256;
        hipLaunchKernelGGL(k_cov_hist<T>, dim3(nb), dim3(256), 0, st, (const T *)v, n, p, (const CovStat *)stat, h);
        hipLaunchKernelGGL(k_cov_pick<T>, dim3(1), dim3(384), 0, st, (const int *)h, p, m, stat);
    }
    const dim3 grid(cdiv(n, 256)), block(256);
    hipLaunchKernelGGL(k_cov_flag<T>, grid, block, 0, st, (const T *)v, n, (const CovStat *)stat, w.eq);
    launch_exclusive_scan(st, w.eq, 6 * n, w.pos, w.bsum);
    hipLaunchKernelGGL(k_cov_emit<T>, grid, block, 0, st, (const T *)v, n, m, stat, (const int *)w.pos, w.cand_idx, (T *)w.cand_v);
}

template <typename T>
void launch_gather_rows(hipStream_t st, const int *pos, const unsigned long long *skey, const int *sidx, int m, int n, const T *X, int xs, const T *N,
                        int ns, const T *desc, int drows, T *out_xyz, int os, T *out_nrm, int ons, T *out_desc, int *kept_idx, int *bucket_out)
{
    hipLaunchKernelGGL(k_gather_rows<T>, dim3(cdiv(m, 256)), dim3(256), 0, st, pos, skey, sidx, m, n, X, xs, N, ns, desc, drows, out_xyz, os, out_nrm, ons,
                       desc ? out_desc : (T *)nullptr, kept_idx, bucket_out);
}

#define INSTANTIATE_COVSAMPLE(T)                                                                                                       \
    template void launch_cov_frame<T>(hipStream_t, const T *, int, const T *, int, int, int, const CovScratch &, CovStat *);          \
    template void launch_cov_select<T>(hipStream_t, const T *, int, const T *, int, int, const CovFrameDev<T> &, int, const CovScratch &, \
                                       CovStat *);                                                                                   \
    template void launch_gather_rows<T>(hipStream_t, const int *, const unsigned long long *, const int *, int, int, const T *, int, const T *, \
                                        int, const T *, int, T *, int, T *, int, T *, int *, int *);
INSTANTIATE_COVSAMPLE(float)
INSTANTIATE_COVSAMPLE(double)
#undef INSTANTIATE_COVSAMPLE
