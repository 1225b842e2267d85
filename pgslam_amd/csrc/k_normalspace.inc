// k_normalspace.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): NormalSpaceDataPointsFilter.
//
// [EXT] libpointmatcher NormalSpaceDataPointsFilter as include/pgicp_normalspace.h states it.  The schedule:
//   1. k_ns_keys: one thread per point -- the bucket of its normal in double (the device library's acos, atan2 and fmod), the
//      not-finite flag, the key (bucket << 24) | r_i paired with the index, and the buckets' histogram with integer atomics: a
//      block counts its tile of 4096 points in LDS when the grid fits (kNsLdsBuckets) and adds its non-zero counts to the global
//      array, on the global array directly otherwise;
//   2. the stable LSD radix sort of (key, index) over the key's bits only: k_vox_hist / k_vox_scatter, unchanged.  The input is
//      in index order, so equal keys end in ascending index: ascending (bucket, r_i, i);
//   3. the host reads the counts and the flag, runs the draw (normalspace_host.hpp) and uploads per pick its position in the
//      sorted order, start[bucket] + rank;
//   4. k_ns_gather: one thread per pick writes index, bucket, coordinates, normal and descriptor rows.
// Wave64; no floating-point atomics.  The angles are double arithmetic: nothing here is under the contraction contract.

constexpr int kNsTile = 4096;        // points a block of k_ns_keys handles: 256 threads x 16 rounds

template <typename T, bool LDS>
__global__ __launch_bounds__(256) void k_ns_keys(const T *__restrict__ N, int ns, int n, NsGrid g, unsigned long long seed,
                                                 unsigned long long *__restrict__ key, int *__restrict__ idx, int *__restrict__ counts)
{
    __shared__ int cnt[LDS ? kNsLdsBuckets : 1];
    if (LDS) {
        for (int b = threadIdx.x; b < g.nb_bucket; b += 256) cnt[b] = 0;
        __syncthreads();
    }
    const double pi = 3.14159265358979323846;
    const long long base = (long long)blockIdx.x * kNsTile;
    for (int r = 0; r < kNsTile / 256; r++) {
        const long long i = base + r * 256 + threadIdx.x;
        if (i >= n) break;
        const T *p = N + i * ns;
        const double nx = (double)p[0], ny = (double)p[1], nz = (double)p[2];
        int b = 0;
        if (isfinite(nx) && isfinite(ny) && isfinite(nz)) {
            const double z = fmax(fmin(nz, 1.0), -1.0);
            double theta = acos(z);
            double phi = fmod(atan2(ny, nx) + 2.0 * pi, 2.0 * pi);
            if (theta == pi) theta = 0.0;
            if (phi == 2.0 * pi) phi = 0.0;
            int it = (int)floor(theta / g.epsilon), ip = (int)floor(phi / g.epsilon);
            it = min(max(it, 0), g.n_theta - 1);                       // (max: nothing finite gets there; it keeps b inside the grid)
            ip = min(max(ip, 0), g.n_phi - 1);
            b = it * g.n_phi + ip;
        } else
            atomicOr(&counts[g.nb_bucket], 1);                         // the flag sits behind the counts
        key[i] = ((unsigned long long)b << 24) | (splitmix(seed * 0x100000001B3ULL + (unsigned long long)i) >> 40);
        idx[i] = (int)i;
        if (LDS) atomicAdd(&cnt[b], 1);
        else atomicAdd(&counts[b], 1);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < g.nb_bucket; b += 256) {
            const int c = cnt[b];
            if (c) atomicAdd(&counts[b], c);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ns_gather(const int *__restrict__ pos, const unsigned long long *__restrict__ skey, const int *__restrict__ sidx,
                                                   int m, int n, const T *__restrict__ X, int xs, const T *__restrict__ N, int ns,
                                                   const T *__restrict__ desc, int drows, T *__restrict__ out_xyz, int os, T *__restrict__ out_nrm,
                                                   int ons, T *__restrict__ out_desc, int *__restrict__ kept_idx, int *__restrict__ bucket_out)
{
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    long long i = j;
    int b = -1;
    if (pos) {
        const int s = pos[j];
        if (s < 0 || s >= n) return;
        i = sidx[s];
        b = (int)(skey[s] >> 24);
    }
    if (i < 0 || i >= n) return;
    if (out_xyz) { const T *x = X + i * xs; T *o = out_xyz + j * os; o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; }
    if (out_nrm) { const T *x = N + i * ns; T *o = out_nrm + j * ons; o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; }
    if (out_desc)
        for (int r = 0; r < drows; r++) out_desc[j * drows + r] = desc[i * drows + r];
    if (kept_idx) kept_idx[j] = (int)i;
    if (bucket_out) bucket_out[j] = b;
}

template <typename T>
int launch_ns_sort(hipStream_t st, const T *N, int ns, int n, const NsGrid &g, unsigned long long seed, const NsScratch &w)
{
    const dim3 b256(256);
    const int nt = cdiv(n, kVoxTile);
    (void)hipMemsetAsync(w.counts, 0, sizeof(int) * ((size_t)g.nb_bucket + 1), st);
    if (g.nb_bucket <= kNsLdsBuckets)
        hipLaunchKernelGGL((k_ns_keys<T, true>), dim3(cdiv(n, kNsTile)), b256, 0, st, N, ns, n, g, seed, w.key[0], w.idx[0], w.counts);
    else
        hipLaunchKernelGGL((k_ns_keys<T, false>), dim3(cdiv(n, kNsTile)), b256, 0, st, N, ns, n, g, seed, w.key[0], w.idx[0], w.counts);
    const int bits = 24 + (g.nb_bucket > 1 ? 32 - __builtin_clz((unsigned)(g.nb_bucket - 1)) : 0);
    int cur = 0;
    for (int shift = 0; shift < bits; shift += 8) {                      // the stable LSD radix sort of VoxelGrid, its kernels unchanged
        hipLaunchKernelGGL(k_vox_hist, dim3(nt), b256, 0, st, (const unsigned long long *)w.key[cur], n, shift, nt, w.hist);
        launch_exclusive_scan(st, w.hist, 256 * nt, w.hoff, w.bsum);
        hipLaunchKernelGGL(k_vox_scatter, dim3(nt), b256, 0, st, (const unsigned long long *)w.key[cur], (const int *)w.idx[cur], n, shift, nt,
                           (const int *)w.hoff, w.key[cur ^ 1], w.idx[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
}

template <typename T>
void launch_ns_gather(hipStream_t st, const int *pos, const unsigned long long *skey, const int *sidx, int m, int n, const T *X, int xs, const T *N,
                      int ns, const T *desc, int drows, T *out_xyz, int os, T *out_nrm, int ons, T *out_desc, int *kept_idx, int *bucket_out)
{
    hipLaunchKernelGGL(k_ns_gather<T>, dim3(cdiv(m, 256)), dim3(256), 0, st, pos, skey, sidx, m, n, X, xs, N, ns, desc, drows, out_xyz, os, out_nrm, ons,
                       desc ? out_desc : (T *)nullptr, kept_idx, bucket_out);
}

#define INSTANTIATE_NORMALSPACE(T)                                                                                                             \
    template int launch_ns_sort<T>(hipStream_t, const T *, int, int, const NsGrid &, unsigned long long, const NsScratch &);                   \
    template void launch_ns_gather<T>(hipStream_t, const int *, const unsigned long long *, const int *, int, int, const T *, int, const T *, \
                                      int, const T *, int, T *, int, T *, int, T *, int *, int *);
INSTANTIATE_NORMALSPACE(float)
INSTANTIATE_NORMALSPACE(double)
#undef INSTANTIATE_NORMALSPACE
