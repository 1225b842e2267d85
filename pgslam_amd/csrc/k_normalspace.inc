// k_normalspace.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): NormalSpaceDataPointsFilter.
//
// [EXT] libpointmatcher NormalSpaceDataPointsFilter as include/pgicp_normalspace.h states it.  The schedule:
//   1. k_ns_keys: one thread per point -- the bucket of its normal in double (the device library's acos, atan2 and fmod), the
//      not-finite flag, the key (bucket << 24) | r_i paired with the index, and the buckets' histogram with integer atomics: a
//      block counts its tile of 4096 points in LDS when the grid fits (kNsLdsBuckets) and adds its non-zero counts to the global
//      array, on the global array directly otherwise;
//   2. the stable LSD radix sort of (key, index) over the key's bits only: launch_pair_sort (k_pairsort.inc).  The input is in
//      index order, so equal keys end in ascending index: ascending (bucket, r_i, i);
//   3. the host reads the counts and the flag, runs the draw (normalspace_host.hpp) and uploads per pick its position in the
//      sorted order, start[bucket] + rank;
//   4. k_gather_rows (k_covsample.inc): one thread per pick writes index, bucket, coordinates, normal and descriptor rows.
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
        key[i] = ((unsigned long long)b << 24) | (seeded_mix(seed, i) >> 40);
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
int launch_ns_sort(hipStream_t st, const T *N, int ns, int n, const NsGrid &g, unsigned long long seed, const NsScratch &w)
{
    const dim3 b256(256);
    (void)hipMemsetAsync(w.counts, 0, sizeof(int) * ((size_t)g.nb_bucket + 1), st);
    if (g.nb_bucket <= kNsLdsBuckets)
        hipLaunchKernelGGL((k_ns_keys<T, true>), dim3(cdiv(n, kNsTile)), b256, 0, st, N, ns, n, g, seed, w.sort.key[0], w.sort.idx[0], w.counts);
    else
        hipLaunchKernelGGL((k_ns_keys<T, false>), dim3(cdiv(n, kNsTile)), b256, 0, st, N, ns, n, g, seed, w.sort.key[0], w.sort.idx[0], w.counts);
    return launch_pair_sort(st, w.sort, n, 24 + (g.nb_bucket > 1 ? 32 - __builtin_clz((unsigned)(g.nb_bucket - 1)) : 0), 0);
}

template int launch_ns_sort<float>(hipStream_t, const float *, int, int, const NsGrid &, unsigned long long, const NsScratch &);
template int launch_ns_sort<double>(hipStream_t, const double *, int, int, const NsGrid &, unsigned long long, const NsScratch &);
