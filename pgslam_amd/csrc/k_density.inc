// k_density.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): the `densities` descriptor and
// MaxDensityDataPointsFilter (include/pgicp_density.h).
//
// The densities are an epilogue of k_surface_normals (k_normals.inc, DENS = true): the neighbour list, its count and its mean
// are in registers there.  MaxDensity is the oracle's orc_max_density_keep:
//   1. k_md_max: the cloud's largest density `last` -- upstream's sequential rule (last = dens[0]; if (dens[i] > last) ...) gives
//      NaN when dens[0] is NaN and the maximum over the non-NaN values otherwise; `last` is only ever compared with ==, so the
//      sign of a zero maximum does not matter.  An order-preserving bit key, a block reduction and one atomicMax a block, as
//      k_gd_max does it; whether dens[0] is a NaN is noted apart;
//   2. k_md_count: saturated = #{dens[i] == last}: ballot, popcount, one integer add a block;
//   3. k_md_keep: the keep flag of every point, the draw being k_filter.inc's seeded_mix on the point's index;
//   4. the three scan kernels of k_build.inc rank the flags, k_filter_compact moves the coordinates, the carried descriptor rows
//      and the kept indices, k_density_compact the rows the normals kernel made (normals, eigenvalues, densities).
// DensStat (kernels.hpp): key = the largest order-preserving key of a non-NaN density (0: none seen); saturated; first_nan.

template <typename T>
__device__ __forceinline__ typename Bits<T>::U md_key(T v)
{
    using U = typename Bits<T>::U;
    const U b = Bits<T>::key(v), sign = (U)1 << (Bits<T>::kBits - 1);
    return (b & sign) ? (U)~b : (U)(b | sign);
}
template <typename T>
__device__ __forceinline__ T md_last(const DensStat &s)
{
    using U = typename Bits<T>::U;
    const U k = (U)s.key, sign = (U)1 << (Bits<T>::kBits - 1);
    if (s.first_nan || k == 0) return Bits<T>::val((U)~(U)0);      // a NaN: equal to nothing
    return Bits<T>::val((k & sign) ? (U)(k ^ sign) : (U)~k);
}

constexpr int kMdItems = 8;           // densities per thread of k_md_max
template <typename T>
__global__ __launch_bounds__(256) void k_md_max(const T *__restrict__ dens, int n, DensStat *__restrict__ stat)
{
    using U = typename Bits<T>::U;
    const long long base = (long long)blockIdx.x * (256 * kMdItems);
    U k = 0;
#pragma unroll
    for (int it = 0; it < kMdItems; it++) {
        const long long i = base + it * 256 + threadIdx.x;
        if (i < n) {
            const T v = dens[i];
            if (v == v) { const U kv = md_key<T>(v); k = kv > k ? kv : k; }
            else if (i == 0) stat->first_nan = 1;
        }
    }
    __shared__ U red[4];
    for (int o = 32; o > 0; o >>= 1) { const U t = __shfl_xor(k, o); k = t > k ? t : k; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) k = red[w] > k ? red[w] : k;
        if (k) atomicMax(&stat->key, (unsigned long long)k);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_md_count(const T *__restrict__ dens, int n, DensStat *__restrict__ stat)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const T last = md_last<T>(*stat);
    const bool eq = i < n && dens[i] == last;
    const int c = __popcll(__ballot(eq));
    __shared__ int red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = (red[0] + red[1]) + (red[2] + red[3]);
        if (s) atomicAdd(&stat->saturated, s);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_md_keep(const T *__restrict__ dens, int n, T max_density, unsigned long long seed,
                                                 const DensStat *__restrict__ stat, int *__restrict__ keep)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T d = dens[i];
    int k = 1;
    if (d > max_density) {
        float accept = (float)(max_density / d);
        if (d == md_last<T>(*stat)) accept = accept * (float)(1 - stat->saturated / n);       // INTEGER division, as upstream writes it
        k = (double)(seeded_mix(seed, i) >> 11) / 9007199254740992.0 < (double)accept ? 1 : 0;
    }
    keep[i] = k;
}

// the rows k_surface_normals made, moved to the kept points' ranks (any row may be null); alone: the kept indices
template <typename T>
__global__ __launch_bounds__(256) void k_density_compact(int n, const int *__restrict__ keep, const int *__restrict__ pos,
                                                         const T *__restrict__ nrm, const T *__restrict__ eig, const T *__restrict__ dens,
                                                         T *__restrict__ out_nrm, int out_nstride, T *__restrict__ out_eig,
                                                         T *__restrict__ out_dens, int *__restrict__ kept_idx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const long long o = pos[i];
    if (out_nrm) { T *q = out_nrm + o * out_nstride; q[0] = nrm[3LL * i]; q[1] = nrm[3LL * i + 1]; q[2] = nrm[3LL * i + 2]; }
    if (out_eig) { out_eig[3 * o] = eig[3LL * i]; out_eig[3 * o + 1] = eig[3LL * i + 1]; out_eig[3 * o + 2] = eig[3LL * i + 2]; }
    if (out_dens) out_dens[o] = dens[i];
    if (kept_idx) kept_idx[o] = i;
}

// ---- launchers ----
template <typename T>
int launch_surface_densities(hipStream_t st, const MapDev<T> *maps, int map, int m, int knn, T max_dist, T eps_rank, T *out_nrm,
                             int out_stride, T *out_eig, T *out_dens)
{
    const dim3 grid(cdiv(m, 128)), block(128);
    int *const no_ids = nullptr;
    T *const no_d2 = nullptr;
    if (knn <= 8) hipLaunchKernelGGL((k_surface_normals<T, 8, true>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, no_ids, no_d2, out_dens);
    else if (knn <= 16) hipLaunchKernelGGL((k_surface_normals<T, 16, true>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, no_ids, no_d2, out_dens);
    else if (knn <= 32) hipLaunchKernelGGL((k_surface_normals<T, 32, true>), grid, block, 0, st, maps, map, knn, max_dist, eps_rank, out_nrm, out_stride, out_eig, no_ids, no_d2, out_dens);
    else return -1;
    return 0;
}

// keep: n + 1 ints, pos: n + 1 ints (pos[n] ends up holding the number kept), block_sums: scan_scratch_ints(n) ints
template <typename T>
void launch_max_density(hipStream_t st, const T *dens, int n, T max_density, unsigned long long seed, DensStat *stat, int *keep, int *pos,
                        int *block_sums)
{
    (void)hipMemsetAsync(stat, 0, sizeof(DensStat), st);
    const dim3 grid(cdiv(n, 256)), block(256);
    hipLaunchKernelGGL(k_md_max<T>, dim3(cdiv(n, 256 * kMdItems)), block, 0, st, dens, n, stat);
    hipLaunchKernelGGL(k_md_count<T>, grid, block, 0, st, dens, n, stat);
    hipLaunchKernelGGL(k_md_keep<T>, grid, block, 0, st, dens, n, max_density, seed, (const DensStat *)stat, keep);
    launch_exclusive_scan(st, keep, n, pos, block_sums);
}

// the compaction after launch_max_density: coordinates (at `stride`, in and out), carried descriptor rows and kept indices through
// k_filter_compact (xyz == null: none of them), the normals kernel's rows through k_density_compact
template <typename T>
void launch_density_compact(hipStream_t st, int n, const int *keep, const int *pos, const T *xyz, int stride, const T *desc, int drows,
                            const T *nrm, const T *eig, const T *dens, T *out_xyz, T *out_desc, T *out_nrm, int out_nstride, T *out_eig,
                            T *out_dens, int *kept_idx)
{
    const dim3 grid(cdiv(n, 256)), block(256);
    if (xyz) {
        Mat34 M;
        for (int i = 0; i < 12; i++) M.v[i] = i % 5 == 0 ? 1.0 : 0.0;
        hipLaunchKernelGGL(k_filter_compact<T>, grid, block, 0, st, xyz, stride, 3, desc, drows, n, keep, pos, M, 0, -1, -1, out_xyz, out_desc,
                           kept_idx, (int *)nullptr, 0);
    }
    if (out_nrm || out_eig || out_dens || (!xyz && kept_idx))
        hipLaunchKernelGGL(k_density_compact<T>, grid, block, 0, st, n, keep, pos, nrm, eig, dens, out_nrm, out_nstride, out_eig, out_dens,
                           xyz ? (int *)nullptr : kept_idx);
}

#define INSTANTIATE_DENSITY(T)                                                                                                         \
    template int launch_surface_densities<T>(hipStream_t, const MapDev<T> *, int, int, int, T, T, T *, int, T *, T *);               \
    template void launch_max_density<T>(hipStream_t, const T *, int, T, unsigned long long, DensStat *, int *, int *, int *);         \
    template void launch_density_compact<T>(hipStream_t, int, const int *, const int *, const T *, int, const T *, int, const T *,   \
                                            const T *, const T *, T *, T *, T *, int, T *, T *, int *);
INSTANTIATE_DENSITY(float)
INSTANTIATE_DENSITY(double)
#undef INSTANTIATE_DENSITY
