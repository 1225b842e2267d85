// k_voxel.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): VoxelGridDataPointsFilter.
//
// [EXT] libpointmatcher VoxelGridDataPointsFilter as include/pgicp.h (pgicp_voxel_grid_*) states it.  The schedule:
//   1. k_vox_bounds: min / max of each axis (atomics on order-preserving keys: exact, any order) and the not-finite flag;
//      the host reads them back and derives minB, numDiv and the key's bit count in T, as the statement writes them;
//   2. k_vox_keys: the 64-bit voxel key of every point, paired with its index;
//   3. the stable LSD radix sort of the (key, index) pairs over the key's bits only (launch_pair_sort, k_pairsort.inc).  The
//      input is in index order, so a voxel's pairs end in ascending index: its first pair is its first point;
//   4. k_vox_heads marks the segment heads, one scan numbers them; k_vox_first flags each voxel's first point (by point
//      index), and one scan of those flags gives every voxel its output slot: ascending first index;
//   5. k_vox_emit, one thread per first point, writes the index, count, centre or first-point values and -- for a voxel of at
//      most kVoxHeavy points -- the sums, sequentially in ascending index; heavier voxels go to a list that k_vox_heavy sums,
//      one block per voxel: the block stages 512 points of up to 8 rows into LDS, then one lane per row adds them in order
//      while the block loads the next 512.
// No floating-point atomics: the order of every sum is the statement's.  The arithmetic contract of kernels.hip holds.

constexpr int kVoxHeavy = 64;        // a voxel of more points is summed by a block (k_vox_heavy)
constexpr int kVoxRows = 8;          // rows one pass of k_vox_heavy stages

// order-preserving key of a coordinate (-0.0 -> +0.0) and its inverse
template <typename T>
__device__ __forceinline__ unsigned long long vox_okey(T v)
{
    using U = typename Bits<T>::U;
    const U sign = (U)1 << (Bits<T>::kBits - 1);
    U k = Bits<T>::key(v);
    if (k == sign) k = 0;
    return (unsigned long long)((k & sign) ? (U)~k : (U)(k | sign));
}

template <typename T>
__global__ __launch_bounds__(256) void k_vox_bounds(const T *__restrict__ X, int xs, int n, VoxStat *__restrict__ st)
{
    unsigned long long lo[3] = {~0ULL, ~0ULL, ~0ULL}, hi[3] = {0, 0, 0};
    int bad = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        for (int a = 0; a < 3; a++) {
            const T v = X[i * xs + a];
            if (!(v - v == (T)0)) bad = 1;                     // NaN or +-inf
            const unsigned long long k = vox_okey<T>(v);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; a++) {
            const unsigned long long l = __shfl_down(lo[a], o, 64), h = __shfl_down(hi[a], o, 64);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
        bad |= __shfl_down(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; a++) { atomicMin(&st->lo[a], lo[a]); atomicMax(&st->hi[a], hi[a]); }
        if (bad) atomicOr(&st->bad, 1);
    }
}

// i_a = (unsigned)floor(x_a / v_a - minB_a); idx = i + j numDivX + k numDivX numDivY, in 64 bits
template <typename T>
__global__ __launch_bounds__(256) void k_vox_keys(const T *__restrict__ X, int xs, int n, VoxGrid<T> g, unsigned long long *__restrict__ key,
                                                  int *__restrict__ idx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned long long c[3];
    for (int a = 0; a < 3; a++) {
        const T t = X[(long long)i * xs + a] / g.v[a] - g.minB[a];
        c[a] = (unsigned long long)(unsigned)floor(t);
    }
    key[i] = c[0] + c[1] * g.nd[0] + c[2] * (g.nd[0] * g.nd[1]);
    idx[i] = i;
}

// head[s] = 1 where a voxel starts in the sorted order
__global__ __launch_bounds__(256) void k_vox_heads(const unsigned long long *__restrict__ key, int n, int *__restrict__ head)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    head[s] = (s == 0 || key[s] != key[s - 1]) ? 1 : 0;
}

// voxel g = hs[s] starts at start[g]; its first point is flagged, with its voxel
__global__ __launch_bounds__(256) void k_vox_first(const int *__restrict__ sidx, int n, const int *__restrict__ head, const int *__restrict__ hs,
                                                   int *__restrict__ start, int *__restrict__ first, int *__restrict__ vox_of)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    if (s == 0) start[hs[n]] = n;
    if (!head[s]) return;
    const int g = hs[s], i = sidx[s];
    start[g] = s;
    first[i] = 1;
    vox_of[i] = g;
}

// one thread per first point: slot o = pos[i]
template <typename T>
__global__ __launch_bounds__(256) void k_vox_emit(const T *__restrict__ X, int xs, int n, VoxGrid<T> g, const int *__restrict__ sidx,
                                                  const unsigned long long *__restrict__ skey, const int *__restrict__ start,
                                                  const int *__restrict__ first, const int *__restrict__ vox_of, const int *__restrict__ pos,
                                                  int centroid, const T *__restrict__ desc, int drows, int average, T *__restrict__ out_xyz, int os,
                                                  T *__restrict__ out_desc, int *__restrict__ kept_idx, int *__restrict__ out_count,
                                                  int2 *__restrict__ heavy, VoxStat *__restrict__ st)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !first[i]) return;
    const int v = vox_of[i], s = start[v], c = start[v + 1] - s;
    const long long o = pos[i];
    if (kept_idx) kept_idx[o] = i;
    if (out_count) out_count[o] = c;
    T *ox = out_xyz + o * os;
    T *od = desc ? out_desc + o * drows : nullptr;
    if (!centroid) {
        // the voxel's centre, i_a recovered from idx by / and -
        const unsigned long long idx = skey[s], pl = g.nd[0] * g.nd[1];
        const unsigned long long k = idx / pl, j = (idx - k * pl) / g.nd[0], ii = idx - k * pl - j * g.nd[0];
        const unsigned long long ia[3] = {ii, j, k};
        for (int a = 0; a < 3; a++) ox[a] = (g.minB[a] + (T)ia[a]) * g.v[a] + g.v[a] / (T)2;
    }
    if (desc && !average)
        for (int r = 0; r < drows; r++) od[r] = desc[(long long)i * drows + r];
    if (c == 1) {                                           // (x / 1 == x, the sign of a zero included)
        if (centroid) for (int a = 0; a < 3; a++) ox[a] = X[(long long)i * xs + a];
        if (desc && average) for (int r = 0; r < drows; r++) od[r] = desc[(long long)i * drows + r];
        return;
    }
    if (c > kVoxHeavy) {
        if (centroid || (desc && average)) heavy[atomicAdd(&st->nheavy, 1)] = make_int2(v, (int)o);
        return;
    }
    const T cnt = (T)c;
    if (centroid) {
        for (int a = 0; a < 3; a++) {
            T sum = X[(long long)i * xs + a];
            for (int k = 1; k < c; k++) sum += X[(long long)sidx[s + k] * xs + a];
            ox[a] = sum / cnt;
        }
    }
    if (desc && average) {
        for (int r = 0; r < drows; r++) {
            T sum = desc[(long long)i * drows + r];
            for (int k = 1; k < c; k++) sum += desc[(long long)sidx[s + k] * drows + r];
            od[r] = sum / cnt;
        }
    }
}

// one block per heavy voxel (list from k_vox_emit): rows 0-2 the coordinates (with useCentroid), then the descriptor rows (with
// averaging).  kVoxChunk points of kVoxRows rows are staged in LDS, lane r adds row r's values in ascending index while the
// block's loads of the next chunk are in flight (registers)
constexpr int kVoxHeavyBlock = 256, kVoxPer = 2, kVoxChunk = kVoxHeavyBlock * kVoxPer;
template <typename T>
__global__ __launch_bounds__(kVoxHeavyBlock) void k_vox_heavy(const T *__restrict__ X, int xs, const int *__restrict__ sidx, const int *__restrict__ start,
                                                              const int2 *__restrict__ heavy, const VoxStat *__restrict__ st, int centroid,
                                                              const T *__restrict__ desc, int drows, int average, T *__restrict__ out_xyz, int os,
                                                              T *__restrict__ out_desc)
{
    __shared__ T buf[kVoxRows][kVoxChunk];
    const int t = threadIdx.x;
    const int nh = st->nheavy;
    const int xr = centroid ? 3 : 0, rows = xr + (desc && average ? drows : 0);
    for (int h = blockIdx.x; h < nh; h += gridDim.x) {
        const int2 e = heavy[h];
        const int s = start[e.x], c = start[e.x + 1] - s;
        const long long o = e.y;
        for (int r0 = 0; r0 < rows; r0 += kVoxRows) {
            const int rn = rows - r0 < kVoxRows ? rows - r0 : kVoxRows;
            T nxt[kVoxPer][kVoxRows];
            auto fetch = [&](int b) {
#pragma unroll
                for (int u = 0; u < kVoxPer; u++) {
                    const int p = b + u * kVoxHeavyBlock + t;
                    if (p >= c) continue;
                    const long long i = sidx[s + p];
#pragma unroll
                    for (int q = 0; q < kVoxRows; q++) {
                        const int r = r0 + q;
                        if (q < rn) nxt[u][q] = r < xr ? X[i * xs + r] : desc[i * drows + (r - xr)];
                    }
                }
            };
            T sum = (T)0;
            fetch(0);
            for (int b = 0; b < c; b += kVoxChunk) {
#pragma unroll
                for (int u = 0; u < kVoxPer; u++) {
                    const int k = u * kVoxHeavyBlock + t;
                    if (b + k >= c) continue;
#pragma unroll
                    for (int q = 0; q < kVoxRows; q++) if (q < rn) buf[q][k] = nxt[u][q];
                }
                __syncthreads();
                if (b + kVoxChunk < c) fetch(b + kVoxChunk);
                if (t < rn) {
                    const int m = c - b < kVoxChunk ? c - b : kVoxChunk;
                    int k = 0;
                    if (b == 0) { sum = buf[t][0]; k = 1; }             // the first point's value starts the sum
                    for (; k + 16 <= m; k += 16) {                       // 16 LDS reads in flight, then the 16 adds in order
                        T x[16];
#pragma unroll
                        for (int u = 0; u < 16; u++) x[u] = buf[t][k + u];
#pragma unroll
                        for (int u = 0; u < 16; u++) sum += x[u];
                    }
                    for (; k < m; k++) sum += buf[t][k];
                }
                __syncthreads();
            }
            if (t < rn) {
                const int r = r0 + t;
                if (r < xr) out_xyz[o * os + r] = sum / (T)c;
                else out_desc[o * drows + (r - xr)] = sum / (T)c;
            }
        }
    }
}

__global__ void k_vox_init(VoxStat *st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int a = 0; a < 3; a++) { st->lo[a] = ~0ULL; st->hi[a] = 0; }
    st->bad = 0; st->kept = 0; st->nheavy = 0; st->pad = 0;
}

template <typename T>
void launch_voxel_bounds(hipStream_t st, const T *X, int xs, int n, VoxStat *stat)
{
    hipLaunchKernelGGL(k_vox_init, dim3(1), dim3(64), 0, st, stat);
    if (n <= 0) return;
    const int nb = std::min(cdiv(n, 256), 1024);
    hipLaunchKernelGGL(k_vox_bounds<T>, dim3(nb), dim3(256), 0, st, X, xs, n, stat);
}

// steps 2-5, after the host has checked the bounds and derived the grid (`bits`: the bits a key can have)
template <typename T>
void launch_voxel_grid(hipStream_t st, const T *X, int xs, int n, const VoxGrid<T> &g, int bits, int centroid, const T *desc, int drows, int average,
                       const VoxScratch &w, T *out_xyz, int os, T *out_desc, int *kept_idx, int *out_count, VoxStat *stat)
{
    if (n <= 0) return;
    const dim3 b256(256);
    auto scan = [&](const int *in, int len, int *out) { launch_exclusive_scan(st, in, len, out, w.sort.bsum); };
    hipLaunchKernelGGL(k_vox_keys<T>, dim3(cdiv(n, 256)), b256, 0, st, X, xs, n, g, w.sort.key[0], w.sort.idx[0]);
    const int cur = launch_pair_sort(st, w.sort, n, bits, 0);
    const unsigned long long *skey = w.sort.key[cur];
    const int *sidx = w.sort.idx[cur];
    hipLaunchKernelGGL(k_vox_heads, dim3(cdiv(n, 256)), b256, 0, st, skey, n, w.head);
    scan(w.head, n, w.hs);
    (void)hipMemsetAsync(w.first, 0, sizeof(int) * (size_t)n, st);
    hipLaunchKernelGGL(k_vox_first, dim3(cdiv(n, 256)), b256, 0, st, sidx, n, (const int *)w.head, (const int *)w.hs, w.start, w.first, w.vox_of);
    scan(w.first, n, w.pos);
    hipLaunchKernelGGL(k_vox_emit<T>, dim3(cdiv(n, 256)), b256, 0, st, X, xs, n, g, sidx, skey, (const int *)w.start, (const int *)w.first,
                       (const int *)w.vox_of, (const int *)w.pos, centroid, desc, drows, average, out_xyz, os, out_desc, kept_idx, out_count, w.heavy, stat);
    hipLaunchKernelGGL(k_vox_heavy<T>, dim3(std::max(1, std::min(cdiv(n, kVoxHeavy + 1), 2048))), dim3(kVoxHeavyBlock), 0, st, X, xs, sidx, (const int *)w.start,
                       (const int2 *)w.heavy, (const VoxStat *)stat, centroid, desc, drows, average, out_xyz, os, out_desc);
    (void)hipMemcpyAsync(&stat->kept, w.pos + n, sizeof(int), hipMemcpyDeviceToDevice, st);
}

template void launch_voxel_bounds<float>(hipStream_t, const float *, int, int, VoxStat *);
template void launch_voxel_bounds<double>(hipStream_t, const double *, int, int, VoxStat *);
template void launch_voxel_grid<float>(hipStream_t, const float *, int, int, const VoxGrid<float> &, int, int, const float *, int, int, const VoxScratch &,
                                       float *, int, float *, int *, int *, VoxStat *);
template void launch_voxel_grid<double>(hipStream_t, const double *, int, int, const VoxGrid<double> &, int, int, const double *, int, int,
                                        const VoxScratch &, double *, int, double *, int *, int *, VoxStat *);
