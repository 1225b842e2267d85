// k_octree.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): OctreeGridDataPointsFilter.
//
// [EXT] libpointmatcher OctreeGridDataPointsFilter as include/pgicp_octree.h states it.  A point's path through the octree
// depends on the root and on that point alone, so the tree is never built: it is a path code per point.  The schedule:
//   1. launch_voxel_bounds (k_voxel.inc, as it is): min / max of each axis and the not-finite flag; the host reads them back
//      and derives the root and the levels of a code, min(21, d_size), in T (octree_host.hpp, shared with the host form);
//   2. k_oct_paths: compare and halve per level, the centre carried in T as the statement writes it; the level-l digit sits
//      above the level-(l+1) digit, so ascending codes are the depth-first order with children 0 .. 7;
//   3. the stable LSD radix sort of (code, index) over the code's bits only: launch_pair_sort (k_pairsort.inc);
//   4. k_oct_depth: per sorted position the leaf depth -- the count of codes sharing a d-prefix is non-increasing in d, so the
//      smallest d meeting the count rule is a binary search over d, each probe a lower bound in the sorted codes and one look
//      maxPointByNode positions ahead -- and the leaf-head flag (the depth-prefix differs from the left neighbour's);
//   5. one launch_exclusive_scan numbers the leaves: the output slots, already in leaf order; k_oct_leaves records each leaf's
//      start and depth;
//   6. (maxPointByNode > 1 only) a leaf above the last level holds points of different codes, sorted by code and not by
//      index: k_oct_leaves also writes (leaf number, index) by INPUT index and a second stable sort over the bits of n - 1
//      brings every leaf to ascending index.  Leaf sizes and order do not change, so the starts stay.  With maxPointByNode 1
//      such a leaf holds one point and a leaf at the last level holds equal codes, which the stable sort left in index order;
//   7. k_oct_emit, one thread per leaf, picks or sums sequentially in ascending index; for methods 2 and 3 a leaf of more
//      than kOctHeavy points goes to a list that k_oct_heavy handles, one block per leaf: 512 points of up to 8 rows staged in
//      LDS, one lane per row adding them in order; the medoid's argmin is a block reduction on (distance, position).
// No floating-point atomics: the order of every sum is the statement's.  The arithmetic contract of kernels.hip holds.

constexpr int kOctHeavy = 64;        // a leaf of more points is summed by a block (k_oct_heavy), methods 2 and 3
constexpr int kOctRows = 8;          // rows one pass of k_oct_heavy stages
constexpr int kOctHeavyBlock = 256, kOctChunk = 512;

template <typename T>
__global__ __launch_bounds__(256) void k_oct_paths(const T *__restrict__ X, int xs, int n, OctRoot<T> R, unsigned long long *__restrict__ key,
                                                   int *__restrict__ idx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T p[3], c[3], r = R.r;
    for (int a = 0; a < 3; a++) { p[a] = X[(long long)i * xs + a]; c[a] = R.c[a]; }
    unsigned long long k = 0;
    for (int l = 0; l < R.levels; l++) {
        const T h = r * (T)0.5;
        unsigned m = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (p[a] > c[a]) { m |= 1u << a; c[a] = c[a] + h; }
            else c[a] = c[a] - h;
        }
        k = (k << 3) | m;
        r = h;
    }
    key[i] = k;
    idx[i] = i;
}

// depth[s]: the leaf depth of sorted position s; head[s] = 1 where a leaf starts
__global__ __launch_bounds__(256) void k_oct_depth(const unsigned long long *__restrict__ key, int n, int levels, int max_pts, int *__restrict__ depth,
                                                   int *__restrict__ head)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const unsigned long long k = key[s];
    int dlo = 0, dhi = levels;
    while (dlo < dhi) {
        const int d = (dlo + dhi) >> 1, sh = 3 * (levels - d);
        const unsigned long long p = k >> sh;
        int lo = 0, hi = s;                                  // the first position whose d-prefix is p
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((key[mid] >> sh) < p) lo = mid + 1; else hi = mid;
        }
        const long long e = (long long)lo + max_pts;         // more than max_pts share the prefix iff position e does
        const bool few = e >= n || (key[e] >> sh) != p;
        if (few) dhi = d; else dlo = d + 1;
    }
    const int sh = 3 * (levels - dlo);
    depth[s] = dlo;
    head[s] = (s == 0 || (key[s - 1] >> sh) != (k >> sh)) ? 1 : 0;
}

// leaf g = hs[s] + head[s] - 1 of position s: its start and depth; with `key2` the (leaf, index) pair of the second sort, by index
__global__ __launch_bounds__(256) void k_oct_leaves(const int *__restrict__ sidx, int n, const int *__restrict__ depth, const int *__restrict__ head,
                                                    const int *__restrict__ hs, int *__restrict__ start, int *__restrict__ ldepth,
                                                    unsigned long long *__restrict__ key2, int *__restrict__ idx2)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    if (s == 0) start[hs[n]] = n;
    const int hd = head[s], g = hs[s] + hd - 1;
    if (hd) { start[g] = s; ldepth[g] = depth[s]; }
    if (key2) { const int i = sidx[s]; key2[i] = (unsigned long long)g; idx2[i] = i; }
}

// one thread per leaf: slot g
template <typename T>
__global__ __launch_bounds__(256) void k_oct_emit(const T *__restrict__ X, int xs, int n, const int *__restrict__ sidx, const int *__restrict__ start,
                                                  const int *__restrict__ ldepth, const int *__restrict__ nleaves, int method, unsigned long long seed,
                                                  const T *__restrict__ desc, int drows, T *__restrict__ out_xyz, int os, T *__restrict__ out_desc,
                                                  int *__restrict__ kept_idx, int *__restrict__ out_count, int *__restrict__ out_depth,
                                                  int *__restrict__ heavy, VoxStat *__restrict__ st)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || g >= *nleaves) return;
    const int s = start[g], c = start[g + 1] - s;
    const int *p = sidx + s;
    const int first = p[0];
    if (out_count) out_count[g] = c;
    if (out_depth) out_depth[g] = ldepth[g];
    if (method >= 2 && c > kOctHeavy) { heavy[atomicAdd(&st->nheavy, 1)] = g; return; }
    int keep = first;
    if (method == 1) keep = p[(int)((seeded_mix(seed, first) >> 11) % (unsigned long long)c)];
    T cen[3] = {(T)0, (T)0, (T)0};
    if (method >= 2) {
        const T cnt = (T)c;
        for (int a = 0; a < 3; a++) {
            T sum = X[(long long)first * xs + a];
            for (int k = 1; k < c; k++) sum += X[(long long)p[k] * xs + a];
            cen[a] = sum / cnt;
        }
    }
    if (method == 3) {
        T best = (T)0;
        for (int k = 0; k < c; k++) {
            const long long i = p[k];
            const T dx = X[i * xs] - cen[0], dy = X[i * xs + 1] - cen[1], dz = X[i * xs + 2] - cen[2];
            const T dd = (dx * dx + dy * dy) + dz * dz;
            if (k == 0 || dd < best) { best = dd; keep = (int)i; }
        }
    }
    if (kept_idx) kept_idx[g] = keep;
    if (out_xyz)
        for (int a = 0; a < 3; a++) out_xyz[(long long)g * os + a] = method == 2 ? cen[a] : X[(long long)keep * xs + a];
    if (desc) {
        T *od = out_desc + (long long)g * drows;
        if (method == 2) {
            const T cnt = (T)c;
            for (int r = 0; r < drows; r++) {
                T sum = desc[(long long)first * drows + r];
                for (int k = 1; k < c; k++) sum += desc[(long long)p[k] * drows + r];
                od[r] = sum / cnt;
            }
        } else
            for (int r = 0; r < drows; r++) od[r] = desc[(long long)keep * drows + r];
    }
}

// one block per heavy leaf (list from k_oct_emit).  Method 2: rows 0-2 the coordinates, then the descriptor rows, each summed
// in ascending index by one lane from LDS.  Method 3: the coordinates' centroid that way, then the block's argmin of the squared
// distance to it -- (distance, position in the leaf) ascending, so ties go to the smallest index -- and the gather of that point
template <typename T>
__global__ __launch_bounds__(kOctHeavyBlock) void k_oct_heavy(const T *__restrict__ X, int xs, const int *__restrict__ sidx, const int *__restrict__ start,
                                                              const int *__restrict__ heavy, const VoxStat *__restrict__ st, int method,
                                                              const T *__restrict__ desc, int drows, T *__restrict__ out_xyz, int os,
                                                              T *__restrict__ out_desc, int *__restrict__ kept_idx)
{
    __shared__ T buf[kOctRows][kOctChunk];
    __shared__ T cen[3];
    __shared__ T bd[kOctHeavyBlock];
    __shared__ int bp[kOctHeavyBlock];
    const int t = threadIdx.x;
    const int nh = st->nheavy;
    const int rows = 3 + (method == 2 && desc ? drows : 0);
    for (int h = blockIdx.x; h < nh; h += gridDim.x) {
        const long long g = heavy[h];
        const int s = start[g], c = start[g + 1] - s;
        const int *p = sidx + s;
        for (int r0 = 0; r0 < rows; r0 += kOctRows) {
            const int rn = rows - r0 < kOctRows ? rows - r0 : kOctRows;
            T sum = (T)0;
            for (int b = 0; b < c; b += kOctChunk) {
                const int m = c - b < kOctChunk ? c - b : kOctChunk;
                for (int k = t; k < m; k += kOctHeavyBlock) {
                    const long long i = p[b + k];
                    for (int q = 0; q < rn; q++) {
                        const int r = r0 + q;
                        buf[q][k] = r < 3 ? X[i * xs + r] : desc[i * drows + (r - 3)];
                    }
                }
                __syncthreads();
                if (t < rn) {
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
                const T v = sum / (T)c;
                if (r < 3) {
                    cen[r] = v;
                    if (method == 2 && out_xyz) out_xyz[g * os + r] = v;
                } else
                    out_desc[g * drows + (r - 3)] = v;
            }
        }
        if (method == 2) {
            if (t == 0 && kept_idx) kept_idx[g] = p[0];
            __syncthreads();
            continue;
        }
        __syncthreads();                                                 // cen is written
        T best = (T)0;
        int bpos = -1;
        for (int k = t; k < c; k += kOctHeavyBlock) {
            const long long i = p[k];
            const T dx = X[i * xs] - cen[0], dy = X[i * xs + 1] - cen[1], dz = X[i * xs + 2] - cen[2];
            const T dd = (dx * dx + dy * dy) + dz * dz;
            if (bpos < 0 || dd < best) { best = dd; bpos = k; }
        }
        bd[t] = best; bp[t] = bpos;                                      // (c > kOctHeavy, but a thread past c holds -1)
        __syncthreads();
        for (int o = kOctHeavyBlock / 2; o > 0; o >>= 1) {
            if (t < o) {
                const T d2 = bd[t + o];
                const int p2 = bp[t + o], p1 = bp[t];
                if (p2 >= 0 && (p1 < 0 || d2 < bd[t] || (d2 == bd[t] && p2 < p1))) { bd[t] = d2; bp[t] = p2; }
            }
            __syncthreads();
        }
        const long long keep = p[bp[0]];
        if (t == 0 && kept_idx) kept_idx[g] = (int)keep;
        if (t < 3 && out_xyz) out_xyz[g * os + t] = X[keep * xs + t];
        if (desc) for (int r = t; r < drows; r += kOctHeavyBlock) out_desc[g * drows + r] = desc[keep * drows + r];
        __syncthreads();                                                 // bd / bp / cen are free for the next leaf
    }
}

// steps 2-7, after the host has checked the bounds and derived the root (stat: zeroed by launch_voxel_bounds)
template <typename T>
void launch_octree_grid(hipStream_t st, const T *X, int xs, int n, const OctRoot<T> &R, int max_pts, int method, unsigned long long seed, const T *desc,
                        int drows, const OctScratch &w, T *out_xyz, int os, T *out_desc, int *kept_idx, int *out_count, int *out_depth, VoxStat *stat)
{
    if (n <= 0) return;
    const dim3 b256(256);
    const int nb = cdiv(n, 256);
    hipLaunchKernelGGL(k_oct_paths<T>, dim3(nb), b256, 0, st, X, xs, n, R, w.sort.key[0], w.sort.idx[0]);
    int cur = launch_pair_sort(st, w.sort, n, 3 * R.levels, 0);
    hipLaunchKernelGGL(k_oct_depth, dim3(nb), b256, 0, st, (const unsigned long long *)w.sort.key[cur], n, R.levels, max_pts, w.depth, w.head);
    launch_exclusive_scan(st, w.head, n, w.hs, w.sort.bsum);
    const bool resort = max_pts > 1;
    hipLaunchKernelGGL(k_oct_leaves, dim3(nb), b256, 0, st, (const int *)w.sort.idx[cur], n, (const int *)w.depth, (const int *)w.head, (const int *)w.hs,
                       w.start, w.ldepth, resort ? w.sort.key[cur ^ 1] : (unsigned long long *)nullptr, resort ? w.sort.idx[cur ^ 1] : (int *)nullptr);
    if (resort) cur = launch_pair_sort(st, w.sort, n, n > 1 ? 32 - __builtin_clz((unsigned)(n - 1)) : 0, cur ^ 1);
    const int *sidx = w.sort.idx[cur];
    hipLaunchKernelGGL(k_oct_emit<T>, dim3(nb), b256, 0, st, X, xs, n, sidx, (const int *)w.start, (const int *)w.ldepth, (const int *)(w.hs + n), method,
                       seed, desc, drows, out_xyz, os, out_desc, kept_idx, out_count, out_depth, w.heavy, stat);
    if (method >= 2)
        hipLaunchKernelGGL(k_oct_heavy<T>, dim3(std::max(1, std::min(cdiv(n, kOctHeavy + 1), 2048))), dim3(kOctHeavyBlock), 0, st, X, xs, sidx,
                           (const int *)w.start, (const int *)w.heavy, (const VoxStat *)stat, method, desc, drows, out_xyz, os, out_desc, kept_idx);
    (void)hipMemcpyAsync(&stat->kept, w.hs + n, sizeof(int), hipMemcpyDeviceToDevice, st);
}

template void launch_octree_grid<float>(hipStream_t, const float *, int, int, const OctRoot<float> &, int, int, unsigned long long, const float *, int,
                                        const OctScratch &, float *, int, float *, int *, int *, int *, VoxStat *);
template void launch_octree_grid<double>(hipStream_t, const double *, int, int, const OctRoot<double> &, int, int, unsigned long long, const double *, int,
                                         const OctScratch &, double *, int, double *, int *, int *, int *, VoxStat *);
