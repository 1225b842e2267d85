// k_build.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): map build: centroid / bounding box, cell sort, cell tables, near / super-cell tables.

// ---------------------------------------------------------------------------
// map build: centroid (order-independent fixed point), bbox, cell sort
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ordered_key(double v)
{
    const long long i = __double_as_longlong(v);
    return (unsigned long long)(i >= 0 ? (i ^ (long long)0x8000000000000000LL) : ~i);
}

// cell index of coordinate offset u on a grid of n cells of width 1 / inv_h (clamped; shared by the build
// and every query so that both sides round identically)
template <typename T>
__device__ __forceinline__ int clamp_cell(T u, T inv_h, int n)
{
    const T lim = (T)16777216.0;
    return min(max((int)fmin(fmax(floor(u * inv_h), -lim), lim), 0), n - 1);
}

template <typename T>
__device__ __forceinline__ int build_cell(const GridDesc<T> &g, T x, T y, T z)
{
    int cx = (int)floor((x - g.ox) * g.inv_h);
    int cy = (int)floor((y - g.oy) * g.inv_h);
    int cz = (int)floor((z - g.oz) * g.inv_h);
    cx = min(max(cx, 0), g.nx - 1);
    cy = min(max(cy, 0), g.ny - 1);
    cz = min(max(cz, 0), g.nz - 1);
    return cx + g.nx * (cy + g.ny * cz);
}

__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// One atomic per distinct key among the lanes of a wave (clouds arrive in scan order, so neighbouring
// lanes mostly share a cell); falls back to per-lane atomics after 8 leader rounds.  Returns the
// lane's arrival position inside its key's bucket.
__device__ __forceinline__ int wave_bucket_add(int *__restrict__ counts, int key, bool live)
{
    // The groups are found first (arithmetic only), then all leaders issue their atomics in ONE instruction: a
    // wave pays one atomic round trip, not one per distinct key.
    const int lane = threadIdx.x & 63;
    bool todo = live;
    int my_leader = lane, my_rank = 0, my_size = 1;          // lanes left over after 8 rounds add for themselves
    for (int round = 0; round < 8; ++round) {
        const unsigned long long pending = __ballot(todo);
        if (pending == 0ULL) break;
        const int leader = __ffsll((long long)pending) - 1;
        const int lkey = __builtin_amdgcn_readlane(key, leader);
        const bool mine = todo && key == lkey;
        const unsigned long long grp = __ballot(mine);
        if (mine) { my_leader = leader; my_rank = __popcll(grp & ((1ULL << lane) - 1ULL)); my_size = __popcll(grp); todo = false; }
    }
    int base = 0;
    if (live && my_leader == lane) base = atomicAdd(&counts[key], my_size);
    base = __shfl(base, my_leader, 64);
    return base + my_rank;
}

// The same service for a whole BLOCK, through a hash table in LDS: one global atomic per distinct key of the block instead
// of one per distinct key of every wave.  Device-scope atomics are resolved on the memory side of the eight XCDs' L2s; a
// cloud in firing order (all rings of one azimuth step, then the next step) puts the 64 lanes of a wave into 64 different
// buckets, so the wave-level grouping above saves nothing there and the kernel runs at the rate of those atomics -- but
// the same ring comes back 64 points later, and a block of 512 points holds each bucket some eight times.
// NT threads (all of them must call), table of 2 NT slots: [keys | counts | bases].  Returns the arrival position inside
// the key's bucket (the order of arrival inside a block is arbitrary, as it is between blocks).
template <int NT>
__device__ __forceinline__ int block_bucket_add(int *__restrict__ counts, int key, bool live, int *lds /* 6 NT ints */)
{
    constexpr int H = 2 * NT;
    int *h_key = lds, *h_cnt = lds + H, *h_base = lds + 2 * H;
    for (int t = threadIdx.x; t < H; t += NT) { h_key[t] = -1; h_cnt[t] = 0; }
    __syncthreads();
    int slot = 0, rank = 0;
    if (live) {
        slot = (int)(((unsigned)key * 2654435761u) >> 16) & (H - 1);
        for (;;) {
            const int prev = atomicCAS(&h_key[slot], -1, key);
            if (prev == -1 || prev == key) break;
            slot = (slot + 1) & (H - 1);
        }
        rank = atomicAdd(&h_cnt[slot], 1);
    }
    __syncthreads();
    if (live && rank == 0) h_base[slot] = atomicAdd(&counts[key], h_cnt[slot]);
    __syncthreads();
    return live ? h_base[slot] + rank : 0;
}

// The same grouping without the arrival positions: the atomics return nothing, so the wave does not wait for them.
__device__ __forceinline__ void wave_bucket_count(int *__restrict__ counts, int key, bool live)
{
    const int lane = threadIdx.x & 63;
    bool todo = live;
    for (int round = 0; round < 4; ++round) {
        const unsigned long long pending = __ballot(todo);
        if (pending == 0ULL) break;
        const int leader = __ffsll((long long)pending) - 1;
        const int lkey = __builtin_amdgcn_readlane(key, leader);
        const bool mine = todo && key == lkey;
        const unsigned long long grp = __ballot(mine);
        if (lane == leader) atomicAdd(&counts[lkey], __popcll(grp));
        if (mine) todo = false;
    }
    if (todo) atomicAdd(&counts[key], 1);
}

// MapDev::sc_dist -- Chebyshev distance, in super-cells, from every super-cell to the nearest occupied
// one (separable: distance along x, then min over y of max(|dy|, .), then the same over z), capped at
// kScReach + 1.  A query whose super-cell is d super-cells from anything has no point closer than
// (d - 1) * 8h: the matcher answers "no neighbour within maxDist" from this one look-up.
__device__ __forceinline__ void scdist_cell(const int *__restrict__ in, int nsx, int nsy, int nsz, int axis, int first,
                                            int *__restrict__ out, int c)
{
    const int x = c % nsx, y = (c / nsx) % nsy, z = c / (nsx * nsy);
    const int pos = axis == 0 ? x : (axis == 1 ? y : z), len = axis == 0 ? nsx : (axis == 1 ? nsy : nsz);
    const int stride = axis == 0 ? 1 : (axis == 1 ? nsx : nsx * nsy);
    int best = kScReach + 1;
    for (int d = -kScReach; d <= kScReach; ++d) {
        const int p = pos + d;
        if (p < 0 || p >= len) continue;
        const int v = in[c + d * stride];
        // first pass reads occupancy flags (occupied = distance 0), the others read distances
        const int dv = first ? (v > 0 ? 0 : kScReach + 1) : v;
        best = min(best, max(abs(d), dv));
    }
    out[c] = best;
}

// three-phase exclusive scan over `n` ints (n up to 2^27)
#ifndef PGICP_CHUNK_COPIES
#define PGICP_CHUNK_COPIES 32
#endif
constexpr int kChunkCopies = PGICP_CHUNK_COPIES;   // partial copies of the scan's chunk sums (a multiple of the 8 XCDs)
constexpr int kQueueCounterStride = 32;            // ints between the queue counters of two segments: one 128-byte line each
// the outlier filter's selection tables (k_select.inc; the fast matcher feeds them too)
constexpr int kSelBits = 12;
constexpr int kSelBins = 1 << kSelBits;
constexpr int kSelStride = kSelBins + 8;       // ints per problem: the table, the compact list's cursor, then (selection with
                                               // a guess) the number of finite distances and of distances below the band
// The band of squared distances a selection with a guess compacts (k_select.inc): around the last selection's result.  An
// iteration's second selection can only come out at or below its first; the first selections of a run's early iterations
// follow a threshold that falls by factors, the later ones one that moves by per cents.
template <typename T>
__device__ __forceinline__ void sel_band_of(const ProblemDev &P, int second, T &lo, T &hi)
{
    const T q = (T)(second || !(P.qraw1 > 0.0) ? P.qraw : P.qraw1);
    // a hint of the previous call's same iteration (ProblemDev::qhint): two octaves either side for a first selection; for a
    // second one, whose guess is this iteration's first selection (it can only come out at or below it), only the band's low end
    const double hint = P.iters < 4 ? P.qhint[second ? 1 : 0][P.iters] : 0.0;
    if (hint > 0.0) {
        if (!second) { lo = (T)(hint * 0.25); hi = (T)(hint * 4.0); return; }
        if (P.iters == 0 && P.far_mode) { lo = (T)fmin((double)q * 0.85, hint * 0.25); hi = q; return; }
    }
    // (a run's first iteration of a scan that has run ahead of its map -- far mode: an eighth of the queries queued -- ends far
    // below its first selection, which saw upper bounds for all of them)
    if (second) { lo = q * (P.iters == 0 && P.far_mode ? (T)(1.0 / 1024.0) : (T)0.85); hi = q; }
    // (the first corrections of a run shrink the quantile by one or two orders of magnitude -- from the initial error's scale to
    // the point spacing's: ten octaves below the guess are in the band then, a slice of it is still a few hundred keys)
    else { lo = q * (P.iters <= 3 ? (T)(1.0 / 1024.0) : (T)0.5); hi = q * (T)1.25; }
}
// the correctly rounded square root in T (libpointmatcher's std::sqrt / Eigen's .norm() on the host)
__device__ __forceinline__ float sqrt_rn_t(float v) { return __builtin_sqrtf(v); }    // (correctly rounded; __fsqrt_rn is the native 1-ulp one)
__device__ __forceinline__ double sqrt_rn_t(double v) { return __builtin_sqrt(v); }

__device__ __forceinline__ int block_exclusive_scan_1024(int v, int *lds /*>=17 ints*/, int &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    if (wid == 0) {
        int w = (lane < (int)(blockDim.x >> 6)) ? lds[lane] : 0;
        int winc = w;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int t = __shfl_up(winc, o, 64);
            if (lane >= o) winc += t;
        }
        if (lane < 16) lds[lane] = winc - w;      // exclusive wave offsets
        if (lane == 15) lds[16] = winc;
    }
    __syncthreads();
    total = lds[16];
    const int res = lds[wid] + inc - v;
    __syncthreads();
    return res;
}

__global__ __launch_bounds__(1024) void k_scan_block_sums(const int *__restrict__ in, int n, int *__restrict__ block_sums)
{
    __shared__ int lds[32];
    const long long base = (long long)blockIdx.x * kScanChunk + threadIdx.x * 4;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) if (base + k < n) s += in[base + k];
    int total;
    block_exclusive_scan_1024(s, lds, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_scan_sums_inplace(int *__restrict__ block_sums, int nb)
{
    __shared__ int lds[32];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? block_sums[i] : 0;
        int total;
        const int ex = block_exclusive_scan_1024(v, lds, total);
        if (i < nb) block_sums[i] = ex + carry;
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void k_scan_final(const int *__restrict__ in, int n, const int *__restrict__ block_offs,
                                                      int *__restrict__ out /* n+1 */, int *__restrict__ cursor, int skip_empty)
{
    __shared__ int lds[32];
    const long long base = (long long)blockIdx.x * kScanChunk + threadIdx.x * 4;
    if (skip_empty && blockIdx.x + 1 < gridDim.x && block_offs[blockIdx.x + 1] == block_offs[blockIdx.x]) {
        // nothing counted in this chunk: every entry is the running offset (block-uniform branch)
        const int ex0 = block_offs[blockIdx.x];
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (base + k < n) { out[base + k] = ex0; if (cursor) cursor[base + k] = ex0; }
        return;
    }
    int v[4];
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = (base + k < n) ? in[base + k] : 0; s += v[k]; }
    int total;
    int ex = block_exclusive_scan_1024(s, lds, total) + block_offs[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + k < n) { out[base + k] = ex; if (cursor) cursor[base + k] = ex; }
        ex += v[k];
    }
    if (base <= n - 1 && n - 1 < base + 4) out[n] = ex;    // the thread holding the last element
}

// Exclusive scan of in[0 .. len) into out[0 .. len]: out[len] is the total.  len >= 1 (every caller returns early on an empty
// input).  block_sums: scan_scratch_ints(len) ints, one per block.  A block per kScanChunk elements suffices, also when len is a
// multiple of the chunk: k_scan_final has the thread that holds element len - 1 write out[len] after its own, and a block past
// that element would read and write nothing.
static void launch_exclusive_scan(hipStream_t st, const int *in, int len, int *out, int *block_sums)
{
    const int nb = (int)scan_scratch_ints((size_t)len);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(1024), 0, st, in, len, block_sums);
    hipLaunchKernelGGL(k_scan_sums_inplace, dim3(1), dim3(1024), 0, st, block_sums, nb);
    hipLaunchKernelGGL(k_scan_final, dim3(nb), dim3(1024), 0, st, in, len, (const int *)block_sums, out, (int *)nullptr, 0);
}

// ---------------------------------------------------------------------------
// Batched index build: n clouds in one set of launches (blockIdx.y = cloud).  Counting, the prefix scan
// and the scatter run on the concatenation of all clouds' points and cells, so a batch of loop-closure
// candidate maps costs a dozen launches instead of a dozen per map.
// ---------------------------------------------------------------------------
// per cloud: stats[0..2] = fixed-point coordinate sums (int64), stats[3..5] = min keys, stats[6..8] = max keys
template <typename T>
__global__ __launch_bounds__(256) void k_centroid_bbox_b(const BuildDesc<T> *__restrict__ descs, unsigned long long *__restrict__ stats)
{
    const BuildDesc<T> &d = descs[blockIdx.y];
    const T *xyz = d.xyz;
    const int stride = d.xstride, m = d.m;
    unsigned long long *st = stats + 9 * (long long)blockIdx.y;
    long long s[3] = {0, 0, 0};
    double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double v = (double)xyz[i * stride + a];
            s[a] += __double2ll_rn(v * 16777216.0);
            mn[a] = fmin(mn[a], v);
            mx[a] = v == v ? fmax(mx[a], v) : HUGE_VAL;
        }
    }
    if ((long long)blockIdx.x * blockDim.x >= m) return;
    // wave results meet in LDS; ONE wave per block then issues the nine atomics (every wave doing so cost
    // 370 us on a 2M-point cloud: ~4000 contended 64-bit atomics per address)
    __shared__ long long w_sum[4][3];
    __shared__ double w_lo[4][3], w_hi[4][3];
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        long long sv = s[a];
        double lo = mn[a], hi = mx[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sv += __shfl_down(sv, o, 64);
            lo = fmin(lo, __shfl_down(lo, o, 64));
            hi = fmax(hi, __shfl_down(hi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) { w_sum[wid][a] = sv; w_lo[wid][a] = lo; w_hi[wid][a] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        long long sv = 0;
        double lo = HUGE_VAL, hi = -HUGE_VAL;
        for (int w = 0; w < 4; w++) { sv += w_sum[w][a]; lo = fmin(lo, w_lo[w][a]); hi = fmax(hi, w_hi[w][a]); }
        atomicAdd(&st[a], (unsigned long long)sv);
        atomicMin(&st[3 + a], ordered_key(lo));
        atomicMax(&st[6 + a], ordered_key(hi));
    }
}

// MapDev::near -- for every 2x2x2 BLOCK of cells a nearby OCCUPIED cell.  Pass -1 picks an occupied cell of
// the block itself; three separable sweeps over blocks follow (nearest answer along x, then the best of the
// neighbouring answers in y, then in z).  Answers travel as 6-bit cell offsets from the block's first cell.
// A heuristic, not a nearest-cell guarantee: the matcher only uses it to give a query that starts in empty
// space a first candidate, so that its exact ring search prunes from the first row on.  (Per cell this table
// cost three sweeps over a grid that is 99 % empty: 1.7 ms of a 4.2 ms map build.)
__device__ __forceinline__ int near_pack(int dx, int dy, int dz) { return (dx + 32) | ((dy + 32) << 6) | ((dz + 32) << 12); }
__device__ __forceinline__ int near_dist(int v, int ax, int ay, int az)
{
    // squared distance (in half cells) from the block's centre to the centre of the cell at offset v + (ax, ay, az)
    const int dx = 2 * ((v & 63) - 32 + ax) - 1, dy = 2 * (((v >> 6) & 63) - 32 + ay) - 1, dz = 2 * (((v >> 12) & 63) - 32 + az) - 1;
    return dx * dx + dy * dy + dz * dz;
}

template <typename T>
__global__ __launch_bounds__(256) void k_near_b(const BuildDesc<T> *__restrict__ descs, int pass, const unsigned *__restrict__ occ,
                                                 int *__restrict__ tmp_a, int *__restrict__ tmp_b, int *__restrict__ near)
{
    const BuildDesc<T> &d = descs[blockIdx.y];
    const int nx = d.g.nx, ny = d.g.ny, nz = d.g.nz;
    const int nbx = (nx + 1) >> 1, nby = (ny + 1) >> 1, nbz = (nz + 1) >> 1;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;         // blocks <= cells <= 2^26: 32-bit index arithmetic
    if (b >= nbx * nby * nbz) return;
    const int reach_c = d.near_reach < 1 ? 1 : (d.near_reach > kNearReach ? kNearReach : d.near_reach);
    const int reach = (reach_c + 1) >> 1;                        // in blocks
    const int brow = b / nbx;
    const int bx = b - brow * nbx, bz = brow / nby, by = brow - bz * nby;
    if (pass < 0) {
        // (which cells of the block hold points: the occupancy bits -- one bit per search cell, written with the tables, whatever
        // kind of table the maps carry)
        const unsigned *ob = occ + d.obase;
        int found = -1;
        for (int k = 0; k < 2 && found < 0; ++k)
            for (int j = 0; j < 2 && found < 0; ++j) {
                const int y = 2 * by + j, z = 2 * bz + k;
                if (y >= ny || z >= nz) continue;
                const int c0 = 2 * bx + nx * (y + ny * z);
                if (ob[c0 >> 5] >> (c0 & 31) & 1u) found = near_pack(0, j, k);
                else if (2 * bx + 1 < nx && (ob[(c0 + 1) >> 5] >> ((c0 + 1) & 31) & 1u)) found = near_pack(1, j, k);
            }
        near[d.cbase + b] = found;                                // (sweep input; overwritten by the last pass)
    } else if (pass == 0) {
        const int *in = near + d.cbase;
        int found = -1;
        for (int t = 0; t <= reach && found < 0; ++t) {
            if (bx - t >= 0 && in[b - t] >= 0) found = in[b - t] - 2 * t;             // the x offset sits in the low bits
            else if (bx + t < nbx && in[b + t] >= 0) found = in[b + t] + 2 * t;
        }
        tmp_a[d.cbase + b] = found;
    } else if (pass == 1) {
        const int *in = tmp_a + d.cbase;
        int best = -1, bd = 0x7FFFFFFF;
        for (int t = -reach; t <= reach; ++t) {
            if (by + t < 0 || by + t >= nby) continue;
            const int v = in[b + t * nbx];
            if (v < 0) continue;
            const int dist = near_dist(v, 0, 2 * t, 0);
            if (dist < bd) { bd = dist; best = v + 2 * t * 64; }
        }
        tmp_b[d.cbase + b] = best;
    } else {
        const int *in = tmp_b + d.cbase;
        const int plane = nbx * nby;
        int best = -1, bd = 0x7FFFFFFF;
        for (int t = -reach; t <= reach; ++t) {
            if (bz + t < 0 || bz + t >= nbz) continue;
            const int v = in[b + t * plane];
            if (v < 0) continue;
            const int dist = near_dist(v, 0, 0, 2 * t);
            if (dist < bd) { bd = dist; best = v + 2 * t * 4096; }
        }
        int out = -1;
        if (best >= 0)
            out = (2 * bx + (best & 63) - 32) + nx * ((2 * by + ((best >> 6) & 63) - 32) + ny * (2 * bz + ((best >> 12) & 63) - 32));
        near[d.cbase + b] = out;
    }
}

// MapDev::sc_wit -- for every super-cell the slot of one point of a nearest occupied super-cell (Chebyshev, as
// sc_dist; the first point of that super-cell in layout order), or -1 beyond kWitReach.  A query the matcher
// could give no candidate at all -- a scan point over ground the map does not hold yet -- tests this one point:
// if it lies within maxDist, "a neighbour exists" is settled and the point is the seed of the next iteration;
// without it every such query walked super-cell rings in the wave-per-query path (70 % of that kernel's time
// in a fleet's first iterations).
template <typename T>
__global__ __launch_bounds__(256) void k_sc_first_b(const BuildDesc<T> *__restrict__ descs, const int *__restrict__ sc_count,
                                                     const int *__restrict__ cell_start, int *__restrict__ sc_first,
                                                     const uint4 *__restrict__ sw, const int *__restrict__ ostart)
{
    const BuildDesc<T> &d = descs[blockIdx.y];
    const int C = blockIdx.x * blockDim.x + threadIdx.x;
    if (C >= d.nsc) return;
    const int nx = d.g.nx, ny = d.g.ny, nz = d.g.nz;
    const int nsx = (nx + 7) >> 3, nsy = (ny + 7) >> 3;
    int first = -1;
    if (sc_count[d.sbase + C] > 0) {
        const int X = C % nsx, Y = (C / nsx) % nsy, Z = C / (nsx * nsy);
        const int *cs = cell_start + d.cbase;
        const int xa = 8 * X, xb = min(8 * X + 8, nx);
        for (int r = 0; r < 64 && first < 0; ++r) {
            const int y = 8 * Y + (r & 7), z = 8 * Z + (r >> 3);
            if (y >= ny || z >= nz) continue;
            const int row = nx * (y + ny * z);
            int a, b;
            if (sw) {                                  // the succinct table: search cell c = fine cell c * kx
                const int fa = (row + xa) * d.kx, fb = (row + xb) * d.kx;
                const int ra = succ_rank(load_word(sw + d.wbase, fa >> 6), fa & 63), rb = succ_rank(load_word(sw + d.wbase, fb >> 6), fb & 63);
                a = 0; b = 0;
                if (ra != rb) { a = ostart[ra]; b = ostart[rb]; }
            } else { a = cs[row + xa]; b = cs[row + xb]; }
            if (b > a) first = a;
        }
    }
    sc_first[d.sbase + C] = first;
}

// MapDev::sc_ext -- per super-cell the box of its OCCUPIED CELLS (offsets from the grid origin; min > max: empty), read off
// the occupancy bits: one thread per super-cell, 64 rows of eight bits each.  The wave-per-query walk tests a super-cell
// by this box, not by its 8 x 8 x 8 cube: ground and walls are thin slices of a cube, and a walker that has to prove
// "nothing within maxDist" otherwise opens every occupied cube its ball touches.  (The exact box of the POINTS was built
// first: scanning them per super-cell cost 0.55-3 ms on the 2 M-pt sliding map -- half a million super-cells, dense where
// occupied --, growing the boxes with atomics while the points are placed 0.8 ms and a sixth of the loop-closing rate.  A
// cell is 1/8 of the cube's edge: nearly all of the pruning for none of the cost.)
template <typename T>
__global__ __launch_bounds__(256) void k_sc_extent_b(const BuildDesc<T> *__restrict__ descs, const int *__restrict__ sc_count,
                                                      const unsigned *__restrict__ occ, float *__restrict__ sc_ext)
{
    const BuildDesc<T> &d = descs[blockIdx.y];
    const int C = blockIdx.x * blockDim.x + threadIdx.x;
    if (C >= d.nsc) return;
    const float inf = __int_as_float(0x7f800000);
    float *e = sc_ext + 6 * (d.sbase + C);
    if (sc_count[d.sbase + C] <= 0) { e[0] = inf; e[1] = inf; e[2] = inf; e[3] = 0.0f; e[4] = 0.0f; e[5] = 0.0f; return; }
    const int nx = d.g.nx, ny = d.g.ny, nz = d.g.nz;
    const int nsx = (nx + 7) >> 3, nsy = (ny + 7) >> 3;
    const int X = C % nsx, Y = (C / nsx) % nsy, Z = C / (nsx * nsy);
    const unsigned *o = occ + d.obase;
    const unsigned xmask = 0xFFu >> max(0, 8 * X + 8 - nx);      // the cells of the span that exist
    unsigned xs = 0u, ys = 0u, zs = 0u;                          // which x / y / z offsets of the cube hold a point
    for (int r = 0; r < 64; ++r) {
        const int y = 8 * Y + (r & 7), z = 8 * Z + (r >> 3);
        if (y >= ny || z >= nz) continue;
        const long long c0 = 8 * X + (long long)nx * (y + (long long)ny * z);
        const int w = (int)(c0 >> 5), sh = (int)(c0 & 31);
        const unsigned bits = (sh <= 24 ? o[w] >> sh : (o[w] >> sh) | (o[w + 1] << (32 - sh))) & xmask;   // (the table has a spare word)
        if (bits) { xs |= bits; ys |= 1u << (r & 7); zs |= 1u << (r >> 3); }
    }
    const float h = (float)d.g.h;
    // (cell borders as floats may sit a rounding off the T-typed ones the cells were assigned with: the walk subtracts the
    // grid's margin, 2 % of a cell, from every box distance)
    e[0] = (float)(8 * X + (__ffs((int)xs) - 1)) * h; e[3] = (float)(8 * X + (32 - __clz((int)xs))) * h;
    e[1] = (float)(8 * Y + (__ffs((int)ys) - 1)) * h; e[4] = (float)(8 * Y + (32 - __clz((int)ys))) * h;
    e[2] = (float)(8 * Z + (__ffs((int)zs) - 1)) * h; e[5] = (float)(8 * Z + (32 - __clz((int)zs))) * h;
    if (!xs) { e[0] = inf; e[1] = inf; e[2] = inf; e[3] = 0.0f; e[4] = 0.0f; e[5] = 0.0f; }
}

template <typename T>
__global__ __launch_bounds__(256) void k_sc_wit_b(const BuildDesc<T> *__restrict__ descs, const int *__restrict__ sc_dist,
                                                   const int *__restrict__ sc_first, int *__restrict__ sc_wit)
{
    const BuildDesc<T> &d = descs[blockIdx.y];
    const int C = blockIdx.x * blockDim.x + threadIdx.x;
    if (C >= d.nsc) return;
    const int nsx = (d.g.nx + 7) >> 3, nsy = (d.g.ny + 7) >> 3, nsz = (d.g.nz + 7) >> 3;
    const int X = C % nsx, Y = (C / nsx) % nsy, Z = C / (nsx * nsy);
    const int r = sc_dist[d.sbase + C];
    int wit = -1;
    if (r == 0) wit = sc_first[d.sbase + C];
    else if (r <= kWitReach) {
        // some super-cell of the shell at Chebyshev distance r is occupied: the first in (z, y, x) order wins
        for (int dz = -r; dz <= r && wit < 0; ++dz) {
            const int z = Z + dz;
            if (z < 0 || z >= nsz) continue;
            for (int dy = -r; dy <= r && wit < 0; ++dy) {
                const int y = Y + dy;
                if (y < 0 || y >= nsy) continue;
                const bool face = dz == r || dz == -r || dy == r || dy == -r;
                for (int dx = -r; dx <= r && wit < 0; dx += face ? 1 : 2 * r) {
                    const int x = X + dx;
                    if (x < 0 || x >= nsx) continue;
                    wit = sc_first[d.sbase + x + nsx * (y + nsy * z)];
                }
            }
        }
    }
    sc_wit[d.sbase + C] = wit;
}

// super-cell distance maps: one block per cloud, three sweeps separated by block barriers
template <typename T>
__global__ __launch_bounds__(1024) void k_scdist_b(const BuildDesc<T> *__restrict__ descs, const int *__restrict__ sc_count,
                                                    int *__restrict__ tmp_a, int *__restrict__ tmp_b, int *__restrict__ sc_dist)
{
    const BuildDesc<T> &d = descs[blockIdx.x];
    const int nsx = (d.g.nx + 7) >> 3, nsy = (d.g.ny + 7) >> 3, nsz = (d.g.nz + 7) >> 3;
    const int n = d.nsc;
    int *ta = tmp_a + d.cbase, *tb = tmp_b + d.cbase;         // ncells >= nsc: the cell scratch is large enough
    for (int c = threadIdx.x; c < n; c += blockDim.x) scdist_cell(sc_count + d.sbase, nsx, nsy, nsz, 0, 1, ta, c);
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += blockDim.x) scdist_cell(ta, nsx, nsy, nsz, 1, 0, tb, c);
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += blockDim.x) scdist_cell(tb, nsx, nsy, nsz, 2, 0, sc_dist + d.sbase, c);
}

// the same sweeps one launch each, for clouds whose super-cell grid is too large for one block
template <typename T>
__global__ __launch_bounds__(256) void k_scdist_pass_b(const BuildDesc<T> *__restrict__ descs, int pass, const int *__restrict__ sc_count,
                                                        int *__restrict__ tmp_a, int *__restrict__ tmp_b, int *__restrict__ sc_dist)
{
    const BuildDesc<T> &d = descs[blockIdx.y];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d.nsc) return;
    const int nsx = (d.g.nx + 7) >> 3, nsy = (d.g.ny + 7) >> 3, nsz = (d.g.nz + 7) >> 3;
    int *ta = tmp_a + d.cbase, *tb = tmp_b + d.cbase;
    if (pass == 0) scdist_cell(sc_count + d.sbase, nsx, nsy, nsz, 0, 1, ta, c);
    else if (pass == 1) scdist_cell(ta, nsx, nsy, nsz, 1, 0, tb, c);
    else scdist_cell(tb, nsx, nsy, nsz, 2, 0, sc_dist + d.sbase, c);
}
