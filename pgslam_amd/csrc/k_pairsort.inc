// k_pairsort.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): the stable LSD radix sort of
// (64-bit key, index) pairs that VoxelGrid, OctreeGrid and NormalSpace run.  A file of its own: three filters call it, none owns it.
//
// 8 bits a pass, over the bits the caller names only: per tile of kPairTile pairs a digit histogram (k_pair_hist), one scan of the
// [digit][tile] counts, and a stable scatter (k_pair_scatter: the rank of a pair among the equal digits of its wave from 8 ballots,
// waves and rounds in input order).  A caller's key kernel writes key[0] / idx[0] with idx[i] = i: the input is in index order, so
// equal keys end in ascending index.  Scratch: PairSort (kernels.hpp).

// per tile: the count of each digit; hist[d * nb + tile]
__global__ __launch_bounds__(256) void k_pair_hist(const unsigned long long *__restrict__ key, int n, int shift, int nb, int *__restrict__ hist)
{
    __shared__ int cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kPairTile;
    for (int r = 0; r < kPairTile / 256; r++) {
        const long long e = base + r * 256 + threadIdx.x;
        if (e < n) atomicAdd(&cnt[(int)((key[e] >> shift) & 255)], 1);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * nb + blockIdx.x] = cnt[threadIdx.x];
}

// stable scatter of one pass: off = the exclusive scan of hist
__global__ __launch_bounds__(256) void k_pair_scatter(const unsigned long long *__restrict__ key, const int *__restrict__ idx, int n, int shift, int nb,
                                                      const int *__restrict__ off, unsigned long long *__restrict__ key_out, int *__restrict__ idx_out)
{
    __shared__ int cnt[4][256];
    __shared__ int run[256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    run[threadIdx.x] = off[(long long)threadIdx.x * nb + blockIdx.x];
    const unsigned long long below = (1ULL << lane) - 1ULL;
    const long long base = (long long)blockIdx.x * kPairTile;
    for (int r = 0; r < kPairTile / 256; r++) {
        const long long e = base + r * 256 + threadIdx.x;
        const bool valid = e < n;
        unsigned long long k = 0;
        int id = 0, d = 0;
        if (valid) { k = key[e]; id = idx[e]; d = (int)((k >> shift) & 255); }
        // the lanes of this wave with the same digit
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const unsigned long long m = __ballot((d >> b) & 1);
            same &= ((d >> b) & 1) ? m : ~m;
        }
        const int rank = __popcll(same & below), wcnt = __popcll(same);
        for (int q = 0; q < 4; q++) cnt[q][threadIdx.x] = 0;
        __syncthreads();
        if (valid && rank == wcnt - 1) cnt[w][d] = wcnt;
        __syncthreads();
        {   // thread t owns digit t: the waves' offsets in order
            int acc = run[threadIdx.x];
            for (int q = 0; q < 4; q++) { const int c = cnt[q][threadIdx.x]; cnt[q][threadIdx.x] = acc; acc += c; }
            run[threadIdx.x] = acc;
        }
        __syncthreads();
        if (valid) { const int dst = cnt[w][d] + rank; key_out[dst] = k; idx_out[dst] = id; }
        __syncthreads();
    }
}

// the passes over bits [0, bits) of the pairs in key[cur] / idx[cur], ping-ponging; returns the side that holds the sorted order
int launch_pair_sort(hipStream_t st, const PairSort &w, int n, int bits, int cur)
{
    const dim3 b256(256);
    const int nt = cdiv(n, kPairTile);
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(k_pair_hist, dim3(nt), b256, 0, st, (const unsigned long long *)w.key[cur], n, shift, nt, w.hist);
        launch_exclusive_scan(st, w.hist, 256 * nt, w.hoff, w.bsum);
        hipLaunchKernelGGL(k_pair_scatter, dim3(nt), b256, 0, st, (const unsigned long long *)w.key[cur], (const int *)w.idx[cur], n, shift, nt,
                           (const int *)w.hoff, w.key[cur ^ 1], w.idx[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
}
