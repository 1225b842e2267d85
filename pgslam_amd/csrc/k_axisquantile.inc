// k_axisquantile.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): MaxQuantileOnAxisDataPointsFilter
// (include/pgicp_quantile.h): the exact k-th smallest of one coordinate over the points a filter list still keeps, and the cut at it.
//
// The selection is k_select.inc's three-stage radix select (k_sel_hist / k_sel_filter / k_sel_final) restated for SIGNED values:
//   k_aq_hist    every block histograms the top kSelBits key bits of its span's survivors in LDS and adds the non-empty bins to
//                the table (integer atomics: the table does not depend on arrival order),
//   k_aq_filter  every block finds the bin of the wanted rank (sel_pick_bin: the survivor count is the table's sum, the rank is
//                made from it in T, on the device) and appends its survivors' keys of that bin to the candidate list,
//   k_aq_final   one block finishes the select on the candidates and leaves {limit, k, values below limit} on the device,
//   k_aq_apply   keep[i] &= v_i < limit, with the limit read from there.
// Keys: the order-preserving map of the IEEE bits (negatives: all bits flipped; the rest: the sign bit flipped), after -0 has
// become +0 and every NaN the largest key -- the NaN-last order of the statement.  The candidate list holds n keys: a cloud
// that is planar on the axis puts every survivor into one bin, and the last stage then walks all of them (slower, still exact).
// The order of the candidates depends on the blocks' arrival; the last stage only counts them, so the result does not.

template <typename T>
__device__ __forceinline__ typename Bits<T>::U aq_key(T v)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    if (v != v) return ~(U)0;                                   // NaN: after +inf (whose key is below all ones)
    if (v == (T)0) return (U)1 << (KB - 1);                     // -0 and +0 are one value
    const U b = Bits<T>::key(v);
    return (b >> (KB - 1)) ? ~b : (b | ((U)1 << (KB - 1)));
}
// (the canonical value of a key: +0 for the zeros, the default quiet NaN for the NaNs)
template <typename T>
__device__ __forceinline__ T aq_val(typename Bits<T>::U key)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    if (key == ~(U)0) return Bits<T>::val(sizeof(T) == 4 ? (U)0x7FC00000u : (U)0x7FF8000000000000ULL);
    return Bits<T>::val((key >> (KB - 1)) ? (key ^ ((U)1 << (KB - 1))) : ~key);
}

// point i's key, if the list still keeps it (keep == null: a whole cloud)
template <typename T>
__device__ __forceinline__ bool aq_load(const T *__restrict__ feat, int stride, int dim, const int *__restrict__ keep, int i, int last,
                                        typename Bits<T>::U &key)
{
    key = 0;
    if (i >= last || (keep && !keep[i])) return false;
    key = aq_key<T>(feat[(long long)i * stride + dim]);
    return true;
}

template <typename T>
__global__ __launch_bounds__(256) void k_aq_hist(const T *__restrict__ feat, int stride, int dim, int n, const int *__restrict__ keep,
                                                  int *__restrict__ table, int span)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    const long long first = (long long)blockIdx.x * span;       // this block's points: [first, first + span)
    if (first >= n) return;
    const int last = (int)min(first + span, (long long)n);
    __shared__ int hist[kSelBins];
    for (int b = threadIdx.x; b < kSelBins; b += 256) hist[b] = 0;
    __syncthreads();
    for (int base = (int)first; base < last; base += kSelTile) {
        U keys[kSelTile / 256];
        bool in[kSelTile / 256];
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u) in[u] = aq_load<T>(feat, stride, dim, keep, base + u * 256 + (int)threadIdx.x, last, keys[u]);
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u)
            if (in[u]) atomicAdd(&hist[(int)(keys[u] >> (KB - kSelBits))], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kSelBins; b += 256) {
        const int v = hist[b];
        if (v) atomicAdd(&table[b], v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_aq_filter(const T *__restrict__ feat, int stride, int dim, int n, const int *__restrict__ keep,
                                                    T ratio, int *__restrict__ table, typename Bits<T>::U *__restrict__ keys_out, int span)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    const long long first = (long long)blockIdx.x * span;
    if (first >= n) return;
    const int last = (int)min(first + span, (long long)n);
    __shared__ int lds_scan[32];
    __shared__ int s_pick[3];
    __shared__ int s_cnt, s_base;
    __shared__ U stage[kSelStage];
    if (threadIdx.x == 0) s_cnt = 0;
    int bin, krem, total;
    sel_pick_bin<T, 256>(table, ratio, lds_scan, s_pick, bin, krem, total);     // barriers inside
    if (total == 0) return;
    for (int base = (int)first; base < last; base += kSelTile) {
        U keys[kSelTile / 256];
        bool in[kSelTile / 256];
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u) in[u] = aq_load<T>(feat, stride, dim, keep, base + u * 256 + (int)threadIdx.x, last, keys[u]);
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u)
            if (in[u] && (int)(keys[u] >> (KB - kSelBits)) == bin) stage[atomicAdd(&s_cnt, 1)] = keys[u];
        __syncthreads();
        const int cnt = s_cnt;                              // (at most kSelStage: flushed whenever another tile might not fit)
        if (cnt > 0 && (cnt + kSelTile > kSelStage || base + kSelTile >= last)) {
            if (threadIdx.x == 0) s_base = atomicAdd(&table[kSelBins], cnt);
            __syncthreads();                                // everyone has read s_cnt by now
            U *dst = keys_out + s_base;                     // (the bin's survivors, all blocks together: at most n)
            for (int j = threadIdx.x; j < cnt; j += 256) dst[j] = stage[j];
            if (threadIdx.x == 0) s_cnt = 0;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(kSelectBlock) void k_aq_final(T ratio, const int *__restrict__ table, const typename Bits<T>::U *__restrict__ keys,
                                                            AqResult *__restrict__ res)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    __shared__ int hist[2048];
    __shared__ int lds_scan[32];
    __shared__ int s_pick[3];
    __shared__ U s_prefix;
    __shared__ int s_k;
    int bin, krem, total;
    sel_pick_bin<T, kSelectBlock>(table, ratio, lds_scan, s_pick, bin, krem, total);
    const int cnt = table[kSelBins];
    U prefix = ~(U)0;                                       // (no survivor: the NaN key -- nothing is below it)
    int k = 0;
    if (total > 0) {
        prefix = (U)bin;
        int done_bits = kSelBits;
        k = krem;
        while (done_bits < KB) {
            const int width = (KB - done_bits) >= 11 ? 11 : (KB - done_bits);
            const int shift = KB - done_bits - width;
            for (int b = threadIdx.x; b < 2048; b += kSelectBlock) hist[b] = 0;
            __syncthreads();
            for (int j = threadIdx.x; j < cnt; j += kSelectBlock) {
                const U key = keys[j];
                if ((key >> (KB - done_bits)) == prefix) atomicAdd(&hist[(int)((key >> shift) & (U)((1u << width) - 1u))], 1);
            }
            __syncthreads();
            const int b0 = 2 * threadIdx.x;
            const int h0 = hist[b0], h1 = hist[b0 + 1];
            int tot;
            const int ex = block_exclusive_scan_1024(h0 + h1, lds_scan, tot);
            if (k >= ex && k < ex + h0) { s_prefix = (prefix << width) | (U)b0; s_k = k - ex; }
            else if (k >= ex + h0 && k < ex + h0 + h1) { s_prefix = (prefix << width) | (U)(b0 + 1); s_k = k - ex - h0; }
            __syncthreads();
            prefix = s_prefix;
            k = s_k;
            done_bits += width;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        // k: by now the rank among the values EQUAL to the limit, so rank - k values lie below it; a NaN limit has nothing below
        const int rank = total > 0 ? (int)select_rank<T>(total, ratio) : 0;
        const T limit = aq_val<T>(prefix);
        res->limit_bits = (unsigned long long)Bits<T>::key(limit);
        res->k = rank;
        res->below = prefix == ~(U)0 ? 0 : rank - k;
        res->count = total;
        res->pad_ = 0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_aq_apply(const T *__restrict__ feat, int stride, int dim, int n, const AqResult *__restrict__ res,
                                                   int *__restrict__ keep)
{
    using U = typename Bits<T>::U;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const T limit = Bits<T>::val((U)res->limit_bits);
    if (!(feat[(long long)i * stride + dim] < limit)) keep[i] = 0;       // (a NaN on either side: not kept)
}
