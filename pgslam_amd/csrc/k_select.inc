// k_select.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): outlier filter: exact order statistic of the finite squared distances.

// ---------------------------------------------------------------------------
// outlier filter: exact order statistic of the finite squared distances
// (radix select on the IEEE bit pattern, 11 bits per level; one block/problem)
// ---------------------------------------------------------------------------
template <typename T>
__device__ void trim_select_block(const T *__restrict__ d2, int n, T ratio, T &limit_out, int &nf_out)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    __shared__ int hist[2048];
    __shared__ int lds_scan[32];
    __shared__ U s_prefix;
    __shared__ long long s_k;
    __shared__ int s_nf;
    U prefix = 0;
    int done_bits = 0;
    long long k = 0;
    const U inf_key = Bits<T>::key(Bits<T>::inf());
    while (done_bits < KB) {
        const int width = (KB - done_bits) >= 11 ? 11 : (KB - done_bits);
        const int shift = KB - done_bits - width;
        for (int b = threadIdx.x; b < 2048; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        // 8 independent loads in flight per thread: with one load per iteration this loop is
        // latency bound (one block owns a whole problem, measured 68 us per selection)
        for (int base = threadIdx.x; base < n; base += 8 * blockDim.x) {
            U keys[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * blockDim.x;
                keys[u] = i < n ? Bits<T>::key(d2[i]) : inf_key;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const U key = keys[u];
                if (key >= inf_key) continue;                     // +inf (no neighbour) is not a value
                if (done_bits == 0 || (key >> (KB - done_bits)) == prefix)
                    atomicAdd(&hist[(int)((key >> shift) & (U)((1u << width) - 1u))], 1);
            }
        }
        __syncthreads();
        // block scan over 2048 bins: 2 bins per thread (blockDim = 1024)
        const int b0 = 2 * threadIdx.x;
        const int h0 = hist[b0], h1 = hist[b0 + 1];
        int total;
        const int ex = block_exclusive_scan_1024(h0 + h1, lds_scan, total);
        if (done_bits == 0) {
            if (threadIdx.x == 0) {
                s_nf = total;
                long long kk;
                if (ratio == (T)1) kk = (long long)total - 1;
                else {
                    kk = (long long)((T)total * ratio);           // `values.size() * quantile` evaluated in T
                    if (kk > (long long)total - 1) kk = (long long)total - 1;
                }
                s_k = kk < 0 ? 0 : kk;
            }
            __syncthreads();
            k = s_k;
            const int nf0 = s_nf;
            __syncthreads();                       // everyone has read s_k before the owner rewrites it
            if (nf0 == 0) { limit_out = Bits<T>::inf(); nf_out = 0; return; }
        }
        if (k >= ex && k < ex + h0) { s_prefix = (prefix << width) | (U)b0; s_k = k - ex; }
        else if (k >= ex + h0 && k < ex + h0 + h1) { s_prefix = (prefix << width) | (U)(b0 + 1); s_k = k - ex - h0; }
        __syncthreads();
        prefix = s_prefix;
        k = s_k;
        done_bits += width;
        __syncthreads();
    }
    limit_out = Bits<T>::val(prefix);
    nf_out = s_nf;
}

// ---------------------------------------------------------------------------
// The batched outlier filter spreads the selection over the chip (one block per problem took 45 us --
// three serial passes over the problem's distances -- and was half of a single scan's iteration):
//   k_sel_hist    every block histograms the top kSelBits key bits of its span of distances in LDS (plain
//                 LDS atomics) and adds the non-empty bins to the problem's table,
//   k_sel_filter  every block finds the bin holding the wanted rank (4096-bin scan, repeated per block: no
//                 cross-block hand-over inside a launch) and appends its distances of that bin -- a few per
//                 cent -- to the problem's compact key list, one global atomic per flush,
//   k_sel_final   one block per problem finishes the radix select on the compact list and clears the table.
// The result is the same exact order statistic as trim_select_block's.  Measured per selection: 17 us for one
// 100k scan, 28 us average for 128 of them.
// ---------------------------------------------------------------------------
constexpr int kSelTile = 2048;                 // distances per block of the two wide passes

template <typename T>
__device__ __forceinline__ long long select_rank(int total, T ratio)
{
    long long kk;
    if (ratio == (T)1) kk = (long long)total - 1;
    else {
        kk = (long long)((T)total * ratio);               // `values.size() * quantile` evaluated in T
        if (kk > (long long)total - 1) kk = (long long)total - 1;
    }
    return kk < 0 ? 0 : kk;
}

// bin of the wanted rank, the rank inside that bin and the number of finite values; NT threads, all return
// the same answer (total == 0: bin = -1)
template <typename T, int NT>
__device__ __forceinline__ void sel_pick_bin(const int *__restrict__ gh, T ratio, int *lds_scan, int *s_out /*3 ints*/,
                                             int &bin, int &krem, int &total)
{
    constexpr int PER = kSelBins / NT;
    int h[PER];
    int sum = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) { h[u] = gh[PER * threadIdx.x + u]; sum += h[u]; }
    const int ex = block_exclusive_scan_1024(sum, lds_scan, total);
    if (total > 0) {
        const long long k = select_rank<T>(total, ratio);
        if (k >= ex && k < (long long)ex + sum) {
            int acc = ex;
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                if (k >= acc && k < (long long)acc + h[u]) { s_out[0] = PER * threadIdx.x + u; s_out[1] = (int)(k - acc); }
                acc += h[u];
            }
        }
    } else if (threadIdx.x == 0) { s_out[0] = -1; s_out[1] = 0; }
    __syncthreads();
    bin = s_out[0];
    krem = s_out[1];
    __syncthreads();
}

__device__ __forceinline__ bool sel_skip(const ProblemDev &P, int second)
{
    return P.done || (second == 1 && P.n_refined == 0);      // the re-selection only runs if the lazy path refined something
}

// the quantile a selection takes: the chain's TrimmedDist ratio, or (second == 2: the selection after k_var_trim) the problem's
// VarTrimmedDist ratio of this iteration -- a float, exact in T
template <typename T>
__device__ __forceinline__ T sel_ratio(const ProblemDev &P, const ChainDev<T> &ch, int second)
{
    return second == 2 ? (T)P.vt_ratio : ch.trim_ratio;
}

// what every final stage of a selection leaves in the problem record (thread 0 of the problem's block)
template <typename T>
__device__ __forceinline__ void sel_store(ProblemDev &P, const ChainDev<T> &ch, int second, T limit, int n_finite)
{
    if (second) P.n_refined = 0;
    else P.prev_limit = P.rlimit;             // the fast pass of this iteration capped its search with it
    // a MaxDistOutlierFilter in the chain multiplies its weights in: pairs beyond its distance are dropped too, so the
    // threshold the minimiser works with is the smaller of the two; the lazy search must be exact up to that AND up to
    // the quantile itself (a MedianDist factor below 1 keeps less than the median it is computed from)
    P.limit = (double)fmin(limit * ch.trim_scale, ch.outlier_max_d2);        // (x 1 is exact: TrimmedDist unchanged)
    P.rlimit = fmax((double)limit, P.limit);
    if (second == 2) {
        // VarTrimmedDist: no positive finite distance (no outlier to filter) keeps nothing -- the solve reports NO_MATCH; the
        // next matcher pass must again find every pair exactly (the ratio is chosen over all of them): no search cap
        if (P.vt_ratio < 0.0) P.limit = -1.0;
        P.rlimit = __longlong_as_double(0x7FF0000000000000LL);
    }
    // GenericDescriptor soft mode: its maximum is over every pair -- the next matcher pass must again find every pair exactly
    if (ch.gd_mode == PGICP_DESC_FILTER_SOFT) P.rlimit = __longlong_as_double(0x7FF0000000000000LL);
    P.qraw = (double)limit;
    if (!second) P.qraw1 = (double)limit;
    if (P.iters < 4) P.qrec[second ? 1 : 0][P.iters] = (double)limit;
    P.n_finite = n_finite;
}

// An iteration's FIRST selection also clears the matcher's segmented queue counters of its problem for the next
// iteration (they are dead once the queue has been compacted: no memset launch per iteration) and reads off them what
// the matcher queued in this pass, over the problem's eight segments: "far mode" for the next pass.
__device__ __forceinline__ void sel_queue_counters(ProblemDev &P, int prob, int second, int *__restrict__ seg_count)
{
    if (seg_count && !second && threadIdx.x < 64) {
        int q = threadIdx.x < 8 ? seg_count[kQueueCounterStride * (prob * 8 + (int)threadIdx.x)] : 0;
        if (threadIdx.x < 8) seg_count[kQueueCounterStride * (prob * 8 + (int)threadIdx.x)] = 0;
        q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
        if (threadIdx.x == 0) P.far_mode = (long long)q * 8 > (long long)P.n ? 1 : 0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_sel_hist(const ProblemDev *__restrict__ probs, const T *__restrict__ d2, int second,
                                                   const int *__restrict__ active, int *__restrict__ tables, int span)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    const int prob = active[blockIdx.y];
    const ProblemDev &P = probs[prob];
    if (sel_skip(P, second)) return;
    const int first = blockIdx.x * span;               // this block's distances: [first, first + span)
    const int np = pairs_n(P);
    const long long poff = pairs_off(P);
    if (first >= np) return;
    const int last = min(first + span, np);
    __shared__ int hist[kSelBins];
    for (int b = threadIdx.x; b < kSelBins; b += 256) hist[b] = 0;
    __syncthreads();
    const U inf_key = Bits<T>::key(Bits<T>::inf());
    for (int base = first; base < last; base += kSelTile) {
        U keys[kSelTile / 256];
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u) {
            const int i = base + u * 256 + threadIdx.x;
            keys[u] = i < last ? Bits<T>::key(d2[poff + i]) : inf_key;
        }
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u) {
            const int bin = (int)(keys[u] >> (KB - kSelBits));
            // plain LDS atomics: aggregating the lanes of a wave per distinct bin first was measured 3.6x
            // SLOWER (37 us against 10 us per pass at 128 x 100k) -- the LDS unit takes same-address adds well
            if (keys[u] < inf_key) atomicAdd(&hist[bin], 1);      // +inf (no neighbour) is not a value
        }
    }
    __syncthreads();
    int *gh = tables + (long long)prob * kSelStride;
    for (int b = threadIdx.x; b < kSelBins; b += 256) {
        const int v = hist[b];
        if (v) atomicAdd(&gh[b], v);
    }
}

constexpr int kSelStage = 2 * kSelTile;

template <typename T>
__global__ __launch_bounds__(256) void k_sel_filter(const ProblemDev *__restrict__ probs, const T *__restrict__ d2,
                                                     ChainDev<T> ch, int second, const int *__restrict__ active,
                                                     int *__restrict__ tables, typename Bits<T>::U *__restrict__ keys_out,
                                                     int span)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    const int prob = active[blockIdx.y];
    const ProblemDev &P = probs[prob];
    if (sel_skip(P, second)) return;
    const int first = blockIdx.x * span;
    const int np = pairs_n(P);
    const long long poff = pairs_off(P);
    if (first >= np) return;
    const int last = min(first + span, np);
    __shared__ int lds_scan[32];
    __shared__ int s_pick[3];
    __shared__ int s_cnt, s_base;
    __shared__ U stage[kSelStage];
    if (threadIdx.x == 0) s_cnt = 0;
    int *gh = tables + (long long)prob * kSelStride;
    // the first tile's loads are in flight while the bin is picked
    U keys[kSelTile / 256];
#pragma unroll
    for (int u = 0; u < kSelTile / 256; ++u) {
        const int i = first + u * 256 + threadIdx.x;
        keys[u] = i < last ? Bits<T>::key(d2[poff + i]) : ~(U)0;
    }
    int bin, krem, total;
    sel_pick_bin<T, 256>(gh, sel_ratio<T>(P, ch, second), lds_scan, s_pick, bin, krem, total);     // barriers inside
    if (total == 0) return;
    for (int base = first; base < last; base += kSelTile) {
        if (base != first) {
#pragma unroll
            for (int u = 0; u < kSelTile / 256; ++u) {
                const int i = base + u * 256 + threadIdx.x;
                keys[u] = i < last ? Bits<T>::key(d2[poff + i]) : ~(U)0;
            }
        }
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u) {
            // the padding key (all ones) is beyond +inf's bin; a few per cent of the lanes hit
            if ((int)(keys[u] >> (KB - kSelBits)) == bin) stage[atomicAdd(&s_cnt, 1)] = keys[u];
        }
        __syncthreads();
        const int cnt = s_cnt;
        // flush when another tile might not fit (and at the end)
        if (cnt > 0 && (cnt + kSelTile > kSelStage || base + kSelTile >= last)) {
            if (threadIdx.x == 0) s_base = atomicAdd(&gh[kSelBins], cnt);
            __syncthreads();                                // everyone has read s_cnt by now
            U *dst = keys_out + poff + s_base;
            for (int j = threadIdx.x; j < cnt; j += 256) dst[j] = stage[j];
            if (threadIdx.x == 0) s_cnt = 0;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(kSelectBlock) void k_sel_final(ProblemDev *__restrict__ probs, ChainDev<T> ch, int second,
                                                             const int *__restrict__ active, int *__restrict__ tables,
                                                             const typename Bits<T>::U *__restrict__ keys_in, int *__restrict__ seg_count)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    const int prob = active[blockIdx.x];
    ProblemDev &P = probs[prob];
    if (sel_skip(P, second)) return;
    sel_queue_counters(P, prob, second, seg_count);
    __shared__ int hist[2048];
    __shared__ int lds_scan[32];
    __shared__ int s_pick[3];
    __shared__ U s_prefix;
    __shared__ int s_k;
    int *gh = tables + (long long)prob * kSelStride;
    int bin, krem, total;
    sel_pick_bin<T, kSelectBlock>(gh, sel_ratio<T>(P, ch, second), lds_scan, s_pick, bin, krem, total);
    const int cnt = gh[kSelBins];
    __syncthreads();
    // leave the table clean for the next selection of this problem
    for (int b = threadIdx.x; b < kSelBins + 1; b += kSelectBlock) gh[b] = 0;
    T limit = Bits<T>::inf();
    if (total > 0) {
        const U *keys = keys_in + pairs_off(P);
        U prefix = (U)bin;
        int done_bits = kSelBits;
        int k = krem;
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
        limit = Bits<T>::val(prefix);
    }
    if (threadIdx.x == 0) sel_store<T>(P, ch, second, limit, total);
}

// ---------------------------------------------------------------------------
// Selection with a guess (every selection but an ICP run's very first): two launches instead of three, one pass over the
// distances instead of two.  Thresholds move little from one selection to the next -- an iteration's second selection can
// only come out at or below its first (the lazy matcher path lowers distances, never raises them), and the next iteration's
// lies near this one's -- so the distances are not histogrammed first:
//   k_sel_band    counts, per problem, the finite distances and those BELOW a band around the guess, and compacts the
//                 distances inside the band (a quarter to a third of N around the 85 % quantile; a few per cent for the
//                 second selection) to the problem's key list;
//   k_sel_final2  one block per problem: if the wanted rank falls inside the band, the radix select runs on the compact
//                 list; if the guess was off (the first iterations of a poor initial pose) the block selects over all of
//                 the problem's distances itself -- exact either way.
// ---------------------------------------------------------------------------
constexpr int kSelSub = 128;                  // slices of a band (k_sel_band counts them, k_sel_final2 selects inside one)
constexpr int kSelSubBytes = 32768;           // LDS for the keys of one slice in the final stage (8 192 float keys, 4 096 double keys)

// slice of a band's key: (key - lo_key) >> shift, shift the smallest with (hi_key - lo_key) >> shift < kSelSub
template <typename T>
__device__ __forceinline__ int sel_sub_shift(typename Bits<T>::U lo_key, typename Bits<T>::U hi_key)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    if (hi_key <= lo_key) return 0;
    const U range = hi_key - lo_key;
    const int bits = KB - (KB == 32 ? __clz((unsigned)range) : __clzll((unsigned long long)range));     // range < 2^bits
    return bits > 7 ? bits - 7 : 0;
}

template <typename T>
__global__ __launch_bounds__(256) void k_sel_band(const ProblemDev *__restrict__ probs, const T *__restrict__ d2, int second,
                                                   const int *__restrict__ active, int *__restrict__ tables,
                                                   typename Bits<T>::U *__restrict__ keys_out, int span)
{
    using U = typename Bits<T>::U;
    const int prob = active[blockIdx.y];
    const ProblemDev &P = probs[prob];
    if (sel_skip(P, second)) return;
    const int first = blockIdx.x * span;
    const int np = pairs_n(P);
    const long long poff = pairs_off(P);
    if (first >= np) return;
    const int last = min(first + span, np);
    __shared__ int s_cnt, s_base, s_nf, s_below;
    __shared__ U stage[kSelStage];
    __shared__ int s_sub[kSelSub];
    if (threadIdx.x == 0) { s_cnt = 0; s_nf = 0; s_below = 0; }
    if (threadIdx.x < kSelSub) s_sub[threadIdx.x] = 0;
    __syncthreads();
    T lo_v, hi_v;
    sel_band_of<T>(P, second, lo_v, hi_v);
    const U inf_key = Bits<T>::key(Bits<T>::inf());
    // (distances are >= +0: the order of the bit patterns is the order of the values; a NaN guess gives an empty band)
    const U lo_key = lo_v >= (T)0 ? Bits<T>::key(lo_v) : inf_key, hi_key = hi_v >= (T)0 ? Bits<T>::key(hi_v) : (U)0;
    const int sub_shift = sel_sub_shift<T>(lo_key, hi_key);
    int *gh = tables + (long long)prob * kSelStride;
    int nf = 0, below = 0;
    for (int base = first; base < last; base += kSelTile) {
        U keys[kSelTile / 256];
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u) {
            const int i = base + u * 256 + threadIdx.x;
            keys[u] = i < last ? Bits<T>::key(d2[poff + i]) : ~(U)0;
        }
#pragma unroll
        for (int u = 0; u < kSelTile / 256; ++u) {
            const U key = keys[u];
            if (key < inf_key) {                                  // +inf (no neighbour) is not a value
                ++nf;
                if (key < lo_key) ++below;
                else if (key <= hi_key) {
                    stage[atomicAdd(&s_cnt, 1)] = key;
                    atomicAdd(&s_sub[(int)((key - lo_key) >> sub_shift)], 1);      // the band in kSelSub equal slices of key space
                }
            }
        }
        __syncthreads();
        const int cnt = s_cnt;
        if (cnt > 0 && (cnt + kSelTile > kSelStage || base + kSelTile >= last)) {
            if (threadIdx.x == 0) s_base = atomicAdd(&gh[kSelBins], cnt);
            __syncthreads();
            U *dst = keys_out + poff + s_base;
            for (int j = threadIdx.x; j < cnt; j += 256) dst[j] = stage[j];
            if (threadIdx.x == 0) s_cnt = 0;
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nf += __shfl_xor(nf, o, 64); below += __shfl_xor(below, o, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_nf, nf); atomicAdd(&s_below, below); }
    __syncthreads();
    if (threadIdx.x == 0) { if (s_nf) atomicAdd(&gh[kSelBins + 1], s_nf); if (s_below) atomicAdd(&gh[kSelBins + 2], s_below); }
    // (the slices' counts travel in the first entries of the problem's histogram table, which the three-launch selection
    // leaves clean and k_sel_final2 clears again)
    if (threadIdx.x < kSelSub && s_sub[threadIdx.x]) atomicAdd(&gh[threadIdx.x], s_sub[threadIdx.x]);
}

__device__ int g_sel_fallbacks = 0;            // diagnostics: selections whose guess was off (k_sel_final2 selected over everything)

template <typename T>
__global__ __launch_bounds__(kSelectBlock) void k_sel_final2(ProblemDev *__restrict__ probs, const T *__restrict__ d2, ChainDev<T> ch,
                                                              int second, const int *__restrict__ active, int *__restrict__ tables,
                                                              const typename Bits<T>::U *__restrict__ keys_in, int *__restrict__ seg_count)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    const int prob = active[blockIdx.x];
    ProblemDev &P = probs[prob];
    if (sel_skip(P, second)) return;
    sel_queue_counters(P, prob, second, seg_count);
    __shared__ int hist[2048];
    __shared__ int lds_scan[32];
    __shared__ U s_prefix;
    __shared__ int s_k, s_slice, s_n;
    constexpr int kSelSubCap = kSelSubBytes / (int)sizeof(U);
    __shared__ U buf[kSelSubCap];
    int *gh = tables + (long long)prob * kSelStride;
    const int cnt = gh[kSelBins], total = gh[kSelBins + 1], below = gh[kSelBins + 2];
    const int my_slice = threadIdx.x < kSelSub ? gh[threadIdx.x] : 0;
    __syncthreads();
    if (threadIdx.x < 3) gh[kSelBins + threadIdx.x] = 0;           // clean for the next selection of this problem
    if (threadIdx.x < kSelSub) gh[threadIdx.x] = 0;
    T limit = Bits<T>::inf();
    int n_finite = total;
    bool selected = false;
    if (total > 0) {
        const long long kk = select_rank<T>(total, sel_ratio<T>(P, ch, second));
        if (kk >= below && kk < (long long)below + cnt) {
            // the slice of the band that holds the rank (counted by k_sel_band), its keys into LDS in one pass over the
            // band's list, the select inside LDS over the bits a slice's keys differ in
            T lo_s, hi_s;
            sel_band_of<T>(P, second, lo_s, hi_s);
            if (lo_s >= (T)0 && hi_s >= lo_s) {
                const U lo_k = Bits<T>::key(lo_s), hi_k = Bits<T>::key(hi_s);
                const int sub_shift = sel_sub_shift<T>(lo_k, hi_k);
                int tot;
                const int ex = block_exclusive_scan_1024(my_slice, lds_scan, tot);
                const int kb = (int)(kk - below);
                if (threadIdx.x == 0) { s_slice = -1; s_n = 0; }
                __syncthreads();
                if (threadIdx.x < kSelSub && kb >= ex && kb < ex + my_slice) { s_slice = threadIdx.x; s_k = kb - ex; s_prefix = (U)my_slice; }
                __syncthreads();
                const int slice = s_slice, n_slice = slice >= 0 ? (int)s_prefix : 0;
                int k = s_k;
                __syncthreads();
                if (slice >= 0 && tot == cnt && n_slice <= kSelSubCap) {
                    const U *keys = keys_in + pairs_off(P);
                    // (eight loads in flight per thread: one block owns the problem, a load per trip is latency bound)
                    for (int j0 = threadIdx.x; j0 < cnt; j0 += 8 * kSelectBlock) {
                        U kk8[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) { const int j = j0 + u * kSelectBlock; kk8[u] = j < cnt ? keys[j] : hi_k + (U)1; }
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (kk8[u] <= hi_k && (int)((kk8[u] - lo_k) >> sub_shift) == slice) buf[atomicAdd(&s_n, 1)] = kk8[u];
                    }
                    __syncthreads();
                    // keys of the slice: lo_k + (slice << sub_shift) + r, r < 2^sub_shift
                    const U base_key = lo_k + ((U)slice << sub_shift);
                    int done = 0;                       // bits of r fixed so far, from the top
                    U r_prefix = 0;
                    while (done < sub_shift) {
                        const int width = (sub_shift - done) >= 11 ? 11 : (sub_shift - done);
                        const int shift = sub_shift - done - width;
                        for (int b = threadIdx.x; b < 2048; b += kSelectBlock) hist[b] = 0;
                        __syncthreads();
                        for (int j = threadIdx.x; j < n_slice; j += kSelectBlock) {
                            const U r = buf[j] - base_key;
                            if (done == 0 || (r >> (sub_shift - done)) == r_prefix) atomicAdd(&hist[(int)((r >> shift) & (U)((1u << width) - 1u))], 1);
                        }
                        __syncthreads();
                        const int b0 = 2 * threadIdx.x;
                        const int h0 = hist[b0], h1 = hist[b0 + 1];
                        int t2;
                        const int e2 = block_exclusive_scan_1024(h0 + h1, lds_scan, t2);
                        if (k >= e2 && k < e2 + h0) { s_prefix = (r_prefix << width) | (U)b0; s_k = k - e2; }
                        else if (k >= e2 + h0 && k < e2 + h0 + h1) { s_prefix = (r_prefix << width) | (U)(b0 + 1); s_k = k - e2 - h0; }
                        __syncthreads();
                        r_prefix = s_prefix;
                        k = s_k;
                        done += width;
                        __syncthreads();
                    }
                    limit = Bits<T>::val(base_key + r_prefix);
                    selected = true;
                }
            }
        }
        if (selected) {
        } else if (kk >= below && kk < (long long)below + cnt) {
            const U *keys = keys_in + pairs_off(P);
            // the keys of a band share their leading bits (sign, exponent, a mantissa bit or two): the select starts below
            // them -- a first level over those bits would be tens of thousands of LDS atomics on two or three counters
            T lo_v, hi_v;
            sel_band_of<T>(P, second, lo_v, hi_v);
            const U lo_key = Bits<T>::key(lo_v), hi_key = Bits<T>::key(hi_v);
            int done_bits = 0;
            if (lo_v >= (T)0 && hi_v >= lo_v) {
                const U diff = lo_key ^ hi_key;
                done_bits = diff == 0 ? KB : (KB == 32 ? __clz((unsigned)diff) : __clzll((unsigned long long)diff));
            }
            U prefix = done_bits == 0 ? (U)0 : (done_bits >= KB ? lo_key : (U)(lo_key >> (KB - done_bits)));
            int k = (int)(kk - below);
            while (done_bits < KB) {
                const int width = (KB - done_bits) >= 11 ? 11 : (KB - done_bits);
                const int shift = KB - done_bits - width;
                for (int b = threadIdx.x; b < 2048; b += kSelectBlock) hist[b] = 0;
                __syncthreads();
                for (int j0 = threadIdx.x; j0 < cnt; j0 += 8 * kSelectBlock) {
                    U kk8[8];
                    bool in8[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int j = j0 + u * kSelectBlock; in8[u] = j < cnt; kk8[u] = in8[u] ? keys[j] : (U)0; }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (in8[u] && (done_bits == 0 || (kk8[u] >> (KB - done_bits)) == prefix))
                            atomicAdd(&hist[(int)((kk8[u] >> shift) & (U)((1u << width) - 1u))], 1);
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
            limit = Bits<T>::val(prefix);
        } else {
            // the wanted rank lies outside the band: this block selects over all of the problem's distances (three passes)
            if (threadIdx.x == 0) atomicAdd(&g_sel_fallbacks, 1);
            trim_select_block<T>(d2 + pairs_off(P), pairs_n(P), sel_ratio<T>(P, ch, second), limit, n_finite);
        }
    }
    if (threadIdx.x == 0) sel_store<T>(P, ch, second, limit, n_finite);
}

// Small problems (a 10 k-pt scan): the three launches above are launch-bound (3 x 5 us for a few microseconds of work, and
// three launches of host time); one block per problem runs the whole radix select over the problem's distances instead.
// Same order statistic, same bookkeeping.
template <typename T>
__global__ __launch_bounds__(kSelectBlock) void k_sel_small(ProblemDev *__restrict__ probs, const T *__restrict__ d2, ChainDev<T> ch,
                                                             int second, const int *__restrict__ active, int *__restrict__ seg_count)
{
    const int prob = active[blockIdx.x];
    ProblemDev &P = probs[prob];
    if (sel_skip(P, second)) return;
    T limit;
    int nf;
    trim_select_block<T>(d2 + pairs_off(P), pairs_n(P), sel_ratio<T>(P, ch, second), limit, nf);
    sel_queue_counters(P, prob, second, seg_count);
    if (threadIdx.x == 0) sel_store<T>(P, ch, second, limit, nf);
}

// stand-alone outlier weights for the stage-level API (one problem)
template <typename T>
__global__ __launch_bounds__(kSelectBlock) void k_trim_select_raw(const T *__restrict__ d2, int n, T ratio, T scale,
                                                                   T *__restrict__ limit_nf /* [0]=limit, [1]=nf */)
{
    T limit;
    int nf;
    trim_select_block<T>(d2, n, ratio, limit, nf);
    if (threadIdx.x == 0) { limit_nf[0] = limit * scale; limit_nf[1] = (T)nf; }
}

template <typename T>
__global__ __launch_bounds__(256) void k_weights(const T *__restrict__ d2, int n, const T *__restrict__ limit_nf,
                                                  T *__restrict__ w)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    w[i] = (d2[i] <= limit_nf[0]) ? (T)1 : (T)0;
}
