// k_vartrim.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): VarTrimmedDistOutlierFilter's
// inlier ratio (optimizeInlierRatio, pgicp.h), one block per problem.

// ---------------------------------------------------------------------------
// [EXT] VarTrimmedDistOutlierFilter: for every active problem
//   1. gather the finite POSITIVE squared distances of its pairs (their number: c) into a key list,
//   2. sort the list: LSD radix sort on the IEEE bit pattern (a positive value sorts as its unsigned bits), 8-bit digits, a pass
//      skipped when every key has the same digit; the scatter is stable through a per-wave multi-split (eight ballots give the
//      lanes that share a digit) and a per-digit scan over the block's sixteen waves,
//   3. prefix sums in double over the window's prefix, FRMS_j, its argmin (lowest j on a tie),
//   4. ProblemDev::vt_ratio = (float)j* / (float)P -- or -1 when c == 0 (no outlier to filter: the selection keeps nothing).
// The selection that follows (second == 2, k_select.inc) reads vt_ratio instead of ChainDev::trim_ratio.
// Sum order (pgicp.h): tiles of 1024 sorted values in sequence; inside a tile, an inclusive shuffle scan per wave of 64 plus the
// totals of the tile's earlier waves, plus the sum of the earlier tiles.
// ---------------------------------------------------------------------------
constexpr int kVtBlock = 1024;
constexpr int kVtWaves = kVtBlock / 64;

template <typename T>
__global__ __launch_bounds__(kVtBlock) void k_var_trim(ProblemDev *__restrict__ probs, const T *__restrict__ d2, const int *__restrict__ active,
                                                       typename Bits<T>::U *__restrict__ ka, typename Bits<T>::U *__restrict__ kb,
                                                       double min_ratio, double max_ratio, double lambda)
{
    using U = typename Bits<T>::U;
    constexpr int KB = Bits<T>::kBits;
    const int prob = active[blockIdx.x];
    ProblemDev &P = probs[prob];
    if (P.done) return;
    const int np = pairs_n(P);
    const long long poff = pairs_off(P);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long lt_mask = (1ULL << lane) - 1ULL;
    __shared__ int s_cnt;
    __shared__ int hist[256];
    __shared__ int base[256];
    __shared__ int wcnt[kVtWaves][256];
    __shared__ int lds_scan[32];
    __shared__ double s_wsum[kVtWaves];
    __shared__ double s_best[kVtWaves];
    __shared__ int s_bestj[kVtWaves];
    const U inf_key = Bits<T>::key(Bits<T>::inf());
    U *src = ka + poff, *dst = kb + poff;

    // 1. gather (the list's order is irrelevant: the sort's result is the sorted multiset)
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    for (int base0 = 0; base0 < np; base0 += kVtBlock) {
        const int i = base0 + (int)threadIdx.x;
        const U key = i < np ? Bits<T>::key(d2[poff + i]) : (U)0;
        const bool keep = key > (U)0 && key < inf_key;       // d > 0 and d != +inf (d2 >= +0: the bits order like the values)
        const unsigned long long m = __ballot(keep);
        int wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&s_cnt, __popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (keep) src[wbase + __popcll(m & lt_mask)] = key;
    }
    __syncthreads();
    const int c = s_cnt;
    if (c == 0) {
        if (threadIdx.x == 0) { P.vt_ratio = -1.0; P.vt_count = 0; }
        return;
    }

    // 2. LSD radix sort, 8 bits per pass
    for (int shift = 0; shift < KB; shift += 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < c; i += kVtBlock) atomicAdd(&hist[(int)((src[i] >> shift) & (U)255)], 1);
        __syncthreads();
        const int h = threadIdx.x < 256 ? hist[threadIdx.x] : 0;
        int tot;
        const int ex = block_exclusive_scan_1024(h, lds_scan, tot);
        if (threadIdx.x < 256) base[threadIdx.x] = ex;
        const bool one_digit = __syncthreads_or(h == c);
        if (one_digit) continue;                              // every key has this digit: the order stays as it is
        for (int t0 = 0; t0 < c; t0 += kVtBlock) {
            for (int e = threadIdx.x; e < kVtWaves * 256; e += kVtBlock) (&wcnt[0][0])[e] = 0;
            const int i = t0 + (int)threadIdx.x;
            const bool valid = i < c;
            const U key = valid ? src[i] : (U)0;
            const int dg = (int)((key >> shift) & (U)255);
            unsigned long long m = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (dg >> b) & 1;
                const unsigned long long bb = __ballot(bit);
                m &= bit ? bb : ~bb;
            }
            const int rank = __popcll(m & lt_mask);
            __syncthreads();                                  // wcnt is clear
            if (valid && rank == 0) wcnt[wid][dg] = __popcll(m);
            __syncthreads();
            if (threadIdx.x < 256) {
                int off = base[threadIdx.x];
                for (int w = 0; w < kVtWaves; ++w) { const int v = wcnt[w][threadIdx.x]; wcnt[w][threadIdx.x] = off; off += v; }
                base[threadIdx.x] = off;
            }
            __syncthreads();
            if (valid) dst[wcnt[wid][dg] + rank] = key;
            __syncthreads();                                  // (the next tile clears wcnt)
        }
        U *t = src; src = dst; dst = t;
    }

    // 3. the window, prefix sums in double, FRMS and its argmin
    const double Ptot = (double)np;
    const int min_el = (int)floor((double)((T)min_ratio * (T)np));       // `T(minRatio) * P` evaluated in T
    const int max_el = (int)floor((double)((T)max_ratio * (T)np));
    const int wend = min(max_el, c);
    double best = __longlong_as_double(0x7FF0000000000000LL);
    int bestj = 0x7FFFFFFF;
    double carry = 0.0;
    for (int t0 = 0; t0 < wend && min_el < wend; t0 += kVtBlock) {
        const int j = t0 + (int)threadIdx.x;
        double v = j < wend ? (double)Bits<T>::val(src[j]) : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        if (lane == 63) s_wsum[wid] = v;
        __syncthreads();
        double before = carry, tile = 0.0;
        for (int w = 0; w < kVtWaves; ++w) { const double s = s_wsum[w]; if (w < wid) before += s; tile += s; }
        __syncthreads();                                      // everyone has read s_wsum
        if (j >= min_el && j < wend) {
            const double S = before + v;
            const double id = (double)(j + 1);
            const double f = id / Ptot;
            const double a = 1.0 / pow(f, lambda);
            const double frms = a * a * S / id;
            if (frms < best) { best = frms; bestj = j; }      // (j grows per thread: a tie keeps the lower one)
        }
        carry += tile;
    }
    // block argmin, the lowest j on a tie
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bestj, o, 64);
        if (ob < best || (ob == best && oj < bestj)) { best = ob; bestj = oj; }
    }
    if (lane == 0) { s_best[wid] = best; s_bestj[wid] = bestj; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = s_best[0];
        int jb = s_bestj[0];
        for (int w = 1; w < kVtWaves; ++w)
            if (s_best[w] < b || (s_best[w] == b && s_bestj[w] < jb)) { b = s_best[w]; jb = s_bestj[w]; }
        const int jstar = min_el < wend && jb != 0x7FFFFFFF ? jb : min_el;      // an empty window: minEl
        const float tuned = (float)jstar / (float)np;                             // in float, as upstream casts it
        P.vt_ratio = (double)tuned;
        P.vt_count = c;
    }
}

template <typename T>
void launch_var_trim(hipStream_t st, ProblemDev *probs, const T *d2, const int *active, int n_active, void *keys_a, void *keys_b,
                     double min_ratio, double max_ratio, double lambda)
{
    using U = typename Bits<T>::U;
    hipLaunchKernelGGL(k_var_trim<T>, dim3(n_active), dim3(kVtBlock), 0, st, probs, d2, active, (U *)keys_a, (U *)keys_b, min_ratio, max_ratio, lambda);
}

template void launch_var_trim<float>(hipStream_t, ProblemDev *, const float *, const int *, int, void *, void *, double, double, double);
template void launch_var_trim<double>(hipStream_t, ProblemDev *, const double *, const int *, int, void *, void *, double, double, double);
