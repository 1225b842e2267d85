// k_vardist.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): KDTreeVarDistMatcher's per-point
// search radii (include/pgicp_vardist.h).
//
// The matcher resolves every pair exactly under maxDist; the pairs come out in ascending (distance, index) order, so the kNN within
// r_i is that list with the entries beyond r_i * r_i cut from its tail.  k_vardist_cut makes the cut into a SECOND pair of arrays:
// the matcher's own slot / d2 / none_r seed its next pass and stay as it left them (slot -1 with none_r is the seeded matcher's
// proof that nothing lies within maxDist; a pair cut at r_i < maxDist has a neighbour there).

// pgicp_arm_reading_radii, device input: one problem's values (src[i * stride]) into the context's packed copy; flag: a value that
// is negative or a NaN was met (+inf is a radius: it cuts nothing)
template <typename T>
__global__ __launch_bounds__(256) void k_vardist_stage(const T *__restrict__ src, int stride, int n, T *__restrict__ dst, int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T v = src[(long long)i * stride];
    dst[i] = v;
    if (!(v >= (T)0)) atomicOr(flag, 1);
}

// One pair a lane, over the pairs of every active problem that is not done.  radii: the armed rows in the callers' point order
// (radii_off[problem]: where the problem's row starts, -1: it has none -- its pairs are copied as they are); order: the reading
// sort's permutation (sorted position -> caller's index), as k_noise_count reads the noise rows.  A pair is kept when it has a
// neighbour and d2 <= r * r, the product formed in T (ChainDev::max_dist2 is formed the same way); otherwise it is "no match":
// slot -1, distance +inf.
template <typename T>
__global__ __launch_bounds__(256) void k_vardist_cut(const ProblemDev *__restrict__ probs, const int *__restrict__ active,
                                                     const int *__restrict__ slot, const T *__restrict__ d2, const int *__restrict__ order,
                                                     const T *__restrict__ radii, const long long *__restrict__ radii_off,
                                                     int *__restrict__ slot_cut, T *__restrict__ d2_cut)
{
    const int prob = active[blockIdx.y];
    const ProblemDev &P = probs[prob];
    if (P.done) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= pairs_n(P)) return;
    const long long at = pairs_off(P) + e;
    int s = slot[at];
    T v = d2[at];
    const long long roff = radii_off[prob];
    if (roff >= 0 && s >= 0) {
        const int i = P.knn == 1 ? e : e / P.knn;
        const T r = radii[roff + order[P.off + i]];
        if (!(v <= r * r)) { s = -1; v = __builtin_huge_val(); }
    }
    slot_cut[at] = s;
    d2_cut[at] = v;
}

// The quantile filters (TrimmedDist / MedianDist) select over the cut distances; a cap derived from them says nothing about the
// search: the next matcher pass is uncapped again, as k_robust_finish leaves it
__global__ __launch_bounds__(64) void k_vardist_reset(ProblemDev *__restrict__ probs, const int *__restrict__ active, int n_active)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_active) return;
    ProblemDev &P = probs[active[a]];
    if (P.done) return;
    P.rlimit = __longlong_as_double(0x7FF0000000000000LL);
    P.n_refined = 0;
}

template <typename T>
void launch_vardist_stage(hipStream_t st, const T *src, int stride, int n, T *dst, int *flag)
{
    hipLaunchKernelGGL(k_vardist_stage<T>, dim3(cdiv(n, 256)), dim3(256), 0, st, src, stride, n, dst, flag);
}
template <typename T>
void launch_vardist_cut(hipStream_t st, const ProblemDev *probs, const int *active, int n_active, int max_pairs, const int *slot, const T *d2,
                        const int *order, const T *radii, const long long *radii_off, int *slot_cut, T *d2_cut)
{
    hipLaunchKernelGGL(k_vardist_cut<T>, dim3(cdiv(max_pairs, 256), n_active), dim3(256), 0, st, probs, active, slot, d2, order, radii, radii_off,
                       slot_cut, d2_cut);
}
void launch_vardist_reset(hipStream_t st, ProblemDev *probs, const int *active, int n_active)
{
    hipLaunchKernelGGL(k_vardist_reset, dim3(cdiv(n_active, 64)), dim3(64), 0, st, probs, active, n_active);
}

#define INSTANTIATE_VARDIST(T)                                                                                                         \
    template void launch_vardist_stage<T>(hipStream_t, const T *, int, int, T *, int *);                                               \
    template void launch_vardist_cut<T>(hipStream_t, const ProblemDev *, const int *, int, int, const int *, const T *, const int *,   \
                                        const T *, const long long *, int *, T *);
INSTANTIATE_VARDIST(float)
INSTANTIATE_VARDIST(double)
#undef INSTANTIATE_VARDIST
