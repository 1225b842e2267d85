// k_elipsoids.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): ElipsoidsDataPointsFilter
// (include/pgicp_elipsoids.h).
//
// The filter shares SamplingSurfaceNormalDataPointsFilter's median-split tree: steps 1.-3. of k_ssn.inc (ssn_build_tree) run as they
// are -- the same keys, radix passes, levels and box list.  What is new is the end of the schedule:
//   4. k_elip_fuse: one thread per box; k_ssn_fuse's body (extent, mean, scatter in T in box order, jacobi3 in double, the maxBoxDim
//      and rank < 2 drops), then the shape values and the planarity drop (elipsoids_host.hpp, shared with the host form), then the
//      box's rows to the per-box scratch and the draw;
//   5. k_elip_compact: the kept points in index order, every requested row gathered from its box.
// FULL = false is the plain case (normals and means only, as k_ssn_fuse<T, false> writes them): no row pointer is passed and no
// row store is compiled.  FULL = true takes the ElipBox / ElipOut pointers; a null one is a row nobody asked for and is skipped.
// The arithmetic contract of kernels.hip holds (no contraction, sqrt_rn_t, correctly rounded divisions); every comparison is T's.

struct ElipNone {};

template <typename T, bool FULL>
__global__ __launch_bounds__(128) void k_elip_fuse(const T *__restrict__ X, int xs, int n, const int *__restrict__ lst, const SsnBox *__restrict__ boxes,
                                                   int nbox, int method, T ratio, T max_box, T min_planarity, unsigned long long seed, T eps,
                                                   int *__restrict__ keep, int *__restrict__ box_of, T *__restrict__ bnrm, T *__restrict__ bmean,
                                                   const int *__restrict__ box_count, int *__restrict__ fused,
                                                   typename std::conditional<FULL, ElipBox<T>, ElipNone>::type x = {})
{
    namespace eh = pgslam_amd::elipsoids;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbox || b >= *box_count) return;
    const SsnBox B = boxes[b];
    const int *L = lst + (long long)(B.axis < 3 ? B.axis : 0) * n + B.first;
    auto member = [&](int k) { return B.axis < 3 ? L[k] : B.first + k; };
    T lo[3], hi[3], sum[3] = {0, 0, 0};
    {
        const int i0 = member(0);
        for (int a = 0; a < 3; a++) { lo[a] = X[(long long)i0 * xs + a]; hi[a] = lo[a]; }
    }
    for (int k = 0; k < B.count; k++) {
        const T *p = X + (long long)member(k) * xs;
        for (int a = 0; a < 3; a++) {
            const T v = p[a];
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
            sum[a] += v;
        }
    }
    T box = hi[0] - lo[0];
    if (hi[1] - lo[1] > box) box = hi[1] - lo[1];
    if (hi[2] - lo[2] > box) box = hi[2] - lo[2];
    if (box > max_box) return;
    const T mean[3] = {sum[0] / (T)B.count, sum[1] / (T)B.count, sum[2] / (T)B.count};
    const T mx = mean[0], my = mean[1], mz = mean[2];
    T c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
    for (int k = 0; k < B.count; k++) {
        const T *p = X + (long long)member(k) * xs;
        const T dx = p[0] - mx, dy = p[1] - my, dz = p[2] - mz;
        c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    double A[3][3] = {{(double)c00, (double)c01, (double)c02}, {(double)c01, (double)c11, (double)c12}, {(double)c02, (double)c12, (double)c22}};
    double V[3][3];
    jacobi3(A, V);
    const double ev[3] = {A[0][0], A[1][1], A[2][2]};
    int l = 0, h = 0;
    for (int k = 1; k < 3; k++) { if (ev[k] < ev[l]) l = k; if (ev[k] > ev[h]) h = k; }
    if (l == h) return;                                          // (mid would not name an eigenvalue)
    const int mid = 3 - l - h;
    if (!(eh::pick3(ev, h) > 0.0) || !(eh::pick3(ev, mid) > 3.0 * (double)eps * eh::pick3(ev, h))) return;      // rank < 2: the box is dropped
    // the shape values; the planarity drop comes after the rank test and before the draw, and a dropped box is not fused
    const eh::Shape<T> shape = eh::shape_of<T>(ev, l, mid, h);
    if (eh::dropped_by_planarity<T>(shape, min_planarity)) return;
    atomicAdd(fused, 1);
    eh::Rows<T> rows;
    rows.normal = bnrm + 3LL * b;
    rows.mean = bmean + 3LL * b;
    if constexpr (FULL) {
        if (x.beig) rows.eig = x.beig + 3LL * b;
        if (x.bvec) rows.vec = x.bvec + 9LL * b;
        if (x.bcov) rows.cov = x.bcov + 9LL * b;
        if (x.bweight) rows.weight = x.bweight + b;
        if (x.bshape) rows.shape = x.bshape + 3LL * b;
    }
    const T scatter[6] = {c00, c01, c02, c11, c12, c22};
    eh::assemble_rows<T>(B.count, mean, scatter, ev, V, l, mid, h, shape, rows);
    if constexpr (FULL) {
        if (x.bdens) {
            // pgicp_ssn_ext.h's density: one more walk over the members
            T r2 = 0;
            for (int k = 0; k < B.count; k++) {
                const T *p = X + (long long)member(k) * xs;
                const T dx = p[0] - mx, dy = p[1] - my, dz = p[2] - mz;
                const T q = (dx * dx + dy * dy) + dz * dz;
                if (q > r2) r2 = q;
            }
            const T r = sqrt_rn_t(r2);
            x.bdens[b] = (T)B.count / ((T)((4.0 / 3.0) * 3.14159265358979323846) * ((r * r) * r));
        }
    }
    if (method == 0) {
        for (int k = 0; k < B.count; k++) {
            const int i = member(k);
            const double u = (double)(seeded_mix(seed, i) >> 11) / 9007199254740992.0;
            if (!(u < (double)ratio)) continue;
            keep[i] = 1; box_of[i] = b;
        }
    } else {
        const int i = member(0);
        keep[i] = 1; box_of[i] = b;
    }
}

// the kept points in index order, as k_ssn_compact leaves them (coordinates, normal, index, descriptors), and with FULL every
// requested row of the point's box
template <typename T, bool FULL>
__global__ __launch_bounds__(256) void k_elip_compact(const T *__restrict__ X, int xs, int n, const int *__restrict__ lst,
                                                      const SsnBox *__restrict__ boxes, const int *__restrict__ keep, const int *__restrict__ pos,
                                                      const int *__restrict__ box_of, const T *__restrict__ bnrm, const T *__restrict__ bmean,
                                                      int method, const T *__restrict__ desc, int drows, int average,
                                                      T *__restrict__ out_xyz, int os, T *__restrict__ out_nrm, int ns, T *__restrict__ out_desc,
                                                      int *__restrict__ kept_idx,
                                                      typename std::conditional<FULL, ElipOut<T>, ElipNone>::type x = {})
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const long long o = pos[i];
    const int b = box_of[i];
    T *ox = out_xyz + o * os;
    if (method == 1) { ox[0] = bmean[3LL * b]; ox[1] = bmean[3LL * b + 1]; ox[2] = bmean[3LL * b + 2]; }
    else { const T *p = X + (long long)i * xs; ox[0] = p[0]; ox[1] = p[1]; ox[2] = p[2]; }
    if (out_nrm) { T *on = out_nrm + o * ns; on[0] = bnrm[3LL * b]; on[1] = bnrm[3LL * b + 1]; on[2] = bnrm[3LL * b + 2]; }
    if (kept_idx) kept_idx[o] = i;
    if constexpr (FULL) {
        if (x.eig) for (int r = 0; r < 3; r++) x.eig[3 * o + r] = x.box.beig[3LL * b + r];
        if (x.eigvec) for (int r = 0; r < 9; r++) x.eigvec[9 * o + r] = x.box.bvec[9LL * b + r];
        if (x.dens) x.dens[o] = x.box.bdens[b];
        if (x.cov) for (int r = 0; r < 9; r++) x.cov[9 * o + r] = x.box.bcov[9LL * b + r];
        if (x.weights) x.weights[o] = x.box.bweight[b];
        if (x.means) for (int r = 0; r < 3; r++) x.means[3 * o + r] = bmean[3LL * b + r];
        if (x.shapes) for (int r = 0; r < 3; r++) x.shapes[3 * o + r] = x.box.bshape[3LL * b + r];
    }
    if (desc) {
        T *od = out_desc + o * drows;
        if (method == 1 && average) {
            const SsnBox B = boxes[b];
            const int *L = lst + (long long)(B.axis < 3 ? B.axis : 0) * n + B.first;
            for (int r = 0; r < drows; r++) {
                T s = 0;
                for (int k = 0; k < B.count; k++) s += desc[(long long)(B.axis < 3 ? L[k] : B.first + k) * drows + r];
                od[r] = s / (T)B.count;
            }
        } else {
            const T *d = desc + (long long)i * drows;
            for (int r = 0; r < drows; r++) od[r] = d[r];
        }
    }
}

// The schedule of one call: SamplingSurfaceNormal's tree (ssn_build_tree), then the two kernels above.  x.box names the per-box
// scratch (elip_scratch), the other members of x the outputs; with none of them asked for the plain instantiations run.  Returns 0,
// or -1 when n / knn are out of range.
template <typename T>
int launch_elipsoids(hipStream_t st, const T *X, int xs, int n, int knn, int method, T ratio, T max_box, T min_planarity, unsigned long long seed,
                     const T *desc, int drows, int average, const SsnScratch &w, T *out_xyz, int os, T *out_nrm, int ns, T *out_desc,
                     int *kept_idx, int *counters /* [0] box slots, [1] boxes fused, [2] not finite, [3] kept */, const ElipOut<T> &x)
{
    if (n <= 0 || knn < 1 || (long long)n * 3 + 1 > 0x7FFFFFFFLL) return -1;
    long long nbox = 0;
    const int *lst = ssn_build_tree<T>(st, X, xs, n, knn, w, counters, nbox);
    const SsnBox *boxes = (const SsnBox *)w.boxes;
    const dim3 b256(256), b128(128);
    const T eps = std::numeric_limits<T>::epsilon();
    // 4. the boxes
    if (x.any())
        hipLaunchKernelGGL((k_elip_fuse<T, true>), dim3(cdiv(nbox, 128)), b128, 0, st, X, xs, n, lst, boxes, (int)nbox, method, ratio, max_box,
                           min_planarity, seed, eps, w.keep, w.box_of, (T *)w.bnrm, (T *)w.bmean, (const int *)counters, counters + 1, x.box);
    else
        hipLaunchKernelGGL((k_elip_fuse<T, false>), dim3(cdiv(nbox, 128)), b128, 0, st, X, xs, n, lst, boxes, (int)nbox, method, ratio, max_box,
                           min_planarity, seed, eps, w.keep, w.box_of, (T *)w.bnrm, (T *)w.bmean, (const int *)counters, counters + 1);
    // 5. the kept points in index order
    launch_exclusive_scan(st, w.keep, n, w.pos, w.bsum);
    if (x.any())
        hipLaunchKernelGGL((k_elip_compact<T, true>), dim3(cdiv(n, 256)), b256, 0, st, X, xs, n, lst, boxes, (const int *)w.keep, (const int *)w.pos,
                           (const int *)w.box_of, (const T *)w.bnrm, (const T *)w.bmean, method, desc, drows, average, out_xyz, os, out_nrm, ns,
                           out_desc, kept_idx, x);
    else
        hipLaunchKernelGGL((k_elip_compact<T, false>), dim3(cdiv(n, 256)), b256, 0, st, X, xs, n, lst, boxes, (const int *)w.keep, (const int *)w.pos,
                           (const int *)w.box_of, (const T *)w.bnrm, (const T *)w.bmean, method, desc, drows, average, out_xyz, os, out_nrm, ns,
                           out_desc, kept_idx);
    (void)hipMemcpyAsync(counters + 3, w.pos + n, sizeof(int), hipMemcpyDeviceToDevice, st);
    return 0;
}

template int launch_elipsoids<float>(hipStream_t, const float *, int, int, int, int, float, float, float, unsigned long long, const float *, int, int,
                                     const SsnScratch &, float *, int, float *, int, float *, int *, int *, const ElipOut<float> &);
template int launch_elipsoids<double>(hipStream_t, const double *, int, int, int, int, double, double, double, unsigned long long, const double *, int,
                                      int, const SsnScratch &, double *, int, double *, int, double *, int *, int *, const ElipOut<double> &);
