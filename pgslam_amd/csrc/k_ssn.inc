// k_ssn.inc -- part of kernels.hip (one translation unit, included inside namespace pgicp): the box filters,
// SamplingSurfaceNormalDataPointsFilter (pgicp_sampling_surface_normal_*, include/pgicp_ssn_ext.h) and ElipsoidsDataPointsFilter
// (include/pgicp_elipsoids.h).  The three entries run one schedule (launch_box_filter): they differ in the per-box rows they offer and
// in the planarity drop, which only Elipsoids has.
//
// [EXT] libpointmatcher SamplingSurfaceNormalDataPointsFilter as the oracle states it (oracle/icp_oracle.c,
// orc_sampling_surface_normal): a range of more than knn points is cut at the median of its widest CARRIED side, ordered by
// (coordinate, original index); a range of at most knn points is a box, fused in the order its parent's cut left it.
//
// The tree's shape does not depend on the data: a range of c points always splits into ceil(c / 2) and floor(c / 2), so
// the ranges of level d are segments of fixed boundaries, and only the cut axis of a segment and the order inside it depend
// on the coordinates.  So the build is level-synchronous:
//   1. the cloud is sorted ONCE per axis by (coordinate, index): three lists of point indices, concatenated into one array
//      of 3n entries, sorted together by an LSD radix sort of one bit per pass (a stable partition per pass: a scan of the
//      bit and a scatter), -0.0 made +0.0 first because the comparison treats them as equal;
//   2. per level, every segment picks its cut axis from its carried bounds, the points of its first `left` entries of the
//      cut axis's list are marked left, and all three lists are stable-partitioned inside every segment by that mark (one
//      scan over the 3n marks): every child stays sorted on every axis, as the parent's sort would have left it;
//   3. a child of at most knn points becomes a box whose member order is its range of the parent's cut-axis list; it is
//      left alone by the later levels, so that range still holds it at the end;
//   4. one thread per box fuses it (k_box_fuse: the oracle's sequential sums in T, jacobi3 in double, the same rank test; the
//      shape values, the planarity drop and the assembly of a box's rows are elipsoids_host.hpp's, shared with the host form);
//   5. the kept points are compacted in index order (k_box_compact), every requested row gathered from the point's box.
// The arithmetic contract of kernels.hip holds (no contraction); every comparison is T's.


// orderable key of a coordinate: unsigned order == T's order, -0.0 and +0.0 the same key
template <typename T>
__device__ __forceinline__ typename Bits<T>::U ssn_key(T v)
{
    using U = typename Bits<T>::U;
    const U sign = (U)1 << (Bits<T>::kBits - 1);
    U k = Bits<T>::key(v);
    if (k == sign) k = 0;                               // -0.0 -> +0.0
    return (k & sign) ? ~k : (k | sign);
}

// the three lists, unsorted (identity), their keys and the first pass's bit; any coordinate that is not finite is flagged
template <typename T>
__global__ __launch_bounds__(256) void k_ssn_keys(const T *__restrict__ X, int xs, int n, typename Bits<T>::U *__restrict__ keys,
                                                  int *__restrict__ lst, int *__restrict__ flag, int *__restrict__ bad)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;        // (3n < 2^31: the caller checks)
    if (q >= 3 * n) return;
    const int a = q / n, i = q - a * n;
    const T v = X[(long long)i * xs + a];
    if (!(v - v == (T)0)) atomicOr(bad, 1);            // NaN or +-inf
    const auto k = ssn_key<T>(v);
    keys[q] = k;
    lst[q] = i;
    flag[q] = (int)(k & 1);
}

// one radix pass: stable partition of every list by bit b (zeros first); writes the next pass's bit at the destination
template <typename T>
__global__ __launch_bounds__(256) void k_ssn_split(int n, int b, const typename Bits<T>::U *__restrict__ keys, const int *__restrict__ lst,
                                                   const int *__restrict__ flag, const int *__restrict__ scan,
                                                   typename Bits<T>::U *__restrict__ keys_out, int *__restrict__ lst_out,
                                                   int *__restrict__ flag_out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 3 * n) return;
    const int first = (q / n) * n;
    const int ones_before = scan[q] - scan[first];
    const int zeros = n - (scan[first + n] - scan[first]);
    const int dst = flag[q] ? first + zeros + ones_before : q - ones_before;
    const auto k = keys[q];
    keys_out[dst] = k;
    lst_out[dst] = lst[q];
    if (b + 1 < Bits<T>::kBits) flag_out[dst] = (int)((k >> (b + 1)) & 1);
}

// the root segment: the cloud's bounding box (the sorted lists' ends)
template <typename T>
__global__ void k_ssn_root(const T *__restrict__ X, int xs, int n, const int *__restrict__ lst, SsnSeg<T> *__restrict__ seg)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SsnSeg<T> s;
    s.first = 0; s.count = n; s.cut = 0; s.pad = 0;
    for (int a = 0; a < 3; a++) {
        s.lo[a] = X[(long long)lst[(long long)a * n] * xs + a];
        s.hi[a] = X[(long long)lst[(long long)a * n + n - 1] * xs + a];
    }
    seg[0] = s;
}

// one level, per segment: the cut axis (argmax of the carried sides, first maximum), the cut value, the two children (the
// next level's segments 2j, 2j + 1; count 0 below a box), and the children that are boxes
template <typename T>
__global__ __launch_bounds__(256) void k_ssn_level(const T *__restrict__ X, int xs, int n, int knn, int nseg, const int *__restrict__ lst,
                                                   SsnSeg<T> *__restrict__ seg, SsnSeg<T> *__restrict__ child, SsnBox *__restrict__ boxes,
                                                   int *__restrict__ box_count)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nseg) return;
    SsnSeg<T> s = seg[j];
    SsnSeg<T> L = s, R = s;
    if (s.count <= knn) {
        L.count = 0; R.count = 0;
        child[2 * j] = L; child[2 * j + 1] = R;
        return;
    }
    int cut = 0;
    for (int a = 1; a < 3; a++) if (s.hi[a] - s.lo[a] > s.hi[cut] - s.lo[cut]) cut = a;
    const int right = s.count / 2, left = s.count - right;
    const T cv = X[(long long)lst[(long long)cut * n + s.first + left] * xs + cut];
    seg[j].cut = cut;
    L.count = left; L.hi[cut] = cv;
    R.first = s.first + left; R.count = right; R.lo[cut] = cv;
    child[2 * j] = L; child[2 * j + 1] = R;
    if (left <= knn) { const int b = atomicAdd(box_count, 1); boxes[b].first = L.first; boxes[b].count = left; boxes[b].axis = cut; }
    if (right <= knn) { const int b = atomicAdd(box_count, 1); boxes[b].first = R.first; boxes[b].count = right; boxes[b].axis = cut; }
}

// one level, per position of the current segments: which side of the cut the point at that position of the cut axis's list
// falls on (by point), and the position's segment at the next level (-1: a box, or no longer cut)
template <typename T>
__global__ __launch_bounds__(256) void k_ssn_side(int n, int knn, const int *__restrict__ lst, const SsnSeg<T> *__restrict__ seg,
                                                  const int *__restrict__ seg_of, int *__restrict__ seg_next, int *__restrict__ side)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int j = seg_of[p];
    if (j < 0) { seg_next[p] = -1; return; }
    const SsnSeg<T> &s = seg[j];
    const int right = s.count / 2, left = s.count - right;
    const int r = p >= s.first + left ? 1 : 0;
    side[lst[(long long)s.cut * n + p]] = r;
    seg_next[p] = (r ? right : left) > knn ? 2 * j + r : -1;
}

template <typename T>
__global__ __launch_bounds__(256) void k_ssn_mark(int n, const int *__restrict__ lst, const int *__restrict__ seg_of, const int *__restrict__ side,
                                                  int *__restrict__ flag)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 3 * n) return;
    const int p = q % n;
    flag[q] = seg_of[p] >= 0 ? side[lst[q]] : 0;
}

// stable partition of every list inside every current segment: the left marks first, then the right ones
template <typename T>
__global__ __launch_bounds__(256) void k_ssn_part(int n, const int *__restrict__ lst, const SsnSeg<T> *__restrict__ seg,
                                                  const int *__restrict__ seg_of, const int *__restrict__ flag, const int *__restrict__ scan,
                                                  int *__restrict__ lst_out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 3 * n) return;
    const int a = q / n, p = q - a * n;
    const int j = seg_of[p];
    if (j < 0) { lst_out[q] = lst[q]; return; }
    const SsnSeg<T> &s = seg[j];
    const int left = s.count - s.count / 2;
    const int first = a * n + s.first;
    const int rb = scan[q] - scan[first];
    lst_out[flag[q] ? first + left + rb : q - rb] = lst[q];
}

// one thread per box: extent, mean and scatter sequentially in box order in T, jacobi3 in double, the maxBoxDim and rank < 2
// drops; with min_planarity > 0 the planarity drop (elipsoids_host.hpp, shared with the host form), after the rank test and before
// the draw; then the box's rows to the per-box scratch (assemble_rows, the same header) and the kept points (method 0: each with
// probability ratio; method 1: the box's first) flagged with their box.
// ROWS = false is the lean case (normal and mean only, 6 stores a box): no row pointer is passed (an empty structure) and no row
// store is compiled.  ROWS = true takes BoxRows' six pointers; a null one is a row nobody asked for and is skipped.  The density of
// the box around its mean takes one more walk over the members (pgicp_density.h's statement: the largest squared distance by
// strict >, from 0).  The shape values cost three divisions, so they are computed only for the planarity drop or the shape row.
struct BoxNoRows {};
template <typename T, bool ROWS>
__global__ __launch_bounds__(128) void k_box_fuse(const T *__restrict__ X, int xs, int n, const int *__restrict__ lst, const SsnBox *__restrict__ boxes,
                                                  int nbox, int method, T ratio, T max_box, T min_planarity, unsigned long long seed, T eps,
                                                  int *__restrict__ keep, int *__restrict__ box_of, T *__restrict__ bnrm, T *__restrict__ bmean,
                                                  const int *__restrict__ box_count, int *__restrict__ fused,
                                                  typename std::conditional<ROWS, BoxRows<T>, BoxNoRows>::type x = {})
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
    // (eigenvalues and eigenvector entries by selection, pick3: a run-time index would send the arrays to scratch memory)
    if (!(eh::pick3(ev, h) > 0.0) || !(eh::pick3(ev, mid) > 3.0 * (double)eps * eh::pick3(ev, h))) return;      // rank < 2: the box is dropped
    eh::Rows<T> rows;
    rows.normal = bnrm + 3LL * b;
    rows.mean = bmean + 3LL * b;
    if constexpr (ROWS) {
        if (x.beig) rows.eig = x.beig + 3LL * b;
        if (x.bvec) rows.vec = x.bvec + 9LL * b;
        if (x.bcov) rows.cov = x.bcov + 9LL * b;
        if (x.bweight) rows.weight = x.bweight + b;
        if (x.bshape) rows.shape = x.bshape + 3LL * b;
    }
    // a box dropped by its planarity is not fused
    eh::Shape<T> shape{};
    if (min_planarity > (T)0 || rows.shape) {
        shape = eh::shape_of<T>(ev, l, mid, h);
        if (eh::dropped_by_planarity<T>(shape, min_planarity)) return;
    }
    atomicAdd(fused, 1);
    const T scatter[6] = {c00, c01, c02, c11, c12, c22};
    eh::assemble_rows<T>(B.count, mean, scatter, ev, V, l, mid, h, shape, rows);
    if constexpr (ROWS) {
        if (x.bdens) {
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

// the kept points in index order: coordinates (method 1: the box mean), the box's normal, the index, the descriptors
// (method 1 with averaging: the box's mean of each row, summed in box order in T)
// ROWS: besides, every requested row of the point's box (each output may be null)
template <typename T, bool ROWS>
__global__ __launch_bounds__(256) void k_box_compact(const T *__restrict__ X, int xs, int n, const int *__restrict__ lst,
                                                     const SsnBox *__restrict__ boxes, const int *__restrict__ keep, const int *__restrict__ pos,
                                                     const int *__restrict__ box_of, const T *__restrict__ bnrm, const T *__restrict__ bmean,
                                                     int method, const T *__restrict__ desc, int drows, int average,
                                                     T *__restrict__ out_xyz, int os, T *__restrict__ out_nrm, int ns, T *__restrict__ out_desc,
                                                     int *__restrict__ kept_idx,
                                                     typename std::conditional<ROWS, BoxOut<T>, BoxNoRows>::type x = {})
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
    if constexpr (ROWS) {
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

// the number of boxes the tree of c points has (its shape depends on c and knn alone; a level holds two sizes at most)
static long long ssn_leaves(long long c, int knn, std::map<long long, long long> &memo)
{
    if (c <= knn) return 1;
    const auto it = memo.find(c);
    if (it != memo.end()) return it->second;
    const long long v = ssn_leaves((c + 1) / 2, knn, memo) + ssn_leaves(c / 2, knn, memo);
    memo[c] = v;
    return v;
}

__global__ void k_ssn_root_box(int n, SsnBox *__restrict__ boxes, int *__restrict__ box_count)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    boxes[0].first = 0; boxes[0].count = n; boxes[0].axis = 3;
    *box_count = 1;
}

// Steps 1.-3. of one call: the counters and the keep flags cleared, the three lists sorted, the tree cut level by level, the box
// list made.  Returns the lists the boxes' member ranges index (w.lst[0] or w.lst[1]); `nbox` gets the number of boxes the tree has.
template <typename T>
static const int *ssn_build_tree(hipStream_t st, const T *X, int xs, int n, int knn, const SsnScratch &w, int *counters, long long &nbox)
{
    using U = typename Bits<T>::U;
    std::map<long long, long long> memo;
    nbox = ssn_leaves(n, knn, memo);
    const dim3 b256(256);
    const long long n3 = 3LL * n;
    (void)hipMemsetAsync(counters, 0, 4 * sizeof(int), st);
    (void)hipMemsetAsync(w.keep, 0, sizeof(int) * (size_t)n, st);
    auto scan = [&](const int *in, int len, int *out) { launch_exclusive_scan(st, in, len, out, w.bsum); };
    SsnBox *boxes = (SsnBox *)w.boxes;
    int *lst = w.lst[0];
    if (n <= knn) {
        // the root is a box: fused in the identity order
        hipLaunchKernelGGL(k_ssn_root_box, dim3(1), dim3(64), 0, st, n, boxes, counters);
        hipLaunchKernelGGL(k_ssn_keys<T>, dim3(cdiv(n3, 256)), b256, 0, st, X, xs, n, (U *)w.keys[0], w.lst[0], w.flag[0], counters + 2);
    } else {
        // 1. the three lists sorted by (coordinate, index)
        hipLaunchKernelGGL(k_ssn_keys<T>, dim3(cdiv(n3, 256)), b256, 0, st, X, xs, n, (U *)w.keys[0], w.lst[0], w.flag[0], counters + 2);
        int cur = 0;
        for (int b = 0; b < Bits<T>::kBits; b++) {
            scan(w.flag[cur], (int)n3, w.scan);
            hipLaunchKernelGGL(k_ssn_split<T>, dim3(cdiv(n3, 256)), b256, 0, st, n, b, (const U *)w.keys[cur], (const int *)w.lst[cur],
                               (const int *)w.flag[cur], (const int *)w.scan, (U *)w.keys[cur ^ 1], w.lst[cur ^ 1], w.flag[cur ^ 1]);
            cur ^= 1;
        }
        // 2.-3. level by level
        SsnSeg<T> *seg[2] = {(SsnSeg<T> *)w.seg[0], (SsnSeg<T> *)w.seg[1]};
        int *seg_of[2] = {w.seg_of[0], w.seg_of[1]};
        hipLaunchKernelGGL(k_ssn_root<T>, dim3(1), dim3(64), 0, st, X, xs, n, (const int *)w.lst[cur], seg[0]);
        (void)hipMemsetAsync(seg_of[0], 0, sizeof(int) * (size_t)n, st);
        int sc = 0, ss = 0;
        long long top = n;                                       // the largest segment of the level
        for (long long nseg = 1; top > knn; nseg *= 2, top = (top + 1) / 2) {
            hipLaunchKernelGGL(k_ssn_level<T>, dim3(cdiv(nseg, 256)), b256, 0, st, X, xs, n, knn, (int)nseg, (const int *)w.lst[cur], seg[sc],
                               seg[sc ^ 1], boxes, counters);
            hipLaunchKernelGGL(k_ssn_side<T>, dim3(cdiv(n, 256)), b256, 0, st, n, knn, (const int *)w.lst[cur], (const SsnSeg<T> *)seg[sc],
                               (const int *)seg_of[ss], seg_of[ss ^ 1], w.side);
            hipLaunchKernelGGL(k_ssn_mark<T>, dim3(cdiv(n3, 256)), b256, 0, st, n, (const int *)w.lst[cur], (const int *)seg_of[ss],
                               (const int *)w.side, w.flag[0]);
            scan(w.flag[0], (int)n3, w.scan);
            hipLaunchKernelGGL(k_ssn_part<T>, dim3(cdiv(n3, 256)), b256, 0, st, n, (const int *)w.lst[cur], (const SsnSeg<T> *)seg[sc],
                               (const int *)seg_of[ss], (const int *)w.flag[0], (const int *)w.scan, w.lst[cur ^ 1]);
            cur ^= 1; sc ^= 1; ss ^= 1;
        }
        lst = w.lst[cur];
    }
    return lst;
}

// The schedule of one call of any of the three entries: the tree, then the two kernels above.  x.box names the per-box scratch
// (box_scratch), the other members of x the outputs; with none of them asked for the lean instantiations run.  min_planarity 0 is
// no planarity drop (the SamplingSurfaceNormal entries).  Returns 0, or -1 when n / knn are out of range.
template <typename T>
int launch_box_filter(hipStream_t st, const T *X, int xs, int n, int knn, int method, T ratio, T max_box, T min_planarity, unsigned long long seed,
                      const T *desc, int drows, int average, const SsnScratch &w, T *out_xyz, int os, T *out_nrm, int ns, T *out_desc,
                      int *kept_idx, int *counters /* [0] box slots, [1] boxes fused, [2] not finite, [3] kept */, const BoxOut<T> &x)
{
    if (n <= 0 || knn < 1 || (long long)n * 3 + 1 > 0x7FFFFFFFLL) return -1;
    long long nbox = 0;
    const int *lst = ssn_build_tree<T>(st, X, xs, n, knn, w, counters, nbox);
    const SsnBox *boxes = (const SsnBox *)w.boxes;
    const dim3 b256(256), b128(128);
    const T eps = std::numeric_limits<T>::epsilon();
    // 4. the boxes
    if (x.any())
        hipLaunchKernelGGL((k_box_fuse<T, true>), dim3(cdiv(nbox, 128)), b128, 0, st, X, xs, n, lst, boxes, (int)nbox, method, ratio, max_box,
                           min_planarity, seed, eps, w.keep, w.box_of, (T *)w.bnrm, (T *)w.bmean, (const int *)counters, counters + 1, x.box);
    else
        hipLaunchKernelGGL((k_box_fuse<T, false>), dim3(cdiv(nbox, 128)), b128, 0, st, X, xs, n, lst, boxes, (int)nbox, method, ratio, max_box,
                           min_planarity, seed, eps, w.keep, w.box_of, (T *)w.bnrm, (T *)w.bmean, (const int *)counters, counters + 1);
    // 5. the kept points in index order
    launch_exclusive_scan(st, w.keep, n, w.pos, w.bsum);
    if (x.any())
        hipLaunchKernelGGL((k_box_compact<T, true>), dim3(cdiv(n, 256)), b256, 0, st, X, xs, n, lst, boxes, (const int *)w.keep, (const int *)w.pos,
                           (const int *)w.box_of, (const T *)w.bnrm, (const T *)w.bmean, method, desc, drows, average, out_xyz, os, out_nrm, ns,
                           out_desc, kept_idx, x);
    else
        hipLaunchKernelGGL((k_box_compact<T, false>), dim3(cdiv(n, 256)), b256, 0, st, X, xs, n, lst, boxes, (const int *)w.keep, (const int *)w.pos,
                           (const int *)w.box_of, (const T *)w.bnrm, (const T *)w.bmean, method, desc, drows, average, out_xyz, os, out_nrm, ns,
                           out_desc, kept_idx);
    (void)hipMemcpyAsync(counters + 3, w.pos + n, sizeof(int), hipMemcpyDeviceToDevice, st);
    return 0;
}

template int launch_box_filter<float>(hipStream_t, const float *, int, int, int, int, float, float, float, unsigned long long, const float *, int, int,
                                      const SsnScratch &, float *, int, float *, int, float *, int *, int *, const BoxOut<float> &);
template int launch_box_filter<double>(hipStream_t, const double *, int, int, int, int, double, double, double, unsigned long long, const double *, int,
                                       int, const SsnScratch &, double *, int, double *, int, double *, int *, int *, const BoxOut<double> &);
