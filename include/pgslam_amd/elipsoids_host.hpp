// elipsoids_host.hpp -- the part of ElipsoidsDataPointsFilter's statement (include/pgicp_elipsoids.h) that is new beside
// SamplingSurfaceNormalDataPointsFilter's, in plain C++: the shape values of a box, the planarity test and the assembly of a box's rows
// from (count, mean, scatter, ev, V, l, mid, h).  The device kernel (pgslam_amd/csrc/k_ssn.inc), the C++ drop-in's host form
// (pointmatcher.hpp) and the stand-alone test program (tests/cpp/test_elipsoids_cpu.cpp) all call these functions, so the three cannot
// drift apart.  Everything is in T unless said; no product is fused with a sum (the translation units that include this are built
// without contraction); divisions are correctly rounded.
#pragma once

#ifndef PGSLAM_ELIP_HD
#define PGSLAM_ELIP_HD          // (the device library defines it as __host__ __device__ before it includes this)
#endif

namespace pgslam_amd {
namespace elipsoids {

// minPlanarity's range: finite and in [0, 1]; a NaN is refused
inline bool min_planarity_ok(double p) { return p >= 0.0 && p <= 1.0; }

// v[k], k in 0 .. 2, by selection: on the device a run-time index into a register array would send the array to scratch memory
PGSLAM_ELIP_HD inline double pick3(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

template <typename T>
struct Shape { T planarity, cylindricality, sphericality; };

// the shape values of a box from its eigenvalues in double and the indices of the smallest (l), the middle (mid) and the largest (h)
template <typename T>
PGSLAM_ELIP_HD inline Shape<T> shape_of(const double ev[3], int l, int mid, int h)
{
    const T e0 = (T)pick3(ev, h), e1 = (T)pick3(ev, mid), e2 = (T)pick3(ev, l);           // descending
    const T s = (e0 + e1) + e2;
    const T v0 = e0 / s, v1 = e1 / s, v2 = e2 / s;
    Shape<T> r;
    r.planarity = T(2) * v1 - T(2) * v2;
    r.cylindricality = v0 - v1;
    r.sphericality = T(3) * v2;
    return r;
}

// the planarity drop: only when minPlanarity > 0, strict <, compared in T (a NaN planarity is not dropped)
template <typename T>
PGSLAM_ELIP_HD inline bool dropped_by_planarity(const Shape<T> &s, T min_planarity)
{
    return min_planarity > T(0) && s.planarity < min_planarity;
}

// where a box's rows go: every pointer may be null (the row is not asked for)
template <typename T>
struct Rows {
    T *normal = nullptr;         // 3: (T)V[.][l]
    T *eig = nullptr;            // 3: ascending
    T *vec = nullptr;            // 9: columns l, mid, h, out[3 c + r]
    T *cov = nullptr;            // 9: the scatter sums, symmetric, out[3 c + r]
    T *weight = nullptr;         // 1: T(count)
    T *mean = nullptr;           // 3
    T *shape = nullptr;          // 3: planarity, cylindricality, sphericality
};

// scatter: c00 c01 c02 c11 c12 c22 (the sums that were decomposed)
template <typename T>
PGSLAM_ELIP_HD inline void assemble_rows(int count, const T mean[3], const T scatter[6], const double ev[3], const double V[3][3], int l, int mid,
                                         int h, const Shape<T> &shape, const Rows<T> &o)
{
    const int col[3] = {l, mid, h};
    if (o.normal) for (int r = 0; r < 3; r++) o.normal[r] = (T)pick3(V[r], l);
    if (o.eig) for (int c = 0; c < 3; c++) o.eig[c] = (T)pick3(ev, col[c]);
    if (o.vec) for (int c = 0; c < 3; c++) for (int r = 0; r < 3; r++) o.vec[3 * c + r] = (T)pick3(V[r], col[c]);
    if (o.cov) {
        o.cov[0] = scatter[0]; o.cov[1] = scatter[1]; o.cov[2] = scatter[2];
        o.cov[3] = scatter[1]; o.cov[4] = scatter[3]; o.cov[5] = scatter[4];
        o.cov[6] = scatter[2]; o.cov[7] = scatter[4]; o.cov[8] = scatter[5];
    }
    if (o.weight) o.weight[0] = (T)count;
    if (o.mean) for (int r = 0; r < 3; r++) o.mean[r] = mean[r];
    if (o.shape) { o.shape[0] = shape.planarity; o.shape[1] = shape.cylindricality; o.shape[2] = shape.sphericality; }
}

}  // namespace elipsoids
}  // namespace pgslam_amd
