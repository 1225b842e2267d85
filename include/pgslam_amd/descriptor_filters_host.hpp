// descriptor_filters_host.hpp -- the per-point statements of the three filters that read a descriptor and act on it
// (include/pgicp_descriptor_filters.h): IncidenceAngle's angle, Sphericality's three values, CutAtDescriptorThreshold's keep test.
// Plain C++ in the style of sensor_chain_host.hpp: the device kernels (k_sensor_chain.inc, k_filter.inc), the C++ drop-in's host
// filters (pointmatcher.hpp) and the stand-alone test program (tests/cpp/test_descriptor_filters_cpu.cpp) all call these functions.
// Everything is in T unless said otherwise; no product is fused with a sum; the root is the correctly rounded one and divisions are
// IEEE.
//
// The filters are restated AS RECALLED from libpointmatcher's DataPointsFilters/IncidenceAngle.cpp, Sphericality.cpp and
// CutAtDescriptorThreshold.cpp; every place the recollection could differ from upstream is marked DEVIATION below.
#pragma once

#include <cfloat>

#include "sensor_chain_host.hpp"
// det_atan2: the one arctangent in IEEE operations only that the device, the host and the oracle's orc_atan2 agree on to the bit
#include "../../pgslam_amd/csrc/icp_math.hpp"

namespace pgslam_amd {
namespace descriptor_filters {

PGSLAM_CHAIN_HD inline float min_normal(float) { return FLT_MIN; }
PGSLAM_CHAIN_HD inline double min_normal(double) { return DBL_MIN; }
PGSLAM_CHAIN_HD inline float quiet_nan(float) { return __builtin_nanf(""); }        // the default quiet NaN (0x7FC00000)
PGSLAM_CHAIN_HD inline double quiet_nan(double) { return __builtin_nan(""); }       // (0x7FF8000000000000)

// acos in double through det_atan2: c clamped to [-1, 1], then atan2(sqrt((1 - c) (1 + c)), c).  A NaN gives NaN; the endpoints and
// 0 are exact (0, pi, pi / 2 as doubles).  Within 2 ulp of the C library's acos where measured (4 by the budget: one rounding each
// for the product, the root, the quotient and the polynomial); rounded to float it equalled float(acos) on every sample.
// DEVIATION: upstream calls std::acos, whose last bit differs between math libraries and which gives NaN for |c| > 1 -- a
//   cosine of two normalised vectors can round above 1.
PGSLAM_CHAIN_HD inline double det_acos(double c)
{
    if (c != c) return c;
    if (c < -1.0) c = -1.0;
    if (c > 1.0) c = 1.0;
    return pgicp::det_atan2(sensor_chain::sqrt_rn((1.0 - c) * (1.0 + c)), c);
}

// IncidenceAngle: the angle between the normal and the observation direction, each normalised by sensor_chain::normalized (left
// as it is when its squared norm is not > 0): c = (a0 b0 + a1 b1) + a2 b2 in T, the angle T(det_acos(double(c))).  No absolute
// value: an un-oriented normal gives angles on both sides of pi / 2.
// DEVIATION: Eigen's normalized() is taken to be the guarded form, as for Shadow (include/pgicp_sensor_chain.h).
template <typename T>
PGSLAM_CHAIN_HD inline T incidence_angle(const T n[3], const T o[3])
{
    T ax = n[0], ay = n[1], az = n[2], bx = o[0], by = o[1], bz = o[2];
    sensor_chain::normalized(ax, ay, az);
    sensor_chain::normalized(bx, by, bz);
    const T c = (ax * bx + ay * by) + az * bz;
    return (T)det_acos((double)c);
}

// Sphericality: the eigenvalues sorted ascending e0 <= e1 <= e2 by a fixed min / max network; u = e0 / e2 (unstructureness),
// s = (e1 / e2) ((e1 - e0) / sqrt(e0 e0 + e1 e1)) (structureness), sphericality = u - s.  A NaN eigenvalue, or e2 or e1 below the
// smallest normal number of T, makes all three the default quiet NaN.
// DEVIATION: upstream sorts with std::sort and tests the eigenvalues against its own epsilon; the guard here is the one under which
//   both quotients are defined.
template <typename T>
PGSLAM_CHAIN_HD inline void sphericality(const T e[3], T &sph, T &unstructureness, T &structureness)
{
    sph = unstructureness = structureness = quiet_nan(T(0));
    T e0 = e[0], e1 = e[1], e2 = e[2];
    if (e0 != e0 || e1 != e1 || e2 != e2) return;
    T lo, hi;
    lo = e0 < e1 ? e0 : e1; hi = e0 < e1 ? e1 : e0; e0 = lo; e1 = hi;
    lo = e1 < e2 ? e1 : e2; hi = e1 < e2 ? e2 : e1; e1 = lo; e2 = hi;
    lo = e0 < e1 ? e0 : e1; hi = e0 < e1 ? e1 : e0; e0 = lo; e1 = hi;
    if (e2 < min_normal(T(0)) || e1 < min_normal(T(0))) return;
    const T u = e0 / e2;
    const T s = (e1 / e2) * ((e1 - e0) / sensor_chain::sqrt_rn(e0 * e0 + e1 * e1));
    unstructureness = u;
    structureness = s;
    sph = u - s;
}

// CutAtDescriptorThreshold: with useLargerThan the values above the threshold are cut -- a point stays iff v <= threshold --,
// otherwise those below it -- it stays iff v >= threshold.  IEEE comparisons with the threshold held as T: a NaN value, or a NaN
// threshold, keeps nothing.
template <typename T>
PGSLAM_CHAIN_HD inline bool cut_keep(T v, T threshold, bool use_larger_than)
{
    return use_larger_than ? v <= threshold : v >= threshold;
}

}  // namespace descriptor_filters
}  // namespace pgslam_amd
