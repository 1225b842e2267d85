/*
 * pgicp_descriptor_filters.h -- companion header of pgicp.h and pgicp_sensor_chain.h: the three filters that read a descriptor and
 * act on it, as stages of the two fused device passes.
 *
 *   - SurfaceNormalDataPointsFilter: {knn: 10, keepEigenValues: 1, keepDensities: 1}
 *   - ObservationDirectionDataPointsFilter
 *   - OrientNormalsDataPointsFilter
 *   - IncidenceAngleDataPointsFilter
 *   - CutAtDescriptorThresholdDataPointsFilter: {descName: incidenceAngles, useLargerThan: 1, threshold: 1.3}
 *   - SphericalityDataPointsFilter
 *   - CutAtDescriptorThresholdDataPointsFilter: {descName: sphericality, useLargerThan: 1, threshold: 0.2}
 *   - MaxDensityDataPointsFilter: {maxDensity: 50}
 *
 * is how a configuration cuts grazing-angle points and unstructured regions.  The three filters are per-point statements, so they
 * have no device call of their own: pgicp_sensor_chain_ext_* is pgicp_sensor_chain_* (pgicp_sensor_chain.h) with three more stage
 * types, and pgicp_filter_cloud_* (pgicp.h) takes one more entry.  Conventions are pgicp.h's; the symbols are part of libpgicp.so;
 * pgicp.h's own set of declarations, PGICP_ABI_VERSION and every structure stay as they are.
 *
 * The statements, in T unless said otherwise, no contraction, correctly rounded root, IEEE division
 * (include/pgslam_amd/descriptor_filters_host.hpp holds them; the kernels and the C++ drop-in's host filters both call it):
 *   INCIDENCE_ANGLE    a = the normal, b = the observation direction, each divided by its norm sqrt((x x + y y) + z z) when the
 *                      squared norm is > 0 and left as it is otherwise; c = (a0 b0 + a1 b1) + a2 b2; the angle is
 *                      T(det_acos(double(c))), det_acos(c) = det_atan2(sqrt((1 - c) (1 + c)), c) in double with c clamped to
 *                      [-1, 1] and det_atan2 the arctangent in IEEE operations only of the covariance's small-angle parameters
 *                      (the same bits on the device, on the host and in the oracle's orc_atan2).  A NaN c gives NaN.  No absolute
 *                      value is taken.  The normal read is the one the stages before have left.
 *   SPHERICALITY       the three eigenvalues sorted ascending e0 <= e1 <= e2 by a fixed min / max network;
 *                      u = e0 / e2, s = (e1 / e2) ((e1 - e0) / sqrt(e0 e0 + e1 e1)), sphericality = u - s, unstructureness = u,
 *                      structureness = s.  A NaN eigenvalue, or e2 or e1 below the smallest normal number of T, makes all three
 *                      the default quiet NaN.
 *   CUT_AT_DESCRIPTOR  with useLargerThan a point is kept iff v <= threshold, otherwise iff v >= threshold; IEEE comparisons,
 *                      the threshold held as T.  A NaN value is never kept; a NaN threshold keeps nothing.
 * DEVIATION (IncidenceAngle): upstream calls std::acos, whose last bit differs between math libraries and which gives NaN for
 *   |c| > 1.  det_acos is within 2 ulp of the C library's double acos over the 28 000 arguments of
 *   tests/test_descriptor_filters_host.py (uniform, and dense near -1, 0 and 1), equal to it once rounded to float, exact at -1, 0
 *   and 1.  Eigen's normalized() is taken to be the guarded form, as for Shadow.
 * DEVIATION (Sphericality): upstream's Sphericality.cpp is restated as recalled; its guard against small eigenvalues is taken to
 *   be the one above, under which both quotients are defined.
 * DEVIATION (CutAtDescriptorThreshold): restated as recalled: useLargerThan cuts the values LARGER than the threshold.
 */
#ifndef PGICP_DESCRIPTOR_FILTERS_H
#define PGICP_DESCRIPTOR_FILTERS_H

#include "pgicp_sensor_chain.h"

#ifdef __cplusplus
extern "C" {
#endif

/* stage types of pgicp_sensor_chain_ext_* beyond pgicp_sensor_chain.h's 1 .. 5 */
#define PGICP_CHAIN_INCIDENCE_ANGLE   6  /* no parameter; needs keep_normals and an OBSERVATION_DIRECTION stage before it */
#define PGICP_CHAIN_SPHERICALITY      7  /* p[0] = keepUnstructureness, p[1] = keepStructureness (0 / 1); needs keep_eig */
#define PGICP_CHAIN_CUT_AT_DESCRIPTOR 8  /* p[0] = the row (PGICP_CHAIN_ROW_*), p[1] = useLargerThan (0 / 1), p[2] = threshold (rounded
                                            to T), p[3] = with PGICP_CHAIN_ROW_DESC the index in [0, drows) of the carried row */
#define PGICP_CHAIN_EXT_MAX_STAGES 12
#define PGICP_CHAIN_EXT_MAX_CUTS 4

/* the one-row descriptor a CUT_AT_DESCRIPTOR stage reads */
#define PGICP_CHAIN_ROW_DESC               0  /* a row of `desc`, the descriptors the cloud already carries */
#define PGICP_CHAIN_ROW_DENSITIES          1  /* the head's, with keep_dens */
#define PGICP_CHAIN_ROW_INCIDENCE_ANGLES   2  /* an INCIDENCE_ANGLE stage's */
#define PGICP_CHAIN_ROW_SPHERICALITY       3  /* a SPHERICALITY stage's */
#define PGICP_CHAIN_ROW_UNSTRUCTURENESS    4  /* ... with keepUnstructureness */
#define PGICP_CHAIN_ROW_STRUCTURENESS      5  /* ... with keepStructureness */
#define PGICP_CHAIN_ROW_SIMPLE_SENSOR_NOISE 6 /* a SIMPLE_SENSOR_NOISE stage's */

/* where the kept points' rows go: pointers to T (float for _f32, double for _f64), each with room for n points.  xyz is required;
 * desc is required with `desc`; every other member may be NULL.  The first nine are pgicp_sensor_chain_*'s outputs of the same
 * names; incidence, sphericality, unstructureness, structureness: 1 value a point. */
typedef struct pgicp_chain_out {
    void *xyz;            /* at the input's stride */
    void *nrm;            /* at nstride (>= 3) */
    int nstride;
    void *eig, *dens, *obs, *noise, *desc;
    void *incidence, *sphericality, *unstructureness, *structureness;
    int32_t *kept_idx;
} pgicp_chain_out;

/* pgicp_sensor_chain_ext = pgicp_sensor_chain (pgicp_sensor_chain.h: arguments, memory, order, n == 0) with up to
 * PGICP_CHAIN_EXT_MAX_STAGES stages of types 1 .. 8.  CUT_AT_DESCRIPTOR is a dropping stage like SHADOW: the stages behind it run on
 * its survivors (a MAX_DENSITY behind it draws by rank) and compute nothing for the points it dropped.  It may appear up to
 * PGICP_CHAIN_EXT_MAX_CUTS times; every other type at most once.  Rows live at the points' input indices, the survivor list and its
 * count stay on the device between stages, one gather at the end.
 * With stages of types 1 .. 5 only the call equals pgicp_sensor_chain_* byte for byte (which keeps refusing types above 5 and more
 * than PGICP_CHAIN_MAX_STAGES stages).
 * PGICP_ERR_ARG (the context stays usable), besides pgicp_sensor_chain_*'s: INCIDENCE_ANGLE without keep_normals or without an
 * OBSERVATION_DIRECTION stage before it; SPHERICALITY without keep_eig; a keep flag or useLargerThan that is not 0 or 1; a cut whose
 * row does not exist when it runs (not kept by the head, made by no earlier stage, or outside [0, drows) / no `desc`); a fifth cut;
 * an output whose row no stage makes (unstructureness / structureness without their keep flag).  A NaN threshold is accepted. */
int pgicp_sensor_chain_ext_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals,
                               int keep_eig, int keep_dens, int n_stages, const pgicp_chain_stage *stages, const float *desc, int drows,
                               const pgicp_chain_out *out, int *n_out);
int pgicp_sensor_chain_ext_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int knn, double max_dist, int keep_normals,
                               int keep_eig, int keep_dens, int n_stages, const pgicp_chain_stage *stages, const double *desc, int drows,
                               const pgicp_chain_out *out, int *n_out);

/* An entry of pgicp_filter_cloud_*'s list (pgicp_filter::type): CutAtDescriptorThreshold over a row of the descriptors handed to
 * the call.  p[0] = the row in [0, drows), p[1] = useLargerThan (0 / 1), p[2] = the threshold as T, widened to double.  A point-wise
 * predicate: a sampler behind it sees the ranks after the cut.  PGICP_ERR_ARG: no descriptors, a row outside [0, drows), and any
 * list holding the entry given to pgicp_filter_cloud_dev_*, which takes no descriptors.  A NaN threshold keeps nothing. */
#define PGICP_FILTER_CUT_AT_DESCRIPTOR 9

#ifdef __cplusplus
}
#endif
#endif /* PGICP_DESCRIPTOR_FILTERS_H */
