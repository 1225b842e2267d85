/*
 * pgicp_vardist.h -- companion header of pgicp.h: KDTreeVarDistMatcher's per-point search radii on the device.
 *
 * libpointmatcher's second matcher, KDTreeVarDistMatcher{knn, epsilon, searchType, maxDistField}, gives every reading point its
 * own search radius, read from a descriptor row of the reading (default name `maxSearchDist`): a range sensor's chain gates its
 * correspondences by range that way (a radius proportional to `simpleSensorNoise`, say).  pgicp_params.max_dist is one number per
 * context; the entry points below hand the next matching call one radius per reading point.  Conventions (buffers, `mem`, status
 * codes, the `_f32` / `_f64` suffixes, threading) are pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of
 * declarations, PGICP_ABI_VERSION and every structure stay as they are.
 *
 * [EXT] Definition (this build's; upstream's matcher is not at hand to compare against).  For reading point i with radius r_i, a
 * value of T, the k neighbours returned are the k nearest map points among those with
 *     d2 <= r_i * r_i,      the product formed in T
 * -- the comparison the uniform bound makes (d2 <= max_dist * max_dist, the product in T).  pgicp_params.max_dist stays in force
 * as the global bound: the effective radius is min(max_dist, r_i).  A neighbour position with no such point is "no match": id -1,
 * distance +inf, weight 0; it is never an error element and is not counted in pgicp_stats.n_finite, exactly as a pair without a
 * neighbour under max_dist.  r_i = +inf is allowed and cuts nothing.  Neighbours come out in ascending (distance, index) order, so
 * the kNN within r_i is the exact kNN within max_dist with the entries beyond r_i * r_i cut from its tail: with radii armed the
 * matcher resolves every pair exactly under max_dist (as it does under the Robust and VarTrimmedDist filters) and one more kernel
 * makes the cut.  Everything downstream of the matcher in that iteration -- the outlier filters' selections and scales, the
 * minimiser's sums, the covariance, the residual pass, the sensor-noise overlap, pgicp_debug_last_matches, pgicp_stats -- sees the
 * cut pairs.  The quantile filters select over the cut distances.
 */
#ifndef PGICP_VARDIST_H
#define PGICP_VARDIST_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pgicp_arm_reading_radii: hands the NEXT matching call of the context the radius row of its readings.  One-shot: it applies to
 * the next pgicp_align_*, pgicp_align_batch_*, pgicp_align_residual_batch_*, pgicp_icp_pair_*, pgicp_match_*,
 * pgicp_partial_chain_* or pgicp_partial_chain_batch_* call on the context, and that call consumes it whether it succeeds or not
 * (every other entry point leaves it armed).  Arming again replaces what was armed; an arm call that fails leaves the context
 * unarmed.
 *   radii[p][i * stride[p]] = the value of reading point i of problem p, in the caller's point order (stride >= 1: one row of
 *   a column-major descriptor matrix is passed without a copy); n[p] = the number of points of that reading.  radii[p] == NULL:
 *   problem p has no radii -- its pairs are bounded by max_dist alone (stride[p] and n[p] are then not looked at).  `mem`
 *   (PGICP_HOST / PGICP_DEVICE) holds for every row.  The values are copied into the context inside this call, which returns
 *   when the copy is complete: no caller pointer is held afterwards.
 * The consuming call fails with PGICP_ERR_ARG before it does any work, and leaves the context usable (and unarmed), when
 *   - n_problems differs from its own (1 for the single-problem entry points), or an n[p] from its reading's size, or the element
 *     type from its own;
 *   - a value is negative or a NaN.
 * pgicp_partial_chain_seeded_* refuses while radii are armed (PGICP_ERR_ARG; the arm is kept): a seeded probe with radii is not
 * offered.  Radii may be armed together with noise rows (pgicp_noise.h), pgicp_set_var_trim, pgicp_set_descriptor_filter, the
 * Robust and SurfaceNormal outlier filters and knn > 1.
 * A call that is not armed launches no kernel and allocates nothing because of this header, and is bit for bit the call it was. */
int pgicp_arm_reading_radii_f32(pgicp_ctx *ctx, int n_problems, const float *const *radii, const int *stride, const int *n, int mem);
int pgicp_arm_reading_radii_f64(pgicp_ctx *ctx, int n_problems, const double *const *radii, const int *stride, const int *n, int mem);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_VARDIST_H */
