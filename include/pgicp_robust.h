/*
 * pgicp_robust.h -- companion header of pgicp.h: the rest of RobustOutlierFilter's parameters on the device.
 *
 * libpointmatcher's RobustOutlierFilter{robustFct, tuning, scaleEstimator, nbIterationForScale, distanceType, approximation}:
 * pgicp_params carries robustFct, tuning, approximation and the scale estimators none and mad, with the weights taken on the
 * matcher's point-to-point distances and the scale estimated in every iteration.  The setter below adds the three settings a
 * point-to-plane chain usually runs with: weights on plane distances (distanceType point2plane), the berg scale estimator, and a
 * scale that is estimated in the first nbIterationForScale iterations and then held.  Conventions (status codes, threading) are
 * pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION, pgicp_params and every
 * structure stay as they are.
 *
 * [EXT] Definition (this build's; upstream's filter is not at hand to compare against).  T is the element type of the call, sqrt_rn
 * the correctly rounded root, every product and sum is formed in T in the order written.
 *
 * Iteration counter and estimate rule.  Every problem of a call counts its iterations it = 1, 2, ...; with nb =
 * nb_iteration_for_scale
 *     estimate = (nb == 0 || it <= nb).
 * [deviation] The counter and the held scale belong to ONE ICP of ONE problem: they start afresh with every call and never travel
 * between the problems of a batch or between calls.  Upstream keeps both in the filter object, so that a filter object reused for a
 * second ICP goes on counting; a batch has no such object, and the results of this library do not depend on call history.
 *
 * Scale s.  Always from the matcher's point-to-point squared distances d2 of the pairs that have a neighbour, also when the weights
 * use plane distances (upstream's behaviour, kept).
 *     none:  s = 1.
 *     mad:   estimate: s = sqrt_rn(MAD), MAD the median of |d2 - median(d2)|, both medians the element of index size / 2 (what
 *            PGICP_ROBUST_SCALE_MAD is without this header); else s is held.
 *     berg:  the TARGET scale is pgicp_params.robust_tuning, and the weight function runs with tuning 1.
 *            estimate, it == 1:  s = T(1.9) * sqrt_rn(median(d2))
 *            estimate, it > 1:   s = T(0.85) * (s - target) + target
 *            else s is held.
 * The pair's e2 is dd / (s * s), the product in T.
 *
 * Distance dd that the weight function and the `approximation` cut see.
 *     point2point:  dd = d2.
 *     point2plane:  with q and n the matched reference point and its normal in the centred reference frame and p' the reading point
 *                   as the iteration moved it,
 *                       dx = p'x - qx, dy = p'y - qy, dz = p'z - qz;  v = (nx * dx + ny * dy) + nz * dz;  dd = v * v.
 * A pair without a neighbour has weight 0.  A MaxDistOutlierFilter beside the robust filter (pgicp_params.outlier_max_dist) still
 * cuts on d2; the SurfaceNormal and GenericDescriptor weights multiply in as they do without this header.  Everything that forms the
 * last error elements again -- the covariance, the sensor-noise overlap (pgicp_noise.h), the residual pass of
 * pgicp_align_residual_batch_* -- uses the same dd and the same held s as the iteration did; the residual pass is one more pass of
 * the chain, it = iterations + 1 of its problem.
 *
 * Single-pass entry points are iteration 1: pgicp_partial_chain_* (the seeded form too) and pgicp_outlier_weights_* -- berg gives
 * T(1.9) * sqrt_rn(median) there, and nb has no effect.
 */
#ifndef PGICP_ROBUST_H
#define PGICP_ROBUST_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGICP_ROBUST_DIST_POINT2POINT 0
#define PGICP_ROBUST_DIST_POINT2PLANE 1
/* a third value of the scale estimator, beside pgicp.h's PGICP_ROBUST_SCALE_NONE (0) and PGICP_ROBUST_SCALE_MAD (1); reachable through
 * pgicp_set_robust_ext only: pgicp_set_params keeps refusing it in pgicp_params.robust_scale */
#define PGICP_ROBUST_SCALE_BERG 2

typedef struct pgicp_robust_ext {
    int distance_type;              /* PGICP_ROBUST_DIST_* */
    int scale_estimator;            /* PGICP_ROBUST_SCALE_NONE / _MAD / _BERG; -1: whatever pgicp_params.robust_scale says */
    int nb_iteration_for_scale;     /* 0: the scale is estimated in every iteration; n > 0: in the first n, then held */
} pgicp_robust_ext;

/* pgicp_set_robust_ext: a setting of the context, like pgicp_set_var_trim: it stays until it is set again; ext == NULL turns it
 * off.  A context on which it was never called, or was last called with NULL, launches what it launched without this header and is
 * bit for bit what it was; so is one set to {PGICP_ROBUST_DIST_POINT2POINT, -1, 0}.
 * Fails with PGICP_ERR_ARG, leaves the previous setting in force and the context usable, when
 *   - distance_type or scale_estimator is an unknown code, or nb_iteration_for_scale < 0;
 *   - the setting asks for anything (point2plane, berg, nb != 0) while pgicp_params.robust_fct is PGICP_ROBUST_NONE.
 * pgicp_set_params and this setter are called separately, so the second rule is checked again by every call that runs the chain
 * (as pgicp_set_var_trim's rules are): such a call fails with PGICP_ERR_ARG before it does any work, and so does
 *   - a call with point2plane on a problem whose map carries no normals;
 *   - pgicp_outlier_weights_* with point2plane: a bare array of distances has no geometry.
 * knn > 1 with a robust filter stays refused by pgicp_set_params. */
int pgicp_set_robust_ext(pgicp_ctx *ctx, const pgicp_robust_ext *ext);
/* on: 1 after a successful call with ext != NULL, 0 otherwise; ext (may be NULL): the setting in force (zeros when off) */
int pgicp_get_robust_ext(const pgicp_ctx *ctx, int *on, pgicp_robust_ext *ext);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_ROBUST_H */
