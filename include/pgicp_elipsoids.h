/*
 * pgicp_elipsoids.h -- companion header of pgicp.h: ElipsoidsDataPointsFilter on the device.
 *
 * libpointmatcher's DataPointsFilters/Elipsoids.cpp cuts the cloud with SamplingSurfaceNormalDataPointsFilter's median-split tree and
 * summarises every box as an ellipsoid: mean, covariance, weight, shape, normal, eigen-decomposition and density; it can drop the
 * boxes that are not planar enough (minPlanarity).  It is restated here AS RECALLED -- upstream's text was not at hand; every place
 * the recollection could differ is a DEVIATION below.  Conventions (buffers, `mem`, status codes, the `_f32` / `_f64` suffixes,
 * threading) are pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION and every
 * structure stay as they are.
 *
 * The statement.  Everything pgicp_sampling_surface_normal_* (pgicp.h) and pgicp_ssn_ext.h state is taken over unchanged: the tree,
 * the boxes and their member order; the box mean (mx, my, mz) in T; the scatter sums c00 .. c22 in T, in box order, nothing fused;
 * jacobi3 in double with eigenvalues ev[0..2] and the indices l / mid / h (first minimum, first maximum); the rank < 2 drop and the
 * maxBoxDim drop (strict >); the seeded draw (kept while u < ratio); sampling_method 1 keeping the box's first member with the mean's
 * coordinates and the descriptors averaged in box order.  `count` is the number of the box's members.  3-D clouds, knn in [3, 1024].
 *
 * For a box that passed the rank test, all in T, divisions correctly rounded, no product fused with a sum:
 *     e0 = (T)ev[h], e1 = (T)ev[mid], e2 = (T)ev[l]              (descending)
 *     s  = (e0 + e1) + e2
 *     v0 = e0 / s, v1 = e1 / s, v2 = e2 / s
 *     planarity = T(2) v1 - T(2) v2,  cylindricality = v0 - v1,  sphericality = T(3) v2
 *
 *   minPlanarity.  When min_planarity > 0, a box with planarity < (T)min_planarity (strict, compared in T) is dropped: it keeps no
 *   point and does not count as fused.  The test comes after the rank test and before the draw.
 *   DEVIATION (a): upstream forms the shape values from its solver's eigenvalue order, which nothing pins.  Here the order is always
 *     descending, first maximum / first minimum.
 *
 *   The rows of a fused box, each to every point the box keeps:
 *   normals (3), densities (1), eigValues (3, ascending), eigVectors (9): pgicp_sampling_surface_normal_*'s normal and
 *     pgicp_ssn_ext.h's statements with their deviations, unchanged.
 *   covariance (9 values).  The matrix that was decomposed, i.e. the scatter sums as T values, symmetric, column after column:
 *     out[3 c + r] = c_rc.  Its eigen-pairs are the two rows above (up to Jacobi's error in double and one rounding to T).
 *   DEVIATION (b): upstream's normalisation is not pinned -- it may divide by the count.  Here: none.
 *   weights (1 value).  T(count).
 *   means (3 values).  mx, my, mz.  With sampling_method 1 these equal the kept point's own coordinates bit for bit.
 *   shapes (3 values).  planarity, cylindricality, sphericality.
 *   DEVIATION (c): upstream's maxTimeWindow splits boxes whose members' times lie too far apart.  This ABI carries no times: there is
 *     no such argument; the drop-in accepts only an absent or infinite maxTimeWindow.
 *   DEVIATION (d): keepNormals has no default the recollection could pin: the drop-in asks for it explicitly from YAML; here out_nrm
 *     is given or NULL.
 *
 * With min_planarity 0 and the seven new outputs NULL the bytes of every output are pgicp_sampling_surface_normal_*'s.
 *
 * The drop-in (include/pgslam_amd/pointmatcher.hpp): ElipsoidsDataPointsFilter appends, after the cloud's own rows and each only when
 * asked, `normals`, `densities`, `eigValues`, `eigVectors`, `covariance`, `weights`, `means`, `shapes`, each overwriting a descriptor
 * of the same name.  The shape values, the planarity test and the row assembly are in include/pgslam_amd/elipsoids_host.hpp, which
 * the device kernel and the drop-in's host form share.
 */
#ifndef PGICP_ELIPSOIDS_H
#define PGICP_ELIPSOIDS_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pgicp_elipsoids = ElipsoidsDataPointsFilter{ratio, knn, samplingMethod, maxBoxDim, minPlanarity, averageExistingDescriptors, keep*}:
 * pgicp_sampling_surface_normal_ext_*'s argument list (see pgicp.h and pgicp_ssn_ext.h for every argument), then min_planarity and
 * four more outputs, for the n_out kept points in ascending input index, packed:
 *   out_cov: 9 values a kept point; out_weights: 1; out_means: 3; out_shapes: 3.  Each may be NULL and each needs room for n points;
 *   `mem` applies to them as to the other arrays.  Inputs and outputs must not overlap.
 * n_boxes reports the boxes fused, i.e. after the planarity drop.
 * Arguments are accepted and refused as pgicp_sampling_surface_normal_* accepts and refuses them (PGICP_ERR_ARG; a NaN or infinite
 * coordinate among them); besides, min_planarity must be finite and in [0, 1] (a NaN is refused).  After any refusal the context
 * stays usable.  Scratch comes from the context's buffers: a second call of the same size makes no new device allocation. */
int pgicp_elipsoids_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method,
                        double max_box_dim, uint64_t seed, const float *desc, int drows, int average_descriptors, float *out_xyz,
                        int out_stride, float *out_nrm, int nrm_stride, float *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes,
                        float *out_eig, float *out_eigvec, float *out_dens, double min_planarity, float *out_cov, float *out_weights,
                        float *out_means, float *out_shapes);
int pgicp_elipsoids_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int knn, double ratio, int sampling_method,
                        double max_box_dim, uint64_t seed, const double *desc, int drows, int average_descriptors, double *out_xyz,
                        int out_stride, double *out_nrm, int nrm_stride, double *out_desc, int32_t *kept_idx, int *n_out, int *n_boxes,
                        double *out_eig, double *out_eigvec, double *out_dens, double min_planarity, double *out_cov, double *out_weights,
                        double *out_means, double *out_shapes);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_ELIPSOIDS_H */
