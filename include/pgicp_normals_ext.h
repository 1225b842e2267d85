/*
 * pgicp_normals_ext.h -- companion header of pgicp.h: the rest of SurfaceNormalDataPointsFilter's outputs on the device.
 *
 * libpointmatcher's DataPointsFilters/SurfaceNormal.cpp can keep, besides the normals, eigenvalues and densities that
 * pgicp_surface_normals_* and pgicp_surface_densities_* (pgicp_density.h) return, the eigenvectors (keepEigenVectors), the ids of
 * the neighbours (keepMatchedIds), the distance of the point to its neighbours' mean (keepMeanDist), and it can average the
 * normals over the neighbourhood (smoothNormals).  They are restated here AS RECALLED -- upstream's text was not at hand; every
 * place the recollection could differ is a DEVIATION below.  Conventions (buffers, `mem`, status codes, the `_f32` / `_f64`
 * suffixes, threading) are pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION
 * and every structure stay as they are.
 *
 * The statement.  Per point i of an n-point cloud in type T:
 *   L_i     the neighbour list pgicp_surface_normals_* returns: knn entries, the point itself included, in (d2, index) order,
 *           padded at the end with -1 / +inf where fewer than knn points lie within max_dist;  cnt_i: its valid entries.
 *   The mean (sum / (T)cnt in list order), the scatter, the Jacobi decomposition V, the columns lo / mid / hi (ascending
 *   eigenvalue, first minimum, first maximum) and the `degenerate` rule (rank < 2) are pgicp_surface_normals_*'s: nothing about
 *   them changes.
 *
 *   eigVectors (9 values a point).  The eigenvectors in ascending-eigenvalue order, column after column:
 *              out[9 i + 3 c + r] = (T)V[r][col_c], col = (lo, mid, hi).
 *            A degenerate neighbourhood gets the columns (0,1,0), (0,0,1), (1,0,0): upstream's defaults (eigenvalues (1,0,0),
 *            eigenvectors I) under the same ascending, first-minimum order that yields the eigenvalues (0,0,1) and the normal
 *            (0,1,0).  The first column equals the raw (unsmoothed) normal bit for bit, always.
 *   DEVIATION (a): upstream with sortEigen: 0 keeps its solver's order, which nothing pins.  Here the order is always ascending,
 *     as the eigenvalues' is.
 *   meanDists (1 value a point).  upstream's (point - mean).norm(): with mx, my, mz the mean above,
 *              dx = x_i - mx, dy = y_i - my, dz = z_i - mz;  meanDist = sqrt((dx dx + dy dy) + dz dz), in T, the root correctly
 *            rounded.  0 when cnt_i = 0 (a point whose own coordinates are not finite).
 *   matchedIds (knn values a point).  (T)id for every entry of L_i, (T)-1 where there is none.
 *   DEVIATION (b): with T = float an index above 2^24 is not representable, so n > PGICP_NORMALS_EXT_MAX_IDS_F32 with this output
 *     requested is PGICP_ERR_ARG.
 *   smoothNormals.  With r_j the raw normals of all points: a = (0,0,0) in T; for every valid entry j of L_i in list order
 *              d = (r_i.x r_j.x + r_i.y r_j.y) + r_i.z r_j.z;  if d > 0, a += r_j componentwise, otherwise a -= r_j;
 *            then q = (a.x a.x + a.y a.y) + a.z a.z, len = sqrt(q) correctly rounded; if len > 0 and finite the result is
 *            a / len componentwise (IEEE division), otherwise r_i.  No product is fused with a sum.
 *   DEVIATION (c): upstream overwrites the normals in place in index order, so later points read already-smoothed neighbours.
 *     Here every point reads raw normals: the result is a function of the cloud alone.
 *   DEVIATION (d): upstream divides the sum by the count.  Here the result has unit length, which a point-to-plane minimiser and
 *     SurfaceNormalOutlierFilter assume.
 *   DEVIATION (e): upstream adds every neighbour's normal as it is; here a neighbour whose normal points into the other half
 *     space is added negated (an eigenvector's sign is the solver's), and the raw normal is returned when the sum vanishes.
 *   eigVectors stay raw when smoothing is on, as upstream.
 *   DEVIATION (f): 3-D clouds, knn <= 32 and an exact search, as pgicp_surface_normals_*.
 */
#ifndef PGICP_NORMALS_EXT_H
#define PGICP_NORMALS_EXT_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest n for which pgicp_surface_normals_ext_f32 writes out_matched_ids: every index is then a float */
#define PGICP_NORMALS_EXT_MAX_IDS_F32 16777216

/* pgicp_surface_normals_ext = SurfaceNormalDataPointsFilter{knn, maxDist, smoothNormals, keep*} over one cloud: a superset of
 * pgicp_surface_normals_* and pgicp_surface_densities_*.
 *   xyz: n points at `stride` (>= 3); mem: PGICP_HOST (host in, host out) or PGICP_DEVICE (device in, device out);
 *   smooth: 0 or 1.  Every output may be NULL:
 *   out_nrm: the normals at `out_stride` (>= 3; only three values of a row are written) -- the smoothed ones when smooth = 1;
 *   out_eig: 3 a point, ascending; out_eigvec: 9 a point; out_mean_dist: 1 a point; out_matched_ids: knn a point, values of T;
 *   out_ids (int32) and out_d2: knn a point, as pgicp_surface_normals_*; out_dens: 1 a point, as pgicp_surface_densities_*.
 *   With smooth = 0 and out_nrm / out_eig / out_ids / out_d2 alone the bytes are pgicp_surface_normals_*'s; out_nrm / out_eig /
 *   out_dens are pgicp_surface_densities_*'s.  The raw normals and the neighbour table smoothing reads live in the context's
 *   scratch.  Inputs and outputs must not overlap.
 * Accepted and refused as the call it stands for: without out_dens as pgicp_surface_normals_* (n >= 1, 1 <= knn <= 32,
 * max_dist > 0), with out_dens as pgicp_surface_densities_* (n >= 0, 3 <= knn <= 32, max_dist > 0).  PGICP_ERR_ARG besides:
 * smooth outside {0, 1}, smooth = 1 without out_nrm, mem neither of the two, DEVIATION (b).  After any refusal the context stays
 * usable. */
int pgicp_surface_normals_ext_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int knn, double max_dist, int smooth,
                                  float *out_nrm, int out_stride, float *out_eig, float *out_eigvec, float *out_mean_dist,
                                  float *out_matched_ids, int32_t *out_ids, float *out_d2, float *out_dens);
int pgicp_surface_normals_ext_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int knn, double max_dist, int smooth,
                                  double *out_nrm, int out_stride, double *out_eig, double *out_eigvec, double *out_mean_dist,
                                  double *out_matched_ids, int32_t *out_ids, double *out_d2, double *out_dens);

/* pgicp_smooth_normals = the smoothing step alone, over the caller's normals and the caller's neighbour table.
 *   nrm: n normals at `nstride` (>= 3); ids: n x knn int32, row i the list of point i, -1 = none (anywhere in the row); any
 *   knn >= 1 with n knn < 2^31 (the table need not come from a search);  out_nrm: n normals at `out_stride` (>= 3).  mem as
 *   above, for all three.  Inputs and outputs must not overlap.  The normals need not have unit length; the result has, unless
 *   the sum vanishes or is not finite (then the point's own normal comes back).
 * n == 0 does nothing.  PGICP_ERR_ARG: n < 0, knn < 1, a stride below 3, a NULL array with n > 0, an id outside [-1, n) --
 * found by the kernel, which never follows such an id, through a flag the call reads back; out_nrm is then unspecified.  After
 * any refusal the context stays usable. */
int pgicp_smooth_normals_f32(pgicp_ctx *ctx, const float *nrm, int nstride, const int32_t *ids, int knn, int n, int mem,
                             float *out_nrm, int out_stride);
int pgicp_smooth_normals_f64(pgicp_ctx *ctx, const double *nrm, int nstride, const int32_t *ids, int knn, int n, int mem,
                             double *out_nrm, int out_stride);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_NORMALS_EXT_H */
