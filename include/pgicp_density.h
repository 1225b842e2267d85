/*
 * pgicp_density.h -- companion header of pgicp.h: the `densities` descriptor of SurfaceNormalDataPointsFilter{keepDensities: 1}
 * and MaxDensityDataPointsFilter on the device, each alone and as one fused call.
 *
 * SurfaceNormal{keepDensities} followed by MaxDensity is libpointmatcher's usual reference-cloud chain; a user's YAML that names
 * it makes it part of every setMap and every loop-closure ICP.  The entry points below keep that chain in device memory: the
 * densities come out of the normals kernel, where the neighbours already are, and the filter's maximum, its keep rule and the
 * compaction follow on the stream.  Conventions (buffers, `mem`, status codes, the `_f32` / `_f64` suffixes, threading) are
 * pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION and every structure
 * stay as they are.
 *
 * The statements are the oracle's, bit for bit (oracle/icp_oracle.c: orc_densities, orc_max_density_keep), in T, no contraction.
 *
 * densities.  For point i, over its neighbour list of pgicp_surface_normals_* (knn entries in (distance, index) order, the point
 * itself among them; fewer when max_dist leaves fewer), walked in list order:
 *   cnt = the neighbours found; (sx, sy, sz) = their coordinates summed in that order; mean = sum / T(cnt);
 *   r2  = the largest (dx dx + dy dy) + dz dz of a neighbour to the mean, by strict >, starting from 0;
 *   r   = sqrt(r2), correctly rounded;  dens = T(cnt) / (T((4 / 3) pi) * ((r r) r)).
 *   A point alone within max_dist, or one whose neighbours all coincide with it, has r = 0 and the density +inf.
 *
 * MaxDensity{maxDensity, seed} over n densities:
 *   last      = dens[0]; for i = 1 .. n-1: if (dens[i] > last) last = dens[i].  A NaN dens[0] therefore gives last = NaN, and
 *               otherwise last is the maximum over the values that are not NaN; +inf is an ordinary value;
 *   saturated = #{ dens[i] == last };
 *   point i is kept when !(dens[i] > maxDensity); else accept = (float)(maxDensity / dens[i]), the division in T, multiplied by
 *   (float)(1 - saturated / n) -- INTEGER division, as upstream writes it: 0 when every point is saturated, else 1 -- when
 *   dens[i] == last; the point is kept when (double)(mix(seed * 0x100000001B3 + i) >> 11) / 2^53 < (double)accept, i the
 *   point's index in the cloud handed in and mix the seeded draw of RandomSampling (pgicp.h, PGICP_FILTER_RANDOM_SAMPLING).
 *   The draw is the build's own, not rand() parity.
 */
#ifndef PGICP_DENSITY_H
#define PGICP_DENSITY_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pgicp_surface_densities = pgicp_surface_normals_* with a densities row and no neighbour table: normals, eigenvalues
 * (ascending) and densities of every point, in the caller's point order, from ONE kernel.
 *   xyz: n points at `stride` (>= 3); mem: PGICP_HOST (host in, host out) or PGICP_DEVICE (device in, device out);
 *   out_nrm: n normals at `out_stride` (>= 3; only the three values of a point are written); out_eig: 3 n values; out_dens: n
 *   values.  Any output may be NULL.  The normals and eigenvalues are bit for bit those of pgicp_surface_normals_*.
 * n == 0 does nothing.  PGICP_ERR_ARG: knn outside [3, 32], n < 0, max_dist not > 0, a coordinate that is not finite. */
int pgicp_surface_densities_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int knn, double max_dist,
                                float *out_nrm, int out_stride, float *out_eig, float *out_dens);
int pgicp_surface_densities_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int knn, double max_dist,
                                double *out_nrm, int out_stride, double *out_eig, double *out_dens);

/* pgicp_max_density = the filter's stage alone.  dens: n contiguous values where `mem` says; kept_idx (room for n, where `mem`
 * says; may be NULL): the ASCENDING indices of the kept points; *n_out (host): their number.  max_density is rounded to T first.
 * n == 0 gives *n_out = 0.  PGICP_ERR_ARG: n < 0, max_density not greater than 0 (in T), a seed at or above 2^53. */
int pgicp_max_density_f32(pgicp_ctx *ctx, const float *dens, int n, int mem, double max_density, uint64_t seed, int32_t *kept_idx,
                          int *n_out);
int pgicp_max_density_f64(pgicp_ctx *ctx, const double *dens, int n, int mem, double max_density, uint64_t seed, int32_t *kept_idx,
                          int *n_out);

/* pgicp_normals_max_density = SurfaceNormalDataPointsFilter{knn, maxDist, keepNormals, keepEigenValues, keepDensities: 1} followed
 * by MaxDensityDataPointsFilter{maxDensity, seed} over one cloud, on the device from end to end: normals, eigenvalues,
 * densities, the filter, the compaction.  The result equals the two calls above followed by a gather of the kept points, bit for
 * bit.
 *   xyz: n points at `stride`; desc: NULL, or `drows` (> 0) values a point, contiguous -- descriptor rows the cloud already
 *   carries, which travel with the kept points;
 *   out_xyz: the kept points at `stride`, as the input (only the three coordinates of a point are written); out_nrm: at
 *   `out_nstride` (>= 3), out_eig: 3 a point, out_dens: 1 a point, out_desc: drows a point (required with desc), kept_idx: the
 *   kept points' ascending input indices.  Every output array needs room for n points; out_nrm, out_eig, out_dens, out_desc
 *   (without desc) and kept_idx may be NULL.  *n_out (host): the number kept.
 *   mem = PGICP_HOST: one upload of the cloud, one download of the kept points.  mem = PGICP_DEVICE: nothing but *n_out crosses
 *   the bus, and (out_xyz, stride, out_nrm, out_nstride, *n_out) are valid arguments of pgicp_map_create_* with PGICP_DEVICE.
 *   Inputs and outputs must not overlap.
 * n == 0 gives *n_out = 0.  PGICP_ERR_ARG: as the two calls above. */
int pgicp_normals_max_density_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int knn, double max_dist,
                                  double max_density, uint64_t seed, const float *desc, int drows, float *out_xyz, float *out_nrm,
                                  int out_nstride, float *out_eig, float *out_dens, float *out_desc, int32_t *kept_idx, int *n_out);
int pgicp_normals_max_density_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int knn, double max_dist,
                                  double max_density, uint64_t seed, const double *desc, int drows, double *out_xyz, double *out_nrm,
                                  int out_nstride, double *out_eig, double *out_dens, double *out_desc, int32_t *kept_idx, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_DENSITY_H */
