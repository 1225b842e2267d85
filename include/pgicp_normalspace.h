/*
 * pgicp_normalspace.h -- companion header of pgicp.h: NormalSpaceDataPointsFilter on the device.
 *
 * Normal-space sampling (Rusinkiewicz & Levoy 2001, "Efficient Variants of the ICP Algorithm"), as libpointmatcher's
 * DataPointsFilters/NormalSpace.cpp runs it, restated AS RECALLED -- upstream's text was not at hand; every place the recollection
 * could differ is a DEVIATION below.  The unit normals are bucketed on the sphere and the picks are drawn evenly from the buckets:
 * the companion of a point-to-plane minimiser on scenes where a few small surfaces carry all the constraint.  Conventions
 * (buffers, `mem`, status codes, the `_f32` / `_f64` suffixes, threading) are pgicp.h's.  The symbols are part of libpgicp.so;
 * pgicp.h's own set of declarations, PGICP_ABI_VERSION and every structure stay as they are.
 *
 * The statement.  Inputs: n points, their normals (3 components each), optional descriptor rows; nbSample >= 1; epsilon, the
 * angular step in radians; seed in [0, 2^53).  mix is the SplitMix64 finaliser RandomSamplingDataPointsFilter and OctreeGrid draw
 * with.  All integer arithmetic is 64-bit unsigned and wraps.
 *
 *   No-op.   nbSample >= n: the cloud comes back unchanged, kept_idx = 0 .. n-1; the normals are not read; bucket_out is filled
 *            with -1; n == 0 gives *n_out = 0.
 *   Grid.    nPhi = ceil(2 pi / epsilon), nTheta = ceil(pi / epsilon), nbBucket = nPhi nTheta: in double from epsilon as a
 *            double, pi = M_PI.
 *   Bucket of point i, all in double from the T-valued components, in this order:
 *              z = max(min(nz, 1), -1);  theta = acos(z);  phi = fmod(atan2(ny, nx) + 2 pi, 2 pi);
 *              if theta == pi, theta = 0;  if phi == 2 pi, phi = 0  (upstream's wraps);
 *              bucket = (int)floor(theta / epsilon) nPhi + (int)floor(phi / epsilon).
 *            Normals are not normalised and not checked for unit length, as in upstream's release build; the zero normal lands
 *            at theta = pi / 2, phi = 0.  acos and atan2 are the platform's double routines: the host form uses libm, the kernel
 *            the device library.  They agree to a few ulp, so a point whose theta / epsilon or phi / epsilon lies within 1e-9 of
 *            an integer may fall on either side: the statement's only freedom.  (Inside that band a quotient may also round up
 *            to nTheta or nPhi itself; every form then takes the last row or column, so that a bucket is always < nbBucket.)
 *   DEVIATION (a): upstream computes the angles in T.  Here they are computed in double for both precisions.
 *   Order inside a bucket.  Ascending (r_i, i), r_i = mix(seed * 0x100000001B3 + i) >> 40.  The 24 bits are deliberate: the sort
 *            key (bucket << 24) | r_i has 24 + bits(nbBucket - 1) bits, five 8-bit passes at the default epsilon, and ties are
 *            common enough -- about a dozen pairs among 20 000 points of one bucket -- that the tie rule is exercised by ordinary
 *            tests.  This stands in for upstream's shuffle before bucketing.
 *   Draw.    Sequential, over counts only.  The list of non-empty buckets is kept in ascending bucket order and has size m.  For
 *            pick j = 0 .. nbSample-1: u_j = mix(~(seed * 0x100000001B3) + j), r = (u_j >> 11) mod m; pick j is the next
 *            not-yet-taken point of the r-th bucket of the list, in that bucket's order.  A bucket whose last point was taken
 *            leaves the list, and later buckets move down one place.  This is upstream's law: each pick is uniform over the
 *            non-empty buckets, then a random point of that bucket.
 *   DEVIATION (b): the generator is the build's seeded one, not std::mt19937 with std::uniform_int_distribution: the same
 *     distribution, not the same points.
 *   Output.  The j-th output point is pick j (upstream's column swaps yield pick order); coordinates, normals and every
 *            descriptor row travel with it; kept_idx[j] is its input index and bucket_out[j] its bucket.
 *            *n_out = min(n, nbSample).
 *   DEVIATION (c): a normal component that is not finite is refused with PGICP_ERR_ARG.  Coordinates are not inspected; they
 *     only travel.
 *   DEVIATION (d): 3-D clouds only.
 *   DEVIATION (e): epsilon must be finite, > 0, <= pi and give nbBucket <= 65536 (an epsilon of about 1 degree or more); anything
 *     else gets PGICP_ERR_ARG.
 *   The YAML loader wants nbSample given: upstream's default of 5000 bears no relation to the cloud's size, and an entry without
 *   it is refused as an omission.  The C ABI, Python and the C++ constructor take any nbSample >= 1.
 */
#ifndef PGICP_NORMALSPACE_H
#define PGICP_NORMALSPACE_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGICP_NORMALSPACE_MAX_BUCKETS 65536

/* pgicp_normal_space_sampling = NormalSpaceDataPointsFilter{nbSample, epsilon, seed} over one cloud.
 *   xyz: n points at `stride` (>= 3); nrm: their normals at `nstride` (>= 3); desc: NULL, or `drows` (> 0) values a point,
 *   contiguous -- descriptor rows the cloud carries besides, which travel with the picks;
 *   mem: PGICP_HOST (host in, host out) or PGICP_DEVICE (device in, device out);
 *   out_xyz: the picks at `stride`, as the input (only the three coordinates of a point are written); out_nrm: at `out_nstride`
 *   (>= 3); out_desc: drows a point (required with desc); kept_idx: the picks' input indices and bucket_out their buckets, in
 *   PICK order.  Every output array needs room for min(n, nb_sample) points; each may be NULL.  *n_out (host): min(n, nb_sample).
 *   mem = PGICP_DEVICE: nothing of length n crosses the bus -- nbBucket counts and the not-finite flag come down, nb_sample
 *   positions go up.  Inputs and outputs must not overlap.
 * n == 0 gives *n_out = 0.  PGICP_ERR_ARG: n < 0, nb_sample < 1, epsilon outside the bounds of DEVIATION (e), seed >= 2^53, a
 * stride below 3, desc without out_desc, a normal component that is not finite.  After any refusal the context stays usable. */
int pgicp_normal_space_sampling_f32(pgicp_ctx *ctx, const float *xyz, int stride, const float *nrm, int nstride, int n, int mem,
                                    int nb_sample, double epsilon, unsigned long long seed, const float *desc, int drows,
                                    float *out_xyz, float *out_nrm, int out_nstride, float *out_desc, int32_t *kept_idx,
                                    int32_t *bucket_out, int *n_out);
int pgicp_normal_space_sampling_f64(pgicp_ctx *ctx, const double *xyz, int stride, const double *nrm, int nstride, int n, int mem,
                                    int nb_sample, double epsilon, unsigned long long seed, const double *desc, int drows,
                                    double *out_xyz, double *out_nrm, int out_nstride, double *out_desc, int32_t *kept_idx,
                                    int32_t *bucket_out, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_NORMALSPACE_H */
