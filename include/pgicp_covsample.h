/*
 * pgicp_covsample.h -- companion header of pgicp.h: CovarianceSamplingDataPointsFilter on the device.
 *
 * The stability sampler of Gelfand et al. 2003 ("Geometrically Stable Sampling for the ICP Algorithm"), as libpointmatcher's
 * DataPointsFilters/CovarianceSampling.cpp runs it: it keeps the nbSample points that best constrain all six degrees of freedom
 * of the point-to-plane solve.  It is a reading filter: once per scan, four passes over the cloud and six order statistics, in
 * device memory next to the reading the ICP takes from there.  Conventions (buffers, `mem`, status codes, the `_f32` / `_f64`
 * suffixes, threading) are pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION
 * and every structure stay as they are.
 *
 * The statement.  Inputs: n points x_i, their normals n_i, nbSample, torqueNorm in {0, 1, 2}.  All arithmetic is in T, no
 * contraction, the expression order as written; accumulations called "double" are the exception.
 *
 *   No-op.   nbSample >= n: the cloud comes back unchanged, kept_idx = 0 .. n-1 (no frame is computed: frame_out is zeroed).
 *   Frame.   A record of doubles holding values that are exactly representable in T:
 *     c      = the mean of the points: the coordinates summed in double (any order; the sum is cascaded -- two-sum, the rounding
 *              errors summed apart -- so it is the exact sum's rounding whatever the order), divided by n, rounded to T;
 *     L      = 1 (torqueNorm 0);
 *              the mean of sqrt((dx dx + dy dy) + dz dz), d = x_i - c, each norm in T with a correctly rounded root, the norms
 *              summed in double (cascaded likewise), divided by n, rounded to T (torqueNorm 1, Lavg);
 *              half the largest of the three extents max - min of the coordinates, in T (torqueNorm 2, Lmax);
 *     C      = sum f_i f_i^T (6 x 6): the products of the T-valued entries of f_i (below) accumulated in double;
 *     X, lambda = an orthonormal eigenbasis of C from a cyclic Jacobi in double on the host, eigenvalues ascending, the columns
 *              rounded to T.
 *     DEVIATION (a): upstream solves with Eigen's general EigenSolver in T, whose column order and signs are unspecified.  Signs
 *     do not matter (the absolute value below); the order only decides ties between lists.
 *   Per point.  p = x_i - c;  cr = (py nz - pz ny, pz nx - px nz, px ny - py nx);  inv = T(1) / L;
 *     f_i  = (inv cr.x, inv cr.y, inv cr.z, nx, ny, nz);
 *     v_ik = |((((f0 X0k + f1 X1k) + f2 X2k) + f3 X3k) + f4 X4k) + f5 X5k|.
 *   Lists.   List k (0 .. 5) holds the points in order of v_ik descending, ties by ascending index (upstream's stable list::sort
 *     with >).
 *   Greedy.  t[0 .. 5] = 0.  nbSample times: k = the first index of the smallest t (if (t[k] > t[kk]) k = kk); pop list k while
 *     its head is already sampled; the head becomes pick j and is marked sampled; t[m] += v_jm v_jm for every m.
 *   Output.  The j-th output point is the j-th pick (upstream's column swaps yield this order); coordinates, normals and every
 *     descriptor row travel with it.
 *   Prefix bound.  Every entry ever popped from a list is a sampled point by the end, so at most nbSample entries of each list
 *     are touched: only each list's first nbSample entries, under the tie rule, are needed.  The device selects exactly those
 *     (a radix selection of the nbSample-th largest key of each list and a ranked cut among its ties), the host sorts 6 nbSample
 *     records and runs the greedy, the device gathers.
 *   DEVIATION (b): a coordinate or normal component that is not finite is refused with PGICP_ERR_ARG (upstream's sort on NaN is
 *     undefined).  So is a cloud whose L is not > 0 (every point at the mean): 1 / L has no value there.
 *   DEVIATION (c): only 3-D clouds (upstream returns 2-D clouds untouched).
 */
#ifndef PGICP_COVSAMPLE_H
#define PGICP_COVSAMPLE_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the frame of a call: the centre, the torque normalisation, the eigenvalues (ascending) and the eigenbasis (column-major: entry
 * (r, k) at basis[6 k + r], column k belongs to eigenvalues[k]); every value is one of T */
typedef struct {
    double center[3], L, eigenvalues[6], basis[36];
} pgicp_cov_frame;

/* pgicp_covariance_sampling = CovarianceSamplingDataPointsFilter{nbSample, torqueNorm} over one cloud.
 *   xyz: n points at `stride` (>= 3); nrm: their normals at `nstride` (>= 3); desc: NULL, or `drows` (> 0) values a point,
 *   contiguous -- descriptor rows the cloud carries besides, which travel with the picks;
 *   mem: PGICP_HOST (host in, host out) or PGICP_DEVICE (device in, device out);
 *   out_xyz: the picks at `stride`, as the input (only the three coordinates of a point are written); out_nrm: at `out_nstride`
 *   (>= 3); out_desc: drows a point (required with desc); kept_idx: the picks' input indices, in PICK order.  Every output array
 *   needs room for min(n, nb_sample) points; each may be NULL.  *n_out (host): min(n, nb_sample).  frame_out (host, may be
 *   NULL): the frame the call used.
 *   mem = PGICP_DEVICE: nothing of length n crosses the bus -- the frame's sums, 6 nb_sample candidate records, nb_sample
 *   indices and *n_out.  Inputs and outputs must not overlap.
 * n == 0 gives *n_out = 0.  PGICP_ERR_ARG: n < 0, nb_sample < 1, torque_norm outside 0 .. 2, a stride below 3, desc without
 * out_desc, an input that is not finite, L not > 0.  After any refusal the context stays usable. */
int pgicp_covariance_sampling_f32(pgicp_ctx *ctx, const float *xyz, int stride, const float *nrm, int nstride, int n, int mem,
                                  int nb_sample, int torque_norm, const float *desc, int drows, float *out_xyz, float *out_nrm,
                                  int out_nstride, float *out_desc, int32_t *kept_idx, int *n_out, pgicp_cov_frame *frame_out);
int pgicp_covariance_sampling_f64(pgicp_ctx *ctx, const double *xyz, int stride, const double *nrm, int nstride, int n, int mem,
                                  int nb_sample, int torque_norm, const double *desc, int drows, double *out_xyz, double *out_nrm,
                                  int out_nstride, double *out_desc, int32_t *kept_idx, int *n_out, pgicp_cov_frame *frame_out);

/* pgicp_covariance_sampling_framed = the selection stage alone: the same call with the frame GIVEN (the frame's passes and the
 * Jacobi are skipped; center, L and basis are rounded to T, the eigenvalues are not read).  kept_idx (where `mem` says, room for
 * min(n, nb_sample)): the picks in pick order.  PGICP_ERR_ARG as above, and for a frame whose L is not > 0 and finite. */
int pgicp_covariance_sampling_framed_f32(pgicp_ctx *ctx, const float *xyz, int stride, const float *nrm, int nstride, int n, int mem,
                                         int nb_sample, const pgicp_cov_frame *frame, int32_t *kept_idx, int *n_out);
int pgicp_covariance_sampling_framed_f64(pgicp_ctx *ctx, const double *xyz, int stride, const double *nrm, int nstride, int n, int mem,
                                         int nb_sample, const pgicp_cov_frame *frame, int32_t *kept_idx, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_COVSAMPLE_H */
