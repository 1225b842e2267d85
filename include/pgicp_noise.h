/*
 * pgicp_noise.h -- companion header of pgicp.h: SimpleSensorNoiseDataPointsFilter's descriptor and the sensor-noise branch of
 * errorMinimizer->getOverlap() on the device.
 *
 * pgslam reads getOverlap() after every ICP: Localizer.hpp:278 decides keyframes with it, LoopCloser.hpp:331 accepts loops
 * with it.  When the user's input-filter YAML adds SimpleSensorNoiseDataPointsFilter, the reading carries a `simpleSensorNoise`
 * descriptor and libpointmatcher's getOverlap() (ErrorMinimizers/PointToPlane.cpp, PointToPoint.cpp) takes another branch: the
 * share of the LAST error elements whose distance lies below mean + noise(point).  The entry points below compute that
 * quantity where the last error elements live, for one ICP and for batches.  Conventions (buffers, `mem`, status codes, the
 * `_f32` / `_f64` suffixes, threading) are pgicp.h's, and so is the meaning of the pgslam call sites cited.  The symbols
 * are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION and every structure stay as they are.
 */
#ifndef PGICP_NOISE_H
#define PGICP_NOISE_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sensorType of SimpleSensorNoiseDataPointsFilter */
#define PGICP_SENSOR_SICK_LMS 0         /* Sick LMS-1xx */
#define PGICP_SENSOR_HOKUYO_URG 1       /* Hokuyo URG-04LX */
#define PGICP_SENSOR_HOKUYO_UTM 2       /* Hokuyo UTM-30LX */
#define PGICP_SENSOR_KINECT 3           /* Kinect / Xtion */
#define PGICP_SENSOR_SICK_TIM 4         /* Sick Tim3xx */

/* pgicp_simple_sensor_noise = [EXT] SimpleSensorNoiseDataPointsFilter{sensorType, gain} (DataPointsFilters/SimpleSensorNoise.cpp)
 * as a user's input-filter YAML applies it (input_filters_.apply, Localizer.hpp:103), for a cloud that already lives where
 * `mem` says: one elementwise kernel.  The statement is the oracle's, bit for bit (oracle/icp_oracle.c,
 * orc_simple_sensor_noise), in T, no contraction:
 *   r2 = (x x + y y) + z z;  r = sqrt(r2), correctly rounded;
 *   types 0, 1, 2, 4: v = max(minRadius, beamAngle r + beamConst), (minRadius, beamAngle, beamConst) =
 *     0 (0.012, 0.0068, 0.0008), 1 (0.028, 0.0013, 0.0001), 2 (0.018, 0.0006, 0.0015), 4 (0.004, 0.0053, -0.0092), each rounded to T;
 *   type 3: v = (r r) * T(0.5 * 0.00285);
 *   noise_out[i] = T(gain) * v.
 * xyz: n points at `stride` (>= 3), `mem` PGICP_HOST or PGICP_DEVICE; noise_out: n contiguous values, `out_mem` the same two
 * (the four combinations are allowed).  n == 0 does nothing.  PGICP_ERR_ARG: a sensor_type outside 0 .. 4, a bad argument. */
int pgicp_simple_sensor_noise_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int sensor_type, double gain,
                                  float *noise_out, int out_mem);
int pgicp_simple_sensor_noise_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int sensor_type, double gain,
                                  double *noise_out, int out_mem);

/* pgicp_arm_reading_noise: hands the NEXT ICP call of the context the `simpleSensorNoise` row of its readings, so that the call
 * also computes getOverlap()'s sensor-noise branch (Localizer.hpp:278 after Localizer.hpp:126; LoopCloser.hpp:331 after
 * LoopCloser.hpp:98).  One-shot: it applies to the next pgicp_align_*, pgicp_align_batch_*, pgicp_align_residual_batch_* or
 * pgicp_icp_pair_* call on the context, and that call consumes it whether it succeeds or not (every other entry point leaves it
 * armed).  Arming again replaces what was armed; an arm call that fails leaves the context unarmed.
 *   noise[p][i * stride[p]] = the value of reading point i of problem p, in the caller's point order (stride >= 1: one row of
 *   a column-major descriptor matrix is passed without a copy); n[p] = the number of points of that reading.  noise[p] == NULL:
 *   problem p has no noise (stride[p] and n[p] are then not looked at).  `mem` (PGICP_HOST / PGICP_DEVICE) holds for every row.
 *   The values are copied into the context inside this call, which returns when the copy is complete: no caller pointer is
 *   held afterwards.
 * The consuming call fails with PGICP_ERR_ARG before it does any work, and leaves the context usable (and unarmed), when
 *   - n_problems differs from its own, or an n[p] from its reading's size, or the element type from its own;
 *   - a value is negative or not finite.
 * A call that is not armed launches no kernel and allocates nothing because of this header. */
int pgicp_arm_reading_noise_f32(pgicp_ctx *ctx, int n_problems, const float *const *noise, const int *stride, const int *n, int mem);
int pgicp_arm_reading_noise_f64(pgicp_ctx *ctx, int n_problems, const double *const *noise, const int *stride, const int *n, int mem);

/* pgicp_last_noise_overlap = errorMinimizer->getOverlap() (Localizer.hpp:278, LoopCloser.hpp:331) for a reading that carries
 * `simpleSensorNoise`: the result for `problem` of the last ICP call of the context, which must have been armed.
 * Definition.  The sums run over the LAST iteration's error elements of the ICP -- for pgicp_align_residual_batch_* the elements
 * BEFORE the residual pass: the reduction runs between the last iteration and that pass, on the state the pass overwrites.
 *   kept     pair e = (point i, neighbour k) is kept when its combined outlier weight is not 0, the weight formed as the
 *            minimiser's reduction formed it in that iteration: a neighbour, d2 <= limit (quantile / MaxDist filters), the
 *            SurfaceNormal test, the Robust weight, the GenericDescriptor weight with that iteration's soft maximum (one device
 *            function serves both kernels).
 *   dist_e   sqrt(d2_e), correctly rounded, in T.
 *   nb       the number of kept pairs; equals pgicp_stats.n_kept.
 *   S        the sum of dist_e in DOUBLE, added in the reduction tree RT-1 at the pair's tree position,
 *            honouring pgicp_params.sum_order -- the layout and fold of the residual.  No floating-point atomics.
 *   mean     T(S / nb).
 *   count    #{ e kept : dist_e < mean + noise_i }, comparison and addition in T; an integer count (wave ballot and popcount,
 *            one integer add a block): order-free.
 *   *overlap = (double)(T(count) / T(nb));  *n_elements = nb.
 * DEVIATION (the mean's sum): upstream, and the oracle's orc_sensor_noise_overlap, add the distances one after the other in T.
 *   A parallel sum cannot reproduce that order; the sum here is in double, in a stated tree.  Only pairs whose dist - noise lies
 *   between the two means can count differently (tests/noise_overlap_ref.py bounds it per case).
 * PGICP_ERR_ARG: `problem` outside the last ICP call's own range (checked on the host), that call was not armed, the problem
 * had no noise, or its status is not PGICP_OK.  Either output pointer may be NULL. */
int pgicp_last_noise_overlap(pgicp_ctx *ctx, int problem, double *overlap, int *n_elements);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_NOISE_H */
