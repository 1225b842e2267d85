/*
 * pgicp_quantile.h -- companion header of pgicp.h: MaxQuantileOnAxisDataPointsFilter on the device.
 *
 * The filter drops the far tail of a cloud along one axis: it cuts at an order statistic of that coordinate.  It is restated here
 * AS RECALLED from libpointmatcher's DataPointsFilters/MaxQuantileOnAxis.cpp -- upstream's text was not at hand; every place the
 * recollection could differ is a DEVIATION below.  Conventions (buffers, `mem`, status codes, the `_f32` / `_f64` suffixes,
 * threading) are pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION and every
 * structure stay as they are.
 *
 * The statement.  A cloud of n points, v_i = features(dim, i), T the cloud's scalar type.
 *   Rank.    k = (int)(T(n) * ratio): the product is rounded in T, with ratio held as T, then truncated -- upstream's
 *            `nbPointsIn * ratio`, the position its nth_element is given.  The rounding is observable: n = 90, ratio = 0.7 gives
 *            k = 63 in float and k = 62 in double.
 *   DEVIATION (b): k is clamped to n - 1.
 *   Limit.   limit = the k-th smallest (0-based) of the v_i.
 *   Cut.     Point i is kept iff v_i < limit, strictly, the IEEE comparison in T.  Order is preserved; the features and every
 *            descriptor row travel with a kept point.  Ties at the limit are all dropped: the kept count is <= k.
 *            n == 0: nothing happens.  k == 0: the cloud comes back empty.
 *   DEVIATION (a): upstream's nth_element over NaNs is undefined.  Here a NaN on the axis orders after +inf and all NaNs are equal
 *     to each other; a NaN is never kept (the comparison is false); -0 and +0 are one value; a NaN limit keeps nothing.  A NaN on
 *     another axis is not looked at.
 *   The limit is reported canonically: +0 for either zero, the default quiet NaN for any NaN (and for n == 0).
 *   Parameters, as upstream: dim in {0, 1, 2}; ratio finite, in (0, 1) (the YAML loader and the C++ constructor hold it to
 *   upstream's [1e-7, 0.9999999]).  The YAML loader wants ratio given: upstream's default of 0.5 drops half of every scan, and an
 *   entry without it is refused as an omission.
 *
 * On the device the limit is an exact radix select over order-preserving integer keys of the IEEE bits (32-bit and 64-bit), spread
 * over the chip with integer atomics only: the result does not depend on the order of arrival.
 */
#ifndef PGICP_QUANTILE_H
#define PGICP_QUANTILE_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An entry of pgicp_filter_cloud_* / pgicp_filter_cloud_dev_*'s list (pgicp_filter::type): p[0] = dim, p[1] = ratio as T, widened
 * to double.  The entry sees exactly the survivors of the entries before it -- n above is their number -- and the count, the rank,
 * the selection and the limit stay on the device.  Any number of such entries, in any order with the other types.
 * PGICP_ERR_ARG (the context stays usable): dim not in {0, 1, 2}; ratio not finite or not in (0, 1). */
#define PGICP_FILTER_MAX_QUANTILE_ON_AXIS 8

/* pgicp_axis_quantile: the same selection over a whole cloud.
 *   feat: n points at `stride` (>= 3) values a point; mem: PGICP_HOST or PGICP_DEVICE -- with PGICP_DEVICE only the three
 *   scalars come down; dim in {0, 1, 2}; ratio: finite, in (0, 1), taken as T.
 *   *limit: the k-th smallest of feat[i * stride + dim]; *k_out: the rank; *below: the number of i with value < *limit (what the
 *   filter keeps).  Each may be NULL.  n == 0: *limit = NaN, *k_out = 0, *below = 0.
 * PGICP_ERR_ARG: n < 0, stride < 3, dim or ratio out of range, a bad `mem`. */
int pgicp_axis_quantile_f32(pgicp_ctx *ctx, const float *feat, int stride, int n, int mem, int dim, double ratio, float *limit,
                            int *k_out, int *below);
int pgicp_axis_quantile_f64(pgicp_ctx *ctx, const double *feat, int stride, int n, int mem, int dim, double ratio, double *limit,
                            int *k_out, int *below);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_QUANTILE_H */
