/*
 * pgicp_octree.h -- companion header of pgicp.h: OctreeGridDataPointsFilter on the device.
 *
 * The adaptive spatial down-sampler of libpointmatcher (DataPointsFilters/OctreeGrid.cpp over utils/octree), restated AS
 * RECALLED -- upstream's text was not at hand; every place the recollection could differ is a DEVIATION below.  One output point
 * per non-empty leaf of an octree built over the cloud.  Conventions (buffers, `mem`, status codes, the `_f32` / `_f64` suffixes,
 * threading) are pgicp.h's.  The symbols are part of libpgicp.so; pgicp.h's own set of declarations, PGICP_ABI_VERSION and every
 * structure stay as they are.
 *
 * The statement.  Inputs: n points x_i (3-D), maxPointByNode >= 1, maxSizeByNode >= 0 (finite), samplingMethod in 0 .. 3, seed.
 * All arithmetic is in T, no contraction, the expression order as written.
 *
 *   Root.    lo_a / hi_a = the min / max of coordinate a (a -0 counts as +0; no result depends on it);  e_a = hi_a - lo_a;
 *            c_a = lo_a + e_a * T(0.5);  r = T(0.5) * max_a e_a.  The root is the node (c, r) at depth 0.
 *   Leaf.    A node (c, r, d) is a leaf if it holds <= maxPointByNode points, or r * T(2) <= maxSizeByNode, or d = 21.
 *   Split.   Otherwise h = r * T(0.5); a point goes to child m = sum_a (x_a > c_a) << a (a point ON a centre plane falls to
 *            the lower child); child m has radius h and centre c_a + h where bit a of m is set, c_a - h where it is not.
 *            The path of a point is therefore a function of the root and of that point alone: a code of 3 bits a level, the
 *            level-l digit above the level-(l+1) digit, at most 63 bits.  The size rule depends on the depth only: d_size is
 *            the smallest depth at which it holds, and a code has 3 min(21, d_size) bits.
 *   Order.   Leaves are visited depth first, children in order 0 .. 7 -- the ascending order of the codes.  Empty leaves emit
 *            nothing.  Inside a leaf the points are in ascending input index.  One output point per non-empty leaf, in leaf
 *            order.
 *   Sampling (count = the leaf's points, first = its smallest index):
 *     0 first     the leaf's first point.
 *     1 random    the leaf's j-th point, j = (mix(seed * 0x100000001B3 + first) >> 11) mod count, in 64-bit unsigned
 *                 arithmetic; mix is the SplitMix64 finaliser RandomSamplingDataPointsFilter draws with.
 *     2 centroid  rows 0-2 become ((x_1 + x_2) + x_3) + ... in ascending index, divided by T(count); every descriptor row is
 *                 averaged the same way (normals are NOT renormalised); kept_idx names the first point, whose further feature
 *                 rows the drop-in keeps.
 *     3 medoid    the centroid as in 2; the point with the smallest (dx dx + dy dy) + dz dz to it, d = x - centroid, ties to the
 *                 smallest index; it is kept with its own rows.
 *   DEVIATION (a): the depth is capped at 21 (a 63-bit code).  Upstream recurses without end on more than maxPointByNode
 *     coincident points.
 *   DEVIATION (b): a coordinate that is not finite is refused with PGICP_ERR_ARG.
 *   DEVIATION (c): an empty cloud gives an empty cloud.
 *   DEVIATION (d): only 3-D clouds (upstream builds a quadtree for 2-D ones).
 *   DEVIATION (e): method 1's draw is the seeded one above, not upstream's generator: the same distribution, not the same points.
 *   `buildParallel` is accepted and ignored by the YAML loader: the result does not depend on it.
 *   The YAML loader wants maxPointByNode or maxSizeByNode given: with neither, the defaults (1 and 0) keep every distinct point --
 *   the cloud whole, reordered, coincident points merged -- and such an entry is refused as an omission.  The C ABI and the C++
 *   constructor take the defaults as they are.
 */
#ifndef PGICP_OCTREE_H
#define PGICP_OCTREE_H

#include "pgicp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PGICP_OCTREE_MAX_DEPTH 21

/* pgicp_octree_grid = OctreeGridDataPointsFilter{maxPointByNode, maxSizeByNode, samplingMethod} over one cloud.
 *   xyz: n points at `stride` (>= 3); mem: PGICP_HOST (host in, host out) or PGICP_DEVICE (device in, device out);
 *   max_size_by_node is rounded to T; seed in [0, 2^53) is read by sampling_method 1 only;
 *   desc: NULL, or `drows` (> 0) values a point, contiguous -- descriptor rows, which travel as the statement says;
 *   out_xyz at `out_stride` (>= 3; only the three coordinates of a point are written); out_desc: drows a point (required with
 *   desc); kept_idx: the leaf's first index for method 2, the kept point's index otherwise; out_count: the leaf's points;
 *   out_depth: the leaf's depth.  Every output array needs room for n points; each may be NULL.  *n_out (host): the leaves.
 *   mem = PGICP_DEVICE: nothing of length n crosses the bus -- the bounds record and *n_out come back.  Inputs and outputs must
 *   not overlap.
 * n == 0 gives *n_out = 0.  PGICP_ERR_ARG: n < 0, max_point_by_node < 1, max_size_by_node negative or not finite (in T),
 * sampling_method outside 0 .. 3, seed >= 2^53, a stride below 3, desc without out_desc, a coordinate that is not finite.
 * After any refusal the context stays usable. */
int pgicp_octree_grid_f32(pgicp_ctx *ctx, const float *xyz, int stride, int n, int mem, int max_point_by_node, double max_size_by_node,
                          int sampling_method, unsigned long long seed, const float *desc, int drows, float *out_xyz, int out_stride,
                          float *out_desc, int32_t *kept_idx, int32_t *out_count, int32_t *out_depth, int *n_out);
int pgicp_octree_grid_f64(pgicp_ctx *ctx, const double *xyz, int stride, int n, int mem, int max_point_by_node, double max_size_by_node,
                          int sampling_method, unsigned long long seed, const double *desc, int drows, double *out_xyz, int out_stride,
                          double *out_desc, int32_t *kept_idx, int32_t *out_count, int32_t *out_depth, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* PGICP_OCTREE_H */
