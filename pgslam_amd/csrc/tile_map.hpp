// tile_map.hpp -- which tile of a problem a block of the fast matcher runs (host and device; no other include needed).
//
// Blocks b and b + 8 of a launch share an XCD (round-robin dispatch, observed), so the class b & 7 is "the XCD".  A problem's
// tiles are consecutive runs of its cell-sorted reading; the sort is z-slowest, so a contiguous eighth of the tiles is one
// height slab of the scan, and the slabs do not cost the same (ground against walls).  The launch lasts as long as its
// slowest XCD.
//
// tile_of_block deals GROUPS of G consecutive tiles round the eight classes instead: the 8 G tiles [8 G g, 8 G (g + 1)) of a
// problem go G to each class, class x taking [(8 g + x) G, (8 g + x + 1) G).  Inside a class the tiles ascend with the block
// number, so consecutive blocks of an XCD still walk neighbouring map cells -- the L2 locality the spans were for, at group
// scale.  What whole groups do not cover (q mod G tiles per class, and the nb & 7 blocks beyond 8 q) is laid out behind them
// as eight contiguous spans, the first nb & 7 of them one tile longer.
//
//   * a bijection of [0, nb) for every nb >= 1 and every G;
//   * class x receives floor(nb / 8) tiles, + 1 if x < (nb & 7): never more than ceil(nb / 8) (the queue segments of
//     finish_query are sized by that: knn_q_cap);
//   * G <= 0 or G >= floor(nb / 8): one contiguous span per class -- xcd_tile (kernels.hip), which the reduce kernels keep
//     (their tiles cost the same, and partial[tile] fixes the reduction tree).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PGICP_TILE_HD __host__ __device__ __forceinline__
#else
#define PGICP_TILE_HD inline
#endif

namespace pgicp {

PGICP_TILE_HD int tile_of_block(int b, int nb, int G)
{
    const int q = nb >> 3, r = nb & 7;
    const int xcd = b & 7, j = b >> 3;
    const int lead = xcd < r ? xcd : r;                // classes before this one that hold an extra tile
    if (G <= 0 || G >= q) return xcd * q + lead + j;
    const int whole = (q / G) * G;                     // tiles per class that lie in whole groups
    if (j < whole) return ((j / G) * 8 + xcd) * G + j % G;
    return whole * 8 + xcd * (q - whole) + lead + (j - whole);
}

}  // namespace pgicp
