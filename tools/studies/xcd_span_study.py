"""Study (CPU: numpy, scipy, synth): how evenly the fast matcher's tiles load the eight XCDs, by tile-group size.

    python3 tools/studies/xcd_span_study.py [G ...]          (default: 0 16 4 1; 0 = one contiguous span per XCD)

Blocks b and b + 8 of a launch share an XCD, and pgslam_amd/csrc/tile_map.hpp (restated below) says which tile of a
problem's cell-sorted reading block b runs.  The reading is sorted as the library sorts it (k_qbin: bins of 4 x 4 x 4 map
cells, x fastest, z slowest; the map's automatic cell), at the initial guess.  Cost proxy of a query: the map points within
(its nearest-neighbour distance, at most maxDist, + one cell) -- what a search that prunes with its best distance must look
at.  Cost of a wave (a tile of 64 queries): 0.4 x mean + 0.6 x busiest lane (NOTES_r03: a wave's instructions are part fixed,
part as long as its busiest lane walks).  Two passes: the initial guess (the unseeded launch) and the true pose (standing for
the seeded launches).  Prints each span's cost relative to the mean, and max / mean over the XCDs for every G -- the figure a
launch's duration follows if the XCDs never idle otherwise (set it against tools/xcd_balance.py's measurement)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from scipy.spatial import cKDTree
from bench import build_workload, CHAIN
from pgslam_amd import synth


def tile_of_block(b, nb, G):
    """tile_map.hpp, on arrays of block numbers"""
    q, r = nb >> 3, nb & 7
    xcd, j = b & 7, b >> 3
    lead = np.minimum(xcd, r)
    if G <= 0 or G >= q:
        return xcd * q + lead + j
    whole = (q // G) * G
    return np.where(j < whole, ((j // G) * 8 + xcd) * G + j % G, whole * 8 + xcd * (q - whole) + lead + (j - whole))


def sort_order(q, lo, h, dims, shift=2):
    """the reading sort's order: (bin of 2^shift cells cubed, cell inside the bin, index)"""
    c = np.clip(np.floor((q - lo) / h).astype(np.int64), 0, dims - 1)
    r = (1 << shift) - 1
    nbx, nby = (dims[0] + r) >> shift, (dims[1] + r) >> shift
    bins = (c[:, 0] >> shift) + nbx * ((c[:, 1] >> shift) + nby * (c[:, 2] >> shift))
    local = (c[:, 0] & r) | ((c[:, 1] & r) << shift) | ((c[:, 2] & r) << (2 * shift))
    return np.lexsort((np.arange(len(q)), local, bins))


def main():
    groups = [int(a) for a in sys.argv[1:]] or [0, 16, 4, 1]
    n_scans = 2
    w = build_workload(100000, 1000000, n_scans)
    m = w.map_xyz.astype(np.float64)
    m = m - m.mean(axis=0)                      # (the library centres the map; the reading follows it)
    mean = w.map_xyz.astype(np.float64).mean(axis=0)
    lo, hi = m.min(axis=0), m.max(axis=0)
    e = hi - lo
    h = np.sqrt(2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2]) / len(m))          # api_maps.inc: the automatic cell
    dims = np.floor(e / h).astype(np.int64) + 1
    tree = cKDTree(m)
    print(f"map: {len(m)} points, cell {h:.3f} m, grid {dims.tolist()}")
    total = {}                                  # (pass, G) -> the XCDs' cost summed over the scans: a launch holds them all
    for s in range(n_scans):
        p = w.scans_xyz[s].astype(np.float64)
        T0 = w.T_truth[s] @ synth.perturbation(s)
        q0 = p @ T0[:3, :3].T + T0[:3, 3] - mean
        order = sort_order(q0, lo, h, dims)
        nb = (-(-len(p) // 64) + 7) & ~7          # the launch's blocks per problem: round8(ceil(n / 64))
        for name, T in (("unseeded (initial guess)", T0), ("seeded (truth pose)", w.T_truth[s])):
            q = (p @ T[:3, :3].T + T[:3, 3] - mean)[order]
            d, _ = tree.query(q, workers=-1)
            cost = tree.query_ball_point(q, np.minimum(d, CHAIN["max_dist"]) + h, return_length=True, workers=-1).astype(np.float64)
            pad = np.full(nb * 64, np.nan)
            pad[:len(cost)] = cost
            lanes = pad.reshape(nb, 64)
            live = ~np.isnan(lanes).all(axis=1)
            wave = np.zeros(nb)
            wave[live] = 0.4 * np.nanmean(lanes[live], axis=1) + 0.6 * np.nanmax(lanes[live], axis=1)
            b = np.arange(nb)
            line = f"scan {s}, {name}: max / mean over the XCDs:"
            for G in groups:
                per_xcd = np.bincount(b & 7, weights=wave[tile_of_block(b, nb, G)], minlength=8)
                if G == groups[0]:
                    spans = np.bincount(b & 7, weights=wave[tile_of_block(b, nb, 0)], minlength=8)
                    print(f"scan {s}, {name}: the eight contiguous spans, cost / mean: " + " ".join(f"{v:.2f}" for v in spans / spans.mean()))
                line += f"  G={G if G > 0 else 'spans'}: {per_xcd.max() / per_xcd.mean():.3f}"
                total[(name, G)] = total.get((name, G), 0.0) + per_xcd
            print(line)
    for name in ("unseeded (initial guess)", "seeded (truth pose)"):
        print(f"all {n_scans} scans in one launch, {name}: max / mean over the XCDs:" +
              "".join(f"  G={G if G > 0 else 'spans'}: {total[(name, G)].max() / total[(name, G)].mean():.3f}" for G in groups))


if __name__ == "__main__":
    main()
