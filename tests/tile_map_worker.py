"""One setting of tests/test_gpu_tile_map.py: a process of its own (PGICP_TILE_GROUP and PGICP_FAST_LANES are read once).

    python tile_map_worker.py OUT.npz

aligns, in float and in double, point-to-plane, one ragged batch of nine problems (more than eight: the queue goes through
k_queue_offsets / k_queue_compact) and one single-problem call against one map, and saves everything the calls leave behind:
T, every pgicp_stats field, the last iteration's matches (ids and distances) and the reading order of every problem, and the
debug counters."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
# max_n = 8191 at 64 queries a wave: 128 tiles, 16 per XCD (at PGICP_FAST_LANES=16: 512 tiles)
SIZES = [1, 63, 64, 65, 500, 513, 1025, 4097, 8191]
SINGLE = 8191
DTYPES = [np.float32, np.float64]


def scene():
    """(map_xyz, map_nrm, readings, T_inits) of the batch; the single call is the batch's last problem from another guess"""
    from pgslam_amd import synth
    w = synth.make_scan_to_map(n_scan=8191, n_map=30_000, n_queries=3, n_map_poses=3, rings=16)
    readings = [w.scans_xyz[k % 3][:n] for k, n in enumerate(SIZES)]
    T_inits = [w.T_truth[k % 3] @ synth.perturbation(40 + k) for k in range(len(SIZES))]
    return w.map_xyz, w.map_nrm, readings, T_inits


def single(readings, T_inits):
    from pgslam_amd import synth
    return readings[-1][:SINGLE], T_inits[-1] @ synth.perturbation(77)


def run(ctx, mid, readings, T_inits, dtype, tag, out):
    T, sa = ctx.align_batch(mid, readings, T_inits, dtype=dtype, raise_on_error=False, _raw_stats=True)
    out[f"{tag}/T"] = T
    for name in sa.dtype.names:
        out[f"{tag}/stats/{name}"] = np.ascontiguousarray(sa[name])
    for p, rd in enumerate(readings):
        ids, d2 = ctx.debug_last_matches(len(rd), problem=p, dtype=dtype)
        out[f"{tag}/ids/{p}"], out[f"{tag}/d2/{p}"] = ids, d2
        out[f"{tag}/order/{p}"] = ctx.reading_order(len(rd), problem=p)
    out[f"{tag}/counters"] = np.asarray(ctx.debug_counters(), dtype=np.int32)


def main():
    from pgslam_amd import icp
    map_xyz, map_nrm, readings, T_inits = scene()
    out = {}
    for dtype in DTYPES:
        name = np.dtype(dtype).name
        ctx = icp.Context(0, **CHAIN)
        mid = ctx.set_map(map_xyz.astype(dtype), map_nrm.astype(dtype), center=True, dtype=dtype)
        run(ctx, mid, [r.astype(dtype) for r in readings], T_inits, dtype, f"{name}/batch", out)
        rd1, T1 = single(readings, T_inits)
        run(ctx, mid, [rd1.astype(dtype)], [T1], dtype, f"{name}/single", out)
        ctx.destroy_map(mid)
        ctx.close()
    np.savez(sys.argv[1], **{k.replace("/", "__"): v for k, v in out.items()})


if __name__ == "__main__":
    main()
