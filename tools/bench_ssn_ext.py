# SamplingSurfaceNormal's further outputs (include/pgicp_ssn_ext.h) on a 100 000-point synth scan and on the benchmark's 1 M-point
# map, f32, knn 7, ratio 0.5, device in / device out (GPU box): call times from device events around the synchronised call
# (median of --reps after 10 warm-up calls) for the older entry, the new entry with no new row and with every row; a SHA-1 over the
# older entry's outputs; the bytes the two changed kernels must move with every row, from shapes.
# PGICP_LIB_OVERRIDE=<another libpgicp.so> with `--old-only` times that library's older entry: the A/B against a parent build.
import argparse
import hashlib
import json
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from pgslam_amd import icp, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--old-only", action="store_true")
ap.add_argument("--no-map", action="store_true")
args = ap.parse_args()

T, s, knn = np.float32, 4, 7
clouds = {"scan100k": np.ascontiguousarray(synth.make_two_scans(100_000, rings=64)["ref_xyz"], dtype=T)}
if not args.no_map:
    from bench import build_workload
    clouds["map1M"] = np.ascontiguousarray(build_workload(100000, 1000000, 16).map_xyz, dtype=T)
ctx = icp.Context(0)
ALL = dict(want_eigen=True, want_eigen_vectors=True, want_densities=True)


def timed(call, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


out = dict(lib=icp.LIB_PATH, knn=knn, ratio=0.5, dtype="float32")
sha = hashlib.sha1()
for name, xyz in clouds.items():
    d = torch.from_numpy(xyz).cuda()
    n = len(xyz)
    calls = {"sampling_surface_normal": lambda: ctx.sampling_surface_normal(d, knn=knn, ratio=0.5)}
    if not args.old_only:
        calls["ext_no_new_row"] = lambda: ctx.sampling_surface_normal_ext(d, knn=knn, ratio=0.5)
        calls["ext_all_rows"] = lambda: ctx.sampling_surface_normal_ext(d, knn=knn, ratio=0.5, **ALL)
    r = calls["sampling_surface_normal"]()
    for key in ("xyz", "normals", "kept_idx"):
        sha.update(r[key].cpu().numpy().tobytes())
    kept, boxes = len(r["kept_idx"]), r["boxes"]
    # bytes the two kernels must move at the least with every row, from shapes: k_box_fuse<T, true> reads the members' indices and
    # coordinates three times (extent and sum, scatter, density) and writes per fused box the normal 3, the mean 3, the eigenvalues 3,
    # the eigenvectors 9 and the density 1, and per kept point its flag and box; k_box_compact<T, true> reads per point the flag and
    # the position, per kept point the box, the coordinates 3 and the box's 3 + 13 values, and writes 3 + 3 + 13 values and the index
    res = dict(points=n, kept=kept, boxes=boxes,
               bytes=dict(fuse_all_rows=3 * n * (4 + 3 * s) + boxes * 19 * s + kept * 8,
                          fuse_old_rows=2 * n * (4 + 3 * s) + boxes * 6 * s + kept * 8,
                          compact_all_rows=n * 8 + kept * (4 + 3 * s + 16 * s + 19 * s + 4),
                          compact_old_rows=n * 8 + kept * (4 + 3 * s + 3 * s + 6 * s + 4)))
    for cname, call in calls.items():
        for _ in range(10):
            call()
        res[cname] = timed(call, args.reps)
    out[name] = res
out["sha1_old_entry_outputs"] = sha.hexdigest()
print(json.dumps(out))
