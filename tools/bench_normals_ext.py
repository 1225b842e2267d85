# The normals' further outputs (include/pgicp_normals_ext.h) on a 100 000-point synth scan, device in / device out (GPU box):
# call times from device events around the synchronised call for the old entry, the new entry with only the old rows, with every
# row, and with smoothing; the bytes each kernel must move, from shapes.  `--once`: one call of each for a kernel trace
# (rocprofv3 --kernel-trace --stats -- python tools/bench_normals_ext.py --once; the kernel times come from there).
# PGICP_LIB_OVERRIDE=<another libpgicp.so> times that library's old entry (`--old-only`): the A/B against a parent build.
import argparse
import json
import sys

import numpy as np
import torch

sys.path.insert(0, '.')
from pgslam_amd import icp, synth

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=100_000)
ap.add_argument("--knn", type=int, default=10)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--once", action="store_true")
ap.add_argument("--old-only", action="store_true")
ap.add_argument("--f64", action="store_true")
args = ap.parse_args()

T = np.float64 if args.f64 else np.float32
n, knn, s = args.points, args.knn, np.dtype(T).itemsize
xyz = np.ascontiguousarray(synth.make_two_scans(n, rings=64)["ref_xyz"], dtype=T)
d = torch.from_numpy(xyz).cuda()
ctx = icp.Context(0)
ALL = dict(want_eigen=True, want_eigen_vectors=True, want_mean_dist=True, want_matched_ids=True, want_ids=True, want_densities=True)
calls = {"surface_normals": lambda: ctx.surface_normals(d, knn=knn, max_dist=2.0)}
if not args.old_only:
    calls.update({
        "ext_old_rows": lambda: ctx.surface_normals_ext(d, knn=knn, max_dist=2.0),
        "ext_all_rows": lambda: ctx.surface_normals_ext(d, knn=knn, max_dist=2.0, **ALL),
        "ext_all_rows_smooth": lambda: ctx.surface_normals_ext(d, knn=knn, max_dist=2.0, smooth=True, **ALL),
    })


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


# bytes a kernel must move at the least (every input read once, every output written once), from shapes.  The normals kernel reads
# the map's 4-value records; with every row it writes normals 3, eigenvalues 3, eigenvectors 9, mean distance 1, matched ids knn,
# d2 knn, densities 1 values of T and knn int32 ids; for smoothing it writes the index 1 and the slots knn int32 besides.
rows_all = (3 + 3 + 9 + 1 + knn + knn + 1) * s + 4 * knn
bytes_ = dict(
    normals_kernel_old_rows=n * (4 * s + 3 * s),
    normals_kernel_all_rows=n * (4 * s + rows_all),
    normals_kernel_all_rows_smooth=n * (4 * s + rows_all + 4 + 4 * knn),          # (the raw normals take the normals' place)
    smoothing_kernel=n * (3 * s + 4 + 4 * knn + 3 * s),
)
out = dict(lib=icp.LIB_PATH, points=n, knn=knn, dtype=np.dtype(T).name, bytes=bytes_)
if args.once:
    for name, call in calls.items():
        call()
    torch.cuda.synchronize()
else:
    for name, call in calls.items():
        for _ in range(10):
            call()
        out[name] = timed(call, args.reps)
print(json.dumps(out))
