# ElipsoidsDataPointsFilter (include/pgicp_elipsoids.h) on a 100 000-point synth scan and on the benchmark's 1 M-point map, f32, knn 7,
# samplingMethod 1, every row asked for, device in / device out (GPU box): call times from device events around the synchronised call
# (median of --reps after 10 warm-up calls) for pgicp_elipsoids_*, for the same with only normals, and for
# pgicp_sampling_surface_normal_ext_* with every row on the same clouds; then the filter's host form (tools/bench_elipsoids_host.cpp,
# built here when its binary is missing; wall time, median of --host-reps).  One JSON line.
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pgslam_amd import icp, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--no-map", action="store_true")
args = ap.parse_args()

T, knn = np.float32, 7
clouds = {"scan100k": np.ascontiguousarray(synth.make_two_scans(100_000, rings=64)["ref_xyz"], dtype=T)}
if not args.no_map:
    from bench import build_workload
    clouds["map1M"] = np.ascontiguousarray(build_workload(100000, 1000000, 16).map_xyz, dtype=T)
ctx = icp.Context(0)
ROWS = tuple(icp.Context.ELIPSOIDS_ROWS)


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


exe = os.path.join(ROOT, "tools", "bench_elipsoids_host")
if not os.path.exists(exe):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp", "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"),
                           "-Wl,-rpath,/opt/rocm/lib"])

out = dict(lib=icp.LIB_PATH, knn=knn, ratio=0.5, method=1, dtype="float32", reps=args.reps)
for name, xyz in clouds.items():
    d = torch.from_numpy(xyz).cuda()
    calls = {
        "elipsoids_all_rows": lambda: ctx.elipsoids(d, knn=knn, ratio=0.5, method=1, keep=ROWS),
        "elipsoids_normals_only": lambda: ctx.elipsoids(d, knn=knn, ratio=0.5, method=1, keep=("normals",)),
        "ssn_ext_all_rows": lambda: ctx.sampling_surface_normal_ext(d, knn=knn, ratio=0.5, sampling_method=1, want_eigen=True,
                                                                    want_eigen_vectors=True, want_densities=True),
    }
    r = calls["elipsoids_all_rows"]()
    res = dict(points=len(xyz), kept=len(r["kept_idx"]), boxes=r["boxes"])
    for cname, call in calls.items():
        for _ in range(10):
            call()
        res[cname] = timed(call, args.reps)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.bin")
        with open(path, "wb") as fh:
            fh.write(struct.pack("<i", len(xyz)) + xyz.tobytes())
        res["host_form"] = json.loads(subprocess.run([exe, path, str(args.host_reps)], capture_output=True, text=True, check=True).stdout)
    out[name] = res
print(json.dumps(out))
