# The sensor's six-filter chain (include/pgicp_sensor_chain.h) -- SimpleSensorNoise, SurfaceNormal{knn 10, keepDensities},
# ObservationDirection, OrientNormals, Shadow{eps 0.2}, MaxDensity{the cloud's median density} -- on a 100 000-point synth scan and on
# the benchmark's 1 M-point map, f32 (GPU box).  pgicp_sensor_chain_*: call times from device events around the synchronised call
# (median of --reps after 10 warm-up calls), device in / device out and host in / host out; beside it the head alone
# (pgicp_surface_densities_*) and pgicp_normals_max_density_*, device in / device out.  Then DataPointsFilters::apply on the same
# list through the C++ drop-in (tools/bench_sensor_chain_host.cpp, built here when its binary is missing): the run as one call
# against the list filter by filter -- what apply did before the call existed --, wall time, median of --host-reps, alternating; and
# the same for the eight-filter list of include/pgicp_descriptor_filters.h (IncidenceAngle, Sphericality, two cuts at 1.3 and 0.2).
# One JSON line.
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
ap.add_argument("--host-reps", type=int, default=5)
ap.add_argument("--no-map", action="store_true")
args = ap.parse_args()

T, knn, eps = np.float32, 10, 0.2
clouds = {"scan100k": np.ascontiguousarray(synth.make_two_scans(100_000, rings=64)["ref_xyz"], dtype=T)}
if not args.no_map:
    from bench import build_workload
    clouds["map1M"] = np.ascontiguousarray(build_workload(100000, 1000000, 16).map_xyz, dtype=T)
ctx = icp.Context(0)


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


exe = os.path.join(ROOT, "tools", "bench_sensor_chain_host")
if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(exe + ".cpp"):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp", "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"),
                           "-Wl,-rpath,/opt/rocm/lib"])

out = dict(lib=icp.LIB_PATH, knn=knn, eps=eps, dtype="float32", reps=args.reps, host_reps=args.host_reps)
for name, xyz in clouds.items():
    d = torch.from_numpy(xyz).cuda()
    dens = ctx.surface_densities(d, knn=knn, want_normals=False, want_eigen=False)["densities"].cpu().numpy()
    md = float(np.median(dens[np.isfinite(dens)]))
    stages = [("simple_sensor_noise", 0, 1.0), ("observation_direction", 0.0, 0.0, 0.0), ("orient_normals", 1), ("shadow", eps), ("max_density", md, 1)]
    calls = {
        "sensor_chain_device": lambda: ctx.sensor_chain(d, knn, np.inf, stages),
        "sensor_chain_host": lambda: ctx.sensor_chain(xyz, knn, np.inf, stages),
        "surface_densities_device": lambda: ctx.surface_densities(d, knn=knn, want_eigen=False),
        "normals_max_density_device": lambda: ctx.normals_max_density(d, knn=knn, max_density=md, seed=1),
    }
    res = dict(points=len(xyz), max_density=md, kept=calls["sensor_chain_device"]()["count"])
    for cname, call in calls.items():
        for _ in range(10):
            call()
        res[cname] = timed(call, args.reps)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.bin")
        with open(path, "wb") as fh:
            fh.write(struct.pack("<i", len(xyz)) + xyz.tobytes())
        res["dropin_apply"] = json.loads(subprocess.run([exe, path, repr(md), str(args.host_reps)], capture_output=True, text=True, check=True).stdout)
        # the list of include/pgicp_descriptor_filters.h: one pgicp_sensor_chain_ext_* call against filter by filter
        res["dropin_apply_descriptor"] = json.loads(subprocess.run([exe, path, repr(md), str(args.host_reps), "descriptor"], capture_output=True, text=True,
                                                                   check=True).stdout)
    out[name] = res
print(json.dumps(out))
