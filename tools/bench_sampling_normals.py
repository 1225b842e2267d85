# SamplingSurfaceNormalDataPointsFilter timing (GPU box), written to profiles/sampling_normals.json: for f32 and f64, a 100 k
# keyframe scan (bench's build_pairs) and the 1 M-point map (bench's build_workload) -- device time from the profile API
# (the "surface_normals" account), wall time of the ABI call host in / host out and device in / device out, and wall time of
# the drop-in shim's filter (tests/cpp/ssn_device_apply: the device path, then the host recursion with
# PGSLAM_HOST_SAMPLING_NORMALS=1) on the 100 k scan.
#   python tools/bench_sampling_normals.py [--reps 10]
import argparse, json, os, struct, subprocess, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'oracle'); sys.path.insert(0, 'tests')
from pgslam_amd import icp
from bench import build_pairs, build_workload

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
xyz, _, _ = build_pairs(100000)
w = build_workload(100000, 1000000, 16)
dev = torch.device('cuda', 0)
ctx = icp.Context(0)
out = dict(filter="SamplingSurfaceNormalDataPointsFilter knn 7 ratio 0.5 samplingMethod 0", reps=args.reps)
for name, cloud in (("scan_100k", xyz[0]), ("map_1M", w.map_xyz)):
    for T in (np.float32, np.float64):
        x = np.ascontiguousarray(cloud, dtype=T)
        d = torch.from_numpy(x).to(dev)
        ctx.sampling_surface_normal(x)                         # scratch allocated, code loaded
        ctx.sampling_surface_normal(d)
        ctx.profile_enable(True); ctx.profile_reset()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            r = ctx.sampling_surface_normal(x)
        host_wall = (time.perf_counter() - t0) / args.reps
        ctx.profile_enable(False)
        prof = ctx.profile()["surface_normals"]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(args.reps):
            ctx.sampling_surface_normal(d)
        torch.cuda.synchronize(); dev_wall = (time.perf_counter() - t0) / args.reps
        out[f"{name}_{T.__name__}"] = dict(points=int(len(x)), kept=int(len(r["kept_idx"])), boxes=int(r["boxes"]),
                                            device_ms=prof["total_ms"] / prof["launches"], wall_ms_host_in_out=host_wall * 1e3,
                                            wall_ms_device_in_out=dev_wall * 1e3)
        print(name, T.__name__, out[f"{name}_{T.__name__}"], flush=True)
# the drop-in filter, device path and host recursion (the driver runs both and says which ran; its wall time covers both)
from test_cpp_dropin import build
exe = build("ssn_device_apply")
with tempfile.TemporaryDirectory() as tmp:
    for T, tag in ((np.float32, "f32"), (np.float64, "f64")):
        x = np.ascontiguousarray(xyz[0], dtype=T)
        fi, fo, fy = (os.path.join(tmp, s) for s in ("in.bin", "out.bin", "f.yaml"))
        open(fi, "wb").write(struct.pack("ii", len(x), 0) + x.tobytes())
        open(fy, "w").write("- SamplingSurfaceNormalDataPointsFilter:\n    knn: 7\n    ratio: 0.5\n")
        env = {k: v for k, v in os.environ.items() if k != "PGSLAM_HOST_SAMPLING_NORMALS"}
        p = subprocess.run([exe, tag, fy, fi, fo], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stdout + p.stderr
        f = dict(kv.split("=") for ln in p.stdout.splitlines() for kv in ln.split()[1:])
        out[f"shim_scan_100k_{tag}"] = dict(wall_ms_knob_off_device=float(f["off"]) if "." in f["off"] else None,
                                            wall_ms_knob_on_host=float(f["on"]) if "." in f["on"] else None, driver=p.stdout.strip().splitlines())
        print(tag, out[f"shim_scan_100k_{tag}"], flush=True)
os.makedirs("profiles", exist_ok=True)
json.dump(out, open("profiles/sampling_normals.json", "w"), indent=1)
print(json.dumps(out, indent=1))
