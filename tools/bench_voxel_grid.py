# VoxelGridDataPointsFilter timing (GPU box), written to profiles/voxel_grid.json: for f32 and f64, a 100 k keyframe scan (bench's
# build_pairs) and the 1 M-point map (bench's build_workload) at 0.1 m and 0.5 m, plus the worst case -- a 1 M-point cloud in ONE
# voxel (its sums one sequential chain) -- wall time of the ABI call host in / host out and device in / device out (centroid,
# 3 descriptor rows averaged), and of the drop-in shim's filter (tests/cpp/test_voxel_grid_cpu apply: the device path, then the
# host form with PGSLAM_HOST_VOXEL_GRID=1) at the same sizes.
#   python tools/bench_voxel_grid.py [--reps 10]
import argparse, json, os, struct, subprocess, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
from pgslam_amd import icp
from bench import build_pairs, build_workload
from test_voxel_grid_host import build_exe

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
xyz, _, _ = build_pairs(100000)
w = build_workload(100000, 1000000, 16)
one = np.random.default_rng(1).uniform(-3, 3, size=(1000000, 3))
dev = torch.device('cuda', 0)
ctx = icp.Context(0)
out = dict(filter="VoxelGridDataPointsFilter useCentroid 1 averageExistingDescriptors 1, 3 descriptor rows", reps=args.reps)
cases = (("scan_100k", xyz[0], 0.1), ("scan_100k", xyz[0], 0.5), ("map_1M", w.map_xyz, 0.1), ("map_1M", w.map_xyz, 0.5),
         ("one_voxel_1M", one, 50.0))
exe = build_exe()
for name, cloud, vs in cases:
    for T in (np.float32, np.float64):
        x = np.ascontiguousarray(cloud, dtype=T)
        d = np.random.default_rng(2).normal(size=(len(x), 3)).astype(T)
        tx, td = torch.from_numpy(x).to(dev), torch.from_numpy(d).to(dev)
        v = (vs, vs, vs)
        r = ctx.voxel_grid(x, v, descriptors=d)                    # scratch allocated, code loaded
        ctx.voxel_grid(tx, v, descriptors=td)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ctx.voxel_grid(x, v, descriptors=d)
        host_wall = (time.perf_counter() - t0) / args.reps
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(args.reps):
            ctx.voxel_grid(tx, v, descriptors=td)
        torch.cuda.synchronize(); dev_wall = (time.perf_counter() - t0) / args.reps
        rec = dict(points=int(len(x)), voxel=vs, voxels=int(len(r["kept_idx"])), max_count=int(r["count"].max()),
                   wall_ms_host_in_out=host_wall * 1e3, wall_ms_device_in_out=dev_wall * 1e3)
        # the drop-in filter (features 4 x n, the descriptors as one 3-row block): device path, then host form
        with tempfile.TemporaryDirectory() as tmp:
            fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            f = np.ones((len(x), 4), dtype=T); f[:, :3] = x
            open(fi, "wb").write(struct.pack("<ii3dii", len(x), 3, vs, vs, vs, 1, 1) + f.tobytes() + d.tobytes())
            for tag, host in (("device", False), ("host", True)):
                env = {k: val for k, val in os.environ.items() if k != "PGSLAM_HOST_VOXEL_GRID"}
                if host:
                    env["PGSLAM_HOST_VOXEL_GRID"] = "1"
                reps = args.reps if not host else max(1, min(args.reps, 3))
                p = subprocess.run([exe, "apply", "f32" if T == np.float32 else "f64", fi, fo, str(reps)], capture_output=True, text=True,
                                   timeout=900, env=env)
                assert p.returncode == 0, p.stdout + p.stderr
                kv = dict(s.split("=") for s in p.stdout.split())
                assert int(kv["on_device"]) == (0 if host else 1)
                rec[f"shim_ms_{tag}"] = float(kv["ms"])
        rec["shim_host_over_device"] = rec["shim_ms_host"] / rec["shim_ms_device"]
        key = f"{name}_v{vs}_{T.__name__}"
        out[key] = rec
        print(key, rec, flush=True)
os.makedirs("profiles", exist_ok=True)
json.dump(out, open("profiles/voxel_grid.json", "w"), indent=1)
print(json.dumps(out, indent=1))
