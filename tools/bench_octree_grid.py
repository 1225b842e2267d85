# OctreeGridDataPointsFilter timing (GPU box), written to profiles/r12_octree_grid.json: for f32 and f64, a 100 k-point scan and
# a 1 M-point cloud, methods 0 and 2, at maxPointByNode 1, at maxSizeByNode 0.2 with a large count and (the 100 k scan only) at
# maxPointByNode 1000, whose leaves are summed by a block each -- wall time of the ABI call
# host in / host out and device in / device out, and of the drop-in's host form (tests/cpp/test_octree_grid_cpu time: the filter
# alone, PGSLAM_HOST_INPUT_STAGE=1), the yardstick.
#   python tools/bench_octree_grid.py [--reps 10]
#   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_octree_grid.py --once     (the per-kernel split of one call)
import argparse, json, os, struct, subprocess, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
from pgslam_amd import icp
from test_density_host import build_exe

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--once", action="store_true", help="one warm-up and one 1 M f32 device call (maxPointByNode 1, method 0), nothing written")
args = ap.parse_args()
rng = np.random.default_rng(4)


def room(n):
    """a 20 x 16 x 3 m room: points on the floor, the ceiling and the four walls, a centimetre of noise"""
    u = rng.uniform(size=(n, 3)) * [20.0, 16.0, 3.0]
    face = rng.integers(0, 6, size=n)
    for f in range(6):
        u[face == f, f // 2] = (f % 2) * [20.0, 16.0, 3.0][f // 2]
    return u + rng.normal(scale=0.01, size=u.shape)


dev = torch.device('cuda', 0)
ctx = icp.Context(0)
SETTINGS = (("count1", dict(max_point_by_node=1, max_size_by_node=0.0)), ("size0.2", dict(max_point_by_node=1_000_000_000, max_size_by_node=0.2)),
            ("count1000", dict(max_point_by_node=1000, max_size_by_node=0.0)))      # leaves above 64 points: method 2 goes through k_oct_heavy
if args.once:
    tx = torch.from_numpy(room(1_000_000).astype(np.float32)).to(dev)
    for _ in range(2):
        ctx.octree_grid(tx, **SETTINGS[0][1])
        torch.cuda.synchronize()
    sys.exit(0)
out = dict(filter="OctreeGridDataPointsFilter", reps=args.reps)
exe = build_exe("test_octree_grid_cpu")
for name, n in (("scan_100k", 100_000), ("cloud_1M", 1_000_000)):
    cloud = room(n)
    for T in (np.float32, np.float64):
        x = np.ascontiguousarray(cloud, dtype=T)
        tx = torch.from_numpy(x).to(dev)
        for tag, kw in SETTINGS:
            if tag == "count1000" and n != 100_000:
                continue
            for method in (0, 2):
                k = dict(kw, sampling_method=method)
                leaves = len(ctx.octree_grid(x, **k)["kept_idx"])         # scratch allocated, code loaded
                ctx.octree_grid(tx, **k)
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    ctx.octree_grid(x, **k)
                host_wall = (time.perf_counter() - t0) / args.reps
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(args.reps):
                    ctx.octree_grid(tx, **k)
                torch.cuda.synchronize(); dev_wall = (time.perf_counter() - t0) / args.reps
                rec = dict(points=n, leaves=leaves, wall_ms_host_in_out=host_wall * 1e3, wall_ms_device_in_out=dev_wall * 1e3)
                with tempfile.TemporaryDirectory() as tmp:
                    fi = os.path.join(tmp, "in.bin")
                    open(fi, "wb").write(struct.pack("<iiiidd", n, min(k["max_point_by_node"], 2147483647), method, 0, k["max_size_by_node"], 1.0) + x.tobytes())
                    p = subprocess.run([exe, "time", "f32" if T == np.float32 else "f64", fi], capture_output=True, text=True, timeout=900,
                                       env=dict(os.environ, PGSLAM_HOST_INPUT_STAGE="1"))
                    assert p.returncode == 0, p.stdout + p.stderr
                    rec["host_form_ms"] = float(p.stdout.split()[1])
                    assert int(p.stdout.split()[3]) == leaves
                rec["host_form_over_device"] = rec["host_form_ms"] / rec["wall_ms_device_in_out"]
                key = f"{name}_{T.__name__}_{tag}_method{method}"
                out[key] = rec
                print(key, rec, flush=True)
os.makedirs("profiles", exist_ok=True)
json.dump(out, open("profiles/r12_octree_grid.json", "w"), indent=1)
