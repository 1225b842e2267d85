# NormalSpaceDataPointsFilter timing (GPU box), written to profiles/r13_normal_space.json: for f32 and f64, a 100 k-point scan and
# a 1 M-point cloud, nbSample 5000 and n / 4 at epsilon 0.09 -- wall time of the ABI call host in / host out and device in / device
# out, and of the drop-in's host form (tests/cpp/test_normal_space_cpu time: the filter alone, PGSLAM_HOST_INPUT_STAGE=1), the
# yardstick.
#   python tools/bench_normal_space.py [--reps 10]
#   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_normal_space.py --once     (the per-kernel split of one call)
import argparse, json, os, struct, subprocess, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
from pgslam_amd import icp
from test_density_host import build_exe

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--once", action="store_true", help="one warm-up and one 1 M f32 device call (nbSample 5000), nothing written")
args = ap.parse_args()
rng = np.random.default_rng(4)
EPSILON = 0.09


def room(n):
    """a 20 x 16 x 3 m room: points on the floor, the ceiling and the four walls with a centimetre of noise, and their normals --
    the face's own, tilted by a few degrees of noise, so that six clusters of buckets hold the cloud"""
    u = rng.uniform(size=(n, 3)) * [20.0, 16.0, 3.0]
    face = rng.integers(0, 6, size=n)
    nrm = rng.normal(scale=0.05, size=(n, 3))
    for f in range(6):
        u[face == f, f // 2] = (f % 2) * [20.0, 16.0, 3.0][f // 2]
        nrm[face == f, f // 2] += 1.0 - 2.0 * (f % 2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return u + rng.normal(scale=0.01, size=u.shape), nrm


dev = torch.device('cuda', 0)
ctx = icp.Context(0)
if args.once:
    x, nr = room(1_000_000)
    tx, tn = torch.from_numpy(x.astype(np.float32)).to(dev), torch.from_numpy(nr.astype(np.float32)).to(dev)
    for _ in range(2):
        ctx.normal_space_sampling(tx, tn, 5000, epsilon=EPSILON)
        torch.cuda.synchronize()
    sys.exit(0)
out = dict(filter="NormalSpaceDataPointsFilter", reps=args.reps, epsilon=EPSILON)
exe = build_exe("test_normal_space_cpu")
for name, n in (("scan_100k", 100_000), ("cloud_1M", 1_000_000)):
    cloud, normals = room(n)
    for T in (np.float32, np.float64):
        x, nr = np.ascontiguousarray(cloud, dtype=T), np.ascontiguousarray(normals, dtype=T)
        tx, tn = torch.from_numpy(x).to(dev), torch.from_numpy(nr).to(dev)
        for nb in (5000, n // 4):
            picks = len(ctx.normal_space_sampling(x, nr, nb, epsilon=EPSILON)["kept_idx"])         # scratch allocated, code loaded
            ctx.normal_space_sampling(tx, tn, nb, epsilon=EPSILON)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                ctx.normal_space_sampling(x, nr, nb, epsilon=EPSILON)
            host_wall = (time.perf_counter() - t0) / args.reps
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(args.reps):
                ctx.normal_space_sampling(tx, tn, nb, epsilon=EPSILON)
            torch.cuda.synchronize(); dev_wall = (time.perf_counter() - t0) / args.reps
            rec = dict(points=n, picks=picks, wall_ms_host_in_out=host_wall * 1e3, wall_ms_device_in_out=dev_wall * 1e3)
            with tempfile.TemporaryDirectory() as tmp:
                fi = os.path.join(tmp, "in.bin")
                open(fi, "wb").write(struct.pack("<iiidd", n, nb, 0, EPSILON, 1.0) + x.tobytes() + nr.tobytes())
                p = subprocess.run([exe, "time", "f32" if T == np.float32 else "f64", fi], capture_output=True, text=True, timeout=900,
                                   env=dict(os.environ, PGSLAM_HOST_INPUT_STAGE="1"))
                assert p.returncode == 0, p.stdout + p.stderr
                rec["host_form_ms"] = float(p.stdout.split()[1])
                assert int(p.stdout.split()[3]) == picks
            rec["host_form_over_device"] = rec["host_form_ms"] / rec["wall_ms_device_in_out"]
            key = f"{name}_{T.__name__}_k{nb}"
            out[key] = rec
            print(key, rec, flush=True)
os.makedirs("profiles", exist_ok=True)
json.dump(out, open("profiles/r13_normal_space.json", "w"), indent=1)
