# CovarianceSamplingDataPointsFilter timing (GPU box), written to profiles/r11_covariance_sampling.json: for f32 and f64, a
# 100 k-point scan and a 1 M-point cloud at nbSample 5000 -- wall time of the ABI call host in / host out and device in / device
# out, and of the drop-in's host form (tests/cpp/test_covariance_sampling_cpu apply, PGSLAM_HOST_INPUT_STAGE=1; process start and
# file reading included, reported beside an empty-filter run of the same program).
#   python tools/bench_covariance_sampling.py [--reps 10]
#   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_covariance_sampling.py --once     (the per-pass split of one call)
import argparse, json, os, struct, subprocess, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
from pgslam_amd import icp
import covariance_sampling_ref as ref
from test_density_host import build_exe

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--once", action="store_true", help="one warm-up and one 100 k f32 device call, nothing written")
args = ap.parse_args()
x100, n100 = ref.cloud("room", 100_000, np.float64)
rng = np.random.default_rng(4)
# the 1 M cloud: the scan ten times over, each copy jittered by a centimetre
x1m = np.concatenate([x100 + rng.normal(scale=0.01, size=x100.shape) for _ in range(10)])
n1m = np.concatenate([n100] * 10)
dev = torch.device('cuda', 0)
ctx = icp.Context(0)
if args.once:
    tx, tn = torch.from_numpy(x100.astype(np.float32)).to(dev), torch.from_numpy(n100.astype(np.float32)).to(dev)
    ctx.covariance_sampling(tx, tn, nb_sample=5000)
    torch.cuda.synchronize()
    ctx.covariance_sampling(tx, tn, nb_sample=5000)
    torch.cuda.synchronize()
    sys.exit(0)
out = dict(filter="CovarianceSamplingDataPointsFilter nbSample 5000 torqueNorm 1", reps=args.reps)
exe = build_exe("test_covariance_sampling_cpu")
for name, cx, cn in (("scan_100k", x100, n100), ("cloud_1M", x1m, n1m)):
    for T in (np.float32, np.float64):
        x, nr = np.ascontiguousarray(cx, dtype=T), np.ascontiguousarray(cn, dtype=T)
        tx, tn = torch.from_numpy(x).to(dev), torch.from_numpy(nr).to(dev)
        ctx.covariance_sampling(x, nr, nb_sample=5000)                 # scratch allocated, code loaded
        ctx.covariance_sampling(tx, tn, nb_sample=5000)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ctx.covariance_sampling(x, nr, nb_sample=5000)
        host_wall = (time.perf_counter() - t0) / args.reps
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(args.reps):
            ctx.covariance_sampling(tx, tn, nb_sample=5000)
        torch.cuda.synchronize(); dev_wall = (time.perf_counter() - t0) / args.reps
        rec = dict(points=int(len(x)), nb_sample=5000, wall_ms_host_in_out=host_wall * 1e3, wall_ms_device_in_out=dev_wall * 1e3)
        with tempfile.TemporaryDirectory() as tmp:
            fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            env = dict(os.environ, PGSLAM_HOST_INPUT_STAGE="1")
            for tag, nb in (("host_form", 5000), ("empty_run", len(x))):          # nbSample = n: the no-op, the program's own overhead
                open(fi, "wb").write(struct.pack("<iii", len(x), nb, 1) + x.tobytes() + nr.tobytes())
                t0 = time.perf_counter()
                p = subprocess.run([exe, "apply", "f32" if T == np.float32 else "f64", fi, fo], capture_output=True, text=True, timeout=900, env=env)
                assert p.returncode == 0, p.stdout + p.stderr
                rec[f"shim_ms_{tag}"] = (time.perf_counter() - t0) * 1e3
        rec["shim_ms_host_form_net"] = rec["shim_ms_host_form"] - rec["shim_ms_empty_run"]
        rec["host_form_over_device"] = rec["shim_ms_host_form_net"] / rec["wall_ms_host_in_out"]
        key = f"{name}_{T.__name__}"
        out[key] = rec
        print(key, rec, flush=True)
os.makedirs("profiles", exist_ok=True)
json.dump(out, open("profiles/r11_covariance_sampling.json", "w"), indent=1)
print(json.dumps(out, indent=1))
