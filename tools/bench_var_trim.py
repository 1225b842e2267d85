# VarTrimmedDistOutlierFilter cost (GPU box), written to profiles/var_trim.json: the headline shape (128 x 100 k scans against
# one 1 M-point map, f32; bench's build_workload) and one facade-sized problem (one 100 k scan), each with TrimmedDist 0.85 and
# with VarTrimmed (0.3, 0.95, 2.0).  Per case: scans/s of align_batch (wall, host in / host out), iterations, and the device
# time of the profile API's accounts -- "trim_select" holds the outlier filter's kernels (the selections and, with VarTrimmed,
# k_var_trim), the matcher's accounts hold the exact resolution VarTrimmed needs.
#   python tools/bench_var_trim.py [--reps 3]
import argparse, json, sys, time
import numpy as np
sys.path.insert(0, '.')
from pgslam_amd import icp
from bench import build_workload

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="profiles/var_trim.json")
args = ap.parse_args()
w = build_workload(100000, 1000000, 128)
CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=40, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
ctx = icp.Context(0, **CHAIN)
mid = ctx.set_map(w.map_xyz, w.map_nrm, center=True)
out = dict(workload="map 1 M pts, scans 100 k pts, f32", reps=args.reps, vt=[0.3, 0.95, 2.0])
for shape, P in (("batch128", 128), ("single", 1)):
    rds, T0 = w.scans_xyz[:P], w.T_init[:P]
    for filt in ("trimmed_0.85", "var_trimmed"):
        if filt == "var_trimmed":
            ctx.set_var_trim(0.3, 0.95, 2.0)
        else:
            ctx.set_var_trim()
        ctx.align_batch(mid, rds, T0)                          # scratch allocated, code loaded
        t0 = time.perf_counter()
        for _ in range(args.reps):
            T, st = ctx.align_batch(mid, rds, T0)
        wall = (time.perf_counter() - t0) / args.reps
        ctx.profile_enable(True); ctx.profile_reset()
        T, st = ctx.align_batch(mid, rds, T0)
        ctx.profile_enable(False)
        prof = {k: round(v["total_ms"], 3) for k, v in ctx.profile().items() if v["launches"]}
        dev_ms = sum(prof.values())
        rec = dict(problems=P, wall_ms=round(wall * 1e3, 3), scans_per_s=round(P / wall, 1),
                   iterations_mean=float(np.mean([s["iterations"] for s in st])), device_ms_by_account=prof,
                   filter_share_of_device=round(prof.get("trim_select", 0.0) / dev_ms, 4) if dev_ms else None,
                   trim_limit_median=float(np.median([s["trim_limit"] for s in st])))
        if filt == "var_trimmed":
            rec["tuned_ratio_median"] = float(np.median([ctx.last_var_trim_ratio(p) for p in range(P)]))
        out[f"{shape}_{filt}"] = rec
        print(shape, filt, rec, flush=True)
ctx.set_var_trim()
json.dump(out, open(args.out, "w"), indent=1)
print("wrote", args.out)
