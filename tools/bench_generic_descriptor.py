# GenericDescriptorOutlierFilter cost (GPU box), written to profiles/generic_descriptor.json: the headline shape (128 x 100 k scans
# against one 1 M-point map; bench's build_workload) through align_batch and one 100 k scan through align, in f32 and f64, each
# with the filter off, in hard mode (useLargerThan, every value passes: the same pairs, so the difference is the filter's own
# cost) and in soft mode (values in [0.5, 1]: every query resolved exactly, the per-iteration maximum, the weight).  Per case:
# wall time (host in / host out), scans/s, iterations and the device time of the profile API's accounts.
#   python tools/bench_generic_descriptor.py [--reps 3] [--out profiles/generic_descriptor.json]
import argparse, json, sys, time
import numpy as np
sys.path.insert(0, '.')
from pgslam_amd import icp, synth
from bench import build_workload

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default="profiles/generic_descriptor.json")
args = ap.parse_args()
w = build_workload(100000, 1000000, 128)
CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=40, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
out = dict(workload="map 1 M pts, scans 100 k pts", reps=args.reps, hard="larger 0.25 (every value passes)", soft="values uniform in [0.5, 1]")
values = synth.uniform(99, len(w.map_xyz), 0.5, 1.0)
for dtype in (np.float32, np.float64):
    ctx = icp.Context(0, **CHAIN)
    mid = ctx.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=True, dtype=dtype)
    ctx.set_map_values(mid, values.astype(dtype))
    scans = [x.astype(dtype) for x in w.scans_xyz]
    for shape, P in (("align_batch128", 128), ("align", 1)):
        rds, T0 = scans[:P], w.T_init[:P]

        def run():
            if P == 1:
                T, st = ctx.align(mid, rds[0], T0[0], dtype=dtype)
                return [st]
            return ctx.align_batch(mid, rds, T0, dtype=dtype)[1]
        for filt, setting in (("off", (None,)), ("hard", ("larger", 0.25)), ("soft", ("soft",))):
            ctx.set_descriptor_filter(*setting)
            run()                                              # scratch allocated, code loaded
            t0 = time.perf_counter()
            for _ in range(args.reps):
                st = run()
            wall = (time.perf_counter() - t0) / args.reps
            ctx.profile_enable(True); ctx.profile_reset()
            st = run()
            ctx.profile_enable(False)
            prof = {k: round(v["total_ms"], 3) for k, v in ctx.profile().items() if v["launches"]}
            rec = dict(problems=P, wall_ms=round(wall * 1e3, 3), scans_per_s=round(P / wall, 1),
                       iterations_mean=float(np.mean([s["iterations"] for s in st])), device_ms=round(sum(prof.values()), 3),
                       device_ms_by_account=prof)
            key = f"{np.dtype(dtype).name}_{shape}_{filt}"
            out[key] = rec
            print(key, rec, flush=True)
        ctx.set_descriptor_filter(None)
    ctx.close()
json.dump(out, open(args.out, "w"), indent=1)
print("wrote", args.out)
