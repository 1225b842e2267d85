"""One child of tests/test_gpu_iteration_graph.py: a process of its own (PGICP_GRAPH_MAX_P is read when a context is made, and the
context says what it captured and replayed when it is closed, under PGICP_GRAPH_DEBUG).

    python iteration_graph_worker.py OUT.npz [PROFILE.json]

ONE context runs every configuration of the iteration driver three times: with readings cut to 257 points, to 5 000, and to 257
again.  Between the first and the third run the buffers have grown, so an iteration graph captured in the first run whose key misses
one of the buffers it names is replayed on the old block in the third.  Saved: T and every stats field, the last matches, and the
tuned ratio / the noise overlap where the call has them.  With PROFILE.json the profile is on (no graph is then captured) and its
launches, units and problems per bucket are written there at the end."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, F64 = np.float32, np.float64
BASE = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
RESET = dict(knn=1, error_minimizer=0, normal_max_angle=0.0, robust_fct=0, robust_tuning=1.0, robust_scale=1, matcher=0)
ROBUST = dict(trim_ratio=1.0, robust_fct=1, robust_tuning=1.0, robust_scale=1)
VT = (0.3, 0.95, 2.0)
SMALL, LARGE = 257, 5000
ROUNDS = (SMALL, LARGE, SMALL)
BATCH = (257, 5000, 63, 5000)                  # align_batch / align_residual_batch; partial_chain_batch takes the first two

# name -> (dtype, parameters over BASE, switches: var_trim, soft (descriptor filter), normals (of the reading), radii, noise)
SINGLES = {
    "p2plane_f32": (F32, {}, ("noise",)),
    "p2plane_f64": (F64, {}, ("noise",)),
    "p2point": (F32, dict(error_minimizer=1), ()),
    "var_trim": (F32, {}, ("var_trim",)),
    "robust": (F32, ROBUST, ()),
    "desc_soft": (F32, {}, ("soft",)),
    "reading_normals": (F32, dict(normal_max_angle=0.5), ("normals",)),
    "radii_trimmed": (F32, {}, ("radii",)),
    "radii_var_trim": (F32, {}, ("radii", "var_trim")),
    "radii_robust": (F32, ROBUST, ("radii",)),
    "knn3": (F32, dict(knn=3), ()),
    "knn3_radii": (F32, dict(knn=3), ("radii",)),
    "brute": (F32, dict(matcher=1), ()),
}


def scene():
    """the scene of tests/test_gpu_var_dist.py's matcher stage, with radii drawn as there"""
    from pgslam_amd import synth
    w = synth.make_scan_to_map(n_scan=LARGE, n_map=20_000, n_queries=1, n_map_poses=3, rings=16)
    r = np.random.default_rng(20)
    radii = np.exp(r.uniform(np.log(0.05), np.log(2.0), LARGE))
    u = r.random(LARGE)
    radii[u < 0.05] = np.inf
    radii[u > 0.95] = 0.0
    values = synth.uniform(13, len(w.map_xyz), 0.0, 1.0)
    return dict(map_xyz=w.map_xyz, map_nrm=w.map_nrm, rd=w.scans_xyz[0], rd_nrm=w.scans_nrm[0], T0=w.T_init[0], radii=radii, values=values)


def put_stats(out, tag, T, sa):
    out[f"{tag}/T"] = np.asarray(T, dtype=np.float64)
    for name in sa.dtype.names:
        out[f"{tag}/stats/{name}"] = np.ascontiguousarray(sa[name])


def put_matches(ctx, out, tag, sizes, dtype):
    for p, n in enumerate(sizes):
        out[f"{tag}/ids/{p}"], out[f"{tag}/d2/{p}"] = ctx.debug_last_matches(n, problem=p, dtype=dtype)


def put_extras(ctx, out, tag, sa, var_trim, noise):
    P = len(sa)
    if var_trim:
        out[f"{tag}/var_trim_ratio"] = np.array([ctx.last_var_trim_ratio(p) for p in range(P)])
    if noise:
        ok = [p for p in range(P) if sa["status"][p] == 0]
        out[f"{tag}/noise_overlap"] = np.array([ctx.last_noise_overlap(p) for p in ok], dtype=np.float64).reshape(len(ok), 2)


def main():
    from pgslam_amd import icp
    prof_path = sys.argv[2] if len(sys.argv) > 2 else None
    s = scene()
    out = {}
    ctx = icp.Context(0, **BASE)
    if prof_path:
        ctx.profile_enable(True)
    maps = {}
    for dtype in (F32, F64):
        maps[dtype] = ctx.set_map(s["map_xyz"].astype(dtype), s["map_nrm"].astype(dtype), center=True, dtype=dtype)
        ctx.set_map_values(maps[dtype], s["values"].astype(dtype))

    def configure(prm, sw):
        ctx.set_params(**dict(BASE, **RESET))
        ctx.set_params(**prm)
        ctx.set_var_trim(*VT) if "var_trim" in sw else ctx.set_var_trim()
        ctx.set_descriptor_filter("soft" if "soft" in sw else None)

    def cut(a, sizes, dtype):
        return [a[:n].astype(dtype) for n in sizes]

    for name, (dtype, prm, sw) in SINGLES.items():
        configure(prm, sw)
        for k, n in enumerate(ROUNDS):
            tag = f"{name}/{k}_{n}"
            rd = s["rd"][:n].astype(dtype)
            noises = [ctx.simple_sensor_noise(rd, 0, 1.0, dtype=dtype)] if "noise" in sw else None
            T, sa = ctx.align_batch(maps[dtype], [rd], [s["T0"]], dtype=dtype, raise_on_error=False, _raw_stats=True,
                                    normals=cut(s["rd_nrm"], [n], dtype) if "normals" in sw else None, noises=noises,
                                    radiis=cut(s["radii"], [n], dtype) if "radii" in sw else None)
            put_stats(out, tag, T, sa)
            put_matches(ctx, out, tag, [n], dtype)
            put_extras(ctx, out, tag, sa, "var_trim" in sw, "noise" in sw)

    configure({}, ())
    dtype, mid = F32, maps[F32]
    for k, n in enumerate(ROUNDS):
        sizes = [min(b, n) for b in BATCH]
        rds, T0s = cut(s["rd"], sizes, dtype), [s["T0"]] * len(sizes)
        tag = f"align_batch/{k}_{n}"
        T, sa = ctx.align_batch(mid, rds, T0s, dtype=dtype, raise_on_error=False, _raw_stats=True)
        put_stats(out, tag, T, sa)
        put_matches(ctx, out, tag, sizes, dtype)
        tag = f"align_residual_batch/{k}_{n}"
        T, sa, res, ratio, rst = ctx.align_residual_batch(mid, rds, T0s, dtype=dtype, raw_stats=True)
        put_stats(out, tag, T, sa)
        put_matches(ctx, out, tag, sizes, dtype)
        out[f"{tag}/residual"], out[f"{tag}/ratio"], out[f"{tag}/res_status"] = res, ratio, rst
        tag = f"partial_chain_batch/{k}_{n}"
        ratio, resid, status = ctx.partial_chain_batch([mid] * 2, rds[:2], T0s[:2], dtype=dtype, raise_on_error=False)
        out[f"{tag}/ratio"], out[f"{tag}/residual"], out[f"{tag}/status"] = ratio, resid, status
        put_matches(ctx, out, tag, sizes[:2], dtype)
        tag = f"match/{k}_{n}"
        out[f"{tag}/ids"], out[f"{tag}/d2"] = ctx.match(mid, rds[1], T=s["T0"], dtype=dtype)
        out[f"{tag}/counters"] = np.asarray(ctx.debug_counters(), dtype=np.int32)

    if prof_path:
        prof = {k: {f: v[f] for f in ("launches", "units", "problems")} for k, v in ctx.profile().items()}
        with open(prof_path, "w") as f:
            json.dump(prof, f, indent=1, sort_keys=True)
    for mid in maps.values():
        ctx.destroy_map(mid)
    ctx.close()                                  # (PGICP_GRAPH_DEBUG: the context's line on stderr)
    np.savez(sys.argv[1], **{k.replace("/", "__"): v for k, v in out.items()})


if __name__ == "__main__":
    main()
