"""Reference statement of KDTreeVarDistMatcher's per-point search radii (include/pgicp_vardist.h), in numpy, and the ICP loop of the
oracle (oracle/icp_oracle.c, orc_icp_map_ex) composed in Python from the oracle's exported stages with that cut behind the matcher.

cut: for reading point i with radius r_i (a value of T) the neighbours kept are those with d2 <= r_i * r_i, the product formed in
T; a neighbour position without one is (-1, +inf).  The matcher's lists are in ascending (distance, index) order, so the cut only
ever takes entries from a list's tail.

icp_ref(radii=None) is orc_icp_ex restated: tests/test_var_dist_host.py pins it bit for bit against Oracle.icp before anything rests
on it.  The 4x4 products are written out in the oracle's summation order (mat4_mul: s = 0; s += a[i][k] * b[k][j], k = 0 .. 3)."""
import numpy as np


def cut(ids, d2, radii, knn, T):
    """ids, d2: (n,) or (n, knn), the exact kNN under max_dist; radii: (n,).  Returns (ids, d2) cut, and the mask of the pairs the
    cut removed (pairs that had a neighbour)."""
    T = np.dtype(T).type
    ids = np.asarray(ids)
    d2 = np.asarray(d2, dtype=T)
    r = np.asarray(radii, dtype=T)
    assert r.shape == (ids.shape[0],) and d2.shape == ids.shape
    assert ids.ndim == 1 if knn == 1 else ids.shape[1] == knn
    r2 = r * r                                   # (formed in T)
    assert r2.dtype == np.dtype(T)
    keep = d2 <= (r2 if ids.ndim == 1 else r2[:, None])
    removed = ~keep & (ids >= 0)
    return np.where(keep, ids, -1).astype(np.int32), np.where(keep, d2, T(np.inf)).astype(T), removed


def mat4_mul(a, b):
    c = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(a[i, k]) * float(b[k, j])
            c[i, j] = s
    return c


def rigid_inverse(t):
    r = np.eye(4)
    for i in range(3):
        for j in range(3):
            r[i, j] = t[j, i]
    for i in range(3):
        r[i, 3] = -(r[i, 0] * t[0, 3] + r[i, 1] * t[1, 3] + r[i, 2] * t[2, 3])
    return r


def icp_ref(orc, reading, ref, nrm, T0, radii=None, **chain):
    """orc: an oracle.Oracle of the element type; reading / ref / nrm: clouds; T0: the initial transform; radii: one per reading
    point or None (no cut); chain: the oracle's parameter names (DEFAULT_CHAIN's, knn, error_minimizer 0 / 1, outlier_max_dist,
    quantile_scale -- with trim_ratio 0.5: MedianDist --, robust_*, pair_order).  Returns what Oracle.icp returns, and per iteration
    the mask of the pairs the cut removed (`removed`) and the cut ids (`ids_hist`)."""
    T = orc.dtype.type
    from oracle import DEFAULT_CHAIN
    prm = dict(DEFAULT_CHAIN, knn=1, error_minimizer=0, outlier_max_dist=0.0, quantile_scale=1.0, robust_fct=0, robust_tuning=1.0,
               robust_scale=1, robust_approx=0.0, pair_order=None)
    assert set(chain) <= set(prm), sorted(set(chain) - set(prm))
    prm.update(chain)
    K = max(1, int(prm["knn"]))
    order = prm["pair_order"]
    reading = np.ascontiguousarray(reading, dtype=T)
    ref = np.ascontiguousarray(ref, dtype=T)
    nrm = np.ascontiguousarray(nrm, dtype=T)
    n = reading.shape[0]
    # the reference side: centred copy (orc_map_create)
    mean = orc.centroid(ref)
    ref_c = np.ascontiguousarray(ref - mean[None, :])
    assert ref_c.dtype == orc.dtype
    T_ref_mean = np.eye(4)
    T_ref_mean[:3, 3] = mean.astype(np.float64)
    T_pre = mat4_mul(rigid_inverse(T_ref_mean), np.asarray(T0, dtype=np.float64))
    rd = orc.transform(T_pre, reading)
    T_iter, dT = np.eye(4), np.eye(4)
    chk = orc.checker(prm["max_iters"], prm["min_diff_rot"], prm["min_diff_trans"], prm["smooth_length"])
    out = dict(status=0, iterations=0, converged=False, max_iter_reached=False, overlap=0.0, residual=0.0, trim_limit=0.0, n_kept=0,
               n_finite=0, removed=[], ids_hist=[])
    md = T(prm["max_dist"])
    omd = T(prm["outlier_max_dist"])
    status, it = 0, 0
    ids = d2 = w = step = None
    while True:
        step = orc.transform(T_iter, rd)
        if K == 1:
            ids, d2 = orc.knn_kdtree(step, ref_c, md)
        else:
            ids, d2 = orc.knn_k(ref_c, step, K, md)
        if radii is not None:
            ids, d2, removed = cut(ids, d2, radii, K, T)
            out["removed"].append(removed)
        out["ids_hist"].append(ids.copy())
        flat = np.ascontiguousarray(d2.reshape(-1))
        if prm["robust_fct"] > 0:
            # (orc_robust_weights fails as the quantile filters do when no pair is finite)
            nf = int(np.count_nonzero(flat != np.inf))
            if nf == 0:
                status = 1
                break
            w, _ = orc.robust_weights(flat, prm["robust_fct"], prm["robust_tuning"], prm["robust_scale"], prm["robust_approx"])
            limit = T(np.inf)
        elif prm["quantile_scale"] != 1.0:
            assert prm["trim_ratio"] == 0.5, "a quantile scale is MedianDistOutlierFilter's: ratio 0.5"
            nf = int(np.count_nonzero(flat != np.inf))
            if nf == 0:
                status = 1
                break
            w, limit, nf = orc.median_weights(flat, prm["quantile_scale"])
        else:
            status, w, limit, nf = orc.trim_weights(flat, prm["trim_ratio"])
            limit = T(limit)
            if status != 0:
                break
        if omd > 0 and not np.isinf(omd):
            w = np.where(flat <= omd * omd, w, T(0)).astype(T)
        w = w.reshape(ids.shape)
        if prm["error_minimizer"] == 1:
            status, sys_ = orc.p2point_system(step, ref_c, ids, w, order=order)
            if status != 0:
                break
            dT, _ = orc.solve_p2point(sys_)
        else:
            status, sys_ = orc.p2plane_system(step, ref_c, nrm, ids, w, order=order)
            if status != 0:
                break
            x, _ = orc.solve6(sys_)
            dT = orc.delta_T(x)
        T_iter = mat4_mul(dT, T_iter)
        out["overlap"] = float(sys_[27]) / (float(n) * K)
        out["residual"] = float(sys_[29])
        out["trim_limit"] = float(limit)
        if omd > 0 and not np.isinf(omd) and omd * omd < limit:
            out["trim_limit"] = float(omd * omd)
        out["n_kept"] = int(sys_[28])
        out["n_finite"] = nf
        it += 1
        f = orc.checker_check(chk, T_iter)
        if f & 8:
            status = 3
            break
        if f & 16:
            status = 4
            break
        if f & 2:
            out["converged"] = True
        if f & 4:
            out["max_iter_reached"] = True
        if not f & 1:
            break
    out["iterations"] = it
    out["status"] = status
    out["last_ids"], out["last_d2"] = ids, d2
    if status == 0:
        out["cov"] = np.zeros((6, 6)) if prm["error_minimizer"] == 1 else \
            orc.covariance(step, ref_c, nrm, ids, w, dT, prm["sensor_std_dev"], order=order)
        out["T"] = mat4_mul(T_ref_mean, mat4_mul(T_iter, T_pre))
    else:
        out["cov"] = np.zeros((6, 6))
        out["T"] = np.eye(4)
    return out


RESULT_KEYS = ("overlap", "residual", "trim_limit", "n_kept", "n_finite", "iterations")


def same_result(a, b):
    """T, cov, residual, overlap, n_kept, n_finite, trim_limit, iterations: bit for bit"""
    return (np.asarray(a["T"]).tobytes() == np.asarray(b["T"]).tobytes() and np.asarray(a["cov"]).tobytes() == np.asarray(b["cov"]).tobytes()
            and all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in RESULT_KEYS))


def diff_report(a, b):
    return {k: (a[k], b[k]) for k in RESULT_KEYS if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes()} | \
        {"T": float(np.abs(np.asarray(a["T"]) - np.asarray(b["T"])).max()), "cov": float(np.abs(np.asarray(a["cov"]) - np.asarray(b["cov"])).max())}


# ---- the scene of the whole-ICP tests (tests/test_var_dist_host.py checks its conditions on the reference alone) ----
# three perturbations of about 0.5 m / 5 degrees: (x, y, z, yaw, pitch, roll)
PERTURBATIONS = ((0.40, -0.25, 0.10, 5.0, 0.5, -0.5), (-0.35, 0.30, -0.10, -4.0, -0.5, 0.5), (0.30, 0.35, 0.15, 4.5, 0.3, 0.4))
_SCENE = {}


def scene():
    """synth.make_two_scans(10 000 points, 16 rings); T_inits: the truth moved by the three perturbations; radii: 0.3 + 0.02 range,
    the range of a reading point in its sensor's frame (computed in double, rounded to the call's type by the caller)"""
    if not _SCENE:
        import math
        from pgslam_amd import synth
        s = synth.make_two_scans(10_000, rings=16)
        rd = s["reading_xyz"]
        rng = np.sqrt((rd.astype(np.float64) ** 2).sum(axis=1))
        _SCENE.update(ref=s["ref_xyz"], ref_nrm=s["ref_nrm"], rd=rd, T_truth=s["T_truth"],
                      T_inits=[s["T_truth"] @ synth.se3(x, y, z, math.radians(yaw), math.radians(pitch), math.radians(roll))
                               for x, y, z, yaw, pitch, roll in PERTURBATIONS],
                      radii=0.3 + 0.02 * rng)
    return _SCENE


CHAINS = {
    "trimmed": dict(trim_ratio=0.85),
    "robust": dict(trim_ratio=1.0, robust_fct=1, robust_tuning=1.0, robust_scale=1),       # cauchy / mad
}
