"""Reference statement of RobustOutlierFilter with distanceType, the berg scale and nbIterationForScale (include/pgicp_robust.h),
in numpy, and the ICP loop of the oracle (oracle/icp_oracle.c, orc_icp_map_ex) composed in Python from the oracle's exported stages
with that filter behind the matcher, the way tests/var_dist_ref.py composes it.

Everything is formed in T (numpy keeps float32 operands in float32), in the order the header writes it:
    e2 = dd / (s * s);  the seven weight expressions of orc_robust_weights;  the 1e-50 floor in double only;  the approximation cut
    s: none 1 | mad sqrt(MAD) while estimating | berg 1.9 sqrt(median) in iteration 1, then 0.85 (s - target) + target
    dd: d2, or ((nx dx + ny dy) + nz dz)^2 with d = p' - q
tests/test_robust_ext_host.py pins weights() to orc_robust_weights and icp_ref(mad, nb 0, point2point) to Oracle.icp before anything
rests on them."""
import numpy as np

from var_dist_ref import cut, mat4_mul, rigid_inverse

FCT = dict(cauchy=1, welsch=2, sc=3, gm=4, tukey=5, huber=6, L1=7)
EST = dict(none=0, mad=1, berg=2)
DIST = dict(point2point=0, point2plane=1)


def median(values):
    """Matches::getDistsQuantile(0.5) as the oracle takes it: the element of index size / 2 of the sorted finite values"""
    v = np.sort(np.asarray(values)[np.asarray(values) != np.inf])
    return v[v.size // 2]


def mad(d2):
    v = np.asarray(d2)[np.asarray(d2) != np.inf]
    med = median(v)
    return median(np.where(v > med, v - med, med - v))


def estimates(nb, it):
    """the estimate rule: it = 1, 2, ..."""
    return nb == 0 or it <= nb


def scale(est, nb, it, s_prev, d2, target, T):
    """the scale of iteration `it` (a value of T) from the finite point-to-point distances of the iteration and the scale before"""
    T = np.dtype(T).type
    if est == EST["none"]:
        return T(1)
    if not estimates(nb, it):
        return T(s_prev)
    if est == EST["mad"]:
        return np.sqrt(T(mad(np.asarray(d2, dtype=T))))
    if it == 1:
        return T(1.9) * np.sqrt(T(median(np.asarray(d2, dtype=T))))
    return T(0.85) * (T(s_prev) - T(target)) + T(target)


def weights(dd, fct, k, s2, approx, T, has_neighbour=None):
    """the weight of every pair: dd (the distance the filter weighs by), tuning k, squared scale s2, approximation (<= 0 or inf: none)"""
    Tt = np.dtype(T).type
    dd = np.asarray(dd, dtype=T)
    k, s2 = Tt(k), Tt(s2)
    k2 = k * k
    with np.errstate(all="ignore"):
        e2 = dd / s2
        if fct == 1:
            w = Tt(1) / (Tt(1) + e2 / k2)
        elif fct == 2:
            w = np.exp(-(e2 / k2))
        elif fct == 3:
            t = k + e2
            w = np.where(e2 >= k, (Tt(4) * k2) / (t * t), Tt(1))
        elif fct == 4:
            t = k + e2
            w = k2 / (t * t)
        elif fct == 5:
            t = Tt(1) - e2 / k2
            w = np.where(e2 >= k2, Tt(0), t * t)
        elif fct == 6:
            w = np.where(e2 >= k2, k / np.sqrt(e2), Tt(1))
        elif fct == 7:
            w = Tt(1) / np.sqrt(e2)
        else:
            raise ValueError(fct)
        w = w.astype(T)
        if np.dtype(T) == np.float64:
            w = np.where(w <= 1e-50, 1e-50, w)
        a = Tt(approx)
        if approx > 0 and not np.isinf(approx):
            w = np.where(e2 >= a * a, Tt(0), w)
    if has_neighbour is None:
        has_neighbour = dd != np.inf
    return np.where(has_neighbour, w, Tt(0)).astype(T)


def plane_dd(step, ref_c, nrm, ids, T):
    """dd of distanceType point2plane for every pair (pairs without a neighbour: +inf)"""
    Tt = np.dtype(T).type
    ok = ids >= 0
    j = np.where(ok, ids, 0)
    p, q, n = np.asarray(step, dtype=T), np.asarray(ref_c, dtype=T)[j], np.asarray(nrm, dtype=T)[j]
    dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
    v = (n[:, 0] * dx + n[:, 1] * dy) + n[:, 2] * dz
    dd = v * v
    assert dd.dtype == np.dtype(T)
    return np.where(ok, dd, Tt(np.inf)).astype(T)


def icp_ref(orc, reading, ref, nrm, T0, radii=None, distance_type=0, scale_estimator=None, nb=0, residual_pass=False, **chain):
    """orc: an oracle.Oracle of the element type; chain: the oracle's parameter names (as var_dist_ref.icp_ref; robust_fct > 0).
    scale_estimator None: what robust_scale says.  Returns a list: entry k - 1 is what Oracle.icp's dict would be for a run with
    max_iters = k (k = 1 .. max_iters; a run that ended earlier repeats its end), each with the per-iteration scales `s_hist`, the
    last iteration's `w` / `dd`, and -- residual_pass -- `res_residual` / `res_ratio` of one more pass of the chain at the result."""
    T = orc.dtype.type
    from oracle import DEFAULT_CHAIN
    prm = dict(DEFAULT_CHAIN, error_minimizer=0, outlier_max_dist=0.0, robust_fct=1, robust_tuning=1.0, robust_scale=1, robust_approx=0.0,
               pair_order=None)
    assert set(chain) <= set(prm), sorted(set(chain) - set(prm))
    prm.update(chain)
    prm["trim_ratio"] = 1.0
    est = prm["robust_scale"] if scale_estimator is None else scale_estimator
    fct, approx = prm["robust_fct"], prm["robust_approx"]
    target = T(prm["robust_tuning"])
    k = T(1) if est == EST["berg"] else T(prm["robust_tuning"])
    order = prm["pair_order"]
    reading = np.ascontiguousarray(reading, dtype=T)
    ref = np.ascontiguousarray(ref, dtype=T)
    nrm = np.ascontiguousarray(nrm, dtype=T)
    n = reading.shape[0]
    mean = orc.centroid(ref)
    ref_c = np.ascontiguousarray(ref - mean[None, :])
    T_ref_mean = np.eye(4)
    T_ref_mean[:3, 3] = mean.astype(np.float64)
    T_pre = mat4_mul(rigid_inverse(T_ref_mean), np.asarray(T0, dtype=np.float64))
    rd = orc.transform(T_pre, reading)
    T_iter, dT = np.eye(4), np.eye(4)
    chk = orc.checker(prm["max_iters"], prm["min_diff_rot"], prm["min_diff_trans"], prm["smooth_length"])
    md, omd = T(prm["max_dist"]), T(prm["outlier_max_dist"])
    has_omd = omd > 0 and not np.isinf(omd)
    state = dict(s=T(0), s_hist=[])

    def one_pass(T_at, it):
        """match, scale, weights, error elements at T_at as iteration `it`: (status, sys, step, ids, d2, w, dd)"""
        step = orc.transform(T_at, rd)
        ids, d2 = orc.knn_kdtree(step, ref_c, md)
        if radii is not None:
            ids, d2, _ = cut(ids, d2, radii, 1, T)
        if not np.count_nonzero(d2 != np.inf):
            return 1, None, step, ids, d2, None, None
        state["s"] = scale(est, nb, it, state["s"], d2, target, T)
        s = state["s"]
        dd = plane_dd(step, ref_c, nrm, ids, T) if distance_type == DIST["point2plane"] else d2
        w = weights(dd, fct, k, s * s, approx, T, has_neighbour=ids >= 0)
        if has_omd:
            w = np.where(d2 <= omd * omd, w, T(0)).astype(T)
        if prm["error_minimizer"] == 1:
            st, sys_ = orc.p2point_system(step, ref_c, ids, w, order=order)
        else:
            st, sys_ = orc.p2plane_system(step, ref_c, nrm, ids, w, order=order)
        return st, sys_, step, ids, d2, w, dd

    out = dict(status=0, iterations=0, converged=False, max_iter_reached=False, overlap=0.0, residual=0.0, trim_limit=0.0, n_kept=0, n_finite=0)
    snaps = []

    def snapshot(status, step, ids, d2, w, dd):
        r = dict(out, status=status, iterations=it, s_hist=list(state["s_hist"]), last_ids=ids, last_d2=d2, w=w, dd=dd)
        if status == 0:
            r["cov"] = np.zeros((6, 6)) if prm["error_minimizer"] == 1 else \
                orc.covariance(step, ref_c, nrm, ids, w, dT, prm["sensor_std_dev"], order=order)
            r["T"] = mat4_mul(T_ref_mean, mat4_mul(T_iter, T_pre))
            if residual_pass:
                keep = state["s"]
                st, sys_, *_ = one_pass(T_iter, it + 1)
                state["s"] = keep
                ok = st == 0 and sys_[28] > 0
                r["res_residual"] = float(sys_[29]) if ok else np.inf
                r["res_ratio"] = float(sys_[27]) / float(n) if ok else 0.0
        else:
            r["cov"], r["T"] = np.zeros((6, 6)), np.eye(4)
        return r

    it = 0
    while True:
        status, sys_, step, ids, d2, w, dd = one_pass(T_iter, it + 1)
        if status != 0:
            snaps.append(snapshot(status, step, ids, d2, w, dd))
            break
        state["s_hist"].append(state["s"])
        if prm["error_minimizer"] == 1:
            dT, _ = orc.solve_p2point(sys_)
        else:
            x, _ = orc.solve6(sys_)
            dT = orc.delta_T(x)
        T_iter = mat4_mul(dT, T_iter)
        out["overlap"] = float(sys_[27]) / float(n)
        out["residual"] = float(sys_[29])
        out["trim_limit"] = float(omd * omd) if has_omd else np.inf
        out["n_kept"] = int(sys_[28])
        out["n_finite"] = int(np.count_nonzero(d2 != np.inf))
        it += 1
        f = orc.checker_check(chk, T_iter)
        status = 3 if f & 8 else 4 if f & 16 else 0
        if f & 2:
            out["converged"] = True
        snaps.append(snapshot(status, step, ids, d2, w, dd))
        if status != 0 or not f & 1:
            break
    while len(snaps) < prm["max_iters"]:
        snaps.append(snaps[-1])
    return snaps


# ---- the scene of the whole-ICP tests (tests/test_robust_ext_host.py checks its conditions on the reference alone) ----
SIZES = (1, 63, 64, 65, 257, 2049)      # the wave, the reduce block, one pair past the 2 048-pair span of a tree block
MAP_POINTS = 4000
# (thresholds no run of six iterations reaches: every case runs the iterations it is given)
BASE = dict(max_dist=1.0, trim_ratio=1.0, max_iters=6, min_diff_rot=1e-9, min_diff_trans=1e-9, smooth_length=3, sensor_std_dev=0.01)
# per scale estimator: the tuning (berg: the target scale, in metres) and an approximation that zeroes some pairs, fewer than half
TUNING = {0: 0.5, 1: 3.0, 2: 0.3}
APPROX = {0: 0.3, 1: 2.0, 2: 1.0}
_SCENE = {}


def scene():
    """synth.make_two_scans(4 000 points, 16 rings): the map with its normals, the other scan as the reading, the first guess"""
    if not _SCENE:
        from pgslam_amd import synth
        s = synth.make_two_scans(MAP_POINTS, rings=16)
        _SCENE.update(ref=s["ref_xyz"], ref_nrm=s["ref_nrm"], rd=s["reading_xyz"], T_truth=s["T_truth"], T_init=s["T_init"])
    return _SCENE


def reading(n):
    """n points of the scene's reading, evenly taken; from 63 points on the second one is moved 50 m up: a point without a
    neighbour under max_dist in every iteration"""
    rd = scene()["rd"]
    out = rd[(np.arange(n, dtype=np.int64) * len(rd)) // n].copy()
    if n >= 63:
        out[1, 2] += 50.0
    return out


def chain(fct, est, approx):
    """the oracle's parameter names of a robust chain of the scene"""
    return dict(BASE, robust_fct=FCT[fct] if isinstance(fct, str) else fct, robust_tuning=TUNING[est], robust_scale=min(est, 1),
                robust_approx=APPROX[est] if approx else 0.0)


RESULT_KEYS = ("overlap", "residual", "trim_limit", "n_kept", "n_finite", "iterations")


def same_result(a, b):
    """T, cov, residual, overlap, n_kept, n_finite, trim_limit, iterations: bit for bit"""
    return (np.asarray(a["T"]).tobytes() == np.asarray(b["T"]).tobytes() and np.asarray(a["cov"]).tobytes() == np.asarray(b["cov"]).tobytes()
            and all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in RESULT_KEYS))


def diff_report(a, b):
    return {k: (a[k], b[k]) for k in RESULT_KEYS if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes()} | \
        {"T": float(np.abs(np.asarray(a["T"]) - np.asarray(b["T"])).max()), "cov": float(np.abs(np.asarray(a["cov"]) - np.asarray(b["cov"])).max())}


# the batch of three: (x, y, z, yaw in degrees) off the truth and the reading's size; they converge after 4, 5 and 6 iterations under
# BATCH_CHECKERS (tests/test_robust_ext_host.py asserts that they differ)
BATCH = (((0.05, 0.02, 0.0, 0.5), 2049), ((0.25, -0.15, 0.05, 3.0), 257), ((-0.4, 0.3, 0.1, -5.0), 2049))
BATCH_CHECKERS = dict(max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01)


def batch_problems():
    """[(reading, T_init)] of BATCH"""
    import math
    from pgslam_amd import synth
    sc = scene()
    return [(reading(n), sc["T_truth"] @ synth.se3(x, y, z, math.radians(yaw))) for (x, y, z, yaw), n in BATCH]
