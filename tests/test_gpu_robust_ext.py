"""RobustOutlierFilter's distanceType, berg scale and nbIterationForScale on the device (include/pgicp_robust.h) against the numpy
statement of tests/robust_ext_ref.py -- the oracle's stages composed per iteration, pinned to the oracle and with its scene's
conditions checked by tests/test_robust_ext_host.py.  Whole ICPs with max_iters = 1 .. 6 bit for bit (T, iterations, covariance,
residual, overlap, n_finite, n_kept), in both element types and both sum orders; both minimisers; a batch against its single runs
and the residual pass behind it; the single-pass entry points; the sensor-noise overlap; armed radii and a MaxDist filter beside the
robust one; the refusals; a setting taken out again; and the launches a held scale spares, through the profile."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pgslam_amd import icp  # noqa: E402
import noise_overlap_ref  # noqa: E402
import robust_ext_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
ORDERS = pytest.mark.parametrize("order", [icp.SUM_ORDER_SORTED, icp.SUM_ORDER_SCAN], ids=["sorted", "scan"])
NBS = (0, 1, 2, 5)
_ORACLES = {}


def _oracle(dtype):
    from oracle import Oracle
    key = np.dtype(dtype).name
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(dtype)
    return _ORACLES[key]


class Rig:
    """one context with the scene's map, and the reading sort of (reading, T_init) -- which no chain parameter changes"""

    def __init__(self, dtype, order):
        sc = ref.scene()
        self.dtype, self.order, self.sc = dtype, order, sc
        self.ctx = icp.Context(0, **dict(ref.BASE, sum_order=order))
        self.ref, self.nrm = sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype)
        self.mid = self.ctx.set_map(self.ref, self.nrm, center=True, dtype=dtype)
        self._orders, self._aux = {}, None

    def pair_order(self, rd, T0):
        """the order the reading's pairs enter the reduction tree in: the caller's, or the reading sort's -- read off a second
        context with the same map, so that the chain set on the first one stays"""
        if self.order == icp.SUM_ORDER_SCAN:
            return None
        key = (len(rd), np.asarray(T0).tobytes())
        if key not in self._orders:
            if self._aux is None:
                self._aux = icp.Context(0, **dict(ref.BASE, trim_ratio=0.9))
                self._aux_mid = self._aux.set_map(self.ref, self.nrm, center=True, dtype=self.dtype)
            self._aux.partial_chain(self._aux_mid, rd.astype(self.dtype), T0, dtype=self.dtype)
            self._orders[key] = self._aux.reading_order(len(rd))
        return self._orders[key]

    def set_chain(self, fct, est, approx, dist, nb, **more):
        ch = dict(ref.chain(fct, est, approx), sum_order=self.order, **more)
        self.ctx.set_params(**ch)
        self.ctx.set_robust_ext(distance_type=dist, scale_estimator=est, nb_iteration_for_scale=nb)
        return {k: v for k, v in ch.items() if k != "sum_order"}

    def reference(self, rd, T0, ch, est, dist, nb, **kw):
        return ref.icp_ref(_oracle(self.dtype), rd, self.sc["ref"], self.sc["ref_nrm"], T0, distance_type=dist, scale_estimator=est, nb=nb,
                           pair_order=self.pair_order(rd, T0), **dict(ch, **kw))

    def align(self, rd, T0, **kw):
        """(T, stats) or the status of the ConvergenceError"""
        try:
            T, st = self.ctx.align(self.mid, rd.astype(self.dtype), T0, dtype=self.dtype, **kw)
            return dict(st, T=T)
        except icp.ConvergenceError as e:
            return dict(status=e.code)

    def close(self):
        self.ctx.close()
        if self._aux is not None:
            self._aux.close()


def check_runs(rig, rd, T0, fct, est, approx, dist, nb, what, **more):
    """max_iters = 1 .. 6 of one chain against the reference's entries"""
    ch = rig.set_chain(fct, est, approx, dist, nb, **more)
    snaps = rig.reference(rd, T0, ch, est, dist, nb)
    for k in range(1, ref.BASE["max_iters"] + 1):
        rig.ctx.set_params(max_iters=k)
        got, want = rig.align(rd, T0), snaps[k - 1]
        print(np.dtype(rig.dtype).name, what, "max_iters", k, "status", got["status"], want["status"], "iterations", got.get("iterations"), want["iterations"],
              "residual", got.get("residual"), want["residual"], "n_kept", got.get("n_kept"), want["n_kept"], "n_finite", got.get("n_finite"), want["n_finite"])
        assert got["status"] == want["status"], (what, k, got["status"], want["status"])
        if want["status"] == 0:
            assert ref.same_result(got, want), (what, k, ref.diff_report(got, want))
    return snaps


# ---- (a) the product of the settings at one size, a diagonal of it at every size -------------------------------------------------
@DTYPES
@ORDERS
@pytest.mark.parametrize("dist", [0, 1], ids=["point2point", "point2plane"])
@pytest.mark.parametrize("est", [0, 1, 2], ids=["none", "mad", "berg"])
def test_every_setting_is_the_reference_loop(dtype, order, dist, est):
    rig = Rig(dtype, order)
    rd, T0 = ref.reading(257), rig.sc["T_init"]
    for nb in NBS:
        for fct in ("cauchy", "tukey"):
            for approx in (False, True):
                check_runs(rig, rd, T0, fct, est, approx, dist, nb, (dist, est, nb, fct, approx))
    rig.close()


@DTYPES
@pytest.mark.parametrize("n", ref.SIZES)
def test_a_diagonal_of_the_settings_at_every_size(dtype, n):
    rigs = [Rig(dtype, icp.SUM_ORDER_SORTED), Rig(dtype, icp.SUM_ORDER_SCAN)]
    rd, T0 = ref.reading(n), rigs[0].sc["T_init"]
    seen = set()
    for i in range(12):
        dist, est, nb, fct, approx = i % 2, i % 3, NBS[i % 4], ("cauchy", "tukey")[(i // 2) % 2], bool((i // 3) % 2)
        snaps = check_runs(rigs[i % 2], rd, T0, fct, est, approx, dist, nb, (n, dist, est, nb, fct, approx))
        seen.add(snaps[-1]["status"])
    assert 0 in seen        # (one point: some chains have no point to minimise -- on both sides -- and the berg chains run)
    for r in rigs:
        r.close()


# ---- (b) both minimisers under plane distances ----------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("minimizer", [icp.MINIMIZER_POINT_TO_PLANE, icp.MINIMIZER_POINT_TO_POINT], ids=["p2plane", "p2point"])
def test_both_minimisers_under_plane_distances(dtype, minimizer):
    rig = Rig(dtype, icp.SUM_ORDER_SORTED)
    T0 = rig.sc["T_init"]
    for n in (65, 2049):
        for est, nb in ((0, 0), (1, 2), (2, 2), (2, 0)):
            check_runs(rig, ref.reading(n), T0, "cauchy", est, True, 1, nb, (minimizer, n, est, nb), error_minimizer=minimizer)
    rig.close()


# ---- (c) a batch whose problems converge at different iterations; the residual pass behind it ----------------------------------------------
@DTYPES
@pytest.mark.parametrize("est,nb", [(1, 5), (2, 3)], ids=["mad-nb5", "berg-nb3"])
def test_batch_is_its_single_runs(dtype, est, nb):
    rig = Rig(dtype, icp.SUM_ORDER_SCAN)
    ch = rig.set_chain("cauchy", est, True, 1, nb, **ref.BATCH_CHECKERS)
    probs = [(rd.astype(dtype), T0) for rd, T0 in ref.batch_problems()]
    singles = [rig.align(rd, T0) for rd, T0 in probs]
    wants = [rig.reference(rd, T0, ch, est, 1, nb, residual_pass=True)[-1] for rd, T0 in probs]
    for p, (got, want) in enumerate(zip(singles, wants)):
        assert got["status"] == want["status"] == 0 and ref.same_result(got, want), (p, ref.diff_report(got, want))
    assert len({w["iterations"] for w in wants}) == 3
    Tb, sb = rig.ctx.align_batch(rig.mid, [rd for rd, _ in probs], [T0 for _, T0 in probs], dtype=dtype)
    for p in range(3):
        assert ref.same_result(dict(sb[p], T=Tb[p]), singles[p]), (p, ref.diff_report(dict(sb[p], T=Tb[p]), singles[p]))
    # the residual pass is one more pass of the chain, iteration `iterations + 1` of its problem: with nb = 5 it estimates the
    # scale of the problem that converged after 4 and holds the scale of the one that took 6
    Tr, sr, res, ratio, rst = rig.ctx.align_residual_batch(rig.mid, [rd for rd, _ in probs], [T0 for _, T0 in probs], dtype=dtype)
    for p in range(3):
        assert rst[p] == 0 and ref.same_result(dict(sr[p], T=Tr[p]), singles[p]), p
        assert np.float64(res[p]).tobytes() == np.float64(wants[p]["res_residual"]).tobytes(), (p, res[p], wants[p]["res_residual"])
        assert np.float64(ratio[p]).tobytes() == np.float64(wants[p]["res_ratio"]).tobytes(), (p, ratio[p], wants[p]["res_ratio"])
    rig.close()


# ---- (d) the single-pass entry points are iteration 1 ---------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("dist", [0, 1], ids=["point2point", "point2plane"])
def test_partial_chain_and_seeded_probe_are_iteration_one(dtype, dist):
    rig = Rig(dtype, icp.SUM_ORDER_SCAN)
    src = icp.Context(0, **dict(ref.BASE, trim_ratio=0.85, min_diff_rot=0.001, min_diff_trans=0.01, max_iters=30))
    src_mid = src.set_map(rig.ref, rig.nrm, center=True, dtype=dtype)
    for n in (65, 2049):
        rd = ref.reading(n).astype(dtype)
        T_src, _ = src.align(src_mid, rd, rig.sc["T_init"], dtype=dtype)
        for est, nb in ((1, 0), (1, 5), (2, 0), (2, 1), (0, 2)):
            for T_at in (rig.sc["T_init"], T_src):
                ch = rig.set_chain("tukey", est, True, dist, nb)
                want = rig.reference(rd, T_at, ch, est, dist, nb)[0]
                ratio, resid = rig.ctx.partial_chain(rig.mid, rd, T_at, dtype=dtype)
                assert want["status"] == 0
                assert np.float64(ratio).tobytes() == np.float64(want["overlap"]).tobytes(), (n, est, nb, ratio, want["overlap"])
                assert np.float64(resid).tobytes() == np.float64(want["residual"]).tobytes(), (n, est, nb, resid, want["residual"])
            # the probe seeded with the source's correspondences of this reading, at the source's result
            sratio, sresid = rig.ctx.partial_chain_seeded(rig.mid, rd, T_src, src, [0, len(rig.ref)], [0], dtype=dtype)
            assert (sratio, sresid) == (ratio, resid), (n, est, nb)
            rb, sb, stb = rig.ctx.partial_chain_batch([rig.mid, rig.mid], [rd, rd], [T_src, rig.sc["T_init"]], dtype=dtype)
            assert (rb[0], sb[0]) == (ratio, resid) and stb[0] == stb[1] == 0
    src.close()
    rig.close()


@DTYPES
def test_stage_weights_are_iteration_one(dtype):
    """pgicp_outlier_weights over a bare array of distances: berg gives T(1.9) sqrt_rn(median), nb has no effect, mad stays mad"""
    T = np.dtype(dtype).type
    rng = np.random.default_rng(11)
    d2 = (rng.gamma(1.5, 0.05, size=5001) ** 2).astype(dtype)
    d2[rng.integers(0, d2.size, 40)] = np.inf
    ctx = icp.Context(0, **ref.BASE)
    for fct in ("cauchy", "tukey", "huber"):
        for est in (0, 1, 2):
            for nb in (0, 3):
                ctx.set_params(**ref.chain(fct, est, True))
                ctx.set_robust_ext(scale_estimator=est, nb_iteration_for_scale=nb)
                w, limit, nf = ctx.outlier_weights(d2)
                s = ref.scale(est, nb, 1, T(0), d2, ref.TUNING[est], dtype)
                want = ref.weights(d2, ref.FCT[fct], 1.0 if est == 2 else ref.TUNING[est], s * s, ref.APPROX[est], dtype)
                assert w.tobytes() == want.tobytes(), (fct, est, nb)
                assert nf == int(np.isfinite(d2).sum()) and np.isinf(limit)
    ctx.close()


# ---- (e) the sensor-noise overlap recomputes the last error elements ----------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("est,nb", [(1, 2), (2, 0)], ids=["mad-nb2", "berg-nb0"])
def test_noise_overlap_counts_the_reference_elements(dtype, est, nb):
    T_ = np.dtype(dtype).type
    o = _oracle(dtype)
    rig = Rig(dtype, icp.SUM_ORDER_SCAN)
    rd, T0 = ref.reading(2049).astype(dtype), rig.sc["T_init"]
    noise = o.simple_sensor_noise(rd, 0, 1.0)
    kept = {}
    for dist in (0, 1):
        ch = rig.set_chain("tukey", est, True, dist, nb)
        want = rig.reference(rd, T0, ch, est, dist, nb)[-1]
        got = rig.align(rd, T0, noise=noise)
        assert ref.same_result(got, want), ref.diff_report(got, want)
        lo, hi, nbk, _ = noise_overlap_ref.count_bounds(want["last_d2"], want["w"], noise, dtype)
        assert lo == hi, (lo, hi)
        assert got["n_elements"] == nbk == want["n_kept"]
        assert got["overlap_noise"] == float(T_(lo) / T_(nbk))
        kept[dist] = (nbk, lo)
    assert kept[0] != kept[1]       # (the plane distances keep other elements: the count is not the point2point one)
    rig.close()


# ---- (f) armed radii, and a MaxDistOutlierFilter beside the robust one ------------------------------------------------------------------------
@DTYPES
def test_with_radii_armed(dtype):
    rig = Rig(dtype, icp.SUM_ORDER_SORTED)
    rd, T0 = ref.reading(2049).astype(dtype), rig.sc["T_init"]
    radii = (0.2 + 0.02 * np.sqrt((rd.astype(F64) ** 2).sum(axis=1))).astype(dtype)
    ch = rig.set_chain("cauchy", 1, True, 1, 2)
    want = rig.reference(rd, T0, ch, 1, 1, 2, radii=radii)[-1]
    free = rig.reference(rd, T0, ch, 1, 1, 2)[-1]
    got = rig.align(rd, T0, radii=radii)
    assert want["n_finite"] < free["n_finite"] - 20                 # the radii cut pairs the scale would have been taken over
    assert ref.same_result(got, want), ref.diff_report(got, want)
    rig.close()


@DTYPES
def test_with_a_max_dist_filter_beside(dtype):
    rig = Rig(dtype, icp.SUM_ORDER_SORTED)
    rd, T0 = ref.reading(2049), rig.sc["T_init"]
    snaps = check_runs(rig, rd, T0, "cauchy", 2, False, 1, 2, "max dist", outlier_max_dist=0.35)
    # it cuts on d2, not on the plane distance: pairs within 0.35 m of their plane and beyond it from their point are dropped
    last = snaps[-1]
    far = (last["last_ids"] >= 0) & (last["last_d2"] > np.dtype(dtype).type(0.35) ** 2)
    assert far.sum() > 20 and (last["dd"][far] < last["last_d2"][far]).all() and (last["w"][far] == 0).all()
    assert last["trim_limit"] == float(np.dtype(dtype).type(0.35) ** 2)
    rig.close()


# ---- (g) refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    sc = ref.scene()
    rd, T0 = ref.reading(257), sc["T_init"]
    ctx = icp.Context(0, **ref.chain("cauchy", 1, False))
    mid = ctx.set_map(sc["ref"], sc["ref_nrm"], center=True)
    bare = ctx.set_map(sc["ref"], None, center=True)
    want = ctx.align(mid, rd, T0)

    def usable(what):
        T, st = ctx.align(mid, rd, T0)
        assert T.tobytes() == want[0].tobytes() and st["residual"] == want[1]["residual"], what

    def refused(match, fn, *a, **kw):
        with pytest.raises(icp.PgicpError, match=match) as e:
            fn(*a, **kw)
        assert e.value.code == icp.ERR_ARG

    # unknown codes, nb < 0: the setter refuses and the previous setting (none) stays in force
    refused("unknown distanceType", ctx.set_robust_ext, distance_type=2)
    refused("unknown distanceType", ctx.set_robust_ext, distance_type=-1)
    refused("unknown scaleEstimator", ctx.set_robust_ext, scale_estimator=3)
    refused("unknown scaleEstimator", ctx.set_robust_ext, scale_estimator=-2)
    refused("nbIterationForScale", ctx.set_robust_ext, nb_iteration_for_scale=-1)
    assert ctx.get_robust_ext() is None
    usable("setter refusals")
    # pgicp_set_params keeps refusing berg
    refused("scaleEstimator", ctx.set_params, robust_scale=2)
    usable("set_params berg")
    # point2plane on a map without normals: the consuming calls refuse before any work (the point-to-point minimiser needs none itself)
    ctx.set_params(error_minimizer=icp.MINIMIZER_POINT_TO_POINT)
    ctx.set_robust_ext(distance_type="point2plane")
    refused("no normals", ctx.align, bare, rd, T0)
    refused("no normals", ctx.partial_chain, bare, rd, T0)
    refused("no normals", ctx.align_batch, [mid, bare], [rd, rd], [T0, T0])
    # ... and the stage-level call over a bare distance array has no geometry
    refused("no geometry", ctx.outlier_weights, np.linspace(0.0, 1.0, 100, dtype=F32))
    ctx.set_params(error_minimizer=icp.MINIMIZER_POINT_TO_PLANE)
    ctx.clear_robust_ext()
    usable("point2plane refusals")
    # berg / nb != 0 / point2plane without a robust function: the setter refuses; set the other way round, the calls do
    ctx.set_params(robust_fct=0, trim_ratio=0.85)
    for kw in (dict(scale_estimator="berg"), dict(nb_iteration_for_scale=2), dict(distance_type="point2plane")):
        refused("need a robustFct", ctx.set_robust_ext, **kw)
    ctx.set_robust_ext()                               # ({point2point, -1, 0} asks for nothing)
    ctx.set_params(**ref.chain("cauchy", 1, False))
    ctx.set_robust_ext(scale_estimator="berg", nb_iteration_for_scale=2)
    ctx.set_params(robust_fct=0, trim_ratio=0.85)
    refused("need a robustFct", ctx.align, mid, rd, T0)
    refused("need a robustFct", ctx.partial_chain, mid, rd, T0)
    refused("need a robustFct", ctx.outlier_weights, np.linspace(0.0, 1.0, 100, dtype=F32))
    assert ctx.get_robust_ext() == dict(distance_type=0, scale_estimator=2, nb_iteration_for_scale=2)
    # knn > 1 with a robust filter stays refused
    ctx.clear_robust_ext()
    refused("knn > 1", ctx.set_params, **dict(ref.chain("cauchy", 1, False), knn=2))
    ctx.set_params(**ref.chain("cauchy", 1, False))
    usable("the rest")
    ctx.close()


# ---- (h) a setting taken out again, and the setting that asks for nothing -------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("chain", ["robust", "trimmed"])
def test_cleared_and_empty_settings_are_the_untouched_context(dtype, chain):
    sc = ref.scene()
    prm = ref.chain("tukey", 1, True) if chain == "robust" else dict(ref.BASE, trim_ratio=0.8)
    rd, T0 = ref.reading(2049).astype(dtype), sc["T_init"]
    rf, nrm = sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype)
    noise = _oracle(dtype).simple_sensor_noise(rd, 0, 1.0)

    def everything(ctx):
        mid = ctx.set_map(rf, nrm, center=True, dtype=dtype)
        T, st = ctx.align(mid, rd, T0, dtype=dtype, noise=noise)
        ids, d2 = ctx.debug_last_matches(len(rd), dtype=dtype)
        out = [T.tobytes(), st["cov"].tobytes(), ids.tobytes(), d2.tobytes()]
        out += [np.float64(st[k]).tobytes() for k in ref.RESULT_KEYS + ("overlap_noise", "n_elements")]
        out += [np.float64(v).tobytes() for v in ctx.partial_chain(mid, rd, T, dtype=dtype)]
        Tr, sr, res, ratio, rst = ctx.align_residual_batch(mid, [rd, rd[:777]], [T0, T0], dtype=dtype)
        out += [Tr.tobytes(), res.tobytes(), ratio.tobytes(), rst.tobytes()]
        w, limit, nf = ctx.outlier_weights(d2)
        return out + [w.tobytes(), np.float64(limit).tobytes(), nf]

    untouched = icp.Context(0, **prm)
    want = everything(untouched)
    untouched.close()
    cleared = icp.Context(0, **prm)
    if chain == "robust":
        cleared.set_robust_ext(distance_type="point2plane", scale_estimator="berg", nb_iteration_for_scale=2)
        mid = cleared.set_map(rf, nrm, center=True, dtype=dtype)
        T, st = cleared.align(mid, rd, T0, dtype=dtype)
        assert T.tobytes() != want[0]                       # (the setting was in force)
    else:
        cleared.set_robust_ext()
    cleared.clear_robust_ext()
    assert cleared.get_robust_ext() is None
    got = everything(cleared)
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    cleared.close()
    empty = icp.Context(0, **prm)
    empty.set_robust_ext(distance_type="point2point", scale_estimator=None, nb_iteration_for_scale=0)
    assert empty.get_robust_ext() == dict(distance_type=0, scale_estimator=-1, nb_iteration_for_scale=0)
    got = everything(empty)
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    empty.close()


# ---- (i) a held scale spares its selections ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("est", [1, 2], ids=["mad", "berg"])
def test_a_held_iteration_records_fewer_selections(est):
    rig = Rig(F32, icp.SUM_ORDER_SORTED)
    rd, T0 = ref.reading(2049), rig.sc["T_init"]

    def entries(nb, max_iters):
        rig.set_chain("cauchy", est, False, 1, nb, max_iters=max_iters)
        rig.ctx.profile_enable(True)
        rig.ctx.profile_reset()
        got = rig.align(rd, T0)
        n = rig.ctx.profile()["trim_select"]["launches"]
        rig.ctx.profile_enable(False)
        assert got["status"] == 0 and got["iterations"] == max_iters
        return n

    # nb = 2: iterations 1 and 2 estimate (berg: iteration 1 takes the median, iteration 2 only the recurrence), iteration 3 holds
    per_iteration = [entries(2, k) - entries(2, k - 1) if k > 1 else entries(2, 1) for k in (1, 2, 3, 4)]
    assert per_iteration[2] == per_iteration[3] < per_iteration[0], per_iteration
    if est == 1:
        assert per_iteration[0] == per_iteration[1] and per_iteration[2] == per_iteration[0] - 2, per_iteration     # the two medians
    else:
        assert per_iteration[1] == per_iteration[2] == per_iteration[0] - 1, per_iteration                             # the one median
    rig.close()
