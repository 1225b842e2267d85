"""A catalogue of self-contained calls through the C ABI, for tests/test_gpu_history.py.

A case is `run(ctx, aux) -> dict`: it sets the WHOLE chain itself, builds its maps, makes its calls, returns every output the
ABI defines for them, destroys its maps and leaves the filters off.  `aux` is a second long-lived context for the calls that
need one (the seeded probe's source, the builder of an adopted map).  Inputs come from pgslam_amd.synth and seeded numpy only.

What a call returns must be a function of its arguments, the context's parameters and the maps it names -- never of the calls
before it or of other contexts (include/pgicp.h, "Conventions").  The history tests run these cases in many orders and compare
every output with the case's baseline (a run on a fresh context pair) bit for bit: `compare` below.  Two documented exceptions:

  * pgicp_debug_last_matches ("lm." keys): "Kept pairs carry exact ids and distances"; for the rest the header allows -2 /
    an upper bound that "lies beyond the trim threshold".  Compared exactly on the kept pairs (distance <= trim_limit in the
    baseline), and the others only asserted to lie beyond trim_limit in both runs.
  * a seeded probe under PGICP_SUM_ORDER_SORTED ("seeded~" keys): the assertions of
    tests/test_gpu_parity.py::test_seeded_partial_chain_equals_the_unseeded_one -- the ratio the same double, the residual
    "the same sum in another order" (rel 1e-12).  Under PGICP_SUM_ORDER_SCAN: identical.

pgicp_debug_counters and the profile are not results and are left out.
"""
import functools
import os
import re

import numpy as np

from pgslam_amd import icp, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01,
             smooth_length=3, sensor_std_dev=0.01)
RESET = dict(knn=1, error_minimizer=0, bound_max_rot=0.0, bound_max_trans=0.0, normal_max_angle=0.0, outlier_max_dist=0.0,
             quantile_scale=1.0, robust_fct=0, robust_tuning=1.0, robust_scale=1, robust_approx=0.0)
WHOLE = dict(CHAIN, **RESET, epsilon=0.0, matcher=icp.MATCHER_GRID, grid_cell=0.0, sum_order=icp.SUM_ORDER_SORTED)
F32, F64 = np.float32, np.float64


def _csrc(name):
    return open(os.path.join(ROOT, "pgslam_amd", "csrc", name)).read()


def library_limits():
    """The two limits the outlier selection's path depends on, read from the sources (k_launch.inc launches what k_select.inc
    defines): the largest problem the one-launch selection takes, and the batch size the band path starts at."""
    src = _csrc("k_launch.inc")
    small_n = int(re.search(r'env_knob\("PGICP_SEL_SMALL_N",\s*(\d+)\)', src).group(1))
    band_p = int(re.search(r"constexpr\s+int\s+kSelBandMinProblems\s*=\s*(\d+)\s*;", src).group(1))
    return small_n, band_p


SEL_SMALL_N, SEL_BAND_MIN_P = library_limits()
BIG_N = SEL_SMALL_N + SEL_SMALL_N // 4              # a reading above the one-launch selection's limit


def set_chain(ctx, **over):
    """the whole chain: filters off first (a VarTrimmed filter refuses some chains), then every parameter"""
    ctx.set_var_trim()
    ctx.set_descriptor_filter(None)
    ctx.set_params(**dict(WHOLE, **over))


# ---- inputs (deterministic; built once per process) --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_scans():
    return synth.make_two_scans(6000, rings=16)


@functools.lru_cache(maxsize=None)
def s2m():
    return synth.make_scan_to_map(n_scan=6000, n_map=40_000, n_queries=3, n_map_poses=3, rings=16)


@functools.lru_cache(maxsize=None)
def s2m_big():
    return synth.make_scan_to_map(n_scan=BIG_N, n_map=150_000, n_queries=2, n_map_poses=3, rings=32)


@functools.lru_cache(maxsize=None)
def far_scene():
    """a scan taken metres ahead of a short-range map (tests/test_gpu_matcher_state.py::test_scan_ahead_of_its_map)"""
    world = synth.make_world()
    poses = [synth.se3(x=-40.0 + 2.0 * k) for k in range(3)]
    ref_inv = synth.se3_inv(poses[0])
    parts = []
    for k, P in enumerate(poses):
        x, n = synth.make_scan(world, P, 8000, 9100 + k, rings=16, max_range=14.0)
        parts.append(synth.transform_cloud(ref_inv @ P, x.astype(np.float64), n.astype(np.float64)))
    ref = np.concatenate([p[0] for p in parts]).astype(np.float32)
    nrm = np.concatenate([p[1] for p in parts]).astype(np.float32)
    P = synth.se3(x=-36.0 + 6.0, y=0.3, yaw=np.deg2rad(2.0))
    rd, _ = synth.make_scan(world, P, 9000, 9206, rings=16, max_range=14.0)
    T0 = ref_inv @ P @ synth.se3(x=0.05, y=-0.04, yaw=np.deg2rad(0.4))
    return ref, nrm, rd, T0


@functools.lru_cache(maxsize=None)
def plane_cloud(n, seed, extent, shape=(1.0, 1.0, 1.0), tilt=0.0):
    """n points on three noisy faces of a box of `extent` x `shape` metres, with their normals (seeded numpy)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 3, n)
    uv = rng.uniform(0.0, 1.0, (n, 2))
    noise = rng.normal(0.0, 0.01, n)
    xyz = np.zeros((n, 3))
    nrm = np.zeros((n, 3))
    for a in range(3):
        m = k == a
        b, c = (a + 1) % 3, (a + 2) % 3
        xyz[m, a] = noise[m] + tilt * uv[m, 0]
        xyz[m, b], xyz[m, c] = uv[m, 0] * extent * shape[b], uv[m, 1] * extent * shape[c]
        nrm[m, a] = 1.0
    return xyz.astype(np.float32), nrm.astype(np.float32)


def batch_problem_set(P, big, dense=False):
    """P ragged problems against one map: (map_xyz, map_nrm, readings, T_inits).  Sizes from 50 points to the largest; `dense`:
    no reading below a third of the largest (a sliver of a scan has a threshold floor of its own)."""
    w = s2m_big() if big else s2m()
    top = len(w.scans_xyz[0])
    sizes = [top, top - 1234, 50, top // 2 + 1, 2049, top - 7, 777, top // 3][:P]
    if dense:
        sizes = [top, top - 1234, top // 3, top // 2 + 1, top - 5000, top - 7, top // 2 + 999, top // 3 + 17][:P]
    rds, T0 = [], []
    for p in range(P):
        q = p % len(w.scans_xyz)
        full = w.scans_xyz[q]
        # (a small reading is a strided sample of the whole scan, not a sliver of it: a sliver constrains no pose)
        rds.append(np.ascontiguousarray(full[:sizes[p]] if sizes[p] * 3 >= top else full[:: len(full) // sizes[p]][:sizes[p]]))
        T0.append(w.T_init[q] @ synth.se3(x=0.01 * p, yaw=0.001 * p))
    return w.map_xyz, w.map_nrm, rds, T0


# ---- outputs -----------------------------------------------------------------------------------------------------------------
STAT_FIELDS = ("status", "iterations", "converged", "max_iter_reached", "overlap", "residual", "trim_limit", "n_kept", "n_finite", "cov")


def put_stats(out, key, st):
    for f in STAT_FIELDS:
        v = st[f]
        out[f"{key}.{f}"] = np.array(v, dtype=np.float64) if f in ("overlap", "residual", "trim_limit", "cov") else int(v)


def put_last_matches(out, key, ctx, n, problem, dtype, limit):
    ids, d2 = ctx.debug_last_matches(n, problem=problem, dtype=dtype)
    out[f"lm.{key}.ids"], out[f"lm.{key}.d2"], out[f"lm.{key}.limit"] = ids, d2, np.array(limit, dtype=np.float64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def compare(base, got, sum_order_sorted=True):
    """the list of differences between a baseline and another run of the same case (empty: the same everywhere)"""
    bad = []
    if sorted(base) != sorted(got):
        return [f"keys differ: {sorted(set(base) ^ set(got))}"]
    for k in base:
        a, b = base[k], got[k]
        if k.startswith("lm."):
            if k.endswith(".ids"):
                stem = k[:-4]
                lim = float(base[stem + ".limit"])
                da, db = base[stem + ".d2"], got[stem + ".d2"]
                kept = da <= lim                       # (the header: "Kept pairs carry exact ids and distances")
                if not (np.array_equal(a[kept], b[kept]) and da[kept].tobytes() == db[kept].tobytes()):
                    bad.append(f"{stem}: kept pairs differ ({int((a[kept] != b[kept]).sum())} ids)")
                if not (np.all(da[~kept] > lim) and np.all(db[~kept] > lim)):      # ("... an upper bound and lies beyond the trim threshold")
                    bad.append(f"{stem}: a pair that is not kept lies inside the threshold")
                if not np.array_equal(np.isfinite(da), np.isfinite(db)):
                    bad.append(f"{stem}: 'has a neighbour within maxDist' differs")
            elif k.endswith(".limit") and not same_bits(a, b):
                bad.append(f"{k}: {a!r} != {b!r}")
            continue
        if k.startswith("seeded~") and sum_order_sorted:
            # the header on pgicp_partial_chain_seeded: "with PGICP_SUM_ORDER_SORTED the residual is the same sum in another order
            # (equal to ~1e-16 relative; identical with PGICP_SUM_ORDER_SCAN)"; the existing test's bound is rel 1e-12
            if not abs(float(a) - float(b)) <= 1e-12 * abs(float(a)):
                bad.append(f"{k}: {a!r} != {b!r} (rel 1e-12)")
            continue
        if isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer)):
            if int(a) != int(b):
                bad.append(f"{k}: {a} != {b}")
        elif not same_bits(a, b):
            aa, bb = np.asarray(a), np.asarray(b)
            where = ""
            if aa.shape == bb.shape and aa.size:
                neq = np.flatnonzero(aa.ravel() != bb.ravel())
                where = f" first at {neq[:4].tolist()} of {aa.size}: {aa.ravel()[neq[:2]]} vs {bb.ravel()[neq[:2]]}"
            bad.append(f"{k}: differs{where}")
    return bad


# ---- the cases -----------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, run, api, size="small", oracle=None, error=False):
        self.name, self.run, self.api, self.size, self.oracle, self.error = name, run, tuple(api), size, oracle, error


CASES = {}


def case(name, api, size="small", oracle=None, error=False, dtypes=(None,)):
    """registers run(ctx, aux[, dtype]); with `dtypes` one case per precision, `api` names then get the _f32 / _f64 suffix"""
    def deco(fn):
        for dt in dtypes:
            if dt is None:
                CASES[name] = Case(name, fn, api, size, oracle, error)
            else:
                sfx = "_f32" if dt == F32 else "_f64"
                full = name + sfx
                names = [a[:-1] + sfx if a.endswith("*") else a for a in api]
                CASES[full] = Case(full, functools.partial(fn, dtype=dt), names, size,
                                   functools.partial(oracle, dtype=dt) if oracle else None, error)
        return fn
    return deco


def _orc(oracles, dtype):
    return oracles[0] if dtype == F32 else oracles[1]


_ICP_RUNS = {}


def _stats_of(out, key):
    st = {f: out[f"{key}.{f}"] for f in STAT_FIELDS}
    st["converged"] = bool(st["converged"])
    st["overlap"], st["residual"], st["trim_limit"] = float(st["overlap"]), float(st["residual"]), float(st["trim_limit"])
    return st


def _check_icp(out, key, orc, rd, ref, nrm, T0, chain, sorted_order=True, share=None):
    """tests/test_gpu_bit_exact.py::check on a recorded ICP: the oracle adds the pairs in the order the call reports.
    share: a key under which the oracle's run is kept (the same problem appears in several batches, in the same order)."""
    from test_gpu_bit_exact import check
    order = out[f"{key}.order"] if sorted_order else None
    tag = None if share is None else (share, None if order is None else order.tobytes())
    if tag is None or tag not in _ICP_RUNS:
        o = orc.icp(rd, ref, nrm, T0, pair_order=order, **chain)
        if tag is not None:
            _ICP_RUNS[tag] = o
    else:
        o = _ICP_RUNS[tag]
    check(_stats_of(out, key), out[f"{key}.T"], o, key)
    return o


def _check_state(out, key, o, dtype):
    """The assertions of tests/test_gpu_matcher_state.py::check_state on a recorded call (its last matches under "lm."): rtol 0
    for the float chain, 1e-11 for the double chain, as the tests there use them."""
    import pytest
    rtol = 0.0 if dtype == F32 else 1e-11
    gi, gd = out[f"lm.{key}.ids"], out[f"lm.{key}.d2"]
    st = _stats_of(out, key)
    assert st["iterations"] == o["iterations"]
    assert st["n_finite"] == o["n_finite"] and st["n_kept"] == o["n_kept"]
    np.testing.assert_array_equal(np.isfinite(gd), np.isfinite(o["last_d2"]))
    kept = o["last_d2"] <= o["trim_limit"]
    np.testing.assert_array_equal(gi[kept], o["last_ids"][kept])
    if rtol == 0.0:
        assert st["trim_limit"] == o["trim_limit"]
        np.testing.assert_array_equal(gd[kept], o["last_d2"][kept])
    else:
        assert st["trim_limit"] == pytest.approx(o["trim_limit"], rel=rtol)
        np.testing.assert_allclose(gd[kept], o["last_d2"][kept], rtol=rtol, atol=1e-18)
    loose = np.isfinite(gd) & ~kept
    assert np.all(gd[loose] >= o["last_d2"][loose] * (1 - rtol)) and np.all(gd[loose] > o["trim_limit"] * (1 - rtol))


def _check_chain(ratio, resid, orc, rd, ref, nrm, T, what):
    """the partial chain against the oracle's (tests/test_gpu_chain.py, tests/test_gpu_parity.py: ratio 1e-12, residual 1e-6)"""
    import pytest
    po = orc.partial_chain(rd, ref, nrm, T, **dict(CHAIN, center_reference=False))
    assert po["status"] == 0, what
    assert float(ratio) == pytest.approx(po["overlap"], rel=1e-12), (what, ratio, po["overlap"])
    assert float(resid) == pytest.approx(po["residual"], rel=1e-6), (what, resid, po["residual"])


# -- align -------------------------------------------------------------------------------------------------------------------------
def _align_oracle(out, oracles, dtype, sum_order=icp.SUM_ORDER_SORTED):
    s = two_scans()
    _check_icp(out, "a", _orc(oracles, dtype), s["reading_xyz"].astype(dtype), s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype),
               s["T_init"], CHAIN, sum_order == icp.SUM_ORDER_SORTED)


@case("align", ["pgicp_map_create*", "pgicp_align*", "pgicp_debug_last_matches*", "pgicp_debug_reading_order", "pgicp_map_destroy",
                "pgicp_set_params", "pgicp_set_var_trim", "pgicp_set_descriptor_filter"], oracle=_align_oracle, dtypes=(F32, F64))
def run_align(ctx, aux, dtype, sum_order=icp.SUM_ORDER_SORTED):
    s = two_scans()
    set_chain(ctx, sum_order=sum_order)
    rd = s["reading_xyz"].astype(dtype)
    mid = ctx.set_map(s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), center=True, dtype=dtype)
    T, st = ctx.align(mid, rd, s["T_init"], dtype=dtype)
    out = {"a.T": T, "a.order": ctx.reading_order(len(rd))}
    put_stats(out, "a", st)
    put_last_matches(out, "a", ctx, len(rd), 0, dtype, st["trim_limit"])
    ctx.destroy_map(mid)
    set_chain(ctx)
    return out


@case("align_scan_order", ["pgicp_map_create*", "pgicp_align*"], oracle=functools.partial(_align_oracle, sum_order=icp.SUM_ORDER_SCAN), dtypes=(F32, F64))
def run_align_scan(ctx, aux, dtype):
    return run_align(ctx, aux, dtype, sum_order=icp.SUM_ORDER_SCAN)


# -- batches -----------------------------------------------------------------------------------------------------------------------
def run_batch(ctx, aux, P, big, dtype, T_scale=None, order=None, kind="align", residual=False, var_trim=None, max_iters=30, dense=False, chain=()):
    """P ragged problems in one call.  T_scale: the initial error made `T_scale` times as large (for the hostile hint pairs);
    order: a permutation of the problems; chain: ((parameter, value), ...) on top of the whole chain."""
    mx, mn, rds, T0 = batch_problem_set(P, big, dense)
    if T_scale is not None:
        w = s2m_big() if big else s2m()
        T0 = [w.T_truth[p % len(w.T_truth)] @ _scaled(np.linalg.inv(w.T_truth[p % len(w.T_truth)]) @ T0[p], T_scale) for p in range(P)]
    if order is not None:
        rds, T0 = [rds[k] for k in order], [T0[k] for k in order]
    rds = [r.astype(dtype) for r in rds]
    set_chain(ctx, max_iters=max_iters, **dict(chain))
    if var_trim:
        ctx.set_var_trim(*var_trim)
    out = {}
    if kind == "align":
        mid = ctx.set_map(mx.astype(dtype), mn.astype(dtype), center=True, dtype=dtype)
        if residual:
            T, sts, res, ratio, rst = ctx.align_residual_batch([mid] * P, rds, T0, dtype=dtype)
            out.update({"res": res, "ratio": ratio, "rstatus": rst})
        else:
            T, sts = ctx.align_batch([mid] * P, rds, T0, dtype=dtype, raise_on_error=False)
        out["T"] = T
        for p in range(P):
            put_stats(out, f"p{p}", sts[p])
            out[f"p{p}.T"] = T[p]
            if not residual:
                out[f"p{p}.order"] = ctx.reading_order(len(rds[p]), problem=p)
                put_last_matches(out, f"p{p}", ctx, len(rds[p]), p, dtype, sts[p]["trim_limit"])
    else:
        mid = ctx.set_map(mx.astype(dtype), mn.astype(dtype), center=False, dtype=dtype)
        ratio, resid, status = ctx.partial_chain_batch([mid] * P, rds, T0, dtype=dtype, raise_on_error=False)
        out.update({"ratio": ratio, "resid": resid, "status": status})
    if var_trim:
        out["vt_ratio"] = np.array([ctx.last_var_trim_ratio(p) for p in range(P)])
    ctx.destroy_map(mid)
    set_chain(ctx)
    return out


def _scaled(dT, s):
    """the perturbation dT with its translation and its (small) rotation angles scaled by s"""
    R = dT[:3, :3]
    yaw, pitch, roll = np.arctan2(R[1, 0], R[0, 0]), -np.arcsin(max(-1.0, min(1.0, R[2, 0]))), np.arctan2(R[2, 1], R[2, 2])
    t = dT[:3, 3] * s
    return synth.se3(t[0], t[1], t[2], yaw * s, pitch * s, roll * s)


def _batch_oracle(out, oracles, P, big, dtype, kind="align"):
    mx, mn, rds, T0 = batch_problem_set(P, big)
    orc = _orc(oracles, dtype)
    for p in range(P):
        if kind == "align":             # (problem p is the same in every batch that holds it: one oracle run serves them all)
            _check_icp(out, f"p{p}", orc, rds[p].astype(dtype), mx.astype(dtype), mn.astype(dtype), T0[p], CHAIN,
                       share=("batch", big, np.dtype(dtype).name, p))
        else:
            assert out["status"][p] == 0
            _check_chain(out["ratio"][p], out["resid"][p], orc, rds[p].astype(dtype), mx.astype(dtype), mn.astype(dtype), T0[p], p)


def _residual_oracle(out, oracles, dtype):
    """tests/test_gpu_parity.py: "the ICPs are those of pgicp_align_batch, bit for bit" (that case is checked against the oracle),
    and the fused residual pass against the oracle's partial chain at the result (residual 1e-3, ratio 1e-9)"""
    import pytest
    sfx = "_f32" if dtype == F32 else "_f64"
    ab = oracles[2]("align_batch_3" + sfx)
    mx, mn, rds, T0 = batch_problem_set(3, False)
    for k in out:
        if k.startswith("p") or k == "T":
            assert same_bits(out[k], ab[k]) if isinstance(out[k], np.ndarray) else out[k] == ab[k], k
    for p in range(3):
        assert out["rstatus"][p] == 0
        po = _orc(oracles, dtype).partial_chain(rds[p].astype(dtype), mx.astype(dtype), mn.astype(dtype), out["T"][p], **CHAIN)
        assert out["res"][p] == pytest.approx(po["residual"], rel=1e-3) and out["ratio"][p] == pytest.approx(po["overlap"], rel=1e-9), p


def _var_trim_batch_oracle(out, oracles):
    """tests/test_gpu_var_trim.py::_check_last_iteration on every problem's recorded last iteration"""
    from var_trim_ref import var_trim
    for p in range(3):
        ids, d2 = out[f"lm.p{p}.ids"], out[f"lm.p{p}.d2"]
        assert (ids >= -1).all()
        ref = var_trim(d2, 0.3, 0.95, 2.0, F32)
        assert ref["gap"] > 1e-12
        assert float(out["vt_ratio"][p]) == ref["tuned"], (p, out["vt_ratio"][p], ref["tuned"])
        assert same_bits(np.float64(out[f"p{p}.trim_limit"]), np.float64(ref["limit"])), p
        assert out[f"p{p}.n_kept"] == int(ref["weights"].sum()) and out[f"p{p}.n_finite"] == ref["n_finite"], p


BATCH_P = (1, 3, 4, 8)
for _P in BATCH_P:
    for _big in (False, True):
        for _dt in (F32, F64):
            if _big and _dt == F64 and _P not in (1, 4):
                continue                        # (f64 above the limit: one batch on each side of the band path's problem count)
            _sfx = "_f32" if _dt == F32 else "_f64"
            _tag = f"{_P}{'big' if _big else ''}{_sfx}"
            _orc_fn = functools.partial(_batch_oracle, P=_P, big=_big, dtype=_dt)
            CASES[f"align_batch_{_tag}"] = Case(f"align_batch_{_tag}", functools.partial(run_batch, P=_P, big=_big, dtype=_dt),
                                                ["pgicp_align_batch" + _sfx, "pgicp_map_create" + _sfx, "pgicp_debug_last_matches" + _sfx],
                                                "large" if _big else "small", _orc_fn)
            if not _big or _P == 4:
                CASES[f"partial_chain_batch_{_tag}"] = Case(f"partial_chain_batch_{_tag}", functools.partial(run_batch, P=_P, big=_big, dtype=_dt, kind="chain"),
                                                            ["pgicp_partial_chain_batch" + _sfx], "large" if _big else "small",
                                                            functools.partial(_batch_oracle, P=_P, big=_big, dtype=_dt, kind="chain"))
for _dt in (F32, F64):
    _sfx = "_f32" if _dt == F32 else "_f64"
    CASES["align_residual_batch" + _sfx] = Case("align_residual_batch" + _sfx, functools.partial(run_batch, P=3, big=False, dtype=_dt, residual=True),
                                                ["pgicp_align_residual_batch" + _sfx], "small", functools.partial(_residual_oracle, dtype=_dt))
CASES["align_batch_var_trim_f32"] = Case("align_batch_var_trim_f32", functools.partial(run_batch, P=3, big=False, dtype=F32, var_trim=(0.3, 0.95, 2.0)),
                                         ["pgicp_align_batch_f32", "pgicp_set_var_trim", "pgicp_last_var_trim_ratio"], "small", _var_trim_batch_oracle)


# -- icp_pair ------------------------------------------------------------------------------------------------------------------------
def _pair_oracle(out, oracles, dtype):
    s = two_scans()
    _check_icp(out, "a", _orc(oracles, dtype), s["reading_xyz"][:5000].astype(dtype), s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype),
               s["T_init"], CHAIN)


@case("icp_pair", ["pgicp_icp_pair*"], oracle=_pair_oracle, dtypes=(F32, F64))
def run_icp_pair(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    rd = s["reading_xyz"][:5000].astype(dtype)
    T, st = ctx.icp_pair(rd, s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), s["T_init"], dtype=dtype)
    out = {"a.T": T, "a.order": ctx.reading_order(len(rd))}
    put_stats(out, "a", st)
    return out


# -- stages --------------------------------------------------------------------------------------------------------------------------
def _match_oracle(out, oracles, dtype, knn, matcher):
    w = s2m()                                    # (tests/test_gpu_chain.py::test_match_knn_bit_exact, tests/test_gpu_topk.py for the double oracle)
    o = _orc(oracles, dtype)
    q = o.transform(w.T_init[0], w.scans_xyz[0].astype(dtype))
    oid, od2 = o.knn_k(w.map_xyz.astype(dtype), q, knn, 2.0)
    ids, d2 = out["ids"].reshape(len(q), knn), out["d2"].reshape(len(q), knn)
    bits = np.uint32 if dtype == F32 else np.uint64
    assert np.array_equal(ids, oid)
    assert np.array_equal(d2.view(bits), od2.view(bits))


def run_match(ctx, aux, dtype, knn, matcher):
    w = s2m()
    set_chain(ctx, knn=knn, matcher=matcher)
    mid = ctx.set_map(w.map_xyz.astype(dtype), None, center=False, dtype=dtype)
    ids, d2 = ctx.match(mid, w.scans_xyz[0].astype(dtype), T=w.T_init[0], dtype=dtype)
    ctx.destroy_map(mid)
    set_chain(ctx)
    return {"ids": ids, "d2": d2}


for _dt in (F32, F64):
    for _knn, _m in ((1, icp.MATCHER_GRID), (3, icp.MATCHER_GRID), (1, icp.MATCHER_BRUTE), (5, icp.MATCHER_BRUTE)):
        _sfx = "_f32" if _dt == F32 else "_f64"
        _n = f"match_knn{_knn}_{'grid' if _m == icp.MATCHER_GRID else 'brute'}{_sfx}"
        CASES[_n] = Case(_n, functools.partial(run_match, dtype=_dt, knn=_knn, matcher=_m), ["pgicp_match" + _sfx, "pgicp_map_create" + _sfx],
                         "small", functools.partial(_match_oracle, dtype=_dt, knn=_knn, matcher=_m))


def _distances(dtype):
    rng = np.random.default_rng(77)
    d2 = (rng.gamma(1.5, 0.02, size=5001) ** 2).astype(dtype)
    d2[rng.integers(0, d2.size, 40)] = np.inf
    d2[rng.integers(0, d2.size, 25)] = 0.0
    return d2


def _weights_oracle(out, oracles, dtype, kind):
    d2 = _distances(dtype)
    bits = np.uint32 if dtype == F32 else np.uint64
    o = _orc(oracles, dtype)
    if kind == "trimmed":
        st, w, limit, nf = o.trim_weights(d2, 0.85)
        assert st == 0 and np.array_equal(out["w"].view(bits), np.asarray(w, dtype=dtype).view(bits)) and out["nf"] == nf
        assert dtype(out["limit"]) == dtype(limit)
    elif kind == "robust":
        ow, _ = o.robust_weights(d2, 1, 1.0, 1, 0.0)
        assert np.array_equal(out["w"].view(bits), ow.view(bits))
    else:
        from var_trim_ref import var_trim
        r = var_trim(d2, 0.3, 0.95, 2.0, dtype)
        assert np.array_equal(out["w"].view(bits), r["weights"].astype(dtype).view(bits))
        assert dtype(out["limit"]) == dtype(r["limit"]) and out["nf"] == r["n_finite"]
        assert float(out["vt_ratio"]) == r["tuned"]


def run_weights(ctx, aux, dtype, kind):
    set_chain(ctx, **(dict(trim_ratio=1.0, robust_fct=1, robust_tuning=1.0, robust_scale=1) if kind == "robust" else {}))
    if kind == "var_trim":
        ctx.set_var_trim(0.3, 0.95, 2.0)
    w, limit, nf = ctx.outlier_weights(_distances(dtype))
    out = {"w": w, "limit": np.array(limit, dtype=np.float64), "nf": nf}
    if kind == "var_trim":
        out["vt_ratio"] = np.array(ctx.last_var_trim_ratio(0))
    set_chain(ctx)
    return out


for _dt in (F32, F64):
    for _kind in ("trimmed", "robust", "var_trim"):
        _sfx = "_f32" if _dt == F32 else "_f64"
        CASES[f"outlier_weights_{_kind}{_sfx}"] = Case(f"outlier_weights_{_kind}{_sfx}", functools.partial(run_weights, dtype=_dt, kind=_kind),
                                                       ["pgicp_outlier_weights" + _sfx] + (["pgicp_last_var_trim_ratio"] if _kind == "var_trim" else []),
                                                       "small", functools.partial(_weights_oracle, dtype=_dt, kind=_kind))


def _error_stats_oracle(out, oracles, dtype):
    from test_gpu_bit_exact import same_bits as sb
    s = two_scans()
    o = _orc(oracles, dtype)
    rd = out["rd"]
    assert same_bits(rd, o.transform(s["T_init"], s["reading_xyz"].astype(dtype)))
    mean = o.centroid(s["ref_xyz"].astype(dtype))
    st, sys_ = o.p2plane_system(rd - mean, s["ref_xyz"].astype(dtype) - mean, s["ref_nrm"].astype(dtype), out["ids"], out["w"])
    assert st == 0 and sb(out["sys"], sys_) and sb(out["resid"], sys_[29]) and sb(out["ratio"], sys_[27] / len(rd))


@case("error_stats", ["pgicp_error_stats*", "pgicp_match*", "pgicp_outlier_weights*"], oracle=_error_stats_oracle, dtypes=(F32, F64))
def run_error_stats(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    mid = ctx.set_map(s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), center=True, dtype=dtype)
    rd = ctx.transform(s["T_init"], s["reading_xyz"].astype(dtype), dtype=dtype)
    ids, d2 = ctx.match(mid, rd, dtype=dtype)
    w, limit, nf = ctx.outlier_weights(d2)
    ratio, resid, sys_ = ctx.error_stats(mid, rd, ids, w, dtype=dtype)
    ctx.destroy_map(mid)
    return {"rd": rd, "ids": ids, "d2": d2, "w": w, "limit": np.array(limit), "nf": nf, "ratio": np.array(ratio), "resid": np.array(resid), "sys": sys_}


def _chain_oracle(out, oracles, dtype):
    import pytest
    s = two_scans()
    po = _orc(oracles, dtype).partial_chain(s["reading_xyz"].astype(dtype), s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), s["T_truth"],
                                            **dict(CHAIN, center_reference=False))
    assert float(out["ratio"]) == pytest.approx(po["overlap"], rel=1e-12) and float(out["resid"]) == pytest.approx(po["residual"], rel=1e-6)


@case("partial_chain", ["pgicp_partial_chain*"], oracle=_chain_oracle, dtypes=(F32, F64))
def run_partial_chain(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    rd = s["reading_xyz"].astype(dtype)
    mid = ctx.set_map(s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), center=False, dtype=dtype)
    ratio, resid = ctx.partial_chain(mid, rd, T=s["T_truth"], dtype=dtype)
    out = {"ratio": np.array(ratio), "resid": np.array(resid), "order": ctx.reading_order(len(rd))}
    ctx.destroy_map(mid)
    return out


@functools.lru_cache(maxsize=None)
def probe_scene():
    """the overlap probe of tests/test_gpu_parity.py::test_seeded_partial_chain_equals_the_unseeded_one, at a smaller size"""
    world = synth.make_world()
    poses = [synth.se3(x=-6.0 + 1.5 * k, yaw=np.deg2rad(1.5 * (k % 3 - 1))) for k in range(5)]
    kf = [synth.make_scan(world, poses[k], 6000, 7100 + k, rings=16) for k in range(4)]
    ref_pose = poses[2]

    def assemble(order):
        xs, ns = [], []
        for k in order:
            x, n = synth.transform_cloud(synth.se3_inv(ref_pose) @ poses[k], kf[k][0], kf[k][1])
            xs.append(x); ns.append(n)
        return np.concatenate(xs).astype(np.float32), np.concatenate(ns).astype(np.float32), [len(x) for x in xs]
    order_a, order_b = [2, 1, 0], [2, 3, 1]
    xa, na, sizes_a = assemble(order_a)
    xb, nb, sizes_b = assemble(order_b)
    scan, _ = synth.make_scan(world, poses[4] @ synth.se3(x=-2.0), 5000, 7200, rings=16)
    T0 = synth.se3_inv(ref_pose) @ poses[4] @ synth.se3(x=-2.0) @ synth.perturbation(41)
    start_a = np.concatenate([[0], np.cumsum(sizes_a)])
    start_b = np.concatenate([[0], np.cumsum(sizes_b)])
    dst = [int(start_b[order_b.index(k)]) if k in order_b else -1 for k in order_a]
    return xa, na, xb, nb, scan.astype(np.float32), T0, start_a, dst


def _seeded_oracle(out, oracles, dtype, sum_order=icp.SUM_ORDER_SORTED, pre=""):
    import pytest
    xa, na, xb, nb, scan, T0, start_a, dst = probe_scene()
    o = _orc(oracles, dtype)
    _check_icp(out, "a", o, scan.astype(dtype), xa.astype(dtype), na.astype(dtype), T0, CHAIN, sum_order == icp.SUM_ORDER_SORTED)
    T = out["a.T"]
    T_off = T @ synth.se3(x=0.4, yaw=np.deg2rad(1.0))
    for key, at in (("plain", T), ("plain_off", T_off)):
        _check_chain(out[key + ".ratio"], out[key + ".resid"], o, scan.astype(dtype), xb.astype(dtype), nb.astype(dtype), at, key)
    # (tests/test_gpu_parity.py: the seeded probe's ratio against the oracle's)
    po = o.partial_chain(scan.astype(dtype), xb.astype(dtype), nb.astype(dtype), T, **dict(CHAIN, center_reference=False))
    assert float(out["seeded.ratio"]) == pytest.approx(po["overlap"], rel=1e-12)


@case("partial_chain_seeded", ["pgicp_partial_chain_seeded*", "pgicp_align*", "pgicp_partial_chain*"], size="medium", oracle=_seeded_oracle, dtypes=(F32, F64))
def run_seeded(ctx, aux, dtype, sum_order=icp.SUM_ORDER_SORTED, first="plain"):
    """first: which probe the case STARTS with -- "plain" (the unseeded probe at the result), or "seeded" / "seeded_off" (a seeded
    probe whose cap comes from whatever probe the context made before this case)"""
    xa, na, xb, nb, scan, T0, start_a, dst = probe_scene()
    scan = scan.astype(dtype)
    set_chain(aux, sum_order=sum_order)
    set_chain(ctx, sum_order=sum_order)
    ma = aux.set_map(xa.astype(dtype), na.astype(dtype), center=True, dtype=dtype)
    mb = ctx.set_map(xb.astype(dtype), nb.astype(dtype), center=False, dtype=dtype)
    T, st = aux.align(ma, scan, T0, dtype=dtype)
    out = {"a.T": T, "a.order": aux.reading_order(len(scan))}
    put_stats(out, "a", st)
    T_off = T @ synth.se3(x=0.4, yaw=np.deg2rad(1.0))
    early = {}
    if first == "seeded":
        early["seeded"] = ctx.partial_chain_seeded(mb, scan, T, aux, start_a, dst, dtype=dtype)
    elif first == "seeded_off":
        early["seeded_off"] = ctx.partial_chain_seeded(mb, scan, T_off, aux, start_a, dst, dtype=dtype)
    plain = ctx.partial_chain(mb, scan, T=T, dtype=dtype)
    seeded = early.get("seeded") or ctx.partial_chain_seeded(mb, scan, T, aux, start_a, dst, dtype=dtype)
    seeded_off = early.get("seeded_off") or ctx.partial_chain_seeded(mb, scan, T_off, aux, start_a, dst, dtype=dtype)   # (capped by the probe before it)
    lying = ctx.partial_chain_seeded(mb, scan, T, aux, start_a, [5, 777, 31], dtype=dtype)
    plain_off = ctx.partial_chain(mb, scan, T=T_off, dtype=dtype)
    out.update({"plain.ratio": np.array(plain[0]), "plain.resid": np.array(plain[1]),
                "plain_off.ratio": np.array(plain_off[0]), "plain_off.resid": np.array(plain_off[1]),
                "seeded.ratio": np.array(seeded[0]), "seeded~resid": np.array(seeded[1]),
                "seeded_off.ratio": np.array(seeded_off[0]), "seeded~off_resid": np.array(seeded_off[1]),
                "lying.ratio": np.array(lying[0]), "seeded~lying_resid": np.array(lying[1])})
    # inside one run: a seed is a candidate only (the existing test's `same`)
    assert seeded[0] == plain[0] and abs(seeded[1] - plain[1]) <= 1e-12 * abs(plain[1]), (seeded, plain)
    assert lying[0] == plain[0] and abs(lying[1] - plain[1]) <= 1e-12 * abs(plain[1]), (lying, plain)
    # a cap that is far too small (the probe before sat on the map, this one is 40 cm off) costs time, never a result
    assert seeded_off[0] == plain_off[0] and abs(seeded_off[1] - plain_off[1]) <= 1e-12 * abs(plain_off[1]), (seeded_off, plain_off)
    if sum_order == icp.SUM_ORDER_SCAN:
        assert seeded == plain and lying == plain and seeded_off == plain_off, (seeded, lying, plain, seeded_off, plain_off)
    aux.destroy_map(ma)
    ctx.destroy_map(mb)
    set_chain(aux)
    set_chain(ctx)
    return out


def _seeded_scan_oracle(out, oracles, dtype):
    _seeded_oracle(out, oracles, dtype, sum_order=icp.SUM_ORDER_SCAN)


@case("partial_chain_seeded_scan_order", ["pgicp_partial_chain_seeded*"], size="medium", oracle=_seeded_scan_oracle, dtypes=(F32,))
def run_seeded_scan(ctx, aux, dtype, first="plain"):
    out = run_seeded(ctx, aux, dtype, sum_order=icp.SUM_ORDER_SCAN, first=first)
    return {k.replace("seeded~", "seeded_scan."): v for k, v in out.items()}       # (scan order: identical, no exception)


# -- transform, local map --------------------------------------------------------------------------------------------------------------
def _transform_oracle(out, oracles, dtype):
    s = two_scans()
    o = _orc(oracles, dtype)
    T = s["T_init"]
    assert same_bits(out["pts"], o.transform(T, s["reading_xyz"].astype(dtype)))
    assert same_bits(out["nrm"], o.transform(T, s["reading_nrm"].astype(dtype), rotate_only=True))


@case("transform", ["pgicp_transform*"], oracle=_transform_oracle, dtypes=(F32, F64))
def run_transform(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    return {"pts": ctx.transform(s["T_init"], s["reading_xyz"].astype(dtype), dtype=dtype),
            "nrm": ctx.transform(s["T_init"], s["reading_nrm"].astype(dtype), rotate_only=True, dtype=dtype)}


def _local_map_inputs(dtype):
    xa, na, xb, nb, scan, T0, start_a, dst = probe_scene()
    cx = [np.ascontiguousarray(xa[start_a[k]:start_a[k + 1]].astype(dtype)) for k in range(3)]
    cn = [np.ascontiguousarray(na[start_a[k]:start_a[k + 1]].astype(dtype)) for k in range(3)]
    Ts = [np.eye(4), synth.se3(x=1.5, yaw=0.02), synth.se3(x=-1.0, y=0.3, yaw=-0.03)]
    return cx, cn, Ts


def _local_map_oracle(out, oracles, dtype):
    cx, cn, Ts = _local_map_inputs(dtype)
    ox, on = _orc(oracles, dtype).build_local_map(cx, cn, Ts)
    assert same_bits(out["xyz"], np.asarray(ox, dtype=dtype)) and same_bits(out["nrm"], np.asarray(on, dtype=dtype))


@case("build_local_map_host", ["pgicp_build_local_map*"], oracle=_local_map_oracle, dtypes=(F32, F64))
def run_local_map_host(ctx, aux, dtype):
    cx, cn, Ts = _local_map_inputs(dtype)
    set_chain(ctx)
    x, n = ctx.build_local_map(cx, cn, Ts, dtype=dtype)
    return {"xyz": x, "nrm": n}


@case("build_local_map_device", ["pgicp_build_local_map*", "pgicp_map_create*", "pgicp_align*"], oracle=_local_map_oracle, dtypes=(F32, F64))
def run_local_map_device(ctx, aux, dtype):
    """device keyframes -> device map cloud -> indexed without crossing PCIe -> an align against it"""
    cx, cn, Ts = _local_map_inputs(dtype)
    xa, na, xb, nb, scan, T0, start_a, dst = probe_scene()
    set_chain(ctx)
    dx = [ctx.device_cloud(c, dtype) for c in cx]
    dn = [ctx.device_cloud(c, dtype) for c in cn]
    ox, on = ctx.build_local_map(dx, dn, Ts, dtype=dtype)
    out = {"xyz": np.ascontiguousarray(ctx.device_download(ox)), "nrm": np.ascontiguousarray(ctx.device_download(on))}
    mid = ctx.set_map(ox, on, center=True, dtype=dtype)
    T, st = ctx.align(mid, scan.astype(dtype), T0, dtype=dtype)
    out["a.T"] = T
    put_stats(out, "a", st)
    ctx.destroy_map(mid)
    for d in dx + dn + [ox, on]:
        ctx.device_free(d)
    return out


# -- input filters -----------------------------------------------------------------------------------------------------------------------
def _normals_oracle(out, oracles, dtype):
    s = two_scans()
    r = _orc(oracles, dtype).surface_normals(s["ref_xyz"][:4000].astype(dtype), 10)
    assert np.array_equal(out["ids"], r["ids"]) and same_bits(out["d2"], r["d2"])


@case("surface_normals", ["pgicp_surface_normals*"], oracle=_normals_oracle, dtypes=(F32, F64))
def run_surface_normals(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    nrm, eig, ids, d2 = ctx.surface_normals(s["ref_xyz"][:4000].astype(dtype), knn=10, dtype=dtype, want_eigen=True, want_ids=True)
    return {"nrm": nrm, "eig": eig, "ids": ids, "d2": d2}


def _ssn_oracle(out, oracles, dtype):
    s = two_scans()
    r = _orc(oracles, dtype).sampling_surface_normal(s["ref_xyz"].astype(dtype), knn=7, ratio=0.5, sampling_method=0, seed=11)
    keep = np.flatnonzero(r["keep"])            # (the assertions of tests/test_gpu_sampling_normals.py::check)
    assert np.array_equal(out["kept_idx"], keep) and out["boxes"] == r["boxes"]
    assert out["xyz"].tobytes() == r["xyz"][keep].tobytes()
    nd, nr = out["normals"].astype(np.float64), r["normals"][keep].astype(np.float64)
    assert np.abs(nd - nr).max() <= {F32: 1e-6, F64: 1e-13}[dtype]


@case("sampling_surface_normal", ["pgicp_sampling_surface_normal*"], oracle=_ssn_oracle, dtypes=(F32, F64))
def run_ssn(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    r = ctx.sampling_surface_normal(s["ref_xyz"].astype(dtype), knn=7, ratio=0.5, sampling_method=0, seed=11, descriptors=s["ref_nrm"].astype(dtype), dtype=dtype)
    r2 = ctx.sampling_surface_normal(s["ref_xyz"].astype(dtype), knn=9, ratio=0.3, sampling_method=1, seed=5, dtype=dtype)
    return {"xyz": r["xyz"], "normals": r["normals"], "kept_idx": r["kept_idx"], "desc": r["descriptors"], "boxes": r["boxes"],
            "m1.xyz": r2["xyz"], "m1.normals": r2["normals"], "m1.kept_idx": r2["kept_idx"], "m1.boxes": r2["boxes"]}


def _voxel_oracle(out, oracles, dtype):
    from voxel_grid_ref import voxel_grid
    s = two_scans()
    r = voxel_grid(s["ref_xyz"].astype(dtype), (0.5, 0.4, 0.3), True, s["ref_nrm"].astype(dtype), True, dtype)
    for k in ("xyz", "descriptors", "kept_idx", "count"):
        assert same_bits(out[k], np.asarray(r[k], dtype=out[k].dtype)), k


@case("voxel_grid", ["pgicp_voxel_grid*"], oracle=_voxel_oracle, dtypes=(F32, F64))
def run_voxel(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    r = ctx.voxel_grid(s["ref_xyz"].astype(dtype), v_size=(0.5, 0.4, 0.3), use_centroid=True, descriptors=s["ref_nrm"].astype(dtype), dtype=dtype)
    r2 = ctx.voxel_grid(s["reading_xyz"].astype(dtype), v_size=(1.0, 1.0, 1.0), use_centroid=False, dtype=dtype)
    return {"xyz": r["xyz"], "descriptors": r["descriptors"], "kept_idx": r["kept_idx"], "count": r["count"],
            "c.xyz": r2["xyz"], "c.kept_idx": r2["kept_idx"], "c.count": r2["count"]}


# the densities and MaxDensity (include/pgicp_density.h), at surface_normals' size; the references of tests/test_gpu_density.py
DENS_KNN, DENS_SEED = 10, 5


def _dens_cloud(dtype):
    return np.ascontiguousarray(two_scans()["ref_xyz"][:4000].astype(dtype))


def _densities_oracle(out, oracles, dtype):
    o, xyz = _orc(oracles, dtype), _dens_cloud(dtype)
    assert same_bits(out["densities"], o.densities(xyz, o.surface_normals(xyz, DENS_KNN)["ids"]))


@case("surface_densities", ["pgicp_surface_densities*"], oracle=_densities_oracle, dtypes=(F32, F64))
def run_surface_densities(ctx, aux, dtype):
    set_chain(ctx)
    r = ctx.surface_densities(_dens_cloud(dtype), knn=DENS_KNN, dtype=dtype)
    return {"normals": r["normals"], "eigen_values": r["eigen_values"], "densities": r["densities"]}


def _max_density_oracle(out, oracles, dtype):
    sfx = "_f32" if dtype == F32 else "_f64"
    dens = oracles[2]("surface_densities" + sfx)["densities"]           # (that case is checked against the oracle)
    md = float(np.median(dens))
    keep = np.flatnonzero(_orc(oracles, dtype).max_density_keep(dens, max_density=md, seed=DENS_SEED)).astype(np.int32)
    assert float(out["md"]) == md and 0 < len(keep) < len(dens) and np.array_equal(out["kept_idx"], keep)


@case("max_density", ["pgicp_max_density*", "pgicp_surface_densities*"], oracle=_max_density_oracle, dtypes=(F32, F64))
def run_max_density(ctx, aux, dtype):
    set_chain(ctx)
    dens = ctx.surface_densities(_dens_cloud(dtype), knn=DENS_KNN, dtype=dtype, want_normals=False, want_eigen=False)["densities"]
    md = float(np.median(dens))
    return {"md": np.array(md), "kept_idx": ctx.max_density(dens, max_density=md, seed=DENS_SEED)}


def _normals_max_density_oracle(out, oracles, dtype):
    """tests/test_gpu_density.py::fused_equals_stages: the fused call's rows are the stage calls' rows of the kept points"""
    sfx = "_f32" if dtype == F32 else "_f64"
    st, keep = oracles[2]("surface_densities" + sfx), oracles[2]("max_density" + sfx)["kept_idx"]
    xyz = _dens_cloud(dtype)
    assert np.array_equal(out["kept_idx"], keep) and same_bits(out["xyz"], xyz[keep])
    for k in ("normals", "eigen_values", "densities"):
        assert same_bits(out[k], st[k][keep]), k
    assert same_bits(out["descriptors"], two_scans()["ref_nrm"][:4000].astype(dtype)[keep])


@case("normals_max_density", ["pgicp_normals_max_density*"], oracle=_normals_max_density_oracle, dtypes=(F32, F64))
def run_normals_max_density(ctx, aux, dtype):
    set_chain(ctx)
    xyz = _dens_cloud(dtype)
    md = float(np.median(ctx.surface_densities(xyz, knn=DENS_KNN, dtype=dtype, want_normals=False, want_eigen=False)["densities"]))
    r = ctx.normals_max_density(xyz, knn=DENS_KNN, max_density=md, seed=DENS_SEED, descriptors=two_scans()["ref_nrm"][:4000].astype(dtype), dtype=dtype)
    return {k: np.ascontiguousarray(r[k]) for k in ("xyz", "normals", "eigen_values", "densities", "descriptors", "kept_idx")}


FILTERS = [(icp.FILTER_MIN_DIST, 1.0, 0), (icp.FILTER_MAX_DIST, 40.0, 0), (icp.FILTER_BOUNDING_BOX, -2.0, -1.0, -5.0, 0.5, 1.0, 5.0, 1),
           (icp.FILTER_RANDOM_SAMPLING, 0.9, 7)]


def _features(dtype, n=None):
    s = two_scans()
    x = s["reading_xyz"][:n] if n else s["reading_xyz"]
    return np.concatenate([x, np.ones((len(x), 1), dtype=np.float32)], axis=1).astype(dtype)


def _filter_oracle(out, oracles, dtype):
    keep = _orc(oracles, dtype).filter_chain(FILTERS, _features(dtype))
    assert np.array_equal(out["idx"], np.asarray(keep, dtype=np.int32))


@case("filter_cloud", ["pgicp_filter_cloud*"], oracle=_filter_oracle, dtypes=(F32, F64))
def run_filter_cloud(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx)
    f = _features(dtype)
    of, od, idx, dev = ctx.filter_cloud(FILTERS, f, descriptors=s["reading_nrm"].astype(dtype), T=synth.se3(x=0.1, z=1.7, yaw=0.01), rotate_rows=(0, -1))
    return {"features": of, "descriptors": od, "idx": idx, "n": int(dev.n)}


def _filter_dev_oracle(out, oracles, dtype):
    s = two_scans()
    o = _orc(oracles, dtype)
    f = _features(dtype)
    keep = o.filter_chain(FILTERS[:2], f)
    assert out["n"] == len(keep) and np.array_equal(out["dropped"], np.setdiff1d(np.arange(len(f)), keep).astype(np.int32))
    _check_icp(out, "a", o, np.ascontiguousarray(f[keep][:, :3]), s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), s["T_init"], CHAIN)


@case("filter_cloud_dev_align", ["pgicp_filter_cloud_dev*", "pgicp_align*"], oracle=_filter_dev_oracle, dtypes=(F32, F64))
def run_filter_dev_align(ctx, aux, dtype, n=None):
    s = two_scans()
    set_chain(ctx)
    mid = ctx.set_map(s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), center=True, dtype=dtype)
    nout, dev, dropped = ctx.filter_cloud_dev(FILTERS[:2], _features(dtype, n), dropped_cap=4096)
    T, st = ctx.align(mid, dev, s["T_init"], dtype=dtype)
    out = {"n": nout, "dropped": dropped, "a.T": T, "a.order": ctx.reading_order(nout)}
    put_stats(out, "a", st)
    ctx.destroy_map(mid)
    return out


def _upload_oracle(out, oracles, dtype):
    w = s2m()
    rds = [w.scans_xyz[0].astype(dtype), np.ascontiguousarray(w.scans_xyz[1][:3333].astype(dtype))]
    for p in range(2):
        _check_icp(out, f"p{p}", _orc(oracles, dtype), rds[p], w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), w.T_init[p], CHAIN)


@case("upload_align", ["pgicp_upload*", "pgicp_align_batch*"], oracle=_upload_oracle, dtypes=(F32, F64))
def run_upload_align(ctx, aux, dtype):
    w = s2m()
    set_chain(ctx)
    mid = ctx.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=True, dtype=dtype)
    rds = [w.scans_xyz[0].astype(dtype), np.ascontiguousarray(w.scans_xyz[1][:3333].astype(dtype))]
    devs = ctx.upload(rds)
    T, sts = ctx.align_batch([mid, mid], devs, [w.T_init[0], w.T_init[1]], dtype=dtype)
    out = {"T": T}
    for p in range(2):
        put_stats(out, f"p{p}", sts[p])
        out[f"p{p}.T"], out[f"p{p}.order"] = T[p], ctx.reading_order(len(rds[p]), problem=p)
    ctx.destroy_map(mid)
    return out


def _values(m):
    return np.random.default_rng(5).uniform(0.0, 1.0, m)


@case("descriptor_filter_align", ["pgicp_map_set_values*", "pgicp_set_descriptor_filter", "pgicp_get_descriptor_filter", "pgicp_align*"], dtypes=(F32, F64))
def run_descriptor_align(ctx, aux, dtype):
    from generic_descriptor_ref import gd_weights, kept_and_overlap
    s = two_scans()
    rd = s["reading_xyz"].astype(dtype)
    vals = _values(len(s["ref_xyz"])).astype(dtype)
    out = {}
    for mode, thr in (("larger", 0.2), ("soft", None)):
        set_chain(ctx)
        mid = ctx.set_map(s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), center=True, dtype=dtype)
        ctx.set_map_values(mid, vals, dtype=dtype)
        ctx.set_descriptor_filter(mode, thr)
        out[f"{mode}.get"] = np.array(ctx.get_descriptor_filter()[1])
        T, st = ctx.align(mid, rd, s["T_init"], dtype=dtype)
        out[f"{mode}.T"] = T
        put_stats(out, mode, st)
        put_last_matches(out, mode, ctx, len(rd), 0, dtype, st["trim_limit"])
        # the reference's weights on the call's own last correspondences (tests/test_gpu_generic_descriptor.py)
        ids, d2 = out[f"lm.{mode}.ids"], out[f"lm.{mode}.d2"]
        kept, overlap = kept_and_overlap(ids, d2, st["trim_limit"], gd_weights(ids, vals, mode, thr, dtype), dtype)
        assert st["n_kept"] == kept, (mode, st["n_kept"], kept)
        if mode != "soft":
            assert st["overlap"] == overlap, (mode, st["overlap"], overlap)
        ctx.destroy_map(mid)
    set_chain(ctx)
    return out


# -- maps --------------------------------------------------------------------------------------------------------------------------------
def _map_batch_inputs(dtype):
    s, w = two_scans(), s2m()
    xs = [s["ref_xyz"].astype(dtype), w.map_xyz[:20_000].astype(dtype), s["ref_xyz"][:3000].astype(dtype)]
    ns = [s["ref_nrm"].astype(dtype), w.map_nrm[:20_000].astype(dtype), s["ref_nrm"][:3000].astype(dtype)]
    rds = [s["reading_xyz"].astype(dtype), w.scans_xyz[0].astype(dtype), s["reading_xyz"][:2000].astype(dtype)]
    return xs, ns, rds, [s["T_init"], w.T_init[0], s["T_init"]]


def _map_batch_oracle(out, oracles, dtype):
    xs, ns, rds, T0 = _map_batch_inputs(dtype)
    assert out["sizes"].tolist() == [len(x) for x in xs]
    for p in range(3):
        _check_icp(out, f"p{p}", _orc(oracles, dtype), rds[p], xs[p], ns[p], T0[p], CHAIN)


@case("map_batch_align", ["pgicp_map_create_batch*", "pgicp_map_size", "pgicp_align_batch*"], oracle=_map_batch_oracle, dtypes=(F32, F64))
def run_map_batch(ctx, aux, dtype):
    xs, ns, rds, T0 = _map_batch_inputs(dtype)
    set_chain(ctx)
    ids = ctx.set_maps(xs, ns, center=True, dtype=dtype)
    out = {"sizes": np.array([ctx.map_size(m) for m in ids])}
    T, sts = ctx.align_batch(ids, rds, T0, dtype=dtype, raise_on_error=False)
    out["T"] = T
    for p in range(3):
        put_stats(out, f"p{p}", sts[p])
        out[f"p{p}.T"], out[f"p{p}.order"] = T[p], ctx.reading_order(len(rds[p]), problem=p)
    for m in ids:
        ctx.destroy_map(m)
    return out


def _adopt_oracle(out, oracles, dtype):
    w = s2m()
    assert out["size"] == len(w.map_xyz)
    _check_icp(out, "a", _orc(oracles, dtype), w.scans_xyz[1].astype(dtype), w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), w.T_init[1], CHAIN)


@case("adopt_map_align", ["pgicp_map_transfer", "pgicp_map_create*", "pgicp_align*"], oracle=_adopt_oracle, dtypes=(F32, F64))
def run_adopt(ctx, aux, dtype):
    """the background builder of pgslam_amd/local_mapper.py: aux indexes the map, ctx takes it over and aligns"""
    return adopt_serve(ctx, aux, adopt_build(aux, dtype), dtype)


def adopt_build(builder, dtype):
    """the builder's half: index the map on its own context, return the id to hand over"""
    w = s2m()
    set_chain(builder)
    return builder.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=True, dtype=dtype)


def adopt_serve(ctx, builder, built, dtype):
    """the server's half: take the map over (pgicp_map_transfer), align against it, destroy it"""
    w = s2m()
    set_chain(ctx)
    mid = ctx.adopt_map(builder, built)
    T, st = ctx.align(mid, w.scans_xyz[1].astype(dtype), w.T_init[1], dtype=dtype)
    out = {"a.T": T, "a.order": ctx.reading_order(len(w.scans_xyz[1])), "size": ctx.map_size(mid)}
    put_stats(out, "a", st)
    ctx.destroy_map(mid)
    return out


def _far_oracle(out, oracles, dtype):
    """tests/test_gpu_matcher_state.py::test_scan_ahead_of_its_map / ..._large_error_and_far_scan: the per-point state"""
    ref, nrm, rd, T0 = far_scene()
    o = _orc(oracles, dtype).icp(rd.astype(dtype), ref.astype(dtype), nrm.astype(dtype), T0, pair_order=out["p0.order"], **CHAIN)
    _check_state(out, "p0", o, dtype)
    if dtype == F32:
        from test_gpu_bit_exact import check
        check(_stats_of(out, "p0"), out["p0.T"], o, "far")


@case("far_mode_align", ["pgicp_align_batch*"], oracle=_far_oracle, dtypes=(F32, F64))
def run_far(ctx, aux, dtype, P=1):
    ref, nrm, rd, T0 = far_scene()
    set_chain(ctx)
    mid = ctx.set_map(ref.astype(dtype), nrm.astype(dtype), center=True, dtype=dtype)
    T, sts = ctx.align_batch([mid] * P, [rd.astype(dtype)] * P, [T0 @ synth.se3(x=0.002 * p) for p in range(P)], dtype=dtype, raise_on_error=False)
    out = {"T": T}
    for p in range(P):
        put_stats(out, f"p{p}", sts[p])
        out[f"p{p}.T"], out[f"p{p}.order"] = T[p], ctx.reading_order(len(rd), problem=p)
        put_last_matches(out, f"p{p}", ctx, len(rd), p, dtype, sts[p]["trim_limit"])
    ctx.destroy_map(mid)
    return out


def _subset_oracle(out, oracles, dtype):
    w = s2m()
    rd = np.ascontiguousarray(w.map_xyz[0::7][:5000].astype(dtype))
    o = _orc(oracles, dtype).icp(rd, w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), np.eye(4), pair_order=out["p0.order"],
                                 **dict(CHAIN, center_reference=False))
    from test_gpu_bit_exact import check
    check(_stats_of(out, "p0"), out["p0.T"], o, "subset")
    assert float(out["p0.trim_limit"]) == 0.0 and float(out["p0.residual"]) == 0.0        # every distance 0, as the case is meant
    _check_chain(out["ratio"][0], out["resid"][0], _orc(oracles, dtype), rd, w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), np.eye(4), "subset")


@case("subset_of_map_align", ["pgicp_align_batch*", "pgicp_partial_chain_batch*"], oracle=_subset_oracle, dtypes=(F32, F64))
def run_subset(ctx, aux, dtype, P=1):
    """a reading that IS part of the map: every distance 0, every quantile 0"""
    w = s2m()
    set_chain(ctx)
    mid = ctx.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=False, dtype=dtype)
    rds = [np.ascontiguousarray(w.map_xyz[p::7][:5000].astype(dtype)) for p in range(P)]
    T, sts = ctx.align_batch([mid] * P, rds, [np.eye(4)] * P, dtype=dtype, raise_on_error=False)
    out = {"T": T}
    for p in range(P):
        put_stats(out, f"p{p}", sts[p])
        out[f"p{p}.T"], out[f"p{p}.order"] = T[p], ctx.reading_order(len(rds[p]), problem=p)
    ratio, resid, status = ctx.partial_chain_batch([mid] * P, rds, [np.eye(4)] * P, dtype=dtype, raise_on_error=False)
    out.update({"ratio": ratio, "resid": resid, "status": status})
    ctx.destroy_map(mid)
    return out


# -- calls that end in an error of the API kind (ordinary returned codes) -------------------------------------------------------------
def _code(fn):
    try:
        fn()
    except icp.PgicpError as e:
        return int(e.code)
    return icp.OK


@case("err_arg_refusals", ["pgicp_set_params", "pgicp_set_var_trim", "pgicp_last_var_trim_ratio", "pgicp_icp_pair_f32", "pgicp_get_params", "pgicp_get_var_trim"], error=True)
def run_err_arg(ctx, aux):
    import ctypes as C
    s = two_scans()
    set_chain(ctx)
    out = {"epsilon": _code(lambda: ctx.set_params(epsilon=-0.5)),
           "var_trim_order": _code(lambda: ctx.set_var_trim(0.9, 0.3, 1.0)),
           "no_var_trim_ran": _code(lambda: (ctx.outlier_weights(_distances(F32)), ctx.last_var_trim_ratio(0)))}
    mid = ctx.set_map(s["ref_xyz"], s["ref_nrm"], center=True)
    ctx.set_params(normal_max_angle=0.5)
    out["normals_missing"] = _code(lambda: ctx.align(mid, s["reading_xyz"], s["T_init"]))
    set_chain(ctx)
    ctx.set_descriptor_filter("larger", 0.5)
    out["map_without_values"] = _code(lambda: ctx.align(mid, s["reading_xyz"], s["T_init"]))
    out["pair_with_descriptor_filter"] = _code(lambda: ctx.icp_pair(s["reading_xyz"], s["ref_xyz"], s["ref_nrm"], s["T_init"]))
    ctx.set_descriptor_filter(None)
    out["bad_map_id"] = _code(lambda: ctx.align(mid + 12345, s["reading_xyz"], s["T_init"]))
    ctx.destroy_map(mid)
    p = icp.Params()
    assert ctx.lib.pgicp_get_params(ctx.h, C.byref(p)) == icp.OK
    out["params_after"] = np.frombuffer(bytes(p), dtype=np.uint8).copy()
    out["var_trim_after"] = int(ctx.get_var_trim() is None)
    for k in ("epsilon", "var_trim_order", "no_var_trim_ran", "normals_missing", "map_without_values", "pair_with_descriptor_filter"):
        assert out[k] == icp.ERR_ARG, (k, out[k])
    assert out["bad_map_id"] != icp.OK
    return out


@case("err_no_match", ["pgicp_align*", "pgicp_partial_chain_batch*"], error=True, dtypes=(F32, F64))
def run_err_no_match(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx, max_dist=0.05)
    mid = ctx.set_map(s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), center=True, dtype=dtype)
    far = s["T_init"] @ synth.se3(x=500.0)
    out = {"align": _code(lambda: ctx.align(mid, s["reading_xyz"].astype(dtype), far, dtype=dtype))}
    T, sts = ctx.align_batch([mid] * 2, [s["reading_xyz"].astype(dtype)] * 2, [far, far], dtype=dtype, raise_on_error=False)
    for p in range(2):
        out[f"p{p}.status"] = int(sts[p]["status"])
    ratio, resid, status = ctx.partial_chain_batch([mid], [s["reading_xyz"].astype(dtype)], [far], dtype=dtype, raise_on_error=False)
    out.update({"status": status})
    ctx.destroy_map(mid)
    set_chain(ctx)
    assert out["align"] == icp.ERR_NO_MATCH and out["p0.status"] == icp.ERR_NO_MATCH and int(status[0]) == icp.ERR_NO_MATCH, out
    return out


@case("err_bound", ["pgicp_align*"], error=True, dtypes=(F32, F64))
def run_err_bound(ctx, aux, dtype):
    s = two_scans()
    set_chain(ctx, bound_max_rot=0.2, bound_max_trans=0.05)
    mid = ctx.set_map(s["ref_xyz"].astype(dtype), s["ref_nrm"].astype(dtype), center=True, dtype=dtype)
    out = {"align": _code(lambda: ctx.align(mid, s["reading_xyz"].astype(dtype), s["T_init"], dtype=dtype))}
    ctx.destroy_map(mid)
    set_chain(ctx)
    assert out["align"] == icp.ERR_BOUND, out
    return out


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
# Declared entry points no case needs to reach: administrative only, nothing that computes on a cloud.
EXCLUDED = {
    # context life cycle and introspection
    "pgicp_abi_version": "library introspection", "pgicp_device_count": "library introspection",
    "pgicp_ctx_create": "context life cycle", "pgicp_ctx_create_priority": "context life cycle (the concurrency test makes one)",
    "pgicp_ctx_destroy": "context life cycle", "pgicp_last_error": "error text", "pgicp_status_string": "error text",
    "pgicp_ctx_stream": "context introspection", "pgicp_ctx_device": "context introspection", "pgicp_ctx_synchronize": "context life cycle",
    "pgicp_default_params": "fills a record, no context",
    # allocation helpers
    "pgicp_host_alloc": "allocation helper", "pgicp_host_free": "allocation helper", "pgicp_device_alloc": "allocation helper",
    "pgicp_device_free": "allocation helper", "pgicp_device_copy": "allocation helper (a plain copy)",
    # the collective and the host dispatcher helpers (no context state: tests/test_comm_host.py, tests/test_abi.py)
    "pgicp_comm_unique_id": "collective", "pgicp_comm_create": "collective", "pgicp_comm_create_host": "collective",
    "pgicp_comm_destroy": "collective", "pgicp_comm_info": "collective", "pgicp_comm_last_error": "collective",
    "pgicp_allgather_edges": "collective", "pgicp_shard_slots": "host dispatcher helper", "pgicp_shard_pairs": "host dispatcher helper",
    "pgicp_check_icp_result": "host dispatcher helper",
    # profile and debug counters: not results
    "pgicp_profile_enable": "profile", "pgicp_profile_reset": "profile", "pgicp_profile_get": "profile", "pgicp_profile_process": "profile",
    "pgicp_debug_counters": "debug counters (read by the hostile hint tests as a precondition)", "pgicp_debug_alloc_stats": "allocation counters",
}


def reached():
    return sorted({a for c in CASES.values() for a in c.api})


def declared():
    """the entry points the catalogue answers for: what include/pgicp.h and include/pgicp_density.h declare"""
    src = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("pgicp.h", "pgicp_density.h"))
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pgicp_[a-z0-9_]+)\s*\(", src)))


ERROR_CASES = [n for n, c in CASES.items() if c.error]
SMALL_MEDIUM = [n for n, c in CASES.items() if c.size != "large"]
