"""KDTreeVarDistMatcher's per-point search radii on the device (include/pgicp_vardist.h, k_vardist.inc) against the numpy statement
of tests/var_dist_ref.py: the matcher stage against the cut of the oracle's brute-force kNN; uniform radii = max_dist against the
same call unarmed, bit for bit; whole ICPs with real radii against the reference loop (the oracle's stages with the cut behind the
matcher -- pinned to the oracle by tests/test_var_dist_host.py, which also checks the scene's conditions), bit for bit; the other
consumers of the cut pairs; refusals and call history."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pgslam_amd import icp, synth  # noqa: E402
import noise_overlap_ref  # noqa: E402
import var_dist_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
BASE = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
_ORACLES = {}


def _oracle(dtype):
    from oracle import Oracle
    key = np.dtype(dtype).name
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(dtype)
    return _ORACLES[key]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def result(T, st):
    return dict(st, T=T)


def assert_same(a, b, what):
    assert a["status"] == b["status"] == 0, (what, a["status"], b["status"])
    assert ref.same_result(a, b), (what, ref.diff_report(a, b))


# ---- the stage ---------------------------------------------------------------------------------------------------------------
_STAGE = {}


def stage_scene(dtype, knn):
    """a 20 000-point map, a 5 000-point reading in its frame, the oracle's brute-force kNN under max_dist (once per type and knn;
    a point's list does not depend on the other points, so every prefix of the reading shares it) and the radii: log-uniform in
    [0.05, 2] m, 5 % +inf, 5 % 0"""
    key = (np.dtype(dtype).name, knn)
    if key not in _STAGE:
        if "w" not in _STAGE:
            _STAGE["w"] = synth.make_scan_to_map(n_scan=5000, n_map=20_000, n_queries=1, n_map_poses=3, rings=16)
        w = _STAGE["w"]
        o = _oracle(dtype)
        m = w.map_xyz.astype(dtype)
        q = o.transform(w.T_init[0], w.scans_xyz[0].astype(dtype))
        ids, d2 = o.knn_brute(q, m, 2.0) if knn == 1 else o.knn_brute_k(q, m, knn, 2.0)
        r = np.random.default_rng(20)
        radii = np.exp(r.uniform(np.log(0.05), np.log(2.0), len(q)))
        u = r.random(len(q))
        radii[u < 0.05] = np.inf
        radii[u > 0.95] = 0.0
        _STAGE[key] = dict(m=m, q=q, ids=ids, d2=d2, radii=radii.astype(dtype))
    return _STAGE[key]


@DTYPES
@pytest.mark.parametrize("knn", [1, 3])
def test_stage_match_is_the_cut_of_the_exact_knn(dtype, knn):
    sc = stage_scene(dtype, knn)
    ctx = icp.Context(0, **dict(BASE, knn=knn))
    mid = ctx.set_map(sc["m"], None, center=False, dtype=dtype)
    for n in (1, 63, 64, 65, 255, 256, 257, 5000):
        ids, d2 = ctx.match(mid, sc["q"][:n], dtype=dtype, radii=sc["radii"][:n])
        rid, rd2, removed = ref.cut(sc["ids"][:n], sc["d2"][:n], sc["radii"][:n], knn, dtype)
        assert np.array_equal(ids, rid), (n, int((ids != rid).sum()))
        assert d2.tobytes() == rd2.tobytes(), n
        if n == 5000:
            assert removed.mean() > 0.05 and (rid >= 0).mean() > 0.05          # the cut both takes and leaves
    # the arm was consumed: the next call is the uncut one
    ids, d2 = ctx.match(mid, sc["q"], dtype=dtype)
    assert np.array_equal(ids, sc["ids"]) and d2.tobytes() == sc["d2"].tobytes()
    ctx.close()


# ---- uniform radii = max_dist: the same call unarmed ----------------------------------------------------------------------------
GPU_CHAINS = {
    "trimmed": dict(trim_ratio=0.85),
    "robust": dict(trim_ratio=1.0, robust_fct=1, robust_tuning=1.0, robust_scale=1),
}


@DTYPES
@pytest.mark.parametrize("chain", sorted(GPU_CHAINS))
def test_uniform_radii_are_the_unarmed_call(dtype, chain):
    w = synth.make_scan_to_map(n_scan=8000, n_map=60_000, n_queries=4, n_map_poses=4, rings=16)
    ctx = icp.Context(0, **dict(BASE, **GPU_CHAINS[chain]))
    m1 = ctx.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=True, dtype=dtype)
    m2 = ctx.set_map(w.map_xyz[::2].astype(dtype), w.map_nrm[::2].astype(dtype), center=True, dtype=dtype)
    rds = [x.astype(dtype)[:k] for x, k in zip(w.scans_xyz, (8000, 5000, 7777, 6001))]
    full = [np.full(len(r), 2.0, dtype=dtype) for r in rds]
    a = ctx.align(m1, rds[0], w.T_init[0], dtype=dtype, radii=full[0])
    b = ctx.align(m1, rds[0], w.T_init[0], dtype=dtype)
    assert_same(result(*a), result(*b), "align")
    maps = [m1, m2, m1, m2]
    full[2] = None                                          # (a problem without a row)
    Ta, sa = ctx.align_batch(maps, rds, w.T_init, dtype=dtype, radiis=full)
    Tb, sb = ctx.align_batch(maps, rds, w.T_init, dtype=dtype)
    for p in range(4):
        assert_same(result(Ta[p], sa[p]), result(Tb[p], sb[p]), ("batch", p))
    # ... and the fused residual pass behind the ICPs
    Ta, sa, res_a, ratio_a, rst_a = ctx.align_residual_batch(maps, rds, w.T_init, dtype=dtype, radiis=full)
    Tb, sb, res_b, ratio_b, rst_b = ctx.align_residual_batch(maps, rds, w.T_init, dtype=dtype)
    for p in range(4):
        assert_same(result(Ta[p], sa[p]), result(Tb[p], sb[p]), ("residual batch", p))
    assert res_a.tobytes() == res_b.tobytes() and ratio_a.tobytes() == ratio_b.tobytes() and (rst_a == rst_b).all() and (rst_a == 0).all()
    ctx.close()


# ---- real radii: the whole ICP against the reference loop -----------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("chain", sorted(GPU_CHAINS))
def test_icp_with_radii_is_the_reference_loop(dtype, chain):
    sc = ref.scene()
    o = _oracle(dtype)
    rd, rf, nrm = sc["rd"].astype(dtype), sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype)
    radii = sc["radii"].astype(dtype)
    ctx = icp.Context(0, **dict(BASE, **GPU_CHAINS[chain]))
    mid = ctx.set_map(rf, nrm, center=True, dtype=dtype)
    singles = []
    for k, T0 in enumerate(sc["T_inits"]):
        T, st = ctx.align(mid, rd, T0, dtype=dtype, radii=radii)
        order = ctx.reading_order(len(rd))
        ids, d2 = ctx.debug_last_matches(len(rd), dtype=dtype)
        r = ref.icp_ref(o, rd, rf, nrm, T0, radii=radii, pair_order=order, **ref.CHAINS[chain])
        print(np.dtype(dtype).name, chain, k, "iterations", st["iterations"], r["iterations"], "n_kept", st["n_kept"], r["n_kept"],
              "n_finite", st["n_finite"], r["n_finite"], "limit", st["trim_limit"], r["trim_limit"], "|dT|", np.abs(T - r["T"]).max())
        assert_same(result(T, st), r, (chain, k))
        assert np.array_equal(ids, r["last_ids"]) and d2.tobytes() == r["last_d2"].tobytes(), k
        # (pairs cut in the first iteration that the last one keeps: what a cut written over the matcher's seeds would lose)
        assert int((r["removed"][0] & (ids >= 0)).sum()) >= 100
        singles.append((T, st))
    Tb, sb = ctx.align_batch(mid, [rd] * 3, sc["T_inits"], dtype=dtype, radiis=[radii] * 3)
    for p in range(3):
        assert_same(result(Tb[p], sb[p]), result(*singles[p]), ("batch", p))
    ctx.close()


# ---- the other consumers of the cut pairs ------------------------------------------------------------------------------------------
@DTYPES
def test_noise_overlap_reads_the_cut_pairs(dtype):
    sc = ref.scene()
    o = _oracle(dtype)
    T_ = np.dtype(dtype).type
    rd = sc["rd"].astype(dtype)
    radii = sc["radii"].astype(dtype)
    noise = o.simple_sensor_noise(rd, 0, 1.0)
    ctx = icp.Context(0, **BASE)
    mid = ctx.set_map(sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype), center=True, dtype=dtype)
    T, st = ctx.align(mid, rd, sc["T_inits"][0], dtype=dtype, radii=radii, noise=noise)
    ids, d2 = ctx.debug_last_matches(len(rd), dtype=dtype)
    assert ((d2 <= radii * radii) | ((ids == -1) & np.isinf(d2))).all()
    assert (ids[np.isfinite(d2)] >= 0).all() and (d2[ids >= 0] <= radii[ids >= 0] * radii[ids >= 0]).all()
    stw, w, limit, nf = o.trim_weights(d2, BASE["trim_ratio"])
    assert stw == 0 and nf == st["n_finite"] and same_bits(limit, st["trim_limit"]) and int(w.sum()) == st["n_kept"]
    lo, hi, nb, m = noise_overlap_ref.count_bounds(d2, w, noise, dtype)
    assert lo == hi, (lo, hi)                               # (the scene decides every pair the same way over the reachable means)
    assert st["n_elements"] == nb == st["n_kept"]
    assert st["overlap_noise"] == float(T_(lo) / T_(nb))
    ctx.close()


@DTYPES
def test_var_trim_selects_over_the_cut_distances(dtype):
    from test_gpu_var_trim import VT, _check_last_iteration
    sc = ref.scene()
    rd = sc["rd"].astype(dtype)
    ctx = icp.Context(0, **BASE)
    mid = ctx.set_map(sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype), center=True, dtype=dtype)
    ctx.set_var_trim(*VT)
    T, st = ctx.align(mid, rd, sc["T_inits"][1], dtype=dtype, radii=sc["radii"].astype(dtype))
    _check_last_iteration(ctx, len(rd), 0, st, dtype)
    ids, d2 = ctx.debug_last_matches(len(rd), dtype=dtype)
    assert np.isinf(d2).mean() > 0.01                        # (the distances it selected over were cut ones)
    ctx.close()


def test_radii_that_cut_every_pair_are_no_match():
    sc = ref.scene()
    ctx = icp.Context(0, **BASE)
    mid = ctx.set_map(sc["ref"], sc["ref_nrm"], center=True)
    with pytest.raises(icp.ConvergenceError, match="no point to minimize"):
        ctx.align(mid, sc["rd"], sc["T_inits"][0], radii=np.full(len(sc["rd"]), 1e-6, dtype=F32))
    T, st = ctx.align(mid, sc["rd"], sc["T_inits"][0])       # the context is usable
    assert st["status"] == 0
    ctx.close()


# ---- refusals, call history ---------------------------------------------------------------------------------------------------------
def test_refusals_and_history():
    sc = ref.scene()
    rd, n = sc["rd"], len(sc["rd"])
    T0 = sc["T_inits"][0]
    radii = sc["radii"].astype(F32)
    fresh = icp.Context(0, **BASE)
    mf = fresh.set_map(sc["ref"], sc["ref_nrm"], center=True)
    want = result(*fresh.align(mf, rd, T0))
    fresh.close()

    ctx = icp.Context(0, **BASE)
    mid = ctx.set_map(sc["ref"], sc["ref_nrm"], center=True)

    def unarmed_and_usable(what):
        assert_same(result(*ctx.align(mid, rd, T0)), want, what)

    for name, bad in (("negative", -0.5), ("nan", np.nan)):
        r = radii.copy()
        r[n // 2] = bad
        with pytest.raises(icp.PgicpError, match="negative or a NaN") as e:
            ctx.align(mid, rd, T0, radii=r)
        assert e.value.code == icp.ERR_ARG, name
        unarmed_and_usable(name)
    with pytest.raises(icp.PgicpError, match="values armed for problem 0") as e:          # wrong count
        ctx.align(mid, rd, T0, radii=radii[:-1])
    assert e.value.code == icp.ERR_ARG
    unarmed_and_usable("count")
    ctx.arm_reading_radii([radii.astype(F64)], F64)                                         # wrong element type
    with pytest.raises(icp.PgicpError, match="another element type") as e:
        ctx.align(mid, rd, T0)
    assert e.value.code == icp.ERR_ARG
    unarmed_and_usable("dtype")
    ctx.arm_reading_radii([radii, radii], F32)                                              # wrong problem count
    with pytest.raises(icp.PgicpError, match="armed for 2 problems") as e:
        ctx.match(mid, rd)
    assert e.value.code == icp.ERR_ARG
    unarmed_and_usable("problems")
    # the seeded probe refuses while armed and keeps the arm: the next matching call consumes it
    ctx.align(mid, rd, T0)
    ctx.arm_reading_radii([radii], F32)
    with pytest.raises(icp.PgicpError, match="seeded probe") as e:
        ctx.partial_chain_seeded(mid, rd, T0, ctx, [0, len(sc["ref"])], [0])
    assert e.value.code == icp.ERR_ARG
    ids_a, d2_a = ctx.match(mid, rd, T=T0)
    ids_u, d2_u = ctx.match(mid, rd, T=T0)
    assert (ids_a == -1).sum() > (ids_u == -1).sum() + 100
    # partial chains consume radii too: fewer pairs, another ratio; and an unarmed call after armed ones is the fresh context's
    ra, _ = ctx.partial_chain(mid, rd, T0, radii=radii)
    ru, _ = ctx.partial_chain(mid, rd, T0)
    rb, _, _ = ctx.partial_chain_batch([mid, mid], [rd, rd], [T0, T0], radiis=[radii, None])
    assert ra != ru and rb[0] == ra and rb[1] == ru
    ctx.align(mid, rd, T0, radii=radii)
    unarmed_and_usable("history")
    ctx.close()
