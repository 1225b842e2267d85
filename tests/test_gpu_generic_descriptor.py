"""[EXT] GenericDescriptorOutlierFilter on the device (pgicp_set_descriptor_filter, pgicp_map_set_values) against the numpy
statement of tests/generic_descriptor_ref.py: filters that weigh every pair 1 give the unfiltered call bit for bit, the last
iteration's pairs give n_kept and overlap, the refusals leave a usable context, the seeded probe is the unseeded one, and the
filter does what it is for -- a moved object in the map, labelled 0, no longer pulls the ICP off."""
import os
import subprocess

import numpy as np
import pytest

from pgslam_amd import icp, synth
from generic_descriptor_ref import gd_weights, kept_and_overlap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01,
             smooth_length=3, sensor_std_dev=0.01)
DTYPES = [np.float32, np.float64]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_same(a, b, what):
    (Ta, sa), (Tb, sb) = a, b
    assert same_bits(Ta, Tb), what
    for k in ("status", "iterations", "n_kept", "n_finite"):
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])
    for k in ("overlap", "residual", "trim_limit"):
        assert same_bits(sa[k], sb[k]), (what, k, sa[k], sb[k])
    if "cov" in sa:
        assert same_bits(sa["cov"], sb["cov"]), (what, "cov")


def _scene(dtype, n_queries=3):
    w = synth.make_scan_to_map(n_scan=8000, n_map=60_000, n_queries=n_queries, n_map_poses=4, rings=16)
    return w, [x.astype(dtype) for x in w.scans_xyz]


# filters that weigh every pair 1: (mode, threshold, value of every map point)
PASS_ALL = [("larger", 0.5, 1.0), ("smaller", 2.0, 1.0), ("soft", None, 0.75)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sum_order", [icp.SUM_ORDER_SORTED, icp.SUM_ORDER_SCAN])
@pytest.mark.parametrize("mode,thr,val", PASS_ALL)
def test_pass_all_filter_is_the_unfiltered_call_bit_for_bit(dtype, sum_order, mode, thr, val):
    w, rds = _scene(dtype)
    ctx = icp.Context(0, **CHAIN, sum_order=sum_order)
    m1 = ctx.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=True, dtype=dtype)
    m2 = ctx.set_map(w.map_xyz[::2].astype(dtype), w.map_nrm[::2].astype(dtype), center=True, dtype=dtype)
    for m, n in ((m1, len(w.map_xyz)), (m2, len(w.map_xyz[::2]))):
        ctx.set_map_values(m, np.full(n, val, dtype=dtype))
    maps = [m1, m2, m1]

    def run():
        out = [ctx.align(m1, rds[0], w.T_init[0], dtype=dtype)]
        Tb, sb = ctx.align_batch(maps, rds, w.T_init, dtype=dtype)
        out += list(zip(Tb, sb))
        Tr, sr, res, ratio, rst = ctx.align_residual_batch(maps, rds, w.T_init, dtype=dtype)
        out += list(zip(Tr, sr))
        extra = [res.tolist(), ratio.tolist(), list(rst)]
        extra.append(ctx.partial_chain(m1, rds[1], T=Tb[1], dtype=dtype))
        extra.append(ctx.partial_chain_batch(maps, rds, list(Tb), dtype=dtype))
        return out, extra
    base, base_extra = run()
    ctx.set_descriptor_filter(mode, thr)
    assert ctx.get_descriptor_filter()[0] == mode
    try:
        got, got_extra = run()
    finally:
        ctx.set_descriptor_filter(None)
    assert all(s["status"] == 0 for _, s in base)
    for k, (a, b) in enumerate(zip(got, base)):
        check_same(a, b, (mode, k))
    assert same_bits(np.array(got_extra[0]), np.array(base_extra[0])) and got_extra[1:3] == base_extra[1:3]
    assert got_extra[3] == base_extra[3]
    for a, b in zip(got_extra[4], base_extra[4]):
        assert same_bits(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64))
    ctx.close()


def _unresolved(orc, reading, T, map_xyz, ids, max_dist):
    """points the matcher left without a neighbour although the map has one well within maxDist at the final pose (the last
    matches were made one small increment before it: a margin of 5 cm)"""
    ids = ids.reshape(len(reading), -1)
    k = ids.shape[1]
    none = (ids < 0).any(axis=1)
    if not none.any():
        return 0
    moved = (reading[none].astype(np.float64) @ T[:3, :3].T) + T[:3, 3]
    _, d2 = orc.knn_k(map_xyz.astype(np.float64), moved, k)          # the r-th nearest map point of every such point
    d2 = d2.reshape(-1, k)
    return int(((ids[none] < 0) & (np.sqrt(d2) < max_dist - 0.05)).sum())


def _check_last_iteration(ctx, n, problem, st, values, mode, thr, dtype, resolved=None):
    ids, d2 = ctx.debug_last_matches(n, problem=problem, dtype=dtype)
    if resolved is not None:
        assert resolved(ids) == 0, (problem, resolved(ids))    # soft mode: every query resolved exactly
    w = gd_weights(ids, values, mode, thr, dtype)
    kept, overlap = kept_and_overlap(ids, d2, st["trim_limit"], w, dtype)
    assert st["n_kept"] == kept, (problem, st["n_kept"], kept)
    if mode == "soft":
        assert st["overlap"] == pytest.approx(overlap, rel=1e-9), (problem, st["overlap"], overlap)
    else:
        assert st["overlap"] == overlap, (problem, st["overlap"], overlap)
    return kept


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knn", [1, 3])
@pytest.mark.parametrize("mode", ["larger", "smaller", "soft"])
def test_last_iteration_follows_the_statement(oracle64, dtype, knn, mode):
    w, rds = _scene(dtype)
    ctx = icp.Context(0, **CHAIN, knn=knn)
    mid = ctx.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=True, dtype=dtype)
    m = len(w.map_xyz)
    if mode == "soft":
        values = synth.uniform(77, m, 0.0, 1.0).astype(dtype)
        thr = None
    else:
        values = (w.map_xyz[:, 0] > np.median(w.map_xyz[:, 0])).astype(dtype)     # 0 / 1 by region
        thr = 0.5
    # a row of a column-major descriptor matrix: stride 2
    desc = np.empty((m, 2), dtype=dtype)
    desc[:, 0] = values
    desc[:, 1] = -7.0
    ctx.set_map_values(mid, desc[:, 0])
    ctx.set_descriptor_filter(mode, thr)
    T, st = ctx.align(mid, rds[0], w.T_init[0], dtype=dtype)
    assert st["status"] == 0
    def res(p, T_p):
        if mode != "soft":
            return None
        return lambda ids: _unresolved(oracle64, rds[p], T_p, w.map_xyz, ids, CHAIN["max_dist"])
    kept = _check_last_iteration(ctx, len(rds[0]), 0, st, values, mode, thr, dtype, res(0, T))
    assert 0 < kept < len(rds[0]) * knn
    Tb, sb = ctx.align_batch(mid, rds, w.T_init, dtype=dtype)
    for p in range(len(rds)):
        assert sb[p]["status"] == 0
        _check_last_iteration(ctx, len(rds[p]), p, sb[p], values, mode, thr, dtype, res(p, Tb[p]))
    assert same_bits(Tb[0], T)                            # a problem's result does not depend on its batch
    ctx.close()


def test_refusals_leave_a_usable_context():
    w, rds = _scene(np.float32, n_queries=1)
    ctx = icp.Context(0, **CHAIN)
    mid = ctx.set_map(w.map_xyz, w.map_nrm, center=True)
    good = ctx.align(mid, rds[0], w.T_init[0])
    m = len(w.map_xyz)

    def refused(fn, code=icp.PgicpError):
        with pytest.raises(code):
            fn()
        setting = ctx.get_descriptor_filter()
        ctx.set_descriptor_filter(None)
        check_same(ctx.align(mid, rds[0], w.T_init[0]), good, "after a refusal")
        if setting[0] is not None:
            ctx.set_descriptor_filter(*setting)
    with pytest.raises(ValueError):
        ctx.set_descriptor_filter("larger")                # a hard mode needs its threshold
    with pytest.raises(icp.PgicpError):
        ctx.set_descriptor_filter("larger", float("nan"))
    # a map without values
    ctx.set_descriptor_filter("larger", 0.5)
    refused(lambda: ctx.align(mid, rds[0], w.T_init[0]))
    ctx.set_descriptor_filter(None)
    # NaN values are refused when handed in
    bad = np.ones(m, np.float32)
    bad[5] = np.nan
    refused(lambda: ctx.set_map_values(mid, bad))
    bad[5] = np.inf
    refused(lambda: ctx.set_map_values(mid, bad))
    # a negative value: fine for a hard mode, refused in soft mode
    neg = np.ones(m, np.float32)
    neg[7] = -1.0
    ctx.set_map_values(mid, neg)
    ctx.set_descriptor_filter("soft")
    try:
        refused(lambda: ctx.align(mid, rds[0], w.T_init[0]))
        ctx.set_descriptor_filter("larger", -2.0)
        check_same(ctx.align(mid, rds[0], w.T_init[0]), good, "hard mode, all pass")
        # a soft maximum of 0: every weight 0, NO_MATCH
        ctx.set_map_values(mid, np.zeros(m, np.float32))
        ctx.set_descriptor_filter("soft")
        refused(lambda: ctx.align(mid, rds[0], w.T_init[0]), icp.ConvergenceError)
        # a destroyed and re-created map id has no values
        ctx.set_map_values(mid, np.ones(m, np.float32))
        ctx.destroy_map(mid)
        mid2 = ctx.set_map(w.map_xyz, w.map_nrm, center=True)
        assert mid2 == mid                                 # the id is reused ...
        with pytest.raises(icp.PgicpError):
            ctx.align(mid2, rds[0], w.T_init[0])           # ... without the values of the map it named before
        ctx.set_map_values(mid2, np.ones(m, np.float32))
        check_same(ctx.align(mid2, rds[0], w.T_init[0]), good, "values set again")
        # a torch CUDA tensor (device memory, a strided view of a descriptor matrix's row) and the dtype check
        import torch
        dev = torch.ones((m, 2), dtype=torch.float32, device="cuda")[:, 0]
        ctx.set_map_values(mid2, dev, dtype=np.float32)
        check_same(ctx.align(mid2, rds[0], w.T_init[0]), good, "values from a CUDA tensor")
        with pytest.raises(TypeError):
            ctx.set_map_values(mid2, dev.double(), dtype=np.float32)
        with pytest.raises(ValueError):
            ctx.set_map_values(mid2, np.ones((m, 2), np.float32))
        ctx.set_map_values(mid2, None)                     # dropped on request
        with pytest.raises(icp.PgicpError):
            ctx.align(mid2, rds[0], w.T_init[0])
    finally:
        ctx.set_descriptor_filter(None)
    check_same(ctx.align(mid, rds[0], w.T_init[0]), good, "filter off")
    ctx.close()


@pytest.mark.parametrize("mode", ["larger", "soft"])
def test_seeded_probe_equals_the_unseeded_one(mode):
    """pgicp_partial_chain_seeded with the filter on searches unseeded: its result is the plain probe's."""
    world = synth.make_world()
    poses = [synth.se3(x=-6.0 + 1.5 * k, yaw=np.deg2rad(1.5 * (k % 3 - 1))) for k in range(5)]
    kf = [synth.make_scan(world, poses[k], 12_000, 7100 + k, rings=16) for k in range(4)]
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
    scan, _ = synth.make_scan(world, poses[4] @ synth.se3(x=-2.0), 10_000, 7200, rings=16)
    scan = scan.astype(np.float32)
    T0 = synth.se3_inv(ref_pose) @ poses[4] @ synth.se3(x=-2.0) @ synth.perturbation(41)
    A, B = icp.Context(0, **CHAIN), icp.Context(0, **CHAIN)
    ma = A.set_map(xa, na, center=True)
    mb = B.set_map(xb, nb, center=False)
    T, st = A.align(ma, scan, T0)
    assert st["status"] == 0
    vb = (xb[:, 2] > np.median(xb[:, 2])).astype(np.float32) if mode == "larger" else synth.uniform(5, len(xb), 0.0, 2.0).astype(np.float32)
    B.set_map_values(mb, vb)
    B.set_descriptor_filter(mode, 0.5 if mode == "larger" else None)
    start_a = np.concatenate([[0], np.cumsum(sizes_a)])
    start_b = np.concatenate([[0], np.cumsum(sizes_b)])
    dst = [int(start_b[order_b.index(k)]) if k in order_b else -1 for k in order_a]

    def probe(T_at, seeded):
        r = B.partial_chain_seeded(mb, scan, T_at, A, start_a, dst) if seeded else B.partial_chain(mb, scan, T=T_at)
        ids, d2 = B.debug_last_matches(len(scan))
        return r, ids, d2
    for T_at in (T, T @ synth.se3(x=0.4, yaw=np.deg2rad(1.0))):
        (ra, ia, da), (rb, ib, db) = probe(T_at, True), probe(T_at, False)
        assert ra == rb
        assert np.array_equal(ia, ib) and np.array_equal(da.view(np.uint32), db.view(np.uint32))
        assert 0.0 < ra[0] < 1.0
    for c in (A, B):
        c.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["larger", "soft"])
def test_moved_object_no_longer_pulls_the_icp_off(dtype, mode):
    """A third of the map (y > 2 m) has moved 0.3 m in x since it was mapped and is labelled 0; the reading sees the world as it
    is.  Without the filter the ICP ends about 0.17 m from the truth; with it, within a few millimetres.  (Margins checked
    first on the host with the oracle's ICP, the moved block in the map and taken out of it: 0.171 m and 0.003 m.)  In soft
    mode the static points carry labels in [0.5, 1]."""
    s = synth.make_two_scans(10_000, rings=16)
    ref, nrm, rd = s["ref_xyz"].copy(), s["ref_nrm"], s["reading_xyz"]
    blk = ref[:, 1] > 2.0
    ref[blk] += np.array([0.3, 0.0, 0.0], dtype=ref.dtype)
    values = np.where(blk, 0.0, 1.0)
    if mode == "soft":
        values = np.where(blk, 0.0, synth.uniform(11, len(ref), 0.5, 1.0))
    ctx = icp.Context(0, **dict(CHAIN, max_iters=40))
    mid = ctx.set_map(ref.astype(dtype), nrm.astype(dtype), center=True, dtype=dtype)
    ctx.set_map_values(mid, values.astype(dtype))

    def err(T):
        return float(np.linalg.norm((np.linalg.inv(s["T_truth"]) @ T)[:3, 3]))
    T_off, s_off = ctx.align(mid, rd.astype(dtype), s["T_init"], dtype=dtype)
    ctx.set_descriptor_filter(mode, 0.5 if mode == "larger" else None)
    T_on, s_on = ctx.align(mid, rd.astype(dtype), s["T_init"], dtype=dtype)
    ctx.set_descriptor_filter(None)
    assert s_off["status"] == 0 and s_on["status"] == 0
    assert err(T_off) > 0.05, err(T_off)
    assert err(T_on) < 0.01, err(T_on)
    ctx.close()


def test_dropin_and_facade():
    """tests/cpp/test_generic_descriptor_gpu.cpp: an ICP from YAML on clouds carrying probabilityStatic, PoseGraphSlam(MT) drives
    whose filter passes everything equal to the unfiltered drive bit for bit, and a drive with labelled dynamic points."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_generic_descriptor_gpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-local-typedefs", "-Wno-unused-variable", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp",
                           "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "generic descriptor gpu tests ok" in out.stdout


# ---------------------------------------------------------------------------------------------------------------------------
# Against the oracle: the ICP loop of oracle/icp_oracle.c (orc_icp_map_ex) spelled out in Python from the oracle's primitives,
# with the GenericDescriptor factor multiplied into the chain's weights in T.  With the factor all ones it is oracle.icp bit for
# bit; the device, with the filter on, must land on its pose.
def _mat4_mul(a, b):
    """mat4_mul of the oracle: row-major 4x4 doubles, each entry summed k = 0..3 in order"""
    c = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(a[i, k]) * float(b[k, j])
            c[i, j] = s
    return c


def _rigid_inverse(t):
    """mat4_rigid_inverse of the oracle"""
    r = np.eye(4)
    r[:3, :3] = t[:3, :3].T
    for i in range(3):
        r[i, 3] = -((float(r[i, 0]) * float(t[0, 3]) + float(r[i, 1]) * float(t[1, 3])) + float(r[i, 2]) * float(t[2, 3]))
    return r


def oracle_loop(orc, reading, ref_xyz, ref_nrm, T_init, chain, gd=None, reading_nrm=None, pair_order=None):
    """orc_icp_map_ex (knn 1, point-to-plane, kd-tree, centred reference) from the oracle's stages.  gd(ids) -> the
    GenericDescriptor weights in T of one iteration's matches (None: no such filter).  Returns (status, T, iterations)."""
    T = np.dtype(orc.dtype).type
    ref_xyz = np.ascontiguousarray(ref_xyz, dtype=orc.dtype)
    mean = orc.centroid(ref_xyz)
    ref = (ref_xyz - mean).astype(orc.dtype)
    T_ref_mean = np.eye(4)
    T_ref_mean[:3, 3] = mean.astype(np.float64)
    T_pre = _mat4_mul(_rigid_inverse(T_ref_mean), np.asarray(T_init, dtype=np.float64))
    rd = orc.transform(T_pre, reading)
    use_nrm = reading_nrm is not None and chain.get("normal_max_angle", 0.0) > 0.0
    rd_n = orc.transform(T_pre, reading_nrm, rotate_only=True) if use_nrm else None
    chk = orc.checker(chain["max_iters"], chain["min_diff_rot"], chain["min_diff_trans"], chain["smooth_length"])
    T_iter = np.eye(4)
    it = 0
    while True:
        step = orc.transform(T_iter, rd)
        ids, d2 = orc.knn_kdtree(step, ref, chain["max_dist"])
        if chain.get("robust_fct", 0) > 0:
            w, _ = orc.robust_weights(d2, chain["robust_fct"], chain.get("robust_tuning", 1.0), chain.get("robust_scale", 1),
                                      chain.get("robust_approx", 0.0))
        else:
            st, w, _, _ = orc.trim_weights(d2, chain["trim_ratio"])
            if st != 0:
                return st, None, it
        md = chain.get("outlier_max_dist", 0.0)
        if md > 0.0 and np.isfinite(md):
            w[~(d2 <= T(md) * T(md))] = T(0)
        if use_nrm:
            w = orc.normal_weights(orc.transform(T_iter, rd_n, rotate_only=True), ref_nrm, ids, chain["normal_max_angle"], w)
        if gd is not None:
            w = (w * gd(ids)).astype(orc.dtype)
        st, sys_ = orc.p2plane_system(step, ref, ref_nrm, ids, w, order=pair_order)
        if st != 0:
            return st, None, it
        x, _ = orc.solve6(sys_)
        T_iter = _mat4_mul(orc.delta_T(x), T_iter)
        it += 1
        f = orc.checker_check(chk, T_iter)
        if f & (8 | 16):
            return f, None, it
        if not f & 1:
            break
    return 0, _mat4_mul(T_ref_mean, _mat4_mul(T_iter, T_pre)), it


def _pose_err(A, B):
    d = np.linalg.inv(A) @ B
    return float(np.linalg.norm(d[:3, 3])), float(np.arccos(min(1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0)))


ORACLE_CASES = {
    "hard": dict(mode="larger"),
    "hard_robust": dict(mode="larger", robust_fct=1, robust_tuning=1.0, robust_scale=1),
    "hard_maxdist": dict(mode="larger", outlier_max_dist=0.3),
    "hard_normals": dict(mode="larger", normal_max_angle=0.7),
    "hard_all": dict(mode="smaller", robust_fct=2, robust_tuning=1.5, robust_scale=1, outlier_max_dist=0.4, normal_max_angle=0.9),
    "soft_robust": dict(mode="soft", robust_fct=1, robust_tuning=1.0, robust_scale=1),
    "soft_normals": dict(mode="soft", normal_max_angle=0.7),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_against_the_oracle_loop(oracle32, oracle64, dtype, case):
    """The moved-object scene of test_moved_object_no_longer_pulls_the_icp_off with labels by region (0 on the moved block and on
    a third of the rest), so that the factor removes pairs the distance filters keep; soft mode labels in [0, 1]."""
    orc = oracle32 if dtype == np.float32 else oracle64
    spec = dict(ORACLE_CASES[case])
    mode = spec.pop("mode")
    chain = dict(CHAIN, max_iters=40, **spec)
    if "robust_fct" in chain:
        chain["trim_ratio"] = 1.0
    s = synth.make_two_scans(10_000, rings=16)
    ref = s["ref_xyz"].copy()
    blk = ref[:, 1] > 2.0
    ref[blk] += np.array([0.3, 0.0, 0.0], dtype=ref.dtype)
    ref, nrm = ref.astype(dtype), s["ref_nrm"].astype(dtype)
    rd, rd_nrm = s["reading_xyz"].astype(dtype), s["reading_nrm"].astype(dtype)
    if mode == "soft":
        values = np.where(blk, 0.0, synth.uniform(13, len(ref), 0.0, 1.0)).astype(dtype)
        thr = None
    else:
        values = np.where(blk | (ref[:, 0] < np.quantile(ref[:, 0], 0.33)), 0.0, 1.0).astype(dtype)
        if mode == "smaller":
            values = (1.0 - values).astype(dtype)
        thr = 0.5
    normals = rd_nrm if "normal_max_angle" in chain else None
    ctx = icp.Context(0, **chain)
    mid = ctx.set_map(ref, nrm, center=True, dtype=dtype)
    ctx.set_map_values(mid, values)
    ctx.set_descriptor_filter(mode, thr)
    T_dev, st = ctx.align(mid, rd, s["T_init"], dtype=dtype, normals=normals)
    order = ctx.reading_order(len(rd))
    ctx.close()
    assert st["status"] == 0
    # the loop is the oracle's ICP: with the factor all ones, oracle.icp bit for bit
    st1, T1, it1 = oracle_loop(orc, rd, ref, nrm, s["T_init"], chain, None, normals, order)
    o = orc.icp(rd, ref, nrm, s["T_init"], reading_nrm=normals, pair_order=order, **chain)
    assert st1 == 0 and o["status"] == 0
    assert same_bits(T1, o["T"]) and it1 == o["iterations"], (case, it1, o["iterations"])
    ones = lambda ids: np.ones(ids.shape, dtype=dtype)
    st1b, T1b, it1b = oracle_loop(orc, rd, ref, nrm, s["T_init"], chain, ones, normals, order)
    assert same_bits(T1b, o["T"]) and it1b == o["iterations"]
    # the device with the filter on lands where the loop with the factor does
    gd = lambda ids: gd_weights(ids, values, mode, thr, dtype)
    st2, T2, it2 = oracle_loop(orc, rd, ref, nrm, s["T_init"], chain, gd, normals, order)
    assert st2 == 0
    dt, dr = _pose_err(T2, T_dev)
    assert dt < 1e-5 and dr < 1e-5, (case, dt, dr)
    assert st["iterations"] == it2, (case, st["iterations"], it2)
    # ... and the factor mattered: the loop without it ends elsewhere
    assert _pose_err(T1, T2)[0] > 1e-4, case
