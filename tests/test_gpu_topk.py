"""The register top-K lists of k_normals.inc at every list size: k_surface_normals<T, K> (pgicp_surface_normals_*, K = 8, 16, 32)
and k_knn_topk<T, K> (KDTreeMatcher.knn > 1, K = 2, 4, 8, 16), in both precisions, against the oracle's statement
(orc_surface_normals, orc_kdtree_knn_k; tests/test_oracle.py pins the k-d tree against orc_knn_brute_k).  Every instance unrolls
into its own code with K - knn dummy entries in front, so each knn is chosen to land on a list's first, middle and full
(knn == K) case.  Neighbour ids and squared distances are asserted bit for bit; so are the normals and eigenvalues (the same
T sums in the same order, the same Jacobi), after the rank decision, the eigenvalues and the normals were checked against
bounds that say what a mismatch would mean.

Which test reaches which instance:
    k_surface_normals<T, 8>   knn 1, 2, 3, 7, 8    test_surface_normals_every_instance, test_memory_forms_give_the_same_bits,
                                                   test_far_from_the_origin
    k_surface_normals<T, 16>  knn 9, 15, 16        test_surface_normals_every_instance, test_memory_forms_give_the_same_bits,
                                                   test_full_size_clouds, test_far_from_the_origin, test_refusals_*,
                                                   test_dropin_filter_normals_are_the_kernels
    k_surface_normals<T, 32>  knn 17, 31, 32       test_surface_normals_every_instance, test_memory_forms_give_the_same_bits,
                                                   test_full_size_clouds, test_far_from_the_origin, test_dropin_filter_*
    k_knn_topk<T, 2>          knn 2                test_match_every_instance
    k_knn_topk<T, 4>          knn 3, 4             test_match_every_instance
    k_knn_topk<T, 8>          knn 5, 8             test_match_every_instance
    k_knn_topk<T, 16>         knn 9, 15, 16        test_match_every_instance, test_icp_at_large_knn, test_ragged_batch_at_large_knn,
                                                   test_partial_chain_and_error_stats_at_knn_16
"""
import ctypes as C
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from pgslam_amd import icp, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "chain_variants_small.npz")
KNNS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32]
TYPES = [np.float32, np.float64]
BITS = {np.float32: np.uint32, np.float64: np.uint64}
CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01,
             smooth_length=3, sensor_std_dev=0.01)
RESET = dict(knn=1, error_minimizer=0, bound_max_rot=0.0, bound_max_trans=0.0, normal_max_angle=0.0, outlier_max_dist=0.0,
             quantile_scale=1.0, robust_fct=0, robust_tuning=1.0, robust_scale=1, robust_approx=0.0)


def _o(T, oracle32, oracle64):
    return oracle32 if T == np.float32 else oracle64


def pose_error(Ta, Tb):
    d = np.linalg.inv(Ta) @ Tb
    c = min(1.0, max(-1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))
    return np.linalg.norm(d[:3, 3]), math.acos(c)


# ------------------------------------------------------------------ clouds
def lattice():
    """a 12 x 12 x 6 lattice of spacing 1/8, shuffled: every distance is a sum of exact squares, ties everywhere, and with
    maxDist 0.25 the second ring's d2 equals maxDist^2 exactly"""
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"), -1).reshape(-1, 3) / 8.0
    return g[np.random.default_rng(3).permutation(len(g))]


def cluster():
    """40 identical points among others: more equal distances than the largest list holds, broken by index"""
    rng = np.random.default_rng(8)
    x = rng.normal(size=(600, 3)) * 0.4
    x[rng.choice(600, 40, replace=False)] = DUP
    return x


DUP = (0.1, -0.2, 0.05)


@pytest.fixture(scope="module")
def scan():
    return synth.make_two_scans(6000, rings=16)["ref_xyz"]


@pytest.fixture(scope="module")
def clouds(scan):
    # (name, cloud, finite maxDist)
    return [("scan", scan, 1.0), ("lattice", lattice(), 0.25), ("cluster", cluster(), 0.5),
            ("n1", np.array([[0.5, -1.0, 2.0]]), 1.0), ("n5", np.random.default_rng(1).normal(size=(5, 3)), 2.0)]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------------ the comparison
def scatter_ratio(xyz, ids):
    """emid / ehi of the scatter of each row of neighbour ids, in float64: the rank test's quantity, free of the T sums' rounding"""
    x = np.asarray(xyz, dtype=np.float64)
    out = np.zeros(len(ids))
    for i, row in enumerate(ids):
        nb = x[row[row >= 0]]
        d = nb - nb.mean(0)
        e = np.linalg.eigvalsh(d.T @ d)
        out[i] = e[1] / e[2] if e[2] > 0 else 0.0
    return out


def compare_pca(nrm, eig, r, xyz, T, label, unequal):
    """normals / eigenvalues of the device against the oracle's: the rank decision, the eigenvalues to a few ulps of the largest,
    the normals (up to sign) to rounding scaled by the gap between the two smaller eigenvalues -- then bit for bit"""
    eps = float(np.finfo(T).eps)
    ro, ev = r["normals"].astype(np.float64), r["eigen_values"].astype(np.float64)
    nd, ed = nrm.astype(np.float64), eig.astype(np.float64)
    deg_o = np.all(r["normals"] == np.array([0, 1, 0], dtype=T), 1) & np.all(r["eigen_values"] == np.array([0, 0, 1], dtype=T), 1)
    deg_d = np.all(nrm == np.array([0, 1, 0], dtype=T), 1) & np.all(eig == np.array([0, 0, 1], dtype=T), 1)
    differ = np.flatnonzero(deg_o != deg_d)
    if len(differ):                          # only where emid / ehi lies within rounding of the threshold 3 eps
        ratio = scatter_ratio(xyz, r["ids"][differ])
        near = np.abs(ratio - 3 * eps) <= (4 * r["ids"].shape[1] + 8) * eps
        assert near.all() and len(differ) <= max(2, len(xyz) // 1000), (label, len(differ), ratio)
    both = ~deg_o & ~deg_d
    ehi = ev[both, 2:3]
    assert np.all(np.abs(ed[both] - ev[both]) <= 8 * eps * ehi), label
    gap = (ev[both, 1] - ev[both, 0])[:, None]
    s = np.sign(np.sum(nd[both] * ro[both], 1, keepdims=True))
    s[s == 0] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(gap > 0, 64 * eps * ehi / gap, np.inf)
    assert np.all(np.abs(nd[both] * s - ro[both]) <= np.maximum(bound, 64 * eps)), label
    k = int(np.count_nonzero(nrm.view(BITS[T]) != r["normals"].view(BITS[T]))) + \
        int(np.count_nonzero(eig.view(BITS[T]) != r["eigen_values"].view(BITS[T])))
    if k:
        print(f"{label}: {k} normal / eigenvalue components not bit-equal")
    unequal.append(k)


def check(ctx, o, xyz, T, knn, md, label, unequal):
    x = np.ascontiguousarray(xyz, dtype=T)
    nrm, eig, ids, d2 = ctx.surface_normals(x, knn=knn, max_dist=md, want_eigen=True, want_ids=True)
    r = o.surface_normals(x, knn, md)
    assert ids.shape == (len(x), knn) and ids.tobytes() == r["ids"].tobytes(), label
    assert d2.tobytes() == r["d2"].tobytes(), label
    compare_pca(nrm, eig, r, x, T, label, unequal)
    return nrm, eig, ids, d2, r


def raw(ctx, x, knn, md, out_stride=3, eig=True, ids=True, d2=True):
    """pgicp_surface_normals_* through ctypes: host in, host out, any out_stride, any subset of the optional outputs"""
    T = x.dtype.type
    n = len(x)
    nrm = np.full((n, out_stride), T(-7.5), dtype=T)
    e = np.full((n, 3), T(-7.5), dtype=T) if eig else None
    i = np.full((n, knn), -9, dtype=np.int32) if ids else None
    d = np.full((n, knn), T(-7.5), dtype=T) if d2 else None
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    fn = getattr(ctx.lib, "pgicp_surface_normals" + ctx._sfx(T))
    rc = fn(ctx.h, C.c_void_p(x.ctypes.data), C.c_int(x.strides[0] // x.itemsize), C.c_int(n), C.c_int(icp.HOST), C.c_int(knn),
            C.c_double(md), p(nrm), C.c_int(out_stride), p(e), p(i), p(d))
    return rc, nrm, e, i, d


# ------------------------------------------------------------------ surface normals
@pytest.mark.parametrize("T", TYPES)
def test_surface_normals_every_instance(ctx, oracle32, oracle64, clouds, T):
    """knn 1 ... 32 (the first, a middle and the full case of every list size) x finite / unbounded maxDist x a Velodyne-shaped
    scan, a lattice with exact ties and d2 == maxDist^2, a cluster of 40 identical points, clouds smaller than knn"""
    o = _o(T, oracle32, oracle64)
    unequal = []
    for name, xyz, md in clouds:
        for knn in KNNS:
            for m in (md, np.inf):
                _, _, ids, d2, r = check(ctx, o, xyz, T, knn, m, f"{name} {T.__name__} knn={knn} maxDist={m}", unequal)
                if name == "lattice" and m == md and knn > 27:   # 27 points lie closer: the <= boundary is reached and kept
                    assert np.any(d2 == T(md) * T(md))
                if name == "cluster":                        # a duplicate's neighbours: the lowest indices of the 40 copies
                    dup = np.flatnonzero(np.all(xyz == np.array(DUP), 1))
                    assert len(dup) == 40 and np.array_equal(ids[dup[0]], dup[:knn]) and np.all(d2[dup[0]] == 0)
                if len(xyz) < knn:
                    assert np.all(ids[:, len(xyz):] == -1) and np.all(np.isinf(d2[:, len(xyz):]))
    print(f"{T.__name__}: {sum(unequal)} normal / eigenvalue components not bit-equal over {len(unequal)} cases")
    assert sum(unequal) == 0


@pytest.mark.parametrize("T", TYPES)
def test_memory_forms_give_the_same_bits(ctx, scan, T):
    """torch in / torch out, a homogeneous (n, 4) cloud, out_stride 5 with the caller's padding untouched, each optional output
    alone: the bits of the plain host call"""
    import torch
    x = np.ascontiguousarray(scan, dtype=T)
    x4 = np.concatenate([x, np.ones((len(x), 1), dtype=T)], 1)
    for knn, md in ((3, 1.0), (8, np.inf), (16, 1.0), (32, 0.5)):
        ref = ctx.surface_normals(x, knn=knn, max_dist=md, want_eigen=True, want_ids=True)
        g = ctx.surface_normals(torch.from_numpy(x).cuda(), knn=knn, max_dist=md, want_eigen=True, want_ids=True)
        for a, b in zip(g, ref):
            assert a.is_cuda and a.cpu().numpy().tobytes() == b.tobytes(), knn
        h = ctx.surface_normals(x4, knn=knn, max_dist=md, want_eigen=True, want_ids=True)
        for a, b in zip(h, ref):
            assert a.tobytes() == b.tobytes(), knn
        rc, nrm5, e, i, d = raw(ctx, x, knn, md, out_stride=5)
        assert rc == icp.OK
        assert np.ascontiguousarray(nrm5[:, :3]).tobytes() == ref[0].tobytes()
        assert np.all(nrm5[:, 3:] == T(-7.5))                               # the caller's padding columns
        assert e.tobytes() == ref[1].tobytes() and i.tobytes() == ref[2].tobytes() and d.tobytes() == ref[3].tobytes()
        for want in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
            rc, nrm, e, i, d = raw(ctx, x, knn, md, eig=want[0], ids=want[1], d2=want[2])
            assert rc == icp.OK and nrm.tobytes() == ref[0].tobytes(), want
            assert e is None or e.tobytes() == ref[1].tobytes()
            assert i is None or i.tobytes() == ref[2].tobytes()
            assert d is None or d.tobytes() == ref[3].tobytes()
        # a device cloud of stride 4 into a device output of stride 5: the same bits, the padding kept
        t4 = torch.from_numpy(x4).cuda()
        out = torch.full((len(x), 5), -7.5, dtype=t4.dtype, device=t4.device)
        fn = getattr(ctx.lib, "pgicp_surface_normals" + ctx._sfx(T))
        rc = fn(ctx.h, C.c_void_p(t4.data_ptr()), C.c_int(4), C.c_int(len(x)), C.c_int(icp.DEVICE), C.c_int(knn), C.c_double(1e300 if np.isinf(md) else md),
                C.c_void_p(out.data_ptr()), C.c_int(5), None, None, None)
        assert rc == icp.OK
        o = out.cpu().numpy()
        assert np.ascontiguousarray(o[:, :3]).tobytes() == ref[0].tobytes() and np.all(o[:, 3:] == T(-7.5))


@pytest.fixture(scope="module")
def big():
    sys.path.insert(0, ROOT)
    from bench import build_pairs, build_workload
    xyz, _, _ = build_pairs(100000)
    w = build_workload(100000, 1000000, 16)
    return dict(scan100k=xyz[0], map1M=w.map_xyz)


@pytest.mark.parametrize("name,knn,T", [("scan100k", 10, np.float32), ("scan100k", 32, np.float32), ("map1M", 10, np.float32),
                                        ("scan100k", 10, np.float64), ("scan100k", 32, np.float64)])
def test_full_size_clouds(ctx, oracle32, oracle64, big, name, knn, T):
    """the benchmark's 100 k-point scan and 1 M-point map: neighbours bit for bit"""
    x = np.ascontiguousarray(big[name], dtype=T)
    ids, d2 = ctx.surface_normals(x, knn=knn, max_dist=1.0, want_ids=True)[1:]
    r = _o(T, oracle32, oracle64).surface_normals(x, knn, 1.0)
    assert ids.tobytes() == r["ids"].tobytes()
    if T == np.float32:
        assert d2.tobytes() == r["d2"].tobytes()
    assert np.mean(ids[:, -1] >= 0) > 0.5


def test_far_from_the_origin(ctx, oracle64, scan, big):
    """float64 clouds far from the origin: the map is built uncentred, coordinates stay exact, neighbours are the oracle's.  A
    200 k-point cloud at 4e6 m passes |coordinate| x n = 8e11 -- beyond the fixed-point centroid's limit, which only a centred
    map needs: pgicp_surface_normals takes it; a centred map of it is still refused."""
    unequal = []
    for off in (3e3, 4e5):
        x = scan.astype(np.float64) + np.array([off, -0.5 * off, 0.25 * off])
        for knn in (8, 16, 32):
            check(ctx, oracle64, x, np.float64, knn, 1.0, f"offset {off} knn={knn}", unequal)
    far = big["map1M"][:200000].astype(np.float64) + np.array([4e6, 1e6, 100.0])
    assert np.abs(far).max() * len(far) >= 5e11
    ids, d2 = ctx.surface_normals(far, knn=10, max_dist=1.0, want_ids=True)[1:]
    oid, od2 = oracle64.knn_k(far, far, 10, 1.0)
    assert ids.tobytes() == oid.tobytes() and d2.tobytes() == od2.tobytes()
    with pytest.raises(icp.PgicpError) as e:
        ctx.set_map(far, None, center=True)
    assert e.value.code == icp.ERR_ARG and "5e11" in str(e.value)
    mid = ctx.set_map(far, None, center=False)                       # uncentred: no centroid, no limit
    ctx.destroy_map(mid)
    print(f"far: {sum(unequal)} normal / eigenvalue components not bit-equal")
    assert sum(unequal) == 0


@pytest.mark.parametrize("T", TYPES)
def test_refusals_leave_the_context_usable(ctx, scan, T):
    x = np.ascontiguousarray(scan[:3000], dtype=T)
    rc, *good = raw(ctx, x, 9, 1.0)
    assert rc == icp.OK
    bad_x = x.copy()
    bad_x[17, 1] = np.nan
    for args in (dict(knn=0), dict(knn=33), dict(md=0.0), dict(md=-1.0), dict(md=float("nan")), dict(x=bad_x), dict(x=x[:0])):
        a = dict(x=x, knn=9, md=1.0)
        a.update(args)
        xx = a["x"] if len(a["x"]) else x                            # (n = 0: a valid pointer, no points)
        n = len(a["x"])
        fn = getattr(ctx.lib, "pgicp_surface_normals" + ctx._sfx(T))
        nrm = np.zeros((max(n, 1), 3), dtype=T)
        rc = fn(ctx.h, C.c_void_p(xx.ctypes.data), C.c_int(3), C.c_int(n), C.c_int(icp.HOST), C.c_int(a["knn"]), C.c_double(a["md"]),
                C.c_void_p(nrm.ctypes.data), C.c_int(3), None, None, None)
        assert rc == icp.ERR_ARG, args
        rc, *again = raw(ctx, x, 9, 1.0)
        assert rc == icp.OK and all(p.tobytes() == q.tobytes() for p, q in zip(again, good)), args


# ------------------------------------------------------------------ KDTreeMatcher.knn > 1
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("max_dist", [2.0, 0.25, float("inf")])
def test_match_every_instance(ctx, oracle32, oracle64, gold, T, max_dist):
    """knn 2 ... 16 (every k_knn_topk list's first and full case): the stage's pairs bit for bit, host and torch readings"""
    import torch
    o = _o(T, oracle32, oracle64)
    mx, rd = gold["map_xyz"].astype(T), gold["reading"].astype(T)
    q = o.transform(gold["T_init"], rd)
    mid = ctx.set_map(mx, None, center=False)
    try:
        for k in (2, 3, 4, 5, 8, 9, 15, 16):
            ctx.set_params(**{**CHAIN, **RESET, "max_dist": max_dist, "knn": k})
            ids, d2 = ctx.match(mid, rd, T=gold["T_init"])
            oid, od2 = o.knn_k(mx, q, k, max_dist)
            assert ids.shape == (len(q), k)
            assert ids.tobytes() == oid.tobytes(), k
            assert d2.tobytes() == od2.tobytes(), k
            tid, td2 = ctx.match(mid, torch.from_numpy(rd).cuda(), T=gold["T_init"])
            assert tid.is_cuda and tid.cpu().numpy().tobytes() == oid.tobytes() and td2.cpu().numpy().tobytes() == od2.tobytes(), k
            if max_dist == 0.25:
                assert np.any(oid[:, -1] < 0) and np.any(oid[:, -1] >= 0)        # short lists and full ones
    finally:
        ctx.destroy_map(mid)
        ctx.set_params(**dict(CHAIN, **RESET))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("knn", [9, 16])
def test_icp_at_large_knn(ctx, oracle32, oracle64, gold, T, knn):
    z = gold
    o = _o(T, oracle32, oracle64)
    chain = dict(CHAIN, knn=knn)
    ctx.set_params(**dict(CHAIN, **RESET))
    ctx.set_params(**chain)
    rd, mx, mn = z["reading"].astype(T), z["map_xyz"].astype(T), z["map_nrm"].astype(T)
    mid = ctx.set_map(mx, mn, center=True, dtype=T)
    try:
        Tg, st = ctx.align(mid, rd, z["T_init"], dtype=T)
        ids, d2 = ctx.debug_last_matches(len(rd), dtype=T)
    finally:
        ctx.destroy_map(mid)
        ctx.set_params(**dict(CHAIN, **RESET))
    r = o.icp(rd, mx, mn, z["T_init"], **chain)
    assert st["status"] == 0 and r["status"] == 0
    dt, dr = pose_error(r["T"], Tg)
    assert dt < 1e-5 and dr < 1e-5, (dt, dr)
    assert st["iterations"] == r["iterations"] and st["converged"] == r["converged"]
    assert st["n_finite"] == r["n_finite"] and st["n_kept"] == r["n_kept"]
    assert st["overlap"] == pytest.approx(r["overlap"], rel=1e-12)
    assert ids.shape == (len(rd), knn)
    if T == np.float32:                                  # the last iteration's knn x N pairs
        assert ids.tobytes() == r["last_ids"].tobytes() and d2.tobytes() == r["last_d2"].tobytes()
    else:
        assert np.mean(ids == r["last_ids"]) > 0.999


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("knn", [9, 16])
def test_ragged_batch_at_large_knn(ctx, oracle32, oracle64, gold, T, knn):
    """three problems of different n on two maps: each problem's knn x N pairs sit at its own pairs_off; the batch gives the
    single calls' results and the oracle's"""
    z = gold
    o = _o(T, oracle32, oracle64)
    chain = dict(CHAIN, knn=knn)
    ctx.set_params(**dict(CHAIN, **RESET))
    ctx.set_params(**chain)
    mx, mn = z["map_xyz"].astype(T), z["map_nrm"].astype(T)
    maps = [(mx, mn), (mx[::2].copy(), mn[::2].copy())]
    mids = [ctx.set_map(a, b, center=True, dtype=T) for a, b in maps]
    rds = [z["reading"].astype(T), z["reading"][:1001].astype(T), z["reading"][700:].astype(T)]
    which = [0, 1, 0]
    T0 = [z["T_init"], z["T_init"] @ synth.se3(x=0.03, yaw=0.004), z["T_init"] @ synth.se3(y=-0.02, yaw=-0.003)]
    try:
        Ts, sts = ctx.align_batch([mids[w] for w in which], rds, T0, dtype=T)
        last = [ctx.debug_last_matches(len(rds[b]), problem=b, dtype=T) for b in range(3)]
        singles = []
        for b in range(3):
            Tb, sb = ctx.align(mids[which[b]], rds[b], T0[b], dtype=T)
            singles.append((Tb, sb, ctx.debug_last_matches(len(rds[b]), dtype=T)))
    finally:
        for m in mids:
            ctx.destroy_map(m)
        ctx.set_params(**dict(CHAIN, **RESET))
    for b in range(3):
        Tb, sb, (ids1, d21) = singles[b]
        np.testing.assert_allclose(Ts[b], Tb, rtol=0, atol=1e-12)
        for k in ("status", "iterations", "n_finite", "n_kept"):
            assert sts[b][k] == sb[k], (b, k)
        ids, d2 = last[b]
        assert ids.shape == (len(rds[b]), knn) and np.array_equal(ids, ids1), b
        r = o.icp(rds[b], maps[which[b]][0], maps[which[b]][1], T0[b], **chain)
        assert r["status"] == 0
        dt, dr = pose_error(r["T"], Ts[b])
        assert dt < 1e-5 and dr < 1e-5, (b, dt, dr)
        assert sts[b]["iterations"] == r["iterations"] and sts[b]["n_finite"] == r["n_finite"] and sts[b]["n_kept"] == r["n_kept"], b


def test_partial_chain_and_error_stats_at_knn_16(ctx, oracle32, gold):
    z = gold
    chain = dict(CHAIN, knn=16)
    ctx.set_params(**dict(CHAIN, **RESET))
    ctx.set_params(**chain)
    mid = ctx.set_map(z["map_xyz"], z["map_nrm"], center=False)
    try:
        ov, res = ctx.partial_chain(mid, z["reading"], T=z["T_truth"])
        moved = oracle32.transform(z["T_truth"], z["reading"])
        ids, d2 = ctx.match(mid, moved)
        w = np.where(ids >= 0, 1.0, 0.0).astype(np.float32)
        w[::7] = 0.5
        _, _, sys_ = ctx.error_stats(mid, moved, ids, w)
    finally:
        ctx.destroy_map(mid)
        ctx.set_params(**dict(CHAIN, **RESET))
    po = oracle32.partial_chain(z["reading"], z["map_xyz"], z["map_nrm"], z["T_truth"], **chain)
    assert po["status"] == 0
    assert ov == pytest.approx(po["overlap"], rel=1e-12) and res == pytest.approx(po["residual"], rel=1e-6)
    oid, od2 = oracle32.knn_k(z["map_xyz"], moved, 16, CHAIN["max_dist"])
    assert ids.tobytes() == oid.tobytes() and d2.tobytes() == od2.tobytes()
    st, osys = oracle32.p2plane_system(moved, z["map_xyz"], z["map_nrm"], ids, w)
    assert st == 0
    np.testing.assert_allclose(sys_, osys, rtol=1e-12, atol=1e-12)


def test_knn_above_the_largest_list_is_refused(ctx):
    ctx.set_params(**dict(CHAIN, **RESET))
    ctx.set_params(knn=16)
    with pytest.raises(icp.PgicpError) as e:
        ctx.set_params(knn=17)
    assert e.value.code == icp.ERR_ARG and ctx.params.knn == 16
    ctx.set_params(**dict(CHAIN, **RESET))


# ------------------------------------------------------------------ the drop-in filter: 4-row features, the same kernel
def _filter_apply(tmp_path, yaml, xyz, T):
    from test_cpp_dropin import build
    exe = build("filter_apply")
    fy, fi, fo = (tmp_path / "f.yaml", tmp_path / "in.bin", tmp_path / "out.bin")
    fy.write_text(yaml)
    fi.write_bytes(struct.pack("i", len(xyz)) + np.ascontiguousarray(xyz, dtype=T).tobytes())
    r = subprocess.run([exe, "f64" if T == np.float64 else "f32", str(fy), str(fi), str(fo)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw_ = fo.read_bytes()
    m, hn, hd = struct.unpack("iii", raw_[:12])
    it = np.dtype(T).itemsize
    off = 12 + 3 * m * it
    nrm = np.frombuffer(raw_, dtype=T, count=3 * m, offset=off).reshape(m, 3) if hn else None
    off += 3 * m * it if hn else 0
    dens = np.frombuffer(raw_, dtype=T, count=m, offset=off) if hd else None
    return m, nrm, dens


@pytest.mark.parametrize("T", TYPES)
def test_dropin_filter_normals_are_the_kernels(ctx, tmp_path, scan, T):
    """SurfaceNormalDataPointsFilter through the YAML loader: its normals come from the 4-row homogeneous features and are the
    bits of pgicp_surface_normals on the xyz"""
    x = np.ascontiguousarray(scan, dtype=T)
    for knn in (16, 32):
        m, nrm, _ = _filter_apply(tmp_path, "- SurfaceNormalDataPointsFilter:\n    knn: %d\n" % knn, x, T)
        assert m == len(x)
        assert nrm.tobytes() == ctx.surface_normals(x, knn=knn).tobytes(), knn


@pytest.mark.parametrize("T", TYPES)
def test_dropin_filter_densities_at_knn_32(oracle32, oracle64, tmp_path, scan, T):
    o = _o(T, oracle32, oracle64)
    x = np.ascontiguousarray(scan, dtype=T)
    m, _, dens = _filter_apply(tmp_path, "- SurfaceNormalDataPointsFilter:\n    knn: 32\n    maxDist: 1.0\n    keepDensities: 1\n", x, T)
    want = o.densities(x, o.surface_normals(x, 32, 1.0)["ids"])
    assert m == len(x) and dens.tobytes() == want.tobytes()
