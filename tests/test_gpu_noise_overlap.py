"""The sensor-noise getOverlap() on the device (include/pgicp_noise.h): the SimpleSensorNoise kernel bit for bit against the
oracle; the overlap of armed ICP calls against the reference statement (tests/noise_overlap_ref.py) over the call's exact last
matches, with the weights of the oracle's own filters; single, batched, residual-batched and pair calls; call history.

What is asserted per case: n_elements == pgicp_stats.n_kept; count_lo == count_hi (the precondition of a fixed scene: the
derived band of reachable means decides every pair the same way) and count == that value; against the oracle's
orc_sensor_noise_overlap (a sequential sum in T) the count differs by at most the kept pairs with
|dist - noise - m*| <= nb eps(T) m*, computed per case.

SurfaceNormalOutlierFilter cases: the weights of the LAST iteration need the rotation that iteration ran with.  An align of the
same inputs stopped one iteration earlier (max_iters = iterations - 1; results do not depend on history, bit for bit) returns
R_iter R_init, from which R_iter follows to a few units of the last place of a double.  The oracle's orc_normal_weights then
filters the normals it rotated with that R_iter.  Precondition, asserted like count_lo == count_hi: no candidate pair's cosine
lies within 64 eps(T) of cos(maxAngle) -- the rotation is known to about one eps(T) after its rounding to T, the rotated and
normalised vectors and their dot product add a few more -- so the filter decides every pair the same way on both sides."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pgslam_amd import icp, synth  # noqa: E402
import noise_overlap_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
BASE = dict(knn=1, max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3,
            sensor_std_dev=0.01, outlier_max_dist=0.0, quantile_scale=1.0, error_minimizer=0, normal_max_angle=0.0, robust_fct=0,
            robust_tuning=1.0, robust_scale=1, robust_approx=0.0, sum_order=icp.SUM_ORDER_SORTED)

# name -> (params, var_trim, descriptor filter (mode, threshold), reading normals)
CHAINS = {
    "trimmed": (dict(), None, None, False),
    "trimmed_scan": (dict(sum_order=icp.SUM_ORDER_SCAN), None, None, False),
    "trimmed_knn3": (dict(knn=3), None, None, False),
    "trimmed_knn3_scan": (dict(knn=3, sum_order=icp.SUM_ORDER_SCAN), None, None, False),
    "median": (dict(trim_ratio=0.5, quantile_scale=0.8), None, None, False),
    "maxdist": (dict(outlier_max_dist=0.3), None, None, False),
    "vartrim": (dict(), (0.3, 0.95, 2.0), None, False),
    "cauchy": (dict(trim_ratio=1.0, robust_fct=1), None, None, False),
    "tukey": (dict(trim_ratio=1.0, robust_fct=5, robust_tuning=2.0), None, None, False),
    "tukey_scan": (dict(trim_ratio=1.0, robust_fct=5, robust_tuning=2.0, sum_order=icp.SUM_ORDER_SCAN), None, None, False),
    "normals": (dict(normal_max_angle=0.5), None, None, True),
    "normals_knn3": (dict(normal_max_angle=0.5, knn=3), None, None, True),
    "gd_hard": (dict(), None, ("larger", 0.3), False),
    "gd_soft": (dict(), None, ("soft", None), False),
    "gd_soft_knn3": (dict(knn=3), None, ("soft", None), False),
    "p2point": (dict(error_minimizer=1), None, None, False),
    "p2point_scan": (dict(error_minimizer=1, sum_order=icp.SUM_ORDER_SCAN), None, None, False),
}


_ORACLES = {}


def _oracle(dtype):
    from oracle import Oracle
    key = np.dtype(dtype).name
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(dtype)
    return _ORACLES[key]


_SCENES = {}


def scene(kind):
    if kind not in _SCENES:
        if kind == "two":
            s = synth.make_two_scans(6000, rings=16)
            _SCENES[kind] = dict(ref=s["ref_xyz"], ref_nrm=s["ref_nrm"], rd=s["reading_xyz"], rd_nrm=s["reading_nrm"], T=s["T_init"])
        else:
            w = synth.make_scan_to_map(n_scan=4000, n_map=30000, n_queries=1, n_map_poses=3, rings=16)
            _SCENES[kind] = dict(ref=w.map_xyz, ref_nrm=w.map_nrm, rd=w.scans_xyz[0], rd_nrm=w.scans_nrm[0], T=w.T_init[0])
    return _SCENES[kind]


def map_values(m):
    u = synth.uniform01(77, m)
    return np.where(u < 0.2, 0.0, u)


def make_ctx(chain, dtype, sc, **over):
    prm, vt, gd, _ = CHAINS[chain]
    ctx = icp.Context(0, **dict(BASE, **prm, **over))
    if vt:
        ctx.set_var_trim(*vt)
    mid = ctx.set_map(sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype), center=True)
    if gd:
        ctx.set_descriptor_filter(*gd)
        ctx.set_map_values(mid, map_values(len(sc["ref"])).astype(dtype))
    return ctx, mid


def noise_of(xyz, dtype, sensor=0, gain=1.0):
    return _oracle(dtype).simple_sensor_noise(xyz.astype(dtype), sensor, gain)


def run(ctx, mid, chain, dtype, sc, noise, rd=None, rd_nrm=None):
    rd = sc["rd"] if rd is None else rd
    rd_nrm = sc["rd_nrm"] if rd_nrm is None else rd_nrm
    nr = rd_nrm.astype(dtype) if CHAINS[chain][3] else None
    return ctx.align(mid, rd.astype(dtype), sc["T"], normals=nr, noise=noise)


def bits(T, st):
    """everything an align returns, as bytes: for the bit-for-bit history comparisons"""
    keys = sorted(k for k in st if k != "cov")
    return T.tobytes() + st["cov"].tobytes() + repr([(k, st[k]) for k in keys]).encode()


def last_iteration_rotation(chain, dtype, sc, st, rd, rd_nrm):
    """R_iter of the call's last iteration (the transform after T_init, as the oracle's loop and the device keep it): what an
    align of the same inputs returns when it is stopped one iteration earlier, with R_init taken off"""
    if st["iterations"] <= 1:
        return np.eye(3)
    ctx, mid = make_ctx(chain, dtype, sc, max_iters=st["iterations"] - 1)
    T, s = run(ctx, mid, chain, dtype, sc, None, rd=rd, rd_nrm=rd_nrm)
    ctx.close()
    assert s["status"] == 0 and s["iterations"] == st["iterations"] - 1
    return T[:3, :3] @ np.asarray(sc["T"], dtype=np.float64)[:3, :3].T


def normal_filter_weights(chain, dtype, sc, st, ids, w, rd, rd_nrm):
    """SurfaceNormalOutlierFilter of the last iteration multiplied into w (orc_normal_weights), with the precondition that no
    candidate pair sits on the threshold (module text)"""
    o = _oracle(dtype)
    ang = dict(BASE, **CHAINS[chain][0])["normal_max_angle"]
    Ti = np.eye(4)
    Ti[:3, :3] = last_iteration_rotation(chain, dtype, sc, st, rd, rd_nrm)
    step_n = o.transform(Ti, o.transform(sc["T"], rd_nrm.astype(dtype), rotate_only=True), rotate_only=True)
    ref_n = sc["ref_nrm"].astype(dtype)
    k = 1 if ids.ndim == 1 else ids.shape[1]
    a = step_n.astype(np.float64)
    a = np.repeat(a / np.linalg.norm(a, axis=1, keepdims=True), k, axis=0)
    b = ref_n.astype(np.float64)[np.maximum(ids.reshape(-1), 0)]
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    cosv = np.einsum("ni,ni->n", a, b)
    cand = (np.asarray(w).reshape(-1) != 0) & (ids.reshape(-1) >= 0)
    edge = int(np.count_nonzero(cand & (np.abs(cosv - math.cos(ang)) <= 64 * np.finfo(dtype).eps)))
    out = o.normal_weights(step_n, ref_n, ids, ang, np.asarray(w).reshape(ids.shape))
    print(f"{chain} {np.dtype(dtype).name}: normal filter: {int(np.count_nonzero(cand))} candidates, "
          f"{int(np.count_nonzero(cand)) - int(np.count_nonzero(out))} dropped, {edge} on the threshold")
    assert edge == 0, "precondition of a fixed scene: no pair's cosine on the normal filter's threshold"
    return out.reshape(-1)


def reference_weights(ctx, mid, chain, dtype, sc, st, ids, d2, rd=None, rd_nrm=None):
    """the chain's weights for the call's last matches, from the oracle's own filters"""
    o = _oracle(dtype)
    prm, vt, gd, nrm = CHAINS[chain]
    p = dict(BASE, **prm)
    flat = np.ascontiguousarray(d2.reshape(-1))
    has = (ids.reshape(-1) >= 0) | (ids.reshape(-1) == -2)
    if p["robust_fct"]:
        w, _ = o.robust_weights(flat, p["robust_fct"], p["robust_tuning"], p["robust_scale"], p["robust_approx"])
        w = np.where(ids.reshape(-1) >= 0, w, 0).astype(dtype)
    elif vt:
        rc, w, _, _ = o.trim_weights(flat, ctx.last_var_trim_ratio(0))
        assert rc == 0
    elif p["quantile_scale"] != 1.0:
        w, _, _ = o.median_weights(flat, p["quantile_scale"])
    else:
        rc, w, _, _ = o.trim_weights(flat, p["trim_ratio"])
        assert rc == 0
    w = np.where(has, w, 0).astype(dtype)
    if p["outlier_max_dist"] > 0:
        md = dtype(p["outlier_max_dist"])
        w = np.where(flat <= md * md, w, 0).astype(dtype)
    if gd:
        v = map_values(len(sc["ref"])).astype(dtype)
        vi = np.where(ids.reshape(-1) >= 0, v[np.maximum(ids.reshape(-1), 0)], 0).astype(dtype)
        if gd[0] == "larger":
            g = (vi > dtype(gd[1])).astype(dtype)
        else:
            g = (vi / vi.max()).astype(dtype)
        w = (w * g).astype(dtype)
    if nrm:
        w = normal_filter_weights(chain, dtype, sc, st, ids, w, sc["rd"] if rd is None else rd, sc["rd_nrm"] if rd_nrm is None else rd_nrm)
    return w.reshape(d2.shape)


def check_against_reference(ctx, mid, chain, dtype, sc, st, noise, n):
    assert st["status"] == 0
    assert st["n_elements"] == st["n_kept"]
    count = round(st["overlap_noise"] * st["n_elements"])
    assert dtype(count) / dtype(st["n_elements"]) == dtype(st["overlap_noise"])
    ids, d2 = ctx.debug_last_matches(n, 0, dtype)
    w = reference_weights(ctx, mid, chain, dtype, sc, st, ids, d2)
    assert int(np.count_nonzero(w)) == st["n_kept"]
    lo, hi, nb, m = ref.count_bounds(d2, w, noise, dtype)
    near = ref.near_mean_pairs(d2, w, noise, dtype)
    seq = _oracle(dtype).sensor_noise_overlap(d2, w, noise)
    print(f"{chain} {np.dtype(dtype).name}: nb={nb} m*={m:.9g} count={count} lo={lo} hi={hi} near_mean={near} "
          f"oracle_seq={seq:.9g} device={st['overlap_noise']:.9g} overlap={st['overlap']:.6f}")
    assert nb == st["n_elements"]
    assert lo == hi, "precondition of a fixed scene: the band of reachable means must decide every pair the same way"
    assert count == lo
    assert abs(count - round(seq * nb)) <= near
    return count


# ---- the noise kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n", [1, 63, 4097, 1_000_000])
def test_simple_sensor_noise_kernel_is_the_oracles_bit_for_bit(dtype, n):
    import torch
    o = _oracle(dtype)
    ctx = icp.Context(0)
    r = synth.uniform(5 + n, 3 * n, -40.0, 40.0).reshape(n, 3)
    r[: min(n, 8)] *= 1e-3                                     # a few points inside minRadius' clamp
    xyz = r.astype(dtype)
    hom = np.ones((n, 4), dtype=dtype)
    hom[:, :3] = xyz
    for sensor in range(5):
        want = o.simple_sensor_noise(xyz, sensor, 1.5)
        got = ctx.simple_sensor_noise(xyz, sensor, 1.5)
        assert got.dtype == np.dtype(dtype) and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (sensor, "host -> host")
        got = ctx.simple_sensor_noise(hom, sensor, 1.5)                    # stride 4: a `features` matrix
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (sensor, "stride 4")
        if sensor in (0, 3):
            t = torch.from_numpy(xyz).cuda()
            got = ctx.simple_sensor_noise(t, sensor, 1.5)                  # device -> device
            torch.cuda.synchronize()
            assert got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8)), (sensor, "device -> device")
            out = np.empty(n, dtype=dtype)
            ctx.simple_sensor_noise(t, sensor, 1.5, out=out)               # device -> host
            assert np.array_equal(out.view(np.uint8), want.view(np.uint8)), (sensor, "device -> host")
            dout = torch.empty(n, dtype=t.dtype, device="cuda")
            ctx.simple_sensor_noise(xyz, sensor, 1.5, out=dout)            # host -> device
            assert np.array_equal(dout.cpu().numpy().view(np.uint8), want.view(np.uint8)), (sensor, "host -> device")
    with pytest.raises(icp.PgicpError) as e:
        ctx.simple_sensor_noise(xyz, 5, 1.0)
    assert e.value.code == icp.ERR_ARG
    with pytest.raises(icp.PgicpError) as e:
        ctx.simple_sensor_noise(xyz, -1, 1.0)
    assert e.value.code == icp.ERR_ARG
    ctx.close()


# ---- the overlap, single align, every chain: reference, oracle bound, history ---------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_overlap_of_a_single_align_and_its_history(chain, dtype):
    sc = scene("two")
    n = len(sc["rd"])
    noise = noise_of(sc["rd"], dtype)
    other = noise_of(sc["rd"], dtype, sensor=3, gain=4.0)
    ctx, mid = make_ctx(chain, dtype, sc)
    T1, s1 = run(ctx, mid, chain, dtype, sc, noise)
    check_against_reference(ctx, mid, chain, dtype, sc, s1, noise, n)
    assert set(s1) - {"overlap_noise", "n_elements"} == {"status", "iterations", "converged", "max_iter_reached", "overlap", "residual",
                                                       "trim_limit", "n_kept", "n_finite", "cov"}
    # twice in a row
    T2, s2 = run(ctx, mid, chain, dtype, sc, noise)
    assert bits(T1, s1) == bits(T2, s2)
    # an unarmed call after an armed one: what a fresh context returns, key for key; nothing left to read
    Tu, su = run(ctx, mid, chain, dtype, sc, None)
    fresh, fmid = make_ctx(chain, dtype, sc)
    Tf, sf = run(fresh, fmid, chain, dtype, sc, None)
    assert "overlap_noise" not in su and sorted(su) == sorted(sf)
    assert bits(Tu, su) == bits(Tf, sf)
    with pytest.raises(icp.PgicpError) as e:
        ctx.last_noise_overlap(0)
    assert e.value.code == icp.ERR_ARG
    # after an unarmed case
    T3, s3 = run(ctx, mid, chain, dtype, sc, noise)
    assert bits(T1, s1) == bits(T3, s3)
    # after a case armed with other noise (which gives another quantity, the same pose)
    To, so = run(ctx, mid, chain, dtype, sc, other)
    assert so["n_elements"] == s1["n_elements"] and To.tobytes() == T1.tobytes()
    T4, s4 = run(ctx, mid, chain, dtype, sc, noise)
    assert bits(T1, s1) == bits(T4, s4)
    # a fresh context gives the armed result too; a strided device row is the same row
    import torch
    mat = np.zeros((n, 3), dtype=dtype)
    mat[:, 1] = noise
    T5, s5 = run(fresh, fmid, chain, dtype, sc, torch.from_numpy(mat).cuda()[:, 1])
    assert bits(T1, s1) == bits(T5, s5)
    T6, s6 = run(fresh, fmid, chain, dtype, sc, mat[:, 1])
    assert bits(T1, s1) == bits(T6, s6)
    fresh.close()
    ctx.close()


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("chain", ["trimmed", "trimmed_knn3_scan", "tukey", "gd_soft", "p2point"])
def test_overlap_on_the_scan_to_map_scene(chain, dtype):
    sc = scene("map")
    noise = noise_of(sc["rd"], dtype)
    ctx, mid = make_ctx(chain, dtype, sc)
    T1, s1 = run(ctx, mid, chain, dtype, sc, noise)
    check_against_reference(ctx, mid, chain, dtype, sc, s1, noise, len(sc["rd"]))
    ctx.close()


def test_the_noise_branch_is_another_quantity_than_the_ratio():
    sc = scene("two")
    noise = noise_of(sc["rd"], F32)
    ctx, mid = make_ctx("trimmed", F32, sc)
    _, st = run(ctx, mid, "trimmed", F32, sc, noise)
    print("headline: overlap_noise", st["overlap_noise"], "weightedPointUsedRatio", st["overlap"])
    assert abs(st["overlap_noise"] - st["overlap"]) > 0.01
    ctx.close()


# ---- batches, the residual batch, the pair call -----------------------------------------------------------------------------
def ragged(sc, P):
    n = len(sc["rd"])
    cuts = [n, n - 1000, n // 2, n - 17, 3000, n - 2048, 2049, n - 1][:P]
    return [sc["rd"][:c] for c in cuts], [sc["rd_nrm"][:c] for c in cuts]


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("chain", ["trimmed", "trimmed_knn3_scan", "cauchy", "normals", "gd_soft"])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_batches_give_every_problem_the_single_aligns_overlap(chain, dtype, P):
    sc = scene("two")
    rds, nrms = ragged(sc, P)
    noises = [noise_of(r, dtype) for r in rds]
    if P >= 3:
        noises[1] = None                                   # a problem without noise among the others
    ctx, mid = make_ctx(chain, dtype, sc)
    with_nrm = CHAINS[chain][3]
    kw = dict(normals=[x.astype(dtype) for x in nrms]) if with_nrm else {}
    singles = []
    for p in range(P):
        singles.append(run(ctx, mid, chain, dtype, sc, noises[p], rd=rds[p], rd_nrm=nrms[p]))
    Tb, sb = ctx.align_batch(mid, [r.astype(dtype) for r in rds], [sc["T"]] * P, noises=noises, **kw)
    Tr, sr, res, ratio, rst = ctx.align_residual_batch([mid] * P, [r.astype(dtype) for r in rds], [sc["T"]] * P, noises=noises, **kw)
    for p in range(P):
        Ts, ss = singles[p]
        for got_T, got in ((Tb[p], sb[p]), (Tr[p], sr[p])):
            assert got["status"] == 0 and got_T.tobytes() == Ts.tobytes()
            if noises[p] is None:
                assert got["overlap_noise"] is None and got["n_elements"] is None
                with pytest.raises(icp.PgicpError) as e:
                    ctx.last_noise_overlap(p)
                assert e.value.code == icp.ERR_ARG
                continue
            # bit for bit the single align's: in the residual batch the reduction ran before the residual pass
            assert got["n_elements"] == ss["n_elements"] == got["n_kept"]
            assert np.float64(got["overlap_noise"]).tobytes() == np.float64(ss["overlap_noise"]).tobytes()
        assert np.isfinite(res[p]) and rst[p] == 0
    with pytest.raises(icp.PgicpError) as e:
        ctx.last_noise_overlap(P)
    assert e.value.code == icp.ERR_ARG
    with pytest.raises(icp.PgicpError) as e:
        ctx.last_noise_overlap(-1)
    assert e.value.code == icp.ERR_ARG
    # the batch twice in a row, and after an unarmed batch
    ctx.align_batch(mid, [r.astype(dtype) for r in rds], [sc["T"]] * P, **kw)
    Tb2, sb2 = ctx.align_batch(mid, [r.astype(dtype) for r in rds], [sc["T"]] * P, noises=noises, **kw)
    assert all(bits(Tb[p], sb[p]) == bits(Tb2[p], sb2[p]) for p in range(P))
    ctx.close()


@pytest.mark.parametrize("dtype", [F32, F64])
def test_icp_pair_carries_the_overlap(dtype):
    sc = scene("two")
    noise = noise_of(sc["rd"], dtype)
    ctx, mid = make_ctx("trimmed", dtype, sc)
    Ta, sa = run(ctx, mid, "trimmed", dtype, sc, noise)
    Tp, sp = ctx.icp_pair(sc["rd"].astype(dtype), sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype), sc["T"], noise=noise)
    assert bits(Ta, sa) == bits(Tp, sp)
    Tq, sq = ctx.icp_pair(sc["rd"].astype(dtype), sc["ref"].astype(dtype), sc["ref_nrm"].astype(dtype), sc["T"])
    assert "overlap_noise" not in sq and Tq.tobytes() == Tp.tobytes()
    ctx.close()


# ---- error exits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_error_exits_leave_the_context_usable(dtype):
    sc = scene("two")
    n = len(sc["rd"])
    noise = noise_of(sc["rd"], dtype)
    ctx, mid = make_ctx("trimmed", dtype, sc)
    T1, s1 = run(ctx, mid, "trimmed", dtype, sc, noise)
    rd = sc["rd"].astype(dtype)

    def refused(fn):
        with pytest.raises(icp.PgicpError) as e:
            fn()
        assert e.value.code == icp.ERR_ARG
        T, s = run(ctx, mid, "trimmed", dtype, sc, noise)          # the context works, and the refused call consumed the arm
        assert bits(T, s) == bits(T1, s1)

    bad = noise.copy()
    bad[n // 2] = -1e-3
    refused(lambda: ctx.align(mid, rd, sc["T"], noise=bad))
    bad[n // 2] = np.nan
    refused(lambda: ctx.align(mid, rd, sc["T"], noise=bad))
    bad[n // 2] = np.inf
    refused(lambda: ctx.align(mid, rd, sc["T"], noise=bad))
    import torch
    bad[n // 2] = -1.0
    refused(lambda: ctx.align(mid, rd, sc["T"], noise=torch.from_numpy(bad).cuda()))
    refused(lambda: ctx.align(mid, rd, sc["T"], noise=noise[:-1]))                      # another size than the reading's

    def wrong_P():
        ctx.arm_reading_noise([noise, noise], dtype)
        ctx.align(mid, rd, sc["T"])
    refused(wrong_P)

    def wrong_type():
        ctx.arm_reading_noise([noise.astype(F64 if dtype == F32 else F32)], F64 if dtype == F32 else F32)
        ctx.align(mid, rd, sc["T"])
    refused(wrong_type)
    # the refused call consumed the arm: the next unarmed call is an ordinary one
    def consumed():
        ctx.arm_reading_noise([noise, noise], dtype)
        with pytest.raises(icp.PgicpError):
            ctx.align(mid, rd, sc["T"])
        T, s = ctx.align(mid, rd, sc["T"])
        assert T.tobytes() == T1.tobytes()
        ctx.last_noise_overlap(0)
    refused(consumed)
    # calls that run no ICP leave the arm in place
    ctx.arm_reading_noise([noise], dtype)
    ctx.match(mid, rd, T=sc["T"])
    ctx.partial_chain(mid, rd, T=sc["T"])
    T, st = ctx.align(mid, rd, sc["T"])
    ov, nb = ctx.last_noise_overlap(0)
    assert (ov, nb) == (s1["overlap_noise"], s1["n_elements"]) and T.tobytes() == T1.tobytes()
    refused(lambda: ctx.last_noise_overlap(1))
    refused(lambda: ctx.last_noise_overlap(-1))
    # the last-call diagnostics check their problem index on the host
    refused(lambda: ctx.debug_last_matches(n, 1, dtype))
    refused(lambda: ctx.reading_order(n, 3))
    ctx.close()


# ---- sensor size ---------------------------------------------------------------------------------------------------------------
def test_overlap_at_100k_points_on_a_1m_point_map():
    dtype = F32
    w = synth.make_scan_to_map(n_scan=100_000, n_map=1_000_000, n_queries=1, n_map_poses=12, rings=64)
    sc = dict(ref=w.map_xyz, ref_nrm=w.map_nrm, rd=w.scans_xyz[0], rd_nrm=w.scans_nrm[0], T=w.T_init[0])
    noise = noise_of(sc["rd"], dtype)
    ctx, mid = make_ctx("trimmed", dtype, sc)
    T1, st = run(ctx, mid, "trimmed", dtype, sc, noise)
    assert st["status"] == 0 and st["n_elements"] == st["n_kept"]
    ids, d2 = ctx.debug_last_matches(len(sc["rd"]), 0, dtype)
    wts = reference_weights(ctx, mid, "trimmed", dtype, sc, st, ids, d2)
    lo, hi, nb, m = ref.count_bounds(d2, wts, noise, dtype)
    count = round(st["overlap_noise"] * nb)
    near = ref.near_mean_pairs(d2, wts, noise, dtype)
    seq = _oracle(dtype).sensor_noise_overlap(d2, wts, noise)
    print(f"100k x 1M: nb={nb} m*={m:.9g} count={count} lo={lo} hi={hi} near_mean={near} oracle_seq={seq:.9g} overlap={st['overlap']:.6f}")
    assert nb == st["n_elements"] and hi - lo <= 2 and lo <= count <= hi
    assert abs(count - round(seq * nb)) <= near
    T2, s2 = run(ctx, mid, "trimmed", dtype, sc, noise)
    assert bits(T1, st) == bits(T2, s2)
    ctx.close()
