"""pgicp_sensor_chain_* on the device (include/pgicp_sensor_chain.h, k_sensor_chain.inc) against the numpy statement
(tests/sensor_chain_ref.py, pinned on the CPU by tests/test_sensor_chain_host.py): every row and the kept indices bit for bit, no
tolerance anywhere, in both precisions, from host and from device memory; against today's separate calls; the refusals.

A normal of zero cannot reach Shadow through this call: the head makes the normals, and it never makes a zero one (a point with
fewer than three neighbours gets (0, 1, 0)).  The guarded normalisation of a zero normal is checked where it can be reached -- the
per-point function the kernel calls, tests/cpp/test_sensor_chain_cpu.cpp."""
import ctypes as C

import numpy as np
import pytest

import sensor_chain_ref as ref
from pgslam_amd import icp

ALL = ("normals", "eigen_values", "densities")


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def check(ctx, xyz, T, stages, device, label, keep=ALL, desc=None, max_dist=np.inf):
    """one call against the statement; returns (got, want)"""
    import torch
    # (numpy gives an empty array zero strides, which from_numpy would carry over: an empty tensor is made by torch)
    to = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if len(a) else torch.zeros(a.shape, dtype=getattr(torch, a.dtype.name), device="cuda")) \
        if device else (lambda a: a)
    want = ref.run(xyz, T, stages, max_dist=max_dist, keep=keep, desc=desc)
    got = ctx.sensor_chain(to(xyz), ref.KNN, max_dist, stages, keep=keep, desc=None if desc is None else to(desc), mem="device" if device else "host")
    assert got["count"] == want["count"], (label, got["count"], want["count"])
    for key in ref.ROWS:
        if want[key] is None:
            assert got[key] is None, (label, key)
            continue
        assert got[key] is not None and (hasattr(got[key], "is_cuda") and got[key].is_cuda) == device, (label, key)
        g = got[key].cpu().numpy() if device else got[key]
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (label, key, g.dtype, g.shape)
        assert bits(g) == want[key].tobytes(), (label, key)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_sizes_across_the_wave_and_the_scan_block(ctx, T, device):
    for n in ref.SIZES:
        x = ref.sized_cloud(n, T) if n else np.zeros((0, 3), dtype=T)
        md = ref.pick_max_density(x, T) if n else 10.0
        lists = ref.stage_lists(md)
        for name in ("six", "md_before_shadow", "no_drop", "head_only") if n not in (65, 4097) else lists:
            _, want = check(ctx, x, T, lists[name], device, f"n={n} {name}")
        if n >= 63:
            six = ref.run(x, T, lists["six"])
            assert 0 < six["passed"][ref.SHADOW] < n and 0 < six["count"] < six["passed"][ref.SHADOW], n


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_main_scene_every_stage_list(ctx, T, device):
    x = ref.scene(ref.MAIN_N, T)
    lists = ref.stage_lists(ref.pick_max_density(x, T))
    res = {name: check(ctx, x, T, st, device, name)[1] for name, st in lists.items()}
    # the rank rule: MaxDensity behind Shadow draws with the survivors' ranks, ahead of it with the input indices
    a, b = res["md_before_shadow"], res["md_after_shadow"]
    assert a["count"] != b["count"] and not np.array_equal(a["kept_idx"], b["kept_idx"])
    both = np.intersect1d(a["kept_idx"], b["kept_idx"])
    assert 0 < len(both) < min(a["count"], b["count"])
    for name in ("six", "md_after_shadow", "orient_after_drops"):
        r = res[name]
        assert 0.1 < r["passed"][ref.SHADOW] / r["arrived"][ref.SHADOW] < 0.9 and 0.1 < r["passed"][ref.MAXDENS] / r["arrived"][ref.MAXDENS] < 0.9
    # OrientNormals does flip some normals and not others, both ways
    h = ref.head(x, T)["normals"]
    for name in ("orient", "orient_away"):
        flipped = np.any(res[name]["normals"] != h, axis=1)
        assert 0 < np.count_nonzero(flipped) < len(x), name
    # with fewer rows kept: the stages that need no row still run, and the strided (n, 4) cloud gives the same bits
    check(ctx, x, T, [(ref.NOISE, 0, 1.0), (ref.OBS, 1.0, 2.0, 3.0)], device, "no rows", keep=())
    check(ctx, x, T, [(ref.SHADOW, ref.EPS)], device, "normals only", keep=("normals",))
    x4 = np.ones((len(x), 4), dtype=T)
    x4[:, :3] = x
    check(ctx, x4, T, lists["six"], device, "stride 4")


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_edges_of_the_dropping_stages(ctx, T):
    x = ref.scene(ref.MAIN_N, T)
    md = ref.pick_max_density(x, T)
    for device in (False, True):
        # a Shadow that drops every point: sin(pi / 2) = 1 in T, and no |cosine| exceeds it here; MaxDensity behind it sees an empty cloud
        for st in ([(ref.SHADOW, float(np.pi / 2))], [(ref.OBS,) + ref.CENTER, (ref.ORIENT, 1), (ref.SHADOW, float(np.pi / 2)), (ref.MAXDENS, md, 3), (ref.NOISE, 0, 1.0)]):
            _, want = check(ctx, x, T, st, device, "shadow drops all")
            assert want["count"] == 0
        # a Shadow that keeps every point (eps = 0): nothing here is exactly perpendicular
        _, want = check(ctx, x, T, [(ref.SHADOW, 0.0), (ref.MAXDENS, md, 3)], device, "shadow keeps all")
        assert want["passed"][ref.SHADOW] == len(x)
    # every density saturated: 40 copies of each point, every neighbour coincides, every density is +inf = the largest: the integer
    # factor 1 - saturated / n is 0 over the survivors too (n is their number, not the cloud's)
    rng = np.random.default_rng(11)
    base = np.round(rng.normal(size=(300, 3)) * 3 * 64) / 64 + np.array([4.0, 0.0, 0.0])
    dup = np.ascontiguousarray(np.repeat(base, 40, axis=0)[rng.permutation(12000)], dtype=T)
    for st in ([(ref.MAXDENS, 100.0, 3)], [(ref.SHADOW, ref.EPS), (ref.MAXDENS, 100.0, 3)], [(ref.MAXDENS, 100.0, 3), (ref.SHADOW, ref.EPS)]):
        _, want = check(ctx, dup, T, st, False, "saturated")
        assert want["count"] == 0 and (st[0][0] != ref.SHADOW or 0 < want["passed"][ref.SHADOW] < len(dup))
    # a point at the origin (its position is not normalised: the cosine is 0, the comparison drops it unless ... it cannot be kept),
    # and isolated points under a finite maxDist (density +inf, the normal (0, 1, 0))
    y = ref.sized_cloud(4097, T)
    y[100] = 0
    y[7] = [50, 50, 50]
    for device in (False, True):
        _, want = check(ctx, y, T, ref.six(ref.pick_max_density(y, T)), device, "origin", max_dist=2.0)
        assert 100 not in want["kept_idx"] and 0 < want["count"] < len(y)
        _, want = check(ctx, y, T, [(ref.SHADOW, 0.0)], device, "origin eps 0", max_dist=2.0)
        assert 100 not in want["kept_idx"] and 7 in want["kept_idx"]


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_against_the_separate_calls(ctx, T):
    import torch
    x = np.ones((ref.MAIN_N, 4), dtype=T)
    x[:, :3] = ref.scene(ref.MAIN_N, T)
    desc = np.random.default_rng(5).normal(size=(len(x), 2)).astype(T)
    md = ref.pick_max_density(x, T)
    for device in (False, True):
        to = (lambda a: torch.from_numpy(a).cuda()) if device else (lambda a: a)
        h = ctx.sensor_chain(to(x), ref.KNN, np.inf, [], keep=ALL)
        s = ctx.surface_densities(to(x), knn=ref.KNN)
        assert h["count"] == len(x) and bits(h["kept_idx"]) == np.arange(len(x), dtype=np.int32).tobytes() and bits(h["xyz"]) == x[:, :3].tobytes()
        for key in ALL:
            assert bits(h[key]) == bits(s[key]), key
        nrm, eig = ctx.surface_normals(np.ascontiguousarray(x[:, :3]), knn=ref.KNN, want_eigen=True)
        assert bits(h["normals"]) == nrm.tobytes() and bits(h["eigen_values"]) == eig.tobytes()
        f = ctx.sensor_chain(to(x), ref.KNN, np.inf, [(ref.MAXDENS, md, 9)], keep=ALL, desc=to(desc))
        o = ctx.normals_max_density(to(x), knn=ref.KNN, max_density=md, seed=9, descriptors=to(desc))
        assert 0 < f["count"] < len(x)
        for key in ("xyz", "normals", "eigen_values", "densities", "descriptors", "kept_idx"):
            assert bits(f[key]) == bits(o[key]), key
        noise = ctx.sensor_chain(to(x), ref.KNN, np.inf, [(ref.NOISE, 4, 1.5)], keep=())["noise"]
        assert bits(noise) == bits(ctx.simple_sensor_noise(np.ascontiguousarray(x[:, :3]), sensor_type=4, gain=1.5))


@pytest.mark.gpu
@pytest.mark.parametrize("drows", [1, 5])
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_descriptor_rows_travel_with_the_kept_points(ctx, T, drows):
    x = ref.sized_cloud(8193, T)
    desc = np.random.default_rng(drows).normal(size=(len(x), drows)).astype(T)
    st = ref.six(ref.pick_max_density(x, T))
    for device in (False, True):
        got, want = check(ctx, x, T, st, device, f"drows={drows}", desc=desc)
        assert 0 < want["count"] < len(x) and want["descriptors"].shape == (want["count"], drows)


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_device_outputs_feed_a_device_map(T):
    import torch
    from pgslam_amd import synth
    w = synth.make_two_scans(6000, rings=16)
    rf, rd = np.ascontiguousarray(w["ref_xyz"], dtype=T), np.ascontiguousarray(w["reading_xyz"], dtype=T)
    st = ref.six(ref.pick_max_density(rf, T))
    c = icp.Context(0, max_dist=2.0, trim_ratio=0.85, max_iters=20)
    try:
        fd = c.sensor_chain(torch.from_numpy(rf).cuda(), ref.KNN, np.inf, st)
        fh = c.sensor_chain(rf, ref.KNN, np.inf, st)
        assert 0 < fh["count"] < len(rf) and bits(fd["xyz"]) == fh["xyz"].tobytes() and bits(fd["normals"]) == fh["normals"].tobytes()
        res = []
        for xx, nr in ((fd["xyz"], fd["normals"]), (np.ascontiguousarray(fh["xyz"]), fh["normals"])):
            mid = c.set_map(xx, nr, center=True)
            Tm, s = c.align(mid, rd, w["T_init"])
            c.destroy_map(mid)
            res.append((Tm.tobytes(), s["iterations"], s["residual"], s["n_kept"]))
        assert res[0] == res[1]
    finally:
        c.close()


def raw_call(ctx, T, x, stages, knn=ref.KNN, max_dist=1e300, keep=(1, 1, 1), n_stages=None, out_nrm=True, out_dens=True, out_obs=False, out_noise=False):
    """the C call itself with host memory: (status, n_out)"""
    n = len(x)
    arr = ctx.chain_stages(stages)
    mk = lambda w: np.empty((max(n, 1), w), dtype=T)
    ox, on, oe, od, ob, oz = mk(3), mk(3), mk(3), mk(1), mk(3), mk(1)
    idx = np.empty(max(n, 1), dtype=np.int32)
    n_out = C.c_int(-5)
    p = lambda a, want=True: C.c_void_p(a.ctypes.data) if want else None
    fn = getattr(ctx.lib, "pgicp_sensor_chain" + ("_f32" if T == np.float32 else "_f64"))
    st = fn(ctx.h, p(x), C.c_int(3), C.c_int(n), C.c_int(icp.HOST), C.c_int(knn), C.c_double(max_dist), C.c_int(keep[0]), C.c_int(keep[1]),
            C.c_int(keep[2]), C.c_int(len(stages) if n_stages is None else n_stages), arr, None, C.c_int(0), p(ox), p(on, out_nrm), C.c_int(3),
            p(oe, bool(keep[1])), p(od, out_dens), p(ob, out_obs), p(oz, out_noise), None, p(idx), C.byref(n_out))
    return st, n_out.value


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_argument_refusals_leave_the_context_usable(ctx, T):
    x = ref.sized_cloud(300, T)
    obs, orient, sh, md, nz = (ref.OBS, 0, 0, 0), (ref.ORIENT, 1), (ref.SHADOW, 0.2), (ref.MAXDENS, 5.0, 1), (ref.NOISE, 0, 1.0)
    ok = lambda *a, **k: raw_call(ctx, T, x, *a, **k)[0]
    assert ok([nz, obs, orient, sh, md]) == icp.OK
    bad = [
        dict(stages=[nz] * 9),                                             # more than PGICP_CHAIN_MAX_STAGES
        dict(stages=[(0,)]), dict(stages=[(6,)]), dict(stages=[(-1,)]),    # an unknown stage type
        dict(stages=[sh, obs, sh]), dict(stages=[obs, obs]), dict(stages=[md, md]), dict(stages=[nz, nz]), dict(stages=[obs, orient, orient]),
        dict(stages=[orient]), dict(stages=[orient, obs]),                 # no observation direction before it
        dict(stages=[obs, orient], keep=(0, 0, 1), out_nrm=False),         # no normals
        dict(stages=[sh], keep=(0, 0, 1), out_nrm=False),
        dict(stages=[md], keep=(1, 0, 0), out_dens=False),                 # no densities
        dict(stages=[(ref.SHADOW, -1e-9)]), dict(stages=[(ref.SHADOW, 3.1416)]), dict(stages=[(ref.SHADOW, float("nan"))]),
        dict(stages=[(ref.MAXDENS, 0.0, 1)]), dict(stages=[(ref.MAXDENS, -1.0, 1)]), dict(stages=[(ref.MAXDENS, float("nan"), 1)]),
        dict(stages=[(ref.MAXDENS, 5.0, 2.0 ** 53)]), dict(stages=[(ref.MAXDENS, 5.0, -1.0)]),
        dict(stages=[(ref.NOISE, 5, 1.0)]), dict(stages=[(ref.NOISE, -1, 1.0)]), dict(stages=[(ref.NOISE, 1.5, 1.0)]),
        dict(stages=[], knn=2), dict(stages=[], knn=33), dict(stages=[], max_dist=0.0), dict(stages=[], max_dist=float("nan")),
        dict(stages=[obs], n_stages=-1),
        dict(stages=[], keep=(0, 0, 1)),                                   # out_nrm handed in, the row not kept
        dict(stages=[], out_obs=True), dict(stages=[], out_noise=True),    # a row whose stage is not listed
    ]
    for k in bad:
        assert ok(**k) == icp.ERR_ARG, k
        assert ctx.lib.pgicp_last_error(ctx.h)
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[37, 1] = v
        assert raw_call(ctx, T, y, [sh])[0] == icp.ERR_ARG
    fn = getattr(ctx.lib, "pgicp_sensor_chain" + ("_f32" if T == np.float32 else "_f64"))
    n_out = C.c_int(-5)
    assert fn(ctx.h, C.c_void_p(x.ctypes.data), C.c_int(3), C.c_int(-1), C.c_int(icp.HOST), C.c_int(10), C.c_double(1.0), C.c_int(1), C.c_int(0), C.c_int(1),
              C.c_int(0), None, None, C.c_int(0), C.c_void_p(x.ctypes.data), None, C.c_int(3), None, None, None, None, None, None, C.byref(n_out)) == icp.ERR_ARG
    assert raw_call(ctx, T, x[:0], [sh, md]) == (icp.OK, 0)                # n == 0
    with pytest.raises(icp.PgicpError) as e:
        ctx.sensor_chain(x, ref.KNN, np.inf, [orient])
    assert e.value.code == icp.ERR_ARG
    # the PI of the header is accepted, and the context is usable after the refusals
    assert ok([(ref.SHADOW, 3.14159265358979323846)]) == icp.OK
    check(ctx, x, T, [nz, obs, orient, sh, md], False, "after the refusals")
