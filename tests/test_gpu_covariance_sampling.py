"""[EXT] CovarianceSamplingDataPointsFilter on the device (include/pgicp_covsample.h) against tests/covariance_sampling_ref.py:
the framed call's picks exactly, the full call's frame within the derived tolerances and its picks and rows exactly given that
frame, the no-op, every refusal, the shared scratch next to the other filters, and an ICP of a filtered corridor reading.

Frame tolerances (derived: one rounding to T per entry, six entries a row, eigenvalues <= trace, about 10 over that):
|c - c_ref| <= eps max|x|, |L - L_ref| <= 4 eps L_ref, max|X^T X - I| <= 64 eps, max|C_ref X - X diag(lambda)| <= 64 eps trace(C_ref);
tests/test_covariance_sampling_host.py checks that numpy's eigh basis rounded to T is inside them on these clouds."""
import functools

import numpy as np
import pytest

import covariance_sampling_ref as ref
from pgslam_amd import icp
from test_covariance_sampling_host import KINDS, SIZES, case_frame, nb_samples

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


@functools.lru_cache(maxsize=None)
def framed_case(kind, n, T):
    """(xyz, normals, frame, {nb: picks}): the reference of a cloud, computed once for the numpy and the torch run"""
    x, nr = ref.cloud(kind, n, T)
    fr = case_frame(x, nr, T)
    return x, nr, fr, {nb: ref.select(x, nr, nb, fr, T) for nb in nb_samples(n)}


def to_torch(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def host(a):
    return a.cpu().numpy() if icp._is_torch(a) else np.asarray(a)


@pytest.mark.parametrize("use_torch", [False, True])
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_framed_call_is_exact(ctx, kind, T, use_torch):
    for n in SIZES:
        x, nr, fr, want = framed_case(kind, n, T)
        dx, dn = to_torch(x, nr) if use_torch else (x, nr)
        for nb, picks in want.items():
            g = ctx.covariance_sampling(dx, dn, nb_sample=nb, frame=fr)
            if use_torch:
                assert g["kept_idx"].is_cuda and g["xyz"].is_cuda
            np.testing.assert_array_equal(host(g["kept_idx"]), picks, err_msg=f"{kind} n {n} nb {nb}")


@pytest.mark.parametrize("T", DTYPES)
def test_framed_call_at_sensor_size(ctx, T):
    x, nr = ref.cloud("room", 100_000, T)
    fr = ref.frame(x, nr, 1, T)
    g = ctx.covariance_sampling(x, nr, nb_sample=5000, frame=fr)
    np.testing.assert_array_equal(g["kept_idx"], ref.select(x, nr, 5000, fr, T))


@pytest.mark.parametrize("use_torch", [False, True])
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("kind", KINDS + ("corridor",))
def test_full_call(ctx, kind, T, use_torch):
    rng = np.random.default_rng(3)
    for n, nb in ((65, 6), (2049, 1024), (8193, 500)):
        x, nr = ref.cloud(kind, n, T)
        desc = rng.normal(size=(n, 2)).astype(T)
        dx, dn, dd = to_torch(x, nr, desc) if use_torch else (x, nr, desc)
        for tn in (0, 1, 2):
            want_fr = ref.frame(x, nr, tn, T)
            g = ctx.covariance_sampling(dx, dn, nb_sample=nb, torque_norm=tn, descriptors=dd)
            for value, bound in ref.frame_bounds_ok(g["frame"], want_fr, x, T):
                print(kind, n, tn, value, bound)
                assert value <= bound, (kind, n, tn, value, bound)
            picks = ref.select(x, nr, nb, g["frame"], T)             # the device's own frame: no basis of the test's own
            if use_torch:
                assert all(g[k].is_cuda for k in ("xyz", "normals", "descriptors", "kept_idx"))
            np.testing.assert_array_equal(host(g["kept_idx"]), picks, err_msg=f"{kind} n {n} torque {tn}")
            np.testing.assert_array_equal(host(g["xyz"]), x[picks])
            np.testing.assert_array_equal(host(g["normals"]), nr[picks])
            np.testing.assert_array_equal(host(g["descriptors"]), desc[picks])


@pytest.mark.parametrize("T", DTYPES)
def test_gather_at_its_block_edge(ctx, T):
    """one pick, a full block of 256, one pick into the second block, and the identity path (nbSample = n), 3 descriptor rows"""
    x, nr = ref.cloud("room", 300, T)
    desc = np.random.default_rng(5).normal(size=(300, 3)).astype(T)
    for nb in (1, 256, 257, 300):
        g = ctx.covariance_sampling(x, nr, nb_sample=nb, descriptors=desc)
        picks = ref.select(x, nr, nb, g["frame"], T) if nb < 300 else np.arange(300)
        assert len(g["kept_idx"]) == nb
        np.testing.assert_array_equal(g["kept_idx"], picks, err_msg=f"nb {nb}")
        np.testing.assert_array_equal(g["xyz"], x[picks])
        np.testing.assert_array_equal(g["normals"], nr[picks])
        np.testing.assert_array_equal(g["descriptors"], desc[picks])


@pytest.mark.parametrize("T", DTYPES)
def test_noop_when_nb_sample_reaches_n(ctx, T):
    x, nr = ref.cloud("room", 300, T)
    for nb in (300, 301, 5000):
        for fr in (None, ref.frame(x, nr, 1, T)):
            g = ctx.covariance_sampling(x, nr, nb_sample=nb, frame=fr)
            np.testing.assert_array_equal(g["kept_idx"], np.arange(300))
            np.testing.assert_array_equal(g["xyz"], x)
            np.testing.assert_array_equal(g["normals"], nr)
    e = ctx.covariance_sampling(np.zeros((0, 3), T), np.zeros((0, 3), T), nb_sample=5)
    assert len(e["kept_idx"]) == 0 and len(e["xyz"]) == 0


@pytest.mark.parametrize("T", DTYPES)
def test_every_refusal_leaves_the_context_usable(ctx, T):
    x, nr = ref.cloud("room", 500, T)
    fr = ref.frame(x, nr, 1, T)
    good = ref.select(x, nr, 50, fr, T)

    def refused(**kw):
        args = dict(xyz=x, normals=nr, nb_sample=50)
        args.update(kw)
        with pytest.raises(icp.PgicpError) as e:
            ctx.covariance_sampling(args.pop("xyz"), args.pop("normals"), **args)
        assert e.value.code == icp.ERR_ARG
        np.testing.assert_array_equal(ctx.covariance_sampling(x, nr, nb_sample=50, frame=fr)["kept_idx"], good)

    refused(nb_sample=0)
    refused(nb_sample=-4)
    refused(torque_norm=3)
    refused(torque_norm=-1)
    for bad in (np.nan, np.inf, -np.inf):
        for arr in ("xyz", "normals"):
            a = (x if arr == "xyz" else nr).copy()
            a[317, 1] = bad
            refused(**{arr: a})
            refused(**{arr: a}, frame=fr)
    refused(frame=dict(fr, L=0.0))
    refused(frame=dict(fr, L=-1.0))
    refused(frame=dict(fr, L=np.nan))
    refused(xyz=np.tile(x[:1], (500, 1)))                    # every point at the mean: L = 0
    # through the C ABI: n < 0, strides below 3, desc without out_desc
    import ctypes as C
    fn = getattr(ctx.lib, "pgicp_covariance_sampling" + ctx._sfx(np.dtype(T)))
    idx, n_out = np.empty(50, np.int32), C.c_int(0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda n=500, xs=3, ns=3, desc=None, drows=0: fn(ctx.h, p(x), C.c_int(xs), p(nr), C.c_int(ns), C.c_int(n), C.c_int(icp.HOST), C.c_int(50),
                                                             C.c_int(1), desc, C.c_int(drows), None, None, C.c_int(3), None, p(idx), C.byref(n_out), None)
    assert call(n=-1) == icp.ERR_ARG and call(xs=2) == icp.ERR_ARG and call(ns=2) == icp.ERR_ARG and call(desc=p(x), drows=3) == icp.ERR_ARG
    assert call() == icp.OK and n_out.value == 50
    np.testing.assert_array_equal(idx, ctx.covariance_sampling(x, nr, nb_sample=50)["kept_idx"])
    assert call(n=0) == icp.OK and n_out.value == 0


@pytest.mark.parametrize("T", DTYPES)
def test_alternation_with_the_other_filters_on_one_context(ctx, T):
    """the dpf scratch is shared with voxel_grid and normals_max_density: each call's result is the one it gives alone"""
    x, nr = ref.cloud("room", 4097, T)
    fr = ref.frame(x, nr, 1, T)
    want = ref.select(x, nr, 700, fr, T)
    vox = ctx.voxel_grid(x, v_size=(0.5, 0.5, 0.5))
    nmd = ctx.normals_max_density(x, knn=8, max_density=50.0)
    for _ in range(2):
        np.testing.assert_array_equal(ctx.covariance_sampling(x, nr, nb_sample=700, frame=fr)["kept_idx"], want)
        v2 = ctx.voxel_grid(x, v_size=(0.5, 0.5, 0.5))
        np.testing.assert_array_equal(v2["xyz"], vox["xyz"])
        np.testing.assert_array_equal(v2["kept_idx"], vox["kept_idx"])
        g = ctx.covariance_sampling(x, nr, nb_sample=700, torque_norm=2)
        np.testing.assert_array_equal(g["kept_idx"], ref.select(x, nr, 700, g["frame"], T))
        m2 = ctx.normals_max_density(x, knn=8, max_density=50.0)
        np.testing.assert_array_equal(m2["kept_idx"], nmd["kept_idx"])
        np.testing.assert_array_equal(m2["normals"], nmd["normals"])


def test_corridor_reading_aligns_as_the_oracle_says(oracle32):
    """a corridor reading (two long walls, a floor, one short end wall), filtered on the device, against a map of the same
    corridor: the device ICP returns the oracle's pose for the same filtered reading, to the parity tests' tolerance"""
    from pgslam_amd import synth
    T = np.float32
    mx, mn = ref.cloud("corridor", 20000, T)
    rx, rn = ref.cloud("corridor", 6001, T)
    truth = synth.se3(x=0.05, y=-0.03, yaw=0.01)
    rx = (rx.astype(np.float64) - truth[:3, 3]) @ truth[:3, :3]
    rx, rn = rx.astype(T), (rn.astype(np.float64) @ truth[:3, :3]).astype(T)
    chain = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
    c = icp.Context(0, **chain)
    try:
        g = c.covariance_sampling(rx, rn, nb_sample=1500)
        assert len(g["kept_idx"]) == 1500
        mid = c.set_map(mx, mn, center=True)
        Tm, st = c.align(mid, g["xyz"], np.eye(4))
        c.destroy_map(mid)
    finally:
        c.close()
    o = oracle32.icp(np.ascontiguousarray(g["xyz"]), mx, mn, np.eye(4), **chain)
    d = np.linalg.inv(o["T"]) @ Tm
    dt = float(np.linalg.norm(d[:3, 3]))
    dr = float(np.arccos(min(1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0)))
    assert st["status"] == 0 and o["status"] == 0
    assert dt < 1e-5 and dr < 1e-5, (dt, dr)
    assert st["iterations"] == o["iterations"]
