"""MaxQuantileOnAxisDataPointsFilter on the device (include/pgicp_quantile.h): the stand-alone selection (pgicp_axis_quantile_*)
from host and from device memory, and filter type 8 in pgicp_filter_cloud* / pgicp_filter_cloud_dev* -- alone, with and without a
transformation, and mixed with the other types -- against the numpy statement (tests/axis_quantile_ref.py) on its scenes, bit for
bit.  The oracle's filter_chain does not know type 8: a mixed list's reference runs the oracle on the runs of old entries and the
numpy statement on the new ones, survivors in and survivors out."""
import numpy as np
import pytest

import axis_quantile_ref as ref
from pgslam_amd import icp, synth

pytestmark = pytest.mark.gpu

Q = icp.FILTER_MAX_QUANTILE_ON_AXIS


def chain_ref(o, filters, f):
    """the kept indices of a list that mixes old types (the oracle's) and type 8 (the numpy statement's)"""
    surv = np.arange(len(f))
    run = []
    for spec in list(filters) + [None]:
        if spec is not None and spec[0] != Q:
            run.append(spec)
            continue
        if run and len(surv):
            surv = surv[o.filter_chain(run, np.ascontiguousarray(f[surv]))]
        run = []
        if spec is not None and len(surv):
            surv = surv[ref.keep_mask(f[surv, int(spec[1])], spec[2])]
    return surv.astype(np.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_selection_from_host_and_device_memory(ctx, dtype):
    assert ref.rank(90, 0.7, dtype) == (63 if dtype == np.float32 else 62)
    last = None
    for sid, dim, f, ratio, (limit, k, below), _ in ref.scenes(dtype):
        if last is None or last[0] is not f:
            if last is not None:
                ctx.device_free(last[1])
            last = (f, ctx.device_cloud(f))
        for where, cloud in (("host", f), ("device", last[1])):
            gl, gk, gb = ctx.axis_quantile(cloud, dim, ratio)
            assert gl.dtype == dtype and ref.canonical(gl) == ref.canonical(limit), (sid, where, gl, limit)
            assert (gk, gb) == (k, below), (sid, where, gk, gb, k, below)
        if sid.startswith("mixed-n90@0.7"):
            assert k == (63 if dtype == np.float32 else 62)                  # the rank is rounded in T on the device too
    ctx.device_free(last[1])
    # an empty cloud: nothing happens
    gl, gk, gb = ctx.axis_quantile(np.zeros((0, 3), dtype=dtype), 0, 0.5)
    assert np.isnan(gl) and (gk, gb) == (0, 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_entry_keeps_what_the_statement_keeps(ctx, oracle32, oracle64, dtype):
    o = oracle32 if dtype == np.float32 else oracle64
    T = synth.se3(x=0.4, y=-0.2, z=1.1, yaw=0.3, pitch=0.05, roll=-0.02)
    for sid, dim, f, ratio, _, mask in ref.scenes(dtype):
        n = len(f)
        want = np.flatnonzero(mask).astype(np.int32)
        # descriptors: three rows that rotate with a transformation, three more, and an id row
        rows = np.clip(np.nan_to_num(f[:, :3][:, ::-1], nan=2.0), -3.0, 3.0) * dtype(0.5)
        d = np.concatenate([rows, np.arange(3 * n, dtype=dtype).reshape(n, 3), np.arange(n, dtype=dtype)[:, None]], axis=1).astype(dtype)
        filters = [(Q, dim, ratio)]
        of, od, idx, dev = ctx.filter_cloud(filters, f, d)
        assert np.array_equal(idx, want), sid
        assert dev.n == len(want) and same_bits(of, f[want]) and same_bits(od, d[want]), sid
        if n != 4097:
            continue                                                         # (the moved rows: one size, every value set and ratio)
        of, od, idx, dev = ctx.filter_cloud(filters, f, d, T=T, rotate_rows=(0, 3))
        assert np.array_equal(idx, want) and len(of) == len(want) and dev.n == len(want), sid
        clean = np.all(np.abs(f[want, :3]) < 1e30, axis=1)                       # (no NaN, and nothing the rotation could overflow)
        if clean.any():
            assert np.array_equal(of[clean, :3], o.transform(T, np.ascontiguousarray(f[want][clean, :3])))     # RigidTransformation: R p + t
        if len(want) == 0:
            continue
        assert same_bits(of[:, 3:], f[want][:, 3:])
        assert np.array_equal(od[:, 0:3], o.transform(T, d[want][:, 0:3], rotate_only=True))
        assert np.array_equal(od[:, 3:6], o.transform(T, d[want][:, 3:6], rotate_only=True))
        assert np.array_equal(od[:, 6], d[want][:, 6])


def scan_cloud(dtype, n=6000):
    w = synth.make_two_scans(n, rings=16)
    xyz = w["ref_xyz"].astype(dtype)
    f = np.concatenate([xyz, np.ones((len(xyz), 1), dtype=dtype)], axis=1)
    f[17, 1] = np.nan
    f[len(f) // 2 + 3, 3] = np.nan                              # (the homogeneous row: only RemoveNaN looks at it)
    f[123, 0] = np.nan
    return f


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lists_that_mix_old_and_new_types(ctx, oracle32, oracle64, dtype):
    o = oracle32 if dtype == np.float32 else oracle64
    f = scan_cloud(dtype)
    n = len(f)
    d = np.concatenate([f[:, :3] * dtype(2), np.arange(n, dtype=dtype)[:, None]], axis=1)
    d = np.nan_to_num(d, nan=5.0).astype(dtype)
    # bait for the box: points whose x lies far beyond every survivor's
    bait = f.copy()
    bait[::50, 0] = dtype(1e6)
    bait[7::50, 0] = dtype(-1e6)
    box = (icp.FILTER_BOUNDING_BOX, -500.0, -500.0, -500.0, 500.0, 500.0, 500.0, 0.0)
    lists = [
        (f, [(icp.FILTER_REMOVE_NAN,), (icp.FILTER_MAX_DIST, 25.0), (Q, 0, 0.9), (Q, 2, 0.8), (icp.FILTER_FIX_STEP, 2)]),
        (f, [(icp.FILTER_FIX_STEP, 3), (Q, 1, 0.7), (icp.FILTER_MAX_POINT_COUNT, 500, 11)]),
        (bait, [box, (Q, 0, 0.95)]),
        (f, [(Q, 2, 0.5), (Q, 2, 0.5), (icp.FILTER_MIN_DIST, 1.0), (Q, 0, 0.3)]),
        (f, [(icp.FILTER_MAX_DIST, 1e-3), (Q, 0, 0.5), (icp.FILTER_FIX_STEP, 2)]),       # the earlier entries drop everything
    ]
    for cloud, filters in lists:
        want = chain_ref(o, filters, cloud)
        of, od, idx, dev = ctx.filter_cloud(filters, cloud, d)
        assert np.array_equal(idx, want), filters
        assert same_bits(of, cloud[want]) and same_bits(od, d[want]) and dev.n == len(want)
    # the limit of the bait list is that of the box's survivors: every kept x is an ordinary one
    want = chain_ref(o, lists[2][1], bait)
    assert 0 < len(want) < n and np.abs(bait[want, 0]).max() < 500 and len(chain_ref(o, lists[4][1], f)) == 0
    # after a list that kept nothing the context is as usable as before
    of, _, idx, _ = ctx.filter_cloud(lists[0][1], f, None)
    assert np.array_equal(idx, chain_ref(o, lists[0][1], f))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_only_pass_with_a_quantile_entry(ctx, oracle32, oracle64, dtype):
    o = oracle32 if dtype == np.float32 else oracle64
    chain = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
    w = synth.make_scan_to_map(n_scan=6000, n_map=40_000, n_queries=1, n_map_poses=4, rings=16)
    f = np.concatenate([w.scans_xyz[0], np.ones((len(w.scans_xyz[0]), 1), dtype=np.float32)], axis=1).astype(dtype)
    f[11, 0] = np.nan
    before = f.copy()
    for filters in ([(icp.FILTER_REMOVE_NAN,), (icp.FILTER_MAX_DIST, 35.0), (Q, 0, 0.9)],
                    [(Q, 2, 0.998)],
                    [(Q, 1, 0.5)]):                                              # (half the cloud dropped: more than the list holds)
        kept, dev, dropped = ctx.filter_cloud_dev(filters, f, dropped_cap=1024)
        want = chain_ref(o, filters, f)
        assert kept == len(want) and np.array_equal(f.view(np.uint8), before.view(np.uint8))
        if len(f) - kept > 1024:
            assert dropped is None
            continue
        assert np.array_equal(dropped, np.setdiff1d(np.arange(len(f)), want))
        ctx.set_params(**chain)
        mid = ctx.set_map(w.map_xyz.astype(dtype), w.map_nrm.astype(dtype), center=True, dtype=dtype)
        Ta, sa = ctx.align(mid, dev, w.T_init[0], dtype=dtype)
        Tb, sb = ctx.align(mid, np.ascontiguousarray(f[want][:, :3]), w.T_init[0], dtype=dtype)
        assert np.array_equal(Ta, Tb) and sa["iterations"] == sb["iterations"] and sa["n_kept"] == sb["n_kept"]
        ctx.destroy_map(mid)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals_leave_the_context_usable(ctx, oracle32, oracle64, dtype):
    o = oracle32 if dtype == np.float32 else oracle64
    f = scan_cloud(dtype, 2000)
    good = [(icp.FILTER_REMOVE_NAN,), (Q, 0, 0.9)]
    for bad in ((Q, 3, 0.5), (Q, -1, 0.5), (Q, 0.5, 0.5), (Q, 0, 0.0), (Q, 0, 1.0), (Q, 0, float("nan")), (Q, 0, float("inf")), (Q, 0, -0.5), (99,)):
        for call in (lambda fl: ctx.filter_cloud(fl, f, None), lambda fl: ctx.filter_cloud_dev(fl, f)):
            with pytest.raises(icp.PgicpError) as e:
                call([(icp.FILTER_REMOVE_NAN,), bad])
            assert e.value.code == icp.ERR_ARG
            _, _, idx, _ = ctx.filter_cloud(good, f, None)
            assert np.array_equal(idx, chain_ref(o, good, f))
    for dim, ratio in ((3, 0.5), (0, 0.0), (0, 1.0), (0, float("nan"))):
        with pytest.raises(icp.PgicpError) as e:
            ctx.axis_quantile(f, dim, ratio)
        assert e.value.code == icp.ERR_ARG
    limit, k, below = ctx.axis_quantile(f, 1, 0.5)
    assert (ref.canonical(limit), k, below) == (ref.canonical(ref.select(f[:, 1], 0.5)[0]),) + ref.select(f[:, 1], 0.5)[1:]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_state_leaks_through_the_scratch(ctx, dtype):
    f = scan_cloud(dtype)
    other = next(s for s in ref.scenes(dtype) if s[0].startswith("planar-n65537@0.5"))
    a = [(icp.FILTER_REMOVE_NAN,), (Q, 0, 0.9), (Q, 2, 0.8)]
    first = ctx.filter_cloud(a, f, None)
    second = ctx.filter_cloud(a, f, None)
    # (four sets of scratch are used in turn: enough different calls in between to come round to every one of them)
    for _ in range(4):
        ctx.filter_cloud([(Q, other[1], other[3])], other[2], None)
        ctx.filter_cloud([(Q, 1, 0.3)], f, None)
    third = ctx.filter_cloud(a, f, None)
    for r in (second, third):
        assert np.array_equal(r[2], first[2]) and same_bits(r[0], first[0])
    q1 = ctx.axis_quantile(f, 0, 0.9)
    ctx.axis_quantile(other[2], other[1], other[3])
    q2 = ctx.axis_quantile(f, 0, 0.9)
    assert (ref.canonical(q1[0]),) + q1[1:] == (ref.canonical(q2[0]),) + q2[1:]
