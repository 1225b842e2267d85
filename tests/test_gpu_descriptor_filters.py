"""pgicp_sensor_chain_ext_* and entry 9 of pgicp_filter_cloud_* on the device (include/pgicp_descriptor_filters.h, k_sensor_chain.inc,
k_filter.inc) against the numpy statement (tests/descriptor_filters_ref.py, pinned on the CPU by
tests/test_descriptor_filters_host.py): every row and the kept indices bit for bit, no tolerance anywhere, in both precisions, from
host and from device memory; against the older call where only its stages are listed; the refusals."""
import ctypes as C

import numpy as np
import pytest

import descriptor_filters_ref as ref
from pgslam_amd import icp
from test_descriptor_filters_host import duplicated_scene

OBS, ORIENT, SHADOW, MAXDENS, NOISE, INC, SPH, CUT = ref.OBS, ref.ORIENT, ref.SHADOW, ref.MAXDENS, ref.NOISE, ref.INC, ref.SPH, ref.CUT


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


def to_device(a):
    import torch
    # (numpy gives an empty array zero strides, which from_numpy would carry over: an empty tensor is made by torch)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if len(a) else torch.zeros(a.shape, dtype=getattr(torch, a.dtype.name), device="cuda")


def check(ctx, xyz, T, stages, device, label, keep=ref.ALL, desc=None):
    """one call against the statement; returns (got, want)"""
    to = to_device if device else (lambda a: a)
    want = ref.run(xyz, T, stages, keep=keep, desc=desc)
    got = ctx.sensor_chain(to(xyz), ref.KNN, np.inf, stages, keep=keep, desc=None if desc is None else to(desc), mem="device" if device else "host")
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
        x = ref.sc.sized_cloud(n, T) if n else np.zeros((0, 3), dtype=T)
        if n < 63:
            # (too few points for medians that mean anything: fixed thresholds; the calls still have to agree)
            lists = dict(yaml=[(OBS,) + ref.CENTER, (ORIENT, 1), (INC,), (CUT, "incidence_angles", 1, 1.3), (SPH, 0, 0), (CUT, "sphericality", 1, 0.2), (MAXDENS, 50.0, ref.SEED)],
                         sph_all=[(SPH, 1, 1)], inc_alone=[(OBS,) + ref.CENTER, (INC,)])
            names = list(lists)
        else:
            lists = ref.stage_lists(x, T)
            names = ("yaml", "two_cuts", "cut_behind_shadow_md", "sph_all") if n not in (65, 4097) else list(lists)
        for name in names:
            check(ctx, x, T, lists[name], device, f"n={n} {name}")
        if n >= 63:
            y = ref.run(x, T, lists["yaml"])
            assert 0 < y["count"] < y["passed"][5] < y["passed"][3] < n, (n, y["passed"])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_main_scene_every_stage_list(ctx, T, device):
    x = ref.sc.scene(ref.MAIN_N, T)
    desc = np.random.default_rng(5).normal(size=(len(x), 3)).astype(T)
    lists = ref.stage_lists(x, T)
    res = {name: check(ctx, x, T, st, device, name)[1] for name, st in lists.items()}
    assert res["cut_drops_all"]["count"] == 0 and res["cut_nan_threshold"]["count"] == 0 and res["cut_keeps_all"]["passed"][2] == len(x)
    # a cut on a carried row, in both directions, then one more on a row of the run; the rows travel
    st = [(CUT, 1, 1, 0.25), (NOISE, 2, 1.0), (CUT, 2, 0, -0.5), (SPH, 1, 0), (CUT, "unstructureness", 1, ref.median_of(x, T, [(SPH, 1, 0)], "unstructureness"))]
    _, want = check(ctx, x, T, st, device, "carried rows", desc=desc)
    assert 0 < want["passed"][4] < want["passed"][2] < want["passed"][0] < len(x) and want["descriptors"].shape == (want["count"], 3)
    # with no row kept: the stages that need none still run
    _, want = check(ctx, x, T, [(NOISE, 0, 1.0), (CUT, "simple_sensor_noise", 1, ref.median_of(x, T, [(NOISE, 0, 1.0)], "simple_sensor_noise", keep=())), (OBS, 1.0, 2.0, 3.0)],
                    device, "no rows", keep=())
    assert 0 < want["count"] < len(x)
    _, want = check(ctx, x, T, [(CUT, 0, 0, 0.0)], device, "no rows, a carried one", keep=(), desc=desc)
    assert 0 < want["count"] < len(x)
    # the strided (n, 4) cloud gives the same bits
    x4 = np.ones((len(x), 4), dtype=T)
    x4[:, :3] = x
    check(ctx, x4, T, lists["yaml"], device, "stride 4")


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_duplicated_points_nan_sphericality_is_never_kept(ctx, T):
    dup = duplicated_scene(T)
    for device in (False, True):
        _, want = check(ctx, dup, T, [(SPH, 1, 1)], device, "dup")
        assert np.isnan(want["sphericality"]).all()
        for larger in (0, 1):
            _, want = check(ctx, dup, T, [(SPH, 0, 0), (CUT, "sphericality", larger, 0.5), (MAXDENS, 100.0, 3)], device, "dup cut")
            assert want["count"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_old_stages_only_equal_the_old_call(ctx, T):
    """pgicp_sensor_chain_ext_* with stage types 1 .. 5 only, against pgicp_sensor_chain_*: byte for byte"""
    x = ref.sc.scene(ref.MAIN_N, T)
    desc = np.random.default_rng(6).normal(size=(len(x), 2)).astype(T)
    old = ref.sc.stage_lists(ref.sc.pick_max_density(x, T))
    for device in (False, True):
        to = to_device if device else (lambda a: a)
        for name, st in old.items():
            a = ctx.sensor_chain(to(x), ref.KNN, np.inf, st, keep=ref.ALL, desc=to(desc))
            b = raw_ext(ctx, T, to(x), st, desc=to(desc), device=device)
            assert a["count"] == b["count"], name
            for key in ref.sc.ROWS:
                assert (a[key] is None) == (b[key] is None) and (a[key] is None or bits(a[key]) == bits(b[key])), (name, key)


def raw_ext(ctx, T, x, stages, keep=(1, 1, 1), desc=None, device=False, n_stages=None, want=(), status_only=False, knn=ref.KNN):
    """pgicp_sensor_chain_ext_* itself: the rows of Context.sensor_chain's result (or the status alone).  want: names of the four new
    outputs to hand in although no stage makes them"""
    import torch
    n = len(x)
    arr = ctx.chain_stages(stages)
    listed = {int(arr[k].type) for k in range(len(stages))}
    m = max(n, 1)
    mk = (lambda shape, dt=T: torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")) if device else (lambda shape, dt=T: np.empty(shape, dtype=dt))
    ptr = (lambda a: None if a is None else C.c_void_p(a.data_ptr())) if device else (lambda a: None if a is None else C.c_void_p(a.ctypes.data))
    sph = [arr[k] for k in range(len(stages)) if arr[k].type == icp.CHAIN_SPHERICALITY]
    rows = dict(xyz=mk((m, 3)), normals=mk((m, 3)) if keep[0] else None, eigen_values=mk((m, 3)) if keep[1] else None, densities=mk((m,)) if keep[2] else None,
                observation_directions=mk((m, 3)) if icp.CHAIN_OBSERVATION_DIRECTION in listed else None,
                noise=mk((m,)) if icp.CHAIN_SIMPLE_SENSOR_NOISE in listed else None, descriptors=None if desc is None else mk((m, desc.shape[1])),
                incidence_angles=mk((m,)) if icp.CHAIN_INCIDENCE_ANGLE in listed or "incidence_angles" in want else None,
                sphericality=mk((m,)) if sph or "sphericality" in want else None,
                unstructureness=mk((m,)) if (sph and sph[0].p[0] == 1.0) or "unstructureness" in want else None,
                structureness=mk((m,)) if (sph and sph[0].p[1] == 1.0) or "structureness" in want else None, kept_idx=mk((m,), np.int32))
    out = icp.ChainOut(ptr(rows["xyz"]), ptr(rows["normals"]), 3, ptr(rows["eigen_values"]), ptr(rows["densities"]), ptr(rows["observation_directions"]),
                       ptr(rows["noise"]), ptr(rows["descriptors"]), ptr(rows["incidence_angles"]), ptr(rows["sphericality"]), ptr(rows["unstructureness"]),
                       ptr(rows["structureness"]), ptr(rows["kept_idx"]))
    n_out = C.c_int(-5)
    fn = getattr(ctx.lib, "pgicp_sensor_chain_ext" + ("_f32" if T == np.float32 else "_f64"))
    st = fn(ctx.h, ptr(x), C.c_int(3), C.c_int(n), C.c_int(icp.DEVICE if device else icp.HOST), C.c_int(knn), C.c_double(1e300), C.c_int(keep[0]), C.c_int(keep[1]),
            C.c_int(keep[2]), C.c_int(len(stages) if n_stages is None else n_stages), arr, ptr(desc), C.c_int(0 if desc is None else desc.shape[1]), C.byref(out),
            C.byref(n_out))
    if status_only:
        return st
    assert st == icp.OK
    k = n_out.value
    return dict(count=k, **{key: (None if a is None else a[:k]) for key, a in rows.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_argument_refusals_leave_the_context_usable(ctx, T):
    x = ref.sc.sized_cloud(300, T)
    desc = np.random.default_rng(3).normal(size=(len(x), 2)).astype(T)
    obs, orient, sh, md, nz, inc = (OBS, 0, 0, 0), (ORIENT, 1), (SHADOW, 0.2), (MAXDENS, 5.0, 1), (NOISE, 0, 1.0), (INC,)
    cut_d = (CUT, "densities", 1, 1.0)
    status = lambda *a, **k: raw_ext(ctx, T, x, *a, status_only=True, **k)
    # the longest list there is -- every type once and four cuts, eleven stages -- is taken
    assert status([nz, obs, orient, inc, (CUT, "incidence_angles", 1, 2.0), (SPH, 1, 1), (CUT, "sphericality", 1, 1.0), (CUT, "unstructureness", 0, 0.0), sh,
                   (CUT, "simple_sensor_noise", 0, 0.0), md]) == icp.OK
    bad = [
        dict(stages=[cut_d] * 4 + [nz] * 9),                                        # more than PGICP_CHAIN_EXT_MAX_STAGES
        dict(stages=[(0,)]), dict(stages=[(9,)]), dict(stages=[(-1,)]),              # an unknown stage type
        dict(stages=[obs, inc, inc]), dict(stages=[(SPH, 0, 0), (SPH, 1, 1)]), dict(stages=[sh, sh]),      # a type twice
        dict(stages=[cut_d] * 5),                                                    # a fifth cut
        dict(stages=[inc]), dict(stages=[inc, obs]),                                 # no observation direction before it
        dict(stages=[obs, inc], keep=(0, 1, 1)),                                     # no normals
        dict(stages=[(SPH, 0, 0)], keep=(1, 0, 1)),                                  # no eigenvalues
        dict(stages=[(SPH, 2, 0)]), dict(stages=[(SPH, 0, 0.5)]),                    # flags that are not 0 or 1
        dict(stages=[(CUT, "densities", 2, 1.0)]),
        dict(stages=[cut_d], keep=(1, 1, 0)),                                        # the row is not there when the cut runs
        dict(stages=[(CUT, "incidence_angles", 1, 1.0), obs, inc]), dict(stages=[(CUT, "sphericality", 1, 1.0), (SPH, 0, 0)]),
        dict(stages=[(SPH, 0, 1), (CUT, "unstructureness", 1, 1.0)]), dict(stages=[(SPH, 1, 0), (CUT, "structureness", 1, 1.0)]),
        dict(stages=[(CUT, "simple_sensor_noise", 1, 1.0), nz]),
        dict(stages=[(CUT, 0, 1, 1.0)]),                                             # no desc
        dict(stages=[(CUT, 2, 1, 1.0)], desc=desc), dict(stages=[(CUT, -1, 1, 1.0)], desc=desc), dict(stages=[(8, 0.0, 1.0, 1.0, 0.5)], desc=desc),
        dict(stages=[(8, 7.0, 1.0, 1.0)]), dict(stages=[(8, 1.5, 1.0, 1.0)]), dict(stages=[(8, float("nan"), 1.0, 1.0)]),      # no such row code
        dict(stages=[], want=("incidence_angles",)), dict(stages=[], want=("sphericality",)),                # an output no stage makes
        dict(stages=[(SPH, 0, 1)], want=("unstructureness",)), dict(stages=[(SPH, 1, 0)], want=("structureness",)),
        dict(stages=[orient]), dict(stages=[md], keep=(1, 1, 0)), dict(stages=[(SHADOW, 4.0)]), dict(stages=[], knn=2),      # the older call's still hold
        dict(stages=[obs], n_stages=-1),
    ]
    for k in bad:
        assert status(**k) == icp.ERR_ARG, k
        assert ctx.lib.pgicp_last_error(ctx.h)
    fn = getattr(ctx.lib, "pgicp_sensor_chain_ext" + ("_f32" if T == np.float32 else "_f64"))
    n_out = C.c_int(-5)
    assert fn(ctx.h, C.c_void_p(x.ctypes.data), C.c_int(3), C.c_int(len(x)), C.c_int(icp.HOST), C.c_int(10), C.c_double(1.0), C.c_int(1), C.c_int(0), C.c_int(1),
              C.c_int(0), None, None, C.c_int(0), None, C.byref(n_out)) == icp.ERR_ARG                       # out is null
    # pgicp_sensor_chain_* itself keeps refusing the new types, through the binding too
    old = getattr(ctx.lib, "pgicp_sensor_chain" + ("_f32" if T == np.float32 else "_f64"))
    arr = ctx.chain_stages([(SPH, 0, 0)])
    ox, oi = np.empty((300, 3), dtype=T), np.empty(300, dtype=np.int32)
    assert old(ctx.h, C.c_void_p(x.ctypes.data), C.c_int(3), C.c_int(len(x)), C.c_int(icp.HOST), C.c_int(10), C.c_double(1e300), C.c_int(1), C.c_int(1), C.c_int(1),
               C.c_int(1), arr, None, C.c_int(0), C.c_void_p(ox.ctypes.data), None, C.c_int(3), None, None, None, None, None, C.c_void_p(oi.ctypes.data),
               C.byref(n_out)) == icp.ERR_ARG
    with pytest.raises(icp.PgicpError) as e:
        ctx.sensor_chain(x, ref.KNN, np.inf, [inc])
    assert e.value.code == icp.ERR_ARG
    # n == 0, a NaN threshold (accepted: it keeps nothing), and the context is usable after the refusals
    assert raw_ext(ctx, T, x[:0], [obs, inc, (CUT, "incidence_angles", 1, 1.0)])["count"] == 0
    assert raw_ext(ctx, T, x, [(CUT, "densities", 0, float("nan"))])["count"] == 0
    check(ctx, x, T, [nz, obs, orient, inc, (CUT, "incidence_angles", 1, 1.2), sh, md], False, "after the refusals")


# ---- entry 9 of pgicp_filter_cloud_* -------------------------------------------------------------------------------------------

def cut_chain_reference(o, f, d, T, filters):
    """the kept indices of a list that holds entries of type 9: the oracle's filter chain for the stretches between them (each on the
    survivors so far, so a sampler sees the ranks after a cut), numpy for the cuts"""
    idx = np.arange(len(f))
    run = []
    for spec in list(filters) + [None]:
        if spec is None or spec[0] == icp.FILTER_CUT_AT_DESCRIPTOR:
            if run and len(idx):
                idx = idx[o.filter_chain(run, np.ascontiguousarray(f[idx]))]
            run = []
            if spec is not None:
                idx = idx[ref.cut_keep(d[idx, int(spec[1])], spec[3], bool(spec[2]), T)]
        else:
            run.append(spec)
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_filter_cloud_cut_at_descriptor(ctx, oracle32, oracle64, T):
    from pgslam_amd import synth
    o = oracle32 if T == np.float32 else oracle64
    Tm = synth.se3(x=0.4, y=-0.2, z=1.1, yaw=0.3, pitch=0.05, roll=-0.02)
    for n in [s for s in ref.SIZES if s] + [20_000]:
        rng = np.random.default_rng(n)
        xyz = ref.sc.sized_cloud(n, T)
        f = np.concatenate([xyz, np.ones((n, 1), dtype=T)], axis=1)
        nrm = rng.normal(size=(n, 3)).astype(T)
        d = np.concatenate([nrm, rng.normal(size=(n, 2)).astype(T)], axis=1)           # normals | two one-row descriptors
        thr = float(d[0, 3])                                                         # a value that occurs: the comparison is not strict
        if n > 3:
            d[1, 3], d[2, 3], d[3, 3] = np.nan, np.inf, -np.inf
        box = (icp.FILTER_BOUNDING_BOX, 1.0, -3.0, -3.0, 7.0, 3.0, 3.0, 0.0)
        chains = [
            [(icp.FILTER_CUT_AT_DESCRIPTOR, 3, 1, thr)], [(icp.FILTER_CUT_AT_DESCRIPTOR, 3, 0, thr)],
            [box, (icp.FILTER_CUT_AT_DESCRIPTOR, 4, 1, 0.3), (icp.FILTER_RANDOM_SAMPLING, 0.5, 7)],
            [(icp.FILTER_CUT_AT_DESCRIPTOR, 4, 0, -0.3), (icp.FILTER_FIX_STEP, 2), (icp.FILTER_CUT_AT_DESCRIPTOR, 3, 1, 0.5), (icp.FILTER_MAX_POINT_COUNT, 40, 3)],
            [(icp.FILTER_CUT_AT_DESCRIPTOR, 3, 1, float("nan"))],
        ]
        for filters in chains:
            want = cut_chain_reference(o, f, d, T, filters)
            for M in (None, Tm):
                of, od, idx, dev = ctx.filter_cloud(filters, f, d, T=M, rotate_rows=(0, -1))
                assert np.array_equal(idx, want), (n, filters)
                assert len(of) == len(want) and dev.n == len(want)
                if M is None:
                    assert bits(of) == f[want].tobytes() and bits(od) == d[want].tobytes(), (n, filters)
                elif len(want):
                    assert np.array_equal(of[:, :3], o.transform(M, f[want][:, :3])) and bits(od[:, 3:]) == np.ascontiguousarray(d[want][:, 3:]).tobytes()
                    assert np.array_equal(od[:, 0:3], o.transform(M, d[want][:, 0:3], rotate_only=True))
            # without kept indices asked for (the short list of dropped points comes back instead) the kept points are the same
            of2, od2, _, _ = ctx.filter_cloud(filters, f, d, want_idx=False)
            assert bits(of2) == f[want].tobytes() and bits(od2) == d[want].tobytes(), (n, filters)
        if n == 4097:
            one = cut_chain_reference(o, f, d, T, chains[0])
            assert 1 not in one and 3 in one and 2 not in one and 0 in one and 0.1 * n < len(one) < 0.9 * n
            other = cut_chain_reference(o, f, d, T, chains[1])
            assert 1 not in other and 2 in other and 3 not in other and 0 in other
            a = cut_chain_reference(o, f, d, T, chains[2])
            b = np.intersect1d(cut_chain_reference(o, f, d, T, chains[2][:2]), o.filter_chain([box, chains[2][2]], f))
            assert 0 < len(a) and not np.array_equal(a, b)                           # the sampler does see the ranks after the cut


@pytest.mark.gpu
@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_filter_cloud_cut_refusals(ctx, T):
    n = 500
    f = np.concatenate([ref.sc.sized_cloud(n, T), np.ones((n, 1), dtype=T)], axis=1)
    d = np.random.default_rng(2).normal(size=(n, 2)).astype(T)
    good = [(icp.FILTER_CUT_AT_DESCRIPTOR, 1, 1, 0.0)]
    for filters, desc in ((good, None), ([(icp.FILTER_CUT_AT_DESCRIPTOR, 2, 1, 0.0)], d), ([(icp.FILTER_CUT_AT_DESCRIPTOR, -1, 1, 0.0)], d),
                          ([(icp.FILTER_CUT_AT_DESCRIPTOR, 0.5, 1, 0.0)], d), ([(icp.FILTER_CUT_AT_DESCRIPTOR, 0, 2, 0.0)], d), ([(10,)], d)):
        with pytest.raises(icp.PgicpError) as e:
            ctx.filter_cloud(filters, f, desc)
        assert e.value.code == icp.ERR_ARG, filters
    # pgicp_filter_cloud_dev_* takes no descriptors: any list that holds the entry is refused
    for filters in (good, [(icp.FILTER_MAX_DIST, 30.0)] + good):
        with pytest.raises(icp.PgicpError) as e:
            ctx.filter_cloud_dev(filters, f)
        assert e.value.code == icp.ERR_ARG
    kept, _, dropped = ctx.filter_cloud_dev([(icp.FILTER_MAX_DIST, 30.0)], f)
    assert kept == n and len(dropped) == 0
    of, od, idx, _ = ctx.filter_cloud(good, f, d)
    assert np.array_equal(idx, np.flatnonzero(d[:, 1] <= 0))
