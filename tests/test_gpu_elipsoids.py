"""pgicp_elipsoids_* (include/pgicp_elipsoids.h) on the device against the numpy statement (tests/elipsoids_ref.py, checked on the CPU
by tests/test_elipsoids_host.py) bit for bit, in f32 and f64, with host and device memory: every case with all rows asked for and with
a sparse subset, the planarity drop, the identities on the device's output, the older entries byte for byte, the refusals, an empty
cloud, the allocation count of a second call, and one cloud past the single-block sizes of the scans.  Every other cloud is small;
the references are computed once (the reference module caches its cases)."""
import ctypes as C

import numpy as np
import pytest

import elipsoids_ref as ref
from pgslam_amd import icp

pytestmark = pytest.mark.gpu

CASES = ref.cases()
ALL, SPARSE, OLD = ref.ALL, ref.SPARSE, ref.OLD


@pytest.fixture(scope="module")
def gctx():
    c = icp.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()              # (a copy: the reference's arrays are read-only)


def host(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def same(a, b, what):
    a, b = host(a), host(b)
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), (what, a, b)


def descriptor_forms(c):
    """0 and 3 descriptor rows, with and without averaging (the rows ride along; the cases of knn 7 carry them)"""
    return ((0, True), (3, True), (3, False)) if c[2] == 7 else ((0, True),)


def call(gctx, x, d, c, keep, min_planarity=0.0, average=True, mem=None):
    name, T, knn, ratio, method, max_box = c
    return gctx.elipsoids(x, knn=knn, ratio=ratio, method=method, max_box=max_box, min_planarity=min_planarity, seed=ref.SEED, desc=d,
                          average=average, keep=keep, mem=mem)


def check(e, r, keep, what):
    """the device's dict against the reference's: what was asked for bit for bit, what was not is None"""
    assert e["boxes"] == r["boxes"], what
    for key in OLD:
        same(e[key], r[key], what + (key,))
    for key in ALL:
        if key in keep:
            same(e[key], r[key], what + (key,))
        else:
            assert e[key] is None, what + (key,)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("c", CASES, ids=ref.case_id)
def test_all_rows_a_sparse_subset_and_identities(gctx, c, mem):
    name, T, knn, ratio, method, max_box = c
    for drows, average in descriptor_forms(c):
        xyz, d, r = ref.case(c, drows, average)
        what = (ref.case_id(c), mem, drows, average)
        x, dd = (xyz, d) if mem == "host" else (dev(xyz), dev(d))
        e = call(gctx, x, dd, c, ALL, average=average, mem=mem)
        check(e, r, ALL, what + ("all",))
        # a sparse subset: a null output leaves the other outputs' bytes as they were
        sp = call(gctx, x, dd, c, SPARSE, average=average, mem=mem)
        check(sp, r, SPARSE, what + ("sparse",))
        # the identities, per kept point, on the device's output
        g = {k: host(e[k]) for k in ALL + ("xyz",)}
        ref.identities(g, method, knn)
        if method == 1:
            assert len(g["weights"]) == e["boxes"] and g["weights"].sum() == sum(len(m) for m in r["members"]), what
        order = np.argsort(r["box_of"], kind="stable")
        twin = np.flatnonzero(np.diff(r["box_of"][order]) == 0)
        assert method == 0 or len(twin) == 0
        for key in ALL:
            a = g[key][order]
            assert np.array_equal(a[twin], a[twin + 1]), what + (key, "one box, one row")


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("T", ref.TYPES, ids=lambda T: np.dtype(T).name)
def test_min_planarity(gctx, T, mem):
    put = (lambda a: a) if mem == "host" else dev
    for name in ("cloud3000", "mixed_line"):
        thr = ref.pick_min_planarity(ref.cloud(name, T), T, 7)
        for method in (0, 1):
            c = (name, T, 7, 0.5, method, np.inf)
            xyz, _, r = ref.case(c, min_planarity=thr)
            full = ref.case(c)[2]
            assert 0 < r["boxes"] < full["boxes"]
            e = call(gctx, put(xyz), None, c, ALL, min_planarity=thr)
            check(e, r, ALL, (name, method, "picked", thr))
            assert np.all(host(e["shapes"])[:, 0] >= T(thr))
            # minPlanarity 0: the boxes fused are SamplingSurfaceNormal's
            old = gctx.sampling_surface_normal(put(xyz), knn=7, ratio=0.5, sampling_method=method, seed=ref.SEED)
            zero = call(gctx, put(xyz), None, c, ALL)
            assert zero["boxes"] == old["boxes"] == full["boxes"]
    # minPlanarity 1.0 on the random cloud: every box is dropped, nothing is kept and nothing is written
    c = ("cloud3000", T, 7, 0.5, 0, np.inf)
    xyz, _, r = ref.case(c, min_planarity=1.0)
    assert r["boxes"] == 0 and len(r["kept_idx"]) == 0
    n = len(xyz)
    lib, sfx = gctx.lib, "_f32" if T == np.float32 else "_f64"
    widths = dict(xyz=3, normals=3, eigen_values=3, eigen_vectors=9, densities=1, covariance=9, weights=1, means=3, shapes=3)
    if mem == "host":
        x = np.ascontiguousarray(xyz)
        out = {k: np.full((n, w), 7.5, dtype=T) for k, w in widths.items()}
        idx = np.full(n, -5, dtype=np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)
        m = icp.HOST
    else:
        import torch
        x = dev(xyz)
        out = {k: torch.full((n, w), 7.5, dtype=x.dtype, device=x.device) for k, w in widths.items()}
        idx = torch.full((n,), -5, dtype=torch.int32, device=x.device)
        p = lambda a: C.c_void_p(a.data_ptr())
        m = icp.DEVICE
    n_out, boxes = C.c_int(-1), C.c_int(-1)
    rc = getattr(lib, "pgicp_elipsoids" + sfx)(
        gctx.h, p(x), C.c_int(3), C.c_int(n), C.c_int(m), C.c_int(7), C.c_double(0.5), C.c_int(0), C.c_double(np.inf), C.c_uint64(ref.SEED), None,
        C.c_int(0), C.c_int(1), p(out["xyz"]), C.c_int(3), p(out["normals"]), C.c_int(3), None, p(idx), C.byref(n_out), C.byref(boxes),
        p(out["eigen_values"]), p(out["eigen_vectors"]), p(out["densities"]), C.c_double(1.0), p(out["covariance"]), p(out["weights"]),
        p(out["means"]), p(out["shapes"]))
    assert rc == icp.OK and n_out.value == 0 and boxes.value == 0
    for k in widths:
        assert np.all(host(out[k]) == T(7.5)), k
    assert np.all(host(idx) == -5)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("c", [c for c in CASES if c[2] == 7 and c[0] in ("cloud3000", "mixed_line", "coincident", "big_box", "far", "n31")],
                         ids=ref.case_id)
def test_only_normals_equals_the_older_entries_byte_for_byte(gctx, c, mem):
    name, T, knn, ratio, method, max_box = c
    for drows, average in descriptor_forms(c):
        xyz, d, _ = ref.case(c, drows, average)
        x, dd = (xyz, d) if mem == "host" else (dev(xyz), dev(d))
        kw = dict(knn=knn, ratio=ratio, sampling_method=method, max_box_dim=max_box, seed=ref.SEED, descriptors=dd, average_descriptors=average)
        old = gctx.sampling_surface_normal(x, **kw)
        ext = gctx.sampling_surface_normal_ext(x, **kw)
        e = call(gctx, x, dd, c, ("normals",), average=average)
        assert e["boxes"] == old["boxes"] == ext["boxes"]
        for key in ("xyz", "normals", "kept_idx", "descriptors"):
            same(e[key], old[key], (ref.case_id(c), key, "older"))
            same(e[key], ext[key], (ref.case_id(c), key, "ext"))
        # and with every row of the ext entry asked of both
        ext = gctx.sampling_surface_normal_ext(x, **kw, want_eigen=True, want_eigen_vectors=True, want_densities=True)
        e = call(gctx, x, dd, c, ("normals", "eigen_values", "eigen_vectors", "densities"), average=average)
        for key in ("xyz", "normals", "kept_idx", "descriptors", "eigen_values", "eigen_vectors", "densities"):
            same(e[key], ext[key], (ref.case_id(c), key, "ext, all its rows"))


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("T", ref.TYPES, ids=lambda T: np.dtype(T).name)
def test_refusals_leave_the_context_usable(gctx, T, mem):
    c = ("cloud3000", T, 7, 0.5, 0, np.inf)
    xyz, _, r = ref.case(c)
    put = (lambda a: a) if mem == "host" else dev
    bad_clouds = []
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[17, 1] = bad
        bad_clouds.append(dict(xyz=put(x)))
    refused = bad_clouds + [dict(xyz=put(xyz), knn=2), dict(xyz=put(xyz), knn=1025), dict(xyz=put(xyz), method=2), dict(xyz=put(xyz), method=-1),
                            dict(xyz=put(xyz), min_planarity=-0.1), dict(xyz=put(xyz), min_planarity=1.5), dict(xyz=put(xyz), min_planarity=np.nan),
                            dict(xyz=put(xyz), min_planarity=np.inf)]
    for kw in refused:
        for keep in (ALL, ("normals",), ()):
            with pytest.raises(icp.PgicpError) as err:
                gctx.elipsoids(**kw, keep=keep)
            assert err.value.code == icp.ERR_ARG, kw
        # the context is still good, and gives what it gave
        e = call(gctx, put(xyz), None, c, ALL)
        check(e, r, ALL, ("after a refusal", str(kw.keys())))


@pytest.mark.parametrize("T", ref.TYPES, ids=lambda T: np.dtype(T).name)
def test_an_empty_cloud(gctx, T):
    e = gctx.elipsoids(np.zeros((0, 3), dtype=T), keep=ALL)
    assert len(e["kept_idx"]) == 0 and e["boxes"] == 0 and all(len(e[k]) == 0 for k in ALL)
    import torch
    e = gctx.elipsoids(torch.zeros((0, 3), dtype=torch.float32 if T == np.float32 else torch.float64, device="cuda"), keep=ALL)
    assert len(e["kept_idx"]) == 0 and e["boxes"] == 0


def alloc_count(ctx):
    """the library's device allocations so far (pgicp_debug_alloc_stats, process-wide)"""
    out = (C.c_longlong * 8)()
    assert ctx.lib.pgicp_debug_alloc_stats(out) == 0
    return int(out[0])


@pytest.mark.parametrize("T", ref.TYPES, ids=lambda T: np.dtype(T).name)
def test_a_second_call_of_the_same_size_allocates_nothing(T):
    ctx = icp.Context(0)
    try:
        xyz, _, r = ref.case(("cloud3000", T, 7, 0.5, 1, np.inf))
        other = np.ascontiguousarray(xyz[::-1])
        for put in ((lambda a: a), dev):
            first = ctx.elipsoids(put(xyz), knn=7, method=1, seed=ref.SEED, keep=ALL)
            before = alloc_count(ctx)
            again = ctx.elipsoids(put(other), knn=7, method=1, seed=ref.SEED, keep=ALL)
            sparse = ctx.elipsoids(put(xyz), knn=7, method=1, seed=ref.SEED, keep=SPARSE)
            assert alloc_count(ctx) == before
            same(first["covariance"], r["covariance"], "first")
            same(sparse["shapes"], r["shapes"], "sparse")
            assert len(again["kept_idx"]) == len(r["kept_idx"])
    finally:
        ctx.close()


@pytest.mark.parametrize("T", ref.TYPES, ids=lambda T: np.dtype(T).name)
def test_twenty_thousand_points_pass_the_single_block_scans(gctx, T):
    """20 000 points: the 60 000 marks of a level no longer fit one block of the scan.  The reference is the numpy statement, computed
    once per type (a few seconds on the host)."""
    x = np.ascontiguousarray(np.random.default_rng(71).uniform(-2, 2, (20000, 3)), dtype=T)
    r = ref.run(x, T, 7, 0.5, 1, np.inf, 0.0, ref.SEED)
    e = gctx.elipsoids(x, knn=7, ratio=0.5, method=1, seed=ref.SEED, keep=ALL)
    check(e, r, ALL, ("20000", np.dtype(T).name))
    ref.identities({k: host(e[k]) for k in ALL + ("xyz",)}, 1, 7)
