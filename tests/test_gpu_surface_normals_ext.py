"""pgicp_surface_normals_ext_* and pgicp_smooth_normals_* (include/pgicp_normals_ext.h) on the device: the superset property against
the two existing calls byte for byte, the new rows against the numpy reference (tests/surface_normals_ext_ref.py) byte for byte, the
plane's known answers, the sign rule of the smoothing step, independence of call history and of other contexts, and the refusals
that need no oversized buffer.  Every cloud is small; the references are computed once (the reference module caches its scenes)."""
import ctypes as C

import numpy as np
import pytest

import surface_normals_ext_ref as ref
from pgslam_amd import icp

pytestmark = pytest.mark.gpu

TYPES = ref.TYPES
ALL = dict(want_eigen=True, want_eigen_vectors=True, want_mean_dist=True, want_matched_ids=True, want_ids=True)


@pytest.fixture(scope="module")
def gctx():
    c = icp.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the reference's arrays are read-only)


def host(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def same(a, b, what):
    a, b = host(a), host(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), (what, a, b)


# ---------------------------------------------------------------- superset
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("knn", ref.SUPERSET_KNN)
@pytest.mark.parametrize("n", ref.SUPERSET_N)
def test_superset_of_the_two_existing_calls(gctx, n, knn, T):
    """(that the finite maxDist leaves short lists at every n and knn is asserted on the oracle's table, on the CPU:
    tests/test_surface_normals_ext_host.py::test_superset_clouds_have_short_lists)"""
    cloud = ref.superset_cloud(n, T)
    for md in (np.inf, ref.SUPERSET_MAX_DIST):
        for xyz in (cloud, dev(cloud)):
            what = (n, knn, T.__name__, md, type(xyz).__name__)
            nrm, eig, ids, d2 = gctx.surface_normals(xyz, knn=knn, max_dist=md, want_eigen=True, want_ids=True)
            e = gctx.surface_normals_ext(xyz, knn=knn, max_dist=md, want_eigen=True, want_ids=True)
            for got, exp, name in ((e["normals"], nrm, "normals"), (e["eigen_values"], eig, "eig"), (e["ids"], ids, "ids"), (e["d2"], d2, "d2")):
                same(got, exp, what + (name,))
            assert e["eigen_vectors"] is None and e["mean_dists"] is None and e["matched_ids"] is None and e["densities"] is None
            d = gctx.surface_densities(xyz, knn=knn, max_dist=md)
            e = gctx.surface_normals_ext(xyz, knn=knn, max_dist=md, want_eigen=True, want_densities=True)
            for k, name in (("normals", "normals"), ("eigen_values", "eigen_values"), ("densities", "densities")):
                same(e[name], d[k], what + ("dens", name))
            # the old rows do not move when every new one is asked for besides
            e = gctx.surface_normals_ext(xyz, knn=knn, max_dist=md, want_densities=True, **ALL)
            same(e["normals"], nrm, what + ("all", "normals"))
            same(e["eigen_values"], eig, what + ("all", "eig"))
            same(e["ids"], ids, what + ("all", "ids"))
            same(e["d2"], d2, what + ("all", "d2"))
            same(e["densities"], d["densities"], what + ("all", "densities"))
            same(host(e["eigen_vectors"])[:, :3], host(nrm), what + ("first column",))
            same(host(e["matched_ids"]).astype(np.int32), host(ids), what + ("matched",))


# ---------------------------------------------------------------- the new rows
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", sorted(ref.SCENES))
def test_new_rows_equal_the_reference(gctx, name, T, mem):
    xyz, knn, md, o, r = ref.scene(name, T)
    x = xyz if mem == "host" else dev(xyz)
    e = gctx.surface_normals_ext(x, knn=knn, max_dist=md, **ALL)
    same(e["ids"], o["ids"], (name, "ids"))
    same(e["d2"], o["d2"], (name, "d2"))
    same(e["normals"], r["normals"], (name, "normals"))
    same(e["eigen_values"], r["eigen_values"], (name, "eigen_values"))
    same(e["eigen_vectors"], r["eigen_vectors"], (name, "eigen_vectors"))
    same(e["mean_dists"], r["mean_dists"], (name, "mean_dists"))
    same(e["matched_ids"], r["matched_ids"], (name, "matched_ids"))
    s = gctx.surface_normals_ext(x, knn=knn, max_dist=md, smooth=True, **ALL)
    same(s["normals"], r["smoothed"], (name, "smoothed"))
    same(s["eigen_vectors"], r["eigen_vectors"], (name, "eigVectors stay raw"))
    # smoothing with nothing else asked for: the raw normals and the table live in the context's scratch
    same(gctx.surface_normals_ext(x, knn=knn, max_dist=md, smooth=True)["normals"], r["smoothed"], (name, "smoothed alone"))
    # each new row alone
    for want, key in (("want_eigen_vectors", "eigen_vectors"), ("want_mean_dist", "mean_dists"), ("want_matched_ids", "matched_ids")):
        same(gctx.surface_normals_ext(x, knn=knn, max_dist=md, want_normals=False, **{want: True})[key], r[key], (name, key, "alone"))


@pytest.mark.parametrize("T", TYPES)
def test_plane_known_answers(gctx, T):
    xyz, interior = ref.plane_case(T)
    e = gctx.surface_normals_ext(xyz, knn=5, smooth=True, **ALL)
    raw = gctx.surface_normals_ext(xyz, knn=5)["normals"]
    k = len(interior)
    assert np.array_equal(raw[interior], np.tile(np.array([0, 0, 1], dtype=T), (k, 1)))
    assert np.array_equal(e["eigen_vectors"][interior], np.tile(np.array([0, 0, 1, 0, 1, 0, 1, 0, 0], dtype=T), (k, 1)))
    assert np.all(e["mean_dists"][interior] == 0)
    assert e["normals"][interior].tobytes() == raw[interior].tobytes()


# ---------------------------------------------------------------- smooth_normals alone
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("T", TYPES)
def test_smooth_normals_sign_rule(gctx, T, mem):
    """(no dot product of the scene is exactly 0: tests/test_surface_normals_ext_host.py)"""
    put = (lambda a: a) if mem == "host" else dev
    nrm, ids, flip = ref.sign_flip_case("random", T)
    raw = ref.scene("random", T)[4]["normals"]
    out_raw = host(gctx.smooth_normals(put(raw), put(ids)))
    out = host(gctx.smooth_normals(put(nrm), put(ids)))
    same(out, ref.smooth(nrm, ids, T), "against the reference")
    same(out_raw, ref.smooth(raw, ids, T), "against the reference, raw")
    # flipping any set of neighbours leaves every other point's output as it was, byte for byte
    assert out[~flip].tobytes() == out_raw[~flip].tobytes()
    # flipping r_i negates out_i exactly (a zero component keeps the sign of its zero: +0 + -0 = +0)
    assert np.array_equal(out[flip], -out_raw[flip])
    nz = out_raw[flip] != 0
    assert out[flip][nz].tobytes() == (-out_raw[flip][nz]).tobytes()
    # a second, different set of flipped neighbours
    nrm2, _, flip2 = ref.sign_flip_case("random", T, seed=9)
    out2 = host(gctx.smooth_normals(put(nrm2), put(ids)))
    assert out2[~flip2].tobytes() == out_raw[~flip2].tobytes()


@pytest.mark.parametrize("T", TYPES)
def test_smooth_normals_padding_and_self_only_rows(gctx, T):
    rng = np.random.default_rng(12)
    n, knn = 300, 7
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(T)
    ids = rng.integers(0, n, (n, knn)).astype(np.int32)
    ids[:, 0] = np.arange(n)
    ids[rng.random((n, knn)) < 0.3] = -1                      # holes anywhere in a row
    ids[::5, 1:] = -1
    ids[::5, 0] = np.arange(n)[::5]                            # rows holding only self
    ids[7] = -1                                                # a row holding nothing: the raw normal comes back
    exp = ref.smooth(nrm, ids, T)
    same(gctx.smooth_normals(nrm, ids), exp, "host")
    same(gctx.smooth_normals(dev(nrm), dev(ids)), exp, "device")
    assert exp[7].tobytes() == nrm[7].tobytes()
    assert np.abs(np.linalg.norm(exp[::5].astype(np.float64), axis=1) - 1).max() <= 4 * np.finfo(T).eps
    # padded normals rows (stride 4) in, packed rows out
    wide = np.zeros((n, 4), dtype=T)
    wide[:, :3] = nrm
    same(gctx.smooth_normals(wide, ids), exp, "stride 4")


# ---------------------------------------------------------------- state
def _calls(T):
    """(name, call(ctx)) of plain, ext and smooth calls with different n and knn"""
    a, b = ref.superset_cloud(2000, T), ref.superset_cloud(129, T)
    xr, kr, mr, o, r = ref.scene("random", T)
    xl, kl, ml, ol, rl = ref.scene("lattice", T)
    return [
        ("ext all 2000/17", lambda c: c.surface_normals_ext(a, knn=17, max_dist=0.35, smooth=True, want_densities=True, **ALL)),
        ("plain 129/3", lambda c: dict(zip("abcd", c.surface_normals(b, knn=3, want_eigen=True, want_ids=True)))),
        ("smooth 2000/10", lambda c: dict(n=c.smooth_normals(r["normals"], o["ids"]))),
        ("ext smooth 129/32", lambda c: c.surface_normals_ext(b, knn=32, smooth=True)),
        ("dens 2000/8", lambda c: c.surface_densities(a, knn=8, max_dist=0.35)),
        ("ext rows 600/6", lambda c: c.surface_normals_ext(xl, knn=kl, max_dist=ml, **ALL)),
        ("smooth 600/6", lambda c: dict(n=c.smooth_normals(rl["normals"], ol["ids"]))),
        ("ext smooth 2000/9", lambda c: c.surface_normals_ext(a, knn=9, max_dist=0.35, smooth=True, want_eigen_vectors=True)),
    ]


def _bytes(d):
    return {k: None if v is None else host(v).tobytes() for k, v in d.items()}


@pytest.mark.parametrize("T", TYPES)
def test_calls_do_not_depend_on_history_or_on_other_contexts(gctx, T):
    calls = _calls(T)
    alone = []
    for name, call in calls:
        c = icp.Context(0)                                     # each call on a context of its own: what it returns alone
        alone.append(_bytes(call(c)))
        c.close()
    second = icp.Context(0)
    try:
        for ctx in (gctx, second):
            for order in (range(len(calls)), reversed(range(len(calls))), (0, 3, 0, 2, 7, 1, 7, 5, 6, 4)):
                for k in order:
                    assert _bytes(calls[k][1](ctx)) == alone[k], (calls[k][0], T.__name__)
    finally:
        second.close()


# ---------------------------------------------------------------- refusals
def _ext_raw(c, T, xyz, stride, n, knn, md=1e300, smooth=0, out_stride=3, want_nrm=True):
    fn = getattr(c.lib, "pgicp_surface_normals_ext" + ("_f32" if T == np.float32 else "_f64"))
    out = np.zeros((max(n, 1), 3), dtype=T)
    return fn(c.h, C.c_void_p(xyz.ctypes.data), C.c_int(stride), C.c_int(n), C.c_int(icp.HOST), C.c_int(knn), C.c_double(md), C.c_int(smooth),
              C.c_void_p(out.ctypes.data) if want_nrm else None, C.c_int(out_stride), None, None, None, None, None, None, None)


@pytest.mark.parametrize("T", TYPES)
def test_refusals_leave_the_context_usable(gctx, T):
    xyz, knn, md, o, r = ref.scene("lattice", T)
    n = len(xyz)

    def still_fine():
        same(gctx.surface_normals_ext(xyz, knn=knn, max_dist=md, want_eigen_vectors=True)["eigen_vectors"], r["eigen_vectors"], "after a refusal")

    for bad_knn in (0, -1, 33):
        assert _ext_raw(gctx, T, xyz, 3, n, bad_knn) == icp.ERR_ARG
        still_fine()
    with pytest.raises(icp.PgicpError):
        gctx.surface_normals_ext(xyz, knn=2, want_densities=True)           # as pgicp_surface_densities_*: knn >= 3
    still_fine()
    assert _ext_raw(gctx, T, xyz, 3, -1, knn) == icp.ERR_ARG
    still_fine()
    assert _ext_raw(gctx, T, xyz, 2, n, knn) == icp.ERR_ARG
    assert _ext_raw(gctx, T, xyz, 3, n, knn, out_stride=2) == icp.ERR_ARG
    still_fine()
    assert _ext_raw(gctx, T, xyz, 3, n, knn, smooth=2) == icp.ERR_ARG
    assert _ext_raw(gctx, T, xyz, 3, n, knn, smooth=1, want_nrm=False) == icp.ERR_ARG
    assert _ext_raw(gctx, T, xyz, 3, n, knn, md=0.0) == icp.ERR_ARG
    still_fine()
    # pgicp_smooth_normals_*: an id >= n, an id below -1, a stride below 3, n < 0
    ids = o["ids"].copy()
    for bad in (n, n + 1000, -2):
        ids2 = ids.copy()
        ids2[n // 2, 1] = bad
        with pytest.raises(icp.PgicpError) as ei:
            gctx.smooth_normals(r["normals"], ids2)
        assert ei.value.code == icp.ERR_ARG
        same(gctx.smooth_normals(r["normals"], ids), r["smoothed"], "after a refused id")
        with pytest.raises(icp.PgicpError):
            gctx.smooth_normals(dev(r["normals"]), dev(ids2))
        still_fine()
    fn = getattr(gctx.lib, "pgicp_smooth_normals" + ("_f32" if T == np.float32 else "_f64"))
    nrm, out = np.ascontiguousarray(r["normals"]), np.zeros((n, 3), dtype=T)
    args = lambda ns, nn, os: (gctx.h, C.c_void_p(nrm.ctypes.data), C.c_int(ns), C.c_void_p(ids.ctypes.data), C.c_int(knn), C.c_int(nn),
                               C.c_int(icp.HOST), C.c_void_p(out.ctypes.data), C.c_int(os))
    assert fn(*args(2, n, 3)) == icp.ERR_ARG
    assert fn(*args(3, n, 2)) == icp.ERR_ARG
    assert fn(*args(3, -1, 3)) == icp.ERR_ARG
    assert fn(*args(3, n, 3)) == icp.OK and out.tobytes() == r["smoothed"].tobytes()
    still_fine()
