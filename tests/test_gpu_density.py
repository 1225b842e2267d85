"""The `densities` descriptor and MaxDensityDataPointsFilter on the device (include/pgicp_density.h, k_density.inc and the
epilogue of k_surface_normals) against the oracle's statements (orc_densities over orc_surface_normals' neighbour ids,
orc_max_density_keep): densities and kept indices bit for bit, in both precisions; the fused call against the two stage calls,
from host and from device memory; the refusals; independence from the context's history."""
import numpy as np
import pytest

from pgslam_amd import icp
from test_density_host import density_arrays

SIZES = lambda knn: (1, 2, knn - 1, knn, 257, 4099, 20011)      # across the 128- and 256-thread blocks and the multi-block reduction


def cloud(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3)) * 3


def oracle_densities(o, xyz, knn, max_dist=np.inf):
    r = o.surface_normals(xyz, knn, max_dist=max_dist)
    return o.densities(xyz, r["ids"]), r


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


@pytest.fixture(scope="module")
def dense_clouds(oracle32, oracle64):
    """clouds (as T) with the oracle's densities, computed once: name -> (xyz, knn, max_dist, densities)"""
    out = {}
    rng = np.random.default_rng(11)
    base = np.round(rng.normal(size=(300, 3)) * 3 * 64) / 64       # few mantissa bits: the sums and the mean of duplicates are exact
    iso = np.concatenate([rng.normal(size=(2000, 3)) * 0.5, rng.uniform(50, 90, size=(25, 3)) * np.array([1, -1, 1])])
    for T, o in ((np.float32, oracle32), (np.float64, oracle64)):
        for name, xyz, knn, md in (("normal4099", cloud(4099, 4099), 5, np.inf), ("isolated", iso, 5, 0.5),
                                   ("dup40", np.repeat(base, 40, axis=0)[rng.permutation(12000)], 5, np.inf)):
            x = np.ascontiguousarray(xyz, dtype=T)
            out[name, T] = (x, knn, md, oracle_densities(o, x, knn, md)[0])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("knn", [3, 5, 32])
def test_densities_normals_eigenvalues_bit_equal(ctx, oracle32, oracle64, T, knn):
    o = oracle32 if T == np.float32 else oracle64
    for n in SIZES(knn):
        xyz = np.ascontiguousarray(cloud(n, 100 * knn + n), dtype=T)
        want, _ = oracle_densities(o, xyz, knn)
        g = ctx.surface_densities(xyz, knn=knn)
        assert g["densities"].dtype == T and bits(g["densities"]) == want.tobytes(), f"n={n} knn={knn}"
        nrm, eig = ctx.surface_normals(xyz, knn=knn, want_eigen=True)
        assert bits(g["normals"]) == nrm.tobytes() and bits(g["eigen_values"]) == eig.tobytes(), f"n={n} knn={knn}"
        only = ctx.surface_densities(xyz, knn=knn, want_normals=False, want_eigen=False)      # any output may be NULL
        assert only["normals"] is None and bits(only["densities"]) == want.tobytes()
    # a strided (n, 4) cloud from device memory: device out
    import torch
    x4 = np.ones((4099, 4), dtype=T)
    x4[:, :3] = cloud(4099, 100 * knn + 4099)
    gd = ctx.surface_densities(torch.from_numpy(x4).cuda(), knn=knn)
    want, _ = oracle_densities(o, np.ascontiguousarray(x4[:, :3]), knn)
    assert gd["densities"].is_cuda and bits(gd["densities"]) == want.tobytes()
    assert bits(gd["normals"]) == bits(ctx.surface_normals(np.ascontiguousarray(x4[:, :3]), knn=knn))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_infinite_densities(ctx, dense_clouds, T):
    # isolated points within a finite maxDist: cnt = 1, r = 0, density +inf; exact duplicates: every neighbour coincides
    for name, at_least in (("isolated", 25), ("dup40", 12000)):
        xyz, knn, md, want = dense_clouds[name, T]
        g = ctx.surface_densities(xyz, knn=knn, max_dist=md)
        assert bits(g["densities"]) == want.tobytes(), name
        assert np.count_nonzero(np.isposinf(g["densities"])) >= at_least, name


def check_max_density(ctx, o, dens, md, seed, label):
    import torch
    want = np.flatnonzero(o.max_density_keep(dens, max_density=md, seed=seed)).astype(np.int32)
    got = ctx.max_density(dens, max_density=md, seed=seed)
    np.testing.assert_array_equal(got, want, err_msg=label)
    got_d = ctx.max_density(torch.from_numpy(dens).cuda(), max_density=md, seed=seed)
    assert got_d.is_cuda
    np.testing.assert_array_equal(got_d.cpu().numpy(), want, err_msg=label + " (device)")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_max_density_against_the_oracle(ctx, oracle32, oracle64, dense_clouds, T):
    o = oracle32 if T == np.float32 else oracle64
    for seed in (1, 77):
        for name in ("normal4099", "isolated", "dup40"):
            dens = dense_clouds[name, T][3]
            md = float(np.median(dens[np.isfinite(dens)])) if np.isfinite(dens).any() else 10.0
            want = check_max_density(ctx, o, dens, md, seed, f"{name} seed {seed}")
            if name == "normal4099":
                assert 0 < len(want) < len(dens)
            if name == "dup40":                        # all +inf, all saturated: the integer factor is 0
                assert len(want) == 0
        for name, dens, md in density_arrays(T):
            want = check_max_density(ctx, o, dens, md, seed, f"{name} seed {seed}")
            if name == "all_saturated":
                assert len(want) == 0
            if name in ("all_below", "one_below"):
                assert len(want) == len(dens)
    assert len(ctx.max_density(np.zeros(0, dtype=T))) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8192, 4_194_305])
def test_kept_indices_at_the_edges_of_the_scan(ctx, oracle32, n):
    """kept_idx comes out of the three-launch exclusive scan (launch_exclusive_scan), which has no entry point of its own: a
    chunk of 4096 elements less one, exactly, plus one, two chunks, and one element past 1024 chunks, where the scan of the
    block sums carries into its second trip.  (n = 1: `one_above` / `one_below` of density_arrays.)  Roughly half the points
    are kept: a fifth lies below maxDensity, a denser point stays with probability maxDensity / density."""
    dens = np.random.default_rng(n).uniform(1.0, 100.0, n).astype(np.float32)
    want = check_max_density(ctx, oracle32, dens, 20.0, 3, f"n={n}")
    assert 0.4 * n < len(want) < 0.6 * n


def fused_equals_stages(ctx, xyz, T, knn, md, seed, desc, device):
    import torch
    to = (lambda a: torch.from_numpy(a).cuda()) if device else (lambda a: a)
    st = ctx.surface_densities(xyz, knn=knn)
    keep = ctx.max_density(st["densities"], max_density=md, seed=seed)
    f = ctx.normals_max_density(to(xyz), knn=knn, max_density=md, seed=seed, descriptors=to(desc) if desc is not None else None)
    assert 0 < len(keep) < len(xyz)
    np.testing.assert_array_equal(bits(f["kept_idx"]), keep.tobytes())
    assert bits(f["xyz"]) == np.ascontiguousarray(xyz[keep, :3]).tobytes()
    assert bits(f["normals"]) == st["normals"][keep].tobytes()
    assert bits(f["eigen_values"]) == st["eigen_values"][keep].tobytes()
    assert bits(f["densities"]) == st["densities"][keep].tobytes()
    if desc is not None:
        assert bits(f["descriptors"]) == desc[keep].tobytes()
    return f, st, keep


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_fused_call_equals_the_stage_calls(ctx, T):
    rng = np.random.default_rng(3)
    for n, knn, stride, drows in ((4099, 5, 3, 0), (20011, 10, 4, 2), (257, 32, 3, 1)):
        xyz = np.ones((n, stride), dtype=T)
        xyz[:, :3] = cloud(n, n + knn)
        desc = rng.normal(size=(n, drows)).astype(T) if drows else None
        md = float(np.median(ctx.surface_densities(xyz, knn=knn)["densities"]))
        for device in (False, True):
            fused_equals_stages(ctx, xyz, T, knn, md, 9, desc, device)
    f = ctx.normals_max_density(np.zeros((0, 3), dtype=T), knn=5)
    assert len(f["kept_idx"]) == 0 and f["xyz"].shape == (0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_device_outputs_feed_a_device_map(T):
    import torch
    from pgslam_amd import synth
    w = synth.make_two_scans(6000, rings=16)
    ref, rd = np.ascontiguousarray(w["ref_xyz"], dtype=T), np.ascontiguousarray(w["reading_xyz"], dtype=T)
    c = icp.Context(0, max_dist=2.0, trim_ratio=0.85, max_iters=20)
    try:
        md = float(np.median(c.surface_densities(ref, knn=10)["densities"]))
        fd = c.normals_max_density(torch.from_numpy(ref).cuda(), knn=10, max_density=md, seed=4)
        fh = c.normals_max_density(ref, knn=10, max_density=md, seed=4)
        assert 0 < len(fh["kept_idx"]) < len(ref) and bits(fd["xyz"]) == fh["xyz"].tobytes() and bits(fd["normals"]) == fh["normals"].tobytes()
        res = []
        for x, nr in ((fd["xyz"], fd["normals"]), (np.ascontiguousarray(fh["xyz"]), fh["normals"])):
            mid = c.set_map(x, nr, center=True)
            Tm, st = c.align(mid, rd, w["T_init"])
            c.destroy_map(mid)
            res.append((Tm.tobytes(), st["iterations"], st["residual"], st["n_kept"]))
        assert res[0] == res[1]
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_argument_refusals(ctx, T):
    xyz = np.ascontiguousarray(cloud(100, 1), dtype=T)
    dens = np.full(10, 5.0, dtype=T)

    def refused(fn, *a, **k):
        with pytest.raises(icp.PgicpError) as e:
            fn(*a, **k)
        assert e.value.code == icp.ERR_ARG

    for knn in (2, 33):
        refused(ctx.surface_densities, xyz, knn=knn)
        refused(ctx.normals_max_density, xyz, knn=knn)
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[37, 1] = bad
        refused(ctx.surface_densities, x, knn=5)
        refused(ctx.normals_max_density, x, knn=5)
    for md in (0.0, -1.0, np.nan):
        refused(ctx.max_density, dens, max_density=md)
        refused(ctx.normals_max_density, xyz, knn=5, max_density=md)
    for seed in (2 ** 53, 2 ** 63):
        refused(ctx.max_density, dens, seed=seed)
        refused(ctx.normals_max_density, xyz, knn=5, seed=seed)
    assert len(ctx.max_density(dens, seed=2 ** 53 - 1)) == 10
    sfx = "_f32" if T == np.float32 else "_f64"
    import ctypes as C
    n_out = C.c_int(5)
    assert getattr(ctx.lib, "pgicp_max_density" + sfx)(ctx.h, C.c_void_p(dens.ctypes.data), C.c_int(-1), C.c_int(icp.HOST), C.c_double(1.0),
                                                        C.c_uint64(1), None, C.byref(n_out)) == icp.ERR_ARG
    assert getattr(ctx.lib, "pgicp_surface_densities" + sfx)(ctx.h, C.c_void_p(xyz.ctypes.data), C.c_int(3), C.c_int(-1), C.c_int(icp.HOST), C.c_int(5),
                                                              C.c_double(1.0), None, C.c_int(3), None, None) == icp.ERR_ARG
    # n == 0: nothing to do, n_out = 0
    assert getattr(ctx.lib, "pgicp_max_density" + sfx)(ctx.h, None, C.c_int(0), C.c_int(icp.HOST), C.c_double(1.0), C.c_uint64(1), None,
                                                        C.byref(n_out)) == icp.OK and n_out.value == 0
    ctx.surface_densities(xyz, knn=5)                      # the context is usable after the refusals


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_independent_of_call_history(T):
    from pgslam_amd import synth
    xyz = np.ascontiguousarray(cloud(4099, 8), dtype=T)
    w = synth.make_two_scans(3000, rings=16)

    def snapshot(c):
        md = 40.0
        f = c.normals_max_density(xyz, knn=7, max_density=md, seed=5)
        d = c.surface_densities(xyz, knn=7)
        k = c.max_density(d["densities"], max_density=md, seed=5)
        return tuple(bits(f[key]) for key in ("xyz", "normals", "eigen_values", "densities", "kept_idx")) + (bits(d["densities"]), k.tobytes())

    c = icp.Context(0, max_dist=2.0)
    try:
        first = snapshot(c)
        assert snapshot(c) == first                                           # the same call twice
        c.normals_max_density(np.ascontiguousarray(cloud(20011, 2), dtype=T), knn=32, max_density=1.0, seed=1)      # larger scratch in between
        mid = c.set_map(np.ascontiguousarray(w["ref_xyz"], dtype=T), np.ascontiguousarray(w["ref_nrm"], dtype=T))
        c.align(mid, np.ascontiguousarray(w["reading_xyz"], dtype=T), np.eye(4))                                      # an unrelated align
        assert snapshot(c) == first
    finally:
        c.close()
    fresh = icp.Context(0)
    try:
        assert snapshot(fresh) == first                                       # and another context
    finally:
        fresh.close()
