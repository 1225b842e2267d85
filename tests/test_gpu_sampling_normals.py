"""SamplingSurfaceNormalDataPointsFilter on the device (pgicp_sampling_surface_normal_*, k_ssn.inc) against the oracle's statement
(orc_sampling_surface_normal): the keep mask, the kept indices, the kept points and the boxes fused bit for bit; the normals too
(the same Jacobi on the same T sums), asserted to rounding and sign.  And the drop-in shim's filter: the device path leaves the
DataPoints the host recursion leaves."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from pgslam_amd import icp, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {np.float32: 1e-6, np.float64: 1e-13}


def check(ctx, o, xyz, T, knn=7, ratio=0.5, method=0, max_box=np.inf, seed=1, label=""):
    xyz = np.ascontiguousarray(xyz, dtype=T)
    g = ctx.sampling_surface_normal(xyz, knn=knn, ratio=ratio, sampling_method=method, max_box_dim=max_box, seed=seed)
    r = o.sampling_surface_normal(xyz, knn=knn, ratio=ratio, sampling_method=method, max_box_dim=max_box, seed=seed)
    k = np.flatnonzero(r["keep"])
    assert g["boxes"] == r["boxes"], label
    np.testing.assert_array_equal(g["kept_idx"], k, err_msg=label)
    assert g["xyz"].tobytes() == r["xyz"][k].tobytes(), label
    nd, nr = g["normals"].astype(np.float64), r["normals"][k].astype(np.float64)
    unequal = int(np.count_nonzero(g["normals"] != r["normals"][k]))
    if unequal:
        print(f"{label}: {unequal} normal components not bit-equal")
    if len(k):
        assert np.abs(nd - nr).max() <= TOL[T], label
        assert np.all(np.sign(nd) == np.sign(nr)) or np.all(np.sum(nd * nr, 1) > 0), label
    return g, r


@pytest.fixture(scope="module")
def clouds():
    sys.path.insert(0, ROOT)
    from bench import build_pairs, build_workload
    xyz, _, _ = build_pairs(100000)
    w = build_workload(100000, 1000000, 16)
    return dict(scan7k=synth.make_two_scans(7000, rings=16)["ref_xyz"], scan100k=xyz[0], map1M=w.map_xyz)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("name", ["scan7k", "scan100k", "map1M"])
def test_parity_with_the_oracle(ctx, oracle32, oracle64, clouds, T, method, name):
    o = oracle32 if T == np.float32 else oracle64
    g, r = check(ctx, o, clouds[name], T, knn=7, ratio=0.5, method=method, seed=3, label=f"{name} {T.__name__} m{method}")
    assert 0 < len(g["kept_idx"]) < len(clouds[name])


@pytest.mark.gpu
@pytest.mark.parametrize("knn", [3, 7, 10, 32, 64])
def test_shapes_and_knn_edges(ctx, oracle32, oracle64, knn):
    rng = np.random.default_rng(knn)
    for T, o in ((np.float32, oracle32), (np.float64, oracle64)):
        for n in (1, 2, knn, knn + 1, 2 * knn + 1, 1000, 4099):
            xyz = rng.normal(size=(n, 3)) * 3
            for method in (0, 1):
                check(ctx, o, xyz, T, knn=knn, method=method, seed=n, label=f"n={n} knn={knn}")
        g = ctx.sampling_surface_normal(np.zeros((0, 3), dtype=T), knn=knn)
        assert len(g["kept_idx"]) == 0 and g["boxes"] == 0


@pytest.mark.gpu
def test_ties_zeros_duplicates_and_degenerate_boxes(ctx, oracle32, oracle64):
    rng = np.random.default_rng(11)
    n = 20000
    grid = rng.integers(-4, 5, size=(n, 3)) * 0.25                 # a coarse grid: runs of equal coordinates
    signed = grid.copy()
    z = signed == 0
    signed[z] = np.where(rng.random(z.sum()) < 0.5, -0.0, 0.0)      # -0.0 and +0.0 mixed
    base = rng.normal(size=(n // 8, 3))
    dup = base[rng.integers(0, len(base), n)]                        # duplicate points: rank-0 boxes dropped
    line = rng.normal(size=(n, 3))
    line[: n // 2, 1:] = 0.0                                         # collinear runs: rank-1 boxes dropped
    line[: n // 2, 0] = np.round(line[: n // 2, 0], 1)
    for T, o in ((np.float32, oracle32), (np.float64, oracle64)):
        for name, xyz in (("grid", grid), ("signed_zeros", signed), ("duplicates", dup), ("collinear", line)):
            for method in (0, 1):
                for knn in (3, 7, 10):
                    g, r = check(ctx, o, xyz, T, knn=knn, method=method, seed=5, label=f"{name} {T.__name__} m{method} knn{knn}")
        g, r = check(ctx, o, dup, T, knn=7, label="dup")
        assert r["boxes"] < len(dup) // 7                           # some boxes were dropped


@pytest.mark.gpu
def test_parameters_max_box_dim_and_ratio(ctx, oracle32, oracle64):
    xyz = synth.make_two_scans(7000, rings=16)["ref_xyz"]
    for T, o in ((np.float32, oracle32), (np.float64, oracle64)):
        full, _ = check(ctx, o, xyz, T, knn=7, max_box=np.inf, label="inf")
        small, r = check(ctx, o, xyz, T, knn=7, max_box=0.5, label="maxBoxDim 0.5")
        assert small["boxes"] < full["boxes"]
        g0, _ = check(ctx, o, xyz, T, ratio=0.0, label="ratio 0")
        assert len(g0["kept_idx"]) == 0 and g0["boxes"] == full["boxes"]
        g1, r1 = check(ctx, o, xyz, T, ratio=1.0, label="ratio 1")
        assert len(g1["kept_idx"]) == r1["keep"].sum() > len(xyz) // 2
        check(ctx, o, xyz, T, ratio=0.3, seed=123456789, label="ratio 0.3")


@pytest.mark.gpu
def test_descriptors_averaged_or_compacted(ctx):
    xyz = synth.make_two_scans(7000, rings=16)["ref_xyz"]
    for T in (np.float32, np.float64):
        x = np.ascontiguousarray(xyz, dtype=T)
        g = ctx.sampling_surface_normal(x, knn=9, sampling_method=1, descriptors=x)
        assert g["descriptors"].tobytes() == g["xyz"].tobytes()          # the mean of the box, the same sums
        const = np.full((len(x), 2), 0.1, dtype=T)
        g = ctx.sampling_surface_normal(x, knn=9, sampling_method=1, descriptors=const)
        assert np.all(g["descriptors"] == T(0.1)) or np.allclose(g["descriptors"], 0.1)
        g = ctx.sampling_surface_normal(x, knn=9, sampling_method=1, descriptors=x, average_descriptors=False)
        assert g["descriptors"].tobytes() == x[g["kept_idx"]].tobytes()
        d = np.random.default_rng(2).normal(size=(len(x), 3)).astype(T)
        g = ctx.sampling_surface_normal(x, knn=9, sampling_method=0, descriptors=d)
        assert g["descriptors"].tobytes() == d[g["kept_idx"]].tobytes()


@pytest.mark.gpu
def test_device_memory_gives_the_same_bits(ctx):
    import torch
    xyz = synth.make_two_scans(7000, rings=16)["ref_xyz"]
    for T in (np.float32, np.float64):
        x = np.ascontiguousarray(xyz, dtype=T)
        d = np.random.default_rng(3).normal(size=(len(x), 2)).astype(T)
        for method in (0, 1):
            h = ctx.sampling_surface_normal(x, knn=7, sampling_method=method, descriptors=d)
            g = ctx.sampling_surface_normal(torch.from_numpy(x).cuda(), knn=7, sampling_method=method, descriptors=torch.from_numpy(d).cuda())
            assert g["xyz"].is_cuda and g["boxes"] == h["boxes"]
            for k in ("xyz", "normals", "kept_idx", "descriptors"):
                assert g[k].cpu().numpy().tobytes() == h[k].tobytes(), k
            # a padded (n, 4) cloud reads the same points
            x4 = np.concatenate([x, np.ones((len(x), 1), dtype=T)], 1)
            g4 = ctx.sampling_surface_normal(x4, knn=7, sampling_method=method)
            assert g4["xyz"].tobytes() == h["xyz"].tobytes()


@pytest.mark.gpu
def test_nan_or_infinite_coordinates_are_refused(ctx):
    xyz = np.random.default_rng(4).normal(size=(500, 3)).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[17, 1] = bad
        with pytest.raises(icp.PgicpError) as e:
            ctx.sampling_surface_normal(x)
        assert e.value.code == icp.ERR_ARG
    with pytest.raises(icp.PgicpError) as e:
        ctx.sampling_surface_normal(xyz, knn=2)
    assert e.value.code == icp.ERR_ARG
    ctx.sampling_surface_normal(xyz)                                    # the context is still good


def _shim(tmp_path, T, yaml, xyz, desc):
    from test_cpp_dropin import build
    exe = build("ssn_device_apply")
    n, drows = len(xyz), 0 if desc is None else desc.shape[1]
    fi, fo, fy = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "f.yaml"
    fy.write_text(yaml)
    body = np.ascontiguousarray(xyz, dtype=T).tobytes() + (b"" if desc is None else np.ascontiguousarray(desc, dtype=T).tobytes())
    fi.write_bytes(struct.pack("ii", n, drows) + body)
    out = subprocess.run([exe, "f64" if T == np.float64 else "f32", str(fy), str(fi), str(fo)], capture_output=True, text=True, timeout=300,
                         env={k: v for k, v in os.environ.items() if k != "PGSLAM_HOST_SAMPLING_NORMALS"})
    assert out.returncode == 0, out.stdout + out.stderr
    line = [s for s in out.stdout.splitlines() if s.startswith("ran_on_device")][0]
    return dict(kv.split("=") for kv in line.split()[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_dropin_filter_runs_on_the_device_and_leaves_the_hosts_datapoints(tmp_path, T):
    xyz = synth.make_two_scans(7000, rings=16)["ref_xyz"]
    desc = np.random.default_rng(6).normal(size=(len(xyz), 3))
    for method in (0, 1):
        for avg in (0, 1):
            yaml = ("- SamplingSurfaceNormalDataPointsFilter:\n    ratio: 0.4\n    knn: 9\n    samplingMethod: %d\n    maxBoxDim: 1.5\n"
                    "    averageExistingDescriptors: %d\n    seed: 23\n" % (method, avg))
            for d in (None, desc):
                r = _shim(tmp_path, T, yaml, xyz, d)
                assert r["off"] == "1" and r["on"] == "0", r
                assert r["identical"] == "1", (method, avg, d is None)
                assert 0 < int(r["n_out"]) < len(xyz)
    # an infinite coordinate: the device refuses the cloud, the host recursion runs
    bad = xyz.copy()
    bad[5, 0] = np.inf
    r = _shim(tmp_path, T, "- SamplingSurfaceNormalDataPointsFilter:\n    knn: 7\n", bad, None)
    assert r["off"] == "0" and r["on"] == "0" and r["identical"] == "1"
