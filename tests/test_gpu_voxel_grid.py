"""VoxelGridDataPointsFilter on the device (pgicp_voxel_grid_*, k_voxel.inc) against the numpy statement of
tests/voxel_grid_ref.py: points, descriptors, kept indices and counts bit for bit, in both precisions.  And the drop-in: the
device path leaves the DataPoints its host form leaves (tests/cpp/test_voxel_grid_cpu.cpp apply), and an ICP object and a
PoseGraphSlam give the same poses on both paths (tests/cpp/test_voxel_grid_gpu.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pgslam_amd import icp
from test_voxel_grid_host import apply_dropin, build_exe
from voxel_grid_ref import grid, voxel_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def check(ctx, xyz, T, v, cen=True, desc=None, avg=True, label=""):
    g = ctx.voxel_grid(xyz, v_size=v, use_centroid=cen, descriptors=desc, average_descriptors=avg, dtype=T)
    r = voxel_grid(np.asarray(xyz), v, cen, desc, avg, T)
    np.testing.assert_array_equal(g["kept_idx"], r["kept_idx"], err_msg=label)
    np.testing.assert_array_equal(g["count"], r["count"], err_msg=label)
    assert g["xyz"].dtype == T and g["xyz"].tobytes() == r["xyz"].tobytes(), label
    if desc is not None:
        assert g["descriptors"].tobytes() == r["descriptors"].tobytes(), label
    return g, r


@pytest.fixture(scope="module")
def clouds():
    sys.path.insert(0, ROOT)
    from bench import build_pairs, build_workload
    xyz, _, _ = build_pairs(100000)
    w = build_workload(100000, 1000000, 16)
    rng = np.random.default_rng(5)
    return dict(scan100k=xyz[0], map1M=w.map_xyz, uni100k=rng.uniform(-30, 30, size=(100000, 3)),
                uni1M=rng.uniform(-50, 50, size=(1000000, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_parity_scans_and_maps(ctx, clouds, T):
    rng = np.random.default_rng(1)
    for name, sizes in (("scan100k", [(0.05,) * 3, (0.3,) * 3, (2.0,) * 3, (0.1, 0.4, 1.0)]), ("uni100k", [(0.5,) * 3, (0.05, 2.0, 0.2)]),
                        ("map1M", [(0.2,) * 3, (2.0, 1.0, 0.5)]), ("uni1M", [(1.0,) * 3])):
        xyz = np.asarray(clouds[name], dtype=T)
        for v in sizes:
            for cen in (True, False):
                d = rng.normal(size=(len(xyz), 3)).astype(T)
                g, r = check(ctx, xyz, T, v, cen, d, cen, label=f"{name} {v} cen={cen}")
                assert 0 < len(g["kept_idx"]) < len(xyz)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_edges(ctx, T):
    rng = np.random.default_rng(2)
    u = rng.uniform(-10, 10, size=(20000, 3))
    g, _ = check(ctx, u, T, (1e-4,) * 3, True, rng.normal(size=(20000, 2)).astype(T), label="alone")          # every point alone
    assert len(g["kept_idx"]) == 20000 and np.all(g["count"] == 1)
    for n in (100000, 1000000):                                                                              # all in one voxel
        x = rng.uniform(-3, 3, size=(n, 3))
        for cen in (True, False):
            g, _ = check(ctx, x, T, (50.0,) * 3, cen, rng.normal(size=(n, 3)).astype(T), True, label=f"one voxel {n}")
            assert g["count"].tolist() == [n]
    lat = rng.integers(-20, 20, size=(30000, 3)) * 0.25                                                     # on voxel boundaries
    for v in ((0.25,) * 3, (0.5, 0.25, 1.0), (0.125,) * 3):
        check(ctx, lat, T, v, True, label=f"lattice {v}")
        check(ctx, lat, T, v, False, label=f"lattice {v}")
    base = rng.normal(size=(2000, 3)) * 4                                                                    # 40-fold duplicates
    dup = np.repeat(base, 40, axis=0)[rng.permutation(80000)]
    g, _ = check(ctx, dup, T, (0.05,) * 3, True, rng.normal(size=(80000, 1)).astype(T), label="dup40")
    assert g["count"].max() >= 40
    for off in (1e5, -1e5):                                                                                  # far offsets
        check(ctx, rng.uniform(-5, 5, size=(20000, 3)) + off, T, (0.2,) * 3, True, label=f"offset {off}")
        check(ctx, rng.uniform(-5, 5, size=(20000, 3)) + off, T, (0.2,) * 3, False, label=f"offset {off}")
    g = ctx.voxel_grid(np.zeros((0, 3), dtype=T))                                                            # n = 0, n = 1
    assert len(g["kept_idx"]) == 0 and len(g["count"]) == 0
    g, _ = check(ctx, np.array([[-0.0, 1.5, -2.25]]), T, (0.3, 0.3, 0.3), True, np.array([[7.0, -0.0]], dtype=T), label="n=1")
    assert g["kept_idx"].tolist() == [0] and g["count"].tolist() == [1]
    x = rng.normal(size=(30000, 3)) * 3                                                                      # drows 0, 1, 3, 7, both flags
    for drows in (0, 1, 3, 7):
        d = rng.normal(size=(30000, drows)).astype(T) if drows else None
        for cen in (True, False):
            for avg in (True, False):
                check(ctx, x, T, (0.4, 0.4, 0.4), cen, d, avg, label=f"drows={drows} cen={cen} avg={avg}")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_every_pass_count_of_the_sort(ctx, T):
    """4097 points -- two tiles of the sort, the second holding one pair -- at voxel sizes whose keys take 1 .. 8 passes of 8 bits:
    which buffer the sort's result lies in (odd and even pass counts) and the shift of every pass"""
    x = np.random.default_rng(11).uniform(-10, 10, size=(4097, 3))
    passes = []
    for k in (0, 3, 6, 8, 11, 14, 17, 19):
        v = (20 / 2 ** k,) * 3
        nd = [int(a) for a in grid(x, v, T)[2]]                   # the statement's numDiv in T
        passes.append(-(-(nd[0] + nd[1] * nd[0] + nd[2] * nd[0] * nd[1]).bit_length() // 8))
        for cen in (True, False):
            check(ctx, x, T, v, cen, label=f"k={k} passes={passes[-1]} cen={cen}")
    assert passes == [1, 2, 3, 4, 5, 6, 7, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_heavy_voxel_two_row_passes(ctx, T):
    """one voxel of c points -- one point into the second chunk of 512, one into the third, a ragged tail -- summed by a block over
    10 rows (3 coordinates, 7 descriptor rows): two row passes, of 8 and of 2; 50 more points lie in voxels of their own"""
    rng = np.random.default_rng(12)
    for c in (513, 1025, 1100):
        x = np.concatenate([rng.uniform(0, 5, size=(c, 3)), rng.uniform(60, 2000, size=(50, 3))])[rng.permutation(c + 50)]
        d = rng.normal(size=(c + 50, 7)).astype(T)
        for stride in (3, 4):
            h = np.ones((c + 50, stride), dtype=T)
            h[:, :3] = x
            g, _ = check(ctx, h, T, (50.0,) * 3, True, d, True, label=f"c={c} stride={stride}")
            assert g["count"].max() == c and np.sort(g["count"])[-2] <= 64


@pytest.mark.gpu
def test_strided_and_torch(ctx):
    import torch
    rng = np.random.default_rng(3)
    for T, tt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        h = np.ones((50000, 4), dtype=T)
        h[:, :3] = rng.normal(size=(50000, 3)) * 5
        d = rng.normal(size=(50000, 3)).astype(T)
        r = voxel_grid(h, (0.3, 0.3, 0.3), True, d, True, T)
        g = ctx.voxel_grid(h, (0.3, 0.3, 0.3), descriptors=d)                        # stride 4, host
        assert g["xyz"].tobytes() == r["xyz"].tobytes() and g["descriptors"].tobytes() == r["descriptors"].tobytes()
        th, td = torch.from_numpy(h).cuda(), torch.from_numpy(d).cuda()             # stride 4, device in -> device out
        g = ctx.voxel_grid(th, (0.3, 0.3, 0.3), descriptors=td)
        assert g["xyz"].is_cuda and g["xyz"].dtype == tt
        assert g["xyz"].cpu().numpy().tobytes() == r["xyz"].tobytes()
        assert g["descriptors"].cpu().numpy().tobytes() == r["descriptors"].tobytes()
        assert g["kept_idx"].cpu().numpy().tolist() == r["kept_idx"].tolist() and g["count"].cpu().numpy().tolist() == r["count"].tolist()


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(ctx):
    ok = np.random.default_rng(4).normal(size=(1000, 3))
    for T in (np.float32, np.float64):
        for xyz, v in ((np.array([[0, 0, 0], [np.nan, 0, 0]]), (1, 1, 1)), (np.array([[0, 0, 0], [0, np.inf, 0]]), (1, 1, 1)),
                       (np.array([[0, 0, 0], [1e4, 0, 0]]), (1e-6, 1, 1)), (np.array([[0, 0, 0], [1e6, 1e6, 1e6]]), (1e-3, 1e-3, 1e-3)),
                       (ok, (0, 1, 1)), (ok, (1, -1, 1)), (ok, (1, 1, np.nan)), (ok, (np.inf, 1, 1))):
            with pytest.raises(icp.PgicpError) as e:
                ctx.voxel_grid(np.asarray(xyz, dtype=T), v)
            assert e.value.code == icp.ERR_ARG
        check(ctx, ok, T, (0.5, 0.5, 0.5), True, label="after the refusals")


@pytest.mark.gpu
def test_dropin_device_path_equals_host_form():
    exe = build_exe()
    rng = np.random.default_rng(6)
    for T in (np.float32, np.float64):
        for xyz, v in ((rng.normal(size=(40000, 3)) * 4, (0.2, 0.2, 0.2)), (rng.uniform(-2, 2, size=(20000, 3)), (10.0, 10.0, 10.0)),
                       (rng.integers(-10, 10, size=(20000, 3)) * 0.5, (0.5, 1.0, 0.5))):
            xyz = xyz.astype(T)
            row3 = rng.uniform(0.5, 2, len(xyz)).astype(T)
            for cen, avg, drows in ((True, True, 3), (False, False, 4), (True, False, 1), (False, True, 0)):
                desc = rng.normal(size=(len(xyz), drows)).astype(T) if drows else None
                dv = apply_dropin(exe, xyz, T, v, cen, avg, desc, row3, host=False)
                hs = apply_dropin(exe, xyz, T, v, cen, avg, desc, row3, host=True)
                assert dv["on_device"] == 1 and hs["on_device"] == 0
                assert dv["features"].tobytes() == hs["features"].tobytes()
                assert dv["descriptors"].tobytes() == hs["descriptors"].tobytes() and dv["labels"] == hs["labels"]
        bad = np.array([[0, 0, 0], [np.nan, 0, 0]], dtype=T)                        # the device refuses, the host form throws
        assert apply_dropin(exe, bad, T, (1, 1, 1), True, True, host=False)["refused"]


@pytest.mark.gpu
def test_dropin_icp_and_slam_device_equals_host():
    exe = os.path.join(CPP, "test_voxel_grid_gpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-local-typedefs", "-Wno-unused-variable", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp",
                           "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "voxel grid gpu tests ok" in out.stdout
