"""[EXT] OctreeGridDataPointsFilter and include/pgicp_octree.h without a device: the numpy reference's two transliterations
against each other on every cloud the device test uses and against three hand-written clouds, the C++ drop-in's host form
(tests/cpp/test_octree_grid_cpu.cpp) against the reference bit for bit, its YAML loading and refusals, the header as strict C99,
and the library's exports against the header's declarations."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import octree_grid_ref as ref
from pgslam_amd import icp
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgicp_octree.h")
KEYS = ("kept_idx", "count", "depth", "xyz", "desc")


def same(a, b, what=""):
    for k in KEYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, a[k], b[k])


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_two_transliterations_agree(T):
    for case in ref.CASES:
        _, mp, ms, method, _, _ = case
        x, d = ref.case_inputs(case, T)
        same(ref.recursive(x, d, mp, ms, method, ref.SEED, T), ref.case_expected(case, T), ref.case_id(case))


def test_the_cases_reach_what_they_are_for():
    """the depth cap, a deep pair under it, a leaf by size among leaves by count, a root leaf, leaves past the block path's chunk"""
    by = {ref.case_id(c): c for c in ref.CASES}
    for T in (np.float32, np.float64):
        w = ref.case_expected(by["coincident-p1-s0-m0-st3-d0"], T)
        assert w["depth"].max() == ref.MAX_DEPTH and w["count"][w["depth"].argmax()] == 2
        w = ref.case_expected(by["n257-p1-s100-m2-st3-d3"], T)
        assert len(w["count"]) == 1 and w["depth"][0] == 0 and w["count"][0] == 257
        w = ref.case_expected(by["n4097-p3-s1.5-m2-st3-d3"], T)
        assert (w["count"] > 3).any() and (w["depth"][w["count"] <= 3] < w["depth"].max()).any()
        for name in ("cluster3000-p100-s6-m2-st3-d7", "cluster3000-p100-s6-m3-st4-d3", "cluster3000-p1000-s0-m2-st3-d0"):
            assert ref.case_expected(by[name], T)["count"].max() > 512
    w = ref.case_expected(by["close_pair-p1-s0-m0-st3-d0"], np.float64)
    assert 15 <= w["depth"].max() < ref.MAX_DEPTH and (w["count"] == 1).all()


# the points (+-1, +-1, +-1) in child order and one point ON the root's plane x = 0: it falls to the lower child (6, with point 6),
# which splits once more about (-0.5, 0.5, 0.5): point 8 to its child 1, point 6 to its child 6
LATTICE = np.array([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [1, 1, -1], [-1, -1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, 1], [0, 0.5, 0.5]], dtype=np.float64)
# a box 0 .. 8 (centre 4, r 4) with five coincident points at (3, 3, 3): child 0 of the root holds them and (0, 0, 0); its centre is
# (2, 2, 2), so (0, 0, 0) goes to its child 0 and the five to its child 7, and on down to the cap
COINCIDENT = np.array([[3, 3, 3], [0, 0, 0], [3, 3, 3], [3, 3, 3], [8, 8, 8], [3, 3, 3], [3, 3, 3]], dtype=np.float64)
# extents (2, 2, 4): r = 2, and r * 2 = 4 <= maxSizeByNode: the root is a leaf
SMALL = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 4]], dtype=np.float64)
HAND = [
    # (name, cloud, maxPointByNode, maxSizeByNode, method, kept_idx, count, depth, xyz or None: the kept points' own)
    ("lattice", LATTICE, 1, 0.0, 0, [0, 1, 2, 3, 4, 5, 8, 6, 7], [1] * 9, [1, 1, 1, 1, 1, 1, 2, 2, 1], None),
    ("lattice centroid", LATTICE, 2, 0.0, 2, [0, 1, 2, 3, 4, 5, 6, 7], [1, 1, 1, 1, 1, 1, 2, 1], [1] * 8,
     [[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [1, 1, -1], [-1, -1, 1], [1, -1, 1], [-0.5, 0.75, 0.75], [1, 1, 1]]),
    ("coincident", COINCIDENT, 1, 0.0, 0, [1, 0, 4], [1, 5, 1], [2, 21, 1], None),
    ("coincident medoid", COINCIDENT, 1, 0.0, 3, [1, 0, 4], [1, 5, 1], [2, 21, 1], None),
    # the five alone: no extent, r = 0 and 0 * 2 <= 0 -- the root is a leaf by the size rule, whatever maxPointByNode
    ("coincident alone", COINCIDENT[[0, 2, 3, 5, 6]], 1, 0.0, 0, [0], [5], [0], None),
    ("root by size", SMALL, 1, 4.0, 0, [0], [4], [0], None),
    ("root by size centroid", SMALL, 1, 10.0, 2, [0], [4], [0], [[1, 1, 1]]),
    ("root by size medoid", SMALL, 1, 4.0, 3, [0], [4], [0], None),           # squared distances 3, 3, 3, 11: the tie goes to index 0
    ("just above the size", SMALL, 4, 3.99, 0, [0], [4], [0], None),          # the count rule holds at the root
    ("split by size", SMALL, 1, 3.99, 0, [0, 1, 2, 3], [1] * 4, [1] * 4, None),
]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_hand_written_clouds(T):
    exe = build_exe("test_octree_grid_cpu")
    for name, pts, mp, ms, method, kept, count, depth, xyz in HAND:
        x = np.ascontiguousarray(pts, dtype=T)
        want = dict(kept_idx=np.array(kept, dtype=np.int32), count=np.array(count, dtype=np.int32), depth=np.array(depth, dtype=np.int32),
                    xyz=np.array(xyz, dtype=T) if xyz is not None else x[kept], desc=None)
        same(ref.recursive(x, None, mp, ms, method, ref.SEED, T), want, name + " (recursive)")
        same(ref.coded(x, None, mp, ms, method, ref.SEED, T), want, name + " (coded)")
        same(host_form(exe, x, None, mp, ms, method, ref.SEED, T), want, name + " (host form)")


def host_form(exe, x, d, mp, ms, method, seed, T):
    """the drop-in's host form through tests/cpp/test_octree_grid_cpu apply"""
    drows = 0 if d is None else d.shape[1]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<iiiidd", len(x), mp, method, drows, float(ms), float(seed)) + x.tobytes() + (d.tobytes() if d is not None else b""))
        env = dict(os.environ, PGSLAM_HOST_INPUT_STAGE="1")
        out = subprocess.run([exe, "apply", "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        b = open(fout, "rb").read()
    m, = struct.unpack_from("<i", b, 0)
    rec = np.dtype([("i", "<i4"), ("xyz", T, (3,)), ("desc", T, (drows,))])
    leaves = np.frombuffer(b, dtype=rec, count=m, offset=4)
    tail = np.frombuffer(b, dtype=np.int32, count=2 * m, offset=4 + m * rec.itemsize)
    assert len(b) == 4 + m * rec.itemsize + 8 * m
    return dict(kept_idx=leaves["i"].astype(np.int32), count=tail[:m].copy(), depth=tail[m:].copy(), xyz=leaves["xyz"].reshape(m, 3).copy(),
                desc=leaves["desc"].reshape(m, drows).copy() if drows else None)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_host_form_equals_the_reference(T):
    exe = build_exe("test_octree_grid_cpu")
    for case in ref.CASES:
        _, mp, ms, method, _, _ = case
        x, d = ref.case_inputs(case, T)
        same(host_form(exe, x, d, mp, ms, method, ref.SEED, T), ref.case_expected(case, T), ref.case_id(case))


def test_yaml_loading_and_refusals():
    exe = build_exe("test_octree_grid_cpu")
    out = subprocess.run([exe, "yaml"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "octree grid cpu tests ok" in out.stdout


def test_reference_refuses_what_the_statement_refuses():
    x = np.zeros((3, 3), dtype=np.float32)
    for f in (ref.recursive, ref.coded):
        for mp, ms, method in ((0, 0.0, 0), (1, -1.0, 0), (1, np.inf, 0), (1, 0.0, 4)):
            with pytest.raises(ValueError):
                f(x, None, mp, ms, method, 1, np.float32)
        bad = x.copy()
        bad[1, 2] = np.nan
        with pytest.raises(ValueError):
            f(bad, None, 1, 0.0, 0, 1, np.float32)


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_octree.h"\nint main(void) { return PGICP_OCTREE_MAX_DEPTH != 21; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.OCTREE_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
