"""SurfaceNormalDataPointsFilter's further outputs through the C++ side.  Without a device (tests/cpp/
test_surface_normals_ext_cpu.cpp): the host statement (include/pgslam_amd/surface_normals_host.hpp) against the numpy reference bit
for bit on every scene in both types; YAML loading of the four parameters, alone and together, the fields they set and the one new
refusal; the companion header as strict C99; the library's exports against its declarations.  On the device (tests/cpp/
test_surface_normals_ext_gpu.cpp): the drop-in's descriptors against the direct call, SurfaceNormal{keepDensities,
keepEigenVectors} -> MaxDensity against the two filters by hand, and an ICP object whose reference chain smooths the normals."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import surface_normals_ext_ref as ref
from pgslam_amd import icp
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgicp_normals_ext.h")


def host_statement(exe, xyz, ids, T):
    """surface_normals_host.hpp through tests/cpp/test_surface_normals_ext_cpu host"""
    n, knn = ids.shape
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<ii", n, knn) + np.ascontiguousarray(xyz, dtype=T).tobytes() + np.ascontiguousarray(ids, dtype=np.int32).tobytes())
        out = subprocess.run([exe, "host", "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        b = np.fromfile(fout, dtype=T)
    widths = [("normals", 3), ("eigen_values", 3), ("eigen_vectors", 9), ("mean_dists", 1), ("matched_ids", knn), ("smoothed", 3)]
    assert len(b) == n * sum(w for _, w in widths)
    res, at = {}, 0
    for name, w in widths:
        res[name] = b[at:at + n * w].reshape(n, w)
        at += n * w
    return res


@pytest.mark.parametrize("T", ref.TYPES)
def test_host_statement_equals_the_reference(T):
    exe = build_exe("test_surface_normals_ext_cpu")
    scenes = [(name,) + ref.scene(name, T)[:1] + (ref.scene(name, T)[3]["ids"], ref.scene(name, T)[4]) for name in sorted(ref.SCENES)]
    xyz, interior = ref.plane_case(T)
    from oracle import Oracle
    ids = Oracle(T).surface_normals(xyz, 5, np.inf)["ids"]
    plane = ref.rows(xyz, ids, T)
    plane["smoothed"] = ref.smooth(plane["normals"], ids, T)
    scenes.append(("plane", xyz, ids, plane))
    for name, xyz, ids, r in scenes:
        got = host_statement(exe, xyz, ids, T)
        for key, val in got.items():
            assert val.tobytes() == np.ascontiguousarray(r[key]).reshape(val.shape).tobytes(), (name, key)


def test_yaml_loading_fields_refusal_and_exports():
    exe = build_exe("test_surface_normals_ext_cpu")
    out = subprocess.run([exe, "yaml"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "surface normals ext cpu tests ok" in out.stdout


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_normals_ext.h"\nint main(void) { return PGICP_NORMALS_EXT_MAX_IDS_F32 != 16777216; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.NORMALS_EXT_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched


@pytest.mark.gpu
def test_dropin_descriptors_max_density_chain_and_smoothing_icp():
    exe = build_exe("test_surface_normals_ext_gpu")
    env = dict(os.environ)
    for knob in ("PGSLAM_HOST_INPUT_STAGE", "PGSLAM_HOST_MAX_DENSITY"):
        env.pop(knob, None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "surface normals ext gpu tests ok" in out.stdout
