"""include/pgicp_sensor_chain.h without a device: the numpy statement (tests/sensor_chain_ref.py) against the oracle's own functions
stage by stage; the condition the GPU tests rest on -- in the main scene both dropping stages keep between 10 % and 90 % of what
reaches them --; the per-point functions of include/pgslam_amd/sensor_chain_host.hpp (which the kernels call) through the drop-in's
host filters against the statement, bit for bit, on vectors that hold a zero normal and the origin; the run detection of
DataPointsFilters (tests/cpp/test_sensor_chain_cpu.cpp); the header as strict C99 and the library's exports."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import sensor_chain_ref as ref
from pgslam_amd import icp
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgicp_sensor_chain.h")


@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_reference_equals_the_oracles_pieces_stage_by_stage(T):
    o = ref.oracle(T)
    x = ref.scene(ref.MAIN_N, T)
    h = ref.head(x, T)
    r = o.surface_normals(x, ref.KNN)
    assert h["normals"].tobytes() == r["normals"].tobytes() and h["eigen_values"].tobytes() == r["eigen_values"].tobytes()
    assert h["densities"].tobytes() == o.densities(x, r["ids"]).tobytes()
    md = ref.pick_max_density(x, T)
    every = np.arange(len(x))
    # each stage alone behind the head
    sh = np.flatnonzero(o.shadow_keep(x, h["normals"], eps_angle=ref.EPS))
    assert np.array_equal(ref.run(x, T, [(ref.SHADOW, ref.EPS)])["kept_idx"], sh)
    mk = np.flatnonzero(o.max_density_keep(h["densities"], max_density=md, seed=ref.SEED))
    assert np.array_equal(ref.run(x, T, [(ref.MAXDENS, md, ref.SEED)])["kept_idx"], mk)
    for st in range(5):
        assert ref.run(x, T, [(ref.NOISE, st, 1.5)])["noise"].tobytes() == o.simple_sensor_noise(x, sensor_type=st, gain=1.5).tobytes()
    c = np.array([0.5, -0.25, 1.0], dtype=T)
    obs = ref.run(x, T, [(ref.OBS, 0.5, -0.25, 1.0)])["observation_directions"]
    assert obs.dtype == T and all(obs[i, a] == c[a] - x[i, a] for i in range(0, len(x), 97) for a in range(3))
    # the flip, scalar by scalar in the stated order, on every 41st point
    for toward in (1, 0):
        got = ref.run(x, T, [(ref.OBS, 0.5, -0.25, 1.0), (ref.ORIENT, toward)], keep=("normals",))["normals"]
        for i in range(0, len(x), 41):
            n_, o_ = h["normals"][i], obs[i]
            dot = ((T(0) + n_[0] * o_[0]) + n_[1] * o_[1]) + n_[2] * o_[2]
            assert type(dot) is T
            flip = dot < 0 if toward else dot > 0
            assert np.array_equal(got[i], -n_ if flip else n_), i
        changed = np.any(got != h["normals"], axis=1)
        assert 0 < np.count_nonzero(changed) < len(x)
    # the rank rule: behind Shadow, MaxDensity sees the survivors' densities as a cloud of its own
    nrm = ref.run(x, T, [(ref.OBS,) + ref.CENTER, (ref.ORIENT, 1)], keep=("normals",))["normals"]
    sh2 = np.flatnonzero(o.shadow_keep(x, nrm, eps_angle=ref.EPS))
    assert np.array_equal(sh2, sh)                                   # |cosine| does not see the flip
    after = sh[o.max_density_keep(h["densities"][sh], max_density=md, seed=ref.SEED)]
    six = ref.run(x, T, ref.six(md), keep=("normals", "eigen_values", "densities"))
    assert np.array_equal(six["kept_idx"], after)
    by_input_index = np.intersect1d(sh, mk)
    assert not np.array_equal(after, by_input_index)                 # what a draw on the input index would have kept
    assert six["normals"].tobytes() == nrm[after].tobytes() and six["densities"].tobytes() == h["densities"][after].tobytes()
    assert six["eigen_values"].tobytes() == h["eigen_values"][after].tobytes() and six["xyz"].tobytes() == x[after].tobytes()
    assert six["noise"].tobytes() == o.simple_sensor_noise(x, 0, 1.0)[after].tobytes()
    before = ref.run(x, T, ref.stage_lists(md)["md_before_shadow"])
    assert np.array_equal(before["kept_idx"], by_input_index)
    assert np.array_equal(ref.run(x, T, [])["kept_idx"], every)


@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_main_scene_exercises_both_dropping_stages(T):
    """the condition: the statement keeps between 10 % and 90 % of what arrives at Shadow and at MaxDensity"""
    x = ref.scene(ref.MAIN_N, T)
    r = ref.run(x, T, ref.six(ref.pick_max_density(x, T)))
    for stage in (ref.SHADOW, ref.MAXDENS):
        share = r["passed"][stage] / r["arrived"][stage]
        print(T.__name__, stage, r["arrived"][stage], "->", r["passed"][stage], f"{share:.3f}")
        assert 0.1 < share < 0.9, (stage, share)
    assert r["arrived"][ref.SHADOW] == len(x) and r["arrived"][ref.MAXDENS] == r["passed"][ref.SHADOW]


def host_filters(exe, T, xyz, nrm, center, toward, eps, sensor_type, gain):
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<iii", len(xyz), toward, sensor_type) + struct.pack("<ddddd", *center, eps, gain))
            fh.write(np.ascontiguousarray(xyz, dtype=T).tobytes() + np.ascontiguousarray(nrm, dtype=T).tobytes())
        out = subprocess.run([exe, "host", "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        blob = open(fout, "rb").read()
    kept = struct.unpack_from("<i", blob, 0)[0]
    w = np.dtype(T).itemsize
    assert len(blob) == 4 + 10 * kept * w
    return (np.frombuffer(blob, dtype=T, count=3 * kept, offset=4).reshape(kept, 3),
            np.frombuffer(blob, dtype=T, count=7 * kept, offset=4 + 3 * kept * w).reshape(kept, 7))


@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_host_functions_equal_the_reference(T):
    exe = build_exe("test_sensor_chain_cpu")
    rng = np.random.default_rng(17)
    x = ref.sized_cloud(4097, T).copy()
    nrm = rng.normal(size=x.shape)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm = nrm.astype(T)
    x[100] = 0                      # the origin: the position is not normalised
    nrm[200] = 0                    # a normal of zero: not normalised, the cosine is 0
    nrm[300] *= T(1e-30)            # a tiny normal (f32: its squared norm underflows to 0)
    x[400] = x[400] * T(1e20)       # a far point (f32: its squared norm overflows)
    for toward, eps, st, gain, center in ((1, 0.2, 0, 1.0, (0.0, 0.0, 0.0)), (0, 0.0, 3, 2.5, (0.5, -0.25, 1.0)), (1, 1.2, 4, 1.5, (4.0, 0.0, 0.0))):
        stages = [(ref.NOISE, st, gain), (ref.OBS,) + center, (ref.ORIENT, toward), (ref.SHADOW, eps)]
        want = ref.run(x, T, stages, keep=("normals",), head_rows=dict(normals=nrm))
        gx, gd = host_filters(exe, T, x, nrm, center, toward, eps, st, gain)
        label = (toward, eps, st)
        assert 0 < want["count"] < len(x) and 100 not in want["kept_idx"] and 200 not in want["kept_idx"], label
        assert gx.tobytes() == want["xyz"].tobytes(), label
        assert np.ascontiguousarray(gd[:, 0:3]).tobytes() == want["normals"].tobytes(), label
        assert np.ascontiguousarray(gd[:, 3]).tobytes() == want["noise"].tobytes(), label
        assert np.ascontiguousarray(gd[:, 4:7]).tobytes() == want["observation_directions"].tobytes(), label


def test_run_detection_and_guards():
    exe = build_exe("test_sensor_chain_cpu")
    env = dict(os.environ)
    env.pop("PGSLAM_HOST_SENSOR_CHAIN", None)
    out = subprocess.run([exe, "runs"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sensor chain cpu tests ok" in out.stdout


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_sensor_chain.h"\nint main(void) { pgicp_chain_stage s; s.type = PGICP_CHAIN_SHADOW; return s.type - 3; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.SENSOR_CHAIN_SYMBOLS)
    assert not set(icp.SENSOR_CHAIN_SYMBOLS) & set(icp.ABI_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
    assert callable(getattr(icp.Context, "sensor_chain", None))
    # the constants of the header and of the binding agree
    for name, value in re.findall(r"#define (PGICP_CHAIN_\w+)\s+(\d+)", open(HEADER).read()):
        assert getattr(icp, name[len("PGICP_"):]) == int(value), name
    assert icp.C.sizeof(icp.ChainStage) == 40
    arr = icp.Context.chain_stages([("shadow", 0.1), ("max_density", 50.0), ("observation_direction", 1, 2, 3)])
    assert (arr[0].type, arr[0].p[0]) == (icp.CHAIN_SHADOW, 0.1) and (arr[1].type, arr[1].p[0], arr[1].p[1]) == (icp.CHAIN_MAX_DENSITY, 50.0, 1.0)
    assert (arr[2].type, list(arr[2].p)) == (icp.CHAIN_OBSERVATION_DIRECTION, [1.0, 2.0, 3.0, 0.0])
    with pytest.raises(ValueError):
        icp.Context.chain_stages([("shadows", 0.1)])
