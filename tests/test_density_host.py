"""[EXT] MaxDensityDataPointsFilter and include/pgicp_density.h without a device: the C++ drop-in's host loop -- forced by
PGSLAM_HOST_MAX_DENSITY=1, and taken anyway when no device is present -- against the oracle's keep mask
(orc_max_density_keep; tests/cpp/test_density_cpu.cpp apply), the refusal without a `densities` descriptor
(tests/cpp/test_density_cpu.cpp refuse), the header as strict C99, and the library's exports against the header's declarations."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from pgslam_amd import icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_density_cpu")
HEADER = os.path.join(ROOT, "include", "pgicp_density.h")


_built = {}


def build_exe(name="test_density_cpu"):
    exe = os.path.join(CPP, name)
    if name in _built:
        return exe
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-local-typedefs", "-Wno-unused-variable", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp",
                           "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    _built[name] = True
    return exe


def apply_dropin(exe, dens, T, max_density, seed, knob):
    """the drop-in filter on a cloud carrying `dens`: dict(kept (k,) indices, on_device, refused)"""
    dens = np.ascontiguousarray(dens, dtype=T)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<idd", len(dens), float(max_density), float(seed)))
            fh.write(dens.tobytes())
        env = dict(os.environ)
        if knob:
            env["PGSLAM_HOST_MAX_DENSITY"] = "1"
        else:
            env.pop("PGSLAM_HOST_MAX_DENSITY", None)
        out = subprocess.run([exe, "apply", "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stdout + out.stderr
        b = open(fout, "rb").read()
    m, dev, refused = struct.unpack_from("<iii", b, 0)
    return dict(kept=np.frombuffer(b, dtype=np.int32, count=m, offset=12), on_device=dev, refused=refused)


def density_arrays(T):
    """(name, densities, maxDensity): the edge cases of the keep rule, as arrays of T"""
    rng = np.random.default_rng(5)
    yield "lognormal", np.exp(rng.normal(4.0, 1.5, 3001)).astype(T), 60.0
    yield "first_nan", np.array([np.nan, 5.0, 500.0, 50.0, 5000.0, 500.0] * 40, dtype=T), 100.0
    a = np.exp(rng.normal(5.0, 1.0, 700)).astype(T)
    a[[3, 350, 699]] = np.nan
    yield "nan_elsewhere", a, 120.0
    a = np.exp(rng.normal(5.0, 1.0, 900)).astype(T)
    a[[0, 17, 450, 899]] = np.inf
    yield "several_inf", a, 100.0
    yield "all_saturated", np.full(300, 250.0, dtype=T), 100.0
    yield "all_below", rng.uniform(1.0, 99.0, 500).astype(T), 100.0
    yield "one_above", np.array([1e6], dtype=T), 100.0
    yield "one_below", np.array([1.0], dtype=T), 100.0
    yield "negatives_and_zeros", np.array([-3.0, -0.0, 0.0, -np.inf, -1e-30] * 20, dtype=T), 1e-3
    yield "max_is_first", np.concatenate([[9e5], np.exp(rng.normal(5.0, 1.0, 400))]).astype(T), 100.0


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_host_loop_matches_the_oracle(oracle32, oracle64, T):
    exe = build_exe()
    o = oracle32 if T == np.float32 else oracle64
    for name, dens, md in density_arrays(T):
        for seed in (1, 77):
            want = np.flatnonzero(o.max_density_keep(dens, max_density=md, seed=seed)).astype(np.int32)
            for knob in (True, False):
                if not knob and icp.load_library().pgicp_device_count() > 0:
                    # The no-device path exists only where there is no device: on a machine with one, the unforced path is the
                    # device's (tests/test_gpu_density.py, tests/test_cpp_density.py), so this case runs on the CPU runner alone.
                    continue
                g = apply_dropin(exe, dens, T, md, seed, knob)
                assert not g["refused"] and g["on_device"] == 0, name
                np.testing.assert_array_equal(g["kept"], want, err_msg=f"{name} seed {seed} knob {knob}")
        if name == "all_saturated":
            assert len(want) == 0
        if name in ("all_below", "one_below", "negatives_and_zeros"):
            assert len(want) == len(dens)


def test_refusal_without_densities():
    exe = build_exe()
    out = subprocess.run([exe, "refuse"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "density cpu tests ok" in out.stdout


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_density.h"\nint main(void) { return PGICP_ABI_VERSION == 0; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.DENSITY_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
