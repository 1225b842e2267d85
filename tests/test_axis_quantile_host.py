"""MaxQuantileOnAxisDataPointsFilter and DistanceLimitDataPointsFilter without a device.  The host statement
(include/pgslam_amd/axis_quantile_host.hpp) alone (tests/cpp/axis_quantile_host_main.cpp, the program a sanitizer build runs) and
through the C++ drop-in's inPlaceFilter (tests/cpp/test_axis_quantile_cpu.cpp apply) against the numpy reference
(tests/axis_quantile_ref.py) on every scene, bit for bit; what the scenes are for; YAML loading, defaults and refusals of both
filters, DistanceLimit against Min / MaxDist at the limit, the ICP chain (tests/cpp/test_axis_quantile_cpu.cpp yaml); the header as
strict C99 and the library's exports against its declarations."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import axis_quantile_ref as ref
from pgslam_amd import icp
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
HEADER = os.path.join(ROOT, "include", "pgicp_quantile.h")


def check_results(got, T, what):
    want = ref.scenes(T)
    assert len(got) == len(want), what
    for (limit, k, below, kept), (sid, _, _, _, (wl, wk, wb), mask) in zip(got, want):
        assert ref.canonical(limit) == ref.canonical(wl), (what, sid, limit, wl)
        assert (k, below) == (wk, wb), (what, sid, k, below, wk, wb)
        assert np.array_equal(kept, np.flatnonzero(mask)), (what, sid)


def test_the_scenes_reach_what_they_are_for():
    for T in (np.float32, np.float64):
        by_id = {s[0]: s for s in ref.scenes(T)}
        assert ref.rank(90, 0.7, T) == (63 if T == np.float32 else 62)       # the product is rounded in T: the precisions differ
        for sid, dim, f, ratio, (limit, k, below), mask in by_id.values():
            n = len(f)
            assert below == mask.sum() <= k <= n - 1
            assert k == ref.rank(n, ratio, T)
            if ratio == 1e-7:
                assert k == 0 and below == 0                                 # k = 0: the cloud comes back empty
            if sid.startswith("all_nan") or sid.startswith("equal"):
                assert below == 0 and np.isnan(limit) == sid.startswith("all_nan")
            if sid.startswith("half_ties") and n >= 90 and k > 0:
                assert limit == 1.0 and below < k and (f[:, dim] == limit).sum() >= n // 2     # ties at the limit are all dropped
            if sid.startswith("planar") or sid.startswith("low8"):
                bits = f[:, dim].view(np.uint32 if T == np.float32 else np.uint64)
                shift = bits.dtype.type(bits.itemsize * 8 - 12 if sid.startswith("planar") else 8)
                assert len(np.unique(bits >> shift)) == 1                    # one first-level bin / only the lowest 8 bits differ
            if sid.startswith("mixed") and n >= 90:
                v = f[:, dim]
                assert np.isnan(v).sum() == 2 and np.isinf(v).sum() == 2 and (v == 0).sum() >= 3 and np.signbit(v[v == 0]).any()
                assert np.isnan(f[:, (dim + 1) % 3]).any()                   # a NaN on another axis only
        s = by_id["mixed-n90@0.7"]
        assert s[4][1] == (63 if T == np.float32 else 62)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_host_statement_equals_the_reference(T):
    exe = os.path.join(CPP, "axis_quantile_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe])
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        ref.write_groups(fin, T)
        out = subprocess.run([exe, "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "host statement ok" in out.stdout, out.stdout + out.stderr
        check_results(ref.read_results(fout, T), T, "host statement")


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_dropin_host_form_equals_the_reference(T):
    exe = build_exe("test_axis_quantile_cpu")
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        ref.write_groups(fin, T)
        out = subprocess.run([exe, "apply", "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        check_results(ref.read_results(fout, T), T, "drop-in host form")


def test_yaml_loading_refusals_distance_limit_chain_and_exports():
    exe = build_exe("test_axis_quantile_cpu")
    out = subprocess.run([exe, "yaml"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "axis quantile cpu tests ok" in out.stdout


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_quantile.h"\nint main(void) { return PGICP_FILTER_MAX_QUANTILE_ON_AXIS != 8; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.QUANTILE_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
    assert icp.FILTER_MAX_QUANTILE_ON_AXIS == 8
