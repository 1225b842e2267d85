"""pgslam_amd/csrc/seed_source.hpp without a device: whether pgicp_partial_chain_seeded may read the source context's state
(tests/cpp/seed_source_host.cpp, a stand-alone program; once more under the address and undefined-behaviour sanitizers).

The program takes one record that is seeded and changes one field at a time: the reading's size on either side, the cloud type,
the device, the caller as its own source, a map entry that is not in use, a stamp older than / equal to / newer than the map's,
the source's knn, 0 / 1 / 16 / 17 segments, and the caller's chain (a batch, knn, the brute matcher, the two filters that are
searched unseeded).  Every row carries the answer it must get."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "seed_source_host.cpp")
N_ROWS = 36


def build_exe(out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I" + os.path.join(ROOT, "pgslam_amd", "csrc"), SRC, "-o", out])
    return out


def test_every_row(tmp_path):
    exe = build_exe(str(tmp_path / "seed_source_host"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"seed source ok: {N_ROWS} rows" in out.stdout


def test_every_row_under_sanitizers(tmp_path):
    san = build_exe(str(tmp_path / "seed_source_host_san"), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([san], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"seed source ok: {N_ROWS} rows" in out.stdout
