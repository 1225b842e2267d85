"""Builds and runs the C++ test of getOverlap()'s sensor-noise branch through the drop-in layer (g++ against include/ and
libpgicp.so)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def build(name):
    exe = os.path.join(CPP, name)
    # always rebuilt: a stale binary must never be what runs
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-local-typedefs", "-Wno-unused-variable", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp",
                           "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_noise_overlap_gpu():
    out = subprocess.run([build("test_noise_overlap_gpu")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "noise overlap gpu tests ok" in out.stdout
