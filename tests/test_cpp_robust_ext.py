"""[EXT] RobustOutlierFilter's distanceType, berg and nbIterationForScale in the C++ drop-in: the constructor's settings and the refusals
(a YAML names upstream's defaults only) without a device (tests/cpp/test_robust_ext_cpu.cpp) and, on the GPU, ICP::operator() against the C calls and the filter's own
compute() (tests/cpp/test_robust_ext_gpu.cpp); g++ against include/ and libpgicp.so."""
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


def test_dropin_yaml_robust_ext():
    out = subprocess.run([build("test_robust_ext_cpu")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "robust ext cpu tests ok" in out.stdout


@pytest.mark.gpu
def test_dropin_robust_ext_on_device():
    out = subprocess.run([build("test_robust_ext_gpu")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "robust ext gpu tests ok" in out.stdout
