"""[EXT] VarTrimmedDistOutlierFilter in the C++ drop-in: the YAML acceptance and refusals without a device
(tests/cpp/test_var_trim_cpu.cpp), the numpy statement of tests/var_trim_ref.py on hand-checked inputs, and (GPU) the drop-in's
ICP object and a PoseGraphSlamMT drive with the filter in the chain (tests/cpp/test_var_trim_gpu.cpp)."""
import math
import os
import subprocess

import numpy as np
import pytest

from var_trim_ref import dists_quantile, var_trim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_dropin_yaml_var_trim():
    exe = os.path.join(CPP, "test_var_trim_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-local-typedefs", "-Wno-unused-variable", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp",
                           "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "var trim cpu tests ok" in out.stdout


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_by_hand(dtype):
    # P = 10 entries: two +inf, one zero; L = 0.1 .. 0.7 (c = 7); minRatio 0.2 -> minEl 2, maxRatio 0.9 -> maxEl 9 -> window [2, 7)
    d = np.array([0.4, np.inf, 0.1, 0.0, 0.7, 0.2, 0.3, np.inf, 0.5, 0.6], dtype=dtype)
    r = var_trim(d, 0.2, 0.9, 1.0, dtype)
    L = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], dtype=dtype).astype(np.float64)
    frms = {j: (10.0 / (j + 1)) ** 2 * L[:j + 1].sum() / (j + 1) for j in range(2, 7)}
    j = min(frms, key=lambda k: (frms[k], k))
    assert (r["c"], r["min_el"], r["max_el"], r["j"]) == (7, 2, 9, j)
    assert r["tuned"] == float(np.float32(j) / np.float32(10))
    lim, nf = dists_quantile(d, r["tuned"], dtype)
    assert nf == 8 and r["limit"] == lim and r["weights"].sum() == (d <= lim).sum()


def test_reference_edges():
    assert var_trim(np.array([0.0, np.inf]), 0.3, 0.9, 1.0, np.float64)["tuned"] is None          # c == 0: no outlier to filter
    r = var_trim(np.array([0.5] + [np.inf] * 9), 0.3, 0.9, 1.0, np.float64)                         # c = 1 <= minEl = 3: empty window
    assert r["j"] == 3 and r["tuned"] == float(np.float32(3) / np.float32(10)) and r["gap"] == math.inf


@pytest.mark.gpu
def test_dropin_and_slam_var_trim_on_device():
    """tests/cpp/test_var_trim_gpu.cpp: an ICP object and a PoseGraphSlamMT drive with a VarTrimmed chain (loop closures
    through the device batch)."""
    exe = os.path.join(CPP, "test_var_trim_gpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-local-typedefs", "-Wno-unused-variable", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp",
                           "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "var trim gpu tests ok" in out.stdout
