"""[EXT] GenericDescriptorOutlierFilter without a device: the numpy statement of tests/generic_descriptor_ref.py on inputs
checked by hand, and the C++ drop-in (tests/cpp/test_generic_descriptor_cpu.cpp) -- YAML acceptance, each refusal, and its
stage-level compute() equal to the statement bit for bit on hand-made Matches with -1 ids."""
import os
import subprocess

import numpy as np
import pytest

from generic_descriptor_ref import gd_weights, kept_and_overlap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

# the C++ test's inputs: six reference values, Matches knn = 2 x N = 5 ([point][neighbour] order)
VALUES = [0.0, 0.25, 0.5, 0.75, 1.0 / 3.0, 2.0]
IDS = np.array([0, 5, -1, 3, 2, 2, 4, -1, 1, 3], dtype=np.int32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_by_hand(dtype):
    T = np.dtype(dtype).type
    v = np.array(VALUES, dtype=dtype)
    assert gd_weights(IDS, v, "larger", 0.5, dtype).tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 0, 1]       # strict: 0.5 is not > 0.5
    assert gd_weights(IDS, v, "smaller", 0.5, dtype).tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 1, 0]      # -1: weight 0 (deviation a)
    soft = gd_weights(IDS, v, "soft", None, dtype)
    mx = T(2.0)                                                                          # over the pairs with a neighbour
    assert soft.dtype == dtype
    assert soft.tolist() == [T(0), T(1), T(0), v[3] / mx, v[2] / mx, v[2] / mx, v[4] / mx, T(0), v[1] / mx, v[3] / mx]
    # the maximum leaves out a value only an invalid id would reach: ids 0..4 only -> max 0.75
    ids = np.array([0, 1, 2, 3, 4, -1])
    assert gd_weights(ids, v, "soft", None, dtype)[3] == T(1)
    # deviation b: a soft maximum of 0 weighs everything 0; negative values and non-finite ones are refused
    assert not gd_weights(IDS, np.zeros(6, dtype), "soft", None, dtype).any()
    with pytest.raises(ValueError):
        gd_weights(IDS, np.array([0, 1, -1, 0, 0, 0], dtype), "soft", None, dtype)
    with pytest.raises(ValueError):
        gd_weights(IDS, np.array([0, 1, np.nan, 0, 0, 0], dtype), "larger", 0.5, dtype)
    # hard modes take negative values
    assert gd_weights(np.array([0, 1]), np.array([-2.0, -0.5], dtype), "smaller", -1.0, dtype).tolist() == [1, 0]


def test_kept_and_overlap_by_hand():
    ids = np.array([0, 1, -1, 2])
    d2 = np.array([0.1, 0.3, np.inf, 0.2], dtype=np.float32)
    w = np.array([1.0, 1.0, 0.0, 0.5], dtype=np.float32)
    assert kept_and_overlap(ids, d2, 0.2, w) == (2, 1.5 / 4)
    assert kept_and_overlap(ids, d2, 1.0, w) == (3, 2.5 / 4)


def test_dropin_yaml_and_stage_compute():
    exe = os.path.join(CPP, "test_generic_descriptor_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-local-typedefs", "-Wno-unused-variable", "-pthread",
                           "-I" + os.path.join(ROOT, "include"), exe + ".cpp", "-o", exe,
                           "-L" + os.path.join(ROOT, "pgslam_amd", "lib"), "-lpgicp",
                           "-Wl,-rpath," + os.path.join(ROOT, "pgslam_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "generic descriptor cpu tests ok" in out.stdout
    seen = 0
    for line in out.stdout.splitlines():
        if not line.startswith("W "):
            continue
        _, mode, tname, *bits = line.split()
        dtype = np.dtype(tname)
        got = np.array([int(b, 16) for b in bits], dtype=np.uint32 if dtype == np.float32 else np.uint64).view(dtype)
        want = gd_weights(IDS, np.array(VALUES, dtype=dtype), mode, 0.5 if mode != "soft" else None, dtype)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (mode, tname, got, want)
        seen += 1
    assert seen == 6
