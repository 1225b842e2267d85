"""CPU-side checks of the sensor-noise getOverlap() surface (include/pgicp_noise.h): header, binding and library agree on the
companion header's symbols; the C++ layer no longer reads the diagnostics entry points; the reference statement
(tests/noise_overlap_ref.py) reproduces the oracle on small inputs.  No GPU call is made."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pgslam_amd import icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import Oracle  # noqa: E402
import noise_overlap_ref as ref  # noqa: E402


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pgicp_[a-z0-9_]+)\s*\(", src)))


def test_noise_header_and_binding_agree():
    assert _declared("pgicp_noise.h") == sorted(icp.NOISE_SYMBOLS)
    assert not set(icp.NOISE_SYMBOLS) & set(icp.ABI_SYMBOLS)
    # pgicp.h keeps its own set: the companion header includes it, not the other way round
    assert "pgicp_noise.h" not in open(os.path.join(ROOT, "include", "pgicp.h")).read()
    assert '#include "pgicp.h"' in open(os.path.join(ROOT, "include", "pgicp_noise.h")).read()


def test_library_exports_the_noise_symbols():
    lib = icp.load_library()
    for name in icp.NOISE_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6


def test_noise_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "pgicp_noise.h"\nint main(void) { return PGICP_SENSOR_SICK_TIM == 4 ? 0 : 1; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", exe + ".o"])


def test_cpp_layer_names_no_diagnostics_entry_point():
    inc = os.path.join(ROOT, "include", "pgslam_amd")
    hits = []
    for name in sorted(os.listdir(inc)):
        text = open(os.path.join(inc, name)).read()
        if "pgicp_debug_" in text:
            hits.append(name)
    assert hits == []


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("knn", [1, 3])
def test_reference_reproduces_the_oracle_on_small_inputs(dtype, knn):
    o = Oracle(dtype)
    rng = np.random.default_rng(20 + knn)
    for n in (1, 2, 17, 400):
        d2 = (rng.random((n, knn)) * 0.04).astype(dtype)
        w = np.ones((n, knn), dtype=dtype)
        noise = (0.012 + 0.01 * rng.random(n)).astype(dtype)
        want = o.sensor_noise_overlap(d2 if knn > 1 else d2[:, 0], w if knn > 1 else w[:, 0], noise)
        lo, hi, nb, _ = ref.count_bounds(d2, w, noise, dtype, rel=1e-3)          # a huge band: every summation order in T
        assert nb == n * knn
        got = round(want * nb)
        assert abs(got / nb - want) < 1e-6
        assert lo <= got <= hi
        # the derived band: the oracle's sequential sum in T may move the count by at most the pairs near the mean
        lo0, hi0, _, _ = ref.count_bounds(d2, w, noise, dtype)
        near = ref.near_mean_pairs(d2, w, noise, dtype)
        assert lo0 - near <= got <= hi0 + near


def test_reference_respects_weights_and_counts_in_T():
    dtype = np.float32
    d2 = np.array([0.01, 0.04, 0.09, 1.0], dtype=dtype)
    w = np.array([1, 1, 0, 1], dtype=dtype)
    noise = np.array([0.0, 0.0, 5.0, 0.0], dtype=dtype)
    lo, hi, nb, m = ref.count_bounds(d2, w, noise, dtype)
    # kept distances 0.1, 0.2, 1.0 -> mean 0.4333: two lie below it; the dropped pair's large noise does not count
    assert (lo, hi, nb) == (2, 2, 3) and abs(m - (0.1 + 0.2 + 1.0) / 3) < 1e-6
    assert Oracle(dtype).sensor_noise_overlap(d2, w, noise) == pytest.approx(2 / 3, abs=1e-6)
