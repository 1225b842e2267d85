"""SurfaceNormalDataPointsFilter{keepDensities} -> MaxDensityDataPointsFilter through the C++ drop-in on the device
(tests/cpp/test_density_gpu.cpp): fused, unfused, with PGSLAM_HOST_MAX_DENSITY=1 and restated on the host -- the same features and
descriptors bit for bit, as float and as double -- and an ICP against the filtered reference."""
import os
import subprocess

import pytest

from test_density_host import build_exe


@pytest.mark.gpu
def test_dropin_fused_unfused_knob_and_restated_agree():
    exe = build_exe("test_density_gpu")
    env = dict(os.environ)
    env.pop("PGSLAM_HOST_MAX_DENSITY", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "density gpu tests ok" in out.stdout
