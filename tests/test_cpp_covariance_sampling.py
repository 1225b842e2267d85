"""CovarianceSamplingDataPointsFilter through the C++ drop-in on the device (tests/cpp/test_covariance_sampling_gpu.cpp): the
device form against the host form given the device's frame, as float and as double, and a YAML chain SurfaceNormal ->
CovarianceSampling on a reading through ICP::operator()."""
import os
import subprocess

import pytest

from test_density_host import build_exe


@pytest.mark.gpu
def test_dropin_device_form_host_form_and_icp_chain():
    exe = build_exe("test_covariance_sampling_gpu")
    env = dict(os.environ)
    env.pop("PGSLAM_HOST_INPUT_STAGE", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "covariance sampling gpu tests ok" in out.stdout
