"""MaxQuantileOnAxisDataPointsFilter through the C++ drop-in on the device (tests/cpp/test_axis_quantile_gpu.cpp): filter lists that
hold it, run as one device pass (filterAndTransformOnDevice, filterOnDeviceDeferred), against DataPointsFilters::apply on the
host, bit for bit in both precisions; and a YAML reading chain with the filter through ICP::operator()."""
import os
import subprocess

import pytest

from test_density_host import build_exe


@pytest.mark.gpu
def test_dropin_device_list_host_filters_and_icp_chain():
    exe = build_exe("test_axis_quantile_gpu")
    env = dict(os.environ)
    env.pop("PGSLAM_HOST_INPUT_STAGE", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "axis quantile gpu tests ok" in out.stdout
