"""OctreeGridDataPointsFilter through the C++ drop-in on the device (tests/cpp/test_octree_grid_gpu.cpp): the device form against
the host form bit for bit, as float and as double, for methods 0, 2 and 3, and a YAML reading chain OctreeGrid -> SurfaceNormal
through ICP::operator() against the same chain under PGSLAM_HOST_INPUT_STAGE=1, bit for bit."""
import os
import subprocess

import pytest

from test_density_host import build_exe


@pytest.mark.gpu
def test_dropin_device_form_host_form_and_icp_chain():
    exe = build_exe("test_octree_grid_gpu")
    env = dict(os.environ)
    env.pop("PGSLAM_HOST_INPUT_STAGE", None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "octree grid gpu tests ok" in out.stdout
