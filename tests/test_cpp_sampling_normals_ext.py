"""SamplingSurfaceNormalDataPointsFilter's further outputs through the C++ drop-in on the device (tests/cpp/
test_sampling_normals_ext_gpu.cpp): the descriptors the filter appends and their order against the direct call
(pgicp_sampling_surface_normal_ext_*), the host form (PGSLAM_HOST_SAMPLING_NORMALS=1) against the device form bit for bit, a
constructed SamplingSurfaceNormal{keepDensities} followed by MaxDensity against the two steps by hand, and ICP objects whose reference
chain is SamplingSurfaceNormal{keepEigenValues: 1} against the same chain without the key.  (The part that needs no device --
tests/cpp/test_sampling_normals_ext_cpu.cpp -- is driven by tests/test_sampling_normals_ext_host.py.)"""
import os
import subprocess

import pytest

from test_density_host import build_exe


@pytest.mark.gpu
def test_dropin_descriptors_host_form_max_density_chain_and_icp():
    exe = build_exe("test_sampling_normals_ext_gpu")
    env = dict(os.environ)
    for knob in ("PGSLAM_HOST_INPUT_STAGE", "PGSLAM_HOST_MAX_DENSITY", "PGSLAM_HOST_SAMPLING_NORMALS"):
        env.pop(knob, None)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sampling normals ext gpu tests ok" in out.stdout
