"""The sensor filter chain through the C++ drop-in on the device (tests/cpp/test_sensor_chain_gpu.cpp): DataPointsFilters::apply with a
run as one pgicp_sensor_chain_* call against the same list under PGSLAM_HOST_SENSOR_CHAIN=1 -- labels, order and bytes, for
PointMatcher<float> and PointMatcher<double> --, lastFusedRun(), the lists that must not take the call, and one ICP whose
referenceDataPointsFilters is the six-filter chain: the same pose as under the knob, bit for bit.  (The part that needs no device --
tests/cpp/test_sensor_chain_cpu.cpp -- is driven by tests/test_sensor_chain_host.py.)"""
import os
import struct
import subprocess

import numpy as np
import pytest

import sensor_chain_ref as ref
from pgslam_amd import synth
from test_density_host import build_exe


@pytest.mark.gpu
def test_fused_apply_equals_filter_by_filter_and_icp_agrees(tmp_path):
    exe = build_exe("test_sensor_chain_gpu")
    s = synth.make_two_scans(10_000, rings=16)
    rd, rf = (np.ascontiguousarray(s[k], dtype=np.float32) for k in ("reading_xyz", "ref_xyz"))
    max_density = ref.pick_max_density(rf, np.float32)
    scans = tmp_path / "scans.bin"
    with open(scans, "wb") as fh:
        fh.write(struct.pack("<ii", len(rd), len(rf)))
        fh.write(np.ascontiguousarray(s["T_init"], dtype=np.float64).tobytes() + np.ascontiguousarray(s["T_truth"], dtype=np.float64).tobytes())
        fh.write(rd.tobytes() + rf.tobytes())
    env = dict(os.environ)
    for knob in ("PGSLAM_HOST_SENSOR_CHAIN", "PGSLAM_HOST_MAX_DENSITY", "PGSLAM_HOST_INPUT_STAGE"):
        env.pop(knob, None)
    out = subprocess.run([exe, str(scans), repr(float(max_density))], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sensor chain gpu tests ok" in out.stdout
