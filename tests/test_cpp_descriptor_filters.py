"""IncidenceAngle, Sphericality and CutAtDescriptorThreshold through the C++ drop-in on the device
(tests/cpp/test_descriptor_filters_gpu.cpp): DataPointsFilters::apply with a run that holds them as one pgicp_sensor_chain_ext_* call
against the same list under PGSLAM_HOST_SENSOR_CHAIN=1 -- labels, order and bytes, for PointMatcher<float> and PointMatcher<double> --,
lastFusedRun(), the lists that must not take the call, filterAndTransformOnDevice with a cut entry against host apply followed by the
transformation, and one ICP whose referenceDataPointsFilters is the list: the same pose as under the knob, bit for bit.  (The part
that needs no device -- tests/cpp/test_descriptor_filters_cpu.cpp -- is driven by tests/test_descriptor_filters_host.py.)"""
import os
import struct
import subprocess

import numpy as np
import pytest

import descriptor_filters_ref as ref
from pgslam_amd import synth
from test_density_host import build_exe


@pytest.mark.gpu
def test_fused_apply_equals_filter_by_filter_and_icp_agrees(tmp_path):
    exe = build_exe("test_descriptor_filters_gpu")
    s = synth.make_two_scans(10_000, rings=16)
    rd, rf = (np.ascontiguousarray(s[k], dtype=np.float32) for k in ("reading_xyz", "ref_xyz"))
    # each threshold the median of what reaches its stage on the reference scan: every cut keeps about half
    st = ref.yaml_list(rf, np.float32)
    thr_inc, thr_sph, max_density = st[3][3], st[5][3], st[6][1]
    thr_uns = ref.median_of(rf, np.float32, [(ref.SPH, 1, 1)], "unstructureness")
    thr_str = ref.median_of(rf, np.float32, [(ref.SPH, 1, 1), (ref.CUT, "unstructureness", 0, thr_uns)], "structureness")
    scans = tmp_path / "scans.bin"
    with open(scans, "wb") as fh:
        fh.write(struct.pack("<ii", len(rd), len(rf)))
        fh.write(np.ascontiguousarray(s["T_init"], dtype=np.float64).tobytes() + np.ascontiguousarray(s["T_truth"], dtype=np.float64).tobytes())
        fh.write(rd.tobytes() + rf.tobytes())
    env = dict(os.environ)
    for knob in ("PGSLAM_HOST_SENSOR_CHAIN", "PGSLAM_HOST_MAX_DENSITY", "PGSLAM_HOST_INPUT_STAGE"):
        env.pop(knob, None)
    out = subprocess.run([exe, str(scans)] + [repr(float(v)) for v in (thr_inc, thr_sph, max_density, thr_uns, thr_str)], capture_output=True, text=True,
                         timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "descriptor filters gpu tests ok" in out.stdout
