"""ElipsoidsDataPointsFilter through the C++ drop-in on the device (tests/cpp/test_elipsoids_gpu.cpp): the device form against the
host form (PGSLAM_HOST_ELIPSOIDS=1) bit for bit, from the constructor and from YAML, and one end-to-end run: an ICP whose reference
filter is this one (keepNormals: 1, samplingMethod 1) on synth.make_two_scans(10_000, rings=16), the pose within the bound of the
SamplingSurfaceNormal end-to-end test (0.02 m of the truth).  (The part that needs no device -- tests/cpp/test_elipsoids_cpu.cpp -- is
driven by tests/test_elipsoids_host.py.)

The end-to-end run's minPlanarity is what elipsoids_ref.pick_min_planarity gives for the reference scan (the midpoint of two adjacent
box planarities at their median, about 0.094), not 0.  Measured: with minPlanarity 0 the filter is SamplingSurfaceNormal's byte for
byte and this ICP ends 0.0254 m from the truth, on the device and equally in the oracle's CPU ICP over the numpy statement's output
-- the scan has 16 rings, and a quarter of its boxes of 7 points are arcs of a single ring or thin two-ring strips (planarity below
0.016), whose smallest eigenvector says little about the surface.  Dropping the less planar half is what the filter's own parameter
is for; with the picked threshold the oracle's CPU ICP ends 0.0067 m from the truth, and the full scan with its analytic normals
0.0036 m."""
import os
import struct
import subprocess

import numpy as np
import pytest

import elipsoids_ref as ref
from pgslam_amd import synth
from test_density_host import build_exe


@pytest.mark.gpu
def test_dropin_device_form_equals_host_form_and_icp_converges(tmp_path):
    exe = build_exe("test_elipsoids_gpu")
    s = synth.make_two_scans(10_000, rings=16)
    rd, rf = (np.ascontiguousarray(s[k], dtype=np.float32) for k in ("reading_xyz", "ref_xyz"))
    min_planarity = ref.pick_min_planarity(rf, np.float32, 7)
    scans = tmp_path / "scans.bin"
    with open(scans, "wb") as fh:
        fh.write(struct.pack("<ii", len(rd), len(rf)))
        fh.write(np.ascontiguousarray(s["T_init"], dtype=np.float64).tobytes() + np.ascontiguousarray(s["T_truth"], dtype=np.float64).tobytes())
        fh.write(rd.tobytes() + rf.tobytes())
    env = dict(os.environ)
    for knob in ("PGSLAM_HOST_INPUT_STAGE", "PGSLAM_HOST_ELIPSOIDS", "PGSLAM_HOST_SAMPLING_NORMALS"):
        env.pop(knob, None)
    out = subprocess.run([exe, str(scans), repr(float(min_planarity))], capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "elipsoids gpu tests ok" in out.stdout
