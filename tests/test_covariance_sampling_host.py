"""[EXT] CovarianceSamplingDataPointsFilter and include/pgicp_covsample.h without a device: the numpy reference's two
transliterations against each other and against three hand-checked clouds, the frame tolerances of the device test checked on the
reference's own eigh basis, the C++ drop-in's host form (tests/cpp/test_covariance_sampling_cpu.cpp) against the reference, the
header as strict C99, and the library's exports against the header's declarations."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import covariance_sampling_ref as ref
from pgslam_amd import icp
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgicp_covsample.h")

SIZES = (2, 65, 2047, 2048, 2049, 4097, 8193)
KINDS = ("room", "plane", "twice", "offset")


def nb_samples(n):
    return sorted({max(1, min(n - 1, nb)) for nb in (1, 6, n // 2, n - 1)})


def case_frame(x, nr, T):
    """the reference frame of a framed case: Lavg, or L = 1 where the cloud has no extent (two coincident points)"""
    try:
        return ref.frame(x, nr, 1, T)
    except ValueError:
        return ref.frame(x, nr, 0, T)


IDENTITY_FRAME = dict(center=np.zeros(3), L=1.0, eigenvalues=np.zeros(6), basis=np.eye(6))
# (p; n) -> f = (p x n, n); with the identity frame v = |f|
AXES = np.array([[1, 0, 0, 0, 1, 0], [0, 2, 0, 0, 0, 1], [0, 0, 3, 1, 0, 0], [-1, 0, 0, 0, 0, 1], [0, -1, 0, 1, 0, 0], [0, 0, -1, 0, 1, 0]], dtype=np.float64)
PLANE = np.array([[1, 0, 0, 0, 0, 1], [0, 2, 0, 0, 0, 1], [3, 1, 0, 0, 0, 1], [-2, -2, 0, 0, 0, 1], [0.5, 0.5, 0, 0, 0, 1]], dtype=np.float64)
HAND = [
    # f: 0 (0,0,1,0,1,0)  1 (2,0,0,0,0,1)  2 (0,3,0,1,0,0)  3 (0,1,0,0,0,1)  4 (0,0,1,1,0,0)  5 (1,0,0,0,1,0)
    # lists: L0 1,5,..  L1 2,3,..  L2 0,4,..  L3 2,4,..  L4 0,5,..  L5 1,3,..
    # t: pick 1 (list 0) -> (4,0,0,0,0,1); 2 (list 1) -> (4,9,0,1,0,1); 0 (list 2) -> (4,9,1,1,1,1); list 2 again: 0 popped, 4 ->
    # (4,9,2,2,1,1); list 4: 0 popped, 5
    ("axes", AXES, 5, [1, 2, 0, 4, 5]),
    # v = (|y|, |x|, 0, 0, 0, 1): L0 1,3,2,4,0  L1 2,3,0,4,1  L2-L5 0,1,2,3,4 (all ties)
    # pick 1 (list 0) -> (4,0,0,0,0,1); 2 (list 1) -> (5,9,0,0,0,2); 0 (list 2) -> (5,10,0,0,0,3); list 2: 0,1,2 popped, 3
    ("plane", PLANE, 4, [1, 2, 0, 3]),
    # the axes cloud twice (i + 6 duplicates i): L0 1,7,5,11,..  L1 2,8,3,9,..  L2 0,4,6,10,..  L4 0,5,6,11,..  L5 1,3,7,9,..
    # as above up to 5; then t = (5,9,2,2,2,1): list 5: 1 popped, 3 -> (5,10,2,2,2,2); list 2: 0, 4 popped, 6
    ("duplicated", np.concatenate([AXES, AXES]), 7, [1, 2, 0, 4, 5, 3, 6]),
]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_hand_checked_clouds(T):
    for name, pn, nb, want in HAND:
        for k in range(1, nb + 1):              # every prefix: the greedy does not look ahead
            for vec in (False, True):
                got = ref.select(pn[:, :3], pn[:, 3:], k, IDENTITY_FRAME, T, vectorised=vec)
                assert got.tolist() == want[:k], (name, k, vec)


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_the_two_transliterations_agree(kind, T):
    for n in SIZES:
        x, nr = ref.cloud(kind, n, T)
        fr = case_frame(x, nr, T)
        for nb in nb_samples(n):
            a = ref.select(x, nr, nb, fr, T, vectorised=False)
            b = ref.select(x, nr, nb, fr, T, vectorised=True)
            np.testing.assert_array_equal(a, b, err_msg=f"{kind} n {n} nb {nb}")
            assert len(np.unique(a)) == nb


def test_the_two_transliterations_agree_at_sensor_size():
    x, nr = ref.cloud("room", 100_000, np.float32)
    fr = ref.frame(x, nr, 1, np.float32)
    np.testing.assert_array_equal(ref.select(x, nr, 5000, fr, np.float32, vectorised=False), ref.select(x, nr, 5000, fr, np.float32, vectorised=True))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_eigh_basis_rounded_to_T_is_inside_the_frame_tolerances(T):
    """the bounds tests/test_gpu_covariance_sampling.py holds the device's frame to, met by the reference's own basis"""
    for kind in KINDS + ("corridor",):
        for n in (65, 2049, 8193):
            x, nr = ref.cloud(kind, n, T)
            for tn in (0, 1, 2):
                fr = ref.frame(x, nr, tn, T)
                for value, bound in ref.frame_bounds_ok(fr, fr, x, T):
                    assert value <= bound, (kind, n, tn, value, bound)


def run_cpp(args, host=True):
    env = dict(os.environ)
    if host:
        env["PGSLAM_HOST_INPUT_STAGE"] = "1"
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def pack_frame(fr):
    return struct.pack("<46d", *fr["center"], fr["L"], *fr["eigenvalues"], *np.asarray(fr["basis"]).T.ravel())


def unpack_frame(b):
    v = struct.unpack("<46d", b)
    return dict(center=np.array(v[0:3]), L=v[3], eigenvalues=np.array(v[4:10]), basis=np.array(v[10:46]).reshape(6, 6).T.copy())


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_host_form_against_the_reference(T):
    exe = build_exe("test_covariance_sampling_cpu")
    sfx = "f32" if T == np.float32 else "f64"
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        for kind, n, nb, tn in (("room", 2049, 300, 1), ("plane", 700, 100, 2), ("twice", 1001, 500, 0), ("offset", 4097, 64, 1), ("corridor", 3000, 200, 1)):
            x, nr = ref.cloud(kind, n, T)
            head = struct.pack("<iii", n, nb, tn) + x.tobytes() + nr.tobytes()
            # the picks of the reference, with the reference's frame, handed in
            fr = ref.frame(x, nr, tn, T)
            want = ref.select(x, nr, nb, fr, T)
            with open(fin, "wb") as fh:
                fh.write(head + pack_frame(fr) + want.astype(np.int32).tobytes())
            run_cpp([exe, "framed", sfx, fin])
            # the whole filter: its own frame inside the tolerances, its picks the reference's given that frame
            with open(fin, "wb") as fh:
                fh.write(head)
            run_cpp([exe, "apply", sfx, fin, fout])
            b = open(fout, "rb").read()
            m, = struct.unpack_from("<i", b, 0)
            got_fr = unpack_frame(b[4:4 + 368])
            got = np.frombuffer(b, dtype=np.int32, count=m, offset=4 + 368)
            assert m == nb
            for value, bound in ref.frame_bounds_ok(got_fr, fr, x, T):
                assert value <= bound, (kind, value, bound)
            np.testing.assert_array_equal(got, ref.select(x, nr, nb, got_fr, T), err_msg=kind)


def test_yaml_refusals_and_noop():
    exe = build_exe("test_covariance_sampling_cpu")
    assert "covariance sampling cpu tests ok" in run_cpp([exe, "yaml"])


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_covsample.h"\nint main(void) { return sizeof(pgicp_cov_frame) != 46 * sizeof(double); }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.COVSAMPLE_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
