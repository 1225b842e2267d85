"""include/pgicp_ssn_ext.h without a device: the numpy reference (tests/sampling_normals_ext_ref.py) pinned by the oracle's
orc_sampling_surface_normal byte for byte on every case of the suite, its densities pinned by the oracle's orc_densities over the
boxes' member lists, the identities the GPU tests rest on, known answers on an exact lattice, and the drop-in without a device
(tests/cpp/test_sampling_normals_ext_cpu.cpp): the filter's host form against the reference bit for bit, the YAML forms, the
constructors, the header as strict C99 and the library's exports."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import sampling_normals_ext_ref as ref
from pgslam_amd import icp
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgicp_ssn_ext.h")
CASES = ref.cases()


def test_the_suite_covers_what_it_says():
    names = {c[0] for c in CASES}
    for knn in ref.KNNS:
        for n in ref.small_n(knn):
            assert f"n{n}" in names
    assert set(ref.SCENES) <= names
    assert {(c[3], c[4]) for c in CASES if c[0] == "cloud3000"} == set(ref.SAMPLINGS)
    assert {c[2] for c in CASES if c[0] == "cloud3000"} == set(ref.KNNS)
    assert all(c[1] == np.float64 for c in CASES if c[0] == "far")


@pytest.mark.parametrize("c", CASES, ids=ref.case_id)
def test_reference_is_pinned_by_the_oracle(c, oracle32, oracle64):
    name, T, knn, ratio, method, max_box = c
    xyz, _, r = ref.case(c)
    o = (oracle32 if T == np.float32 else oracle64).sampling_surface_normal(xyz, knn=knn, ratio=ratio, sampling_method=method, max_box_dim=max_box,
                                                                            seed=ref.SEED)
    ref.pinned(r, o)
    k = len(r["kept_idx"])
    assert r["eigen_values"].dtype == T and r["eigen_values"].shape == (k, 3)
    assert r["eigen_vectors"].dtype == T and r["eigen_vectors"].shape == (k, 9)
    assert r["densities"].dtype == T and r["densities"].shape == (k,)


@pytest.mark.parametrize("c", CASES, ids=ref.case_id)
def test_identities_on_the_reference(c):
    name, T, knn, ratio, method, max_box = c
    xyz, _, r = ref.case(c)
    ref.identities(r, method)
    # the columns are an orthonormal frame (Jacobi's V is a product of rotations)
    V = r["eigen_vectors"].astype(np.float64).reshape(-1, 3, 3)
    if len(V):
        assert np.abs(V @ V.transpose(0, 2, 1) - np.eye(3)).max() < 8 * np.finfo(T).eps
    # two kept points of one box carry identical rows; with samplingMethod 1 no two kept points share a box
    order = np.argsort(r["box_of"], kind="stable")
    same = np.flatnonzero(np.diff(r["box_of"][order]) == 0)
    if method == 1:
        assert len(same) == 0 and len(r["kept_idx"]) == r["boxes"]
    for key in ("eigen_values", "eigen_vectors", "densities", "normals"):
        a = r[key][order]
        assert np.array_equal(a[same], a[same + 1])


def test_scenes_do_what_they_are_for():
    for T in ref.TYPES:
        kw = lambda name, method=0: (name, T, 7, 0.5, method, ref.MAX_BOX.get(name, np.inf))
        assert ref.case(kw("collinear"))[2]["boxes"] == 0 and len(ref.case(kw("collinear"))[2]["kept_idx"]) == 0
        for name in ("mixed_line", "coincident", "big_box"):                               # some boxes are dropped, not all
            x, _, r = ref.case(kw(name, 1))
            assert 0 < r["boxes"] < len(ref.boxes_of(x, 7)), name
        x, _, r = ref.case(kw("big_box", 1))
        assert r["boxes"] < ref.run(x, T, 7, 0.5, 1, np.inf, ref.SEED)["boxes"]          # maxBoxDim drops at least one
        x, _, r = ref.case(kw("planar", 1))
        assert r["boxes"] > 0 and np.all(np.abs(r["normals"][:, 2]) == 1) and np.all(r["eigen_values"][:, 0] == 0)
    # the draw: ratio 1e-3 keeps few, 0.999 nearly all
    few = ref.case(("cloud3000", np.float32, 7, 1e-3, 0, np.inf))[2]
    most = ref.case(("cloud3000", np.float32, 7, 0.999, 0, np.inf))[2]
    assert 0 < len(few["kept_idx"]) < 15 and 2950 < len(most["kept_idx"]) < 3000
    # two box sizes on one level
    for knn in ref.KNNS:
        sizes = {len(m) for m in ref.boxes_of(ref.cloud(f"n{4 * knn + 3}", np.float64), knn)}
        assert len(sizes) == 2


@pytest.mark.parametrize("T", ref.TYPES)
def test_known_answers_on_an_exact_lattice(T):
    """flat_boxes: an 8 x 8 unit lattice in the plane z = 0.  With knn 4 the median cuts leave 16 boxes of 4; a box that is a unit
    square has its mean at its centre, the scatter diag(1, 1, 0), r2 = 1/2 and the density 4 / ((4/3) pi (1/2)^(3/2)): every
    operation exact up to the root"""
    x = ref.cloud("flat_boxes", T)
    r = ref.run(x, T, 4, 0.5, 1, np.inf, ref.SEED)
    squares = [i for i, m in enumerate(r["members"]) if len(m) == 4 and np.ptp(x[m, 0]) == 1 and np.ptp(x[m, 1]) == 1]
    assert len(squares) > 0
    rr = np.sqrt(T(0.5))
    want = T(4) / (T((4.0 / 3.0) * 3.14159265358979323846) * ((rr * rr) * rr))
    for i in squares:
        assert np.array_equal(r["eigen_values"][i], np.array([0, 1, 1], dtype=T))
        assert np.array_equal(np.abs(r["eigen_vectors"][i][:3]), np.array([0, 0, 1], dtype=T))
        assert r["densities"][i] == want and type(want) is T


@pytest.mark.parametrize("c", [c for c in CASES if c[4] == 1 and (c[0] in ref.SCENES or c[2] == 7)], ids=ref.case_id)
def test_densities_are_the_oracles_over_the_member_lists(c, oracle32, oracle64):
    """pgicp_density.h's statement is the oracle's orc_densities: handed the members of each kept point's box, in box order, as that
    point's neighbour list, it must give the reference's density bit for bit"""
    name, T, knn, ratio, method, max_box = c
    xyz, _, r = ref.case(c)
    ids = np.full((len(xyz), knn), -1, dtype=np.int32)
    for i, m in zip(r["kept_idx"], r["members"]):
        ids[i, :len(m)] = m
    with np.errstate(all="ignore"):
        d = (oracle32 if T == np.float32 else oracle64).densities(xyz, ids)
    assert d[r["kept_idx"]].tobytes() == r["densities"].tobytes()


def dropin_host(exe, T, cases, drows, average):
    """the filter's host form with all three rows on `cases`: a list of (kept xyz, descriptors (k, drows + 16))"""
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<i", len(cases)))
            for c in cases:
                name, _, knn, ratio, method, max_box = c
                xyz, d, _ = ref.case(c, drows, average)
                fh.write(struct.pack("<iiiiiddd", len(xyz), drows, knn, method, int(average), float(ratio), float(max_box), float(ref.SEED)))
                fh.write(xyz.tobytes() + (b"" if d is None else d.tobytes()))
        out = subprocess.run([exe, "host", "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        blob = open(fout, "rb").read()
    res, at, w = [], 0, np.dtype(T).itemsize
    for _ in cases:
        kept, dr = struct.unpack_from("<ii", blob, at)
        at += 8
        xyz = np.frombuffer(blob, dtype=T, count=3 * kept, offset=at).reshape(kept, 3)
        at += 3 * kept * w
        desc = np.frombuffer(blob, dtype=T, count=dr * kept, offset=at).reshape(kept, dr)
        at += dr * kept * w
        res.append((xyz, desc))
    assert at == len(blob)
    return res


@pytest.mark.parametrize("drows,average", [(0, True), (3, True), (3, False)])
@pytest.mark.parametrize("T", ref.TYPES)
def test_dropin_host_form_equals_the_reference(T, drows, average):
    exe = build_exe("test_sampling_normals_ext_cpu")
    cases = [c for c in CASES if c[1] == T and (drows == 0 or c[2] == 7)]
    got = dropin_host(exe, T, cases, drows, average)
    for c, (xyz, desc) in zip(cases, got):
        _, d, r = ref.case(c, drows, average)
        label = ref.case_id(c)
        assert xyz.tobytes() == r["xyz"].tobytes(), label
        assert desc.shape == (len(r["kept_idx"]), drows + 16), label
        if drows:
            assert desc[:, :drows].tobytes() == r["descriptors"].tobytes(), label
        at = drows
        for key, w in (("normals", 3), ("densities", 1), ("eigen_values", 3), ("eigen_vectors", 9)):
            assert np.ascontiguousarray(desc[:, at:at + w]).tobytes() == r[key].tobytes(), (label, key)
            at += w


def test_yaml_loading_refusals_constructors_and_exports():
    exe = build_exe("test_sampling_normals_ext_cpu")
    out = subprocess.run([exe, "yaml"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sampling normals ext cpu tests ok" in out.stdout


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_ssn_ext.h"\nint main(void) { return 0; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.SSN_EXT_SYMBOLS)
    assert not set(icp.SSN_EXT_SYMBOLS) & set(icp.ABI_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
