"""include/pgicp_elipsoids.h without a device: the numpy statement (tests/elipsoids_ref.py, built on the oracle-pinned
tests/sampling_normals_ext_ref.py) against itself -- identities, the planarity drop, a known answer --, and the drop-in without a
device (tests/cpp/test_elipsoids_cpu.cpp): the filter's host form (PGSLAM_HOST_ELIPSOIDS=1) against the statement bit for bit, with
only keepNormals and minPlanarity 0 against SamplingSurfaceNormalDataPointsFilter's host form byte for byte, the YAML forms and
refusals, the constructors, descriptor order and overwrite-when-present, the header as strict C99 and the library's exports."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import elipsoids_ref as ref
import sampling_normals_ext_ref as ssn
from pgslam_amd import icp
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgicp_elipsoids.h")
CASES = ref.cases()
# name -> the cloud and knn whose picked threshold the planarity cases use
PICKED = ("cloud3000", "mixed_line")


def test_the_suite_covers_what_it_says():
    names = {c[0] for c in CASES}
    for knn in ref.KNNS:
        for n in ssn.small_n(knn):
            assert f"n{n}" in names
    assert set(ssn.SCENES) <= names
    assert {c[2] for c in CASES} == {3, 7, 1024}
    assert {c[4] for c in CASES if c[0] == "cloud3000" and c[2] == 7} == {0, 1}
    assert all(c[1] == np.float64 for c in CASES if c[0] == "far")


@pytest.mark.parametrize("c", CASES, ids=ref.case_id)
def test_reference_equals_the_pinned_statement_and_keeps_its_identities(c):
    """with minPlanarity 0 the older outputs are sampling_normals_ext_ref's (which the oracle pins) byte for byte"""
    name, T, knn, ratio, method, max_box = c
    xyz, _, r = ref.case(c)
    o = ssn.run(xyz, T, knn, ratio, method, max_box, ref.SEED)
    assert r["boxes"] == o["boxes"]
    for key in ("kept_idx", "xyz", "normals", "eigen_values", "eigen_vectors", "densities"):
        assert r[key].tobytes() == o[key].tobytes() and r[key].dtype == o[key].dtype, key
    k = len(r["kept_idx"])
    for key, w in ref.ROWS.items():
        assert r[key].dtype == T and r[key].shape == ((k, w) if w > 1 else (k,)), key
    ref.identities(r, method, knn)
    if method == 1:
        assert k == r["boxes"] and r["weights"].sum() == sum(len(m) for m in r["members"])


@pytest.mark.parametrize("T", ref.TYPES)
@pytest.mark.parametrize("name", PICKED)
def test_picked_threshold_drops_some_boxes_and_not_others(name, T):
    x = ref.cloud(name, T)
    thr = ref.pick_min_planarity(x, T, 7)
    c = (name, T, 7, 0.5, 1, np.inf)
    full, part, none = (ref.case(c, min_planarity=m)[2] for m in (0.0, thr, 1.0))
    assert 0 < part["boxes"] < full["boxes"] and none["boxes"] == 0 and len(none["kept_idx"]) == 0
    assert np.all(part["shapes"][:, 0] >= T(thr))
    dropped = np.setdiff1d(full["kept_idx"], part["kept_idx"])
    assert len(dropped) == full["boxes"] - part["boxes"]
    pl = dict(zip(full["kept_idx"].tolist(), full["shapes"][:, 0]))
    assert all(pl[i] < T(thr) for i in dropped.tolist())
    # what stays keeps its rows
    at = np.searchsorted(full["kept_idx"], part["kept_idx"])
    for key in ref.ALL:
        assert part[key].tobytes() == full[key][at].tobytes(), key


@pytest.mark.parametrize("T", ref.TYPES)
def test_known_answers_on_an_exact_lattice(T):
    """flat_boxes: an 8 x 8 unit lattice in the plane z = 0.  With knn 4 a box that is a unit square has the scatter diag(1, 1, 0):
    eigenvalues 0, 1, 1, so v = (1/2, 1/2, 0), planarity 1, cylindricality 0, sphericality 0, weight 4 -- every operation exact"""
    x = ref.cloud("flat_boxes", T)
    r = ref.run(x, T, 4, 0.5, 1, np.inf, 0.0, ref.SEED)
    squares = [i for i, m in enumerate(r["members"]) if len(m) == 4 and np.ptp(x[m, 0]) == 1 and np.ptp(x[m, 1]) == 1]
    assert len(squares) > 0
    for i in squares:
        assert np.array_equal(r["shapes"][i], np.array([1, 0, 0], dtype=T))
        assert np.array_equal(r["covariance"][i], np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], dtype=T))
        assert r["weights"][i] == 4
    # minPlanarity 1.0 keeps exactly the boxes whose planarity is 1 (strict <)
    one = ref.run(x, T, 4, 0.5, 1, np.inf, 1.0, ref.SEED)
    assert one["boxes"] == int(np.sum(r["shapes"][:, 0] == 1)) > 0


def dropin_host(exe, T, cases, drows, average, min_planarity):
    """the filter's host form with every row on `cases`: a list of (kept xyz, descriptors (k, drows + 32))"""
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<i", len(cases)))
            for c, mp in zip(cases, min_planarity):
                name, _, knn, ratio, method, max_box = c
                xyz, d, _ = ref.case(c, drows, average, mp)
                fh.write(struct.pack("<iiiiidddd", len(xyz), drows, knn, method, int(average), float(ratio), float(max_box), float(ref.SEED), float(mp)))
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


def planarity_cases(T):
    """(case, minPlanarity): the picked threshold on the random and the mixed-line cloud, both methods, and 1.0 on the random cloud"""
    out = []
    for name in PICKED:
        thr = ref.pick_min_planarity(ref.cloud(name, T), T, 7)
        out += [((name, T, 7, 0.5, method, np.inf), thr) for method in (0, 1)]
    out.append((("cloud3000", T, 7, 0.5, 0, np.inf), 1.0))
    return out


@pytest.mark.parametrize("drows,average", [(0, True), (3, True), (3, False)])
@pytest.mark.parametrize("T", ref.TYPES)
def test_dropin_host_form_equals_the_reference(T, drows, average):
    exe = build_exe("test_elipsoids_cpu")
    cases = [(c, 0.0) for c in CASES if c[1] == T and (drows == 0 or c[2] == 7)] + planarity_cases(T)
    got = dropin_host(exe, T, [c for c, _ in cases], drows, average, [m for _, m in cases])
    for (c, mp), (xyz, desc) in zip(cases, got):
        _, d, r = ref.case(c, drows, average, mp)
        label = (ref.case_id(c), mp)
        assert xyz.tobytes() == r["xyz"].tobytes(), label
        assert desc.shape == (len(r["kept_idx"]), drows + 32), label
        if drows:
            assert desc[:, :drows].tobytes() == r["descriptors"].tobytes(), label
        at = drows
        for key, w in ref.ROWS.items():                                  # the statement's order
            assert np.ascontiguousarray(desc[:, at:at + w]).tobytes() == r[key].tobytes(), (label, key)
            at += w


def test_yaml_loading_refusals_constructors_and_exports():
    exe = build_exe("test_elipsoids_cpu")
    out = subprocess.run([exe, "yaml"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "elipsoids cpu tests ok" in out.stdout


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_elipsoids.h"\nint main(void) { return 0; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.ELIPSOIDS_SYMBOLS)
    assert not set(icp.ELIPSOIDS_SYMBOLS) & set(icp.ABI_SYMBOLS)
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
    assert callable(getattr(icp.Context, "elipsoids", None))
