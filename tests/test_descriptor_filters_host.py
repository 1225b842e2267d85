"""include/pgicp_descriptor_filters.h without a device: the numpy arctangent of tests/descriptor_filters_ref.py against the oracle's
orc_atan2 and the product's det_atan2, to the bit; det_acos against the C library's acos; the per-point functions of
include/pgslam_amd/descriptor_filters_host.hpp (which the kernels call) through the drop-in's host filters against the statement, bit
for bit, on vectors that hold every guard; the YAML keys, refusals, labels, run detection and supportedNames()
(tests/cpp/test_descriptor_filters_cpu.cpp); the header as strict C99 and the library's exports; and the conditions the GPU tests
rest on, asserted on the reference alone."""
import ctypes as C
import math
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import descriptor_filters_ref as ref
from pgslam_amd import icp
from test_checkers_ref_host import ProductChecker
from test_density_host import build_exe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgicp_descriptor_filters.h")
EXE = "test_descriptor_filters_cpu"


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    p = ProductChecker(tmp_path_factory.mktemp("descriptor_filters_host"))
    p.lib.pgicp_host_atan2.restype = C.c_double
    return p


def acos_arguments():
    rng = np.random.default_rng(23)
    near = 10.0 ** rng.uniform(-17, -1, 4000)
    edge = np.array([0.4375, 0.6875, 1.1875, 2.4375])           # the reduction's breakpoints, as tangents: c = 1 / sqrt(1 + t t)
    c_edge = 1.0 / np.sqrt(1.0 + edge * edge)
    return np.concatenate([rng.uniform(-1.0, 1.0, 12000), 1.0 - near, near - 1.0, near, -near, c_edge, -c_edge,
                           np.nextafter(c_edge, 0.0), np.nextafter(c_edge, 1.0),
                           [1.0, -1.0, 0.0, -0.0, np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0), 1.0000001, -1.5, np.inf, -np.inf]])


def test_numpy_arctangent_equals_the_oracles_and_the_products(oracle32, product):
    rng = np.random.default_rng(5)
    n = 20_000
    y = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-14, 3, n) * rng.random(n)
    x = rng.choice([-1.0, 1.0, 1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 1, n)
    edge = np.array([0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -29, 2.0 ** 66, 1.0, 1e-300, 1e300])
    y = np.concatenate([y, edge, np.nextafter(edge, 0.0), np.nextafter(edge, np.inf), -edge, [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 1.0, np.nan, 1.0]])
    x = np.concatenate([x, np.ones(3 * len(edge)), -np.ones(len(edge)), [1.0, 1.0, -1.0, -1.0, 0.0, -0.0, 0.0, 0.0, -0.0, 1.0, np.nan]])
    # and the pairs det_acos forms: (sqrt((1 - c) (1 + c)), c)
    c = np.clip(acos_arguments(), -1.0, 1.0)
    y, x = np.concatenate([y, np.sqrt((1.0 - c) * (1.0 + c))]), np.concatenate([x, c])
    got = ref.atan2(y, x)
    for a, b, g in zip(y.tolist(), x.tolist(), got.tolist()):
        want = product.lib.pgicp_host_atan2(C.c_double(a), C.c_double(b))
        assert struct.pack("<d", want) == struct.pack("<d", oracle32.atan2(a, b)) or (math.isnan(want) and math.isnan(oracle32.atan2(a, b))), (a, b)
        assert struct.pack("<d", g) == struct.pack("<d", want) or (math.isnan(g) and math.isnan(want)), (a, b, g, want)


def product_acos(v):
    exe = build_exe(EXE)
    v = np.ascontiguousarray(v, dtype=np.float64)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<i", len(v)) + v.tobytes())
        out = subprocess.run([exe, "acos", fin, fout], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        return np.fromfile(fout, dtype=np.float64)


def test_det_acos_against_the_c_library():
    """within 4 ulp of acos in double -- one rounding each for the product, the root, the quotient and the polynomial (2 ulp was
    measured) --, equal to it once rounded to float, exact at the endpoints and 0, clamped outside [-1, 1], the same bits from the
    numpy statement"""
    c = acos_arguments()
    got = product_acos(c)
    assert got.tobytes() == ref.acos(c).tobytes()
    worst = 0.0
    for a, g in zip(c.tolist(), got.tolist()):
        want = math.acos(min(1.0, max(-1.0, a)))
        err = abs(g - want) / math.ulp(want) if want else abs(g)
        worst = max(worst, err)
        assert err <= 4.0, (a, g, want, err)
        assert np.float32(g) == np.float32(want), (a, g, want)
    print("det_acos: worst error", worst, "ulp over", len(c), "arguments")
    for a, want in ((1.0, 0.0), (-1.0, math.pi), (0.0, math.pi / 2), (-0.0, math.pi / 2), (1.0000001, 0.0), (-1.5, math.pi), (np.inf, 0.0), (-np.inf, math.pi)):
        assert product_acos([a])[0] == want, a
    assert np.isnan(product_acos([np.nan])[0]) and np.isnan(ref.acos(np.array([np.nan]))[0])


def host_vectors(T):
    """normals, observation directions, eigenvalues and values to cut that reach every guard of the three statements"""
    rng = np.random.default_rng(31)
    n = 6000
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    obs = rng.normal(size=(n, 3)) * 5
    obs[1000:2500] = nrm[1000:2500] * rng.uniform(0.1, 30, (1500, 1))          # parallel: |c| rounds to 1 and, for some, above it
    obs[2500:4000] = -nrm[2500:4000] * rng.uniform(0.1, 30, (1500, 1))         # antiparallel
    nrm, obs = nrm.astype(T), obs.astype(T)
    nrm[10] = 0                         # a zero normal: not normalised, c = 0, the angle pi / 2 exactly
    obs[20] = 0                         # a point at the sensor centre: the same
    nrm[30] *= T(1e-30)                 # (f32: the squared norm underflows to 0)
    obs[40] *= T(1e25)                  # (f32: the squared norm overflows: the direction becomes 0)
    nrm[50, 1] = np.nan
    eig = np.sort(rng.uniform(1e-4, 2.0, (n, 3)), axis=1).astype(T)
    eig[100:400] = eig[100:400][:, [2, 0, 1]]                                  # unsorted
    eig[400] = 0
    eig[401] = [0, 0, 1]
    eig[402] = [0, 1, 1]
    eig[403] = [np.finfo(T).smallest_subnormal, 1, 2]
    eig[404] = [np.finfo(T).smallest_subnormal, 2, np.finfo(T).smallest_subnormal]
    eig[405] = [np.finfo(T).tiny, np.finfo(T).tiny, np.finfo(T).tiny]
    eig[406] = [0.5, 0.5, 0.5]
    eig[407] = [1, 1, 2]
    eig[408] = [np.nan, 1, 2]
    eig[409] = [1, 2, np.nan]
    eig[410] = [-1e-7, 1, 2]
    eig[411] = [3, 2, 1]
    val = rng.normal(size=n).astype(T)
    thr = float(val[7])
    val[500:520] = T(thr)               # exactly the threshold
    val[600], val[601], val[602] = np.nan, np.inf, -np.inf
    return nrm, obs, eig, val, thr


def host_filters(T, nrm, obs, eig, val, thr, keep_u, keep_s, larger):
    exe = build_exe(EXE)
    n = len(nrm)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<iiii", n, keep_u, keep_s, larger) + struct.pack("<d", thr))
            for a in (nrm, obs, eig, val):
                fh.write(np.ascontiguousarray(a, dtype=T).tobytes())
        out = subprocess.run([exe, "host", "f32" if T == np.float32 else "f64", fin, fout], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        blob = open(fout, "rb").read()
    w, rows = np.dtype(T).itemsize, 2 + keep_u + keep_s
    made = np.frombuffer(blob, dtype=T, count=rows * n).reshape(rows, n)
    kept = struct.unpack_from("<i", blob, rows * n * w)[0]
    assert len(blob) == rows * n * w + 4 + 4 * kept
    return made, np.frombuffer(blob, dtype=np.int32, count=kept, offset=rows * n * w + 4)


@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_host_filters_equal_the_reference(T):
    nrm, obs, eig, val, thr = host_vectors(T)
    want_inc = ref.incidence_angle(nrm, obs, T)
    want_sph = ref.sphericality(eig, T)
    # the vectors do reach the guards
    a, b = ref.normalized(nrm, T), ref.normalized(obs, T)
    with np.errstate(all="ignore"):
        c = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(np.float64)
    assert np.any(c > 1.0) and np.any(c < -1.0)
    assert want_inc[c > 1.0].max() == 0 and np.all(want_inc[c < -1.0] == T(math.pi))
    assert want_inc[10] == want_inc[20] == T(math.pi / 2) and np.isnan(want_inc[50])
    assert np.isnan(want_sph[0][[400, 401, 404, 408, 409]]).all() and not np.isnan(want_sph[0][[402, 403, 406, 407, 410, 411]]).any()
    assert want_sph[0][406] == 1 and want_sph[1][406] == 1 and want_sph[2][406] == 0
    assert [v[411] for v in want_sph] == [v[0] for v in ref.sphericality(np.array([[1, 2, 3]], dtype=T), T)]
    half_pi = T(math.pi / 2)
    assert np.any(want_inc < half_pi) and np.any(want_inc > half_pi)
    for keep_u, keep_s, larger in ((0, 0, 1), (1, 0, 0), (0, 1, 1), (1, 1, 0)):
        made, kept = host_filters(T, nrm, obs, eig, val, thr, keep_u, keep_s, larger)
        label = (keep_u, keep_s, larger)
        assert made[0].tobytes() == want_inc.tobytes(), label
        assert made[1].tobytes() == want_sph[0].tobytes(), label
        if keep_u:
            assert made[2].tobytes() == want_sph[1].tobytes(), label
        if keep_s:
            assert made[2 + keep_u].tobytes() == want_sph[2].tobytes(), label
        want_kept = np.flatnonzero(ref.cut_keep(val, thr, larger, T))
        assert np.array_equal(kept, want_kept), label
        assert 0.1 * len(val) < len(kept) < 0.9 * len(val) and 600 not in kept and set(range(500, 520)) <= set(kept.tolist()), label
        assert (601 in kept) == (not larger) and (602 in kept) == bool(larger), label


def test_yaml_keys_refusals_labels_and_run_detection():
    exe = build_exe(EXE)
    env = dict(os.environ)
    env.pop("PGSLAM_HOST_SENSOR_CHAIN", None)
    out = subprocess.run([exe, "yaml"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "descriptor filters cpu tests ok" in out.stdout


def test_header_is_strict_c99():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        with open(src, "w") as fh:
            fh.write('#include "pgicp_descriptor_filters.h"\nint main(void) { pgicp_chain_out o; pgicp_chain_stage s; o.nstride = 3; '
                     's.type = PGICP_CHAIN_CUT_AT_DESCRIPTOR; return s.type - 8 + o.nstride - 3 + PGICP_FILTER_CUT_AT_DESCRIPTOR - 9; }\n')
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pgicp_\w+)\s*\(", text)))
    assert declared == sorted(icp.DESCRIPTOR_FILTERS_SYMBOLS)
    assert not set(icp.DESCRIPTOR_FILTERS_SYMBOLS) & (set(icp.ABI_SYMBOLS) | set(icp.SENSOR_CHAIN_SYMBOLS))
    lib = icp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pgicp_abi_version() == 6                      # the pinned ABI is untouched
    # the constants of the header and of the binding agree
    defines = dict(re.findall(r"#define (PGICP_\w+)\s+(\d+)", open(HEADER).read()))
    for name in ("CHAIN_INCIDENCE_ANGLE", "CHAIN_SPHERICALITY", "CHAIN_CUT_AT_DESCRIPTOR", "CHAIN_EXT_MAX_STAGES", "CHAIN_EXT_MAX_CUTS", "FILTER_CUT_AT_DESCRIPTOR"):
        assert getattr(icp, name) == int(defines["PGICP_" + name]), name
    for name, value in icp.CHAIN_ROWS.items():
        assert int(defines["PGICP_CHAIN_ROW_" + name.upper()]) == value, name
    assert icp.C.sizeof(icp.ChainOut) == 13 * 8
    arr = icp.Context.chain_stages([("incidence_angle",), ("sphericality", 1, 0), ("cut_at_descriptor", "sphericality", 1, 0.2), ("cut_at_descriptor", 2, 0, -1.5)])
    assert [a.type for a in arr] == [icp.CHAIN_INCIDENCE_ANGLE, icp.CHAIN_SPHERICALITY, icp.CHAIN_CUT_AT_DESCRIPTOR, icp.CHAIN_CUT_AT_DESCRIPTOR]
    assert list(arr[1].p) == [1.0, 0.0, 0.0, 0.0] and list(arr[2].p) == [3.0, 1.0, 0.2, 0.0] and list(arr[3].p) == [0.0, 0.0, -1.5, 2.0]
    with pytest.raises(ValueError):
        icp.Context.chain_stages([("cut_at_descriptor", "sphericity", 1, 0.2)])


# ---- the conditions the GPU tests rest on, on the reference alone ----------------------------------------------------------

@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_main_scene_every_cut_keeps_between_a_tenth_and_nine_tenths(T):
    x = ref.sc.scene(ref.MAIN_N, T)
    lists = ref.stage_lists(x, T)
    for name in ("yaml", "cut_alone_dens", "cut_alone_dens_smaller", "cut_ahead_of_shadow_md", "cut_behind_shadow_md", "md_behind_cut", "inc_behind_shadow", "two_cuts"):
        r = ref.run(x, T, lists[name])
        seen = 0
        for stage, arrived, passed in zip(r["names"], r["arrived"], r["passed"]):
            if stage in (ref.CUT, ref.SHADOW, ref.MAXDENS):
                print(T.__name__, name, stage, arrived, "->", passed)
                assert 0 < passed < arrived, (name, stage, arrived, passed)            # every dropping stage drops some and keeps some
            if stage == ref.CUT:
                assert 0.1 < passed / arrived < 0.9, (name, stage, arrived, passed)
                seen += 1
        assert seen >= 1, name
    assert ref.run(x, T, lists["cut_drops_all"])["count"] == 0 and ref.run(x, T, lists["cut_nan_threshold"])["count"] == 0
    r = ref.run(x, T, lists["cut_keeps_all"])
    assert r["passed"][2] == len(x) and 0 < r["count"] < len(x)
    # the rank rule: MaxDensity behind a cut draws with the survivors' ranks -- not what a draw on the input index would keep
    r = ref.run(x, T, lists["md_behind_cut"])
    alone = ref.run(x, T, [lists["md_behind_cut"][-1]])
    cut_only = ref.run(x, T, lists["md_behind_cut"][:-1])
    assert not np.array_equal(r["kept_idx"], np.intersect1d(cut_only["kept_idx"], alone["kept_idx"]))


@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_unoriented_normals_give_angles_on_both_sides_of_half_pi(T):
    x = ref.sc.scene(ref.MAIN_N, T)
    a = ref.run(x, T, ref.stage_lists(x, T)["inc_alone"])["incidence_angles"]
    half_pi = T(math.pi / 2)
    assert np.count_nonzero(a < half_pi) > 0.1 * len(a) and np.count_nonzero(a > half_pi) > 0.1 * len(a)
    oriented = ref.run(x, T, [(ref.OBS,) + ref.CENTER, (ref.ORIENT, 1), (ref.INC,)])["incidence_angles"]
    assert np.all(oriented <= half_pi)


def duplicated_scene(T):
    """40 copies of each of 300 points, as tests/test_gpu_sensor_chain.py builds it: every neighbour coincides, every eigenvalue is 0"""
    rng = np.random.default_rng(11)
    base = np.round(rng.normal(size=(300, 3)) * 3 * 64) / 64 + np.array([4.0, 0.0, 0.0])
    return np.ascontiguousarray(np.repeat(base, 40, axis=0)[rng.permutation(12000)], dtype=T)


@pytest.mark.parametrize("T", ref.TYPES, ids=["f32", "f64"])
def test_duplicated_points_give_nan_sphericality(T):
    dup = duplicated_scene(T)
    r = ref.run(dup, T, [(ref.SPH, 1, 1)])
    assert np.isnan(r["sphericality"]).all() and np.isnan(r["unstructureness"]).all() and np.isnan(r["structureness"]).all()
    for larger in (0, 1):
        assert ref.run(dup, T, [(ref.SPH, 0, 0), (ref.CUT, "sphericality", larger, 0.5)])["count"] == 0
