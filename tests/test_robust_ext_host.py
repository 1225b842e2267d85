"""CPU-side checks of RobustOutlierFilter's distanceType, berg scale and nbIterationForScale (include/pgicp_robust.h): header,
binding and library agree on the symbols and the header is strict C99; the numpy statement of tests/robust_ext_ref.py is the
oracle's wherever the oracle has a statement (the seven weight expressions; the whole loop at mad / nb 0 / point2point), bit for
bit, before anything rests on it; berg's recurrence against values worked out by hand; the hold rule; and the conditions the GPU
tests (tests/test_gpu_robust_ext.py) need of their scene, asserted on the reference alone."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pgslam_amd import icp  # noqa: E402
import robust_ext_ref as ref  # noqa: E402

F32, F64 = np.float32, np.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
_ORACLES = {}


def _oracle(dtype):
    from oracle import Oracle
    key = np.dtype(dtype).name
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(dtype)
    return _ORACLES[key]


def test_header_binding_and_library_agree():
    path = os.path.join(ROOT, "include", "pgicp_robust.h")
    text = open(path).read()
    declared = sorted(set(re.findall(r"\b(pgicp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(icp.ROBUST_SYMBOLS)
    assert "pgicp_robust.h" not in open(os.path.join(ROOT, "include", "pgicp.h")).read()
    assert '#include "pgicp.h"' in text
    for name, code in (("PGICP_ROBUST_DIST_POINT2POINT", 0), ("PGICP_ROBUST_DIST_POINT2PLANE", 1), ("PGICP_ROBUST_SCALE_BERG", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, code), text), name
    assert icp.ROBUST_DIST == ref.DIST and icp.ROBUST_SCALE == ref.EST
    lib = icp.load_library()
    assert lib.pgicp_abi_version() == 6
    for name in icp.ROBUST_SYMBOLS:
        assert hasattr(lib, name), name
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:      # (strict C99, as pgicp.h is)
        r = subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ---- the weight expressions ----------------------------------------------------------------------------------------------------
@DTYPES
def test_weight_expressions_are_the_oracles(dtype):
    """all seven functions, scale none and mad, with and without an approximation, pairs without a neighbour: bit for bit those of
    orc_robust_weights -- welsch to the allowance tests/test_gpu_chain.py grants its exp(), and no wider"""
    o = _oracle(dtype)
    bits = np.uint32 if dtype == F32 else np.uint64
    rng = np.random.default_rng(77)
    d2 = (rng.gamma(1.5, 0.02, size=5001) ** 2).astype(dtype)
    d2[rng.integers(0, d2.size, 40)] = np.inf
    for fct in range(1, 8):
        for est in (0, 1):
            for tuning, approx in ((1.0, 0.0), (2.5, 0.0), (1.0, 1.5)):
                ow, os2 = o.robust_weights(d2, fct, tuning, est, approx)
                s = ref.scale(est, 0, 1, 0, d2, tuning, dtype)
                s2 = s * s
                assert np.asarray(s2, dtype=dtype).tobytes() == np.asarray(os2, dtype=dtype).tobytes()
                w = ref.weights(d2, fct, tuning, s2, approx, dtype)
                assert w.dtype == np.dtype(dtype)
                if fct == 2:
                    np.testing.assert_allclose(w, ow, rtol=8 * np.finfo(dtype).eps, atol=np.finfo(dtype).tiny)
                else:
                    assert np.array_equal(w.view(bits), ow.view(bits)), (fct, est, tuning, approx)
                assert np.all(w[np.isinf(d2)] == 0)


@DTYPES
@pytest.mark.parametrize("minimizer", [0, 1], ids=["p2plane", "p2point"])
@pytest.mark.parametrize("fct", ["cauchy", "tukey"])
def test_reference_loop_is_the_oracles(dtype, minimizer, fct):
    """mad, nb = 0, point2point: the composition itself -- every entry of the list against a run of Oracle.icp with that max_iters"""
    sc = ref.scene()
    o = _oracle(dtype)
    for n in (257, 2049):
        rd = ref.reading(n)
        for approx in (False, True):
            ch = ref.chain(fct, 1, approx)
            snaps = ref.icp_ref(o, rd, sc["ref"], sc["ref_nrm"], sc["T_init"], error_minimizer=minimizer, **ch)
            assert len(snaps) == ch["max_iters"]
            for k in (1, 2, 3, 6):
                b = o.icp(rd, sc["ref"], sc["ref_nrm"], sc["T_init"], error_minimizer=minimizer, **dict(ch, max_iters=k))
                a = snaps[k - 1]
                assert a["status"] == b["status"] == 0 and a["iterations"] == k
                assert ref.same_result(a, b), (n, approx, k, ref.diff_report(a, b))
                assert np.array_equal(a["last_ids"], b["last_ids"]) and a["last_d2"].tobytes() == b["last_d2"].tobytes()


# ---- the scale rules -------------------------------------------------------------------------------------------------------------
# median 0.0625 (its root 0.25 is exact), target 0.3; every operation rounded once to the type, worked out in exact rationals:
#   s1 = rn(rn(1.9) / 4);  s(k + 1) = rn(rn(rn(0.85) * rn(s(k) - rn(0.3))) + rn(0.3))
BERG_HAND = {
    "float32": ["0x1.e66666p-2", "0x1.cb8520p-2", "0x1.b4ac0ap-2", "0x1.a14050p-2", "0x1.90be58p-2"],
    "float64": ["0x1.e666666666666p-2", "0x1.cb851eb851eb8p-2", "0x1.b4ac083126e97p-2", "0x1.a1404ea4a8c15p-2", "0x1.90be5753a3ec0p-2"],
}


@DTYPES
def test_berg_recurrence_by_hand(dtype):
    T = np.dtype(dtype).type
    d2 = np.array([0.01, 0.0625, 0.25, np.inf, 0.04, 0.09], dtype=dtype)        # finite, sorted: .01 .04 .0625 .09 .25 -> [5 // 2]
    assert ref.median(d2) == T(0.0625)
    s = T(0)
    for it, want in enumerate(BERG_HAND[np.dtype(dtype).name], start=1):
        s = ref.scale(ref.EST["berg"], 0, it, s, d2, 0.3, dtype)
        assert isinstance(s, T) and float(s) == float.fromhex(want), (it, float(s).hex(), want)
    # later iterations read no distance
    assert ref.scale(ref.EST["berg"], 0, 2, T(0.5), None, 0.3, dtype) == T(0.85) * (T(0.5) - T(0.3)) + T(0.3)


@DTYPES
@pytest.mark.parametrize("nb", [0, 1, 2, 5])
def test_hold_rule(dtype, nb):
    T = np.dtype(dtype).type
    assert [ref.estimates(nb, it) for it in range(1, 8)] == [nb == 0 or it <= nb for it in range(1, 8)]
    rng = np.random.default_rng(5)
    clouds = [(rng.gamma(2.0, 0.05 * (it + 1), size=301) ** 2).astype(dtype) for it in range(7)]
    for est in ("mad", "berg"):
        s, hist = T(0), []
        for it in range(1, 8):
            s = ref.scale(ref.EST[est], nb, it, s, clouds[it - 1], 0.3, dtype)
            hist.append(s)
        free = [ref.scale(ref.EST["mad"], 0, it, T(0), clouds[it - 1], 0.3, dtype) for it in range(1, 8)]
        for it in range(1, 8):
            if est == "mad" and ref.estimates(nb, it):
                assert hist[it - 1] == free[it - 1] == np.sqrt(T(ref.mad(clouds[it - 1])))
            elif not ref.estimates(nb, it):
                assert hist[it - 1] == hist[nb - 1]                       # held: the scale of the last estimating iteration
            elif it > 1:
                assert hist[it - 1] == T(0.85) * (hist[it - 2] - T(0.3)) + T(0.3) != hist[it - 2]
    assert ref.scale(ref.EST["none"], nb, 3, T(7), clouds[0], 0.3, dtype) == T(1)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_scene_conditions(dtype):
    """what a pass of tests/test_gpu_robust_ext.py rests on, on the reference alone"""
    sc = ref.scene()
    o = _oracle(dtype)
    assert len(sc["ref"]) == ref.MAP_POINTS
    for n in ref.SIZES:
        rd = ref.reading(n)
        assert len(rd) == n
        run = lambda dist, est, nb, fct, approx: ref.icp_ref(o, rd, sc["ref"], sc["ref_nrm"], sc["T_init"], distance_type=dist, scale_estimator=est,
                                                             nb=nb, **ref.chain(fct, est, approx))       # noqa: E731
        if n == 1:
            # the one pair has a neighbour; the berg chain runs on it; under mad the deviation of one value is 0, the pair's weight 0
            # in float (no point to minimise) and the floor 1e-50 in double -- all three ends are compared on the device
            assert run(0, 2, 0, "cauchy", False)[0]["status"] == 0
            assert run(0, 1, 0, "cauchy", False)[0]["status"] == (1 if dtype == F32 else 0)
            continue
        for est in (0, 1, 2):
            for fct in ("cauchy", "tukey"):
                point, plane = run(0, est, 0, fct, False), run(1, est, 0, fct, False)
                for r in point + plane:
                    assert r["status"] == 0
                assert point[-1]["iterations"] == plane[-1]["iterations"] == ref.BASE["max_iters"]     # every iteration asked for runs
                # at least one reading point has no neighbour under max_dist, in every iteration (the moved one)
                assert all(r["last_ids"][1] == -1 and r["w"][1] == 0 for r in point + plane)
                # plane and point weights differ on more than a tenth of the pairs
                has = point[0]["last_ids"] >= 0
                assert np.array_equal(point[0]["last_ids"], plane[0]["last_ids"])
                assert (point[0]["w"][has] != plane[0]["w"][has]).mean() > 0.1, (n, est, fct)
                if est:
                    # from iteration 3 on the nb = 2 scale is not the nb = 0 scale (and before, it is)
                    for dist in (0, 1):
                        held, free = run(dist, est, 2, fct, False)[-1]["s_hist"], (point, plane)[dist][-1]["s_hist"]
                        assert held[:2] == free[:2] and all(held[k] == held[1] != free[k] for k in range(2, 6)), (n, est, fct, dist)
                if n >= 257:
                    # the approximation zeroes some pairs in the first iteration and in the last, there fewer than half of those with
                    # a neighbour (the smaller readings have too few pairs far from their planes for the first half of that; the
                    # first guess leaves more than half of the pairs beyond it at scale 1)
                    for dist in (0, 1):
                        a = run(dist, est, 0, fct, True)
                        for r, most in ((a[0], 1.0), (a[-1], 0.5)):
                            s, a_ = r["s_hist"][r["iterations"] - 1], np.dtype(dtype).type(ref.APPROX[est])
                            has = r["last_ids"] >= 0
                            cutoff = has & (np.where(has, r["dd"], 0) / (s * s) >= a_ * a_)
                            assert (r["w"][cutoff] == 0).all()
                            assert 0 < cutoff.sum() < most * has.sum(), (n, est, fct, dist)


@DTYPES
def test_batch_scene_converges_at_different_iterations(dtype):
    sc = ref.scene()
    o = _oracle(dtype)
    for est, dist, nb in ((1, 1, 5), (2, 1, 3)):
        its = []
        for rd, T0 in ref.batch_problems():
            r = ref.icp_ref(o, rd, sc["ref"], sc["ref_nrm"], T0, distance_type=dist, scale_estimator=est, nb=nb,
                            **dict(ref.chain("cauchy", est, True), **ref.BATCH_CHECKERS))[-1]
            assert r["status"] == 0 and r["converged"]
            its.append(r["iterations"])
        assert len(set(its)) == 3, its
        # with nb = 5 the residual pass behind the ICPs estimates the scale of one problem and holds another's
        assert min(its) + 1 <= 5 < max(its) + 1
