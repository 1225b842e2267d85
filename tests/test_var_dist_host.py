"""CPU-side checks of KDTreeVarDistMatcher's radii (include/pgicp_vardist.h): header, binding and library agree on the symbols; the
reference loop of tests/var_dist_ref.py is the oracle's, bit for bit, before anything rests on it; the cut's unit cases; and the
conditions the whole-ICP GPU tests (tests/test_gpu_var_dist.py) need of their scene, asserted on the reference alone."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pgslam_amd import icp  # noqa: E402
import var_dist_ref as ref  # noqa: E402

F32, F64 = np.float32, np.float64
_ORACLES = {}


def _oracle(dtype):
    from oracle import Oracle
    key = np.dtype(dtype).name
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(dtype)
    return _ORACLES[key]


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", "pgicp_vardist.h")).read()
    declared = sorted(set(re.findall(r"\b(pgicp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(icp.VARDIST_SYMBOLS)
    assert "pgicp_vardist.h" not in open(os.path.join(ROOT, "include", "pgicp.h")).read()
    assert '#include "pgicp.h"' in text
    lib = icp.load_library()
    assert lib.pgicp_abi_version() == 6
    for name in icp.VARDIST_SYMBOLS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("chain", sorted(ref.CHAINS))
@pytest.mark.parametrize("minimizer", [0, 1], ids=["p2plane", "p2point"])
def test_reference_loop_is_the_oracles(dtype, chain, minimizer):
    sc = ref.scene()
    o = _oracle(dtype)
    for T0 in sc["T_inits"]:
        a = ref.icp_ref(o, sc["rd"], sc["ref"], sc["ref_nrm"], T0, error_minimizer=minimizer, **ref.CHAINS[chain])
        b = o.icp(sc["rd"], sc["ref"], sc["ref_nrm"], T0, error_minimizer=minimizer, **ref.CHAINS[chain])
        assert a["status"] == b["status"] == 0
        assert ref.same_result(a, b), ref.diff_report(a, b)
        assert np.array_equal(a["last_ids"], b["last_ids"]) and a["last_d2"].tobytes() == b["last_d2"].tobytes()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_cut_unit_cases(dtype):
    T = np.dtype(dtype).type
    inf = T(np.inf)
    # r = inf cuts nothing; a point without a neighbour stays one
    ids, d2, rem = ref.cut(np.array([4, -1], np.int32), np.array([T(1.5), inf]), np.array([inf, inf]), 1, dtype)
    assert ids.tolist() == [4, -1] and d2.tolist() == [1.5, np.inf] and not rem.any()
    # r = 0 keeps d2 = 0 and nothing else
    ids, d2, rem = ref.cut(np.array([7, 8], np.int32), np.array([T(0), np.nextafter(T(0), T(1))]), np.array([T(0), T(0)]), 1, dtype)
    assert ids.tolist() == [7, -1] and d2[0] == 0 and d2[1] == inf and rem.tolist() == [False, True]
    # knn = 3: the tail beyond r * r goes; an all-cut point
    ids, d2, rem = ref.cut(np.array([[1, 2, 3], [4, 5, 6]], np.int32), np.array([[T(0.01), T(0.04), T(0.09)], [T(0.5), T(0.6), T(0.7)]]),
                           np.array([T(0.25), T(0.5)]), 3, dtype)
    assert ids.tolist() == [[1, 2, -1], [-1, -1, -1]]
    assert d2[0, :2].tolist() == [T(0.01), T(0.04)] and np.isinf(d2[0, 2]) and np.isinf(d2[1]).all()
    assert rem.tolist() == [[False, False, True], [True, True, True]]
    # d2 == r * r (the product in T) is kept; the next value up is not
    r = T(0.3)
    ids, d2, rem = ref.cut(np.array([9, 9], np.int32), np.array([r * r, np.nextafter(r * r, inf)]), np.array([r, r]), 1, dtype)
    assert ids.tolist() == [9, -1]
    assert d2.dtype == np.dtype(dtype) and ids.dtype == np.int32


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("chain", sorted(ref.CHAINS))
def test_scene_conditions(dtype, chain):
    """what tests/test_gpu_var_dist.py's whole-ICP cases need of the scene, on the reference alone: in iteration 1 at least 10 % of
    the pairs are cut; at least 100 points are cut in iteration 1 and kept in the last (the case a cut written over the matcher's
    own seeds would break); the ICP converges within 0.05 m of truth"""
    sc = ref.scene()
    o = _oracle(dtype)
    for T0 in sc["T_inits"]:
        a = ref.icp_ref(o, sc["rd"], sc["ref"], sc["ref_nrm"], T0, radii=sc["radii"].astype(dtype), **ref.CHAINS[chain])
        assert a["status"] == 0 and a["converged"]
        assert a["removed"][0].mean() >= 0.10
        assert int((a["removed"][0] & (a["last_ids"] >= 0)).sum()) >= 100
        d = np.linalg.inv(sc["T_truth"]) @ a["T"]
        assert np.linalg.norm(d[:3, 3]) < 0.05
