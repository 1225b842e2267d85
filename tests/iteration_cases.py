"""The scene, the trajectory and the cases of tests/test_gpu_iteration_control.py.  They live here, apart from the GPU test,
because tests/test_checkers_ref_host.py walks the same cases on the CPU: through the product's checker_check compiled for the
host, against tests/checkers_ref.py.  TEST INFRASTRUCTURE ONLY.

The trajectory.  One small scene, synth.make_two_scans(3000, rings=16), map not centred (T_out = T_iter T_init then).  The
cases need an ICP that still moves at iteration 20 and whose smoothed step series fall by at least 1 % an iteration for every
smoothLength of the grid -- smoothLength 1, the raw steps, included.  A trimmed chain does not give that on this scene from any
start error or maxDist / ratio tried (64 combinations: the kept set changes by whole points, the raw steps go up and down;
with a large start error they wander for 26 iterations).  A chain whose weights are a smooth function of the distances does:
RobustOutlierFilter{GM, tuning 0.02, MAD scale} (a rational weight: no transcendental, bit for bit on the device) converges
linearly, each step about 0.65 of the one before, once its first six iterations are over.  So the start pose is where the
float64 oracle stands after those six: from there 24 iterations shrink the steps by 3e-5, which stays above float32's floor."""
import math

import numpy as np

import checkers_ref as cr
from pgslam_amd import synth

SMOOTH = (1, 2, 3, 7, 15)
K_TRAJ = 24                                  # iterations of the recorded trajectory
PREROLL = 6
BASE = dict(max_dist=2.0, trim_ratio=1.0, sensor_std_dev=0.01, robust_fct=4, robust_tuning=0.02, robust_scale=1)
FREE = dict(min_diff_rot=0.0, min_diff_trans=0.0, smooth_length=3, bound_max_rot=0.0, bound_max_trans=0.0)
# the device keeps 16 history entries, the identity first: its 16th check is the first that shifts them
STOPS = {1: (2, 9, 17), 2: (3, 10, 18), 3: (4, 11, 19), 7: (8, 12, 20), 15: (16, 17, 20)}

CASES = (
    [("a", s, k) for s in SMOOTH for k in STOPS[s]] +                      # Differential stops on both sides of the shift
    [("b", s, m) for s in (1, 15) for m in (1, 2, 15, 16, 17, 18, 24)] +   # Counter stops straddling it; 1, 2: the pass enqueued ahead
    [("c", 3, 11), ("c", 15, 16), ("c", 1, 17), ("c", 7, 8)] +             # Counter and Differential on the same iteration
    [("d", "rot", 3), ("d", "trans", 2), ("d", "both", 3), ("d", "both", 2)] +     # Bound exceeded at k < max_iters
    [("e", "rot", 3), ("e", "trans", 2), ("e", "both", 4)]                 # Bound first exceeded at k = max_iters: the Counter's stop stands
)


def case_id(case):
    return "-".join(str(x) for x in case)


def scene(oracle64):
    """(reading, map points, map normals) in float32 as the generator gives them, and the start pose"""
    s = synth.make_two_scans(3000, rings=16)
    T_far = s["T_init"] @ synth.se3(0.3, -0.2, 0.1, math.radians(2.0), math.radians(0.5), math.radians(-0.4))
    o = oracle64.icp(s["reading_xyz"], s["ref_xyz"], s["ref_nrm"], T_far, center_reference=False, max_iters=PREROLL, **dict(FREE, **BASE))
    assert o["status"] == 0 and o["iterations"] == PREROLL
    return s["reading_xyz"], s["ref_xyz"], s["ref_nrm"], o["T"].copy()


def mat4_mul(a, b):
    """a b as the library and the oracle form it: every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3, no fused multiply-add"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    c = np.zeros((4, 4))
    for k in range(4):
        c = c + a[:, k:k + 1] * b[k:k + 1, :]
    return c


def trajectory(orc, dtype, sc):
    """the oracle's trace of K_TRAJ free iterations: T_iter after every iteration, and T_out = T_iter T_init for each"""
    rd, ref, nrm, T_init = sc
    o = orc.icp(rd.astype(dtype), ref.astype(dtype), nrm.astype(dtype), T_init, trace=True, center_reference=False,
                max_iters=K_TRAJ, **dict(FREE, **BASE))
    assert o["status"] == 0 and o["iterations"] == K_TRAJ and o["max_iter_reached"] and not o["converged"]
    trace = [o["trace"][k].copy() for k in range(K_TRAJ)]
    T_out = [mat4_mul(T, T_init) for T in trace]
    assert T_out[-1].tobytes() == o["T"].tobytes()                 # center=False: T_out = T_iter T_init, to the bit
    return trace, T_out


def assert_moves_through_20(trace):
    """what the cases stand on: every smoothed series falls by at least 1 % an iteration through iteration 20, and the Bound
    checker's two quantities grow by at least 1 % an iteration over the iterations the Bound cases use"""
    for s in SMOOTH:
        ser = cr.smoothed_series(trace, s)
        for k in range(s, 20):
            for j in (0, 1):
                assert 0.0 < ser[k + 1][j] <= 0.99 * ser[k][j], (s, k, j, ser[k][j], ser[k + 1][j])
    b = cr.bound_series(trace)
    for k in range(1, 5):
        for j in (0, 1):
            assert b[k + 1][j] >= 1.01 * b[k][j], (k, j, b[k][j], b[k + 1][j])


def settings(case, trace):
    """the checkers' parameters of a case: every limit is the geometric mean of two adjacent values of the series it is
    compared with (checkers_ref.between), so every decision sits half a percent away from a double"""
    kind, x, k = case
    p = dict(FREE, max_iters=K_TRAJ)
    if kind in ("a", "c"):
        ser = cr.smoothed_series(trace, x)
        p.update(smooth_length=x, min_diff_rot=cr.between(ser[k - 1][0], ser[k][0]), min_diff_trans=cr.between(ser[k - 1][1], ser[k][1]))
        if kind == "c":
            p.update(max_iters=k)
    elif kind == "b":
        p.update(smooth_length=x, max_iters=k)
    else:
        b = cr.bound_series(trace)
        if x == "rot":
            p.update(bound_max_rot=cr.between(b[k - 1][0], b[k][0]))
        elif x == "trans":
            p.update(bound_max_trans=cr.between(b[k - 1][1], b[k][1]))
        elif k % 2:          # both limits set; the translation's is passed first, the rotation's an iteration later
            p.update(bound_max_rot=cr.between(b[k][0], b[k + 1][0]), bound_max_trans=cr.between(b[k - 1][1], b[k][1]))
        else:                # ... and the other way round
            p.update(bound_max_rot=cr.between(b[k - 1][0], b[k][0]), bound_max_trans=cr.between(b[k][1], b[k + 1][1]))
        if kind == "e":
            p.update(max_iters=k)
    return p


def expected(case, trace):
    """(iterations, converged, max_iter_reached, status) by the plain reference, and the margin of its decisions"""
    p = settings(case, trace)
    args = (p["min_diff_rot"], p["min_diff_trans"], p["smooth_length"], p["bound_max_rot"], p["bound_max_trans"])
    want = cr.run(trace, p["max_iters"], *args)
    return want, cr.margin(trace, want[0], *args)


def foreseen(case):
    """what the case is built to show, written down before any checker runs: (iterations, converged, max_iter_reached, status)"""
    kind, x, k = case
    return {"a": (k, True, False, cr.OK), "b": (k, False, True, cr.OK), "c": (k, True, True, cr.OK),
            "d": (k, False, False, cr.ERR_BOUND), "e": (k, False, True, cr.OK)}[kind]
