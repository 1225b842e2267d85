"""The plain reference of the transformation checkers (tests/checkers_ref.py: written from the definition, unbounded history,
rotation distances from the matrices) against the two routines that restate each other almost line for line:
  * the oracle's orc_checker_check (64 history entries, ORC_HIST), and
  * the product's checker_check of pgslam_amd/csrc/icp_math.hpp (16 entries, kHist; what k_solve_update runs for every problem),
    compiled here for the host (tests/cpp/checker_host.cpp).
Random rigid trajectories with geometrically shrinking steps, up to 80 iterations long -- past both capacities --, every
smoothLength of the grid, the Bound checker off, with either limit alone and with both.  The flags of all three must be equal
at every step.  Every limit follows the margin rule (the geometric mean of two adjacent values of the series it is compared
with), so no decision is closer than half a percent to a double and nothing is skipped.  No GPU is involved."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import checkers_ref as cr
import iteration_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pgslam_amd", "csrc")
SMOOTH = (1, 2, 3, 7, 15)
BOUNDS = ("off", "rot", "trans", "both")
LENGTH = 80


class ProductChecker:
    """checker_check of an icp_math.hpp, compiled for the host"""

    def __init__(self, out_dir, csrc=CSRC):
        lib = os.path.join(str(out_dir), "libchecker_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I" + csrc,
                               os.path.join(ROOT, "tests", "cpp", "checker_host.cpp"), "-o", lib])
        self.lib = C.CDLL(lib)
        self.size, self.hist = self.lib.pgicp_host_checker_size(), self.lib.pgicp_host_checker_hist()

    def start(self):
        state = C.create_string_buffer(self.size)
        self.lib.pgicp_host_checker_init(state)
        return state

    def check(self, state, T, max_iters, min_rot, min_trans, smooth, bound_rot=0.0, bound_trans=0.0):
        T = np.ascontiguousarray(T, dtype=np.float64)
        return self.lib.pgicp_host_checker_check(state, T.ctypes.data_as(C.c_void_p), C.c_int(max_iters), C.c_double(min_rot), C.c_double(min_trans),
                                                 C.c_int(smooth), C.c_double(bound_rot), C.c_double(bound_trans))

    def run(self, T_iters, max_iters, min_rot, min_trans, smooth, bound_rot=0.0, bound_trans=0.0):
        """the loop of k_solve_update around it: (iterations, converged, max_iter_reached, status)"""
        state = self.start()
        for k, T in enumerate(T_iters, start=1):
            f = self.check(state, T, max_iters, min_rot, min_trans, smooth, bound_rot, bound_trans)
            if f & 8:
                return k, False, False, cr.ERR_NAN
            if f & 16:
                return k, False, False, cr.ERR_BOUND
            if not f & 1:
                return k, bool(f & 2), bool(f & 4), cr.OK
        raise ValueError("the trajectory ends before the checkers stop the loop")


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    p = ProductChecker(tmp_path_factory.mktemp("checker_host"))
    assert p.hist == 16
    return p


def flags_of(events):
    """checkers_ref.check's set as the flag word of the two C routines: bit0 go on, bit1 Differential, bit2 Counter, 8 NaN, 16 Bound"""
    if "nan" in events:
        return 8
    if "bound" in events:
        return 16
    return (2 if "differential" in events else 0) | (4 if "counter" in events else 0) | (0 if events else 1)


def rodrigues(axis, angle):
    x, y, z = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def random_trajectory(seed, length=LENGTH):
    """T_1 .. T_length: step k turns by a0 rho^k about an axis that wobbles around a fixed one and moves by b0 rho^k along a
    direction that does the same, so the steps shrink geometrically and the distance from the identity grows"""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.86, 0.95)
    a0, b0 = rng.uniform(0.02, 0.08), rng.uniform(0.1, 0.5)
    axis0, dir0 = rng.normal(size=3), rng.normal(size=3)
    axis0, dir0 = axis0 / np.linalg.norm(axis0), dir0 / np.linalg.norm(dir0)
    R, t, out = np.eye(3), np.zeros(3), []
    for k in range(1, length + 1):
        R = rodrigues(axis0 + 0.1 * rng.normal(size=3), a0 * rho ** k) @ R
        d = dir0 + 0.1 * rng.normal(size=3)
        t = t + b0 * rho ** k * d / np.linalg.norm(d)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        out.append(T)
    return out


def limits(T, smooth, stop, bounds, bound_at):
    """min_rot, min_trans to stop at `stop`; the Bound's limits to be passed at `bound_at`: all by the margin rule"""
    ser, b = cr.smoothed_series(T, smooth), cr.bound_series(T)
    min_rot, min_trans = cr.between(ser[stop - 1][0], ser[stop][0]), cr.between(ser[stop - 1][1], ser[stop][1])
    bound_rot = cr.between(b[bound_at - 1][0], b[bound_at][0]) if bounds in ("rot", "both") else 0.0
    bound_trans = cr.between(b[bound_at][1], b[bound_at + 1][1]) if bounds == "both" else cr.between(b[bound_at - 1][1], b[bound_at][1]) if bounds == "trans" else 0.0
    return min_rot, min_trans, bound_rot, bound_trans


def walk_all_three(oracle, product, T, max_iters, min_rot, min_trans, smooth, bound_rot, bound_trans):
    """feeds the whole trajectory to the three checkers (past their stops: each is a state machine) and returns the first step
    at which their flag words differ, with the three words -- or None"""
    assert cr.margin(T, len(T), min_rot, min_trans, smooth, bound_rot, bound_trans) >= 0.004
    oc = oracle.checker(max_iters, min_rot, min_trans, smooth)
    oracle.checker_set_bound(oc, bound_rot, bound_trans)
    pc = product.start()
    hist = [np.eye(4)]
    for k, Tk in enumerate(T, start=1):
        hist.append(Tk)
        want = flags_of(cr.check(hist, k, max_iters, min_rot, min_trans, smooth, bound_rot, bound_trans))
        got = (oracle.checker_check(oc, Tk), product.check(pc, Tk, max_iters, min_rot, min_trans, smooth, bound_rot, bound_trans))
        if got != (want, want):
            return k, want, got
    return None


@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("smooth", SMOOTH)
def test_reference_oracle_and_product_checkers_agree_at_every_step(oracle32, product, smooth, bounds):
    """stops before the product's shift (16 entries), between the two capacities and past the oracle's (64); the Counter three
    steps before the end, or on the very iteration of the Differential stop"""
    for seed in range(3):
        T = random_trajectory(1000 * smooth + seed)
        for stop in (smooth + 1, 17 + seed, 40, 66 + seed, 75):
            for max_iters in (LENGTH - 3, stop):
                for bound_at in (3, 9 + seed):
                    lim = limits(T, smooth, stop, bounds, bound_at)
                    bad = walk_all_three(oracle32, product, T, max_iters, lim[0], lim[1], smooth, lim[2], lim[3])
                    assert bad is None, (seed, stop, max_iters, bound_at, bad)
                    if bounds == "off":
                        break


def test_the_three_outcomes_by_hand(oracle32, product):
    """the order and the exits, on a trajectory short enough to follow: 5 equal steps of 0.01 rad / 0.1 m, then 5 of a tenth"""
    T, ang, x = [], 0.0, 0.0
    for k in range(10):
        ang, x = ang + (0.01 if k < 5 else 0.001), x + (0.1 if k < 5 else 0.01)
        M = np.eye(4)
        M[:3, :3], M[0, 3] = rodrigues(np.array([0.0, 0.0, 1.0]), ang), x
        T.append(M)
    ser = cr.smoothed_series(T, 2)
    assert ser[5] == pytest.approx((0.01, 0.1)) and ser[6] == pytest.approx((0.0055, 0.055)) and ser[7] == pytest.approx((0.001, 0.01))
    assert cr.bound_series(T)[4] == pytest.approx((0.04, 0.4))
    assert cr.run(T, 10, 0.002, 0.02, 2) == (7, True, False, cr.OK)              # Differential alone, once both means are below
    assert cr.run(T, 10, 0.002, 0.06, 2) == (7, True, False, cr.OK)              # (the translation was below at 6: the rotation was not)
    assert cr.run(T, 10, 0.0, 0.0, 2) == (10, False, True, cr.OK)                # Counter alone
    assert cr.run(T, 7, 0.002, 0.02, 2) == (7, True, True, cr.OK)                # both on the same iteration
    assert cr.run(T, 10, 0.0, 0.0, 2, bound_rot=0.035) == (4, False, False, cr.ERR_BOUND)      # rotation limit alone
    assert cr.run(T, 10, 0.0, 0.0, 2, bound_trans=0.25) == (3, False, False, cr.ERR_BOUND)     # translation limit alone
    assert cr.run(T, 10, 0.0, 0.0, 2, 0.035, 0.45) == (4, False, False, cr.ERR_BOUND)
    assert cr.run(T, 4, 0.0, 0.0, 2, 0.035, 0.45) == (4, False, True, cr.OK)     # the Counter's stop leaves before the Bound is looked at
    assert cr.run(T, 10, 0.002, 0.02, 2, bound_rot=0.0515) == (7, False, False, cr.ERR_BOUND)  # ... a Differential stop does not
    for args in ((10, 0.002, 0.02, 2, 0.0, 0.0), (7, 0.002, 0.02, 2, 0.0, 0.0), (4, 0.0, 0.0, 2, 0.035, 0.45), (10, 0.0, 0.0, 2, 0.035, 0.0),
                 (10, 0.0, 0.0, 2, 0.0, 0.25), (10, 0.002, 0.02, 2, 0.0515, 0.0)):
        assert walk_all_three(oracle32, product, T, *args) is None, args


@pytest.mark.parametrize("smooth", (1, 3, 15))
def test_nan_is_an_error_while_it_is_in_the_window(oracle32, product, smooth):
    T = random_trajectory(77, 40)
    T[19] = T[19].copy()
    T[19][1, 3] = math.nan                        # iteration 20: in the last `smooth` steps for iterations 20 .. 20 + smooth
    oc, pc, hist = oracle32.checker(100, 0.0, 0.0, smooth), product.start(), [np.eye(4)]
    for k, Tk in enumerate(T, start=1):
        hist.append(Tk)
        want = 8 if 20 <= k <= 20 + smooth else 1
        assert flags_of(cr.check(hist, k, 100, 0.0, 0.0, smooth)) == want, k
        assert oracle32.checker_check(oc, Tk) == want and product.check(pc, Tk, 100, 0.0, 0.0, smooth) == want, k
    assert cr.run(T, 100, 0.0, 0.0, smooth) == (20, False, False, cr.ERR_NAN)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_device_cases_on_the_host(oracle32, oracle64, product, dtype):
    """every case of tests/test_gpu_iteration_control.py before a GPU is involved: the trajectory moves as the cases need, the
    plain reference gives what each case was built to show, at the margin the rule promises, and the product's checker
    (host-compiled) and the whole oracle ICP give the same"""
    orc = oracle32 if dtype == np.float32 else oracle64
    sc = ic.scene(oracle64)
    trace, T_out = ic.trajectory(orc, dtype, sc)
    ic.assert_moves_through_20(trace)
    rd, ref, nrm, T_init = sc
    for case in ic.CASES:
        p = ic.settings(case, trace)
        want, margin = ic.expected(case, trace)
        assert want == ic.foreseen(case), (case, want)
        assert margin >= 0.0049, (case, margin)
        assert product.run(trace, p["max_iters"], p["min_diff_rot"], p["min_diff_trans"], p["smooth_length"], p["bound_max_rot"],
                           p["bound_max_trans"]) == want, case
        o = orc.icp(rd.astype(dtype), ref.astype(dtype), nrm.astype(dtype), T_init, center_reference=False, **dict(ic.BASE, **p))
        assert (o["iterations"], o["converged"], o["max_iter_reached"], o["status"]) == want, case
        if want[3] == cr.OK:
            assert o["T"].tobytes() == T_out[want[0] - 1].tobytes(), case


MUTATIONS = {
    # the smoothed mean over one step too many
    "mean_over_smooth_plus_1": ("rsum /= (double)smooth;\n        tsum /= (double)smooth;",
                                "rsum /= (double)(smooth + 1);\n        tsum /= (double)(smooth + 1);"),
    # the full history moved down by two entries instead of one
    "history_shift_by_two": ("for (int i = 1; i < kHist; i++) {\n            for (int j = 0; j < 4; j++) c.quat[i - 1][j] = c.quat[i][j];\n"
                             "            for (int j = 0; j < 3; j++) c.trans[i - 1][j] = c.trans[i][j];",
                             "for (int i = 2; i < kHist; i++) {\n            for (int j = 0; j < 4; j++) c.quat[i - 2][j] = c.quat[i][j];\n"
                             "            for (int j = 0; j < 3; j++) c.trans[i - 2][j] = c.trans[i][j];"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_a_wrong_checker_is_caught(oracle32, oracle64, tmp_path, name):
    """the checks above are worth something: checker_check with the smoothed mean divided by smoothLength + 1, or with its full
    history shifted by two, compiled for the host from an edited copy of icp_math.hpp, fails them (and the device cases)"""
    old, new = MUTATIONS[name]
    src = open(os.path.join(CSRC, "icp_math.hpp")).read()
    assert src.count(old) == 1, "icp_math.hpp changed: restate the mutation"
    with open(os.path.join(str(tmp_path), "icp_math.hpp"), "w") as f:
        f.write(src.replace(old, new))
    mutant = ProductChecker(tmp_path, csrc=str(tmp_path))
    T = random_trajectory(3000)
    caught = 0
    for smooth in SMOOTH:
        for stop in (smooth + 1, 17, 40):
            lim = limits(T, smooth, stop, "off", 3)
            caught += walk_all_three(oracle32, mutant, T, LENGTH - 3, lim[0], lim[1], smooth, 0.0, 0.0) is not None
    # (smoothLength 1, 2, 3 scale the mean by 1/2, 2/3, 3/4, far below the limit's sqrt(rho) >= 0.92 of the value before the stop: 9 walks;
    #  a shift by two doubles the newest step of every window after the 16th check: at least smoothLength 1's three walks and one more each)
    assert caught >= (9 if name == "mean_over_smooth_plus_1" else 5), caught
    trace, _ = ic.trajectory(oracle32, np.float32, ic.scene(oracle64))
    wrong = []
    for case in ic.CASES:
        p = ic.settings(case, trace)
        got = mutant.run(trace, p["max_iters"], p["min_diff_rot"], p["min_diff_trans"], p["smooth_length"], p["bound_max_rot"], p["bound_max_trans"])
        if got != ic.foreseen(case):
            wrong.append(case)
    kinds = {c[0] for c in wrong}
    assert "a" in kinds and "c" in kinds, wrong
    if name == "mean_over_smooth_plus_1":
        assert any(c[0] == "a" and c[2] < 16 for c in wrong) and any(c[0] == "a" and c[2] > 16 for c in wrong), wrong     # on both sides of the shift
    else:
        assert all(c[2] >= 16 for c in wrong), wrong                            # nothing before the first shift is touched
