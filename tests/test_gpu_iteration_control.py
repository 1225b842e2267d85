"""The device's iteration control -- k_solve_update with checker_check and its 16-entry history, k_compact_active,
single_bookkeeping and the host loop around them (check_every, the matcher pass enqueued ahead of a single problem's next
iteration, wait_iteration_flag) -- away from smoothLength 3 and 300 problems.

The trajectory, the cases and the margin rule are in tests/iteration_cases.py (tests/test_checkers_ref_host.py walks the same
cases on the CPU).  Every case is asserted three ways: (status, iterations, converged, max_iter_reached) against the plain
reference tests/checkers_ref.py on the trajectory; T, bit for bit, against the trajectory's entry of that iteration; the whole
result against oracle.icp with test_gpu_bit_exact.py's check.  Then the same case as a batch of three copies and with
check_every 2 and 7: the bytes of the single run.

Large batches: 1024, 1025 and 2049 problems in one call (k_compact_active places them 1024 at a time and carries two counts
from chunk to chunk), sum_order = SCAN, every problem against oracle.icp of that problem alone, bit for bit."""
import numpy as np
import pytest

import checkers_ref as cr
import iteration_cases as ic
from pgslam_amd import icp, synth
from test_gpu_bit_exact import check, same_bits

pytestmark = pytest.mark.gpu

RESET = dict(knn=1, error_minimizer=0, normal_max_angle=0.0, outlier_max_dist=0.0, quantile_scale=1.0, robust_fct=0, robust_tuning=1.0,
             robust_scale=1, robust_approx=0.0, bound_max_rot=0.0, bound_max_trans=0.0, check_every=1)
STATUS = {cr.OK: icp.OK, cr.ERR_NAN: icp.ERR_NAN, cr.ERR_BOUND: icp.ERR_BOUND}


def result_bytes(T, st):
    """everything a problem returns, as bytes"""
    return (np.asarray(T, dtype=np.float64).tobytes(), st["status"], st["iterations"], st["converged"], st["max_iter_reached"], st["n_kept"], st["n_finite"],
            np.array([st["overlap"], st["residual"], st["trim_limit"]]).tobytes(), np.asarray(st["cov"], dtype=np.float64).tobytes())


class Rig:
    """one context, the scene's map (not centred) in one precision, the oracle's trajectory"""

    def __init__(self, dtype, orc, oracle64):
        self.dtype, self.orc = dtype, orc
        self.sc = ic.scene(oracle64)
        rd, ref, nrm, self.T_init = self.sc
        self.rd, self.ref, self.nrm = rd.astype(dtype), ref.astype(dtype), nrm.astype(dtype)
        self.trace, self.T_out = ic.trajectory(orc, dtype, self.sc)
        ic.assert_moves_through_20(self.trace)
        self.ctx = icp.Context(0, **dict(RESET, **ic.BASE), sum_order=icp.SUM_ORDER_SCAN)
        self.mid = self.ctx.set_map(self.ref, self.nrm, center=False, dtype=dtype)

    def single(self, **params):
        self.ctx.set_params(**params)
        T, st = self.ctx.align_batch(self.mid, [self.rd], [self.T_init], dtype=self.dtype, raise_on_error=False)
        return T[0], st[0]

    def close(self):
        self.ctx.destroy_map(self.mid)
        self.ctx.close()


@pytest.fixture(scope="module", params=[np.float32, np.float64], ids=["float32", "float64"])
def rig(request, oracle32, oracle64):
    r = Rig(request.param, oracle32 if request.param == np.float32 else oracle64, oracle64)
    yield r
    r.close()


def test_the_device_walks_the_oracles_trajectory(rig):
    """min_diff = 0, max_iters = K for K = 1 .. 24: the device's T after K iterations is T_iter(K) T_init of the oracle's
    trace, bit for bit (the map is not centred: api_icp.inc forms T_out = T_ref (T_iter T_pre) with T_ref = I, T_pre = T_init)"""
    for K in range(1, ic.K_TRAJ + 1):
        T, st = rig.single(**dict(ic.FREE, max_iters=K, check_every=1))
        assert (st["status"], st["iterations"], st["converged"], st["max_iter_reached"]) == (icp.OK, K, False, True), K
        assert same_bits(T, rig.T_out[K - 1]), (K, np.abs(T - rig.T_out[K - 1]).max())


@pytest.mark.parametrize("case", ic.CASES, ids=ic.case_id)
def test_case(rig, case):
    p = ic.settings(case, rig.trace)
    want, margin = ic.expected(case, rig.trace)
    assert want == ic.foreseen(case) and margin >= 0.0049, (want, margin)
    k, converged, max_iter_reached, status = want
    T, st = rig.single(**dict(p, check_every=1))
    # 1. the plain reference on the trajectory
    assert (st["status"], st["iterations"], st["converged"], st["max_iter_reached"]) == (STATUS[status], k, converged, max_iter_reached)
    # 2. T is the trajectory's entry of that iteration (an error returns the identity)
    assert same_bits(T, rig.T_out[k - 1] if status == cr.OK else np.eye(4)), np.abs(T - rig.T_out[k - 1]).max()
    # 3. the whole result against the oracle's ICP
    o = rig.orc.icp(rig.rd, rig.ref, rig.nrm, rig.T_init, center_reference=False, **dict(ic.BASE, **p))
    if status == cr.OK:
        check(st, T, o, case)
        assert st["max_iter_reached"] == o["max_iter_reached"]
    else:
        assert (o["status"], o["iterations"]) == (7, k) and same_bits(o["T"], np.eye(4))
        with pytest.raises(icp.ConvergenceError) as e:                 # (the single-problem entry point raises it)
            rig.ctx.align(rig.mid, rig.rd, rig.T_init, dtype=rig.dtype)
        assert e.value.code == icp.ERR_BOUND
    # f. three copies in one batch, and the host looking at the flag every 2nd / 7th iteration only: the same bytes
    ref_bytes = result_bytes(T, st)
    T3, st3 = rig.ctx.align_batch(rig.mid, [rig.rd] * 3, [rig.T_init] * 3, dtype=rig.dtype, raise_on_error=False)
    for c in range(3):
        assert result_bytes(T3[c], st3[c]) == ref_bytes, ("batch of 3", c)
    for every in (2, 7):
        Te, ste = rig.single(check_every=every)
        assert result_bytes(Te, ste) == ref_bytes, ("check_every", every)


# ---- large batches ------------------------------------------------------------------------------------------------------
BIG_CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
BIG_P = 2049
BOUND_TRANS = 0.5


class Big:
    """2049 small problems against one map of 2000 points; the batches of 1024 and 1025 are its first problems.  Readings of 64
    to 200 points, every k-th point of the scan (a reading that covers the scene, not one arc of it); the start errors graded from
    a twentieth of synth.perturbation to one and a half times it, so that the problems finish after different numbers of
    iterations; every 97th reading 500 m away from the map: no pair within maxDist, NO_MATCH."""

    def __init__(self, orc):
        s = synth.make_two_scans(2000, rings=16)
        self.ref, self.nrm = s["ref_xyz"], s["ref_nrm"]
        rng = np.random.default_rng(2049)
        self.readings, self.T0 = [], []
        for p in range(BIG_P):
            n = int(rng.integers(64, 201))
            start = int(rng.integers(0, 2000 - (2000 // n) * (n - 1)))
            rd = np.ascontiguousarray(s["reading_xyz"][start::2000 // n][:n])
            assert len(rd) == n
            if p % 97 == 96:
                rd = rd + np.array([500.0, 0.0, 0.0], dtype=rd.dtype)
            g = 0.05 + 1.45 * (p % 29) / 28.0
            P = synth.perturbation(p)
            D = np.eye(4)
            D[:3, :3] = cr_rotation_power(P[:3, :3], g)
            D[:3, 3] = g * P[:3, 3]
            self.readings.append(rd)
            self.T0.append(s["T_init"] @ D)
        m = orc.map_create(self.ref, self.nrm, center=True)
        self.want = [orc.icp_map(m, self.readings[p], self.T0[p], **BIG_CHAIN) for p in range(BIG_P)]
        self.want_bound = [orc.icp_map(m, self.readings[p], self.T0[p], **dict(BIG_CHAIN, bound_max_trans=BOUND_TRANS)) for p in range(1025)]
        orc.map_free(m)


def cr_rotation_power(R, g):
    """R^g: the same axis, g times the angle"""
    ang = cr.rotation_angle(R, np.eye(3))
    if ang == 0.0:
        return np.eye(3)
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    x, y, z = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(g * ang) * K + (1.0 - np.cos(g * ang)) * (K @ K)


@pytest.fixture(scope="module")
def big(oracle32):
    b = Big(oracle32)
    # what the batches are for, checked on the CPU: several iteration counts, NO_MATCH among them, BOUND / OK / NO_MATCH mixed
    for P in (1024, 1025, BIG_P):
        ok = [w for w in b.want[:P] if w["status"] == 0]
        assert len({w["iterations"] for w in ok}) >= 5, sorted({w["iterations"] for w in ok})
        assert all(b.want[p]["status"] == 1 for p in range(96, P, 97)) and len(ok) == P - len(range(96, P, 97))
    kinds = [w["status"] for w in b.want_bound]
    assert kinds.count(0) >= 100 and kinds.count(7) >= 100 and kinds.count(1) == len(range(96, 1025, 97))
    return b


@pytest.fixture(scope="module")
def big_ctx():
    ctx = icp.Context(0, **dict(RESET, **BIG_CHAIN), sum_order=icp.SUM_ORDER_SCAN)
    yield ctx
    ctx.close()


def assert_problem(T, st, o, what):
    assert st["status"] == o["status"] and st["iterations"] == o["iterations"], (what, st["status"], o["status"], st["iterations"], o["iterations"])
    assert st["converged"] == o["converged"] and st["max_iter_reached"] == o["max_iter_reached"], what
    if o["status"] == 0:
        check(st, T, o, what)
    else:
        assert same_bits(T, np.eye(4)), what


def problems_that_differ(T, st, want):
    """every problem is compared (the first that differs does not hide the rest, nor the checks that follow): [(problem, what)]"""
    differ = []
    for p, o in enumerate(want):
        try:
            assert_problem(T[p], st[p], o, p)
        except AssertionError as e:
            differ.append((p, str(e).splitlines()[0]))
    return differ


@pytest.mark.parametrize("P", [1024, 1025, BIG_P])
def test_large_batch_every_problem_as_alone(big, big_ctx, P):
    """(Problem 783 -- 65 points, stopped by the Counter at 30 iterations while it still moves -- is the one that showed that the
    covariance's small-angle parameters, taken from asin / atan2 / cos of two math libraries, need not be the same doubles:
    icp_math.hpp's small_angles, tests/test_small_angles_host.py.)"""
    ctx = big_ctx
    ctx.set_params(**dict(RESET, **BIG_CHAIN))
    mid = ctx.set_map(big.ref, big.nrm, center=True)
    T, st = ctx.align_batch(mid, big.readings[:P], big.T0[:P], raise_on_error=False)
    differ = problems_that_differ(T, st, big.want[:P])
    # the problems around the chunk boundaries of k_compact_active, each as a device batch of one
    for p in (1023, 1024, 1025, 2047, 2048):
        if p < P:
            T1, st1 = ctx.align_batch(mid, [big.readings[p]], [big.T0[p]], raise_on_error=False)
            assert result_bytes(T1[0], st1[0]) == result_bytes(T[p], st[p]), (P, p)
    if P == 1025:
        ctx.set_params(check_every=3)
        Te, ste = ctx.align_batch(mid, big.readings[:P], big.T0[:P], raise_on_error=False)
        for p in range(P):
            assert result_bytes(Te[p], ste[p]) == result_bytes(T[p], st[p]), ("check_every 3", p)
    ctx.destroy_map(mid)
    assert not differ, differ


def test_large_batch_with_bound_ok_and_no_match_mixed(big, big_ctx):
    """720 OK, 295 BOUND and 10 NO_MATCH problems in the one batch (the fixture checks the mix on the CPU)"""
    ctx = big_ctx
    ctx.set_params(**dict(RESET, **BIG_CHAIN, bound_max_trans=BOUND_TRANS))
    mid = ctx.set_map(big.ref, big.nrm, center=True)
    T, st = ctx.align_batch(mid, big.readings[:1025], big.T0[:1025], raise_on_error=False)
    differ = problems_that_differ(T, st, big.want_bound)
    assert {s["status"] for s in st} == {icp.OK, icp.ERR_NO_MATCH, icp.ERR_BOUND}
    ctx.destroy_map(mid)
    ctx.set_params(**dict(RESET, **BIG_CHAIN))
    assert not differ, differ
