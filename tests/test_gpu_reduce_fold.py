"""The register fold of a wave's sums (wave_fold in k_minimise.inc) and the staged k_cov_reduce, at the tree's boundaries.

block_reduce_store<NT> folds the NT sums of a wave with lane swaps and DPP moves instead of NT calls of wave_sum; tree RT-1
(oracle/icp_oracle.c) is unchanged, so every sum must keep its bits.  A wrong pairing at any level only
shows on terms whose additions round differently in another association: the inputs here mix magnitudes between ~1e-3 and ~1e3
(per-pair terms over a dozen binades) and non-trivial weights, and the direct test first shows that the oracle itself gives other
bits when the same pairs enter the tree in another order -- inputs without that property would prove nothing.
Sizes: a wave (64), a block (256), a tree block (kReduceSpan = 2048), each minus one, exact and plus one, and two tree blocks
plus one."""
import numpy as np
import pytest

from pgslam_amd import icp

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4097)
BATCH = (2047, 2048, 2049, 513, 65)
CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01,
             smooth_length=3, sensor_std_dev=0.01)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def log_uniform(rng, shape):
    """+-10^U(-3, 3)"""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@pytest.fixture(scope="module")
def scene():
    """Three mutually orthogonal planes through the origin, turned so that no normal is an axis; the in-plane coordinates of the
    points are +-10^U(-3, 3).  Readings: map points moved by a small transform, with noise in proportion to their distance from
    the origin.  Computed once, read only."""
    rng = np.random.default_rng(2020)
    R0 = rotation((1.0, 2.0, 3.0), 0.7)
    m = 6000
    pts = log_uniform(rng, (m, 3))
    plane = rng.integers(0, 3, size=m)
    pts[np.arange(m), plane] = 0.0
    nrm = np.zeros((m, 3))
    nrm[np.arange(m), plane] = 1.0
    ref_xyz, ref_nrm = pts @ R0.T, nrm @ R0.T
    readings, T0 = [], []
    for k, n in enumerate(BATCH):
        pick = rng.choice(m, size=n, replace=False)
        p = ref_xyz[pick]
        p = p + rng.normal(size=p.shape) * (1e-4 + 1e-3 * np.linalg.norm(p, axis=1, keepdims=True))
        T = np.eye(4)
        T[:3, :3] = rotation(rng.normal(size=3), 1e-3 * (1 + k))
        T[:3, 3] = rng.normal(size=3) * 0.03
        readings.append(p)
        T0.append(T)
    # the stage-level pairs: readings of mixed magnitude against arbitrary map points, weights 0, 1 and reals
    n = max(SIZES)
    rd = log_uniform(rng, (n, 3))
    ids = rng.integers(0, m, size=n).astype(np.int32)
    ids[rng.random(n) < 0.03] = -1
    w = rng.choice([0.0, 1.0, -1.0], size=n, p=[0.15, 0.35, 0.5])
    w = np.where(w < 0, rng.uniform(0.01, 3.0, size=n), w)
    return dict(ref_xyz=ref_xyz, ref_nrm=ref_nrm, readings=readings, T0=T0, rd=rd, ids=ids, w=w, perm=rng.permutation(n))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_error_stats_all_sums_at_every_boundary(scene, oracle32, oracle64, dtype):
    """k_error_stats<T, 0> -> block_reduce_store<30> -> k_sum_partials against the oracle's tree: 30 sums, bit for bit"""
    orc = oracle32 if dtype == np.float32 else oracle64
    ref, nrm, rd, w = (scene[k].astype(dtype) for k in ("ref_xyz", "ref_nrm", "rd", "w"))
    ids = scene["ids"]
    ctx = icp.Context(0, **CHAIN)
    mid = ctx.set_map(ref, nrm, center=False, dtype=dtype)
    try:
        for n in SIZES:
            st, want = orc.p2plane_system(rd[:n], ref, nrm, ids[:n], w[:n])
            assert st == 0
            if n >= 65:
                # the inputs have teeth: the oracle's own sums change bits when the pairs enter the tree in another order
                perm = scene["perm"][scene["perm"] < n].astype(np.int32)
                st, other = orc.p2plane_system(rd[:n], ref, nrm, ids[:n], w[:n], order=perm)
                assert st == 0 and not same_bits(other, want), ("inputs without teeth", n)
            ratio, resid, got = ctx.error_stats(mid, rd[:n], ids[:n], w[:n], dtype=dtype)
            assert same_bits(got, want), (np.dtype(dtype).name, n, np.flatnonzero(got != want))
            assert same_bits(resid, want[29]) and same_bits(ratio, want[27] / n), (n, ratio, resid)
    finally:
        ctx.destroy_map(mid)
        ctx.close()


@pytest.mark.parametrize("sum_order", [icp.SUM_ORDER_SORTED, icp.SUM_ORDER_SCAN])
@pytest.mark.parametrize("minimizer", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ragged_batch_whole_icp_bit_for_bit(scene, oracle32, oracle64, dtype, minimizer, sum_order):
    """one batch with readings of 2047, 2048, 2049, 513 and 65 points: every iteration's sums (k_p2plane_reduce, 30) and the
    covariance's (k_cov_reduce, 42) pass through the fold at those boundaries; T, cov, residual, overlap, limit and counts"""
    orc = oracle32 if dtype == np.float32 else oracle64
    chain = dict(CHAIN, error_minimizer=minimizer)
    ref, nrm = scene["ref_xyz"].astype(dtype), scene["ref_nrm"].astype(dtype)
    readings = [r.astype(dtype) for r in scene["readings"]]
    ctx = icp.Context(0, **chain, sum_order=sum_order)
    mid = ctx.set_map(ref, nrm, center=True, dtype=dtype)
    try:
        T, st = ctx.align_batch(mid, readings, scene["T0"], dtype=dtype)
        for p, rd in enumerate(readings):
            order = ctx.reading_order(len(rd), problem=p) if sum_order == icp.SUM_ORDER_SORTED else None
            o = orc.icp(rd, ref, nrm, scene["T0"][p], pair_order=order, **chain)
            what = (np.dtype(dtype).name, minimizer, sum_order, len(rd))
            assert st[p]["status"] == 0 and o["status"] == 0, what
            assert st[p]["iterations"] == o["iterations"] and st[p]["converged"] == o["converged"], what
            assert same_bits(T[p], o["T"]), (what, np.abs(T[p] - o["T"]).max())
            assert same_bits(st[p]["cov"], o["cov"]), (what, "cov")
            assert same_bits(st[p]["residual"], o["residual"]) and same_bits(st[p]["overlap"], o["overlap"]), what
            assert same_bits(st[p]["trim_limit"], o["trim_limit"]), what
            assert st[p]["n_kept"] == o["n_kept"] and st[p]["n_finite"] == o["n_finite"], what
    finally:
        ctx.destroy_map(mid)
        ctx.close()
