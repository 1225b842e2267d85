"""The exact-arithmetic scenes on the CPU (tests/exact_scenes.py): every scene the GPU tests use stays inside the bit budget of
its formats (the guard), and the oracle agrees with the closed forms on each of them -- so a device-versus-closed-form mismatch
in tests/test_gpu_exact_scenes.py is a finding about the device, and a disagreement HERE one about oracle/icp_oracle.c."""
from fractions import Fraction

import numpy as np
import pytest

import exact_scenes as X

DTYPES = [np.float32, np.float64]
CHAIN = dict(max_dist=X.MAX_DIST, trim_ratio=0.85, max_iters=1, min_diff_rot=0.0, min_diff_trans=0.0, smooth_length=3, sensor_std_dev=0.01)


def orc_of(oracle32, oracle64, dtype):
    return oracle32 if dtype == np.float32 else oracle64


def frac_d2(v):
    return Fraction(v, 1 << (2 * X.K))


def distinct(scenes):
    seen, out = set(), []
    for sc in scenes:
        key = (sc.note, sc.reading.tobytes())
        if key not in seen:
            seen.add(key)
            out.append(sc)
    return out


def check_selection(orc, sc, ratio, dtype, icp=True):
    """the oracle's outlier filter and one oracle iteration against expected_limit"""
    d2 = sc.d2_int()
    limit, nf, nk = X.expected_limit(d2, ratio, dtype)
    st, w, o_limit, o_nf = orc.trim_weights(sc.d2_float().astype(dtype), ratio)
    assert st == 0 and o_nf == nf, sc.note
    assert Fraction(float(o_limit)) == frac_d2(limit), (sc.note, ratio)
    assert int(w.sum()) == nk and np.array_equal(w != 0, np.array([v is not None and v <= limit for v in d2])), (sc.note, ratio)
    if icp:
        o = orc.icp(sc.reading.astype(dtype), sc.ref.astype(dtype), sc.nrm.astype(dtype), np.eye(4), center_reference=False,
                    **dict(CHAIN, trim_ratio=ratio))
        assert o["status"] == 0, sc.note
        assert Fraction(o["trim_limit"]) == frac_d2(limit) and o["n_kept"] == nk and o["n_finite"] == nf, (sc.note, ratio)
        assert np.array_equal(o["last_ids"], sc.ids), sc.note
        assert np.array_equal(o["last_d2"].astype(np.float64), sc.d2_float()), sc.note


@pytest.mark.parametrize("kind", X.SELECTION_KINDS)
def test_selection_scenes_guard_and_oracle(oracle32, kind):
    """test A's float32 scenes: the guard, the oracle's filter and one oracle iteration at every ratio, every reading"""
    for ratio in X.RATIOS:
        for sc in distinct(X.selection_batch(kind, ratio, np.float32)):
            X.assert_exact_in_T(sc, np.float32)
            check_selection(oracle32, sc, ratio, np.float32)


def test_selection_ramp_of_distinct_keys_f64(oracle64):
    """test A's float64 ramp: 43 264 distinct exact squares"""
    for ratio in X.RATIOS:
        for sc in distinct(X.selection_batch("ramp", ratio, np.float64)):
            X.assert_exact_in_T(sc, np.float64)
            check_selection(oracle64, sc, ratio, np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(X.BAND_CASES))
def test_band_scenes_guard_and_oracle(oracle32, oracle64, case, dtype):
    """test B's scenes: the designed rank really lies where the case says, relative to the band [h / 4, 4 h] of the hint h = D0^2"""
    orc = orc_of(oracle32, oracle64, dtype)
    batch = X.band_batch(case, dtype)
    for sc in distinct(batch):
        X.assert_exact(sc, dtype, minimizers=(0,))
    sc = batch[0]
    check_selection(orc, sc, X.BAND_RATIO, dtype)
    d2 = sorted(sc.d2_int())
    h = int(X.D0 * X.D0 * 2 ** (2 * X.K))
    lo, hi = h // 4, 4 * h
    k = X.select_rank(len(d2), X.BAND_RATIO, dtype)
    below, inside = sum(v < lo for v in d2), sum(lo <= v <= hi for v in d2)
    assert (not (below <= k < below + inside)) == X.BAND_CASES[case]
    edge = {"rank_on_low_edge": (d2[k] == lo and k == below), "rank_just_below_band": (k == below - 1 and d2[k] < lo),
            "rank_on_high_edge": (d2[k] == hi and k == below + inside - 1), "rank_just_above_band": (k == below + inside and d2[k] > hi)}
    assert edge.get(case, True), case
    # the partial chain over the same reading: ratio and residual
    limit, nf, keep, sums = X.chain_expectation(sc, X.BAND_RATIO, dtype)
    o = orc.partial_chain(sc.reading.astype(dtype), sc.ref.astype(dtype), sc.nrm.astype(dtype), np.eye(4), center_reference=False,
                          **dict(CHAIN, trim_ratio=X.BAND_RATIO))
    assert o["status"] == 0 and o["overlap"] == int(keep.sum()) / sc.n and Fraction(o["residual"]) == sums[29], case


def test_primer_checkerboard_zero_and_stage_scenes(oracle32, oracle64):
    """tests C and D: the guard (with the sums: T must stay the identity exactly), the oracle's b = 0 and limit"""
    scenes = distinct(X.primer_batch() + X.checkerboard_batch() + X.zero_batch(0) + X.zero_batch(2) + X.stage_batch())
    for sc in scenes:
        for dtype in DTYPES:
            X.assert_exact_in_T(sc, dtype)
        X.assert_exact_sums(sc, minimizers=(0,))
        for dtype in DTYPES:
            check_selection(orc_of(oracle32, oracle64, dtype), sc, 0.85, dtype, icp=dtype == np.float32)
    for sc in distinct(X.checkerboard_batch() + X.zero_batch(0)[:1]):
        p, q, n, _ = sc.pairs()
        sums = X.expected_sums(p, q, n, np.ones(sc.n))
        assert all(v == 0 for v in sums[21:27]), sc.note                       # b = 0: the closed form says T stays the identity
        o = oracle32.icp(sc.reading, sc.ref, sc.nrm, np.eye(4), center_reference=False,
                         **dict(CHAIN, max_iters=6))
        assert o["status"] == 0 and o["iterations"] == 6 and np.array_equal(o["T"], np.eye(4)), sc.note
        lim = X.D0 ** 2 if "zero" not in sc.note else 0.0
        assert o["trim_limit"] == lim and o["n_kept"] == sc.n, sc.note
        # a plane with one normal constrains three of six degrees of freedom: H is exactly singular here, and the covariance says
        # "no information" the way the library does (largest double on the diagonal) -- not NaN from a division by a zero pivot
        assert np.array_equal(o["cov"], np.diag([np.finfo(np.float64).max] * 6)), sc.note


def test_launch_arithmetic_of_the_stage_batch():
    """test D's shape: with 256 problems and 43 264 distances in the largest, a block's span is three tiles"""
    tiles = -(-X.BIG_L * X.BIG_L // 2048)
    per_problem = min(tiles, max(1, 2048 // X.STAGE_P))
    assert (tiles, per_problem, -(-tiles // per_problem)) == (22, 8, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_sums_guard_and_oracle(oracle32, oracle64, dtype):
    """test E's stage-level scene: all 30 sums of both minimisers at every pair count, oracle against closed form"""
    orc = orc_of(oracle32, oracle64, dtype)
    sc = X.sums_scene()
    w = X.weights_pattern(sc.n)
    X.assert_exact_in_T(sc, dtype, w=w)
    if dtype == np.float32:
        X.assert_exact_sums(sc, w=w)
    p, q, n, _ = sc.pairs()
    rd, ref, nrm, ids = sc.reading.astype(dtype), sc.ref.astype(dtype), sc.nrm.astype(dtype), sc.ids.astype(np.int32)
    for m in (0, 1):
        want = X.expected_sums(p, q, n, w, minimizer=m, prefixes=list(X.PAIR_SIZES))
        for cnt in X.PAIR_SIZES:
            if m == 0:
                st, got = orc.p2plane_system(rd[:cnt], ref, nrm, ids[:cnt], w[:cnt].astype(dtype))
            else:
                st, got = orc.p2point_system(rd[:cnt], ref, ids[:cnt], w[:cnt].astype(dtype))
            assert got.tobytes() == X.to_floats(want[cnt]).tobytes(), (m, cnt)


@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_scenes_guard_and_oracle(oracle32, oracle64, dtype):
    """test E's whole-chain scenes (one neighbour, three neighbours): the oracle's partial chain against the closed form"""
    orc = orc_of(oracle32, oracle64, dtype)
    for sizes, make, knn in ((X.PAIR_SIZES, X.chain_scene, 1), (X.KNN3_SIZES, X.knn3_scene, 3)):
        for cnt in sizes:
            sc = make(cnt)
            X.assert_exact_in_T(sc, dtype)
            if dtype == np.float32 and cnt == sizes[-1]:
                X.assert_exact_sums(sc, minimizers=(0,))                     # (the smaller scenes are prefixes of the largest)
            limit, nf, keep, sums = X.chain_expectation(sc, X.CHAIN_RATIO, dtype)
            o = orc.partial_chain(sc.reading.astype(dtype), sc.ref.astype(dtype), sc.nrm.astype(dtype), np.eye(4), center_reference=False,
                                  **dict(CHAIN, trim_ratio=X.CHAIN_RATIO, knn=knn))
            if nf == 0:
                assert o["status"] != 0, (knn, cnt)
                continue
            assert o["status"] == 0 and np.array_equal(o["ids"], sc.ids), (knn, cnt)
            assert np.array_equal(o["d2"].astype(np.float64), sc.d2_float()), (knn, cnt)
            assert o["overlap"] == int(keep.sum()) / (sc.n * knn) and Fraction(o["residual"]) == sums[29], (knn, cnt)


def test_angle_scenes_guard_and_oracle(oracle32):
    """test E's scene with a SurfaceNormalOutlierFilter: the reading's normals lie clearly inside or clearly outside the angle"""
    for cnt in (65, 2049, 18433):
        sc = X.angle_scene(cnt)
        X.assert_exact(sc, np.float32, minimizers=(0,))
        a = sc.reading_nrm / np.linalg.norm(sc.reading_nrm, axis=1, keepdims=True)
        b = np.asarray(X.NORMAL_SUM) / np.linalg.norm(X.NORMAL_SUM)
        cosine = a @ b
        assert np.all((cosine > 0.99) == sc.angle_inside) and np.all((cosine > 0.99) | (cosine < 0.5))
        assert 0.5 < np.cos(X.NORMAL_MAX_ANGLE) < 0.99
        limit, nf, keep, sums = X.chain_expectation(sc, X.CHAIN_RATIO, np.float32, extra_keep=sc.angle_inside)
        o = oracle32.icp(sc.reading, sc.ref, sc.nrm, np.eye(4), reading_nrm=sc.reading_nrm, center_reference=False,
                         **dict(CHAIN, trim_ratio=X.CHAIN_RATIO, normal_max_angle=X.NORMAL_MAX_ANGLE))
        assert o["status"] == 0 and o["n_kept"] == int(keep.sum()) and o["n_finite"] == nf, cnt
        assert o["overlap"] == int(keep.sum()) / cnt and Fraction(o["residual"]) == sums[29], cnt
