"""The tie scenes' references held against each other on the CPU (tests/tie_scenes.py): the integer expectation against the
budget guard and the oracle's three matchers, the plain evaluation in T against the oracle, the conditions the D-pairs must meet
to be an adversary at all, and the planar tie scene through the oracle's whole ICP."""
import numpy as np
import pytest

import tie_scenes as ts
from exact_scenes import assert_exact_in_T

BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


@pytest.fixture(scope="module")
def oracles(oracle32, oracle64):
    return {np.dtype(np.float32): oracle32, np.dtype(np.float64): oracle64}


def same(got, want, T, what):
    gi, gd = got
    wi, wd = want
    assert np.array_equal(gi, wi), (what, "ids", int((np.asarray(gi) != np.asarray(wi)).sum()))
    u = BITS[np.dtype(T)]
    assert np.array_equal(np.ascontiguousarray(gd, dtype=T).view(u), np.ascontiguousarray(wd, dtype=T).view(u)), (what, "d2")


@pytest.mark.parametrize("T", ts.TYPES, ids=lambda t: np.dtype(t).name)
def test_every_exact_scene_fits_its_type(T):
    for sc in ts.exact_scenes(T):
        assert_exact_in_T(sc, T)
    # the nudge is the smallest the format allows, found by the guard and not written down: in float32
    # 2^-15, -15, -13, -11, -9 toward a corner and 2^-15, -14, -12, -10, -8 along x at the five heights
    n1 = [ts.plane_scene("N1", h, T).k for h in ts.HEIGHTS]
    n2 = [ts.plane_scene("N2", h, T).k for h in ts.HEIGHTS]
    if T is np.float32:
        assert n1 == [15, 15, 13, 11, 9] and n2 == [15, 14, 12, 10, 8]
    else:
        assert all(23 <= k <= 30 for k in n1 + n2)


def test_the_scenes_tie_where_they_say_and_the_winning_corner_varies():
    pl = ts.plane()
    c4, n1 = ts.knn_scene("C4", 5, np.float32), ts.knn_scene("N1", 2, np.float32)
    d = c4.d2_float()
    assert np.all(d[:, 0] == d[:, 3]) and np.all(d[:, 3] < d[:, 4])            # four tied, then the next shell
    d = n1.d2_float()
    assert np.all(d[:, 0] < d[:, 1])                                           # a unique winner
    n2 = ts.plane_scene("N2", 0, np.float32)
    d = ts.Scene(pl, n2.reading, ts.int_knn(n2.reading, pl.ref, 3)).d2_float()
    assert np.all(d[:, 0] == d[:, 1]) and np.all(d[:, 1] < d[:, 2])            # the two nearer corners tied
    # the map is shuffled: "lowest index" is each of the four corners for about a quarter of the squares
    for sc in (ts.plane_scene("C4", 0, np.float32), ts.plane_scene("N1", 0, np.float32)):
        i, j = ts._squares(pl.L)
        corner = (pl.i[sc.ids] - i).astype(int) * 2 + (pl.j[sc.ids] - j).astype(int)
        share = np.bincount(corner, minlength=4) / sc.n
        assert share.shape == (4,) and np.all(share > 0.15), share
    # the cube centres: eight tied, every corner wins somewhere
    cc = ts.cube_scene("CC8", np.float32)
    assert len(np.unique((ts.cube().ijk[cc.ids] - np.floor(cc.reading / ts.S)).astype(int) @ np.array([4, 2, 1]))) == 8


@pytest.mark.parametrize("T", ts.TYPES, ids=lambda t: np.dtype(t).name)
def test_integer_expectation_equals_the_oracles_three_matchers(oracles, T):
    o = oracles[np.dtype(T)]
    for sc in ts.exact_scenes(T):
        want = (sc.ids, sc.d2_float())
        if sc.knn == 1:
            same(o.knn_brute(sc.reading, sc.ref), want, T, (sc.note, "brute"))
            same(o.knn_kdtree(sc.reading, sc.ref), want, T, (sc.note, "kdtree"))
            # (maxDist 2: at 16 s the query over a lattice point sits AT maxDist^2 and keeps its neighbour, the others have none)
            same(o.knn_brute(sc.reading, sc.ref, 2.0), ts.apply_max_dist(*want, 2.0, T), T, (sc.note, "brute, maxDist 2"))
        else:
            same(o.knn_brute_k(sc.reading, sc.ref, sc.knn), want, T, (sc.note, "brute_k"))


@pytest.mark.parametrize("T", ts.TYPES, ids=lambda t: np.dtype(t).name)
def test_plain_evaluation_equals_the_oracle_on_the_rounded_lattice(oracles, T):
    o = oracles[np.dtype(T)]
    moved = 0
    for r in ts.r_lattice(T):
        ids, d2 = ts.brute_in_T(r.q, r.m, np.inf, 1, T)
        same((ids, d2), o.knn_brute(r.q, r.m), T, r.note)
        same(ts.apply_max_dist(ids, d2, 2.0, T), o.knn_brute(r.q, r.m, 2.0), T, (r.note, "maxDist 2"))
        if r.h is not None:
            assert np.all(ids >= 0) and np.all(ts.apply_max_dist(ids, d2, 2.0, T)[0] >= 0) == (r.h <= 4)
        moved += int((ids != ts.int_knn(np.rint(r.q.astype(np.float64) * 32) / 32, r.m.astype(np.float64))).sum())
    assert moved > 0            # (a few ulps do break ties: the scene is not the exact one again)


@pytest.mark.parametrize("o", ts.OFFSETS)
def test_plain_evaluation_equals_the_oracle_on_the_pairs(oracle64, o):
    d = ts.d_pairs(o)
    ids, d2 = ts.brute_in_T(d.q, d.m, np.inf, 1, np.float64)
    same((ids, d2), oracle64.knn_brute(d.q, d.m), np.float64, d.note)
    same(ts.apply_max_dist(ids, d2, 2.0, np.float64), oracle64.knn_brute(d.q, d.m, 2.0), np.float64, (d.note, "maxDist 2"))
    same(ts.brute_in_T(d.q, d.m, 2.0, 2, np.float64), oracle64.knn_brute_k(d.q, d.m, 2, 2.0), np.float64, (d.note, "knn 2"))


def reversed_share(d):
    """of the queries whose two nearest map points are their own pair: the share whose winner in float32, on the clouds rounded to
    float32, is not the winner in double"""
    i64, _ = ts.brute_in_T(d.q, d.m, np.inf, 2, np.float64)
    i32, d32 = ts.brute_in_T(d.q.astype(np.float32), d.m.astype(np.float32), np.inf, 2, np.float32)
    own = (np.minimum(i64[:, 0], i64[:, 1]) == np.minimum(d.ia, d.ib)) & (np.maximum(i64[:, 0], i64[:, 1]) == np.maximum(d.ia, d.ib))
    return float((i32[own, 0] != i64[own, 0]).mean()), int(own.sum()), d32[:, 0]


@pytest.mark.parametrize("o", ts.OFFSETS)
def test_the_pairs_are_an_adversary_of_a_float_prefilter(o):
    """Conditions, not measurements (a seed that misses them is changed, never the bound).  Reversed share, of the queries whose two
    nearest points are their own pair (3 846 to 3 881 of 4 000): 46.3 % at the origin, 47.7 % at 3 km, 50.4 % at 400 km."""
    d = ts.d_pairs(o)
    share, n_own, fb = reversed_share(d)
    print(f"D-pairs o={o:g}: own pair nearest for {n_own} of {len(d.q)}, float32 winner reversed for {100 * share:.1f} %")
    assert n_own >= len(d.q) // 2 and share >= 0.25
    # the prefilter's error unit as k_match_fast.inc computes it: 2^-22 of the largest coordinate either cloud has
    U = 2.0 ** -22 * max(np.abs(d.q).max(), np.abs(d.m).max())
    below = float((fb < 100 * U * U).mean())
    print(f"D-pairs o={o:g}: U = {U:.3e}, fb below 100 U^2 for {100 * below:.1f} %, below 400 U^2 for {100 * float((fb < 400 * U * U).mean()):.1f} %")
    if o == 3.0e3:
        assert 0.10 <= below <= 0.90
    elif o == 0.0:
        assert below == 0.0                             # the slope branch only
    else:
        assert float((fb < 400 * U * U).mean()) == 1.0  # the floor only


@pytest.mark.parametrize("T", ts.TYPES, ids=lambda t: np.dtype(t).name)
def test_planar_tie_scene_through_the_oracles_icp(oracles, T):
    o = oracles[np.dtype(T)]
    reading, T0, sc = ts.icp_scene()
    # an ICP centres its map: the lattice mean is dyadic and the centred scene is still exact
    cen, mean = ts.centred(sc)
    assert np.array_equal(mean, [23.5 * ts.S, 23.5 * ts.S, 0.0]) and np.array_equal(o.centroid(sc.ref).astype(np.float64), mean)
    assert_exact_in_T(cen, T)
    assert np.array_equal(reading.astype(T).astype(np.float64), reading)
    r = o.icp(reading, sc.ref, sc.nrm, T0, **ts.ICP_CHAIN)
    assert r["status"] == 0 and r["iterations"] == 3 and r["converged"]
    assert np.array_equal(r["T"], T0)
    assert np.array_equal(r["last_ids"], sc.ids)
    assert np.array_equal(r["last_d2"], sc.d2_float().astype(T))
