"""The matchers' (distance, index) order on scenes that consist of nothing but ties and near-ties (tests/tie_scenes.py): every
query of every scene, ids equal and squared distances bit for bit.  The expectations are integer arithmetic (exact scenes) or the
contract's arithmetic evaluated elementwise in T by numpy (rounded scenes); tests/test_tie_scenes_host.py holds both against the
oracle on the CPU.  Maps are not centred and T is the identity unless a test says otherwise."""
import numpy as np
import pytest

import tie_scenes as ts
from pgslam_amd import icp

pytestmark = pytest.mark.gpu

INF = float("inf")
BASE = dict(ts.ICP_CHAIN, trim_ratio=0.85, knn=1)     # the matcher calls
ALIGN = dict(ts.ICP_CHAIN, knn=1)                       # the ICP scene: trim_ratio 1
BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
TYPE_IDS = dict(ids=lambda t: np.dtype(t).name)


@pytest.fixture(scope="module")
def ctx():
    c = icp.Context(0, **BASE)
    yield c
    c.close()


def same(got, want, T, what, parts=None):
    """ids equal and d2 bit for bit, for every query; the message names the scene's first part that differs"""
    u = BITS[np.dtype(T)]
    gi, gd = got
    wi, wd = np.asarray(want[0]), np.ascontiguousarray(want[1], dtype=T)
    assert gi.shape == wi.shape and gd.dtype == np.dtype(T)
    bad = (gi != wi) | (gd.view(u) != wd.view(u))
    if bad.any():
        for note, sl in parts or [(what, slice(None))]:
            if bad[sl].any():
                k = int(np.flatnonzero(bad[sl].reshape(bad[sl].shape[0], -1).any(axis=1))[0])
                pytest.fail(f"{what} / {note}: {int(bad[sl].sum())} entries differ; first at query {k}: got {gi[sl][k]} {gd[sl][k]}, "
                            f"expected {wi[sl][k]} {wd[sl][k]}")


def match(ctx, mid, q, T, max_dist=INF, matcher=icp.MATCHER_GRID, knn=1):
    ctx.set_params(**dict(BASE, max_dist=max_dist, matcher=matcher, knn=knn))
    return ctx.match(mid, np.ascontiguousarray(q, dtype=T), dtype=T)


def check_scene(ctx, mid, sc, T, matchers, max_dists):
    want = (sc.ids, sc.d2_float().astype(T))
    for md in max_dists:
        w = want if md == INF else ts.apply_max_dist(*want, md, T)
        for matcher in matchers:
            same(match(ctx, mid, sc.reading, T, md, matcher, sc.knn), w, T, (sc.note, "maxDist", md, "matcher", matcher), getattr(sc, "parts", None))
    return want


BOTH = (icp.MATCHER_GRID, icp.MATCHER_BRUTE)


@pytest.mark.parametrize("T", ts.TYPES, **TYPE_IDS)
def test_exact_plane(ctx, T):
    """P48: every square's centre (4 tied), edge midpoint (2), the centre nudged toward a corner (unique, by the smallest exact
    margin) and along x (2), and the corner itself, at heights 0, s, 4 s, 16 s, 64 s; grid and brute matcher.  maxDist 2 on the
    layers up to 16 s -- at 16 s the query over a lattice point sits AT maxDist^2 = 4 and keeps it, every other one has none."""
    mid = ctx.set_map(ts.plane().ref.astype(T), None, center=False, dtype=T)
    for h in ts.HEIGHTS:
        sc = ts.plane_layer(h, T)
        want = check_scene(ctx, mid, sc, T, BOTH, (INF,) if h > 16 else (INF, 2.0))
        if h == 16:
            ids2, d2 = ts.apply_max_dist(*want, 2.0, T)
            v0 = dict(sc.parts)[ts.plane_scene("V0", h, T).note]
            assert np.all(ids2[v0] >= 0) and np.all(d2[v0] == 4.0) and int((ids2 >= 0).sum()) == v0.stop - v0.start
    ctx.destroy_map(mid)


@pytest.mark.parametrize("T", ts.TYPES, **TYPE_IDS)
def test_exact_cube(ctx, T):
    """C16: cube centres (8 tied, across two z rows), face centres (4) and edge midpoints (2) of every orientation, the cube centre
    nudged toward a corner (unique) and along an axis (4)"""
    mid = ctx.set_map(ts.cube().ref.astype(T), None, center=False, dtype=T)
    check_scene(ctx, mid, ts.cube_all(T), T, BOTH, (INF, 2.0))
    ctx.destroy_map(mid)


@pytest.mark.parametrize("T", ts.TYPES, **TYPE_IDS)
def test_exact_knn_lists(ctx, T):
    """knn 2, 4, 5, 9, 16 around a square's centre, where the shells hold 4, 8, 4 equidistant points: 4 and 16 end on a shell's
    edge, 2, 5 and 9 cut a shell and take its lowest indices; and the same with the centre nudged toward a corner"""
    mid = ctx.set_map(ts.plane().ref.astype(T), None, center=False, dtype=T)
    for kind in ts.KNN_KINDS:
        for knn in ts.KNNS:
            check_scene(ctx, mid, ts.knn_scene(kind, knn, T), T, (icp.MATCHER_GRID,), (INF,))
    ctx.destroy_map(mid)


@pytest.mark.parametrize("T", ts.TYPES, **TYPE_IDS)
def test_rounded_lattice(ctx, T):
    """the tied queries a few ulps off: rounding makes and breaks ties between mathematically different distances"""
    mids = {}
    for r in ts.r_lattice(T):
        key = r.m.shape[0]
        if key not in mids:
            mids[key] = ctx.set_map(r.m, None, center=False, dtype=T)
        want = ts.brute_in_T(r.q, r.m, INF, 1, T)
        same(match(ctx, mids[key], r.q, T), want, T, r.note)
        if r.h is None or r.h <= 16:
            same(match(ctx, mids[key], r.q, T, 2.0), ts.apply_max_dist(*want, 2.0, T), T, (r.note, "maxDist 2"))
    for mid in mids.values():
        ctx.destroy_map(mid)


@pytest.mark.parametrize("o", ts.OFFSETS)
def test_double_pairs_against_the_float_prefilter(ctx, o):
    """Two map points at nearly the same distance from every query (relative difference 0 to 1e-3, radius 0.1 mm to 30 cm), at the
    origin, 3 km and 400 km from it: in float32 about half the pairs have the wrong winner (asserted on the CPU), so the double
    matcher's float prefilter (item_rounds_dp) must let both through -- its threshold's slope branch at the origin, both branches
    at 3 km, its 400 U^2 floor at 400 km."""
    d = ts.d_pairs(o)
    mid = ctx.set_map(d.m, None, center=False, dtype=np.float64)
    want = ts.brute_in_T(d.q, d.m, INF, 1, np.float64)
    same(match(ctx, mid, d.q, np.float64), want, np.float64, d.note)
    same(match(ctx, mid, d.q, np.float64, 2.0), ts.apply_max_dist(*want, 2.0, np.float64), np.float64, (d.note, "maxDist 2"))
    ctx.destroy_map(mid)


def test_two_maps_of_one_batch(ctx):
    """P48 and C16 indexed by one call: their points share one allocation, and a tie must not be won from next door"""
    T = np.float64
    mp, mc = ctx.set_maps([ts.plane().ref, ts.cube().ref], None, center=False, dtype=T)
    for h in ts.HEIGHTS:
        check_scene(ctx, mp, ts.plane_layer(h, T), T, (icp.MATCHER_GRID,), (INF,))
    check_scene(ctx, mc, ts.cube_all(T), T, (icp.MATCHER_GRID,), (INF,))
    ctx.destroy_map(mp)
    ctx.destroy_map(mc)


@pytest.mark.parametrize("T", ts.TYPES, **TYPE_IDS)
def test_seeded_passes_on_the_tied_plane(ctx, oracle32, oracle64, T):
    """The planar 4-way tie scene through the ICP loop (the map centred, as an ICP's is): every point-to-plane error is exactly 0
    whichever corner is taken, so the pose stays T_init bit for bit and passes 2 and 3 are seeded with a point that is one of four
    equidistant ones.  Per-point state against the oracle, and ids / distances against the integers after every pass."""
    from test_gpu_matcher_state import check_state
    reading, T0, sc = ts.icp_scene()
    oracle = oracle32 if T is np.float32 else oracle64
    ref, nrm, rd = sc.ref.astype(T), sc.nrm.astype(T), reading.astype(T)
    check_state(ctx, oracle, rd, ref, nrm, T0, (1, 2, 3), chain=ALIGN, dtype=T, rtol=0.0 if T is np.float32 else 1e-11)
    mid = ctx.set_map(ref, nrm, dtype=T)
    for it in (1, 2, 3):
        ctx.set_params(**dict(ALIGN, max_iters=it))
        Tout, st = ctx.align(mid, rd, T0, dtype=T)
        assert st["iterations"] == it and np.array_equal(Tout, T0), it
        same(ctx.debug_last_matches(sc.n, dtype=T), (sc.ids, sc.d2_float().astype(T)), T, (sc.note, "after pass", it))
    ctx.destroy_map(mid)
    ctx.set_params(**BASE)


@pytest.mark.parametrize("T", ts.TYPES, **TYPE_IDS)
def test_a_seed_that_is_tied_but_not_the_lowest_index(T):
    """A seeded pass whose seed is one of several equidistant points and NOT the one that must win.  Context A aligns the tied plane
    against the lattice stored as (first half, second half); context B holds the halves the other way round and is seeded with A's
    correspondences through the segment offsets.  Where a square's corners lie in both halves, A's winner (lowest index in A) is a
    corner of the first half, and in B the corners of the second half have the lower indices: the seed ties with the winner."""
    reading, T0, sc = ts.icp_scene()
    n1 = sc.ref.shape[0] // 2
    ref_b = np.concatenate([sc.ref[n1:], sc.ref[:n1]])
    want_ids = ts.int_knn(sc.reading, ref_b)
    seed_in_b = np.where(sc.ids < n1, sc.ids + (sc.ref.shape[0] - n1), sc.ids - n1)
    assert int((seed_in_b != want_ids).sum()) > sc.n // 4                   # the seed is the wrong one of the tied for many queries
    A, B = icp.Context(0, **ts.ICP_CHAIN), icp.Context(0, **ts.ICP_CHAIN)
    try:
        ma = A.set_map(sc.ref.astype(T), sc.nrm.astype(T), center=True, dtype=T)
        mb = B.set_map(ref_b.astype(T), np.concatenate([sc.nrm[n1:], sc.nrm[:n1]]).astype(T), center=False, dtype=T)
        rd = reading.astype(T)
        Tout, st = A.align(ma, rd, T0, dtype=T)
        assert st["status"] == 0 and np.array_equal(Tout, T0)
        same(A.debug_last_matches(sc.n, dtype=T), (sc.ids, sc.d2_float().astype(T)), T, "context A")
        B.partial_chain_seeded(mb, rd, Tout, A, [0, n1, sc.ref.shape[0]], [sc.ref.shape[0] - n1, 0], dtype=T)
        same(B.debug_last_matches(sc.n, dtype=T), (want_ids, sc.d2_float().astype(T)), T, "context B, seeded")
    finally:
        A.close()
        B.close()


def test_which_path_a_layer_reached():
    """Default knobs only (tests/test_gpu_knobs.py leaves this function out): the fast kernel's queue count after the match of each
    height layer of P48, maxDist inf.  A query on the plane is settled by the 3 x 3 x 3 block; one high above it has nothing inside
    the rings the fast kernel walks and goes to the queue, where k_knn_med / k_knn_slow decide its tie.
    Observed on an MI355X (queued of 11 045 queries, the same in float32 and float64): z = 0, s and 4 s: 0; 16 s and 64 s: all 11 045."""
    c = icp.Context(0, **BASE)
    try:
        for T in ts.TYPES:
            mid = c.set_map(ts.plane().ref.astype(T), None, center=False, dtype=T)
            queued = {}
            for h in ts.HEIGHTS:
                sc = ts.plane_layer(h, T)
                same(match(c, mid, sc.reading, T), (sc.ids, sc.d2_float().astype(T)), T, sc.note, sc.parts)
                queued[h] = c.debug_counters()[0]
            print(f"queued by the fast path, {np.dtype(T).name}: " + ", ".join(f"z={h}s: {v} of {ts.plane_layer(h, T).n}" for h, v in queued.items()))
            assert queued[0] == 0, queued
            assert queued[ts.HEIGHTS[-1]] > 0 and queued[ts.HEIGHTS[-2]] > 0, queued
            c.destroy_map(mid)
    finally:
        c.close()
