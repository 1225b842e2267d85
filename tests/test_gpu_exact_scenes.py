"""Outlier selection and pair sums on scenes whose arithmetic is exact (tests/exact_scenes.py).

Every other GPU test of the ICP pipeline compares the device with oracle/icp_oracle.c, which since the shared reduction tree
mirrors the device's block, lane and chain shape.  Here the expected threshold, counts and sums come from integer arithmetic
that shares nothing with either; the oracle is compared as well (whole stats record and T, bit for bit), and
tests/test_exact_scenes_host.py has already shown that it agrees with the closed forms on the CPU.  No tolerances: `==` on
values that are exactly representable, or bytes.

  A  the unguessed wide selection (k_sel_hist, k_sel_filter, k_sel_final): one value, two values split at the rank, ramps
  B  a hinted first selection (k_sel_band, k_sel_final2): the rank on and beside both band edges, slice overflow, slice select;
     the fallback counter in both directions; the same through the partial chain's own hint slot
  C  later iterations without hints: 43 264 ties at the quantile for six iterations, and the band [0, 0]
  D  256 problems: the stage buffers of k_sel_filter and k_sel_band filled to exactly kSelStage
  E  the 30 pair sums at the wave, block, round, span and chain edges of the reduction tree: stage level, whole chain in both
     summation orders, three neighbours per point, a normal filter (the two GEN = true instances)
Default knobs: B's fallback assertions and D's shape depend on them (tests/test_gpu_knobs.py runs A and E under every setting)."""
import contextlib
import os
import re

import numpy as np
import pytest

import exact_scenes as X
from pgslam_amd import icp

pytestmark = pytest.mark.gpu

CHAIN = dict(max_dist=X.MAX_DIST, trim_ratio=0.85, max_iters=1, min_diff_rot=0.0, min_diff_trans=0.0, smooth_length=3, sensor_std_dev=0.01)
DTYPES = [np.float32, np.float64]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pgslam_amd", "csrc")
EYE = np.eye(4)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class Rig:
    """a fresh context (no hints from any earlier call) with the scene's plane as its map, and the oracle's copy of that map"""

    def __init__(self, orc, plane, dtype, **chain):
        self.orc, self.dtype, self.plane = orc, dtype, plane
        self.chain = dict(CHAIN, **chain)
        self.ctx = icp.Context(0, **self.chain)
        self.mid = self.ctx.set_map(plane.ref.astype(dtype), plane.nrm.astype(dtype), center=False, dtype=dtype)
        self.omap = orc.map_create(plane.ref.astype(dtype), plane.nrm.astype(dtype), center=False)
        self._oracle_cache = {}

    def close(self):
        self.orc.map_free(self.omap)
        self.ctx.destroy_map(self.mid)
        self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def align(self, scenes, normals=None):
        rds = [sc.reading.astype(self.dtype) for sc in scenes]
        nr = None if normals is None else [a.astype(self.dtype) for a in normals]
        return self.ctx.align_batch([self.mid] * len(rds), rds, [EYE] * len(rds), dtype=self.dtype, raise_on_error=False, normals=nr)

    def chain_pass(self, scenes):
        rds = [sc.reading.astype(self.dtype) for sc in scenes]
        return self.ctx.partial_chain_batch([self.mid] * len(rds), rds, [EYE] * len(rds), dtype=self.dtype, raise_on_error=False)

    def oracle_icp(self, sc, p):
        """the oracle's run of problem p of the call just made, its pairs in the order the device sorted that reading in"""
        order = self.ctx.reading_order(sc.n, problem=p)
        key = (sc.reading.tobytes(), order.tobytes(), tuple(sorted(self.chain.items())))
        if key not in self._oracle_cache:
            self._oracle_cache[key] = self.orc.icp_map(self.omap, sc.reading.astype(self.dtype), EYE, pair_order=order, **self.chain)
        return self._oracle_cache[key]


@contextlib.contextmanager
def mapped_context(plane, dtype, **chain):
    """a fresh context with `plane` as its map, for the tests that ask no oracle; released whatever the body does"""
    ctx = icp.Context(0, **dict(CHAIN, **chain))
    try:
        mid = ctx.set_map(plane.ref.astype(dtype), plane.nrm.astype(dtype), center=False, dtype=dtype)
        yield ctx, mid
    finally:
        ctx.close()


def check_closed_form(st, sc, ratio, dtype, what):
    limit, nf, nk = X.expected_limit(sc.d2_int(), ratio, dtype)
    want = float(limit) / 2.0 ** (2 * X.K)
    assert st["status"] == 0, what
    assert st["trim_limit"] == want and st["n_finite"] == nf and st["n_kept"] == nk and st["overlap"] == nk / sc.n, \
        (what, st["trim_limit"], want, st["n_finite"], nf, st["n_kept"], nk)


def check_oracle(st, T, o, what):
    for k in ("status", "iterations", "converged", "max_iter_reached", "n_kept", "n_finite"):
        assert st[k] == o[k], (what, k, st[k], o[k])
    for k in ("overlap", "residual", "trim_limit", "cov"):
        assert same_bits(st[k], o[k]), (what, k, st[k], o[k])
    assert same_bits(T, o["T"]), (what, "T", np.abs(T - o["T"]).max())


def check_batch(rig, scenes, T, st, ratio, what, oracle_for=None):
    for p, sc in enumerate(scenes):
        check_closed_form(st[p], sc, ratio, rig.dtype, (what, p))
        if oracle_for is None or p in oracle_for:
            check_oracle(st[p], T[p], rig.oracle_icp(sc, p), (what, p))


def orc_of(oracle32, oracle64, dtype):
    return oracle32 if dtype == np.float32 else oracle64


# ---- A: the unguessed wide selection -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", X.RATIOS)
@pytest.mark.parametrize("kind", X.SELECTION_KINDS)
def test_a_wide_selection_without_a_guess(oracle32, kind, ratio):
    """P = 4 (big, big, 5 000, 64), one iteration on a fresh context: the first selection has neither a guess nor a hint"""
    scenes = X.selection_batch(kind, ratio, np.float32)
    with Rig(oracle32, X.big_plane(), np.float32, trim_ratio=ratio) as rig:
        T, st = rig.align(scenes)
        check_batch(rig, scenes, T, st, ratio, (kind, ratio))


@pytest.mark.parametrize("ratio", X.RATIOS)
def test_a_wide_selection_all_keys_distinct_f64(oracle64, ratio):
    """The same in float64, where a ramp of 43 264 DISTINCT exact squares exists (in float32 a height may carry 12 bits only, so
    the ramps above repeat each of 2 048 values about 21 times)"""
    scenes = X.selection_batch("ramp", ratio, np.float64)
    assert len(set(scenes[0].d2_int())) == scenes[0].n
    with Rig(oracle64, X.big_plane(), np.float64, trim_ratio=ratio) as rig:
        T, st = rig.align(scenes)
        check_batch(rig, scenes, T, st, ratio, ("ramp64", ratio))


# ---- B: a hinted first selection ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(X.BAND_CASES))
def test_b_hinted_first_selection(oracle32, oracle64, case, dtype):
    """A primer call with every height D0 leaves the hint h = D0^2 for each problem index; the second call's first selection then
    compacts the band [h / 4, 4 h].  Problem 0 carries the designed distribution (exact_scenes.band_batch), the other three
    stay at D0 -- inside the band -- so the fallback counter speaks about problem 0: above 0 where the rank was put outside
    the band, 0 where it was put inside (on an edge included)."""
    forced = X.BAND_CASES[case]
    primer, scenes = X.primer_batch(), X.band_batch(case, dtype)
    with Rig(orc_of(oracle32, oracle64, dtype), X.big_plane(), dtype, trim_ratio=X.BAND_RATIO) as rig:
        T, st = rig.align(primer)
        check_batch(rig, primer, T, st, X.BAND_RATIO, (case, "primer"), oracle_for=())
        rig.ctx.debug_counters()                                   # (reading clears the fallback counter)
        T, st = rig.align(scenes)
        fallbacks = rig.ctx.debug_counters()[3]
        check_batch(rig, scenes, T, st, X.BAND_RATIO, (case, "align"), oracle_for=(0,))
        assert (fallbacks > 0) if forced else (fallbacks == 0), (case, "align", fallbacks)
        # the partial chain keeps hints of its own
        for name, batch in (("primer", primer), ("chain", scenes)):
            rig.ctx.debug_counters()
            ratio, resid, status = rig.chain_pass(batch)
            fallbacks = rig.ctx.debug_counters()[3]
            for p, sc in enumerate(batch):
                _, nf, keep, sums = X.chain_expectation(sc, X.BAND_RATIO, dtype)
                assert status[p] == 0 and ratio[p] == int(keep.sum()) / sc.n and resid[p] == float(sums[29]), (case, name, p, ratio[p], resid[p])
        assert (fallbacks > 0) if forced else (fallbacks == 0), (case, "chain", fallbacks)


# ---- C: later iterations without hints -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["checkerboard", "zero_big", "zero_5000"])
def test_c_later_iterations_tie_at_the_quantile(oracle32, oracle64, which, dtype):
    """Six iterations (min_diff 0): the selections of iterations 2-4 take the band [q / 1024, 1.25 q], those of 5-6
    [q / 2, 1.25 q], each with every key of a reading tied at q.  b = 0 exactly (the checkerboard cancels), so T must stay the
    identity and every iteration sees the same distances.  The all-zero reading (reading = map points) has limit 0, the band
    [0, 0] and slice shift 0: as the big problem (more keys than the final stage holds) and as the 5 000-point one (within)."""
    scenes = {"checkerboard": X.checkerboard_batch, "zero_big": lambda: X.zero_batch(0), "zero_5000": lambda: X.zero_batch(2)}[which]()
    with Rig(orc_of(oracle32, oracle64, dtype), X.big_plane(), dtype, max_iters=6) as rig:
        T, st = rig.align(scenes)
        for p, sc in enumerate(scenes):
            assert st[p]["iterations"] == 6 and same_bits(T[p], EYE), (which, p, st[p]["iterations"], T[p])
            assert st[p]["trim_limit"] == (0.0 if "zero" in sc.note else X.D0 ** 2), (which, p, st[p]["trim_limit"])
        check_batch(rig, scenes, T, st, 0.85, which)


# ---- D: stage buffers at capacity ------------------------------------------------------------------------------------------------
def launch_constants():
    """what launch_trim_select's span depends on, read from the sources"""
    sel = open(os.path.join(CSRC, "k_select.inc")).read()
    lau = open(os.path.join(CSRC, "k_launch.inc")).read()
    tile = int(re.search(r"constexpr\s+int\s+kSelTile\s*=\s*(\d+)\s*;", sel).group(1))
    stage_tiles = int(re.search(r"constexpr\s+int\s+kSelStage\s*=\s*(\d+)\s*\*\s*kSelTile\s*;", sel).group(1))
    blocks = int(re.search(r"per_problem\s*=\s*std::min\(tiles,\s*std::max\(1,\s*(\d+)\s*/\s*P\)\)", lau).group(1))
    assert re.search(r"span\s*=\s*cdiv\(tiles,\s*per_problem\)\s*\*\s*kSelTile", lau) and re.search(r"tiles\s*=\s*cdiv\(max_n,\s*kSelTile\)", lau)
    return tile, stage_tiles, blocks


def test_d_stage_buffers_filled_to_capacity(oracle32):
    """P = 256: one big all-equal reading and 255 readings of 64 points; the primer call (k_sel_filter), then the hinted one
    (k_sel_band).  launch_trim_select: tiles = cdiv(max_n, kSelTile) = cdiv(43 264, 2 048) = 22; per_problem = min(tiles,
    max(1, 2 048 / P)) = min(22, 8) = 8; span = cdiv(22, 8) * kSelTile = 3 tiles.  Every key of the big reading goes to the
    stage buffer: after a block's second tile it holds 2 * kSelTile = kSelStage keys exactly -- full, flushed because a third
    tile would not fit -- and the third tile is flushed at the end.
    The fallback counter is the only signal the library exposes about the selection's path, and 0 says only that no selection
    went over everything: that the hinted call ran k_sel_band at all follows from P >= kSelBandMinProblems and the hints of the
    primer (test B shows that mechanism at work at P = 4 through its forced fallbacks), not from anything asserted here."""
    tile, stage_tiles, blocks = launch_constants()
    n, P = X.BIG_L * X.BIG_L, X.STAGE_P
    tiles = -(-n // tile)
    per_problem = min(tiles, max(1, blocks // P))
    span_tiles = -(-tiles // per_problem)
    assert span_tiles == 3 and stage_tiles == 2 and span_tiles > stage_tiles and n >= span_tiles * tile
    scenes = X.stage_batch()
    assert len(scenes) == P
    with Rig(oracle32, X.big_plane(), np.float32) as rig:
        for call in ("primer", "hinted"):
            rig.ctx.debug_counters()
            T, st = rig.align(scenes)
            assert rig.ctx.debug_counters()[3] == 0, call
            check_batch(rig, scenes, T, st, 0.85, call)


# ---- E: pair sums at the tree's edges -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage_sums():
    """the closed forms of the stage-level scene at every pair count, both minimisers: computed once, read only"""
    sc = X.sums_scene()
    w = X.weights_pattern(sc.n)
    p, q, n, _ = sc.pairs()
    return sc, w, {m: {c: X.to_floats(v) for c, v in X.expected_sums(p, q, n, w, minimizer=m, prefixes=list(X.PAIR_SIZES)).items()} for m in (0, 1)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("minimizer", [0, 1])
def test_e_error_stats_at_every_edge(stage_sums, minimizer, dtype):
    """k_error_stats + k_sum_partials: all 30 sums, ratio and residual at every pair count, about one weight in seven zero"""
    sc, w, want = stage_sums
    rd, ids = sc.reading.astype(dtype), sc.ids.astype(np.int32)
    with mapped_context(sc.plane, dtype, error_minimizer=minimizer) as (ctx, mid):
        for cnt in X.PAIR_SIZES:
            ratio, resid, sums = ctx.error_stats(mid, rd[:cnt], ids[:cnt], w[:cnt].astype(dtype), dtype=dtype)
            e = want[minimizer][cnt]
            assert sums.tobytes() == e.tobytes(), (minimizer, cnt, np.flatnonzero(sums != e), sums[27:], e[27:])
            assert ratio == e[27] / cnt and resid == e[29], (minimizer, cnt)


def check_chain_batch(ctx, mid, scenes, dtype, knn, what):
    rds = [sc.reading.astype(dtype) for sc in scenes]
    ratio, resid, status = ctx.partial_chain_batch([mid] * len(rds), rds, [EYE] * len(rds), dtype=dtype, raise_on_error=False)
    for p, sc in enumerate(scenes):
        _, nf, keep, sums = X.chain_expectation(sc, X.CHAIN_RATIO, dtype)
        if nf == 0:
            assert status[p] != 0, (what, p)
            continue
        assert status[p] == 0 and ratio[p] == int(keep.sum()) / (sc.n * knn) and resid[p] == float(sums[29]), \
            (what, sc.n, ratio[p], int(keep.sum()), resid[p], float(sums[29]))
    return ratio, resid


@pytest.mark.parametrize("dtype", DTYPES)
def test_e_chain_batch_at_every_edge_both_orders(dtype):
    """k_p2plane_reduce<T, 0, false> + k_sum_partials: every pair count in one ragged batch, both summation orders -- the
    answers are the closed form's, hence identical"""
    scenes = [X.chain_scene(n) for n in X.PAIR_SIZES]
    plane = scenes[0].plane
    got = []
    for order in (icp.SUM_ORDER_SORTED, icp.SUM_ORDER_SCAN):
        with mapped_context(plane, dtype, trim_ratio=X.CHAIN_RATIO, sum_order=order) as (ctx, mid):
            got.append(check_chain_batch(ctx, mid, scenes, dtype, 1, ("order", order)))
    assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_e_chain_batch_three_neighbours(dtype):
    """GEN = true through knn = 3: pairs [point][neighbour], 3 n crossing the same edges (exact_scenes.lift_knn3 says why the
    three neighbours are exact and free of ties)"""
    scenes = [X.knn3_scene(n) for n in X.KNN3_SIZES]
    plane = scenes[0].plane
    for order in (icp.SUM_ORDER_SORTED, icp.SUM_ORDER_SCAN):
        with mapped_context(plane, dtype, trim_ratio=X.CHAIN_RATIO, knn=3, sum_order=order) as (ctx, mid):
            check_chain_batch(ctx, mid, scenes, dtype, 3, ("knn3", order))


def test_e_normal_filter_in_the_sums(oracle32):
    """GEN = true through a SurfaceNormalOutlierFilter: reading normals clearly inside or clearly outside the angle"""
    sizes = (65, 2049, 18433)
    scenes = [X.angle_scene(n) for n in sizes]
    with Rig(oracle32, scenes[0].plane, np.float32, trim_ratio=X.CHAIN_RATIO, normal_max_angle=X.NORMAL_MAX_ANGLE) as rig:
        T, st = rig.align(scenes, normals=[sc.reading_nrm for sc in scenes])
        for p, sc in enumerate(scenes):
            limit, nf, keep, sums = X.chain_expectation(sc, X.CHAIN_RATIO, np.float32, extra_keep=sc.angle_inside)
            nk = int(keep.sum())
            assert st[p]["status"] == 0 and st[p]["n_finite"] == nf and st[p]["n_kept"] == nk, (p, st[p]["n_kept"], nk)
            assert st[p]["trim_limit"] == float(limit) and st[p]["overlap"] == nk / sc.n and st[p]["residual"] == float(sums[29]), p
