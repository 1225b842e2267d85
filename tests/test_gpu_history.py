"""A call's outputs are a function of its arguments, the context's parameters and the maps it names -- never of the calls made
before it on the context, nor of what other contexts do beside it (include/pgicp.h, "Conventions").

A pgicp_ctx carries state across calls that must only ever change how a call runs: selection hints per problem index, the
seeded probe's cap, pooled map blocks shared by every context of the device, round-robin upload and filter buffers, a
speculative matcher pass, captured iteration graphs, "counters are clean" flags, scratch that only grows.  Every test here runs
cases of tests/history_cases.py in some order on ONE long-lived context pair and compares every output with the case's baseline
-- the same case on a fresh context pair -- bit for bit (history_cases.compare states the two documented exceptions).  So that
"the same everywhere" cannot mean "wrong everywhere" the baselines are first checked against the oracle with the assertions of
the parity tests.  A failure names the case that ran BEFORE the one that differs.

The same file runs once more in a child process per knob setting (test_history_holds_for_every_knob_setting), and four threads
walk the catalogue at the same time on contexts of their own (test_four_contexts_at_the_same_time)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import history_cases as hc
from history_cases import CASES, F32, F64, compare
from pgslam_amd import icp, synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMUTATION_SEEDS = (20260101, 20260102, 20260103)
N_THREADS = 4                                       # never more than eight
HINTS_ON = os.environ.get("PGICP_SEL_HINTS", "1") != "0"

_BASE = {}
_CALLED = {}


class RecordingLib:
    """the library with the names of the entry points looked up on it written down (what a case really calls)"""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        if name.startswith("pgicp_"):
            self.names.add(name)
        return getattr(self._lib, name)


def fresh_pair():
    return icp.Context(0), icp.Context(0)


def baseline(key, run=None):
    """the case on a fresh context pair, closed afterwards (computed once per process)"""
    if key not in _BASE:
        ctx, aux = fresh_pair()
        rec = RecordingLib(ctx.lib)
        ctx.lib = aux.lib = rec
        try:
            _BASE[key] = (run or CASES[key].run)(ctx, aux)
            _CALLED[key] = set(rec.names)
        finally:
            ctx.close(); aux.close()
    return _BASE[key]


class Walk:
    """one long-lived context pair; every step is compared with its baseline and blamed on the step before it"""

    def __init__(self, pair=None):
        self.ctx, self.aux = pair or fresh_pair()
        self.prev = "(a fresh context)"

    def step(self, key, run=None):
        base = baseline(key, run)
        got = (run or CASES[key].run)(self.ctx, self.aux)
        bad = compare(base, got)
        assert not bad, f"{key} directly after {self.prev} differs from its baseline: {bad[:6]}"
        self.prev = key
        return got

    def close(self):
        self.ctx.close(); self.aux.close()


@pytest.fixture(scope="module")
def walk():
    w = Walk()
    yield w
    w.close()


# ---- the baselines can be trusted ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.oracle is not None])
def test_baseline_against_the_oracle(oracle32, oracle64, name):
    CASES[name].oracle(baseline(name), (oracle32, oracle64, baseline))


@gpu
def test_every_case_calls_what_it_declares():
    """tests/test_history_catalogue.py counts an entry point as reached where a case DECLARES it: here every declaration is held
    against what the case looked up on the library during its baseline run, and the header's list against the union of it"""
    for name, c in CASES.items():
        baseline(name)
        missing = set(c.api) - _CALLED[name]
        assert not missing, f"{name} declares {sorted(missing)} and does not call them"
    declared = set(hc.declared())
    called = set().union(*(_CALLED[n] for n in CASES))
    assert not declared - called - set(hc.EXCLUDED), sorted(declared - called - set(hc.EXCLUDED))


@gpu
def test_baseline_matcher_state_against_the_oracle(oracle32):
    from test_gpu_matcher_state import check_state
    s = hc.two_scans()
    ctx = icp.Context(0)
    hc.set_chain(ctx)
    check_state(ctx, oracle32, s["reading_xyz"], s["ref_xyz"], s["ref_nrm"], s["T_init"], (1, 2, 30), chain=hc.WHOLE)
    ctx.close()


# ---- history -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_each_case_twice_in_a_row(walk, name):
    """its own hint, its own recycled blocks"""
    walk.step(name)
    walk.step(name)


@gpu
@pytest.mark.parametrize("seed", PERMUTATION_SEEDS)
def test_seeded_permutation_of_the_catalogue(walk, seed):
    names = list(CASES)
    for k in np.random.default_rng(seed).permutation(len(names)):
        walk.step(names[k])


# -- hostile pairs: selection hints ---------------------------------------------------------------------------------------------
def batch_run(P, dtype=F32, kind="align", **kw):
    key = f"batch[{kind},P={P},{np.dtype(dtype).name}," + ",".join(f"{k}={v}" for k, v in sorted(kw.items())) + "]"
    return key, functools.partial(hc.run_batch, P=P, big=True, dtype=dtype, kind=kind, **kw)


def first_thresholds(P, T_scale):
    """every problem's FIRST threshold: trim_limit of the one-iteration ICP from the same start (baseline values)"""
    key, run = batch_run(P, T_scale=T_scale, max_iters=1, dense=True)
    b = baseline(key, run)
    return np.array([float(b[f"p{p}.trim_limit"]) for p in range(P)])


def band_path_taken(P):
    """launch_trim_select: the band path runs when there is a guess, the batch's largest problem is above the one-launch
    selection's limit and PGICP_SEL_BAND says so (unset: from kSelBandMinProblems problems on)"""
    band = os.environ.get("PGICP_SEL_BAND")
    small_n = int(os.environ.get("PGICP_SEL_SMALL_N", hc.SEL_SMALL_N))
    return (int(band) != 0 if band else P >= hc.SEL_BAND_MIN_P) and hc.BIG_N > small_n


FAR, NEAR = 4.0, 0.0            # the initial error scaled: four times the catalogue's perturbation, and none (the truth)


@gpu
@pytest.mark.parametrize("kind", ["align", "chain"])
@pytest.mark.parametrize("first", ["near", "far"])
@pytest.mark.parametrize("P", hc.BATCH_P)
def test_hint_far_outside_the_band_either_way(P, kind, first):
    """(a) the same P again from a start whose first threshold is more than 16x / less than 1/16 of the hint it inherits (the
    band around a hint is two octaves either side: sel_band_of): the rank lies outside the band, the full select must run"""
    near, far = first_thresholds(P, NEAR), first_thresholds(P, FAR)
    assert np.all(far > 16.0 * near), (near, far)              # the precondition, on baseline values: hostile both ways
    # (kind = "chain": pgicp_partial_chain_batch returns no threshold, so nothing better is available through the ABI than the
    #  first threshold of the ALIGN from the same start -- the same reading at the same pose against the same cloud, there indexed
    #  centred: the distances, and so the quantile, agree to rounding.  The chain has its own hint slot, filled by its own calls.)
    w = Walk()
    try:
        hinted = False                                         # (the first call of a fresh context inherits nothing)
        for scale in ((NEAR, FAR, NEAR, FAR) if first == "near" else (FAR, NEAR, FAR, NEAR)):
            before = w.ctx.debug_counters()[3]                 # (reading it clears it)
            w.step(*batch_run(P, kind=kind, T_scale=scale, dense=True))
            missed = w.ctx.debug_counters()[3]
            print(f"guess misses: P={P} {kind} scale={scale}: {missed}")
            if hinted and band_path_taken(P) and HINTS_ON:
                # the hinted first selection took the band path with a hint more than 16x too low (FAR after NEAR) or too high
                # (NEAR after FAR): either way the rank lies outside the band and k_sel_final2 must have fallen back to the full
                # select (g_sel_fallbacks counts exactly that, on both sides).  Below kSelBandMinProblems problems (and with
                # the hints off) no selection of a run's first iteration takes the band path: the counter does not count
                # there, and the comparison with the baseline is all that is asserted.
                assert missed > 0, (P, kind, scale, before, missed)
            hinted = True
    finally:
        w.close()


@gpu
@pytest.mark.parametrize("P", [p for p in hc.BATCH_P if p >= hc.SEL_BAND_MIN_P])
def test_a_chain_change_drops_the_hints(P):
    """pgicp_set_params: "another chain: its thresholds are not this one's" -- the hints are dropped.  A hint never reaches a result
    (the tests above), so a hint that wrongly survives shows only in how the call runs: after a chain change the call must miss
    its guesses exactly as often as the same call on a fresh context does (the guess-miss count is a function of the data and the
    guesses).  Added because a library whose hints survived a chain change passed every comparison of results."""
    other = batch_run(P, T_scale=NEAR, dense=True, chain=(("trim_ratio", 0.8),))
    fresh = Walk()
    try:
        fresh.ctx.debug_counters()
        fresh.step(*other)
        want = fresh.ctx.debug_counters()[3]
    finally:
        fresh.close()
    w = Walk()
    try:
        w.step(*batch_run(P, T_scale=FAR, dense=True))            # leaves hints 16x and more above what follows
        w.ctx.debug_counters()
        w.step(*other)
        got = w.ctx.debug_counters()[3]
        print(f"guess misses after a chain change: P={P}: {got}, on a fresh context: {want}")
        assert got == want, (P, got, want)
    finally:
        w.close()


@gpu
@pytest.mark.parametrize("kind", ["align", "chain"])
@pytest.mark.parametrize("P", [3, 4, 8])
def test_hint_of_another_problem(P, kind):
    """(b) the problems permuted, so that index p inherits another problem's hint; (c) with it sizes swap between 50 points and
    the largest (the ragged set holds both)"""
    w = Walk()
    try:
        rot = tuple(np.roll(np.arange(P), 1).tolist())
        rev = tuple(range(P - 1, -1, -1))
        for order in (None, rot, rev, None, rev):
            w.step(*batch_run(P, kind=kind, order=order))
    finally:
        w.close()


def single_run(n, kind):
    """one problem of n points (a strided sample of the largest scan) against the large map"""
    def run(ctx, aux):
        w = hc.s2m_big()
        full = w.scans_xyz[0]
        rd = np.ascontiguousarray(full[:: len(full) // n][:n])
        hc.set_chain(ctx)
        mid = ctx.set_map(w.map_xyz, w.map_nrm, center=kind == "align")
        out = {}
        if kind == "align":
            T, sts = ctx.align_batch([mid], [rd], [w.T_init[0]], raise_on_error=False)
            out["T"] = T
            hc.put_stats(out, "p0", sts[0])
            hc.put_last_matches(out, "p0", ctx, n, 0, F32, sts[0]["trim_limit"])
        else:
            ratio, resid, status = ctx.partial_chain_batch([mid], [rd], [w.T_init[0]], raise_on_error=False)
            out.update({"ratio": ratio, "resid": resid, "status": status})
        ctx.destroy_map(mid)
        return out
    return f"single[{kind},n={n}]", run


@gpu
@pytest.mark.parametrize("kind", ["align", "chain"])
def test_one_problem_of_50_points_and_of_the_largest_size(kind):
    """(c) for P = 1: 50 points, the largest size, 50 points again, the largest again -- index 0 inherits the other size's hint"""
    w = Walk()
    try:
        for n in (50, hc.BIG_N, 50, hc.BIG_N, 50):
            w.step(*single_run(n, kind))
    finally:
        w.close()


def probe_end(far):
    """a case that ENDS with a plain probe: far off the map (a large threshold is left behind) or on it (a small one)"""
    def run(ctx, aux):
        xa, na, xb, nb, scan, T0, start_a, dst = hc.probe_scene()
        hc.set_chain(ctx)
        mb = ctx.set_map(xb, nb, center=False)
        T_on = T0 @ synth.se3_inv(synth.perturbation(41))
        ratio, resid = ctx.partial_chain(mb, scan, T=T_on @ synth.se3(x=1.2, y=0.5, yaw=np.deg2rad(4.0)) if far else T_on)
        ctx.destroy_map(mb)
        return {"ratio": np.array(ratio), "resid": np.array(resid)}
    return f"probe_end[{'far' if far else 'on the map'}]", run


@gpu
def test_the_probes_cap_comes_from_another_case():
    """pgicp_partial_chain_seeded caps its search at a multiple of the threshold the context's PREVIOUS probe ended with ("a cap
    that is wrong costs time, never a result").  In the catalogue's seeded case the previous probe belongs to the case itself;
    here it belongs to the case before: one that ends far off the map (a cap far too large) and one that ends on it (far too
    small for the probe 40 cm off), each directly followed by a case whose FIRST probe is the seeded one."""
    far, on = baseline(*probe_end(True)), baseline(*probe_end(False))
    assert float(far["resid"]) > 4.0 * float(on["resid"]), (far, on)      # (as tests/test_gpu_parity.py states its precondition)
    followers = [(f"seeded_first[{first},{np.dtype(dt).name},{fn.__name__}]", functools.partial(fn, dtype=dt, first=first))
                 for first in ("seeded", "seeded_off") for fn, dt in ((hc.run_seeded, F32), (hc.run_seeded, F64), (hc.run_seeded_scan, F32))]
    w = Walk()
    try:
        for key, run in followers:
            for end in (True, False, True):
                w.step(*probe_end(end))
                w.step(key, run)
    finally:
        w.close()


def subset_run(P, dtype):
    return f"subset[P={P},{np.dtype(dtype).name}]", functools.partial(hc.run_subset, P=P, dtype=dtype)


def far_run(P, dtype):
    return f"far_mode[P={P},{np.dtype(dtype).name}]", functools.partial(hc.run_far, P=P, dtype=dtype)


def no_match_at(P, p_bad, dtype=F32):
    def run(ctx, aux):
        mx, mn, rds, T0 = hc.batch_problem_set(P, True)
        hc.set_chain(ctx)
        mid = ctx.set_map(mx.astype(dtype), mn.astype(dtype), center=True, dtype=dtype)
        T0 = list(T0)
        T0[p_bad] = T0[p_bad] @ synth.se3(x=500.0)
        T, sts = ctx.align_batch([mid] * P, [r.astype(dtype) for r in rds], T0, dtype=dtype, raise_on_error=False)
        out = {"T": T}
        for p in range(P):
            hc.put_stats(out, f"p{p}", sts[p])
        ctx.destroy_map(mid)
        assert out[f"p{p_bad}.status"] == icp.ERR_NO_MATCH, out[f"p{p_bad}.status"]
        return out
    return f"no_match_at[{p_bad} of {P}]", run


@gpu
@pytest.mark.parametrize("P", hc.BATCH_P)
def test_hints_across_zero_quantiles_types_errors_and_far_mode(P):
    w = Walk()
    try:
        normal = batch_run(P)
        # (d) a reading that is a subset of the map -- every distance 0, quantile 0 -- before and after a normal one
        w.step(*normal); w.step(*subset_run(P, F32)); w.step(*normal); w.step(*subset_run(P, F32))
        # (e) f32, f64, f32 with the same P: the hints live in the context, not in the typed state
        w.step(*batch_run(P, dtype=F64)); w.step(*normal); w.step(*batch_run(P, dtype=F64))
        w.step(*batch_run(P, kind="chain")); w.step(*batch_run(P, kind="chain", dtype=F64)); w.step(*batch_run(P, kind="chain"))
        # (f) a problem that ended ERR_NO_MATCH at index p, then a good one at p
        w.step(*no_match_at(P, P - 1)); w.step(*normal); w.step(*no_match_at(P, 0)); w.step(*normal)
        # (g) a far-mode scan (ahead of its map) after an ordinary one and the reverse
        w.step(*far_run(P, F32)); w.step(*normal); w.step(*far_run(P, F32)); w.step(*far_run(P, F64)); w.step(*normal)
    finally:
        w.close()


# -- hostile pairs: the device pool of map blocks -------------------------------------------------------------------------------
def alloc_count():
    out = (C.c_longlong * 8)()
    assert icp.load_library().pgicp_debug_alloc_stats(out) == 0
    return int(out[0])


def map_run(n, seed, extent, shape=(1.0, 1.0, 1.0), n_scan=4000):
    """index a plane cloud, match and align a reading cut from it"""
    def run(ctx, aux, builder=None):
        xyz, nrm = hc.plane_cloud(n, seed, extent, shape)
        hc.set_chain(ctx)
        if builder is None:
            mid = ctx.set_map(xyz, nrm, center=True)
        else:                                   # built by the other context, handed over (pgicp_map_transfer)
            hc.set_chain(builder)
            mid = ctx.adopt_map(builder, builder.set_map(xyz, nrm, center=True))
        rd = np.ascontiguousarray(xyz[:: max(1, n // n_scan)][:n_scan])
        T0 = synth.se3(x=0.05, y=-0.03, yaw=0.004)
        T, st = ctx.align(mid, rd, T0)
        ids, d2 = ctx.match(mid, rd, T=T0)
        out = {"T": T, "ids": ids, "d2": d2, "size": ctx.map_size(mid)}
        hc.put_stats(out, "a", st)
        ctx.destroy_map(mid)
        return out
    return run


@gpu
def test_a_new_map_on_a_previous_maps_block(walk):
    """block_alloc hands a pooled block of S bytes to any request of b bytes with b <= S <= b + b / 2 + 1 MiB, and allocates a new
    block an eighth larger than asked for: after a map of request r is destroyed, any request between 3/4 r and 9/8 r lands on
    its tables.  A 1 M-point map is built and destroyed; maps of OTHER clouds follow whose requests fall in that window.  The
    request of these box-shaped clouds is dominated by the cell tables (map_create_batch: h = sqrt(2 area / m), about
    volume / h^3 cells of 8 to 40 bytes against 52 bytes a point; the 1 M-point cube is cut back once by the 2^26-cell bound to
    3.4e7 cells): 580 k points in a cube of another size and 675 k points in a 4 : 2 : 1 box (other grid dimensions, another
    density) both come to about 3.0e7 cells.  That they were served from the pool is asserted, not assumed: no hipMalloc during the
    build (all scratch has its final size by then)."""
    big = map_run(1_000_000, 1, 60.0)
    specs = [("pool_map[580k,cube]", (580_000, 2, 200.0)), ("pool_map[675k,box]", (675_000, 3, 40.0, (1.0, 0.5, 0.25)))]
    # The baselines first: each leaves its map's block in the pool, where the same map would find it again -- stale contents
    # that are the right contents.  A holder context takes those blocks out of the pool (it builds the same maps and keeps them),
    # so that the only block large enough for the maps below is the 1 M-point map's.
    baseline("pool_map[1M]", big)
    holder = icp.Context(0)
    for key, spec in specs:
        baseline(key, map_run(*spec))
    for key, spec in specs:                 # (both contexts' scratch at its final size before hipMalloc calls are counted)
        run = map_run(*spec)
        walk.step(key, run)
        walk.step(key, lambda c, a: run(c, a, builder=a))
    for key, spec in specs:
        holder.set_map(*hc.plane_cloud(*spec), center=True)
    try:
        for key, spec in specs:
            run = map_run(*spec)
            for builder in ("ctx", "aux"):
                if builder == "ctx":
                    walk.step("pool_map[1M]", big)
                    again = run
                else:           # the block built by aux, adopted and destroyed by ctx, then reused by aux for its next build
                    walk.step("pool_map[1M]", lambda c, a: big(c, a, builder=a))
                    again = lambda c, a: run(c, a, builder=a)
                before = alloc_count()
                walk.step(key, again)
                print(f"{key} built by {builder}: {alloc_count() - before} hipMalloc calls")
                assert alloc_count() == before, f"{key}: the map was not served from the pool ({alloc_count() - before} hipMalloc calls)"
    finally:
        holder.close()


# -- hostile pairs: uploads and filter result sets ------------------------------------------------------------------------------
def _align_dev(ctx, mid, dev, T0, out, key):
    T, st = ctx.align(mid, dev, T0)
    out[f"{key}.T"] = T
    hc.put_stats(out, key, st)


def run_upload_ring(ctx, aux):
    """six uploads of growing and shrinking sizes, each aligned while the next is already in flight (two uploads are kept)"""
    w = hc.s2m()
    hc.set_chain(ctx)
    mid = ctx.set_map(w.map_xyz, w.map_nrm, center=True)
    sizes = [500, 6000, 50, 4097, 6000, 1]
    rds = [np.ascontiguousarray(w.scans_xyz[k % 3][:n]) for k, n in enumerate(sizes)]
    out = {}
    devs = [ctx.upload([rds[0]])[0]]
    for k in range(len(sizes)):
        if k + 1 < len(sizes):
            devs.append(ctx.upload([rds[k + 1]])[0])
        if sizes[k] > 50:
            _align_dev(ctx, mid, devs[k], w.T_init[k % 3], out, f"u{k}")
        else:
            ratio, resid = ctx.partial_chain(mid, devs[k], T=w.T_init[k % 3])
            out[f"u{k}.ratio"], out[f"u{k}.resid"] = np.array(ratio), np.array(resid)
    ctx.destroy_map(mid)
    return out


def run_filter_ring(ctx, aux):
    """five pgicp_filter_cloud_dev calls of different sizes; the pointer of call k is aligned on after calls k+1 .. k+3 (the header:
    "valid for the next three pgicp_filter_cloud calls on the context")"""
    s = hc.two_scans()
    hc.set_chain(ctx)
    mid = ctx.set_map(s["ref_xyz"], s["ref_nrm"], center=True)
    sizes = [6000, 700, 3000, 5000, 1500, 6000, 200, 4000]
    devs, out = [], {}
    for k, n in enumerate(sizes):
        nout, dev, dropped = ctx.filter_cloud_dev(hc.FILTERS[:2], hc._features(F32, n))
        devs.append(dev)
        out[f"f{k}.n"], out[f"f{k}.dropped"] = nout, dropped
        if k >= 3:
            _align_dev(ctx, mid, devs[k - 3], s["T_init"], out, f"f{k - 3}")
    ctx.destroy_map(mid)
    return out


@gpu
def test_upload_and_filter_buffers_reused_round_robin(walk):
    for _ in range(2):
        walk.step("upload_ring", run_upload_ring)
        walk.step("filter_ring", run_filter_ring)
        walk.step("upload_align_f64")
        walk.step("filter_cloud_dev_align_f64")


# -- hostile pairs: speculation, error exits, scratch ---------------------------------------------------------------------------
@gpu
def test_a_converged_single_align_followed_by_every_other_kind_of_call(walk):
    """a single problem's next matcher pass is enqueued behind its last iteration (PGICP_SPECULATE): what follows directly must
    not see it"""
    assert baseline("align_f32")["a.converged"] == 1
    for follower in ("match_knn1_grid_f32", "match_knn3_grid_f64", "partial_chain_f32", "partial_chain_batch_3_f32", "voxel_grid_f32",
                     "sampling_surface_normal_f32", "align_batch_3_f64", "align_batch_4big_f32", "surface_normals_f32", "build_local_map_device_f32",
                     "partial_chain_seeded_f32", "outlier_weights_var_trim_f32", "icp_pair_f64"):
        walk.step("align_f32")
        walk.step(follower)


@gpu
@pytest.mark.parametrize("err", hc.ERROR_CASES)
def test_an_error_exit_followed_by_ordinary_calls(walk, err):
    for follower in ("align_f32", "partial_chain_batch_4_f32", "voxel_grid_f64"):
        walk.step(err)
        walk.step(follower)


@gpu
def test_scratch_grown_by_the_largest_case_serves_the_smallest(walk):
    for name in ("align_batch_8big_f32", "outlier_weights_trimmed_f32", "align_batch_8big_f32", "transform_f32", "align_batch_4big_f64",
                 "match_knn1_brute_f32"):
        walk.step(name)


@gpu
def test_the_filter_families_share_their_scratch(walk):
    """SamplingSurfaceNormal, VoxelGrid and the densities carve the same three buffers: every call lays out what another family's
    call left behind -- the largest layout first, then smaller ones of the other families, both precisions"""
    for name in ("sampling_surface_normal_f64", "max_density_f32", "voxel_grid_f64", "normals_max_density_f32", "surface_densities_f64",
                 "voxel_grid_f32", "sampling_surface_normal_f32", "normals_max_density_f64"):
        walk.step(name)


# ---- the same file under other settings -----------------------------------------------------------------------------------------
SETTINGS = [
    {"PGICP_SEL_HINTS": "0"},
    {"PGICP_TABLES": "succinct"},
    {"PGICP_GRAPH_MAX_P": "4096"},          # every iteration replayed from a captured graph: more than eight shapes pass the eight-entry cache
    {"PGICP_SEL_BAND": "1", "PGICP_SEL_SMALL_N": "0"},
]


@gpu
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k[6:]}={v}" for k, v in s.items()))
def test_history_holds_for_every_knob_setting(setting):
    # (the history tests only: the oracle checks, the concurrency pass and this test itself belong to the parent run)
    env = dict(os.environ, **setting)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_history.py", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "not four_contexts and not knob_setting and not against_the_oracle"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


# ---- concurrency -------------------------------------------------------------------------------------------------------------------
def priority_context(high):
    lib = icp.load_library()
    c = icp.Context.__new__(icp.Context)
    c.lib = lib
    h = C.c_void_p()
    st = lib.pgicp_ctx_create_priority(C.c_int(0), C.c_int(int(high)), C.byref(h))
    if st != icp.OK:
        raise icp.PgicpError(st, "pgicp_ctx_create_priority failed")
    c.h, c.device, c.params = h, 0, icp.Params()
    lib.pgicp_default_params(C.byref(c.params))
    return c


N_HANDOVERS = 8


@gpu
def test_four_contexts_at_the_same_time():
    """Four host threads, a context pair each on device 0, released together, each walking its own permutation of the small and
    medium cases ONCE (ctypes releases the GIL during a call: the calls overlap on the device).  Map-building cases stay in, so
    blocks migrate between contexts through the device pool while others align.

    Threads 0 and 1 also play server and builder across threads, as pgslam_amd/local_mapper.py does: after every few cases of its
    own walk the builder (thread 1) indexes a map on ITS context and hands the id over through a queue; the server (thread 0)
    takes it over on its own context (pgicp_map_transfer of a block built on another thread's stream, while the server's stream
    has work of its own), aligns against it, compares with the baseline of adopt_map_align and destroys it.  The builder touches
    its context again only once the server has acknowledged the transfer (a context is thread-compatible), so its next case runs
    while the server aligns on the adopted map.  Thread 2's context has a high-priority stream.

    A single fixed pass.  After any failure no thread starts another call; after a HIP error or a timeout nothing further is
    started on the device in this process: the session ends."""
    import queue
    names = hc.SMALL_MEDIUM
    for n in names:
        baseline(n)                                     # (all baselines first, single-threaded)
    pairs = [(priority_context(True) if t == 2 else icp.Context(0), icp.Context(0)) for t in range(N_THREADS)]
    barrier = threading.Barrier(N_THREADS)
    stop = threading.Event()
    errors, hip_error = [], []
    handed, taken = queue.Queue(), queue.Queue()        # builder -> server: (map id, dtype); server -> builder: acknowledged
    SERVER, BUILDER = 0, 1
    every = max(1, len(names) // N_HANDOVERS)

    def check(t, key, got, prev):
        bad = compare(_BASE[key], got)
        if bad:
            raise AssertionError(f"thread {t}: {key} directly after {prev} differs from its baseline: {bad[:6]}")

    def work(t):
        ctx, aux = pairs[t]
        prev = "(a fresh context)"
        served = 0
        try:
            barrier.wait(timeout=120)
            for j, k in enumerate(np.random.default_rng(777 + t).permutation(len(names))):
                if stop.is_set():
                    return
                check(t, names[k], CASES[names[k]].run(ctx, aux), prev)
                prev = names[k]
                if j % every != every - 1 or j // every >= N_HANDOVERS:
                    continue
                dtype = F32 if (j // every) % 2 == 0 else F64
                key = "adopt_map_align" + ("_f32" if dtype == F32 else "_f64")
                if t == BUILDER:
                    handed.put((hc.adopt_build(ctx, dtype), dtype))
                    while not stop.is_set():            # the builder's context is the server's to touch until it says so
                        try:
                            taken.get(timeout=1.0)
                            break
                        except queue.Empty:
                            pass
                    prev = f"building a map for thread {SERVER}"
                elif t == SERVER:
                    built = None
                    for _ in range(300):
                        if stop.is_set():
                            return
                        try:
                            built, bdtype = handed.get(timeout=1.0)
                            break
                        except queue.Empty:
                            pass
                    if built is None:
                        raise TimeoutError("no map was handed over within 300 s")
                    assert bdtype == dtype
                    builder_ctx = pairs[BUILDER][0]

                    class Acknowledging:                # adopt_serve calls ctx.adopt_map(builder, id): acknowledge right after it
                        def __getattr__(self, n):
                            return getattr(ctx, n)

                        def adopt_map(self, other, mid):
                            try:
                                return ctx.adopt_map(other, mid)
                            finally:
                                taken.put(True)
                    check(t, key, hc.adopt_serve(Acknowledging(), builder_ctx, built, dtype), prev)
                    prev = f"{key} on a map built by thread {BUILDER}"
                    served += 1
            if t == SERVER:
                assert served == N_HANDOVERS, served
        except BaseException as e:          # noqa: BLE001 -- collected, the main thread fails with all of them
            errors.append(f"thread {t} after {prev}: {type(e).__name__}: {e}")
            if isinstance(e, icp.PgicpError) and e.code == icp.ERR_HIP:
                hip_error.append(t)
            stop.set()
            barrier.abort()

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(N_THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=600)
    hung = [th.name for th in threads if th.is_alive()]
    if hung or hip_error:
        stop.set()
        pytest.exit(f"test_four_contexts_at_the_same_time: {'threads still inside a call after the timeout: ' + str(hung) if hung else 'HIP error'}; "
                    f"nothing further is started on the device in this process.  {errors}", returncode=3)
    for c, a in pairs:
        c.close(); a.close()
    assert not errors, "\n".join(errors)
