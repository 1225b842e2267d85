"""pgicp_partial_chain_seeded against every kind of source and every chain of the caller.

The seeded probe is the one entry that reads ANOTHER context's device state: context B takes context A's reading order and A's
correspondences -- slots of the map A aligned against -- and follows them into that map.  pgslam_amd/csrc/seed_source.hpp says
whether A's state is still what it claims to be (every map carries a stamp; map ids are reused, stamps are not), and
k_borrow_order drops a seed that names no slot of A's map.  Here, on the device:

  * sources that must be REFUSED (a ... j): the probe runs unseeded -- B's reading order is the order of B's own plain probe;
  * sources that must stay SEEDED (k ... m): B's reading order is A's;
  * hostile segment tables and a reading A never aligned (n ... q): whatever the seeds are, they are candidates only;
  * B's chain in every variant the probe has a path for -- robust weights (the threshold opened to +inf), a quantile-scaled
    threshold, no trimming, no maxDist, point to point, scan-order sums -- as B's first probe (no cap), with a cap, and with a
    cap that is far too large / far too small.

Results, every time: the ratio is the double of B.partial_chain at the same pose; the residual agrees to 1e-12 relative
(PGICP_SUM_ORDER_SORTED: the same sum in another order) or is identical (PGICP_SUM_ORDER_SCAN); the ratio agrees with the
oracle's partial chain; inside the trim threshold the matches are those of the oracle's k-d tree on the transformed scan.

The scene is history_cases.probe_scene at a smaller size: four keyframes of 3 000 points, map A = keyframes (2, 1, 0) centred,
map B = keyframes (2, 3, 1) not centred, a scan of 2 500 points (no multiple of k_borrow_order's 256-thread block)."""
import functools

import numpy as np
import pytest

from pgslam_amd import icp, synth

pytestmark = pytest.mark.gpu

CHAIN = dict(max_dist=2.0, trim_ratio=0.85, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01,
             smooth_length=3, sensor_std_dev=0.01)
F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
N_KF, N_SCAN = 3000, 2500
SORTED, SCAN = icp.SUM_ORDER_SORTED, icp.SUM_ORDER_SCAN


@functools.lru_cache(maxsize=None)
def scene():
    world = synth.make_world()
    poses = [synth.se3(x=-6.0 + 1.5 * k, yaw=np.deg2rad(1.5 * (k % 3 - 1))) for k in range(5)]
    kf = [synth.make_scan(world, poses[k], N_KF, 7100 + k, rings=16) for k in range(4)]
    ref_pose = poses[2]

    def assemble(order):
        xs, ns = [], []
        for k in order:
            x, n = synth.transform_cloud(synth.se3_inv(ref_pose) @ poses[k], kf[k][0], kf[k][1])
            xs.append(x); ns.append(n)
        return np.concatenate(xs).astype(np.float32), np.concatenate(ns).astype(np.float32), [len(x) for x in xs]
    order_a, order_b = [2, 1, 0], [2, 3, 1]
    xa, na, sizes_a = assemble(order_a)
    xb, nb, sizes_b = assemble(order_b)
    scan, _ = synth.make_scan(world, poses[4] @ synth.se3(x=-2.0), N_SCAN, 7200, rings=16)
    T0 = synth.se3_inv(ref_pose) @ poses[4] @ synth.se3(x=-2.0) @ synth.perturbation(41)
    start_a = np.concatenate([[0], np.cumsum(sizes_a)]).astype(np.int64)
    start_b = np.concatenate([[0], np.cumsum(sizes_b)])
    dst = [int(start_b[order_b.index(k)]) if k in order_b else -1 for k in order_a]
    assert len(scan) == N_SCAN and N_SCAN % 256 != 0 and len(xa) == len(xb) == 3 * N_KF
    assert dst[0] == 0 and dst[1] == 2 * N_KF and dst[2] == -1
    return dict(xa=xa, na=na, xb=xb, nb=nb, scan=scan.astype(np.float32), T0=T0, start_a=start_a, dst=dst)


def split(start, dst, k):
    """the same two maps described as k segments: the segments of (start, dst) cut into pieces as equal as k allows"""
    start, parts = [int(s) for s in start], len(dst)
    per = [k // parts + (1 if i < k % parts else 0) for i in range(parts)]
    src, out = [], []
    for i in range(parts):
        cuts = np.linspace(start[i], start[i + 1], per[i] + 1).astype(np.int64)
        for lo in cuts[:-1]:
            src.append(int(lo))
            out.append(-1 if dst[i] < 0 else dst[i] + int(lo) - start[i])
    src.append(start[-1])
    assert len(out) == k and len(src) == k + 1 and all(b > a for a, b in zip(src, src[1:]))
    return src, out


_ORACLE = {}


def oracle_of(orc, dtype, chain, T):
    """the oracle's partial chain and k-d tree matches for (cloud type, chain, pose): computed once, handed out read-only"""
    key = (np.dtype(dtype).name, tuple(sorted(chain.items())), np.asarray(T).tobytes())
    if key not in _ORACLE:
        s = scene()
        scan, xb, nb = s["scan"].astype(dtype), s["xb"].astype(dtype), s["nb"].astype(dtype)
        po = orc.partial_chain(scan, xb, nb, T, **dict(chain, center_reference=False))
        oid, od2 = orc.knn_kdtree(orc.transform(T, scan), xb, chain["max_dist"])
        for a in (oid, od2):
            a.setflags(write=False)
        _ORACLE[key] = (po["overlap"], po["residual"], oid, od2)
    return _ORACLE[key]


class Pair:
    """fresh contexts for one test: A the source, B the prober, C a third one; closed when the test ends"""

    def __init__(self, dtype, chain_b=CHAIN, sum_order=SORTED, dtype_a=None, knn_a=1, normals_b=True):
        s = scene()
        self.dtype, self.dtype_a = dtype, dtype_a or dtype
        self.chain_b, self.sum_order = chain_b, sum_order
        self.A = icp.Context(0, **dict(CHAIN, knn=knn_a))
        self.B = icp.Context(0, **chain_b, sum_order=sum_order)
        self.ctxs = [self.A, self.B]
        self.scan = s["scan"].astype(dtype)
        self.ma = self.A.set_map(s["xa"].astype(self.dtype_a), s["na"].astype(self.dtype_a), center=True, dtype=self.dtype_a)
        self.mb = self.B.set_map(s["xb"].astype(dtype), s["nb"].astype(dtype) if normals_b else None, center=False, dtype=dtype)
        self.segs = (s["start_a"], s["dst"])

    def third(self):
        self.ctxs.append(icp.Context(0, **CHAIN))
        return self.ctxs[-1]

    def align(self, reading=None):
        """A aligns the scan (or `reading`) against its map: the pose the probes are asked at, and A's reading order"""
        s = scene()
        rd = (s["scan"] if reading is None else reading).astype(self.dtype_a)
        self.T, st = self.A.align(self.ma, rd, s["T0"], dtype=self.dtype_a)
        assert st["status"] == 0
        self.order_a = self.A.reading_order(N_SCAN)
        return self.T

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture
def pair():
    made = []

    def make(*a, **kw):
        made.append(Pair(*a, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


def orc_for(dtype, oracle32, oracle64):
    return oracle32 if dtype == F32 else oracle64


def same(got, plain, sum_order):
    if sum_order == SCAN:
        assert got == plain, (got, plain)
    else:       # (tests/test_gpu_parity.py's same(): the ratio the same double, the residual the same sum in another order)
        assert got[0] == plain[0] and got[1] == pytest.approx(plain[1], rel=1e-12), (got, plain)


def check_result(p, orc, got, matches, plain, T):
    """one probe's ratio and residual against B's plain probe and the oracle, its matches against the oracle's k-d tree"""
    chain, f32 = p.chain_b, p.dtype == F32
    same(got, plain, p.sum_order)
    ov, res, oid, od2 = oracle_of(orc, p.dtype, chain, T)
    if chain.get("robust_fct", 0):  # (test_gpu_chain.py::test_robust_filter_in_a_batch_and_in_the_partial_chain's comparison)
        assert got[0] == pytest.approx(ov, rel=1e-6 if f32 else 1e-12) and got[1] == pytest.approx(res, rel=1e-6), (got, ov, res)
    else:                           # (test_gpu_parity.py::test_seeded_partial_chain_equals_the_unseeded_one's)
        assert got[0] == pytest.approx(ov, rel=1e-12), (got, ov)
    # inside the trim threshold (beyond it the capped search is lazy): the 0.8 quantile under the default ratio, the median -- "well
    # inside", as the same test has it -- under a chain that keeps half
    ids, _ = matches
    fin = np.isfinite(od2)
    kept = (od2 <= np.quantile(od2[fin], 0.8 if chain["trim_ratio"] >= 0.85 else 0.5)) & (oid >= 0)
    assert kept.sum() > N_SCAN // 4                                  # (the mask is worth something)
    assert np.array_equal(ids[kept], oid[kept]), int((ids[kept] != oid[kept]).sum())


def probe_thrice(p, orc, expect, segs=None, src=None):
    """The seeded call as B's first probe (no hint, so no cap), B's plain probe, the seeded call again (a hint, so a cap when it is
    seeded): results every time; which path ran by B's reading order -- A's when seeded, its own sort's when not."""
    B, n, T = p.B, N_SCAN, p.T
    segs = p.segs if segs is None else segs
    src = p.A if src is None else src

    def seeded_call():
        got = B.partial_chain_seeded(p.mb, p.scan, T, src, segs[0], segs[1], dtype=p.dtype)
        return got, B.reading_order(n), B.debug_last_matches(n, dtype=p.dtype)
    first = seeded_call()
    plain = B.partial_chain(p.mb, p.scan, T=T, dtype=p.dtype)
    order_plain = B.reading_order(n)
    check_result(p, orc, plain, B.debug_last_matches(n, dtype=p.dtype), plain, T)
    again = seeded_call()
    for got, order, matches in (first, again):
        check_result(p, orc, got, matches, plain, T)
        if expect == "any":
            continue
        assert not np.array_equal(p.order_a, order_plain)            # (the two orders can be told apart)
        assert sorted(order) == list(range(n))
        if expect == "seeded":
            assert np.array_equal(order, p.order_a)
        else:
            assert np.array_equal(order, order_plain)
            assert got == plain, (got, plain)                        # (its own sort: the very same call)


# ---------------------------------------------------------------- sources that must be refused
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_map_destroyed(pair, oracle32, oracle64, dtype):
    p = pair(dtype)
    p.align()
    p.A.destroy_map(p.ma)
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


def _replace_map(p, xyz, nrm):
    p.A.destroy_map(p.ma)
    new = p.A.set_map(xyz.astype(p.dtype_a), nrm.astype(p.dtype_a), center=True, dtype=p.dtype_a)
    assert new == p.ma                                               # the freed id is handed out again


@pytest.mark.parametrize("dtype", DTYPES)
def test_b_id_reused_by_a_smaller_map(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    p.align()
    _replace_map(p, s["xa"][:300], s["na"][:300])
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_id_reused_by_a_map_of_the_same_size(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    p.align()
    perm = np.random.default_rng(5).permutation(len(s["xa"]))
    _replace_map(p, s["xa"][perm], s["na"][perm])
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_d_id_reused_by_a_map_twice_the_size(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    p.align()
    _replace_map(p, np.concatenate([s["xa"], s["xa"] + np.float32(0.01)]), np.concatenate([s["na"], s["na"]]))
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_e_id_filled_by_an_adopted_map(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    C = p.third()
    mc = C.set_map(s["xb"].astype(dtype), s["nb"].astype(dtype), center=True, dtype=dtype)
    p.align()
    p.A.destroy_map(p.ma)
    assert p.A.adopt_map(C, mc) == p.ma
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_f_map_transferred_away(pair, oracle32, oracle64, dtype):
    p = pair(dtype)
    C = p.third()
    p.align()
    C.adopt_map(p.A, p.ma)
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_g_source_aligned_with_knn_3(pair, oracle32, oracle64, dtype):
    p = pair(dtype, knn_a=3)
    p.align()
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_h_source_aligned_as_the_other_cloud_type(pair, oracle32, oracle64, dtype):
    p = pair(dtype, dtype_a=F64 if dtype == F32 else F32)
    p.align()
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_i_caller_names_itself(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    p.align()                                                        # (A's order: what a seeded probe would show)
    T, st = p.B.align(p.mb, p.scan, s["T0"], dtype=dtype)            # B aligns the scan against a map of its own
    assert st["status"] == 0
    p.T = T
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded", src=p.B)


@pytest.mark.parametrize("dtype", DTYPES)
def test_j_seventeen_segments(pair, oracle32, oracle64, dtype):
    p = pair(dtype)
    p.align()
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "unseeded", segs=split(*p.segs, 17))


# ---------------------------------------------------------------- sources that must stay seeded
@pytest.mark.parametrize("dtype", DTYPES)
def test_k_other_maps_of_the_source_come_and_go(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    p.align()
    x, n = s["xb"].astype(dtype), s["nb"].astype(dtype)
    one = p.A.set_map(x, n, center=True, dtype=dtype)
    two = p.A.set_map(x[:500], n[:500], center=False, dtype=dtype)
    assert len({one, two, p.ma}) == 3
    p.A.destroy_map(one)
    p.A.destroy_map(two)
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "seeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_l_source_ran_a_batch_with_the_scan_first(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    rds = [p.scan, p.scan[:1000], p.scan[300:1077]]
    Ts, sts = p.A.align_batch(p.ma, rds, [s["T0"]] * 3, dtype=dtype)
    assert all(st["status"] == 0 for st in sts)
    p.T, p.order_a = Ts[0], p.A.reading_order(N_SCAN, problem=0)
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "seeded")


@pytest.mark.parametrize("dtype", DTYPES)
def test_m_sixteen_segments(pair, oracle32, oracle64, dtype):
    p = pair(dtype)
    p.align()
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "seeded", segs=split(*p.segs, 16))


# ---------------------------------------------------------------- hostile tables: exact, whatever path
@pytest.mark.parametrize("dtype", DTYPES)
def test_n_a_reading_of_the_same_size_the_source_never_aligned(pair, oracle32, oracle64, dtype):
    p, s = pair(dtype), scene()
    p.align(reading=s["scan"][::-1].copy())                          # the same points in another order: every seed is another point's
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "any")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["o_gap", "p_beyond", "q_absent"])
def test_opq_hostile_segment_tables(pair, oracle32, oracle64, dtype, case):
    p = pair(dtype)
    p.align()
    m = 3 * N_KF
    segs = dict(o_gap=([500, N_KF, 2 * N_KF, m - 1000], p.segs[1]),              # indices below 500 and from 8 000 on lie in no segment
                p_beyond=(p.segs[0], [m - 100, 20_000, 2**31 - 1]),              # a segment that runs off B's map, two that lie beyond it
                q_absent=(p.segs[0], [-1, -1, -1]))[case]
    probe_thrice(p, orc_for(dtype, oracle32, oracle64), "any", segs=segs)


# ---------------------------------------------------------------- B's chain, on a valid source
VARIANTS = dict(
    robust_cauchy=(dict(trim_ratio=1.0, robust_fct=1, robust_tuning=1.0, robust_scale=1), SCAN),        # (test_gpu_chain.py's three settings;
    robust_huber=(dict(trim_ratio=1.0, robust_fct=6, robust_tuning=2.0, robust_scale=1), SCAN),         #  a sum of real-valued weights is the
    robust_tukey_none=(dict(trim_ratio=1.0, robust_fct=5, robust_tuning=0.3, robust_scale=0, robust_approx=0.25), SCAN),   # same double in scan order only)
    median_maxdist=(dict(trim_ratio=0.5, quantile_scale=3.0, outlier_max_dist=0.8), SORTED),            # (test_gpu_bit_exact.py's setting)
    no_trim=(dict(trim_ratio=1.0), SORTED),
    no_max_dist=(dict(max_dist=float("inf")), SORTED),
    p2point=(dict(error_minimizer=icp.MINIMIZER_POINT_TO_POINT), SORTED),                               # on a map without normals
    scan_order=(dict(), SCAN))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_chain_variant_first_capped_and_wrongly_capped(pair, oracle32, oracle64, dtype, name):
    over, sum_order = VARIANTS[name]
    orc = orc_for(dtype, oracle32, oracle64)
    p = pair(dtype, chain_b=dict(CHAIN, **over), sum_order=sum_order, normals_b=name != "p2point")
    T = p.align()
    # B's first probe (no cap), then with the cap of the plain probe at the same pose
    probe_thrice(p, orc, "seeded")
    B, n = p.B, N_SCAN
    T_off = T @ synth.se3(x=0.4, yaw=np.deg2rad(1.0))

    def at(pose, seeded):
        if seeded:
            got = B.partial_chain_seeded(p.mb, p.scan, pose, p.A, *p.segs, dtype=dtype)
            assert np.array_equal(B.reading_order(n), p.order_a)
        else:
            got = B.partial_chain(p.mb, p.scan, T=pose, dtype=dtype)
        return got, B.debug_last_matches(n, dtype=dtype)
    plain, _ = at(T, False)
    plain_off, m_plain_off = at(T_off, False)                        # the hint: 40 cm off, a threshold several times the one at T
    check_result(p, orc, plain_off, m_plain_off, plain_off, T_off)
    got, matches = at(T, True)                                       # a cap that is far too large
    check_result(p, orc, got, matches, plain, T)
    at(T, False)                                                     # the hint: the small threshold
    got, matches = at(T_off, True)                                   # a cap that is far too small
    check_result(p, orc, got, matches, plain_off, T_off)
