"""Scenes whose ICP arithmetic is exact, and their expected results in integer arithmetic.

The map is a planar lattice with dyadic coordinates and one constant dyadic normal; the reading's points stand straight above
lattice points at dyadic heights.  Then the nearest neighbour of a reading point is the lattice point below it (the next
candidate is a whole lattice step further: d2 = s^2 + dz^2 > dz^2), its squared distance is dz^2 exactly, and every product
and every partial sum of the error minimiser is a dyadic number that fits its format.  What such a scene must give -- the
order statistic of the outlier filter, the kept pairs, the 30 sums -- does not depend on any summation order and is written
here with Python integers and fractions.Fraction: no code, no reduction tree and no selection shared with the device
library or with oracle/icp_oracle.c.  The only floating-point operation on this side is the one the filter's definition
names: `values.size() * ratio` evaluated in T (expected_limit).

assert_exact() is the budget check: a scene that would need one bit more than its format has fails THERE, on the CPU, with
the offending quantity named -- never as a mismatch on the device.

Plain module: no GPU, no oracle import."""
import bisect
import math
from fractions import Fraction

import numpy as np

S = 0.125                      # lattice step
BIG_L = 208                    # 208 x 208 = 43 264 points: above the one-launch selection's 32 768
NORMAL_Z = (0.0, 0.0, 1.0)     # where only distances matter
NORMAL_SUM = (0.5, 0.25, 1.0)  # non-unit, off every axis: all 21 entries of A and all 6 of b are non-trivial
FAR_X = 300.0                  # a reading point shifted this far in x has no neighbour within MAX_DIST
MAX_DIST = 2.0
D0 = 2.0 ** -6                 # the reference height: d2 = 2^-12
K = 40                         # every input times 2^K is an integer (asserted)
MANT = {np.dtype(np.float32): 24, np.dtype(np.float64): 53}

PAIR_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 18433, 43264)
# reading points whose three pairs each cross the same edges (3 n around 64, 256, 1024, 2048, 16384, 18432, then nearly everything)
KNN3_SIZES = (1, 21, 22, 85, 86, 341, 342, 682, 683, 5461, 5462, 6144, 6145, 14283)


class Plane:
    """L x L lattice points (i s, j s, 0), stored in a shuffled order (fixed seed); at(i, j) is the index of a lattice point"""

    def __init__(self, L, s=S, normal=NORMAL_Z, seed=15):
        self.L, self.s = L, s
        ii, jj = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
        perm = np.random.default_rng(seed).permutation(L * L)
        self.i, self.j = ii.ravel()[perm], jj.ravel()[perm]
        self.ref = np.stack([self.i * s, self.j * s, np.zeros(L * L)], 1).astype(np.float64)
        self.nrm = np.tile(np.asarray(normal, dtype=np.float64), (L * L, 1))
        self._at = np.empty((L, L), dtype=np.int64)
        self._at[self.i, self.j] = np.arange(L * L)

    def at(self, i, j):
        return self._at[i, j]

    def block(self, ni, nj, i0=0, j0=0):
        """indices of the ni x nj sub-lattice at (i0, j0), row by row"""
        ii, jj = np.meshgrid(np.arange(i0, i0 + ni), np.arange(j0, j0 + nj), indexing="ij")
        return self._at[ii.ravel(), jj.ravel()]

    def parity(self, idx):
        """+1 / -1 by the checkerboard colour of lattice points `idx`"""
        return np.where((self.i[idx] + self.j[idx]) % 2 == 0, 1.0, -1.0)


class Scene:
    """ref / nrm: the map; reading (n, 3); ids (n,) or (n, k): the expected neighbours, -1 where there is none; all float64 arrays of
    dyadic numbers (a test casts them to its T: exact, assert_exact checks it)"""

    def __init__(self, plane, reading, ids, reading_nrm=None, note=""):
        self.plane, self.ref, self.nrm = plane, plane.ref, plane.nrm
        self.reading = np.ascontiguousarray(reading, dtype=np.float64)
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        self.reading_nrm = reading_nrm
        self.note = note

    @property
    def n(self):
        return self.reading.shape[0]

    @property
    def knn(self):
        return 1 if self.ids.ndim == 1 else self.ids.shape[1]

    def pairs(self):
        """(p, q, nrm, has) per pair, [point][neighbour]: p the reading point, q / nrm the neighbour (row 0 where there is none)"""
        ids = self.ids.reshape(self.n, -1)
        k = ids.shape[1]
        p = np.repeat(self.reading, k, axis=0)
        flat = ids.ravel()
        has = flat >= 0
        safe = np.where(has, flat, 0)
        return p, self.ref[safe], self.nrm[safe], has

    def d2_int(self):
        """squared distance of every pair times 2^(2K), a Python integer; None where there is no neighbour"""
        p, q, _, has = self.pairs()
        d = _ints(p) - _ints(q)
        d2 = (d * d).sum(axis=1)
        return [int(v) if h else None for v, h in zip(d2, has)]

    def d2_float(self):
        """the same as float64 (exact: assert_exact), +inf where there is no neighbour; shape of ids"""
        out = np.array([math.inf if v is None else float(Fraction(v, 1 << (2 * K))) for v in self.d2_int()])
        return out.reshape(self.ids.shape)


def lift(plane, idx, dz, far=None, note=""):
    """reading points above lattice points `idx` at heights `dz`; `far`: boolean mask of points shifted by FAR_X in x (no neighbour)"""
    idx = np.asarray(idx, dtype=np.int64)
    rd = plane.ref[idx].copy()
    rd[:, 2] += np.broadcast_to(np.asarray(dz, dtype=np.float64), idx.shape)
    ids = idx.copy()
    if far is not None:
        rd[far, 0] += FAR_X
        ids[far] = -1
    return Scene(plane, rd, ids, note=note)


def lift_knn3(plane, idx, dz, note=""):
    """Three exact, tie-free neighbours per reading point: the point stands at (+3/8 s, +1/8 s, dz) from lattice point (i, j),
    i, j < L - 1.  With 0 < ey < ex < s / 2 the squared horizontal distances order strictly: own ex^2 + ey^2 < (i+1, j):
    (s-ex)^2 + ey^2 < (i, j+1): ex^2 + (s-ey)^2 < every other lattice point ((i-1, j): (s+ex)^2 + ey^2 and the diagonal
    (s-ex)^2 + (s-ey)^2 are both larger) -- and the common dz^2 does not change the order."""
    idx = np.asarray(idx, dtype=np.int64)
    i, j = plane.i[idx], plane.j[idx]
    assert np.all(i < plane.L - 1) and np.all(j < plane.L - 1)
    rd = plane.ref[idx].copy()
    rd[:, 0] += 3 * plane.s / 8
    rd[:, 1] += plane.s / 8
    rd[:, 2] += np.broadcast_to(np.asarray(dz, dtype=np.float64), idx.shape)
    ids = np.stack([idx, plane.at(i + 1, j), plane.at(i, j + 1)], 1)
    return Scene(plane, rd, ids, note=note)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def select_rank(n_finite, ratio, T):
    """index of the order statistic: `int(values.size() * ratio)` evaluated in T, clamped; a ratio of exactly 1 is the last element"""
    T = np.dtype(T).type
    if T(ratio) == T(1):
        return n_finite - 1
    return max(0, min(int(T(n_finite) * T(ratio)), n_finite - 1))


def expected_limit(d2, ratio, T):
    """d2: exact squared distances (any exact comparable numbers), None where there is no neighbour.
    Returns (limit, n_finite, n_kept = #(d2 <= limit)); limit None when nothing is finite."""
    fin = sorted(v for v in d2 if v is not None)
    if not fin:
        return None, 0, 0
    limit = fin[select_rank(len(fin), ratio, T)]
    return limit, len(fin), bisect.bisect_right(fin, limit)


def _ints(a):
    """float64 array times 2^K as Python integers (object array); the inputs are dyadic with at most K fractional bits"""
    a = np.asarray(a, dtype=np.float64)
    v = np.ldexp(a, K)
    assert np.all(np.isfinite(v)) and np.all(v == np.rint(v)) and np.all(np.abs(v) < 2.0 ** 53), "not a dyadic number within 2^-K"
    return np.array([int(x) for x in v.ravel()], dtype=object).reshape(a.shape)


def _terms(p, q, n, w, minimizer):
    """per-pair terms of the 30 sums as integer columns with their scales: list of (column, power of 2^K)"""
    P, Q, N, W = _ints(p), _ints(q), _ints(n), _ints(w)
    one = 1 << K
    cols = []
    if minimizer == 0:
        d = P - Q
        e = (N * d).sum(axis=1)                                          # 2K
        J = [P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1], P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2], P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0],
             N[:, 0] * one, N[:, 1] * one, N[:, 2] * one]                # 2K each
        for a in range(6):
            for b in range(a, 6):
                cols.append((W * (J[a] * J[b]), 5))
        for a in range(6):
            cols.append((-(W * (J[a] * e)), 5))
        cols += [(W, 1), (W * 0 + 1, 0), (W * (e * e), 5)]
        inter = [(J[a], 2) for a in range(6)] + [(e, 2)] + [(J[a] * J[b], 4) for a in range(6) for b in range(a, 6)] + \
                [(J[a] * e, 4) for a in range(6)] + [(e * e, 4)]
    else:
        for a in range(3):
            cols.append((W * P[:, a], 2))
        for a in range(3):
            cols.append((W * Q[:, a], 2))
        for a in range(3):
            for b in range(3):
                cols.append((W * (Q[:, a] * P[:, b]), 3))
        cols += [(W * 0, 0)] * 12
        d = P - Q
        dd = (d * d).sum(axis=1)                                         # 2K
        root = np.array([math.isqrt(int(v)) for v in dd], dtype=object)  # K
        assert np.all(root * root == dd), "point-to-point residual: |p - q| is not a dyadic number"
        cols += [(W, 1), (W * 0 + 1, 0), (root, 1)]
        inter = [(Q[:, a] * P[:, b], 2) for a in range(3) for b in range(3)] + [(dd, 2)]
    return cols, inter


def expected_sums(p, q, n, w, minimizer=0, prefixes=None):
    """The 30 values of kSys over the pairs with w != 0 (p, q, n: (N, 3) per pair; w: (N,)), as Fractions.
    minimizer 0: point-to-plane (21 upper entries of A = sum w J J^T, 6 of b = -sum w J e, sum w, pairs, sum w e^2 with
    J = (p x n, n), e = n . (p - q)); 1: point-to-point (sum w p, sum w q, sum w q p^T, twelve zeros, sum w, pairs, sum |p - q|).
    prefixes: a list of pair counts -> {count: the 30 sums over the first `count` pairs} from one pass."""
    w = np.asarray(w, dtype=np.float64)
    use = w != 0
    cols, _ = _terms(p, q, n, w, minimizer)
    usei = np.array([1 if u else 0 for u in use], dtype=object)
    out = {}
    acc = [np.cumsum(c * usei) if prefixes is not None else None for c, _ in cols]
    for cnt in (prefixes if prefixes is not None else [len(w)]):
        if prefixes is not None:
            out[cnt] = [Fraction(int(a[cnt - 1]), 1 << (K * s)) for a, (_, s) in zip(acc, cols)]
        else:
            out[cnt] = [Fraction(int((c * usei).sum()), 1 << (K * s)) for c, s in cols]
    return out if prefixes is not None else out[len(w)]


def to_floats(fracs):
    """Fractions -> float64, once; every value must be representable (assert_exact proved it before)"""
    out = np.array([float(f) for f in fracs], dtype=np.float64)
    assert all(Fraction(float(v)) == f for v, f in zip(out, fracs)), "an expected sum is not a double"
    return out


# ---- the guard ------------------------------------------------------------------------------------------------------------------
def _bits(v):
    """significant bits of an integer (trailing zeros do not count)"""
    v = abs(int(v))
    return 0 if v == 0 else v.bit_length() - ((v & -v).bit_length() - 1)


def _max_bits(col):
    return max((_bits(v) for v in set(np.asarray(col, dtype=object).ravel().tolist())), default=0)


def _sum_bits(col):
    """bits the worst partial sum of a column can need in ANY order: sum |term| in units of the finest term"""
    vals = [abs(v) for v in np.asarray(col, dtype=object).ravel().tolist() if v != 0]
    if not vals:
        return 0
    unit = min((v & -v).bit_length() - 1 for v in set(vals))
    return (sum(vals) >> unit).bit_length()


def assert_exact_in_T(scene, T, w=None, what=""):
    """every coordinate, weight, difference, square and squared distance the device computes in T needs at most T's significand
    (24 bits / 53 bits) and survives the cast to T.  Integers only."""
    mt = MANT[np.dtype(T)]
    tag = (what or scene.note, np.dtype(T).name)
    for name, a in (("map", scene.ref), ("normal", scene.nrm), ("reading", scene.reading), ("reading normal", scene.reading_nrm)):
        if a is not None:
            assert _max_bits(_ints(a)) <= mt, (tag, name, "coordinate bits", _max_bits(_ints(a)))
            assert np.array_equal(np.asarray(a, dtype=T).astype(np.float64), a), (tag, name, "does not survive the cast")
    p, q, _, has = scene.pairs()
    d = _ints(p[has]) - _ints(q[has])
    sq = d * d
    assert _max_bits(d) <= mt and _max_bits(sq) <= mt, (tag, "difference / square bits", _max_bits(d), _max_bits(sq))
    assert _max_bits(sq[:, 0] + sq[:, 1]) <= mt and _max_bits(sq.sum(axis=1)) <= mt, (tag, "squared distance bits")
    if w is not None:
        assert _max_bits(_ints(w)) <= mt, (tag, "weight bits")


def assert_exact_sums(scene, w=None, minimizers=(0, 1), what=""):
    """every product of accumulate_pair (computed in double whatever T is) and every total of the 30 sums -- in whatever order
    the pairs are added -- needs at most 53 bits.  Integers only.  w: the pairs' weights (default 1); pairs without a neighbour
    do not enter."""
    tag = what or scene.note
    p, q, n, has = scene.pairs()
    ww = np.ones(int(has.sum())) if w is None else np.asarray(w, dtype=np.float64).ravel()[has]
    for m in minimizers:
        cols, inter = _terms(p[has], q[has], n[has], ww, m)
        for k, (c, _) in enumerate(inter):
            assert _max_bits(c) <= 53, (tag, "minimizer", m, "intermediate", k, _max_bits(c))
        for k, (c, _) in enumerate(cols):
            assert _max_bits(c) <= 53 and _sum_bits(c) <= 53, (tag, "minimizer", m, "sum", k, _max_bits(c), _sum_bits(c))


def assert_exact(scene, T, w=None, minimizers=(0, 1), what=""):
    """the guard: a scene outside the budget of its formats fails here, on the CPU, and never as a device mismatch"""
    assert_exact_in_T(scene, T, w, what)
    if minimizers:
        assert_exact_sums(scene, w, minimizers, what)


# ---- the heights the GPU tests use ----------------------------------------------------------------------------------------------
# (dz has at most 12 significant bits so that dz^2 is exact in float32; the band of a hinted first selection around h = D0^2 is
#  [h / 4, 4 h]: heights D0 / 2 ... 2 D0)
DZ_FAR_BELOW = D0 / 4                          # d2 = h / 16
DZ_BELOW = D0 / 2 * (1 - 2.0 ** -12)           # the largest 12-bit height below D0 / 2: just under the band
DZ_LO = D0 / 2                                 # d2 = h / 4: the band's low edge
DZ_HI = 2 * D0                                 # d2 = 4 h: the band's high edge
DZ_ABOVE = 2 * D0 * (1 + 2.0 ** -11)           # the smallest 12-bit height above 2 D0: just over the band
DZ_FAR_ABOVE = 3 * D0


def shuffled(values, seed=3):
    v = np.asarray(values, dtype=np.float64)
    return v[np.random.default_rng(seed).permutation(len(v))]


def counts(*value_count):
    """heights from (value, count) runs, shuffled"""
    return shuffled(np.concatenate([np.full(c, v) for v, c in value_count if c > 0]))


def ramp(n, T, narrow=False):
    """n heights rising from D0, every distinct value repeated equally often, shuffled.
    Wide: over [D0, 2 D0), 32 of the band's slices (a slice of the band [h / 4, 4 h] is a 16th of an octave of d2: 3.08 % in
    dz).  float64: n distinct values D0 (1 + i 2^-16).  float32: a square is exact only for a 12-bit height, so 2 048
    distinct values D0 (1 + j 2^-11).
    Narrow: everything in ONE slice.  float64: 6 144 distinct values D0 (1 + j 2^-18), + 2.3 % -- more than the 4 096 keys the
    final stage holds in LDS, and 18 bits so that the sum of the squares still fits a double.  float32: the 60 distinct
    12-bit values within + 2.9 % (more than 8 192 DISTINCT float keys in one slice cannot have exact squares)."""
    i = np.arange(n, dtype=np.float64)
    if np.dtype(T) == np.float64:
        distinct, step = (6144, 2.0 ** -18) if narrow else (n, 2.0 ** -16)
    else:
        distinct, step = (60, 2.0 ** -11) if narrow else (2048, 2.0 ** -11)
    distinct = min(distinct, n)
    return shuffled(D0 * (1 + np.floor(i * distinct / n) * step))


def small_idx(plane, n):
    """the small readings beside a big one: sub-lattices with even sides (a checkerboard on them cancels), 2 049 = 32 x 64 + 1"""
    if n == 64:
        return plane.block(8, 8, 3, 5)
    if n == 5000:
        return plane.block(50, 100, 7, 9)
    if n == 2049:
        return np.concatenate([plane.block(32, 64, 100, 100), plane.block(1, 1, 0, 0)])
    raise ValueError(n)


def dist_one(n, T=None):
    return np.full(n, D0)


def dist_two(n, ratio, T, rank_on_upper):
    """two heights split exactly at the rank: it falls on the last point of the lower height, or on the first of the upper one"""
    k = select_rank(n, ratio, T)
    lower = k if rank_on_upper else k + 1
    return counts((D0, lower), (DZ_HI, n - lower))


def weights_pattern(n):
    """about one weight in seven zero, the others 1, 1/2, 1/4"""
    i = np.arange(n)
    return np.where(i % 7 == 3, 0.0, np.choose(i % 3, [1.0, 0.5, 0.25]))


def heights_pattern(n):
    """small signed heights, 5 bits: (i * 7 mod 31 - 15) / 512, never above 15 / 512 < s / 2"""
    i = np.arange(n)
    return ((i * 7) % 31 - 15) / 512.0


# ---- the batches the GPU tests run (tests/test_exact_scenes_host.py checks every one of them against the guard and the oracle) ----
_PLANES = {}


def big_plane(normal=NORMAL_Z):
    if normal not in _PLANES:
        _PLANES[normal] = Plane(BIG_L, S, normal)
    return _PLANES[normal]


BATCH_SIZES = (BIG_L * BIG_L, BIG_L * BIG_L, 5000, 64)          # P = 4: big, big, 5 000, 64
RATIOS = (0.85, 0.5, 0.999, 1.0, 0.01)
SELECTION_KINDS = ("one_value", "two_values_rank_on_lower", "two_values_rank_on_upper", "ramp", "ramp_one_in_nine_without_neighbour")


def _idx(plane, n):
    return np.arange(n) if n == plane.L * plane.L else small_idx(plane, n)


def selection_batch(kind, ratio, T):
    """test A: four readings (BATCH_SIZES) with the same kind of distance distribution"""
    pl = big_plane()
    out = []
    for n in BATCH_SIZES:
        far = None
        if kind == "one_value":
            dz = dist_one(n)
        elif kind.startswith("two_values"):
            dz = dist_two(n, ratio, T, kind.endswith("upper"))
        else:
            dz = ramp(n, T)
            if kind != "ramp":
                far = np.arange(n) % 9 == 4
                if far.all():
                    far[0] = False
        out.append(lift(pl, _idx(pl, n), dz, far, note=f"A/{kind}/{ratio}/{n}"))
    return out


def primer_batch(sizes=BATCH_SIZES):
    """every height D0: the selections of this call leave the hint h = D0^2 for every problem index"""
    pl = big_plane()
    return [lift(pl, _idx(pl, n), dist_one(n), note=f"primer/{n}") for n in sizes]


BAND_RATIO = 0.5
# case -> does the big reading's rank lie outside the band [h / 4, 4 h] (the fallback over everything must run), by construction
BAND_CASES = {"rank_on_low_edge": False, "rank_just_below_band": True, "rank_on_high_edge": False, "rank_just_above_band": True,
              "all_equal": False, "narrow_ramp": False, "wide_ramp": False}


def band_batch(case, T):
    """test B: the second call's readings.  Problem 0 (big) carries the designed distribution; the other three keep every height
    at D0 (rank inside the band), so a fallback counted is problem 0's.  With BAND_RATIO = 0.5 the rank is k = n / 2 exactly."""
    pl = big_plane()
    n = BATCH_SIZES[0]
    k = select_rank(n, BAND_RATIO, T)
    if case == "rank_on_low_edge":            # k keys below the band, then the band's first key h / 4 at rank k: below == k
        dz = counts((DZ_FAR_BELOW, k), (DZ_LO, 100), (D0, n - k - 100))
    elif case == "rank_just_below_band":      # the largest key below h / 4 at rank k = below - 1
        dz = counts((DZ_FAR_BELOW, k), (DZ_BELOW, 1), (D0, n - k - 1))
    elif case == "rank_on_high_edge":         # the band's last key 4 h at rank k = below + cnt - 1
        dz = counts((D0, k - 99), (DZ_HI, 100), (DZ_ABOVE, 1), (DZ_FAR_ABOVE, n - k - 2))
    elif case == "rank_just_above_band":      # the smallest key above 4 h at rank k = below + cnt
        dz = counts((D0, k), (DZ_ABOVE, 1), (DZ_FAR_ABOVE, n - k - 1))
    elif case == "all_equal":                 # 43 264 keys in one slice: over kSelSubCap in both precisions; the 5 000-point
        dz = dist_one(n)                      # problem beside it: under the float32 cap (8 192), over the float64 cap (4 096)
    elif case == "narrow_ramp":               # one slice holds everything
        dz = ramp(n, T, narrow=True)
    elif case == "wide_ramp":                 # 32 slices of ~1 350 keys: the select inside LDS
        dz = ramp(n, T)
    else:
        raise ValueError(case)
    first = lift(pl, _idx(pl, n), dz, note=f"B/{case}")
    return [first] + primer_batch()[1:]


def checkerboard_batch():
    """test C: +D0 / -D0 alternating over the lattice, normal (0, 0, 1): J e of the kept pairs cancels exactly (every reading is a
    sub-lattice with even sides, all its pairs tie at D0^2 and are kept), so b = 0 and T stays the identity"""
    pl = big_plane()
    return [lift(pl, _idx(pl, n), D0 * pl.parity(_idx(pl, n)), note=f"C/checkerboard/{n}") for n in BATCH_SIZES]


def zero_batch(zero_at):
    """test C: the all-zero reading (reading = map points: limit 0, band [0, 0]) as problem `zero_at`, checkerboards beside it"""
    pl = big_plane()
    out = checkerboard_batch()
    n = BATCH_SIZES[zero_at]
    out[zero_at] = lift(pl, _idx(pl, n), np.zeros(n), note=f"C/zero/{n}")
    return out


STAGE_P = 256


def stage_batch():
    """test D: one big all-equal reading and 255 readings of 64 points"""
    pl = big_plane()
    n = BIG_L * BIG_L
    small = lift(pl, small_idx(pl, 64), dist_one(64), note="D/64")
    return [lift(pl, _idx(pl, n), dist_one(n), note="D/big")] + [small] * (STAGE_P - 1)


def sums_scene(n=BIG_L * BIG_L):
    """test E: the first n lattice points in map order, signed 5-bit heights, the off-axis normal"""
    pl = big_plane(NORMAL_SUM)
    return lift(pl, np.arange(n), heights_pattern(n), note=f"E/sums/{n}")


CHAIN_RATIO = 0.75


def chain_scene(n):
    """test E through the whole chain: one point in seven without a neighbour; of the others the quantile filter (CHAIN_RATIO)
    keeps those up to the order statistic"""
    pl = big_plane(NORMAL_SUM)
    far = np.arange(n) % 7 == 3
    if far.all():
        far[:] = False
    return lift(pl, np.arange(n), heights_pattern(n), far, note=f"E/chain/{n}")


def knn3_scene(n):
    pl = big_plane(NORMAL_SUM)
    inner = np.flatnonzero((pl.i < pl.L - 1) & (pl.j < pl.L - 1))[:n]
    assert len(inner) == n
    return lift_knn3(pl, inner, heights_pattern(n), note=f"E/knn3/{n}")


NORMAL_MAX_ANGLE = 0.5      # radians; cos = 0.8776


def angle_scene(n):
    """reading normals either the map's own (angle 0: clearly inside NORMAL_MAX_ANGLE) or (1, 0, 0) (cos = 0.5 / |(0.5, 0.25, 1)|
    = 0.436, 64 degrees: clearly outside); no pair is near the cosine"""
    sc = chain_scene(n)
    out = np.arange(n) % 5 == 2
    sc.reading_nrm = np.where(out[:, None], np.array([1.0, 0.0, 0.0]), np.asarray(NORMAL_SUM))
    sc.angle_inside = ~out
    sc.note = f"E/angle/{n}"
    return sc


def chain_expectation(sc, ratio, T, extra_keep=None):
    """what one pass of the chain over `sc` must give: (limit as Fraction or None, n_finite, kept mask per pair, the 30 sums as
    Fractions); extra_keep: a further 0 / 1 filter per pair (the normal filter)"""
    d2 = sc.d2_int()
    limit, nf, _ = expected_limit(d2, ratio, T)
    keep = np.array([v is not None and limit is not None and v <= limit for v in d2])
    if extra_keep is not None:
        keep &= np.repeat(np.asarray(extra_keep, dtype=bool), sc.knn)
    p, q, nr, _ = sc.pairs()
    sums = expected_sums(p, q, nr, keep.astype(np.float64))
    return (None if limit is None else Fraction(limit, 1 << (2 * K))), nf, keep, sums
