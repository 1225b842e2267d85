"""Scenes that consist of nothing but ties and near-ties, and what the matcher must give on them.

The arithmetic contract makes a neighbour the argmin over (d2, original index).  Real scans rarely tie (the tie
census), so these scenes tie everywhere: queries at the centres, edge midpoints and corners of a dyadic lattice that is stored
in a shuffled order -- "lowest index" is then a different corner for every query --, the same queries nudged by the smallest
dyadic step whose arithmetic is still exact in T (a unique winner by the smallest exact margin), shells of equidistant points
cut by knn, and two families whose distances are NOT exact: lattice queries moved by a few ulps, and pairs of map points at
nearly the same distance from their query, far from the origin (the adversary of the double matcher's float prefilter).

Exact scenes: the expectation is integer arithmetic over the whole lattice (int_knn).  Rounded scenes: the expectation is the
contract's arithmetic evaluated elementwise in T by numpy (brute_in_T).  Neither shares code with the device library or with
oracle/icp_oracle.c; tests/test_tie_scenes_host.py holds both against the oracle.

Plain module: no GPU, no oracle import."""
import functools
import types

import numpy as np

from exact_scenes import K, NORMAL_Z, S, Plane, Scene, assert_exact_in_T

P_L = 48                              # plane P48: 2 304 points
C_L = 16                              # cube C16: 4 096 points
HEIGHTS = (0, 1, 4, 16, 64)           # query heights over the plane, in lattice steps
PLANE_KINDS = ("C4", "E2", "N1", "N2", "V0")
CUBE_KINDS = ("CC8", "F4", "E2", "CN1", "CN4")
KNNS = (2, 4, 5, 9, 16)
KNN_KINDS = ("C4", "N1")
TYPES = (np.float32, np.float64)
OFFSETS = (0.0, 3.0e3, 4.0e5)         # D-pairs: the offsets of test_double_clouds_far_from_the_origin_match_bit_for_bit
D_QUERIES, D_DUPLICATES = 4000, 200
ICP_SHIFT = (0.25, -0.5, 0.0)         # dyadic, lattice aligned (2 and -4 steps)
ICP_CHAIN = dict(max_dist=2.0, trim_ratio=1.0, max_iters=30, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=3, sensor_std_dev=0.01)
_STEP_BITS = 3
assert S == 2.0 ** -_STEP_BITS


class Cube:
    """L x L x L lattice points (i s, j s, k s) stored in a shuffled order (fixed seed); the interface Scene asks of a map"""

    def __init__(self, L, s=S, seed=16):
        self.L, self.s = L, s
        g = np.stack(np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij"), -1).reshape(-1, 3)
        self.ijk = g[np.random.default_rng(seed).permutation(L ** 3)]
        self.ref = (self.ijk * s).astype(np.float64)
        self.nrm = np.tile(np.asarray(NORMAL_Z, dtype=np.float64), (L ** 3, 1))


@functools.lru_cache(maxsize=None)
def plane():
    return Plane(P_L)


@functools.lru_cache(maxsize=None)
def cube():
    return Cube(C_L)


# ---- the expectation of an exact scene: integers ----------------------------------------------------------------------------------
def int_knn(q, m, knn=1, s=S):
    """ids (n,) / (n, knn): the first knn map points by (exact squared distance, index), over the whole map, in int64.
    With m = M s (M integer) and q = Q 2^-kk (Q integer, kk >= 3) the squared distance is
    |q|^2 + 2^-2kk 2^(kk-3) (|M|^2 2^(kk-3) - 2 Q.M): for one query the order of the points is the order of the bracket, an
    integer far below 2^62 (asserted) where the squared distance itself, at 2^-2kk, would not fit a word."""
    q, m = np.asarray(q, dtype=np.float64), np.asarray(m, dtype=np.float64)
    M = m / s
    assert np.array_equal(M, np.rint(M)), "the map is not on the lattice"
    M = M.astype(np.int64)
    for kk in range(_STEP_BITS, K + 1):
        v = np.ldexp(q, kk)
        if np.array_equal(v, np.rint(v)):
            break
    else:
        raise AssertionError("a query coordinate is not a dyadic number within 2^-K")
    Q = v.astype(np.int64)
    sh = kk - _STEP_BITS
    m2 = (M * M).sum(axis=1) << sh
    bound = int(m2.max()) + 2 * sum(int(np.abs(Q[:, a]).max()) * int(np.abs(M[:, a]).max()) for a in range(3))
    assert bound < 2 ** 62, "the order key does not fit int64"
    N = M.shape[0]
    packed = bound * N < 2 ** 62                       # (key, index) in one word: a partition instead of a stable sort
    out = np.empty((q.shape[0], knn), dtype=np.int64)
    axes = [a for a in range(3) if M[:, a].any() and Q[:, a].any()]
    cols = [np.ascontiguousarray(-2 * M[:, a])[None, :] for a in axes]
    rows = 256                                         # (a block and its scratch stay in the cache)
    tmp = np.empty((rows, N), dtype=np.int64)
    for a in range(0, q.shape[0], rows):
        Qc = Q[a:a + rows]
        key = np.repeat(m2[None, :], len(Qc), axis=0)
        for ax, col in zip(axes, cols):
            key += np.multiply(Qc[:, ax:ax + 1], col, out=tmp[:len(Qc)])
        if knn == 1:
            out[a:a + rows, 0] = np.argmin(key, axis=1)            # (the first occurrence of the minimum: the lowest index)
        elif packed:
            key *= N
            key += np.arange(N)[None, :]
            out[a:a + rows] = np.sort(np.partition(key, knn - 1, axis=1)[:, :knn], axis=1) % N
        else:
            out[a:a + rows] = np.argsort(key, axis=1, kind="stable")[:, :knn]
    return out[:, 0] if knn == 1 else out


def _scene(mp, q, knn, note, **tags):
    sc = Scene(mp, q, int_knn(q, mp.ref, knn), note=note)
    for k, v in tags.items():
        setattr(sc, k, v)
    return sc


def budget_k(mp, base, step, competitors, T):
    """the largest k for which the queries base + step 2^-k are exact in T against every competitor (assert_exact_in_T: every
    coordinate, difference, square and partial sum fits T's significand).  competitors: (n, c) map indices -- the tied points the
    nudge decides between, not only the winner.  More bits for a larger k: a bisection."""
    def fits(k):
        try:
            assert_exact_in_T(Scene(mp, base + step * 2.0 ** -k, competitors), T)
        except AssertionError:
            return False
        return True
    lo, hi = _STEP_BITS + 2, K                         # (2^-5: a quarter of a step -- the nudge stays inside its square)
    assert fits(lo), "no budget for a nudge"
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
    return lo


# ---- plane P48 --------------------------------------------------------------------------------------------------------------------
def _squares(L):
    i, j = np.meshgrid(np.arange(L - 1), np.arange(L - 1), indexing="ij")
    return i.ravel().astype(np.float64), j.ravel().astype(np.float64)


def _plane_base(kind, h):
    """(queries before any nudge, nudge direction per query or None)"""
    pl = plane()
    i, j = _squares(pl.L)
    z = np.full(i.shape, float(h))
    half = np.full(i.shape, 0.5)
    zero = np.zeros(i.shape)
    step = None
    if kind in ("C4", "N1", "N2"):
        q = np.stack([i + half, j + half, z], 1)
        if kind == "N1":                               # toward one corner, drawn per query: all four occur
            sg = np.random.default_rng(100 + h).integers(0, 2, size=(len(i), 2)) * 2.0 - 1.0
            step = np.concatenate([sg, zero[:, None]], 1)
        elif kind == "N2":
            step = np.stack([half * 2, zero, zero], 1)
    elif kind == "E2":                                 # an edge along x or along y, by the square's colour: a tie inside a row, a tie across two
        along_x = (i + j) % 2 == 0
        q = np.stack([i + np.where(along_x, half, zero), j + np.where(along_x, zero, half), z], 1)
    elif kind == "V0":
        q = np.stack([i, j, z], 1)
    else:
        raise ValueError(kind)
    return q * pl.s, step


@functools.lru_cache(maxsize=None)
def _corners(h, c=4):
    """the c nearest lattice points of every square's centre at height h: the points a nudge of the centre decides between"""
    return int_knn(_plane_base("C4", h)[0], plane().ref, c)


@functools.lru_cache(maxsize=None)
def _plane_scene(kind, h, tname):
    pl = plane()
    base, step = _plane_base(kind, h)
    if step is None:
        return _scene(pl, base, 1, f"P48/{kind}/z={h}s", kind=kind, h=h, k=None)
    k = budget_k(pl, base, step, _corners(h), np.dtype(tname))
    return _scene(pl, base + step * 2.0 ** -k, 1, f"P48/{kind}/z={h}s/{tname}/k={k}", kind=kind, h=h, k=k)


def plane_scene(kind, h, T):
    """one kind of query over every square of P48 at height h steps; N1 / N2 carry their nudge exponent as .k"""
    return _plane_scene(kind, h, np.dtype(T).name if kind in ("N1", "N2") else "")


def join(scenes, note):
    """several scenes over one map as one (one matcher call); .parts: (note, slice) of every member"""
    sc = Scene(scenes[0].plane, np.concatenate([s.reading for s in scenes]), np.concatenate([s.ids for s in scenes]), note=note)
    sc.parts, a = [], 0
    for s in scenes:
        assert s.plane is scenes[0].plane and s.knn == scenes[0].knn
        sc.parts.append((s.note, slice(a, a + s.n)))
        a += s.n
    return sc


def plane_layer(h, T):
    """every kind at one height"""
    sc = join([plane_scene(kind, h, T) for kind in PLANE_KINDS], f"P48/z={h}s/{np.dtype(T).name}")
    sc.h = h
    return sc


@functools.lru_cache(maxsize=None)
def _knn16(kind, tname):
    """(queries, their first sixteen neighbours, nudge exponent): the shells around a square's centre hold 4, 8, 4, 8 ... points,
    sixteen are three whole shells -- the competitors of the budget and every list up to knn 16"""
    pl = plane()
    base, step = _plane_base(kind, 0)
    if step is None:
        return base, _corners(0, 16), None
    k = budget_k(pl, base, step, _corners(0, 16), np.dtype(tname))
    q = base + step * 2.0 ** -k
    return q, int_knn(q, pl.ref, 16), k


@functools.lru_cache(maxsize=None)
def _knn_scene(kind, knn, tname):
    q, ids, k = _knn16(kind, tname)
    sc = Scene(plane(), q, ids[:, :knn], note=f"P48/{kind}/knn={knn}" + (f"/{tname}/k={k}" if k else ""))
    sc.kind, sc.k = kind, k
    return sc


def knn_scene(kind, knn, T):
    return _knn_scene(kind, knn, np.dtype(T).name if kind == "N1" else "")


# ---- cube C16 ---------------------------------------------------------------------------------------------------------------------
def _cube_base(kind):
    cb = cube()
    L = cb.L
    cell, node = np.arange(L - 1) + 0.5, np.arange(L, dtype=np.float64)

    def grid(*axes):
        return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    step = None
    if kind in ("CC8", "CN1", "CN4"):
        q = grid(cell, cell, cell)
        rng = np.random.default_rng({"CC8": 200, "CN1": 201, "CN4": 204}[kind])
        if kind == "CN1":                              # toward one of the eight corners
            step = rng.integers(0, 2, size=q.shape) * 2.0 - 1.0
        elif kind == "CN4":                            # along one axis, either way: the four corners of one face stay tied
            step = np.zeros(q.shape)
            step[np.arange(len(q)), rng.integers(0, 3, size=len(q))] = rng.integers(0, 2, size=len(q)) * 2.0 - 1.0
    elif kind == "F4":                                 # the centres of the faces, every orientation
        q = np.concatenate([grid(node, cell, cell), grid(cell, node, cell), grid(cell, cell, node)])
    elif kind == "E2":                                 # the midpoints of the edges, every orientation
        q = np.concatenate([grid(cell, node, node), grid(node, cell, node), grid(node, node, cell)])
    else:
        raise ValueError(kind)
    return q * cb.s, step


@functools.lru_cache(maxsize=None)
def _cube_scene(kind, tname):
    cb = cube()
    base, step = _cube_base(kind)
    if step is None:
        return _scene(cb, base, 1, f"C16/{kind}", kind=kind, k=None)
    k = budget_k(cb, base, step, int_knn(base, cb.ref, 8), np.dtype(tname))
    return _scene(cb, base + step * 2.0 ** -k, 1, f"C16/{kind}/{tname}/k={k}", kind=kind, k=k)


def cube_scene(kind, T):
    return _cube_scene(kind, np.dtype(T).name if kind in ("CN1", "CN4") else "")


def cube_all(T):
    return join([cube_scene(kind, T) for kind in CUBE_KINDS], f"C16/{np.dtype(T).name}")


def exact_scenes(T):
    """every exact scene, one by one (the host test's list)"""
    return [plane_scene(kind, h, T) for h in HEIGHTS for kind in PLANE_KINDS] + [cube_scene(kind, T) for kind in CUBE_KINDS] + \
           [knn_scene(kind, knn, T) for kind in KNN_KINDS for knn in KNNS]


# ---- the ICP scene: C4 at z = 0 behind a lattice-aligned translation ----------------------------------------------------------------
def icp_scene():
    """(reading, T_init, the C4 scene): the reading is the C4 queries shifted by -ICP_SHIFT and T_init shifts it back.  Every
    point-to-plane error is exactly 0 whichever tied corner is taken, so b = 0, the step is the identity and T stays T_init."""
    sc = plane_scene("C4", 0, np.float32)
    T0 = np.eye(4)
    T0[:3, 3] = ICP_SHIFT
    return sc.reading - np.asarray(ICP_SHIFT), T0, sc


def centred(sc):
    """the scene as an ICP sees it: map and queries minus the map's mean (dyadic for these lattices: asserted by the host test)"""
    mean = sc.ref.mean(axis=0)
    return Scene(types.SimpleNamespace(ref=sc.ref - mean, nrm=sc.nrm), sc.reading - mean, sc.ids, note=sc.note + "/centred"), mean


# ---- rounded scenes: the contract's arithmetic, elementwise in T --------------------------------------------------------------------
def apply_max_dist(ids, d2, max_dist, T):
    """-1 / +inf beyond maxDist^2 (evaluated in T, a pair AT maxDist^2 stays)"""
    T = np.dtype(T).type
    with np.errstate(over="ignore"):
        md2 = T(max_dist) * T(max_dist)
    far = ~(d2 <= md2)
    return np.where(far, -1, ids).astype(np.int32), np.where(far, T(np.inf), d2)


def brute_in_T(q, m, max_dist, knn, T):
    """dx = q - m in T, ((dx dx + dy dy) + dz dz) in T -- numpy, elementwise, nothing fused --, then the first knn by (d2, index);
    -1 / +inf beyond maxDist^2.  ids (n,) int32 and d2 (n,) in T, or (n, knn)."""
    T = np.dtype(T)
    q, m = np.ascontiguousarray(q, dtype=T), np.ascontiguousarray(m, dtype=T)
    ids = np.empty((q.shape[0], knn), dtype=np.int64)
    d2 = np.empty((q.shape[0], knn), dtype=T)
    mx, my, mz = (np.ascontiguousarray(m[:, a])[None, :] for a in range(3))
    for a in range(0, q.shape[0], 1024):
        c = q[a:a + 1024]
        dx, dy, dz = c[:, 0:1] - mx, c[:, 1:2] - my, c[:, 2:3] - mz
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == T
        o = np.empty((len(c), knn), dtype=np.int64)
        w = d.copy() if knn > 1 else d
        for j in range(knn):                           # the minimum's first occurrence is its lowest index; struck out, the next one
            o[:, j] = np.argmin(w, axis=1)
            if j + 1 < knn:
                w[np.arange(len(c)), o[:, j]] = np.inf
        ids[a:a + 1024] = o
        d2[a:a + 1024] = np.take_along_axis(d, o, axis=1)
    ids, d2 = apply_max_dist(ids, d2, max_dist, T)
    return (ids[:, 0], d2[:, 0]) if knn == 1 else (ids, d2)


def ulp_nudge(q, T, seed):
    """every coordinate moved by -2 ... +2 ulps of T at that coordinate"""
    q = np.asarray(q, dtype=T)
    k = np.random.default_rng(seed).integers(-2, 3, size=q.shape)
    return (q + k.astype(T) * np.spacing(q)).astype(T)


@functools.lru_cache(maxsize=None)
def _r_lattice(tname):
    T = np.dtype(tname)
    out = []
    for h in HEIGHTS:
        sc = join([plane_scene("C4", h, T), plane_scene("E2", h, T)], "")
        out.append(types.SimpleNamespace(note=f"R/P48/z={h}s/{tname}", h=h, q=ulp_nudge(sc.reading, T, 300 + h), m=sc.ref.astype(T)))
    sc = cube_scene("CC8", T)
    out.append(types.SimpleNamespace(note=f"R/C16/{tname}", h=None, q=ulp_nudge(sc.reading, T, 399), m=sc.ref.astype(T)))
    return out


def r_lattice(T):
    """the C4 and E2 queries of every height and the cube centres, a few ulps off: rounding makes and breaks the ties"""
    return _r_lattice(np.dtype(T).name)


@functools.lru_cache(maxsize=None)
def d_pairs(o, seed=41):
    """float64.  Every query q has two map points a = q + r u and b = q + r (1 + eps) v (u, v random directions, r log-uniform in
    [1e-4, 0.3], eps log-uniform in [1e-16, 1e-3] and zero for a third); 200 of the a's are in the map twice; the map is shuffled.
    .q (4000, 3), .m (8200, 3), .ia / .ib: where a query's own pair went."""
    rng = np.random.default_rng(seed)
    n = D_QUERIES
    q = rng.uniform(-20.0, 20.0, size=(n, 3)) + np.array([o, -0.7 * o, 0.01 * o])

    def unit():
        v = rng.normal(size=(n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    r = np.exp(rng.uniform(np.log(1e-4), np.log(0.3), size=n))[:, None]
    eps = np.exp(rng.uniform(np.log(1e-16), np.log(1e-3), size=n))[:, None]
    eps[rng.permutation(n)[:n // 3]] = 0.0
    a, b = q + r * unit(), q + r * (1.0 + eps) * unit()
    dup = rng.permutation(n)[:D_DUPLICATES]
    m = np.concatenate([a, b, a[dup]])
    perm = rng.permutation(len(m))
    where = np.empty(len(m), dtype=np.int64)
    where[perm] = np.arange(len(m))                    # where[old] = new position
    m = m[perm]
    ia, ib = where[:n].copy(), where[n:2 * n]
    ia[dup] = np.minimum(ia[dup], where[2 * n:])       # (a point and its copy are the same bits: the lower slot is "the" a)
    assert np.array_equal(m[ia], a) and np.array_equal(m[ib], b)
    return types.SimpleNamespace(note=f"D/o={o:g}", o=o, q=q, m=np.ascontiguousarray(m), ia=ia, ib=ib, r=r[:, 0], eps=eps[:, 0])
