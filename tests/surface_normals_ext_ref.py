"""The statement of include/pgicp_normals_ext.h in numpy: eigVectors, meanDists, matchedIds and smoothNormals from a cloud and the
neighbour table oracle.surface_normals(...)["ids"] gives.  It shares no code with the device library, with oracle/icp_oracle.c or
with include/pgslam_amd/surface_normals_host.hpp: the sums run in list order over numpy arrays of the cloud's type T (numpy rounds
every elementwise operation to T and never fuses), the Jacobi decomposition runs point by point on Python floats (IEEE doubles,
math.sqrt correctly rounded).  Its Jacobi is pinned by the oracle: pinned() asserts that the first eigenvector column and the
eigenvalues equal the oracle's normals and eigen_values byte for byte (tests/test_surface_normals_ext_host.py, every scene).

Plain module: no GPU."""
import functools
import math

import numpy as np

DEFAULT_COLUMNS = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0)      # eigenvalues (1,0,0), eigenvectors I, ascending first-minimum


def jacobi3(a):
    """cyclic Jacobi on a symmetric 3x3 (lists of Python floats): (eigenvalues, V with the eigenvectors as columns)"""
    a = [list(r) for r in a]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(16):
        if a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2] == 0.0:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if a[p][q] == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for r in range(3):
                    x, y = a[r][p], a[r][q]
                    a[r][p], a[r][q] = c * x - s * y, s * x + c * y
                for r in range(3):
                    x, y = a[p][r], a[q][r]
                    a[p][r], a[q][r] = c * x - s * y, s * x + c * y
                for r in range(3):
                    x, y = v[r][p], v[r][q]
                    v[r][p], v[r][q] = c * x - s * y, s * x + c * y
    return [a[0][0], a[1][1], a[2][2]], v


def rows(xyz, ids, T):
    """dict(normals (n,3), eigen_values (n,3), eigen_vectors (n,9), mean_dists (n,), matched_ids (n,knn)) in T; the normals raw"""
    T = np.dtype(T).type
    x = np.ascontiguousarray(xyz, dtype=T)
    ids = np.asarray(ids)
    n, knn = ids.shape
    valid = ids >= 0
    safe = np.where(valid, ids, 0)
    cnt = valid.sum(1)
    s = np.zeros((n, 3), dtype=T)
    for j in range(knn):
        s = np.where(valid[:, j:j + 1], s + x[safe[:, j]], s)
    with np.errstate(all="ignore"):
        mean = s / cnt.astype(T)[:, None]
    c = np.zeros((n, 6), dtype=T)                                    # c00 c01 c02 c11 c12 c22
    for j in range(knn):
        d = x[safe[:, j]] - mean
        t = np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1)
        c = np.where((valid[:, j] & (cnt > 0))[:, None], c + t, c)
    d = x - mean
    with np.errstate(all="ignore"):
        md = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    md = np.where(cnt > 0, md, T(0)).astype(T)
    eps = float(np.finfo(T).eps)
    vec = np.empty((n, 9), dtype=T)
    val = np.empty((n, 3), dtype=T)
    for i in range(n):
        c00, c01, c02, c11, c12, c22 = (float(v) for v in c[i])
        ev, V = jacobi3([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]])
        lo = hi = 0
        for k in (1, 2):
            if ev[k] < ev[lo]:
                lo = k
            if ev[k] > ev[hi]:
                hi = k
        mid = 3 - lo - hi
        if lo == hi or not ev[hi] > 0.0 or not ev[mid] > 3.0 * eps * ev[hi]:
            vec[i] = DEFAULT_COLUMNS
            val[i] = (0.0, 0.0, 1.0)
        else:
            vec[i] = [V[r][col] for col in (lo, mid, hi) for r in range(3)]          # float -> T: one rounding
            val[i] = [ev[lo], ev[mid], ev[hi]]
    return dict(normals=vec[:, :3].copy(), eigen_values=val, eigen_vectors=vec, mean_dists=md, matched_ids=np.where(valid, ids, -1).astype(T))


def smooth_dots(nrm, ids, T):
    """(n,knn) the dot products the sign rule looks at (NaN where the entry is none)"""
    T = np.dtype(T).type
    r = np.ascontiguousarray(nrm, dtype=T)[:, :3]
    ids = np.asarray(ids)
    out = np.full(ids.shape, np.nan, dtype=T)
    for j in range(ids.shape[1]):
        ok = ids[:, j] >= 0
        p = r[np.where(ok, ids[:, j], 0)]
        d = (r[:, 0] * p[:, 0] + r[:, 1] * p[:, 1]) + r[:, 2] * p[:, 2]
        out[:, j] = np.where(ok, d, T(np.nan))
    return out


def smooth(nrm, ids, T):
    """the smoothing step over raw normals `nrm` (n, >= 3) and the table `ids` (n,knn), -1 = none: (n,3) in T"""
    T = np.dtype(T).type
    r = np.ascontiguousarray(nrm, dtype=T)[:, :3]
    ids = np.asarray(ids)
    dots = smooth_dots(r, ids, T)
    a = np.zeros((len(r), 3), dtype=T)
    for j in range(ids.shape[1]):
        ok = ids[:, j] >= 0
        p = r[np.where(ok, ids[:, j], 0)]
        plus = dots[:, j] > 0
        a = np.where(ok[:, None], np.where(plus[:, None], a + p, a - p), a)
    with np.errstate(all="ignore"):
        ln = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
        ok = (ln > 0) & np.isfinite(ln)
        out = np.where(ok[:, None], a / ln[:, None], r)
    return out.astype(T)


# ---- the scenes of the new rows: name -> (cloud in float64, knn, maxDist) ----
def _random():
    return np.random.default_rng(41).uniform(-1, 1, (2000, 3)), 10, 0.2


def _lattice():
    return np.round(np.random.default_rng(5).uniform(-1, 1, (600, 3)) * 8) / 8, 6, 0.3          # tests/test_normals.py's: exact ties


def _line():
    return np.stack([np.linspace(0, 1, 50), np.zeros(50), np.zeros(50)], 1), 5, 10.0            # rank 1 scatter


def _lonely():
    return np.array([[0, 0, 0], [100, 0, 0], [0, 100, 0]], dtype=np.float64), 3, 1.0             # only itself within maxDist


def _doubled():
    p = np.random.default_rng(43).uniform(-1, 1, (500, 3))
    return np.concatenate([p, p]), 8, np.inf                                                      # zero distances, index ties


SCENES = dict(random=_random, lattice=_lattice, line=_line, lonely=_lonely, doubled=_doubled)
TYPES = (np.float32, np.float64)


@functools.lru_cache(maxsize=None)
def _scene(name, tname):
    from oracle import Oracle
    T = np.dtype(tname).type
    pts, knn, md = SCENES[name]()
    xyz = np.ascontiguousarray(pts, dtype=T)
    o = Oracle(T).surface_normals(xyz, knn, md)
    ref = rows(xyz, o["ids"], T)
    ref["smoothed"] = smooth(ref["normals"], o["ids"], T)
    ref["ids"], ref["d2"] = o["ids"], o["d2"]
    for a in list(ref.values()) + [xyz, o["normals"], o["eigen_values"]]:
        a.setflags(write=False)
    return xyz, knn, md, o, ref


def scene(name, T):
    """(xyz in T, knn, maxDist, the oracle's dict, the reference's dict with `smoothed`, `ids`, `d2` besides); computed once"""
    return _scene(name, np.dtype(T).name)


def pinned(ref, o):
    """the reference's Jacobi, ordering and degenerate rule against the oracle it shares no code with"""
    assert ref["normals"].tobytes() == o["normals"].tobytes()
    assert ref["eigen_vectors"][:, :3].tobytes() == o["normals"].tobytes()
    assert ref["eigen_values"].tobytes() == o["eigen_values"].tobytes()


# ---- the clouds of the superset test ----
SUPERSET_N = (1, 2, 3, 127, 128, 129, 2000)
SUPERSET_KNN = (3, 8, 9, 16, 17, 32)
SUPERSET_MAX_DIST = 0.35


def superset_cloud(n, T):
    """random points in [-1,1]^3, every 16th -- the first among them -- moved onto a 5 x 5 x 5 block of isolated points 1 m apart
    beside it: with maxDist 0.35 those have cnt = 1, and they are 1/16 > 5 % of every prefix"""
    p = np.random.default_rng(47).uniform(-1, 1, (2000, 3))
    k = np.arange(0, 2000, 16)
    q = k // 16
    p[k] = np.stack([3.0 + q % 5, -2.0 + (q // 5) % 5, -2.0 + q // 25], 1)
    return np.ascontiguousarray(p[:n], dtype=T)


# ---- the plane of known answers (exact_scenes.Plane, knn = 5, maxDist = inf) ----
def plane_case(T, L=12):
    """(xyz in T, the indices of the interior lattice points): an interior point's 5 nearest are itself and its 4 lattice
    neighbours at distance s, the 8 next ones lie further: the list is unambiguous as a set, and the scatter is diag(2 s^2, 2 s^2, 0)
    in any order of summation"""
    from exact_scenes import Plane
    pl = Plane(L)
    interior = np.flatnonzero((pl.i > 0) & (pl.i < L - 1) & (pl.j > 0) & (pl.j < L - 1))
    return np.ascontiguousarray(pl.ref, dtype=T), interior


def sign_flip_case(name, T, seed=3):
    """the reference's raw normals of scene `name` with a seeded half negated: (normals, ids, the flipped mask)"""
    _, _, _, o, ref = scene(name, T)
    flip = np.random.default_rng(seed).permutation(len(ref["normals"])) % 2 == 0
    nrm = np.where(flip[:, None], -ref["normals"], ref["normals"]).astype(T)
    return nrm, o["ids"], flip
