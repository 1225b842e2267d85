"""The statement of pgicp_sampling_surface_normal_* (include/pgicp.h) and of include/pgicp_ssn_ext.h in numpy: the whole filter --
the tree, the boxes in their order, the drops, the draw, the kept points, the box means, descriptor averaging, the normals -- and the
rows the companion header adds: eigValues, eigVectors, densities.  It shares no code with the device library, with
oracle/icp_oracle.c or with include/pgslam_amd/pointmatcher.hpp: the tree is an explicit stack over np.lexsort, the sums run in box
order over numpy scalars of the cloud's type T (numpy rounds every operation to T and never fuses), the Jacobi decomposition runs
box by box on Python floats (IEEE doubles, math.sqrt correctly rounded).  pinned() asserts that what the oracle states too (the keep
mask, the kept points, the normals, the boxes fused) is the oracle's byte for byte; only then is this the reference of the new rows
(tests/test_sampling_normals_ext_host.py, every scene).

Plain module: no GPU."""
import functools
import math

import numpy as np

TYPES = (np.float32, np.float64)
M64 = (1 << 64) - 1


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


def draw(seed, idx):
    """the build's counter-based uniform draw (SplitMix64 of seed * FNV prime + index, top 53 bits), in Python integers"""
    z = (int(seed) * 0x100000001B3 + int(idx)) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 11) / 9007199254740992.0


def boxes_of(x, knn):
    """the members of every box, in box order (the order its parent's cut left; a root of at most knn points: the identity)"""
    n = len(x)
    out = []
    stack = [(np.arange(n), x.min(0), x.max(0))]
    while stack:
        idx, lo, hi = stack.pop()
        if len(idx) <= knn:
            out.append(idx)
            continue
        side = hi - lo                                               # in T
        cut = 0
        for a in (1, 2):
            if side[a] > side[cut]:
                cut = a
        idx = idx[np.lexsort((idx, x[idx, cut]))]                   # (coordinate, index); -0.0 == +0.0
        right = len(idx) // 2
        left = len(idx) - right
        cv = x[idx[left], cut]
        lhi, rlo = hi.copy(), lo.copy()
        lhi[cut] = cv
        rlo[cut] = cv
        stack.append((idx[left:], rlo, hi))
        stack.append((idx[:left], lo, lhi))
    return out


def fuse(x, members, max_box, T):
    """one box: None when it is dropped, else dict(mean (3,), normal (3,), eig (3,), vec (9,), dens) in T"""
    p = x[members]
    cnt = T(len(members))
    if (p.max(0) - p.min(0)).max() > max_box:
        return None
    s = np.zeros(3, dtype=T)
    for row in p:
        s = s + row
    mean = s / cnt
    c = np.zeros(6, dtype=T)                                         # c00 c01 c02 c11 c12 c22
    for row in p:
        d = row - mean
        c = c + np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]], dtype=T)
    c00, c01, c02, c11, c12, c22 = (float(v) for v in c)
    ev, V = jacobi3([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]])
    lo = hi = 0
    for k in (1, 2):
        if ev[k] < ev[lo]:
            lo = k
        if ev[k] > ev[hi]:
            hi = k
    mid = 3 - lo - hi
    if lo == hi or not ev[hi] > 0.0 or not ev[mid] > 3.0 * float(np.finfo(T).eps) * ev[hi]:
        return None
    vec = np.array([V[r][col] for col in (lo, mid, hi) for r in range(3)], dtype=T)      # float -> T: one rounding
    eig = np.array([ev[lo], ev[mid], ev[hi]], dtype=T)
    r2 = T(0)
    for row in p:
        d = row - mean
        q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        if q > r2:
            r2 = q
    r = np.sqrt(r2)
    with np.errstate(all="ignore"):
        dens = cnt / (T((4.0 / 3.0) * 3.14159265358979323846) * ((r * r) * r))
    assert type(dens) is T and type(r) is T
    return dict(mean=mean, normal=vec[:3].copy(), eig=eig, vec=vec, dens=dens)


@functools.lru_cache(maxsize=None)
def _fused(key, knn, max_box, tname):
    T = np.dtype(tname).type
    x = _CLOUDS[key]
    with np.errstate(over="ignore"):
        mb = T(max_box)
    return [(m, fuse(x, m, mb, T)) for m in boxes_of(x, knn)]


_CLOUDS = {}


def run(xyz, T, knn=7, ratio=0.5, method=0, max_box=np.inf, seed=1, desc=None, average=True):
    """The filter over `xyz`: dict(keep (n,) bool, kept_idx (k,) int32, xyz (k,3), normals (k,3), descriptors (k,drows) or None,
    boxes: boxes fused, eigen_values (k,3), eigen_vectors (k,9), densities (k,), box_of (k,): the kept point's box) in T, the kept
    points in ascending input index."""
    T = np.dtype(T).type
    x = np.ascontiguousarray(xyz, dtype=T)
    key = (x.tobytes(), x.shape)
    _CLOUDS.setdefault(key, x)
    n = len(x)
    d = None if desc is None else np.ascontiguousarray(desc, dtype=T)
    keep = np.zeros(n, bool)
    box_of = np.full(n, -1)
    oxyz, odesc = x.copy(), None if d is None else d.copy()
    fused = _fused(key, int(knn), float(max_box), np.dtype(T).name)
    rt = float(T(ratio))
    nb = 0
    for b, (members, f) in enumerate(fused):
        if f is None:
            continue
        nb += 1
        if method == 0:
            for i in members:
                if draw(seed, i) < rt:
                    keep[i] = True
                    box_of[i] = b
        else:
            i = members[0]
            keep[i] = True
            box_of[i] = b
            oxyz[i] = f["mean"]
            if d is not None and average:
                s = np.zeros(d.shape[1], dtype=T)
                for m in members:
                    s = s + d[m]
                odesc[i] = s / T(len(members))
    k = np.flatnonzero(keep)
    pick = lambda name, w: np.array([fused[box_of[i]][1][name] for i in k], dtype=T).reshape(len(k), w)
    return dict(keep=keep, kept_idx=k.astype(np.int32), xyz=oxyz[k], normals=pick("normal", 3), descriptors=None if d is None else odesc[k],
                boxes=nb, eigen_values=pick("eig", 3), eigen_vectors=pick("vec", 9), densities=pick("dens", 1).reshape(-1), box_of=box_of[k],
                members=[fused[b][0] for b in box_of[k]])


def pinned(ref, o):
    """the reference against the oracle's dict (Oracle.sampling_surface_normal) it shares no code with: byte for byte"""
    k = np.flatnonzero(o["keep"])
    assert ref["boxes"] == o["boxes"]
    assert np.array_equal(ref["keep"], o["keep"]) and np.array_equal(ref["kept_idx"], k)
    assert ref["xyz"].tobytes() == o["xyz"][k].tobytes()
    assert ref["normals"].tobytes() == o["normals"][k].tobytes()


# ---- the scenes: name -> the cloud in float64 (knn is the case's) ----
def _cloud(n, seed=61):
    return np.random.default_rng(seed).uniform(-2, 2, (n, 3))


def _planar():
    p = _cloud(200, 62)
    p[:, 2] = 0.25                                                    # every box has rank 2: fused, the normal is +-z
    return p


def _flat_boxes():
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.zeros((64, 1))], 1)                   # an exact lattice in a plane


def _collinear():
    p = np.zeros((60, 3))
    p[:, 0] = np.arange(60) * 0.125                                   # rank 1: every box dropped
    return p


def _mixed_line():
    p = _cloud(300, 63)
    p[:120, 1:] = 0.0                                                 # a collinear run beside a cloud: some boxes dropped
    p[:120, 0] = 10.0 + np.arange(120) * 0.0625
    return p


def _coincident():
    p = _cloud(80, 64)
    return np.concatenate([p, p[:40], p[:40], np.tile(p[:1], (30, 1))])      # equal points: index ties, rank-0 boxes


def _big_box():
    p = _cloud(400, 65) * 0.25
    p[:5] += 50.0                                                     # a far cluster: its boxes' parents are long, one box is large
    p[5] = (25.0, 25.0, 25.0)
    return p


def _far():
    return _cloud(500, 66) + np.array([4.0e5, -4.0e5, 4.0e5])         # 400 km from the origin (f64 only)


SCENES = dict(cloud3000=lambda: _cloud(3000), planar=_planar, flat_boxes=_flat_boxes, collinear=_collinear, mixed_line=_mixed_line,
              coincident=_coincident, big_box=_big_box, far=_far)
SCENE_TYPES = dict(far=(np.float64,))
KNNS = (3, 7, 33)
# (ratio, samplingMethod)
SAMPLINGS = ((1e-3, 0), (0.5, 0), (0.999, 0), (0.5, 1))
MAX_BOX = dict(big_box=3.0)


def small_n(knn):
    """the sizes at which the tree changes shape: one point, the single root box, one cut, two box sizes on a level"""
    return (1, knn - 1, knn, knn + 1, 2 * knn + 1, 4 * knn + 3)


def cases():
    """every (name, T, knn, ratio, method, max_box) of the suite; `name` is a scene or n<size>"""
    out = []
    for knn in KNNS:
        for n in small_n(knn):
            for T in TYPES:
                for ratio, method in ((0.999, 0), (0.5, 1)):
                    out.append((f"n{n}", T, knn, ratio, method, np.inf))
    for name in SCENES:
        for T in SCENE_TYPES.get(name, TYPES):
            for knn in (KNNS if name == "cloud3000" else (7,)):
                for ratio, method in (SAMPLINGS if name in ("cloud3000", "big_box") and knn == 7 else ((0.5, 0), (0.5, 1))):
                    out.append((name, T, knn, ratio, method, MAX_BOX.get(name, np.inf)))
    return out


def case_id(c):
    name, T, knn, ratio, method, max_box = c
    return f"{name}-{np.dtype(T).name}-knn{knn}-r{ratio}-m{method}"


@functools.lru_cache(maxsize=None)
def _points(name):
    p = _cloud(int(name[1:]), 67) if name[0] == "n" and name[1:].isdigit() else SCENES[name]()
    p = np.ascontiguousarray(p, dtype=np.float64)
    p.setflags(write=False)
    return p


def cloud(name, T):
    return np.ascontiguousarray(_points(name), dtype=T)


def descriptors(n, T, rows=3):
    return np.random.default_rng(68).normal(size=(n, rows)).astype(T)


SEED = 29


@functools.lru_cache(maxsize=None)
def _case(name, tname, knn, ratio, method, max_box, drows, average):
    T = np.dtype(tname).type
    x = cloud(name, T)
    d = descriptors(len(x), T, drows) if drows else None
    ref = run(x, T, knn, ratio, method, max_box, SEED, d, average)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x, d, ref


def case(c, drows=0, average=True):
    """(xyz in T, descriptors or None, the reference's dict) of a case; computed once, read-only"""
    name, T, knn, ratio, method, max_box = c
    return _case(name, np.dtype(T).name, knn, ratio, method, float(max_box), drows, bool(average))


def identities(r, method):
    """what must hold of any result dict (the reference's or the device's), per kept point"""
    vec, eig, dens = np.asarray(r["eigen_vectors"]), np.asarray(r["eigen_values"]), np.asarray(r["densities"])
    assert vec[:, :3].tobytes() == np.asarray(r["normals"]).tobytes()
    assert np.all(eig[:, 0] <= eig[:, 1]) and np.all(eig[:, 1] <= eig[:, 2])
    assert np.all(np.isfinite(dens)) and np.all(dens > 0)
