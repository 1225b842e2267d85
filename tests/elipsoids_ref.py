"""The statement of include/pgicp_elipsoids.h in numpy, built on tests/sampling_normals_ext_ref.py (whose tree, scatter and Jacobi
parts the oracle pins byte for byte): its boxes_of, draw and named clouds, and its fuse restated with what the new rows need -- the
scatter sums and the eigenvalues in double are not among fuse's results, so box() walks the members again, by the same numpy
operations in the same order, and asserts that what both compute (mean, normal, eigenvalues, eigenvectors, density) is fuse's bit
for bit.  New here: the shape values, the planarity drop and the rows covariance, weights, means, shapes, in the cloud's type T.

pick_min_planarity() chooses a threshold a cloud's boxes straddle with room on either side; its conditions are on the reference alone.

Plain module: no GPU."""
import functools

import numpy as np

import sampling_normals_ext_ref as ssn

TYPES = ssn.TYPES
SEED = ssn.SEED
ROWS = dict(normals=3, densities=1, eigen_values=3, eigen_vectors=9, covariance=9, weights=1, means=3, shapes=3)
ALL = tuple(ROWS)
SPARSE = ("eigen_values", "weights", "shapes")                       # a subset without normals: the sparse request of the GPU tests
OLD = ("xyz", "kept_idx", "descriptors")


def box(x, members, max_box, T):
    """one box: None when maxBoxDim or the rank test drops it, else ssn.fuse's dict and cov (9,), weight, shapes (3,),
    planarity in T"""
    f = ssn.fuse(x, members, max_box, T)
    if f is None:
        return None
    p = x[members]
    cnt = T(len(members))
    s = np.zeros(3, dtype=T)
    for row in p:
        s = s + row
    mean = s / cnt
    c = np.zeros(6, dtype=T)                                         # c00 c01 c02 c11 c12 c22
    for row in p:
        d = row - mean
        c = c + np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]], dtype=T)
    c00, c01, c02, c11, c12, c22 = (float(v) for v in c)
    ev, V = ssn.jacobi3([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]])
    lo = hi = 0
    for k in (1, 2):
        if ev[k] < ev[lo]:
            lo = k
        if ev[k] > ev[hi]:
            hi = k
    mid = 3 - lo - hi
    # the same box as fuse saw: what both state is the same bits
    assert mean.tobytes() == f["mean"].tobytes()
    assert np.array([ev[lo], ev[mid], ev[hi]], dtype=T).tobytes() == f["eig"].tobytes()
    assert np.array([V[r][col] for col in (lo, mid, hi) for r in range(3)], dtype=T).tobytes() == f["vec"].tobytes()
    e0, e1, e2 = T(ev[hi]), T(ev[mid]), T(ev[lo])                    # descending; double -> T: one rounding
    with np.errstate(all="ignore"):
        tot = (e0 + e1) + e2
        v0, v1, v2 = e0 / tot, e1 / tot, e2 / tot
        planarity = T(2) * v1 - T(2) * v2
        shapes = np.array([planarity, v0 - v1, T(3) * v2], dtype=T)
    assert type(planarity) is T
    cov = np.array([c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]], dtype=T)
    return dict(f, cov=cov, weight=cnt, shapes=shapes, planarity=planarity)


@functools.lru_cache(maxsize=None)
def _boxes(key, knn, max_box, tname):
    T = np.dtype(tname).type
    x = ssn._CLOUDS[key]
    with np.errstate(over="ignore"):
        mb = T(max_box)
    return [(m, box(x, m, mb, T)) for m in ssn.boxes_of(x, knn)]


def _key(xyz, T):
    x = np.ascontiguousarray(xyz, dtype=T)
    key = (x.tobytes(), x.shape)
    ssn._CLOUDS.setdefault(key, x)
    return x, key


def planarities(xyz, T, knn=7, max_box=np.inf):
    """the planarity of every box that passes the maxBoxDim and rank tests, in T"""
    T = np.dtype(T).type
    x, key = _key(xyz, T)
    return np.array([b["planarity"] for _, b in _boxes(key, int(knn), float(max_box), np.dtype(T).name) if b is not None], dtype=T)


def pick_min_planarity(xyz, T, knn=7, max_box=np.inf):
    """A minPlanarity the cloud's boxes straddle: the midpoint of two adjacent sorted planarities near their median, such that at
    least one box falls on each side and no box's planarity lies within 4 ulp of the threshold (as T sees it)."""
    T = np.dtype(T).type
    p = np.sort(planarities(xyz, T, knn, max_box).astype(np.float64))
    p = p[np.isfinite(p)]
    assert len(p) >= 2
    gaps = np.flatnonzero(np.diff(p) > 0)
    assert len(gaps) > 0, "every box has the same planarity"
    at = gaps[np.argmin(np.abs(gaps - (len(p) - 1) // 2))]          # the distinct pair nearest the median
    thr = 0.5 * (p[at] + p[at + 1])
    t = T(thr)                                                       # what the device compares with
    assert 0.0 < thr <= 1.0
    below, above = int(np.sum(p.astype(T) < t)), int(np.sum(~(p.astype(T) < t)))
    assert below >= 1 and above >= 1, (below, above)
    assert np.all(np.abs(p - float(t)) > 4 * float(np.spacing(t))), "a box's planarity lies within 4 ulp of the threshold"
    return float(thr)


def run(xyz, T, knn=7, ratio=0.5, method=0, max_box=np.inf, min_planarity=0.0, seed=1, desc=None, average=True):
    """The filter over `xyz`: dict(keep (n,) bool, kept_idx (k,) int32, xyz (k,3), descriptors (k,drows) or None, boxes: boxes fused
    (after the planarity drop), box_of (k,), members, and every row of ROWS) in T, the kept points in ascending input index."""
    T = np.dtype(T).type
    x, key = _key(xyz, T)
    n = len(x)
    d = None if desc is None else np.ascontiguousarray(desc, dtype=T)
    keep = np.zeros(n, bool)
    box_of = np.full(n, -1)
    oxyz, odesc = x.copy(), None if d is None else d.copy()
    boxes = _boxes(key, int(knn), float(max_box), np.dtype(T).name)
    rt = float(T(ratio))
    mp = T(min_planarity)
    nb = 0
    for b, (members, f) in enumerate(boxes):
        if f is None:
            continue
        if mp > T(0) and f["planarity"] < mp:                        # strict, in T; after the rank test, before the draw
            continue
        nb += 1
        if method == 0:
            for i in members:
                if ssn.draw(seed, i) < rt:
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
    pick = lambda name, w: np.array([boxes[box_of[i]][1][name] for i in k], dtype=T).reshape(len(k), w)
    return dict(keep=keep, kept_idx=k.astype(np.int32), xyz=oxyz[k], descriptors=None if d is None else odesc[k], boxes=nb,
                normals=pick("normal", 3), densities=pick("dens", 1).reshape(-1), eigen_values=pick("eig", 3), eigen_vectors=pick("vec", 9),
                covariance=pick("cov", 9), weights=pick("weight", 1).reshape(-1), means=pick("mean", 3), shapes=pick("shapes", 3),
                box_of=box_of[k], members=[boxes[b][0] for b in box_of[k]])


# ---- the cases: sampling_normals_ext_ref's named clouds and small sizes, knn 3 and 7, and one case at knn 1024 ----
KNNS = (3, 7)
BIG_KNN = ("cloud3000", np.float32, 1024, 0.5, 1, np.inf)


def cases():
    """every (name, T, knn, ratio, method, max_box) of the suite; `name` is a scene of sampling_normals_ext_ref or n<size>"""
    out = [c for c in ssn.cases() if c[2] in KNNS]
    out.append(BIG_KNN)
    return out


case_id = ssn.case_id
cloud = ssn.cloud
descriptors = ssn.descriptors


@functools.lru_cache(maxsize=None)
def _case(name, tname, knn, ratio, method, max_box, min_planarity, drows, average):
    T = np.dtype(tname).type
    x = cloud(name, T)
    d = descriptors(len(x), T, drows) if drows else None
    ref = run(x, T, knn, ratio, method, max_box, min_planarity, SEED, d, average)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x, d, ref


def case(c, drows=0, average=True, min_planarity=0.0):
    """(xyz in T, descriptors or None, the reference's dict) of a case; computed once, read-only"""
    name, T, knn, ratio, method, max_box = c
    return _case(name, np.dtype(T).name, knn, ratio, method, float(max_box), float(min_planarity), drows, bool(average))


def identities(r, method, knn, x=None):
    """what must hold of any result dict (the reference's or the device's) with every row, per kept point"""
    g = {k: np.asarray(r[k]) for k in ALL + ("xyz",)}
    assert g["eigen_vectors"][:, :3].tobytes() == g["normals"].tobytes()
    cov = g["covariance"].reshape(-1, 3, 3)
    assert cov.tobytes() == np.ascontiguousarray(cov.transpose(0, 2, 1)).tobytes()              # symmetric bit for bit
    w = g["weights"]
    assert np.all(w == np.round(w)) and np.all(w >= 1) and np.all(w <= knn)
    if method == 1:
        assert g["means"].tobytes() == g["xyz"].tobytes()
    # the covariance is the matrix whose eigen-pairs eigValues / eigVectors are: |C v - lambda v| is bounded by what the decomposition
    # and the roundings can add -- cyclic Jacobi in double makes at most 16 sweeps of 3 rotations, each perturbing the matrix by about
    # one eps of double times its norm (48 eps), and v and lambda are each rounded once to T (half an eps of T on every term of the
    # three-term row sums and on lambda v: 2 eps of T) -- so 64 eps of T times the sum of |C|'s entries holds for both types
    C = cov.astype(np.float64)
    Vc = g["eigen_vectors"].astype(np.float64).reshape(-1, 3, 3)                                 # [point][column][row]
    lam = g["eigen_values"].astype(np.float64)
    scale = np.abs(C).sum((1, 2))
    for c in range(3):
        v = Vc[:, c, :]
        res = np.einsum("kij,kj->ki", C, v) - lam[:, c:c + 1] * v
        assert np.all(np.abs(res).max(1) <= 64 * np.finfo(g["covariance"].dtype).eps * scale)
    sh = g["shapes"]
    ok = np.isfinite(sh).all(1)
    assert np.all(sh[ok, 0] >= 0) and np.all(sh[ok, 1] >= 0)         # (e0 >= e1 >= e2 and rounding is monotone)
