"""CovarianceSamplingDataPointsFilter restated in numpy (the statement: include/pgicp_covsample.h), and the clouds its tests share.

frame(): the frame in float64 numpy, its values rounded to T where the statement says so.  select(): the selection given a frame,
transliterated twice -- plain Python lists with pop (`vectorised=False`), and a stable argsort on (-v, index) with head cursors --
every step a numpy operation in T, so each rounding is the statement's."""
import functools
import math

import numpy as np


def _f(xyz, nrm, c, L, T):
    """f_i of every point, (n, 6), in T"""
    x = np.ascontiguousarray(xyz, dtype=T)[:, :3]
    n = np.ascontiguousarray(nrm, dtype=T)[:, :3]
    c = np.asarray(c, dtype=T)
    px, py, pz = x[:, 0] - c[0], x[:, 1] - c[1], x[:, 2] - c[2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    cx = py * nz - pz * ny
    cy = pz * nx - px * nz
    cz = px * ny - py * nx
    inv = T(1) / T(L)
    return np.stack([inv * cx, inv * cy, inv * cz, nx, ny, nz], axis=1)


def frame(xyz, nrm, torque_norm, T):
    """dict(center (3,), L, eigenvalues (6,) ascending, basis (6,6) eigenvectors as columns, C (6,6)): float64 arrays whose
    center, L and basis hold values of T"""
    x = np.ascontiguousarray(xyz, dtype=T)[:, :3]
    n = len(x)
    # (fsum: the exact sum, rounded once -- what "summed in double in any order" has to mean for the result not to depend on the
    #  order when T is double, where a plain sum's n 2^-53 is n / 2 eps of T)
    c = (np.array([math.fsum(x[:, a].astype(np.float64)) for a in range(3)]) / n).astype(T)
    if torque_norm == 0:
        L = T(1)
    elif torque_norm == 1:
        d = x - c
        norms = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        L = T(math.fsum(norms.astype(np.float64)) / n)
    else:
        L = T(0.5) * (x.max(axis=0) - x.min(axis=0)).max()
    if not L > 0:
        raise ValueError("L is not > 0: every point lies at the mean")
    f = _f(x, nrm, c, L, T).astype(np.float64)
    C = f.T @ f
    lam, X = np.linalg.eigh(C)
    return dict(center=c.astype(np.float64), L=float(L), eigenvalues=lam, basis=X.astype(T).astype(np.float64), C=C)


def values(xyz, nrm, fr, T):
    """v (n, 6) in T"""
    f = _f(xyz, nrm, fr["center"], fr["L"], T)
    X = np.asarray(fr["basis"], dtype=T)
    v = np.empty((len(f), 6), dtype=T)
    for k in range(6):
        v[:, k] = np.abs(((((f[:, 0] * X[0, k] + f[:, 1] * X[1, k]) + f[:, 2] * X[2, k]) + f[:, 3] * X[3, k]) + f[:, 4] * X[4, k])
                         + f[:, 5] * X[5, k])
    return v


def select(xyz, nrm, nb_sample, fr, T, vectorised=True):
    """the picks (int32, pick order) of the statement, given the frame"""
    n = len(xyz)
    if nb_sample >= n:
        return np.arange(n, dtype=np.int32)
    v = values(xyz, nrm, fr, T)
    t = np.zeros(6, dtype=T)
    picks = []
    if not vectorised:
        lists = []
        for k in range(6):
            order = sorted(range(n), key=lambda i: (-float(v[i, k]), i)) if n <= 4096 else list(np.lexsort((np.arange(n), -v[:, k])))
            lists.append([int(i) for i in order])
        sampled = set()
        for _ in range(nb_sample):
            k = 0
            for kk in range(1, 6):
                if t[k] > t[kk]:
                    k = kk
            while lists[k][0] in sampled:
                lists[k].pop(0)
            j = lists[k].pop(0)
            sampled.add(j)
            picks.append(j)
            for m in range(6):
                t[m] = t[m] + v[j, m] * v[j, m]
        return np.array(picks, dtype=np.int32)
    idx = np.arange(n)
    order = [np.lexsort((idx, -v[:, k])) for k in range(6)]
    head = [0] * 6
    sampled = np.zeros(n, dtype=bool)
    for _ in range(nb_sample):
        k = int(np.argmin(t))                       # the first index of the smallest t
        o = order[k]
        while sampled[o[head[k]]]:
            head[k] += 1
        j = int(o[head[k]])
        head[k] += 1
        sampled[j] = True
        picks.append(j)
        t += v[j] * v[j]
    return np.array(picks, dtype=np.int32)


# ---- the clouds of the tests -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _room():
    from pgslam_amd import synth
    xyz, nrm = synth.make_scan(synth.make_world(), synth.se3(), 100_000, 0, rings=32)
    # firing order is azimuth-major: a prefix would be a thin sector, so the prefixes are taken from a fixed shuffle
    perm = np.random.default_rng(11).permutation(len(xyz))
    return xyz[perm].astype(np.float64), nrm[perm].astype(np.float64)


def cloud(kind, n, T):
    """(xyz (n,3), normals (n,3)) as arrays of T"""
    rng = np.random.default_rng(1000 + n)
    if kind == "room":
        x, nr = _room()
        x, nr = x[:n], nr[:n]
    elif kind == "offset":
        x, nr = _room()
        x, nr = x[:n] + np.array([1000.0, -1000.0, 1000.0]), nr[:n]
    elif kind == "plane":                           # constant normals: v of three lists is 0 for every point
        x = np.stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), np.zeros(n)], axis=1)
        nr = np.tile([0.0, 0.0, 1.0], (n, 1))
    elif kind == "twice":                           # every point appears twice (n odd: the last one once)
        x, nr = _room()
        h = (n + 1) // 2
        x, nr = np.concatenate([x[:h], x[:n - h]]), np.concatenate([nr[:h], nr[:n - h]])
    elif kind == "corridor":                        # two long walls, a floor, one short end wall
        q = n // 4
        w1 = np.stack([rng.uniform(0, 30, q), np.full(q, 1.5), rng.uniform(0, 2.5, q)], 1)
        w2 = np.stack([rng.uniform(0, 30, q), np.full(q, -1.5), rng.uniform(0, 2.5, q)], 1)
        fl = np.stack([rng.uniform(0, 30, q), rng.uniform(-1.5, 1.5, q), np.zeros(q)], 1)
        e = n - 3 * q
        end = np.stack([np.full(e, 30.0), rng.uniform(-1.5, 1.5, e), rng.uniform(0, 2.5, e)], 1)
        x = np.concatenate([w1, w2, fl, end])
        nr = np.concatenate([np.tile([0.0, -1.0, 0.0], (q, 1)), np.tile([0.0, 1.0, 0.0], (q, 1)), np.tile([0.0, 0.0, 1.0], (q, 1)),
                             np.tile([-1.0, 0.0, 0.0], (e, 1))])
        p = rng.permutation(n)
        x, nr = x[p], nr[p]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=T), np.ascontiguousarray(nr, dtype=T)


def frame_bounds_ok(fr, ref, xyz, T):
    """the issue's four frame tolerances; returns the four (value, bound) pairs"""
    eps = float(np.finfo(T).eps)
    X, lam = np.asarray(fr["basis"]), np.asarray(fr["eigenvalues"])
    C = ref["C"]
    return [
        (float(np.abs(np.asarray(fr["center"]) - ref["center"]).max()), eps * float(np.abs(np.asarray(xyz, dtype=np.float64)).max())),
        (abs(fr["L"] - ref["L"]), 4 * eps * ref["L"]),
        (float(np.abs(X.T @ X - np.eye(6)).max()), 64 * eps),
        (float(np.abs(C @ X - X * lam[None, :]).max()), 64 * eps * float(np.trace(C))),
    ]
