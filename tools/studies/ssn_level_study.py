"""Study (CPU, numpy): does a level-synchronous schedule reproduce the oracle's SamplingSurfaceNormal boxes?

orc_sampling_surface_normal recurses: a range of more than knn points is sorted on (coordinate of its widest carried side,
index) and cut into ceil / floor halves.  The tree's shape depends on n and knn alone, so the device build (k_ssn.inc) runs
it level by level instead: the cloud sorted ONCE per axis by (coordinate, index) -- a stable LSD radix sort of orderable
keys, -0.0 made +0.0 --, then per level a cut axis per segment, the first `left` entries of that axis's list marked left, and
a stable partition of all three lists inside every segment by that mark.  A child of at most knn points is a box whose
member order is its range of the parent's cut-axis list.

This script states that schedule in numpy step for step (the same arrays the kernels keep: three concatenated lists,
seg_of per position, side per point) and checks, on tie-heavy clouds, that every box and its member order -- hence the
keep mask, the normals and the means -- are the oracle's.  Run from the repository root after `make`:
    python tools/studies/ssn_level_study.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle  # noqa: E402


def keys_of(v):
    """orderable unsigned keys of a coordinate column (T's order, -0.0 == +0.0)"""
    v = np.where(v == 0, np.zeros_like(v), v)                   # -0.0 -> +0.0
    u = v.view(np.uint32 if v.dtype == np.float32 else np.uint64)
    sign = u.dtype.type(1) << u.dtype.type(u.dtype.itemsize * 8 - 1)
    return np.where(u & sign, ~u, u | sign)


def radix_lists(xyz):
    """the three lists sorted by (coordinate, index): one stable partition per bit, as k_ssn_split does"""
    n = len(xyz)
    lst = np.tile(np.arange(n), 3).reshape(3, n)
    keys = np.stack([keys_of(xyz[:, a]) for a in range(3)])
    for b in range(keys.dtype.itemsize * 8):
        bit = (keys >> keys.dtype.type(b)) & keys.dtype.type(1)
        for a in range(3):
            order = np.concatenate([np.flatnonzero(bit[a] == 0), np.flatnonzero(bit[a] == 1)])
            lst[a], keys[a] = lst[a][order], keys[a][order]
    return lst


def level_boxes(xyz, knn):
    """[(member indices in box order)] of the level-synchronous schedule"""
    n = len(xyz)
    if n <= knn:
        return [np.arange(n)]
    lst = radix_lists(xyz)
    segs = [dict(first=0, count=n, lo=xyz[lst[:, 0], range(3)].copy(), hi=xyz[lst[:, -1], range(3)].copy())]
    seg_of = np.zeros(n, dtype=np.int64)
    boxes = []
    top = n
    while top > knn:
        child = []
        side = np.zeros(n, dtype=np.int64)
        nxt = np.full(n, -1, dtype=np.int64)
        for j, s in enumerate(segs):
            if s["count"] <= knn:
                child += [dict(first=0, count=0, lo=s["lo"], hi=s["hi"])] * 2
                continue
            span = s["hi"] - s["lo"]
            cut = 0
            for a in (1, 2):
                if span[a] > span[cut]:
                    cut = a
            right = s["count"] // 2
            left = s["count"] - right
            cv = xyz[lst[cut, s["first"] + left], cut]
            s["cut"] = cut
            L = dict(first=s["first"], count=left, lo=s["lo"].copy(), hi=s["hi"].copy())
            R = dict(first=s["first"] + left, count=right, lo=s["lo"].copy(), hi=s["hi"].copy())
            L["hi"][cut] = cv
            R["lo"][cut] = cv
            child += [L, R]
            for c in (L, R):
                if c["count"] <= knn:
                    boxes.append((c["first"], c["count"], cut))
            pos = np.arange(s["first"], s["first"] + s["count"])
            r = (pos >= s["first"] + left).astype(np.int64)
            side[lst[cut, pos]] = r
            nxt[pos] = np.where(np.where(r == 1, right, left) > knn, 2 * j + r, -1)
        out = lst.copy()
        for j, s in enumerate(segs):
            if s["count"] <= knn:
                continue
            left = s["count"] - s["count"] // 2
            for a in range(3):
                part = lst[a, s["first"]:s["first"] + s["count"]]
                f = side[part]
                out[a, s["first"]:s["first"] + s["count"]] = np.concatenate([part[f == 0], part[f == 1]])
                assert (f == 0).sum() == left
        lst, segs, seg_of = out, child, nxt
        top = (top + 1) // 2
    return [lst[a, f:f + c] for f, c, a in boxes]


def jacobi3(a):
    """the oracle's cyclic Jacobi (icp_oracle.c jacobi3), operation for operation: (eigenvalues, V)"""
    a = [list(map(float, r)) for r in a]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(16):
        if a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2] == 0.0:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if a[p][q] == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q])
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for r in range(3):
                    arp, arq = a[r][p], a[r][q]
                    a[r][p], a[r][q] = c * arp - s * arq, s * arp + c * arq
                for r in range(3):
                    apr, aqr = a[p][r], a[q][r]
                    a[p][r], a[q][r] = c * apr - s * aqr, s * apr + c * aqr
                for r in range(3):
                    vrp, vrq = v[r][p], v[r][q]
                    v[r][p], v[r][q] = c * vrp - s * vrq, s * vrp + c * vrq
    return [a[0][0], a[1][1], a[2][2]], v


def fuse(xyz, boxes, knn, ratio, method, max_box, seed, T):
    """the oracle's fuseRange on the listed boxes (numpy, sequential in T where it matters)"""
    n = len(xyz)
    keep = np.zeros(n, dtype=bool)
    nrm = np.zeros((n, 3), dtype=T)
    out = np.zeros((n, 3), dtype=T)
    fused = 0
    eps = np.finfo(T).eps
    for m in boxes:
        P = xyz[m]
        lo, hi, s = P[0].copy(), P[0].copy(), np.zeros(3, dtype=T)
        for p in P:
            lo = np.where(p < lo, p, lo)
            hi = np.where(p > hi, p, hi)
            s = (s + p).astype(T)
        ext = hi - lo
        box = ext[0]
        if ext[1] > box:
            box = ext[1]
        if ext[2] > box:
            box = ext[2]
        if box > T(max_box):
            continue
        mean = (s / T(len(m))).astype(T)
        C = np.zeros(6, dtype=T)
        for p in P:
            d = (p - mean).astype(T)
            C = (C + np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]], dtype=T)).astype(T)
        A = np.array([[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]], dtype=np.float64)
        ev, V = jacobi3(A)
        lo_, hi_ = 0, 0
        for k in (1, 2):
            if ev[k] < ev[lo_]:
                lo_ = k
            if ev[k] > ev[hi_]:
                hi_ = k
        if lo_ == hi_ or not (ev[hi_] > 0.0) or not (ev[3 - lo_ - hi_] > 3.0 * float(eps) * ev[hi_]):
            continue
        fused += 1
        if method == 0:
            for i in m:
                z = (seed * 0x100000001B3 + int(i)) & (2**64 - 1)
                z = (z + 0x9E3779B97F4A7C15) & (2**64 - 1)
                z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
                z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
                z ^= z >> 31
                if (z >> 11) / 9007199254740992.0 < float(T(ratio)):
                    keep[i] = True
                    out[i] = xyz[i]
        else:
            keep[m[0]] = True
            out[m[0]] = mean
    return keep, out, fused


def cloud(rng, n, kind, T):
    if kind == "grid":                                  # coarse grid: many equal coordinates, -0.0 and +0.0 mixed
        x = rng.integers(-3, 4, size=(n, 3)).astype(T) * T(0.5)
        z = x == 0
        x[z] = np.where(rng.random(z.sum()) < 0.5, T(-0.0), T(0.0))
        return x
    if kind == "dup":                                   # duplicates and collinear runs
        base = rng.normal(size=(n // 4 + 1, 3)).astype(T)
        x = base[rng.integers(0, len(base), n)]
        x[: n // 5, 1:] = 0
        return x
    return rng.normal(size=(n, 3)).astype(T) * T(4)


def main():
    rng = np.random.default_rng(5)
    checked = 0
    for T in (np.float32, np.float64):
        o = Oracle(T)
        for kind in ("grid", "dup", "normal"):
            for n, knn in ((1, 3), (7, 7), (8, 7), (100, 3), (1000, 7), (4097, 10), (3001, 64), (20000, 7)):
                xyz = cloud(rng, n, kind, T)
                for method in (0, 1):
                    boxes = level_boxes(xyz, knn)
                    assert sorted(np.concatenate(boxes).tolist()) == list(range(n))
                    keep, out, fused = fuse(xyz, boxes, knn, 0.5, method, np.inf, 3, T)
                    r = o.sampling_surface_normal(xyz, knn=knn, ratio=0.5, sampling_method=method, seed=3)
                    assert np.array_equal(keep, r["keep"]), (T, kind, n, knn, method)
                    assert fused == r["boxes"], (T, kind, n, knn, method, fused, r["boxes"])
                    if method == 1:                     # the box order's FIRST point carries the mean
                        assert np.array_equal(out[keep], r["xyz"][keep]), (T, kind, n, knn)
                    checked += 1
    print(f"level-synchronous schedule == oracle on {checked} clouds (keep mask, boxes fused, method-1 points)")


if __name__ == "__main__":
    main()
