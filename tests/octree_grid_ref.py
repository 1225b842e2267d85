"""[EXT] OctreeGridDataPointsFilter as include/pgicp_octree.h states it, in numpy, written twice: `recursive` is the literal
recursion (node lists, children 0 .. 7), `coded` the path-code form (codes, a stable argsort, prefix counts).  Every operation is
in T; leaf sums are sequential (np.cumsum), never the pairwise np.sum.  Both return dict(kept_idx, count, depth, xyz, desc), one
entry per non-empty leaf in leaf order.  CASES is the list of clouds and parameters the host and the device tests share."""
import functools

import numpy as np

MAX_DEPTH = 21
M64 = (1 << 64) - 1


def mix(z):
    """the SplitMix64 finaliser of RandomSamplingDataPointsFilter, in Python integers"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def root(x, T):
    """(c (3,), r): every operation in T"""
    lo, hi = x.min(axis=0), x.max(axis=0)
    e = (hi - lo).astype(T)
    c = (lo + e * T(0.5)).astype(T)
    r = T(T(0.5) * e.max())
    return c, r


def _emit(x, desc, idx, depth, method, seed, T, out):
    """one leaf: idx ascending"""
    count = len(idx)
    first = int(idx[0])
    keep = first
    cen = None
    if method == 1:
        keep = int(idx[(mix((seed * 0x100000001B3 + first) & M64) >> 11) % count])
    if method >= 2:
        cen = (np.cumsum(x[idx], axis=0, dtype=T)[-1] / T(count)).astype(T)
    if method == 3:
        d = (x[idx] - cen).astype(T)
        dd = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(T)
        keep = int(idx[int(np.argmin(dd))])                     # (argmin: the first of equal values, idx ascending)
    out["kept_idx"].append(keep)
    out["count"].append(count)
    out["depth"].append(depth)
    out["xyz"].append(cen if method == 2 else x[keep])
    if desc is not None:
        out["desc"].append((np.cumsum(desc[idx], axis=0, dtype=T)[-1] / T(count)).astype(T) if method == 2 else desc[keep])


def _finish(out, T, drows):
    k = len(out["kept_idx"])
    return dict(kept_idx=np.array(out["kept_idx"], dtype=np.int32), count=np.array(out["count"], dtype=np.int32),
                depth=np.array(out["depth"], dtype=np.int32), xyz=np.array(out["xyz"], dtype=T).reshape(k, 3),
                desc=np.array(out["desc"], dtype=T).reshape(k, drows) if drows else None)


def _check(x, max_pts, max_size, method, T):
    assert x.dtype == T and x.ndim == 2 and x.shape[1] == 3
    if max_pts < 1 or not (T(max_size) >= 0) or not np.isfinite(T(max_size)) or method not in (0, 1, 2, 3):
        raise ValueError("bad parameter")
    if not np.isfinite(x).all():
        raise ValueError("a coordinate is not finite")


def recursive(x, desc, max_pts, max_size, method, seed, T):
    """the literal recursion"""
    _check(x, max_pts, max_size, method, T)
    out = dict(kept_idx=[], count=[], depth=[], xyz=[], desc=[])
    drows = 0 if desc is None else desc.shape[1]
    if len(x) == 0:
        return _finish(out, T, drows)
    ms = T(max_size)

    def node(idx, c, r, d):
        if len(idx) == 0:
            return
        if len(idx) <= max_pts or r * T(2) <= ms or d == MAX_DEPTH:
            _emit(x, desc, idx, d, method, seed, T, out)
            return
        h = T(r * T(0.5))
        p = x[idx]
        m = (p[:, 0] > c[0]).astype(np.int64) + ((p[:, 1] > c[1]).astype(np.int64) << 1) + ((p[:, 2] > c[2]).astype(np.int64) << 2)
        for child in range(8):
            cc = np.array([c[a] + h if (child >> a) & 1 else c[a] - h for a in range(3)], dtype=T)
            node(idx[m == child], cc, h, d + 1)

    c, r = root(x, T)
    node(np.arange(len(x)), c, r, 0)
    return _finish(out, T, drows)


def codes(x, max_size, T):
    """(keys (n,) uint64, levels): levels = min(21, d_size)"""
    c0, r = root(x, T)
    ms = T(max_size)
    levels = 0
    rr = r
    while levels < MAX_DEPTH and not (rr * T(2) <= ms):
        rr = T(rr * T(0.5))
        levels += 1
    key = np.zeros(len(x), dtype=np.uint64)
    c = np.tile(c0, (len(x), 1)).astype(T)
    for _ in range(levels):
        h = T(r * T(0.5))
        up = x > c
        m = up[:, 0].astype(np.uint64) | (up[:, 1].astype(np.uint64) << np.uint64(1)) | (up[:, 2].astype(np.uint64) << np.uint64(2))
        c = np.where(up, c + h, c - h).astype(T)
        key = (key << np.uint64(3)) | m
        r = h
    return key, levels


def coded(x, desc, max_pts, max_size, method, seed, T):
    """the path-code form"""
    _check(x, max_pts, max_size, method, T)
    out = dict(kept_idx=[], count=[], depth=[], xyz=[], desc=[])
    drows = 0 if desc is None else desc.shape[1]
    n = len(x)
    if n == 0:
        return _finish(out, T, drows)
    key, levels = codes(x, max_size, T)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    depth = np.full(n, levels, dtype=np.int64)
    for d in range(levels, -1, -1):                              # the count of a d-prefix is non-increasing in d: the smallest d stays
        pre = sk >> np.uint64(3 * (levels - d))
        _, inv, cnt = np.unique(pre, return_inverse=True, return_counts=True)
        depth[cnt[inv] <= max_pts] = d
    s = 0
    while s < n:
        sh = np.uint64(3 * (levels - int(depth[s])))
        e = s + 1
        while e < n and (sk[e] >> sh) == (sk[s] >> sh):
            e += 1
        _emit(x, desc, np.sort(order[s:e]), int(depth[s]), method, seed, T, out)
        s = e
    return _finish(out, T, drows)


# ---- the clouds and cases the host and the device tests share ----------------------------------------------------------------
def cloud(name):
    """float64 (n, 3); the tests round it to T"""
    rng = np.random.default_rng(abs(hash_name(name)))
    if name.startswith("n"):
        n = int(name[1:])
        return rng.uniform([-10, -7, -1], [10, 8, 4], size=(n, 3))
    box = np.array([[0.0, 0.0, 0.0], [100.0, 100.0, 100.0]])
    if name == "coincident":                                      # two points of equal coordinates: the depth cap
        return np.concatenate([box, [[37.3, 41.1, 12.7]] * 2, [[80.0, 20.0, 60.0]]])
    if name == "close_pair":                                      # 1e-4 m apart in a 100 m box: deep, under the cap as double
        return np.concatenate([box, [[37.3, 41.1, 12.7], [37.3001, 41.1, 12.7]], [[80.0, 20.0, 60.0]]])
    if name == "lattice":                                         # symmetric integers: node centres land on points
        g = np.arange(-2.0, 3.0)
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        return p[rng.permutation(len(p))]
    if name == "cluster3000":                                     # 2000 points in one cubic metre of a 10 m box
        p = np.concatenate([rng.uniform(0.5, 1.5, size=(2000, 3)), rng.uniform(0, 10, size=(1000, 3))])
        return p[rng.permutation(len(p))]
    raise KeyError(name)


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def descriptors(n, drows, T):
    if drows == 0:
        return None
    return np.random.default_rng(7 + drows).normal(size=(n, drows)).astype(T)


# (cloud, maxPointByNode, maxSizeByNode, samplingMethod, stride, drows)
CASES = [
    ("n0", 1, 0.0, 0, 3, 0), ("n1", 1, 0.0, 0, 3, 3), ("n1", 3, 0.0, 2, 4, 0), ("n2", 1, 0.0, 0, 3, 0), ("n2", 3, 0.0, 3, 3, 7),
    ("n255", 1, 0.0, 0, 3, 0), ("n256", 1, 0.0, 1, 4, 3), ("n257", 3, 0.0, 2, 3, 7), ("n257", 64, 0.0, 3, 3, 3),
    ("n4097", 1, 0.0, 0, 3, 0), ("n4097", 3, 0.0, 2, 4, 3), ("n4097", 64, 0.0, 1, 3, 0), ("n4097", 64, 0.0, 3, 3, 7),
    ("n4097", 3, 1.5, 2, 3, 3),                                   # some branches stop by size before the count rule does
    ("n4097", 1, 1.5, 0, 3, 0), ("n4097", 64, 1.5, 3, 4, 0),
    ("n20001", 1, 0.0, 0, 3, 0), ("n20001", 8, 0.0, 2, 3, 3), ("n20001", 200, 0.0, 3, 4, 0),   # several tiles of the sort and chunks of the scan
    ("n257", 1, 100.0, 2, 3, 3), ("n257", 1, 100.0, 3, 3, 0),     # >= 2 r: the root is a leaf, one output
    ("n257", 3, 20.0, 0, 3, 0),                                   # exactly 2 r of the largest extent
    ("coincident", 1, 0.0, 0, 3, 0), ("coincident", 1, 0.0, 2, 3, 3), ("coincident", 1, 0.0, 1, 3, 0), ("coincident", 3, 0.0, 3, 3, 0),
    ("close_pair", 1, 0.0, 0, 3, 0), ("close_pair", 1, 0.0, 2, 4, 7),
    ("lattice", 1, 0.0, 0, 3, 0), ("lattice", 3, 0.0, 2, 3, 3), ("lattice", 64, 0.0, 3, 3, 0), ("lattice", 3, 1.0, 1, 3, 0),
    ("cluster3000", 100, 6.0, 2, 3, 7), ("cluster3000", 100, 6.0, 3, 4, 3), ("cluster3000", 100, 6.0, 0, 3, 0), ("cluster3000", 100, 6.0, 1, 3, 3),
    ("cluster3000", 1000, 0.0, 2, 3, 0), ("cluster3000", 1000, 0.0, 3, 3, 0),
]
SEED = 12345


def case_id(case):
    name, mp, ms, method, stride, drows = case
    return f"{name}-p{mp}-s{ms:g}-m{method}-st{stride}-d{drows}"


@functools.lru_cache(maxsize=None)
def case_inputs(case, T):
    """(x (n, 3) in T, desc (n, drows) in T or None); shared, read-only"""
    name, _, _, _, _, drows = case
    x = np.ascontiguousarray(cloud(name).reshape(-1, 3), dtype=T)
    d = descriptors(len(x), drows, T)
    x.setflags(write=False)
    if d is not None:
        d.setflags(write=False)
    return x, d


@functools.lru_cache(maxsize=None)
def case_expected(case, T):
    """the reference's result of a case (the path-code form), computed once and shared"""
    _, mp, ms, method, _, _ = case
    x, d = case_inputs(case, T)
    want = coded(x, d, mp, ms, method, SEED, T)
    for v in want.values():
        if v is not None:
            v.setflags(write=False)
    return want
