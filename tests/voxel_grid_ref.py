"""numpy statement of [EXT] VoxelGridDataPointsFilter as include/pgicp.h (pgicp_voxel_grid_*) states it: rules 1-8 and deviations
(a)-(c), every operation in T.  The voxel sums are sequential in ascending input index: the pairs are sorted by (key, index),
then added rank by rank (voxels of at most 64 points) or by np.add.accumulate, a strictly sequential running sum (larger ones);
never np.sum, whose pairwise order is not the statement's."""
import numpy as np


class Refused(ValueError):
    pass


def grid(xyz, v_size, dtype):
    """rules 1-3: (v, minB, numDiv, keys) in T / uint64; Refused where the statement refuses"""
    T = np.dtype(dtype).type
    X = np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=T)
    v = np.asarray(v_size, dtype=np.float64).astype(T)
    if not np.all(np.isfinite(v) & (v > T(0))):
        raise Refused("a voxel size is not finite and > 0 in T")
    if len(X) == 0:
        return v, None, None, np.zeros(0, np.uint64)
    if not np.all(np.isfinite(X)):
        raise Refused("a coordinate is NaN or infinite")
    minB = X.min(0) / v
    maxB = X.max(0) / v
    d = (T(1) + maxB) - minB
    if not np.all(d < T(2.0 ** 31)):
        raise Refused("numDiv >= 2^31")
    nd = d.astype(np.uint64)
    if int(nd[0]) * int(nd[1]) * int(nd[2]) >= 2 ** 62:
        raise Refused("numDivX numDivY numDivZ >= 2^62")
    ia = np.floor(X / v - minB).astype(np.uint64)
    key = ia[:, 0] + ia[:, 1] * nd[0] + ia[:, 2] * (nd[0] * nd[1])
    return v, minB, nd, key


def _seq_means(vals, order, heads, count, T):
    """per voxel: ((v_first + v_2nd) + ...) / T(count) in ascending index; vals (n, r) in T, order the (key, index) sort"""
    out = vals[order[heads]].copy()
    small = np.flatnonzero(count <= 64)
    for r in range(1, int(count[small].max()) if len(small) else 1):
        m = small[count[small] > r]
        out[m] = out[m] + vals[order[heads[m] + r]]
    for g in np.flatnonzero(count > 64):
        seg = vals[order[heads[g]:heads[g] + count[g]]]
        out[g] = np.add.accumulate(seg, axis=0)[-1]
    return out / count.astype(T)[:, None]


def voxel_grid(xyz, v_size=(1.0, 1.0, 1.0), use_centroid=True, desc=None, average=True, dtype=np.float32):
    """dict(xyz (k,3), descriptors (k,drows) or None, kept_idx (k,) int32, count (k,) int32), ascending first-point index"""
    T = np.dtype(dtype).type
    X = np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=T)
    D = None if desc is None else np.ascontiguousarray(desc, dtype=T).reshape(len(X), -1)
    v, minB, nd, key = grid(X, v_size, dtype)
    n = len(X)
    if n == 0:
        return dict(xyz=np.zeros((0, 3), T), descriptors=None if D is None else np.zeros((0, D.shape[1]), T),
                    kept_idx=np.zeros(0, np.int32), count=np.zeros(0, np.int32))
    order = np.argsort(key, kind="stable")                    # (key, index): the input is in index order
    sk = key[order]
    heads = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    count = np.diff(np.r_[heads, n])
    first = order[heads]
    if use_centroid:
        pts = _seq_means(X, order, heads, count, T)
    else:
        idx = sk[heads]
        pl = nd[0] * nd[1]
        k = idx // pl
        j = (idx - k * pl) // nd[0]
        i = idx - k * pl - j * nd[0]
        ia = np.stack([i, j, k], 1).astype(T)
        pts = (minB + ia) * v + v / T(2)
    dout = None
    if D is not None:
        dout = _seq_means(D, order, heads, count, T) if average else D[first].copy()
    o = np.argsort(first, kind="stable")                      # rule 8: ascending first-point index
    return dict(xyz=np.ascontiguousarray(pts[o]), descriptors=None if dout is None else np.ascontiguousarray(dout[o]),
                kept_idx=first[o].astype(np.int32), count=count[o].astype(np.int32))
