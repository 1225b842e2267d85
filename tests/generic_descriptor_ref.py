"""numpy restatement of [EXT] GenericDescriptorOutlierFilter (include/pgicp.h, pgicp_set_descriptor_filter): the reference the
device and drop-in tests compare against.  Every weight is evaluated in T; deviations (a) and (b) of the header are stated here."""
import numpy as np


def gd_weights(ids, values, mode, threshold=None, dtype=np.float32):
    """ids: the matcher's neighbour ids (any shape, -1: no neighbour); values: the reference's one-row descriptor (one value per
    reference point).  mode "larger" / "smaller" (hard, strict comparison with `threshold` in T) or "soft" (value / the largest
    value over the pairs with a neighbour).  Returns weights of ids' shape in T.
    (a) a pair without a neighbour weighs 0 and does not enter the soft maximum; (b) a soft maximum of 0 gives every weight 0."""
    T = np.dtype(dtype).type
    ids = np.asarray(ids)
    v = np.asarray(values).astype(dtype)
    if not np.isfinite(v).all():
        raise ValueError("GenericDescriptorOutlierFilter: values must be finite (deviation b)")
    has = ids >= 0
    d = np.zeros(ids.shape, dtype=dtype)
    d[has] = v[ids[has]]
    if mode == "larger":
        w = np.where(has & (d > T(threshold)), T(1), T(0))
    elif mode == "smaller":
        w = np.where(has & (d < T(threshold)), T(1), T(0))
    elif mode == "soft":
        if (v < 0).any():
            raise ValueError("GenericDescriptorOutlierFilter: soft mode needs values >= 0 (deviation b)")
        mx = d[has].max() if has.any() else T(0)
        if not mx > 0:
            return np.zeros(ids.shape, dtype=dtype)
        w = np.where(has, d / T(mx), T(0))
    else:
        raise ValueError(mode)
    return w.astype(dtype)


def kept_and_overlap(ids, d2, limit, weights, dtype=np.float32):
    """What pgicp_stats reports from one iteration's pairs: n_kept (pairs of nonzero combined weight) and overlap (the sum of the
    combined weights over knn * N), for a TrimmedDist (+ MaxDist) chain whose threshold is `limit` (squared).  The distance
    filter's weight is 1 for a pair with a neighbour within the limit; the combined weight multiplies it with `weights` in T."""
    T = np.dtype(dtype).type
    ids = np.asarray(ids)
    d2 = np.asarray(d2, dtype=dtype)
    dist = np.where((ids >= 0) & (d2 <= T(limit)), T(1), T(0))
    w = (dist * np.asarray(weights, dtype=dtype)).astype(dtype)
    return int((w != 0).sum()), float(w.astype(np.float64).sum()) / ids.size
