"""Reference statement of the sensor-noise getOverlap() (include/pgicp_noise.h), in numpy.

Input: the exact last matches of an ICP call (squared distances d2, one per pair) and the chain's outlier weights for them,
taken from the oracle's own filters; the reading's noise row.  The device adds the kept pairs' distances in double in a
parallel tree; whatever the order, a double sum of nb non-negative terms lies within nb * 2^-53 (relative) of the exact sum.
So the set of means the device may form is DERIVED, not measured:

    m*   = fsum(dist) / nb                         (exact sum, one rounding)
    f32:   m* rounded to float -- and a neighbouring float only if m* lies within nb * 2^-53 * m* of the rounding boundary
           between the two;
    f64:   the interval m* (1 -+ nb * 2^-53).

count_bounds returns the smallest and the largest count over that set: count = #{kept e : dist_e < mean + noise_e}, the
comparison and the addition in T.  The count is monotone in the mean, so the ends of the set give the bounds.

near_mean_pairs gives the bound against the oracle's orc_sensor_noise_overlap, which adds the distances one after the other
in T: that sum is within nb * eps(T) (relative) of the exact one, so only kept pairs with |dist - noise - m*| <= nb eps(T) m*
can count differently.
"""
import math

import numpy as np


def _kept(d2, w, noise, dtype):
    T = np.dtype(dtype).type
    d2 = np.asarray(d2, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    n = len(noise)
    d2 = d2.reshape(n, -1)
    w = w.reshape(n, -1)
    keep = w != 0
    dist = np.sqrt(d2[keep])                                   # correctly rounded in T
    assert dist.dtype == np.dtype(dtype)
    noise_e = np.broadcast_to(np.asarray(noise, dtype=dtype)[:, None], d2.shape)[keep]
    del T
    return dist, noise_e


def _count(dist, noise_e, mean, dtype):
    T = np.dtype(dtype).type
    return int(np.count_nonzero(dist < (T(mean) + noise_e)))   # T + T array -> T


def exact_mean(dist):
    return math.fsum(float(v) for v in dist) / len(dist)


def count_bounds(d2, w, noise, dtype, rel=None):
    """(count_lo, count_hi, nb, m*).  rel: the relative half-width of the band of reachable sums (default nb * 2^-53)."""
    dist, noise_e = _kept(d2, w, noise, dtype)
    nb = int(dist.size)
    if nb == 0:
        return 0, 0, 0, float("nan")
    m = exact_mean(dist)
    if rel is None:
        rel = nb * 2.0 ** -53
    if np.dtype(dtype) == np.float32:
        f = np.float32(m)
        means = {float(f)}
        for other in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
            boundary = 0.5 * (float(f) + float(other))
            if abs(m - boundary) <= rel * m:
                means.add(float(other))
        if rel * m > abs(float(np.nextafter(f, np.float32(np.inf))) - float(f)):        # a band wider than a float step
            means.add(float(np.float32(m * (1.0 - rel))))
            means.add(float(np.float32(m * (1.0 + rel))))
        lo, hi = min(means), max(means)
    else:
        lo, hi = m * (1.0 - rel), m * (1.0 + rel)
    return _count(dist, noise_e, lo, dtype), _count(dist, noise_e, hi, dtype), nb, m


def near_mean_pairs(d2, w, noise, dtype):
    """kept pairs whose dist - noise lies within nb * eps(T) * m* of m*: how far a sequential sum in T may move the count"""
    dist, noise_e = _kept(d2, w, noise, dtype)
    nb = int(dist.size)
    if nb == 0:
        return 0
    m = exact_mean(dist)
    band = nb * float(np.finfo(dtype).eps) * m
    return int(np.count_nonzero(np.abs(dist.astype(np.float64) - noise_e.astype(np.float64) - m) <= band))
