"""numpy restatement of [EXT] VarTrimmedDistOutlierFilter (steps 1-7 of include/pgicp.h): the reference the device tests compare
against.  Sorts with np.sort, sums with np.cumsum in float64, and selects the quantile as getDistsQuantile."""
import math

import numpy as np


def dists_quantile(d, ratio, dtype):
    """getDistsQuantile: the element (int)(size * ratio) (in T) of the sorted finite entries, zeros included; the last one at ratio
    1.  Returns (limit, number of finite entries); (+inf, 0) when there is none."""
    T = np.dtype(dtype).type
    v = np.sort(d[np.isfinite(d)])
    n = len(v)
    if n == 0:
        return T(np.inf), 0
    if T(ratio) == T(1):
        k = n - 1
    else:
        k = int(T(n) * T(ratio))
        k = min(k, n - 1)
    return v[max(k, 0)], n


def var_trim(d, min_ratio, max_ratio, lam, dtype):
    """The filter on the matcher's squared distances d (every entry, +inf: no neighbour).  Returns a dict: tuned (the ratio, a
    Python float), j (j*, None when c == 0), c, P, min_el, max_el, limit, n_finite, weights, and `gap`: the relative difference
    between the two smallest FRMS values of the window (inf when it has fewer than two)."""
    T = np.dtype(dtype).type
    d = np.asarray(d, dtype=dtype).ravel()
    P = d.size
    L = np.sort(d[(d != np.inf) & (d > 0)])
    c = L.size
    out = dict(P=P, c=c)
    if c == 0:
        out.update(tuned=None, j=None, limit=None, n_finite=int(np.isfinite(d).sum()), weights=None, gap=math.inf)
        return out
    min_el = int(math.floor(T(min_ratio) * T(P)))
    max_el = int(math.floor(T(max_ratio) * T(P)))
    wend = min(max_el, c)
    S = np.cumsum(L.astype(np.float64))
    gap = math.inf
    if min_el < wend:
        j = np.arange(min_el, wend)
        idv = (j + 1).astype(np.float64)
        f = idv / float(P)
        a = 1.0 / np.power(f, float(lam))
        frms = a * a * S[min_el:wend] / idv
        jstar = int(min_el + np.argmin(frms))          # argmin: the first of equal values, as Eigen's minCoeff
        if frms.size >= 2:
            two = np.partition(frms, 1)[:2]
            gap = abs(two[1] - two[0]) / max(abs(two[0]), 1e-300)
    else:
        jstar = min_el
    tuned = float(np.float32(np.float32(jstar) / np.float32(P)))
    limit, nf = dists_quantile(d, T(tuned), dtype)
    w = (d <= limit).astype(dtype)
    out.update(tuned=tuned, j=jstar, min_el=min_el, max_el=max_el, limit=limit, n_finite=nf, weights=w, gap=gap)
    return out
