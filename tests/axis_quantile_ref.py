"""MaxQuantileOnAxisDataPointsFilter's statement (include/pgicp_quantile.h) in numpy, and the scenes every form of it is tested on.

The reference: k = int(T(n) * T(ratio)), clamped to n - 1; limit = np.partition(v, k)[k] -- numpy's sort order places NaN last and
holds -0 equal to +0, the order of the header's DEVIATION (a) --; keep = v < limit.  The limit is compared canonically (+0 for
either zero, NaN for any NaN), as the header reports it.

The scenes are the smallest that can break a radix select: sizes around the block and tile sizes, ratios from "nothing" to "all but
the top", and value sets that put the whole decision into the lowest key bits, the highest, one bin, a tie, or the specials.
"""
import struct

import numpy as np

SIZES = (1, 2, 90, 255, 256, 257, 4097, 65537)
RATIOS = (1e-7, 0.3, 0.5, 0.7, 0.998, 0.9999999)
VALUE_SETS = ("mixed", "equal", "half_ties", "low8", "top_bits", "upper32_equal", "planar", "all_nan")


def rank(n, ratio, T):
    """k of the statement: the product rounded in T, truncated, clamped to n - 1"""
    k = int(T(n) * T(ratio))
    return max(0, min(k, n - 1))


def canonical(x):
    """a limit as the header reports it, as bytes: +0 for either zero, one NaN for every NaN"""
    x = np.asarray(x)
    T = x.dtype.type
    if np.isnan(x):
        return b"nan"
    return (T(0) if x == 0 else T(x)).tobytes()


def select(v, ratio):
    """(limit, k, number of values < limit) of the values v (1-D, float32 or float64); n == 0: (NaN, 0, 0)"""
    v = np.asarray(v)
    T = v.dtype.type
    if len(v) == 0:
        return T(np.nan), 0, 0
    k = rank(len(v), ratio, T)
    limit = np.partition(v, k)[k]
    return limit, k, int(np.count_nonzero(v < limit))


def keep_mask(v, ratio):
    v = np.asarray(v)
    if len(v) == 0:
        return np.zeros(0, dtype=bool)
    limit, _, _ = select(v, ratio)
    return v < limit


def _bits(T):
    return (np.uint32, 32) if T == np.float32 else (np.uint64, 64)


def values(name, n, T, rng, ratio_for_ties=0.5):
    """the n axis values of one value set"""
    U, kb = _bits(T)
    tiny = np.finfo(T).tiny
    if name == "mixed":
        v = (rng.normal(size=n) * 10.0).astype(T)
        special = np.array([0.0, -0.0, np.inf, -np.inf, tiny / 4, -tiny / 4, np.nan, np.nan, tiny / 8, -0.0, 0.0], dtype=T)
        if n < 16:
            v[:] = np.resize(np.roll(special, n), n)
        else:
            pos = rng.choice(n, size=len(special), replace=False)
            v[pos] = special
        return v
    if name == "equal":
        return np.full(n, 3.25, dtype=T)
    if name == "half_ties":
        # half the values equal the limit: `low` values below it, the tie group, the rest above; the rank falls into the group
        k = rank(n, ratio_for_ties, T)
        ties = max(1, n // 2)
        low = max(0, k - n // 4)
        low = min(low, n - ties)
        v = np.concatenate([rng.uniform(-5.0, 0.5, low), np.full(ties, 1.0), rng.uniform(1.5, 9.0, n - ties - low)]).astype(T)
        rng.shuffle(v)
        return v
    if name == "low8":
        base = np.array([1.5], dtype=T).view(U)[0]
        return (base + rng.integers(0, 256, n).astype(U)).view(T)
    if name == "top_bits":
        return (rng.integers(0, 4096, n).astype(U) << U(kb - 12)).view(T)
    if name == "upper32_equal":
        base = np.array([-2.5], dtype=np.float64).view(np.uint64)[0]
        return (base + rng.integers(0, 2 ** 32, n, dtype=np.uint64)).view(np.float64).astype(T)
    if name == "planar":
        return (2.0 + rng.uniform(0.0, 0.1, n)).astype(T)          # one bin of the first level holds every value
    if name == "all_nan":
        return np.full(n, np.nan, dtype=T)
    raise KeyError(name)


_groups = {}


def groups(T):
    """[(id, dim, features (n, 4), ratios)]: every value set at every size, made once per dtype and never changed.  The axis values
    sit in column `dim`; the other coordinates are ordinary, but for a NaN here and there (a point is kept or dropped by its axis
    value alone); column 3 is the homogeneous 1.  half_ties is made per ratio (the tie group must hold the rank)."""
    T = np.dtype(T).type
    if T in _groups:
        return _groups[T]
    out = []
    rng = np.random.default_rng(20240607)
    j = 0
    for name in VALUE_SETS:
        if name == "upper32_equal" and T == np.float32:
            continue
        for n in SIZES:
            per_ratio = RATIOS if name == "half_ties" else (None,)
            for r in per_ratio:
                dim = j % 3
                j += 1
                f = np.ones((n, 4), dtype=T)
                f[:, :3] = (rng.normal(size=(n, 3)) * 4.0).astype(T)
                f[:, dim] = values(name, n, T, rng, r if r is not None else 0.5)
                if n >= 4:
                    f[rng.choice(n, size=max(1, n // 64), replace=False), (dim + 1) % 3] = np.nan
                f.setflags(write=False)
                out.append((f"{name}-n{n}" + (f"-r{r}" if r is not None else ""), dim, f, (r,) if r is not None else RATIOS))
    _groups[T] = out
    return out


_scenes = {}


def scenes(T):
    """[(id, dim, features, ratio, (limit, k, below), keep mask)]: the groups with every ratio, and the reference's answer"""
    T = np.dtype(T).type
    if T not in _scenes:
        out = []
        for gid, dim, f, ratios in groups(T):
            for r in ratios:
                v = f[:, dim]
                out.append((f"{gid}@{r}", dim, f, r, select(v, r), keep_mask(v, r)))
        _scenes[T] = out
    return _scenes[T]


def write_groups(path, T):
    """the groups as the C++ test programs read them: int32 count; per group int32 n, dim, number of ratios, the ratios as double,
    the features (n, 4) row-major in T"""
    with open(path, "wb") as fh:
        gs = groups(T)
        fh.write(struct.pack("<i", len(gs)))
        for _, dim, f, ratios in gs:
            fh.write(struct.pack("<iii", len(f), dim, len(ratios)) + struct.pack("<%dd" % len(ratios), *ratios) + f.tobytes())


def read_results(path, T):
    """what the programs write, one record per scene in scenes(T)'s order: limit (T), k, below, kept count (int32), the kept indices"""
    T = np.dtype(T)
    b = open(path, "rb").read()
    out, off = [], 0
    while off < len(b):
        limit = np.frombuffer(b, dtype=T, count=1, offset=off)[0]
        k, below, kept = struct.unpack_from("<iii", b, off + T.itemsize)
        off += T.itemsize + 12
        out.append((limit, k, below, np.frombuffer(b, dtype=np.int32, count=kept, offset=off)))
        off += 4 * kept
    return out
