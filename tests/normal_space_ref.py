"""[EXT] NormalSpaceDataPointsFilter as include/pgicp_normalspace.h states it, in plain Python / numpy, written twice: `literal`
keeps per-bucket Python lists and pops the drawn bucket from a plain list, `sorted_form` orders the points with np.lexsort on
(bucket, r, i) and draws through a Fenwick tree over the buckets' counts.  Both return dict(kept_idx, bucket), one entry per pick in
pick order; coordinates, normals and descriptor rows are the kept points' own.  The angles are libm's (math.acos / math.atan2 /
math.fmod), as the statement says of the reference.  CASES is the list of clouds and parameters the host and the device tests
share; case_inputs asserts that no point of a case lies in the statement's band of freedom."""
import functools
import math
import os
import struct

import numpy as np

M64 = (1 << 64) - 1
MAX_BUCKETS = 65536
PI = math.pi
BAND = 1e-9


def mix(z):
    """the SplitMix64 finaliser of RandomSamplingDataPointsFilter, in Python integers"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def grid(epsilon):
    """(nPhi, nTheta); ValueError outside the statement's bounds"""
    epsilon = float(epsilon)
    if not math.isfinite(epsilon) or not epsilon > 0.0 or not epsilon <= PI:
        raise ValueError("epsilon")
    n_phi, n_theta = math.ceil(2.0 * PI / epsilon), math.ceil(PI / epsilon)
    if n_phi * n_theta > MAX_BUCKETS:
        raise ValueError("too many buckets")
    return n_phi, n_theta


def angles(normal):
    """(theta, phi) of one normal (three Python floats holding the T-valued components), after the wraps"""
    nx, ny, nz = normal
    z = max(min(nz, 1.0), -1.0)
    theta = math.acos(z)
    phi = math.fmod(math.atan2(ny, nx) + 2.0 * PI, 2.0 * PI)
    if theta == PI:
        theta = 0.0
    if phi == 2.0 * PI:
        phi = 0.0
    return theta, phi


def bucket_of(normal, epsilon, n_phi, n_theta):
    theta, phi = angles(normal)
    it, ip = min(int(math.floor(theta / epsilon)), n_theta - 1), min(int(math.floor(phi / epsilon)), n_phi - 1)
    return it * n_phi + ip


def _check(nrm, nb_sample, seed, T):
    assert nrm.dtype == T and nrm.ndim == 2 and nrm.shape[1] == 3
    if nb_sample < 1 or not 0 <= seed < (1 << 53):
        raise ValueError("bad parameter")


def _finish(kept, bucket):
    return dict(kept_idx=np.array(kept, dtype=np.int32), bucket=np.array(bucket, dtype=np.int32))


def _buckets(nrm, epsilon):
    n_phi, n_theta = grid(epsilon)
    if not np.isfinite(nrm).all():
        raise ValueError("a normal component is not finite")
    return [bucket_of([float(v) for v in row], float(epsilon), n_phi, n_theta) for row in nrm], n_phi * n_theta


def literal(nrm, nb_sample, epsilon, seed, T):
    """per-bucket lists, the non-empty list a plain Python list"""
    _check(nrm, nb_sample, seed, T)
    n = len(nrm)
    if nb_sample >= n:
        grid(epsilon)
        return _finish(list(range(n)), [-1] * n)
    b, nb_bucket = _buckets(nrm, epsilon)
    lists = {}
    for i in range(n):
        lists.setdefault(b[i], []).append((mix((seed * 0x100000001B3 + i) & M64) >> 40, i))
    for v in lists.values():
        v.sort()
    alive = sorted(lists)
    kept, bucket = [], []
    base = ~(seed * 0x100000001B3) & M64
    for j in range(nb_sample):
        r = (mix((base + j) & M64) >> 11) % len(alive)
        k = alive[r]
        kept.append(lists[k].pop(0)[1])
        bucket.append(k)
        if not lists[k]:
            alive.pop(r)
    return _finish(kept, bucket)


def sorted_form(nrm, nb_sample, epsilon, seed, T):
    """np.lexsort on (bucket, r, i) and a Fenwick draw over the counts"""
    _check(nrm, nb_sample, seed, T)
    n = len(nrm)
    if nb_sample >= n:
        grid(epsilon)
        return _finish(np.arange(n), np.full(n, -1))
    b, nb_bucket = _buckets(nrm, epsilon)
    b = np.array(b, dtype=np.int64)
    r = np.array([mix((seed * 0x100000001B3 + i) & M64) >> 40 for i in range(n)], dtype=np.int64)
    order = np.lexsort((np.arange(n), r, b))
    counts = np.bincount(b, minlength=nb_bucket)
    start = np.concatenate([[0], np.cumsum(counts)])
    tree = [0] * (nb_bucket + 1)

    def add(k, v):
        k += 1
        while k <= nb_bucket:
            tree[k] += v
            k += k & -k

    def select(r):
        """the 0-based position of the r-th (0-based) set flag"""
        pos, step = 0, 1 << nb_bucket.bit_length()
        while step:
            if pos + step <= nb_bucket and tree[pos + step] <= r:
                pos += step
                r -= tree[pos]
            step >>= 1
        return pos

    m = 0
    for k in np.nonzero(counts)[0]:
        add(int(k), 1)
        m += 1
    taken = np.zeros(nb_bucket, dtype=np.int64)
    kept, bucket = [], []
    base = ~(seed * 0x100000001B3) & M64
    for j in range(nb_sample):
        k = select((mix((base + j) & M64) >> 11) % m)
        kept.append(int(order[start[k] + taken[k]]))
        bucket.append(k)
        taken[k] += 1
        if taken[k] == counts[k]:
            add(k, -1)
            m -= 1
    return _finish(kept, bucket)


# ---- the clouds and cases the host and the device tests share ----------------------------------------------------------------
def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def _direction(theta, phi):
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=-1)


# the hand-written pole and seam cloud, epsilon 0.5: nPhi 13, nTheta 7; the zero normal and every normal on the equator sit in
# row floor((pi / 2) / 0.5) = 3
POLES = np.array([
    [0.0, 0.0, 1.0],              # theta 0, phi 0                                               -> 0
    [0.0, 0.0, -1.0],             # theta pi wraps to 0                                          -> 0
    [0.0, 0.0, 1.0000001],        # the clamp (as float 1 + 2^-23)                               -> 0
    [0.0, 0.0, 0.0],              # the zero normal: theta pi / 2, phi 0                         -> 39
    [1.0, -1e-30, 0.0],           # atan2 = -1e-30, + 2 pi = 2 pi, fmod = 0                      -> 39
    [-1.0, 0.0, 0.0],             # atan2(+0, -1) = pi: floor(pi / 0.5) = 6                      -> 45
    [-1.0, -0.0, 0.0],            # atan2(-0, -1) = -pi, + 2 pi = pi                             -> 45
    [1.0, 0.0, 0.0],              # phi 0                                                        -> 39
    [1.0, -0.0, 0.0],             # atan2(-0, 1) = -0, + 2 pi = 2 pi, fmod = 0                   -> 39
    [0.0, -1.0, 0.0],             # atan2 = -pi / 2: phi = 3 pi / 2, floor(9.42) = 9             -> 48
    [0.0, 0.0, -0.5],             # theta 2 pi / 3 = 2.094: row 4, phi 0                         -> 52
], dtype=np.float64)
POLES_EPSILON = 0.5
POLES_BUCKETS = [0, 0, 0, 39, 39, 45, 45, 39, 39, 48, 52]
HAND_CLOUDS = ("poles",)


def normals(name):
    """float64 (n, 3); the tests round it to T"""
    rng = np.random.default_rng(abs(hash_name(name)))
    if name == "poles":
        return POLES.copy()
    if name.startswith("n"):
        v = rng.normal(size=(int(name[1:]), 3))
        return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    eps = 0.09
    if name == "one_bucket":                                       # 20001 normals inside one bucket of epsilon 0.09
        return _direction((11.5 + rng.uniform(-0.3, 0.3, 20001)) * eps, (20.5 + rng.uniform(-0.3, 0.3, 20001)) * eps)
    if name == "two_planes":                                       # 4000 + 97 points, two buckets of epsilon 0.09, interleaved
        th = np.concatenate([np.full(4000, 5.5), np.full(97, 17.5)]) + rng.uniform(-0.2, 0.2, 4097)
        ph = np.concatenate([np.full(4000, 3.5), np.full(97, 0.5)]) + rng.uniform(-0.2, 0.2, 4097)
        return _direction(th * eps, ph * eps)[rng.permutation(4097)]
    if name == "one_each":                                         # one point in each of the 91 buckets of epsilon 0.5
        e = 0.5
        n_phi, n_theta = grid(e)
        t, p = np.meshgrid(np.arange(n_theta), np.arange(n_phi), indexing="ij")
        th = 0.5 * (t * e + np.minimum((t + 1) * e, PI))
        ph = 0.5 * (p * e + np.minimum((p + 1) * e, 2 * PI))
        return _direction(th.ravel(), ph.ravel())[rng.permutation(n_phi * n_theta)]
    raise KeyError(name)


def descriptors(n, drows, T):
    if drows == 0:
        return None
    return np.random.default_rng(7 + drows).normal(size=(n, drows)).astype(T)


# (cloud, nbSample, epsilon, stride, drows)
CASES = [
    ("n0", 1, 0.09, 3, 0),
    ("n1", 1, 0.09, 3, 3), ("n1", 2, 0.5, 4, 0),                  # the no-op: n and n + 1
    ("n2", 1, PI, 3, 0), ("n2", 2, 0.09, 3, 7), ("n2", 3, 0.09, 4, 0),
    ("n255", 1, 0.09, 3, 0), ("n255", 254, 0.5, 4, 3), ("n255", 64, PI, 3, 0),
    ("n256", 64, 0.09, 4, 7), ("n256", 255, 0.0175, 3, 0), ("n256", 256, 0.09, 3, 3), ("n256", 257, 0.09, 3, 0),
    ("n257", 256, PI, 3, 3), ("n257", 64, 0.0175, 3, 0), ("n257", 1, 0.5, 4, 7),
    ("n300", 1, 0.09, 3, 3), ("n300", 256, 0.09, 4, 3), ("n300", 257, 0.09, 3, 3), ("n300", 300, 0.09, 4, 3),   # the gather's block edge
    ("n4097", 1024, 0.09, 3, 0), ("n4097", 4096, 0.5, 4, 3), ("n4097", 1, 0.0175, 3, 7), ("n4097", 1024, PI, 3, 0),
    ("n4097", 4097, 0.09, 3, 0), ("n4097", 4098, 0.09, 4, 3),
    ("n20001", 5000, 0.09, 3, 3), ("n20001", 20000, 0.09, 4, 0), ("n20001", 5000, 0.0175, 3, 0), ("n20001", 1, 0.5, 3, 0),
    ("n20001", 20001, 0.09, 3, 0), ("n20001", 20002, 0.5, 3, 7),   # several tiles of the sort and chunks of the scan
    ("one_bucket", 10000, 0.09, 3, 0),                             # ties of r_i inside the one bucket
    ("one_each", 90, 0.5, 3, 3), ("one_each", 23, 0.5, 4, 0),      # every pick empties a bucket
    ("two_planes", 300, 0.09, 3, 3),                               # the small bucket empties mid-draw
    ("poles", 4, POLES_EPSILON, 3, 0), ("poles", 10, POLES_EPSILON, 4, 3),
]
SEED = 12345


def case_id(case):
    name, nb, eps, stride, drows = case
    return f"{name}-k{nb}-e{eps:.4g}-st{stride}-d{drows}"


def _assert_out_of_band(name, nrm, epsilon):
    """no theta / epsilon or phi / epsilon within BAND of an integer -- a condition on the inputs, not a tolerance on the outputs.
    The exception: an angle of a hand-written cloud that is exactly 0 in double (nz = +-1, nx = ny = 0, ny = +-0 with nx != 0, a
    phi that wraps to 0), which every platform computes as exactly 0."""
    for i, row in enumerate(nrm):
        for a in angles([float(v) for v in row]):
            if a == 0.0 and name in HAND_CLOUDS:
                continue
            q = a / epsilon
            assert abs(q - round(q)) > BAND, (name, i, row, q, "change the cloud's seed")


@functools.lru_cache(maxsize=None)
def case_inputs(case, T):
    """(xyz (n, 3), normals (n, 3), desc (n, drows) or None) in T; shared, read-only"""
    name, nb, eps, _, drows = case
    nrm = np.ascontiguousarray(normals(name).reshape(-1, 3), dtype=T)
    n = len(nrm)
    if nb < n:
        _assert_out_of_band(name, nrm, float(eps))
    x = np.random.default_rng(11 + n).uniform(-10, 10, size=(n, 3)).astype(T)
    d = descriptors(n, drows, T)
    for v in (x, nrm, d):
        if v is not None:
            v.setflags(write=False)
    return x, nrm, d


@functools.lru_cache(maxsize=None)
def case_expected(case, T):
    """the reference's result of a case (the sorted form), computed once and shared: dict(kept_idx, bucket, xyz, normals, desc)"""
    _, nb, eps, _, _ = case
    x, nrm, d = case_inputs(case, T)
    want = sorted_form(nrm, nb, eps, SEED, T)
    k = want["kept_idx"]
    want.update(xyz=x[k], normals=nrm[k], desc=d[k] if d is not None else None)
    for v in want.values():
        if v is not None:
            v.setflags(write=False)
    return want


# ---- the fixture of tests/cpp/test_normal_space_cpu.cpp ------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normal_space_small.bin")
GOLDEN_CASES = [("poles", 4, POLES_EPSILON, 3, 0), ("n257", 64, 0.0175, 3, 0), ("n256", 64, 0.09, 4, 7), ("one_each", 90, 0.5, 3, 3),
                ("two_planes", 300, 0.09, 3, 3), ("n2", 2, 0.09, 3, 7)]


def golden_bytes():
    """the recorded results of GOLDEN_CASES, as float and as double: int32 count, then per record int32 n, nbSample, is_f32, m; double
    epsilon, seed; the normals (n x 3 of T); kept_idx and bucket (m int32 each)"""
    out = [struct.pack("<i", 2 * len(GOLDEN_CASES))]
    for case in GOLDEN_CASES:
        for T in (np.float32, np.float64):
            _, nb, eps, _, _ = case
            _, nrm, _ = case_inputs(case, T)
            want = case_expected(case, T)
            m = len(want["kept_idx"])
            out.append(struct.pack("<iiiidd", len(nrm), nb, int(T == np.float32), m, float(eps), float(SEED)))
            out.append(nrm.tobytes() + want["kept_idx"].tobytes() + want["bucket"].tobytes())
    return b"".join(out)


if __name__ == "__main__":
    with open(GOLDEN, "wb") as fh:
        fh.write(golden_bytes())
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
