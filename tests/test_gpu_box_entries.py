"""The three entries of the box filters -- pgicp_sampling_surface_normal_*, pgicp_sampling_surface_normal_ext_* and pgicp_elipsoids_* --
share one body, one pair of kernels and one work buffer, which each carves to its own layout (no per-box rows, three, six).  Here
they are called on ONE context in an interleaved order, then in the reverse order, and every output of every call is compared byte
for byte with the numpy statement (tests/elipsoids_ref.py at minPlanarity 0, which is SamplingSurfaceNormal's): an entry must not see
what another left in the buffer, the planarity drop of an Elipsoids call must not reach the plain entry that follows it, and the
second round allocates nothing.  knn 7, 2 descriptor rows, averaged; the sizes are the smallest at which each path of the build can
go wrong: 5 (the root is a box, identity order), 8 (one split), 31 (uneven leaves), 3000 (several levels, a multi-block scan of the
3 n marks).  The references are computed once (the reference module caches its cases)."""
import ctypes as C

import numpy as np
import pytest

import elipsoids_ref as ref
from pgslam_amd import icp

pytestmark = pytest.mark.gpu

ALL = ref.ALL
PLAIN = ("normals",)
EXT = ("normals", "eigen_values", "eigen_vectors", "densities")
SIZES = ("n5", "n8", "n31", "cloud3000")
KNN, RATIO, DROWS = 7, 0.5, 2


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                     # (a copy: the reference's arrays are read-only)


def host(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def alloc_count(ctx):
    """the library's device allocations so far (pgicp_debug_alloc_stats, process-wide)"""
    out = (C.c_longlong * 8)()
    assert ctx.lib.pgicp_debug_alloc_stats(out) == 0
    return int(out[0])


def check(e, r, rows, absent, what):
    """a call's dict against the reference's: the boxes fused, the kept points and the rows asked for bit for bit; the rows the entry
    offers but was not asked for are None"""
    assert e["boxes"] == r["boxes"], what
    for key in ("xyz", "kept_idx", "descriptors") + tuple(rows):
        a, b = host(e[key]), r[key]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, key, a, b)
    for key in absent:
        assert e[key] is None, (what, key)


def calls_of(name):
    """the interleaved sequence of one cloud: (entry, rows asked for, whether the picked minPlanarity is set)"""
    seq = [("plain", PLAIN, False), ("elipsoids", ALL, False), ("ext", EXT, False), ("elipsoids", PLAIN, False), ("plain", PLAIN, False)]
    if name == "cloud3000":
        seq += [("elipsoids", ALL, True), ("plain", PLAIN, False)]
    return seq


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("T", ref.TYPES, ids=lambda T: np.dtype(T).name)
def test_interleaved_entries_on_one_context_equal_the_reference(T, mem):
    ctx = icp.Context(0)
    try:
        put = (lambda a: a) if mem == "host" else dev
        thr = ref.pick_min_planarity(ref.cloud("cloud3000", T), T, KNN)

        def one(name, method, entry, rows, planar):
            c = (name, T, KNN, RATIO, method, np.inf)
            xyz, d, r = ref.case(c, DROWS, True, thr if planar else 0.0)
            what = (name, np.dtype(T).name, mem, method, entry, rows, planar)
            x, dd = put(xyz), put(d)
            if entry == "plain":
                e = ctx.sampling_surface_normal(x, knn=KNN, ratio=RATIO, sampling_method=method, seed=ref.SEED, descriptors=dd)
                check(e, r, rows, (), what)
            elif entry == "ext":
                e = ctx.sampling_surface_normal_ext(x, knn=KNN, ratio=RATIO, sampling_method=method, seed=ref.SEED, descriptors=dd,
                                                    want_eigen=True, want_eigen_vectors=True, want_densities=True)
                check(e, r, rows, (), what)
            else:
                e = ctx.elipsoids(x, knn=KNN, ratio=RATIO, method=method, min_planarity=thr if planar else 0.0, seed=ref.SEED, desc=dd,
                                  keep=rows)
                check(e, r, rows, tuple(k for k in ALL if k not in rows), what)
            return r

        full = {m: ref.case(("cloud3000", T, KNN, RATIO, m, np.inf), DROWS, True)[2]["boxes"] for m in (0, 1)}
        for name in SIZES:
            for method in (0, 1):
                for entry, rows, planar in calls_of(name):
                    r = one(name, method, entry, rows, planar)
                    if planar:
                        assert 0 < r["boxes"] < full[method]          # the threshold drops some boxes and not all
        before = alloc_count(ctx)
        for name in reversed(SIZES):
            for method in (1, 0):
                for entry, rows, planar in reversed(calls_of(name)):
                    one(name, method, entry, rows, planar)
        assert alloc_count(ctx) == before
    finally:
        ctx.close()
