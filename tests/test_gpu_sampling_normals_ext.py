"""pgicp_sampling_surface_normal_ext_* (include/pgicp_ssn_ext.h) on the device: the new rows against the numpy reference
(tests/sampling_normals_ext_ref.py, pinned by the oracle on the CPU) bit for bit, the older outputs against
pgicp_sampling_surface_normal_* byte for byte -- with every new row, with none, with each alone --, the identities of the header per
kept point, and the refusals.  Every case runs in both types and in host and device memory.  Every cloud is small; the references
are computed once (the reference module caches its cases)."""
import numpy as np
import pytest

import sampling_normals_ext_ref as ref
from pgslam_amd import icp

pytestmark = pytest.mark.gpu

CASES = ref.cases()
OLD = ("xyz", "normals", "kept_idx", "descriptors")
NEW = ("eigen_values", "eigen_vectors", "densities")
WANT = dict(eigen_values="want_eigen", eigen_vectors="want_eigen_vectors", densities="want_densities")
ALL = dict(want_eigen=True, want_eigen_vectors=True, want_densities=True)


@pytest.fixture(scope="module")
def gctx():
    c = icp.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()              # (a copy: the reference's arrays are read-only)


def host(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()


def same(a, b, what):
    a, b = host(a), host(b)
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), (what, a, b)


def descriptor_forms(c):
    """0 and 3 descriptor rows, with and without averaging (the rows ride along; the cases of knn 7 carry them)"""
    return ((0, True), (3, True), (3, False)) if c[2] == 7 else ((0, True),)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("c", CASES, ids=ref.case_id)
def test_new_rows_older_outputs_and_identities(gctx, c, mem):
    name, T, knn, ratio, method, max_box = c
    for drows, average in descriptor_forms(c):
        xyz, d, r = ref.case(c, drows, average)
        what = (ref.case_id(c), mem, drows, average)
        x, dd = (xyz, d) if mem == "host" else (dev(xyz), dev(d))
        kw = dict(knn=knn, ratio=ratio, sampling_method=method, max_box_dim=max_box, seed=ref.SEED, descriptors=dd, average_descriptors=average)
        old = gctx.sampling_surface_normal(x, **kw)
        e = gctx.sampling_surface_normal_ext(x, **kw, **ALL)
        # the new rows: the reference's, bit for bit (and with them what the reference says of the older outputs)
        assert e["boxes"] == r["boxes"] == old["boxes"], what
        for key in NEW + OLD:
            same(e[key], r[key], what + (key, "reference"))
        # the older outputs: the older call's, byte for byte -- with every new row, with none, with each alone
        for key in OLD:
            same(e[key], old[key], what + (key, "all"))
        none = gctx.sampling_surface_normal_ext(x, **kw)
        assert none["boxes"] == old["boxes"] and all(none[k] is None for k in NEW), what
        for key in OLD:
            same(none[key], old[key], what + (key, "none"))
        for key in NEW if drows == 0 else ():                        # (the descriptor rows have no part in which rows are asked for)
            one = gctx.sampling_surface_normal_ext(x, **kw, **{WANT[key]: True})
            assert one["boxes"] == old["boxes"] and all(one[k] is None for k in NEW if k != key), what
            same(one[key], e[key], what + (key, "alone"))
            for k in OLD:
                same(one[k], old[k], what + (k, "beside", key))
        # the identities, per kept point
        g = {k: host(e[k]) for k in NEW + ("normals",)}
        ref.identities(g, method)
        order = np.argsort(r["box_of"], kind="stable")
        twin = np.flatnonzero(np.diff(r["box_of"][order]) == 0)
        assert method == 0 or len(twin) == 0
        for key in NEW:
            a = g[key][order]
            assert np.array_equal(a[twin], a[twin + 1]), what + (key, "one box, one row")


@pytest.mark.parametrize("T", ref.TYPES)
def test_without_normals_and_on_an_empty_cloud(gctx, T):
    c = ("cloud3000", T, 7, 0.5, 0, np.inf)
    xyz, _, r = ref.case(c)
    e = gctx.sampling_surface_normal_ext(xyz, knn=7, ratio=0.5, seed=ref.SEED, want_normals=False, **ALL)
    assert e["normals"] is None
    for key in NEW + ("xyz", "kept_idx"):
        same(e[key], r[key], key)
    e = gctx.sampling_surface_normal_ext(np.zeros((0, 3), dtype=T), **ALL)
    assert len(e["kept_idx"]) == 0 and e["boxes"] == 0 and all(len(e[k]) == 0 for k in NEW)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("T", ref.TYPES)
def test_refused_as_the_older_call_refuses_and_the_context_stays_usable(gctx, T, mem):
    xyz, _, r = ref.case(("cloud3000", T, 7, 0.5, 0, np.inf))
    put = (lambda a: a) if mem == "host" else dev
    bad_clouds = []
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[17, 1] = bad
        bad_clouds.append(dict(xyz=put(x)))
    refused = bad_clouds + [dict(xyz=put(xyz), knn=2), dict(xyz=put(xyz), knn=1025), dict(xyz=put(xyz), sampling_method=2),
                            dict(xyz=put(xyz), sampling_method=-1)]
    for kw in refused:
        for call, more in ((gctx.sampling_surface_normal, {}), (gctx.sampling_surface_normal_ext, ALL), (gctx.sampling_surface_normal_ext, {})):
            with pytest.raises(icp.PgicpError) as err:
                call(**kw, **more)
            assert err.value.code == icp.ERR_ARG, kw
        # the context is still good, and gives what it gave
        e = gctx.sampling_surface_normal_ext(put(xyz), knn=7, ratio=0.5, seed=ref.SEED, **ALL)
        for key in NEW + ("xyz", "normals", "kept_idx"):
            same(e[key], r[key], key)
