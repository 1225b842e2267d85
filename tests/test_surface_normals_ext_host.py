"""include/pgicp_normals_ext.h without a device: the numpy reference (tests/surface_normals_ext_ref.py) pinned by the oracle on every
scene in both types, its known answers on the exact plane, the degenerate defaults, the unit length of the smoothed normals, and
the conditions the GPU tests rest on (the superset clouds' short lists, no zero dot product in the sign-flip scene)."""
import numpy as np
import pytest

import surface_normals_ext_ref as ref

TYPES = ref.TYPES


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", sorted(ref.SCENES))
def test_reference_is_pinned_by_the_oracle(name, T):
    xyz, knn, md, o, r = ref.scene(name, T)
    ref.pinned(r, o)
    assert r["eigen_vectors"].dtype == T and r["eigen_vectors"].shape == (len(xyz), 9)
    assert r["matched_ids"].dtype == T and np.array_equal(r["matched_ids"].astype(np.int64), o["ids"])
    assert r["mean_dists"].dtype == T and np.all(np.isfinite(r["mean_dists"])) and np.all(r["mean_dists"] >= 0)
    # a non-degenerate point's columns are an orthonormal frame (Jacobi's V is a product of rotations)
    nd = ~np.all(r["eigen_vectors"] == np.array(ref.DEFAULT_COLUMNS, dtype=T), axis=1)
    V = r["eigen_vectors"][nd].astype(np.float64).reshape(-1, 3, 3)
    if len(V):
        assert np.abs(V @ V.transpose(0, 2, 1) - np.eye(3)).max() < 8 * np.finfo(T).eps


@pytest.mark.parametrize("T", TYPES)
def test_plane_known_answers(T, oracle32, oracle64):
    xyz, interior = ref.plane_case(T)
    o = (oracle32 if T == np.float32 else oracle64).surface_normals(xyz, 5, np.inf)
    r = ref.rows(xyz, o["ids"], T)
    ref.pinned(r, o)
    assert len(interior) == 100
    assert np.array_equal(r["normals"][interior], np.tile(np.array([0, 0, 1], dtype=T), (100, 1)))
    assert np.array_equal(r["eigen_vectors"][interior], np.tile(np.array([0, 0, 1, 0, 1, 0, 1, 0, 0], dtype=T), (100, 1)))      # e_z, e_y, e_x
    s2 = T(2 * 0.125 * 0.125)
    assert np.array_equal(r["eigen_values"][interior], np.tile(np.array([0, s2, s2], dtype=T), (100, 1)))
    assert np.all(r["mean_dists"][interior] == 0)
    sm = ref.smooth(r["normals"], o["ids"], T)
    assert sm[interior].tobytes() == r["normals"][interior].tobytes()


@pytest.mark.parametrize("T", TYPES)
def test_degenerate_and_lonely_points_take_the_default_columns(T):
    for name in ("line", "lonely"):
        xyz, knn, md, o, r = ref.scene(name, T)
        assert np.array_equal(r["eigen_vectors"], np.tile(np.array(ref.DEFAULT_COLUMNS, dtype=T), (len(xyz), 1)))
        assert np.array_equal(r["eigen_values"], np.tile(np.array([0, 0, 1], dtype=T), (len(xyz), 1)))
        assert r["smoothed"].tobytes() == r["normals"].tobytes()                       # every neighbour's normal is (0,1,0)
    _, _, _, o, r = ref.scene("lonely", T)
    assert np.array_equal(r["matched_ids"], np.array([[0, -1, -1], [1, -1, -1], [2, -1, -1]], dtype=T))
    assert np.all(r["mean_dists"] == 0)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", sorted(ref.SCENES))
def test_smoothed_normals_have_unit_length(name, T):
    """|a / len| : three roundings in the sum of squares, one in the root, one per division -- each a relative eps / 2 at most on a
    quantity of size about 1, so | |n| - 1 | <= 4 eps with room to spare"""
    _, _, _, _, r = ref.scene(name, T)
    ln = np.sqrt(np.sum(r["smoothed"].astype(np.float64) ** 2, axis=1))
    assert np.abs(ln - 1).max() <= 4 * np.finfo(T).eps


@pytest.mark.parametrize("T", TYPES)
def test_sign_flip_scene_has_no_zero_dot_product(T):
    """the condition of tests/test_gpu_surface_normals_ext.py's sign-rule test: d > 0 and d < 0 are then each other's complement"""
    nrm, ids, flip = ref.sign_flip_case("random", T)
    assert 0.4 < flip.mean() < 0.6
    d = ref.smooth_dots(nrm, ids, T)
    assert not np.any(d == 0)
    raw = ref.smooth(ref.scene("random", T)[4]["normals"], ids, T)
    out = ref.smooth(nrm, ids, T)
    assert out[~flip].tobytes() == raw[~flip].tobytes()
    # exactly the negated value; not the negated bytes: a sum that starts at +0 and adds -0 stays +0, so a component that is zero
    # (the default normal (0,1,0) has two) keeps its sign where every other component changes it
    assert np.array_equal(out[flip], -raw[flip])
    nz = raw[flip] != 0
    assert out[flip][nz].tobytes() == (-raw[flip][nz]).tobytes()


@pytest.mark.parametrize("T", TYPES)
def test_superset_clouds_have_short_lists(T, oracle32, oracle64):
    """the finite maxDist of the superset test: at least 5 % of the points have cnt < knn and some have cnt = 1, at every n and knn"""
    o = oracle32 if T == np.float32 else oracle64
    for n in ref.SUPERSET_N:
        xyz = ref.superset_cloud(n, T)
        for knn in ref.SUPERSET_KNN:
            cnt = (o.surface_normals(xyz, knn, ref.SUPERSET_MAX_DIST)["ids"] >= 0).sum(1)
            assert (cnt < knn).mean() >= 0.05 and np.any(cnt == 1), (n, knn)
            assert np.all(cnt >= 1)
