"""[EXT] NormalSpaceDataPointsFilter's statement (include/pgicp_normalspace.h) without a device: the numpy reference's two
transliterations against each other on every case the device test uses, as float and as double; the hand-written pole and seam
cloud against buckets and picks written out; what the special clouds are for; the draw's law over seeds on a two-bucket cloud; and
the fixture of the C++ test against what the reference gives now."""
import numpy as np
import pytest

import normal_space_ref as ref


def same(a, b, what=""):
    for k in ("kept_idx", "bucket"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, a[k], b[k])


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_the_two_transliterations_agree(T):
    for case in ref.CASES:
        _, nb, eps, _, _ = case
        _, nrm, _ = ref.case_inputs(case, T)
        want = ref.case_expected(case, T)
        same(ref.literal(nrm, nb, eps, ref.SEED, T), want, ref.case_id(case))
        assert len(want["kept_idx"]) == min(len(nrm), nb)
        if nb >= len(nrm):
            assert (want["kept_idx"] == np.arange(len(nrm))).all() and (want["bucket"] == -1).all()
        else:
            assert len(np.unique(want["kept_idx"])) == nb          # no point is taken twice


# The picks of the pole and seam cloud with seed 12345: recorded from the reference once and checked by hand against the law --
# the buckets present are 0 {0, 1, 2}, 39 {3, 4, 7, 8}, 45 {5, 6}, 48 {9}, 52 {10}; 48 and 52 leave the list at picks 2 and 3,
# 45 at pick 4, and every bucket hands its points out in one fixed order (0: 2, 1, 0; 39: 7, 8, 3, (4); 45: 6, 5).
POLES_PICKS = [6, 2, 9, 10, 5, 7, 1, 0, 8, 3]
POLES_PICK_BUCKETS = [45, 0, 48, 52, 45, 39, 0, 0, 39, 39]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_hand_written_pole_and_seam_cloud(T):
    nrm = np.ascontiguousarray(ref.POLES, dtype=T)
    assert nrm[2, 2] > 1                                           # the clamp is exercised in both precisions
    n_phi, n_theta = ref.grid(ref.POLES_EPSILON)
    assert (n_phi, n_theta) == (13, 7)
    assert [ref.bucket_of([float(v) for v in row], ref.POLES_EPSILON, n_phi, n_theta) for row in nrm] == ref.POLES_BUCKETS
    for nb in (4, 10):
        want = dict(kept_idx=np.array(POLES_PICKS[:nb], dtype=np.int32), bucket=np.array(POLES_PICK_BUCKETS[:nb], dtype=np.int32))
        same(ref.literal(nrm, nb, ref.POLES_EPSILON, ref.SEED, T), want, f"literal {nb}")
        same(ref.sorted_form(nrm, nb, ref.POLES_EPSILON, ref.SEED, T), want, f"sorted {nb}")
    assert [ref.POLES_BUCKETS[i] for i in POLES_PICKS] == POLES_PICK_BUCKETS


def test_grid_sizes():
    assert ref.grid(0.09) == (70, 35)
    assert ref.grid(np.pi) == (2, 1)
    assert ref.grid(0.0175) == (360, 180)                          # 64 800 buckets: past the LDS histogram
    for eps in (0.0, -1.0, 4.0, 0.001, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ref.grid(eps)


def test_the_cases_reach_what_they_are_for():
    by = {ref.case_id(c): c for c in ref.CASES}
    for T in (np.float32, np.float64):
        # one bucket, and ties of r_i among the points taken: the tie rule (ascending index) decides
        w = ref.case_expected(by["one_bucket-k10000-e0.09-st3-d0"], T)
        assert len(np.unique(w["bucket"])) == 1
        r = np.array([ref.mix((ref.SEED * 0x100000001B3 + int(i)) & ref.M64) >> 40 for i in w["kept_idx"]])
        assert len(np.unique(r)) < len(r)
        assert (np.diff(r) >= 0).all() and (np.diff(w["kept_idx"])[np.diff(r) == 0] > 0).all()
        # one point per bucket: every pick empties a bucket
        w = ref.case_expected(by["one_each-k90-e0.5-st3-d3"], T)
        assert len(np.unique(w["bucket"])) == 90
        # the small bucket is emptied mid-draw: all 97 of its points are taken, before the last pick
        w = ref.case_expected(by["two_planes-k300-e0.09-st3-d3"], T)
        ids, counts = np.unique(w["bucket"], return_counts=True)
        assert sorted(counts) == [97, 203]
        small = ids[np.argmin(counts)]
        assert np.nonzero(w["bucket"] == small)[0].max() < 299
        # the fine grid is past what the kernel counts in LDS
        n_phi, n_theta = ref.grid(0.0175)
        assert n_phi * n_theta > 8192
        # a random cloud fills many buckets
        assert len(np.unique(ref.case_expected(by["n20001-k5000-e0.09-st3-d3"], T)["bucket"])) > 1000


def test_draw_follows_the_law_over_seeds():
    """Two buckets of 600 and 40 points, 30 picks, 10 seeds: neither bucket runs out, so each pick is a fair coin between the two.
    Of the 300 picks the small bucket's share is Binomial(300, 1/2): mean 150, sigma 8.7; five sigma is 107 .. 193 -- and far from
    the 19 a draw proportional to the buckets' sizes would give."""
    rng = np.random.default_rng(5)
    th = np.concatenate([np.full(600, 5.5), np.full(40, 17.5)]) + rng.uniform(-0.2, 0.2, 640)
    ph = np.concatenate([np.full(600, 3.5), np.full(40, 0.5)]) + rng.uniform(-0.2, 0.2, 640)
    nrm = ref._direction(th * 0.09, ph * 0.09)
    n_phi, n_theta = ref.grid(0.09)
    small = 17 * n_phi
    took = 0
    for seed in range(1, 11):
        for form in (ref.literal, ref.sorted_form):
            got = form(nrm, 30, 0.09, seed, np.float64)
            assert set(np.unique(got["bucket"])) <= {5 * n_phi + 3, small}
        took += int((got["bucket"] == small).sum())
    assert 107 <= took <= 193, took


def test_reference_refuses_what_the_statement_refuses():
    nrm = np.zeros((3, 3), dtype=np.float32)
    for f in (ref.literal, ref.sorted_form):
        for nb, eps, seed in ((0, 0.09, 1), (1, 0.0, 1), (1, 4.0, 1), (1, 0.001, 1), (1, float("inf"), 1), (1, 0.09, 1 << 53)):
            with pytest.raises(ValueError):
                f(nrm, nb, eps, seed, np.float32)
        bad = nrm.copy()
        bad[1, 2] = np.nan
        with pytest.raises(ValueError):
            f(bad, 1, 0.09, 1, np.float32)
        assert len(f(bad, 3, 0.09, 1, np.float32)["kept_idx"]) == 3      # the no-op does not read the normals


def test_the_fixture_is_what_the_reference_gives():
    assert open(ref.GOLDEN, "rb").read() == ref.golden_bytes()
