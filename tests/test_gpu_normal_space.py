"""NormalSpaceDataPointsFilter on the device (pgicp_normal_space_sampling_*, k_normalspace.inc) through the C ABI from Python,
against the plain statement of tests/normal_space_ref.py: kept indices, buckets, coordinates, normals and descriptor rows bit for
bit, in both precisions, host memory and device memory alike.  The cases are the reference module's: n = 0, 1, 2, the sort's tile
and round boundaries, nbSample 1, n - 1, n, n + 1 and about n / 4, the gather's block edge (256 and 257 picks of 300), epsilon 0.09, 0.5, pi (two buckets) and 0.0175 (64 800 buckets:
the histogram on the global array), strides 3 and 4, descriptor rows 0, 3 and 7, one bucket with ties of r_i, one point per
bucket, a small bucket that empties mid-draw, and the hand-written pole and seam cloud.  No input lies in the statement's band of
freedom (the reference module asserts it), so nothing here has a tolerance."""
import numpy as np
import pytest

import normal_space_ref as ref
from pgslam_amd import icp

KEYS = (("kept_idx", "kept_idx"), ("bucket", "bucket"), ("xyz", "xyz"), ("normals", "normals"), ("descriptors", "desc"))


def strided(x, stride):
    if stride == 3:
        return x
    out = np.ones((len(x), stride), dtype=x.dtype)
    out[:, :3] = x
    return out


def compare(got, want, label):
    assert len(got["kept_idx"]) == len(want["kept_idx"]), (label, "n_out", len(got["kept_idx"]), len(want["kept_idx"]))
    for gk, wk in KEYS:
        g, w = got[gk], want[wk]
        if w is None:
            assert g is None, (label, gk)
            continue
        g = np.ascontiguousarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (label, gk, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{label}: {gk} differs at {len(bad)} picks, first {bad[:5]}: {g[bad[:5]]} against {w[bad[:5]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_against_the_reference_host_and_device_memory(ctx, case, T):
    import torch
    _, nb, eps, stride, _ = case
    x, nrm, d = ref.case_inputs(case, T)
    want = ref.case_expected(case, T)
    xs, ns = strided(x, stride), strided(nrm, stride)
    kw = dict(nb_sample=nb, epsilon=eps, seed=ref.SEED)
    host = ctx.normal_space_sampling(xs, ns, descriptors=d, dtype=T, **kw)
    compare(host, want, ref.case_id(case) + " host memory")
    if len(x) == 0:
        return
    dev = torch.device("cuda", 0)
    tx, tn = torch.from_numpy(np.array(xs)).to(dev), torch.from_numpy(np.array(ns)).to(dev)
    td = torch.from_numpy(np.array(d)).to(dev) if d is not None else None
    got = ctx.normal_space_sampling(tx, tn, descriptors=td, **kw)
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}
    compare(got, want, ref.case_id(case) + " device memory")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_refusals_leave_the_context_usable(ctx, T):
    case = next(c for c in ref.CASES if ref.case_id(c) == "n256-k64-e0.09-st4-d7")
    x, nrm, d = ref.case_inputs(case, T)
    bad = np.array(nrm)
    bad[100, 1] = np.nan
    ok = dict(xyz=x, normals=nrm, nb_sample=64)
    for args in (dict(ok, normals=bad), dict(ok, nb_sample=0), dict(ok, epsilon=0.0), dict(ok, epsilon=4.0), dict(ok, epsilon=0.001),
                 dict(ok, epsilon=float("inf")), dict(ok, seed=1 << 53)):
        with pytest.raises(icp.PgicpError) as e:
            ctx.normal_space_sampling(dtype=T, **args)
        assert e.value.code == icp.ERR_ARG, args
        got = ctx.normal_space_sampling(x, nrm, 64, epsilon=0.09, seed=ref.SEED, descriptors=d, dtype=T)     # the next call succeeds
        compare(got, ref.case_expected(case, T), "after a refusal")
    whole = ctx.normal_space_sampling(x, bad, len(x), dtype=T)       # the no-op does not read the normals
    assert (whole["kept_idx"] == np.arange(len(x))).all() and (whole["bucket"] == -1).all()


@pytest.mark.gpu
def test_same_seed_agrees_and_two_seeds_differ(ctx):
    case = next(c for c in ref.CASES if ref.case_id(c) == "n4097-k1024-e0.09-st3-d0")
    x, nrm, _ = ref.case_inputs(case, np.float32)
    a = ctx.normal_space_sampling(x, nrm, 1024, seed=7)
    b = ctx.normal_space_sampling(x, nrm, 1024, seed=7)
    c = ctx.normal_space_sampling(x, nrm, 1024, seed=8)
    assert a["kept_idx"].tobytes() == b["kept_idx"].tobytes() and a["bucket"].tobytes() == b["bucket"].tobytes()
    assert a["kept_idx"].tobytes() != c["kept_idx"].tobytes()
    assert len(np.unique(c["kept_idx"])) == 1024
