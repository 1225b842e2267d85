"""OctreeGridDataPointsFilter on the device (pgicp_octree_grid_*, k_octree.inc) through the C ABI from Python, against the numpy
statement of tests/octree_grid_ref.py: kept indices, counts, depths, coordinates, descriptor rows and the number of leaves bit for
bit, in both precisions, host memory and device memory alike.  The cases are the reference module's: n = 0, 1, 2, the sort's tile
and round boundaries, the depth cap, a deep pair, a lattice whose node centres land on points, maxPointByNode 1, 3, 64 and more,
maxSizeByNode 0, one that stops some branches early and one that makes the root a leaf, the four methods, strides 3 and 4,
descriptor rows 0, 3 and 7, and leaves past the block path's 512-point chunk."""
import numpy as np
import pytest

import octree_grid_ref as ref
from pgslam_amd import icp

KEYS = (("kept_idx", "kept_idx"), ("count", "count"), ("depth", "depth"), ("xyz", "xyz"), ("descriptors", "desc"))


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
            raise AssertionError(f"{label}: {gk} differs at {len(bad)} leaves, first {bad[:5]}: {g[bad[:5]]} against {w[bad[:5]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_against_the_reference_host_and_device_memory(ctx, case, T):
    import torch
    _, mp, ms, method, stride, _ = case
    x, d = ref.case_inputs(case, T)
    want = ref.case_expected(case, T)
    xs = strided(x, stride)
    kw = dict(max_point_by_node=mp, max_size_by_node=ms, sampling_method=method, seed=ref.SEED)
    host = ctx.octree_grid(xs, descriptors=d, dtype=T, **kw)
    compare(host, want, ref.case_id(case) + " host memory")
    if len(x) == 0:
        return
    dev = torch.device("cuda", 0)
    tx = torch.from_numpy(np.array(xs)).to(dev)
    td = torch.from_numpy(np.array(d)).to(dev) if d is not None else None
    got = ctx.octree_grid(tx, descriptors=td, **kw)
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in got.items()}
    compare(got, want, ref.case_id(case) + " device memory")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_refusals_leave_the_context_usable(ctx, T):
    case = next(c for c in ref.CASES if ref.case_id(c) == "n257-p3-s0-m2-st3-d7")
    x, d = ref.case_inputs(case, T)
    bad = np.array(x)
    bad[100, 1] = np.nan
    for args in (dict(xyz=bad), dict(xyz=x, max_point_by_node=0), dict(xyz=x, max_size_by_node=-1.0), dict(xyz=x, max_size_by_node=float("inf")),
                 dict(xyz=x, sampling_method=4), dict(xyz=x, sampling_method=-1), dict(xyz=x, seed=1 << 53)):
        with pytest.raises(icp.PgicpError) as e:
            ctx.octree_grid(dtype=T, **args)
        assert e.value.code == icp.ERR_ARG, args
        got = ctx.octree_grid(x, descriptors=d, max_point_by_node=3, sampling_method=2, seed=ref.SEED, dtype=T)     # the next call succeeds
        compare(got, ref.case_expected(case, T), "after a refusal")
