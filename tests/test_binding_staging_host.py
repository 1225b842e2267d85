"""What the filter bindings of pgslam_amd/icp.py share (_Staged): the views, checks and output buffers every one of them takes
before its C call.  numpy inputs only: no Context, no library, no device."""
import numpy as np
import pytest

from pgslam_amd import icp
from pgslam_amd.icp import _Staged


def test_an_empty_cloud_keeps_a_row_stride():
    for dtype in (np.float32, np.float64):
        s = _Staged(np.zeros((0, 3), dtype=dtype), normals=np.zeros((0, 3), dtype=dtype))
        assert s.n == 0 and s.x.n == 0 and s.x.stride != 0 and s.dtype == dtype and s.mem == icp.HOST
        assert s.nb.n == 0 and s.nb.stride != 0 and s.nb.dtype == dtype
        assert s.d is None and s.drows == 0


def test_view_of_a_homogeneous_cloud_cast_to_the_asked_dtype():
    s = _Staged(np.arange(20, dtype=np.float64).reshape(5, 4), dtype=np.float32)
    assert (s.n, s.x.stride, s.dtype, s.mem) == (5, 4, np.float32, icp.HOST)
    assert s.x.keep.dtype == np.float32 and s.x.ptr == s.x.keep.ctypes.data


def test_descriptors_come_contiguous_in_the_clouds_dtype():
    xyz = np.zeros((5, 3), dtype=np.float32)
    desc = np.arange(20, dtype=np.float64).reshape(5, 4)[:, ::2]        # (5, 2), neither contiguous nor float32
    s = _Staged(xyz, descriptors=desc)
    assert s.drows == 2 and s.d.shape == (5, 2) and s.d.flags["C_CONTIGUOUS"] and s.d.dtype == np.float32
    assert np.array_equal(s.d, desc.astype(np.float32))
    assert s.ptr(s.d).value == s.d.ctypes.data


def test_mismatched_rows_are_refused():
    xyz = np.zeros((5, 3), dtype=np.float32)
    with pytest.raises(AssertionError):
        _Staged(xyz, descriptors=np.zeros((4, 2), dtype=np.float32))
    with pytest.raises(AssertionError):
        _Staged(xyz, normals=np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(AssertionError):
        _Staged(np.zeros((0, 3), dtype=np.float32), normals=np.zeros((4, 3), dtype=np.float32))


def test_outputs_and_their_addresses():
    s = _Staged(np.zeros((5, 4), dtype=np.float64))
    out, idx = s.mk((1, 3)), s.mk((7,), np.int32)
    assert isinstance(out, np.ndarray) and out.shape == (1, 3) and out.dtype == np.float64
    assert idx.shape == (7,) and idx.dtype == np.int32
    assert s.ptr(None) is None and s.ptr(out).value == out.ctypes.data
    assert np.array_equal(s.rows(np.arange(10).reshape(5, 2), np.array([3, 0], dtype=np.int32)), [[6, 7], [0, 1]])


def test_the_entry_point_follows_the_clouds_precision():
    class Lib:
        pgicp_voxel_grid_f32, pgicp_voxel_grid_f64 = "f32", "f64"
    assert _Staged(np.zeros((2, 3), dtype=np.float32)).fn(Lib, "voxel_grid") == "f32"
    assert _Staged(np.zeros((2, 3), dtype=np.float64)).fn(Lib, "voxel_grid") == "f64"
    assert _Staged(np.zeros((2, 3), dtype=np.float64), dtype=np.float32).fn(Lib, "voxel_grid") == "f32"
