"""Python binding of the C ABI in include/pgicp.h (ctypes, no torch types cross it).

This is plumbing for tests and bench.py; the C++ drop-in host layer lives in
include/pgslam_amd/.  The names mirror the libpointmatcher objects pgslam drives
(reference src/pgslam/Localizer.hpp:126,148,309-347, LoopCloser.hpp:98,343-365):

    ICPSequence.setMap(cloud)            -> Context.set_map(xyz, normals)
    ICPSequence.__call__(reading, T)     -> Context.align(map, reading, T_init)
    ICP.__call__(reading, reference, T)  -> Context.icp_pair(...)
    matcher.findClosests                 -> Context.match(...)
    outlierFilters.compute               -> Context.outlier_weights(...)
    ErrorElements / getResidualError     -> Context.error_stats(...)

There is no CPU fallback: if libpgicp.so is missing, or no GPU is present,
construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PGICP_LIB_OVERRIDE") or os.path.join(_HERE, "lib", "libpgicp.so")

OK, ERR_NO_MATCH, ERR_NAN, ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_NOT_RIGID, ERR_BOUND = range(8)
MINIMIZER_POINT_TO_PLANE, MINIMIZER_POINT_TO_POINT, MINIMIZER_POINT_TO_PLANE_4DOF, MINIMIZER_POINT_TO_POINT_WITH_COV = 0, 1, 2, 3
HOST, DEVICE, HOST_PINNED = 0, 1, 2
MATCHER_GRID, MATCHER_BRUTE = 0, 1
PROF_NAMES = ["knn_grid", "knn_brute", "trim_select", "p2plane_reduce", "solve_update", "pretransform",
              "covariance", "grid_build", "knn_slow", "surface_normals", "knn_grid_unseeded"]

# every symbol include/pgicp.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "pgicp_abi_version", "pgicp_device_count", "pgicp_ctx_create", "pgicp_ctx_destroy", "pgicp_last_error",
    "pgicp_ctx_stream", "pgicp_ctx_synchronize", "pgicp_default_params", "pgicp_set_params", "pgicp_get_params",
    "pgicp_map_create_f32", "pgicp_map_create_f64", "pgicp_map_create_batch_f32", "pgicp_map_create_batch_f64",
    "pgicp_map_destroy", "pgicp_map_size", "pgicp_map_transfer",
    "pgicp_align_f32", "pgicp_align_f64", "pgicp_align_batch_f32", "pgicp_align_batch_f64",
    "pgicp_align_residual_batch_f32", "pgicp_align_residual_batch_f64", "pgicp_filter_cloud_f32", "pgicp_filter_cloud_f64",
    "pgicp_device_alloc", "pgicp_device_free", "pgicp_device_copy",
    "pgicp_icp_pair_f32", "pgicp_icp_pair_f64", "pgicp_match_f32", "pgicp_match_f64",
    "pgicp_outlier_weights_f32", "pgicp_outlier_weights_f64", "pgicp_error_stats_f32", "pgicp_error_stats_f64",
    "pgicp_partial_chain_f32", "pgicp_partial_chain_f64", "pgicp_partial_chain_batch_f32",
    "pgicp_partial_chain_batch_f64", "pgicp_transform_f32", "pgicp_transform_f64",
    "pgicp_build_local_map_f32", "pgicp_build_local_map_f64", "pgicp_surface_normals_f32", "pgicp_surface_normals_f64", "pgicp_shard_pairs", "pgicp_check_icp_result",
    "pgicp_profile_enable", "pgicp_profile_reset", "pgicp_profile_get", "pgicp_debug_counters", "pgicp_debug_alloc_stats", "pgicp_ctx_create_priority", "pgicp_filter_cloud_dev_f32", "pgicp_filter_cloud_dev_f64",
    "pgicp_debug_last_matches_f32", "pgicp_debug_last_matches_f64",
    "pgicp_status_string", "pgicp_upload_f32", "pgicp_upload_f64", "pgicp_host_alloc", "pgicp_host_free",
    "pgicp_ctx_device", "pgicp_comm_unique_id", "pgicp_comm_create", "pgicp_comm_destroy", "pgicp_comm_info",
    "pgicp_comm_last_error", "pgicp_shard_slots", "pgicp_allgather_edges", "pgicp_comm_create_host", "pgicp_profile_process",
    "pgicp_debug_reading_order", "pgicp_partial_chain_seeded_f32", "pgicp_partial_chain_seeded_f64",
    "pgicp_sampling_surface_normal_f32", "pgicp_sampling_surface_normal_f64",
    "pgicp_set_var_trim", "pgicp_get_var_trim", "pgicp_last_var_trim_ratio",
    "pgicp_set_descriptor_filter", "pgicp_get_descriptor_filter", "pgicp_map_set_values_f32", "pgicp_map_set_values_f64",
    "pgicp_voxel_grid_f32", "pgicp_voxel_grid_f64",
]
SUM_ORDER_SORTED, SUM_ORDER_SCAN = 0, 1
# every symbol the companion header include/pgicp_vardist.h declares (checked by tests/test_var_dist_host.py)
VARDIST_SYMBOLS = ("pgicp_arm_reading_radii_f32", "pgicp_arm_reading_radii_f64")
# every symbol the companion header include/pgicp_robust.h declares (checked by tests/test_robust_ext_host.py)
ROBUST_SYMBOLS = ("pgicp_set_robust_ext", "pgicp_get_robust_ext")
ROBUST_DIST = dict(point2point=0, point2plane=1)
ROBUST_SCALE = dict(none=0, mad=1, berg=2)
# every symbol the companion header include/pgicp_noise.h declares (checked by tests/test_noise_overlap_host.py)
NOISE_SYMBOLS = (
    "pgicp_simple_sensor_noise_f32", "pgicp_simple_sensor_noise_f64",
    "pgicp_arm_reading_noise_f32", "pgicp_arm_reading_noise_f64", "pgicp_last_noise_overlap",
)
# every symbol the companion header include/pgicp_density.h declares (checked by tests/test_density_host.py)
DENSITY_SYMBOLS = (
    "pgicp_surface_densities_f32", "pgicp_surface_densities_f64", "pgicp_max_density_f32", "pgicp_max_density_f64",
    "pgicp_normals_max_density_f32", "pgicp_normals_max_density_f64",
)
# every symbol the companion header include/pgicp_covsample.h declares (checked by tests/test_covariance_sampling_host.py)
COVSAMPLE_SYMBOLS = (
    "pgicp_covariance_sampling_f32", "pgicp_covariance_sampling_f64",
    "pgicp_covariance_sampling_framed_f32", "pgicp_covariance_sampling_framed_f64",
)
# every symbol the companion header include/pgicp_octree.h declares (checked by tests/test_octree_grid_host.py)
OCTREE_SYMBOLS = ("pgicp_octree_grid_f32", "pgicp_octree_grid_f64")
# every symbol the companion header include/pgicp_normalspace.h declares (checked by tests/test_cpp_normal_space.py)
NORMALSPACE_SYMBOLS = ("pgicp_normal_space_sampling_f32", "pgicp_normal_space_sampling_f64")
# every symbol the companion header include/pgicp_normals_ext.h declares (checked by tests/test_cpp_surface_normals_ext.py)
NORMALS_EXT_SYMBOLS = (
    "pgicp_surface_normals_ext_f32", "pgicp_surface_normals_ext_f64", "pgicp_smooth_normals_f32", "pgicp_smooth_normals_f64",
)
# every symbol the companion header include/pgicp_quantile.h declares (checked by tests/test_axis_quantile_host.py)
QUANTILE_SYMBOLS = ("pgicp_axis_quantile_f32", "pgicp_axis_quantile_f64")
# every symbol the companion header include/pgicp_ssn_ext.h declares (checked by tests/test_sampling_normals_ext_host.py)
SSN_EXT_SYMBOLS = ("pgicp_sampling_surface_normal_ext_f32", "pgicp_sampling_surface_normal_ext_f64")
# every symbol the companion header include/pgicp_elipsoids.h declares (checked by tests/test_elipsoids_host.py)
ELIPSOIDS_SYMBOLS = ("pgicp_elipsoids_f32", "pgicp_elipsoids_f64")
# every symbol the companion header include/pgicp_sensor_chain.h declares (checked by tests/test_sensor_chain_host.py)
SENSOR_CHAIN_SYMBOLS = ("pgicp_sensor_chain_f32", "pgicp_sensor_chain_f64")
CHAIN_OBSERVATION_DIRECTION, CHAIN_ORIENT_NORMALS, CHAIN_SHADOW, CHAIN_MAX_DENSITY, CHAIN_SIMPLE_SENSOR_NOISE = range(1, 6)
CHAIN_MAX_STAGES = 8
# every symbol the companion header include/pgicp_descriptor_filters.h declares (checked by tests/test_descriptor_filters_host.py)
DESCRIPTOR_FILTERS_SYMBOLS = ("pgicp_sensor_chain_ext_f32", "pgicp_sensor_chain_ext_f64")
CHAIN_INCIDENCE_ANGLE, CHAIN_SPHERICALITY, CHAIN_CUT_AT_DESCRIPTOR = 6, 7, 8
CHAIN_EXT_MAX_STAGES, CHAIN_EXT_MAX_CUTS = 12, 4
# the row a cut_at_descriptor stage reads (PGICP_CHAIN_ROW_*); an integer names a row of `desc`
CHAIN_ROWS = dict(desc=0, densities=1, incidence_angles=2, sphericality=3, unstructureness=4, structureness=5, simple_sensor_noise=6)
SENSOR_SICK_LMS, SENSOR_HOKUYO_URG, SENSOR_HOKUYO_UTM, SENSOR_KINECT, SENSOR_SICK_TIM = range(5)


class Params(C.Structure):
    _fields_ = [("knn", C.c_int), ("epsilon", C.c_double), ("max_dist", C.c_double), ("trim_ratio", C.c_double),
                ("max_iters", C.c_int), ("min_diff_rot", C.c_double), ("min_diff_trans", C.c_double),
                ("smooth_length", C.c_int), ("sensor_std_dev", C.c_double), ("matcher", C.c_int),
                ("grid_cell", C.c_double), ("check_every", C.c_int), ("outlier_max_dist", C.c_double),
                ("quantile_scale", C.c_double), ("error_minimizer", C.c_int), ("bound_max_rot", C.c_double),
                ("bound_max_trans", C.c_double), ("normal_max_angle", C.c_double), ("robust_fct", C.c_int), ("robust_tuning", C.c_double),
                ("robust_scale", C.c_int), ("robust_approx", C.c_double), ("sum_order", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("converged", C.c_int), ("max_iter_reached", C.c_int),
                ("overlap", C.c_double), ("residual", C.c_double), ("trim_limit", C.c_double), ("n_kept", C.c_int),
                ("n_finite", C.c_int), ("cov", C.c_double * 36)]

    def as_dict(self):
        return dict(status=self.status, iterations=self.iterations, converged=bool(self.converged),
                    max_iter_reached=bool(self.max_iter_reached), overlap=self.overlap, residual=self.residual,
                    trim_limit=self.trim_limit, n_kept=self.n_kept, n_finite=self.n_finite,
                    cov=np.array(self.cov[:]).reshape(6, 6))


class RobustExt(C.Structure):
    """pgicp_robust_ext (include/pgicp_robust.h)"""
    _fields_ = [("distance_type", C.c_int), ("scale_estimator", C.c_int), ("nb_iteration_for_scale", C.c_int)]


class Problem(C.Structure):
    _fields_ = [("map_id", C.c_int), ("reading", C.c_void_p), ("stride", C.c_int), ("n", C.c_int), ("mem", C.c_int),
                ("T_init", C.c_double * 16), ("normals", C.c_void_p), ("nstride", C.c_int)]


class Filter(C.Structure):
    _fields_ = [("type", C.c_int), ("p", C.c_double * 8)]


class ChainStage(C.Structure):
    """pgicp_chain_stage (include/pgicp_sensor_chain.h)"""
    _fields_ = [("type", C.c_int), ("p", C.c_double * 4)]


class ChainOut(C.Structure):
    """pgicp_chain_out (include/pgicp_descriptor_filters.h)"""
    _fields_ = [("xyz", C.c_void_p), ("nrm", C.c_void_p), ("nstride", C.c_int), ("eig", C.c_void_p), ("dens", C.c_void_p), ("obs", C.c_void_p),
                ("noise", C.c_void_p), ("desc", C.c_void_p), ("incidence", C.c_void_p), ("sphericality", C.c_void_p),
                ("unstructureness", C.c_void_p), ("structureness", C.c_void_p), ("kept_idx", C.c_void_p)]


FILTER_IDENTITY, FILTER_MAX_DIST, FILTER_MIN_DIST, FILTER_BOUNDING_BOX, FILTER_REMOVE_NAN, FILTER_FIX_STEP, FILTER_RANDOM_SAMPLING, \
    FILTER_MAX_POINT_COUNT = range(8)
FILTER_MAX_QUANTILE_ON_AXIS = 8         # (include/pgicp_quantile.h) p[0] = dim, p[1] = ratio
FILTER_CUT_AT_DESCRIPTOR = 9            # (include/pgicp_descriptor_filters.h) p[0] = descriptor row, p[1] = useLargerThan, p[2] = threshold


class CovFrame(C.Structure):
    """pgicp_cov_frame (include/pgicp_covsample.h); basis is column-major"""
    _fields_ = [("center", C.c_double * 3), ("L", C.c_double), ("eigenvalues", C.c_double * 6), ("basis", C.c_double * 36)]

    def as_dict(self):
        return dict(center=np.array(self.center[:]), L=float(self.L), eigenvalues=np.array(self.eigenvalues[:]),
                    basis=np.array(self.basis[:]).reshape(6, 6).T.copy())

    @classmethod
    def from_dict(cls, d):
        f = cls()
        f.center[:] = [float(x) for x in d["center"]]
        f.L = float(d["L"])
        f.eigenvalues[:] = [float(x) for x in d.get("eigenvalues", np.zeros(6))]
        f.basis[:] = [float(x) for x in np.asarray(d["basis"], dtype=np.float64).reshape(6, 6).T.ravel()]
        return f


class Edge(C.Structure):
    _fields_ = [("from_id", C.c_int64), ("to_id", C.c_int64), ("accepted", C.c_int32), ("status", C.c_int32),
                ("iterations", C.c_int32), ("max_iter_reached", C.c_int32), ("overlap", C.c_double),
                ("residual", C.c_double), ("T_from_to", C.c_double * 16), ("cov", C.c_double * 36),
                ("reserved", C.c_double * 6)]


assert C.sizeof(Edge) == 512


class PgicpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pgicp error {code}: {msg}")
        self.code = code


class ConvergenceError(PgicpError):
    """PM::ConvergenceError: 'no point to minimize' / NaN in the checkers / BoundTransformationChecker's limit exceeded."""


_lib = None


def load_library() -> C.CDLL:
    """dlopen libpgicp.so.  Raises (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `make` (or __graft_entry__.build()); "
                              "pgslam_amd has no CPU fallback")
        # PyTorch wheels carry their own libamdhip64.  If libpgicp (linked against /opt/rocm's copy) enters the process
        # first and torch later, the process holds two HIP runtimes and torch reports "No HIP GPUs are available"; with
        # torch loaded first the loader resolves libpgicp's dependency to the copy that is already there.
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                import torch  # noqa: F401
        except Exception:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.pgicp_last_error.restype = C.c_char_p
        _lib.pgicp_status_string.restype = C.c_char_p
        _lib.pgicp_comm_last_error.restype = C.c_char_p
        _lib.pgicp_ctx_stream.restype = C.c_void_p
    return _lib


_TORCH_DTYPES = {}          # torch dtype -> numpy dtype (the string round trip costs microseconds per reading of a batch)

# numpy views of the two ctypes records a batch call exchanges (same layout: ctypes' natural alignment)
_PROBLEM_DTYPE = np.dtype({"names": ["map_id", "reading", "stride", "n", "mem", "T_init", "normals", "nstride"],
                           "formats": ["<i4", "<u8", "<i4", "<i4", "<i4", ("<f8", (16,)), "<u8", "<i4"],
                           "offsets": [0, 8, 16, 20, 24, 32, 160, 168], "itemsize": 176})
assert C.sizeof(Problem) == _PROBLEM_DTYPE.itemsize
_STATS_DTYPE = np.dtype({"names": ["status", "iterations", "converged", "max_iter_reached", "overlap", "residual", "trim_limit",
                                   "n_kept", "n_finite", "cov"],
                         "formats": ["<i4", "<i4", "<i4", "<i4", "<f8", "<f8", "<f8", "<i4", "<i4", ("<f8", (36,))],
                         "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 44, 48], "itemsize": 336})


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class DevPtr:
    """A reading already on the device, as pgicp_upload_* hands it out: raw address, stride, point count."""

    def __init__(self, ptr, stride, n, dtype, keep=None):
        self.ptr, self.stride, self.n, self.dtype, self.keep = ptr, stride, n, np.dtype(dtype), keep


class _Buf:
    """(pointer, stride, n, mem, dtype) view of a numpy array or a torch CUDA tensor.
    Accepts (N,3) packed xyz or (N,4) homogeneous rows (= libpointmatcher's 4xN
    column-major `features`)."""

    def __init__(self, x, dtype=None):
        if isinstance(x, DevPtr):
            self.keep, self.ptr, self.stride, self.n, self.mem, self.dtype = x, x.ptr, x.stride, x.n, DEVICE, x.dtype
            return
        if _is_torch(x):
            if not x.is_cuda:
                x = x.numpy()
            else:
                assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= 3
                self.keep = x
                self.ptr = x.data_ptr()
                self.stride = x.stride(0)
                self.n = x.shape[0]
                self.mem = DEVICE
                dt = _TORCH_DTYPES.get(x.dtype)
                if dt is None:
                    dt = _TORCH_DTYPES[x.dtype] = np.dtype(str(x.dtype).replace("torch.", ""))
                self.dtype = dt
                return
        x = np.asarray(x)
        if dtype is not None:
            x = x.astype(dtype, copy=False)
        assert x.ndim == 2 and x.shape[1] >= 3 and x.strides[1] == x.itemsize
        self.keep = x
        self.ptr = x.ctypes.data
        self.stride = x.strides[0] // x.itemsize
        self.n = x.shape[0]
        self.mem = HOST
        self.dtype = x.dtype


def _bufs(xs, dtype=None):
    """_Buf views of a list of clouds; the same object listed twice (a keyframe that is the reference of several loop-closure
    candidates) is looked at once -- 1.2 us per torch tensor, three lists of 512 in a loop-closure step."""
    seen = {}
    out = []
    for x in xs:
        b = seen.get(id(x))
        if b is None:
            b = seen[id(x)] = _Buf(x, dtype)
        out.append(b)
    return out


def _unempty(a, dtype):
    """numpy gives an empty array zero strides; the C ABI wants the row stride of a real cloud"""
    if not _is_torch(a) and np.shape(a)[0] == 0:
        return np.zeros((1, 3), dtype=dtype or np.asarray(a).dtype)[:0]
    return a


def _host_ptr(t):
    return None if t is None else C.c_void_p(t.ctypes.data)


def _device_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Staged:
    """The inputs of one filter binding, staged for its C call: `x` (and `nb`) the _Buf views of the cloud (and its normals),
    `d` / `drows` the descriptors made contiguous in the cloud's memory and dtype, `mk(shape, dtype=None)` an uninitialised
    output in that memory (`dtype` a numpy dtype; None: the cloud's), `ptr(t)` its address (None for None), `rows(a, idx)` the
    rows of an input that an int32 output names, `fn(lib, name)` the entry point of the cloud's precision.  Needs no Context
    and, for numpy inputs, no library."""
    __slots__ = ("x", "nb", "n", "mem", "dtype", "d", "drows", "mk", "ptr")

    def __init__(self, xyz, normals=None, descriptors=None, dtype=None):
        x = self.x = _Buf(_unempty(xyz, dtype), dtype)
        n, dt = self.n, self.dtype = x.n, x.dtype
        self.mem = x.mem
        if x.mem == DEVICE:
            import torch
            like = x.keep
            self.mk = lambda shape, dtype=None: torch.empty(shape, dtype=like.dtype if dtype is None else getattr(torch, np.dtype(dtype).name),
                                                            device=like.device)
            self.ptr = _device_ptr
        else:
            self.mk = lambda shape, dtype=None: np.empty(shape, dtype=dtype or dt)
            self.ptr = _host_ptr
        self.nb = None
        if normals is not None:
            nb = self.nb = _Buf(_unempty(normals, dt), dt if x.mem == HOST else None)
            assert nb.n == n and nb.mem == x.mem and nb.dtype == dt
        self.d, self.drows = None, 0
        if descriptors is not None:
            if x.mem == DEVICE:
                d = descriptors.contiguous()
                assert d.is_cuda and d.dtype == x.keep.dtype and d.shape[0] == n
            else:
                d = np.ascontiguousarray(descriptors, dtype=dt)
                assert d.ndim == 2 and d.shape[0] == n
            self.d, self.drows = d, int(d.shape[1])

    def rows(self, a, idx):
        return a[idx if self.mem == HOST else idx.long()]

    def fn(self, lib, name):
        return getattr(lib, "pgicp_" + name + ("_f32" if self.dtype == np.float32 else "_f64"))


def _T16(T):
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4))
    return (C.c_double * 16)(*T.ravel())


UNIQUE_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """pgicp_comm_unique_id (rank 0); pass the bytes to the other ranks by any channel."""
    lib = load_library()
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    st = lib.pgicp_comm_unique_id(buf)
    if st != OK:
        raise PgicpError(st, lib.pgicp_comm_last_error().decode())
    return buf.raw


def shard_slots(costs, world_size: int) -> int:
    """Largest shard of the deterministic split: the block size of the edge all-gather, known to every rank."""
    lib = load_library()
    n = len(costs)
    arr = (C.c_int64 * max(n, 1))(*[int(c) for c in costs])
    out = C.c_int()
    st = lib.pgicp_shard_slots(C.c_int(n), arr, C.c_int(world_size), C.byref(out))
    if st != OK:
        raise PgicpError(st, "pgicp_shard_slots failed")
    return out.value


class Comm:
    """RCCL communicator of one rank (pgicp_comm_create) on a context's device."""

    def __init__(self, ctx: "Context", world_size: int, rank: int, unique_id: bytes):
        self.lib = ctx.lib
        self.ctx = ctx
        self.world_size, self.rank = world_size, rank
        h = C.c_void_p()
        st = self.lib.pgicp_comm_create(ctx.h, C.c_int(world_size), C.c_int(rank), C.create_string_buffer(unique_id, UNIQUE_ID_BYTES), C.byref(h))
        if st != OK:
            raise PgicpError(st, self.lib.pgicp_comm_last_error().decode())
        self.h = h

    @classmethod
    def host(cls, world_size: int, rank: int, shm_path: str, max_slots_per_rank: int) -> "Comm":
        """pgicp_comm_create_host: the same collective with the blocks travelling through a shared-memory file
        (no device; the host 'fake all-gather' of SURVEY.md section 4 T4)."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.ctx = None
        self.world_size, self.rank = world_size, rank
        h = C.c_void_p()
        st = self.lib.pgicp_comm_create_host(C.c_int(world_size), C.c_int(rank), shm_path.encode(), C.c_int(max_slots_per_rank), C.byref(h))
        if st != OK:
            raise PgicpError(st, self.lib.pgicp_comm_last_error().decode())
        self.h = h
        return self

    def info(self):
        """(world_size, rank) as the communicator itself reports them (pgicp_comm_info)."""
        w, r = C.c_int(), C.c_int()
        self.lib.pgicp_comm_info(self.h, C.byref(w), C.byref(r))
        return w.value, r.value

    def allgather_edges(self, local_edges: np.ndarray, pair_index, slots_per_rank: int, n_total: int) -> np.ndarray:
        """pgicp_allgather_edges on numpy records of the 512-byte pgicp_edge layout."""
        assert local_edges.dtype.itemsize == C.sizeof(Edge)
        local = np.ascontiguousarray(local_edges)
        idx = np.ascontiguousarray(np.asarray(pair_index, dtype=np.int32))
        out = np.zeros(n_total, dtype=local_edges.dtype)
        st = self.lib.pgicp_allgather_edges(self.h, C.c_void_p(local.ctypes.data), C.c_void_p(idx.ctypes.data), C.c_int(len(local)),
                                            C.c_int(slots_per_rank), C.c_int(n_total), C.c_void_p(out.ctypes.data))
        if st != OK:
            raise PgicpError(st, self.lib.pgicp_comm_last_error().decode())
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.pgicp_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, device: int = 0, **params):
        self.lib = load_library()
        h = C.c_void_p()
        st = self.lib.pgicp_ctx_create(C.c_int(device), C.byref(h))
        if st != OK:
            raise PgicpError(st, "pgicp_ctx_create failed" + (": PGICP_ERR_NO_DEVICE (no usable gfx950 device for this rank; the product has no CPU path)" if st == ERR_NO_DEVICE else ""))
        self.h = h
        self.device = device
        self.params = Params()
        self.lib.pgicp_default_params(C.byref(self.params))
        if params:
            self.set_params(**params)

    def close(self):
        if getattr(self, "h", None):
            self.lib.pgicp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st == OK:
            return
        msg = self.lib.pgicp_last_error(self.h).decode()
        if st in (ERR_NO_MATCH, ERR_NAN, ERR_BOUND):
            raise ConvergenceError(st, msg)
        raise PgicpError(st, msg)

    # ---- host-input pipeline ------------------------------------------------
    def host_alloc(self, shape, dtype=np.float32):
        """numpy array in pinned host memory (pgicp_host_alloc); release it with host_free(array)."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._check(self.lib.pgicp_host_alloc(self.h, C.c_size_t(nbytes), C.byref(p)))
        buf = (C.c_char * nbytes).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a):
        p = self._pinned.pop(a.ctypes.data)
        self._check(self.lib.pgicp_host_free(self.h, C.c_void_p(p)))

    # ---- device memory the caller owns between calls (keyframe clouds of a local map stay in HBM) ----
    def device_empty(self, n, stride=3, dtype=np.float32):
        """pgicp_device_alloc: room for n points at `stride` elements each; a DevPtr (release it with device_free)."""
        dtype = np.dtype(dtype)
        p = C.c_void_p()
        self._check(self.lib.pgicp_device_alloc(self.h, C.c_size_t(max(1, n * stride) * dtype.itemsize), C.byref(p)))
        return DevPtr(p.value, stride, n, dtype)

    def device_cloud(self, xyz, dtype=None):
        """A host cloud copied to device memory of its own (pgicp_device_alloc + pgicp_device_copy); strides as on the host."""
        b = _Buf(xyz, dtype)
        assert b.mem == HOST
        d = self.device_empty(b.n, b.stride, b.dtype)
        if b.n:
            nbytes = ((b.n - 1) * b.stride + 3) * b.dtype.itemsize
            self._check(self.lib.pgicp_device_copy(self.h, C.c_void_p(d.ptr), C.c_void_p(b.ptr), C.c_size_t(nbytes), C.c_int(0)))
        return d

    def device_download(self, d):
        """numpy (n, 3) copy of a DevPtr cloud"""
        out = np.zeros((d.n, d.stride), dtype=d.dtype)
        if d.n:
            nbytes = ((d.n - 1) * d.stride + 3) * d.dtype.itemsize
            self._check(self.lib.pgicp_device_copy(self.h, C.c_void_p(out.ctypes.data), C.c_void_p(d.ptr), C.c_size_t(nbytes), C.c_int(1)))
        return out[:, :3]

    def device_free(self, d):
        self._check(self.lib.pgicp_device_free(self.h, C.c_void_p(d.ptr)))
        d.ptr = None

    def upload(self, readings, pinned=False, dtype=None):
        """pgicp_upload_*: start the H2D transfer of host readings on the copy stream, return DevPtr handles at once."""
        bufs = [_Buf(r, dtype) for r in readings]
        assert all(b.mem == HOST for b in bufs)
        n = len(bufs)
        ct = C.c_float if bufs[0].dtype == np.float32 else C.c_double
        hosts = (C.c_void_p * n)(*[b.ptr for b in bufs])
        strides = (C.c_int * n)(*[b.stride for b in bufs])
        counts = (C.c_int * n)(*[b.n for b in bufs])
        out = (C.c_void_p * n)()
        fn = getattr(self.lib, "pgicp_upload" + self._sfx(bufs[0].dtype))
        self._check(fn(self.h, C.c_int(n), hosts, strides, counts, C.c_int(HOST_PINNED if pinned else HOST), out))
        del ct
        return [DevPtr(out[k], bufs[k].stride, bufs[k].n, bufs[k].dtype, keep=bufs[k].keep) for k in range(n)]

    def set_params(self, **kw):
        before = Params.from_buffer_copy(self.params)
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise KeyError(k)
            setattr(self.params, k, v)
        try:
            self._check(self.lib.pgicp_set_params(self.h, C.byref(self.params)))
        except PgicpError:
            self.params = before            # a refused setting leaves the context (and this mirror of it) as it was
            raise

    def set_var_trim(self, min_ratio=None, max_ratio=None, lam=None):
        """[EXT] VarTrimmedDistOutlierFilter{minRatio, maxRatio, lambda} in the chain's quantile slot (pgicp_set_var_trim); called
        with no arguments it takes the filter out.  align*, partial_chain* and outlier_weights then apply it."""
        if min_ratio is None and max_ratio is None and lam is None:
            self._check(self.lib.pgicp_set_var_trim(self.h, None))
            return
        p = (C.c_double * 3)(float(min_ratio), float(max_ratio), float(lam))
        self._check(self.lib.pgicp_set_var_trim(self.h, p))

    def get_var_trim(self):
        """(minRatio, maxRatio, lambda), or None when the filter is off."""
        on = C.c_int(0)
        p = (C.c_double * 3)()
        self._check(self.lib.pgicp_get_var_trim(self.h, C.byref(on), p))
        return tuple(p[:]) if on.value else None

    def last_var_trim_ratio(self, problem=0):
        """The tuned ratio of the last iteration of `problem` in the last align / partial-chain / outlier-weights call
        (-1: the problem had no positive finite distance)."""
        r = C.c_double(0)
        self._check(self.lib.pgicp_last_var_trim_ratio(self.h, C.c_int(problem), C.byref(r)))
        return r.value

    def set_robust_ext(self, distance_type="point2point", scale_estimator=None, nb_iteration_for_scale=0):
        """[EXT] RobustOutlierFilter's distanceType ("point2point" / "point2plane"), scaleEstimator ("none" / "mad" / "berg"; None:
        what the parameters' robust_scale says) and nbIterationForScale (pgicp_set_robust_ext, include/pgicp_robust.h).  A setting
        of the context: it stays until set again or cleared.  The names' codes are accepted too."""
        x = RobustExt(ROBUST_DIST.get(distance_type, distance_type), -1 if scale_estimator is None else ROBUST_SCALE.get(scale_estimator, scale_estimator),
                      int(nb_iteration_for_scale))
        self._check(self.lib.pgicp_set_robust_ext(self.h, C.byref(x)))

    def clear_robust_ext(self):
        """takes set_robust_ext's setting out: the context is what it was without it"""
        self._check(self.lib.pgicp_set_robust_ext(self.h, None))

    def get_robust_ext(self):
        """dict(distance_type, scale_estimator, nb_iteration_for_scale) of codes, or None when the setting is off."""
        on = C.c_int(0)
        x = RobustExt()
        self._check(self.lib.pgicp_get_robust_ext(self.h, C.byref(on), C.byref(x)))
        return dict(distance_type=x.distance_type, scale_estimator=x.scale_estimator, nb_iteration_for_scale=x.nb_iteration_for_scale) if on.value else None

    _DESC_MODES = {None: 0, "larger": 1, "smaller": 2, "soft": 3}

    def set_descriptor_filter(self, mode=None, threshold=None):
        """[EXT] GenericDescriptorOutlierFilter (pgicp_set_descriptor_filter): mode None (off), "larger" / "smaller" (hard,
        useLargerThan 1 / 0: weight 1 where the map point's value is strictly above / below `threshold`) or "soft" (weight =
        value / the largest value over the pairs).  The values are the map's (set_map_values)."""
        if mode not in self._DESC_MODES:
            raise ValueError(f"set_descriptor_filter: unknown mode {mode!r}")
        if mode in ("larger", "smaller") and threshold is None:
            raise ValueError("set_descriptor_filter: a hard mode needs a threshold")
        self._check(self.lib.pgicp_set_descriptor_filter(self.h, C.c_int(self._DESC_MODES[mode]),
                                                          C.c_double(0.0 if threshold is None else float(threshold))))

    def get_descriptor_filter(self):
        """(mode, threshold) as set_descriptor_filter takes them; (None, 0.0) when the filter is off."""
        m, t = C.c_int(0), C.c_double(0)
        self._check(self.lib.pgicp_get_descriptor_filter(self.h, C.byref(m), C.byref(t)))
        return {v: k for k, v in self._DESC_MODES.items()}[m.value], t.value

    def set_map_values(self, map_id, values, dtype=None):
        """One value per point of map `map_id`, in the order its cloud was given (pgicp_map_set_values); None drops them.
        values: a 1-D numpy array (any stride -- a row of a descriptor matrix) or a 1-D torch CUDA tensor.  dtype: the map's
        precision (default: the values' own float32 / float64)."""
        if values is None:
            fn = self.lib.pgicp_map_set_values_f64 if map_id & 0x40000000 else self.lib.pgicp_map_set_values_f32
            self._check(fn(self.h, C.c_int(map_id), None, C.c_int(1), C.c_int(HOST)))
            return
        if _is_torch(values) and values.is_cuda:
            if values.dim() != 1 or values.stride(0) < 1:
                raise ValueError("set_map_values: values must be a 1-D tensor with a positive stride")
            dt = np.dtype(str(values.dtype).replace("torch.", ""))
            if dt not in (np.float32, np.float64):
                raise TypeError("set_map_values: a float32 or float64 tensor is needed")
            if dtype is not None and dt != np.dtype(dtype):
                raise TypeError("set_map_values: the tensor's dtype must be the map's")
            keep, ptr, stride, mem = values, values.data_ptr(), values.stride(0), DEVICE
        else:
            v = np.asarray(values.cpu() if _is_torch(values) else values)
            if dtype is not None:
                v = v.astype(dtype, copy=False)
            if v.dtype not in (np.float32, np.float64):
                v = v.astype(np.float32)
            if v.ndim != 1 or v.strides[0] <= 0 or v.strides[0] % v.itemsize != 0:
                raise ValueError("set_map_values: values must be 1-D with a positive stride of whole elements")
            dt = v.dtype
            keep, ptr, stride, mem = v, v.ctypes.data, v.strides[0] // v.itemsize, HOST
        fn = getattr(self.lib, "pgicp_map_set_values" + self._sfx(dt))
        self._check(fn(self.h, C.c_int(map_id), C.c_void_p(ptr), C.c_int(stride), C.c_int(mem)))
        del keep

    @property
    def stream(self):
        return self.lib.pgicp_ctx_stream(self.h)

    def synchronize(self):
        self._check(self.lib.pgicp_ctx_synchronize(self.h))

    @staticmethod
    def _sfx(dtype):
        return "_f32" if np.dtype(dtype) == np.float32 else "_f64"

    # ---- map -------------------------------------------------------------
    def set_map(self, xyz, normals=None, center=True, dtype=None) -> int:
        x = _Buf(xyz, dtype)
        nb = _Buf(normals, x.dtype) if normals is not None else None
        assert nb is None or (nb.n == x.n and nb.mem == x.mem)
        mid = C.c_int(-1)
        fn = getattr(self.lib, "pgicp_map_create" + self._sfx(x.dtype))
        self._check(fn(self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_void_p(nb.ptr if nb else None),
                       C.c_int(nb.stride if nb else 0), C.c_int(x.n), C.c_int(x.mem), C.c_int(int(center)), C.byref(mid)))
        return mid.value

    def set_maps(self, xyzs, normals=None, center=True, dtype=None):
        """Index several reference clouds with one host round trip (pgicp_map_create_batch)."""
        n = len(xyzs)
        xb = _bufs(xyzs, dtype)
        nb = _bufs(normals, xb[0].dtype) if normals is not None else None
        assert all(b.mem == xb[0].mem and b.dtype == xb[0].dtype for b in xb)
        assert nb is None or all(b.n == x.n and b.mem == x.mem for b, x in zip(nb, xb))
        ptrs = (C.c_void_p * n)(*[b.ptr for b in xb])
        strides = (C.c_int * n)(*[b.stride for b in xb])
        sizes = (C.c_int * n)(*[b.n for b in xb])
        nptrs = (C.c_void_p * n)(*[b.ptr for b in nb]) if nb else None
        nstrides = (C.c_int * n)(*[b.stride for b in nb]) if nb else None
        ids = (C.c_int * n)()
        fn = getattr(self.lib, "pgicp_map_create_batch" + self._sfx(xb[0].dtype))
        self._check(fn(self.h, C.c_int(n), ptrs, strides, nptrs, nstrides, sizes, C.c_int(xb[0].mem), C.c_int(int(center)), ids))
        return list(ids)

    def destroy_map(self, map_id):
        self._check(self.lib.pgicp_map_destroy(self.h, C.c_int(map_id)))

    def map_size(self, map_id):
        m = C.c_int(0)
        self._check(self.lib.pgicp_map_size(self.h, C.c_int(map_id), C.byref(m)))
        return m.value

    # ---- sensor noise (include/pgicp_noise.h) ---------------------------------
    def simple_sensor_noise(self, xyz, sensor_type=0, gain=1.0, dtype=None, out=None):
        """SimpleSensorNoiseDataPointsFilter's descriptor on the device (pgicp_simple_sensor_noise_*): one value per point.
        numpy in -> numpy out, torch CUDA in -> torch CUDA out; `out`: a contiguous 1-D array / CUDA tensor of the cloud's dtype
        to fill instead (host and device may be mixed)."""
        if not _is_torch(xyz) and np.shape(xyz)[0] == 0:           # (numpy gives an empty array zero strides)
            xyz = np.zeros((1, 3), dtype=dtype or np.asarray(xyz).dtype)[:0]
        x = _Buf(xyz, dtype)
        if out is None:
            if x.mem == DEVICE and _is_torch(xyz):
                import torch
                out = torch.empty((x.n,), dtype=xyz.dtype, device=xyz.device)
            else:
                out = np.empty(x.n, dtype=x.dtype)
        if _is_torch(out) and out.is_cuda:
            assert out.dim() == 1 and out.is_contiguous() and out.shape[0] == x.n
            assert np.dtype(str(out.dtype).replace("torch.", "")) == x.dtype
            optr, omem = out.data_ptr(), DEVICE
        else:
            assert isinstance(out, np.ndarray) and out.ndim == 1 and out.flags.c_contiguous and out.shape[0] == x.n and out.dtype == x.dtype
            optr, omem = out.ctypes.data, HOST
        fn = getattr(self.lib, "pgicp_simple_sensor_noise" + self._sfx(x.dtype))
        self._check(fn(self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(x.n), C.c_int(x.mem), C.c_int(int(sensor_type)),
                       C.c_double(float(gain)), C.c_void_p(optr), C.c_int(omem)))
        return out

    def arm_reading_noise(self, noises, dtype):
        """pgicp_arm_reading_noise_*: the `simpleSensorNoise` row of every reading of the NEXT align / align_batch /
        align_residual_batch / icp_pair call (one-shot).  noises: one entry per problem -- a 1-D numpy array (any positive
        stride: a row of a descriptor matrix), a 1-D torch CUDA tensor, or None (that problem has no noise); all in host
        memory or all on the device.  dtype: the element type of the ICP call."""
        self._arm_rows("arm_reading_noise", noises, dtype)

    def arm_reading_radii(self, radii, dtype):
        """pgicp_arm_reading_radii_* (include/pgicp_vardist.h): KDTreeVarDistMatcher's search radius of every point of every
        reading of the NEXT align / align_batch / align_residual_batch / icp_pair / match / partial_chain / partial_chain_batch
        call (one-shot).  radii: one entry per problem, shaped as arm_reading_noise's rows (None: that problem has none);
        +inf is a radius.  dtype: the element type of the consuming call."""
        self._arm_rows("arm_reading_radii", radii, dtype)

    def _arm_rows(self, what, noises, dtype):
        dtype = np.dtype(dtype)
        P = len(noises)
        ptrs, strides, counts, keep, mems = [], [], [], [], set()
        for v in noises:
            if v is None:
                ptrs.append(None), strides.append(1), counts.append(0)
                continue
            if _is_torch(v) and v.is_cuda:
                if v.dim() != 1 or v.stride(0) < 1 or np.dtype(str(v.dtype).replace("torch.", "")) != dtype:
                    raise ValueError(what + ": a 1-D tensor of the call's dtype with a positive stride is needed")
                ptrs.append(v.data_ptr()), strides.append(v.stride(0)), counts.append(v.shape[0]), mems.add(DEVICE)
            else:
                v = np.asarray(v.cpu() if _is_torch(v) else v).astype(dtype, copy=False)
                if v.ndim != 1 or v.strides[0] <= 0 or v.strides[0] % v.itemsize != 0:
                    raise ValueError(what + ": values must be 1-D with a positive stride of whole elements")
                ptrs.append(v.ctypes.data), strides.append(v.strides[0] // v.itemsize), counts.append(v.shape[0]), mems.add(HOST)
            keep.append(v)
        if len(mems) > 1:
            raise ValueError(what + ": the rows must all be in host memory or all on the device")
        fn = getattr(self.lib, "pgicp_" + what + self._sfx(dtype))
        self._check(fn(self.h, C.c_int(P), (C.c_void_p * max(P, 1))(*ptrs), (C.c_int * max(P, 1))(*strides),
                       (C.c_int * max(P, 1))(*counts), C.c_int(mems.pop() if mems else HOST)))
        del keep

    def last_noise_overlap(self, problem=0):
        """pgicp_last_noise_overlap: (overlap, n_elements) of `problem` of the last ICP call, which must have been armed."""
        ov, nb = C.c_double(0), C.c_int(0)
        self._check(self.lib.pgicp_last_noise_overlap(self.h, C.c_int(problem), C.byref(ov), C.byref(nb)))
        return ov.value, nb.value

    def _noise_into(self, stats, noises):
        """overlap_noise / n_elements into the stats dicts of an armed call (None for a problem without noise or one that failed)"""
        for p, st in enumerate(stats):
            ov = nb = None
            if noises[p] is not None and st["status"] == OK:
                ov, nb = self.last_noise_overlap(p)
            st["overlap_noise"], st["n_elements"] = ov, nb

    # ---- full ICP -----------------------------------------------------------
    def align(self, map_id, reading, T_init, dtype=None, normals=None, noise=None, radii=None):
        """normals: the reading's `normals` descriptor (a SurfaceNormalOutlierFilter in the chain needs it); noise: its
        `simpleSensorNoise` row -- the stats then carry overlap_noise (getOverlap()'s sensor-noise branch) and n_elements;
        radii: KDTreeVarDistMatcher's search radius of every reading point (arm_reading_radii)"""
        if normals is not None:
            T, st = self.align_batch(map_id, [reading], [T_init], dtype=dtype, normals=[normals], noises=None if noise is None else [noise],
                                     radiis=None if radii is None else [radii])
            return T[0], st[0]
        r = _Buf(reading, dtype)
        T_out = (C.c_double * 16)()
        st = Stats()
        fn = getattr(self.lib, "pgicp_align" + self._sfx(r.dtype))
        if noise is not None:
            self.arm_reading_noise([noise], r.dtype)
        if radii is not None:
            self.arm_reading_radii([radii], r.dtype)
        self._check(fn(self.h, C.c_int(map_id), C.c_void_p(r.ptr), C.c_int(r.stride), C.c_int(r.n), C.c_int(r.mem),
                       _T16(T_init), T_out, C.byref(st)))
        sd = st.as_dict()
        if noise is not None:
            self._noise_into([sd], [noise])
        return np.array(T_out[:]).reshape(4, 4), sd

    def align_residual_batch(self, map_ids, readings, T_inits, dtype=None, normals=None, raw_stats=False, noises=None, radiis=None):
        """pgicp_align_residual_batch: the ICPs of a batch of loop-closure candidates and, fused, the residual check of every
        result (LoopCloser.hpp:98, 343-365).  Returns (T (P,4,4), stats, residual (P,), ratio (P,), status (P,)); never raises
        for a failed candidate (its residual is +inf)."""
        return self.align_batch(map_ids, readings, T_inits, dtype=dtype, raise_on_error=False, normals=normals, _residual=True, _raw_stats=raw_stats,
                                noises=noises, radiis=radiis)

    def align_batch(self, map_ids, readings, T_inits, dtype=None, raise_on_error=True, normals=None, _residual=False, _raw_stats=False,
                    noises=None, radiis=None):
        """`_raw_stats`: the pgicp_stats records come back as ONE numpy record array (fields as in include/pgicp.h) instead of a
        list of dicts -- a batch of 512 loop-closure candidates does not need 512 dictionaries to fill 512 edge records.
        `noises`: one `simpleSensorNoise` row per reading (or None for a reading without): the stats dicts then carry
        overlap_noise and n_elements (with `_raw_stats`: read them with last_noise_overlap(p)).
        `radiis`: one row of search radii per reading (or None for a reading without), as arm_reading_radii takes them."""
        P = len(readings)
        if noises is not None and len(noises) != P:
            raise ValueError("align_batch: one noise row (or None) per reading is needed")
        if radiis is not None and len(radiis) != P:
            raise ValueError("align_batch: one row of radii (or None) per reading is needed")
        if isinstance(map_ids, int):
            map_ids = [map_ids] * P
        bufs = _bufs(readings, dtype)
        nbufs = _bufs(normals, bufs[0].dtype) if normals is not None else None
        # the records are filled and read back through numpy views, column by column: per-problem attribute access on
        # ctypes structures cost ~9 us a problem, 1.2 ms of a 15 ms step at 128 problems
        pa = np.zeros(P, dtype=_PROBLEM_DTYPE)
        pa["map_id"] = map_ids
        pa["reading"] = [b.ptr for b in bufs]
        pa["stride"] = [b.stride for b in bufs]
        pa["n"] = [b.n for b in bufs]
        pa["mem"] = [b.mem for b in bufs]
        pa["T_init"] = np.asarray(T_inits, dtype=np.float64).reshape(P, 16)
        if nbufs is not None:
            assert all(nb.n == b.n and nb.mem == b.mem for nb, b in zip(nbufs, bufs))
            pa["normals"] = [b.ptr for b in nbufs]
            pa["nstride"] = [b.stride for b in nbufs]
        T_out = np.empty((P, 4, 4), dtype=np.float64)
        sa = np.zeros(P, dtype=_STATS_DTYPE)
        if noises is not None:
            self.arm_reading_noise(noises, bufs[0].dtype)
        if radiis is not None:
            self.arm_reading_radii(radiis, bufs[0].dtype)
        if _residual:
            res, ratio, rst = np.zeros(P), np.zeros(P), np.zeros(P, dtype=np.int32)
            fn = getattr(self.lib, "pgicp_align_residual_batch" + self._sfx(bufs[0].dtype))
            rc = fn(self.h, C.c_int(P), C.c_void_p(pa.ctypes.data), C.c_void_p(T_out.ctypes.data), C.c_void_p(sa.ctypes.data),
                    C.c_void_p(res.ctypes.data), C.c_void_p(ratio.ctypes.data), C.c_void_p(rst.ctypes.data))
        else:
            fn = getattr(self.lib, "pgicp_align_batch" + self._sfx(bufs[0].dtype))
            rc = fn(self.h, C.c_int(P), C.c_void_p(pa.ctypes.data), C.c_void_p(T_out.ctypes.data), C.c_void_p(sa.ctypes.data))
        if raise_on_error:
            self._check(rc)
        elif rc not in (OK, ERR_NO_MATCH, ERR_NAN, ERR_BOUND):
            self._check(rc)
        if _raw_stats:
            return (T_out, sa, res, ratio, rst) if _residual else (T_out, sa)
        cov = sa["cov"].reshape(P, 6, 6)
        cols = [sa[k].tolist() for k in ("status", "iterations", "converged", "max_iter_reached", "overlap", "residual", "trim_limit",
                                          "n_kept", "n_finite")]
        stats = [dict(status=st, iterations=it, converged=bool(cv), max_iter_reached=bool(mx), overlap=ov, residual=rs, trim_limit=tl,
                      n_kept=nk, n_finite=nf, cov=cov[p])
                 for p, (st, it, cv, mx, ov, rs, tl, nk, nf) in enumerate(zip(*cols))]
        if noises is not None:
            self._noise_into(stats, noises)
        if _residual:
            return T_out, stats, res, ratio, rst
        return T_out, stats

    def icp_pair(self, reading, ref_xyz, ref_nrm, T_init, dtype=None, noise=None, radii=None):
        r = _Buf(reading, dtype)
        x = _Buf(ref_xyz, r.dtype)
        nb = _Buf(ref_nrm, r.dtype)
        assert r.mem == x.mem == nb.mem
        T_out = (C.c_double * 16)()
        st = Stats()
        fn = getattr(self.lib, "pgicp_icp_pair" + self._sfx(r.dtype))
        if noise is not None:
            self.arm_reading_noise([noise], r.dtype)
        if radii is not None:
            self.arm_reading_radii([radii], r.dtype)
        self._check(fn(self.h, C.c_void_p(r.ptr), C.c_int(r.stride), C.c_int(r.n), C.c_void_p(x.ptr), C.c_int(x.stride),
                       C.c_void_p(nb.ptr), C.c_int(nb.stride), C.c_int(x.n), C.c_int(r.mem), _T16(T_init), T_out,
                       C.byref(st)))
        sd = st.as_dict()
        if noise is not None:
            self._noise_into([sd], [noise])
        return np.array(T_out[:]).reshape(4, 4), sd

    # ---- stages -----------------------------------------------------------
    def match(self, map_id, reading, T=None, dtype=None, radii=None):
        """radii: KDTreeVarDistMatcher's search radius of every reading point (arm_reading_radii)"""
        r = _Buf(reading, dtype)
        fn = getattr(self.lib, "pgicp_match" + self._sfx(r.dtype))
        if radii is not None:
            self.arm_reading_radii([radii], r.dtype)
        Tp = _T16(T) if T is not None else None
        k = max(1, int(self.params.knn))
        shape = (r.n,) if k == 1 else (r.n, k)              # knn entries per reading point
        if r.mem == DEVICE:
            import torch
            ids = torch.empty(shape, dtype=torch.int32, device=r.keep.device)
            d2 = torch.empty(shape, dtype=r.keep.dtype, device=r.keep.device)
            self._check(fn(self.h, C.c_int(map_id), C.c_void_p(r.ptr), C.c_int(r.stride), C.c_int(r.n), C.c_int(r.mem),
                           Tp, C.c_void_p(ids.data_ptr()), C.c_void_p(d2.data_ptr())))
            return ids, d2
        ids = np.empty(shape, dtype=np.int32)
        d2 = np.empty(shape, dtype=r.dtype)
        self._check(fn(self.h, C.c_int(map_id), C.c_void_p(r.ptr), C.c_int(r.stride), C.c_int(r.n), C.c_int(r.mem), Tp,
                       C.c_void_p(ids.ctypes.data), C.c_void_p(d2.ctypes.data)))
        return ids, d2

    def outlier_weights(self, d2):
        d2 = np.ascontiguousarray(d2)
        assert d2.dtype in (np.float32, np.float64)
        w = np.empty_like(d2)
        real = C.c_float if d2.dtype == np.float32 else C.c_double
        limit = real(0)
        nf = C.c_int(0)
        fn = getattr(self.lib, "pgicp_outlier_weights" + self._sfx(d2.dtype))
        self._check(fn(self.h, C.c_void_p(d2.ctypes.data), C.c_int(d2.shape[0]), C.c_int(HOST), C.c_void_p(w.ctypes.data),
                       C.byref(limit), C.byref(nf)))
        return w, limit.value, nf.value

    def error_stats(self, map_id, reading, ids, weights, dtype=None):
        r = _Buf(reading, dtype)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=r.dtype)
        ratio, resid = C.c_double(0), C.c_double(0)
        sys_ = (C.c_double * 30)()
        fn = getattr(self.lib, "pgicp_error_stats" + self._sfx(r.dtype))
        self._check(fn(self.h, C.c_int(map_id), C.c_void_p(r.ptr), C.c_int(r.stride), C.c_int(r.n), C.c_int(r.mem),
                       C.c_void_p(ids.ctypes.data), C.c_void_p(w.ctypes.data), C.byref(ratio), C.byref(resid), sys_))
        return ratio.value, resid.value, np.array(sys_[:])

    def partial_chain(self, map_id, reading, T=None, dtype=None, radii=None):
        r = _Buf(reading, dtype)
        ratio, resid = C.c_double(0), C.c_double(0)
        fn = getattr(self.lib, "pgicp_partial_chain" + self._sfx(r.dtype))
        if radii is not None:
            self.arm_reading_radii([radii], r.dtype)
        self._check(fn(self.h, C.c_int(map_id), C.c_void_p(r.ptr), C.c_int(r.stride), C.c_int(r.n), C.c_int(r.mem),
                       _T16(T) if T is not None else None, C.byref(ratio), C.byref(resid)))
        return ratio.value, resid.value

    def partial_chain_seeded(self, map_id, reading, T, src: "Context", src_start, dst_start, dtype=None):
        """pgicp_partial_chain_seeded: the partial chain with its matcher seeded from the correspondences `src`'s last align of THIS
        reading ended with; the two maps as concatenations of keyframe clouds (src_start: n_seg + 1 index boundaries in the ICP's
        map; dst_start: where each segment sits in this map, -1 = absent).  Same result as partial_chain, bit for bit."""
        r = _Buf(reading, dtype)
        ss = np.ascontiguousarray(src_start, dtype=np.int32)
        ds = np.ascontiguousarray(dst_start, dtype=np.int32)
        assert len(ss) == len(ds) + 1
        ratio, resid = C.c_double(0), C.c_double(0)
        fn = getattr(self.lib, "pgicp_partial_chain_seeded" + self._sfx(r.dtype))
        self._check(fn(self.h, C.c_int(map_id), C.c_void_p(r.ptr), C.c_int(r.stride), C.c_int(r.n), C.c_int(r.mem),
                       _T16(T) if T is not None else None, src.h if src is not None else None, C.c_int(len(ds)),
                       C.c_void_p(ss.ctypes.data), C.c_void_p(ds.ctypes.data), C.byref(ratio), C.byref(resid)))
        return ratio.value, resid.value

    def partial_chain_batch(self, map_ids, readings, Ts, dtype=None, raise_on_error=True, radiis=None):
        """(weightedPointUsedRatio, residual, status) arrays of a batch of (map, reading, T) in one device pass.
        radiis: one row of search radii per reading (or None for a reading without), as arm_reading_radii takes them."""
        P = len(readings)
        if radiis is not None and len(radiis) != P:
            raise ValueError("partial_chain_batch: one row of radii (or None) per reading is needed")
        bufs = [_Buf(r, dtype) for r in readings]
        pa = np.zeros(P, dtype=_PROBLEM_DTYPE)              # (numpy views of the records: see align_batch)
        pa["map_id"] = map_ids
        pa["reading"] = [b.ptr for b in bufs]
        pa["stride"] = [b.stride for b in bufs]
        pa["n"] = [b.n for b in bufs]
        pa["mem"] = [b.mem for b in bufs]
        pa["T_init"] = np.asarray(Ts, dtype=np.float64).reshape(P, 16)
        ratio, resid, status = np.zeros(P, dtype=np.float64), np.zeros(P, dtype=np.float64), np.zeros(P, dtype=np.int32)
        fn = getattr(self.lib, "pgicp_partial_chain_batch" + self._sfx(bufs[0].dtype))
        if radiis is not None:
            self.arm_reading_radii(radiis, bufs[0].dtype)
        rc = fn(self.h, C.c_int(P), C.c_void_p(pa.ctypes.data), C.c_void_p(ratio.ctypes.data), C.c_void_p(resid.ctypes.data),
                C.c_void_p(status.ctypes.data))
        if raise_on_error or rc not in (OK, ERR_NO_MATCH):
            self._check(rc)
        return ratio, resid, status

    def transform(self, T, pts, rotate_only=False, dtype=None):
        r = _Buf(pts, dtype)
        assert r.mem == HOST
        out = np.array(r.keep, copy=True)
        fn = getattr(self.lib, "pgicp_transform" + self._sfx(r.dtype))
        self._check(fn(self.h, _T16(T), C.c_void_p(r.ptr), C.c_int(r.stride), C.c_void_p(out.ctypes.data),
                       C.c_int(out.strides[0] // out.itemsize), C.c_int(r.n), C.c_int(int(rotate_only)), C.c_int(HOST)))
        return out

    def build_local_map(self, clouds_xyz, clouds_nrm, T_ref_kf, dtype=np.float32):
        """LocalMap::BuildCloudFromData.  numpy clouds -> numpy outputs; torch CUDA clouds (a device-resident
        keyframe cache) -> torch CUDA outputs, nothing crosses PCIe."""
        k = len(clouds_xyz)
        xs = [_Buf(c, dtype) for c in clouds_xyz]
        ns = [_Buf(c, dtype) for c in clouds_nrm]
        dtype = xs[0].dtype
        mem = xs[0].mem
        assert all(b.mem == mem and b.dtype == dtype for b in xs + ns)
        counts = (C.c_int * k)(*[b.n for b in xs])
        sx = (C.c_int * k)(*[b.stride for b in xs])
        sn = (C.c_int * k)(*[b.stride for b in ns])
        Ts = np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.float64).reshape(4, 4) for t in T_ref_kf]))
        total = sum(b.n for b in xs)
        if mem == DEVICE and isinstance(clouds_xyz[0], DevPtr):
            out_x, out_n = self.device_empty(total, 3, dtype), self.device_empty(total, 3, dtype)     # (the caller frees them)
            px, pn = out_x.ptr, out_n.ptr
        elif mem == DEVICE:
            import torch
            like = clouds_xyz[0]
            out_x = torch.empty((total, 3), dtype=like.dtype, device=like.device)
            out_n = torch.empty((total, 3), dtype=like.dtype, device=like.device)
            px, pn = out_x.data_ptr(), out_n.data_ptr()
        else:
            out_x = np.zeros((total, 3), dtype=dtype)
            out_n = np.zeros((total, 3), dtype=dtype)
            px, pn = out_x.ctypes.data, out_n.ctypes.data
        PP = C.c_void_p * k
        fn = getattr(self.lib, "pgicp_build_local_map" + self._sfx(dtype))
        self._check(fn(self.h, C.c_int(k), PP(*[b.ptr for b in xs]), PP(*[b.ptr for b in ns]), sx, sn, counts,
                       C.c_void_p(Ts.ctypes.data), C.c_void_p(px), C.c_int(3), C.c_void_p(pn), C.c_int(3), C.c_int(mem)))
        return out_x, out_n

    def surface_normals(self, xyz, knn=10, max_dist=float("inf"), dtype=None, want_eigen=False, want_ids=False):
        """SurfaceNormalDataPointsFilter on the device.  numpy in -> numpy out, torch CUDA in -> torch CUDA out.
        Returns normals (n,3) [, eigenvalues (n,3) ascending] [, ids (n,knn), d2 (n,knn)]."""
        s = _Staged(xyz, dtype=dtype)
        x, n, mk, ptr = s.x, s.n, s.mk, s.ptr
        md = 1e300 if not np.isfinite(max_dist) else float(max_dist)
        nrm = mk((n, 3))
        eig = mk((n, 3)) if want_eigen else None
        ids = mk((n, knn), np.int32) if want_ids else None
        d2 = mk((n, knn)) if want_ids else None
        self._check(s.fn(self.lib, "surface_normals")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), C.c_int(knn), C.c_double(md),
            ptr(nrm), C.c_int(3), ptr(eig), ptr(ids), ptr(d2)))
        out = [nrm]
        if want_eigen:
            out.append(eig)
        if want_ids:
            out += [ids, d2]
        return out[0] if len(out) == 1 else tuple(out)

    ELIPSOIDS_ROWS = dict(normals=3, densities=1, eigen_values=3, eigen_vectors=9, covariance=9, weights=1, means=3, shapes=3)
    # the box filters' three entries: what each takes after n_boxes, in its order
    _BOX_ENTRIES = {"sampling_surface_normal": (),
                    "sampling_surface_normal_ext": ("eigen_values", "eigen_vectors", "densities"),
                    "elipsoids": ("eigen_values", "eigen_vectors", "densities", "min_planarity", "covariance", "weights", "means", "shapes")}

    def _box_filter(self, entry, xyz, knn, ratio, method, max_box, seed, desc, average, keep, dtype, min_planarity=0.0, mem=None):
        """One call of an entry of _BOX_ENTRIES: the staging, the outputs (of ELIPSOIDS_ROWS those in `keep`), the call.  Returns
        dict(xyz, kept_idx, descriptors, boxes, and every row of ELIPSOIDS_ROWS), cut to the kept points; what was not asked for is None."""
        s = _Staged(xyz, descriptors=desc, dtype=dtype)
        x, n, d, drows, mk, ptr = s.x, s.n, s.d, s.drows, s.mk, s.ptr
        if mem is not None and {"host": HOST, "device": DEVICE}[mem] != x.mem:
            raise ValueError(f"{entry}: mem={mem!r} but xyz lies in {'host' if x.mem == HOST else 'device'} memory")
        m = max(n, 1)
        ox, oi = mk((m, 3)), mk((m,), np.int32)
        od = mk((m, drows)) if d is not None else None
        rows = {k: (mk((m, w) if w > 1 else (m,)) if k in keep else None) for k, w in self.ELIPSOIDS_ROWS.items()}
        n_out, boxes = C.c_int(0), C.c_int(0)
        tail = [C.c_double(min_planarity) if a == "min_planarity" else ptr(rows[a]) for a in self._BOX_ENTRIES[entry]]
        self._check(s.fn(self.lib, entry)(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), C.c_int(knn), C.c_double(ratio),
            C.c_int(method), C.c_double(max_box), C.c_uint64(int(seed)), ptr(d), C.c_int(drows),
            C.c_int(int(bool(average))), ptr(ox), C.c_int(3), ptr(rows["normals"]), C.c_int(3), ptr(od), ptr(oi),
            C.byref(n_out), C.byref(boxes), *tail))
        k = n_out.value
        cut = lambda a: a[:k] if a is not None else None
        return dict(xyz=ox[:k], kept_idx=oi[:k], descriptors=cut(od), boxes=boxes.value, **{key: cut(a) for key, a in rows.items()})

    def sampling_surface_normal(self, xyz, knn=7, ratio=0.5, sampling_method=0, max_box_dim=float("inf"), seed=1, descriptors=None,
                                average_descriptors=True, dtype=None):
        """SamplingSurfaceNormalDataPointsFilter on the device (pgicp_sampling_surface_normal_*).  numpy in -> numpy out, torch
        CUDA in -> torch CUDA out.  `descriptors`: (n, drows) or None, in the same memory as xyz.  Returns dict(xyz (k,3),
        normals (k,3), kept_idx (k,) int32, descriptors (k,drows) or None, boxes: boxes fused) for the k kept points, in
        ascending input index."""
        r = self._box_filter("sampling_surface_normal", xyz, knn, ratio, sampling_method, max_box_dim, seed, descriptors, average_descriptors,
                             ("normals",), dtype)
        return {key: r[key] for key in ("xyz", "normals", "kept_idx", "descriptors", "boxes")}

    def sampling_surface_normal_ext(self, xyz, knn=7, ratio=0.5, sampling_method=0, max_box_dim=float("inf"), seed=1, descriptors=None,
                                    average_descriptors=True, want_eigen=False, want_eigen_vectors=False, want_densities=False,
                                    want_normals=True, dtype=None):
        """SamplingSurfaceNormalDataPointsFilter with every output it can keep (pgicp_sampling_surface_normal_ext_*, statement in
        include/pgicp_ssn_ext.h).  numpy in -> numpy out, torch CUDA in -> torch CUDA out.  Returns sampling_surface_normal's dict
        and eigen_values (k,3) ascending, eigen_vectors (k,9): three columns in that order, densities (k,) -- the kept point's
        box's; what was not asked for is None."""
        want = dict(normals=want_normals, eigen_values=want_eigen, eigen_vectors=want_eigen_vectors, densities=want_densities)
        r = self._box_filter("sampling_surface_normal_ext", xyz, knn, ratio, sampling_method, max_box_dim, seed, descriptors, average_descriptors,
                             tuple(k for k, w in want.items() if w), dtype)
        return {key: r[key] for key in ("xyz", "normals", "kept_idx", "descriptors", "boxes", "eigen_values", "eigen_vectors", "densities")}

    def elipsoids(self, xyz, knn=7, ratio=0.5, method=0, max_box=float("inf"), min_planarity=0.0, seed=1, desc=None, average=True,
                  keep=("normals",), mem=None, dtype=None):
        """ElipsoidsDataPointsFilter on the device (pgicp_elipsoids_*, statement in include/pgicp_elipsoids.h).  numpy in -> numpy out,
        torch CUDA in -> torch CUDA out; `mem` ("host" or "device"), when given, must name the memory xyz lies in.  `keep`: the rows
        asked for, of ELIPSOIDS_ROWS.  Returns sampling_surface_normal_ext's dict and covariance (k,9), weights (k,), means (k,3),
        shapes (k,3): planarity, cylindricality, sphericality -- the kept point's box's; what was not asked for is None."""
        unknown = set(keep) - set(self.ELIPSOIDS_ROWS)
        if unknown:
            raise ValueError(f"elipsoids: unknown rows {sorted(unknown)} (known: {sorted(self.ELIPSOIDS_ROWS)})")
        return self._box_filter("elipsoids", xyz, knn, ratio, method, max_box, seed, desc, average, keep, dtype, min_planarity, mem)

    def voxel_grid(self, xyz, v_size=(1.0, 1.0, 1.0), use_centroid=True, descriptors=None, average_descriptors=True, dtype=None):
        """VoxelGridDataPointsFilter on the device (pgicp_voxel_grid_*, statement in include/pgicp.h).  numpy in -> numpy out, torch
        CUDA in -> torch CUDA out.  `descriptors`: (n, drows) or None, in the same memory as xyz.  Returns dict(xyz (k,3),
        descriptors (k,drows) or None, kept_idx (k,) int32: each voxel's first point, count (k,) int32: its points) for the k
        non-empty voxels, in ascending first-point index."""
        s = _Staged(xyz, descriptors=descriptors, dtype=dtype)
        x, n, d, drows, mk, ptr = s.x, s.n, s.d, s.drows, s.mk, s.ptr
        m = max(n, 1)
        ox, oi, oc = mk((m, 3)), mk((m,), np.int32), mk((m,), np.int32)
        od = mk((m, drows)) if d is not None else None
        v = (C.c_double * 3)(*[float(c) for c in v_size])
        n_out = C.c_int(0)
        self._check(s.fn(self.lib, "voxel_grid")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), v, C.c_int(int(bool(use_centroid))), ptr(d),
            C.c_int(drows), C.c_int(int(bool(average_descriptors))), ptr(ox), C.c_int(3), ptr(od), ptr(oi), ptr(oc), C.byref(n_out)))
        k = n_out.value
        return dict(xyz=ox[:k], descriptors=od[:k] if od is not None else None, kept_idx=oi[:k], count=oc[:k])

    # ---- densities and MaxDensity (include/pgicp_density.h) ------------------------
    def surface_densities(self, xyz, knn=10, max_dist=float("inf"), dtype=None, want_normals=True, want_eigen=True):
        """SurfaceNormalDataPointsFilter{keepDensities: 1} on the device (pgicp_surface_densities_*): one kernel, no neighbour
        table.  numpy in -> numpy out, torch CUDA in -> torch CUDA out.  Returns dict(normals (n,3) or None, eigen_values (n,3)
        ascending or None, densities (n,))."""
        s = _Staged(xyz, dtype=dtype)
        x, n, mk, ptr = s.x, s.n, s.mk, s.ptr
        md = 1e300 if not np.isfinite(max_dist) else float(max_dist)
        nrm = mk((n, 3)) if want_normals else None
        eig = mk((n, 3)) if want_eigen else None
        dens = mk((n,))
        self._check(s.fn(self.lib, "surface_densities")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), C.c_int(knn), C.c_double(md),
            ptr(nrm), C.c_int(3), ptr(eig), ptr(dens)))
        return dict(normals=nrm, eigen_values=eig, densities=dens)

    def max_density(self, densities, max_density=10.0, seed=1, dtype=None):
        """MaxDensityDataPointsFilter's stage on the device (pgicp_max_density_*): the ascending indices (int32) of the points it
        keeps.  numpy in -> numpy out, torch CUDA in -> torch CUDA out.  (Its input is one-dimensional, not a cloud, so it stages
        its own two buffers.)"""
        if _is_torch(densities) and densities.is_cuda:
            import torch
            d = densities.contiguous()
            n, mem, dt = int(d.shape[0]), DEVICE, np.dtype(str(d.dtype).replace("torch.", ""))
            idx = torch.empty((max(n, 1),), dtype=torch.int32, device=d.device)
            pd, pi = C.c_void_p(d.data_ptr()), C.c_void_p(idx.data_ptr())
        else:
            d = np.ascontiguousarray(np.asarray(densities), dtype=dtype)
            assert d.ndim == 1 and d.dtype in (np.float32, np.float64)
            n, mem, dt = len(d), HOST, d.dtype
            idx = np.empty(max(n, 1), dtype=np.int32)
            pd, pi = C.c_void_p(d.ctypes.data), C.c_void_p(idx.ctypes.data)
        n_out = C.c_int(0)
        fn = getattr(self.lib, "pgicp_max_density" + self._sfx(dt))
        self._check(fn(self.h, pd, C.c_int(n), C.c_int(mem), C.c_double(float(max_density)), C.c_uint64(int(seed)), pi, C.byref(n_out)))
        return idx[:n_out.value]

    def normals_max_density(self, xyz, knn=10, max_dist=float("inf"), max_density=10.0, seed=1, descriptors=None, dtype=None):
        """SurfaceNormal{keepDensities} -> MaxDensity as one device pass (pgicp_normals_max_density_*).  numpy in -> numpy out,
        torch CUDA in -> torch CUDA out.  `descriptors`: (n, drows) or None, in the same memory as xyz.  Returns dict(xyz (k,3),
        normals (k,3), eigen_values (k,3), densities (k,), descriptors (k,drows) or None, kept_idx (k,) int32) for the k kept
        points, in ascending input index."""
        s = _Staged(xyz, descriptors=descriptors, dtype=dtype)
        x, n, d, drows, mk, ptr = s.x, s.n, s.d, s.drows, s.mk, s.ptr
        md = 1e300 if not np.isfinite(max_dist) else float(max_dist)
        m = max(n, 1)
        ox, on, oe, od, oi = mk((m, x.stride)), mk((m, 3)), mk((m, 3)), mk((m,)), mk((m,), np.int32)
        oc = mk((m, drows)) if d is not None else None
        n_out = C.c_int(0)
        self._check(s.fn(self.lib, "normals_max_density")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), C.c_int(knn), C.c_double(md),
            C.c_double(float(max_density)), C.c_uint64(int(seed)), ptr(d), C.c_int(drows), ptr(ox), ptr(on), C.c_int(3), ptr(oe),
            ptr(od), ptr(oc), ptr(oi), C.byref(n_out)))
        k = n_out.value
        return dict(xyz=ox[:k, :3], normals=on[:k], eigen_values=oe[:k], densities=od[:k],
                    descriptors=oc[:k] if oc is not None else None, kept_idx=oi[:k])

    # ---- the sensor filter chain (include/pgicp_sensor_chain.h) ------------------------
    SENSOR_CHAIN_STAGES = dict(observation_direction=(CHAIN_OBSERVATION_DIRECTION, 3), orient_normals=(CHAIN_ORIENT_NORMALS, 1),
                               shadow=(CHAIN_SHADOW, 1), max_density=(CHAIN_MAX_DENSITY, 2), simple_sensor_noise=(CHAIN_SIMPLE_SENSOR_NOISE, 2),
                               incidence_angle=(CHAIN_INCIDENCE_ANGLE, 0), sphericality=(CHAIN_SPHERICALITY, 2),
                               cut_at_descriptor=(CHAIN_CUT_AT_DESCRIPTOR, 4))
    SENSOR_CHAIN_ROWS = dict(normals=3, eigen_values=3, densities=1)

    @classmethod
    def chain_stages(cls, stages):
        """a list of tuples such as ("shadow", 0.1), ("observation_direction", 0, 0, 0), ("max_density", 100.0, 1) as an array of
        pgicp_chain_stage; a stage may also be given as (type number, p0, ...).  Parameters left out are 0 (max_density's seed: 1).
        ("sphericality", keepUnstructureness, keepStructureness); ("cut_at_descriptor", row, useLargerThan, threshold) with row a
        name of CHAIN_ROWS, or the index of a row of `desc`."""
        arr = (ChainStage * max(len(stages), 1))()
        for k, s in enumerate(stages):
            name, args = s[0], list(s[1:])
            if name == "cut_at_descriptor" and args:
                if isinstance(args[0], str):
                    if args[0] not in CHAIN_ROWS or args[0] == "desc":
                        raise ValueError(f"sensor_chain: unknown row {args[0]!r} (known: {sorted(set(CHAIN_ROWS) - {'desc'})}, or an index into desc)")
                    args = [CHAIN_ROWS[args[0]]] + args[1:3]
                else:
                    args = [CHAIN_ROWS["desc"]] + args[1:3] + [0] * (3 - len(args)) + [int(args[0])]
            args = [float(v) for v in args]
            if isinstance(name, str):
                if name not in cls.SENSOR_CHAIN_STAGES:
                    raise ValueError(f"sensor_chain: unknown stage {name!r} (known: {sorted(cls.SENSOR_CHAIN_STAGES)})")
                typ, np_ = cls.SENSOR_CHAIN_STAGES[name]
                if len(args) > np_:
                    raise ValueError(f"sensor_chain: stage {name!r} takes at most {np_} parameters")
                if name == "max_density" and len(args) == 1:
                    args.append(1.0)
            else:
                typ = int(name)
            arr[k].type = typ
            for j, v in enumerate(args[:4]):
                arr[k].p[j] = v
        return arr

    def sensor_chain(self, xyz, knn=10, max_dist=float("inf"), stages=(), keep=("normals", "densities"), desc=None, mem=None, dtype=None):
        """SurfaceNormalDataPointsFilter{knn, maxDist} and a list of stages -- ObservationDirection, OrientNormals, Shadow,
        MaxDensity, SimpleSensorNoise -- as one device call (pgicp_sensor_chain_*, statement in include/pgicp_sensor_chain.h); a
        list that holds IncidenceAngle, Sphericality or CutAtDescriptor goes to pgicp_sensor_chain_ext_*
        (include/pgicp_descriptor_filters.h) and may be CHAIN_EXT_MAX_STAGES long.  numpy
        in -> numpy out, torch CUDA in -> torch CUDA out; `mem` ("host" or "device"), when given, must name the memory xyz lies in.
        `stages`: see chain_stages.  `keep`: the head's rows, of SENSOR_CHAIN_ROWS.  Returns dict(xyz (k,3), kept_idx (k,) int32,
        count, descriptors (k,drows) or None, normals, eigen_values, densities, observation_directions (k,3), noise (k,),
        incidence_angles, sphericality, unstructureness, structureness (k,)) for the k kept points in input order; a row that is not kept, or whose stage is not listed, is None."""
        unknown = set(keep) - set(self.SENSOR_CHAIN_ROWS)
        if unknown:
            raise ValueError(f"sensor_chain: unknown rows {sorted(unknown)} (known: {sorted(self.SENSOR_CHAIN_ROWS)})")
        stages = list(stages)
        arr = self.chain_stages(stages)
        listed = {int(arr[k].type) for k in range(len(stages))}
        s = _Staged(xyz, descriptors=desc, dtype=dtype)
        x, n, d, drows, mk, ptr = s.x, s.n, s.d, s.drows, s.mk, s.ptr
        if mem is not None and {"host": HOST, "device": DEVICE}[mem] != x.mem:
            raise ValueError(f"sensor_chain: mem={mem!r} but xyz lies in {'host' if x.mem == HOST else 'device'} memory")
        md = 1e300 if not np.isfinite(max_dist) else float(max_dist)
        m = max(n, 1)
        ox, oi = mk((m, x.stride)), mk((m,), np.int32)
        oc = mk((m, drows)) if d is not None else None
        rows = {k: (mk((m, w) if w > 1 else (m,)) if k in keep else None) for k, w in self.SENSOR_CHAIN_ROWS.items()}
        obs = mk((m, 3)) if CHAIN_OBSERVATION_DIRECTION in listed else None
        noise = mk((m,)) if CHAIN_SIMPLE_SENSOR_NOISE in listed else None
        n_out = C.c_int(0)
        head = (self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), C.c_int(knn), C.c_double(md),
                C.c_int(int("normals" in keep)), C.c_int(int("eigen_values" in keep)), C.c_int(int("densities" in keep)),
                C.c_int(len(stages)), arr, ptr(d), C.c_int(drows))
        more = dict(incidence_angles=None, sphericality=None, unstructureness=None, structureness=None)
        if listed & {CHAIN_INCIDENCE_ANGLE, CHAIN_SPHERICALITY, CHAIN_CUT_AT_DESCRIPTOR}:
            sph = [arr[k] for k in range(len(stages)) if arr[k].type == CHAIN_SPHERICALITY]
            more["incidence_angles"] = mk((m,)) if CHAIN_INCIDENCE_ANGLE in listed else None
            more["sphericality"] = mk((m,)) if sph else None
            more["unstructureness"] = mk((m,)) if sph and sph[0].p[0] == 1.0 else None
            more["structureness"] = mk((m,)) if sph and sph[0].p[1] == 1.0 else None
            out = ChainOut(ptr(ox), ptr(rows["normals"]), 3, ptr(rows["eigen_values"]), ptr(rows["densities"]), ptr(obs), ptr(noise), ptr(oc),
                           ptr(more["incidence_angles"]), ptr(more["sphericality"]), ptr(more["unstructureness"]), ptr(more["structureness"]), ptr(oi))
            self._check(s.fn(self.lib, "sensor_chain_ext")(*head, C.byref(out), C.byref(n_out)))
        else:
            self._check(s.fn(self.lib, "sensor_chain")(*head, ptr(ox), ptr(rows["normals"]), C.c_int(3), ptr(rows["eigen_values"]),
                                                       ptr(rows["densities"]), ptr(obs), ptr(noise), ptr(oc), ptr(oi), C.byref(n_out)))
        k = n_out.value
        cut = lambda a: a[:k] if a is not None else None
        return dict(xyz=ox[:k, :3], kept_idx=oi[:k], count=k, descriptors=cut(oc), observation_directions=cut(obs), noise=cut(noise),
                    **{key: cut(a) for key, a in rows.items()}, **{key: cut(a) for key, a in more.items()})

    # ---- CovarianceSampling (include/pgicp_covsample.h) ------------------------
    def covariance_sampling(self, xyz, normals, nb_sample=5000, torque_norm=1, descriptors=None, dtype=None, frame=None):
        """CovarianceSamplingDataPointsFilter on the device (pgicp_covariance_sampling_*, statement in include/pgicp_covsample.h).
        numpy in -> numpy out, torch CUDA in -> torch CUDA out.  `normals` (n, >= 3) and `descriptors` ((n, drows) or None) in the
        same memory as xyz.  Returns dict(xyz (k,3), normals (k,3), descriptors (k,drows) or None, kept_idx (k,) int32, frame) for
        the k = min(n, nb_sample) picks, in pick order; frame = dict(center (3,), L, eigenvalues (6,) ascending, basis (6,6):
        eigenvectors as columns).  `frame` given: the selection stage alone (pgicp_covariance_sampling_framed_*) -- kept_idx is
        the stage's, the rows are gathered from it here, the frame comes back as given."""
        s = _Staged(xyz, normals, descriptors, dtype)
        x, nb, n, d, drows, mk, ptr = s.x, s.nb, s.n, s.d, s.drows, s.mk, s.ptr
        m = max(min(n, int(nb_sample)), 1)
        oi = mk((m,), np.int32)
        n_out = C.c_int(0)
        if frame is not None:
            fr = CovFrame.from_dict(frame)
            self._check(s.fn(self.lib, "covariance_sampling_framed")(
                self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_void_p(nb.ptr), C.c_int(nb.stride), C.c_int(n), C.c_int(x.mem),
                C.c_int(int(nb_sample)), C.byref(fr), ptr(oi), C.byref(n_out)))
            idx = oi[:n_out.value]
            return dict(xyz=s.rows(x.keep, idx)[:, :3], normals=s.rows(nb.keep, idx)[:, :3],
                        descriptors=s.rows(d, idx) if d is not None else None, kept_idx=idx, frame=fr.as_dict())
        ox, on = mk((m, x.stride)), mk((m, 3))
        oc = mk((m, drows)) if d is not None else None
        fr = CovFrame()
        self._check(s.fn(self.lib, "covariance_sampling")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_void_p(nb.ptr), C.c_int(nb.stride), C.c_int(n), C.c_int(x.mem),
            C.c_int(int(nb_sample)), C.c_int(int(torque_norm)), ptr(d), C.c_int(drows), ptr(ox), ptr(on), C.c_int(3), ptr(oc), ptr(oi),
            C.byref(n_out), C.byref(fr)))
        k = n_out.value
        return dict(xyz=ox[:k, :3], normals=on[:k], descriptors=oc[:k] if oc is not None else None, kept_idx=oi[:k], frame=fr.as_dict())

    # ---- OctreeGrid (include/pgicp_octree.h) ------------------------
    def octree_grid(self, xyz, max_point_by_node=1, max_size_by_node=0.0, sampling_method=0, seed=1, descriptors=None, dtype=None):
        """OctreeGridDataPointsFilter on the device (pgicp_octree_grid_*, statement in include/pgicp_octree.h).  numpy in -> numpy
        out, torch CUDA in -> torch CUDA out.  `descriptors`: (n, drows) or None, in the same memory as xyz.  sampling_method: 0
        first point, 1 random (seeded), 2 centroid, 3 medoid.  Returns dict(xyz (k,3), descriptors (k,drows) or None, kept_idx (k,)
        int32: the leaf's first point for method 2, the kept point otherwise, count (k,) int32: the leaf's points, depth (k,)
        int32: the leaf's depth) for the k non-empty leaves, in depth-first leaf order."""
        s = _Staged(xyz, descriptors=descriptors, dtype=dtype)
        x, n, d, drows, mk, ptr = s.x, s.n, s.d, s.drows, s.mk, s.ptr
        m = max(n, 1)
        ox, oi, oc, op = mk((m, 3)), mk((m,), np.int32), mk((m,), np.int32), mk((m,), np.int32)
        od = mk((m, drows)) if d is not None else None
        n_out = C.c_int(0)
        self._check(s.fn(self.lib, "octree_grid")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), C.c_int(int(max_point_by_node)),
            C.c_double(float(max_size_by_node)), C.c_int(int(sampling_method)), C.c_uint64(int(seed)), ptr(d), C.c_int(drows), ptr(ox),
            C.c_int(3), ptr(od), ptr(oi), ptr(oc), ptr(op), C.byref(n_out)))
        k = n_out.value
        return dict(xyz=ox[:k], descriptors=od[:k] if od is not None else None, kept_idx=oi[:k], count=oc[:k], depth=op[:k])

    # ---- NormalSpace (include/pgicp_normalspace.h) ------------------------
    def normal_space_sampling(self, xyz, normals, nb_sample, epsilon=0.09, seed=1, descriptors=None, dtype=None):
        """NormalSpaceDataPointsFilter on the device (pgicp_normal_space_sampling_*, statement in include/pgicp_normalspace.h).
        numpy in -> numpy out, torch CUDA in -> torch CUDA out.  `normals` (n, >= 3) and `descriptors` ((n, drows) or None) in the
        same memory as xyz.  Returns dict(xyz (k,3), normals (k,3), descriptors (k,drows) or None, kept_idx (k,) int32, bucket (k,)
        int32: the pick's bucket, -1 for the no-op) for the k = min(n, nb_sample) picks, in pick order."""
        s = _Staged(xyz, normals, descriptors, dtype)
        x, nb, n, d, drows, mk, ptr = s.x, s.nb, s.n, s.d, s.drows, s.mk, s.ptr
        m = max(min(n, max(int(nb_sample), 0)), 1)
        ox, on, oi, ob = mk((m, x.stride)), mk((m, 3)), mk((m,), np.int32), mk((m,), np.int32)
        oc = mk((m, drows)) if d is not None else None
        n_out = C.c_int(0)
        self._check(s.fn(self.lib, "normal_space_sampling")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_void_p(nb.ptr), C.c_int(nb.stride), C.c_int(n), C.c_int(x.mem),
            C.c_int(int(nb_sample)), C.c_double(float(epsilon)), C.c_uint64(int(seed)), ptr(d), C.c_int(drows), ptr(ox), ptr(on),
            C.c_int(3), ptr(oc), ptr(oi), ptr(ob), C.byref(n_out)))
        k = n_out.value
        return dict(xyz=ox[:k, :3], normals=on[:k], descriptors=oc[:k] if oc is not None else None, kept_idx=oi[:k], bucket=ob[:k])

    # ---- the rest of SurfaceNormal's outputs (include/pgicp_normals_ext.h) ------------------------
    def surface_normals_ext(self, xyz, knn=10, max_dist=float("inf"), smooth=False, want_normals=True, want_eigen=False,
                            want_eigen_vectors=False, want_mean_dist=False, want_matched_ids=False, want_ids=False, want_densities=False,
                            dtype=None):
        """SurfaceNormalDataPointsFilter with every output it can keep (pgicp_surface_normals_ext_*, statement in
        include/pgicp_normals_ext.h).  numpy in -> numpy out, torch CUDA in -> torch CUDA out.  Returns dict(normals (n,3) --
        smoothed when `smooth` --, eigen_values (n,3) ascending, eigen_vectors (n,9): three columns in that order, mean_dists (n,),
        matched_ids (n,knn) in the cloud's dtype, ids (n,knn) int32, d2 (n,knn), densities (n,)); what was not asked for is None."""
        s = _Staged(xyz, dtype=dtype)
        x, n, mk, ptr = s.x, s.n, s.mk, s.ptr
        md = 1e300 if not np.isfinite(max_dist) else float(max_dist)
        knn = int(knn)
        k = max(knn, 0)
        nrm = mk((n, 3)) if want_normals else None
        eig = mk((n, 3)) if want_eigen else None
        vec = mk((n, 9)) if want_eigen_vectors else None
        dist = mk((n,)) if want_mean_dist else None
        mid = mk((n, k)) if want_matched_ids else None
        ids = mk((n, k), np.int32) if want_ids else None
        d2 = mk((n, k)) if want_ids else None
        dens = mk((n,)) if want_densities else None
        self._check(s.fn(self.lib, "surface_normals_ext")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(n), C.c_int(x.mem), C.c_int(knn), C.c_double(md), C.c_int(int(bool(smooth))),
            ptr(nrm), C.c_int(3), ptr(eig), ptr(vec), ptr(dist), ptr(mid), ptr(ids), ptr(d2), ptr(dens)))
        return dict(normals=nrm, eigen_values=eig, eigen_vectors=vec, mean_dists=dist, matched_ids=mid, ids=ids, d2=d2, densities=dens)

    def smooth_normals(self, normals, ids, dtype=None):
        """The smoothing step of SurfaceNormalDataPointsFilter{smoothNormals: 1} alone (pgicp_smooth_normals_*): `normals` (n, >= 3),
        `ids` (n, knn) integers in the same memory, row i the neighbours of point i, -1 = none.  numpy in -> numpy out, torch CUDA
        in -> torch CUDA out.  Returns the smoothed normals (n,3); an id outside [-1, n) raises."""
        s = _Staged(normals, dtype=dtype)
        x, n, mk, ptr = s.x, s.n, s.mk, s.ptr
        if s.mem == DEVICE:
            import torch
            t = ids.to(torch.int32).contiguous()
            assert t.is_cuda and t.dim() == 2 and t.shape[0] == n
        else:
            t = np.ascontiguousarray(ids, dtype=np.int32)
            assert t.ndim == 2 and t.shape[0] == n
        out = mk((n, 3))
        self._check(s.fn(self.lib, "smooth_normals")(
            self.h, C.c_void_p(x.ptr), C.c_int(x.stride), ptr(t), C.c_int(int(t.shape[1])), C.c_int(n), C.c_int(x.mem), ptr(out), C.c_int(3)))
        return out

    # ---- MaxQuantileOnAxis (include/pgicp_quantile.h) ------------------------
    def axis_quantile(self, features, dim, ratio, dtype=None):
        """The selection of MaxQuantileOnAxisDataPointsFilter{dim, ratio} over a whole cloud (pgicp_axis_quantile_*, statement in
        include/pgicp_quantile.h): `features` (n, >= 3) a host array, a torch CUDA tensor or a DevPtr -- from device memory only
        the three scalars come down.  Returns (limit as a scalar of the cloud's dtype, k, the number of values below limit)."""
        x = _Buf(features if isinstance(features, DevPtr) else _unempty(features, dtype), dtype)
        assert x.dtype in (np.float32, np.float64)
        limit = (C.c_float if x.dtype == np.float32 else C.c_double)(0)
        k, below = C.c_int(0), C.c_int(0)
        fn = getattr(self.lib, "pgicp_axis_quantile" + self._sfx(x.dtype))
        self._check(fn(self.h, C.c_void_p(x.ptr), C.c_int(x.stride), C.c_int(x.n), C.c_int(x.mem), C.c_int(int(dim)), C.c_double(float(ratio)),
                       C.byref(limit), C.byref(k), C.byref(below)))
        return x.dtype.type(limit.value), k.value, below.value

    def adopt_map(self, other: "Context", map_id: int) -> int:
        """Take over a map built by another context of the same device (pgicp_map_transfer)."""
        new_id = C.c_int(-1)
        self._check(self.lib.pgicp_map_transfer(other.h, C.c_int(map_id), self.h, C.byref(new_id)))
        return new_id.value

    def filter_cloud(self, filters, features, descriptors=None, T=None, rotate_rows=(-1, -1), want_idx=True):
        """pgicp_filter_cloud: `filters` = [(type, p0, p1, ...)], `features` (n, frows) host array (a point per row),
        `descriptors` (n, drows) or None.  Returns (features_out, descriptors_out, kept_idx, DevPtr of the device copy)."""
        f = np.ascontiguousarray(features)
        assert f.dtype in (np.float32, np.float64) and f.ndim == 2
        n, frows = f.shape
        d = np.ascontiguousarray(descriptors, dtype=f.dtype) if descriptors is not None else None
        drows = d.shape[1] if d is not None else 0
        fl = (Filter * max(1, len(filters)))()
        for k, spec in enumerate(filters):
            fl[k].type = int(spec[0])
            for j, v in enumerate(spec[1:]):
                fl[k].p[j] = float(v)
        of = np.empty_like(f)
        od = np.empty_like(d) if d is not None else None
        idx = np.empty(n, dtype=np.int32) if want_idx else None
        n_out = C.c_int(0)
        dev = C.c_void_p()
        fn = getattr(self.lib, "pgicp_filter_cloud" + self._sfx(f.dtype))
        self._check(fn(self.h, C.c_int(len(filters)), fl, C.c_void_p(f.ctypes.data), C.c_int(frows),
                       C.c_void_p(d.ctypes.data) if d is not None else None, C.c_int(drows), C.c_int(n), _T16(T) if T is not None else None,
                       C.c_int(rotate_rows[0]), C.c_int(rotate_rows[1]), C.c_void_p(of.ctypes.data),
                       C.c_void_p(od.ctypes.data) if od is not None else None, C.c_void_p(idx.ctypes.data) if idx is not None else None,
                       C.byref(n_out), C.byref(dev)))
        k = n_out.value
        return of[:k], (od[:k] if od is not None else None), (idx[:k] if idx is not None else None), DevPtr(dev.value, frows, k, f.dtype)

    # ---- measurement --------------------------------------------------------
    def filter_cloud_dev(self, filters, features, dropped_cap=4096):
        """pgicp_filter_cloud_dev: the device pass alone (no transformation, the host arrays untouched): (kept count, DevPtr of the
        filtered features, ascending indices of the dropped points -- None when more than dropped_cap were dropped)"""
        f = np.ascontiguousarray(features)
        assert f.ndim == 2 and f.dtype in (np.float32, np.float64)
        n, frows = f.shape
        specs = (Filter * max(1, len(filters)))()
        for k, s_ in enumerate(filters):
            specs[k].type = int(s_[0])
            for j, v in enumerate(s_[1:]):
                specs[k].p[j] = float(v)
        dropped = np.empty(max(1, dropped_cap), dtype=np.int32)
        nd, nout, dev = C.c_int(0), C.c_int(0), C.c_void_p(0)
        fn = getattr(self.lib, "pgicp_filter_cloud_dev" + self._sfx(f.dtype))
        self._check(fn(self.h, C.c_int(len(filters)), specs, C.c_void_p(f.ctypes.data), C.c_int(frows), C.c_int(n), C.c_void_p(dropped.ctypes.data),
                       C.c_int(dropped_cap), C.byref(nd), C.byref(nout), C.byref(dev)))
        return nout.value, DevPtr(dev.value, frows, nout.value, f.dtype), (dropped[:nd.value].copy() if nd.value <= dropped_cap else None)

    def profile_enable(self, on=True):
        self._check(self.lib.pgicp_profile_enable(self.h, C.c_int(int(on))))

    def debug_counters(self):
        out = (C.c_int * 4)()
        self._check(self.lib.pgicp_debug_counters(self.h, out))
        return list(out)

    def debug_last_matches(self, n, problem=0, dtype=np.float32):
        """Correspondences of the last iteration of the last align call (diagnostics; see pgicp.h)."""
        k = max(1, int(self.params.knn))
        ids = np.empty(n if k == 1 else (n, k), dtype=np.int32)
        d2 = np.empty(n if k == 1 else (n, k), dtype=dtype)
        fn = getattr(self.lib, "pgicp_debug_last_matches" + self._sfx(dtype))
        self._check(fn(self.h, C.c_int(problem), C.c_void_p(ids.ctypes.data), C.c_void_p(d2.ctypes.data)))
        return ids, d2

    def reading_order(self, n, problem=0):
        """pgicp_debug_reading_order: order[j] = index, in the caller's reading, of the point the last call sorted to position j --
        with sum_order = SUM_ORDER_SORTED the order the pairs entered the reduction tree in (hand it to the oracle as pair_order)."""
        out = np.empty(n, dtype=np.int32)
        self._check(self.lib.pgicp_debug_reading_order(self.h, C.c_int(problem), C.c_void_p(out.ctypes.data)))
        return out

    def profile_reset(self):
        self._check(self.lib.pgicp_profile_reset(self.h))

    def profile(self):
        out = {}
        for kid, name in enumerate(PROF_NAMES):
            n, ms, u, pr = C.c_longlong(0), C.c_double(0), C.c_longlong(0), C.c_longlong(0)
            self._check(self.lib.pgicp_profile_get(self.h, C.c_int(kid), C.byref(n), C.byref(ms), C.byref(u), C.byref(pr)))
            out[name] = dict(launches=n.value, total_ms=ms.value, units=u.value, problems=pr.value)
        return out


def shard_pairs(costs, world_size, rank):
    """pgicp_shard_pairs: host-only LPT split of candidate ICPs over ranks."""
    lib = load_library()
    costs = np.ascontiguousarray(costs, dtype=np.int64)
    n = costs.shape[0]
    out = np.empty(max(n, 1), dtype=np.int32)
    cnt = C.c_int(0)
    st = lib.pgicp_shard_pairs(C.c_int(n), C.c_void_p(costs.ctypes.data), C.c_int(world_size), C.c_int(rank),
                               C.c_void_p(out.ctypes.data), C.c_int(n), C.byref(cnt))
    if st != OK:
        raise PgicpError(st, "pgicp_shard_pairs")
    return out[: cnt.value].copy()


def check_icp_results(stats_records: np.ndarray, residual_error: np.ndarray, overlap_threshold=0.8, residual_error_threshold=5000.0) -> np.ndarray:
    """LoopCloser::CheckIcpResult (LoopCloser.hpp:308-340) over a record array of pgicp_stats: pgicp_check_icp_result called on
    every record in place (no per-candidate Python objects)."""
    lib = load_library()
    sa = np.ascontiguousarray(stats_records)
    assert sa.dtype == _STATS_DTYPE
    res = np.asarray(residual_error, dtype=np.float64)
    out = np.empty(len(sa), dtype=np.int32)
    base, step = sa.ctypes.data, sa.dtype.itemsize
    fn = lib.pgicp_check_icp_result
    ot, rt = C.c_double(overlap_threshold), C.c_double(residual_error_threshold)
    for k in range(len(sa)):
        out[k] = fn(C.c_void_p(base + k * step), C.c_double(res[k]), ot, rt)
    return out


def check_icp_result(stats: dict, residual_error, overlap_threshold=0.8, residual_error_threshold=5000.0) -> bool:
    """LoopCloser::CheckIcpResult (LoopCloser.hpp:308-340) through the C ABI."""
    lib = load_library()
    s = Stats()
    s.status = stats["status"]
    s.max_iter_reached = int(stats["max_iter_reached"])
    s.overlap = stats["overlap"]
    return bool(lib.pgicp_check_icp_result(C.byref(s), C.c_double(residual_error), C.c_double(overlap_threshold),
                                           C.c_double(residual_error_threshold)))
