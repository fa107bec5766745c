"""Host-side mirror of the scan-matcher interface, over the C-ABI (include/ndt_hip.h).

``NdtMatcher2D`` is the Python twin of the C++ adapter ``ndt::NdtMatcherHip``
(include/ndt_matcher_hip.hpp): set a target scan/submap, align a source scan from an
initial SE(2) guess, get back pose + information matrix - the quantities a
scan-matcher -> GTSAM BetweenFactor<Pose2> bridge needs (BASELINE.json north_star; the
reference's own interface is not observable, /root/reference/README.md:1).

numpy arrays go through the host-pointer entry points; torch CUDA tensors (or any object
with ``data_ptr()``) go through the ``_dev`` entry points without a copy.  PyTorch is only
plumbing for device memory here.

The 2D and the 3D classes share their code: ``_Dim`` says what differs between ``ndt2d_*`` and ``ndt3d_*`` (coordinate
count, pose length, struct types, result dataclass; the prefix is the class's ``_prefix``), ``_Handle`` is the life cycle of a library handle,
and ``_NdtMatcher`` / ``_NdtBatch`` / ``_NdtMulti`` / ``_NdtPyramid`` / ``_NdtMapPyramid`` hold every method once,
over a tuple of coordinate arrays.  The public classes add the explicit per-dimension signatures (one-line forwards)
and what the ABI really has twice: the constructors, ``reserve_target`` and the search window.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .search import SearchHit


@dataclass
class AlignResult:
    pose: tuple            # (tx, ty, theta)
    H: np.ndarray          # 3x3 Hessian of -score (information up to score scaling)
    g: np.ndarray
    score: float
    iterations: int
    n_hit: int
    status: int

    @property
    def converged(self) -> bool:
        return self.status == L.NDT_OK

    def covariance(self, hessian_mode: int = L.HESSIAN_GAUSS_NEWTON) -> np.ndarray:
        """The calibrated pose covariance a BetweenFactor noise model is built from
        (ndt2d_calibrated_covariance: S H^-1 S, factors from the Monte-Carlo calibration;
        hessian_mode = the form of H, i.e. the matcher's hessian_mode).  H^-1 alone underestimates
        the scatter of the estimate 3 to 4 times in standard deviation."""
        H = np.ascontiguousarray(self.H, dtype=np.float64)
        cov = np.zeros(9, dtype=np.float64)
        st = L.load().ndt2d_calibrated_covariance(H.ctypes.data_as(C.POINTER(C.c_double)), int(hessian_mode),
                                                  cov.ctypes.data_as(C.POINTER(C.c_double)))
        if st != L.NDT_OK:
            raise np.linalg.LinAlgError("Hessian is not positive definite")
        return cov.reshape(3, 3)


@dataclass
class AlignResult3D:
    pose: tuple            # (tx, ty, tz, roll, pitch, yaw), R = Rz(yaw) Ry(pitch) Rx(roll)
    H: np.ndarray          # 6x6 Gauss-Newton Hessian of -score
    g: np.ndarray
    score: float
    iterations: int
    n_hit: int
    status: int


@dataclass
class PointFit:
    """What fit_points / select_points report (ndt_point_fit of include/ndt_hip.h).  The four class counts add up to
    the scan's length and count points: with overlap_grids = 4 a point in valid cells of several grids is one hit here."""
    m: object              # float32 [n]: q' Sigma^-1 q of every hit, +inf for a miss, NaN for an invalid point (None after select_points)
    cls: object            # uint8 [n]: L.POINT_CLASS (None after select_points)
    n_invalid: int
    n_miss: int
    n_misfit: int
    n_fit: int
    n_selected: int = 0

    @property
    def n_hit(self) -> int:
        return self.n_misfit + self.n_fit

    @property
    def fitness(self) -> float:
        """The share of the finite points that lie within max_m of their cell (0 for a scan without one)."""
        finite = self.n_miss + self.n_misfit + self.n_fit
        return self.n_fit / finite if finite else 0.0


@dataclass
class VoxelFilterInfo:
    """What voxel_filter counted (ndt_voxel_filter_info of include/ndt_hip.h)."""
    n_invalid: int         # points skipped: a coordinate not finite, or a lattice index of 2^30 or more
    n_voxels: int          # occupied voxels
    n_out: int             # those with n >= min_points: the length of the outputs


def _keep_mask(keep) -> int:
    """keep of select_points: a mask of 1 << class, or class names out of L.POINT_CLASS."""
    if isinstance(keep, str):
        keep = (keep,)
    if isinstance(keep, (int, np.integer)):
        return int(keep)
    mask = 0
    for k in keep:
        if k not in L.POINT_CLASS:
            raise ValueError(f"keep: {k!r} is not one of {sorted(L.POINT_CLASS)}")
        mask |= 1 << L.POINT_CLASS[k]
    return mask


def _default_params(prefix: str, overrides: dict) -> L.Params2D:
    p = L.Params2D()
    getattr(L.load(), prefix + "_default_params")(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(f"{prefix}_params has no field {k!r}")
        setattr(p, k, v)
    return p


def default_params(**overrides) -> L.Params2D:
    return _default_params("ndt2d", overrides)


def default_params3d(**overrides) -> L.Params2D:
    return _default_params("ndt3d", overrides)


def _params_2d(params: L.Params2D | None, overrides: dict) -> L.Params2D:
    """The params= / **overrides of the 2D constructors: the overrides go into the caller's struct when there is one."""
    if params is None:
        return default_params(**overrides)
    for k, v in overrides.items():
        setattr(params, k, v)
    return params


class _Dim:
    """What differs between the ndt2d_* and the ndt3d_* half of the ABI, for the code both share."""

    def __init__(self, ncoord, npose, Result, Eval, GridInfo, SearchHit, AlignResult, default_params):
        self.ncoord = ncoord                    # coordinate arrays of a cloud, and the width of a mean row
        self.nsym = ncoord * (ncoord + 1) // 2  # the width of a covariance row: 3 / 6
        self.npose = npose                      # 3 / 6
        self.Pose = C.c_double * npose
        self.Result, self.Eval, self.GridInfo, self.SearchHit = Result, Eval, GridInfo, SearchHit
        self.AlignResult = AlignResult
        self.default_params = default_params
        self.result_doubles = C.sizeof(Result) // 8

    def pose(self, values):
        return self.Pose(*[float(v) for v in values])

    def poses(self, values, m: int = -1) -> np.ndarray:
        return np.ascontiguousarray(values, dtype=np.float64).reshape(m, self.npose)

    def result(self, r):
        return self.AlignResult(tuple(r.pose), np.array(r.H, dtype=np.float64).reshape(self.npose, self.npose),
                                np.array(r.g, dtype=np.float64), float(r.score), int(r.iterations), int(r.n_hit),
                                int(r.status))

    def results(self, buf: np.ndarray, n: int):
        """n result rows held as float64 words -> list of AlignResult."""
        arr = (self.Result * n).from_buffer_copy(np.ascontiguousarray(buf).tobytes())
        return [self.result(r) for r in arr]

    def evaluation(self, e):
        """(H, g, score, n_hit) of an Eval struct."""
        return (np.array(e.H, dtype=np.float64).reshape(self.npose, self.npose), np.array(e.g, dtype=np.float64),
                float(e.score), int(e.n_hit))


_DIM2 = _Dim(2, 3, L.Result2D, L.Eval2D, L.GridInfo2D, L.SearchHit2D, AlignResult, default_params)
_DIM3 = _Dim(3, 6, L.Result3D, L.Eval3D, L.GridInfo3D, L.SearchHit3D, AlignResult3D, default_params3d)

RESULT_DOUBLES = _DIM2.result_doubles      # 16 doubles + 4 int32
RESULT3_DOUBLES = _DIM3.result_doubles     # 51: ndt3d_result as float64 words


def _is_dev(a) -> bool:
    return hasattr(a, "data_ptr")


def _host_coords(coords):
    """The coordinate arrays of one host cloud as contiguous float32: 1-D and equally long, since the library gets
    one length for all of them."""
    a = [np.ascontiguousarray(c, dtype=np.float32) for c in coords]
    shape = a[0].shape
    for c in a:
        if c.shape != shape or len(shape) != 1:
            raise ValueError(("x and y" if len(a) == 2 else "x, y and z") + " must be 1-D arrays of equal length")
    return a


def _dev_ptrs(coords, n: int):
    """The addresses of a device cloud's coordinate tensors, each checked to hold n contiguous float32."""
    import torch
    f32 = torch.float32
    for t in coords:
        if not (t.is_cuda and t.dtype == f32 and t.is_contiguous() and t.numel() == n):
            raise ValueError("device arrays must be contiguous float32 CUDA tensors of equal length")
    return [t.data_ptr() for t in coords]


def _dev_layout(what: str, t, toff, s, soff, init, *out):
    """The addresses of a device batch - clouds, offsets, clouds, offsets, initial poses and, for a batch, the result
    rows - each tensor checked to be contiguous, on the device and of the documented dtype."""
    import torch
    f32, i64, f64 = torch.float32, torch.int64, torch.float64
    tensors = (*t, toff, *s, soff, init, *out)
    for x, dtype in zip(tensors, (*[f32] * len(t), i64, *[f32] * len(s), i64, f64, f64)):
        if not (x.is_cuda and x.dtype == dtype and x.is_contiguous()):
            raise ValueError(f"{what} tensors must be contiguous CUDA tensors of the documented dtypes")
    return [x.data_ptr() for x in tensors]


def _torch_stream():
    """torch's current stream, which device arrays handed to this module may still be written on."""
    import torch
    return torch.cuda.current_stream()


def _torch_stream_ptr():
    return C.c_void_p(_torch_stream().cuda_stream)


def _hits(hits, n: int):
    return [SearchHit(tuple(h.pose), float(h.score), int(h.index)) for h in hits[:n]]


class _Calls:
    """The C functions of one prefix under their short names, each resolved on its first use:
    _Calls(lib, "ndt2d_batch").align_dev is lib.ndt2d_batch_align_dev."""

    def __init__(self, lib, prefix: str):
        self._lib, self._prefix = lib, prefix

    def __getattr__(self, name):                # reached only while `name` is not yet an instance attribute
        fn = getattr(self._lib, f"{self._prefix}_{name}")
        setattr(self, name, fn)
        return fn


class _Handle:
    """A library handle and its life cycle.  `_prefix` names the C functions that act on it: {_prefix}_destroy frees
    it, and a negative status of {_prefix}_<what> raises NdtError("{_prefix}_<what>: ...")."""
    _prefix = None
    _h = None

    def _bind(self):
        self._lib = L.load()
        self._c = _Calls(self._lib, self._prefix)

    def _check(self, status: int, what: str) -> int:
        if status < 0:
            raise L.NdtError(status, f"{self._prefix}_{what}")
        return status

    def set_tuning(self, knob: str, value: int):
        self._check(self._c.set_tuning(self._h, L.TUNING[knob], int(value)), "set_tuning")

    def close(self):
        if self._h:
            self._c.destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _NdtMatcher(_Handle):
    """One handle = one device stream + one cached target grid.  Every method that takes a cloud takes it as the tuple
    of its coordinate arrays; NdtMatcher2D / NdtMatcher3D spell the coordinates out."""
    _dim = None
    _where_set_target_dev = None    # the NdtError text of a failed device set_target: not the same in 2D and 3D

    def _create(self, device: int, tuning: dict | None):
        self._bind()
        h = C.c_void_p()
        self._check(self._c.create(C.byref(self.params), int(device), C.byref(h)), "create")
        self._h = h
        self._device = int(device)
        self._keep = None
        for k, v in (tuning or {}).items():
            self.set_tuning(k, v)

    # ---- (i) target grid
    def _set_target(self, coords):
        if _is_dev(coords[0]):
            n = coords[0].numel()
            self._check(self._c.set_target_dev(self._h, *_dev_ptrs(coords, n), n, _torch_stream_ptr()),
                        self._where_set_target_dev)
        else:
            a = _host_coords(coords)
            self._check(self._c.set_target(self._h, *[c.ctypes.data for c in a], a[0].size), "set_target")
        return self.grid_info()

    def _target_points(self, host_fn, dev_fn, what: str, coords, pose) -> int:
        """add_target_points / remove_target_points: the same call, on its two C functions."""
        out = C.c_size_t(0)
        if _is_dev(coords[0]):
            n = coords[0].numel()
            p = self._dim.pose(pose) if pose is not None else None
            self._check(dev_fn(self._h, *_dev_ptrs(coords, n), n, p, C.byref(out), _torch_stream_ptr()), what + "_dev")
            return int(out.value)
        if pose is not None:
            raise ValueError("pose is applied on the device: pass device tensors")
        a = _host_coords(coords)
        self._check(host_fn(self._h, *[c.ctypes.data for c in a], a[0].size, C.byref(out)), what)
        return int(out.value)

    def _add_target_points(self, coords, pose) -> int:
        return self._target_points(self._c.add_target_points, self._c.add_target_points_dev, "add_target_points",
                                   coords, pose)

    def _remove_target_points(self, coords, pose) -> int:
        return self._target_points(self._c.remove_target_points, self._c.remove_target_points_dev,
                                   "remove_target_points", coords, pose)

    def grid_info(self):
        info = self._dim.GridInfo()
        self._check(self._c.get_grid_info(self._h, C.byref(info)), "get_grid_info")
        return info

    def grid(self):
        """(count int32 [cells], mean float32 [cells, 2 | 3], icov float32 [cells, 3 | 6]) of the cached grid."""
        info = self.grid_info()
        nc = info.width * info.height * getattr(info, "depth", 1)
        count = np.zeros(nc, dtype=np.int32)
        mean = np.zeros((nc, self._dim.ncoord), dtype=np.float32)
        icov = np.zeros((nc, self._dim.nsym), dtype=np.float32)
        self._check(self._c.get_grid(self._h, count.ctypes.data, mean.ctypes.data, icov.ctypes.data), "get_grid")
        return count, mean, icov

    # ---- submap persistence
    def save_map(self) -> np.ndarray:
        """The cached grid as a flat uint8 buffer (ndt_map_header + the exact per-cell sums; ndt2d/ndt3d_save_map)."""
        buf = np.empty(int(self._c.map_size(self._h)) or 1, dtype=np.uint8)
        self._check(self._c.save_map(self._h, buf.ctypes.data, buf.size, None), "save_map")
        return buf

    def load_map(self, buf):
        """Make a saved map this handle's target: the sums are re-finalised with THIS handle's min_points /
        eig_ratio (ndt2d/ndt3d_load_map); cell_size and overlap_grids must match."""
        buf = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8))
        self._check(self._c.load_map(self._h, buf.ctypes.data, buf.size), "load_map")

    def coarsen_into(self, dst) -> int:
        """Give `dst` - a matcher whose cell_size is exactly 2 or 4 times this one's - the grid whose cells are unions of
        this grid's cells (2^2 or 4^2 of them; 2^3 or 4^3 voxels in 3D), from the exact per-cell sums alone
        (ndt2d/ndt3d_coarsen_map: no points, on the device, deterministic to the bit), finalised with dst's min_points /
        eig_ratio.  Returns dst's valid-cell count."""
        self._check(self._c.coarsen_map(self._h, dst._h), "coarsen_map")
        return int(dst.grid_info().n_valid)

    def _merge(self, fn, what: str, src, pose) -> int:
        out = C.c_size_t(0)
        self._check(fn(self._h, src._h, self._dim.pose(pose), C.byref(out)), what)
        return int(out.value)

    def merge_map(self, src, pose) -> int:
        """Fold the submap of `src` - a matcher of this dimension whose cell_size is at most this one's - into this
        matcher's at `pose` (src's frame in this one's: what self.align_map(src) returns), from src's exact per-cell sums
        alone (ndt2d/ndt3d_merge_map: no points, so it works on a map that came back from load_map).  Each source cell is
        filed as a block under the cell of its mean.  Returns the number of points that fell outside this grid."""
        return self._merge(self._c.merge_map, "merge_map", src, pose)

    def unmerge_map(self, src, pose) -> int:
        """Take out again what merge_map(src, pose) put in - exactly, whatever was added or removed in between
        (ndt2d/ndt3d_unmerge_map).  Content that is not in the map is an error that leaves this matcher without a target."""
        return self._merge(self._c.unmerge_map, "unmerge_map", src, pose)

    # ---- (ii)+(iii) one evaluation
    def _evaluate(self, coords, pose):
        p = self._dim.pose(pose)
        out = self._dim.Eval()
        if _is_dev(coords[0]):
            n = coords[0].numel()
            self.wait_stream()
            self._check(self._c.evaluate_dev(self._h, *_dev_ptrs(coords, n), n, p, C.byref(out)), "evaluate_dev")
        else:
            a = _host_coords(coords)
            self._check(self._c.evaluate(self._h, *[c.ctypes.data for c in a], a[0].size, p, C.byref(out)), "evaluate")
        return self._dim.evaluation(out)

    # ---- per-point fit and selection (docs/ALGORITHM.md section 2.19)
    def _point_fit(self, fit: L.PointFit, m=None, cls=None) -> PointFit:
        return PointFit(m, cls, int(fit.n_invalid), int(fit.n_miss), int(fit.n_misfit), int(fit.n_fit), int(fit.n_selected))

    def _fit_points(self, coords, pose, max_m: float) -> PointFit:
        p = self._dim.pose(pose)
        fit = L.PointFit()
        if _is_dev(coords[0]):
            import torch
            n = coords[0].numel()
            m = torch.empty(n, dtype=torch.float32, device=coords[0].device)
            cls = torch.empty(n, dtype=torch.uint8, device=coords[0].device)
            self.wait_stream()
            self._check(self._c.fit_points_dev(self._h, *_dev_ptrs(coords, n), n, p, float(max_m), m.data_ptr(), cls.data_ptr(),
                                               C.byref(fit)), "fit_points_dev")
        else:
            a = _host_coords(coords)
            m = np.empty(a[0].size, dtype=np.float32)
            cls = np.empty(a[0].size, dtype=np.uint8)
            self._check(self._c.fit_points(self._h, *[c.ctypes.data for c in a], a[0].size, p, float(max_m), m.ctypes.data,
                                           cls.ctypes.data, C.byref(fit)), "fit_points")
        return self._point_fit(fit, m, cls)

    def _select_points(self, coords, pose, max_m: float, keep):
        """-> (coords of the kept points, their indices (int64), PointFit without m / cls): of the kind of the input."""
        import torch
        host = not _is_dev(coords[0])
        dev = self._on_device(coords)
        n = dev[0].numel()
        out = [torch.empty_like(c) for c in dev]
        index = torch.empty(n, dtype=torch.int32, device=dev[0].device)      # uint32 words, below 2^31
        fit = L.PointFit()
        self._check(self._c.select_points_dev(self._h, *_dev_ptrs(dev, n), n, self._dim.pose(pose), float(max_m),
                                              _keep_mask(keep), *[o.data_ptr() for o in out], index.data_ptr(),
                                              C.byref(fit)), "select_points_dev")
        k = int(fit.n_selected)
        out, index = tuple(o[:k] for o in out), index[:k].to(torch.int64)
        if host:
            out, index = tuple(o.cpu().numpy() for o in out), index.cpu().numpy()
        return out, index, self._point_fit(fit)

    # ---- voxel-grid scan filter (docs/ALGORITHM.md section 2.24)
    def _voxel_filter(self, coords, leaf: float, min_points: int, with_counts: bool, with_info: bool):
        """-> coords of the centroids [, counts (int64)] [, VoxelFilterInfo]: of the kind of the input, n_out long."""
        info = L.VoxelFilterInfo()
        if _is_dev(coords[0]):
            import torch
            n = coords[0].numel()
            out = [torch.empty_like(c) for c in coords]
            cnt = torch.empty(n, dtype=torch.int32, device=coords[0].device) if with_counts else None     # uint32 words, below 2^31
            self.wait_stream()
            self._check(self._c.voxel_filter_dev(self._h, *_dev_ptrs(coords, n), n, float(leaf), int(min_points),
                                                 *[o.data_ptr() for o in out], cnt.data_ptr() if with_counts else None, n,
                                                 C.byref(info)), "voxel_filter_dev")
            k = int(info.n_out)
            res = [tuple(o[:k] for o in out)]
            if with_counts:
                res.append(cnt[:k].to(torch.int64))
        else:
            a = _host_coords(coords)
            n = a[0].size
            out = [np.empty(n, dtype=np.float32) for _ in a]
            cnt = np.empty(n, dtype=np.uint32) if with_counts else None
            self._check(self._c.voxel_filter(self._h, *[c.ctypes.data for c in a], n, float(leaf), int(min_points),
                                             *[o.ctypes.data for o in out], cnt.ctypes.data if with_counts else None, n,
                                             C.byref(info)), "voxel_filter")
            k = int(info.n_out)
            res = [tuple(o[:k].copy() for o in out)]
            if with_counts:
                res.append(cnt[:k].astype(np.int64))
        self.voxel_filter_info = VoxelFilterInfo(int(info.n_invalid), int(info.n_voxels), int(info.n_out))
        if with_info:
            res.append(self.voxel_filter_info)
        return res[0] if len(res) == 1 else tuple(res)

    def wait_stream(self, stream=None):
        """Order the handle's stream behind `stream` (default: torch's current stream): device arrays
        written there are complete before the handle's next kernels read them (ndt2d/ndt3d_wait_stream)."""
        self._check(self._c.wait_stream(self._h, _torch_stream_ptr() if stream is None else C.c_void_p(int(stream))),
                    "wait_stream")

    # ---- full alignment
    def _align(self, coords, init_pose):
        p = self._dim.pose(init_pose)
        r = self._dim.Result()
        if _is_dev(coords[0]):
            n = coords[0].numel()
            self.wait_stream()           # the tensors may still be in flight on torch's current stream
            st = self._c.align_dev(self._h, *_dev_ptrs(coords, n), n, p, C.byref(r))
        else:
            a = _host_coords(coords)
            st = self._c.align(self._h, *[c.ctypes.data for c in a], a[0].size, p, C.byref(r))
        self._check(st, "align")
        return self._dim.result(r)

    def _align_trace(self, coords, init_pose, capacity: int):
        a = _host_coords(coords)
        p = self._dim.pose(init_pose)
        rows = (self._dim.Result * capacity)()
        n_rows = C.c_int32(0)
        self._check(self._c.align_trace(self._h, *[c.ctypes.data for c in a], a[0].size, p, C.cast(rows, C.c_void_p), capacity,
                                        C.byref(n_rows), None), "align_trace")
        return [self._dim.result(rows[j]) for j in range(n_rows.value)]

    def _align_multi_start(self, coords, init_poses):
        poses = self._dim.poses(init_poses)
        m, n = poses.shape[0], coords[0].numel()
        out = (self._dim.Result * m)()
        self.wait_stream()
        self._check(self._c.align_multi_start_dev(self._h, *_dev_ptrs(coords, n), n, poses.ctypes.data_as(L._dp), m,
                                                  C.cast(out, C.c_void_p)), "align_multi_start_dev")
        return [self._dim.result(r) for r in out]

    def align_multi_scan(self, scans, init_poses):
        """Up to 64 different device scans, each a tuple of its coordinate CUDA tensors, against the cached grid, each
        from its own initial pose, in one launch chain (ndt2d/ndt3d_align_multi_scan_dev).  Returns a list of
        AlignResult; scan k's equals align(scan k, pose k) bit for bit."""
        m = len(scans)
        poses = self._dim.poses(init_poses, m)
        ns = (C.c_size_t * m)(*[int(s[0].numel()) for s in scans])
        ptr = zip(*[_dev_ptrs(s[:self._dim.ncoord], s[0].numel()) for s in scans])      # per scan -> per axis
        out = (self._dim.Result * m)()
        self.wait_stream()
        self._check(self._c.align_multi_scan_dev(self._h, *[(C.c_void_p * m)(*axis) for axis in ptr], ns,
                                                 poses.ctypes.data_as(L._dp), m,
                                                 C.cast(out, C.c_void_p)), "align_multi_scan_dev")
        return [self._dim.result(r) for r in out]

    def _align_async(self, coords, init_pose, producer_complete: bool):
        p = self._dim.pose(init_pose)
        n = coords[0].numel()
        self._keep = coords
        if not producer_complete:
            self.wait_stream()
        self._check(self._c.align_dev_async(self._h, *_dev_ptrs(coords, n), n, p), "align_dev_async")

    def finish(self):
        """Wait for the alignment that align_async enqueued and fetch its AlignResult."""
        r = self._dim.Result()
        self._check(self._c.align_finish(self._h, C.byref(r)), "align_finish")
        self._keep = None
        return self._dim.result(r)

    @property
    def stream(self) -> int:
        return int(self._c.stream(self._h) or 0)

    # ---- map-to-map alignment (distribution-to-distribution NDT): no points, two cached grids
    def align_map(self, source, init_pose=None):
        """Align `source`'s cached grid to this handle's (ndt2d/ndt3d_align_map): pose maps the source map's frame into
        this map's frame (init_pose=None starts from the identity).  This handle's parameters drive the solve; `source`
        may be this handle."""
        p = self._dim.pose(init_pose) if init_pose is not None else self._dim.Pose()
        r = self._dim.Result()
        self._check(self._c.align_map(self._h, source._h, p, C.byref(r)), "align_map")
        return self._dim.result(r)

    def align_map_multi(self, sources, init_poses):
        """Up to 64 map-to-map alignments against this handle's grid in one launch chain (ndt2d/ndt3d_align_map_multi).
        sources: one matcher (a multi-start: every pose starts that matcher's map) or a sequence of matchers, one per
        pose; a matcher may repeat and may be this one.  Returns a list of AlignResult, entry k bit for bit what
        align_map(sources[k], init_poses[k]) returns."""
        poses = self._dim.poses(init_poses)
        m = poses.shape[0]
        srcs = [sources] * m if isinstance(sources, _NdtMatcher) else list(sources)
        if len(srcs) != m:
            raise ValueError(f"{len(srcs)} sources for {m} initial poses")
        hs = (C.c_void_p * max(m, 1))(*[s._h.value for s in srcs])
        out = (self._dim.Result * max(m, 1))()
        self._check(self._c.align_map_multi(self._h, hs, poses.ctypes.data, m, C.cast(out, C.c_void_p)), "align_map_multi")
        return [self._dim.result(r) for r in out[:m]]

    def evaluate_map(self, source, pose):
        """(H, g, score, n_hit) of the map-to-map objective at `pose` (ndt2d/ndt3d_evaluate_map)."""
        out = self._dim.Eval()
        self._check(self._c.evaluate_map(self._h, source._h, self._dim.pose(pose), C.byref(out)), "evaluate_map")
        return self._dim.evaluation(out)

    def components(self):
        """(key int32 [n], mean float32 [n, 2 | 3], cov float32 [n, 3 | 6] = (xx xy yy) | (xx xy xz yy yz zz)) of the
        cached grid's valid cells, in cell-key order: what this handle contributes as the source of align_map
        (ndt2d/ndt3d_get_components)."""
        n = C.c_int32(0)
        self._check(self._c.get_components(self._h, None, None, None, 0, C.byref(n)), "get_components")
        key = np.zeros(n.value, dtype=np.int32)
        mean = np.zeros((n.value, self._dim.ncoord), dtype=np.float32)
        cov = np.zeros((n.value, self._dim.nsym), dtype=np.float32)
        if n.value:
            self._check(self._c.get_components(self._h, mean.ctypes.data, cov.ctypes.data, key.ctypes.data, n.value,
                                               C.byref(n)), "get_components")
        return key, mean, cov

    # ---- exhaustive pose search over an (x, y, theta | yaw) window (ndt2d/ndt3d_search_*; search.py restates it)
    def _hit_rows(self, k: int):
        return (self._dim.SearchHit * max(int(k), 1))()

    def _lattice_dims(self, w):
        dims = (C.c_int32 * 3)()
        self._check(self._c.search_lattice_size(C.byref(w), C.cast(dims, C.c_void_p)), "search_lattice_size")
        return tuple(dims)

    def _on_device(self, coords):
        """The cloud as CUDA tensors on the handle's device (numpy arrays are uploaded), after wait_stream."""
        if not _is_dev(coords[0]):
            import torch
            coords = tuple(torch.from_numpy(a).to(f"cuda:{self._device}") for a in _host_coords(coords))
        self.wait_stream()
        return coords

    def _search(self, coords, center, half_extent, step, k, min_sep):
        w = self._window(center, half_extent, step, min_sep)
        hits = self._hit_rows(k)
        nh = C.c_int32(0)
        if _is_dev(coords[0]):
            n = coords[0].numel()
            self.wait_stream()
            st = self._c.search_dev(self._h, *_dev_ptrs(coords, n), n, C.byref(w), int(k), C.cast(hits, C.c_void_p),
                                    C.byref(nh))
        else:
            a = _host_coords(coords)
            st = self._c.search(self._h, *[c.ctypes.data for c in a], a[0].size, C.byref(w), int(k), C.cast(hits, C.c_void_p),
                                C.byref(nh))
        self._check(st, "search")
        return _hits(hits, nh.value)

    def _search_scores(self, coords, center, half_extent, step):
        import torch
        w = self._window(center, half_extent, step)
        dims = self._lattice_dims(w)
        coords = self._on_device(coords)
        out = torch.empty(dims, dtype=torch.float32, device=coords[0].device)
        n = coords[0].numel()
        self._check(self._c.search_scores_dev(self._h, *_dev_ptrs(coords, n), n, C.byref(w), out.data_ptr()),
                    "search_scores_dev")
        return out

    def _search_align(self, coords, center, half_extent, step, k, min_sep):
        w = self._window(center, half_extent, step, min_sep)
        hits, res = self._hit_rows(k), (self._dim.Result * max(int(k), 1))()
        nh = C.c_int32(0)
        coords = self._on_device(coords)
        n = coords[0].numel()
        self._check(self._c.search_align_dev(self._h, *_dev_ptrs(coords, n), n, C.byref(w), int(k),
                                             C.cast(hits, C.c_void_p), C.cast(res, C.c_void_p), C.byref(nh)),
                    "search_align_dev")
        return list(zip(_hits(hits, nh.value), [self._dim.result(r) for r in res[:nh.value]]))

    # ---- the score at a list of poses (ndt2d/ndt3d_score_poses*, _best_poses*; search.select_best restates the hits)
    def _pose_list(self, poses, device):
        """The list as a contiguous float64 CUDA tensor [m, 3 | 6] on `device` (a numpy list is uploaded)."""
        import torch
        if not _is_dev(poses):
            poses = torch.from_numpy(self._dim.poses(poses)).to(device)
        if not (poses.is_cuda and poses.dtype == torch.float64 and poses.is_contiguous() and poses.dim() == 2
                and poses.shape[1] == self._dim.npose):
            raise ValueError(f"poses must be a contiguous float64 CUDA tensor [m, {self._dim.npose}]")
        return poses

    def _score_poses(self, coords, poses):
        if _is_dev(coords[0]) != _is_dev(poses):
            raise ValueError("the scan and the poses must both be CUDA tensors or both be host arrays")
        if _is_dev(poses):
            import torch
            poses = self._pose_list(poses, coords[0].device)
            n, m = coords[0].numel(), poses.shape[0]
            out = torch.empty(m, dtype=torch.float32, device=poses.device)
            self.wait_stream()
            self._check(self._c.score_poses_dev(self._h, *_dev_ptrs(coords, n), n, poses.data_ptr(), m, out.data_ptr()),
                        "score_poses_dev")
            return out
        a, p = _host_coords(coords), self._dim.poses(poses)
        out = np.empty(p.shape[0], dtype=np.float32)
        self._check(self._c.score_poses(self._h, *[c.ctypes.data for c in a], a[0].size, p.ctypes.data, p.shape[0],
                                        out.ctypes.data), "score_poses")
        return out

    def _score_particles(self, coords, poses, with_hits: bool, sync: bool):
        """score_particles() of both matchers (ndt2d/ndt3d_score_particles*): a team of lanes per pose, the hit counts,
        and with sync=False the asynchronous call with torch's current stream ordered behind the handle's."""
        if _is_dev(coords[0]) != _is_dev(poses):
            raise ValueError("the scan and the poses must both be CUDA tensors or both be host arrays")
        if _is_dev(poses):
            import torch
            poses = self._pose_list(poses, coords[0].device)
            n, m = coords[0].numel(), poses.shape[0]
            out = torch.empty(m, dtype=torch.float32, device=poses.device)
            cnt = torch.empty(m, dtype=torch.int32, device=poses.device) if with_hits else None
            args = (self._h, *_dev_ptrs(coords, n), n, poses.data_ptr(), m, out.data_ptr(), cnt.data_ptr() if with_hits else None)
            self.wait_stream()
            if sync:
                self._check(self._c.score_particles_dev(*args), "score_particles_dev")
            else:
                self._check(self._c.score_particles_async(*args), "score_particles_async")
                # torch's current stream behind the handle's: the outputs can be consumed there in order, and the caching
                # allocator does not hand the scan, the list or the outputs out again before the launch has read them
                _torch_stream().wait_stream(torch.cuda.ExternalStream(self.stream))
            return (out, cnt.view(torch.uint32)) if with_hits else out
        if not sync:
            raise ValueError("sync=False takes CUDA tensors: host arrays are staged and fetched by a synchronous call")
        a, p = _host_coords(coords), self._dim.poses(poses)
        out = np.empty(p.shape[0], dtype=np.float32)
        cnt = np.empty(p.shape[0], dtype=np.uint32) if with_hits else None
        self._check(self._c.score_particles(self._h, *[c.ctypes.data for c in a], a[0].size, p.ctypes.data, p.shape[0],
                                            out.ctypes.data, cnt.ctypes.data if with_hits else None), "score_particles")
        return (out, cnt) if with_hits else out

    def _best_poses(self, coords, poses, k, min_sep, align: bool):
        coords = self._on_device(coords)
        poses = self._pose_list(poses, coords[0].device)
        self.wait_stream()
        n, m = coords[0].numel(), poses.shape[0]
        hits, nh = self._hit_rows(k), C.c_int32(0)
        args = (self._h, *_dev_ptrs(coords, n), n, poses.data_ptr(), m, float(min_sep[0]), float(min_sep[1]), int(k),
                C.cast(hits, C.c_void_p))
        if not align:
            self._check(self._c.best_poses_dev(*args, C.byref(nh)), "best_poses_dev")
            return _hits(hits, nh.value)
        res = (self._dim.Result * max(int(k), 1))()
        self._check(self._c.best_poses_align_dev(*args, C.cast(res, C.c_void_p), C.byref(nh)), "best_poses_align_dev")
        return list(zip(_hits(hits, nh.value), [self._dim.result(r) for r in res[:nh.value]]))

    # ---- the same search for map-to-map alignment: `source`'s component list instead of a scan
    def search_map(self, source, center, half_extent, step, k: int = 8, min_sep=(0.5, 0.1)):
        """The best k (1..64) well-separated peaks of the map-to-map score (evaluate_map's) over the lattice of the
        window (ndt2d/ndt3d_search_map; in 3D the (x, y, yaw) lattice, z, roll and pitch pinned to the centre's): a list
        of SearchHit, best first.  Neither handle needs a point."""
        w = self._window(center, half_extent, step, min_sep)
        hits = self._hit_rows(k)
        nh = C.c_int32(0)
        self._check(self._c.search_map(self._h, source._h, C.byref(w), int(k), C.cast(hits, C.c_void_p), C.byref(nh)),
                    "search_map")
        return _hits(hits, nh.value)

    def search_map_scores(self, source, center, half_extent, step):
        """The map-to-map score volume of the window's lattice (ndt2d/ndt3d_search_map_scores): a float32 CUDA tensor
        [n_theta | n_yaw, n_y, n_x]."""
        import torch
        w = self._window(center, half_extent, step)
        out = torch.empty(self._lattice_dims(w), dtype=torch.float32, device=f"cuda:{self._device}")
        self._check(self._c.search_map_scores(self._h, source._h, C.byref(w), out.data_ptr()), "search_map_scores")
        return out

    def search_align_map(self, source, center, half_extent, step, k: int = 8, min_sep=(0.5, 0.1)):
        """search_map(), then align_map() from every hit's pose (ndt2d/ndt3d_search_align_map): a list of
        (SearchHit, AlignResult), best lattice score first."""
        w = self._window(center, half_extent, step, min_sep)
        hits, res = self._hit_rows(k), (self._dim.Result * max(int(k), 1))()
        nh = C.c_int32(0)
        self._check(self._c.search_align_map(self._h, source._h, C.byref(w), int(k), C.cast(hits, C.c_void_p),
                                             C.cast(res, C.c_void_p), C.byref(nh)), "search_align_map")
        return list(zip(_hits(hits, nh.value), [self._dim.result(r) for r in res[:nh.value]]))

    # ---- the map-to-map score at a list of poses (ndt2d/ndt3d_score_map_poses*, _best_map_poses*)
    def score_map_poses(self, source, poses, with_hits: bool = False):
        """evaluate_map(source, pose)'s score at every pose of a list [m, 3 | 6] in one launch
        (ndt2d/ndt3d_score_map_poses*): a CUDA float64 list gives a CUDA float32 tensor [m], a host list a numpy array.
        with_hits=True: (scores, n_hit), n_hit the uint32 counts of components that fell in a valid target cell
        (evaluate_map's n_hit).  A non-finite pose scores 0 with count 0.  In 3D every coordinate is free - z, roll and
        pitch too, which search_map pins."""
        if _is_dev(poses):
            import torch
            poses = self._pose_list(poses, poses.device)
            m = poses.shape[0]
            out = torch.empty(m, dtype=torch.float32, device=poses.device)
            cnt = torch.empty(m, dtype=torch.int32, device=poses.device) if with_hits else None
            self.wait_stream()
            self._check(self._c.score_map_poses_dev(self._h, source._h, poses.data_ptr(), m, out.data_ptr(),
                                                    cnt.data_ptr() if with_hits else None), "score_map_poses_dev")
            return (out, cnt.view(torch.uint32)) if with_hits else out
        p = self._dim.poses(poses)
        out = np.empty(p.shape[0], dtype=np.float32)
        cnt = np.empty(p.shape[0], dtype=np.uint32) if with_hits else None
        self._check(self._c.score_map_poses(self._h, source._h, p.ctypes.data, p.shape[0], out.ctypes.data,
                                            cnt.ctypes.data if with_hits else None), "score_map_poses")
        return (out, cnt) if with_hits else out

    def _best_map_poses(self, source, poses, k, min_sep, align: bool):
        poses = self._pose_list(poses, f"cuda:{self._device}")
        self.wait_stream()
        hits, nh = self._hit_rows(k), C.c_int32(0)
        args = (self._h, source._h, poses.data_ptr(), poses.shape[0], float(min_sep[0]), float(min_sep[1]), int(k),
                C.cast(hits, C.c_void_p))
        if not align:
            self._check(self._c.best_map_poses_dev(*args, C.byref(nh)), "best_map_poses_dev")
            return _hits(hits, nh.value)
        res = (self._dim.Result * max(int(k), 1))()
        self._check(self._c.best_map_poses_align_dev(*args, C.cast(res, C.c_void_p), C.byref(nh)), "best_map_poses_align_dev")
        return list(zip(_hits(hits, nh.value), [self._dim.result(r) for r in res[:nh.value]]))

    def best_map_poses(self, source, poses, k: int = 8, min_sep=(0.5, 0.1)):
        """The best k (1..64) poses of the list by score_map_poses' score that lie min_sep = (translation, rotation)
        apart (ndt2d/ndt3d_best_map_poses_dev; search.select_best restates the rule): a list of SearchHit, best first;
        hit.index is the position in the list, hit.pose the list's row as it stands there."""
        return self._best_map_poses(source, poses, k, min_sep, False)

    def best_map_poses_align(self, source, poses, k: int = 8, min_sep=(0.5, 0.1)):
        """best_map_poses(), then align_map() from every hit's pose in one launch chain
        (ndt2d/ndt3d_best_map_poses_align_dev): a list of (SearchHit, AlignResult), best list score first; result q is
        bit for bit align_map(source, hit q's pose)."""
        return self._best_map_poses(source, poses, k, min_sep, True)


class NdtMatcher2D(_NdtMatcher):
    """One handle = one device stream + one cached target grid (ndt2d_* of include/ndt_hip.h)."""
    _prefix = "ndt2d"
    _dim = _DIM2
    _where_set_target_dev = "set_target"

    def __init__(self, device: int = 0, params: L.Params2D | None = None, tuning: dict | None = None, **overrides):
        """tuning: execution-strategy knobs by name (L.TUNING), e.g. {"short_scan_kernel": 0}."""
        self.params = _params_2d(params, overrides)
        self._create(device, tuning)

    def set_target(self, x, y):
        return self._set_target((x, y))

    def reserve_target(self, xmin: float, ymin: float, xmax: float, ymax: float):
        """Empty grid over a chosen extent; fill it with add_target_points()."""
        self._check(self._c.reserve_target(self._h, float(xmin), float(ymin), float(xmax), float(ymax)), "reserve_target")
        return self.grid_info()

    def add_target_points(self, x, y, pose=None) -> int:
        """Merge more points into the cached grid; returns how many fell outside its extent.
        Device tensors may carry a pose (tx, ty, theta) that moves them into the map frame first."""
        return self._add_target_points((x, y), pose)

    def remove_target_points(self, x, y, pose=None) -> int:
        """Take points out of the cached grid again - the exact inverse of add_target_points() for points (and a pose)
        that were added before; returns how many fell outside its extent.  Points that are not in the map raise
        NdtError (NDT_ERR_INVALID_ARG) and leave the matcher without a target."""
        return self._remove_target_points((x, y), pose)

    def evaluate(self, sx, sy, pose):
        return self._evaluate((sx, sy), pose)

    def fit_points(self, sx, sy, pose, max_m: float) -> PointFit:
        """Score every point of the scan against the cached grid at `pose` (ndt2d_fit_points*): m = q' Sigma^-1 q in
        its cell and a class byte per point (L.POINT_CLASS: fit = a valid cell and m <= max_m), of the kind of the
        input - numpy arrays or CUDA tensors - and the four class counts."""
        return self._fit_points((sx, sy), pose, max_m)

    def voxel_filter(self, x, y, leaf: float, min_points: int = 1, with_counts: bool = False, with_info: bool = False):
        """Downsample a cloud to the centroid of every occupied voxel of the absolute lattice floor(x / leaf)
        (ndt2d_voxel_filter*; docs/ALGORITHM.md section 2.24): (x, y) of the kind of the input - CUDA tensors or numpy
        arrays - in ascending lattice order (iy, ix), the same bits for every order of the input.  Voxels with fewer
        than min_points points are dropped.  with_counts: also the points per emitted voxel; with_info: also the
        VoxelFilterInfo, which is kept as self.voxel_filter_info either way.  Needs no target."""
        return self._voxel_filter((x, y), leaf, min_points, with_counts, with_info)

    def select_points(self, sx, sy, pose, max_m: float, keep=("fit", "miss")):
        """The points of the scan whose class at `pose` is in `keep` (class names, or a mask of 1 << class), in the
        source frame, bit for bit and in their order (ndt2d_select_points_dev): ((x, y), index, PointFit), trimmed to
        n_selected - what add_target_points(x, y, pose) and remove_target_points take.  The default keeps what fits
        the map and what extends it, and drops what lies in a mapped cell but off its Gaussian."""
        return self._select_points((sx, sy), pose, max_m, keep)

    def align(self, sx, sy, init_pose=(0.0, 0.0, 0.0)) -> AlignResult:
        return self._align((sx, sy), init_pose)

    def align_trace(self, sx, sy, init_pose=(0.0, 0.0, 0.0), capacity: int = 256):
        """Per-iteration trace (ndt2d_align_trace; host arrays): a list of AlignResult, entry j = the state
        after j + 1 updates (H, g, score, n_hit of the evaluation behind that update)."""
        return self._align_trace((sx, sy), init_pose, capacity)

    def align_multi_start(self, sx, sy, init_poses):
        """Up to 64 alignments of the same device scan from different initial poses in one launch chain
        (ndt2d_align_multi_start_dev).  Returns a list of AlignResult, one per start."""
        return self._align_multi_start((sx, sy), init_poses)

    def align_async(self, sx, sy, init_pose=(0.0, 0.0, 0.0), producer_complete: bool = False):
        """Enqueue the whole loop on the handle's stream (device tensors only); finish() waits and fetches.
        producer_complete=True: the caller knows the tensors are complete (their stream was synchronised), no
        ordering needed."""
        self._align_async((sx, sy), init_pose, producer_complete)

    @staticmethod
    def _window(center, half_extent, step, min_sep=(0.0, 0.0)) -> L.SearchWindow2D:
        w = L.SearchWindow2D()
        for a in range(3):
            w.center[a], w.half_extent[a], w.step[a] = float(center[a]), float(half_extent[a]), float(step[a])
        w.min_sep_trans, w.min_sep_rot = float(min_sep[0]), float(min_sep[1])
        return w

    def search(self, sx, sy, center, half_extent, step, k: int = 8, min_sep=(0.5, 0.1)):
        """The best k (1..64) well-separated peaks of the NDT score over the (x, y, theta) lattice of the window
        (ndt2d_search / ndt2d_search_dev): a list of SearchHit, best first."""
        return self._search((sx, sy), center, half_extent, step, k, min_sep)

    def search_scores(self, sx, sy, center, half_extent, step):
        """The score volume of the window's lattice (ndt2d_search_scores_dev): a float32 CUDA tensor [n_theta, n_y, n_x]."""
        return self._search_scores((sx, sy), center, half_extent, step)

    def search_align(self, sx, sy, center, half_extent, step, k: int = 8, min_sep=(0.5, 0.1)):
        """search(), then align_multi_start() from the hits' poses (ndt2d_search_align_dev): a list of
        (SearchHit, AlignResult), best lattice score first."""
        return self._search_align((sx, sy), center, half_extent, step, k, min_sep)

    def score_poses(self, sx, sy, poses):
        """The NDT score of the scan at every pose of a list [m, 3] of (x, y, theta), in one launch
        (ndt2d_score_poses*): the weights of a particle filter's particles.  CUDA tensors (float32 scan, float64
        poses) return a float32 CUDA tensor [m]; numpy arrays return a numpy array through the host form; the scan and
        the poses must be of the same kind (ValueError otherwise: the result's kind would be a guess).  A pose with a
        non-finite coordinate scores 0."""
        return self._score_poses((sx, sy), poses)

    def score_particles(self, sx, sy, poses, with_hits: bool = False, sync: bool = True):
        """score_poses() for SHORT lists - a particle filter's few hundred to few thousand particles - with a team of 64
        or 256 lanes per pose instead of one lane (ndt2d_score_particles*; tuning knob "particle_team").  It was the faster
        call at every list size measured, 256 to 1 048 576 poses (4096 particles: 4x in 2D, 17x in 3D): no
        size was found from which score_poses is faster, which remains for the search volume's bits.  The scores differ from score_poses' only by the
        order of the float32 sum (docs/ALGORITHM.md), and depend on nothing but the grid, the scan and the pose.  Inputs as
        score_poses.  with_hits=True: (scores, n_hit), n_hit the uint32 counts of lookups that hit a valid cell -
        evaluate()'s n_hit at that pose.  sync=False (CUDA tensors only) returns after the enqueue, with torch's current
        stream ordered behind the handle's: the result is consumed in torch order, with no host synchronisation."""
        return self._score_particles((sx, sy), poses, with_hits, sync)

    def best_poses(self, sx, sy, poses, k: int = 8, min_sep=(0.5, 0.1)):
        """The best k (1..64) well-separated poses of the list by score (ndt2d_best_poses_dev; search.select_best
        restates the rule): a list of SearchHit, best first, whose index is the pose's position in the list.  The hits
        are host objects either way, so the scan and the poses may each be numpy arrays or CUDA tensors: what is on the
        host is uploaded."""
        return self._best_poses((sx, sy), poses, k, min_sep, False)

    def best_poses_align(self, sx, sy, poses, k: int = 8, min_sep=(0.5, 0.1)):
        """best_poses(), then align_multi_start() from the hits' poses (ndt2d_best_poses_align_dev): a list of
        (SearchHit, AlignResult), best list score first.  Inputs as best_poses."""
        return self._best_poses((sx, sy), poses, k, min_sep, True)


class NdtMatcher3D(_NdtMatcher):
    """3D SE(3) variant (BASELINE config 5); mirrors ndt3d_* of include/ndt_hip.h."""
    _prefix = "ndt3d"
    _dim = _DIM3
    _where_set_target_dev = "set_target_dev"

    def __init__(self, device: int = 0, tuning: dict | None = None, neighbourhood: int = 1, map_neighbourhood: int = 1,
                 **overrides):
        """tuning: execution-strategy knobs by name (L.TUNING; 3D handles know "single_sync_build",
        "map_multi_from" and "fused_begin").  neighbourhood: set_neighbourhood() of the new handle; map_neighbourhood:
        its set_map_neighbourhood()."""
        self.params = default_params3d(**overrides)
        self._create(device, tuning)
        if neighbourhood != 1:
            self.set_neighbourhood(neighbourhood)
        if map_neighbourhood != 1:
            self.set_map_neighbourhood(map_neighbourhood)

    def set_neighbourhood(self, n: int):
        """1: a point is scored against the voxel its image lies in; 7: and against that voxel's six face neighbours
        (ndt3d_set_neighbourhood).  Honoured by evaluate, align*, align_trace, align_multi_start and align_multi_scan;
        the searches, pose lists, particle scores and per-point fits raise NdtError while 7 is set."""
        self._check(self._c.set_neighbourhood(self._h, int(n)), "set_neighbourhood")

    @property
    def neighbourhood(self) -> int:
        return self._check(self._c.neighbourhood(self._h), "neighbourhood")

    def set_map_neighbourhood(self, n: int):
        """Map-to-map alignment with this matcher as the TARGET (ndt3d_set_map_neighbourhood).  1: a source component
        is scored against the voxel the image of its mean falls into; 7: and against that voxel's six face neighbours,
        which takes the pull towards the identity out of two maps on one lattice.  Honoured by evaluate_map, align_map and
        align_map_multi; search_map, search_align_map, score_map_poses, best_map_poses and best_map_poses_align raise
        NdtError while 7 is set: search with 1, refine with 7.  A source's own setting is ignored."""
        self._check(self._c.set_map_neighbourhood(self._h, int(n)), "set_map_neighbourhood")

    @property
    def map_neighbourhood(self) -> int:
        return self._check(self._c.map_neighbourhood(self._h), "map_neighbourhood")

    def set_target(self, x, y, z):
        return self._set_target((x, y, z))

    def reserve_target(self, lo, hi):
        """Empty voxel grid over the box lo .. hi (x, y, z); fill it with add_target_points()."""
        a = (C.c_double * 3)(*[float(v) for v in lo])
        b = (C.c_double * 3)(*[float(v) for v in hi])
        self._check(self._c.reserve_target(self._h, a, b), "reserve_target")
        return self.grid_info()

    def add_target_points(self, x, y, z, pose=None) -> int:
        """Merge more points into the cached voxel grid; returns how many fell outside its extent.
        Device tensors may carry a pose (tx, ty, tz, roll, pitch, yaw) that moves them into the map frame first."""
        return self._add_target_points((x, y, z), pose)

    def remove_target_points(self, x, y, z, pose=None) -> int:
        """The exact inverse of add_target_points(), as NdtMatcher2D.remove_target_points."""
        return self._remove_target_points((x, y, z), pose)

    def evaluate(self, sx, sy, sz, pose):
        return self._evaluate((sx, sy, sz), pose)

    def fit_points(self, sx, sy, sz, pose, max_m: float) -> PointFit:
        """Per-point m and class against the cached voxel grid (ndt3d_fit_points*), as NdtMatcher2D.fit_points."""
        return self._fit_points((sx, sy, sz), pose, max_m)

    def voxel_filter(self, x, y, z, leaf: float, min_points: int = 1, with_counts: bool = False, with_info: bool = False):
        """(x, y, z) centroids of the occupied voxels in order (iz, iy, ix) (ndt3d_voxel_filter*), as
        NdtMatcher2D.voxel_filter."""
        return self._voxel_filter((x, y, z), leaf, min_points, with_counts, with_info)

    def select_points(self, sx, sy, sz, pose, max_m: float, keep=("fit", "miss")):
        """((x, y, z), index, PointFit) of the points whose class is in `keep` (ndt3d_select_points_dev), as
        NdtMatcher2D.select_points."""
        return self._select_points((sx, sy, sz), pose, max_m, keep)

    def align(self, sx, sy, sz, init_pose=(0.0,) * 6) -> AlignResult3D:
        return self._align((sx, sy, sz), init_pose)

    def align_trace(self, sx, sy, sz, init_pose=(0.0,) * 6, capacity: int = 256):
        """Per-iteration trace (ndt3d_align_trace; host arrays), as NdtMatcher2D.align_trace."""
        return self._align_trace((sx, sy, sz), init_pose, capacity)

    def align_multi_start(self, sx, sy, sz, init_poses):
        """Up to 64 alignments of one device scan from different initial poses in one launch chain."""
        return self._align_multi_start((sx, sy, sz), init_poses)

    def align_async(self, sx, sy, sz, init_pose=(0.0,) * 6, producer_complete: bool = False):
        """Enqueue the loop on the handle's stream (device tensors only); finish() waits and fetches."""
        self._align_async((sx, sy, sz), init_pose, producer_complete)

    @staticmethod
    def _window(center, half_extent, step, min_sep=(0.0, 0.0)) -> L.SearchWindow3D:
        if len(center) != 6:
            raise ValueError("center is a pose (tx, ty, tz, roll, pitch, yaw); x, y and yaw are searched")
        w = L.SearchWindow3D()
        for a in range(6):
            w.center[a] = float(center[a])
        for a in range(3):
            w.half_extent[a], w.step[a] = float(half_extent[a]), float(step[a])
        w.min_sep_trans, w.min_sep_rot = float(min_sep[0]), float(min_sep[1])
        return w

    def search(self, sx, sy, sz, center, half_extent, step, k: int = 8, min_sep=(0.5, 0.1)):
        """The best k (1..64) well-separated peaks of the NDT score over the (x, y, yaw) lattice of the window, with
        z, roll and pitch pinned to the centre's (ndt3d_search / ndt3d_search_dev): a list of SearchHit whose poses
        are 6-vectors, best first."""
        return self._search((sx, sy, sz), center, half_extent, step, k, min_sep)

    def search_scores(self, sx, sy, sz, center, half_extent, step):
        """The score volume of the window's lattice (ndt3d_search_scores_dev): a float32 CUDA tensor [n_yaw, n_y, n_x]."""
        return self._search_scores((sx, sy, sz), center, half_extent, step)

    def search_align(self, sx, sy, sz, center, half_extent, step, k: int = 8, min_sep=(0.5, 0.1)):
        """search(), then align_multi_start() from the hits' poses (ndt3d_search_align_dev): a list of
        (SearchHit, AlignResult3D), best lattice score first."""
        return self._search_align((sx, sy, sz), center, half_extent, step, k, min_sep)

    def score_poses(self, sx, sy, sz, poses):
        """The NDT score of the scan at every pose of a list [m, 6] of (tx, ty, tz, roll, pitch, yaw), in one launch
        (ndt3d_score_poses*), as NdtMatcher2D.score_poses: all six coordinates are free, so the list covers what the
        lattice search pins."""
        return self._score_poses((sx, sy, sz), poses)

    def score_particles(self, sx, sy, sz, poses, with_hits: bool = False, sync: bool = True):
        """score_poses() for short lists, a team of lanes per pose, with hit counts and an asynchronous form
        (ndt3d_score_particles*), as NdtMatcher2D.score_particles: the faster call at every list size measured."""
        return self._score_particles((sx, sy, sz), poses, with_hits, sync)

    def best_poses(self, sx, sy, sz, poses, k: int = 8, min_sep=(0.5, 0.1)):
        """The best k (1..64) well-separated poses of the list (ndt3d_best_poses_dev): translation distance over
        (x, y, z), rotation distance the largest wrapped difference of roll, pitch and yaw.  Inputs as
        NdtMatcher2D.best_poses: host arrays are uploaded, where score_poses wants both of one kind."""
        return self._best_poses((sx, sy, sz), poses, k, min_sep, False)

    def best_poses_align(self, sx, sy, sz, poses, k: int = 8, min_sep=(0.5, 0.1)):
        """best_poses(), then align_multi_start() from the hits' poses (ndt3d_best_poses_align_dev): a list of
        (SearchHit, AlignResult3D)."""
        return self._best_poses((sx, sy, sz), poses, k, min_sep, True)


def pyramid_params(fine: L.Params2D | None = None, **overrides):
    """The library's standard 3-level coarse-to-fine schedule (ndt2d_default_pyramid) as a
    ctypes array of ndt2d_params, for NdtBatch2D(levels=...) / NdtMulti2D(levels=...)."""
    lib = L.load()
    fine = fine if fine is not None else default_params(**overrides)
    levels = (L.Params2D * 3)()
    L.check(lib.ndt2d_default_pyramid(C.byref(fine), levels), "ndt2d_default_pyramid")
    return levels


def _as_levels(levels):
    if isinstance(levels, C.Array):
        return levels, len(levels)
    arr = (L.Params2D * len(levels))(*levels)
    return arr, len(levels)


def _concat_pairs(ncoord: int, clouds):
    """Clouds (tuples of coordinate arrays) end to end: the concatenated coordinate arrays and the offsets [n + 1]."""
    off = np.zeros(len(clouds) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c[0]) for c in clouds])
    per_cloud = [_host_coords(c[:ncoord]) for c in clouds]
    return [np.concatenate([a[k] for a in per_cloud]) for k in range(ncoord)], off


def multi_plan(n_shards: int, toff, soff, iterations_hint: int = 0, pair_iterations=None) -> np.ndarray:
    """The pair split ndt2d_multi_align uses (ndt2d_multi_plan; needs no device).  pair_iterations: optional per-pair
    iteration hints (ndt2d_multi_plan_hinted) for converged-mode batches."""
    lib = L.load()
    toff = np.ascontiguousarray(toff, dtype=np.uint64)
    soff = np.ascontiguousarray(soff, dtype=np.uint64)
    begin = np.zeros(int(n_shards) + 1, dtype=np.uint64)
    if pair_iterations is None:
        L.check(lib.ndt2d_multi_plan(int(n_shards), toff.ctypes.data, soff.ctypes.data, len(toff) - 1,
                                     int(iterations_hint), begin.ctypes.data), "ndt2d_multi_plan")
    else:
        hints = np.ascontiguousarray(pair_iterations, dtype=np.int32)
        if hints.shape != (len(toff) - 1,):
            raise ValueError("pair_iterations needs one entry per pair")
        L.check(lib.ndt2d_multi_plan_hinted(int(n_shards), toff.ctypes.data, soff.ctypes.data, len(toff) - 1,
                                            int(iterations_hint), hints.ctypes.data, begin.ctypes.data), "ndt2d_multi_plan_hinted")
    return begin


class _Context(_Handle):
    """What a batch and a multi-device handle share: creation with one level or a coarse-to-fine list of them, and the
    host-array align."""
    _dim = None

    def _create(self, levels, *where):
        """{_prefix}_create, or _create_pyramid with `levels` (the last level's parameters become self.params);
        `where` = the device, or the device list and its length."""
        self._bind()
        h = C.c_void_p()
        if levels is not None:
            self._levels, nl = _as_levels(levels)
            self.params = self._levels[nl - 1]
            self._check(self._c.create_pyramid(self._levels, nl, *where, C.byref(h)), "create_pyramid")
        else:
            self._check(self._c.create(C.byref(self.params), *where, C.byref(h)), "create")
        self._h = h

    def align(self, targets, sources, inits):
        """targets / sources: lists of (x, y) or (x, y, z) numpy tuples; inits: [n][3 | 6].  Returns a list of
        AlignResult in pair order.  A batch re-runs pairs over the on-chip capacity through the general path."""
        n, dim = len(targets), self._dim
        t, toff = _concat_pairs(dim.ncoord, targets)
        s, soff = _concat_pairs(dim.ncoord, sources)
        init = dim.poses(inits, n)
        out = np.zeros(n * dim.result_doubles, dtype=np.float64)
        self._check(self._c.align(self._h, *[c.ctypes.data for c in t], toff.ctypes.data, *[c.ctypes.data for c in s], soff.ctypes.data,
                                  init.ctypes.data, n, out.ctypes.data), "align")
        return dim.results(out, n)


class _NdtBatch(_Context):
    """Loop-closure candidate batch: independent scan pairs aligned concurrently on one GPU (one persistent workgroup
    per CU, the pair's target grid resident in LDS)."""

    def _create_batch(self, device: int, levels, **tuning):
        self._create(levels, int(device))
        self._keep = None
        for knob, value in tuning.items():
            if value is not None:
                self.set_tuning(knob, value)

    @property
    def stream(self) -> int:
        return int(self._c.stream(self._h) or 0)

    def _align_dev(self, t, toff, s, soff, init, out, stream):
        import torch
        n = int(toff.numel()) - 1
        if out is None:
            out = torch.empty((n, self._dim.result_doubles), dtype=torch.float64, device=t[0].device)
        *ptr, out_ptr = _dev_layout("batch", t, toff, s, soff, init, out)
        self._keep = (t, toff, s, soff, init, out)
        if not stream:
            # the context's own stream: order it behind torch's current stream, which may still be
            # writing the clouds
            self._check(self._c.wait_stream(self._h, _torch_stream_ptr()), "wait_stream")
        self._check(self._c.align_dev(self._h, *ptr, n, out_ptr, C.c_void_p(stream if stream is not None else 0)),
                    "align_dev")
        if not stream:
            # ... and torch's current stream behind the context's: `out` can be consumed there in order
            _torch_stream().wait_stream(torch.cuda.ExternalStream(self.stream))
        return out

    @classmethod
    def decode(cls, out_tensor):
        """float64 [n, 18 | 51] device/host tensor -> list of AlignResult (synchronises)."""
        a = out_tensor.detach().cpu().numpy()
        return cls._dim.results(a.reshape(-1), a.shape[0])


class NdtBatch2D(_NdtBatch):
    """The 2D batch; mirrors ndt2d_batch_* of include/ndt_hip.h."""
    _prefix = "ndt2d_batch"
    _dim = _DIM2

    def __init__(self, device: int = 0, params: L.Params2D | None = None, levels=None, small_variant: bool = True,
                 global_workgroups: int | None = None, **overrides):
        """levels: coarse-to-fine list of Params2D (e.g. pyramid_params()); otherwise one level.
        small_variant=False: every pair on the 1024-thread kernel (ndt2d_batch_set_tuning).
        global_workgroups: workgroups (and 3.7 MB table slabs) of the global-table variant, 1..256 (default 256)."""
        self.params = _params_2d(params, overrides)
        self._create_batch(device, levels, batch_small_variant=None if small_variant else 0,
                           batch_global_workgroups=global_workgroups)

    @property
    def last_large_count(self) -> int:
        """Pairs of the last align() call that needed the 1024-thread kernel variant (diagnostic)."""
        return int(self._c.last_large_count(self._h))

    def align_dev(self, tx, ty, toff, sx, sy, soff, init, out=None, stream=None):
        """Everything already on the device (torch CUDA tensors: float32 clouds, int64
        offsets [n+1], float64 init [n,3]).  Asynchronous; returns the float64 [n,18] result
        tensor (decode with ``decode``) - valid once the stream is synchronised.  stream=None runs on
        the context's own stream, ordered behind torch's current stream on the way in and ahead of it
        on the way out, so the call composes with torch code like any torch op."""
        return self._align_dev((tx, ty), toff, (sx, sy), soff, init, out, stream)


class NdtBatch3D(_NdtBatch):
    """The 3D batch (ndt3d_batch_* of include/ndt_hip.h), the pair's voxel grid in LDS."""
    _prefix = "ndt3d_batch"
    _dim = _DIM3

    def __init__(self, device: int = 0, levels=None, global_workgroups: int | None = None, **overrides):
        """global_workgroups: workgroups (and 7.9 MB table slabs) of the global-table variant, 1..256 (default 256)."""
        self.params = default_params3d(**overrides)
        self._create_batch(device, levels, batch_global_workgroups=global_workgroups)

    def align_dev(self, t, toff, s, soff, init, out=None, stream=None):
        """Everything already on the device: t / s = (x, y, z) float32 CUDA tensors (concatenated clouds),
        int64 offsets [n+1], float64 init [n,6].  Asynchronous; returns the float64 [n,51] result tensor
        (decode with ``decode``).  Stream semantics as NdtBatch2D.align_dev."""
        return self._align_dev(t, toff, s, soff, init, out, stream)


class _NdtMulti(_Context):
    """The loop-closure batch over several devices from one host process (one batch-like context and one host thread
    per device): `align` takes host pairs, `align_dev` device-resident shards whose result rows are exchanged with one
    RCCL all-gather."""

    def _create_multi(self, devices, levels):
        if devices is None:
            ids, n = None, 0
        else:
            ids, n = (C.c_int32 * len(devices))(*[int(d) for d in devices]), len(devices)
        self._create(levels, ids, n)
        self.last_shard_stride = 0

    @property
    def device_count(self) -> int:
        return int(self._c.device_count(self._h))

    def _align_dev(self, shards):
        """shards[d] = (t, toff, s, soff, init) of torch tensors resident on device d, t / s the tuples of the
        concatenated clouds' coordinates (the layout of the batch align_dev), or None for an empty shard."""
        import torch
        nd = self.device_count
        if len(shards) != nd:
            raise ValueError("one shard per device context")
        ptr = [(C.c_void_p * nd)() for _ in range(2 * self._dim.ncoord + 3)]
        n_pairs = (C.c_size_t * nd)()
        for d, sh in enumerate(shards):
            if sh is None:
                continue
            for column, address in zip(ptr, _dev_layout("shard", *sh)):
                column[d] = address
            n_pairs[d] = int(sh[1].numel()) - 1
            torch.cuda.synchronize(sh[0][0].device)     # the contexts' streams are not torch's: finish the producers
        total = sum(n_pairs)
        out = np.zeros(total * self._dim.result_doubles, dtype=np.float64)
        stride = C.c_size_t(0)
        self._check(self._c.align_dev(self._h, *ptr, n_pairs, None, C.byref(stride), out.ctypes.data), "align_dev")
        self.last_shard_stride = int(stride.value)
        return self._dim.results(out, total)


class NdtMulti2D(_NdtMulti):
    """The 2D multi-device batch; mirrors ndt2d_multi_* of include/ndt_hip.h."""
    _prefix = "ndt2d_multi"
    _dim = _DIM2

    def __init__(self, devices=None, params: L.Params2D | None = None, levels=None, **overrides):
        """levels: coarse-to-fine list of Params2D (e.g. pyramid_params()); otherwise one level."""
        self.params = _params_2d(params, overrides)
        self._create_multi(devices, levels)

    def align_dev(self, shards):
        """ndt2d_multi_align_dev: shards[d] = dict of torch tensors resident on device d (tx, ty, toff, sx,
        sy, soff, init - the layout of NdtBatch2D.align_dev; an empty shard is None).  Every shard is
        aligned on its device and the rows are exchanged with one RCCL all-gather; returns the list of
        AlignResult in global pair order (shard 0's pairs, shard 1's, ...)."""
        return self._align_dev([sh and ((sh["tx"], sh["ty"]), sh["toff"], (sh["sx"], sh["sy"]), sh["soff"], sh["init"])
                                for sh in shards])


class NdtMulti3D(_NdtMulti):
    """The 3D multi-device batch (ndt3d_multi_* of include/ndt_hip.h)."""
    _prefix = "ndt3d_multi"
    _dim = _DIM3

    def __init__(self, devices=None, levels=None, **overrides):
        self.params = default_params3d(**overrides)
        self._create_multi(devices, levels)

    def align_dev(self, shards):
        """shards[d] = dict(t=(x, y, z), toff, s=(x, y, z), soff, init) of torch tensors resident on device d (the layout
        of NdtBatch3D.align_dev; None for an empty shard).  Returns the results in global pair order."""
        return self._align_dev([sh and (sh["t"], sh["toff"], sh["s"], sh["soff"], sh["init"]) for sh in shards])


def magnusson_constants(outlier_ratio: float, cell_size: float, dim: int = 2):
    """(d1, d2) of Magnusson's outlier-mixture score for ndt2d_params / ndt3d_params."""
    d1, d2 = C.c_double(), C.c_double()
    L.check(L.load().ndt_magnusson_constants(float(outlier_ratio), float(cell_size), int(dim), C.byref(d1), C.byref(d2)),
            "ndt_magnusson_constants")
    return d1.value, d2.value


def _motion(motion, n: int):
    """A sweep's motion as the C array the de-skewing entry points take: n doubles."""
    if len(motion) != n:
        raise ValueError(f"the sweep's motion must have {n} entries")
    return (C.c_double * n)(*[float(v) for v in motion])


def _sweep_frac(frac, n: int):
    """(frac0, frac_inc) of a conversion's beams or columns; by default they fill the sweep, [0, 1)."""
    return (0.0, 1.0 / n) if frac is None else (float(frac[0]), float(frac[1]))


def polar_to_points(ranges, angle_min: float, angle_inc: float, range_min: float = 0.0, range_max: float = 1e30, *,
                    motion=None, frac=None, ref_frac: float = 1.0):
    """Range/bearing scan (torch CUDA float32 tensor) -> (x, y) CUDA tensors, on the device.  motion = (dx, dy, dtheta),
    the sensor's pose at the end of the sweep in its frame at the start, undoes the motion within the sweep
    (ndt2d_polar_to_points_deskew_dev): beam i was fired at sweep fraction frac[0] + i * frac[1] (default (0, 1 / n)) and
    the points come out in the sensor frame at fraction ref_frac (1 = the end of the sweep)."""
    import torch
    n = ranges.numel()
    x = torch.empty(n, dtype=torch.float32, device=ranges.device)
    y = torch.empty(n, dtype=torch.float32, device=ranges.device)
    if motion is not None:
        L.check(L.load().ndt2d_polar_to_points_deskew_dev(*_dev_ptrs((ranges,), n), n, float(angle_min), float(angle_inc),
                                                          float(range_min), float(range_max), _motion(motion, 3),
                                                          *_sweep_frac(frac, n), float(ref_frac), *_dev_ptrs((x, y), n),
                                                          _torch_stream_ptr()), "ndt2d_polar_to_points_deskew_dev")
        return x, y
    L.check(L.load().ndt2d_polar_to_points_dev(*_dev_ptrs((ranges,), n), n, float(angle_min), float(angle_inc),
                                               float(range_min), float(range_max), *_dev_ptrs((x, y), n),
                                               _torch_stream_ptr()), "ndt2d_polar_to_points_dev")
    return x, y


def range_image_to_points(ranges, elevations, azimuth0: float, azimuth_inc: float, range_min: float = 0.0,
                          range_max: float = 1e30, *, motion=None, frac=None, ref_frac: float = 1.0):
    """Range image [n_elev, n_azim] (torch CUDA float32 tensor) of a multi-beam lidar -> (x, y, z) CUDA tensors of
    n_elev * n_azim points, on the device (ndt3d_range_image_to_points_dev).  motion = (tx, ty, tz, roll, pitch, yaw)
    undoes the motion within the sweep (ndt3d_range_image_to_points_deskew_dev): azimuth column j was fired at sweep
    fraction frac[0] + j * frac[1] (default (0, 1 / n_azim)), the points come out in the sensor frame at ref_frac."""
    import torch
    n_elev, n_azim = ranges.shape
    n = n_elev * n_azim
    out = [torch.empty(n, dtype=torch.float32, device=ranges.device) for _ in range(3)]
    el = (C.c_double * n_elev)(*[float(v) for v in elevations])
    if motion is not None:
        L.check(L.load().ndt3d_range_image_to_points_deskew_dev(*_dev_ptrs((ranges,), n), n_elev, n_azim, el, float(azimuth0),
                                                                float(azimuth_inc), float(range_min), float(range_max),
                                                                _motion(motion, 6), *_sweep_frac(frac, n_azim),
                                                                float(ref_frac), *_dev_ptrs(out, n), _torch_stream_ptr()),
                "ndt3d_range_image_to_points_deskew_dev")
        return tuple(out)
    L.check(L.load().ndt3d_range_image_to_points_dev(*_dev_ptrs((ranges,), n), n_elev, n_azim, el, float(azimuth0), float(azimuth_inc),
                                                     float(range_min), float(range_max), *_dev_ptrs(out, n),
                                                     _torch_stream_ptr()), "ndt3d_range_image_to_points_dev")
    return tuple(out)


def deskew_points(coords, frac, motion, ref_frac: float = 1.0, out=None):
    """Cartesian device points with a sweep fraction each -> the points in the sensor frame at fraction ref_frac
    (ndt2d_deskew_points_dev / ndt3d_deskew_points_dev).  coords is a 2- or 3-tuple of CUDA float32 tensors, frac one
    more of the same length, motion the 3- or 6-vector of the sweep; out (default: new tensors) may be coords itself."""
    import torch
    dim = len(coords)
    if dim not in (2, 3):
        raise ValueError("coords must be (x, y) or (x, y, z)")
    n = coords[0].numel()
    if out is None:
        out = tuple(torch.empty(n, dtype=torch.float32, device=coords[0].device) for _ in range(dim))
    if len(out) != dim:
        raise ValueError("out must have as many tensors as coords")
    name = f"ndt{dim}d_deskew_points_dev"
    L.check(getattr(L.load(), name)(*_dev_ptrs((*coords, frac), n), n, _motion(motion, 3 * dim - 3), float(ref_frac),
                                    *_dev_ptrs(out, n), _torch_stream_ptr()), name)
    return tuple(out)


def sweep_motion(prev, cur):
    """prev^-1 o cur of two poses (both 3- or both 6-vectors) in one frame: the motion between the last two estimates,
    the constant-velocity guess of the motion within the next sweep (ndt2d_sweep_motion / ndt3d_sweep_motion)."""
    n = len(prev)
    if n not in (3, 6) or len(cur) != n:
        raise ValueError("poses have 3 or 6 entries, both the same")
    delta = (C.c_double * n)()
    name = f"ndt{n // 3 + 1}d_sweep_motion"
    L.check(getattr(L.load(), name)(_motion(prev, n), _motion(cur, n), delta), name)
    return tuple(delta)


def motion_twist(delta):
    """The constant twist Log(delta) of a sweep's motion: (vx, vy, omega) or (rho[3], phi[3]) (ndt2d_motion_twist /
    ndt3d_motion_twist)."""
    n = len(delta)
    if n not in (3, 6):
        raise ValueError("a motion has 3 or 6 entries")
    xi = (C.c_double * n)()
    name = f"ndt{n // 3 + 1}d_motion_twist"
    L.check(getattr(L.load(), name)(_motion(delta, n), xi), name)
    return tuple(xi)


# Coarse-to-fine schedule relative to the finest cell: (cell multiplier, eig_ratio).  Coarse
# levels widen the Gaussians (larger cells AND a larger eigenvalue floor) so that alignments
# started outside the fine grid's ~0.2-cell basin still converge.
PYRAMID_LEVELS = ((4.0, 0.1), (2.0, 0.03))


def _coarse_level(fine, mult, eig_ratio) -> dict:
    """A coarse level of `fine`: `mult` times its cell, a stronger eigenvalue floor and loose stops."""
    return dict(cell_size=fine.cell_size * mult, eig_ratio=eig_ratio, eps_trans=1e-3, eps_rot=1e-4, max_iterations=30,
                fixed_iterations=0, step_max_trans=fine.step_max_trans * mult)


def map_level_params(fine, level):
    """Keyword parameters of one coarse level of a map pyramid: the fine matcher's, with the level's cell size and - for
    a (multiplier, eig_ratio) level - the eigenvalue floor and loose stops of NdtPyramid2D / NdtPyramid3D; a
    (multiplier, dict) level takes the dict's parameters and nothing else."""
    mult, spec = level
    kw = {k: getattr(fine, k) for k, _ in L.Params2D._fields_ if not k.startswith("reserved")}
    kw["cell_size"] = fine.cell_size * mult
    kw.update(spec if isinstance(spec, dict) else _coarse_level(fine, mult, spec))
    return kw


class _Pyramid:
    """Matchers coarse to fine in `levels`, and the walk down them."""
    _Matcher = None
    levels = ()

    def close(self):
        for m in self.levels:
            m.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _descend(levels, align, pose):
        """align(level, pose) for every level, each started from the pose of the one before; a level that fails ends
        the walk.  Returns the last result with the iterations of all levels summed."""
        total, r = 0, None
        for level in levels:
            r = align(level, pose)
            total += r.iterations
            if r.status not in (L.NDT_OK, L.NDT_NOT_CONVERGED):
                break
            pose = r.pose
        r.iterations = total
        return r


class _NdtPyramid(_Pyramid):
    """Multi-resolution alignment: one matcher per level (cells 4c and 2c with a stronger eigenvalue clamp and loose
    stops, then the caller's parameters), each level started from the previous level's pose."""

    def __init__(self, device: int = 0, levels=PYRAMID_LEVELS, **overrides):
        fine = self._Matcher._dim.default_params(**overrides)
        self.levels = [self._Matcher(device, **{**overrides, **_coarse_level(fine, mult, er)}) for mult, er in levels]
        self.levels.append(self._Matcher(device, **overrides))

    def _set_target(self, coords):
        return [m._set_target(coords) for m in self.levels][-1]

    def _align(self, coords, init_pose):
        return self._descend(self.levels, lambda m, pose: m._align(coords, pose), tuple(init_pose))


class NdtPyramid2D(_NdtPyramid):
    _Matcher = NdtMatcher2D

    def set_target(self, x, y):
        return self._set_target((x, y))

    def align(self, sx, sy, init_pose=(0.0, 0.0, 0.0)) -> AlignResult:
        return self._align((sx, sy), init_pose)


class NdtPyramid3D(_NdtPyramid):
    _Matcher = NdtMatcher3D

    def __init__(self, device: int = 0, levels=PYRAMID_LEVELS, neighbourhood: int = 1, **overrides):
        """neighbourhood: NdtMatcher3D.set_neighbourhood() of every level's handle."""
        super().__init__(device, levels, **overrides)
        if neighbourhood != 1:
            for m in self.levels:
                m.set_neighbourhood(neighbourhood)

    def set_target(self, x, y, z):
        return self._set_target((x, y, z))

    def align(self, sx, sy, sz, init_pose=(0.0,) * 6) -> AlignResult3D:
        return self._align((sx, sy, sz), init_pose)


class _NdtMapPyramid(_Pyramid):
    """Coarse-to-fine map-to-map alignment between submaps that hold no points: the coarse levels are derived from the
    fine matcher's exact per-cell sums (coarsen_into), so a submap that came back from load_map gets the same escape
    from the fine lattice's local optimum that NdtPyramid2D / NdtPyramid3D give scans."""

    def __init__(self, fine, levels=PYRAMID_LEVELS, _owns_fine: bool = False):
        """fine: a matcher that holds a target (it stays the caller's, and is the last level).  levels: (cell
        multiplier, eig_ratio) or (cell multiplier, dict of parameters), multipliers 2 or 4, coarse to fine."""
        self._fine, self._owns_fine = fine, _owns_fine
        self.levels = []
        try:
            for level in levels:
                m = self._Matcher(fine._device, **map_level_params(fine.params, level))
                self.levels.append(m)
                fine.coarsen_into(m)
        except Exception:
            self.close()
            raise
        self.levels.append(fine)

    @classmethod
    def from_blob(cls, blob, device: int = 0, levels=PYRAMID_LEVELS, **params):
        """The pyramid of a saved submap (save_map's buffer): a fresh fine matcher with `params` (cell_size defaults to
        the blob's) loads it, and the coarse levels follow from it.  close() frees all of them."""
        head = L.MapHeader.from_buffer_copy(bytes(memoryview(np.ascontiguousarray(blob).view(np.uint8))[:C.sizeof(L.MapHeader)]))
        params.setdefault("cell_size", head.cell_size)
        fine = cls._Matcher(device, **params)
        try:
            fine.load_map(blob)
            return cls(fine, levels, _owns_fine=True)
        except Exception:
            fine.close()
            raise

    def close(self):
        for m in self.levels:
            if m is not self._fine or self._owns_fine:
                m.close()
        self.levels = []

    def align_map(self, source, init_pose=None):
        """level.align_map(source.level, pose) coarse to fine, each level from the one before; returns the last level's
        result with the iterations of all levels summed (as NdtPyramid2D.align)."""
        if len(source.levels) != len(self.levels):
            raise ValueError("both pyramids need the same levels")
        return self._descend(zip(self.levels, source.levels), lambda pair, pose: pair[0].align_map(pair[1], pose),
                             tuple(init_pose) if init_pose is not None else None)

    def merge(self, other, pose) -> int:
        """level.merge_map(other.level, pose) for every level: the other pyramid's submap folded into this one's at `pose`
        (what self.align_map(other) returns).  Returns the fine level's count of points that fell outside."""
        if len(other.levels) != len(self.levels):
            raise ValueError("both pyramids need the same levels")
        out = 0
        for mine, theirs in zip(self.levels, other.levels):
            out = mine.merge_map(theirs, pose)
        return out


class NdtMapPyramid2D(_NdtMapPyramid):
    _Matcher = NdtMatcher2D


class NdtMapPyramid3D(_NdtMapPyramid):
    _Matcher = NdtMatcher3D

    def __init__(self, fine, levels=PYRAMID_LEVELS, map_neighbourhood: int = 1, _owns_fine: bool = False):
        """map_neighbourhood: NdtMatcher3D.set_map_neighbourhood() of every level's handle, `fine` included, when it is
        not 1 (1 leaves `fine` as the caller set it)."""
        super().__init__(fine, levels, _owns_fine)
        if map_neighbourhood != 1:
            for m in self.levels:
                m.set_map_neighbourhood(map_neighbourhood)

    @classmethod
    def from_blob(cls, blob, device: int = 0, levels=PYRAMID_LEVELS, map_neighbourhood: int = 1, **params):
        """_NdtMapPyramid.from_blob, with map_neighbourhood for every level."""
        pyr = super().from_blob(blob, device, levels, **params)
        if map_neighbourhood != 1:
            for m in pyr.levels:
                m.set_map_neighbourhood(map_neighbourhood)
        return pyr
