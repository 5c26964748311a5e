"""Host-side mirror of the reference's plugin surface for the scan-matching hot path, over the C ABI.

Class and method names follow the reference so that tests read like its own drivers:

* ``CorrespondenceFinderProjective2f`` / ``CorrespondenceFinderKDTree2D`` -- ``setFixed``, ``setMoving``,
  ``setLocalMapInSensor``, ``compute`` (apps/visual_test_correspondence_finder_projective_2d.cpp:74-79;
  parameters of registration/correspondence_finder_projective_2d.h:16-26, ..._kd_tree_2d.h:23-34).
* ``AlignerSliceProcessorLaser2D`` / ``...WithSensor`` (registration/aligner_slice_processor_laser_2d.h:7-42;
  config fields configurations/stage_segway_double_config_MULTI.json:160-188).
* ``MultiAligner2D`` -- ``param_slice_processors``, ``setFixed``, ``setMoving``, ``setMovingInFixed``, ``compute``,
  ``movingInFixed``, ``iterationStats`` (apps/visual_test_aligner_2d.cpp:123-156), plus ``compute_batch`` for the
  loop-closure / relocalisation sweeps the reference runs as a sequential loop (MULTI.json:964-986).

Errors: the reference throws ``std::runtime_error`` on missing inputs
(registration/correspondence_finder_projective_2d.cpp:21-31); here that is ``RuntimeError``; device/ABI failures raise
``Lsm2dError``.  All compute happens in the HIP library; nothing here falls back to a CPU path.
"""
from __future__ import annotations

import collections
import ctypes as C
import weakref
import dataclasses
import math
from typing import Optional, Sequence

import numpy as np

from . import _capi
from ._capi import (FINDER_NN, FINDER_PROJECTIVE, ROBUST_CAUCHY, ROBUST_NONE, AlignerParams, Batch, Correspondence,
                    IterationStats, Lsm2dError, Prior, Projector, SliceParams, check)
from ._capi import SELECT_MAX_K, SELECT_TILE      # noqa: F401  (LSM2D_SELECT_MAX_K; the selection's tile: where it takes another pass)

from ._capi import VOXELIZE_MAX_GROUPS, VOXELIZE_MAX_POINTS      # noqa: F401  (LSM2D_VOXELIZE_MAX_POINTS / _MAX_GROUPS)
from ._capi import OCCUPANCY_MAX_CELLS, OCCUPANCY_MAX_RAY_CELLS, OCCUPANCY_MAX_RAYS, OCCUPANCY_MAX_SIDE      # noqa: F401  (LSM2D_OCCUPANCY_MAX_*)

STATUS_NAMES = {0: "Success", 1: "NotEnoughCorrespondences", 2: "NotEnoughInliers", 3: "SingularH"}


class Context:
    """One device + one HIP stream (lsm2d_context)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None, kernel_timing: bool = True):
        """kernel_timing: record HIP events around the hot-path launches so that ``last_kernel_ms()`` / ``BatchResult.kernel_ms``
        work (what the tests and bench.py want; the library's own default is off: the events cost a latency-critical caller
        ~20 % of a tracker step)."""
        self._lib = _capi.load()
        h = C.c_void_p()
        rc = self._lib.lsm2d_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != 0:
            raise Lsm2dError(rc, "lsm2d_create", self._lib.lsm2d_last_error(None).decode())
        self._h = h
        self._sets = weakref.WeakSet()      # the cloud sets living on this context: close() destroys them first (a set outliving its context would touch freed memory)
        self.device = device
        self.kernel_timing = bool(kernel_timing)
        if kernel_timing:
            check(self._lib.lsm2d_set_option(self._h, b"kernel_timing", 1), "lsm2d_set_option", self._h)

    @property
    def handle(self):
        return self._h

    def synchronize(self):
        check(self._lib.lsm2d_synchronize(self._h), "lsm2d_synchronize", self._h)

    def set_option(self, key: str, value: int):
        """e.g. ``set_option("align_path", 2)``: 0 automatic, 1 one workgroup per alignment, 2 split over many workgroups,
        3 two projective slices side by side in one workgroup."""
        if key == "kernel_timing":
            self.kernel_timing = bool(value)
        check(self._lib.lsm2d_set_option(self._h, key.encode(), int(value)), "lsm2d_set_option", self._h)

    def get_option(self, key: str) -> int:
        """Reads a knob back; ``"last_align_path"`` tells which kernels the latest ``align_batch`` ran (1, 2 or 3)."""
        v = C.c_int64()
        check(self._lib.lsm2d_get_option(self._h, key.encode(), C.byref(v)), "lsm2d_get_option", self._h)
        return int(v.value)

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        check(self._lib.lsm2d_last_kernel_ms(self._h, C.byref(ms)), "lsm2d_last_kernel_ms", self._h)
        return ms.value

    def close(self):
        if getattr(self, "_h", None):
            for cs in list(getattr(self, "_sets", ())):
                cs.close()
            self._lib.lsm2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr(a):
    """a numpy array or a torch tensor as a pointer argument; None stays NULL"""
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data_as(C.c_void_p)


_Made = collections.namedtuple("_Made", "handle n_clouds n_points counts capacity")      # a set the library has made already: CloudSet._adopt's way into __init__


class CloudSet:
    """Device-resident ragged set of PointNormal2fVectorCloud (lsm2d_cloudset)."""

    def __init__(self, ctx: Context, points, offsets=None):
        """``points``: float32 [N, 4] (x, y, nx, ny) on the host, or a torch tensor of that shape on ctx's device; ``offsets`` [n_clouds + 1] cuts them into
        clouds (None: one cloud).  Every field a set has is set here and nowhere else."""
        made = points if isinstance(points, _Made) else self._create(ctx, points, offsets)
        self._ctx = ctx
        self._lib = ctx._lib
        self._h = made.handle
        self.n_clouds = made.n_clouds
        self.capacity = made.capacity      # points a cloud of a reserved set has room for; None for every other set
        self._n_points, self._counts = made.n_points, made.counts
        self._pending = False
        ctx._sets.add(self)

    @classmethod
    def _adopt(cls, ctx: Context, handle, n_clouds: int, n_points: int, counts: np.ndarray, capacity: Optional[int] = None) -> "CloudSet":
        """The one way to put a CloudSet around a handle the library returned: every constructor ends here."""
        return cls(ctx, _Made(handle, int(n_clouds), int(n_points), counts, capacity))

    @staticmethod
    def _create(ctx: Context, points, offsets) -> _Made:
        """lsm2d_cloudset_create / _create_from_device: host points [N, 4] or a torch tensor already on ctx's device"""
        if hasattr(points, "data_ptr"):
            if not points.is_cuda or not points.is_contiguous() or points.dtype.itemsize != 4 or points.shape[-1] != 4:
                raise ValueError("device points must be a contiguous float32 [N, 4] tensor on the GPU")
            pts, create = points, ctx._lib.lsm2d_cloudset_create_from_device
            _producer_stream_wait(points)
        else:
            pts, create = np.ascontiguousarray(points, np.float32), ctx._lib.lsm2d_cloudset_create
            if pts.ndim != 2 or pts.shape[1] != 4:
                raise ValueError("points must be [N, 4] (x, y, nx, ny)")
        total = int(pts.shape[0])
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        n_clouds = 1 if offs is None else len(offs) - 1
        h = C.c_void_p()
        check(create(ctx.handle, _ptr(pts), _ptr(offs), n_clouds, total, C.byref(h)), "lsm2d_cloudset_create", ctx.handle)
        return _Made(h, n_clouds, total, np.array([total], np.int64) if offs is None else np.diff(offs.astype(np.int64)), None)

    @property
    def handle(self):
        return self._h

    @classmethod
    def reserved(cls, ctx: Context, capacity: int) -> "CloudSet":
        """One growable device cloud (the local map a tracker keeps merging into / a clipped scene)."""
        h = C.c_void_p()
        check(ctx._lib.lsm2d_cloudset_create_reserved(ctx.handle, int(capacity), C.byref(h)), "lsm2d_cloudset_create_reserved", ctx.handle)
        return cls._adopt(ctx, h, 1, 0, np.zeros(1, np.int64), int(capacity))

    @classmethod
    def reserved_many(cls, ctx: Context, n_clouds: int, capacity: int) -> "CloudSet":
        """``n_clouds`` growable device clouds, each with room for ``capacity`` points (the local maps of N trackers, or their clipped
        scenes: lsm2d_cloudset_create_reserved_many).  The single-cloud calls refuse such a set; the batched clipper / merger fill it."""
        h = C.c_void_p()
        check(ctx._lib.lsm2d_cloudset_create_reserved_many(ctx.handle, int(n_clouds), int(capacity), C.byref(h)),
              "lsm2d_cloudset_create_reserved_many", ctx.handle)
        return cls._adopt(ctx, h, n_clouds, 0, np.zeros(int(n_clouds), np.int64), int(capacity))

    def clear(self, indices=None):
        """Empties clouds ``indices`` (None: all) of a ``reserved_many`` set, asynchronously (lsm2d_cloudset_clear_clouds)."""
        idx = None if indices is None else np.ascontiguousarray(indices, np.int32).ravel()
        check(self._lib.lsm2d_cloudset_clear_clouds(self._h, 0 if idx is None else len(idx), _ptr(idx)), "lsm2d_cloudset_clear_clouds", self._ctx.handle)
        if not self._pending:
            c = self._counts.copy(); c[slice(None) if idx is None else idx] = 0
            self._counts = c; self._n_points = int(c.sum())

    # n_points / counts of a reserved set can be "known to the device only" after an asynchronous clip / merge
    # (SceneClipperProjective2D / MergerProjective2D with asynchronous=True): reading them then asks the library, which
    # synchronises once.
    @property
    def n_points(self) -> int:
        self._resolve()
        return self._n_points

    @property
    def counts(self) -> np.ndarray:
        self._resolve()
        return self._counts

    def _resolve(self):
        if not self._pending:
            return
        if self.n_clouds > 1:      # all sizes of a multi-cloud set with one wait
            c = np.empty(self.n_clouds, np.int32)
            check(min(self._lib.lsm2d_cloudset_cloud_sizes(self._h, _ptr(c), self.n_clouds), 0), "lsm2d_cloudset_cloud_sizes", self._ctx.handle)
            counts = c.astype(np.int64)
        else:
            counts = np.array([int(self._lib.lsm2d_cloudset_cloud_size(self._h, 0))], np.int64)
        self._pending = False
        self._n_points, self._counts = int(counts.sum()), counts

    def _set_count(self, n: int):
        self._pending = False
        self._n_points = int(n); self._counts = np.array([int(n)], np.int64)

    def _set_pending(self):
        self._pending = True

    def upload(self, points):
        """Refill this single-cloud set in place (no allocation, no wait for the stream: the points are copied into the
        set's pinned staging buffer before the call returns)."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        check(self._lib.lsm2d_cloudset_upload(self._h, _ptr(pts), len(pts)), "lsm2d_cloudset_upload", self._ctx.handle)
        self._set_count(len(pts))

    def download(self, cloud_index: int = 0) -> np.ndarray:
        cap = int(self.counts[cloud_index])
        out = np.empty((max(cap, 1), 4), np.float32); n = C.c_int64(0)
        check(self._lib.lsm2d_cloudset_download(self._h, cloud_index, _ptr(out), cap, C.byref(n)), "lsm2d_cloudset_download", self._ctx.handle)
        return out[: n.value].copy()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsm2d_cloudset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _producer_stream_wait(tensor):
    """A device tensor handed to the C ABI is read on the CONTEXT's stream, which knows nothing about the stream that produced the
    tensor (torch's current stream): wait for that stream here, so a tensor computed a moment ago is read complete (include/lsm2d.h,
    ORDERING note).  A context created on torch's own stream would not need this; the wait is cheap when the stream is idle."""
    if getattr(tensor, "is_cuda", False):
        import torch
        torch.cuda.current_stream(tensor.device).synchronize()


def _as_cloudset(ctx: Context, cloud) -> CloudSet:
    return cloud if isinstance(cloud, CloudSet) else CloudSet(ctx, cloud)


class _BatchItems:
    """The items of a batched finder / factor / score call, marshalled once for every wrapper of the family: the sets as CloudSet, ``poses`` as float32
    ``[n, 3]``, the optional index arrays as int32 ``[n]`` or NULL.  ``head(slice_params)`` is the argument list all these entry points begin with (context,
    slice, fixed set and index, moving set and index, n_items); ``rows`` = max(n, 1) sizes the outputs, so that an empty batch still passes real pointers."""

    def __init__(self, ctx: Context, fixed, moving, poses, fixed_index, moving_index):
        self.ctx = ctx
        self.fixed, self.moving = _as_cloudset(ctx, fixed), _as_cloudset(ctx, moving)
        self.poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
        self.n = len(self.poses)
        self.rows = max(self.n, 1)
        self.fixed_index = None if fixed_index is None else np.ascontiguousarray(fixed_index, np.int32).reshape(self.n)
        self.moving_index = None if moving_index is None else np.ascontiguousarray(moving_index, np.int32).reshape(self.n)

    def head(self, slice_params: SliceParams) -> tuple:
        return (self.ctx.handle, C.byref(slice_params), self.fixed.handle, _ptr(self.fixed_index), self.moving.handle, _ptr(self.moving_index), self.n)


def _pair_capacity(slice_params: SliceParams, moving: CloudSet, moving_index: Optional[int] = None) -> int:
    """How many pairs a slice can return, at least 1 (an output buffer is never empty): the projective finder gives at most one per canvas column, the
    others at most one per moving point -- of cloud ``moving_index``, or of the set's largest cloud when the call spans the set."""
    if slice_params.finder == FINDER_PROJECTIVE:
        return max(int(slice_params.projector.canvas_cols), 1)
    counts = moving.counts
    if moving_index is not None:
        return max(int(counts[moving_index]), 1)
    return max(int(counts.max()) if len(counts) else 0, 1)


@dataclasses.dataclass
class PointNormal2fProjectorPolar:
    """Parameters of the polar projector (apps/synthetic_scene_generator.cpp:69-75; MULTI.json:71-97)."""
    param_canvas_cols: int = 721
    param_angle_col_min: float = -math.pi
    param_angle_col_max: float = math.pi
    param_range_min: float = 0.3
    param_range_max: float = 20.0
    col_offset: float = 0.0

    def struct(self) -> Projector:
        return Projector(self.param_canvas_cols, self.param_angle_col_min, self.param_angle_col_max,
                         self.param_range_min, self.param_range_max, self.col_offset)

    def compute(self, ctx: Context, cloud, pose=(0.0, 0.0, 0.0), cloud_index: int = 0):
        """One z-buffer pass; ``pose`` maps cloud points into the camera frame (= camera_pose^-1).
        Returns (source_idx int32 [cols], depth float32 [cols], transformed float32 [cols, 4])."""
        cs = _as_cloudset(ctx, cloud)
        cols = self.param_canvas_cols
        src = np.empty(cols, np.int32); depth = np.empty(cols, np.float32); xy = np.empty((cols, 4), np.float32)
        pose = np.ascontiguousarray(pose, np.float32)
        pr = self.struct()
        check(ctx._lib.lsm2d_project(ctx.handle, C.byref(pr), cs.handle, cloud_index, _ptr(pose), _ptr(src), _ptr(depth), _ptr(xy)), "lsm2d_project", ctx.handle)
        return src, depth, xy


class _FinderBase:
    finder_kind = FINDER_PROJECTIVE

    def __init__(self, ctx: Context):
        self._ctx = ctx
        self._fixed = None
        self._moving = None
        self._local_map_in_sensor = np.zeros(3, np.float32)
        self._correspondences = np.zeros((0, 2), np.int32)
        self._fixed_index = 0
        self._moving_index = 0

    # CorrespondenceFinder_ base-class surface (registration/correspondence_finder_normal_2f.h:9-13)
    def setFixed(self, fixed, index: int = 0):
        self._fixed = _as_cloudset(self._ctx, fixed); self._fixed_index = index

    def setMoving(self, moving, index: int = 0):
        self._moving = _as_cloudset(self._ctx, moving); self._moving_index = index

    def setLocalMapInSensor(self, pose):
        self._local_map_in_sensor = np.ascontiguousarray(pose, np.float32).reshape(3)

    def correspondences(self) -> np.ndarray:
        return self._correspondences

    def slice_params(self, **kw) -> SliceParams:
        raise NotImplementedError

    def compute(self) -> np.ndarray:
        if self._fixed is None:
            raise RuntimeError(type(self).__name__ + "::compute| Missing fixed!")
        if self._moving is None:
            raise RuntimeError(type(self).__name__ + "::compute| Missing moving!")
        sp = self.slice_params()
        cap = _pair_capacity(sp, self._moving, self._moving_index)
        out = np.empty((cap, 2), np.int32)
        n = C.c_int32(0)
        lib = self._ctx._lib
        check(lib.lsm2d_find_correspondences(self._ctx.handle, C.byref(sp), self._fixed.handle, self._fixed_index, self._moving.handle, self._moving_index,
                                             _ptr(self._local_map_in_sensor), _ptr(out), cap, C.byref(n)),
              "lsm2d_find_correspondences", self._ctx.handle)
        self._correspondences = out[:n.value].copy()
        return self._correspondences

    def compute_batch(self, fixed, moving, poses, fixed_index=None, moving_index=None) -> list:
        """compute() for ``len(poses)`` independent (fixed, moving, pose) triples in one launch (lsm2d_find_correspondences_batch): item ``i``
        matches cloud ``fixed_index[i]`` of the set ``fixed`` against cloud ``moving_index[i]`` of the set ``moving`` under ``poses[i]``
        (None: cloud ``i``, or the only cloud of a one-cloud set).  Returns a list of int32 ``[k, 2]`` arrays (fixed_idx, moving_idx): per
        item what ``compute()`` returns, in the same order."""
        ctx = self._ctx
        it = _BatchItems(ctx, fixed, moving, poses, fixed_index, moving_index)
        sp = self.slice_params()
        cap = _pair_capacity(sp, it.moving)
        out = np.empty((it.rows, cap, 2), np.int32); cnt = np.zeros(it.rows, np.int32)
        check(ctx._lib.lsm2d_find_correspondences_batch(*it.head(sp), _ptr(it.poses), _ptr(out), cap, _ptr(cnt)), "lsm2d_find_correspondences_batch", ctx.handle)
        return [out[i, : cnt[i]].copy() for i in range(it.n)]


class CorrespondenceFinderProjective2f(_FinderBase):
    """registration/correspondence_finder_projective_2d.{h,cpp}"""
    finder_kind = FINDER_PROJECTIVE

    def __init__(self, ctx: Context, projector: Optional[PointNormal2fProjectorPolar] = None,
                 point_distance: float = 0.5, normal_cos: float = 0.8):
        super().__init__(ctx)
        self.param_projector = projector
        self.param_point_distance = point_distance
        self.param_normal_cos = normal_cos

    def slice_params(self, **kw) -> SliceParams:
        if self.param_projector is None:
            raise RuntimeError("CorrespondenceFinderProjective2f::compute| Missing Projector")
        return make_slice_params(finder=FINDER_PROJECTIVE, projector=self.param_projector,
                                 point_distance=self.param_point_distance, normal_cos=self.param_normal_cos, **kw)


class CorrespondenceFinderKDTree2D(_FinderBase):
    """registration/correspondence_finder_kd_tree_2d.{h,cpp}.  ``search``: "exact" (LSM2D_FINDER_NN: exact nearest neighbour on a uniform
    grid; max_leaf_range / min_leaf_points have no meaning there) or "kdtree" (LSM2D_FINDER_KDTREE: the reference's own tree --
    KDTree2D(coordinates, max_leaf_range, min_leaf_points), .cpp:36-37 -- and its single-leaf descent, hence approximate).  The SRRG-side
    sibling (adapters/srrg) defaults to "kdtree"; this mirror keeps "exact" as its default so that existing drivers read unchanged."""

    def __init__(self, ctx: Context, max_distance_m: float = 1e-2, normal_cos: float = 0.8,
                 max_leaf_range: float = 1e-2, min_leaf_points: int = 20, search: str = "exact"):
        super().__init__(ctx)
        if search not in ("exact", "kdtree"):
            raise ValueError('search must be "exact" or "kdtree"')
        self.param_max_distance_m = max_distance_m
        self.param_normal_cos = normal_cos
        self.param_max_leaf_range = max_leaf_range      # honoured by search="kdtree"
        self.param_min_leaf_points = min_leaf_points
        self.search = search

    @property
    def finder_kind(self):
        return _capi.FINDER_KDTREE if self.search == "kdtree" else FINDER_NN

    def slice_params(self, **kw) -> SliceParams:
        return make_slice_params(finder=self.finder_kind, projector=PointNormal2fProjectorPolar(),
                                 max_distance=self.param_max_distance_m, normal_cos=self.param_normal_cos,
                                 kd_max_leaf_range=self.param_max_leaf_range, kd_min_leaf_points=self.param_min_leaf_points, **kw)


class CorrespondenceFinderNN2D(_FinderBase):
    """registration/correspondence_finder_nn_2d.{h,cpp}: distance-map finder (one grid lookup per query)."""
    finder_kind = _capi.FINDER_DISTMAP

    def __init__(self, ctx: Context, max_distance_m: float = 1.0, resolution: float = 5e-2, normal_cos: float = 0.8):
        super().__init__(ctx)
        self.param_max_distance_m = max_distance_m
        self.param_resolution = resolution
        self.param_normal_cos = normal_cos

    def slice_params(self, **kw) -> SliceParams:
        if self.param_resolution <= 0:
            raise RuntimeError("resolution must be > 0")               # correspondence_finder_nn_2d.cpp:11-14
        if self.param_max_distance_m < 0:
            raise RuntimeError("please set max_distance_m > 0")        # :15-18
        return make_slice_params(finder=_capi.FINDER_DISTMAP, projector=PointNormal2fProjectorPolar(),
                                 max_distance=self.param_max_distance_m, resolution=self.param_resolution,
                                 normal_cos=self.param_normal_cos, **kw)


def make_slice_params(finder=FINDER_PROJECTIVE, projector: Optional[PointNormal2fProjectorPolar] = None,
                      point_distance=0.5, normal_cos=0.8, max_distance=0.5, resolution=0.05,
                      robustifier=ROBUST_NONE, chi_threshold=0.05, min_num_correspondences=10,
                      sensor_in_robot=(0.0, 0.0, 0.0), kd_max_leaf_range=1e-2, kd_min_leaf_points=20) -> SliceParams:
    sp = SliceParams()
    sp.finder = finder
    sp.projector = (projector or PointNormal2fProjectorPolar()).struct()
    sp.point_distance, sp.normal_cos, sp.max_distance, sp.resolution = point_distance, normal_cos, max_distance, resolution
    sp.robustifier, sp.chi_threshold, sp.min_num_correspondences = robustifier, chi_threshold, min_num_correspondences
    sp.sensor_in_robot = (C.c_float * 3)(*[float(v) for v in sensor_in_robot])
    sp.kd_max_leaf_range, sp.kd_min_leaf_points = float(kd_max_leaf_range), int(kd_min_leaf_points)
    return sp


@dataclasses.dataclass
class RobustifierCauchy:
    """MULTI.json:153-158"""
    param_chi_threshold: float = 0.01


class AlignerSliceProcessorLaser2D:
    """registration/aligner_slice_processor_laser_2d.h:7-17 -- finder + SE2Plane2PlaneErrorFactor (+ robustifier)."""

    def __init__(self, finder: _FinderBase, robustifier: Optional[RobustifierCauchy] = None,
                 min_num_correspondences: int = 0, fixed_slice_name: str = "points", moving_slice_name: str = "points"):
        self.param_finder = finder
        self.param_robustifier = robustifier
        self.param_min_num_correspondences = min_num_correspondences
        self.param_fixed_slice_name = fixed_slice_name
        self.param_moving_slice_name = moving_slice_name
        self.sensor_in_robot = (0.0, 0.0, 0.0)

    def slice_params(self) -> SliceParams:
        rb = self.param_robustifier
        return self.param_finder.slice_params(
            robustifier=ROBUST_CAUCHY if rb else ROBUST_NONE,
            chi_threshold=rb.param_chi_threshold if rb else 0.0,
            min_num_correspondences=self.param_min_num_correspondences, sensor_in_robot=self.sensor_in_robot)


class AlignerSliceProcessorLaser2DWithSensor(AlignerSliceProcessorLaser2D):
    """registration/aligner_slice_processor_laser_2d.h:21-42: the estimate lives in the robot frame, the
    fixed scan in the sensor frame; ``sensor_in_robot`` comes from the tf Platform in the reference
    (apps/visual_test_aligner_2d.cpp:96-107)."""

    def __init__(self, finder, sensor_in_robot=(0.0, 0.0, 0.0), **kw):
        super().__init__(finder, **kw)
        self.sensor_in_robot = tuple(float(v) for v in sensor_in_robot)


@dataclasses.dataclass
class BatchResult:
    pose: np.ndarray          # [n, 3]  movingInFixed
    information: np.ndarray   # [n, 3, 3]
    status: np.ndarray        # [n]
    iterations: np.ndarray    # [n]
    stats: Optional[np.ndarray]  # structured [n, lsm2d_stats_capacity] or None
    kernel_ms: float
    kernel_clock_mhz: float = 0.0      # clock the chip held inside the k_align launch (in-kernel stamps; 0 when not timed / another kernel ran)
    workgroup_lifetime_ms: float = 0.0  # median lifetime of the stamped workgroups
    pairs: Optional[list] = None        # want_pairs: pairs[i][s] = int32 [k, 2] (fixed_idx, moving_idx) the aligner leaves in slice s of alignment i

    def status_names(self):
        return [STATUS_NAMES.get(int(s), str(int(s))) for s in self.status]

    def last_stats(self) -> np.ndarray:
        """Statistics of the last iteration each alignment started (structured [n])."""
        if self.stats is None:
            raise RuntimeError("compute_batch(..., want_stats=True) is needed for per-alignment statistics")
        idx = np.clip(self.iterations - 1, 0, self.stats.shape[1] - 1)
        return self.stats[np.arange(len(idx)), idx]

    def loop_closure_accept(self, relocalize_min_inliers: int = 500, relocalize_max_chi_inliers: float = 0.1,
                            relocalize_min_inliers_ratio: float = 0.8) -> np.ndarray:
        """Acceptance test MultiLoopDetectorBruteForce2D applies to every candidate after relocalize_aligner
        (configurations/stage_segway_double_config_MULTI.json:964-986): aligner succeeded, inliers >= min,
        chi_inliers / inliers <= max, inliers / correspondences >= ratio.  The relocaliser uses the same test with
        700 / 0.01 / 0.75 (MULTI.json:749-769).  Returns bool [n]."""
        st = self.last_stats()
        return (self.status == 0) & _accept(st["n_inliers"], st["n_correspondences"], st["chi_inliers"], relocalize_min_inliers, relocalize_max_chi_inliers,
                                            relocalize_min_inliers_ratio)

    @classmethod
    def _from_arrays(cls, ctx: Context, arrays, timed: bool, copy: bool = False, pairs=None) -> "BatchResult":
        """The result of an aligner call from the arrays it wrote, ``(pose [n, 3], H [n, 9], status, iterations, stats or None)``: as they are, or copies
        of them.  timed: the call was a k_align launch with the context's events around it, so the three timing reads are its own."""
        if copy:
            arrays = [None if a is None else a.copy() for a in arrays]
        pose, H, status, iterations, stats = arrays
        if not timed:
            return cls(pose, H.reshape(len(pose), 3, 3), status, iterations, stats, 0.0, 0.0, 0.0, pairs)
        return cls(pose, H.reshape(len(pose), 3, 3), status, iterations, stats, ctx.last_kernel_ms(), ctx.get_option("last_kernel_clock_khz") * 1e-3,
                   ctx.get_option("last_workgroup_lifetime_ns") * 1e-6, pairs)


def _accept(n_inliers, n_correspondences, chi_inliers, min_inliers, max_chi_inliers, min_inliers_ratio) -> np.ndarray:
    """The loop detector's acceptance test in float64, on statistics: inliers >= min, chi_inliers / inliers <= max, inliers / correspondences >= ratio
    (``_select_accept`` is the device's float32 form of it).  bool [n]."""
    n_in = np.asarray(n_inliers, np.float64); n_c = np.maximum(np.asarray(n_correspondences, np.float64), 1.0)
    return (n_in >= min_inliers) & (np.asarray(chi_inliers, np.float64) / np.maximum(n_in, 1.0) <= max_chi_inliers) & (n_in / n_c >= min_inliers_ratio)


STATS_DTYPE = np.dtype([("n_correspondences", np.int32), ("n_inliers", np.int32), ("n_outliers", np.int32),
                        ("chi_inliers", np.float32), ("chi_outliers", np.float32),
                        ("pair_digest_lo", np.uint32), ("pair_digest_hi", np.uint32)])


def _result_arrays(lib, aligner_params: AlignerParams, n: int, want_stats: bool) -> tuple:
    """the arrays an aligner call of ``n`` alignments writes: (pose, H, status, iterations, stats or None), in the order of the ABI's arguments"""
    stats = np.zeros((n, int(lib.lsm2d_stats_capacity(C.byref(aligner_params)))), STATS_DTYPE) if want_stats else None
    return np.empty((n, 3), np.float32), np.empty((n, 9), np.float32), np.empty(n, np.int32), np.empty(n, np.int32), stats


def pair_digests(stats: np.ndarray) -> np.ndarray:
    """uint64 digest of every iteration's correspondence set (lsm2d_iteration_stats.pair_digest_lo / _hi)."""
    return (stats["pair_digest_hi"].astype(np.uint64) << np.uint64(32)) | stats["pair_digest_lo"].astype(np.uint64)


# what a batch descriptor (MultiAligner2D._batch) points to; the index arrays and the priors are None where the call has none
_BatchKeep = collections.namedtuple("_BatchKeep", "fixed_sets moving_sets slices fixed_handles moving_handles x0 fixed_index moving_index prior")


class MultiAligner2D:
    """The upstream aligner as the reference drives it (apps/visual_test_aligner_2d.cpp:123-156), with the
    whole iteration loop running on the device."""

    def __init__(self, ctx: Context, max_iterations: int = 10, min_num_inliers: int = 10, damping: float = 0.0,
                 termination_chi_epsilon: float = 0.0):
        self._ctx = ctx
        self.param_max_iterations = max_iterations
        self.param_min_num_inliers = min_num_inliers
        self.param_damping = damping
        # the options both shipped aligners carry at their defaults (MULTI.json:606-610,627-630,704-708,729-731); semantics in include/lsm2d.h
        # (restated from the parameters' doc strings: the upstream class is not in the reference tree).  The termination criterion exists as
        # an epsilon on the relative decay of the total chi^2 (lsm2d.h); 0 = not set = max_iterations.
        self.param_enable_inlier_only_runs = False
        self.param_keep_only_inlier_correspondences = False
        self.param_termination_chi_epsilon = termination_chi_epsilon
        self.store_correspondences = False      # compute() also fetches what the reference leaves in slice->correspondences()
        self.param_slice_processors: list[AlignerSliceProcessorLaser2D] = []
        self._fixed = {}
        self._moving = {}
        self._moving_in_fixed = np.zeros(3, np.float32)
        self._prior = None
        self._result: Optional[BatchResult] = None

    # --- single-alignment surface ---------------------------------------------------------------
    def setFixed(self, container: dict):
        """``container`` maps slice names to clouds (the PropertyContainer of the reference)."""
        self._fixed = {k: _as_cloudset(self._ctx, v) for k, v in container.items()}

    def setMoving(self, container: dict):
        self._moving = {k: _as_cloudset(self._ctx, v) for k, v in container.items()}

    def setMovingInFixed(self, pose):
        self._moving_in_fixed = np.ascontiguousarray(pose, np.float32).reshape(3)

    def setPrior(self, z, omega):
        """Odometry-prior cue (AlignerSliceOdom2DPrior, MULTI.json:402-422)."""
        self._prior = (np.asarray(z, np.float32).reshape(3), np.asarray(omega, np.float32).reshape(3, 3))

    def compute(self):
        if not self.param_slice_processors:
            raise RuntimeError("MultiAligner2D::compute| no slice processors")
        fixed = [self._fixed[s.param_fixed_slice_name] for s in self.param_slice_processors]
        moving = [self._moving[s.param_moving_slice_name] for s in self.param_slice_processors]
        prior = None if self._prior is None else [self._prior]
        self._result = self.compute_batch(fixed, moving, self._moving_in_fixed[None, :], priors=prior, want_stats=True,
                                          want_pairs=self.store_correspondences)
        return self.status()

    def correspondences(self, slice_index: int = 0) -> np.ndarray:
        """slice->correspondences() after compute() (apps/visual_test_aligner_2d.cpp:129-143): int32 [k, 2] (fixed_idx, moving_idx).
        Needs ``store_correspondences = True`` before compute(): the device loop keeps no pair lists, they cost a finder pass per slice."""
        if self._result is None or self._result.pairs is None:
            raise RuntimeError("MultiAligner2D::correspondences| set store_correspondences = True before compute()")
        return self._result.pairs[0][slice_index]

    def movingInFixed(self) -> np.ndarray:
        return self._result.pose[0]

    def informationMatrix(self) -> np.ndarray:
        return self._result.information[0]

    def status(self) -> int:
        return int(self._result.status[0])

    def iterationStats(self):
        r = self._result
        return r.stats[0][: int(r.iterations[0])]

    # --- batched surface ---------------------------------------------------------------------------
    def compute_batch(self, fixed: Sequence[CloudSet], moving: Sequence[CloudSet], init_poses, priors=None,
                      fixed_index=None, moving_index=None, want_stats: bool = False, want_pairs: bool = False) -> BatchResult:
        """``fixed[s]`` / ``moving[s]``: cloud set of slice ``s`` (one cloud = shared by the batch, else one per
        alignment or chosen through ``*_index[s][i]``).  ``init_poses``: [n, 3].  want_pairs: also the correspondences the aligner
        leaves in its slices (lsm2d_align_batch_pairs: after the aligner kernel ONE batched finder pass per slice over the alignments that started an
        iteration -- a workgroup per alignment, one wait per launch; a single alignment keeps one single-call pass per slice)."""
        ctx, lib = self._ctx, self._ctx._lib
        slices = self.param_slice_processors
        ns = len(slices)
        b, keep = self._batch(fixed, moving, init_poses, priors, fixed_index, moving_index)
        n = b.n_alignments
        ap = self._aligner_params()
        arrays = _result_arrays(lib, ap, n, want_stats)
        out = [_ptr(a) for a in arrays]
        pairs = None
        if want_pairs and n:
            cap = max([_pair_capacity(s.slice_params(), m) for s, m in zip(slices, keep.moving_sets)], default=1)
            pbuf = np.empty((n, ns, cap, 2), np.int32); pcnt = np.zeros((n, ns), np.int32)
            check(lib.lsm2d_align_batch_pairs(ctx.handle, C.byref(ap), C.byref(b), *out, _ptr(pbuf), cap, _ptr(pcnt)), "lsm2d_align_batch_pairs", ctx.handle)
            pairs = [[pbuf[i, s_, : pcnt[i, s_]].copy() for s_ in range(ns)] for i in range(n)]
        else:
            check(lib.lsm2d_align_batch(ctx.handle, C.byref(ap), C.byref(b), *out), "lsm2d_align_batch", ctx.handle)
        timed = bool(n and ctx.kernel_timing) and not pairs      # (the finder passes behind a pairs call overwrite the timed events)
        return BatchResult._from_arrays(ctx, arrays, timed, pairs=pairs)

    def _aligner_params(self) -> AlignerParams:
        """lsm2d_aligner_params of this aligner as it is configured now"""
        return AlignerParams(self.param_max_iterations, self.param_min_num_inliers, self.param_damping, self.param_termination_chi_epsilon,
                             1 if self.param_enable_inlier_only_runs else 0, 1 if self.param_keep_only_inlier_correspondences else 0)

    def _batch(self, fixed, moving, init_poses, priors=None, fixed_index=None, moving_index=None):
        """lsm2d_batch descriptor of a call, and in ``keep`` (a ``_BatchKeep``) everything it points to, to be kept alive by the caller"""
        ctx = self._ctx
        slices = self.param_slice_processors
        ns = len(slices)
        x0 = np.array(init_poses, dtype=np.float32, order="C", copy=True).reshape(-1, 3)      # the descriptor's OWN copy (round-4 advisor: PreparedBatch.set_init_poses wrote into the caller's array)
        n = len(x0)
        sp = (SliceParams * ns)(*[s.slice_params() for s in slices])
        fixed_sets = [_as_cloudset(ctx, f) for f in fixed]          # keep host-array uploads alive for the duration of the call
        moving_sets = [_as_cloudset(ctx, m) for m in moving]
        fx = (C.c_void_p * ns)(*[f.handle.value for f in fixed_sets])
        mv = (C.c_void_p * ns)(*[m.handle.value for m in moving_sets])
        fi = None if fixed_index is None else np.ascontiguousarray(fixed_index, np.int32).reshape(ns, n)
        mi = None if moving_index is None else np.ascontiguousarray(moving_index, np.int32).reshape(ns, n)
        pr = None
        if priors is not None:
            pr = (Prior * n)()
            for i, (z, om) in enumerate(priors):
                pr[i].z = (C.c_float * 3)(*np.asarray(z, np.float32).ravel())
                pr[i].omega = (C.c_float * 9)(*np.asarray(om, np.float32).ravel())
        b = Batch()
        b.n_alignments, b.n_slices = n, ns
        b.slices = sp
        b.fixed = C.cast(fx, C.POINTER(C.c_void_p)); b.moving = C.cast(mv, C.POINTER(C.c_void_p))
        b.fixed_index = C.cast(_ptr(fi), C.POINTER(C.c_int32)); b.moving_index = C.cast(_ptr(mi), C.POINTER(C.c_int32))
        b.init_pose = C.cast(_ptr(x0), C.POINTER(C.c_float))
        if pr is not None:
            b.prior = pr
        return b, _BatchKeep(fixed_sets, moving_sets, sp, fx, mv, x0, fi, mi, pr)

    def estimate_work(self, fixed, moving, init_poses, fixed_index=None, moving_index=None) -> np.ndarray:
        """lsm2d_estimate_work: per alignment, what it will cost relative to the others (chunks of the moving cloud its first iteration streams),
        without running it -- what a sweep sharded over devices or ranks balances its shards by (distributed.shard_by_work).  int32 [n]."""
        b, keep = self._batch(fixed, moving, init_poses, None, fixed_index, moving_index)
        work = np.empty(b.n_alignments, np.int32)
        check(self._ctx._lib.lsm2d_estimate_work(self._ctx.handle, C.byref(b), _ptr(work)), "lsm2d_estimate_work", self._ctx.handle)
        return work

    def prepare_batch(self, fixed, moving, init_poses, priors=None, fixed_index=None, moving_index=None, want_stats: bool = False) -> "PreparedBatch":
        """compute_batch's arguments, marshalled once: ``prepare_batch(...).run()`` == ``compute_batch(...)`` (tests), call after call."""
        return PreparedBatch(self, fixed, moving, init_poses, priors, fixed_index, moving_index, want_stats)


class PreparedBatch:
    """A batch whose descriptor, parameters and result arrays are built ONCE and handed to lsm2d_align_batch again and again -- what a host loop in the
    reference's own language does with its vectors (a candidate sweep re-aligns the same sets from new poses; the bench times the call, not the
    interpreter's marshalling of it: ~25 us of ctypes / numpy per call otherwise).  ``set_init_poses`` overwrites the start poses in place; every
    ``run()`` overwrites the result arrays of the BatchResult it returns: the results of successive runs SHARE their arrays (``run(copy=True)`` hands back
    arrays of their own).  The library keeps the placement of a batch it has seen before -- a run with unchanged sets and start poses launches no estimate
    (``Context.get_option("last_cull_estimate")`` tells)."""

    def __init__(self, aligner, fixed, moving, init_poses, priors=None, fixed_index=None, moving_index=None, want_stats: bool = False):
        self._aligner = aligner
        self._ctx = aligner._ctx
        self._b, self._keep = aligner._batch(fixed, moving, init_poses, priors, fixed_index, moving_index)
        self._x0 = self._keep.x0
        self._ap = aligner._aligner_params()
        lib = self._ctx._lib
        self._arrays = _result_arrays(lib, self._ap, self._b.n_alignments, want_stats)
        self.pose, self._H, self.status, self.iterations, self.stats = self._arrays
        self._out = tuple(_ptr(a) for a in self._arrays)
        self._args = (self._ctx.handle, C.byref(self._ap), C.byref(self._b)) + self._out
        self._fn = lib.lsm2d_align_batch
        self._pending = None      # the handle of lsm2d_align_batch_begin while the batch is in flight

    def set_init_poses(self, init_poses) -> None:
        self._x0[...] = np.asarray(init_poses, np.float32).reshape(self._x0.shape)

    def begin(self) -> None:
        """lsm2d_align_batch_begin: queue the batch and return; ``wait()`` hands its results over.  At most two batches of a context may be in flight, waited for in
        the order they were begun -- two PreparedBatch objects alternating (each keeps its own result arrays)."""
        if self._pending is not None:
            raise RuntimeError("PreparedBatch.begin: this batch is in flight already")
        h = C.c_void_p()
        check(self._ctx._lib.lsm2d_align_batch_begin(self._ctx.handle, C.byref(self._ap), C.byref(self._b), 1 if self.stats is not None else 0, C.byref(h)),
              "lsm2d_align_batch_begin", self._ctx.handle)
        self._pending = h

    def wait(self, copy: bool = False) -> BatchResult:
        if self._pending is None:
            raise RuntimeError("PreparedBatch.wait: nothing in flight")
        h, self._pending = self._pending, None
        ctx = self._ctx
        check(ctx._lib.lsm2d_align_batch_wait(h, *self._out), "lsm2d_align_batch_wait", ctx.handle)
        return BatchResult._from_arrays(ctx, self._arrays, bool(self._b.n_alignments and ctx.kernel_timing), copy)

    def run(self, copy: bool = False) -> BatchResult:
        ctx = self._ctx
        check(self._fn(*self._args), "lsm2d_align_batch", ctx.handle)
        return BatchResult._from_arrays(ctx, self._arrays, bool(self._b.n_alignments and ctx.kernel_timing), copy)


def run_pipelined(batches, copy: bool = True):
    """A queue of prepared batches with two in flight: ``begin(k)`` ; ``wait(k - 1)`` -- each asynchronously begun batch launches on its lane's own stream, so the
    younger launch's workgroups fill the slots the older one's tail leaves free (configs[1]: 0.70 ms per batch against 0.77 one at a time).  Yields the BatchResults in
    the order of the batches; every result is what ``run()`` of that batch returns, bit for bit.  Consecutive entries must be DIFFERENT PreparedBatch objects (each
    keeps its own result arrays; the same object may come again once its previous run has been yielded, i.e. two entries later)."""
    prev = None
    for b in batches:
        b.begin()
        if prev is not None:
            yield prev.wait(copy=copy)
        prev = b
    if prev is not None:
        yield prev.wait(copy=copy)


def linearize(ctx: Context, slice_params: SliceParams, fixed, moving, correspondences, pose,
              fixed_index: int = 0, moving_index: int = 0):
    """SE2Plane2PlaneErrorFactor over a correspondence vector: returns (H [3,3], b [3], IterationStats)."""
    fx, mv = _as_cloudset(ctx, fixed), _as_cloudset(ctx, moving)
    corr = np.ascontiguousarray(correspondences, np.int32).reshape(-1, 2)
    pose = np.ascontiguousarray(pose, np.float32)
    H = np.empty(9, np.float32); b = np.empty(3, np.float32); st = IterationStats()
    check(ctx._lib.lsm2d_linearize(ctx.handle, C.byref(slice_params), fx.handle, fixed_index, mv.handle, moving_index,
                                   _ptr(corr), len(corr), _ptr(pose), _ptr(H), _ptr(b), C.byref(st)), "lsm2d_linearize", ctx.handle)
    return H.reshape(3, 3), b, st


def linearize_batch(ctx: Context, slice_params: SliceParams, fixed, moving, correspondences, poses, fixed_index=None, moving_index=None):
    """``linearize`` for ``len(poses)`` independent (fixed, moving, correspondence vector, pose) items in one launch (lsm2d_linearize_batch): item ``i`` is
    between cloud ``fixed_index[i]`` of the set ``fixed`` and cloud ``moving_index[i]`` of the set ``moving`` (None: cloud ``i``, or the only cloud of a
    one-cloud set) at ``poses[i]``.  ``correspondences``: the list of int32 ``[k, 2]`` arrays ``finder.compute_batch`` returns, or a tuple
    ``(padded [n, cap, 2], counts [n])`` as lsm2d_find_correspondences_batch writes them (only the first ``counts[i]`` pairs of a row are read).
    Returns ``(H [n, 3, 3], b [n, 3], stats)``, ``stats`` a list of ``n`` IterationStats; per item the bits of ``linearize``."""
    it = _BatchItems(ctx, fixed, moving, poses, fixed_index, moving_index)
    n = it.n
    if isinstance(correspondences, tuple):
        padded, cnt = correspondences
        padded = np.ascontiguousarray(padded, np.int32)
        cnt = np.ascontiguousarray(cnt, np.int32).reshape(-1)
        if padded.ndim != 3 or padded.shape[2] != 2 or len(padded) != n or len(cnt) != n:
            raise ValueError("linearize_batch: padded correspondences must be [n, cap, 2] with n counts, n = len(poses)")
        cap = padded.shape[1]
    else:
        rows = [np.ascontiguousarray(c, np.int32).reshape(-1, 2) for c in correspondences]
        if len(rows) != n:
            raise ValueError("linearize_batch: one correspondence vector per pose")
        cnt = np.array([len(r) for r in rows], np.int32)
        cap = max(int(cnt.max()) if n else 0, 1)
        padded = np.empty((it.rows, cap, 2), np.int32)
        for i, r in enumerate(rows):
            padded[i, : len(r)] = r
    H = np.empty((it.rows, 9), np.float32); b = np.empty((it.rows, 3), np.float32); st = (IterationStats * it.rows)()
    check(ctx._lib.lsm2d_linearize_batch(*it.head(slice_params), _ptr(padded), cap, _ptr(cnt), _ptr(it.poses), _ptr(H), _ptr(b), st),
          "lsm2d_linearize_batch", ctx.handle)
    return H[:n].reshape(n, 3, 3), b[:n], [st[i] for i in range(n)]


def score_batch(ctx: Context, slice_params: SliceParams, fixed, moving, poses, fixed_index=None, moving_index=None):
    """Finder, then factor, for ``len(poses)`` pose hypotheses in one call with the pairs kept on the device (lsm2d_score_batch): item ``i`` matches cloud
    ``fixed_index[i]`` of the set ``fixed`` against cloud ``moving_index[i]`` of the set ``moving`` (None: cloud ``i``, or the only cloud of a one-cloud set)
    at ``poses[i]`` with the slice's finder and linearises what it found there.  Returns ``(H [n, 3, 3], b [n, 3], stats)``, ``stats`` a list of ``n``
    IterationStats: per item the bits of ``finder.compute_batch`` followed by ``linearize_batch``, one copy down and one wait.  ``score_accept(stats, ...)``
    applies the loop detector's acceptance test to them."""
    it = _BatchItems(ctx, fixed, moving, poses, fixed_index, moving_index)
    n = it.n
    H = np.empty((it.rows, 9), np.float32); b = np.empty((it.rows, 3), np.float32); st = (IterationStats * it.rows)()
    check(ctx._lib.lsm2d_score_batch(*it.head(slice_params), _ptr(it.poses), _ptr(H), _ptr(b), st), "lsm2d_score_batch", ctx.handle)
    return H[:n].reshape(n, 3, 3), b[:n], [st[i] for i in range(n)]


def score_accept(stats, relocalize_min_inliers: int = 500, relocalize_max_chi_inliers: float = 0.1, relocalize_min_inliers_ratio: float = 0.8) -> np.ndarray:
    """``BatchResult.loop_closure_accept``'s test (MULTI.json:964-986; the relocaliser's 700 / 0.01 / 0.75: :749-769) on the statistics ``score_batch``
    returns, minus the aligner's status, which a scored hypothesis does not have: inliers >= min, chi_inliers / inliers <= max,
    inliers / correspondences >= ratio.  Returns bool [n]."""
    st = _stats_array(stats)
    return _accept(st["n_inliers"], st["n_correspondences"], st["chi_inliers"], relocalize_min_inliers, relocalize_max_chi_inliers, relocalize_min_inliers_ratio)


@dataclasses.dataclass
class SelectParams:
    """lsm2d_select_params: the thresholds of the candidate loops' acceptance test.  The class defaults are the loop detector's (MULTI.json:964-986),
    ``relocalizer()`` gives the relocaliser's (:749-769)."""
    min_inliers: int = 500
    max_chi_per_inlier: float = 0.1
    min_inlier_ratio: float = 0.8

    @classmethod
    def relocalizer(cls) -> "SelectParams":
        return cls(700, 0.01, 0.75)

    def struct(self) -> _capi.SelectParamsC:
        return _capi.SelectParamsC(int(self.min_inliers), float(self.max_chi_per_inlier), float(self.min_inlier_ratio))


def _stats_array(stats) -> np.ndarray:
    """a list of IterationStats or a structured array as a structured STATS_DTYPE array [n]"""
    if isinstance(stats, np.ndarray):
        return stats.reshape(-1)
    out = np.zeros(len(stats), STATS_DTYPE)
    for i, s in enumerate(stats):
        out[i] = (s.n_correspondences, s.n_inliers, s.n_outliers, s.chi_inliers, s.chi_outliers, s.pair_digest_lo, s.pair_digest_hi)
    return out


def _select_accept(st: np.ndarray, select: SelectParams) -> np.ndarray:
    """lsm2d_score_select's acceptance test in numpy float32 (IEEE division, like the kernel's): bool [n]; a NaN on either side of a comparison rejects"""
    n_in = st["n_inliers"].astype(np.float32)
    n_c = np.maximum(st["n_correspondences"], 1).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        per_inlier = st["chi_inliers"].astype(np.float32) / np.maximum(n_in, np.float32(1.0))
        ratio = n_in / n_c
        return (st["n_inliers"] >= np.int32(select.min_inliers)) & (per_inlier <= np.float32(select.max_chi_per_inlier)) & \
               (ratio >= np.float32(select.min_inlier_ratio))


def score_rank(stats, select: SelectParams, k: int, active=None):
    """lsm2d_score_select's acceptance test and ranking on statistics the caller already holds (from ``score_batch``, an aligner or the oracle), in numpy
    float32 / integer arithmetic: accepted are the items with inliers >= min, chi_inliers / max(inliers, 1) <= max and inliers / max(correspondences, 1) >=
    ratio; they are ranked by inliers descending, then chi_inliers ascending on its bit pattern as uint32, then index ascending.  ``stats``: a list of
    IterationStats or a structured STATS_DTYPE array.  ``active`` (``score_aligner``'s, optional): an item whose count is 0 is rejected whatever the
    thresholds are, as lsm2d_score_aligner_select rejects it.  Returns ``(index int32 [min(k, n_accepted)], n_accepted)``."""
    if k < 1:
        raise ValueError("score_rank: k must be >= 1")
    st = _stats_array(stats)
    acc = _select_accept(st, select)
    if active is not None:
        acc = acc & (np.asarray(active).reshape(-1) > 0)
    ok = np.flatnonzero(acc)
    key = ((np.uint64(0x7fffffff) - st["n_inliers"][ok].astype(np.uint64)) << np.uint64(32)) | \
        np.ascontiguousarray(st["chi_inliers"][ok], np.float32).view(np.uint32).astype(np.uint64)
    order = np.lexsort((ok, key))      # by key, ties by index
    return ok[order][:k].astype(np.int32), int(len(ok))


def score_select(ctx: Context, slice_params: SliceParams, fixed, moving, poses, select: SelectParams, k: int, fixed_index=None, moving_index=None):
    """``score_batch``'s scoring, then the acceptance test and the best ``k`` accepted hypotheses ranked on the device (lsm2d_score_select): only ``k`` rows
    come down, with one copy and one wait.  Returns ``(index int32 [m], H [m, 3, 3], b [m, 3], stats structured STATS_DTYPE [m], n_accepted)``,
    ``m = min(k, n_accepted)``, best first: ``index`` is what ``score_rank`` gives on ``score_batch``'s statistics, the rows are ``score_batch``'s for
    those items, bit for bit."""
    it = _BatchItems(ctx, fixed, moving, poses, fixed_index, moving_index)
    kk = max(int(k), 1)
    index = np.empty(kk, np.int32); H = np.empty((kk, 9), np.float32); b = np.empty((kk, 3), np.float32); st = np.zeros(kk, STATS_DTYPE)
    n_sel = C.c_int32(0); n_acc = C.c_int32(0)
    sel = select.struct()
    check(ctx._lib.lsm2d_score_select(*it.head(slice_params), _ptr(it.poses), C.byref(sel), int(k), _ptr(index), _ptr(H), _ptr(b), _ptr(st), C.byref(n_sel),
                                      C.byref(n_acc)),
          "lsm2d_score_select", ctx.handle)
    m = n_sel.value
    return index[:m], H[:m].reshape(m, 3, 3), b[:m], st[:m], n_acc.value


def score_aligner(aligner: "MultiAligner2D", fixed, moving, poses, priors=None, fixed_index=None, moving_index=None):
    """``len(poses)`` pose hypotheses scored against the whole aligner -- every slice with its sensor offset and ``min_num_correspondences``, the optional
    prior per hypothesis -- in one call with one wait (lsm2d_score_aligner_batch): what the first iteration of ``aligner.compute_batch`` holds just before
    its solve.  ``fixed[s]`` / ``moving[s]``, ``priors``, ``*_index[s][i]``: as ``compute_batch`` takes them.  Returns ``(H [n, 3, 3], b [n, 3], stats
    structured STATS_DTYPE [n], active int32 [n])``; ``active[i]`` counts the slices that contributed (0: zeros, the hypothesis an aligner would end with
    NotEnoughCorrespondences).  With ``"sum_order"`` 1 an item is the sequential oracle's ``align(max_iterations=1)`` bit for bit."""
    ctx = aligner._ctx
    bd, keep = aligner._batch(fixed, moving, poses, priors, fixed_index, moving_index)      # (keep: what bd points to, alive until this function returns)
    n = bd.n_alignments; rows = max(n, 1)
    H = np.empty((rows, 9), np.float32); b = np.empty((rows, 3), np.float32); st = np.zeros(rows, STATS_DTYPE); active = np.zeros(rows, np.int32)
    check(ctx._lib.lsm2d_score_aligner_batch(ctx.handle, C.byref(bd), _ptr(H), _ptr(b), _ptr(st), _ptr(active)), "lsm2d_score_aligner_batch", ctx.handle)
    return H[:n].reshape(n, 3, 3), b[:n], st[:n], active[:n]


def score_aligner_select(aligner: "MultiAligner2D", fixed, moving, poses, select: SelectParams, k: int, priors=None, fixed_index=None, moving_index=None):
    """``score_aligner``'s scoring, then the acceptance test and the best ``k`` accepted hypotheses ranked on the device (lsm2d_score_aligner_select); a
    hypothesis no slice contributed to is rejected.  Returns ``(index int32 [m], H [m, 3, 3], b [m, 3], stats [m], active int32 [m], n_accepted)``,
    ``m = min(k, n_accepted)``, best first: ``index`` is ``score_rank(stats, select, k, active)`` on ``score_aligner``'s results, the rows are its rows."""
    ctx = aligner._ctx
    bd, keep = aligner._batch(fixed, moving, poses, priors, fixed_index, moving_index)      # (keep: as in score_aligner)
    kk = max(int(k), 1)
    index = np.empty(kk, np.int32); H = np.empty((kk, 9), np.float32); b = np.empty((kk, 3), np.float32); st = np.zeros(kk, STATS_DTYPE)
    active = np.zeros(kk, np.int32)
    n_sel = C.c_int32(0); n_acc = C.c_int32(0)
    sel = select.struct()
    check(ctx._lib.lsm2d_score_aligner_select(ctx.handle, C.byref(bd), C.byref(sel), int(k), _ptr(index), _ptr(H), _ptr(b), _ptr(st), _ptr(active),
                                              C.byref(n_sel), C.byref(n_acc)), "lsm2d_score_aligner_select", ctx.handle)
    m = n_sel.value
    return index[:m], H[:m].reshape(m, 3, 3), b[:m], st[:m], active[:m], n_acc.value


def last_stats_rows(iterations, stats) -> np.ndarray:
    """Row ``iterations[i] - 1`` of every candidate's statistics ``[n, capacity]`` -- the last iteration it started -- as a structured STATS_DTYPE array
    ``[n]``; a candidate that started none gets zeros (lsm2d_sweep_align's ``out_last_stats``).  ``stats`` of one dimension is taken as those rows already."""
    its = np.asarray(iterations, np.int64).reshape(-1)
    st = np.asarray(stats)
    if st.ndim == 1:
        last = st.copy()
    else:
        last = st[np.arange(len(its)), np.clip(its - 1, 0, st.shape[1] - 1)] if len(its) else np.zeros(0, STATS_DTYPE)
    last[its < 1] = np.zeros(1, STATS_DTYPE)[0]
    return last


def align_rank(status, iterations, stats, select: SelectParams, k: int):
    """lsm2d_align_select's acceptance test and ranking on results the caller already holds (a ``BatchResult``'s or the oracle's), in numpy float32 /
    integer arithmetic: candidate i is accepted when ``status[i] == 0``, ``iterations[i] >= 1`` and ``_select_accept`` passes on row ``iterations[i] - 1``
    of its statistics; the accepted are ranked by ``score_rank``'s key on that row -- inliers descending, chi_inliers ascending on its bit pattern, index
    ascending.  ``stats``: structured ``[n, capacity]`` (every iteration's rows) or ``[n]`` (the last rows).  Returns ``(index int32 [min(k, n_accepted)],
    n_accepted, n_success)``."""
    status = np.asarray(status).reshape(-1); its = np.asarray(iterations).reshape(-1)
    ok = (status == 0) & (its >= 1)
    index, n_acc = score_rank(last_stats_rows(its, stats), select, k, active=ok.astype(np.int32))
    return index, n_acc, int(np.count_nonzero(status == 0))


@dataclasses.dataclass
class AlignSelectResult:
    index: np.ndarray          # int32 [m]: the selected candidates, best first; m = min(k, n_accepted)
    pose: np.ndarray           # [m, 3]: compute_batch's pose of candidate index[j]
    information: np.ndarray    # [m, 3, 3]
    iterations: np.ndarray     # int32 [m]
    last_stats: np.ndarray     # structured [m]: the statistics of the last iteration each started
    n_accepted: int            # candidates whose aligner succeeded and whose last iteration passes the thresholds, of all
    n_success: int             # candidates whose aligner succeeded, of all
    kernel_ms: float = 0.0     # the aligner's launch plus the selection (0 when the context is not timed)


def align_select(aligner: "MultiAligner2D", fixed, moving, init_poses, select: SelectParams, k: int, priors=None, fixed_index=None,
                 moving_index=None) -> AlignSelectResult:
    """``aligner.compute_batch(..., want_stats=True)``'s alignment, then the candidate loops' verdict made on the device (lsm2d_align_select): aligner
    succeeded, the last started iteration passes ``select``, the best ``k`` of those ranked -- ``k`` rows come down with one copy and one wait, not every
    iteration's statistics of every candidate.  ``index`` is ``align_rank`` on ``compute_batch``'s results, the rows are its rows, bit for bit."""
    ctx = aligner._ctx
    bd, keep = aligner._batch(fixed, moving, init_poses, priors, fixed_index, moving_index)      # (keep: what bd points to, alive until this function returns)
    ap = aligner._aligner_params()
    kk = max(int(k), 1)
    index = np.empty(kk, np.int32); pose = np.empty((kk, 3), np.float32); H = np.empty((kk, 9), np.float32); its = np.empty(kk, np.int32)
    st = np.zeros(kk, STATS_DTYPE)
    n_sel = C.c_int32(0); n_acc = C.c_int32(0); n_suc = C.c_int32(0)
    sel = select.struct()
    check(ctx._lib.lsm2d_align_select(ctx.handle, C.byref(ap), C.byref(bd), C.byref(sel), int(k), _ptr(index), _ptr(pose), _ptr(H), _ptr(its), _ptr(st),
                                      C.byref(n_sel), C.byref(n_acc), C.byref(n_suc)), "lsm2d_align_select", ctx.handle)
    m = n_sel.value
    ms = ctx.last_kernel_ms() if (bd.n_alignments and ctx.kernel_timing) else 0.0
    return AlignSelectResult(index[:m], pose[:m], H[:m].reshape(m, 3, 3), its[:m], st[:m], n_acc.value, n_suc.value, ms)


# ---- the select calls per GROUP of the batch: a fleet's candidates, the best k per robot (lsm2d_*_select_grouped) ----

def _group_offsets(offsets) -> np.ndarray:
    """``offsets`` as the contiguous int32 array the C calls take (n_groups + 1 values; the calls check the rest)"""
    return np.ascontiguousarray(offsets, np.int32).reshape(-1)


def _ragged(a: np.ndarray, n_sel: np.ndarray, k: int) -> list:
    """views ``a[g * k : g * k + n_sel[g]]`` of an array of n_groups x k rows, one per group"""
    return [a[g * k: g * k + int(m)] for g, m in enumerate(n_sel)]


def score_rank_grouped(stats, offsets, select: SelectParams, k: int, active=None):
    """``score_rank`` per group: group ``g`` is items ``offsets[g] .. offsets[g + 1]`` and is ranked on its own, its indices shifted by ``offsets[g]`` so
    that they are batch item indices.  The restatement the grouped select calls are held to.  Returns ``(index: list of int32 arrays, one per group,
    n_accepted int32 [n_groups])``."""
    st = _stats_array(stats); off = _group_offsets(offsets)
    act = None if active is None else np.asarray(active).reshape(-1)
    index, n_acc = [], np.zeros(len(off) - 1, np.int32)
    for g in range(len(off) - 1):
        lo, hi = int(off[g]), int(off[g + 1])
        idx, n_acc[g] = score_rank(st[lo:hi], select, k, None if act is None else act[lo:hi])
        index.append((idx + np.int32(lo)).astype(np.int32))
    return index, n_acc


def align_rank_grouped(status, iterations, stats, offsets, select: SelectParams, k: int):
    """``align_rank`` per group, indices shifted by the group's offset.  Returns ``(index: list of int32 arrays, one per group, n_accepted int32
    [n_groups], n_success int32 [n_groups])``."""
    status = np.asarray(status).reshape(-1); its = np.asarray(iterations).reshape(-1); st = np.asarray(stats); off = _group_offsets(offsets)
    index, n_acc, n_suc = [], np.zeros(len(off) - 1, np.int32), np.zeros(len(off) - 1, np.int32)
    for g in range(len(off) - 1):
        lo, hi = int(off[g]), int(off[g + 1])
        idx, n_acc[g], n_suc[g] = align_rank(status[lo:hi], its[lo:hi], st[lo:hi], select, k)
        index.append((idx + np.int32(lo)).astype(np.int32))
    return index, n_acc, n_suc


def score_select_grouped(ctx: Context, slice_params: SliceParams, fixed, moving, poses, offsets, select: SelectParams, k: int, fixed_index=None,
                         moving_index=None):
    """``score_select`` per group of the batch in ONE call with one copy down and one wait (lsm2d_score_select_grouped): group ``g`` is hypotheses
    ``offsets[g] .. offsets[g + 1]``, and its block is what ``score_select`` returns for that sub-batch, with batch item indices.  Returns ``(index, H, b,
    stats, n_accepted)``: the first four are lists with one entry per group (views of ``m_g = min(k, n_accepted[g])`` rows, best first), ``n_accepted``
    int32 ``[n_groups]``."""
    it = _BatchItems(ctx, fixed, moving, poses, fixed_index, moving_index)
    off = _group_offsets(offsets); G = max(len(off) - 1, 0); kk = max(int(k), 1); rows = max(G, 1) * kk
    index = np.empty(rows, np.int32); H = np.empty((rows, 3, 3), np.float32); b = np.empty((rows, 3), np.float32); st = np.zeros(rows, STATS_DTYPE)
    n_sel = np.zeros(max(G, 1), np.int32); n_acc = np.zeros(max(G, 1), np.int32)
    sel = select.struct()
    check(ctx._lib.lsm2d_score_select_grouped(*it.head(slice_params), _ptr(it.poses), C.byref(sel), int(k), G, _ptr(off), _ptr(index), _ptr(H), _ptr(b),
                                              _ptr(st), _ptr(n_sel), _ptr(n_acc)), "lsm2d_score_select_grouped", ctx.handle)
    n_sel = n_sel[:G]
    return _ragged(index, n_sel, kk), _ragged(H, n_sel, kk), _ragged(b, n_sel, kk), _ragged(st, n_sel, kk), n_acc[:G]


def score_aligner_select_grouped(aligner: "MultiAligner2D", fixed, moving, poses, offsets, select: SelectParams, k: int, priors=None, fixed_index=None,
                                 moving_index=None):
    """``score_aligner_select`` per group of the batch in one call (lsm2d_score_aligner_select_grouped).  Returns ``(index, H, b, stats, active,
    n_accepted)``: lists with one entry per group, and ``n_accepted`` int32 ``[n_groups]``."""
    ctx = aligner._ctx
    bd, keep = aligner._batch(fixed, moving, poses, priors, fixed_index, moving_index)      # (keep: what bd points to, alive until this function returns)
    off = _group_offsets(offsets); G = max(len(off) - 1, 0); kk = max(int(k), 1); rows = max(G, 1) * kk
    index = np.empty(rows, np.int32); H = np.empty((rows, 3, 3), np.float32); b = np.empty((rows, 3), np.float32); st = np.zeros(rows, STATS_DTYPE)
    active = np.zeros(rows, np.int32)
    n_sel = np.zeros(max(G, 1), np.int32); n_acc = np.zeros(max(G, 1), np.int32)
    sel = select.struct()
    check(ctx._lib.lsm2d_score_aligner_select_grouped(ctx.handle, C.byref(bd), C.byref(sel), int(k), G, _ptr(off), _ptr(index), _ptr(H), _ptr(b), _ptr(st),
                                                      _ptr(active), _ptr(n_sel), _ptr(n_acc)), "lsm2d_score_aligner_select_grouped", ctx.handle)
    n_sel = n_sel[:G]
    return _ragged(index, n_sel, kk), _ragged(H, n_sel, kk), _ragged(b, n_sel, kk), _ragged(st, n_sel, kk), _ragged(active, n_sel, kk), n_acc[:G]


@dataclasses.dataclass
class AlignSelectGroupedResult:
    index: list                # per group: int32 [m_g], the group's selected candidates as BATCH indices, best first; m_g = min(k, n_accepted[g])
    pose: list                 # per group: [m_g, 3]
    information: list          # per group: [m_g, 3, 3]
    iterations: list           # per group: int32 [m_g]
    last_stats: list           # per group: structured [m_g]
    n_accepted: np.ndarray     # int32 [n_groups]
    n_success: np.ndarray      # int32 [n_groups]
    kernel_ms: float = 0.0     # the aligner's launch plus the selection (0 when the context is not timed)


def align_select_grouped(aligner: "MultiAligner2D", fixed, moving, init_poses, offsets, select: SelectParams, k: int, priors=None, fixed_index=None,
                         moving_index=None) -> AlignSelectGroupedResult:
    """``align_select`` per group of the batch -- every robot's own candidates, its own verdict -- in ONE call with one copy down and one wait
    (lsm2d_align_select_grouped): group ``g``'s entries are what ``align_select`` returns for candidates ``offsets[g] .. offsets[g + 1]`` alone, with batch
    indices; ``align_rank_grouped`` on ``compute_batch``'s results restates it."""
    ctx = aligner._ctx
    bd, keep = aligner._batch(fixed, moving, init_poses, priors, fixed_index, moving_index)      # (keep: what bd points to, alive until this function returns)
    ap = aligner._aligner_params()
    off = _group_offsets(offsets); G = max(len(off) - 1, 0); kk = max(int(k), 1); rows = max(G, 1) * kk
    index = np.empty(rows, np.int32); pose = np.empty((rows, 3), np.float32); H = np.empty((rows, 3, 3), np.float32); its = np.empty(rows, np.int32)
    st = np.zeros(rows, STATS_DTYPE)
    n_sel = np.zeros(max(G, 1), np.int32); n_acc = np.zeros(max(G, 1), np.int32); n_suc = np.zeros(max(G, 1), np.int32)
    sel = select.struct()
    check(ctx._lib.lsm2d_align_select_grouped(ctx.handle, C.byref(ap), C.byref(bd), C.byref(sel), int(k), G, _ptr(off), _ptr(index), _ptr(pose), _ptr(H),
                                              _ptr(its), _ptr(st), _ptr(n_sel), _ptr(n_acc), _ptr(n_suc)), "lsm2d_align_select_grouped", ctx.handle)
    n_sel = n_sel[:G]
    ms = ctx.last_kernel_ms() if (bd.n_alignments and ctx.kernel_timing) else 0.0
    return AlignSelectGroupedResult(_ragged(index, n_sel, kk), _ragged(pose, n_sel, kk), _ragged(H, n_sel, kk), _ragged(its, n_sel, kk),
                                    _ragged(st, n_sel, kk), n_acc[:G], n_suc[:G], ms)


@dataclasses.dataclass
class RelocalizeResult:
    index: np.ndarray          # int32 [m]: the selected hypotheses, best first
    score_stats: np.ndarray    # structured [m]: their statistics at their own poses
    n_accepted: int            # hypotheses that passed the acceptance test, of all
    result: BatchResult        # the aligner's results for the selected hypotheses, started from their own poses
    accepted: np.ndarray       # bool [m]: aligner succeeded and the aligned statistics pass the acceptance test


def relocalize(aligner: MultiAligner2D, fixed, moving, poses, select: SelectParams, k: int, fixed_index=None, moving_index=None, priors=None) -> RelocalizeResult:
    """The candidate loop of the relocaliser / loop detector (MULTI.json:749-769, :964-986) over ``len(poses)`` hypotheses: ``score_select`` with the
    aligner's (one) slice, then ``aligner.compute_batch`` on the selected hypotheses from their own poses, then the acceptance test on the statistics of
    the last iteration each started.  Pure composition: the same as calling the two entry points by hand.
    An aligner with several slices and / or ``priors`` (one ``(z, omega)`` per hypothesis) takes ``fixed`` / ``moving`` as lists of sets, one per slice
    (``*_index``: ``[n_slices][n]``), scores with ``score_aligner_select`` and hands the selected hypotheses' priors on to the aligner."""
    ctx = aligner._ctx
    ns = len(aligner.param_slice_processors)
    if ns < 1:
        raise ValueError("relocalize: the aligner has no slice")
    whole_aligner = ns != 1 or priors is not None or isinstance(fixed, (list, tuple)) or isinstance(moving, (list, tuple))
    as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]
    fx = [_as_cloudset(ctx, f) for f in as_list(fixed)]; mv = [_as_cloudset(ctx, m) for m in as_list(moving)]
    if len(fx) != ns or len(mv) != ns:
        raise ValueError("relocalize: one fixed and one moving set per slice of the aligner")
    x = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
    n = len(x)
    if priors is not None and len(priors) != n:
        raise ValueError("relocalize: one prior per hypothesis")
    fi = None if fixed_index is None else np.ascontiguousarray(fixed_index, np.int32).reshape(ns, n)      # (one slice without priors: the [1, n] case)
    mi = None if moving_index is None else np.ascontiguousarray(moving_index, np.int32).reshape(ns, n)
    if whole_aligner:
        index, _, _, st, _, n_acc = score_aligner_select(aligner, fx, mv, x, select, k, priors, fi, mi)
    else:
        index, _, _, st, n_acc = score_select(ctx, aligner.param_slice_processors[0].slice_params(), fx[0], mv[0], x, select, k, fi, mi)
    if not len(index):      # nothing passed: nothing to align
        z = np.zeros
        return RelocalizeResult(index, st, n_acc, BatchResult(z((0, 3), np.float32), z((0, 3, 3), np.float32), z(0, np.int32), z(0, np.int32), None, 0.0), z(0, bool))

    def chosen(sets, idx):      # the selected items' clouds, spelled out for every slice: NULL means "cloud i" only while the batch is the whole set
        if idx is None and all(cs.n_clouds == 1 for cs in sets):
            return None
        rows = []
        for s_, cs in enumerate(sets):
            full = idx[s_] if idx is not None else (np.zeros(n, np.int32) if cs.n_clouds == 1 else np.arange(n, dtype=np.int32))
            rows.append(full[index])
        return np.stack(rows)

    pr = None if priors is None else [priors[int(i)] for i in index]
    res = aligner.compute_batch(fx, mv, x[index], priors=pr, fixed_index=chosen(fx, fi), moving_index=chosen(mv, mi), want_stats=True)
    return RelocalizeResult(index, st, n_acc, res, (res.status == 0) & _select_accept(res.last_stats(), select))


class SceneClipperProjective2D:
    """mapping/scene_clipper_projective_2d.{h,cpp}: keeps what the sensor sees of the local map, at most one point per projector
    column, in the robot frame; ``voxelize_resolution`` > 0 additionally voxelises the clipped cloud (.cpp:36-48; both shipped configs
    use 0, MULTI.json:673-683).  The clipped scene stays on the device (a reserved CloudSet) and is what the tracker hands to the
    aligner as ``moving``."""

    def __init__(self, ctx: Context, projector: Optional[PointNormal2fProjectorPolar] = None, voxelize_resolution: float = 0.1,
                 asynchronous: bool = False):
        self._ctx = ctx
        self.param_projector = projector
        self.param_voxelize_resolution = voxelize_resolution
        # asynchronous: compute() only queues the work -- nothing is copied back (source_indices stays empty) and the clipped
        # set's size is fetched when somebody reads it; the aligner and the merger take such a set as it is
        self.asynchronous = asynchronous
        self._full_scene = None
        self._clipped = None
        self._robot_in_local_map = np.zeros(3, np.float32)
        self._sensor_in_robot = np.zeros(3, np.float32)
        self.source_indices = np.zeros(0, np.int32)

    def setFullScene(self, scene):
        self._full_scene = _as_cloudset(self._ctx, scene)

    def setClippedSceneInRobot(self, clipped: CloudSet):
        self._clipped = clipped

    def setRobotInLocalMap(self, pose):
        self._robot_in_local_map = np.ascontiguousarray(pose, np.float32).reshape(3)

    def setSensorInRobot(self, pose):
        self._sensor_in_robot = np.ascontiguousarray(pose, np.float32).reshape(3)

    def compute(self) -> CloudSet:
        if self._full_scene is None:
            raise RuntimeError("SceneClipperProjective2D::compute| missing local OR global scene")
        if self.param_projector is None:
            raise RuntimeError("SceneClipperProjective2D::compute| Missing Projector")
        cols = self.param_projector.param_canvas_cols
        if self._clipped is None:
            self._clipped = CloudSet.reserved(self._ctx, cols)
        pr = self.param_projector.struct()
        vox = float(self.param_voxelize_resolution)
        lib = self._ctx._lib
        args = (self._ctx.handle, C.byref(pr), self._full_scene.handle, 0, _ptr(self._robot_in_local_map), _ptr(self._sensor_in_robot))

        def call(out_n, out_src):      # voxelize_resolution > 0: the branch of scene_clipper_projective_2d.cpp:36-48 (no source indices)
            if vox > 0:
                return check(lib.lsm2d_clip_scene_voxelized(*args, vox, self._clipped.handle, out_n, None), "lsm2d_clip_scene_voxelized", self._ctx.handle)
            return check(lib.lsm2d_clip_scene(*args, self._clipped.handle, out_n, out_src), "lsm2d_clip_scene", self._ctx.handle)

        if self.asynchronous:
            call(None, None)
            self._clipped._set_pending()
            self.source_indices = np.zeros(0, np.int32)
            return self._clipped
        n = C.c_int32(0); src = np.empty(cols, np.int32)
        call(C.byref(n), _ptr(src))
        self._clipped._set_count(n.value)
        self.source_indices = src[: n.value].copy() if not vox > 0 else np.zeros(0, np.int32)
        return self._clipped

    def compute_batch(self, scenes: CloudSet, robot_in_local_map, clipped: CloudSet, scene_index=None):
        """compute() for N trackers at once, in one launch (lsm2d_clip_scene_batch; ``voxelize_resolution`` > 0:
        lsm2d_clip_scene_voxelized_batch, the branch of .cpp:36-48 per tracker, canvas_cols <= 2048): tracker i clips cloud
        ``scene_index[i]`` (None: i) of ``scenes`` at ``robot_in_local_map[i]`` * the sensor offset into cloud i of ``clipped`` (a
        ``CloudSet.reserved_many`` of >= N clouds of >= canvas_cols points).  Returns the N sizes, or None when asynchronous."""
        if self.param_projector is None:
            raise RuntimeError("SceneClipperProjective2D::compute| Missing Projector")
        poses = np.ascontiguousarray(robot_in_local_map, np.float32).reshape(-1, 3)
        n = len(poses)
        idx = None if scene_index is None else np.ascontiguousarray(scene_index, np.int32).ravel()
        pr = self.param_projector.struct()
        vox = float(self.param_voxelize_resolution)
        out = None if self.asynchronous else np.empty(n, np.int32)
        lib = self._ctx._lib
        head = (self._ctx.handle, C.byref(pr), scenes.handle, n, _ptr(idx), _ptr(poses), _ptr(self._sensor_in_robot))
        tail = (clipped.handle, _ptr(out))
        if vox > 0:
            check(lib.lsm2d_clip_scene_voxelized_batch(*head, vox, *tail), "lsm2d_clip_scene_voxelized_batch", self._ctx.handle)
        else:
            check(lib.lsm2d_clip_scene_batch(*head, *tail), "lsm2d_clip_scene_batch", self._ctx.handle)
        clipped._set_pending()
        return out


class MergerProjective2D:
    """mapping/merger_projective_2d.{h,cpp}: folds a measurement into the device-resident scene, in place."""

    def __init__(self, ctx: Context, projector: Optional[PointNormal2fProjectorPolar] = None, merge_threshold: float = 0.2,
                 asynchronous: bool = False):
        self._ctx = ctx
        self.param_projector = projector
        self.param_merge_threshold = merge_threshold
        self.asynchronous = asynchronous      # compute() only queues the merge; the scene's new size is fetched when it is read
        self._scene = None
        self._measurement = None
        self._measurement_in_scene = np.zeros(3, np.float32)
        self.counts = (0, 0, 0)      # new, merged, replaced

    def setScene(self, scene: CloudSet):
        self._scene = scene

    def setMeasurement(self, measurement, index: int = 0):
        self._measurement = _as_cloudset(self._ctx, measurement); self._measurement_index = index

    def setMeasurementInScene(self, pose):
        self._measurement_in_scene = np.ascontiguousarray(pose, np.float32).reshape(3)

    def compute(self) -> int:
        if self.param_projector is None:
            raise RuntimeError("MergerProjective2D::compute| Missing Projector")
        if self._scene is None or self._measurement is None:
            raise RuntimeError("MergerProjective2D::compute| missing scene or measurement")
        pr = self.param_projector.struct()
        size, counts = self._outputs(1)
        check(self._ctx._lib.lsm2d_merge_scene(self._ctx.handle, C.byref(pr), self._scene.handle, self._measurement.handle, self._measurement_index,
                                               _ptr(self._measurement_in_scene), float(self.param_merge_threshold), None if size is None else C.byref(size), counts),
              "lsm2d_merge_scene", self._ctx.handle)
        self.counts = (0, 0, 0) if counts is None else tuple(counts)
        return self._scene_size(size)

    def _outputs(self, n_measurements: int):
        """What lsm2d_merge_scene / _scenes write when somebody waits for it: the scene's new size and one (new, merged, replaced) triple per measurement.
        Asynchronous: nobody waits, None (NULL) both."""
        return (None, None) if self.asynchronous else (C.c_int32(0), (C.c_int32 * (3 * n_measurements))())

    def _scene_size(self, size) -> int:
        """tells the scene its new size -- or, asynchronous, that the device alone knows it (-1)"""
        if size is None:
            self._scene._set_pending()
            return -1
        self._scene._set_count(size.value)
        return size.value

    def compute_all(self, measurements: Sequence, poses, indices: Optional[Sequence[int]] = None) -> int:
        """Merges several measurements, each at its own pose in the scene, in the given order -- what one setMeasurement /
        setMeasurementInScene / compute() round per measurement does, as ONE call (lsm2d_merge_scenes: one launch when the scene and
        the measurements are small).  Returns the scene's new size (-1 when asynchronous); ``counts`` then holds one triple per measurement."""
        if self.param_projector is None:
            raise RuntimeError("MergerProjective2D::compute| Missing Projector")
        if self._scene is None or not len(measurements):
            raise RuntimeError("MergerProjective2D::compute| missing scene or measurement")
        sets = [_as_cloudset(self._ctx, m) for m in measurements]
        n = len(sets)
        handles = (C.c_void_p * n)(*[s_.handle for s_ in sets])
        p = np.ascontiguousarray(poses, np.float32).reshape(n, 3)
        idx = None if indices is None else (C.c_int32 * n)(*[int(i) for i in indices])      # which cloud of each (multi-cloud) set
        pr = self.param_projector.struct()
        size, counts = self._outputs(n)
        check(self._ctx._lib.lsm2d_merge_scenes(self._ctx.handle, C.byref(pr), self._scene.handle, n, handles, idx, _ptr(p), float(self.param_merge_threshold),
                                                None if size is None else C.byref(size), counts), "lsm2d_merge_scenes", self._ctx.handle)
        self.counts = (0, 0, 0) if counts is None else [tuple(counts[3 * k:3 * k + 3]) for k in range(n)]
        return self._scene_size(size)

    def compute_batch(self, scenes: CloudSet, measurements: Sequence[CloudSet], poses, scene_index=None, meas_index=None):
        """compute_all() for N trackers at once (lsm2d_merge_scene_batch): cloud ``scene_index[i]`` (None: i) of the ``reserved_many``
        set ``scenes`` gets cloud ``meas_index[k][i]`` (None: i) of ``measurements[k]``, k = 0 .. K-1 (K <= 4), in order, at ``poses[i][k]``.
        Returns the N new sizes (``counts``: [N][K][3] new, merged, replaced), or None when asynchronous."""
        if self.param_projector is None:
            raise RuntimeError("MergerProjective2D::compute| Missing Projector")
        k = len(measurements)
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, k, 3)
        n = len(p)
        handles = (C.c_void_p * max(k, 1))(*[m.handle.value for m in measurements])
        sidx = None if scene_index is None else np.ascontiguousarray(scene_index, np.int32).ravel()
        midx = None if meas_index is None else np.ascontiguousarray(meas_index, np.int32).reshape(k, n)
        pr = self.param_projector.struct()
        sizes = None if self.asynchronous else np.empty(n, np.int32)
        counts = None if self.asynchronous else np.empty((n, k, 3), np.int32)
        check(self._ctx._lib.lsm2d_merge_scene_batch(self._ctx.handle, C.byref(pr), scenes.handle, n, _ptr(sidx), k, handles, _ptr(midx), _ptr(p),
                                                     float(self.param_merge_threshold), _ptr(sizes), _ptr(counts)), "lsm2d_merge_scene_batch", self._ctx.handle)
        scenes._set_pending()
        self.counts = counts
        return sizes


class RawDataPreprocessorProjective2D:
    """sensor_processing/raw_data_preprocessor_projective_2d.{h,cpp}: LaserMessage ranges -> PointNormal2fVectorCloud
    (polar unprojection, sliding-window normals, voxelisation), batched over scans; the clouds stay on the device."""

    def __init__(self, ctx: Context, range_min: float = 0.0, range_max: float = 1000.0, voxelize_resolution: float = 0.02,
                 normal_point_distance: float = 0.3, normal_min_points: int = 5):
        self._ctx = ctx
        self.param_range_min = range_min                    # .h:39
        self.param_range_max = range_max                    # .h:40
        self.param_voxelize_resolution = voxelize_resolution  # .h:41-45
        self.param_normal_point_distance = normal_point_distance   # NormalComputator1DSlidingWindow (MULTI.json:845-853)
        self.param_normal_min_points = normal_min_points
        self._msg = None
        self._meas: Optional[CloudSet] = None

    def setRawData(self, ranges, angle_min: float, angle_max: float, range_min: float = 0.0, range_max: float = float("inf")) -> bool:
        """One LaserMessage (ranges [n_beams]) or a batch of them ([n_scans, n_beams]) with the message's own limits.  A torch tensor is
        taken as it is: on the context's GPU the ranges are read in place, in pinned host memory they are copied from directly."""
        if hasattr(ranges, "data_ptr"):
            r = ranges if ranges.dim() == 2 else ranges[None, :]
            if r.dtype.itemsize != 4 or not r.dtype.is_floating_point or not r.is_contiguous():
                raise ValueError("tensor ranges must be contiguous float32")
        else:
            r = np.ascontiguousarray(ranges, np.float32)
            if r.ndim == 1:
                r = r[None, :]
        if r.ndim != 2 or r.shape[1] < 1:
            raise RuntimeError("RawDataPreprocessorProjective2D::setMeasurement|measurement is not set")     # .cpp:54-57
        self._msg = (r, float(angle_min), float(angle_max), float(range_min), float(range_max))
        return True

    def _message(self):
        """the ranges set with setRawData and their lsm2d_preprocessor: the message's limits clamped by this preprocessor's"""
        if self._msg is None:
            raise RuntimeError("RawDataPreprocessorProjective2D::compute| no raw data")
        r, a0, a1, m_rmin, m_rmax = self._msg
        return r, _capi.Preprocessor(r.shape[1], a0, a1, max(m_rmin, self.param_range_min), min(m_rmax, self.param_range_max),   # .cpp:83-84
                                     self.param_normal_point_distance, self.param_normal_min_points, self.param_voxelize_resolution)

    def compute(self) -> CloudSet:
        r, pp = self._message()
        ctx, lib = self._ctx, self._ctx._lib
        h = C.c_void_p()
        _producer_stream_wait(r)
        check(lib.lsm2d_preprocess_scans(ctx.handle, C.byref(pp), _ptr(r), r.shape[0], C.byref(h)), "lsm2d_preprocess_scans", ctx.handle)
        n_points = lib.lsm2d_cloudset_num_points(h)
        sizes = np.empty(r.shape[0], np.int32)
        check(min(lib.lsm2d_cloudset_cloud_sizes(h, _ptr(sizes), len(sizes)), 0), "lsm2d_cloudset_cloud_sizes", ctx.handle)
        self._meas = CloudSet._adopt(ctx, h, r.shape[0], n_points, sizes.astype(np.int64))
        return self._meas

    def refill(self, out: CloudSet) -> CloudSet:
        """The streaming form: the batch of messages set with setRawData goes into ``out`` -- a set an earlier ``compute()`` made for the same number of scans
        and beams -- with no allocation and no wait (lsm2d_preprocess_scans_refill): the ranges are fetched by an asynchronous copy (keep them untouched until
        the batch that reads ``out`` has been waited for), the clouds' sizes stay on the device.  Same kernel, same bits as ``compute()``."""
        r, pp = self._message()
        _producer_stream_wait(r)
        check(self._ctx._lib.lsm2d_preprocess_scans_refill(self._ctx.handle, C.byref(pp), _ptr(r), r.shape[0], out.handle),
              "lsm2d_preprocess_scans_refill", self._ctx.handle)
        self._meas = out
        return out

    def compute_into(self, out: CloudSet) -> CloudSet:
        """The live tracker's form: the ONE scan set with setRawData goes into the reserved set ``out`` -- no allocation,
        nothing waits; the cloud's size stays on the device until it is read (lsm2d_preprocess_scan_into)."""
        r, pp = self._message()
        if r.shape[0] != 1:
            raise ValueError("compute_into takes one scan")
        if hasattr(r, "data_ptr") and r.is_cuda:
            raise ValueError("compute_into stages the scan from host memory")
        check(self._ctx._lib.lsm2d_preprocess_scan_into(self._ctx.handle, C.byref(pp), _ptr(r), out.handle), "lsm2d_preprocess_scan_into", self._ctx.handle)
        out._set_pending()
        self._meas = out
        return out


class TrackerBatch:
    """N independent live trackers stepped together, one robot model for all of them: the reference's tracker step (clip the local map
    around the odometry guess, align the front and the rear scan with the odometry prior, merge both scans at the corrected pose;
    MULTI.json:464-482) as ONE call of each batched kernel per step.  Every tracker's result is what the single-tracker calls give for it.

    ``aligner`` carries two projective ``AlignerSliceProcessorLaser2DWithSensor`` slices (front, rear); their sensor offsets place the scans,
    the first one the clip.  The pose composition is float64 per tracker, as a single tracker's host side does it.  One wait per step:
    the aligner's poses."""

    def __init__(self, ctx: Context, n_trackers: int, projector: PointNormal2fProjectorPolar, preprocessor: RawDataPreprocessorProjective2D,
                 aligner: MultiAligner2D, angle_min: float, angle_max: float, range_min: float = 0.0, range_max: float = float("inf"),
                 merge_threshold: float = 0.2, prior_omega=None, map_capacity: int = 50000, clip_voxelize_resolution: float = 0.0):
        from . import synth
        if len(aligner.param_slice_processors) != 2:
            raise ValueError("TrackerBatch: the aligner needs two slices (front and rear scan)")
        self._ctx, self.n = ctx, int(n_trackers)
        self._synth = synth
        self.projector, self.preprocessor, self.aligner = projector, preprocessor, aligner
        self._msg = (float(angle_min), float(angle_max), float(range_min), float(range_max))
        self.sensor_in_robot = [np.asarray(getattr(s, "sensor_in_robot", (0.0, 0.0, 0.0)), np.float32).reshape(3)
                                for s in aligner.param_slice_processors]
        self.maps = CloudSet.reserved_many(ctx, self.n, map_capacity)
        self.clipped = CloudSet.reserved_many(ctx, self.n, projector.param_canvas_cols)
        self.scans = [None, None]            # the two scan sets (lsm2d_preprocess_scans once, refilled every step)
        # clip_voxelize_resolution > 0: the clipper voxelises what it clipped (the reference class's default is 0.1; the shipped configurations use 0)
        self.clipper = SceneClipperProjective2D(ctx, projector, voxelize_resolution=float(clip_voxelize_resolution), asynchronous=True)
        self.clipper.setSensorInRobot(self.sensor_in_robot[0])
        self.merger = MergerProjective2D(ctx, projector, merge_threshold, asynchronous=True)
        om = np.diag([100.0, 100.0, 100.0]) if prior_omega is None else prior_omega
        self._priors = [(np.zeros(3, np.float32), np.asarray(om, np.float32).reshape(3, 3))] * self.n
        self.estimate = np.zeros((self.n, 3), np.float64)      # robot in local map, per tracker
        self.guess = np.zeros((self.n, 3), np.float32)

    def _sensor_poses(self, poses):
        c, s_ = self._synth.compose_poses, self.sensor_in_robot
        return np.array([[np.float32(c(np.asarray(p, np.float64)[None, :], s.astype(np.float64)[None, :])[0]) for s in s_] for p in poses], np.float32)

    def _fill(self, k: int, ranges):
        a0, a1, r0, r1 = self._msg
        self.preprocessor.setRawData(np.ascontiguousarray(ranges, np.float32).reshape(self.n, -1), a0, a1, r0, r1)
        if self.scans[k] is None:
            self.scans[k] = self.preprocessor.compute()
        else:
            self.preprocessor.refill(self.scans[k])
            self.scans[k]._set_pending()      # (the sizes are the device's until asked for)

    def reset(self, indices, ranges_front, ranges_rear, poses):
        """Trackers ``indices`` start a new local map at ``poses`` [len(indices)][3] (robot in local map) from the two scans given
        [len(indices)][beams]: their maps are emptied and both scans merged, as a single tracker starts."""
        idx = np.ascontiguousarray(indices, np.int32).ravel()
        p = np.asarray(poses, np.float64).reshape(len(idx), 3)
        a0, a1, r0, r1 = self._msg
        meas = []
        for r in (ranges_front, ranges_rear):
            self.preprocessor.setRawData(np.ascontiguousarray(r, np.float32).reshape(len(idx), -1), a0, a1, r0, r1)
            meas.append(self.preprocessor.compute())
        self.maps.clear(idx)
        self.merger.compute_batch(self.maps, meas, self._sensor_poses(p), scene_index=idx)
        self.estimate[idx] = p
        self._reset_meas = meas      # (read by the merge launch: kept until the next reset)

    def step(self, ranges_front, ranges_rear, odometry):
        """One tracker step of all N trackers: returns (pose [N][3] float32 -- the aligner's moving-in-fixed --, status [N], information [N][3][3]).
        ``estimate`` then holds every tracker's corrected pose, float64."""
        c, inv = self._synth.compose_poses, self._synth.invert_poses
        odo = np.asarray(odometry, np.float64).reshape(self.n, 3)
        self._fill(0, ranges_front); self._fill(1, ranges_rear)
        self.guess = np.array([c(self.estimate[i][None, :], odo[i][None, :])[0] for i in range(self.n)], np.float32)
        self.clipper.compute_batch(self.maps, self.guess, self.clipped)
        r = self.aligner.compute_batch(self.scans, [self.clipped, self.clipped], np.zeros((self.n, 3), np.float32), priors=self._priors)
        x = r.pose
        self.estimate = np.array([c(self.guess[i][None, :].astype(np.float64), inv(x[i][None, :].astype(np.float64)))[0] for i in range(self.n)], np.float64)
        self.merger.compute_batch(self.maps, self.scans, self._sensor_poses(self.estimate))
        return x, r.status, r.information


@dataclasses.dataclass
class RelocalizeSelectResult:
    scored_index: np.ndarray   # int32 [m]: stage 1's selection, best first (``score_aligner_select``'s index); m = min(k_score, n_scored_accepted)
    scored_stats: np.ndarray   # structured [m]: their statistics at their own poses
    n_scored_accepted: int     # hypotheses that passed stage 1's acceptance test, of all
    index: np.ndarray          # int32 [r]: the aligned and accepted hypotheses as BATCH indices, best first; r = min(k, n_accepted)
    pose: np.ndarray           # [r, 3]
    information: np.ndarray    # [r, 3, 3]
    iterations: np.ndarray     # int32 [r]
    last_stats: np.ndarray     # structured [r]: the statistics of the last iteration each started
    n_accepted: int            # of the m aligned hypotheses: aligner succeeded and the last iteration passes stage 2's thresholds
    n_success: int             # of the m aligned hypotheses: aligner succeeded
    kernel_ms: float = 0.0     # from stage 1's first launch to the final selection (0 when the context is not timed)


def relocalize_select(aligner: "MultiAligner2D", fixed, moving, poses, score_select: SelectParams, k_score: int, align_select: SelectParams = None,
                      k: int = None, priors=None, fixed_index=None, moving_index=None) -> RelocalizeSelectResult:
    """The relocaliser / loop detector's candidate loop (MULTI.json:749-769, :964-986) in ONE call with one upload, one copy down and one wait
    (lsm2d_relocalize_select): ``score_aligner_select(..., score_select, k_score)``, then ``align_select(..., align_select, k)`` over the selected
    hypotheses -- their poses, priors and clouds gathered on the device -- with ``index`` mapped back to batch indices.  Every output is the two calls'
    bit for bit.  ``align_select`` None: ``score_select``; ``k`` None: ``k_score``.  The aligner always runs ``k_score`` alignments (slots nothing was
    selected for repeat a selected hypothesis and are never returned), so where mostly nothing passes stage 1 the two calls are cheaper."""
    ctx = aligner._ctx
    bd, keep = aligner._batch(fixed, moving, poses, priors, fixed_index, moving_index)      # (keep: what bd points to, alive until this function returns)
    ap = aligner._aligner_params()
    k2 = int(k_score if k is None else k)
    ks, kk = max(int(k_score), 1), max(k2, 1)
    s_index = np.empty(ks, np.int32); s_st = np.zeros(ks, STATS_DTYPE)
    index = np.empty(kk, np.int32); pose = np.empty((kk, 3), np.float32); H = np.empty((kk, 9), np.float32); its = np.empty(kk, np.int32)
    st = np.zeros(kk, STATS_DTYPE)
    n_ssel = C.c_int32(0); n_sacc = C.c_int32(0); n_sel = C.c_int32(0); n_acc = C.c_int32(0); n_suc = C.c_int32(0)
    sel1 = score_select.struct(); sel2 = None if align_select is None else align_select.struct()
    check(ctx._lib.lsm2d_relocalize_select(ctx.handle, C.byref(ap), C.byref(bd), C.byref(sel1), int(k_score), None if sel2 is None else C.byref(sel2), k2,
                                           _ptr(s_index), _ptr(s_st), C.byref(n_ssel), C.byref(n_sacc), _ptr(index), _ptr(pose), _ptr(H), _ptr(its), _ptr(st),
                                           C.byref(n_sel), C.byref(n_acc), C.byref(n_suc)), "lsm2d_relocalize_select", ctx.handle)
    m, r = n_ssel.value, n_sel.value
    ms = ctx.last_kernel_ms() if (bd.n_alignments and ctx.kernel_timing) else 0.0
    return RelocalizeSelectResult(s_index[:m], s_st[:m], n_sacc.value, index[:r], pose[:r], H[:r].reshape(r, 3, 3), its[:r], st[:r], n_acc.value,
                                  n_suc.value, ms)


# ---- a pose grid made on the device and scored coarse to fine (lsm2d_score_grid_select) ----

@dataclasses.dataclass
class PoseGrid:
    """lsm2d_pose_grid: a grid of pose hypotheses of ONE scan against one map and how it is refined.  Level 0 is ``count`` = (nx, ny, nt) cells spaced
    ``step`` round ``center``; every further level keeps the ``k_parents`` best cells and splits each into ``refine`` = (rx, ry, rt) children, whose
    spacing is the parent's divided by ``refine``.  NOT upstream (the reference does not say how its relocaliser chooses hypotheses), and NOT the
    exhaustive fine grid: the search finds that grid's winner only if its coarse cell is among the parents kept."""
    center: Sequence[float] = (0.0, 0.0, 0.0)
    step: Sequence[float] = (0.0, 0.0, 0.0)
    count: Sequence[int] = (1, 1, 1)
    n_levels: int = 1
    refine: Sequence[int] = (1, 1, 1)
    k_parents: int = 1

    def struct(self) -> _capi.PoseGridC:
        g = _capi.PoseGridC()
        g.center = (C.c_float * 3)(*[float(v) for v in self.center]); g.step = (C.c_float * 3)(*[float(v) for v in self.step])
        g.count = (C.c_int32 * 3)(*[int(v) for v in self.count]); g.n_levels = int(self.n_levels)
        g.refine = (C.c_int32 * 3)(*[int(v) for v in self.refine]); g.k_parents = int(self.k_parents)
        return g

    def spacing(self, level: int) -> np.ndarray:
        """float32 [3]: level 0's is ``step``; each further level's is the one above divided by ``refine`` in float32, division after division"""
        s = np.asarray(self.step, np.float32).copy()
        r = np.asarray(self.refine, np.int64).astype(np.float32)
        for _ in range(int(level)):
            s = (s / r).astype(np.float32)
        return s


def _grid_offsets(n: int) -> np.ndarray:
    """o(i, n) = i - 0.5 (n - 1), float32 [n]: exact"""
    return (np.arange(n, dtype=np.float32) - np.float32(0.5) * np.float32(n - 1)).astype(np.float32)


def grid_level_poses(grid: PoseGrid, level: int, parent_poses=None) -> np.ndarray:
    """The hypotheses of one level of ``grid`` as lsm2d_score_grid_select makes them on the device, restated in numpy float32: a coordinate is
    ``base + (o * s)`` -- the product rounded to float32, then the sum rounded to float32, two operations, never fused -- with ``o(i, n) = i - 0.5 (n - 1)``
    and ``s = grid.spacing(level)``.  Level 0 (``parent_poses`` unused): item ``(it * ny + iy) * nx + ix``, base ``center``, n ``count``.  Level >= 1: with
    ``R = rx * ry * rt``, item ``j * R + (ct * ry + cy) * rx + cx`` is a child of ``parent_poses[j]`` (the previous level's selected poses, best first, bit
    for bit as they were scored), n ``refine``.  theta is not wrapped.  Returns float32 ``[n, 3]``."""
    s = grid.spacing(level)
    if int(level) == 0:
        n = [int(v) for v in grid.count]
        base = np.asarray(grid.center, np.float32).reshape(1, 3)
    else:
        n = [int(v) for v in grid.refine]
        base = np.asarray(parent_poses, np.float32).reshape(-1, 3)
    d = [(_grid_offsets(n[a]) * s[a]).astype(np.float32) for a in range(3)]      # the products, rounded
    per = n[0] * n[1] * n[2]
    c = np.arange(per)
    ia = (c % n[0], (c // n[0]) % n[1], c // (n[0] * n[1]))
    out = np.empty((len(base), per, 3), np.float32)
    for a in range(3):
        out[:, :, a] = (base[:, a:a + 1] + d[a][ia[a]][None, :]).astype(np.float32)      # the sums, rounded
    return out.reshape(-1, 3)


@dataclasses.dataclass
class ScoreGridResult:
    pose: np.ndarray           # [m, 3]: the best hypotheses of the last level at the poses they were scored at, best first; m = min(k, n_accepted)
    origin: np.ndarray         # int32 [m]: the level-0 cell each descends from
    H: np.ndarray              # [m, 3, 3]
    b: np.ndarray              # [m, 3]
    stats: np.ndarray          # structured [m]
    active: np.ndarray         # int32 [m]
    n_accepted: int            # hypotheses of the last level that passed ``select``, pads never among them
    level_counts: np.ndarray   # int32 [n_levels, 2]: {accepted, selected} per level
    kernel_ms: float = 0.0     # from the first launch to the last selection (0 when the context is not timed)


def score_grid_select(aligner: "MultiAligner2D", fixed, moving, grid: PoseGrid, coarse_select: Optional[SelectParams], select: SelectParams, k: int,
                      fixed_cloud=None, moving_cloud=None) -> ScoreGridResult:
    """``grid`` scored coarse to fine against the whole aligner in ONE call with no upload of hypotheses, one copy down and one wait
    (lsm2d_score_grid_select): the poses are made on the device, level l is ``score_aligner_select`` over ``grid_level_poses(grid, l, parents)`` bit for
    bit -- ``coarse_select`` / ``grid.k_parents`` below the last level, ``select`` / ``k`` at the last -- and a level's selection becomes the next level's
    parents without leaving the device.  ``fixed[s]`` / ``moving[s]``: a set per slice; ``fixed_cloud[s]`` / ``moving_cloud[s]``: the one cloud of it all
    hypotheses use (None: cloud 0).  Below level 0 the device always runs ``k_parents * R`` slots: those of parents that were not selected are pads, paid
    for but never accepted, counted or returned; once a level selects nothing the deeper ones report (0, 0)."""
    ctx = aligner._ctx
    slices = aligner.param_slice_processors
    ns = len(slices)
    sp = (SliceParams * ns)(*[s.slice_params() for s in slices])
    fixed_sets = [_as_cloudset(ctx, f) for f in fixed]; moving_sets = [_as_cloudset(ctx, m) for m in moving]      # (alive until this function returns)
    fx = (C.c_void_p * ns)(*[f.handle.value for f in fixed_sets]); mv = (C.c_void_p * ns)(*[m.handle.value for m in moving_sets])
    fc = None if fixed_cloud is None else np.ascontiguousarray(fixed_cloud, np.int32).reshape(ns)
    mc = None if moving_cloud is None else np.ascontiguousarray(moving_cloud, np.int32).reshape(ns)
    g = grid.struct()
    levels = max(int(grid.n_levels), 1)
    kk = max(int(k), 1)
    pose = np.empty((kk, 3), np.float32); origin = np.empty(kk, np.int32); H = np.empty((kk, 9), np.float32); b = np.empty((kk, 3), np.float32)
    st = np.zeros(kk, STATS_DTYPE); active = np.zeros(kk, np.int32); counts = np.zeros((levels, 2), np.int32)
    n_sel = C.c_int32(0); n_acc = C.c_int32(0)
    sel0 = None if coarse_select is None else coarse_select.struct(); sel = select.struct()
    check(ctx._lib.lsm2d_score_grid_select(ctx.handle, ns, sp, C.cast(fx, C.POINTER(C.c_void_p)), _ptr(fc), C.cast(mv, C.POINTER(C.c_void_p)), _ptr(mc),
                                           C.byref(g), None if sel0 is None else C.byref(sel0), C.byref(sel), int(k), _ptr(pose), _ptr(origin), _ptr(H),
                                           _ptr(b), _ptr(st), _ptr(active), C.byref(n_sel), C.byref(n_acc), _ptr(counts)),
          "lsm2d_score_grid_select", ctx.handle)
    m = n_sel.value
    ms = ctx.last_kernel_ms() if ctx.kernel_timing else 0.0
    return ScoreGridResult(pose[:m], origin[:m], H[:m].reshape(m, 3, 3), b[:m], st[:m], active[:m], n_acc.value, counts, ms)


@dataclasses.dataclass
class RelocalizeGridResult:
    scored: ScoreGridResult        # the grid search's answer: the hypotheses that were aligned, best first
    aligned: AlignSelectResult     # ``align_select`` over ``scored.pose``; its ``index`` points into ``scored``


def relocalize_grid(aligner: "MultiAligner2D", fixed, moving, grid: PoseGrid, coarse_select: Optional[SelectParams], select: SelectParams, k_score: int,
                    align_select_params: SelectParams = None, k: int = None, fixed_cloud=None, moving_cloud=None) -> RelocalizeGridResult:
    """The relocaliser's candidate loop over a pose grid: ``score_grid_select(..., k_score)``, then the existing ``align_select`` from the returned poses
    (``align_select_params`` None: ``select``; ``k`` None: ``k_score``).  That is TWO calls and TWO waits, on purpose: fusing the aligned stage behind the
    scoring was measured at 0.4 % in 0.7.9 (``relocalize_select``), so the second stage is not chained here.  Where nothing passes the grid search no
    alignment is run."""
    scored = score_grid_select(aligner, fixed, moving, grid, coarse_select, select, k_score, fixed_cloud, moving_cloud)
    ns = len(aligner.param_slice_processors)
    m = len(scored.pose)
    kk = int(k_score if k is None else k)
    sel2 = select if align_select_params is None else align_select_params
    if m == 0:
        z = np.zeros
        return RelocalizeGridResult(scored, AlignSelectResult(z(0, np.int32), z((0, 3), np.float32), z((0, 3, 3), np.float32), z(0, np.int32), z(0, STATS_DTYPE), 0, 0))

    def spelled(cloud):      # every slot's cloud in every slice: the batch is m candidates of the same clouds
        c = np.zeros(ns, np.int32) if cloud is None else np.ascontiguousarray(cloud, np.int32).reshape(ns)
        return np.repeat(c[:, None], m, axis=1)

    return RelocalizeGridResult(scored, align_select(aligner, fixed, moving, scored.pose, sel2, kk, None, spelled(fixed_cloud), spelled(moving_cloud)))


# ---- device-resident clouds voxelised and assembled in one call (lsm2d_voxelize) ----

@dataclasses.dataclass
class VoxelizeParams:
    """lsm2d_voxelize_params: PointCloud::voxelize's coefficients (resolution, resolution, normal_resolution, normal_resolution).  ``normal_resolution``
    1 is the raw-scan preprocessor's (res, res, 1, 1), 0.1 the scene clipper's (res, res, 0.1, 0.1)."""
    resolution: float = 0.05
    normal_resolution: float = 1.0

    @classmethod
    def preprocessor(cls, resolution: float) -> "VoxelizeParams":
        return cls(resolution, 1.0)

    @classmethod
    def clipper(cls, resolution: float) -> "VoxelizeParams":
        return cls(resolution, 0.1)

    def struct(self) -> _capi.VoxelizeParamsC:
        return _capi.VoxelizeParamsC(float(self.resolution), float(self.normal_resolution))


def voxelize(ctx: Context, params: VoxelizeParams, src: CloudSet, src_index=None, poses=None, groups=None, n_groups: int = 1, dst: Optional[CloudSet] = None,
             dst_index=None):
    """Clouds of ``src`` voxelised on the device into the clouds of the reserved set ``dst`` in ONE call (lsm2d_voxelize): output cloud g is the voxelisation
    of the concatenation of every input k with ``groups[k] == g`` in list order, each first moved by ``poses[k]`` (None: no transform at all).
    ``src_index`` None: every cloud of ``src`` in order; ``groups`` None: all inputs in group 0; ``dst_index`` None: group g to cloud g.  ``dst`` None
    reserves a set sized by the inputs (``n_groups`` clouds, each with room for every input point); ``dst`` may be ``src`` (a fleet's maps decimated in
    place: ``groups=range(n)``, ``n_groups=n``).  Returns ``(dst, counts, dropped)``: int32 ``[n_groups]`` voxels written and points that had no key.
    All or nothing: when a group does not fit its destination cloud nothing is written and ``Lsm2dError`` (CAPACITY_EXCEEDED) carries the needed counts
    as ``.counts``."""
    idx = None if src_index is None else np.ascontiguousarray(src_index, np.int32).ravel()
    n_inputs = src.n_clouds if idx is None else len(idx)
    ps = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(n_inputs, 3)
    gr = None if groups is None else np.ascontiguousarray(groups, np.int32).reshape(n_inputs)
    n_groups = int(n_groups)
    di = None if dst_index is None else np.ascontiguousarray(dst_index, np.int32).reshape(n_groups)
    if dst is None:
        c = src.counts
        room = max(int(c.sum() if idx is None else c[idx].sum()), 1)
        dst = CloudSet.reserved(ctx, room) if n_groups == 1 else CloudSet.reserved_many(ctx, n_groups, room)
    p = params.struct()
    counts = np.zeros(max(n_groups, 1), np.int32); dropped = np.zeros(max(n_groups, 1), np.int32)
    try:
        check(ctx._lib.lsm2d_voxelize(ctx.handle, C.byref(p), src.handle, n_inputs, _ptr(idx), _ptr(ps), _ptr(gr), n_groups, dst.handle, _ptr(di), _ptr(counts),
                                      _ptr(dropped)), "lsm2d_voxelize", ctx.handle)
    except Lsm2dError as e:
        e.counts, e.dropped = counts[:n_groups].copy(), dropped[:n_groups].copy()
        raise
    if not dst._pending:
        c = dst._counts.copy(); c[np.arange(n_groups) if di is None else di] = counts[:n_groups]
        dst._counts = c; dst._n_points = int(c.sum())
    return dst, counts[:n_groups], dropped[:n_groups]


# ---- occupancy grids on the device (lsm2d_gridset, lsm2d_occupancy_update, lsm2d_occupancy_render; not in the reference, which has no grid mapper) ----

@dataclasses.dataclass
class GridGeometry:
    """lsm2d_grid_geometry: cell (cx, cy) covers [origin + c * resolution, origin + (c + 1) * resolution) on each axis; arrays are [height][width]."""
    origin_x: float = 0.0
    origin_y: float = 0.0
    resolution: float = 0.05
    width: int = 1
    height: int = 1

    def struct(self) -> _capi.GridGeometryC:
        return _capi.GridGeometryC(float(self.origin_x), float(self.origin_y), float(self.resolution), int(self.width), int(self.height))


@dataclasses.dataclass
class LogOddsParams:
    """lsm2d_logodds_params, in integer units of the caller's choice: the vote of a hit (1 .. 2^20) and of a miss (-2^20 .. -1) and the clamps
    (-2^30 <= l_min <= 0 <= l_max <= 2^30).  With ``unit`` log-odds per integer unit, l_hit = round(log(p_hit / (1 - p_hit)) / unit)."""
    l_hit: int
    l_miss: int
    l_min: int
    l_max: int

    def struct(self) -> _capi.LogOddsParamsC:
        return _capi.LogOddsParamsC(int(self.l_hit), int(self.l_miss), int(self.l_min), int(self.l_max))


class GridSet:
    """``n_grids`` device-resident occupancy grids of one geometry (lsm2d_gridset), zero at creation.  A counts set (``logodds`` None) holds two uint32
    counters per cell, hits and misses; a log-odds set (``logodds`` a LogOddsParams; 0.7.14) holds {int32 value, uint32 observed}: every scan of an update
    gives a cell ONE clamped vote, the scans in list order, and ``observed`` counts the scans that voted (0: unknown)."""

    def __init__(self, ctx: Context, geometry: GridGeometry, n_grids: int = 1, logodds: Optional[LogOddsParams] = None):
        self._ctx, self._lib = ctx, ctx._lib
        self.geometry, self.n_grids, self.logodds = geometry, int(n_grids), logodds
        g = geometry.struct(); h = C.c_void_p()
        if logodds is None:
            check(self._lib.lsm2d_gridset_create(ctx.handle, C.byref(g), int(n_grids), C.byref(h)), "lsm2d_gridset_create", ctx.handle)
        else:
            p = logodds.struct()
            check(self._lib.lsm2d_gridset_create_logodds(ctx.handle, C.byref(g), int(n_grids), C.byref(p), C.byref(h)), "lsm2d_gridset_create_logodds", ctx.handle)
        self._h = h
        ctx._sets.add(self)      # closed with its context, like a cloud set

    @property
    def handle(self):
        return self._h

    @property
    def shape(self) -> tuple:
        return (int(self.geometry.height), int(self.geometry.width))

    def clear(self, indices=None):
        """Zeroes grids ``indices`` (None: every grid); queued, no wait (lsm2d_gridset_clear)."""
        idx = None if indices is None else np.ascontiguousarray(indices, np.int32).ravel()
        check(self._lib.lsm2d_gridset_clear(self._h, 0 if idx is None else len(idx), _ptr(idx)), "lsm2d_gridset_clear", self._ctx.handle)

    def upload(self, grid_index: int = 0, hits=None, misses=None):
        """Sets the counters of one grid from uint32 ``[height][width]`` arrays; None leaves that counter as it is (lsm2d_gridset_upload)."""
        h = None if hits is None else np.ascontiguousarray(hits, np.uint32).reshape(self.shape)
        m = None if misses is None else np.ascontiguousarray(misses, np.uint32).reshape(self.shape)
        check(self._lib.lsm2d_gridset_upload(self._h, int(grid_index), _ptr(h), _ptr(m)), "lsm2d_gridset_upload", self._ctx.handle)

    def download(self, grid_index: int = 0) -> tuple:
        """-> (hits, misses), uint32 ``[height][width]`` (lsm2d_gridset_download)."""
        h = np.empty(self.shape, np.uint32); m = np.empty(self.shape, np.uint32)
        check(self._lib.lsm2d_gridset_download(self._h, int(grid_index), _ptr(h), _ptr(m)), "lsm2d_gridset_download", self._ctx.handle)
        return h, m

    def set_logodds(self, params: LogOddsParams):
        """The votes and clamps of LATER updates of a log-odds set; host-side only (lsm2d_gridset_set_logodds)."""
        p = params.struct()
        check(self._lib.lsm2d_gridset_set_logodds(self._h, C.byref(p)), "lsm2d_gridset_set_logodds", self._ctx.handle)
        self.logodds = params

    def upload_logodds(self, grid_index: int = 0, value=None, observed=None):
        """Sets one grid of a log-odds set from an int32 and a uint32 ``[height][width]`` array; None leaves that word as it is.  Values outside the clamps
        are legal: the next vote pulls them in (lsm2d_gridset_upload_logodds)."""
        v = None if value is None else np.ascontiguousarray(value, np.int32).reshape(self.shape)
        o = None if observed is None else np.ascontiguousarray(observed, np.uint32).reshape(self.shape)
        check(self._lib.lsm2d_gridset_upload_logodds(self._h, int(grid_index), _ptr(v), _ptr(o)), "lsm2d_gridset_upload_logodds", self._ctx.handle)

    def download_logodds(self, grid_index: int = 0) -> tuple:
        """-> (value int32, observed uint32), ``[height][width]`` (lsm2d_gridset_download_logodds)."""
        v = np.empty(self.shape, np.int32); o = np.empty(self.shape, np.uint32)
        check(self._lib.lsm2d_gridset_download_logodds(self._h, int(grid_index), _ptr(v), _ptr(o)), "lsm2d_gridset_download_logodds", self._ctx.handle)
        return v, o

    def decay(self, amount: int, indices=None):
        """Every observed cell of grids ``indices`` (None: every grid) moves toward 0 by ``amount`` >= 0, never past it; queued, no wait
        (lsm2d_occupancy_decay)."""
        idx = None if indices is None else np.ascontiguousarray(indices, np.int32).ravel()
        check(self._lib.lsm2d_occupancy_decay(self._ctx.handle, self._h, 0 if idx is None else len(idx), _ptr(idx), int(amount)), "lsm2d_occupancy_decay",
              self._ctx.handle)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsm2d_gridset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def occupancy_update(ctx: Context, grids: GridSet, src: CloudSet, src_index=None, poses=None, grid=None):
    """The points of clouds of ``src`` ray-traced into the counters of ``grids`` in ONE call (lsm2d_occupancy_update): input k's points are moved by
    ``poses[k]`` (the sensor in the grid's frame; None: no transform, rays start at (0, 0)); each ray from the sensor's cell to the point's cell adds 1 to
    ``misses`` of every cell before its last and 1 to ``hits`` of its last, in grid ``grid[k]`` (None: grid 0).  ``src_index`` None: every cloud of ``src``
    in order.  Returns ``(rays, dropped)``: int32 ``[n_grids]`` rays walked and points that gave no ray."""
    idx = None if src_index is None else np.ascontiguousarray(src_index, np.int32).ravel()
    n_inputs = src.n_clouds if idx is None else len(idx)
    ps = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(n_inputs, 3)
    gr = None if grid is None else np.ascontiguousarray(grid, np.int32).reshape(n_inputs)
    rays = np.zeros(grids.n_grids, np.int32); dropped = np.zeros(grids.n_grids, np.int32)
    check(ctx._lib.lsm2d_occupancy_update(ctx.handle, grids.handle, src.handle, n_inputs, _ptr(idx), _ptr(ps), _ptr(gr), _ptr(rays), _ptr(dropped)),
          "lsm2d_occupancy_update", ctx.handle)
    return rays, dropped


@dataclasses.dataclass
class OccupancyScanParams:
    """lsm2d_occupancy_scan_params: the sensor geometry as the preprocessor takes it, the gate of a return (range_min <= r <= range_max), the cut no ray
    is traced beyond (trace_range <= range_max) and whether a beam without a return (r > range_max, +Inf included) clears out to the cut."""
    n_beams: int
    angle_min: float
    angle_max: float
    range_min: float = 0.0
    range_max: float = 30.0
    trace_range: float = 30.0
    clear_no_return: bool = True

    def struct(self) -> _capi.OccupancyScanParamsC:
        return _capi.OccupancyScanParamsC(int(self.n_beams), float(self.angle_min), float(self.angle_max), float(self.range_min), float(self.range_max),
                                          float(self.trace_range), int(self.clear_no_return))


def occupancy_update_scans(ctx: Context, grids: GridSet, params: OccupancyScanParams, ranges, poses=None, grid=None):
    """Raw range scans ray-traced into the counters of ``grids`` in ONE call (lsm2d_occupancy_update_scans): ``ranges`` is ``[n_scans, n_beams]`` (or one
    scan ``[n_beams]``), a numpy array or a torch tensor taken as it is (on the context's GPU it is read in place, in pinned host memory it is copied from
    directly).  A return up to ``trace_range`` is a HIT ray (misses along it, a hit at its end); a return beyond it, and with ``clear_no_return`` a beam
    without a return, is a CLEAR ray of length ``trace_range`` (misses on every cell, no hit); NaN, -Inf and ranges below ``range_min`` are dropped.
    ``poses[k]``: the sensor of scan k in the grid's frame (None: no transform, rays start at (0, 0)); ``grid[k]``: its grid (None: grid 0).
    Returns ``(hit_rays, clear_rays, dropped)``: int32 ``[n_grids]`` each; per grid they sum to the beams sent to it."""
    if hasattr(ranges, "data_ptr"):
        r = ranges if ranges.dim() == 2 else ranges[None, :]
        if r.dtype.itemsize != 4 or not r.dtype.is_floating_point or not r.is_contiguous():
            raise ValueError("tensor ranges must be contiguous float32")
        _producer_stream_wait(r)
    else:
        r = np.ascontiguousarray(ranges, np.float32)
        if r.ndim == 1:
            r = r[None, :]
    if len(r.shape) != 2 or r.shape[1] != int(params.n_beams):
        raise ValueError("ranges must be [n_scans, n_beams]")
    n_scans = int(r.shape[0])
    ps = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(n_scans, 3)
    gr = None if grid is None else np.ascontiguousarray(grid, np.int32).reshape(n_scans)
    p = params.struct()
    hit = np.zeros(grids.n_grids, np.int32); clear = np.zeros(grids.n_grids, np.int32); dropped = np.zeros(grids.n_grids, np.int32)
    check(ctx._lib.lsm2d_occupancy_update_scans(ctx.handle, grids.handle, C.byref(p), _ptr(r), n_scans, _ptr(ps), _ptr(gr), _ptr(hit), _ptr(clear), _ptr(dropped)),
          "lsm2d_occupancy_update_scans", ctx.handle)
    return hit, clear, dropped


def occupancy_render(ctx: Context, grids: GridSet, grid_index: int = 0, min_visits: int = 1) -> np.ndarray:
    """One grid as a consumer reads it (lsm2d_occupancy_render): int8 ``[height][width]``, -1 where hits + misses < max(min_visits, 1), else the share of
    hits in percent, 0 .. 100.  Bit for bit ``occupancy_values`` of the downloaded counters."""
    p = _capi.OccupancyRenderParamsC(int(min_visits))
    out = np.empty(grids.shape, np.int8)
    check(ctx._lib.lsm2d_occupancy_render(ctx.handle, grids.handle, int(grid_index), C.byref(p), _ptr(out)), "lsm2d_occupancy_render", ctx.handle)
    return out


def occupancy_values(hits, misses, min_visits: int = 1) -> np.ndarray:
    """lsm2d_occupancy_render's rule in numpy float32: v = hits + misses in 64 bits; v < max(min_visits, 1) gives -1; else rint(100 * (float32(hits) /
    float32(v))), each operation rounded once to float32, ties to even."""
    h = np.asarray(hits, np.uint32).astype(np.uint64); v = h + np.asarray(misses, np.uint32).astype(np.uint64)
    known = v >= np.uint64(max(int(min_visits), 1))
    den = np.where(known, v, np.uint64(1)).astype(np.float32)
    p = h.astype(np.float32) / den
    val = np.rint(np.float32(100.0) * p).astype(np.int8)
    return np.where(known, val, np.int8(-1)).astype(np.int8)


# ---- log-odds grid sets (0.7.14; PARITY.md section 3, item 17e) ----

def logodds_render_table(unit: float) -> np.ndarray:
    """lsm2d_logodds_render_table: int32 ``[100]``, entry j - 1 = ceil(log((j - 0.5) / (100.5 - j)) / unit) -- the smallest value that renders as j percent
    or more.  Host only; launches nothing."""
    t = np.empty(100, np.int32)
    code = _capi.load().lsm2d_logodds_render_table(C.c_float(unit), _ptr(t))
    if code < 0:
        raise Lsm2dError(code, "lsm2d_logodds_render_table", "unit must be finite and > 0")
    return t


def occupancy_render_logodds(ctx: Context, grids: GridSet, grid_index: int = 0, unit: float = 0.01, min_scans: int = 1) -> np.ndarray:
    """One grid of a log-odds set as a consumer reads it (lsm2d_occupancy_render_logodds): int8 ``[height][width]``, -1 where observed < max(min_scans, 1),
    else the probability in percent, 0 .. 100, by the table of ``unit``.  Bit for bit ``logodds_values`` of the downloaded cells."""
    p = _capi.LogOddsRenderParamsC(int(min_scans), float(unit))
    out = np.empty(grids.shape, np.int8)
    check(ctx._lib.lsm2d_occupancy_render_logodds(ctx.handle, grids.handle, int(grid_index), C.byref(p), _ptr(out)), "lsm2d_occupancy_render_logodds", ctx.handle)
    return out


def logodds_values(value, observed, unit: float, min_scans: int = 1) -> np.ndarray:
    """lsm2d_occupancy_render_logodds' rule in numpy: -1 where observed < max(min_scans, 1), else the number of entries of ``logodds_render_table(unit)``
    that are <= value."""
    t = logodds_render_table(unit)
    n = np.searchsorted(t, np.asarray(value, np.int32), side="right").astype(np.int8)
    known = np.asarray(observed, np.uint32) >= np.uint32(max(int(min_scans), 1))
    return np.where(known, n, np.int8(-1)).astype(np.int8)
