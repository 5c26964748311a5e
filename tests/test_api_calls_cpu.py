"""The C ABI calls ``srrg2_laser_slam_2d_amd/api.py`` makes, checked without a GPU: ``_capi.load`` is replaced by a stand-in library that records every
call -- the symbol and every argument -- and the record of one script over every public entry point is compared with the stored one
(tests/golden/api_call_trace.json, taken from api.py as it stood BEFORE its marshalling was rewritten; ``python tests/test_api_calls_cpu.py --write`` writes the
file from the api.py it runs on: only ever do that on a commit whose api.py is trusted, never to make a failing comparison pass).

What is recorded: integers, floats and bytes by value; NULL as "NULL"; a set's / context's / batch's handle by the order it was handed out ("h3"); any other
pointer as "ptr"; a struct passed by reference by its bytes; a batch descriptor by its counts and by what each pointer member points to (NULL where absent); an
out-parameter by its width.  ``lsm2d_destroy`` / ``lsm2d_cloudset_destroy`` are left out of the record (when an object dies is the interpreter's affair), but a
handle that comes in a call after its destroy fails the run.  Nothing computes: the stand-in returns 0 and writes only what api.py reads back."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from srrg2_laser_slam_2d_amd import _capi, api      # noqa: E402  (importing loads no library)

GOLDEN = os.path.join(ROOT, "tests", "golden", "api_call_trace.json")
STATS_CAPACITY = 4                 # what the stand-in's lsm2d_stats_capacity answers
CLOUD_SIZE = 9                     # ... its lsm2d_cloudset_cloud_size
CLOUD_SIZES = (3, 4, 5, 6)         # ... the first entries its lsm2d_cloudset_cloud_sizes writes
NUM_POINTS = 7                     # ... its lsm2d_cloudset_num_points
INDEX_ARG = {"lsm2d_score_select": 10, "lsm2d_score_aligner_select": 4}      # where out_index stands in the two selecting calls


class FakeLib:
    """Stands in for liblsm2d_hip.so: every attribute is a function that records its call."""

    def __init__(self):
        self.trace = []
        self.handles = {}          # value -> "h<k>"
        self.destroyed = set()
        self.n_selected = []       # scripted answers of the selecting calls, first come first served; 0 when empty

    def _handle(self, value):
        if value in self.destroyed:
            raise AssertionError("handle %s used after its destroy" % self.handles[value])
        return self.handles.get(value, "ptr")

    def _new_handle(self, out):
        out.value = 0x1000 * (len(self.handles) + 1)
        self.handles[out.value] = "h%d" % len(self.handles)

    def _pointer(self, p):
        return "NULL" if not p.value else self._handle(p.value)

    def _batch(self, b):
        n, ns = b.n_alignments, b.n_slices
        data = lambda p, size: C.string_at(p, size).hex() if p else "NULL"
        return {"n_alignments": n, "n_slices": ns,
                "slices": [bytes(b.slices[i]).hex() for i in range(ns)] if b.slices else "NULL",
                "fixed": [self._pointer(C.c_void_p(b.fixed[i])) for i in range(ns)] if b.fixed else "NULL",
                "moving": [self._pointer(C.c_void_p(b.moving[i])) for i in range(ns)] if b.moving else "NULL",
                "fixed_index": data(b.fixed_index, 4 * ns * n), "moving_index": data(b.moving_index, 4 * ns * n),
                "init_pose": data(b.init_pose, 12 * n), "prior": data(b.prior, C.sizeof(_capi.Prior) * n)}

    def _record(self, a):
        if a is None:
            return "NULL"
        if isinstance(a, bytes):
            return "b:" + a.decode()
        if isinstance(a, (int, float, np.integer, np.floating)):
            return a.item() if isinstance(a, np.generic) else a
        if hasattr(a, "_obj"):                       # byref(...)
            o = a._obj
            if isinstance(o, _capi.Batch):
                return self._batch(o)
            if isinstance(o, C.Structure):
                return type(o).__name__ + ":" + bytes(o).hex()
            if isinstance(o, C.c_void_p):
                return "out:handle"
            return "out:%s%d" % ("f" if isinstance(o, (C.c_float, C.c_double)) else "i", 8 * C.sizeof(o))
        if isinstance(a, C.c_void_p):
            return self._pointer(a)
        if isinstance(a, C.Array):
            if issubclass(a._type_, C.c_void_p):
                return [self._pointer(C.c_void_p(v)) for v in a]
            if issubclass(a._type_, C.Structure):
                return "%s[%d]" % (a._type_.__name__, len(a))
            return list(a)
        raise AssertionError("an argument the record has no form for: %r" % (a,))

    def __getattr__(self, name):
        if not name.startswith("lsm2d_"):
            raise AttributeError(name)

        def call(*args):
            if name in ("lsm2d_destroy", "lsm2d_cloudset_destroy"):
                self.destroyed.add(args[0].value)
                return None
            self.trace.append([name] + [self._record(a) for a in args])
            return self._answer(name, args)
        return call

    def _answer(self, name, args):
        for a in args:                                # a fresh handle into every out-handle (create, preprocess, begin)
            if hasattr(a, "_obj") and isinstance(a._obj, C.c_void_p):
                self._new_handle(a._obj)
        if name == "lsm2d_stats_capacity":
            return STATS_CAPACITY
        if name == "lsm2d_cloudset_cloud_size":
            return CLOUD_SIZE
        if name == "lsm2d_cloudset_num_points":
            return NUM_POINTS
        if name == "lsm2d_cloudset_cloud_sizes":
            assert args[2] <= len(CLOUD_SIZES)
            out = C.cast(args[1], C.POINTER(C.c_int32))
            for i in range(args[2]):
                out[i] = CLOUD_SIZES[i]
        if name == "lsm2d_cloudset_download":
            args[4]._obj.value = args[3]              # as many points as the caller made room for
        if name in ("lsm2d_align_batch", "lsm2d_align_batch_pairs"):      # zero poses, statuses and iteration counts: the tracker and relocalize read them
            n = args[2]._obj.n_alignments
            for p, width in ((args[3], 3), (args[5], 1), (args[6], 1)):
                C.memset(p, 0, 4 * width * n)
        if name in INDEX_ARG:
            m = self.n_selected.pop(0) if self.n_selected else 0
            assert m <= 1
            if m:
                C.cast(args[INDEX_ARG[name]], C.POINTER(C.c_int32))[0] = 0
            args[-2]._obj.value = m; args[-1]._obj.value = m
        if name == "lsm2d_last_error":
            return b""
        return 0


def _pts(n, shift=0.0):
    return (np.arange(4 * n, dtype=np.float32).reshape(n, 4) + np.float32(shift)) / np.float32(10)


POSES = np.array([[0.1, 0.2, 0.3], [-0.4, 0.5, -0.6]], np.float32)
PRIORS = [(np.array([0.1, 0.0, -0.1], np.float32), np.eye(3, dtype=np.float32) * 7), (np.zeros(3, np.float32), np.arange(9, dtype=np.float32).reshape(3, 3))]


class Script:
    """Every public entry point of api.py once, on tiny inputs; keeps what the tests look at afterwards."""

    def __init__(self, lib):
        self.lib = lib
        ctx = self.ctx = api.Context(0)
        ctx.set_option("align_path", 2)
        assert ctx.get_option("last_align_path") == 0
        ctx.synchronize()
        ctx.last_kernel_ms()
        self.cloud_sets()
        self.projector_and_finders()
        self.factor_and_scores()
        self.aligner()
        self.relocalize()
        self.mapping()
        self.preprocessor_and_trackers()

    def cloud_sets(self):
        ctx = self.ctx
        self.one = api.CloudSet(ctx, _pts(7))                          # one cloud
        self.many = api.CloudSet(ctx, _pts(10, 1.0), [0, 4, 10])       # two clouds of 4 and 6 points
        assert self.one.n_points == 7 and self.many.counts.tolist() == [4, 6] and self.many.n_clouds == 2
        self.res1 = api.CloudSet.reserved(ctx, 64)
        self.resN = api.CloudSet.reserved_many(ctx, 2, 64)
        assert self.res1.capacity == 64 and self.resN.capacity == 64 and self.resN.counts.tolist() == [0, 0]
        self.resN.clear()
        self.resN.clear([1])
        self.res1.upload(_pts(6))
        assert self.res1.n_points == 6 and self.res1.download(0).shape == (6, 4)
        self.res1._set_pending()                                       # a pending size, read back: one cloud ...
        assert self.res1.n_points == CLOUD_SIZE and self.res1.counts.tolist() == [CLOUD_SIZE]
        self.resN._set_pending()                                       # ... and many
        assert self.resN.counts.tolist() == list(CLOUD_SIZES[:2]) and self.resN.n_points == sum(CLOUD_SIZES[:2])
        self.resN._set_pending()
        self.resN.clear([0])                                           # (clearing a pending set leaves its sizes to the device)
        assert self.resN.counts.tolist() == list(CLOUD_SIZES[:2])
        self.resN.clear([0])
        assert self.resN.counts.tolist() == [0, CLOUD_SIZES[1]] and self.resN.n_points == CLOUD_SIZES[1]

    def projector_and_finders(self):
        ctx = self.ctx
        self.proj = api.PointNormal2fProjectorPolar(64, -3.0, 3.0, 0.3, 30.0)
        src, depth, xy = self.proj.compute(ctx, self.many, (0.1, 0.2, 0.3), 1)
        assert src.shape == (64,) and depth.shape == (64,) and xy.shape == (64, 4)
        self.finders = [api.CorrespondenceFinderProjective2f(ctx, self.proj, point_distance=0.4, normal_cos=0.7),
                        api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.3, search="exact"),
                        api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.3, max_leaf_range=0.05, min_leaf_points=3, search="kdtree"),
                        api.CorrespondenceFinderNN2D(ctx, max_distance_m=0.9, resolution=0.1)]
        for f in self.finders:
            f.setFixed(self.one); f.setMoving(self.many, 0); f.setLocalMapInSensor(POSES[0])      # (the chosen moving cloud is the set's smaller one)
            assert f.compute().shape == (0, 2) and f.correspondences().shape == (0, 2)
            assert len(f.compute_batch(self.one, self.many, POSES)) == 2
            assert len(f.compute_batch(self.many, self.many, POSES, fixed_index=[1, 0], moving_index=[0, 0])) == 2
            assert f.compute_batch(self.one, self.one, np.zeros((0, 3))) == []

    def factor_and_scores(self):
        ctx = self.ctx
        self.sp = sp = self.finders[0].slice_params(robustifier=api.ROBUST_CAUCHY, chi_threshold=0.05, min_num_correspondences=2, sensor_in_robot=(0.1, 0.0, 0.2))
        H, b, st = api.linearize(ctx, sp, self.many, self.one, [[0, 1], [1, 2]], POSES[0], fixed_index=1, moving_index=0)
        assert H.shape == (3, 3) and b.shape == (3,)
        rows = [np.array([[0, 1], [1, 2]], np.int32), np.zeros((0, 2), np.int32)]
        H, b, st = api.linearize_batch(ctx, sp, self.many, self.one, rows, POSES)
        assert H.shape == (2, 3, 3) and b.shape == (2, 3) and len(st) == 2
        padded = np.zeros((2, 3, 2), np.int32)
        H, b, st = api.linearize_batch(ctx, sp, self.many, self.many, (padded, [2, 0]), POSES, fixed_index=[0, 0], moving_index=[1, 1])
        assert H.shape == (2, 3, 3)
        H, b, st = api.score_batch(ctx, sp, self.many, self.one, POSES)
        assert H.shape == (2, 3, 3) and b.shape == (2, 3) and len(st) == 2 and api.score_accept(st).tolist() == [False, False]
        H, b, st = api.score_batch(ctx, sp, self.many, self.many, POSES, fixed_index=[1, 1], moving_index=[0, 1])
        index, H, b, st, n_acc = api.score_select(ctx, sp, self.many, self.one, POSES, api.SelectParams(), 2)
        assert index.shape == (0,) and H.shape == (0, 3, 3) and st.shape == (0,) and n_acc == 0
        self.lib.n_selected = [1]
        index, H, b, st, n_acc = api.score_select(ctx, sp, self.many, self.many, POSES, api.SelectParams.relocalizer(), 1, fixed_index=[1, 0], moving_index=[0, 1])
        assert index.tolist() == [0] and H.shape == (1, 3, 3) and b.shape == (1, 3) and st.shape == (1,) and n_acc == 1

    def _two_slice_aligner(self):
        al = api.MultiAligner2D(self.ctx, max_iterations=3, min_num_inliers=2, damping=0.5, termination_chi_epsilon=1e-3)
        al.param_enable_inlier_only_runs = True
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(self.finders[0], sensor_in_robot=(0.2, 0.0, 0.0), min_num_correspondences=2))
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(self.finders[1], sensor_in_robot=(-0.2, 0.0, 3.0),
                                                                                    robustifier=api.RobustifierCauchy(0.02)))
        return al

    def aligner(self):
        ctx = self.ctx
        al = self.al = api.MultiAligner2D(ctx, max_iterations=4, min_num_inliers=3)
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(self.finders[0], min_num_correspondences=2))
        al.setFixed({"points": self.one}); al.setMoving({"points": self.many}); al.setMovingInFixed(POSES[1])
        assert al.compute() == 0 and al.movingInFixed().shape == (3,) and al.informationMatrix().shape == (3, 3) and al.status() == 0
        assert al.iterationStats().shape == (0,)
        al.store_correspondences = True
        al.setPrior(*PRIORS[0])
        assert al.compute() == 0 and al.correspondences(0).shape == (0, 2)
        al.store_correspondences = False

        al2 = self.al2 = self._two_slice_aligner()
        fixed, moving = [self.many, self.one], [self.one, self.many]
        fi, mi = [[1, 0], [0, 0]], [[0, 0], [0, 1]]
        r = al2.compute_batch(fixed, moving, POSES, priors=PRIORS, fixed_index=fi, moving_index=mi, want_stats=True)
        assert r.pose.shape == (2, 3) and r.information.shape == (2, 3, 3) and r.stats.shape == (2, STATS_CAPACITY) and r.pairs is None
        assert r.last_stats().shape == (2,) and r.loop_closure_accept().tolist() == [False, False]
        r = al2.compute_batch(fixed, moving, POSES, priors=PRIORS, fixed_index=fi, moving_index=mi, want_pairs=True)
        assert r.stats is None and len(r.pairs) == 2 and len(r.pairs[0]) == 2 and r.kernel_ms == 0.0
        r = al.compute_batch([self.many], [self.one], POSES)
        assert r.stats is None and r.pairs is None
        r = al.compute_batch([self.many], [self.one], np.zeros((0, 3)), want_stats=True, want_pairs=True)      # an empty batch: no pairs call, nothing timed
        assert r.pose.shape == (0, 3) and r.pairs is None
        assert al2.estimate_work(fixed, moving, POSES, fixed_index=fi, moving_index=mi).shape == (2,)
        assert al.estimate_work([self.many], [self.one], POSES).shape == (2,)

        H, b, st, active = api.score_aligner(al2, fixed, moving, POSES, priors=PRIORS, fixed_index=fi, moving_index=mi)
        assert H.shape == (2, 3, 3) and b.shape == (2, 3) and st.shape == (2,) and active.shape == (2,)
        api.score_aligner(al, [self.many], [self.one], POSES)
        got = api.score_aligner_select(al2, fixed, moving, POSES, api.SelectParams(), 2, priors=PRIORS, fixed_index=fi, moving_index=mi)
        assert got[0].shape == (0,) and got[-1] == 0
        self.lib.n_selected = [1]
        got = api.score_aligner_select(al, [self.many], [self.one], POSES, api.SelectParams.relocalizer(), 1)
        assert got[0].tolist() == [0] and got[1].shape == (1, 3, 3) and got[4].shape == (1,) and got[-1] == 1

        p = self.prepared = al2.prepare_batch(fixed, moving, POSES, PRIORS, fi, mi, want_stats=True)
        q = al.prepare_batch([self.many], [self.one], POSES)
        mark = len(self.lib.trace)
        self.run_a, self.run_b = p.run(), p.run()
        self.calls_of_two_runs = [c[0] for c in self.lib.trace[mark:]]
        self.run_copy = p.run(copy=True)
        p.set_init_poses(POSES[::-1])
        p.run()
        p.begin()
        with pytest.raises(RuntimeError):
            p.begin()
        assert p.wait().stats.shape == (2, STATS_CAPACITY)
        with pytest.raises(RuntimeError):
            p.wait()
        q.begin()
        assert q.wait(copy=True).stats is None
        out = list(api.run_pipelined([p, q, p]))
        assert len(out) == 3 and out[0].pose is not out[2].pose
        out = list(api.run_pipelined([p, q], copy=False))
        assert out[0].pose is p.pose and out[1].pose is q.pose
        ctx.set_option("kernel_timing", 0)
        mark = len(self.lib.trace)
        r = p.run()
        self.calls_of_an_untimed_run = [c[0] for c in self.lib.trace[mark:]]
        assert r.kernel_ms == 0.0
        al.compute_batch([self.many], [self.one], POSES)
        ctx.set_option("kernel_timing", 1)

    def relocalize(self):
        al, al2, sel = self.al, self.al2, api.SelectParams.relocalizer()
        for n_selected in (1, 0):          # a hypothesis passes: the aligner runs on it; none passes: the empty result
            for kw in ({}, {"fixed_index": [1, 0], "moving_index": [0, 0]}):
                self.lib.n_selected = [n_selected]
                r = api.relocalize(al, self.many, self.one if not kw else self.many, POSES, sel, 1, **kw)
                assert r.index.tolist() == [0] * n_selected and r.n_accepted == n_selected and r.accepted.tolist() == [False] * n_selected
                assert r.result.pose.shape == (n_selected, 3) and r.result.information.shape == (n_selected, 3, 3)
            for kw in ({}, {"fixed_index": [[1, 0], [0, 0]], "moving_index": [[0, 0], [0, 1]]}):
                self.lib.n_selected = [n_selected]
                r = api.relocalize(al2, [self.many, self.one], [self.one, self.many], POSES, sel, 1, priors=PRIORS, **kw)
                assert r.index.tolist() == [0] * n_selected and r.n_accepted == n_selected and r.accepted.tolist() == [False] * n_selected
                assert r.result.pose.shape == (n_selected, 3) and r.score_stats.shape == (n_selected,)
            self.lib.n_selected = [n_selected]
            r = api.relocalize(al, [self.many], [self.one], POSES, sel, 1)      # one slice, given as lists: the aligner's form
            assert r.index.tolist() == [0] * n_selected

    def mapping(self):
        ctx = self.ctx
        for vox in (0.0, 0.1):
            for asynchronous in (False, True):
                clip = api.SceneClipperProjective2D(ctx, self.proj, voxelize_resolution=vox, asynchronous=asynchronous)
                clip.setFullScene(self.one); clip.setRobotInLocalMap(POSES[0]); clip.setSensorInRobot((0.2, 0.0, 0.0))
                clipped = clip.compute()
                assert clipped.capacity == 64 and clipped.n_points == (CLOUD_SIZE if asynchronous else 0) and clip.source_indices.shape == (0,)
                target = api.CloudSet.reserved_many(ctx, 2, 64)
                sizes = clip.compute_batch(self.resN, POSES, target)
                assert (sizes is None) if asynchronous else (sizes.shape == (2,))
                clip.compute_batch(self.resN, POSES, target, scene_index=[1, 0])
                assert target.counts.tolist() == list(CLOUD_SIZES[:2])
        for asynchronous in (False, True):
            m = api.MergerProjective2D(ctx, self.proj, merge_threshold=0.25, asynchronous=asynchronous)
            m.setScene(self.res1); m.setMeasurement(self.many, 1); m.setMeasurementInScene(POSES[1])
            assert m.compute() == (-1 if asynchronous else 0) and m.counts == (0, 0, 0)
            assert m.compute_all([self.one, self.many], POSES, indices=[0, 1]) == (-1 if asynchronous else 0)
            assert m.counts == ((0, 0, 0) if asynchronous else [(0, 0, 0)] * 2)
            m.compute_all([self.one], POSES[:1])
            assert self.res1.n_points == (CLOUD_SIZE if asynchronous else 0)
            sizes = m.compute_batch(self.resN, [self.many, self.many], np.zeros((2, 2, 3), np.float32))
            assert (sizes is None and m.counts is None) if asynchronous else (sizes.shape == (2,) and m.counts.shape == (2, 2, 3))
            m.compute_batch(self.resN, [self.many], np.zeros((2, 1, 3), np.float32), scene_index=[1, 0], meas_index=[[1, 0]])

    def preprocessor_and_trackers(self):
        ctx = self.ctx
        ranges = np.linspace(1.0, 2.0, 32, dtype=np.float32).reshape(2, 16)
        pre = self.pre = api.RawDataPreprocessorProjective2D(ctx, range_min=0.5, range_max=10.0, voxelize_resolution=0.0, normal_point_distance=0.2, normal_min_points=3)
        for call in (pre.compute, lambda: pre.refill(self.res1), lambda: pre.compute_into(self.res1)):
            with pytest.raises(RuntimeError):
                call()
        pre.setRawData(ranges, -1.5, 1.5, 0.1, 20.0)
        scans = self.scans = pre.compute()
        assert scans.n_clouds == 2 and scans.n_points == NUM_POINTS and scans.counts.tolist() == list(CLOUD_SIZES[:2]) and scans.counts.dtype == np.int64
        assert pre.refill(scans) is scans
        with pytest.raises(ValueError):
            pre.compute_into(self.res1)
        pre.setRawData(ranges[0], -1.5, 1.5)
        assert pre.compute_into(self.res1) is self.res1 and self.res1.n_points == CLOUD_SIZE

        al = api.MultiAligner2D(ctx, max_iterations=2)
        for s in ((0.2, 0.0, 0.0), (-0.2, 0.0, 3.0)):
            al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(api.CorrespondenceFinderProjective2f(ctx, self.proj), sensor_in_robot=s))
        tb = self.trackers = api.TrackerBatch(ctx, 2, self.proj, pre, al, -1.5, 1.5, 0.1, 20.0, map_capacity=128, clip_voxelize_resolution=0.0)
        tb.reset([0, 1], ranges, ranges[::-1], np.zeros((2, 3)))
        for _ in range(2):                 # the first step makes the scan sets, the second refills them
            pose, status, information = tb.step(ranges, ranges[::-1], [[0.1, 0.0, 0.0], [0.0, 0.1, 0.05]])
            assert pose.shape == (2, 3) and status.tolist() == [0, 0] and information.shape == (2, 3, 3)


@pytest.fixture(scope="module")
def script():
    lib = FakeLib()
    mp = pytest.MonkeyPatch()
    mp.setattr(_capi, "load", lambda build_if_missing=True: lib)
    try:
        s = Script(lib)
        yield s
        s.ctx.close()
    finally:
        mp.undo()


def _as_json(trace):
    return json.loads(json.dumps(trace))


def test_the_calls_are_the_recorded_ones(script):
    want = json.load(open(GOLDEN))
    got = _as_json(script.lib.trace)
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "call %d" % i


def test_every_cloud_set_has_all_its_fields_however_it_was_made(script):
    made_each_way = [script.one, script.many, script.res1, script.resN, script.scans]      # __init__ twice, reserved, reserved_many, the preprocessor
    sets = set(script.ctx._sets)
    assert sets.issuperset(made_each_way + [script.trackers.maps, script.trackers.clipped] + script.trackers.scans)
    for cs in sets:
        for name in ("_pending", "capacity", "n_clouds", "counts"):
            assert hasattr(cs, name), name
    assert script.one.capacity is None and script.scans.capacity is None and script.res1.capacity == 64 and script.trackers.maps.capacity == 128


def test_prepared_runs_share_their_arrays_and_a_copy_does_not(script):
    a, b, c = script.run_a, script.run_b, script.run_copy
    for name in ("pose", "information", "status", "iterations", "stats"):
        assert np.shares_memory(getattr(a, name), getattr(b, name)), name
        assert not np.shares_memory(getattr(a, name), getattr(c, name)), name
    assert np.shares_memory(a.pose, script.prepared.pose)


def test_a_prepared_run_makes_the_launch_and_the_three_timing_reads_only(script):
    one_run = ["lsm2d_align_batch", "lsm2d_last_kernel_ms", "lsm2d_get_option", "lsm2d_get_option"]
    assert script.calls_of_two_runs == one_run + one_run
    assert script.calls_of_an_untimed_run == ["lsm2d_align_batch"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_api_calls_cpu.py --write      (writes %s from the api.py it runs on)" % GOLDEN)
    lib = FakeLib()
    _capi.load = lambda build_if_missing=True: lib
    Script(lib)
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in lib.trace) + "\n]\n")
    print("%d calls, %d bytes" % (len(lib.trace), os.path.getsize(GOLDEN)))
