"""GPU tests of lsm2d_score_grid_select: a grid of pose hypotheses made on the device and scored coarse to fine.  Every output, the per-level counts
included, must be bit for bit what score_grid_cases.reference gives on the same context -- a loop over the levels that scores api.grid_level_poses(...) with
lsm2d_score_aligner_select and gathers the parents on the host -- across finders, Cauchy on and off, both orders of summation, one slice and two WithSensor
slices, 1 .. 4 levels, the refinements, pads, empty selections, sets of several clouds; for "sum_order" 1 also the pyramid on the CPU oracle.  No tolerance
appears in this file."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import align_select_cases as ac
import relocalize_cases as rc
import score_grid_cases as gc
from srrg2_laser_slam_2d_amd import _capi, api
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, CAPACITY_EXCEEDED

pytestmark = pytest.mark.gpu

MAX_K = api.SELECT_MAX_K
EVERYTHING, NOTHING = gc.EVERYTHING, gc.NOTHING
FILL = -77


class _Slice(api.AlignerSliceProcessorLaser2DWithSensor):
    """a slice with or without the Cauchy robustifier, the inlier threshold kept either way"""

    def __init__(self, finder, cauchy, sensor_in_robot=(0.0, 0.0, 0.0)):
        super().__init__(finder, sensor_in_robot=sensor_in_robot, robustifier=api.RobustifierCauchy(ac.TAU), min_num_correspondences=ac.MIN_CORR)
        self.cauchy = cauchy

    def slice_params(self):
        return self.param_finder.slice_params(robustifier=_capi.ROBUST_CAUCHY if self.cauchy else _capi.ROBUST_NONE, chi_threshold=ac.TAU,
                                              min_num_correspondences=self.param_min_num_correspondences, sensor_in_robot=self.sensor_in_robot)


def _finder(ctx, kind):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(ac.COLS, -math.pi, math.pi, 0.3, 30.0))
    return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=ac.MD, search="exact" if kind == "nn" else "kdtree")


def _aligner(ctx, kind="proj", cauchy=True, sensors=((0.0, 0.0, 0.0),)):
    al = api.MultiAligner2D(ctx, max_iterations=ac.ITERATIONS, min_num_inliers=0)
    for S in sensors:
        al.param_slice_processors.append(_Slice(_finder(ctx, kind), cauchy, S))
    return al


@pytest.fixture(scope="module")
def cs(ctx):
    c = gc.make_cases()
    c.scan_set = api.CloudSet(ctx, c.scan); c.map_set = api.CloudSet(ctx, c.map)
    fixed, moving, _, _ = rc.two_slice_inputs(c)      # per slice: the scan moved by S^-1 and, as a second cloud, thinned out; the map and a thinned map
    c.fixed2 = [api.CloudSet(ctx, p, o) for p, o in fixed]; c.moving2 = [api.CloudSet(ctx, m) for m in moving]
    thin_scan, thin_map = np.ascontiguousarray(c.scan[::2]), np.ascontiguousarray(c.map[::3])
    c.scan_pair = api.CloudSet(ctx, np.ascontiguousarray(np.concatenate([thin_scan, c.scan])), np.int32([0, len(thin_scan), len(thin_scan) + len(c.scan)]))
    c.map_pair = api.CloudSet(ctx, np.ascontiguousarray(np.concatenate([thin_map, c.map])), np.int32([0, len(thin_map), len(thin_map) + len(c.map)]))
    c.grids = gc.cases(c)
    return c


@pytest.fixture()
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)


def _mid(al, fx, mv, grid, fixed_cloud=None, moving_cloud=None):
    """"mid" on the device's own level-0 rows"""
    poses = api.grid_level_poses(grid, 0)
    ns, n = len(fx), len(poses)
    rep = lambda sets, cl: None if all(s.n_clouds == 1 for s in sets) else np.repeat((np.zeros(ns, np.int32) if cl is None else np.int32(cl))[:, None], n, axis=1)
    _, _, st, active = api.score_aligner(al, fx, mv, poses, None, rep(fx, fixed_cloud), rep(mv, moving_cloud))
    return gc.mid_of(st, active)


def _both(al, fx, mv, grid, coarse, select, k, tag, fixed_cloud=None, moving_cloud=None):
    want = gc.reference(al, fx, mv, grid, coarse, select, k, fixed_cloud, moving_cloud)
    got = api.score_grid_select(al, fx, mv, grid, coarse, select, k, fixed_cloud, moving_cloud)
    print(tag, "counts", got.level_counts.tolist(), "k_parents", grid.k_parents, "k", k, "returned", len(got.pose))
    gc.assert_same(got, want, tag)
    return got


def _run_case(al, fx, mv, cs, name, tag, **kw):
    grid, coarse, last, k = cs.grids[name]
    mid = _mid(al, fx, mv, grid, **kw)
    return _both(al, fx, mv, grid, gc.select_of(coarse, mid), gc.select_of(last, mid), k, (tag, name), **kw)


# ---- 1. the call equals the composition of existing calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cauchy", [True, False], ids=["cauchy", "plain"])
@pytest.mark.parametrize("kind", ["proj", "nn", "kd"])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_equals_the_reference_one_slice(order_ctx, cs, kind, cauchy):
    ctx = order_ctx
    al = _aligner(ctx, kind, cauchy)
    seen = {}
    for name in cs.grids:
        seen[name] = _run_case(al, [cs.scan_set], [cs.map_set], cs, name, (kind, cauchy, ctx.get_option("sum_order")))
    assert ctx.last_kernel_ms() > 0.0
    assert seen["none_at_0"].level_counts.tolist() == [[0, 0]] * 3 and seen["none_deeper"].level_counts.tolist() == [[1, 1], [0, 0], [0, 0]]
    assert all(len(seen[n].pose) > 0 for n in ("single", "two", "three", "four", "big_level0", "big_children", "one_cell", "duplicates"))
    assert seen["big_children"].level_counts[0, 1] == 300


@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_equals_the_reference_two_slices_with_sensor_offsets(order_ctx, cs, kind):
    """two WithSensor slices; the fixed sets hold two clouds each and the call names one of them per slice"""
    ctx = order_ctx
    al = _aligner(ctx, kind, True, rc.S_OFF)
    for fixed_cloud in ([0, 0], [1, 0], [0, 1]):
        for name in ("two", "three", "some", "four", "none_deeper", "duplicates"):
            got = _run_case(al, cs.fixed2, cs.moving2, cs, name, (kind, "two slices", tuple(fixed_cloud)), fixed_cloud=fixed_cloud)
    assert np.all(got.active <= 2) and ctx.last_kernel_ms() > 0.0


def test_sets_of_several_clouds_equal_their_one_cloud_copies(ctx, cs):
    """cloud 1 of a two-cloud scan set against cloud 1 of a two-cloud map set: the same bits as the call on one-cloud sets holding those clouds"""
    al = _aligner(ctx, "proj")
    for name in ("two", "three", "some", "big_children"):
        grid, coarse, last, k = cs.grids[name]
        mid = _mid(al, [cs.scan_set], [cs.map_set], grid)
        a, b = gc.select_of(coarse, mid), gc.select_of(last, mid)
        alone = api.score_grid_select(al, [cs.scan_set], [cs.map_set], grid, a, b, k)
        for fx, mv, fc, mc in (([cs.scan_pair], [cs.map_pair], [1], [1]), ([cs.scan_pair], [cs.map_set], [1], None), ([cs.scan_set], [cs.map_pair], None, [1])):
            got = _both(al, fx, mv, grid, a, b, k, ("several clouds", name), fixed_cloud=fc, moving_cloud=mc)
            gc.assert_same(got, alone, ("one-cloud copies", name))
        other = api.score_grid_select(al, [cs.scan_pair], [cs.map_pair], grid, a, b, k)      # cloud 0 of both: the thinned clouds, another answer
        assert len(other.pose) == 0 or other.stats.tobytes() != alone.stats.tobytes()


# ---- 2. k_parents and k round the accepted counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [(1, 1, 1), (2, 2, 2), (3, 1, 2)])
def test_k_parents_and_k_round_the_accepted_counts(ctx, cs, refine):
    al = _aligner(ctx, "proj")
    fx, mv = [cs.scan_set], [cs.map_set]
    base = dataclasses.replace(cs.grids["some"][0], refine=refine, n_levels=3)
    mid = _mid(al, fx, mv, base)
    n_acc0 = int(api.score_grid_select(al, fx, mv, dataclasses.replace(base, n_levels=1), None, mid, 1).n_accepted)
    assert 2 < n_acc0 < 64
    seen = set()
    for k_parents in (1, 2, n_acc0, n_acc0 + 5):
        grid = dataclasses.replace(base, k_parents=k_parents)
        full = _both(al, fx, mv, grid, mid, mid, MAX_K, ("k_parents", refine))
        assert full.level_counts[0].tolist() == [n_acc0, min(k_parents, n_acc0)]
        seen.add((k_parents > n_acc0, int(full.level_counts[1, 1]) < k_parents))
        n_last = full.n_accepted
        for k in sorted({1, max(n_last, 1), n_last + 3}):      # 1, the accepted count, above it (1024 above)
            got = _both(al, fx, mv, grid, mid, mid, k, ("k", refine, k_parents))
            assert len(got.pose) == min(k, n_last)
            assert got.pose.tobytes() == full.pose[:k].tobytes() and np.array_equal(got.origin, full.origin[:k])
    assert any(t[0] for t in seen)                                  # pads at level 1
    assert refine != (1, 1, 1) or any(t[1] for t in seen)           # ... and at level 2: with one child per parent the count cannot grow back


# ---- 3. "sum_order" 1 against the CPU oracle's pyramid ------------------------------------------------------------------------------------------------------------
def test_reference_order_against_the_cpu_pyramid(ctx, po, cs):
    al = _aligner(ctx, "proj")
    cache = {}
    ctx.set_option("sum_order", 1)
    try:
        for name in ("two", "three", "some", "none_deeper", "duplicates", "big_level0"):
            grid, coarse, last, k = cs.grids[name]
            st0, act0, _ = gc.oracle_rows(po, cs, api.grid_level_poses(grid, 0), cache)
            mid = gc.mid_of(st0, act0)
            a, b = gc.select_of(coarse, mid), gc.select_of(last, mid)
            want, _ = gc.oracle_pyramid(po, cs, grid, a, b, k, cache)
            got = api.score_grid_select(al, [cs.scan_set], [cs.map_set], grid, a, b, k)
            print(name, got.level_counts.tolist())
            gc.assert_same(got, want, ("oracle", name), with_b=False, with_H=False)      # (the oracle's alignment returns the solved system's H; the rows' statistics and digests decide)
    finally:
        ctx.set_option("sum_order", 0)


# ---- 4. refusals, sentinels, repeatability, neighbours ------------------------------------------------------------------------------------------------------------
def _raw(ctx, al, fx, mv, grid, coarse, select, k, rows=None, fixed_cloud=None, moving_cloud=None, n_slices=None, null=()):
    """the bare C call into buffers filled with a pattern; null: names of arguments passed as NULL"""
    slices = al.param_slice_processors
    ns = len(slices)
    sp = (api.SliceParams * ns)(*[s.slice_params() for s in slices])
    fxa = (C.c_void_p * ns)(*[f.handle.value for f in fx]); mva = (C.c_void_p * ns)(*[m.handle.value for m in mv])
    rows = max(k, 1) if rows is None else rows
    levels = max(min(grid.n_levels, 8), 1)
    bufs = dict(pose=np.full((rows, 3), FILL, np.float32), origin=np.full(rows, FILL, np.int32), H=np.full((rows, 9), FILL, np.float32),
                b=np.full((rows, 3), FILL, np.float32), stats=np.full((rows, 7), FILL, np.int32), active=np.full(rows, FILL, np.int32),
                counts=np.full((levels, 2), FILL, np.int32))
    n_sel, n_acc = C.c_int32(FILL), C.c_int32(FILL)
    g = grid.struct(); s0 = None if coarse is None else coarse.struct(); s1 = select.struct()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fc = None if fixed_cloud is None else np.ascontiguousarray(fixed_cloud, np.int32); mc = None if moving_cloud is None else np.ascontiguousarray(moving_cloud, np.int32)
    arg = dict(ctx=ctx.handle, slices=sp, fixed=C.cast(fxa, C.POINTER(C.c_void_p)), moving=C.cast(mva, C.POINTER(C.c_void_p)), grid=C.byref(g),
               coarse=None if s0 is None else C.byref(s0), select=C.byref(s1), pose=p(bufs["pose"]), n_sel=C.byref(n_sel), n_acc=C.byref(n_acc))
    for name in null:
        arg[name] = None
    code = ctx._lib.lsm2d_score_grid_select(arg["ctx"], ns if n_slices is None else n_slices, arg["slices"], arg["fixed"], p(fc), arg["moving"], p(mc), arg["grid"],
                                            arg["coarse"], arg["select"], k, arg["pose"], p(bufs["origin"]), p(bufs["H"]), p(bufs["b"]), p(bufs["stats"]),
                                            p(bufs["active"]), arg["n_sel"], arg["n_acc"], p(bufs["counts"]))
    return code, n_sel.value, n_acc.value, bufs


def _untouched(n_sel, n_acc, bufs):
    return n_sel == FILL and n_acc == FILL and all(np.all(b == (np.float32(FILL) if b.dtype == np.float32 else FILL)) for b in bufs.values())


def test_refusals_leave_the_outputs_alone(ctx, cs):
    al = _aligner(ctx, "proj")
    fx, mv = [cs.scan_set], [cs.map_set]
    good = cs.grids["two"][0]
    R = dataclasses.replace
    nan, inf = float("nan"), float("inf")
    bad_grids = [R(good, count=(0, 5, 3)), R(good, count=(5, 5, -1)), R(good, refine=(2, 0, 2)), R(good, k_parents=0), R(good, k_parents=MAX_K + 1),
                 R(good, n_levels=0), R(good, n_levels=api._capi.GRID_MAX_LEVELS + 1),
                 R(good, step=(-0.1, 0.1, 0.1)), R(good, step=(0.1, nan, 0.1)), R(good, step=(0.1, 0.1, inf)), R(good, center=(nan, 0.0, 0.0)),
                 R(good, center=(0.0, -inf, 0.0)), R(good, count=(1024, 1024, 1)), R(good, count=(1 << 30, 1 << 30, 1 << 30)),
                 R(good, k_parents=1024, refine=(8, 8, 8)), R(good, refine=(1 << 30, 1 << 30, 4))]
    for g in bad_grids:
        code, n_sel, n_acc, bufs = _raw(ctx, al, fx, mv, g, EVERYTHING, EVERYTHING, 4)
        assert code == BAD_ARGUMENT and _untouched(n_sel, n_acc, bufs), g
    for k in (0, -1, MAX_K + 1):
        code, n_sel, n_acc, bufs = _raw(ctx, al, fx, mv, good, EVERYTHING, EVERYTHING, k, rows=4)
        assert code == BAD_ARGUMENT and _untouched(n_sel, n_acc, bufs), k
    for n_slices in (0, 5):
        code, n_sel, n_acc, bufs = _raw(ctx, al, fx, mv, good, EVERYTHING, EVERYTHING, 4, n_slices=n_slices)
        assert code == BAD_ARGUMENT and _untouched(n_sel, n_acc, bufs), n_slices
    for name in ("ctx", "slices", "fixed", "moving", "grid", "select", "pose", "n_sel", "n_acc", "coarse"):
        code, n_sel, n_acc, bufs = _raw(ctx, al, fx, mv, good, EVERYTHING, EVERYTHING, 4, null=(name,))
        assert code == BAD_ARGUMENT and _untouched(n_sel, n_acc, bufs), name
    # coarse_select may be NULL with one level
    code, n_sel, n_acc, bufs = _raw(ctx, al, fx, mv, R(good, n_levels=1, k_parents=0), None, EVERYTHING, 4)
    assert code == 0 and n_sel == 4 and np.all(bufs["pose"][:4] != np.float32(FILL))
    # a cloud index out of range: the message names the slice
    al2 = _aligner(ctx, "proj", True, rc.S_OFF)
    for kw in (dict(fixed_cloud=[0, 2]), dict(fixed_cloud=[0, -1]), dict(moving_cloud=[0, 1])):
        code, n_sel, n_acc, bufs = _raw(ctx, al2, cs.fixed2, cs.moving2, good, EVERYTHING, EVERYTHING, 4, **kw)
        assert code == BAD_ARGUMENT and _untouched(n_sel, n_acc, bufs), kw
        assert b"slice 1" in ctx._lib.lsm2d_last_error(ctx.handle), ctx._lib.lsm2d_last_error(ctx.handle)
    # what lsm2d_score_aligner_select refuses for the slices
    nn = _aligner(ctx, "nn"); nn.param_slice_processors[0].param_finder.param_max_distance_m = 0.0
    code, n_sel, n_acc, bufs = _raw(ctx, nn, fx, mv, good, EVERYTHING, EVERYTHING, 4)
    assert code == BAD_ARGUMENT and _untouched(n_sel, n_acc, bufs)
    wide = _aligner(ctx, "proj"); wide.param_slice_processors[0].param_finder = api.CorrespondenceFinderProjective2f(
        ctx, api.PointNormal2fProjectorPolar(ctx.get_option("max_dyn_lds") // 16 + 64, -math.pi, math.pi, 0.3, 30.0))
    code, n_sel, n_acc, bufs = _raw(ctx, wide, fx, mv, good, EVERYTHING, EVERYTHING, 4)
    assert code == CAPACITY_EXCEEDED and _untouched(n_sel, n_acc, bufs)
    # two batches in flight
    p1 = al.prepare_batch(fx, mv, cs.poses[:8]); p2 = al.prepare_batch(fx, mv, cs.poses[8:16])
    p1.begin(); p2.begin()
    try:
        code, n_sel, n_acc, bufs = _raw(ctx, al, fx, mv, good, EVERYTHING, EVERYTHING, 4)
        assert code == BAD_ARGUMENT and _untouched(n_sel, n_acc, bufs)
    finally:
        p1.wait(); p2.wait()
    # the context is usable and the call still right
    _run_case(al, fx, mv, cs, "two", "after refusals")


def test_positions_beyond_the_count_are_not_written(ctx, cs):
    al = _aligner(ctx, "proj")
    fx, mv = [cs.scan_set], [cs.map_set]
    for name in ("some", "none_at_0", "none_deeper", "four"):
        grid, coarse, last, k = cs.grids[name]
        mid = _mid(al, fx, mv, grid)
        code, n_sel, n_acc, bufs = _raw(ctx, al, fx, mv, grid, gc.select_of(coarse, mid), gc.select_of(last, mid), MAX_K)
        assert code == 0 and n_sel == min(n_acc, MAX_K) < MAX_K
        counts = bufs.pop("counts")
        assert counts[grid.n_levels - 1].tolist() == [n_acc, n_sel] and np.all(counts != FILL)
        for key, b in bufs.items():
            assert np.all(b[n_sel:] == (np.float32(FILL) if b.dtype == np.float32 else FILL)), (name, key)
            assert n_sel == 0 or not np.all(b[:n_sel] == (np.float32(FILL) if b.dtype == np.float32 else FILL)), (name, key)
        n0 = int(np.prod(grid.count))
        assert np.all((bufs["origin"][:n_sel] >= 0) & (bufs["origin"][:n_sel] < n0))


def test_two_runs_give_the_same_bits_and_the_call_is_timed(ctx, cs):
    al = _aligner(ctx, "nn")
    fx, mv = [cs.scan_set], [cs.map_set]
    for name in ("some", "big_children"):
        grid, coarse, last, k = cs.grids[name]
        mid = _mid(al, fx, mv, grid)
        a = api.score_grid_select(al, fx, mv, grid, gc.select_of(coarse, mid), gc.select_of(last, mid), k)
        b = api.score_grid_select(al, fx, mv, grid, gc.select_of(coarse, mid), gc.select_of(last, mid), k)
        gc.assert_same(a, b, name)
        assert a.kernel_ms > 0.0 and b.kernel_ms > 0.0 and ctx.last_kernel_ms() > 0.0


def test_neighbouring_calls_keep_their_bits(ctx, cs):
    """lsm2d_score_aligner_select and lsm2d_align_batch before and after the new call on the same context: the lane's scratch is shared, nobody's answer moves"""
    al = _aligner(ctx, "proj")
    fx, mv = [cs.scan_set], [cs.map_set]

    def neighbours():
        s = api.score_aligner_select(al, fx, mv, cs.poses, EVERYTHING, 64)
        r = al.compute_batch(fx, mv, cs.poses, want_stats=True)
        return (s[0].tobytes(), s[1].tobytes(), s[2].tobytes(), s[3].tobytes(), s[4].tobytes(), s[5],
                r.pose.tobytes(), r.information.tobytes(), r.status.tobytes(), r.iterations.tobytes(), r.stats.tobytes())

    before = neighbours()
    for name in ("big_level0", "big_children", "some"):      # larger and smaller than the neighbours' own layouts
        _run_case(al, fx, mv, cs, name, "between neighbours")
        assert neighbours() == before, name
