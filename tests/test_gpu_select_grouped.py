"""GPU tests of the grouped select calls (lsm2d_score_select_grouped, lsm2d_score_aligner_select_grouped, lsm2d_align_select_grouped: the siblings' scoring
or alignment, then k_select_group_one -- or k_select_keys_seg / k_select_tile_seg / k_select_gather_group when a group is larger than a tile -- on the rows
where they lie).  Every group's block must be exactly what api.score_rank_grouped / api.align_rank_grouped -- a plain loop of the ungrouped restatements
over the groups -- select from the rows of the same items, with the rows' own bits.  The rows come from the CPU oracle where the batch is small and from the
ungrouped device calls (score_batch, score_aligner, compute_batch: unchanged code, held to the oracle by their own tests) elsewhere.  Every comparison is on
integers: indices, counts, and row words as bit patterns."""
import ctypes as C
import math

import numpy as np
import pytest

import align_select_cases as acases
import score_aligner_cases as sacases
import score_select_cases as scases
import select_grouped_cases as gc
from srrg2_laser_slam_2d_amd import _capi, api, synth
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT

pytestmark = pytest.mark.gpu

T = api.SELECT_TILE
MAX_K = api.SELECT_MAX_K
EVERYTHING = api.SelectParams(0, float("inf"), 0.0)
NOTHING = api.SelectParams(10 ** 9, 0.0, 2.0)
KS = (1, 2, 7, 64, 1024)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture()
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)


# ==== the score form ==============================================================================================================================================
@pytest.fixture(scope="module")
def cs(ctx):
    c = scases.make_cases()
    c.scan_set = api.CloudSet(ctx, c.scan)
    c.map_set = api.CloudSet(ctx, c.map)
    c.pairs = {}
    return c


def _finder(ctx, kind):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(scases.COLS, -math.pi, math.pi, 0.3, 30.0))
    if kind == "nn":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=scases.MD, search="exact")
    if kind == "kd":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=scases.MD, search="kdtree")
    return api.CorrespondenceFinderNN2D(ctx, max_distance_m=scases.MD)


def _slice(ctx, kind="proj", robust=api.ROBUST_CAUCHY):
    sp = _finder(ctx, kind).slice_params()
    sp.robustifier = robust; sp.chi_threshold = scases.TAU
    return sp


def _check_score(got, H, b, st, off, sel, k, tag, active=None, got_active=None):
    """got = (index, H, b, stats, n_accepted) of a grouped score call; (H, b, st) the rows of ALL items"""
    index, gH, gb, gst, n_acc = got
    want, want_acc = api.score_rank_grouped(st, off, sel, k, active)
    assert n_acc.dtype == np.int32 and np.array_equal(n_acc, want_acc), (tag, n_acc.tolist(), want_acc.tolist())
    assert len(index) == len(off) - 1 == len(gH) == len(gb) == len(gst)
    for g, w in enumerate(want):
        assert index[g].dtype == np.int32 and np.array_equal(index[g], w), (tag, g, index[g][:16], w[:16])
        assert gH[g].shape == (len(w), 3, 3) and gb[g].shape == (len(w), 3) and gst[g].shape == (len(w),), (tag, g)
        assert np.array_equal(_u32(gH[g]), _u32(H[w])) and np.array_equal(_u32(gb[g]), _u32(b[w])), (tag, g)
        assert gst[g].tobytes() == np.ascontiguousarray(st[w]).tobytes(), (tag, g)
        if got_active is not None:
            assert np.array_equal(got_active[g], active[w]), (tag, g)
    return want, want_acc


@pytest.mark.parametrize("robust", [api.ROBUST_NONE, api.ROBUST_CAUCHY], ids=["plain", "cauchy"])
@pytest.mark.parametrize("kind", scases.KINDS)
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_score_against_the_oracle(order_ctx, po, cs, kind, robust):
    ctx = order_ctx
    order = ctx.get_option("sum_order")
    if kind not in cs.pairs:
        cs.pairs[kind] = scases.oracle_pairs(po, cs, kind)
    H, b, st = scases.oracle_rows(po, cs, kind, po.ROBUST_CAUCHY if robust == api.ROBUST_CAUCHY else po.ROBUST_NONE, order, cs.pairs[kind])
    sel = scases.middle_thresholds(st)
    sp = _slice(ctx, kind, robust)
    n = len(cs.poses)
    args = (ctx, sp, cs.scan_set, cs.map_set, cs.poses)
    for sizes, k in (([n], 64), (gc.SIZES_GRAINS, 7), (gc.SIZES_GRAINS, 64), (gc.SIZES_MIXED, gc.K_MIXED), ([1] * n, 2)):
        off = gc.offsets(sizes)
        want, n_acc = _check_score(api.score_select_grouped(*args, off, sel, k), H, b, st, off, sel, k, (kind, robust, order, len(sizes), k))
        assert int(n_acc.sum()) == api.score_rank(st, sel, 1)[1] > 0
    kd = gc.kinds(n_acc, [1] * n, 2)
    assert kd["none"] and kd["some"]      # 300 groups of one: accepted or not
    # one group: the block is lsm2d_score_select's output, word for word
    one = api.score_select(*args, sel, 64); grp = api.score_select_grouped(*args, [0, n], sel, 64)
    assert np.array_equal(one[0], grp[0][0]) and one[4] == int(grp[4][0])
    assert np.array_equal(_u32(one[1]), _u32(grp[1][0])) and np.array_equal(_u32(one[2]), _u32(grp[2][0])) and one[3].tobytes() == grp[3][0].tobytes()
    assert ctx.last_kernel_ms() > 0.0


@pytest.fixture(scope="module")
def large(ctx, cs):
    """3 T + 7 hypotheses scored once by api.score_batch; duplicates of the best pose of all on both sides of the first tile boundary of the first group of
    SIZES_TWO_TILES (every other item of T - 9 .. T + 9) and on both sides of the boundary between the first two groups of SIZES_TILE_EDGES (T - 2, T - 1)"""
    n = 3 * T + 7
    poses = scases.many_poses(cs, n)
    sp = _slice(ctx)
    st0 = api._stats_array(api.score_batch(ctx, sp, cs.scan_set, cs.map_set, poses)[2])
    best = int(api.score_rank(st0, EVERYTHING, 1)[0][0])
    same = np.concatenate([np.arange(T - 9, T + 10, 2), [T - 2]])
    poses[same] = poses[best]
    H, b, st = api.score_batch(ctx, sp, cs.scan_set, cs.map_set, poses)
    st = api._stats_array(st)
    tied = np.sort(np.unique(np.append(same, best)))
    assert len(set(st[i].tobytes() for i in tied)) == 1 and st["n_inliers"][best] > 0
    return poses, H, b, st, scases.middle_thresholds(st), tied


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sizes", [gc.SIZES_TILE_EDGES, gc.SIZES_TWO_TILES], ids=["tile_edges", "two_tiles"])
def test_score_one_tile_launch_and_segmented_passes(ctx, cs, large, sizes, k):
    """T - 1, T, T + 1, 7: a group past the tile next to one-tile groups; 2 T + 1, 0, T + 6: two passes for the first group at k = 1024 (3 tiles, then 2)"""
    poses, H, b, st, mid, tied = large
    sp = _slice(ctx)
    off = gc.offsets(sizes)
    for sel in (mid, EVERYTHING):
        want, n_acc = _check_score(api.score_select_grouped(ctx, sp, cs.scan_set, cs.map_set, poses, off, sel, k), H, b, st, off, sel, k, (sizes, k))
        if sel is EVERYTHING:
            assert n_acc.tolist() == sizes
            g = 0
            t_g = tied[(tied >= off[g]) & (tied < off[g + 1])]      # the copies lead their group's ranking, by index
            m = min(k, len(t_g))
            assert len(t_g) >= 2 and np.array_equal(want[g][:m], t_g[:m])
    if sizes is gc.SIZES_TILE_EDGES:      # the copy at T - 1 is the first item of group 1: it leads there, alone
        assert want[1][0] == T - 1


def test_score_only_one_tile_groups_at_the_tile(ctx, cs, large):
    """every group at most a tile: the one launch, with groups of exactly T and of T - 1 items"""
    poses, H, b, st, mid, _ = large
    sp = _slice(ctx)
    sizes = [T, 0, T - 1, 1, 7, T]
    off = gc.offsets(sizes)
    n = int(off[-1])
    for k in (1, 1024):
        _check_score(api.score_select_grouped(ctx, sp, cs.scan_set, cs.map_set, poses[:n], off, mid, k), H[:n], b[:n], st[:n], off, mid, k, ("one tile", k))


def test_score_groups_equal_the_ungrouped_call_on_the_sub_batch(ctx, cs, large):
    poses, H, b, st, mid, _ = large
    sp = _slice(ctx)
    off = gc.offsets(gc.SIZES_TILE_EDGES)
    k = 64
    index, gH, gb, gst, n_acc = api.score_select_grouped(ctx, sp, cs.scan_set, cs.map_set, poses, off, mid, k)
    for g in (0, 2, 3):      # a one-tile group, the group past the tile, the small one
        lo, hi = int(off[g]), int(off[g + 1])
        one = api.score_select(ctx, sp, cs.scan_set, cs.map_set, poses[lo:hi], mid, k)
        assert np.array_equal(one[0] + lo, index[g]) and one[4] == int(n_acc[g]), g
        assert np.array_equal(_u32(one[1]), _u32(gH[g])) and np.array_equal(_u32(one[2]), _u32(gb[g])) and one[3].tobytes() == gst[g].tobytes(), g


def test_score_duplicates_in_adjacent_groups(ctx, cs):
    """the same pose as the last item of one group and the first of the next: each is ranked in its own group; the tie-break never crosses the boundary"""
    sp = _slice(ctx)
    poses = cs.poses.copy()
    off = gc.offsets(gc.SIZES_GRAINS)
    a, bnd = int(off[4]) - 1, int(off[4])      # items 65 | 66: the boundary between the groups of 63 and 64
    poses[a] = poses[0]; poses[bnd] = poses[0]; poses[bnd + 1] = poses[0]
    H, b, st = api.score_batch(ctx, sp, cs.scan_set, cs.map_set, poses)
    st = api._stats_array(st)
    assert st[a].tobytes() == st[bnd].tobytes() == st[bnd + 1].tobytes()
    want, _ = _check_score(api.score_select_grouped(ctx, sp, cs.scan_set, cs.map_set, poses, off, EVERYTHING, MAX_K), H, b, st, off, EVERYTHING, MAX_K, "adjacent")
    assert a in want[3].tolist() and bnd not in want[3].tolist()
    j = want[4].tolist().index(bnd)
    assert want[4][j + 1] == bnd + 1 and a not in want[4].tolist()


# ==== the score-aligner form ========================================================================================================================================
@pytest.fixture(scope="module")
def sa(ctx):
    c = sacases.make_inputs()
    which = [0, 1]      # the projective slice with S0, the exact NN slice with S1: two slices with sensor offsets
    fixed, moving = [], []
    for s in which:
        off = np.zeros(c.n + 1, np.int32); off[1:] = np.cumsum([len(a) for a in c.fixed[s]])
        fixed.append(api.CloudSet(ctx, np.concatenate(c.fixed[s]), off)); moving.append(api.CloudSet(ctx, c.moving[s]))
    c.fx, c.mv = fixed, moving
    n = 300
    rng = np.random.default_rng(11)
    c.scan = (np.arange(n) % c.n).astype(np.int32)
    c.hyp = (c.poses[c.scan] + rng.uniform(-0.03, 0.03, (n, 3)).astype(np.float32)).astype(np.float32)
    c.hyp[5::7] = c.hyp[4::7][: len(c.hyp[5::7])]; c.scan[5::7] = c.scan[4::7][: len(c.scan[5::7])]      # ties
    c.hyp[3::11, :2] += np.float32(500.0)       # nothing in reach: active 0, here and there
    c.hyp[40:50, :2] += np.float32(500.0)       # ... and a whole group of them
    c.sizes = [0, 40, 10, 0, 100, 150]
    c.priors = [sacases.asym_prior(X, seed=3) for X in c.hyp]
    return c


def _sa_aligner(ctx):
    al = api.MultiAligner2D(ctx, max_iterations=1, min_num_inliers=10)
    for s in (0, 1):
        kind, cols, md, tau = sacases.SLICES[s]
        finder = (api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0)) if kind == "proj"
                  else api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=md, search="exact"))
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(
            finder, sensor_in_robot=sacases.S_OFF[s], robustifier=None if tau is None else api.RobustifierCauchy(tau), min_num_correspondences=sacases.MIN_CORR))
    return al


@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_score_aligner_grouped(order_ctx, sa):
    ctx = order_ctx
    al = _sa_aligner(ctx)
    kw = dict(fixed_index=np.stack([sa.scan, sa.scan]), priors=sa.priors)
    H, b, st, active = api.score_aligner(al, sa.fx, sa.mv, sa.hyp, **kw)
    off = gc.offsets(sa.sizes)
    assert np.all(active[40:50] == 0) and np.any(active[:40] == 0) and np.any(active[:40] > 0) and np.any(active[50:] == 0)
    mid = api.SelectParams(int(np.median(st["n_inliers"][active > 0])), 0.015, 0.9)
    for sel, k in ((EVERYTHING, 64), (EVERYTHING, 7), (mid, 16), (NOTHING, 5)):
        got = api.score_aligner_select_grouped(al, sa.fx, sa.mv, sa.hyp, off, sel, k, **kw)
        want, n_acc = _check_score(got[:4] + got[5:], H, b, st, off, sel, k, ("score_aligner", sel, k), active=active, got_active=got[4])
        assert n_acc[0] == n_acc[2] == n_acc[3] == 0      # empty groups, and the group in which every item is inactive
        if sel is EVERYTHING:
            assert n_acc[1] == int(np.sum(active[:40] > 0)) < 40 and n_acc[4] > k
    n_mid = api.score_rank(st, mid, 1, active)[1]
    assert 0 < n_mid < int(np.sum(active > 0))
    # one group: lsm2d_score_aligner_select's output
    one = api.score_aligner_select(al, sa.fx, sa.mv, sa.hyp, EVERYTHING, 64, **kw)
    grp = api.score_aligner_select_grouped(al, sa.fx, sa.mv, sa.hyp, [0, 300], EVERYTHING, 64, **kw)
    assert np.array_equal(one[0], grp[0][0]) and one[3].tobytes() == grp[3][0].tobytes() and np.array_equal(one[4], grp[4][0]) and one[5] == int(grp[5][0])
    assert np.array_equal(_u32(one[1]), _u32(grp[1][0])) and np.array_equal(_u32(one[2]), _u32(grp[2][0]))


# ==== the align form ================================================================================================================================================
SMALL_COLS, SMALL_MAP, SMALL_ITS = 64, 300, 3


def _al_finder(ctx, kind, cols):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0))
    return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=acases.MD, search="exact")


def _aligner(ctx, kind="proj", iterations=acases.ITERATIONS, min_num_inliers=10, cols=acases.COLS):
    al = api.MultiAligner2D(ctx, max_iterations=iterations, min_num_inliers=min_num_inliers)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(_al_finder(ctx, kind, cols), robustifier=api.RobustifierCauchy(acases.TAU),
                                                                      min_num_correspondences=acases.MIN_CORR))
    return al


@pytest.fixture(scope="module")
def small(ctx):
    """test_gpu_align_select.py's small workload: 64-beam scan, 300-point map, 3 iterations, the candidates' start poses repeated cyclically"""
    class S:
        pass
    s = S()
    s.c = acases.make_cases()
    wl = synth.make_workload(1, SMALL_MAP, seed=5, n_beams=SMALL_COLS, map_noise=acases.NOISE, scan_noise=acases.NOISE)
    s.scan_set = api.CloudSet(ctx, np.ascontiguousarray(wl.scan_points)); s.map_set = api.CloudSet(ctx, np.ascontiguousarray(wl.map_points))
    first = _aligner(ctx, iterations=SMALL_ITS, min_num_inliers=0, cols=SMALL_COLS).compute_batch([s.scan_set], [s.map_set], s.c.poses, want_stats=True)
    n_in = first.last_stats()["n_inliers"][first.status == 0]
    s.M = int(np.sort(n_in)[len(n_in) // 2])
    s.aligner = lambda: _aligner(ctx, iterations=SMALL_ITS, min_num_inliers=s.M, cols=SMALL_COLS)
    return s


def _check_align(got, res, off, sel, k, tag):
    """got = api.align_select_grouped's result; res = compute_batch's (want_stats=True) for ALL candidates"""
    want, want_acc, want_suc = api.align_rank_grouped(res.status, res.iterations, res.stats, off, sel, k)
    assert np.array_equal(got.n_accepted, want_acc) and np.array_equal(got.n_success, want_suc), (tag, got.n_accepted.tolist(), want_acc.tolist(), got.n_success.tolist())
    last = api.last_stats_rows(res.iterations, res.stats)
    info = np.asarray(res.information).reshape(-1, 3, 3)
    assert len(got.index) == len(off) - 1
    for g, w in enumerate(want):
        assert got.index[g].dtype == np.int32 and np.array_equal(got.index[g], w), (tag, g, got.index[g][:16], w[:16])
        assert got.pose[g].shape == (len(w), 3) and got.information[g].shape == (len(w), 3, 3), (tag, g)
        assert np.array_equal(_u32(got.pose[g]), _u32(res.pose[w])) and np.array_equal(_u32(got.information[g]), _u32(info[w])), (tag, g)
        assert np.array_equal(got.iterations[g], np.asarray(res.iterations)[w]) and got.last_stats[g].tobytes() == np.ascontiguousarray(last[w]).tobytes(), (tag, g)
    return want, want_acc, want_suc


def _both(al, s, poses, sizes_list, ks, tag):
    res = al.compute_batch([s.scan_set], [s.map_set], poses, want_stats=True)
    ok = res.status == 0
    sels = [EVERYTHING]
    if np.any(ok):
        last = res.last_stats()
        sels += [acases.middle_thresholds(last[ok]), acases.status_thresholds(last[res.iterations >= 1])]
    for sizes in sizes_list:
        off = gc.offsets(sizes)
        for sel in sels:
            for k in ks:
                _check_align(api.align_select_grouped(al, [s.scan_set], [s.map_set], poses, off, sel, k), res, off, sel, k, (tag, len(sizes), k))
    return res


@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_align_groups_of_300(order_ctx, small):
    poses = acases.cyclic(small.c, 300)
    res = _both(small.aligner(), small, poses, [gc.SIZES_ALIGN, gc.SIZES_MIXED, [300]], (7, 64), "300")
    assert all(np.any(res.status == s) for s in (0, 1, 2))
    assert order_ctx.last_kernel_ms() > 0.0
    # one group: lsm2d_align_select's output
    al = small.aligner()
    one = api.align_select(al, [small.scan_set], [small.map_set], poses, EVERYTHING, 64)
    grp = api.align_select_grouped(al, [small.scan_set], [small.map_set], poses, [0, 300], EVERYTHING, 64)
    assert np.array_equal(one.index, grp.index[0]) and (one.n_accepted, one.n_success) == (int(grp.n_accepted[0]), int(grp.n_success[0]))
    assert np.array_equal(_u32(one.pose), _u32(grp.pose[0])) and one.last_stats.tobytes() == grp.last_stats[0].tobytes()


def test_align_1049_candidates(ctx, small):
    poses = acases.cyclic(small.c, 1049)
    _both(small.aligner(), small, poses, [[1024, 25]], (1, 7, MAX_K), "1049")
    _both(small.aligner(), small, poses, [[1] * 1049], (1, 7), "1049 groups of one")      # (1049 x 1024 rows would be above LSM2D_SELECT_MAX_GROUP_ROWS)


def test_align_a_group_past_the_tile(ctx, small):
    """2 T + 9 candidates as 2 T + 1, 0, 8: the segmented passes behind the aligner, the groups' Success counts from the gather's own loop"""
    poses = acases.cyclic(small.c, 2 * T + 9)
    _both(small.aligner(), small, poses, [[2 * T + 1, 0, 8]], (7, MAX_K), "past the tile")


@pytest.mark.parametrize("options", [dict(align_path=0), dict(align_path=1), dict(align_path=2), dict(align_path=3), dict(fast_forward=0), dict(fast_forward=2),
                                     dict(inlier_only_runs=1)], ids=lambda o: "%s=%d" % next(iter(o.items())))
def test_align_under_every_path_and_option(ctx, small, options):
    al = small.aligner()
    if options.get("inlier_only_runs"):
        al.param_enable_inlier_only_runs = True
    defaults = dict(align_path=0, fast_forward=2)
    try:
        for key, v in options.items():
            if key in defaults:
                ctx.set_option(key, v)
        res = _both(al, small, acases.cyclic(small.c, 300), [gc.SIZES_ALIGN], (7,), options)
        if options.get("inlier_only_runs"):
            assert res.stats.shape[1] == 2 * SMALL_ITS and np.any(res.iterations > SMALL_ITS)
        if "align_path" in options and options["align_path"]:
            assert ctx.get_option("last_align_path") == options["align_path"]
    finally:
        for key, v in defaults.items():
            ctx.set_option(key, v)


# ==== refusals ======================================================================================================================================================
class _Out:
    def __init__(self, rows, groups):
        self.index = np.full(rows, -7, np.int32); self.pose = np.full((rows, 3), -7.0, np.float32); self.H = np.full((rows, 9), -7.0, np.float32)
        self.b = np.full((rows, 3), -7.0, np.float32); self.its = np.full(rows, -7, np.int32); self.active = np.full(rows, -7, np.int32)
        self.st = np.full(rows * 7, 0x5A5A5A5A, np.uint32).view(api.STATS_DTYPE)
        self.n_sel = np.full(groups, -7, np.int32); self.n_acc = np.full(groups, -7, np.int32); self.n_suc = np.full(groups, -7, np.int32)

    def untouched(self):
        return bool(np.all(self.index == -7) and np.all(self.pose == -7.0) and np.all(self.H == -7.0) and np.all(self.b == -7.0) and np.all(self.its == -7) and
                    np.all(self.active == -7) and np.all(self.st.view(np.uint32) == 0x5A5A5A5A) and np.all(self.n_sel == -7) and np.all(self.n_acc == -7) and
                    np.all(self.n_suc == -7))


# (n_groups, offsets or None, k, what lsm2d_last_error says); n = 8 items
BAD_GROUPS = [(2, None, 4, "null argument"), (0, [0], 4, "n_groups must be >= 1"), (-1, [0, 8], 4, "n_groups must be >= 1"),
              (3, [0, 5, 4, 8], 4, "group_offsets decrease"), (2, [1, 4, 8], 4, "must start at 0 and end"), (2, [0, 4, 7], 4, "must start at 0 and end"),
              (2, [0, 4, 9], 4, "must start at 0 and end"), (2, [0, -1, 8], 4, "group_offsets decrease"),
              (_capi.SELECT_MAX_GROUP_ROWS // 4 + 1, "many", 4, "above LSM2D_SELECT_MAX_GROUP_ROWS"), (2, [0, 4, 8], 0, "k outside"), (2, [0, 4, 8], MAX_K + 1, "k outside")]


def _offsets_arg(G, offs):
    if offs is None:
        return None
    if isinstance(offs, str):
        a = np.zeros(G + 1, np.int32); a[1:] = 8
        return a
    return np.int32(offs)


def test_refusals_write_nothing_and_launch_nothing(ctx, cs, sa, small):
    lib = ctx._lib
    sp = _slice(ctx)
    sel = EVERYTHING.struct()
    poses = np.ascontiguousarray(cs.poses[:8])
    al = small.aligner()
    api.align_select_grouped(al, [small.scan_set], [small.map_set], acases.cyclic(small.c, 8), [0, 8], EVERYTHING, 4)
    sal = _sa_aligner(ctx)
    bd_sa, keep_sa = sal._batch(sa.fx, sa.mv, sa.hyp[:8], None, np.stack([sa.scan[:8], sa.scan[:8]]), None)
    bd_al, keep_al = al._batch([small.scan_set], [small.map_set], acases.cyclic(small.c, 8), None, None, None)
    ap = al._aligner_params()
    uploads = ctx.get_option("uploads"); path = ctx.get_option("last_align_path")

    def calls(G, off, k, out):
        o = _ptr(off)
        yield "score_select_grouped", lib.lsm2d_score_select_grouped(ctx.handle, C.byref(sp), cs.scan_set.handle, None, cs.map_set.handle, None, 8, _ptr(poses),
                                                                     C.byref(sel), k, G, o, _ptr(out.index), _ptr(out.H), _ptr(out.b), _ptr(out.st), _ptr(out.n_sel),
                                                                     _ptr(out.n_acc))
        yield "score_aligner_select_grouped", lib.lsm2d_score_aligner_select_grouped(ctx.handle, C.byref(bd_sa), C.byref(sel), k, G, o, _ptr(out.index), _ptr(out.H),
                                                                                     _ptr(out.b), _ptr(out.st), _ptr(out.active), _ptr(out.n_sel), _ptr(out.n_acc))
        yield "align_select_grouped", lib.lsm2d_align_select_grouped(ctx.handle, C.byref(ap), C.byref(bd_al), C.byref(sel), k, G, o, _ptr(out.index), _ptr(out.pose),
                                                                     _ptr(out.H), _ptr(out.its), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc), _ptr(out.n_suc))

    for G, offs, k, text in BAD_GROUPS:
        out = _Out(16, 4)
        for name, rc in calls(G, _offsets_arg(G, offs), k, out):
            err = lib.lsm2d_last_error(ctx.handle).decode()
            assert rc == BAD_ARGUMENT and out.untouched(), (name, G, offs, k)
            assert name + ":" in err and text in err, (name, text, err)
    # what the ungrouped siblings refuse: a NULL the call needs, a cloud index out of range, a bad descriptor
    out = _Out(16, 4); off = np.int32([0, 4, 8])
    rc = lib.lsm2d_score_select_grouped(ctx.handle, C.byref(sp), cs.scan_set.handle, None, cs.map_set.handle, None, 8, None, C.byref(sel), 4, 2, _ptr(off),
                                        _ptr(out.index), _ptr(out.H), _ptr(out.b), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc))
    assert rc == BAD_ARGUMENT and out.untouched()      # NULL poses
    rc = lib.lsm2d_score_select_grouped(ctx.handle, C.byref(sp), cs.scan_set.handle, None, cs.map_set.handle, None, 8, _ptr(poses), C.byref(sel), 4, 2, _ptr(off),
                                        None, _ptr(out.H), _ptr(out.b), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc))
    assert rc == BAD_ARGUMENT and out.untouched()      # NULL out_index
    fi = np.int32([0, 0, 1, 0, 0, 0, 0, 0])
    rc = lib.lsm2d_score_select_grouped(ctx.handle, C.byref(sp), cs.scan_set.handle, _ptr(fi), cs.map_set.handle, None, 8, _ptr(poses), C.byref(sel), 4, 2, _ptr(off),
                                        _ptr(out.index), _ptr(out.H), _ptr(out.b), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc))
    assert rc == BAD_ARGUMENT and out.untouched() and "score_select_grouped: item 2" in lib.lsm2d_last_error(ctx.handle).decode()
    bd_al.n_slices = 0
    rc = lib.lsm2d_align_select_grouped(ctx.handle, C.byref(ap), C.byref(bd_al), C.byref(sel), 4, 2, _ptr(off), _ptr(out.index), _ptr(out.pose), _ptr(out.H),
                                        _ptr(out.its), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc), _ptr(out.n_suc))
    assert rc == BAD_ARGUMENT and out.untouched() and "bad batch descriptor" in lib.lsm2d_last_error(ctx.handle).decode()
    bd_al.n_slices = 1
    rc = lib.lsm2d_align_select_grouped(ctx.handle, C.byref(ap), C.byref(bd_al), C.byref(sel), 4, 2, _ptr(off), _ptr(out.index), None, _ptr(out.H),
                                        _ptr(out.its), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc), _ptr(out.n_suc))
    assert rc == BAD_ARGUMENT and out.untouched()      # NULL out_pose
    bd_sa.n_slices = 5
    rc = lib.lsm2d_score_aligner_select_grouped(ctx.handle, C.byref(bd_sa), C.byref(sel), 4, 2, _ptr(off), _ptr(out.index), _ptr(out.H), _ptr(out.b), _ptr(out.st),
                                                _ptr(out.active), _ptr(out.n_sel), _ptr(out.n_acc))
    assert rc == BAD_ARGUMENT and out.untouched()
    bd_sa.n_slices = 2
    assert ctx.get_option("uploads") == uploads and ctx.get_option("last_align_path") == path      # nothing was launched
    with pytest.raises(api.Lsm2dError):
        api.score_select_grouped(ctx, sp, cs.scan_set, cs.map_set, poses, [0, 4, 7], EVERYTHING, 4)
    # an empty batch: every group reports zeros, nothing else is written
    out = _Out(16, 4); zero = np.zeros(5, np.int32)
    rc = lib.lsm2d_score_select_grouped(ctx.handle, C.byref(sp), cs.scan_set.handle, None, cs.map_set.handle, None, 0, None, C.byref(sel), 4, 4, _ptr(zero),
                                        _ptr(out.index), _ptr(out.H), _ptr(out.b), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc))
    assert rc == 0 and np.all(out.n_sel == 0) and np.all(out.n_acc == 0) and np.all(out.index == -7) and np.all(out.st.view(np.uint32) == 0x5A5A5A5A)
    # ... and the context works normally afterwards
    for name, rc in calls(2, off, 4, _Out(16, 4)):
        assert rc == 0, name
    got = api.score_select_grouped(ctx, sp, cs.scan_set, cs.map_set, poses, [0, 4, 8], EVERYTHING, 4)
    assert got[4].tolist() == [4, 4] and [len(i) for i in got[0]] == [4, 4]
    res = al.compute_batch([small.scan_set], [small.map_set], acases.cyclic(small.c, 8), want_stats=True)
    _check_align(api.align_select_grouped(al, [small.scan_set], [small.map_set], acases.cyclic(small.c, 8), [0, 4, 8], EVERYTHING, 4), res, np.int32([0, 4, 8]),
                 EVERYTHING, 4, "afterwards")


def test_outputs_beyond_n_selected_are_untouched(ctx, cs):
    sp = _slice(ctx)
    sel = NOTHING.struct(); sel_all = EVERYTHING.struct()
    poses = np.ascontiguousarray(cs.poses[:9])
    off = np.int32([0, 2, 2, 9]); k = 4
    out = _Out(12, 3)
    args = (ctx.handle, C.byref(sp), cs.scan_set.handle, None, cs.map_set.handle, None, 9, _ptr(poses))
    rc = ctx._lib.lsm2d_score_select_grouped(*args, C.byref(sel), k, 3, _ptr(off), _ptr(out.index), _ptr(out.H), _ptr(out.b), _ptr(out.st), _ptr(out.n_sel), _ptr(out.n_acc))
    assert rc == 0 and np.all(out.n_sel == 0) and np.all(out.n_acc == 0) and np.all(out.index == -7) and np.all(out.H == -7.0)
    rc = ctx._lib.lsm2d_score_select_grouped(*args, C.byref(sel_all), k, 3, _ptr(off), _ptr(out.index), None, None, None, _ptr(out.n_sel), _ptr(out.n_acc))
    assert rc == 0 and out.n_sel.tolist() == [2, 0, 4] and out.n_acc.tolist() == [2, 0, 7]
    assert np.all(out.index[[2, 3, 4, 5, 6, 7]] == -7) and np.all(out.index[[0, 1, 8, 9, 10, 11]] >= 0) and np.all(out.H == -7.0)      # slots g * k + j, j < n_selected[g]
