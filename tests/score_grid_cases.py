"""The cases of the lsm2d_score_grid_select tests, the composition of existing calls they are held to, and the same pyramid on the CPU oracle (not a test
module).

The workload is relocalize_cases' one-slice one: a 128-beam scan as the fixed cloud, a 600-point map as the moving one, the truth at c.wl.x0[0]; grids are
centred near the truth.  A case names its thresholds -- "mid": the middle of the level-0 rows of the active hypotheses (every threshold an item's own fp32
value, score_select_cases.middle_thresholds), "everything", "nothing" -- and whoever runs it resolves "mid" on the rows it has: the oracle's for the CPU
test, the device's own for the GPU tests.

`reference` is include/lsm2d.h's definition spelled out with existing calls: a loop over the levels that scores api.grid_level_poses(...) with
api.score_aligner_select and gathers the parents on the host.  `oracle_pyramid` is the same loop with po.align(max_iterations=1) rows (the sequential sums:
"sum_order" 1) ranked by api.score_rank."""
import types

import numpy as np

import align_select_cases as ac
import relocalize_cases as rc
from srrg2_laser_slam_2d_amd import api

EVERYTHING, NOTHING = rc.EVERYTHING, rc.NOTHING
STEP = (0.1, 0.1, 0.04)
OFF = (0.013, -0.021, 0.007)      # the grid's centre relative to the truth: no cell sits on it exactly


def make_cases():
    c = rc.make_cases()
    c.center = tuple(float(v) for v in (np.asarray(c.wl.x0[0], np.float32) + np.asarray(OFF, np.float32)))
    return c


def _grid(c, count, n_levels=1, refine=(1, 1, 1), k_parents=1, step=STEP, center=None):
    return api.PoseGrid(center=c.center if center is None else center, step=step, count=count, n_levels=n_levels, refine=refine, k_parents=k_parents)


def cases(c):
    """name -> (grid, coarse thresholds' name, last thresholds' name, k).  What each is for is asserted on the oracle by test_score_grid_abi.py."""
    far = 100.0      # metres: the children of a cell split this wide see nothing of the scan
    return {
        # n_levels 1 .. 4, refine (2, 2, 2) and (3, 1, 2)
        "single":        (_grid(c, (5, 5, 3)), None, "mid", 16),
        "two":           (_grid(c, (5, 5, 3), 2, (2, 2, 2), 8), "everything", "mid", 16),                # m == k_parents < accepted
        "three":         (_grid(c, (4, 4, 2), 3, (3, 1, 2), 5), "everything", "everything", 7),
        "four":          (_grid(c, (3, 3, 2), 4, (2, 2, 2), 4), "everything", "mid", 1024),              # a last level where k exceeds the accepted count
        # pads: 0 < m < k_parents at level 0 (k_parents above the accepted count), and k_parents == the accepted count (see k_parents_cases)
        "some":          (_grid(c, (5, 5, 3), 3, (2, 2, 2), 64), "mid", "everything", 1024),
        "one_parent":    (_grid(c, (5, 5, 3), 2, (2, 2, 2), 1), "mid", "mid", 1),
        "two_parents":   (_grid(c, (5, 5, 3), 2, (3, 1, 2), 2), "mid", "everything", 1024),
        # nothing selected: at level 0, and first at a deeper level (the one cell passes, its children 25 m away see nothing)
        "none_at_0":     (_grid(c, (5, 5, 3), 3, (2, 2, 2), 8), "nothing", "everything", 16),
        "none_deeper":   (_grid(c, (1, 1, 1), 3, (2, 1, 1), 4, step=(far, 0.0, 0.0), center=tuple(float(v) for v in c.wl.x0[0])), "everything", "everything", 16),
        # duplicates ranked by index: a zero step with count 2, and refine (1, 1, 1)
        "duplicates":    (_grid(c, (2, 3, 1), 3, (1, 1, 1), 4, step=(0.0, 0.1, 0.04)), "everything", "everything", 1024),
        # count (1, 1, 1)
        "one_cell":      (_grid(c, (1, 1, 1), 2, (2, 2, 2), 3), "everything", "everything", 1024),
        # past one select tile at level 0 (13^3 = 2197) and below it (300 x 8 = 2400)
        "big_level0":    (_grid(c, (13, 13, 13), 2, (2, 2, 2), 16, step=(0.04, 0.04, 0.02)), "mid", "mid", 16),
        "big_children":  (_grid(c, (8, 8, 6), 2, (2, 2, 2), 300, step=(0.06, 0.06, 0.04)), "everything", "mid", 1024),
    }


def select_of(name, mid):
    return {None: None, "mid": mid, "everything": EVERYTHING, "nothing": NOTHING}[name]


def mid_of(st, active):
    """"mid" on the level-0 rows given"""
    st = np.asarray(st); live = st[np.asarray(active) > 0]
    return ac.middle_thresholds(live) if len(live) else EVERYTHING


def _result(levels, n_levels, k):
    """levels: per level that ran (poses, origins, idx, H, b, stats, active, n_accepted)"""
    counts = np.zeros((n_levels, 2), np.int32)
    for l, lv in enumerate(levels):
        counts[l] = (lv[7], len(lv[2]))
    if len(levels) == n_levels:
        poses, origins, idx, H, b, st, active, n_acc = levels[-1]
        return types.SimpleNamespace(pose=poses[idx], origin=origins[idx].astype(np.int32), H=H, b=b, stats=st, active=active, n_accepted=n_acc, level_counts=counts)
    z = np.zeros      # a level selected nothing: every deeper level reports (0, 0), the final counts are 0
    return types.SimpleNamespace(pose=z((0, 3), np.float32), origin=z(0, np.int32), H=z((0, 3, 3), np.float32), b=z((0, 3), np.float32),
                                 stats=z(0, api.STATS_DTYPE), active=z(0, np.int32), n_accepted=0, level_counts=counts)


def _walk(grid, coarse, select, k, score_select):
    """the loop over the levels; score_select(poses, thresholds, k) -> (idx, H, b, stats, active, n_accepted) stands for lsm2d_score_aligner_select"""
    levels = []
    poses = api.grid_level_poses(grid, 0)
    origins = np.arange(len(poses), dtype=np.int32)
    R = int(np.prod(grid.refine))
    for l in range(grid.n_levels):
        last = l == grid.n_levels - 1
        idx, H, b, st, active, n_acc = score_select(poses, select if last else coarse, k if last else grid.k_parents)
        levels.append((poses, origins, idx, H, b, st, active, n_acc))
        if last or len(idx) == 0:
            break
        poses = api.grid_level_poses(grid, l + 1, poses[idx])      # the parents' poses, bit for bit as they were scored
        origins = np.repeat(origins[idx], R)
    return _result(levels, grid.n_levels, k), levels


def reference(al, fixed, moving, grid, coarse, select, k, fixed_cloud=None, moving_cloud=None):
    """lsm2d_score_grid_select from existing calls: api.score_aligner_select per level over the level's REAL items, the same cloud in every slice for every
    item (constant index arrays, or none for one-cloud sets), the parents gathered on the host"""
    ns = len(fixed)

    def constant(sets, cloud, n):
        if all(s.n_clouds == 1 for s in sets):
            return None
        c = np.zeros(ns, np.int32) if cloud is None else np.asarray(cloud, np.int32).reshape(ns)
        return np.ascontiguousarray(np.repeat(c[:, None], n, axis=1))

    def score_select(poses, thresholds, kk):
        n = len(poses)
        return api.score_aligner_select(al, fixed, moving, poses, thresholds, kk, None, constant(fixed, fixed_cloud, n), constant(moving, moving_cloud, n))

    return _walk(grid, coarse, select, k, score_select)[0]


def oracle_rows(po, c, poses, cache=None):
    """(stats STATS [n], active int32 [n], H [n, 3, 3]) of po.align(max_iterations=1) at every pose: the one-slice projective workload with Cauchy, sequential sums"""
    osp = ac.oracle_slice(po, "proj", po.ROBUST_CAUCHY)
    ap = po.aligner_params(1, min_num_inliers=0, device_order=False)
    st = np.zeros(len(poses), api.STATS_DTYPE); active = np.zeros(len(poses), np.int32); H = np.zeros((len(poses), 3, 3), np.float32)
    for i, x in enumerate(np.ascontiguousarray(poses, np.float32)):
        key = x.tobytes()
        if cache is None or key not in cache:
            o = po.align(ap, [osp], [c.scan], [c.map], x)
            s = o["stats"][0]
            row = ((s.n_corr, s.n_in, s.n_out, s.chi_in, s.chi_out, s.pair_digest_lo, s.pair_digest_hi), int(o["status"] != 1), np.asarray(o["H"], np.float32).reshape(3, 3))
            if cache is not None:
                cache[key] = row
        else:
            row = cache[key]
        st[i], active[i], H[i] = row
    return st, active, H


def oracle_pyramid(po, c, grid, coarse, select, k, cache=None):
    """the pyramid on the CPU oracle; returns (result, levels); b is not restated (zeros)"""
    def score_select(poses, thresholds, kk):
        st, active, H = oracle_rows(po, c, poses, cache)
        idx, n_acc = api.score_rank(st, thresholds, kk, active)
        return idx, H[idx], np.zeros((len(idx), 3), np.float32), st[idx], active[idx], n_acc

    return _walk(grid, coarse, select, k, score_select)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, tag, with_b=True, with_H=True):
    """got: api.score_grid_select's result; want: reference's or the oracle pyramid's.  Bit for bit, the per-level counts included."""
    assert np.array_equal(got.level_counts, want.level_counts), (tag, got.level_counts.tolist(), want.level_counts.tolist())
    assert got.n_accepted == want.n_accepted and len(got.pose) == len(want.pose), (tag, got.n_accepted, want.n_accepted, len(got.pose), len(want.pose))
    assert np.array_equal(u32(got.pose), u32(want.pose)), (tag, "pose")
    assert got.origin.dtype == np.int32 and np.array_equal(got.origin, want.origin), (tag, got.origin[:8], want.origin[:8])
    if with_H:
        assert np.array_equal(u32(got.H), u32(want.H)), (tag, "H")
    if with_b:
        assert np.array_equal(u32(got.b), u32(want.b)), (tag, "b")
    assert got.stats.tobytes() == np.ascontiguousarray(want.stats).tobytes(), (tag, "stats")
    assert np.array_equal(got.active, want.active), (tag, "active")
