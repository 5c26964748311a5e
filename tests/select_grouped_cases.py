"""Group tables of the lsm2d_*_select_grouped tests and the plain loops they are held to (not a test module).  The workloads are the ungrouped tests' own
(score_select_cases.py, align_select_cases.py, score_aligner_cases.py); what is new is how their items are cut into groups.  Shared by the CPU checks
(test_select_grouped_abi.py) and the GPU tests (test_gpu_select_grouped.py, test_gpu_select_grouped_cpp.py)."""
import numpy as np

from srrg2_laser_slam_2d_amd import api

T = api.SELECT_TILE
K_MIXED = 7
# 300 items.  Boundaries off the 64-lane and the 256-thread grains, an empty group in front:
SIZES_GRAINS = [0, 1, 2, 63, 64, 65, 105]
# 300 candidates of the aligner tests: a group across the split path's limit (192) and the rest
SIZES_ALIGN = [0, 1, 2, 192, 105]
# 300 items cut so that, at k = K_MIXED and the workloads' middle thresholds, all four kinds of group occur (test_select_grouped_abi.py checks it on the
# oracle's rows): empty groups (first, in the middle, last); item 1 alone -- the pose that finds nothing -- accepts nobody; groups of ten accept a few;
# the large groups accept more than k
SIZES_MIXED = [0, 1, 1, 0, 10, 10, 10, 10, 10, 60, 0, 88, 100, 0]
# n = 3 T + 7: one-tile groups at the tile's edge with one group a tile and one item (segmented passes, small groups riding along), and a group of more
# than two tiles next to an empty one
SIZES_TILE_EDGES = [T - 1, T, T + 1, 7]
SIZES_TWO_TILES = [2 * T + 1, 0, T + 6]
assert sum(SIZES_GRAINS) == sum(SIZES_ALIGN) == sum(SIZES_MIXED) == 300 and sum(SIZES_TILE_EDGES) == sum(SIZES_TWO_TILES) == 3 * T + 7


def offsets(sizes) -> np.ndarray:
    """int32 [len(sizes) + 1]: 0, then the running sum"""
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def kinds(n_accepted, sizes, k) -> dict:
    """which groups are empty, accept nobody, accept fewer than k, accept more than k"""
    g = range(len(sizes))
    return dict(empty=[i for i in g if sizes[i] == 0], none=[i for i in g if sizes[i] > 0 and n_accepted[i] == 0],
                some=[i for i in g if 0 < n_accepted[i] < k], more=[i for i in g if n_accepted[i] > k])


def hand_loop_score(st, off, sel: api.SelectParams, k: int, active=None):
    """The grouped verdict on statistics rows as a plain Python loop over groups and items (fp32 through numpy scalars): per group the batch indices of the
    best k accepted items, and the accepted count"""
    index, n_acc = [], []
    for g in range(len(off) - 1):
        keyed = []
        for i in range(int(off[g]), int(off[g + 1])):
            if active is not None and active[i] <= 0:
                continue
            n_in, n_c, chi = int(st["n_inliers"][i]), int(st["n_correspondences"][i]), np.float32(st["chi_inliers"][i])
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                per_inlier = chi / np.float32(max(np.float32(n_in), np.float32(1.0)))
                ratio = np.float32(n_in) / np.float32(max(n_c, 1))
            if n_in >= sel.min_inliers and per_inlier <= np.float32(sel.max_chi_per_inlier) and ratio >= np.float32(sel.min_inlier_ratio):
                keyed.append((-n_in, int(chi.view(np.uint32)), i))
        keyed.sort()
        index.append(np.int32([t[2] for t in keyed[:k]])); n_acc.append(len(keyed))
    return index, np.int32(n_acc)


def hand_loop_align(status, iterations, stats, off, sel: api.SelectParams, k: int):
    """... on an aligner's results: Success, an iteration started, the last started row passes; plus the Success count per group"""
    last = api.last_stats_rows(iterations, stats)
    ok = ((np.asarray(status) == 0) & (np.asarray(iterations) >= 1)).astype(np.int32)
    index, n_acc = hand_loop_score(last, off, sel, k, active=ok)
    n_suc = np.int32([int(np.count_nonzero(np.asarray(status)[int(off[g]):int(off[g + 1])] == 0)) for g in range(len(off) - 1)])
    return index, n_acc, n_suc


def same_lists(a, b) -> bool:
    return len(a) == len(b) and all(x.dtype == np.int32 and np.array_equal(x, y) for x, y in zip(a, b))
