"""The small candidate workload of the lsm2d_align_select tests and what the CPU oracle says about it (not a test module; it follows score_select_cases.py):
one scan of 128 beams as the fixed cloud, a map of 600 points as the moving one, about 300 start poses within +-(0.25 m, 0.25 m, 0.12 rad) of the truth, one
pose at (1000, 1000, 0.3) that finds nothing, and exact duplicates of a few candidates at distant indices.  The aligner runs 5 iterations with Cauchy 0.01 and
a ``min_num_inliers`` in the middle of the oracle's inlier counts, so that some candidates end NotEnoughInliers.  Shared by the CPU check that the workload
exercises every term of the verdict (test_align_select_abi.py) and by the GPU tests (test_gpu_align_select.py)."""
import numpy as np

import score_select_cases as sc
from srrg2_laser_slam_2d_amd import api, synth

COLS = 128
N_MAP = 600
N_CAND = 300
TAU = 0.01
MD = 0.3
ITERATIONS = 5
MIN_CORR = 10
NOISE = 0.1      # metres, on map and scan: at the 5 iterations' end the residuals straddle the Cauchy threshold, so the candidates' inlier counts differ
# (original, copy): the copy's start pose is the original's, bit for bit.  The originals are candidates the middle thresholds accept for the projective and the
# grid finder in both orders of summation (test_align_select_abi.py checks that they are), so equal keys reach the index tie-break.
DUPLICATES = ((8, 250), (14, 291), (8, 180))


class Cases:
    pass


def make_cases() -> Cases:
    c = Cases()
    wl = synth.make_workload(1, N_MAP, seed=5, n_beams=COLS, map_noise=NOISE, scan_noise=NOISE)
    c.wl, c.scan, c.map = wl, np.ascontiguousarray(wl.scan_points), np.ascontiguousarray(wl.map_points)
    rng = np.random.default_rng(3)
    d = rng.uniform(-1.0, 1.0, (N_CAND, 3)) * np.array([0.25, 0.25, 0.12])
    c.poses = np.ascontiguousarray(wl.x0[0][None, :] + d, np.float32)
    c.poses[0] = wl.x0[0]
    c.poses[1] = [1000.0, 1000.0, 0.3]      # finds nothing: NotEnoughCorrespondences after one iteration
    for src, dst in DUPLICATES:
        c.poses[dst] = c.poses[src]
    return c


def oracle_slice(po, kind, robust):
    if kind == "proj":
        return po.slice_params(canvas_cols=COLS, robustifier=robust, chi_threshold=TAU, min_num_correspondences=MIN_CORR)
    fk = dict(nn=po.FINDER_NN, kd=po.FINDER_KDTREE_APPROX, dm=po.FINDER_DISTMAP)[kind]
    return po.slice_params(finder=fk, max_distance=MD, robustifier=robust, chi_threshold=TAU, min_num_correspondences=MIN_CORR)


class Results:
    """what an aligner leaves for n candidates: pose [n, 3], H [n, 3, 3], status [n], iterations [n], stats STATS_DTYPE [n, capacity]"""

    def __init__(self, n, capacity):
        self.pose = np.zeros((n, 3), np.float32); self.H = np.zeros((n, 3, 3), np.float32)
        self.status = np.zeros(n, np.int32); self.iterations = np.zeros(n, np.int32); self.stats = np.zeros((n, capacity), api.STATS_DTYPE)

    def last(self):
        return api.last_stats_rows(self.iterations, self.stats)


def oracle_results(po, c, kind, robust, device_order, min_num_inliers, poses=None, iterations=ITERATIONS, scan=None, map_=None) -> Results:
    """po.align per candidate: the sequential fp32 oracle (what "sum_order" 1 must equal) or its device-order mirror (the default order)"""
    poses = c.poses if poses is None else poses
    scan = c.scan if scan is None else scan; map_ = c.map if map_ is None else map_
    osp = oracle_slice(po, kind, robust)
    ap = po.aligner_params(iterations, min_num_inliers=min_num_inliers, device_order=bool(device_order))
    r = Results(len(poses), max(iterations, 1))
    for i, x in enumerate(poses):
        o = po.align(ap, [osp], [scan], [map_], x)
        r.pose[i] = o["pose"]; r.H[i] = np.asarray(o["H"], np.float32).reshape(3, 3); r.status[i] = o["status"]; r.iterations[i] = o["iterations"]
        for t, s in enumerate(o["stats"]):
            r.stats[i, t] = (s.n_corr, s.n_in, s.n_out, s.chi_in, s.chi_out, s.pair_digest_lo, s.pair_digest_hi)
    return r


def middle_min_inliers(po, c, kind, robust, device_order) -> int:
    """``min_num_inliers`` in the middle of the oracle's inlier counts: the median of the last rows' n_inliers over the candidates that found something.  The
    aligner looks at it only after its loop (last row's inliers below it: NotEnoughInliers), so nothing else of a candidate's result depends on it."""
    r = oracle_results(po, c, kind, robust, device_order, 0)
    n_in = r.last()["n_inliers"][r.status == 0]
    return int(np.sort(n_in)[len(n_in) // 2])


def middle_thresholds(last_rows) -> api.SelectParams:
    """score_select_cases.middle_thresholds on the rows given (the Success candidates' last rows): every threshold an item's own fp32 value"""
    return sc.middle_thresholds(last_rows)


def status_thresholds(last_rows) -> api.SelectParams:
    """Thresholds under which the STATUS term decides.  A candidate ends NotEnoughInliers exactly when its last row has fewer inliers than
    ``min_num_inliers``, and every Success candidate has at least that many: thresholds taken from the Success rows alone can never pass a candidate that
    is not Success.  These are taken from the rows of ALL candidates that started an iteration, a quarter of the way up the distinct inlier counts and
    ratios and three quarters of the way up the distinct chi^2 per inlier -- each still an item's own fp32 value -- so candidates below ``min_num_inliers``
    pass them."""
    per_inlier, ratio = sc.quotients(last_rows)
    u_n = np.unique(last_rows["n_inliers"]); u_c = np.unique(per_inlier[~np.isnan(per_inlier)]); u_r = np.unique(ratio)
    return api.SelectParams(int(u_n[len(u_n) // 4]), float(u_c[(3 * (len(u_c) - 1)) // 4]), float(u_r[len(u_r) // 4]))


def conditions(last_rows, sel):
    return sc.conditions(last_rows, sel)


def plain_loop_rank(status, iterations, stats, sel: api.SelectParams, k: int):
    """The verdict as a plain Python loop over the candidates (fp32 through numpy scalars): what api.align_rank restates with arrays"""
    keyed = []
    n_success = 0
    for i in range(len(status)):
        n_success += int(status[i] == 0)
        if status[i] != 0 or iterations[i] < 1:
            continue
        row = stats[i, iterations[i] - 1]
        n_in, n_c, chi = int(row["n_inliers"]), int(row["n_correspondences"]), np.float32(row["chi_inliers"])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            per_inlier = chi / np.float32(max(np.float32(n_in), np.float32(1.0)))
            ratio = np.float32(n_in) / np.float32(max(n_c, 1))
        if n_in >= sel.min_inliers and per_inlier <= np.float32(sel.max_chi_per_inlier) and ratio >= np.float32(sel.min_inlier_ratio):
            keyed.append((-n_in, int(np.float32(chi).view(np.uint32)), i))
    keyed.sort()
    return np.int32([t[2] for t in keyed[:k]]), len(keyed), n_success


def cyclic(c: Cases, n: int) -> np.ndarray:
    """n start poses: the workload's, repeated cyclically"""
    return np.ascontiguousarray(c.poses[np.arange(n) % len(c.poses)])
