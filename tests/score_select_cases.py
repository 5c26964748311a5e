"""The small hypothesis workload of the lsm2d_score_select tests and what the CPU oracle says about it (not a test module): one scan of 128 beams as the
fixed cloud, a map of 600 points as the moving one, about 300 poses scattered around the truth -- shared by the CPU check that the workload exercises every
condition of the acceptance test (test_score_select_abi.py) and by the GPU tests (test_gpu_score_select.py)."""
import numpy as np

from srrg2_laser_slam_2d_amd import api, synth

COLS = 128
N_MAP = 600
N_HYP = 300
TAU = 0.01
MD = 0.3
KINDS = ["proj", "nn", "kd", "dm"]


class Cases:
    pass


def make_cases() -> Cases:
    c = Cases()
    wl = synth.make_workload(1, N_MAP, seed=5, n_beams=COLS, map_noise=0.004, scan_noise=0.004)
    c.wl, c.scan, c.map = wl, np.ascontiguousarray(wl.scan_points), np.ascontiguousarray(wl.map_points)
    rng = np.random.default_rng(3)
    d = rng.uniform(-1.0, 1.0, (N_HYP, 3)) * np.array([0.25, 0.25, 0.12])
    c.poses = np.ascontiguousarray(wl.x0[0][None, :] + d, np.float32)
    c.poses[0] = wl.x0[0]
    c.poses[1] = [1000.0, 1000.0, 0.3]      # a hypothesis that finds nothing: without a robustifier the only one whose inlier ratio is not 1
    return c


def oracle_slice(po, kind, robust):
    if kind == "proj":
        return po.slice_params(canvas_cols=COLS, robustifier=robust, chi_threshold=TAU)
    fk = dict(nn=po.FINDER_NN, kd=po.FINDER_KDTREE_APPROX, dm=po.FINDER_DISTMAP)[kind]
    return po.slice_params(finder=fk, max_distance=MD, robustifier=robust, chi_threshold=TAU)


def oracle_pairs(po, c, kind):
    """po.find for every hypothesis (the pairs depend on neither the robustifier nor the order of summation)"""
    osp = oracle_slice(po, kind, po.ROBUST_NONE)
    return [po.find(osp, c.scan, c.map, p) for p in c.poses]


def oracle_rows(po, c, kind, robust, order, pairs):
    """(H [n, 3, 3], b [n, 3], stats STATS_DTYPE [n]) of every hypothesis: the sequential factor for "sum_order" 1, the kernels' tree order for 0"""
    osp = oracle_slice(po, kind, robust)
    lin = po.linearize if order else po.linearize_device_order
    n = len(c.poses)
    H = np.zeros((n, 3, 3), np.float32); b = np.zeros((n, 3), np.float32); st = np.zeros(n, api.STATS_DTYPE)
    for i in range(n):
        Hi, bi, s = lin(osp, c.scan, c.map, pairs[i], c.poses[i])
        H[i] = np.asarray(Hi, np.float32).reshape(3, 3); b[i] = bi
        st[i] = (s.n_corr, s.n_in, s.n_out, s.chi_in, s.chi_out, s.pair_digest_lo, s.pair_digest_hi)
    return H, b, st


def quotients(st):
    """the two fp32 quotients of the acceptance test, as the kernel forms them"""
    n_in = st["n_inliers"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        return st["chi_inliers"] / np.maximum(n_in, np.float32(1.0)), n_in / np.maximum(st["n_correspondences"], 1).astype(np.float32)


def middle_thresholds(st) -> api.SelectParams:
    """every threshold the exact value of an item in the middle of the distinct values: each condition alone passes that item (>= / <= at equality) and rejects
    another as soon as two values are distinct"""
    per_inlier, ratio = quotients(st)
    u_n = np.unique(st["n_inliers"]); u_c = np.unique(per_inlier[~np.isnan(per_inlier)]); u_r = np.unique(ratio)
    return api.SelectParams(int(u_n[len(u_n) // 2]), float(u_c[(len(u_c) - 1) // 2]), float(u_r[len(u_r) // 2]))


def conditions(st, sel: api.SelectParams):
    """the three conditions one by one: bool [3, n]"""
    per_inlier, ratio = quotients(st)
    with np.errstate(invalid="ignore"):
        return np.stack([st["n_inliers"] >= sel.min_inliers, per_inlier <= np.float32(sel.max_chi_per_inlier), ratio >= np.float32(sel.min_inlier_ratio)])


def many_poses(c: Cases, n: int, seed: int = 11) -> np.ndarray:
    """n distinct hypotheses around the truth (float32 [n, 3]), the first the start pose itself"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([0.25, 0.25, 0.12])
    p = np.ascontiguousarray(c.wl.x0[0][None, :] + d, np.float32)
    p[0] = c.wl.x0[0]
    return p
