"""The workloads of the lsm2d_relocalize_select tests, the two-call route they are held to, and what the CPU oracle says about the one-slice workload (not a
test module).

One slice: align_select_cases.make_cases() -- a 128-beam scan, a 600-point map, 300 poses with duplicates and one that finds nothing, 5 iterations, Cauchy
0.01.  Two slices: the same scan seen by two sensors (WithSensor offsets; the fixed clouds are the scan moved by S^-1, a second cloud of every set is the
scan thinned out, chosen by index arrays), the map and a thinned map as moving clouds, a prior per hypothesis: the shape of score_aligner_cases.

Stage 1 on the oracle: a hypothesis' combined row is the first statistics row of the sequential po.align(max_iterations = 1) -- include/lsm2d.h says so for
"sum_order" 1 -- and it is active unless that alignment ends NotEnoughCorrespondences.  Stage 2 on the oracle: po.align over 5 iterations from the same
pose.  Every threshold is an item's own fp32 value (score_select_cases.middle_thresholds)."""
import types

import numpy as np

import align_select_cases as ac
import score_aligner_cases as sac
from srrg2_laser_slam_2d_amd import api, synth

EVERYTHING = api.SelectParams(0, float("inf"), 0.0)
NOTHING = api.SelectParams(10 ** 9, 0.0, 2.0)
K_SCORES = (1, 2, 7, 64, 257)
S_OFF = [(0.1, -0.05, 0.3), (-0.2, 0.0, 3.0)]


def make_cases():
    return ac.make_cases()


def two_slice_inputs(c):
    """(fixed [2] of (points, offsets), moving [2], fixed_index [2, n], priors [n]) over c.poses"""
    n = len(c.poses)
    fixed = []
    for S in S_OFF:
        inv = synth.invert_poses(np.array([S], np.float64))[0]
        a = sac._move(c.scan, inv); b = np.ascontiguousarray(a[::2])
        fixed.append((np.ascontiguousarray(np.concatenate([a, b])), np.int32([0, len(a), len(a) + len(b)])))
    moving = [c.map, np.ascontiguousarray(c.map[::2])]
    fixed_index = np.ascontiguousarray(np.stack([np.arange(n) % 2, (np.arange(n) // 3) % 2]).astype(np.int32))
    priors = [sac.asym_prior(x, seed=i % 5) for i, x in enumerate(c.poses)]
    return fixed, moving, fixed_index, priors


def two_calls(al, fixed, moving, poses, score_select, k_score, align_select, k, priors=None, fixed_index=None, moving_index=None):
    """lsm2d_score_aligner_select, the host's gather, lsm2d_align_select: every output lsm2d_relocalize_select has, from the two existing calls"""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
    n, ns = len(poses), len(fixed)
    idx, _, _, st, _, n_acc1 = api.score_aligner_select(al, fixed, moving, poses, score_select, k_score, priors, fixed_index, moving_index)
    out = types.SimpleNamespace(scored_index=idx, scored_stats=st, n_scored_accepted=n_acc1, index=np.zeros(0, np.int32), pose=np.zeros((0, 3), np.float32),
                                information=np.zeros((0, 3, 3), np.float32), iterations=np.zeros(0, np.int32), last_stats=np.zeros(0, api.STATS_DTYPE),
                                n_accepted=0, n_success=0)
    if not len(idx):
        return out

    def chosen(sets, index):      # candidate j's cloud in every slice, spelled out
        rows = []
        for s, cs in enumerate(sets):
            full = np.asarray(index)[s] if index is not None else (np.zeros(n, np.int32) if cs.n_clouds == 1 else np.arange(n, dtype=np.int32))
            rows.append(full[idx])
        return np.ascontiguousarray(np.stack(rows), np.int32).reshape(ns, len(idx))

    got = api.align_select(al, fixed, moving, poses[idx], score_select if align_select is None else align_select, k_score if k is None else k,
                           priors=None if priors is None else [priors[int(i)] for i in idx], fixed_index=chosen(fixed, fixed_index),
                           moving_index=chosen(moving, moving_index))
    out.index = idx[got.index].astype(np.int32); out.pose = got.pose; out.information = got.information; out.iterations = got.iterations
    out.last_stats = got.last_stats; out.n_accepted = got.n_accepted; out.n_success = got.n_success
    return out


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, tag):
    """got: api.relocalize_select's result; want: two_calls' (or the oracle's restatement with the same fields)"""
    assert got.n_scored_accepted == want.n_scored_accepted and np.array_equal(got.scored_index, want.scored_index), (tag, got.scored_index[:8], want.scored_index[:8])
    assert got.scored_stats.tobytes() == np.ascontiguousarray(want.scored_stats).tobytes(), tag
    assert (got.n_accepted, got.n_success) == (want.n_accepted, want.n_success), (tag, got.n_accepted, got.n_success, want.n_accepted, want.n_success)
    assert got.index.dtype == np.int32 and np.array_equal(got.index, want.index), (tag, got.index[:8], want.index[:8])
    assert np.array_equal(u32(got.pose), u32(want.pose)) and np.array_equal(u32(got.information), u32(want.information)), tag
    assert np.array_equal(got.iterations, want.iterations) and got.last_stats.tobytes() == np.ascontiguousarray(want.last_stats).tobytes(), tag


# ---- the one-slice projective workload on the CPU oracle ------------------------------------------------------------------------------------------------------
def oracle_stages(po, c):
    """(rows1 STATS [n], active int32 [n], M, full Results): the sequential oracle ("sum_order" 1)"""
    first = ac.oracle_results(po, c, "proj", po.ROBUST_CAUCHY, 0, 0, iterations=1)
    M = ac.middle_min_inliers(po, c, "proj", po.ROBUST_CAUCHY, 0)
    full = ac.oracle_results(po, c, "proj", po.ROBUST_CAUCHY, 0, M)
    return np.ascontiguousarray(first.stats[:, 0]), (first.status != 1).astype(np.int32), M, full


def restate(rows1, active, full, score_select, k_score, align_select, k):
    """the CPU restatement end to end: api.score_rank, the selected hypotheses' oracle alignments, api.align_rank, indices taken back through stage 1's"""
    idx, n_acc1 = api.score_rank(rows1, score_select, k_score, active)
    j, n_acc, n_suc = api.align_rank(full.status[idx], full.iterations[idx], full.stats[idx], align_select, k)
    sub = idx[j]
    return types.SimpleNamespace(scored_index=idx, scored_stats=rows1[idx], n_scored_accepted=n_acc1, index=sub.astype(np.int32), pose=full.pose[sub],
                                 information=full.H[sub], iterations=full.iterations[sub], last_stats=full.last()[sub], n_accepted=n_acc, n_success=n_suc)


def threshold_cases(rows1, active, full):
    """name -> (score_select, k_score, align_select): thresholds from the oracle's own fp32 row values.  `mid1`: the middle of the active hypotheses'
    first-iteration rows.  `mid2`: the middle of the last rows of the Success hypotheses among those `mid1` selects without a cut."""
    mid1 = ac.middle_thresholds(rows1[active > 0])
    idx_all, _ = api.score_rank(rows1, mid1, 1024, active)
    ok = full.status[idx_all] == 0
    mid2 = ac.middle_thresholds(full.last()[idx_all][ok])
    return {
        "some":    (mid1, 257, mid2),            # 0 < m < k_score; the verdict accepts some of the selected and rejects others
        "cut":     (mid1, 7, mid2),              # m = k_score < accepted
        "none":    (NOTHING, 64, EVERYTHING),    # m = 0
        "all":     (EVERYTHING, 1024, mid2),     # every active hypothesis: the duplicates are inside the selection
    }
