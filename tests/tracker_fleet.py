"""N live trackers on distinct seeds: tests/tracker_chain.py's chain (same scenario generator, parameters and digest fields) run two ways --
per seed on the CPU oracle, and as ONE batch through api.TrackerBatch (lsm2d_clip_scene_batch -> lsm2d_align_batch -> lsm2d_merge_scene_batch,
one workgroup per tracker) -- so that every member can be held to the oracle's record for its seed, and the seed-4 member to the committed
goldens of the single tracker.  Also the same trackers stepped one after another through the single-tracker calls (tracker_chain.run_device
restated with a seed), the sequential loop a batch replaces.
"""
import math

import numpy as np

import tracker_chain as tc
from srrg2_laser_slam_2d_amd import synth


def has_scenario(seed: int, steps: int = 8, max_tries: int = 4000) -> bool:
    """tracker_chain.scenario's walk restated with a bound: False for a seed whose start pose leaves the walk no free step (there the
    generator never returns)"""
    world = synth.make_world(seed)
    st = synth.Stream(seed, salt=11)
    traj = [synth.sample_poses(world, 1, seed=seed + 3)[0]]
    for _ in range(max_tries):
        if len(traj) >= steps + 1:
            return True
        nxt = synth.compose_poses(traj[-1][None, :], st.uniform(3, -0.05, 0.05)[None, :])[0]
        if synth._free(world, nxt[None, :2], 0.8)[0]:
            traj.append(nxt)
    return len(traj) >= steps + 1


def fleet_seeds(n: int, steps: int = 8, first: int = 1):
    """the first n seeds from `first` on whose scenario exists (distinct seeds, one per tracker)"""
    out, s = [], first
    while len(out) < n:
        if has_scenario(s, steps):
            out.append(s)
        s += 1
    return out


def run_oracle(po, seed: int, steps: int = 8, record_every: int = 1):
    """tracker_chain.run_oracle with the scenario's seed as an argument (pass tracker_chain_seq._SequentialOracle(po) for "sum_order" 1)"""
    traj, ranges, odo = tc.scenario(steps, seed)
    pp = po.Preprocessor(tc.N_BEAMS, tc.A0, tc.A1, tc.RMIN, tc.RMAX, 0.3, 5, 0.02)
    opr = po.Projector(tc.COLS, -math.pi, math.pi, tc.RMIN, tc.RMAX, 0.0)
    osl = [po.slice_params(canvas_cols=tc.COLS, range_max=tc.RMAX, normal_cos=0.9, robustifier=po.ROBUST_CAUCHY, chi_threshold=0.01,
                           min_num_correspondences=5, sensor_in_robot=tuple(tc.S[0])),
           po.slice_params(canvas_cols=tc.COLS, range_max=tc.RMAX, normal_cos=0.8, min_num_correspondences=5, sensor_in_robot=tuple(tc.S[1]))]
    host_map = np.zeros((0, 4), np.float32)
    for i, s in enumerate(tc.S):
        host_map, _ = po.merge_scene(opr, host_map, po.preprocess_scan(pp, ranges[i][0]), tc._sensor_pose(traj[0], s), 0.2)
    est = traj[0].copy(); out = []
    for k in range(1, steps + 1):
        meas = [po.preprocess_scan(pp, ranges[i][k]) for i in range(2)]
        guess = synth.compose_poses(est[None, :], odo[k - 1][None, :])[0].astype(np.float32)
        clip, _ = po.clip_scene(opr, host_map, guess, tc.S[0])
        r = po.align(po.aligner_params(tc.ITS, prior_z=[0, 0, 0], prior_omega=tc.OMEGA, device_order=True), osl, meas, [clip, clip], np.zeros(3, np.float32))
        est = synth.compose_poses(guess[None, :].astype(np.float64), synth.invert_poses(np.asarray(r["pose"], np.float64)[None, :]))[0]
        for i, s in enumerate(tc.S):
            host_map, _ = po.merge_scene(opr, host_map, meas[i], tc._sensor_pose(est, s), 0.2)
        if k % record_every and k != steps:
            continue
        out.append({"step": k, "scans": [tc.digest(m) for m in meas], "scan_points": [int(len(m)) for m in meas], "clip_points": int(len(clip)), "clip": tc.digest(clip),
                    "status": int(r["status"]), "pose_hex": [float(v).hex() for v in np.asarray(r["pose"], np.float32)],
                    "information": tc.digest(np.asarray(r["H"], np.float32)), "map_points": int(len(host_map)), "map": tc.digest(host_map)})
    return out


def make_batch(api, ctx, n: int, map_capacity: int = 50000):
    """api.TrackerBatch with tracker_chain's parameters (MULTI.json)"""
    proj = api.PointNormal2fProjectorPolar(tc.COLS, -math.pi, math.pi, tc.RMIN, tc.RMAX)
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=tc.RMIN, range_max=tc.RMAX, voxelize_resolution=0.02)
    al = api.MultiAligner2D(ctx, max_iterations=tc.ITS, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(
        api.CorrespondenceFinderProjective2f(ctx, proj, 0.5, 0.9), sensor_in_robot=tc.S[0], robustifier=api.RobustifierCauchy(0.01),
        min_num_correspondences=5, fixed_slice_name="points_0", moving_slice_name="points"))
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(
        api.CorrespondenceFinderProjective2f(ctx, proj, 0.5, 0.8), sensor_in_robot=tc.S[1], min_num_correspondences=5,
        fixed_slice_name="points_1", moving_slice_name="points"))
    return api.TrackerBatch(ctx, n, proj, pre, al, tc.A0, tc.A1, 0.0, 30.0, merge_threshold=0.2, prior_omega=tc.OMEGA, map_capacity=map_capacity)


def run_fleet(api, ctx, seeds, steps: int = 8, record_every: int = 1, map_capacity: int = 50000):
    """every seed's chain as one member of ONE TrackerBatch; returns one record list per member (tracker_chain's fields).  Between recorded
    steps nothing but the aligner's poses comes back to the host."""
    scen = [tc.scenario(steps, s) for s in seeds]
    n = len(seeds)
    tb = make_batch(api, ctx, n, map_capacity)
    tb.reset(np.arange(n), [sc[1][0][0] for sc in scen], [sc[1][1][0] for sc in scen], [sc[0][0] for sc in scen])
    out = [[] for _ in range(n)]
    for k in range(1, steps + 1):
        x, status, info = tb.step([sc[1][0][k] for sc in scen], [sc[1][1][k] for sc in scen], [sc[2][k - 1] for sc in scen])
        if k % record_every and k != steps:
            continue
        for j in range(n):
            meas = [s_.download(j) for s_ in tb.scans]; clip = tb.clipped.download(j); m = tb.maps.download(j)
            out[j].append({"step": k, "status": int(status[j]), "pose_hex": [float(v).hex() for v in x[j]],
                           "information": tc.digest(info[j].astype(np.float32)),
                           "scans": [tc.digest(v) for v in meas], "scan_points": [int(len(v)) for v in meas], "clip_points": int(len(clip)),
                           "clip": tc.digest(clip), "map_points": int(len(m)), "map": tc.digest(m)})
    return out
