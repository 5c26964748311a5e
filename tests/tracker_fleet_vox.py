"""tests/tracker_fleet.py's chains with a clipper that voxelises (SceneClipperProjective2D's voxelize_resolution > 0 branch,
mapping/scene_clipper_projective_2d.cpp:36-48): per seed on the CPU oracle with po.clip_scene_voxelized, and as ONE batch through
api.TrackerBatch(..., clip_voxelize_resolution=res) (lsm2d_clip_scene_voxelized_batch -> lsm2d_align_batch -> lsm2d_merge_scene_batch).
The record fields are tracker_fleet's; the oracle's records carry the plain clip's size beside them ("plain_clip_points", not a field of
the device's record) so that a test can see that every step really voxelised.
"""
import math

import numpy as np

import tracker_chain as tc
from srrg2_laser_slam_2d_amd import synth
from tracker_fleet import fleet_seeds, make_batch  # noqa: F401  (re-exported: the seeds and the batch's parameters are tracker_fleet's)


def run_oracle(po, seed: int, steps: int, res: float):
    """tracker_fleet.run_oracle with the voxelising clipper (pass tracker_chain_seq._SequentialOracle(po) for "sum_order" 1)"""
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
        clip = po.clip_scene_voxelized(opr, host_map, guess, tc.S[0], res)
        plain, _ = po.clip_scene(opr, host_map, guess, tc.S[0])
        r = po.align(po.aligner_params(tc.ITS, prior_z=[0, 0, 0], prior_omega=tc.OMEGA, device_order=True), osl, meas, [clip, clip], np.zeros(3, np.float32))
        est = synth.compose_poses(guess[None, :].astype(np.float64), synth.invert_poses(np.asarray(r["pose"], np.float64)[None, :]))[0]
        for i, s in enumerate(tc.S):
            host_map, _ = po.merge_scene(opr, host_map, meas[i], tc._sensor_pose(est, s), 0.2)
        out.append({"step": k, "scans": [tc.digest(m) for m in meas], "scan_points": [int(len(m)) for m in meas], "clip_points": int(len(clip)), "clip": tc.digest(clip),
                    "status": int(r["status"]), "pose_hex": [float(v).hex() for v in np.asarray(r["pose"], np.float32)],
                    "information": tc.digest(np.asarray(r["H"], np.float32)), "map_points": int(len(host_map)), "map": tc.digest(host_map),
                    "plain_clip_points": int(len(plain))})
    return out


def run_fleet(api, ctx, seeds, steps: int, res: float):
    """tracker_fleet.run_fleet with clip_voxelize_resolution = res: one record list per member"""
    scen = [tc.scenario(steps, s) for s in seeds]
    n = len(seeds)
    proto = make_batch(api, ctx, 1)      # tracker_fleet's parameters (MULTI.json), read off its own batch
    tb = api.TrackerBatch(ctx, n, proto.projector, proto.preprocessor, proto.aligner, tc.A0, tc.A1, 0.0, 30.0, merge_threshold=0.2, prior_omega=tc.OMEGA,
                          clip_voxelize_resolution=res)
    tb.reset(np.arange(n), [sc[1][0][0] for sc in scen], [sc[1][1][0] for sc in scen], [sc[0][0] for sc in scen])
    out = [[] for _ in range(n)]
    for k in range(1, steps + 1):
        x, status, info = tb.step([sc[1][0][k] for sc in scen], [sc[1][1][k] for sc in scen], [sc[2][k - 1] for sc in scen])
        for j in range(n):
            meas = [s_.download(j) for s_ in tb.scans]; clip = tb.clipped.download(j); m = tb.maps.download(j)
            out[j].append({"step": k, "status": int(status[j]), "pose_hex": [float(v).hex() for v in x[j]],
                           "information": tc.digest(info[j].astype(np.float32)),
                           "scans": [tc.digest(v) for v in meas], "scan_points": [int(len(v)) for v in meas], "clip_points": int(len(clip)),
                           "clip": tc.digest(clip), "map_points": int(len(m)), "map": tc.digest(m)})
    return out
