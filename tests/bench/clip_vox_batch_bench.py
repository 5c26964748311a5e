#!/usr/bin/env python3
"""The batched clipper's voxelised form against what it replaces, through the ctypes binding: N trackers' local maps clipped at
voxelize_resolution 0.1 (721 columns) three ways, alternating call by call, medians of --reps:
  (a) batch_vox:    one asynchronous lsm2d_clip_scene_voxelized_batch (ONE launch) + lsm2d_synchronize
  (b) single_vox:   N asynchronous lsm2d_clip_scene_voxelized calls (two launches each, more above 32 768 points) + one lsm2d_synchronize
  (c) batch_plain:  one asynchronous lsm2d_clip_scene_batch (resolution 0: what voxelising costs inside the batch) + lsm2d_synchronize
for scenes of about 800 points (the tracker chain's local maps) and of 40 000 points; the scene set holds up to 16 distinct clouds that the
trackers cycle through.  Before timing, every tracker's cloud of (a) is checked bitwise against (b).  Then one api.TrackerBatch step at
--step-n trackers with clip_voxelize_resolution 0.1 against 0.  One JSON line per measurement.
    python tests/bench/clip_vox_batch_bench.py [--n 1,16,64,256,1024] [--reps 20] [--step-n 256]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

COLS, RES, DISTINCT = 721, 0.1, 16
SENSOR = np.float32([0.2, 0.1, 0.1])


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _cloud(rng, n):
    r = rng.uniform(0.5, 20.0, n); a = rng.uniform(-math.pi, math.pi, n); b = rng.uniform(-math.pi, math.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), np.cos(b), np.sin(b)], 1).astype(np.float32)


def _median_ms(ts):
    return 1e3 * float(np.median(ts))


def clip_routes(api, ctx, n, scene_points, reps):
    lib = ctx._lib
    rng = np.random.default_rng(1000 + n + scene_points)
    d = min(n, DISTINCT)
    clouds = [_cloud(rng, scene_points) for _ in range(d)]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    scenes = api.CloudSet(ctx, np.concatenate(clouds), offs if d > 1 else None)
    idx = (np.arange(n) % d).astype(np.int32)
    poses = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(-math.pi, math.pi, (n, 1))], 1).astype(np.float32)
    pr = api.PointNormal2fProjectorPolar(COLS, -math.pi, math.pi, 0.3, 20.0)
    prs = pr.struct()
    many = api.CloudSet.reserved_many(ctx, n, COLS)
    plain = api.CloudSet.reserved_many(ctx, n, COLS)
    singles = [api.CloudSet.reserved(ctx, COLS) for _ in range(n)]
    sens = _ptr(SENSOR)
    pose_ptrs = [_ptr(poses[i]) for i in range(n)]

    def batch_vox():
        assert lib.lsm2d_clip_scene_voxelized_batch(ctx.handle, C.byref(prs), scenes.handle, n, _ptr(idx), _ptr(poses), sens, RES, many.handle, None) == 0
        ctx.synchronize()

    def single_vox():
        for i in range(n):
            assert lib.lsm2d_clip_scene_voxelized(ctx.handle, C.byref(prs), scenes.handle, int(idx[i]), pose_ptrs[i], sens, RES, singles[i].handle, None, None) == 0
        ctx.synchronize()

    def batch_plain():
        assert lib.lsm2d_clip_scene_batch(ctx.handle, C.byref(prs), scenes.handle, n, _ptr(idx), _ptr(poses), sens, plain.handle, None) == 0
        ctx.synchronize()

    routes = [("batch_vox", batch_vox), ("single_vox", single_vox), ("batch_plain", batch_plain)]
    for _, f in routes:          # warm-up, and the bitwise check of (a) against (b)
        f(); f()
    many._set_pending(); plain._set_pending()
    n_vox = n_plain = 0
    for i in range(0, n, max(1, n // 64)):
        singles[i]._set_pending()
        a, b = many.download(i), singles[i].download()
        if not np.array_equal(a, b):
            raise RuntimeError("tracker %d: the batched voxelised clip differs from the single call" % i)
        n_vox += len(a); n_plain += len(plain.download(i))
    ts = {k: [] for k, _ in routes}
    for _ in range(reps):
        for k, f in routes:
            t0 = time.perf_counter(); f(); ts[k].append(time.perf_counter() - t0)
    out = {"what": "clip_routes", "n_trackers": n, "scene_points": scene_points, "cols": COLS, "resolution": RES, "reps": reps,
           "checked_points_voxelised": n_vox, "checked_points_plain": n_plain}
    for k in ts:
        out["ms_" + k] = round(_median_ms(ts[k]), 5); out["ms_" + k + "_min"] = round(1e3 * min(ts[k]), 5)
    out["single_over_batch"] = round(out["ms_single_vox"] / out["ms_batch_vox"], 3)
    out["vox_over_plain"] = round(out["ms_batch_vox"] / out["ms_batch_plain"], 3)
    for s in [scenes, many, plain] + singles:
        s.close()
    return out


def tracker_step(api, ctx, n, reps):
    import tracker_chain as tc
    import tracker_fleet
    steps, m = 8, 16
    scen = [tc.scenario(steps, s) for s in tracker_fleet.fleet_seeds(m, steps)]
    pick = [scen[j % m] for j in range(n)]
    proto = tracker_fleet.make_batch(api, ctx, 1)
    tbs = {res: api.TrackerBatch(ctx, n, proto.projector, proto.preprocessor, proto.aligner, tc.A0, tc.A1, 0.0, 30.0, merge_threshold=0.2, prior_omega=tc.OMEGA,
                                 clip_voxelize_resolution=res) for res in (RES, 0.0)}
    ts = {res: [] for res in tbs}
    episodes = 1 + (reps + steps - 1) // steps          # the first episode of each is a warm-up
    for e in range(episodes):
        for tb in tbs.values():
            tb.reset(np.arange(n), [sc[1][0][0] for sc in pick], [sc[1][1][0] for sc in pick], [sc[0][0] for sc in pick])
        ctx.synchronize()
        for k in range(1, steps + 1):
            args = ([sc[1][0][k] for sc in pick], [sc[1][1][k] for sc in pick], [sc[2][k - 1] for sc in pick])
            for res, tb in tbs.items():      # the two trackers alternate step by step
                t0 = time.perf_counter(); tb.step(*args); ctx.synchronize(); dt = time.perf_counter() - t0
                if e:
                    ts[res].append(dt)
    clip = {res: int(np.sum(tb.clipped.counts)) for res, tb in tbs.items()}
    return {"what": "tracker_batch_step", "n_trackers": n, "timed_steps": len(ts[RES]), "ms_step_res_0.1": round(_median_ms(ts[RES]), 4),
            "ms_step_res_0": round(_median_ms(ts[0.0]), 4), "ratio": round(_median_ms(ts[RES]) / _median_ms(ts[0.0]), 4),
            "clip_points_last_step_res_0.1": clip[RES], "clip_points_last_step_res_0": clip[0.0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,16,64,256,1024")
    ap.add_argument("--scene-points", default="800,40000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-n", type=int, default=256, help="trackers of the TrackerBatch step measurement (0: skip)")
    args = ap.parse_args()
    from srrg2_laser_slam_2d_amd import api
    ctx = api.Context(0, kernel_timing=False)
    try:
        for sp in [int(v) for v in args.scene_points.split(",")]:
            for n in [int(v) for v in args.n.split(",")]:
                print(json.dumps(clip_routes(api, ctx, n, sp, args.reps)), flush=True)
        if args.step_n > 0:
            print(json.dumps(tracker_step(api, ctx, args.step_n, args.reps)), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
