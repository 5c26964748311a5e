#!/usr/bin/env python3
"""lsm2d_voxelize (device-resident clouds voxelised and assembled in one call) against the route a caller had before it: lsm2d_cloudset_download per cloud,
the same voxelisation on the host (std::sort on (key, index), the sums in that order) and the result sent up again.  Both routes run through the bare C ABI
from one C++ program (tests/cpp/voxelize_bench.cpp with tests/cpp/voxelize_ref.cpp, built here with g++), alternating call by call; medians over --steps
timed calls after --warmup, wall clock round calls that end in their wait, kernel timing off; `device_kernel_ms` is lsm2d_last_kernel_ms of one more call with
kernel timing on.  The program is run --runs times (default 2): the host route's own movement between the runs is the yardstick's noise.

Parts:
  map100k, map1m   synth's 100 000- and 1 000 000-point maps (bench.py's world) at a resolution of ten times the maps' point spacing: roughly a tenth is left
  fleet            256 maps of 8 000 points decimated in place in a reserved-many set
  assembly         64 clouds of 16 000 points, each with a pose, into one cloud
  aligner          REPORT, no bar, a fact about this synthetic world: bench.py --full's configs[4] geometry (1000 scans against the 1M-point map, projective
                   finder, 10 iterations) against the map as it is and against its voxelisation at map1m's resolution: ms per step and the largest distance
                   of the poses to the generating poses, for both

Parity gate, inside every run and before any time is reported: every output cloud and count of the device route equals the host route's byte for byte.
Speed gate (map100k, map1m): the device route is faster than the host route by more than the host route's median moved between the runs.

    python tests/bench/voxelize_bench.py [--steps 20] [--warmup 2] [--runs 2] [--parts map100k,map1m,fleet,assembly,aligner]

Measured figures: README.md and profiles/r32/."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

import bench_common
from bench_common import HERE_ROOT, bits_arg

SEED = 1


def _tenth_resolution(synth, world, n):
    """ten times the point spacing of synth.make_map(world, n): about ten points to a voxel along a wall"""
    return float(np.float32(10.0 * float(world.lengths.sum()) / n))


def _inputs(synth, part):
    """(clouds, poses or None, mode, resolution)"""
    world = synth.make_world(SEED)
    if part in ("map100k", "map1m"):
        n = 100000 if part == "map100k" else 1000000
        return [synth.make_map(world, n, seed=SEED)], None, "into_one", _tenth_resolution(synth, world, n)
    if part == "fleet":
        return [synth.make_map(synth.make_world(100 + k), 8000, seed=k) for k in range(256)], None, "fleet", 0.05
    if part == "assembly":      # pieces of one map, each given in the frame of a local map: the poses put them back
        m = synth.make_map(world, 64 * 16000, seed=SEED, shuffle=True)
        poses = np.concatenate([synth.sample_poses(world, 64, seed=5)[:, :2], np.linspace(-3.0, 3.0, 64)[:, None]], 1)
        inv = synth.invert_poses(poses)
        clouds = []
        for k in range(64):
            p = m[16000 * k:16000 * (k + 1)].astype(np.float64)
            c, s = np.cos(inv[k, 2]), np.sin(inv[k, 2])
            xy = p[:, :2] @ np.array([[c, s], [-s, c]]) + inv[k, :2]; nn = p[:, 2:] @ np.array([[c, s], [-s, c]])
            clouds.append(np.concatenate([xy, nn], 1).astype(np.float32))
        return clouds, poses.astype(np.float32), "into_one", _tenth_resolution(synth, world, 64 * 16000)
    raise ValueError(part)


def _aligner_report(args):
    from srrg2_laser_slam_2d_amd import api, synth
    world = synth.make_world(SEED)
    wl = synth.make_workload(1000, 100000, seed=SEED, world=world)
    ctx = api.Context(0)
    scans = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets)
    full = api.CloudSet(ctx, synth.make_map(world, 1000000, seed=SEED))
    res = _tenth_resolution(synth, world, 1000000)
    small, counts, _ = api.voxelize(ctx, api.VoxelizeParams(res, 1.0), full)
    al = api.MultiAligner2D(ctx, max_iterations=10, min_num_inliers=10)
    proj = api.PointNormal2fProjectorPolar(1081, -np.pi, np.pi, 0.3, 30.0)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(api.CorrespondenceFinderProjective2f(ctx, proj, point_distance=0.5, normal_cos=0.8), min_num_correspondences=10))
    out = {}
    for name, m in (("map_1m", full), ("voxelised", small)):
        prepared = al.prepare_batch([scans], [m], wl.x0)
        for _ in range(2):
            r = prepared.run()
        t0 = time.perf_counter()
        for _ in range(3):
            r = prepared.run()
        wall = (time.perf_counter() - t0) / 3 * 1e3
        err = np.abs(r.pose - wl.x_true); err[:, 2] = np.abs((err[:, 2] + np.pi) % (2 * np.pi) - np.pi)
        out[name] = dict(points=int(m.n_points), ms_per_step=round(wall, 4), kernel_ms=round(float(r.kernel_ms), 4), n_success=int((r.status == 0).sum()),
                         max_pose_distance_m=float(err[:, :2].max()), max_pose_distance_rad=float(err[:, 2].max()))
    ctx.close()
    return dict(bench="voxelize", part="aligner", note="report, no bar: a fact about this synthetic world (noise-free map, uniform point spacing)", resolution=res,
                scans=1000, iterations=10, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parts", default="map100k,map1m,fleet,assembly,aligner")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import synth
    failed = False
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build(["voxelize_bench.cpp", "voxelize_ref.cpp"], tmp, flags=("-O2", "-ffp-contract=off"))
        for part in args.parts.split(","):
            if part == "aligner":
                line = _aligner_report(args)
            else:
                clouds, poses, mode, res = _inputs(synth, part)
                offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
                fp, fo, fq = (os.path.join(tmp, n) for n in ("points.bin", "offsets.bin", "poses.bin"))
                np.ascontiguousarray(np.concatenate(clouds), np.float32).tofile(fp); offs.tofile(fo)
                if poses is not None:
                    np.ascontiguousarray(poses, np.float32).tofile(fq)
                runs = []
                for _ in range(args.runs):
                    p = subprocess.run([exe, fp, fo, fq if poses is not None else "-", mode, bits_arg(res), bits_arg(1.0), str(args.steps), str(args.warmup)],
                                       capture_output=True, text=True)
                    assert p.returncode in (0, 3), p.stderr[-2000:]
                    r = json.loads(p.stdout)
                    assert r["outputs_equal"] == 1, "parity: the device route's outputs against the host route's"
                    runs.append(r)
                dev = [r["device_ms"][0] for r in runs]; host = [r["host_route_ms"][0] for r in runs]
                moved = max(host) - min(host)
                line = dict(bench="voxelize", part=part, mode=mode, inputs=runs[0]["inputs"], points=runs[0]["points"], voxels=runs[0]["voxels"], resolution=res,
                            steps=args.steps, runs=args.runs, device_ms=dev, host_route_ms=host, host_route_movement_ms=round(moved, 4),
                            device_ms_min_max=[r["device_ms"][1:] for r in runs], host_route_ms_min_max=[r["host_route_ms"][1:] for r in runs],
                            device_kernel_ms=[r["device_kernel_ms"] for r in runs], parity="ok")
                if part in ("map100k", "map1m"):
                    line["gate_device_faster_by_more_than_the_movement"] = bool(min(host) - max(dev) > moved)
                    failed = failed or not line["gate_device_faster_by_more_than_the_movement"]
            bench_common.emit(line, args.label)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
