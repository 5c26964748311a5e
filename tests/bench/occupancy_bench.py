#!/usr/bin/env python3
"""lsm2d_occupancy_update / lsm2d_occupancy_render (scans ray-traced into hit / miss grids on the device, and the grids rendered) against the routes a caller
had before them: lsm2d_cloudset_download per cloud, the definition's loops on ONE host core (tests/cpp/occupancy_ref.cpp at -O2) and the grid kept on the
host; for the render, a download of the counters and the rule on the host.  Both routes run through the bare C ABI from one C++ program
(tests/cpp/occupancy_bench.cpp, built here with g++), alternating call by call; medians over --steps timed calls after --warmup, wall clock round calls
that end in their wait, kernel timing off.  The program is run --runs times (default 2): each route's own movement between the runs is the yardstick's
noise.  One more update with kernel timing on gives lsm2d_last_kernel_ms and the median and the longest lifetime of the tile workgroups that had work.

Parts:
  live     one 1081-beam scan into a 2048 x 2048 grid at 0.05 m (the live step)
  redraw   1000 scans of bench.py's world (configs[1]: 1081 beams, 270 degrees, the 40 m x 30 m room) into one 1024 x 768 grid (a redraw of a whole map)
  fleet    256 robots x one scan into 256 grids of 512 x 512 at 0.1 m
Every part also times the render of its grid 0.

Parity gate, inside every run: the device's counters equal the host route's byte for byte after the first call of each route and after the last, and the
render equals the host rule's bytes.  There is no speed gate: `host_route_wins` says where the host route is the faster one.

    python tests/bench/occupancy_bench.py [--steps 20] [--warmup 2] [--runs 2] [--parts live,redraw,fleet]

Measured figures: README.md, DESIGN.md section 8 and profiles/r33/."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import bench_common
from bench_common import HERE_ROOT, bits_arg

SEED = 1


def _inputs(synth, part):
    """(points, offsets, poses, grid or None, n_grids, (ox, oy, resolution, width, height))"""
    world = synth.make_world(SEED)
    if part == "live":
        poses = synth.sample_poses(world, 1, seed=SEED)
        pts, offs = synth.make_scans(world, poses, n_beams=1081)
        return pts, offs, poses, None, 1, (-51.2, -51.2, 0.05, 2048, 2048)
    if part == "redraw":
        poses = synth.sample_poses(world, 1000, seed=SEED)
        pts, offs = synth.make_scans(world, poses, n_beams=1081)
        return pts, offs, poses, None, 1, (-20.0, -15.0, 40.0 / 1024.0, 1024, 768)
    if part == "fleet":
        poses = synth.sample_poses(world, 256, seed=SEED + 1)
        pts, offs = synth.make_scans(world, poses, n_beams=1081)
        return pts, offs, poses, np.arange(256, dtype=np.int32), 256, (-25.6, -25.6, 0.1, 512, 512)
    raise ValueError(part)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parts", default="live,redraw,fleet")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build(["occupancy_bench.cpp", "occupancy_ref.cpp"], tmp, flags=("-O2", "-ffp-contract=off"))
        for part in args.parts.split(","):
            pts, offs, poses, grid, n_grids, geo = _inputs(synth, part)
            fp, fo, fq, fg = (os.path.join(tmp, n) for n in ("points.bin", "offsets.bin", "poses.bin", "grid.bin"))
            np.ascontiguousarray(pts, np.float32).tofile(fp); np.ascontiguousarray(offs, np.int32).tofile(fo); np.ascontiguousarray(poses, np.float32).tofile(fq)
            if grid is not None:
                grid.tofile(fg)
            runs = []
            for _ in range(args.runs):
                p = subprocess.run([exe, fp, fo, fq, fg if grid is not None else "-", str(n_grids), bits_arg(geo[0]), bits_arg(geo[1]), bits_arg(geo[2]), str(geo[3]), str(geo[4]),
                                    str(args.steps), str(args.warmup)], capture_output=True, text=True)
                assert p.returncode in (0, 3), p.stderr[-2000:]
                r = json.loads(p.stdout)
                assert r["outputs_equal"] == 1 and r["render_equal"] == 1, "parity: the device route's outputs against the host route's"
                runs.append(r)
            med = lambda key: [r[key][0] for r in runs]      # noqa: E731
            dev, host, ren, ren_host = med("device_ms"), med("host_route_ms"), med("render_ms"), med("render_download_route_ms")
            line = dict(bench="occupancy", part=part, inputs=runs[0]["inputs"], points=runs[0]["points"], grids=n_grids, width=geo[3], height=geo[4], resolution=geo[2],
                        rays=runs[0]["rays"], dropped=runs[0]["dropped"], steps=args.steps, runs=args.runs,
                        device_ms=dev, host_route_ms=host, device_movement_ms=round(max(dev) - min(dev), 4), host_route_movement_ms=round(max(host) - min(host), 4),
                        device_ms_min_max=[r["device_ms"][1:] for r in runs], host_route_ms_min_max=[r["host_route_ms"][1:] for r in runs],
                        device_kernel_ms=[r["device_kernel_ms"] for r in runs],
                        tile_workgroup_median_us=[r["tile_workgroup_median_us"] for r in runs], tile_workgroup_longest_us=[r["tile_workgroup_longest_us"] for r in runs],
                        render_ms=ren, render_download_route_ms=ren_host, render_movement_ms=round(max(ren) - min(ren), 4),
                        render_download_route_movement_ms=round(max(ren_host) - min(ren_host), 4),
                        host_route_wins=bool(min(host) < max(dev)), render_download_route_wins=bool(min(ren_host) < max(ren)), parity="ok")
            bench_common.emit(line, args.label)


if __name__ == "__main__":
    main()
