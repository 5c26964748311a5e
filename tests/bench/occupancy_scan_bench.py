#!/usr/bin/env python3
"""lsm2d_occupancy_update_scans (raw range scans ray-traced into hit / miss grids on the device, the beams without a return cleared) against the routes a
caller had before it: the definition's loops on ONE host core (tests/cpp/occupancy_scan_ref.cpp at -O2) with the grid kept on the host, and -- where no
beam is without a return -- the two-call device route of 0.7.12, lsm2d_preprocess_scans_refill then lsm2d_occupancy_update.  All routes run through the bare
C ABI from one C++ program (tests/cpp/occupancy_scan_bench.cpp, built here with g++), alternating call by call; medians over --steps timed calls after
--warmup, wall clock round calls that end in their wait, kernel timing off.  The program is run --runs times (default 2): each route's own movement between
the runs is the yardstick's noise.  One more call with kernel timing on gives lsm2d_last_kernel_ms and the median and the longest lifetime of the tile
workgroups that had work.

Parts (the three of tests/bench/occupancy_bench.py, made from ranges: bench.py's world, the 40 m x 30 m room, 1081 beams over 270 degrees):
  live     one scan into a 2048 x 2048 grid at 0.05 m (the live step)
  redraw   1000 scans into one 1024 x 768 grid (a redraw of a whole map)
  fleet    256 robots x one scan into 256 grids of 512 x 512 at 0.1 m
Variants of every part:
  none       range_max = trace_range = 60 m, beyond the room's diagonal: every beam has a return and is a HIT ray
  no_return  range_max = 12 m, trace_range = 10 m, below the diagonal: the share of beams beyond range_max (reported as no_return_share) has no return and
             clears out to 10 m, as do the returns between 10 and 12 m

Parity gate, inside every run: the device's counters and counts equal the host route's byte for byte after the first call of each route and after the
last.  There is no speed gate: `new_call_above_two_call` says whether the new call's median lies above the two-call route's by more than that route's own
movement between its runs.

    python tests/bench/occupancy_scan_bench.py [--steps 20] [--warmup 2] [--runs 2] [--parts live,redraw,fleet] [--variants none,no_return]

Measured figures: README.md, DESIGN.md section 8 and profiles/r36/."""
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
N_BEAMS, ANGLE_MIN, ANGLE_MAX, RANGE_MIN = 1081, -0.75 * np.pi, 0.75 * np.pi, 0.1
VARIANTS = {"none": (60.0, 60.0), "no_return": (12.0, 10.0)}      # (range_max, trace_range)


def _inputs(synth, part):
    """(ranges, poses, grid or None, n_grids, (ox, oy, resolution, width, height))"""
    world = synth.make_world(SEED)
    n, seed, grid, n_grids, geo = {"live": (1, SEED, None, 1, (-51.2, -51.2, 0.05, 2048, 2048)),
                                   "redraw": (1000, SEED, None, 1, (-20.0, -15.0, 40.0 / 1024.0, 1024, 768)),
                                   "fleet": (256, SEED + 1, np.arange(256, dtype=np.int32), 256, (-25.6, -25.6, 0.1, 512, 512))}[part]
    poses = synth.sample_poses(world, n, seed=seed)
    ranges = synth.make_scan_ranges(world, poses, n_beams=N_BEAMS, angle_min=ANGLE_MIN, angle_max=ANGLE_MAX)
    return ranges, poses, grid, n_grids, geo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parts", default="live,redraw,fleet")
    ap.add_argument("--variants", default="none,no_return")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build(["occupancy_scan_bench.cpp", "occupancy_scan_ref.cpp"], tmp, flags=("-O2", "-ffp-contract=off"))
        for part in args.parts.split(","):
            ranges, poses, grid, n_grids, geo = _inputs(synth, part)
            fr, fq, fg = (os.path.join(tmp, n) for n in ("ranges.bin", "poses.bin", "grid.bin"))
            np.ascontiguousarray(ranges, np.float32).tofile(fr); np.ascontiguousarray(poses, np.float32).tofile(fq)
            if grid is not None:
                grid.tofile(fg)
            for variant in args.variants.split(","):
                range_max, trace = VARIANTS[variant]
                share = float(np.mean(~(ranges <= np.float32(range_max))))
                two_call = variant == "none"
                assert not two_call or share == 0.0, "the two-call route cannot clear: it is timed where no beam is without a return"
                runs = []
                for _ in range(args.runs):
                    p = subprocess.run([exe, fr, fq, fg if grid is not None else "-", str(n_grids), str(N_BEAMS), bits_arg(ANGLE_MIN), bits_arg(ANGLE_MAX), bits_arg(RANGE_MIN),
                                        bits_arg(range_max), bits_arg(trace), "1", bits_arg(geo[0]), bits_arg(geo[1]), bits_arg(geo[2]), str(geo[3]), str(geo[4]), str(args.steps),
                                        str(args.warmup), "1" if two_call else "0"], capture_output=True, text=True)
                    assert p.returncode in (0, 3), p.stderr[-2000:]
                    r = json.loads(p.stdout)
                    assert r["outputs_equal"] == 1, "parity: the device's counters and counts against the host route's"
                    runs.append(r)
                med = lambda key: [r[key][0] for r in runs]      # noqa: E731
                new, host, two = med("new_call_ms"), med("host_route_ms"), med("two_call_ms")
                line = dict(bench="occupancy_scan", part=part, variant=variant, scans=runs[0]["scans"], beams=runs[0]["beams"], grids=n_grids, width=geo[3], height=geo[4],
                            resolution=geo[2], range_max=range_max, trace_range=trace, no_return_share=round(share, 4), hit_rays=runs[0]["hit_rays"],
                            clear_rays=runs[0]["clear_rays"], dropped=runs[0]["dropped"], steps=args.steps, runs=args.runs,
                            new_call_ms=new, host_route_ms=host, new_call_movement_ms=round(max(new) - min(new), 4), host_route_movement_ms=round(max(host) - min(host), 4),
                            new_call_ms_min_max=[r["new_call_ms"][1:] for r in runs], host_route_ms_min_max=[r["host_route_ms"][1:] for r in runs],
                            new_call_kernel_ms=[r["new_call_kernel_ms"] for r in runs],
                            tile_workgroup_median_us=[r["tile_workgroup_median_us"] for r in runs], tile_workgroup_longest_us=[r["tile_workgroup_longest_us"] for r in runs],
                            host_route_wins=bool(min(host) < max(new)), parity="ok")
                if two_call:
                    line.update(two_call_ms=two, two_call_movement_ms=round(max(two) - min(two), 4), two_call_ms_min_max=[r["two_call_ms"][1:] for r in runs],
                                two_call_rays=runs[0]["two_call_rays"], two_call_update_kernel_ms=[r["two_call_update_kernel_ms"] for r in runs],
                                two_call_tile_workgroup_median_us=[r["two_call_tile_workgroup_median_us"] for r in runs],
                                two_call_tile_workgroup_longest_us=[r["two_call_tile_workgroup_longest_us"] for r in runs],
                                new_call_above_two_call=bool(float(np.median(new)) - float(np.median(two)) > max(two) - min(two)))
                bench_common.emit(line, args.label)


if __name__ == "__main__":
    main()
