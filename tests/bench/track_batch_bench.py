#!/usr/bin/env python3
"""N independent trackers per step through the C ABI alone: builds tests/cpp/track_batch_driver.cpp with g++ against liblsm2d_hip.so, feeds it
tests/tracker_chain.py's scenarios (raw ranges in, MULTI.json parameters; tracker j runs the (j % --scenarios)-th seed of tracker_fleet.fleet_seeds) and prints one JSON line per N:
ms per batched step and tracker-steps/s against the same trackers stepped one after another (single-tracker calls), episodes of both sides
alternated in one process, every pose and every local map checked bitwise between the two inside the run.
    python tests/bench/track_batch_bench.py [--n 1,16,64,256,1024,4096] [--episodes 3]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cpp_build      # noqa: E402


def write_inputs(d, n_scenarios, steps):
    import tracker_chain as tc
    import tracker_fleet
    scen = [tc.scenario(steps, s) for s in tracker_fleet.fleet_seeds(n_scenarios, steps)]
    ranges = np.stack([np.stack([np.stack([np.asarray(sc[1][i][k], np.float32) for i in range(2)]) for k in range(steps + 1)]) for sc in scen])
    np.ascontiguousarray(ranges, np.float32).tofile(os.path.join(d, "ranges.bin"))
    np.ascontiguousarray([np.stack(sc[2]) for sc in scen], np.float64).tofile(os.path.join(d, "odo.bin"))
    np.ascontiguousarray([sc[0][0] for sc in scen], np.float64).tofile(os.path.join(d, "start.bin"))
    return tc


def build_driver(d):
    return cpp_build.build("track_batch_driver.cpp", d)


def run(exe, d, tc, n_scenarios, steps, n, episodes, timeout=900):
    r = subprocess.run([exe, d, str(n_scenarios), str(steps), str(tc.N_BEAMS), repr(tc.A0), repr(tc.A1), str(n), str(episodes)],
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode not in (0, 3):
        raise RuntimeError("track_batch_driver failed (%d): %s" % (r.returncode, r.stderr))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,16,64,256,1024,4096")
    ap.add_argument("--scenarios", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--episodes", type=int, default=3, help="per side; the first of each side is a warm-up")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        tc = write_inputs(d, args.scenarios, args.steps)
        exe = build_driver(d)
        for n in [int(v) for v in args.n.split(",")]:
            out = run(exe, d, tc, args.scenarios, args.steps, n, args.episodes)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
