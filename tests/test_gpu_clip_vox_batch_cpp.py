"""lsm2d_host::TrackerBatch of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d.hpp) with Params::clip_voxelize_resolution = 0.1, built with plain
g++ and run on the GPU (tests/cpp/clip_vox_batch_driver.cpp): 3 trackers, 4 steps, fed from files written here.  Every pose, status, clipped
size and local-map size must be api.TrackerBatch's for the same input, bit for bit."""
import os
import sys

import numpy as np
import pytest

import tracker_chain as tc
import tracker_fleet_vox as tfv
import cpp_build
from conftest import ROOT
from cpp_driver import run_json
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu

N, STEPS, RES = 3, 4, 0.1


def test_cpp_tracker_batch_voxelised_clip(ctx, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests", "bench"))
    import track_batch_bench as tbb
    exe = cpp_build.build("clip_vox_batch_driver.cpp", tmp_path)
    tbb.write_inputs(str(tmp_path), N, STEPS)
    seeds = tfv.fleet_seeds(N, STEPS)
    r = run_json(exe, [tmp_path, N, STEPS, tc.N_BEAMS, repr(tc.A0), repr(tc.A1), N, repr(RES)])
    assert r["n_trackers"] == N and len(r["steps"]) == STEPS
    want = tfv.run_fleet(api, ctx, seeds, STEPS, RES)
    plain = tfv.run_fleet(api, ctx, seeds, 1, 0.0)
    for k in range(STEPS):
        for j in range(N):
            g, w = r["steps"][k][j], want[j][k]
            pose_hex = [float(v).hex() for v in np.array([int(h, 16) for h in g["pose"]], np.uint32).view(np.float32)]
            assert pose_hex == w["pose_hex"], (k, j)
            assert int(g["status"], 16) == w["status"] == 0 and int(g["clip_points"], 16) == w["clip_points"] and int(g["map_points"], 16) == w["map_points"], (k, j, g, w)
    assert all(want[j][0]["clip_points"] < plain[j][0]["clip_points"] for j in range(N))      # the C++ side really voxelised
