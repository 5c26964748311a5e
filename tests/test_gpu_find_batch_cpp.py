"""computeBatch of the C++ host mirror's finders (srrg2_laser_slam_2d_amd/host/lsm2d.hpp), built with plain g++ and run on the GPU: the batches equal the
mirror's own single compute() calls item by item (checked inside the driver) and the CPU oracle (checked here), bit for bit."""
import numpy as np
import pytest

import cpp_build
from cpp_driver import run_json, write_bins
from srrg2_laser_slam_2d_amd import synth

pytestmark = pytest.mark.gpu


def test_cpp_compute_batch(po, tmp_path):
    exe = cpp_build.build("find_batch_driver.cpp", tmp_path)
    world = synth.make_world(4)
    m = synth.make_map(world, 6000, seed=2)
    robots = synth.sample_poses(world, 6, seed=8)
    pts, offs = synth.make_scans(world, robots, n_beams=1081, noise_sigma=0.01, seed=5)
    x0 = synth.invert_poses(synth.compose_poses(robots, np.array([[0.12, -0.08, 0.04]] * 6))).astype(np.float32)
    x0[5] = np.float32([500.0, 500.0, 1.0])
    f = write_bins(tmp_path, scans=pts, offsets=offs.astype(np.int32), map=m, poses=x0)
    r = run_json(exe, [f["scans"], f["offsets"], f["map"], f["poses"], 1081, "0.4"])
    assert r["n"] == 6 and r["equal_single"] == 1 and r["equal_reversed"] == 1 and r["n_empty"] == 0
    osp = po.slice_params(canvas_cols=1081, range_max=25.0)
    onn = po.slice_params(finder=po.FINDER_NN, max_distance=0.4, normal_cos=0.7)
    counts = []
    for i in range(6):
        scan = pts[offs[i]:offs[i + 1]]
        got = np.array(r["projective"][i], np.int32).reshape(-1, 2)
        assert np.array_equal(got, po.find(osp, scan, m, x0[i])), i
        counts.append(len(got))
        inv = np.float32(r["inv"][i])      # the driver's own host-side inverse, as printed
        assert np.array_equal(np.array(r["nn"][i], np.int32).reshape(-1, 2), po.find(onn, m, scan, inv)), i
    assert counts == [404, 516, 404, 430, 466, 0]
