"""scoreBatch of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d.hpp), built with plain g++ and run on the GPU: the batch equals the mirror's own
computeBatch -> linearizeBatch item by item, byte for byte (checked inside the driver), and the CPU oracle -- po.find, then the factor in the order of
summation asked for (checked here), bit for bit."""
import numpy as np
import pytest

import cpp_build
from cpp_driver import f32_bits, run_json, write_bins
from srrg2_laser_slam_2d_amd import synth

pytestmark = pytest.mark.gpu

TAU = 0.01


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_batch_cpp")
    exe = cpp_build.build("score_batch_driver.cpp", d)
    wl = synth.make_workload(3, 3000, seed=5, map_noise=0.004, scan_noise=0.004)
    # five items over the three scans: every scan once, one of them again under another pose, and one from so far away that it finds no pair
    which = [0, 1, 2, 1, 0]
    scans = [wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in which]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    x0 = np.ascontiguousarray(wl.x0[which], np.float32)
    x0[3] += np.float32([0.02, -0.01, 0.005]); x0[4] = np.float32([1000.0, 1000.0, 0.3])
    return exe, write_bins(d, scans=np.concatenate(scans), offsets=offs, map=wl.map_points, poses=x0), scans, wl.map_points, x0


@pytest.mark.parametrize("order", [0, 1])
def test_cpp_score_batch(po, driver, order):
    exe, f, scans, m, x0 = driver
    r = run_json(exe, [f["scans"], f["offsets"], f["map"], f["poses"], 1081, repr(TAU), order])
    assert r["n"] == 5 and r["equal_two_calls"] == 1 and r["equal_reversed"] == 1 and r["n_empty"] == 0
    osp = po.slice_params(robustifier=po.ROBUST_CAUCHY, chi_threshold=TAU)
    oracle = po.linearize if order else po.linearize_device_order
    split = False
    for i, it in enumerate(r["items"]):
        pairs = po.find(po.slice_params(), scans[i], m, x0[i])
        assert np.array_equal(np.array(it["pairs"], np.int32).reshape(-1, 2), pairs), i
        assert (len(pairs) == 0) == (i == 4)
        H, b, st = oracle(osp, scans[i], m, pairs, x0[i])
        assert np.array_equal(np.array(it["H"], np.uint32), H.ravel().view(np.uint32)), i
        assert np.array_equal(np.array(it["b"], np.uint32), b.view(np.uint32)), i
        assert it["counts"] == [st.n_corr, st.n_in, st.n_out], i
        assert it["chi"] == f32_bits([st.chi_in, st.chi_out]), i
        assert it["digest"] == [st.pair_digest_lo, st.pair_digest_hi], i
        split = split or (st.n_in > 0 and st.n_out > 0)
    assert split
