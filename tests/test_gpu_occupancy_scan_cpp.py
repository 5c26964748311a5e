"""occupancyUpdateScans of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_occupancy.hpp), built with plain g++ and run on the GPU: the counters
and the render the driver writes are the Python call's bytes on the same inputs -- five posed scans with beams of every class into two grids, updated twice."""
import numpy as np
import pytest

import cpp_build
import occupancy_scan_cases as sc
from cpp_driver import f32_bits_arg as bits_arg, run_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_cpp_occupancy_scans(ctx, tmp_path):
    exe = cpp_build.build("occupancy_scan_driver.cpp", tmp_path, flags=("-O2", "-pthread"))
    case = sc.all_cases()["random"]
    prm = case["params"]
    w, h, min_visits = sc.W, sc.H, 2
    f = write_bins(tmp_path, ranges=case["ranges"], poses=np.asarray(case["poses"], F32), grid=np.asarray(case["grids"], np.int32))
    # the Python mirror, the same two updates
    gs = api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], w, h), case["n_grids"])
    api.occupancy_update_scans(ctx, gs, prm, case["ranges"], case["poses"], case["grids"])
    hit, clear, dropped = api.occupancy_update_scans(ctx, gs, prm, case["ranges"], case["poses"], case["grids"])
    want = b""
    for g in range(case["n_grids"]):
        hh, mm = gs.download(g)
        want += hh.tobytes() + mm.tobytes() + api.occupancy_render(ctx, gs, g, min_visits).tobytes()
    assert hit.sum() > 500 and clear.sum() > 200
    gs.close()
    r = run_json(exe, [f["ranges"], f["poses"], f["grid"], case["n_grids"], prm.n_beams, bits_arg(prm.angle_min), bits_arg(prm.angle_max), bits_arg(prm.range_min),
                       bits_arg(prm.range_max), bits_arg(prm.trace_range), int(prm.clear_no_return), bits_arg(case["origin"][0]), bits_arg(case["origin"][1]),
                       bits_arg(case["resolution"]), w, h, min_visits, tmp_path / "out.bin"])
    assert r == dict(hit_rays=hit.tolist(), clear_rays=clear.tolist(), dropped=dropped.tolist())
    assert (tmp_path / "out.bin").read_bytes() == want
