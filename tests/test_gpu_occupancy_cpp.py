"""The occupancy calls of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_occupancy.hpp), built with plain g++ and run on the GPU: the counters and
the render the driver writes are the Python calls' bytes on the same inputs -- five posed inputs into two grids, updated twice."""
import numpy as np
import pytest

import cpp_build
import occupancy_cases as oc
from cpp_driver import f32_bits_arg, run_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_cpp_occupancy(ctx, tmp_path):
    exe = cpp_build.build("occupancy_driver.cpp", tmp_path, flags=("-O2", "-pthread"))
    case = oc.all_cases()["random"]
    w, h, min_visits = oc.W, oc.H, 2
    clouds = case["clouds"]
    offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate(clouds), F32)
    f = write_bins(tmp_path, points=pts, offsets=offs, poses=np.asarray(case["poses"], F32), grid=np.asarray(case["grids"], np.int32))
    # the Python mirror, the same two updates
    gs = api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], w, h), case["n_grids"])
    src = api.CloudSet(ctx, pts, offs)
    api.occupancy_update(ctx, gs, src, None, case["poses"], case["grids"])
    rays, dropped = api.occupancy_update(ctx, gs, src, None, case["poses"], case["grids"])
    want = b""
    for g in range(case["n_grids"]):
        hh, mm = gs.download(g)
        want += hh.tobytes() + mm.tobytes() + api.occupancy_render(ctx, gs, g, min_visits).tobytes()
    assert rays.sum() > 1000
    gs.close()
    r = run_json(exe, [f["points"], f["offsets"], f["poses"], f["grid"], case["n_grids"], f32_bits_arg(case["origin"][0]), f32_bits_arg(case["origin"][1]),
                       f32_bits_arg(case["resolution"]), w, h, min_visits, tmp_path / "out.bin"])
    assert r == dict(rays=rays.tolist(), dropped=dropped.tolist())
    assert (tmp_path / "out.bin").read_bytes() == want
