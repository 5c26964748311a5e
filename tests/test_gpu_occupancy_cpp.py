"""The occupancy calls of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_occupancy.hpp), built with plain g++ and run on the GPU: the counters and
the render the driver writes are the Python calls' bytes on the same inputs -- five posed inputs into two grids, updated twice."""
import json
import subprocess

import numpy as np
import pytest

import cpp_build
import occupancy_cases as oc
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(v):
    return str(int(F32(v).view(np.uint32)))


def test_cpp_occupancy(ctx, tmp_path):
    exe = cpp_build.build("occupancy_driver.cpp", tmp_path, flags=("-O2", "-pthread"))
    case = oc.all_cases()["random"]
    w, h, min_visits = oc.W, oc.H, 2
    clouds = case["clouds"]
    offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate(clouds), F32)
    pts.tofile(tmp_path / "points.bin"); offs.tofile(tmp_path / "offsets.bin")
    np.ascontiguousarray(case["poses"], F32).tofile(tmp_path / "poses.bin"); np.ascontiguousarray(case["grids"], np.int32).tofile(tmp_path / "grid.bin")
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
    args = [str(tmp_path / n) for n in ("points.bin", "offsets.bin", "poses.bin", "grid.bin")] + [str(case["n_grids"]), _bits(case["origin"][0]), _bits(case["origin"][1]),
                                                                                                  _bits(case["resolution"]), str(w), str(h), str(min_visits), str(tmp_path / "out.bin")]
    r = json.loads(subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=120).stdout)
    assert r == dict(rays=rays.tolist(), dropped=dropped.tolist())
    assert (tmp_path / "out.bin").read_bytes() == want
