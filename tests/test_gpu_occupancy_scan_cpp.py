"""occupancyUpdateScans of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_occupancy.hpp), built with plain g++ and run on the GPU: the counters
and the render the driver writes are the Python call's bytes on the same inputs -- five posed scans with beams of every class into two grids, updated twice."""
import json
import subprocess

import numpy as np
import pytest

import cpp_build
import occupancy_scan_cases as sc
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(v):
    return str(int(F32(v).view(np.uint32)))


def test_cpp_occupancy_scans(ctx, tmp_path):
    exe = cpp_build.build("occupancy_scan_driver.cpp", tmp_path, flags=("-O2", "-pthread"))
    case = sc.all_cases()["random"]
    prm = case["params"]
    w, h, min_visits = sc.W, sc.H, 2
    case["ranges"].tofile(tmp_path / "ranges.bin")
    np.ascontiguousarray(case["poses"], F32).tofile(tmp_path / "poses.bin"); np.ascontiguousarray(case["grids"], np.int32).tofile(tmp_path / "grid.bin")
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
    args = [str(tmp_path / n) for n in ("ranges.bin", "poses.bin", "grid.bin")] + [
        str(case["n_grids"]), str(prm.n_beams), _bits(prm.angle_min), _bits(prm.angle_max), _bits(prm.range_min), _bits(prm.range_max), _bits(prm.trace_range),
        str(int(prm.clear_no_return)), _bits(case["origin"][0]), _bits(case["origin"][1]), _bits(case["resolution"]), str(w), str(h), str(min_visits), str(tmp_path / "out.bin")]
    r = json.loads(subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=120).stdout)
    assert r == dict(hit_rays=hit.tolist(), clear_rays=clear.tolist(), dropped=dropped.tolist())
    assert (tmp_path / "out.bin").read_bytes() == want
