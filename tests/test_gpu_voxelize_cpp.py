"""voxelize of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_voxelize.hpp), built with plain g++ and run on the GPU: what the driver prints is
api.voxelize's answer on the same inputs, bit for bit -- seven inputs in three groups followed by a pass in place, and five clouds assembled with poses."""
import numpy as np
import pytest

import cpp_build
import voxelize_cases as vc
from cpp_driver import f32_bits as _cloud_bits, f32_bits_arg as bits_arg, run_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("voxelize_cpp")
    return cpp_build.build("voxelize_driver.cpp", d, flags=("-O2", "-pthread")), d


@pytest.mark.parametrize("name,res2", [("inputs7_groups3", 2.0), ("assembly", 0.0)])
def test_cpp_voxelize(ctx, driver, name, res2):
    exe, d = driver
    case = vc.all_cases()[name]
    clouds, n_groups, (res, nres) = case["clouds"], case["n_groups"], case["params"]
    offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate(clouds), F32)
    capacity = len(pts)
    optional = {key: np.asarray(case[key], t) for key, t in (("poses", F32), ("groups", np.int32)) if case[key] is not None}
    f = write_bins(d, points=pts, offsets=offs, **optional)
    # the Python mirror, the same two passes
    dst = api.CloudSet.reserved_many(ctx, n_groups, capacity)
    _, counts, dropped = api.voxelize(ctx, api.VoxelizeParams(res, nres), api.CloudSet(ctx, pts, offs), None, case["poses"], case["groups"], n_groups, dst)
    first = dict(fits=1, counts=counts.tolist(), dropped=dropped.tolist(), clouds=[_cloud_bits(dst.download(g)) for g in range(n_groups)])
    assert sum(first["counts"]) > 1000
    second = None
    if res2:
        _, c2, d2 = api.voxelize(ctx, api.VoxelizeParams(res2, nres), dst, None, None, np.arange(n_groups), n_groups, dst)
        second = dict(fits=1, counts=c2.tolist(), dropped=d2.tolist(), clouds=[_cloud_bits(dst.download(g)) for g in range(n_groups)])
        assert 0 < sum(second["counts"]) < sum(first["counts"])
    r = run_json(exe, [f["points"], f["offsets"], f.get("poses", "-"), f.get("groups", "-"), n_groups, capacity, bits_arg(res), bits_arg(nres), bits_arg(res2) if res2 else "0"])
    assert r["first"] == first
    assert r.get("in_place") == second
