"""The log-odds grid set of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_occupancy.hpp), built with plain g++ and run on the GPU: the cells and the
render the driver writes are the Python mirror's bytes on the same inputs -- five posed scans with beams of every class into two grids, updated with one set
of parameters, then with another, decayed, and one grid sent through a download and an upload."""
import numpy as np
import pytest

import cpp_build
import occupancy_logodds_cases as lc
import occupancy_scan_cases as sc
from cpp_driver import f32_bits_arg as bits_arg, run_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_cpp_occupancy_logodds(ctx, tmp_path):
    exe = cpp_build.build("occupancy_logodds_driver.cpp", tmp_path, flags=("-O2", "-pthread"))
    case = sc.all_cases()["random"]
    prm = case["params"]
    first, second = lc.PARAMS, api.LogOddsParams(60, -90, -150, 120)
    w, h, decay, unit, min_scans = sc.W, sc.H, 25, lc.UNIT, 2
    f = write_bins(tmp_path, ranges=case["ranges"], poses=np.asarray(case["poses"], F32), grid=np.asarray(case["grids"], np.int32))
    # the Python mirror, the same steps
    gs = api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], w, h), case["n_grids"], first)
    api.occupancy_update_scans(ctx, gs, prm, case["ranges"], case["poses"], case["grids"])
    gs.set_logodds(second)
    hit, clear, dropped = api.occupancy_update_scans(ctx, gs, prm, case["ranges"], case["poses"], case["grids"])
    gs.decay(decay)
    want = b""
    for g in range(case["n_grids"]):
        vv, oo = gs.download_logodds(g)
        want += vv.tobytes() + oo.tobytes() + api.occupancy_render_logodds(ctx, gs, g, unit, min_scans).tobytes()
    # ... which is the restatement's
    v, o = lc.reference(case, w, h, first)
    v, o = lc.reference(case, w, h, second, v, o)
    v = lc.decay(v, o, decay)
    ref = b"".join(v[g].tobytes() + o[g].tobytes() + api.logodds_values(v[g], o[g], unit, min_scans).tobytes() for g in range(case["n_grids"]))
    assert want == ref and hit.sum() > 500 and clear.sum() > 200 and np.abs(v).max() > 0
    gs.close()
    args = [f["ranges"], f["poses"], f["grid"], case["n_grids"], prm.n_beams, bits_arg(prm.angle_min), bits_arg(prm.angle_max), bits_arg(prm.range_min),
            bits_arg(prm.range_max), bits_arg(prm.trace_range), int(prm.clear_no_return), bits_arg(case["origin"][0]), bits_arg(case["origin"][1]),
            bits_arg(case["resolution"]), w, h]
    args += [x for p in (first, second) for x in (p.l_hit, p.l_miss, p.l_min, p.l_max)] + [decay, bits_arg(unit), min_scans, tmp_path / "out.bin"]
    r = run_json(exe, args)
    assert r == dict(hit_rays=hit.tolist(), clear_rays=clear.tolist(), dropped=dropped.tolist())
    assert (tmp_path / "out.bin").read_bytes() == want
