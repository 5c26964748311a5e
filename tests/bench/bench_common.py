"""What the bench scripts of this directory share: where the package and the test support lie, the synthetic workload kept between invocations, the g++ line
of their C++ program (tests/cpp_build.py), the bit pattern of a float argument (tests/cpp_driver.py) and the labelled JSON line they print.  The scripts run as
scripts, so `import bench_common` finds this file beside them."""
import json
import os
import sys

import numpy as np

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (os.path.join(HERE_ROOT, "tests"), HERE_ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from cpp_driver import f32_bits_arg as bits_arg      # noqa: E402,F401


def workload(synth, workdir, n, n_map):
    """(scan_points, scan_offsets, map_points, x0) of synth.make_workload(n, n_map, seed=1), kept as an npz under `workdir` if one is given."""
    path = os.path.join(workdir, "pairs_bench_%d_%d.npz" % (n, n_map)) if workdir else None
    if path and os.path.exists(path):
        z = np.load(path)
        return z["scan_points"], z["scan_offsets"], z["map_points"], z["x0"]
    wl = synth.make_workload(n, n_map, seed=1)
    if path:
        os.makedirs(workdir, exist_ok=True)
        np.savez(path, scan_points=wl.scan_points, scan_offsets=wl.scan_offsets, map_points=wl.map_points, x0=wl.x0)
    return wl.scan_points, wl.scan_offsets, wl.map_points, wl.x0


def build(source, out_dir, **kw):
    """cpp_build.build of a program (or list of sources) of tests/cpp/ into out_dir."""
    import cpp_build
    return cpp_build.build(source, out_dir, **kw)


def emit(line, label=None):
    """One result line on stdout, with the caller's --label if it gave one."""
    if label:
        line["label"] = label
    print(json.dumps(line), flush=True)
