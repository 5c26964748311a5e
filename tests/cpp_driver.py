"""The Python half of the protocol the C++ drivers of tests/cpp/ speak (tests/cpp/driver_common.h is the other half): arrays go in as raw files, float
thresholds as the decimal string of their bit pattern, and one JSON line comes out with floats as bit patterns and statistics as the counts / chi / digest triple."""
import json
import os
import subprocess

import numpy as np


def f32_bits(a):
    """The bit patterns of `a` as float32, flat: what print_bits_list writes."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()


def f32_bits_arg(v):
    """One float32 as a command-line argument: what from_bits_arg reads."""
    return str(int(np.float32(v).view(np.uint32)))


def stats_json(s):
    """A row of lsm2d_iteration_stats as print_stats writes it."""
    return {"counts": [int(s["n_correspondences"]), int(s["n_inliers"]), int(s["n_outliers"])],
            "chi": f32_bits([s["chi_inliers"], s["chi_outliers"]]), "digest": [int(s["pair_digest_lo"]), int(s["pair_digest_hi"])]}


def write_bins(directory, **arrays):
    """Writes every array (in the dtype it has) to <directory>/<name>.bin; returns {name: path}."""
    paths = {}
    for name, a in arrays.items():
        paths[name] = os.path.join(str(directory), name + ".bin")
        np.ascontiguousarray(a).tofile(paths[name])
    return paths


def run_json(exe, args, timeout=120):
    """Runs a driver and returns the JSON line it printed; a driver that fails does so with its stderr in the assertion's message."""
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "%s exited with %d:\n%s" % (os.path.basename(str(exe)), r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout)
