"""lsm2d_voxelize (ABI 0.7.11): the definition restated on the host, and the cases the GPU tests run.

`reference(...)` is items 1-5 of PARITY.md section 3, item 17b, in fp32 with libm's fmaf where the definition has a fused multiply-add: a small C++ file
(tests/cpp/voxelize_ref.cpp) built once per process through tests/cpp_build.py.  tests/test_voxelize_abi.py pins it to the CPU oracle bit for bit and checks
that the cases below contain what they claim; tests/test_gpu_voxelize.py compares the device with it bit for bit.

A case is a dict: clouds (list of float32 [n, 4]), poses ([n_inputs, 3] or None), groups ([n_inputs] or None), n_groups, params (resolution,
normal_resolution).  Keys are made directly: with resolution 0.5 (inverse 2, exact) a point at x = 0.5 (k + u), 0 < u < 1, has the x floor k."""
import ctypes as C
import os
import tempfile

import numpy as np

import cpp_build
from srrg2_laser_slam_2d_amd import _capi

F32 = np.float32
TILE = _capi.VOXELIZE_TILE      # keys per sort tile of the device side (the GPU test checks it against the library's "voxelize_tile")
SCAN_TILES = _capi.VOXELIZE_SCAN_TILES      # tiles whose counters one pass of the device side's scan takes ("voxelize_scan_tiles")
RES = 0.5

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="voxref_")
        so = cpp_build.build("voxelize_ref.cpp", _dir.name, flags=("-O2", "-fPIC", "-shared", "-ffp-contract=off"), link=False)
        _lib = C.CDLL(so)
        _lib.voxref_voxelize.restype = C.c_int
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def transform(points, pose) -> np.ndarray:
    """item 1 alone: the points moved by one pose"""
    pts = np.ascontiguousarray(points, F32).reshape(-1, 4); out = np.empty_like(pts)
    lib().voxref_transform(_p(pts), len(pts), _p(np.ascontiguousarray(pose, F32)), _p(out))
    return out


def keys(points, resolution, normal_resolution) -> np.ndarray:
    """item 2 alone: int64 [n], the 42-bit key of every point as it is, -1 where it has none"""
    pts = np.ascontiguousarray(points, F32).reshape(-1, 4); out = np.empty(len(pts), np.int64)
    lib().voxref_keys(_p(pts), len(pts), C.c_float(resolution), C.c_float(normal_resolution), _p(out))
    return out


def reference(clouds, poses=None, groups=None, n_groups=1, params=(RES, 1.0)):
    """-> (list of float32 [count_g, 4] per group, counts int32 [n_groups], dropped int32 [n_groups])"""
    clouds = [np.ascontiguousarray(c, F32).reshape(-1, 4) for c in clouds]
    offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate(clouds) if clouds else np.zeros((0, 4), F32), F32)
    ps = None if poses is None else np.ascontiguousarray(poses, F32).reshape(len(clouds), 3)
    gr = None if groups is None else np.ascontiguousarray(groups, np.int32).reshape(len(clouds))
    out = np.empty((max(len(pts), 1), 4), F32); counts = np.zeros(n_groups, np.int32); dropped = np.zeros(n_groups, np.int32)
    n = lib().voxref_voxelize(_p(pts), _p(offs), len(clouds), _p(ps), _p(gr), int(n_groups), C.c_float(params[0]), C.c_float(params[1]), _p(out), _p(counts), _p(dropped))
    assert n == int(counts.sum())
    cuts = np.concatenate([[0], np.cumsum(counts)])
    return [out[cuts[g]:cuts[g + 1]].copy() for g in range(n_groups)], counts, dropped


def case_reference(case):
    return reference(case["clouds"], case["poses"], case["groups"], case["n_groups"], case["params"])


# ---- points with chosen keys ----------------------------------------------------------------------------------------------------------------------------
def points_at(kx, ky, knx, kny, rng, nres=1.0):
    """float32 [n, 4] whose floors at (RES, nres) are the given integers: a random place inside the cell"""
    kx, ky, knx, kny = (np.asarray(v, np.float64) for v in np.broadcast_arrays(kx, ky, knx, kny))
    u = rng.uniform(0.25, 0.75, (4, len(kx)))
    return np.stack([(kx + u[0]) * RES, (ky + u[1]) * RES, (knx + u[2]) * nres, (kny + u[3]) * nres], 1).astype(F32)


def random_cloud(n, rng, nres=1.0, n_bad=0):
    """n points over a small grid of cells (equal keys abound), n_bad of them without a key"""
    pts = points_at(rng.integers(-20, 20, n), rng.integers(-3, 3, n), rng.integers(-1, 1, n), rng.integers(-1, 1, n), rng, nres)
    if min(n_bad, n):
        bad = rng.choice(n, min(n_bad, n), replace=False)
        pts[bad, 0] = F32(1.0e6)
    return pts


def _case(clouds, poses=None, groups=None, n_groups=1, params=(RES, 1.0)):
    return dict(clouds=[np.ascontiguousarray(c, F32) for c in clouds], poses=None if poses is None else np.asarray(poses, F32),
                groups=None if groups is None else np.asarray(groups, np.int32), n_groups=n_groups, params=params)


def size_cases():
    """one input, one group, n in {0, 1, 2, T-1, T, T+1, 2T+1, 3T+5}"""
    rng = np.random.default_rng(11)
    return {"n%d" % n: _case([random_cloud(n, rng, n_bad=min(n // 50, 7))]) for n in (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 5)}


def distinct(n, rng):
    """n points with n different keys, in ascending key order"""
    k = np.arange(n)
    return points_at(k // 64 - 30, k % 64 - 32, 0, 0, rng)


def edge_points():
    """keys at the ends of every range, a point one ulp outside each bound, NaN and Inf in every component: (points, has_key)"""
    up, down = F32(np.inf), F32(-np.inf)
    mid = [F32(0.3), F32(0.3), F32(0.5), F32(0.5)]
    lo_in = [F32(-16384.0), F32(-16384.0), F32(-16.0), F32(-16.0)]                     # floors -32768, -32768, -16, -16
    hi_in = [np.nextafter(F32(16384.0), down), np.nextafter(F32(16384.0), down), np.nextafter(F32(16.0), down), np.nextafter(F32(16.0), down)]      # 32767, 32767, 15, 15
    lo_out = [np.nextafter(v, down) for v in lo_in]
    hi_out = [F32(16384.0), F32(16384.0), F32(16.0), F32(16.0)]
    rows, ok = [], []
    for c in range(4):
        for vals, good in ((lo_in, True), (hi_in, True), (lo_out, False), (hi_out, False)):
            p = list(mid); p[c] = vals[c]; rows.append(p); ok.append(good)
        for v in (F32(np.nan), up, down):
            p = list(mid); p[c] = v; rows.append(p); ok.append(False)
    rows.append(lo_in); ok.append(True); rows.append(hi_in); ok.append(True)
    return np.array(rows, F32), np.array(ok)


def structure_cases():
    """what the sort and the heads pass can get wrong, by construction (test_voxelize_abi.py checks each claim)"""
    rng = np.random.default_rng(12)
    T = TILE
    out = {}
    # a run of 10 equal keys in sorted positions T-3 .. T+7: T-3 smaller keys in front, T-6 larger behind; shuffled
    small, large = distinct(3 * T, rng)[:T - 3], distinct(3 * T, rng)[T + 10:2 * T + 4]
    run = points_at(np.full(10, -30 + (T - 3) // 64), np.full(10, (T - 3) % 64 - 32), 0, 1, rng)      # the last small key's cell, a larger normal floor
    pts = np.concatenate([small, run, large]); out["straddle"] = _case([pts[rng.permutation(len(pts))]])
    # a run longer than a tile among others
    run = points_at(np.full(T + 50, 3), np.full(T + 50, 3), 0, 0, rng)
    pts = np.concatenate([random_cloud(2 * T - 45, rng), run]); out["long_run"] = _case([pts[rng.permutation(len(pts))]])
    # a batch that is one voxel
    out["one_voxel"] = _case([points_at(np.full(2 * T + 1, -7), np.full(2 * T + 1, 5), -1, 0, rng)])
    # all-distinct keys, sorted and reverse-sorted
    d = distinct(3 * T + 5, rng)
    out["distinct_sorted"] = _case([d]); out["distinct_reversed"] = _case([d[::-1]])
    # the ends of the key's ranges, one ulp outside, NaN and Inf -- among ordinary points
    e, _ = edge_points()
    out["edges"] = _case([np.concatenate([random_cloud(100, rng), e, random_cloud(100, rng)])])
    return out


def group_cases():
    """1, 3 and 7 inputs; 1 and 3 groups with sizes that cross tiles; the same key in two groups; an empty group; a group dropped entirely"""
    rng = np.random.default_rng(13)
    T = TILE
    out = {}
    out["inputs3_group1"] = _case([random_cloud(n, rng) for n in (700, 0, T + 9)])
    out["inputs7_groups3"] = _case([random_cloud(n, rng, n_bad=2) for n in (T + 30, 5, 0, 900, T, 17, 333)], groups=[0, 2, 1, 2, 0, 1, 2], n_groups=3)
    # group 1 has no input with points; group 2's points all lack a key; groups 0 and 3 share every key
    same = random_cloud(500, rng)
    bad = random_cloud(40, rng); bad[:, 1] = F32(np.nan)
    out["empty_and_dropped"] = _case([same, np.zeros((0, 4), F32), bad, same[::-1].copy()], groups=[0, 1, 2, 3], n_groups=4)
    # the clipper's coefficients, unit normals
    a = rng.uniform(-np.pi, np.pi, 2 * T + 1); r = rng.uniform(1.0, 6.0, len(a))
    pts = np.stack([r * np.cos(a), r * np.sin(a), -np.cos(a + 0.1), -np.sin(a + 0.1)], 1).astype(F32)
    out["clipper_coefficients"] = _case([pts], params=(0.25, 0.1))
    out["preprocessor_coefficients"] = _case([pts], params=(0.25, 1.0))
    return out


def assembly_case():
    """5 clouds with poses (every sign of x, y and theta) into one cloud"""
    rng = np.random.default_rng(14)
    clouds = []
    for n in (900, TILE + 3, 650, 1200, 777):
        a = rng.uniform(-np.pi, np.pi, n); r = rng.uniform(1.0, 8.0, n)
        clouds.append(np.stack([r * np.cos(a), r * np.sin(a), -np.cos(a), -np.sin(a)], 1).astype(F32))
    poses = np.array([[0.5, -1.0, 0.3], [-2.0, 0.25, -1.2], [1.5, 2.0, 2.9], [-0.75, -0.5, -3.0], [0.0, 0.0, 0.0]], F32)
    return _case(clouds, poses=poses, params=(0.1, 1.0))


def scan_boundary_case():
    """just past the tiles one pass of the scan takes: all-distinct small integers as keys (the reference stays cheap), in a shuffled order"""
    rng = np.random.default_rng(15)
    n = SCAN_TILES * TILE + 5
    return _case([distinct(n, rng)[rng.permutation(n)]])


def all_cases():
    out = {"scan_boundary": scan_boundary_case()}
    for part in (size_cases(), structure_cases(), group_cases()):
        out.update(part)
    out["assembly"] = assembly_case()
    return out
