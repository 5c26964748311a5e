"""lsm2d_occupancy_update_scans (ABI 0.7.13): the definition restated on the host, and the cases the GPU tests run.

`reference(...)` is PARITY.md section 3, item 17d, as plain loops: a small C++ file (tests/cpp/occupancy_scan_ref.cpp) built once per process through
tests/cpp_build.py, written independently of the kernels (its walk is the incremental error-term one).  tests/test_occupancy_scan_abi.py pins it to what is
pinned already -- occupancy_cases.reference over clouds made of its end points, and the oracle's preprocessor for the end points themselves -- and checks
that the cases below contain what they claim; tests/test_gpu_occupancy_scan.py compares the device with it bit for bit.

A case is a dict: params (api.OccupancyScanParams), ranges (float32 [n_scans, n_beams]), poses ([n_scans, 3] or None), grids ([n_scans] or None), n_grids,
origin (ox, oy), resolution.  The grid's SIZE is not part of a case.  Rays with chosen cells use a sensor of FOUR beams over a full turn, whose beam 2 has
the bearing 0 and the direction (1, 0) exactly: with resolution 0.5 and a sensor in the middle of cell (x0, y0) at heading 0, a ray of length 0.5 k along
beam 2 ends in the middle of cell (x0 + k, y0), every operation exact in fp32; at heading pi / 2 it ends in cell (x0, y0 + k) (the sine and cosine of
item 11b are within 1e-7 there: the end stays in the middle of its cell)."""
import ctypes as C
import math
import tempfile

import numpy as np

import cpp_build
import occupancy_cases as oc
from srrg2_laser_slam_2d_amd import api

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
W, H = oc.W, oc.H
SIZES = oc.SIZES
RES = oc.RES
CAP = oc.CAP
MAX_RAY = oc.MAX_RAY
DROPPED, HIT, CLEAR = -1, 0, 1
WHOLE_SCAN = 1000.0      # a normal_point_distance no two points of a scan exceed: the preprocessor then keeps every valid beam (each window is the whole scan)

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="occsref_")
        so = cpp_build.build("occupancy_scan_ref.cpp", _dir.name, flags=("-O2", "-fPIC", "-shared", "-ffp-contract=off"), link=False)
        _lib = C.CDLL(so)
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def points(params, scan):
    """ONE scan: (class 1 .. 4 [n_beams], kind -1 / 0 / 1 by the class alone [n_beams], sensor-frame end points float32 [n_beams, 2])"""
    r = np.ascontiguousarray(scan, F32).reshape(int(params.n_beams)); p = params.struct()
    cls = np.zeros(len(r), np.int32); kind = np.zeros(len(r), np.int32); xy = np.zeros((len(r), 2), F32)
    lib().occsref_points(C.byref(p), _p(r), _p(cls), _p(kind), _p(xy))
    return cls, kind, xy


def rays_of(params, scan, pose, origin, resolution):
    """ONE scan: (int32 [n_beams, 4] = x0, y0, x1, y1; kind [n_beams] = -1 no ray (by its class or by the cell tests) / 0 HIT / 1 CLEAR)"""
    r = np.ascontiguousarray(scan, F32).reshape(int(params.n_beams)); p = params.struct()
    rays = np.zeros((len(r), 4), np.int32); kind = np.zeros(len(r), np.int32)
    ps = None if pose is None else np.ascontiguousarray(pose, F32)
    lib().occsref_rays(C.byref(p), _p(r), _p(ps), C.c_float(origin[0]), C.c_float(origin[1]), C.c_float(resolution), _p(rays), _p(kind))
    return rays, kind


def case_rays(case):
    """every beam of a case: (rays int32 [n_scans, n_beams, 4], kind [n_scans, n_beams], class [n_scans, n_beams])"""
    rr, kk, cc = [], [], []
    for k, scan in enumerate(case["ranges"]):
        r, kd = rays_of(case["params"], scan, None if case["poses"] is None else case["poses"][k], case["origin"], case["resolution"])
        rr.append(r); kk.append(kd); cc.append(points(case["params"], scan)[0])
    return np.stack(rr), np.stack(kk), np.stack(cc)


def reference(case, width, height, hits=None, misses=None):
    """-> (hits, misses uint32 [n_grids, height, width], hit_rays, clear_rays, dropped int32 [n_grids]); hits / misses given: accumulated into copies"""
    r = np.ascontiguousarray(case["ranges"], F32); n_scans = len(r); p = case["params"].struct()
    assert r.shape == (n_scans, int(case["params"].n_beams))
    ps = None if case["poses"] is None else np.ascontiguousarray(case["poses"], F32).reshape(n_scans, 3)
    gr = None if case["grids"] is None else np.ascontiguousarray(case["grids"], np.int32).reshape(n_scans)
    ng = int(case["n_grids"])
    h = np.zeros((ng, height, width), np.uint32) if hits is None else np.ascontiguousarray(hits, np.uint32).copy().reshape(ng, height, width)
    m = np.zeros((ng, height, width), np.uint32) if misses is None else np.ascontiguousarray(misses, np.uint32).copy().reshape(ng, height, width)
    nh = np.zeros(ng, np.int32); nc = np.zeros(ng, np.int32); nd = np.zeros(ng, np.int32)
    lib().occsref_update(C.byref(p), _p(r), n_scans, _p(ps), _p(gr), ng, C.c_float(case["origin"][0]), C.c_float(case["origin"][1]),
                         C.c_float(case["resolution"]), int(width), int(height), _p(h), _p(m), _p(nh), _p(nc), _p(nd))
    return h, m, nh, nc, nd


def _case(params, ranges, poses=None, grids=None, n_grids=1, origin=(0.0, 0.0), resolution=RES):
    r = np.ascontiguousarray(ranges, F32).reshape(-1, int(params.n_beams))
    return dict(params=params, ranges=r, poses=None if poses is None else np.asarray(poses, F32).reshape(len(r), 3),
                grids=None if grids is None else np.asarray(grids, np.int32).reshape(len(r)), n_grids=n_grids, origin=(float(origin[0]), float(origin[1])),
                resolution=float(resolution))


# ---- the classes at their thresholds -------------------------------------------------------------------------------------------------------------------------
RMIN, TRACE, RMAX = F32(0.75), F32(4.5), F32(7.25)


def threshold_ranges(rmin=RMIN, trace=TRACE, rmax=RMAX):
    """(ranges, the class each must get): every threshold and one ulp either side of it, the non-finite values, zero and a negative range"""
    up, down = F32(np.inf), F32(-np.inf)
    rows = [(rmin, 2), (np.nextafter(rmin, down), 1), (np.nextafter(rmin, up), 2),
            (trace, 2), (np.nextafter(trace, up), 3), (np.nextafter(trace, down), 2),
            (rmax, 3), (np.nextafter(rmax, up), 4), (np.nextafter(rmax, down), 3),
            (INF, 4), (-INF, 1), (NAN, 1), (F32(0.0), 1), (F32(-1.0), 1), (F32(2.0), 2), (F32(6.0), 3), (F32(100.0), 4)]
    return np.array([r for r, _ in rows], F32), np.array([c for _, c in rows], np.int32)


def classes_case(clear_no_return=True):
    """two scans of the threshold ranges (forward and reversed over the beams) from rotated poses, over 17 beams of a 270 degree sensor"""
    r, _ = threshold_ranges()
    prm = api.OccupancyScanParams(len(r), -2.35, 2.35, float(RMIN), float(RMAX), float(TRACE), clear_no_return)
    return _case(prm, [r, r[::-1]], poses=[[20.3, 15.2, 0.4], [41.7, 22.9, -2.0]], origin=(-0.35, 0.15), resolution=0.5)


def trace_is_max_case():
    """trace_range == range_max: class 3 is empty, a return is a HIT ray up to the gate"""
    r, _ = threshold_ranges(RMIN, RMAX, RMAX)
    prm = api.OccupancyScanParams(len(r), -2.35, 2.35, float(RMIN), float(RMAX), float(RMAX), True)
    return _case(prm, [r], poses=[[30.0, 17.0, 1.0]])


# ---- rays with chosen cells: four beams over a full turn, beam 2 along the heading -----------------------------------------------------------------------------
def four_beams(range_min, range_max, trace_range, clear_no_return=True):
    return api.OccupancyScanParams(4, -math.pi, math.pi, range_min, range_max, trace_range, clear_no_return)


def _sensor(x0, y0, heading=0.0, origin=(0.0, 0.0), frac=0.5, res=RES):
    return [origin[0] + res * (x0 + frac), origin[1] + res * (y0 + frac), heading]


UP = math.pi / 2
TRACE_CELLS = 80      # the chosen-cell cases trace 40 m = 80 cells of 0.5 m


def geometry_scans():
    """(pose, ranges of the four beams, what the scan is for).  Beam 2 points along the heading."""
    n, far = NAN, INF
    return [(_sensor(-17, 10), [n, n, far, n], "clear ray ends on 63 of the 63 | 64 tile edge in x"),
            (_sensor(-16, 12), [n, n, far, n], "clear ray ends on 64 of the tile edge in x"),
            (_sensor(5, -17, UP), [n, n, far, n], "clear ray ends on 63 of the tile edge in y"),
            (_sensor(6, -16, UP), [n, n, far, n], "clear ray ends on 64 of the tile edge in y"),
            (_sensor(20, -5, UP), [n, n, far, n], "clear ray crosses the grid, both ends outside"),
            (_sensor(100, 30), [n, n, far, n], "clear ray starts inside and ends outside"),
            (_sensor(33, 10), [n, n, 15.0, n], "hit ray of another scan ends in (63, 10), where the first scan's clear ray ends"),
            (_sensor(-100, -100), [n, n, 50.0, n], "a return beyond the cut, wholly outside the grid"),
            (_sensor(40, 40), [3.0, 2.0, 1.0, 4.0], "four short hit rays")]


def geometry_case():
    scans = geometry_scans()
    return _case(four_beams(0.25, 60.0, RES * TRACE_CELLS), [s[1] for s in scans], poses=[s[0] for s in scans])


def clear_only_case():
    """scans of CLEAR rays only (no return, and returns beyond the cut): the boxes come from clear rays, hits stay 0 everywhere"""
    rng = np.random.default_rng(12)
    prm = api.OccupancyScanParams(65, -2.0, 2.0, 0.5, 30.0, 6.0, True)
    r = np.where(rng.random((3, 65)) < 0.5, INF, rng.uniform(6.5, 29.0, (3, 65))).astype(F32)
    return _case(prm, r, poses=[[12.0, 9.0, 0.3], [33.0, 20.0, 2.5], [50.0, 8.0, -1.2]], grids=[0, 1, 0], n_grids=2, origin=(-0.5, -0.25), resolution=0.5)


def dropped_scan_case():
    """three scans: ordinary, wholly dropped (NaN, too close, and no return at clear_no_return 0), ordinary; the dropped one alone feeds grid 1"""
    rng = np.random.default_rng(13)
    prm = api.OccupancyScanParams(40, -2.0, 2.0, 0.5, 12.0, 8.0, False)
    a = rng.uniform(0.6, 11.0, 40).astype(F32)
    bad = np.array(([NAN, 0.1, INF, -INF, 13.0] * 8), F32)
    return _case(prm, [a, bad, a[::-1]], poses=[[10.0, 9.0, 0.3], [20.0, 20.0, 1.0], [30.0, 12.0, -1.2]], grids=[0, 1, 2], n_grids=3)


def clear_zero_length_case():
    """a cut shorter than half a cell from a sensor in the middle of its cell: CLEAR rays with L = 0, one miss in the sensor's cell each"""
    prm = four_beams(0.0, 0.125, 0.125, True)
    return _case(prm, [[INF, INF, INF, 0.0625], [INF, 0.1, NAN, INF]], poses=[_sensor(7, 9), _sensor(64, 63, 0.7)])


def long_case():
    """L = 32767 kept and 32768 dropped through a fine resolution (2^-10 m), not a long range: the cut is 32767.5 cells, so a sensor a quarter into its
    cell ends 32767 cells on and one in the middle of its cell 32768 cells on.  Nearly all of it outside a small grid."""
    res = 2.0 ** -10
    prm = four_beams(0.0, 40.0, res * (MAX_RAY + 0.5), True)
    n = NAN
    poses = [_sensor(67 - MAX_RAY, 10, 0.0, frac=0.25, res=res), _sensor(67 - MAX_RAY, 12, 0.0, frac=0.5, res=res)]
    return _case(prm, [[n, n, INF, n], [n, n, INF, n]], poses=poses, resolution=res)


def cap_case():
    """an end cell at +-2^20 on both sides of the cap: CLEAR rays of 80 cells along +x (beam 2) and -x (beam 0)"""
    n = NAN
    scans = [(_sensor(CAP - 1 - TRACE_CELLS, 5), [n, n, INF, n]), (_sensor(CAP - TRACE_CELLS, 5), [n, n, INF, n]),
             (_sensor(-CAP + TRACE_CELLS, 5), [INF, n, n, n]), (_sensor(-CAP - 1 + TRACE_CELLS, 5), [INF, n, n, n])]
    return _case(four_beams(0.25, 60.0, RES * TRACE_CELLS), [s[1] for s in scans], poses=[s[0] for s in scans])


# ---- realistic numbers ---------------------------------------------------------------------------------------------------------------------------------------
def random_case(seed=17, n_scans=5, n_beams=257, n_grids=2, poses=True, grids=True, no_return=0.2, clear_no_return=True):
    """resolution 0.1, an origin that is no multiple of it, rotated poses, returns up to 14 m against a gate of 12 and a cut of 9, `no_return` of the beams
    +Inf and a few NaN and too close"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0, 14.0, (n_scans, n_beams)).astype(F32)
    u = rng.random((n_scans, n_beams))
    r[u < no_return] = INF; r[u > 0.98] = NAN
    prm = api.OccupancyScanParams(n_beams, -2.35, 2.35, 0.3, 12.0, 9.0, clear_no_return)
    ps = np.stack([rng.uniform(-2.0, 9.0, n_scans), rng.uniform(-1.0, 5.0, n_scans), rng.uniform(-3.1, 3.1, n_scans)], 1).astype(F32) if poses else None
    gr = rng.integers(0, n_grids, n_scans).astype(np.int32) if grids and n_grids > 1 else None
    return _case(prm, r, ps, gr, n_grids, origin=(-3.33, -2.1), resolution=0.1)


def beams_case(n_beams, seed=3):
    """THREE scans of n_beams beams: 65 and 257 make a wave straddle two scans"""
    return random_case(seed + n_beams, 3, n_beams, 1, True, False)


def many_scans_case(n_scans, seed=4):
    """n_scans scans of 5 beams into ONE grid: 256 fill a round of box tests, 300 exceed it"""
    return random_case(seed + n_scans, n_scans, 5, 1, True, False)


def fan_case(n_beams=1081):
    """ONE scan without a single return: n_beams CLEAR rays of one origin (contention on one LDS word)"""
    prm = api.OccupancyScanParams(n_beams, -math.pi, math.pi, 0.3, 30.0, 25.0, True)
    return _case(prm, np.full((1, n_beams), INF, F32), poses=[_sensor(33, 31, 0.2)])


def returns_only_case(seed=21, n_scans=3, n_beams=721):
    """every beam in class 1 or 2 and trace_range == range_max: what lsm2d_preprocess_scans (normal_min_points 1, resolution 0) followed by
    lsm2d_occupancy_update traces too"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0, 19.5, (n_scans, n_beams)).astype(F32)
    r[rng.random((n_scans, n_beams)) > 0.97] = NAN
    prm = api.OccupancyScanParams(n_beams, -2.35, 2.35, 0.3, 20.0, 20.0, True)
    ps = np.stack([rng.uniform(5.0, 30.0, n_scans), rng.uniform(5.0, 20.0, n_scans), rng.uniform(-3.1, 3.1, n_scans)], 1).astype(F32)
    return _case(prm, r, ps, None, 1, origin=(-3.33, -2.1), resolution=0.25)


def all_cases():
    out = {}
    out["classes_clear"] = classes_case(True)
    out["classes_drop"] = classes_case(False)
    out["trace_is_max"] = trace_is_max_case()
    out["geometry"] = geometry_case()
    out["clear_only"] = clear_only_case()
    out["dropped_scan"] = dropped_scan_case()
    out["clear_zero_length"] = clear_zero_length_case()
    out["long"] = long_case()
    out["cap"] = cap_case()
    out["random"] = random_case()
    out["random_drop"] = random_case(clear_no_return=False)
    out["no_pose"] = random_case(seed=19, n_scans=2, poses=False, grids=False, n_grids=1)
    out["returns_only"] = returns_only_case()
    return out


# ---- the clouds the pins compare against ---------------------------------------------------------------------------------------------------------------------
def clouds_of(case, kind):
    """an occupancy_cases case whose clouds are the sensor-frame end points of the case's rays of ONE kind (by the class alone), normals (1, 0), a cloud per
    scan, with the case's poses and grids: what lsm2d_occupancy_update would be given for them"""
    clouds = []
    for scan in case["ranges"]:
        _, kd, xy = points(case["params"], scan)
        sel = xy[kd == kind]
        clouds.append(np.concatenate([sel, np.ones((len(sel), 1), F32), np.zeros((len(sel), 1), F32)], 1).astype(F32))
    return oc._case(clouds, case["poses"], case["grids"], case["n_grids"], case["origin"], case["resolution"])
