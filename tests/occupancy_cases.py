"""lsm2d_occupancy_update (ABI 0.7.12): the definition restated on the host, and the cases the GPU tests run.

`reference(...)` is PARITY.md section 3, item 17c, as plain loops: a small C++ file (tests/cpp/occupancy_ref.cpp) built once per process through
tests/cpp_build.py.  tests/test_occupancy_abi.py pins its transform to voxelize_cases.transform (itself pinned to the oracle's merger), its walk to an
independent incremental one and to the ideal line in exact rationals, and checks that the cases below contain what they claim;
tests/test_gpu_occupancy.py compares the device with it bit for bit.

A case is a dict: clouds (list of float32 [n, 4]), poses ([n_inputs, 3] or None), grids ([n_inputs] or None), n_grids, origin (ox, oy), resolution.  The
grid's SIZE is not part of a case: the GPU test runs every case on several sizes.  Cells are chosen directly: with resolution 0.5 (inverse 2, exact) and
an origin that is a multiple of 0.25, a sensor at pose (ox + 0.5 (x0 + 0.5), oy + 0.5 (y0 + 0.5), 0) stands in cell (x0, y0) and the sensor-frame point
(0.5 (x1 - x0), 0.5 (y1 - y0)) lands in the middle of cell (x1, y1): every operation is exact in fp32."""
import ctypes as C
import tempfile

import numpy as np

import cpp_build
from srrg2_laser_slam_2d_amd import _capi

F32 = np.float32
TILE = _capi.OCCUPANCY_TILE
BLOCK = _capi.OCCUPANCY_BLOCK
MAX_RAY = _capi.OCCUPANCY_MAX_RAY_CELLS
CAP = 1 << 20
RES = 0.5
W, H = 130, 70      # the size the cases' claims about the grid's borders and tile edges refer to
SIZES = [(1, 1), (64, 64), (65, 63), (W, H)]

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="occref_")
        so = cpp_build.build("occupancy_ref.cpp", _dir.name, flags=("-O2", "-fPIC", "-shared", "-ffp-contract=off"), link=False)
        _lib = C.CDLL(so)
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def transform(points, pose) -> np.ndarray:
    """item 17c.1 alone: x and y of the points moved by one pose (the normals copied)"""
    pts = np.ascontiguousarray(points, F32).reshape(-1, 4); out = np.empty_like(pts)
    lib().occref_transform(_p(pts), len(pts), _p(np.ascontiguousarray(pose, F32)), _p(out))
    return out


def rays_of(points, pose, origin, resolution):
    """items 17c.1-2 for ONE input: (int32 [n, 4] = x0, y0, x1, y1; bool [n] live)"""
    pts = np.ascontiguousarray(points, F32).reshape(-1, 4)
    rays = np.zeros((len(pts), 4), np.int32); live = np.zeros(len(pts), np.int32)
    ps = None if pose is None else np.ascontiguousarray(pose, F32)
    lib().occref_rays(_p(pts), len(pts), _p(ps), C.c_float(origin[0]), C.c_float(origin[1]), C.c_float(resolution), _p(rays), _p(live))
    return rays, live.astype(bool)


def walk(ray) -> np.ndarray:
    """item 17c.3: the L + 1 cells of a ray in step order, int32 [L + 1, 2]"""
    r = np.ascontiguousarray(ray, np.int32)
    L = int(max(abs(int(r[2]) - int(r[0])), abs(int(r[3]) - int(r[1]))))
    out = np.empty((L + 1, 2), np.int32)
    lib().occref_walk(_p(r), _p(out))
    return out


def case_rays(case):
    """every ray of a case: (int32 [n, 4], live [n]) over the concatenated inputs"""
    rr, ll = [], []
    for k, c in enumerate(case["clouds"]):
        r, l = rays_of(c, None if case["poses"] is None else case["poses"][k], case["origin"], case["resolution"])
        rr.append(r); ll.append(l)
    return np.concatenate(rr), np.concatenate(ll)


def reference(case, width, height, hits=None, misses=None):
    """-> (hits, misses uint32 [n_grids, height, width], rays, dropped int32 [n_grids]); hits / misses given: accumulated into copies of them"""
    clouds = [np.ascontiguousarray(c, F32).reshape(-1, 4) for c in case["clouds"]]
    offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate(clouds) if clouds else np.zeros((0, 4), F32), F32)
    ps = None if case["poses"] is None else np.ascontiguousarray(case["poses"], F32).reshape(len(clouds), 3)
    gr = None if case["grids"] is None else np.ascontiguousarray(case["grids"], np.int32).reshape(len(clouds))
    ng = int(case["n_grids"])
    h = np.zeros((ng, height, width), np.uint32) if hits is None else np.ascontiguousarray(hits, np.uint32).copy().reshape(ng, height, width)
    m = np.zeros((ng, height, width), np.uint32) if misses is None else np.ascontiguousarray(misses, np.uint32).copy().reshape(ng, height, width)
    rays = np.zeros(ng, np.int32); dropped = np.zeros(ng, np.int32)
    lib().occref_update(_p(pts), _p(offs), len(clouds), _p(ps), _p(gr), ng, C.c_float(case["origin"][0]), C.c_float(case["origin"][1]),
                        C.c_float(case["resolution"]), int(width), int(height), _p(h), _p(m), _p(rays), _p(dropped))
    return h, m, rays, dropped


# ---- rays with chosen cells --------------------------------------------------------------------------------------------------------------------------------
def _case(clouds, poses=None, grids=None, n_grids=1, origin=(0.0, 0.0), resolution=RES):
    return dict(clouds=[np.ascontiguousarray(c, F32).reshape(-1, 4) for c in clouds], poses=None if poses is None else np.asarray(poses, F32).reshape(-1, 3),
                grids=None if grids is None else np.asarray(grids, np.int32), n_grids=n_grids, origin=(float(origin[0]), float(origin[1])), resolution=float(resolution))


def cell_rays(rays, origin=(0.0, 0.0), grids=None, n_grids=1):
    """a case whose rays are exactly `rays` (x0, y0, x1, y1 in cells): one input per run of equal (x0, y0), in order"""
    clouds, poses, cur, key = [], [], [], None
    for x0, y0, x1, y1 in rays:
        if (x0, y0) != key:
            if cur:
                clouds.append(np.array(cur, F32))
            cur, key = [], (x0, y0)
            poses.append([origin[0] + RES * (x0 + 0.5), origin[1] + RES * (y0 + 0.5), 0.0])
        cur.append([RES * (x1 - x0), RES * (y1 - y0), 1.0, 0.0])
    clouds.append(np.array(cur, F32))
    return _case(clouds, poses, grids, n_grids, origin)


def octant_rays(x0=40, y0=30):
    ends = [(7, 3), (3, 7), (-3, 7), (-7, 3), (-7, -3), (-3, -7), (3, -7), (7, -3),      # the eight octants
            (9, 0), (-9, 0), (0, 9), (0, -9),                                            # both axes, both ways
            (5, 5), (-5, 5), (-5, -5), (5, -5),                                          # ax == ay: x-major by the tie rule
            (8, 4), (-8, 4), (8, -4), (-8, -4), (4, 8), (-4, 8), (4, -8), (-4, -8),      # a / L = 1 / 2: rounding ties at every odd step
            (0, 0), (1, 0), (0, -1), (1, 1), (-1, 1)]                                    # L = 0 and L = 1
    return [(x0, y0, x0 + dx, y0 + dy) for dx, dy in ends]


def border_rays():
    """against a grid of W x H cells: rays that enter, leave, cross with both ends outside, miss; the last row and column; the 63 | 64 tile edge"""
    return [(-6, 10, 9, 14), (20, -9, 24, 6),                     # enter: start outside, end inside
            (120, 60, 140, 66), (10, 60, 14, 80),                 # leave: start inside, end outside
            (-5, 20, 135, 44), (30, -8, 50, 78), (-4, -4, 80, 80),      # cross: both ends outside
            (-20, -3, 150, -1), (140, 0, 160, 69), (-9, 75, -1, 100),   # miss entirely
            (3, H - 1, 127, H - 1), (W - 1, 2, W - 1, 68),        # along the last row and the last column
            (0, 0, W - 1, 0), (0, 0, 0, H - 1),                   # ... and the first
            (50, 5, 80, 9), (80, 9, 50, 5),                       # crosses 63 | 64 on the major axis (x), both ways
            (70, 50, 74, 69), (74, 69, 70, 50),                   # ... on the major axis (y)
            (20, 60, 50, 67), (66, 20, 60, 50),                   # ... on the minor axis: x-major with y over 63 | 64, y-major with x over 64 | 63
            (63, 63, 64, 64), (64, 64, 63, 63), (63, 64, 64, 63)]      # the four cells round the tile corner


def long_rays():
    """L = 32767 kept and L = 32768 dropped, nearly all of it outside a small grid; x-major and y-major"""
    return [(67 - MAX_RAY, 10, 67, 20), (67 - MAX_RAY, 10, 68, 20), (30, 40 + MAX_RAY, 12, 40), (30, 40 + MAX_RAY, 12, 39)]


def cap_rays():
    """a cell coordinate at +-2^20, on both sides of the cap, on both axes; and a sensor outside the cap"""
    return [(CAP - 10, 5, CAP - 1, 5), (CAP - 10, 5, CAP, 5), (5, CAP - 10, 5, CAP - 1), (5, CAP - 10, 5, CAP),
            (-CAP + 3, 5, -CAP, 5), (-CAP + 3, 5, -CAP - 1, 5), (5, -CAP + 3, 5, -CAP), (5, -CAP + 3, 5, -CAP - 1),
            (CAP, 0, CAP - 3, 0), (0, -CAP - 1, 0, -CAP + 2)]


def edge_points():
    """no pose, origin (0, 0), so the sensor is in cell (0, 0): end points exactly on a cell edge and one ulp either side, in x and in y.
    -> (points, expected end cells)"""
    up, down = F32(np.inf), F32(-np.inf)
    pts, cells = [], []
    for c in (1, 7, 64, -1, -3):
        e = F32(RES * c)      # the edge between cells c - 1 and c
        for v, cc in ((e, c), (np.nextafter(e, up), c), (np.nextafter(e, down), c - 1)):
            pts.append([v, F32(1.3), 0, 1]); cells.append((cc, 2))
            pts.append([F32(-0.7), v, 0, 1]); cells.append((-2, cc))
    return np.array(pts, F32), np.array(cells, np.int32)


def nonfinite_points():
    """NaN and both infinities in x and in y, among ordinary points: (points, has a ray)"""
    rows, ok = [], []
    for v in (F32(np.nan), F32(np.inf), F32(-np.inf)):
        rows += [[v, 1.0, 1, 0], [1.0, v, 1, 0], [v, v, 1, 0]]; ok += [False] * 3
        rows.append([2.25, -1.75, 1, 0]); ok.append(True)
    return np.array(rows, F32), np.array(ok)


def random_case(seed=17, n_inputs=5, n_points=300, n_grids=2):
    """realistic numbers: resolution 0.1, an origin that is no multiple of it, rotated poses, ranges up to 9 m"""
    rng = np.random.default_rng(seed)
    clouds = []
    for _ in range(n_inputs):
        a = rng.uniform(-np.pi, np.pi, n_points); r = rng.uniform(0.0, 9.0, n_points)
        clouds.append(np.stack([r * np.cos(a), r * np.sin(a), -np.cos(a), -np.sin(a)], 1).astype(F32))
    poses = np.stack([rng.uniform(-2.0, 9.0, n_inputs), rng.uniform(-1.0, 5.0, n_inputs), rng.uniform(-3.1, 3.1, n_inputs)], 1).astype(F32)
    return _case(clouds, poses, rng.integers(0, n_grids, n_inputs) if n_grids > 1 else None, n_grids, origin=(-3.33, -2.1), resolution=0.1)


def fan_case(n_rays, x0=33, y0=31, seed=3):
    """ONE input of n_rays rays from one cell, ends scattered over and beyond a W x H grid"""
    rng = np.random.default_rng(seed)
    ends = np.stack([rng.integers(-20, W + 20, n_rays), rng.integers(-20, H + 20, n_rays)], 1)
    return cell_rays([(x0, y0, int(ex), int(ey)) for ex, ey in ends])


def many_inputs_case(n_inputs, seed=4):
    """n_inputs inputs of a few rays each into ONE grid, every input its own sensor cell (two of them outside the grid)"""
    rng = np.random.default_rng(seed)
    rays = []
    for k in range(n_inputs):
        x0, y0 = (k * 7) % (W + 8) - 4, (k * 13) % (H + 6) - 3
        for _ in range(1 + k % 3):
            rays.append((x0, y0, int(rng.integers(-10, W + 10)), int(rng.integers(-10, H + 10))))
        if k + 1 < n_inputs and ((k + 1) * 7) % (W + 8) - 4 == x0 and ((k + 1) * 13) % (H + 6) - 3 == y0:
            raise AssertionError("two inputs in a row share a sensor cell")
    return cell_rays(rays)


def all_cases():
    out = {}
    out["octants"] = cell_rays(octant_rays())
    out["negative"] = cell_rays(octant_rays(-5, -7) + [(-3, -2, 6, 4), (4, 3, -6, -9)], origin=(-1.25, 0.75))
    out["borders"] = cell_rays(border_rays())
    out["long"] = cell_rays(long_rays())
    out["cap"] = cell_rays(cap_rays())
    out["edges"] = _case([edge_points()[0]])
    nf = nonfinite_points()[0]
    out["nonfinite"] = _case([nf])
    rng = np.random.default_rng(9)
    ordinary = np.stack([rng.uniform(-5, 30, 40), rng.uniform(-5, 20, 40), np.ones(40), np.zeros(40)], 1).astype(F32)
    bad = np.full((25, 4), np.nan, F32)
    out["empty_and_dropped"] = _case([ordinary, np.zeros((0, 4), F32), bad, ordinary[::-1] + F32(0.5)], poses=[[3.25, 2.25, 0.4], [1.0, 1.0, 0.0], [2.0, 2.0, 1.0], [9.75, 7.25, -2.0]],
                                     grids=[0, 1, 2, 0], n_grids=3)
    out["random"] = random_case()
    return out
