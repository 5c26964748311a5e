"""Log-odds grid sets (ABI 0.7.14): the accumulation restated on the host, and the cases the GPU tests run.

`reference(...)` is PARITY.md section 3, item 17e, as plain loops: tests/cpp/occupancy_logodds_ref.cpp, built once per process through tests/cpp_build.py --
scan after scan, a per-scan mark array, one clamped vote per marked cell.  It takes integer rays with a kind, which `scan_list` makes for a case of either
update call: occupancy_scan_cases.rays_of for a case with ranges, occupancy_cases.rays_of for a case with clouds (both pinned by the CPU suites of 0.7.12 and
0.7.13).  `pinned(...)` is the same result the long way round -- occupancy_scan_cases.reference / occupancy_cases.reference on each scan ALONE into a fresh
grid, H_s = hits > 0, M_s = misses > 0 and not H_s, the clamped votes in numpy in list order -- and tests/test_occupancy_logodds_abi.py holds the one to the
other bit for bit; tests/test_gpu_occupancy_logodds.py compares the device with `reference`.

The cases are occupancy_scan_cases' and occupancy_cases' (a case's dict is theirs, unchanged) and, below, the ones that are about the once-per-scan rule."""
import ctypes as C
import tempfile

import numpy as np

import cpp_build
import occupancy_cases as oc
import occupancy_scan_cases as sc
from srrg2_laser_slam_2d_amd import api

F32 = np.float32
W, H = oc.W, oc.H
SIZES = oc.SIZES
DROPPED, HIT, CLEAR = sc.DROPPED, sc.HIT, sc.CLEAR
UNIT = 0.01      # log-odds per integer unit of the default parameters
PARAMS = api.LogOddsParams(l_hit=85, l_miss=-40, l_min=-200, l_max=350)      # p_hit 0.7, p_miss 0.4, clamps at 0.12 and 0.97
I32_MAX, I32_MIN, U32_MAX = 2 ** 31 - 1, -2 ** 31, 2 ** 32 - 1

_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="occlref_")
        so = cpp_build.build("occupancy_logodds_ref.cpp", _dir.name, flags=("-O2", "-fPIC", "-shared"), link=False)
        _lib = C.CDLL(so)
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def is_scan_case(case) -> bool:
    return "ranges" in case


def n_scans(case) -> int:
    return len(case["ranges"]) if is_scan_case(case) else len(case["clouds"])


def grids_of(case) -> np.ndarray:
    return np.zeros(n_scans(case), np.int32) if case["grids"] is None else np.ascontiguousarray(case["grids"], np.int32)


def scan_list(case):
    """a case of either update call -> [(rays int32 [n, 4], kind int32 [n] = -1 / 0 HIT / 1 CLEAR)], a scan per entry in list order"""
    out = []
    for k in range(n_scans(case)):
        pose = None if case["poses"] is None else case["poses"][k]
        if is_scan_case(case):
            out.append(sc.rays_of(case["params"], case["ranges"][k], pose, case["origin"], case["resolution"]))
        else:
            rays, live = oc.rays_of(case["clouds"][k], pose, case["origin"], case["resolution"])
            out.append((rays, np.where(live, HIT, DROPPED).astype(np.int32)))      # a cloud holds returns only
    return out


def _start(n_grids, width, height, value, observed):
    v = np.zeros((n_grids, height, width), np.int32) if value is None else np.ascontiguousarray(value, np.int32).copy().reshape(n_grids, height, width)
    o = np.zeros((n_grids, height, width), np.uint32) if observed is None else np.ascontiguousarray(observed, np.uint32).copy().reshape(n_grids, height, width)
    return v, o


def reference_of(scans, grids, n_grids, width, height, params=PARAMS, value=None, observed=None):
    """the restatement over a list of (rays, kind): -> (value int32, observed uint32), [n_grids, height, width]; value / observed given: voted on in copies"""
    v, o = _start(n_grids, width, height, value, observed)
    first = np.zeros(len(scans) + 1, np.int32); first[1:] = np.cumsum([len(k) for _, k in scans])
    rays = np.ascontiguousarray(np.concatenate([r for r, _ in scans]) if scans else np.zeros((0, 4)), np.int32).reshape(-1, 4)
    kind = np.ascontiguousarray(np.concatenate([k for _, k in scans]) if scans else np.zeros(0), np.int32)
    p = params.struct()
    lib().occlref_update(C.byref(p), _p(rays), _p(kind), _p(first), len(scans), _p(np.ascontiguousarray(grids, np.int32)), int(n_grids), int(width), int(height),
                         _p(v), _p(o))
    return v, o


def reference(case, width, height, params=PARAMS, value=None, observed=None):
    return reference_of(scan_list(case), grids_of(case), case["n_grids"], width, height, params, value, observed)


def decay(value, observed, amount):
    """lsm2d_occupancy_decay restated: -> value (a copy)"""
    v = np.ascontiguousarray(value, np.int32).copy(); o = np.ascontiguousarray(observed, np.uint32)
    lib().occlref_decay(_p(v), _p(o), C.c_longlong(v.size), C.c_int32(int(amount)))
    return v


def vote(value, observed, hit, miss, params=PARAMS):
    """one scan's votes in numpy, in place: hit / miss are boolean masks of one grid (the caller has taken the hits out of the misses)"""
    v = value.astype(np.int64)
    v = np.where(hit, v + params.l_hit, np.where(miss, v + params.l_miss, v))
    voted = hit | miss
    value[...] = np.where(voted, np.clip(v, params.l_min, params.l_max), value).astype(np.int32)
    observed[...] = np.where(voted & (observed != U32_MAX), observed + np.uint32(1), observed)


def single(case, k):
    """scan k of a case alone, sent to grid 0 of one grid"""
    one = dict(case)
    one["poses"] = None if case["poses"] is None else case["poses"][k:k + 1]
    one["grids"] = None; one["n_grids"] = 1
    if is_scan_case(case):
        one["ranges"] = case["ranges"][k:k + 1]
    else:
        one["clouds"] = [case["clouds"][k]]
    return one


def scan_sets(case, width, height):
    """[(H_s, M_s)] by the pinned COUNTS references: each scan alone into a fresh grid, H_s = hits > 0, M_s = misses > 0 and not H_s"""
    out = []
    for k in range(n_scans(case)):
        one = single(case, k)
        h, m = (sc.reference(one, width, height) if is_scan_case(case) else oc.reference(one, width, height))[:2]
        out.append((h[0] > 0, (m[0] > 0) & ~(h[0] > 0)))
    return out


def pinned(case, width, height, params=PARAMS, value=None, observed=None):
    v, o = _start(case["n_grids"], width, height, value, observed)
    for (hit, miss), g in zip(scan_sets(case, width, height), grids_of(case)):
        vote(v[g], o[g], hit, miss, params)
    return v, o


# ---- the cases that are about the rule ---------------------------------------------------------------------------------------------------------------------------
def fan_with_returns_case(n_beams=1081, seed=8):
    """ONE scan of 1081 beams over a full turn from the middle of cell (33, 31): returns between 1 and 12 m, a fifth of the beams without one"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(1.0, 12.0, n_beams).astype(F32)
    r[rng.random(n_beams) < 0.2] = sc.INF
    prm = api.OccupancyScanParams(n_beams, -np.pi, np.pi, 0.3, 30.0, 10.0, True)
    return sc._case(prm, r[None, :], poses=[sc._sensor(33, 31, 0.2)])


def repeat_case(n, base=None):
    """ONE scan n times in one list: every H cell must read min(n l_hit, l_max), every M cell max(n l_miss, l_min), observed n"""
    base = fan_with_returns_case() if base is None else base
    return sc._case(base["params"], np.repeat(base["ranges"][:1], n, 0), poses=np.repeat(base["poses"][:1], n, 0), origin=base["origin"], resolution=base["resolution"])


def sheaf_case(n_beams=2048):
    """a sheaf of 2048 beams within +-0.01 rad of the heading: the even beams return from 5 m (cell x0 + 10), the odd ones return nothing and CLEAR 40 cells
    out through the cells the even ones end in.  The end cell is hit AND crossed in ONE scan: it must get l_hit."""
    r = np.where(np.arange(n_beams) % 2 == 0, F32(5.0), sc.INF).astype(F32)
    prm = api.OccupancyScanParams(n_beams, -0.01, 0.01, 0.25, 60.0, 20.0, True)
    return sc._case(prm, r[None, :], poses=[sc._sensor(20, 30)])


HIT_CELL = (30, 20)      # (x, y) of the cell the order cases are about


def order_case(n, reverse=False, far_every_third=False):
    """n scans of four beams to ONE tile from the middle of cell (10, 20): an even scan's beam 2 returns from 10 m and ends in HIT_CELL, an odd scan's returns
    nothing and clears 80 cells through it; with far_every_third every third scan stands 1000 cells away (its box misses the tile)"""
    nan = sc.NAN
    ranges, poses = [], []
    for i in range(n):
        ranges.append([nan, nan, 10.0 if i % 2 == 0 else sc.INF, nan])
        poses.append(sc._sensor(1010, 1020) if far_every_third and i % 3 == 2 else sc._sensor(10, 20))
    if reverse:
        ranges, poses = ranges[::-1], poses[::-1]
    return sc._case(sc.four_beams(0.25, 60.0, sc.RES * sc.TRACE_CELLS), ranges, poses=poses)


ORDER_PARAMS = api.LogOddsParams(l_hit=5, l_miss=-3, l_min=-3, l_max=5)      # l_max = l_hit, l_min = l_miss


def interleaved_case():
    """seven scans whose list alternates between two grids (and visits a third once)"""
    c = sc.random_case(seed=23, n_scans=7, n_beams=129, n_grids=3)
    c["grids"] = np.array([0, 1, 0, 1, 2, 1, 0], np.int32)
    return c


def edge_case():
    """rays ending on cell 63 and on cell 64, in x and in y (the 63 | 64 tile edge), as HIT rays of four scans"""
    n = sc.NAN
    scans = [(sc._sensor(33, 10), [n, n, 15.0, n]), (sc._sensor(34, 12), [n, n, 15.0, n]), (sc._sensor(5, 33, sc.UP), [n, n, 15.0, n]),
             (sc._sensor(6, 34, sc.UP), [n, n, 15.0, n])]
    return sc._case(sc.four_beams(0.25, 60.0, sc.RES * sc.TRACE_CELLS), [s[1] for s in scans], poses=[s[0] for s in scans])


def dropped_between_case():
    """occupancy_scan_cases' three scans -- ordinary, wholly dropped, ordinary -- all to ONE grid"""
    c = sc.dropped_scan_case()
    c["grids"] = None; c["n_grids"] = 1
    return c


def stress_start(width=W, height=H, params=PARAMS, seed=77):
    """uploaded cells for ONE scan of fan_with_returns_case: -> (value, observed, [(what, mask, value the cell must read, observed it must read)]).  The H
    cells and the M cells of the scan (by the pinned counts reference) are dealt start values round robin: the clamp reached exactly, exceeded by one, not
    reached by one; far outside the clamps on both sides; INT32_MAX and INT32_MIN; observed at 0, 5, 2^32 - 2 and 2^32 - 1.  Every other cell holds random
    bits, which it must keep."""
    rng = np.random.default_rng(seed)
    hit, miss = scan_sets(fan_with_returns_case(), width, height)[0]
    value = rng.integers(I32_MIN, I32_MAX, (height, width), dtype=np.int64).astype(np.int32)
    observed = rng.integers(0, U32_MAX, (height, width), dtype=np.uint64).astype(np.uint32)
    p = params
    clamp = lambda v: min(max(v, p.l_min), p.l_max)      # noqa: E731
    starts = [("reaches the clamp", lambda l, end: end - l), ("exceeds it by one", lambda l, end: end - l + (1 if l > 0 else -1)),
              ("misses it by one", lambda l, end: end - l - (1 if l > 0 else -1)), ("far above", lambda l, end: p.l_max + 1000), ("far below", lambda l, end: p.l_min - 1000),
              ("INT32_MAX", lambda l, end: I32_MAX), ("INT32_MIN", lambda l, end: I32_MIN), ("zero", lambda l, end: 0)]
    obs = [0, 5, U32_MAX - 1, U32_MAX]
    checks = []
    for name, mask, l, end in (("hit", hit, p.l_hit, p.l_max), ("miss", miss, p.l_miss, p.l_min)):
        ys, xs = np.nonzero(mask)
        assert len(ys) >= len(starts) * len(obs), (name, len(ys))
        for i, (y, x) in enumerate(zip(ys, xs)):
            what, f = starts[i % len(starts)]
            o = obs[(i // len(starts)) % len(obs)]
            v = f(l, end)
            value[y, x] = v; observed[y, x] = o
            if i < len(starts) * len(obs):
                checks.append(("%s cell, %s, observed %d" % (name, what, o), (y, x), clamp(v + l), min(o + 1, U32_MAX)))
    return value, observed, checks, hit, miss


def scan_cases():
    out = dict(sc.all_cases())
    out["dropped_between"] = dropped_between_case()
    out["fan"] = sc.fan_case()
    out["fan_with_returns"] = fan_with_returns_case()
    out["sheaf"] = sheaf_case()
    out["repeat_3"] = repeat_case(3)
    out["order_7"] = order_case(7)
    out["order_far_9"] = order_case(9, far_every_third=True)
    out["interleaved"] = interleaved_case()
    out["edge"] = edge_case()
    return out


def cloud_cases():
    return dict(oc.all_cases())
