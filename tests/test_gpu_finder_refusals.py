"""GPU tests of what the finder, factor and score entry points REFUSE: one table of bad calls through the raw ABI for lsm2d_find_correspondences,
lsm2d_find_correspondences_batch, lsm2d_linearize_batch, lsm2d_score_batch and lsm2d_score_select.  Every row states the status and the text of
lsm2d_last_error literally; the rows with two things wrong at once pin which check comes first.  A refused call leaves its outputs as they were (a row
says so where the ABI defines otherwise: lsm2d_find_correspondences sets its count once the arguments are accepted).  Six items, scans of 721 beams
against a map of 4000 points; all but two rows are refused before anything is launched, and every call is one the ABI defines a refusal for."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import _projector
from srrg2_laser_slam_2d_amd import api, synth
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, CAPACITY_EXCEEDED

pytestmark = pytest.mark.gpu

N = 6
COLS = 721
MAP = 4000
MD = 0.4
BUSY = "two batches are in flight on this context and its staging buffers are theirs: wait for the older one first (lsm2d_align_batch_wait)"

# the arguments of the five entry points, in the ABI's order
ARGS = {
    "find": ("ctx", "sp", "fixed", "fi", "moving", "mi", "pose", "out_pairs", "capacity", "out_n"),
    "find_batch": ("ctx", "sp", "fixed", "fixed_index", "moving", "moving_index", "n_items", "poses", "out_pairs", "pair_capacity", "out_n_pairs"),
    "linearize_batch": ("ctx", "sp", "fixed", "fixed_index", "moving", "moving_index", "n_items", "pairs", "pair_capacity", "n_pairs", "poses", "out_H",
                        "out_b", "st"),
    "score_batch": ("ctx", "sp", "fixed", "fixed_index", "moving", "moving_index", "n_items", "poses", "out_H", "out_b", "st"),
    "score_select": ("ctx", "sp", "fixed", "fixed_index", "moving", "moving_index", "n_items", "poses", "select", "k", "out_index", "out_H", "out_b",
                     "out_stats", "out_n_selected", "out_n_accepted"),
}
SYMBOL = {"find": "lsm2d_find_correspondences", "find_batch": "lsm2d_find_correspondences_batch", "linearize_batch": "lsm2d_linearize_batch",
          "score_batch": "lsm2d_score_batch", "score_select": "lsm2d_score_select"}
OUTPUTS = ("out_pairs", "out_n", "out_n_pairs", "out_H", "out_b", "st", "out_index", "out_stats", "out_n_selected", "out_n_accepted")


class _Fx:
    pass


@pytest.fixture(scope="module")
def fx(ctx):
    f = _Fx()
    f.ctx = ctx
    world = synth.make_world(4)
    f.map = synth.make_map(world, MAP, seed=2)
    assert len(f.map) == MAP
    robots = synth.sample_poses(world, N, seed=8)
    pts, offs = synth.make_scans(world, robots, n_beams=COLS, noise_sigma=0.01, seed=5)
    f.counts = np.diff(offs).tolist()
    assert len(f.counts) == N and min(f.counts) > 100
    f.x0 = synth.invert_poses(synth.compose_poses(robots, np.array([[0.12, -0.08, 0.04]] * N))).astype(np.float32)
    f.scans = api.CloudSet(ctx, pts, offs)
    f.map_set = api.CloudSet(ctx, f.map)
    third = np.ascontiguousarray(f.map[::3])
    f.three = api.CloudSet(ctx, np.ascontiguousarray(np.concatenate([f.map, third, third])), np.int32([0, MAP, MAP + len(third), MAP + 2 * len(third)]))
    f.other = api.Context(0)
    f.foreign = api.CloudSet(f.other, f.map)
    f.proj = api.CorrespondenceFinderProjective2f(ctx, _projector(COLS))
    f.nn = api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=MD, search="exact")
    f.n_found = {}
    for kind, finder in (("proj", f.proj), ("nn", f.nn)):      # what the single call finds for item 0: the rows "one short" need the number
        finder.setFixed(f.scans, 0); finder.setMoving(f.map_set); finder.setLocalMapInSensor(f.x0[0])
        f.n_found[kind] = len(finder.compute())
        assert f.n_found[kind] > 1, kind
    yield f
    del f.foreign
    f.other.close()


# ---- the values a row may put in an argument's place: fx -> value --------------------------------------------------------------------------------------------------
def sp_proj(cols):
    return lambda f: api.CorrespondenceFinderProjective2f(f.ctx, _projector(cols)).slice_params()


def sp_nn(md=MD):
    return lambda f: api.CorrespondenceFinderKDTree2D(f.ctx, max_distance_m=md, search="exact").slice_params()


def sp_unknown_finder(f):
    sp = f.proj.slice_params(); sp.finder = 99
    return sp


def sp_cols(cols):      # a projector the Python classes would not build
    def make(f):
        sp = f.proj.slice_params(); sp.projector.canvas_cols = cols
        return sp
    return make


def index(*v):
    return lambda f: np.int32(v)


def counts(**at):      # n_pairs: 3 everywhere but where the row says
    def make(f):
        c = np.full(N, 3, np.int32)
        for k, v in at.items():
            c[int(k[1:])] = v
        return c
    return make


def pairs_with(item, k, fixed_idx, moving_idx):      # the correspondence vectors: (0, 0) everywhere but pair k of one item
    def make(f):
        p = np.zeros((N, COLS, 2), np.int32); p[item, k] = (fixed_idx, moving_idx)
        return p
    return make


foreign = lambda f: f.foreign
three = lambda f: f.three
found_less_one = lambda kind: (lambda f: f.n_found[kind] - 1)
found = lambda kind: (lambda f: f.n_found[kind])
LDS_COLS = 16384      # two canvases of 8-byte cells: 256 KiB, more LDS than a workgroup can have


def _good(f, entry):
    """the arguments of a call that succeeds, outputs filled with a pattern"""
    cap = max(COLS, MAP)
    a = dict(ctx=f.ctx.handle, sp=f.proj.slice_params(), fixed=f.scans, moving=f.map_set, fixed_index=None, moving_index=None, n_items=N,
             poses=np.ascontiguousarray(f.x0), out_H=np.full((N, 9), -7.0, np.float32), out_b=np.full((N, 3), -7.0, np.float32),
             st=np.full(N * 7, 0x5A5A5A5A, np.uint32))
    if entry == "find":
        a.update(fi=0, mi=0, pose=np.ascontiguousarray(f.x0[0]), out_pairs=np.full((cap, 2), -7, np.int32), capacity=COLS, out_n=C.c_int32(-7))
    elif entry == "find_batch":
        a.update(out_pairs=np.full((N, LDS_COLS, 2), -7, np.int32), pair_capacity=COLS, out_n_pairs=np.full(N, -7, np.int32))
    elif entry == "linearize_batch":
        a.update(pairs=np.zeros((N, COLS, 2), np.int32), pair_capacity=COLS, n_pairs=np.full(N, 3, np.int32))
    elif entry == "score_select":
        a.update(select=api.SelectParams(0, float("inf"), 0.0).struct(), k=4, out_index=np.full(4, -7, np.int32), out_stats=np.full(4 * 7, 0x5A5A5A5A, np.uint32),
                 out_n_selected=C.c_int32(-7), out_n_accepted=C.c_int32(-7))
    return {name: a[name] for name in ARGS[entry]}


def _c(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data_as(C.c_void_p)
    if isinstance(v, api.CloudSet):
        return v.handle
    if isinstance(v, (C.Structure, C.c_int32)):
        return C.byref(v)
    return v


def _snapshot(a):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v.value) for k, v in a.items() if k in OUTPUTS and v is not None}


def _call(f, entry, a):
    return getattr(f.ctx._lib, SYMBOL[entry])(*[_c(a[name]) for name in ARGS[entry]])


def _last_error(f, a):
    return f.ctx._lib.lsm2d_last_error(a["ctx"]).decode()      # a call without a context leaves its text with the thread


@contextlib.contextmanager
def _both_lanes_busy(f):
    al = api.MultiAligner2D(f.ctx, max_iterations=5, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(f.proj, min_num_correspondences=10))
    a, b = al.prepare_batch([f.scans], [f.map_set], f.x0), al.prepare_batch([f.scans], [f.map_set], f.x0[::-1].copy(), fixed_index=np.int32([[5, 4, 3, 2, 1, 0]]))
    a.begin(); b.begin()
    try:
        yield
    finally:
        a.wait(copy=True); b.wait(copy=True)


# ---- the table: (entry point, what is wrong: argument -> value or fx -> value, status, text[, outputs the refusal does write: name -> value]) -----------------------
def _who(entry):
    return SYMBOL[entry][len("lsm2d_"):]


def _rows():
    R = []
    BA, CAP = BAD_ARGUMENT, CAPACITY_EXCEEDED

    def row(entry, wrong, status, text, writes=None, busy=False):
        R.append(pytest.param(entry, wrong, status, text, writes or {}, busy, id="%s-%02d-%s" % (entry, len(R), "+".join(wrong) or "lanes_busy")))

    # -- lsm2d_find_correspondences: one check, one text, for everything about the arguments' shape
    bad = "find_correspondences: bad argument"
    for wrong in (dict(ctx=None), dict(sp=None), dict(fixed=None), dict(moving=None), dict(pose=None), dict(out_n=None), dict(out_pairs=None), dict(capacity=-1),
                  dict(fi=-1), dict(fi=N), dict(mi=-1), dict(mi=1)):
        row("find", wrong, BA, bad)
    row("find", dict(sp=sp_unknown_finder), BA, "find_correspondences: finder not supported yet", dict(out_n=0))
    row("find", dict(sp=sp_cols(0)), BA, "find_correspondences: bad projector", dict(out_n=0))
    row("find", dict(sp=sp_proj(LDS_COLS)), CAP, "find_correspondences: canvases do not fit LDS", dict(out_n=0))
    row("find", dict(sp=sp_nn(0.0)), BA, "find_correspondences: max_distance must be > 0", dict(out_n=0))
    row("find", dict(capacity=found_less_one("proj")), CAP, "find_correspondences: out_pairs too small", dict(out_n=found("proj")))      # (these two run the finder)
    row("find", dict(sp=sp_nn(), capacity=found_less_one("nn")), CAP, "find_correspondences: out_pairs too small", dict(out_n=found("nn")))
    row("find", {}, BA, BUSY, dict(out_n=0), busy=True)
    row("find", dict(fi=-1, sp=sp_unknown_finder), BA, bad)
    row("find", dict(capacity=-1, sp=sp_cols(0)), BA, bad)

    # -- the head and the index rules of the four batch entry points
    for entry in ("find_batch", "linearize_batch", "score_batch", "score_select"):
        who = _who(entry)
        item = (lambda i: "") if entry == "find_batch" else (lambda i: "item %d: " % i)      # find_correspondences_batch does not name the item
        first_null = dict(find_batch="out_n_pairs", linearize_batch="n_pairs", score_batch="out_H", score_select="poses")[entry]
        for wrong in (dict(ctx=None), dict(sp=None), dict(fixed=None), dict(moving=None), dict(n_items=-1)):
            row(entry, wrong, BA, who + ": bad argument")
        if "pair_capacity" in ARGS[entry]:
            row(entry, dict(pair_capacity=-1), BA, who + ": bad argument")
        row(entry, dict(fixed=foreign), BA, who + ": cloud set from another (or a destroyed) context")
        row(entry, dict(moving=foreign), BA, who + ": cloud set from another (or a destroyed) context")
        row(entry, {}, BA, BUSY, busy=True)
        nulls = dict(find_batch=("poses", "out_n_pairs", "out_pairs"), linearize_batch=("n_pairs", "poses", "out_H", "out_b", "pairs"),
                     score_batch=("poses", "out_H", "out_b"), score_select=("poses", "select", "out_index", "out_n_selected", "out_n_accepted"))[entry]
        for name in nulls:
            row(entry, {name: None}, BA, who + ": null argument")
        row(entry, dict(fixed=three), BA, who + ": fixed set must hold 1 or n_items clouds")      # NULL index, 3 clouds, 6 items
        row(entry, dict(moving=three), BA, who + ": moving set must hold 1 or n_items clouds")
        row(entry, dict(fixed_index=index(0, 1, 2, 3, 4, 6)), BA, who + ": " + item(5) + "cloud index out of range")
        row(entry, dict(fixed_index=index(0, 1, -1, 3, 4, 5)), BA, who + ": " + item(2) + "cloud index out of range")
        row(entry, dict(moving_index=index(0, 0, 0, 1, 0, 0)), BA, who + ": " + item(3) + "cloud index out of range")
        row(entry, dict(moving_index=index(-1, 0, 0, 0, 0, 0)), BA, who + ": " + item(0) + "cloud index out of range")
        # two things wrong at once: the earlier check answers
        row(entry, {"n_items": -1, first_null: None}, BA, who + ": bad argument")
        row(entry, dict(moving=foreign, fixed_index=index(0, 1, 2, 3, 4, 6)), BA, who + ": cloud set from another (or a destroyed) context")
        row(entry, dict(n_items=0), BA, BUSY, busy=True)      # an empty batch is a no-op only on a context that could run it
        row(entry, {first_null: None, "fixed_index": index(0, 1, 2, 3, 4, 6)}, BA, who + ": null argument")
        row(entry, dict(fixed=three, moving_index=index(0, 0, 0, 1, 0, 0)), BA, who + ": fixed set must hold 1 or n_items clouds")
        row(entry, dict(fixed=three, moving=three), BA, who + ": fixed set must hold 1 or n_items clouds")
        if entry != "linearize_batch":      # the finder's own checks come behind the index rules
            row(entry, dict(fixed_index=index(0, 1, 2, 3, 4, 6), sp=sp_unknown_finder), BA, who + ": " + item(5) + "cloud index out of range")

    # -- lsm2d_find_correspondences_batch: the capacity rule, then the finder
    who, short = "find_correspondences_batch", "find_correspondences_batch: pair_capacity below the largest possible correspondence vector"
    row("find_batch", dict(pair_capacity=COLS - 1), CAP, short)
    row("find_batch", dict(sp=sp_nn(), pair_capacity=MAP - 1), CAP, short)      # a point-query finder: the largest moving cloud
    row("find_batch", dict(pair_capacity=COLS - 1, moving_index=index(0, 0, 0, 1, 0, 0)), BA, who + ": cloud index out of range")
    row("find_batch", dict(sp=sp_unknown_finder), CAP, short)      # not projective: sized like a point query, before the finder is looked at
    row("find_batch", dict(sp=sp_unknown_finder, pair_capacity=MAP), BA, who + ": finder not supported")
    row("find_batch", dict(sp=sp_cols(0)), BA, who + ": bad projector")
    row("find_batch", dict(sp=sp_cols(-5)), BA, who + ": bad projector")
    row("find_batch", dict(sp=sp_proj(LDS_COLS), pair_capacity=LDS_COLS), CAP, who + ": canvases do not fit LDS")
    row("find_batch", dict(sp=sp_nn(0.0), pair_capacity=MAP), BA, who + ": max_distance must be > 0")

    # -- lsm2d_linearize_batch: every item's vector is checked before anything is launched
    who = "linearize_batch"
    row(who, dict(n_pairs=counts(i3=-1)), BA, "linearize_batch: item 3: n_pairs -1 outside [0, pair_capacity 721]")
    row(who, dict(n_pairs=counts(i4=COLS + 1)), BA, "linearize_batch: item 4: n_pairs 722 outside [0, pair_capacity 721]")
    row(who, dict(pair_capacity=2), BA, "linearize_batch: item 0: n_pairs 3 outside [0, pair_capacity 2]")      # one short of what every item holds
    row(who, dict(pairs=pairs_with(2, 1, 100000, 0)), BA, "linearize_batch: item 2: correspondence 1 (100000, 0) out of range")
    row(who, dict(pairs=pairs_with(5, 0, 0, MAP)), BA, "linearize_batch: item 5: correspondence 0 (0, 4000) out of range")
    row(who, dict(pairs=pairs_with(1, 2, -1, 0)), BA, "linearize_batch: item 1: correspondence 2 (-1, 0) out of range")
    row(who, dict(n_pairs=counts(i1=-1), pairs=pairs_with(0, 1, 0, MAP)), BA, "linearize_batch: item 0: correspondence 1 (0, 4000) out of range")      # item by item
    row(who, dict(n_pairs=counts(i0=-1), fixed_index=index(0, 1, 2, 3, 4, 6)), BA, "linearize_batch: item 5: cloud index out of range")
    row(who, dict(pairs=None, n_pairs=counts(i0=0, i1=-1)), BA, "linearize_batch: item 1: n_pairs -1 outside [0, pair_capacity 721]")      # item 0 holds nothing: no vector needed

    # -- lsm2d_score_batch and lsm2d_score_select: the finder's checks, with the caller's name
    for entry in ("score_batch", "score_select"):
        who = _who(entry)
        row(entry, dict(sp=sp_unknown_finder), BA, who + ": finder not supported")
        row(entry, dict(sp=sp_cols(0)), BA, who + ": bad projector")
        row(entry, dict(sp=sp_cols(-5)), BA, who + ": bad projector")
        row(entry, dict(sp=sp_proj(LDS_COLS)), CAP, who + ": canvases do not fit LDS")
        row(entry, dict(sp=sp_nn(0.0)), BA, who + ": max_distance must be > 0")

    # -- lsm2d_score_select: its own arguments come first of all
    krange = "score_select: k outside [1, LSM2D_SELECT_MAX_K]"
    for k in (0, -3, api.SELECT_MAX_K + 1):
        row("score_select", dict(k=k), BA, krange)
    row("score_select", dict(ctx=None, k=0), BA, krange)
    row("score_select", dict(n_items=-1, k=api.SELECT_MAX_K + 1), BA, krange)
    row("score_select", dict(select=None, k=0), BA, "score_select: null argument")
    row("score_select", dict(out_index=None, ctx=None), BA, "score_select: null argument")
    row("score_select", dict(k=0), BA, krange, busy=True)
    return R


@pytest.mark.parametrize("entry,wrong,status,text,writes,busy", _rows())
def test_refused(fx, entry, wrong, status, text, writes, busy):
    a = _good(fx, entry)
    for name, v in wrong.items():
        assert name in a, name
        a[name] = v(fx) if callable(v) else v
    before = _snapshot(a)
    with (_both_lanes_busy(fx) if busy else contextlib.nullcontext()):
        rc = _call(fx, entry, a)
        message = _last_error(fx, a)
    print(entry, sorted(wrong), "->", rc, repr(message))
    assert rc == status and message == text, (rc, message)
    after = _snapshot(a)
    for name, was in before.items():
        want = writes[name](fx) if callable(writes.get(name)) else writes.get(name, was)
        assert np.array_equal(after[name], want), (name, "written by a refused call")


@pytest.mark.parametrize("entry", list(ARGS))
def test_the_table_s_call_succeeds_with_nothing_wrong(fx, entry):
    a = _good(fx, entry)
    assert _call(fx, entry, a) == 0, _last_error(fx, a)
    if entry == "find":
        assert a["out_n"].value == fx.n_found["proj"]
    if entry == "score_select":
        assert a["out_n_selected"].value == 4 and a["out_n_accepted"].value == N
