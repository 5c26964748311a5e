"""Every device buffer, pinned buffer, event and stream the host side of the C ABI acquires is released exactly once: the process-wide count of live
handles ("live_handles", a read-only option: csrc/lsm2d_capi_own.h counts where an owner acquires and where it releases) returns to where it stood once a
context and its sets are gone -- in either order.  Free-memory readings cannot show this on a GPU that others use; integers can.

One sequence makes a set of every kind and every derived structure, walks the drop / recycle paths of a reserved set, provokes two refused calls half-way,
begins a batch asynchronously, and destroys half the sets before the context and half after it (the orphans).  Clouds have 64 to 2000 points, scans 181
beams, batches 2 alignments of 3 iterations -- with one exception: the tile bounds of the point-query finders' culling are only built for a moving cloud
of at least 4096 points (AlignBatch::lay_out_lds), so that one call's moving cloud has 4200."""
import ctypes as C
import gc

import numpy as np
import pytest

from srrg2_laser_slam_2d_amd import _capi, api, synth

pytestmark = pytest.mark.gpu

ITS = 3


def _clouds():
    world = synth.make_world(6)
    c = {n: synth.make_map(world, n, noise_sigma=0.002, seed=n) for n in (64, 600, 700, 1281, 1500, 2000, 4200)}
    poses = synth.sample_poses(world, 2, seed=5)
    c["ranges"] = synth.make_scan_ranges(world, poses, n_beams=181, angle_min=-2.3, angle_max=2.3, noise_sigma=0.004, seed=9)
    return c


def _aligner(ctx, finder):
    al = api.MultiAligner2D(ctx, max_iterations=ITS, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, min_num_correspondences=10))
    return al


def _sequence(observer, c, tag):
    """-> the live-handle counts seen on the way; the context it makes and everything on it is gone when it returns"""
    live = lambda: observer.get_option("live_handles")
    seen = [live()]

    def grew(what):      # the step just made something: the count says so
        seen.append(live())
        print("%s: %-34s live_handles %d (+%d)" % (tag, what, seen[-1], seen[-1] - seen[-2]))
        assert seen[-1] > seen[-2], (what, seen)

    ctx = api.Context(0)
    grew("context")
    x2 = np.zeros((2, 3), np.float32); x2[1] = (0.01, -0.01, 0.005)
    x1 = x2[:1]
    proj = api.PointNormal2fProjectorPolar(361, -np.pi, np.pi, 0.3, 30.0)
    # ---- one set of each kind
    scans = api.CloudSet(ctx, np.concatenate([c[700], c[64]]), np.int32([0, 700, 764]))      # lsm2d_cloudset_create, two clouds
    grew("cloudset_create")
    m2000, m4200, one1281 = api.CloudSet(ctx, c[2000]), api.CloudSet(ctx, c[4200]), api.CloudSet(ctx, c[1281])
    reserved = api.CloudSet.reserved(ctx, 2048)
    grew("reserved")
    many = api.CloudSet.reserved_many(ctx, 3, 256)
    grew("reserved-many")
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=0.3, range_max=20.0)
    pre.setRawData(c["ranges"], -2.3, 2.3, 0.0, 30.0)
    prep = pre.compute()                                                                     # lsm2d_preprocess_scans
    grew("preprocess_scans")
    grids = api.GridSet(ctx, api.GridGeometry(-8.0, -8.0, 0.25, 64, 48), 2)
    grew("grid set")
    # ---- every derived structure once
    nn = _aligner(ctx, api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.5))
    kd = _aligner(ctx, api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.5, search="kdtree"))
    nn.compute_batch([scans], [m2000], x2)
    grew("NN grid")
    _aligner(ctx, api.CorrespondenceFinderNN2D(ctx, max_distance_m=0.5)).compute_batch([scans], [m2000], x2)
    grew("distance map")
    kd.compute_batch([scans], [m2000], x2)
    grew("KD-tree, scan form")
    kd.compute_batch([one1281], [m2000], x2)
    grew("KD-tree, level loop + working set")
    projective = _aligner(ctx, api.CorrespondenceFinderProjective2f(ctx, proj))
    projective.compute_batch([scans], [m2000], x2)
    grew("lane layout, block bounds")
    ctx.set_option("align_path", 1)      # (a batch this small takes the slice-pair kernel by default, which gathers from the split arrays: the AoS rows are k_align's)
    projective.compute_batch([scans], [m2000], x2)
    grew("AoS rows")
    projective.compute_batch([prep], [m2000], x2)
    grew("AoS rows of the scans' set")
    before = live()
    pre.refill(prep)                                                                         # ... which the refill keeps and its launch rewrites
    projective.compute_batch([prep], [m2000], x2)
    pre.refill(prep)
    projective.compute_batch([prep], [m2000], x2)
    # (what lsm2d_preprocess_scans_refill acquires on its first call from pageable memory: the set's device copy of the ranges, the set's pinned staging
    # buffer, the context's beam directions of this sensor -- and on the second call nothing; the AoS rows are neither dropped nor made again)
    assert live() == before + 3, (before, live())
    ctx.set_option("align_path", 0)
    nn.compute_batch([scans], [m4200], x2)
    grew("tile bounds")
    # ---- the drop and the KD recycle of a reserved set: two uploads between two KD aligner calls, across both forms of the build
    reserved.upload(c[700])
    kd.compute_batch([reserved], [m2000], x1)
    grew("KD-tree of the reserved set")
    before = live()
    reserved.upload(c[1500]); reserved.upload(c[1500])
    kd.compute_batch([reserved], [m2000], x1)          # (more than 1280 points: the level loop takes the kept block)
    reserved.upload(c[600]); reserved.upload(c[600])
    kd.compute_batch([reserved], [m2000], x1)          # (the scan form takes it back)
    assert live() == before, "a recycled KD-tree block is neither lost nor doubled"
    # ---- two refused calls, half-way
    with pytest.raises(_capi.Lsm2dError) as e:
        reserved.upload(np.zeros((3000, 4), np.float32))
    assert e.value.code == _capi.CAPACITY_EXCEEDED
    with pytest.raises(_capi.Lsm2dError) as e:
        _aligner(ctx, api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(0, -np.pi, np.pi, 0.3, 30.0))).compute_batch([scans], [m2000], x2)
    assert e.value.code == _capi.BAD_ARGUMENT
    assert live() == before
    # ---- one batch begun asynchronously and waited for
    pb = projective.prepare_batch([scans], [m2000], x2)
    pb.begin()
    assert (pb.wait().status >= 0).all()
    seen.append(live())
    assert min(seen[1:]) > seen[0], seen
    # ---- half the sets, the context, the other half (the orphans)
    for s in (scans, m4200, many, grids):
        s.close()
    assert seen[0] < live() < seen[-1]
    ctx._lib.lsm2d_destroy(ctx.handle); ctx._h = None      # (not Context.close(), which would destroy the sets first)
    assert live() > seen[0], "the orphans still hold their buffers"
    for s in (m2000, one1281, reserved, prep):
        s.close()
    seen.append(live())
    return seen


def test_handles_balance_over_a_contexts_life_and_its_orphans():
    c = _clouds()
    gc.collect()      # (sets that earlier tests left to the collector go now, not half-way through the count)
    observer = api.Context(0)
    try:
        h0 = observer.get_option("live_handles")
        assert h0 > 0      # the observer's own events and staging
        v = C.c_int64(7)
        assert observer._lib.lsm2d_set_option(observer.handle, b"live_handles", 0) == _capi.BAD_ARGUMENT      # read-only
        first = _sequence(observer, c, "first")
        assert first[0] == h0 and first[-1] == h0, first
        second = _sequence(observer, c, "second")
        assert second[0] == h0 and second[-1] == h0, second
        assert observer._lib.lsm2d_get_option(observer.handle, b"live_handles", C.byref(v)) == 0 and v.value == h0
    finally:
        observer.close()
