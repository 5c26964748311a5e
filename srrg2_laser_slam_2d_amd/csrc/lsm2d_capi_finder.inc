// lsm2d_capi_finder.inc -- plugin interface #1 (CorrespondenceFinder_::compute for the four finder kinds), the factor over a correspondence vector, and both
// for a whole batch: apart (lsm2d_find_correspondences_batch, lsm2d_linearize_batch) and with the pairs kept on the device (lsm2d_score_batch; for a whole
// aligner: lsm2d_score_aligner_batch; the select calls that rank those rows on the device are in lsm2d_capi_select.inc, behind this part).  The steps these entry points share are stated once, up front: what a refusal says (failf), the cloud sets settled (settle_sets),
// the timing bracket round a call's launches (TimedLaunch), a batch's head checks and index rules (batch_head, resolve_items), how many items a launch
// takes (items_per_launch) and what a result row of the factor means (lin_row_out).  Where a call's parts lie in the lane's buffers is a *Layout struct.
// Part of lsm2d_capi.hip (included there); not a translation unit of its own.
#include <stdarg.h>

// ---- the shared steps ------------------------------------------------------------------------------------------------------
static int failf(lsm2d_context* ctx, int code, const char* fmt, ...) {
  char msg[200];
  va_list ap; va_start(ap, fmt); vsnprintf(msg, sizeof msg, fmt, ap); va_end(ap);
  return fail(ctx, code, msg);
}

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t) 255; }

// sizes only the device knows and pending unpacking / preprocessing, settled for both sets of a call before their sizes are read or a kernel reads them
static int settle_sets(const lsm2d_cloudset* fixed, const lsm2d_cloudset* moving) {
  int rc = resolve_count(fixed); if (rc) return rc;
  rc = resolve_count(moving); if (rc) return rc;
  rc = flush_pending(fixed); if (rc) return rc;
  return flush_pending(moving);
}

// The bracket round the launches lsm2d_last_kernel_ms answers for: with `timed` ("kernel_timing") the lane's two events are recorded on the stream in front
// of and behind them; end() is also where a launch that failed surfaces, and it points lsm2d_last_kernel_ms at this lane (note_timed).
struct TimedLaunch {
  lsm2d_context* ctx; Lane& L; hipStream_t stream; bool timed;
  TimedLaunch(lsm2d_context* c, Lane& lane_, hipStream_t s) : ctx(c), L(lane_), stream(s), timed(c->kernel_timing) {}
  hipError_t begin() const { return timed ? hipEventRecord(L.ev0, stream) : hipSuccess; }
  hipError_t end() const {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && timed) e = hipEventRecord(L.ev1, stream);
    if (e == hipSuccess) note_timed(ctx, timed);
    return e;
  }
};

// What every batch entry point checks before it looks at n_items: the arguments' shape (pair_capacity: 0 where the call has none), sets of this context,
// a lane to stage through.  `who` heads the messages.
static int batch_head(lsm2d_context* ctx, const char* who, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const lsm2d_cloudset* moving,
                      int32_t n_items, int32_t pair_capacity) {
  if (!ctx || !sp || !fixed || !moving || n_items < 0 || pair_capacity < 0) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: bad argument", who);
  if (fixed->ctx != ctx || moving->ctx != ctx) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: cloud set from another (or a destroyed) context", who);
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  return LSM2D_SUCCESS;
}

// Item i of a batch is between cloud fc[i] of `fixed` and cloud mc[i] of `moving`: the caller's index, or without one the set's only cloud or cloud i -- the
// set must then hold 1 or n_items clouds.  `name_item`: the message of an index out of range names the item (all callers but find_correspondences_batch,
// whose text is older than the habit and stays what callers may match on).
static int resolve_items(lsm2d_context* ctx, const char* who, bool name_item, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                         const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, std::vector<int32_t>& fc, std::vector<int32_t>& mc) {
  if (!fixed_index && fixed->n_clouds != 1 && fixed->n_clouds != n_items) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: fixed set must hold 1 or n_items clouds", who);
  if (!moving_index && moving->n_clouds != 1 && moving->n_clouds != n_items) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: moving set must hold 1 or n_items clouds", who);
  fc.resize((size_t) n_items); mc.resize((size_t) n_items);
  for (int32_t i = 0; i < n_items; ++i) {
    fc[(size_t) i] = fixed_index ? fixed_index[i] : (fixed->n_clouds == 1 ? 0 : i);
    mc[(size_t) i] = moving_index ? moving_index[i] : (moving->n_clouds == 1 ? 0 : i);
    if (valid_cloud_index(fixed, fc[(size_t) i]) && valid_cloud_index(moving, mc[(size_t) i])) continue;
    return name_item ? failf(ctx, LSM2D_BAD_ARGUMENT, "%s: item %d: cloud index out of range", who, (int) i) : failf(ctx, LSM2D_BAD_ARGUMENT, "%s: cloud index out of range", who);
  }
  return LSM2D_SUCCESS;
}

// The device room for the pairs of ONE launch of a batched pass, in pairs (8 bytes each: 16 MiB, and for the finder as much pinned staging behind it).  Every
// item counts with its whole slot -- pair_capacity, or the slice's largest possible vector -- whatever it finds or holds (the rule depends on the arguments'
// shape alone), so a launch takes kBatchPairBudget / slot items: at least one, at most max_items (kLinBatchMaxItems where an item table has to be bounded, n
// where nothing has), at most all n.  A batch beyond that runs as several launches over consecutive items -- same results.  1000 scans against a 1081-column
// canvas (8.6 MB) are one launch; point-query items of a 100 000-point moving cloud go 20 to a launch.
static constexpr size_t kBatchPairBudget = (size_t) 2 << 20;
static constexpr size_t kLinBatchMaxItems = (size_t) 1 << 16;
static size_t items_per_launch(size_t slot, size_t n, size_t max_items) {
  size_t per = kBatchPairBudget / (slot > 0 ? slot : 1);
  if (per > max_items) per = max_items;
  if (per < 1) per = 1;
  return per > n ? n : per;
}

// One result row of the factor as the ABI's H, b and statistics: the sums and counts are kAccumWords words at h; the digest of the pairs lies behind them (a
// row of kLinOutWords words, as the batch kernels write it) unless the caller says where else.
static void lin_row_out(const float* h, float* H, float* b, lsm2d_iteration_stats* s, const void* digest = nullptr) {
  H[0] = h[0]; H[1] = h[1]; H[2] = h[2]; H[3] = h[1]; H[4] = h[3]; H[5] = h[4]; H[6] = h[2]; H[7] = h[4]; H[8] = h[5];
  b[0] = h[6]; b[1] = h[7]; b[2] = h[8];
  if (s) {
    int32_t iv[3]; memcpy(iv, h + 11, sizeof iv);
    s->n_inliers = iv[0]; s->n_outliers = iv[1]; s->n_correspondences = iv[2]; s->chi_inliers = h[9]; s->chi_outliers = h[10];
    unsigned long long dg; memcpy(&dg, digest ? digest : h + kAccumWords, sizeof dg);
    s->pair_digest_lo = (uint32_t) dg; s->pair_digest_hi = (uint32_t) (dg >> 32);
  }
}

// ---- plugin interface #1 ---------------------------------------------------------------------------------
static bool is_point_query(int finder) { return finder == LSM2D_FINDER_NN || finder == LSM2D_FINDER_DISTMAP || finder == LSM2D_FINDER_KDTREE; }

// A point-query finder's reach checked and the fixed set's search structure built (or found) for it: it covers every cloud of the set.  `fixed_dev`: the
// set's device view, which gets the structure.  `who` heads the message for a reach that is not > 0.
static int prepare_point_query(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, CloudDev& fixed_dev, const char* who) {
  if (sp->finder != LSM2D_FINDER_DISTMAP && !(sp->max_distance > 0.0f)) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: max_distance must be > 0", who);
  return sp->finder == LSM2D_FINDER_DISTMAP ? ensure_distmap(ctx, fixed, sp->max_distance, sp->resolution, &fixed_dev.dist)
       : sp->finder == LSM2D_FINDER_KDTREE  ? ensure_kdtree(ctx, fixed, sp->kd_max_leaf_range, sp->kd_min_leaf_points, &fixed_dev.kd)
                                            : ensure_grid(ctx, fixed, sp->max_distance, &fixed_dev.grid);
}

// The single call's tail, whichever kernels ran: they have left [count | pad to 16 | pairs] in the lane's pinned staging buffer, or a copy there is queued.
static int find_finish(lsm2d_context* ctx, Lane& L, lsm2d_correspondence* out_pairs, int32_t capacity, int32_t* out_n) {
  HIPCHK(ctx, stream_sync(ctx));
  const int32_t n = *(const int32_t*) L.h_stage;
  *out_n = n;
  if (n > capacity) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "find_correspondences: out_pairs too small");
  memcpy(out_pairs, (char*) L.h_stage + 16, sizeof(lsm2d_correspondence) * (size_t) n);
  return LSM2D_SUCCESS;
}

// inl_tau > 0: only the pairs whose factor is an inlier under a Cauchy robustifier of that threshold (FindArgs::inl_tau)
static int find_correspondences_impl(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed,
                                     int32_t fi, const lsm2d_cloudset* moving, int32_t mi, const float pose[3],
                                     lsm2d_correspondence* out_pairs, int32_t capacity, int32_t* out_n, float inl_tau) {
  if (!ctx || !sp || !pose || !out_n || !valid_cloud_index(fixed, fi) || !valid_cloud_index(moving, mi) || capacity < 0 ||
      (capacity > 0 && !out_pairs))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences: bad argument");
  { const int rc0 = settle_sets(fixed, moving); if (rc0) return rc0; }
  *out_n = 0;
  if (is_point_query(sp->finder)) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FindNNArgs N;
    N.fixed = cloud_dev(fixed, nullptr); N.moving = cloud_dev(moving, nullptr); N.fc = fi; N.mc = mi;
    N.use_distmap = sp->finder == LSM2D_FINDER_DISTMAP; N.use_kd = sp->finder == LSM2D_FINDER_KDTREE;
    int rc = prepare_point_query(ctx, sp, fixed, N.fixed, "find_correspondences"); if (rc) return rc;
    const size_t nm = (size_t) moving->h_count[mi], bytes = nm * 8 + 16;
    N.max_distance = sp->max_distance; N.normal_cos = sp->normal_cos; N.T = make_iso(pose); N.inl_tau = inl_tau;
    N.nn_group = fixed->h_count[fi] >= 4 * (int64_t) moving->h_count[mi] ? kNNGroup : 1;     // dense fixed cloud: cooperative search
    // more queries than one workgroup takes in a trip: one workgroup per trip's worth, two launches (search, then ordered compaction)
    const int per_step = kFindBlock / ((N.use_distmap || N.use_kd) ? 1 : N.nn_group);
    const int n_blocks = (int) ((nm + (size_t) per_step - 1) / (size_t) per_step);
    const bool multi = n_blocks > 2 && ctx->find_path != 1;      // (two trips of one workgroup beat two launches: 23 vs 29 us for 1081 distance-map queries)
    const size_t o_match = up256(bytes), o_cnt = o_match + up256(nm * 4);      // behind [count | pairs]: the multi path's matches and per-block counts
    rc = ensure_scratch(ctx, multi ? o_cnt + 4 * (size_t) n_blocks : bytes); if (rc) return rc;
    rc = ensure_stage(ctx, bytes); if (rc) return rc;
    Lane& L = lane(ctx);
    const bool direct = bytes <= (1u << 16);             // up to 8k pairs: written straight to pinned host memory
    char* dv = (char*) (direct ? L.h_stage.dev() : L.d_scratch);
    N.out_count = (int32_t*) dv; N.out_pairs = (int32_t*) (dv + 16);
    N.match = (int32_t*) ((char*) L.d_scratch + o_match); N.block_count = (int32_t*) ((char*) L.d_scratch + o_cnt);
    const TimedLaunch timing(ctx, L, ctx->stream);
    HIPCHK(ctx, timing.begin());
    if (multi) {
      hipLaunchKernelGGL(k_find_nn_multi<0>, dim3((unsigned) n_blocks), dim3(kFindBlock), 0, ctx->stream, N);
      hipLaunchKernelGGL(k_find_nn_multi<1>, dim3((unsigned) n_blocks), dim3(kFindBlock), 0, ctx->stream, N);
    } else {
      hipLaunchKernelGGL(k_find_nn, dim3(1), dim3(kFindBlock), 0, ctx->stream, N);
    }
    HIPCHK(ctx, timing.end());
    if (!direct) HIPCHK(ctx, hipMemcpyAsync(L.h_stage, L.d_scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return find_finish(ctx, L, out_pairs, capacity, out_n);
  }
  if (sp->finder != LSM2D_FINDER_PROJECTIVE) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences: finder not supported yet");
  FindArgs A;
  if (!make_projk(sp->projector, &A.proj)) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences: bad projector");
  const size_t cols = (size_t) A.proj.cols, lds = sizeof(u64) * 2 * cols;
  if ((int) lds > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "find_correspondences: canvases do not fit LDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = cols * 8 + 16;
  // a map-sized cloud is z-buffered over many workgroups first (the clipper's large-scene kernel; u64 minima do not depend on the order)
  const bool big_f = fixed->h_count[fi] > 32768 && ctx->find_path != 1, big_m = moving->h_count[mi] > 32768 && ctx->find_path != 1;
  const size_t o_can = up256(bytes);      // behind [count | pairs]: the two canvases of the map-sized clouds
  int rc = ensure_scratch(ctx, o_can + 2 * cols * sizeof(u64)); if (rc) return rc;
  rc = ensure_stage(ctx, bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  A.fixed = cloud_dev(fixed, nullptr); A.moving = cloud_dev(moving, nullptr); A.fc = fi; A.mc = mi;
  A.point_distance = sp->point_distance; A.normal_cos = sp->normal_cos; A.T = make_iso(pose); A.inl_tau = inl_tau;
  char* dv = (char*) L.h_stage.dev();       // <= one pair per column: written straight to pinned host memory
  A.out_count = (int32_t*) dv; A.out_pairs = (int32_t*) (dv + 16);
  A.fcan_global = nullptr; A.mcan_global = nullptr;
  const TimedLaunch timing(ctx, L, ctx->stream);
  HIPCHK(ctx, timing.begin());
  if (big_f) {
    u64* g = (u64*) ((char*) L.d_scratch + o_can); const Iso ident = {1.0f, 0.0f, 0.0f, 0.0f};
    rc = project_split(ctx, fixed->d_xy + fixed->h_start[fi], fixed->h_count[fi], ident, A.proj, g); if (rc) return rc;
    A.fcan_global = g;
  }
  if (big_m) {
    u64* g = (u64*) ((char*) L.d_scratch + o_can) + cols;
    rc = project_split(ctx, moving->d_xy + moving->h_start[mi], moving->h_count[mi], A.T, A.proj, g); if (rc) return rc;
    A.mcan_global = g;
  }
  hipLaunchKernelGGL(k_find_projective, dim3(1), dim3(kFindBlock), lds, ctx->stream, A);
  HIPCHK(ctx, timing.end());
  return find_finish(ctx, L, out_pairs, capacity, out_n);
}

extern "C" int lsm2d_find_correspondences(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed,
                                          int32_t fi, const lsm2d_cloudset* moving, int32_t mi, const float pose[3],
                                          lsm2d_correspondence* out_pairs, int32_t capacity, int32_t* out_n) {
  return find_correspondences_impl(ctx, sp, fixed, fi, moving, mi, pose, out_pairs, capacity, out_n, 0.0f);
}

// ---- plugin interface #1 for a whole batch ------------------------------------------------------------------------
// The launch part of a batched finder pass, shared by lsm2d_find_correspondences_batch (find_batch_impl) and the scoring (score_batch_queue): what is the same
// for every item -- the sets' device views, the fixed set's search structure or the projector, the gates, the slot size -- and which kernel runs.
struct FindBatchLaunch {
  bool point_query = false;
  FindBatchArgs A; FindNNBatchArgs N;
  size_t lds = 0;
};

// The sets are settled once for the whole batch, the fixed set's search structure is built or found, the launch arguments but the three per-launch
// pointers are filled in.  `who` heads the messages.
static int find_batch_prepare(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const lsm2d_cloudset* moving, float inl_tau,
                              int32_t capacity, const char* who, FindBatchLaunch& P) {
  if (lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  { const int rc0 = settle_sets(fixed, moving); if (rc0) return rc0; }
  P.point_query = is_point_query(sp->finder);
  if (!P.point_query && sp->finder != LSM2D_FINDER_PROJECTIVE) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: finder not supported", who);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  FindBatchArgs& A = P.A; FindNNBatchArgs& N = P.N;
  if (P.point_query) {
    N.fixed = cloud_dev(fixed, nullptr); N.moving = cloud_dev(moving, nullptr);
    N.use_distmap = sp->finder == LSM2D_FINDER_DISTMAP; N.use_kd = sp->finder == LSM2D_FINDER_KDTREE;
    const int rc = prepare_point_query(ctx, sp, fixed, N.fixed, who); if (rc) return rc;
    N.max_distance = sp->max_distance; N.normal_cos = sp->normal_cos; N.inl_tau = inl_tau; N.pair_capacity = capacity;
  } else {
    if (!make_projk(sp->projector, &A.proj)) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: bad projector", who);
    P.lds = sizeof(u64) * 2 * (size_t) A.proj.cols;
    if ((int) P.lds > ctx->max_dyn_lds) return failf(ctx, LSM2D_CAPACITY_EXCEEDED, "%s: canvases do not fit LDS", who);
    A.fixed = cloud_dev(fixed, nullptr); A.moving = cloud_dev(moving, nullptr);
    A.point_distance = sp->point_distance; A.normal_cos = sp->normal_cos; A.inl_tau = inl_tau; A.pair_capacity = capacity;
  }
  return LSM2D_SUCCESS;
}

// the arguments of cnt items, item k = (cloud fc[k] of `fixed`, cloud mc[k] of `moving`, poses[k]), as the kernels read them
static void find_batch_fill_items(FindItem* items, const lsm2d_cloudset* fixed, const int32_t* fc, const lsm2d_cloudset* moving, const int32_t* mc,
                                  const float* poses, size_t cnt) {
  for (size_t k = 0; k < cnt; ++k) {
    FindItem& it = items[k];
    it.fc = fc[k]; it.mc = mc[k]; it.T = make_iso(poses + 3 * k); it.pad = 0;
    it.nn_group = fixed->h_count[it.fc] >= 4 * (int64_t) moving->h_count[it.mc] ? kNNGroup : 1;      // dense fixed cloud: cooperative search, item by item
  }
}

// one launch: a workgroup per item; item k's count goes to d_count[k], its pairs to slot k of d_pairs (all three device addresses)
static void find_batch_launch(lsm2d_context* ctx, FindBatchLaunch& P, const FindItem* d_items, size_t cnt, int32_t* d_count, int32_t* d_pairs) {
  if (P.point_query) {
    P.N.items = d_items; P.N.out_count = d_count; P.N.out_pairs = d_pairs;
    hipLaunchKernelGGL(k_find_nn_batch, dim3((unsigned) cnt), dim3(kFindBlock), 0, ctx->stream, P.N);
  } else {
    P.A.items = d_items; P.A.out_count = d_count; P.A.out_pairs = d_pairs;
    hipLaunchKernelGGL(k_find_projective_batch, dim3((unsigned) cnt), dim3(kFindBlock), P.lds, ctx->stream, P.A);
  }
}

// one layout for the lane's device scratch and its pinned staging: the items' arguments (up), then counts and pairs (down, ONE copy)
struct FindBatchLayout {
  size_t o_cnt, o_pairs, bytes;
  FindBatchLayout(size_t per_launch, size_t capacity) {
    o_cnt = up256(sizeof(FindItem) * per_launch); o_pairs = up256(o_cnt + sizeof(int32_t) * per_launch);
    bytes = o_pairs + sizeof(lsm2d_correspondence) * per_launch * capacity;
  }
};

// n items, item k = (cloud fc[k] of `fixed`, cloud mc[k] of `moving`, poses[k]); its pairs go to out_pairs + slot * pair_stride and its count to
// out_n + slot * count_stride, slot = slots ? slots[k] : k.  The callers have checked the pointers, the indices and the capacity rule.  Every launch
// (items_per_launch of a slot of `capacity` pairs) has its own wait.
static int find_batch_impl(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fc, const lsm2d_cloudset* moving,
                           const int32_t* mc, int32_t n_items, const float* poses, float inl_tau, lsm2d_correspondence* out_pairs, int32_t capacity,
                           int32_t* out_n, const int32_t* slots, size_t pair_stride, size_t count_stride) {
  FindBatchLaunch P;
  { const int rc = find_batch_prepare(ctx, sp, fixed, moving, inl_tau, capacity, "find_correspondences_batch", P); if (rc) return rc; }
  const size_t n = (size_t) n_items, per_launch = items_per_launch((size_t) capacity, n, n);
  const FindBatchLayout Y(per_launch, (size_t) capacity);
  { int rc = ensure_scratch(ctx, Y.bytes); if (rc) return rc; rc = ensure_stage(ctx, Y.bytes); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  const TimedLaunch timing(ctx, L, ctx->stream);
  for (size_t k0 = 0; k0 < n; k0 += per_launch) {
    const size_t cnt = std::min(per_launch, n - k0);
    find_batch_fill_items((FindItem*) hs, fixed, fc + k0, moving, mc + k0, poses + 3 * k0, cnt);
    HIPCHK(ctx, hipMemcpyAsync(ds, hs, sizeof(FindItem) * cnt, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, timing.begin());
    find_batch_launch(ctx, P, (const FindItem*) ds, cnt, (int32_t*) (ds + Y.o_cnt), (int32_t*) (ds + Y.o_pairs));
    HIPCHK(ctx, timing.end());
    const size_t down = Y.o_pairs - Y.o_cnt + sizeof(lsm2d_correspondence) * cnt * (size_t) capacity;
    HIPCHK(ctx, hipMemcpyAsync(hs + Y.o_cnt, ds + Y.o_cnt, down, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_sync(ctx));      // the one wait of this launch
    const int32_t* h_cnt = (const int32_t*) (hs + Y.o_cnt);
    for (size_t k = 0; k < cnt; ++k) {
      const size_t slot = slots ? (size_t) slots[k0 + k] : k0 + k;
      const int32_t np = h_cnt[k];
      if (np < 0 || np > capacity) return fail(ctx, LSM2D_DEVICE_ERROR, "find_correspondences_batch: an item reported more pairs than its slot holds");
      out_n[slot * count_stride] = np;
      if (np) memcpy(out_pairs + slot * pair_stride, hs + Y.o_pairs + sizeof(lsm2d_correspondence) * k * (size_t) capacity, sizeof(lsm2d_correspondence) * (size_t) np);
    }
  }
  return LSM2D_SUCCESS;
}

// a slice's largest possible correspondence vector: one pair per column, or per point of the largest moving cloud
static int find_batch_need(const lsm2d_slice_params* sp, const lsm2d_cloudset* moving, long long* need) {
  *need = 0;
  if (sp->finder == LSM2D_FINDER_PROJECTIVE) { *need = sp->projector.canvas_cols; return LSM2D_SUCCESS; }
  const int rc0 = resolve_count(moving); if (rc0) return rc0;
  *need = max_cloud_count(moving);
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_find_correspondences_batch(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                                const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses,
                                                lsm2d_correspondence* out_pairs, int32_t pair_capacity, int32_t* out_n_pairs) {
  static const char who[] = "find_correspondences_batch";
  { const int rc = batch_head(ctx, who, sp, fixed, moving, n_items, pair_capacity); if (rc) return rc; }
  if (n_items == 0) return LSM2D_SUCCESS;
  if (!poses || !out_n_pairs || (pair_capacity > 0 && !out_pairs)) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences_batch: null argument");
  std::vector<int32_t> fc, mc;
  { const int rc = resolve_items(ctx, who, false, fixed, fixed_index, moving, moving_index, n_items, fc, mc); if (rc) return rc; }
  long long need = 0;
  { const int rc0 = find_batch_need(sp, moving, &need); if (rc0) return rc0; }
  if (need > pair_capacity) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "find_correspondences_batch: pair_capacity below the largest possible correspondence vector");
  return find_batch_impl(ctx, sp, fixed, fc.data(), moving, mc.data(), n_items, poses, 0.0f, out_pairs, pair_capacity, out_n_pairs, nullptr, (size_t) pair_capacity, 1);
}

// ---- factor ---------------------------------------------------------------------------------------------------
// where the single call's parts lie, in the lane's pinned staging (a vector of up to 8k pairs: the kernels work there) or its device scratch
struct LinLayout {
  size_t pair_bytes, part_off, out_off, dig_off, bytes;
  LinLayout(size_t n_pairs, size_t blocks) {
    pair_bytes = sizeof(lsm2d_correspondence) * n_pairs;
    part_off = up256(pair_bytes); out_off = part_off + sizeof(float) * kAccumWords * blocks;
    dig_off = out_off + sizeof(float) * kAccumWords;      // 8-byte aligned: out_off is a multiple of 256, kAccumWords is even
    static_assert(kAccumWords % 2 == 0, "the digest behind the sums must be 8-byte aligned");
    bytes = dig_off + sizeof(unsigned long long);
  }
};

extern "C" int lsm2d_linearize(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, int32_t fi,
                               const lsm2d_cloudset* moving, int32_t mi, const lsm2d_correspondence* pairs, int32_t n_pairs,
                               const float pose[3], float out_H[9], float out_b[3], lsm2d_iteration_stats* st) {
  if (!ctx || !sp || !pose || !out_H || !out_b || !valid_cloud_index(fixed, fi) || !valid_cloud_index(moving, mi) || n_pairs < 0 ||
      (n_pairs > 0 && !pairs))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize: bad argument");
  { const int rc0 = settle_sets(fixed, moving); if (rc0) return rc0; }
  for (int32_t k = 0; k < n_pairs; ++k)
    if (pairs[k].fixed_idx < 0 || pairs[k].fixed_idx >= fixed->h_count[fi] || pairs[k].moving_idx < 0 || pairs[k].moving_idx >= moving->h_count[mi])
      return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize: correspondence index out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int blocks = (n_pairs + 255) / 256; if (blocks < 1) blocks = 1; if (blocks > 1024) blocks = 1024;
  const LinLayout Y((size_t) n_pairs, (size_t) blocks);
  int rc = ensure_scratch(ctx, Y.bytes); if (rc) return rc;
  rc = ensure_stage(ctx, Y.bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  if (n_pairs) memcpy(L.h_stage, pairs, Y.pair_bytes);
  // up to 8k pairs (a canvas worth): the kernels read the pairs from, and write the sums to, the pinned staging buffer directly
  const bool direct = n_pairs <= 8192;
  char* dv = (char*) (direct ? L.h_stage.dev() : L.d_scratch);
  if (!direct && n_pairs) HIPCHK(ctx, hipMemcpyAsync(L.d_scratch, L.h_stage, Y.pair_bytes, hipMemcpyHostToDevice, ctx->stream));
  LinArgs A;
  A.fixed = cloud_dev(fixed, nullptr); A.moving = cloud_dev(moving, nullptr); A.fc = fi; A.mc = mi;
  A.pairs = (const int32_t*) dv; A.n_pairs = n_pairs; A.T = make_iso(pose);
  A.cauchy = sp->robustifier == LSM2D_ROBUST_CAUCHY; A.tau = sp->chi_threshold;
  A.partial = (float*) ((char*) L.d_scratch + Y.part_off); A.out = (float*) (dv + Y.out_off);
  A.dig = (unsigned long long*) (dv + Y.dig_off);
  if (direct) *(unsigned long long*) ((char*) L.h_stage + Y.dig_off) = 0ull;
  else HIPCHK(ctx, hipMemsetAsync(A.dig, 0, sizeof(unsigned long long), ctx->stream));
  const TimedLaunch timing(ctx, L, ctx->stream);
  HIPCHK(ctx, timing.begin());
  if (ctx->sum_order) hipLaunchKernelGGL(k_linearize_seq, dim3(1), dim3(kAlignBlock), 0, ctx->stream, A);      // pair after pair, the order of the vector
  else {
    hipLaunchKernelGGL(k_linearize_partial, dim3(blocks), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_linearize_final, dim3(1), dim3(64), 0, ctx->stream, (const float*) A.partial, blocks, A.out);
  }
  HIPCHK(ctx, timing.end());
  float* h = (float*) ((char*) L.h_stage + Y.out_off);
  if (!direct) HIPCHK(ctx, hipMemcpyAsync(h, A.out, sizeof(float) * kAccumWords + sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  lin_row_out(h, out_H, out_b, st, (char*) L.h_stage + Y.dig_off);
  return LSM2D_SUCCESS;
}

// ---- factor for a whole batch ---------------------------------------------------------------------------------------
// A launch takes items_per_launch of a slot of pair_capacity pairs, at most kLinBatchMaxItems, and has its own wait.  Only the first n_pairs[i] entries of
// a row travel: they are packed one vector after the other on their way to the staging buffer.

// where the parts of a launch over cnt items (vector k of n_pairs[k] pairs) lie in the lane's device scratch and (the first three and the results) in its
// pinned staging
struct LinBatchLayout {
  size_t blocks = 0, npairs = 0;      // workgroups of the partial kernel and pairs, over the launch's items
  size_t o_wg, o_pairs, up_bytes, o_part, o_dig, o_out, d_bytes, h_out, h_bytes;
  LinBatchLayout(const int32_t* n_pairs, size_t cnt) {
    for (size_t k = 0; k < cnt; ++k) { blocks += (size_t) lin_blocks(n_pairs[k]); npairs += (size_t) n_pairs[k]; }
    o_wg = up256(sizeof(LinItem) * cnt); o_pairs = up256(o_wg + sizeof(int32_t) * blocks); up_bytes = o_pairs + sizeof(lsm2d_correspondence) * npairs;
    o_part = up256(up_bytes); o_dig = up256(o_part + sizeof(float) * kAccumWords * blocks); o_out = up256(o_dig + sizeof(unsigned long long) * cnt);
    d_bytes = o_out + sizeof(float) * kLinOutWords * cnt;
    h_out = up256(up_bytes); h_bytes = h_out + sizeof(float) * kLinOutWords * cnt;
  }
};

extern "C" int lsm2d_linearize_batch(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                     const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const lsm2d_correspondence* pairs,
                                     int32_t pair_capacity, const int32_t* n_pairs, const float* poses, float* out_H, float* out_b, lsm2d_iteration_stats* st) {
  static const char who[] = "linearize_batch";
  { const int rc = batch_head(ctx, who, sp, fixed, moving, n_items, pair_capacity); if (rc) return rc; }
  if (n_items == 0) return LSM2D_SUCCESS;
  if (!n_pairs || !poses || !out_H || !out_b) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: null argument");
  std::vector<int32_t> fc, mc;
  { const int rc = resolve_items(ctx, who, true, fixed, fixed_index, moving, moving_index, n_items, fc, mc); if (rc) return rc; }
  { const int rc0 = settle_sets(fixed, moving); if (rc0) return rc0; }      // once for the whole batch (the validation below needs the sizes)
  // every item is checked before anything is launched or written
  for (int32_t i = 0; i < n_items; ++i) {
    const int32_t np = n_pairs[i];
    if (np > 0 && !pairs) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: null argument");
    if (np < 0 || np > pair_capacity)
      return failf(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: item %d: n_pairs %d outside [0, pair_capacity %d]", (int) i, (int) np, (int) pair_capacity);
    const lsm2d_correspondence* row = np ? pairs + (size_t) i * (size_t) pair_capacity : nullptr;
    const int32_t nf = fixed->h_count[fc[(size_t) i]], nm = moving->h_count[mc[(size_t) i]];
    for (int32_t k = 0; k < np; ++k)
      if (row[k].fixed_idx < 0 || row[k].fixed_idx >= nf || row[k].moving_idx < 0 || row[k].moving_idx >= nm)
        return failf(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: item %d: correspondence %d (%d, %d) out of range", (int) i, (int) k, (int) row[k].fixed_idx, (int) row[k].moving_idx);
  }
  const size_t n = (size_t) n_items, per_launch = items_per_launch((size_t) pair_capacity, n, kLinBatchMaxItems);
  // the largest launch decides the buffers' sizes: they are grown (and waited for) once, ahead of the first launch
  size_t d_need = 0, h_need = 0;
  for (size_t k0 = 0; k0 < n; k0 += per_launch) {
    const LinBatchLayout Y(n_pairs + k0, std::min(per_launch, n - k0));
    d_need = std::max(d_need, Y.d_bytes); h_need = std::max(h_need, Y.h_bytes);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  { int rc = ensure_scratch(ctx, d_need); if (rc) return rc; rc = ensure_stage(ctx, h_need); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  const TimedLaunch timing(ctx, L, ctx->stream);
  LinBatchArgs A;
  A.fixed = cloud_dev(fixed, nullptr); A.moving = cloud_dev(moving, nullptr);
  A.cauchy = sp->robustifier == LSM2D_ROBUST_CAUCHY; A.tau = sp->chi_threshold;
  for (size_t k0 = 0; k0 < n; k0 += per_launch) {
    const size_t cnt = std::min(per_launch, n - k0);
    const LinBatchLayout Y(n_pairs + k0, cnt);
    LinItem* items = (LinItem*) hs; int32_t* wg = (int32_t*) (hs + Y.o_wg); char* hp = hs + Y.o_pairs;
    size_t b0 = 0, p0 = 0;
    for (size_t k = 0; k < cnt; ++k) {
      LinItem& it = items[k];
      it.fc = fc[k0 + k]; it.mc = mc[k0 + k]; it.n_pairs = n_pairs[k0 + k]; it.blocks = lin_blocks(it.n_pairs); it.T = make_iso(poses + 3 * (k0 + k));
      it.block_base = (int32_t) b0; it.pair_base = (int32_t) p0; it.pad0 = it.pad1 = 0;
      for (int b = 0; b < it.blocks; ++b) wg[b0 + (size_t) b] = (int32_t) k;
      if (it.n_pairs) memcpy(hp + sizeof(lsm2d_correspondence) * p0, pairs + (k0 + k) * (size_t) pair_capacity, sizeof(lsm2d_correspondence) * (size_t) it.n_pairs);
      b0 += (size_t) it.blocks; p0 += (size_t) it.n_pairs;
    }
    HIPCHK(ctx, hipMemcpyAsync(ds, hs, Y.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    A.items = (const LinItem*) ds; A.wg_item = (const int32_t*) (ds + Y.o_wg); A.pairs = (const int32_t*) (ds + Y.o_pairs); A.n_items = (int32_t) cnt;
    A.partial = (float*) (ds + Y.o_part); A.dig = (unsigned long long*) (ds + Y.o_dig); A.out = (float*) (ds + Y.o_out);
    if (!ctx->sum_order) HIPCHK(ctx, hipMemsetAsync(A.dig, 0, sizeof(unsigned long long) * cnt, ctx->stream));
    HIPCHK(ctx, timing.begin());
    if (ctx->sum_order) hipLaunchKernelGGL(k_linearize_seq_batch, dim3((unsigned) cnt), dim3(kAlignBlock), 0, ctx->stream, A);      // pair after pair, a workgroup per item
    else {
      hipLaunchKernelGGL(k_linearize_partial_batch, dim3((unsigned) Y.blocks), dim3(256), 0, ctx->stream, A);
      hipLaunchKernelGGL(k_linearize_final_batch, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, ctx->stream, A);
    }
    HIPCHK(ctx, timing.end());
    HIPCHK(ctx, hipMemcpyAsync(hs + Y.h_out, A.out, sizeof(float) * kLinOutWords * cnt, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_sync(ctx));      // the one wait of this launch
    for (size_t k = 0; k < cnt; ++k)
      lin_row_out((const float*) (hs + Y.h_out) + kLinOutWords * k, out_H + 9 * (k0 + k), out_b + 3 * (k0 + k), st ? st + (k0 + k) : nullptr);
  }
  return LSM2D_SUCCESS;
}

// ---- finder + factor for a whole batch: pose hypotheses scored on the device ------------------------------------------------------------------------
// The batch finder's kernels write every item's pairs into its slot of the lane's device scratch and its count next to them; the k_score_* kernels linearise
// them there.  A slot is the slice's largest possible vector (find_batch_need), and a launch group takes items_per_launch of it, at most kLinBatchMaxItems:
// the groups are queued one behind the other on the stream and reuse the same pair and partial-row scratch, while the items' arguments (uploaded once), their
// counts, digests and result rows are arrays over the whole batch.  One copy down and ONE wait, at the end.
// The scoring is shared by lsm2d_score_batch, which copies every row down, and lsm2d_score_select, which ranks the rows where they lie: after batch_head,
// their own pointers and an empty batch, score_batch_queue is everything from the index rules to the last launch group -- it leaves the rows on the device
// (ds + o_out), waits for nothing and has begun the timing bracket in front of the LAST group alone (finder and factor together); the caller ends it.

// device: [items | counts | digests | result rows] over the whole batch, then [pairs | partial rows] of one launch group, then d_extra bytes of the caller's;
// staging: the items' arguments (up), then h_down bytes of the caller's
// (up_extra: bytes of the caller's that ride up behind the items in the same copy -- the grouped selection's table; 0 for every other call)
struct ScoreLayout {
  size_t n = 0, o_up = 0, up_bytes = 0, o_cnt = 0, o_dig = 0, o_out = 0, o_pairs = 0, o_part = 0, o_extra = 0, d_bytes = 0, h_out = 0, h_bytes = 0;
  ScoreLayout() = default;
  ScoreLayout(size_t n_, size_t per_group, size_t slot, size_t blocks_per_item, size_t d_extra, size_t h_down, size_t up_extra = 0) : n(n_) {
    o_up = up256(sizeof(FindItem) * n); up_bytes = up_extra ? o_up + up_extra : sizeof(FindItem) * n;
    o_cnt = up256(o_up + up_extra); o_dig = up256(o_cnt + sizeof(int32_t) * n); o_out = up256(o_dig + sizeof(unsigned long long) * n);
    o_pairs = up256(o_out + sizeof(float) * kLinOutWords * n); o_part = up256(o_pairs + sizeof(lsm2d_correspondence) * per_group * slot);
    o_extra = up256(o_part + sizeof(float) * kAccumWords * per_group * blocks_per_item); d_bytes = o_extra + d_extra;
    h_out = up256(o_up + up_extra); h_bytes = h_out + h_down;
  }
};

// Where one slice's arrays over the whole batch and the launch groups' shared scratch lie (device addresses), and the salt of its pairs' digest: what
// lsm2d_score_batch's one slice (salt 0) and every slice of lsm2d_score_aligner_batch (slice * 0x632BE5AB, each at its own base in the scratch) hand to
// the launch groups.
struct ScoreSliceDev {
  const FindItem* items; int32_t* cnt; unsigned long long* dig; float* out;      // [n] each, rows of kLinOutWords
  int32_t* pairs; float* partial;                                                 // of ONE launch group
  uint32_t salt;
};

// The launch groups of one slice over n items, per_group items each (every item a slot of `slot` pairs), queued one behind the other: finder, then factor.
// `timed`: the timing bracket is begun in front of the last group.  Waits for nothing.
static int score_slice_queue(lsm2d_context* ctx, FindBatchLaunch& P, const lsm2d_slice_params* sp, size_t n, size_t per_group, int32_t slot,
                             const ScoreSliceDev& D, bool timed) {
  Lane& L = lane(ctx);
  const size_t B = (size_t) lin_blocks(slot);
  ScoreBatchArgs S;
  S.fixed = P.point_query ? P.N.fixed : P.A.fixed; S.moving = P.point_query ? P.N.moving : P.A.moving;
  S.slot = slot; S.blocks_per_item = (int32_t) B; S.cauchy = sp->robustifier == LSM2D_ROBUST_CAUCHY; S.tau = sp->chi_threshold; S.slice_salt = D.salt;
  S.pairs = D.pairs; S.partial = D.partial;
  for (size_t k0 = 0; k0 < n; k0 += per_group) {
    const size_t cnt = std::min(per_group, n - k0);
    S.items = D.items + k0; S.count = D.cnt + k0; S.n_items = (int32_t) cnt;
    S.dig = D.dig + k0; S.out = D.out + kLinOutWords * k0;
    if (timed && k0 + cnt == n) HIPCHK(ctx, TimedLaunch(ctx, L, ctx->stream).begin());      // the last launch group
    find_batch_launch(ctx, P, S.items, cnt, D.cnt + k0, D.pairs);
    if (ctx->sum_order) hipLaunchKernelGGL(k_score_seq_batch, dim3((unsigned) cnt), dim3(kAlignBlock), 0, ctx->stream, S);      // pair after pair, a workgroup per item
    else {
      hipLaunchKernelGGL(k_score_partial_batch, dim3((unsigned) (cnt * B)), dim3(256), 0, ctx->stream, S);
      hipLaunchKernelGGL(k_score_final_batch, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, ctx->stream, S);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  return LSM2D_SUCCESS;
}

static int score_batch_queue(lsm2d_context* ctx, const char* who, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                             const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses, size_t d_extra, size_t h_down,
                             ScoreLayout& Y, const void* up_extra = nullptr, size_t up_extra_bytes = 0) {
  std::vector<int32_t> fc, mc;
  { const int rc = resolve_items(ctx, who, true, fixed, fixed_index, moving, moving_index, n_items, fc, mc); if (rc) return rc; }
  long long need = 0;
  { const int rc0 = find_batch_need(sp, moving, &need); if (rc0) return rc0; }
  if (need < 0 || need > 0x7fffffffll) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: bad projector", who);
  const int32_t slot = (int32_t) need;
  FindBatchLaunch P;
  { const int rc = find_batch_prepare(ctx, sp, fixed, moving, 0.0f, slot, who, P); if (rc) return rc; }
  const size_t n = (size_t) n_items, per_group = items_per_launch((size_t) slot, n, kLinBatchMaxItems), B = (size_t) lin_blocks(slot);
  Y = ScoreLayout(n, per_group, (size_t) slot, B, d_extra, h_down, up_extra_bytes);
  { int rc = ensure_scratch(ctx, Y.d_bytes); if (rc) return rc; rc = ensure_stage(ctx, Y.h_bytes); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  find_batch_fill_items((FindItem*) hs, fixed, fc.data(), moving, mc.data(), poses, n);
  if (up_extra_bytes) memcpy(hs + Y.o_up, up_extra, up_extra_bytes);
  HIPCHK(ctx, hipMemcpyAsync(ds, hs, Y.up_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (!ctx->sum_order) HIPCHK(ctx, hipMemsetAsync(ds + Y.o_dig, 0, sizeof(unsigned long long) * n, ctx->stream));
  const ScoreSliceDev D = {(const FindItem*) ds, (int32_t*) (ds + Y.o_cnt), (unsigned long long*) (ds + Y.o_dig), (float*) (ds + Y.o_out),
                           (int32_t*) (ds + Y.o_pairs), (float*) (ds + Y.o_part), 0u};
  return score_slice_queue(ctx, P, sp, n, per_group, slot, D, true);
}

extern "C" int lsm2d_score_batch(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                 const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses, float* out_H, float* out_b,
                                 lsm2d_iteration_stats* st) {
  { const int rc = batch_head(ctx, "score_batch", sp, fixed, moving, n_items, 0); if (rc) return rc; }
  if (n_items == 0) return LSM2D_SUCCESS;
  if (!poses || !out_H || !out_b) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_batch: null argument");
  ScoreLayout Y;
  { const int rc = score_batch_queue(ctx, "score_batch", sp, fixed, fixed_index, moving, moving_index, n_items, poses, 0, sizeof(float) * kLinOutWords * (size_t) n_items, Y); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  HIPCHK(ctx, TimedLaunch(ctx, L, ctx->stream).end());
  HIPCHK(ctx, hipMemcpyAsync(hs + Y.h_out, ds + Y.o_out, sizeof(float) * kLinOutWords * Y.n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  for (size_t k = 0; k < Y.n; ++k) lin_row_out((const float*) (hs + Y.h_out) + kLinOutWords * k, out_H + 9 * k, out_b + 3 * k, st ? st + k : nullptr);
  return LSM2D_SUCCESS;
}

// ---- hypotheses scored against an ALIGNER: all its slices, sensor offsets, the skip rule, the prior (lsm2d_k_score_aligner.h) ---------------------------------
// Up, once: poses, priors (as PriorDev, the aligner's own host-side form) and the per-slice index tables.  k_score_aligner_items turns them into every
// slice's FindItem table on the device; then slice after slice runs lsm2d_score_batch's launch groups (score_slice_queue) on its OWN items, counts, digests
// and rows, with its slice's salt, all slices sharing the pair and partial-row scratch of one launch group -- sized by the largest slot among them, which
// also decides the groups; k_score_combine leaves one combined row per item.  The timing bracket is begun in front of the last group of the last slice.

// device: [poses | priors | fixed index | moving index] (the upload), then per slice [items | counts | digests | rows] over the whole batch, the combined
// rows, [pairs | partial rows] of one launch group, d_extra bytes of the caller's; staging: the upload, then h_down bytes of the caller's
struct ScoreAlignerLayout {
  size_t n = 0, ns = 0, o_prior = 0, o_fidx = 0, o_midx = 0, up_bytes = 0, o_items = 0, o_cnt = 0, o_dig = 0, o_out = 0, o_comb = 0, o_pairs = 0, o_part = 0,
         o_extra = 0, d_bytes = 0, h_out = 0, h_bytes = 0;
  ScoreAlignerLayout() = default;
  size_t o_up_extra = 0;      // (up_extra bytes of the caller's behind the upload, in the same copy: the grouped selection's table; 0 for every other call)
  ScoreAlignerLayout(size_t n_, size_t ns_, bool prior, bool fidx, bool midx, size_t per_group, size_t slot_max, size_t d_extra, size_t h_down,
                     size_t up_extra = 0) : n(n_), ns(ns_) {
    o_prior = up256(sizeof(float) * 3 * n); o_fidx = up256(o_prior + (prior ? sizeof(PriorDev) * n : 0));
    o_midx = up256(o_fidx + (fidx ? sizeof(int32_t) * ns * n : 0)); up_bytes = o_midx + (midx ? sizeof(int32_t) * ns * n : 0);
    if (up_extra) { o_up_extra = up256(up_bytes); up_bytes = o_up_extra + up_extra; }
    o_items = up256(up_bytes); o_cnt = up256(o_items + sizeof(FindItem) * ns * n); o_dig = up256(o_cnt + sizeof(int32_t) * ns * n);
    o_out = up256(o_dig + sizeof(unsigned long long) * ns * n); o_comb = up256(o_out + sizeof(float) * kLinOutWords * ns * n);
    o_pairs = up256(o_comb + sizeof(float) * kCombWords * n); o_part = up256(o_pairs + sizeof(lsm2d_correspondence) * per_group * slot_max);
    o_extra = up256(o_part + sizeof(float) * kAccumWords * per_group * (size_t) lin_blocks((int) slot_max)); d_bytes = o_extra + d_extra;
    h_out = up256(up_bytes); h_bytes = h_out + h_down;
  }
};

// one combined row as the ABI's H, b, statistics and active count
static void comb_row_out(const float* h, float* H, float* b, lsm2d_iteration_stats* s, int32_t* active) {
  if (H) memcpy(H, h, sizeof(float) * 9);
  if (b) memcpy(b, h + kCombB, sizeof(float) * 3);
  int32_t iv[4]; memcpy(iv, h + CombRow::kNin, sizeof iv);      // n_inliers, n_outliers, n_correspondences, active
  if (s) {
    s->n_inliers = iv[0]; s->n_outliers = iv[1]; s->n_correspondences = iv[2]; s->chi_inliers = h[CombRow::kChi]; s->chi_outliers = h[kCombChiOut];
    unsigned long long dg; memcpy(&dg, h + kCombDigest, sizeof dg);
    s->pair_digest_lo = (uint32_t) dg; s->pair_digest_hi = (uint32_t) (dg >> 32);
  }
  if (active) *active = iv[3];
}

// the descriptor's shape, the sets, a lane to stage through: what is checked before n_alignments is looked at
static int score_aligner_head(lsm2d_context* ctx, const char* who, const lsm2d_batch* b) {
  if (!ctx || !b || b->n_alignments < 0 || b->n_slices < 1 || b->n_slices > kMaxSlices || !b->slices || !b->fixed || !b->moving)
    return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: bad batch descriptor (1 .. %d slices)", who, kMaxSlices);
  for (int s = 0; s < b->n_slices; ++s) { const int rc = batch_head(ctx, who, b->slices + s, b->fixed[s], b->moving[s], b->n_alignments, 0); if (rc) return rc; }
  return LSM2D_SUCCESS;
}

// every refusal of score_aligner_queue, which makes them first: the index rules per slice, then what the slices' finders need (lsm2d_relocalize_select makes
// them ahead of its second stage's preparation as well)
static int score_aligner_refusals(lsm2d_context* ctx, const char* who, const lsm2d_batch* b) {
  const int ns = b->n_slices; const int32_t n_items = b->n_alignments; const size_t n = (size_t) n_items;
  if (!b->init_pose) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: null argument", who);
  for (int s = 0; s < ns; ++s) {
    const lsm2d_cloudset* f = b->fixed[s]; const lsm2d_cloudset* m = b->moving[s];
    const int32_t* fi = b->fixed_index ? b->fixed_index + (size_t) s * n : nullptr; const int32_t* mi = b->moving_index ? b->moving_index + (size_t) s * n : nullptr;
    if (!fi && f->n_clouds != 1 && f->n_clouds != n_items) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: slice %d: fixed set must hold 1 or n_alignments clouds", who, s);
    if (!mi && m->n_clouds != 1 && m->n_clouds != n_items) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: slice %d: moving set must hold 1 or n_alignments clouds", who, s);
    for (int32_t i = 0; i < n_items; ++i) {
      const int32_t fc = fi ? fi[i] : (f->n_clouds == 1 ? 0 : i), mc = mi ? mi[i] : (m->n_clouds == 1 ? 0 : i);
      if (!valid_cloud_index(f, fc) || !valid_cloud_index(m, mc)) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: item %d, slice %d: cloud index out of range", who, (int) i, s);
    }
  }
  for (int s = 0; s < ns; ++s) {
    const lsm2d_slice_params& sp = b->slices[s];
    if (is_point_query(sp.finder)) { if (sp.finder != LSM2D_FINDER_DISTMAP && !(sp.max_distance > 0.0f)) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: max_distance must be > 0", who); continue; }
    if (sp.finder != LSM2D_FINDER_PROJECTIVE) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: finder not supported", who);
    ProjK pk;
    if (!make_projk(sp.projector, &pk)) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: bad projector", who);
    if ((long long) (sizeof(u64) * 2) * (long long) pk.cols > (long long) ctx->max_dyn_lds) return failf(ctx, LSM2D_CAPACITY_EXCEEDED, "%s: canvases do not fit LDS", who);
  }
  return LSM2D_SUCCESS;
}

// Everything from the index rules to k_score_combine: leaves the combined rows on the device (ds + Y.o_comb), waits for nothing, has begun the timing
// bracket; the caller ends it.  n_alignments > 0 and score_aligner_head have been checked.
// (chained: lsm2d_relocalize_select's stage 1 -- the caller has made the refusals already, an O(n_slices x n) pass over the index tables that is not made
// twice, and has begun a timing bracket of its own in front of the call, which runs to its final selection)
// (dev: lsm2d_score_grid_select's levels -- the poses were made ON THE DEVICE, at dev->o_poses inside the caller's d_extra region, and so were the constant
// index tables where the descriptor says there are any: nothing is staged or copied up, no pass is made over the items, b->init_pose is not read.  The
// layout is the one of dev->n_cap items whatever this level's n is, so every level of the call asks for the same scratch and finds every array in the same
// place; always chained)
struct ScoreDevicePoses { size_t n_cap, o_poses; };
static int score_aligner_queue(lsm2d_context* ctx, const char* who, const lsm2d_batch* b, size_t d_extra, size_t h_down, ScoreAlignerLayout& Y,
                               const void* up_extra = nullptr, size_t up_extra_bytes = 0, bool chained = false, const ScoreDevicePoses* dev = nullptr) {
  const int ns = b->n_slices; const int32_t n_items = b->n_alignments; const size_t n = (size_t) n_items;
  const size_t n_lay = dev ? dev->n_cap : n;      // the arrays' stride per slice
  if (!chained) { const int rc = score_aligner_refusals(ctx, who, b); if (rc) return rc; }
  FindBatchLaunch P[kMaxSlices]; int32_t slot[kMaxSlices]; int32_t slot_max = 1;
  for (int s = 0; s < ns; ++s) {
    long long need = 0;
    { const int rc0 = find_batch_need(b->slices + s, b->moving[s], &need); if (rc0) return rc0; }
    if (need < 0 || need > 0x7fffffffll) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: bad projector", who);
    slot[s] = (int32_t) need; slot_max = std::max(slot_max, slot[s]);
    { const int rc = find_batch_prepare(ctx, b->slices + s, b->fixed[s], b->moving[s], 0.0f, slot[s], who, P[s]); if (rc) return rc; }
  }
  const size_t per_group = items_per_launch((size_t) slot_max, n, kLinBatchMaxItems);
  Y = ScoreAlignerLayout(n_lay, (size_t) ns, b->prior != nullptr, b->fixed_index != nullptr, b->moving_index != nullptr,
                         dev ? items_per_launch((size_t) slot_max, n_lay, kLinBatchMaxItems) : per_group, (size_t) slot_max, d_extra, h_down, up_extra_bytes);
  { int rc = ensure_scratch(ctx, Y.d_bytes); if (rc) return rc; rc = ensure_stage(ctx, Y.h_bytes); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  if (!dev) {
    memcpy(hs, b->init_pose, sizeof(float) * 3 * n);
    if (up_extra_bytes) memcpy(hs + Y.o_up_extra, up_extra, up_extra_bytes);
    if (b->prior) {
      PriorDev* p = (PriorDev*) (hs + Y.o_prior);
      for (size_t i = 0; i < n; ++i) {      // as the aligner stages them (AlignBatch::stage_inputs)
        inverse_host(b->prior[i].z, p[i].z_inv); sincos_fixed(p[i].z_inv[2], p[i].sz, p[i].cz);
        memcpy(p[i].omega, b->prior[i].omega, sizeof(float) * 9);
      }
    }
    if (b->fixed_index) memcpy(hs + Y.o_fidx, b->fixed_index, sizeof(int32_t) * (size_t) ns * n);
    if (b->moving_index) memcpy(hs + Y.o_midx, b->moving_index, sizeof(int32_t) * (size_t) ns * n);
    HIPCHK(ctx, hipMemcpyAsync(ds, hs, Y.up_bytes, hipMemcpyHostToDevice, ctx->stream));      // the one copy up
  }
  if (!ctx->sum_order) HIPCHK(ctx, hipMemsetAsync(ds + Y.o_dig, 0, sizeof(unsigned long long) * (size_t) ns * n_lay, ctx->stream));
  ScoreAlignerArgs A;
  A.poses = dev ? (const float*) (ds + Y.o_extra + dev->o_poses) : (const float*) ds; A.prior = b->prior ? (const PriorDev*) (ds + Y.o_prior) : nullptr; A.n_items = n_items; A.n_slices = ns;
  A.out = (float*) (ds + Y.o_comb);
  ScoreSliceDev D[kMaxSlices];
  for (int s = 0; s < kMaxSlices; ++s) {
    ScoreAlignerSlice& S = A.s[s];
    memset(&S, 0, sizeof S);
    if (s >= ns) continue;
    const lsm2d_slice_params& sp = b->slices[s];
    S.f_count = b->fixed[s]->d_count; S.m_count = b->moving[s]->d_count;
    S.f_index = b->fixed_index ? (const int32_t*) (ds + Y.o_fidx) + (size_t) s * n_lay : nullptr;
    S.m_index = b->moving_index ? (const int32_t*) (ds + Y.o_midx) + (size_t) s * n_lay : nullptr;
    S.f_clouds = b->fixed[s]->n_clouds; S.m_clouds = b->moving[s]->n_clouds;
    S.has_sensor = !(sp.sensor_in_robot[0] == 0.0f && sp.sensor_in_robot[1] == 0.0f && sp.sensor_in_robot[2] == 0.0f);      // the aligner's test (fill_align_args)
    inverse_host(sp.sensor_in_robot, S.Sinv); sincos_fixed(S.Sinv[2], S.sSinv, S.cSinv);
    S.items = (FindItem*) (ds + Y.o_items) + (size_t) s * n_lay;
    S.count = (const int32_t*) (ds + Y.o_cnt) + (size_t) s * n_lay; S.rows = (const float*) (ds + Y.o_out) + kLinOutWords * (size_t) s * n_lay;
    S.slot = slot[s]; S.min_corr = sp.min_num_correspondences;
    D[s] = ScoreSliceDev{S.items, (int32_t*) (ds + Y.o_cnt) + (size_t) s * n_lay, (unsigned long long*) (ds + Y.o_dig) + (size_t) s * n_lay,
                         (float*) (ds + Y.o_out) + kLinOutWords * (size_t) s * n_lay, (int32_t*) (ds + Y.o_pairs), (float*) (ds + Y.o_part), (uint32_t) s * 0x632BE5ABu};
  }
  hipLaunchKernelGGL(k_score_aligner_items, dim3((unsigned) ((n + 255) / 256), (unsigned) ns), dim3(256), 0, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  for (int s = 0; s < ns; ++s) { const int rc = score_slice_queue(ctx, P[s], b->slices + s, n, per_group, slot[s], D[s], !chained && s == ns - 1); if (rc) return rc; }
  hipLaunchKernelGGL(k_score_combine, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_score_aligner_batch(lsm2d_context* ctx, const lsm2d_batch* batch, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats,
                                         int32_t* out_active) {
  static const char who[] = "score_aligner_batch";
  { const int rc = score_aligner_head(ctx, who, batch); if (rc) return rc; }
  if (batch->n_alignments == 0) return LSM2D_SUCCESS;
  if (!out_H || !out_b) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_aligner_batch: null argument");
  ScoreAlignerLayout Y;
  { const int rc = score_aligner_queue(ctx, who, batch, 0, sizeof(float) * kCombWords * (size_t) batch->n_alignments, Y); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  HIPCHK(ctx, TimedLaunch(ctx, L, ctx->stream).end());
  HIPCHK(ctx, hipMemcpyAsync(hs + Y.h_out, ds + Y.o_comb, sizeof(float) * kCombWords * Y.n, hipMemcpyDeviceToHost, ctx->stream));      // the one copy down
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  for (size_t k = 0; k < Y.n; ++k)
    comb_row_out((const float*) (hs + Y.h_out) + kCombWords * k, out_H + 9 * k, out_b + 3 * k, out_stats ? out_stats + k : nullptr, out_active ? out_active + k : nullptr);
  return LSM2D_SUCCESS;
}
