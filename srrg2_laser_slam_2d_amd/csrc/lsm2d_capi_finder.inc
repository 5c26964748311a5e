// lsm2d_capi_finder.inc -- plugin interface #1 (CorrespondenceFinder_::compute for the four finder kinds) and the factor over a correspondence vector.
// Part of lsm2d_capi.hip (included there); not a translation unit of its own.
// ---- plugin interface #1 ---------------------------------------------------------------------------------
static bool is_point_query(int finder) { return finder == LSM2D_FINDER_NN || finder == LSM2D_FINDER_DISTMAP || finder == LSM2D_FINDER_KDTREE; }

// A point-query finder's reach checked and the fixed set's search structure built (or found) for it: it covers every cloud of the set.  `fixed_dev`: the
// set's device view, which gets the structure.  `bad_distance`: the caller's message for a reach that is not > 0.
static int prepare_point_query(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, CloudDev& fixed_dev, const char* bad_distance) {
  if (sp->finder != LSM2D_FINDER_DISTMAP && !(sp->max_distance > 0.0f)) return fail(ctx, LSM2D_BAD_ARGUMENT, bad_distance);
  return sp->finder == LSM2D_FINDER_DISTMAP ? ensure_distmap(ctx, fixed, sp->max_distance, sp->resolution, &fixed_dev.dist)
       : sp->finder == LSM2D_FINDER_KDTREE  ? ensure_kdtree(ctx, fixed, sp->kd_max_leaf_range, sp->kd_min_leaf_points, &fixed_dev.kd)
                                            : ensure_grid(ctx, fixed, sp->max_distance, &fixed_dev.grid);
}

// inl_tau > 0: only the pairs whose factor is an inlier under a Cauchy robustifier of that threshold (FindArgs::inl_tau)
static int find_correspondences_impl(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed,
                                     int32_t fi, const lsm2d_cloudset* moving, int32_t mi, const float pose[3],
                                     lsm2d_correspondence* out_pairs, int32_t capacity, int32_t* out_n, float inl_tau) {
  if (!ctx || !sp || !pose || !out_n || !valid_cloud_index(fixed, fi) || !valid_cloud_index(moving, mi) || capacity < 0 ||
      (capacity > 0 && !out_pairs))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences: bad argument");
  { int rc0 = resolve_count(fixed); if (rc0) return rc0; rc0 = resolve_count(moving); if (rc0) return rc0; }
  { int rc0 = flush_pending(fixed); if (rc0) return rc0; rc0 = flush_pending(moving); if (rc0) return rc0; }
  *out_n = 0;
  if (is_point_query(sp->finder)) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    FindNNArgs N;
    N.fixed = cloud_dev(fixed, nullptr); N.moving = cloud_dev(moving, nullptr); N.fc = fi; N.mc = mi;
    N.use_distmap = sp->finder == LSM2D_FINDER_DISTMAP; N.use_kd = sp->finder == LSM2D_FINDER_KDTREE;
    int rc = prepare_point_query(ctx, sp, fixed, N.fixed, "find_correspondences: max_distance must be > 0"); if (rc) return rc;
    const size_t nm = (size_t) moving->h_count[mi], bytes = nm * 8 + 16;
    N.max_distance = sp->max_distance; N.normal_cos = sp->normal_cos; N.T = make_iso(pose); N.inl_tau = inl_tau;
    N.nn_group = fixed->h_count[fi] >= 4 * (int64_t) moving->h_count[mi] ? kNNGroup : 1;     // dense fixed cloud: cooperative search
    // more queries than one workgroup takes in a trip: one workgroup per trip's worth, two launches (search, then ordered compaction)
    const int per_step = kFindBlock / ((N.use_distmap || N.use_kd) ? 1 : N.nn_group);
    const int n_blocks = (int) ((nm + (size_t) per_step - 1) / (size_t) per_step);
    const bool multi = n_blocks > 2 && ctx->find_path != 1;      // (two trips of one workgroup beat two launches: 23 vs 29 us for 1081 distance-map queries)
    const size_t o_match = (bytes + 255) & ~(size_t) 255, o_cnt = o_match + ((nm * 4 + 255) & ~(size_t) 255);
    rc = ensure_scratch(ctx, multi ? o_cnt + 4 * (size_t) n_blocks : bytes); if (rc) return rc;
    rc = ensure_stage(ctx, bytes); if (rc) return rc;
    Lane& L = lane(ctx);
    const bool direct = bytes <= (1u << 16);             // up to 8k pairs: written straight to pinned host memory
    char* dv = (char*) (direct ? L.h_stage_dev : L.d_scratch);
    N.out_count = (int32_t*) dv; N.out_pairs = (int32_t*) (dv + 16);
    N.match = (int32_t*) ((char*) L.d_scratch + o_match); N.block_count = (int32_t*) ((char*) L.d_scratch + o_cnt);
    if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
    if (multi) {
      hipLaunchKernelGGL(k_find_nn_multi<0>, dim3((unsigned) n_blocks), dim3(kFindBlock), 0, ctx->stream, N);
      hipLaunchKernelGGL(k_find_nn_multi<1>, dim3((unsigned) n_blocks), dim3(kFindBlock), 0, ctx->stream, N);
    } else {
      hipLaunchKernelGGL(k_find_nn, dim3(1), dim3(kFindBlock), 0, ctx->stream, N);
    }
    HIPCHK(ctx, hipGetLastError());
    if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
    note_timed(ctx, ctx->kernel_timing);
    if (!direct) HIPCHK(ctx, hipMemcpyAsync(L.h_stage, L.d_scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_sync(ctx));
    const int32_t n = *(const int32_t*) L.h_stage;
    *out_n = n;
    if (n > capacity) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "find_correspondences: out_pairs too small");
    memcpy(out_pairs, (char*) L.h_stage + 16, sizeof(lsm2d_correspondence) * (size_t) n);
    return LSM2D_SUCCESS;
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
  const size_t o_can = (bytes + 255) & ~(size_t) 255;
  int rc = ensure_scratch(ctx, o_can + 2 * cols * sizeof(u64)); if (rc) return rc;
  rc = ensure_stage(ctx, bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  A.fixed = cloud_dev(fixed, nullptr); A.moving = cloud_dev(moving, nullptr); A.fc = fi; A.mc = mi;
  A.point_distance = sp->point_distance; A.normal_cos = sp->normal_cos; A.T = make_iso(pose); A.inl_tau = inl_tau;
  char* dv = (char*) L.h_stage_dev;       // <= one pair per column: written straight to pinned host memory
  A.out_count = (int32_t*) dv; A.out_pairs = (int32_t*) (dv + 16);
  A.fcan_global = nullptr; A.mcan_global = nullptr;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
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
  HIPCHK(ctx, hipGetLastError());
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  HIPCHK(ctx, stream_sync(ctx));
  const int32_t n = *(const int32_t*) L.h_stage;
  *out_n = n;
  if (n > capacity) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "find_correspondences: out_pairs too small");
  memcpy(out_pairs, (char*) L.h_stage + 16, sizeof(lsm2d_correspondence) * (size_t) n);
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_find_correspondences(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed,
                                          int32_t fi, const lsm2d_cloudset* moving, int32_t mi, const float pose[3],
                                          lsm2d_correspondence* out_pairs, int32_t capacity, int32_t* out_n) {
  return find_correspondences_impl(ctx, sp, fixed, fi, moving, mi, pose, out_pairs, capacity, out_n, 0.0f);
}

// ---- plugin interface #1 for a whole batch ------------------------------------------------------------------------
// The device room for the pairs of ONE launch of the batched finder, in pairs (8 bytes each: 16 MiB, and as much pinned staging behind it).  Every item owns
// pair_capacity slots of it whatever it finds, so a launch takes kFindBatchPairBudget / pair_capacity items (at least one); a batch beyond that runs as several
// launches over consecutive items, each with its own wait -- same results.  1000 scans against a 1081-column canvas (8.6 MB) are one launch; point-query items of
// a 100 000-point moving cloud go 20 to a launch.
static constexpr size_t kFindBatchPairBudget = (size_t) 2 << 20;

// The launch part of a batched finder pass, shared by lsm2d_find_correspondences_batch (find_batch_impl) and lsm2d_score_batch: what is the same for every
// item -- the sets' device views, the fixed set's search structure or the projector, the gates, the slot size -- and which kernel runs.
struct FindBatchLaunch {
  bool point_query = false;
  FindBatchArgs A; FindNNBatchArgs N;
  size_t lds = 0;
};

// Sizes only the device knows and pending unpacking / preprocessing are settled once for the whole batch, the fixed set's search structure is built or
// found, the launch arguments but the three per-launch pointers are filled in.  `who` heads the messages.
static int find_batch_prepare(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const lsm2d_cloudset* moving, float inl_tau,
                              int32_t capacity, const char* who, FindBatchLaunch& P) {
  char msg[160];
  if (lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  { int rc0 = resolve_count(fixed); if (rc0) return rc0; rc0 = resolve_count(moving); if (rc0) return rc0; }
  { int rc0 = flush_pending(fixed); if (rc0) return rc0; rc0 = flush_pending(moving); if (rc0) return rc0; }
  P.point_query = is_point_query(sp->finder);
  if (!P.point_query && sp->finder != LSM2D_FINDER_PROJECTIVE) { snprintf(msg, sizeof msg, "%s: finder not supported", who); return fail(ctx, LSM2D_BAD_ARGUMENT, msg); }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  FindBatchArgs& A = P.A; FindNNBatchArgs& N = P.N;
  if (P.point_query) {
    N.fixed = cloud_dev(fixed, nullptr); N.moving = cloud_dev(moving, nullptr);
    N.use_distmap = sp->finder == LSM2D_FINDER_DISTMAP; N.use_kd = sp->finder == LSM2D_FINDER_KDTREE;
    snprintf(msg, sizeof msg, "%s: max_distance must be > 0", who);
    const int rc = prepare_point_query(ctx, sp, fixed, N.fixed, msg); if (rc) return rc;
    N.max_distance = sp->max_distance; N.normal_cos = sp->normal_cos; N.inl_tau = inl_tau; N.pair_capacity = capacity;
  } else {
    if (!make_projk(sp->projector, &A.proj)) { snprintf(msg, sizeof msg, "%s: bad projector", who); return fail(ctx, LSM2D_BAD_ARGUMENT, msg); }
    P.lds = sizeof(u64) * 2 * (size_t) A.proj.cols;
    if ((int) P.lds > ctx->max_dyn_lds) { snprintf(msg, sizeof msg, "%s: canvases do not fit LDS", who); return fail(ctx, LSM2D_CAPACITY_EXCEEDED, msg); }
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

// n items, item k = (cloud fc[k] of `fixed`, cloud mc[k] of `moving`, poses[k]); its pairs go to out_pairs + slot * pair_stride and its count to
// out_n + slot * count_stride, slot = slots ? slots[k] : k.  The callers have checked the pointers, the indices and the capacity rule.
static int find_batch_impl(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fc, const lsm2d_cloudset* moving,
                           const int32_t* mc, int32_t n, const float* poses, float inl_tau, lsm2d_correspondence* out_pairs, int32_t capacity,
                           int32_t* out_n, const int32_t* slots, size_t pair_stride, size_t count_stride) {
  FindBatchLaunch P;
  { const int rc = find_batch_prepare(ctx, sp, fixed, moving, inl_tau, capacity, "find_correspondences_batch", P); if (rc) return rc; }
  size_t per_launch = kFindBatchPairBudget / (size_t) (capacity > 0 ? capacity : 1);
  if (per_launch < 1) per_launch = 1;
  if (per_launch > (size_t) n) per_launch = (size_t) n;
  // one layout for the lane's device scratch and its pinned staging: the items' arguments (up), then counts and pairs (down, ONE copy)
  const size_t o_cnt = (sizeof(FindItem) * per_launch + 255) & ~(size_t) 255, o_pairs = (o_cnt + sizeof(int32_t) * per_launch + 255) & ~(size_t) 255;
  const size_t bytes = o_pairs + sizeof(lsm2d_correspondence) * per_launch * (size_t) capacity;
  { int rc = ensure_scratch(ctx, bytes); if (rc) return rc; rc = ensure_stage(ctx, bytes); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  for (size_t k0 = 0; k0 < (size_t) n; k0 += per_launch) {
    const size_t cnt = (size_t) n - k0 < per_launch ? (size_t) n - k0 : per_launch;
    find_batch_fill_items((FindItem*) hs, fixed, fc + k0, moving, mc + k0, poses + 3 * k0, cnt);
    HIPCHK(ctx, hipMemcpyAsync(ds, hs, sizeof(FindItem) * cnt, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
    find_batch_launch(ctx, P, (const FindItem*) ds, cnt, (int32_t*) (ds + o_cnt), (int32_t*) (ds + o_pairs));
    HIPCHK(ctx, hipGetLastError());
    if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
    note_timed(ctx, ctx->kernel_timing);
    const size_t down = o_pairs - o_cnt + sizeof(lsm2d_correspondence) * cnt * (size_t) capacity;
    HIPCHK(ctx, hipMemcpyAsync(hs + o_cnt, ds + o_cnt, down, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_sync(ctx));      // the one wait of this launch
    const int32_t* h_cnt = (const int32_t*) (hs + o_cnt);
    for (size_t k = 0; k < cnt; ++k) {
      const size_t slot = slots ? (size_t) slots[k0 + k] : k0 + k;
      const int32_t np = h_cnt[k];
      if (np < 0 || np > capacity) return fail(ctx, LSM2D_DEVICE_ERROR, "find_correspondences_batch: an item reported more pairs than its slot holds");
      out_n[slot * count_stride] = np;
      if (np) memcpy(out_pairs + slot * pair_stride, hs + o_pairs + sizeof(lsm2d_correspondence) * k * (size_t) capacity, sizeof(lsm2d_correspondence) * (size_t) np);
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
  if (!ctx || !sp || !fixed || !moving || n_items < 0 || pair_capacity < 0) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences_batch: bad argument");
  if (fixed->ctx != ctx || moving->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences_batch: cloud set from another (or a destroyed) context");
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  if (n_items == 0) return LSM2D_SUCCESS;
  if (!poses || !out_n_pairs || (pair_capacity > 0 && !out_pairs)) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences_batch: null argument");
  if (!fixed_index && fixed->n_clouds != 1 && fixed->n_clouds != n_items) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences_batch: fixed set must hold 1 or n_items clouds");
  if (!moving_index && moving->n_clouds != 1 && moving->n_clouds != n_items) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences_batch: moving set must hold 1 or n_items clouds");
  std::vector<int32_t> fc((size_t) n_items), mc((size_t) n_items);
  for (int32_t i = 0; i < n_items; ++i) {
    fc[(size_t) i] = fixed_index ? fixed_index[i] : (fixed->n_clouds == 1 ? 0 : i);
    mc[(size_t) i] = moving_index ? moving_index[i] : (moving->n_clouds == 1 ? 0 : i);
    if (!valid_cloud_index(fixed, fc[(size_t) i]) || !valid_cloud_index(moving, mc[(size_t) i])) return fail(ctx, LSM2D_BAD_ARGUMENT, "find_correspondences_batch: cloud index out of range");
  }
  long long need = 0;
  { const int rc0 = find_batch_need(sp, moving, &need); if (rc0) return rc0; }
  if (need > pair_capacity) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "find_correspondences_batch: pair_capacity below the largest possible correspondence vector");
  return find_batch_impl(ctx, sp, fixed, fc.data(), moving, mc.data(), n_items, poses, 0.0f, out_pairs, pair_capacity, out_n_pairs, nullptr, (size_t) pair_capacity, 1);
}

// ---- factor ---------------------------------------------------------------------------------------------------
extern "C" int lsm2d_linearize(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, int32_t fi,
                               const lsm2d_cloudset* moving, int32_t mi, const lsm2d_correspondence* pairs, int32_t n_pairs,
                               const float pose[3], float out_H[9], float out_b[3], lsm2d_iteration_stats* st) {
  if (!ctx || !sp || !pose || !out_H || !out_b || !valid_cloud_index(fixed, fi) || !valid_cloud_index(moving, mi) || n_pairs < 0 ||
      (n_pairs > 0 && !pairs))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize: bad argument");
  { int rc0 = resolve_count(fixed); if (rc0) return rc0; rc0 = resolve_count(moving); if (rc0) return rc0; }
  { int rc0 = flush_pending(fixed); if (rc0) return rc0; rc0 = flush_pending(moving); if (rc0) return rc0; }
  for (int32_t k = 0; k < n_pairs; ++k)
    if (pairs[k].fixed_idx < 0 || pairs[k].fixed_idx >= fixed->h_count[fi] || pairs[k].moving_idx < 0 || pairs[k].moving_idx >= moving->h_count[mi])
      return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize: correspondence index out of range");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int blocks = (n_pairs + 255) / 256; if (blocks < 1) blocks = 1; if (blocks > 1024) blocks = 1024;
  const size_t pair_bytes = sizeof(lsm2d_correspondence) * (size_t) n_pairs;
  const size_t part_off = (pair_bytes + 255) & ~(size_t) 255, out_off = part_off + sizeof(float) * kAccumWords * (size_t) blocks;
  const size_t dig_off = out_off + sizeof(float) * kAccumWords;      // 8-byte aligned: out_off is a multiple of 256, kAccumWords is even
  static_assert(kAccumWords % 2 == 0, "the digest behind the sums must be 8-byte aligned");
  const size_t bytes = dig_off + sizeof(unsigned long long);
  int rc = ensure_scratch(ctx, bytes); if (rc) return rc;
  rc = ensure_stage(ctx, bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  if (n_pairs) memcpy(L.h_stage, pairs, pair_bytes);
  // up to 8k pairs (a canvas worth): the kernels read the pairs from, and write the sums to, the pinned staging buffer directly
  const bool direct = n_pairs <= 8192;
  char* dv = (char*) (direct ? L.h_stage_dev : L.d_scratch);
  if (!direct && n_pairs) HIPCHK(ctx, hipMemcpyAsync(L.d_scratch, L.h_stage, pair_bytes, hipMemcpyHostToDevice, ctx->stream));
  LinArgs A;
  A.fixed = cloud_dev(fixed, nullptr); A.moving = cloud_dev(moving, nullptr); A.fc = fi; A.mc = mi;
  A.pairs = (const int32_t*) dv; A.n_pairs = n_pairs; A.T = make_iso(pose);
  A.cauchy = sp->robustifier == LSM2D_ROBUST_CAUCHY; A.tau = sp->chi_threshold;
  A.partial = (float*) ((char*) L.d_scratch + part_off); A.out = (float*) (dv + out_off);
  A.dig = (unsigned long long*) (dv + dig_off);
  if (direct) *(unsigned long long*) ((char*) L.h_stage + dig_off) = 0ull;
  else HIPCHK(ctx, hipMemsetAsync(A.dig, 0, sizeof(unsigned long long), ctx->stream));
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  if (ctx->sum_order) hipLaunchKernelGGL(k_linearize_seq, dim3(1), dim3(kAlignBlock), 0, ctx->stream, A);      // pair after pair, the order of the vector
  else {
    hipLaunchKernelGGL(k_linearize_partial, dim3(blocks), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_linearize_final, dim3(1), dim3(64), 0, ctx->stream, (const float*) A.partial, blocks, A.out);
  }
  HIPCHK(ctx, hipGetLastError());
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  float* h = (float*) ((char*) L.h_stage + out_off);
  if (!direct) HIPCHK(ctx, hipMemcpyAsync(h, A.out, sizeof(float) * kAccumWords + sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  out_H[0] = h[0]; out_H[1] = h[1]; out_H[2] = h[2]; out_H[3] = h[1]; out_H[4] = h[3]; out_H[5] = h[4]; out_H[6] = h[2]; out_H[7] = h[4]; out_H[8] = h[5];
  out_b[0] = h[6]; out_b[1] = h[7]; out_b[2] = h[8];
  if (st) {
    int32_t iv[3]; memcpy(iv, h + 11, sizeof iv);
    st->n_inliers = iv[0]; st->n_outliers = iv[1]; st->n_correspondences = iv[2]; st->chi_inliers = h[9]; st->chi_outliers = h[10];
    unsigned long long dg; memcpy(&dg, (char*) L.h_stage + dig_off, sizeof dg);
    st->pair_digest_lo = (uint32_t) dg; st->pair_digest_hi = (uint32_t) (dg >> 32);
  }
  return LSM2D_SUCCESS;
}

// ---- factor for a whole batch ---------------------------------------------------------------------------------------
// The device room for the pairs of ONE launch of the batched factor, in pairs: the batch finder's.  As there, every item counts with its pair_capacity
// slots whatever it holds (the rule depends on the arguments' shape alone), so a launch takes kLinBatchPairBudget / pair_capacity items -- at least one, at
// most kLinBatchMaxItems, which bounds the item table -- and a batch beyond that runs as several launches over consecutive items, each with its own wait.
// Only the first n_pairs[i] entries of a row travel: they are packed one vector after the other on their way to the staging buffer.
static constexpr size_t kLinBatchPairBudget = (size_t) 2 << 20;
static constexpr size_t kLinBatchMaxItems = (size_t) 1 << 16;

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t) 255; }

// where a launch's parts lie in the lane's device scratch and (the first three and the results) in its pinned staging
struct LinBatchLayout {
  size_t o_wg, o_pairs, up_bytes, o_part, o_dig, o_out, d_bytes, h_out, h_bytes;
  LinBatchLayout(size_t cnt, size_t blocks, size_t npairs) {
    o_wg = up256(sizeof(LinItem) * cnt); o_pairs = up256(o_wg + sizeof(int32_t) * blocks); up_bytes = o_pairs + sizeof(lsm2d_correspondence) * npairs;
    o_part = up256(up_bytes); o_dig = up256(o_part + sizeof(float) * kAccumWords * blocks); o_out = up256(o_dig + sizeof(unsigned long long) * cnt);
    d_bytes = o_out + sizeof(float) * kLinOutWords * cnt;
    h_out = up256(up_bytes); h_bytes = h_out + sizeof(float) * kLinOutWords * cnt;
  }
};

extern "C" int lsm2d_linearize_batch(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                     const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const lsm2d_correspondence* pairs,
                                     int32_t pair_capacity, const int32_t* n_pairs, const float* poses, float* out_H, float* out_b, lsm2d_iteration_stats* st) {
  if (!ctx || !sp || !fixed || !moving || n_items < 0 || pair_capacity < 0) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: bad argument");
  if (fixed->ctx != ctx || moving->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: cloud set from another (or a destroyed) context");
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  if (n_items == 0) return LSM2D_SUCCESS;
  if (!n_pairs || !poses || !out_H || !out_b) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: null argument");
  if (!fixed_index && fixed->n_clouds != 1 && fixed->n_clouds != n_items) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: fixed set must hold 1 or n_items clouds");
  if (!moving_index && moving->n_clouds != 1 && moving->n_clouds != n_items) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: moving set must hold 1 or n_items clouds");
  char msg[160];
  std::vector<int32_t> fc((size_t) n_items), mc((size_t) n_items);
  for (int32_t i = 0; i < n_items; ++i) {
    fc[(size_t) i] = fixed_index ? fixed_index[i] : (fixed->n_clouds == 1 ? 0 : i);
    mc[(size_t) i] = moving_index ? moving_index[i] : (moving->n_clouds == 1 ? 0 : i);
    if (!valid_cloud_index(fixed, fc[(size_t) i]) || !valid_cloud_index(moving, mc[(size_t) i])) {
      snprintf(msg, sizeof msg, "linearize_batch: item %d: cloud index out of range", (int) i);
      return fail(ctx, LSM2D_BAD_ARGUMENT, msg);
    }
  }
  // sizes only the device knows, pending unpacking / preprocessing: once for the whole batch (the validation below needs the sizes)
  { int rc0 = resolve_count(fixed); if (rc0) return rc0; rc0 = resolve_count(moving); if (rc0) return rc0; }
  { int rc0 = flush_pending(fixed); if (rc0) return rc0; rc0 = flush_pending(moving); if (rc0) return rc0; }
  // every item is checked before anything is launched or written
  for (int32_t i = 0; i < n_items; ++i) {
    const int32_t np = n_pairs[i];
    if (np > 0 && !pairs) return fail(ctx, LSM2D_BAD_ARGUMENT, "linearize_batch: null argument");
    if (np < 0 || np > pair_capacity) {
      snprintf(msg, sizeof msg, "linearize_batch: item %d: n_pairs %d outside [0, pair_capacity %d]", (int) i, (int) np, (int) pair_capacity);
      return fail(ctx, LSM2D_BAD_ARGUMENT, msg);
    }
    const lsm2d_correspondence* row = np ? pairs + (size_t) i * (size_t) pair_capacity : nullptr;
    const int32_t nf = fixed->h_count[fc[(size_t) i]], nm = moving->h_count[mc[(size_t) i]];
    for (int32_t k = 0; k < np; ++k)
      if (row[k].fixed_idx < 0 || row[k].fixed_idx >= nf || row[k].moving_idx < 0 || row[k].moving_idx >= nm) {
        snprintf(msg, sizeof msg, "linearize_batch: item %d: correspondence %d (%d, %d) out of range", (int) i, (int) k, (int) row[k].fixed_idx, (int) row[k].moving_idx);
        return fail(ctx, LSM2D_BAD_ARGUMENT, msg);
      }
  }
  size_t per_launch = kLinBatchPairBudget / (size_t) (pair_capacity > 0 ? pair_capacity : 1);
  if (per_launch > kLinBatchMaxItems) per_launch = kLinBatchMaxItems;
  if (per_launch < 1) per_launch = 1;
  if (per_launch > (size_t) n_items) per_launch = (size_t) n_items;
  // the largest launch decides the buffers' sizes: they are grown (and waited for) once, ahead of the first launch
  size_t d_need = 0, h_need = 0;
  for (size_t k0 = 0; k0 < (size_t) n_items; k0 += per_launch) {
    const size_t cnt = (size_t) n_items - k0 < per_launch ? (size_t) n_items - k0 : per_launch;
    size_t blocks = 0, np = 0;
    for (size_t k = 0; k < cnt; ++k) { blocks += (size_t) lin_blocks(n_pairs[k0 + k]); np += (size_t) n_pairs[k0 + k]; }
    const LinBatchLayout Y(cnt, blocks, np);
    d_need = std::max(d_need, Y.d_bytes); h_need = std::max(h_need, Y.h_bytes);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  { int rc = ensure_scratch(ctx, d_need); if (rc) return rc; rc = ensure_stage(ctx, h_need); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  LinBatchArgs A;
  A.fixed = cloud_dev(fixed, nullptr); A.moving = cloud_dev(moving, nullptr);
  A.cauchy = sp->robustifier == LSM2D_ROBUST_CAUCHY; A.tau = sp->chi_threshold;
  for (size_t k0 = 0; k0 < (size_t) n_items; k0 += per_launch) {
    const size_t cnt = (size_t) n_items - k0 < per_launch ? (size_t) n_items - k0 : per_launch;
    size_t blocks = 0, np = 0;
    for (size_t k = 0; k < cnt; ++k) { blocks += (size_t) lin_blocks(n_pairs[k0 + k]); np += (size_t) n_pairs[k0 + k]; }
    const LinBatchLayout Y(cnt, blocks, np);
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
    if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
    if (ctx->sum_order) hipLaunchKernelGGL(k_linearize_seq_batch, dim3((unsigned) cnt), dim3(kAlignBlock), 0, ctx->stream, A);      // pair after pair, a workgroup per item
    else {
      hipLaunchKernelGGL(k_linearize_partial_batch, dim3((unsigned) blocks), dim3(256), 0, ctx->stream, A);
      hipLaunchKernelGGL(k_linearize_final_batch, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, ctx->stream, A);
    }
    HIPCHK(ctx, hipGetLastError());
    if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
    note_timed(ctx, ctx->kernel_timing);
    HIPCHK(ctx, hipMemcpyAsync(hs + Y.h_out, A.out, sizeof(float) * kLinOutWords * cnt, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_sync(ctx));      // the one wait of this launch
    for (size_t k = 0; k < cnt; ++k) {
      const float* h = (const float*) (hs + Y.h_out) + kLinOutWords * k;
      float* H = out_H + 9 * (k0 + k); float* b = out_b + 3 * (k0 + k);
      H[0] = h[0]; H[1] = h[1]; H[2] = h[2]; H[3] = h[1]; H[4] = h[3]; H[5] = h[4]; H[6] = h[2]; H[7] = h[4]; H[8] = h[5];
      b[0] = h[6]; b[1] = h[7]; b[2] = h[8];
      if (st) {
        lsm2d_iteration_stats& s = st[k0 + k];
        int32_t iv[3]; memcpy(iv, h + 11, sizeof iv);
        s.n_inliers = iv[0]; s.n_outliers = iv[1]; s.n_correspondences = iv[2]; s.chi_inliers = h[9]; s.chi_outliers = h[10];
        unsigned long long dg; memcpy(&dg, h + kAccumWords, sizeof dg);
        s.pair_digest_lo = (uint32_t) dg; s.pair_digest_hi = (uint32_t) (dg >> 32);
      }
    }
  }
  return LSM2D_SUCCESS;
}

// ---- finder + factor for a whole batch: pose hypotheses scored on the device ------------------------------------------------------------------------
// One result row of the batched factor (kLinOutWords words) as the ABI's H, b and statistics.
static void lin_row_out(const float* h, float* H, float* b, lsm2d_iteration_stats* s) {
  H[0] = h[0]; H[1] = h[1]; H[2] = h[2]; H[3] = h[1]; H[4] = h[3]; H[5] = h[4]; H[6] = h[2]; H[7] = h[4]; H[8] = h[5];
  b[0] = h[6]; b[1] = h[7]; b[2] = h[8];
  if (s) {
    int32_t iv[3]; memcpy(iv, h + 11, sizeof iv);
    s->n_inliers = iv[0]; s->n_outliers = iv[1]; s->n_correspondences = iv[2]; s->chi_inliers = h[9]; s->chi_outliers = h[10];
    unsigned long long dg; memcpy(&dg, h + kAccumWords, sizeof dg);
    s->pair_digest_lo = (uint32_t) dg; s->pair_digest_hi = (uint32_t) (dg >> 32);
  }
}

// The batch finder's kernels write every item's pairs into its slot of the lane's device scratch and its count next to them; the k_score_* kernels linearise
// them there.  A slot is the slice's largest possible vector (find_batch_need), so a launch group takes kFindBatchPairBudget / slot items (at least one, at
// most kLinBatchMaxItems): the groups are queued one behind the other on the stream and reuse the same pair and partial-row scratch, while the items'
// arguments (uploaded once), their counts, digests and result rows are arrays over the whole batch.  One copy down and ONE wait, at the end.
// The scoring is shared by lsm2d_score_batch, which copies every row down, and lsm2d_score_select, which ranks the rows where they lie: score_batch_head is
// what both check before they look at n_items, score_batch_queue everything from the index rules to the last launch group -- it leaves the rows on the device
// (ds + o_out), waits for nothing and, with "kernel_timing", has recorded the lane's first event in front of the last group; the caller records the second.
struct ScoreQueued {
  size_t n = 0;
  size_t o_out = 0;       // device: the result rows, [n][kLinOutWords]
  size_t o_extra = 0;     // device: d_extra bytes of the caller's behind everything the scoring uses
  size_t h_out = 0;       // staging: h_down bytes of the caller's behind the items' arguments
};

static int score_batch_head(lsm2d_context* ctx, const char* who, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const lsm2d_cloudset* moving,
                            int32_t n_items) {
  char msg[160];
  if (!ctx || !sp || !fixed || !moving || n_items < 0) { snprintf(msg, sizeof msg, "%s: bad argument", who); return fail(ctx, LSM2D_BAD_ARGUMENT, msg); }
  if (fixed->ctx != ctx || moving->ctx != ctx) {
    snprintf(msg, sizeof msg, "%s: cloud set from another (or a destroyed) context", who);
    return fail(ctx, LSM2D_BAD_ARGUMENT, msg);
  }
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  return LSM2D_SUCCESS;
}

static int score_batch_queue(lsm2d_context* ctx, const char* who, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                             const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses, size_t d_extra, size_t h_down,
                             ScoreQueued& Q) {
  char msg[160];
  if (!fixed_index && fixed->n_clouds != 1 && fixed->n_clouds != n_items) { snprintf(msg, sizeof msg, "%s: fixed set must hold 1 or n_items clouds", who); return fail(ctx, LSM2D_BAD_ARGUMENT, msg); }
  if (!moving_index && moving->n_clouds != 1 && moving->n_clouds != n_items) { snprintf(msg, sizeof msg, "%s: moving set must hold 1 or n_items clouds", who); return fail(ctx, LSM2D_BAD_ARGUMENT, msg); }
  const size_t n = (size_t) n_items;
  std::vector<int32_t> fc(n), mc(n);
  for (int32_t i = 0; i < n_items; ++i) {
    fc[(size_t) i] = fixed_index ? fixed_index[i] : (fixed->n_clouds == 1 ? 0 : i);
    mc[(size_t) i] = moving_index ? moving_index[i] : (moving->n_clouds == 1 ? 0 : i);
    if (!valid_cloud_index(fixed, fc[(size_t) i]) || !valid_cloud_index(moving, mc[(size_t) i])) {
      snprintf(msg, sizeof msg, "%s: item %d: cloud index out of range", who, (int) i);
      return fail(ctx, LSM2D_BAD_ARGUMENT, msg);
    }
  }
  long long need = 0;
  { const int rc0 = find_batch_need(sp, moving, &need); if (rc0) return rc0; }
  if (need < 0 || need > 0x7fffffffll) { snprintf(msg, sizeof msg, "%s: bad projector", who); return fail(ctx, LSM2D_BAD_ARGUMENT, msg); }
  const int32_t slot = (int32_t) need;
  FindBatchLaunch P;
  { const int rc = find_batch_prepare(ctx, sp, fixed, moving, 0.0f, slot, who, P); if (rc) return rc; }
  size_t per_group = kFindBatchPairBudget / (size_t) (slot > 0 ? slot : 1);
  if (per_group > kLinBatchMaxItems) per_group = kLinBatchMaxItems;
  if (per_group < 1) per_group = 1;
  if (per_group > n) per_group = n;
  const size_t B = (size_t) lin_blocks(slot);
  // device: [items | counts | digests | result rows] over the whole batch, then [pairs | partial rows] of one launch group, then the caller's; host: items
  // up, the caller's down
  const size_t o_cnt = up256(sizeof(FindItem) * n), o_dig = up256(o_cnt + sizeof(int32_t) * n), o_out = up256(o_dig + sizeof(unsigned long long) * n);
  const size_t o_pairs = up256(o_out + sizeof(float) * kLinOutWords * n), o_part = up256(o_pairs + sizeof(lsm2d_correspondence) * per_group * (size_t) slot);
  const size_t o_extra = up256(o_part + sizeof(float) * kAccumWords * per_group * B), d_bytes = o_extra + d_extra;
  const size_t h_out = up256(sizeof(FindItem) * n), h_bytes = h_out + h_down;
  { int rc = ensure_scratch(ctx, d_bytes); if (rc) return rc; rc = ensure_stage(ctx, h_bytes); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  find_batch_fill_items((FindItem*) hs, fixed, fc.data(), moving, mc.data(), poses, n);
  HIPCHK(ctx, hipMemcpyAsync(ds, hs, sizeof(FindItem) * n, hipMemcpyHostToDevice, ctx->stream));
  if (!ctx->sum_order) HIPCHK(ctx, hipMemsetAsync(ds + o_dig, 0, sizeof(unsigned long long) * n, ctx->stream));
  ScoreBatchArgs S;
  S.fixed = P.point_query ? P.N.fixed : P.A.fixed; S.moving = P.point_query ? P.N.moving : P.A.moving;
  S.slot = slot; S.blocks_per_item = (int32_t) B; S.cauchy = sp->robustifier == LSM2D_ROBUST_CAUCHY; S.tau = sp->chi_threshold;
  S.pairs = (const int32_t*) (ds + o_pairs); S.partial = (float*) (ds + o_part);
  for (size_t k0 = 0; k0 < n; k0 += per_group) {
    const size_t cnt = n - k0 < per_group ? n - k0 : per_group;
    const bool timed = ctx->kernel_timing && k0 + cnt == n;      // the last launch group, finder and factor together
    S.items = (const FindItem*) ds + k0; S.count = (const int32_t*) (ds + o_cnt) + k0; S.n_items = (int32_t) cnt;
    S.dig = (unsigned long long*) (ds + o_dig) + k0; S.out = (float*) (ds + o_out) + kLinOutWords * k0;
    if (timed) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
    find_batch_launch(ctx, P, S.items, cnt, (int32_t*) (ds + o_cnt) + k0, (int32_t*) (ds + o_pairs));
    if (ctx->sum_order) hipLaunchKernelGGL(k_score_seq_batch, dim3((unsigned) cnt), dim3(kAlignBlock), 0, ctx->stream, S);      // pair after pair, a workgroup per item
    else {
      hipLaunchKernelGGL(k_score_partial_batch, dim3((unsigned) (cnt * B)), dim3(256), 0, ctx->stream, S);
      hipLaunchKernelGGL(k_score_final_batch, dim3((unsigned) ((cnt + 255) / 256)), dim3(256), 0, ctx->stream, S);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  Q.n = n; Q.o_out = o_out; Q.o_extra = o_extra; Q.h_out = h_out;
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_score_batch(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                 const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses, float* out_H, float* out_b,
                                 lsm2d_iteration_stats* st) {
  { const int rc = score_batch_head(ctx, "score_batch", sp, fixed, moving, n_items); if (rc) return rc; }
  if (n_items == 0) return LSM2D_SUCCESS;
  if (!poses || !out_H || !out_b) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_batch: null argument");
  ScoreQueued Q;
  { const int rc = score_batch_queue(ctx, "score_batch", sp, fixed, fixed_index, moving, moving_index, n_items, poses, 0, sizeof(float) * kLinOutWords * (size_t) n_items, Q); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  const size_t n = Q.n;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  HIPCHK(ctx, hipMemcpyAsync(hs + Q.h_out, ds + Q.o_out, sizeof(float) * kLinOutWords * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  for (size_t k = 0; k < n; ++k) lin_row_out((const float*) (hs + Q.h_out) + kLinOutWords * k, out_H + 9 * k, out_b + 3 * k, st ? st + k : nullptr);
  return LSM2D_SUCCESS;
}

// ---- ... and ranked on the device: the acceptance test and the best k (lsm2d_k_select.h) ------------------------------------------------------------------------
// Behind the last launch group, on the same stream: keys and the accepted count (k_select_keys), passes of k_select_tile over two ping-pong arrays of (key,
// index) entries until one tile is left -- a pass turns m entries into ceil(m / tile) x k, less than half of them while m > tile -- and k_select_gather,
// which fills the one region that comes down: [n_accepted, n_selected, 0, 0 | index[k] | rows[k][kLinOutWords]], 16 + 68 k bytes whatever n_items is.  A
// batch of at most one tile does all three in ONE launch (k_select_tile_one: four launches and a memset less, which is what counts at 1000 items).
extern "C" int lsm2d_score_select(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                  const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses,
                                  const lsm2d_select_params* select, int32_t k, int32_t* out_index, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats,
                                  int32_t* out_n_selected, int32_t* out_n_accepted) {
  static_assert(LSM2D_SELECT_MAX_K == kSelectMaxK, "the ABI's limit is the kernels'");
  if (!select || !out_index || !out_n_selected || !out_n_accepted) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select: null argument");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select: k outside [1, LSM2D_SELECT_MAX_K]");
  { const int rc = score_batch_head(ctx, "score_select", sp, fixed, moving, n_items); if (rc) return rc; }
  if (n_items == 0) { *out_n_selected = 0; *out_n_accepted = 0; return LSM2D_SUCCESS; }
  if (!poses) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select: null argument");
  const size_t n = (size_t) n_items, K = (size_t) k;
  const size_t n_first = ((n + kSelectTile - 1) / kSelectTile) * K;      // what the first pass leaves
  // the caller's part of the scratch: [keys A | index A] of n entries, [keys B | index B] of n_first, the accepted count, the region that goes down
  const size_t e_idx_a = up256(sizeof(u64) * n), e_key_b = up256(e_idx_a + sizeof(int32_t) * n), e_idx_b = up256(e_key_b + sizeof(u64) * n_first);
  const size_t e_acc = up256(e_idx_b + sizeof(int32_t) * n_first), e_down = e_acc + 256;
  const size_t down_bytes = sizeof(int32_t) * (kSelectHeaderWords + K) + sizeof(float) * kLinOutWords * K;
  ScoreQueued Q;
  { const int rc = score_batch_queue(ctx, "score_select", sp, fixed, fixed_index, moving, moving_index, n_items, poses, e_down + down_bytes, down_bytes, Q); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch; char* const de = ds + Q.o_extra;
  u64* key[2] = {(u64*) de, (u64*) (de + e_key_b)}; int32_t* idx[2] = {(int32_t*) (de + e_idx_a), (int32_t*) (de + e_idx_b)};
  SelectArgs A;
  A.rows = (const float*) (ds + Q.o_out); A.n_items = n_items; A.k = k;
  A.min_inliers = select->min_inliers; A.max_chi_per_inlier = select->max_chi_per_inlier; A.min_inlier_ratio = select->min_inlier_ratio;
  A.keys = key[0]; A.index = idx[0]; A.n_accepted = (int32_t*) (de + e_acc);
  if (n <= (size_t) kSelectTile) {      // one tile: keys, sort and gather in one launch of one workgroup
    int32_t sort_size = 2;
    while ((size_t) sort_size < n) sort_size <<= 1;
    hipLaunchKernelGGL(k_select_tile_one, dim3(1), dim3(kSelectBlock), 0, ctx->stream, A, sort_size, (int32_t*) (de + e_down));
  } else {
    HIPCHK(ctx, hipMemsetAsync(A.n_accepted, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_select_keys, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    size_t m = n; int src = 0;
    for (;;) {      // array A has room for n entries, B for n_first: pass p writes fewer than pass p - 2 read
      const size_t tiles = (m + kSelectTile - 1) / kSelectTile;
      hipLaunchKernelGGL(k_select_tile, dim3((unsigned) tiles), dim3(kSelectBlock), 0, ctx->stream, (const u64*) key[src], (const int32_t*) idx[src], (int32_t) m,
                         k, key[src ^ 1], idx[src ^ 1]);
      src ^= 1; m = tiles * K;
      if (tiles == 1) break;
    }
    hipLaunchKernelGGL(k_select_gather, dim3(1), dim3(256), 0, ctx->stream, A, (const u64*) key[src], (const int32_t*) idx[src], (int32_t*) (de + e_down));
  }
  HIPCHK(ctx, hipGetLastError());
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));      // the last launch group and the selection
  note_timed(ctx, ctx->kernel_timing);
  HIPCHK(ctx, hipMemcpyAsync(hs + Q.h_out, de + e_down, down_bytes, hipMemcpyDeviceToHost, ctx->stream));      // the one copy down
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  const int32_t* h = (const int32_t*) (hs + Q.h_out);
  const int32_t n_acc = h[0], n_sel = h[1];
  if (n_acc < 0 || n_acc > n_items || n_sel != (n_acc < k ? n_acc : k)) return fail(ctx, LSM2D_DEVICE_ERROR, "score_select: the selection's counters are inconsistent");
  const int32_t* h_index = h + kSelectHeaderWords; const float* h_rows = (const float*) (h + kSelectHeaderWords + K);
  float H[9], b[3];
  for (int32_t j = 0; j < n_sel; ++j) {
    out_index[j] = h_index[j];
    lin_row_out(h_rows + kLinOutWords * (size_t) j, out_H ? out_H + 9 * (size_t) j : H, out_b ? out_b + 3 * (size_t) j : b, out_stats ? out_stats + j : nullptr);
  }
  *out_n_selected = n_sel; *out_n_accepted = n_acc;
  return LSM2D_SUCCESS;
}
