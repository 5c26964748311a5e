// lsm2d_capi_mapping.inc -- the steps either side of the aligner: RawDataPreprocessorProjective2D (batched, refill, single scan), SceneClipperProjective2D, MergerProjective2D, the projector.
// Part of lsm2d_capi.hip (included there); not a translation unit of its own.
static void launch_preprocess_scans(const PrepArgs& A, int n_scans, hipStream_t st) {
  if (n_scans >= 8 && A.n_beams <= kPrepSmallBeams) hipLaunchKernelGGL(k_preprocess_scans_small, dim3((unsigned) n_scans), dim3(kPrepSmallBlock), 0, st, A);
  else hipLaunchKernelGGL(k_preprocess_scans, dim3((unsigned) n_scans), dim3(kPrepBlock), 0, st, A);
}
// the preprocessor's parameters, checked the same way by every entry point (`who`: its name, as the messages carry it)
static int check_preprocessor(lsm2d_context* ctx, const lsm2d_preprocessor* pp, const char* who) {
  char msg[96];
  if (pp->n_beams < 1 || pp->n_beams > kPrepMaxBeams) { snprintf(msg, sizeof msg, "%s: n_beams must be in [1, 2048]", who); return fail(ctx, LSM2D_CAPACITY_EXCEEDED, msg); }
  if (!(pp->angle_max > pp->angle_min) || pp->normal_min_points < 1 || !(pp->normal_point_distance >= 0.0f)) { snprintf(msg, sizeof msg, "%s: bad parameters", who); return fail(ctx, LSM2D_BAD_ARGUMENT, msg); }
  return LSM2D_SUCCESS;
}
// beam directions with the host libm (the oracle does the same): angle = (c - n/2) * sensor_res
static void beam_dirs_host(const lsm2d_preprocessor* pp, float2* hd) {
  const int nb = pp->n_beams;
  const float sensor_res = (pp->angle_max - pp->angle_min) / (float) nb, k01 = (float) nb * 0.5f;
  for (int c = 0; c < nb; ++c) { const float a = ((float) c - k01) * sensor_res; hd[c] = make_float2(cosf(a), sinf(a)); }
}
// ... on the device, once per sensor geometry (lsm2d_context::beam_dirs)
static int beam_dirs_device(lsm2d_context* ctx, const lsm2d_preprocessor* pp, const float2** out) {
  const int nb = pp->n_beams;
  for (const auto& bd : ctx->beam_dirs) if (bd.n_beams == nb && bd.angle_min == pp->angle_min && bd.angle_max == pp->angle_max) { *out = bd.d_dir; return LSM2D_SUCCESS; }
  std::vector<float2> hd((size_t) nb);
  beam_dirs_host(pp, hd.data());
  DevBuf<float2> d;
  HIPCHK(ctx, d.alloc(sizeof(float2) * (size_t) nb));
  HIPCHK(ctx, hipMemcpy(d, hd.data(), sizeof(float2) * (size_t) nb, hipMemcpyHostToDevice));
  *out = d;
  ctx->beam_dirs.push_back({nb, pp->angle_min, pp->angle_max, std::move(d)});
  return LSM2D_SUCCESS;
}
// the preprocessing kernels' arguments: the scans' ranges and beam directions in, the clouds of `out` out (a stride of n_beams, made even, per cloud)
static PrepArgs make_prep_args(const lsm2d_preprocessor* pp, const float* ranges, const float2* beam_dir, const lsm2d_cloudset* out) {
  PrepArgs A;
  A.ranges = ranges; A.beam_dir = beam_dir;
  A.n_beams = pp->n_beams; A.stride = pp->n_beams + (pp->n_beams & 1); A.rmin = pp->range_min; A.rmax = pp->range_max;
  A.d2max = pp->normal_point_distance * pp->normal_point_distance; A.min_points = pp->normal_min_points;
  A.inv_res = pp->voxelize_resolution > 0.0f ? 1.0f / pp->voxelize_resolution : 0.0f;
  A.out_xy = out->d_xy; A.out_nrm = out->d_nrm; A.out_count = out->d_count;
  return A;
}
// ---- RawDataPreprocessorProjective2D, batched -------------------------------------------------------------------
extern "C" int lsm2d_preprocess_scans(lsm2d_context* ctx, const lsm2d_preprocessor* pp, const float* ranges, int32_t n_scans,
                                      lsm2d_cloudset** out) {
  if (!ctx || !pp || !out || n_scans < 1 || !ranges) return fail(ctx, LSM2D_BAD_ARGUMENT, "preprocess_scans: bad argument");
  *out = nullptr;
  { const int rc0 = check_preprocessor(ctx, pp, "preprocess_scans"); if (rc0) return rc0; }
  const int nb = pp->n_beams;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int stride = nb + (nb & 1);
  if ((int64_t) stride * n_scans > 0x7ffffff0) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "preprocess_scans: too many points");
  CloudsetGuard cs;
  int rc = cloudset_new(ctx, cs, [&](lsm2d_cloudset* s) { cloudset_slots(s, n_scans, stride); return LSM2D_SUCCESS; });
  if (rc != LSM2D_SUCCESS) return rc;
  // where the ranges live: device memory is read in place, pinned (or registered) host memory is copied from directly, pageable
  // host memory goes through the context's pinned staging buffer (one more pass over it on the host)
  int rdev = -1;
  const PtrKind kind = pointer_kind(ranges, &rdev);
  if (kind == PtrKind::device && rdev != ctx->device) return fail(ctx, LSM2D_BAD_ARGUMENT, "preprocess_scans: device-resident ranges must live on the context's device");
  // (the beam directions travel in the staging buffer on every call here)
  const size_t rbytes = sizeof(float) * (size_t) nb * (size_t) n_scans, dbytes = sizeof(float2) * (size_t) nb;
  const size_t o_rng = (dbytes + 255) & ~(size_t) 255;
  rc = ensure_scratch(ctx, o_rng + (kind == PtrKind::device ? 0 : rbytes)); if (rc) return rc;
  rc = ensure_stage(ctx, o_rng + (kind == PtrKind::pageable ? rbytes : 0)); if (rc) return rc;
  Lane& L = lane(ctx);
  if (kind == PtrKind::pageable) memcpy((char*) L.h_stage + o_rng, ranges, rbytes);
  beam_dirs_host(pp, (float2*) L.h_stage);
  const PrepArgs A = make_prep_args(pp, kind == PtrKind::device ? ranges : (const float*) ((char*) L.d_scratch + o_rng), (const float2*) L.d_scratch, cs.get());
  HIPCHK(ctx, hipMemcpyAsync(L.d_scratch, L.h_stage, kind == PtrKind::pageable ? o_rng + rbytes : dbytes, hipMemcpyHostToDevice, ctx->stream));
  if (kind == PtrKind::pinned) HIPCHK(ctx, hipMemcpyAsync((char*) L.d_scratch + o_rng, ranges, rbytes, hipMemcpyHostToDevice, ctx->stream));
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  launch_preprocess_scans(A, n_scans, ctx->stream);
  HIPCHK(ctx, hipGetLastError());
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(cs->h_count.data(), cs->d_count, sizeof(int32_t) * (size_t) n_scans, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  note_timed(ctx, ctx->kernel_timing);
  cs->total = 0; for (int c = 0; c < n_scans; ++c) cs->total += cs->h_count[c];
  *out = cs.release();
  return LSM2D_SUCCESS;
}

// The same operation INTO an existing set of lsm2d_preprocess_scans (same number of scans and beams): no allocation, nothing waits -- the streaming form (a batch of
// fresh scans per step while the previous batch aligns).  The ranges are copied to a device buffer of the set's own (pinned host memory: an asynchronous DMA;
// pageable: staged through the set's pinned buffer; device memory: read in place) and preprocessed by one launch, both on the stream a batch's pre-kernels go to
// (pre_stream: the second stream while a batch is in flight).  The clouds' sizes stay on the device (the host keeps the upper bound n_beams per scan) until
// somebody asks; the set's AoS rows, if it has them, are rewritten by the same launch.
extern "C" int lsm2d_preprocess_scans_refill(lsm2d_context* ctx, const lsm2d_preprocessor* pp, const float* ranges, int32_t n_scans, lsm2d_cloudset* set) {
  if (!ctx || !pp || !ranges || !set || set->ctx != ctx || n_scans < 1) return fail(ctx, LSM2D_BAD_ARGUMENT, "preprocess_scans_refill: bad argument");
  { const int rc0 = check_preprocessor(ctx, pp, "preprocess_scans_refill"); if (rc0) return rc0; }
  const int nb = pp->n_beams;
  const int stride = nb + (nb & 1);
  if (set->n_clouds != n_scans || set->capacity > 0 || set->padded_total != (int64_t) stride * n_scans + 2 || (n_scans > 1 && set->h_start[1] != stride))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "preprocess_scans_refill: the set must come from lsm2d_preprocess_scans with the same number of scans and beams");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rdev = -1;
  const PtrKind kind = pointer_kind(ranges, &rdev);
  if (kind == PtrKind::device && rdev != ctx->device) return fail(ctx, LSM2D_BAD_ARGUMENT, "preprocess_scans_refill: device-resident ranges must live on the context's device");
  const size_t rbytes = sizeof(float) * (size_t) nb * (size_t) n_scans;
  // everything derived from the old contents goes -- except the AoS rows, which this launch rewrites in place (releasing a device buffer is a device-wide wait)
  cloudset_drop_grids(set, /* keep_aos */ true);
  if (kind != PtrKind::device && !set->d_ranges) HIPCHK(ctx, set->d_ranges.alloc(rbytes));
  const float2* d_dir = nullptr;
  { const int rc0 = beam_dirs_device(ctx, pp, &d_dir); if (rc0) return rc0; }
  const hipStream_t pre = refill_stream(ctx), cpy = refill_copy_stream(ctx, pre);
  if (set->ev_prep) HIPCHK(ctx, hipStreamWaitEvent(cpy, set->ev_prep, 0));      // (the same set refilled twice in a row: its previous launch, on the refill stream, may still read d_ranges and write the clouds)
  if (kind == PtrKind::pageable) {
    const int rc = acquire_upload_stage(set, rbytes + 16); if (rc) return rc;
    memcpy(set->h_upload, ranges, rbytes);
    HIPCHK(ctx, hipMemcpyAsync(set->d_ranges, set->h_upload, rbytes, hipMemcpyHostToDevice, cpy));
    set->staged_epoch = ctx->sync_epoch;
    if (cpy != ctx->stream) {      // (round-5 advisor: the epoch above speaks for the context's stream only)
      if (!set->ev_stage && set->ev_stage.create(hipEventDisableTiming) != hipSuccess) (void) hipGetLastError();
      if (set->ev_stage) { HIPCHK(ctx, hipEventRecord(set->ev_stage, cpy)); set->stage_on_side = true; }
      else HIPCHK(ctx, hipStreamSynchronize(cpy));
    }
  }
  else if (kind == PtrKind::pinned) HIPCHK(ctx, hipMemcpyAsync(set->d_ranges, ranges, rbytes, hipMemcpyHostToDevice, cpy));
  if (cpy != pre && kind != PtrKind::device) { HIPCHK(ctx, hipEventRecord(ctx->side_copy.ev, cpy)); HIPCHK(ctx, hipStreamWaitEvent(pre, ctx->side_copy.ev, 0)); }
  ++ctx->uploads; ctx->last_h2d_bytes = kind == PtrKind::device ? 0 : (long long) rbytes;
  PrepArgs A = make_prep_args(pp, kind == PtrKind::device ? ranges : (const float*) set->d_ranges, d_dir, set);
  A.out_aos = set->derived.d_aos;
  launch_preprocess_scans(A, n_scans, pre);
  HIPCHK(ctx, hipGetLastError());
  if (pre != ctx->stream) {
    HIPCHK(ctx, hipEventRecord(ctx->side_refill.ev, pre)); ctx->side_refill.dirty = true;      // the next aligner call waits for it (join_refill_stream)
    if (!set->ev_prep && set->ev_prep.create(hipEventDisableTiming) != hipSuccess) (void) hipGetLastError();
    if (set->ev_prep) HIPCHK(ctx, hipEventRecord(set->ev_prep, pre));
    else HIPCHK(ctx, hipStreamSynchronize(pre));      // (no event to be had: the only safe order left)
  }
  for (int c = 0; c < n_scans; ++c) set->h_count[c] = nb;      // upper bounds: the real sizes are on the device
  set->total = (int64_t) nb * n_scans; set->count_pending = true; set->unpack_pending = false; set->prep_pending = false;
  return LSM2D_SUCCESS;
}

// the live tracker's form: ONE scan into an existing reserved set, no allocation, no wait (size pending on the device)
extern "C" int lsm2d_preprocess_scan_into(lsm2d_context* ctx, const lsm2d_preprocessor* pp, const float* ranges, lsm2d_cloudset* out) {
  if (!ctx || !pp || !ranges || !out || out->ctx != ctx || out->n_clouds != 1 || out->many) return fail(ctx, LSM2D_BAD_ARGUMENT, "preprocess_scan_into: bad argument");
  { const int rc0 = check_preprocessor(ctx, pp, "preprocess_scan_into"); if (rc0) return rc0; }
  const int nb = pp->n_beams;
  const int64_t cap = out->capacity > 0 ? out->capacity : out->padded_total - 2;
  if (cap < nb) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "preprocess_scan_into: the set must have room for n_beams points");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  cloudset_drop_grids(out);
  const float2* d_dir = nullptr;
  { const int rc0 = beam_dirs_device(ctx, pp, &d_dir); if (rc0) return rc0; }
  const size_t rbytes = sizeof(float) * (size_t) nb;
  out->unpack_pending = false;                  // an upload nobody read is simply replaced
  int rc = acquire_upload_stage(out, rbytes + 16); if (rc) return rc;
  memcpy(out->h_upload, ranges, rbytes);
  const PrepArgs A = make_prep_args(pp, (const float*) out->h_upload.dev(), d_dir, out);      // the kernel reads the ranges straight from the pinned buffer: no copy, no extra launch
  out->h_count[0] = nb; out->total = nb; out->count_pending = true;          // at most one point per beam
  if (!ctx->kernel_timing) {                    // the launch is queued by the set's first reader (flush_pending / flush_preprocessing_together)
    out->prep_pending = true; out->prep_args = A;
    return LSM2D_SUCCESS;
  }
  out->prep_pending = false;
  Lane& L = lane(ctx);
  HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  hipLaunchKernelGGL(k_preprocess_scans, dim3(1), dim3(kPrepBlock), 0, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  out->staged_epoch = ctx->sync_epoch;                    // the staging buffer is free again once the kernel has run
  note_timed(ctx, true);
  return LSM2D_SUCCESS;
}

// ---- SceneClipperProjective2D ------------------------------------------------------------------------------
// vox_res > 0: the voxelize_resolution branch (mapping/scene_clipper_projective_2d.cpp:36-48) -- the clip kernels leave the cloud in the
// SENSOR frame and k_voxelize_clipped voxelises it and moves it to the robot frame
static int clip_scene_impl(lsm2d_context* ctx, const lsm2d_projector* pr, const lsm2d_cloudset* scene, int32_t si,
                           const float robot_in_local_map[3], const float sensor_in_robot[3], float vox_res, lsm2d_cloudset* clipped,
                           int32_t* out_n, int32_t* out_src) {
  if (!ctx || !pr || !robot_in_local_map || !sensor_in_robot || !clipped || !valid_cloud_index(scene, si) || clipped->n_clouds != 1 ||
      clipped == scene || clipped->many || scene->many || (!out_n && out_src))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "clip_scene: bad argument");
  const bool vox = vox_res > 0.0f;
  if (vox && out_src) return fail(ctx, LSM2D_BAD_ARGUMENT, "clip_scene: a voxelised cloud has no source indices");
  if (vox && pr->canvas_cols > kVoxMax) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "clip_scene: voxelisation takes at most 2048 columns");
  // out_n == NULL: asynchronous -- nothing comes back, the clipped set's size stays on the device until somebody asks
  if (scene->count_pending && scene->h_count[si] > 32768) { const int rc0 = resolve_count(scene); if (rc0) return rc0; }
  ProjK P;
  if (!make_projk(*pr, &P)) return fail(ctx, LSM2D_BAD_ARGUMENT, "clip_scene: bad projector");
  const int64_t cap = clipped->capacity > 0 ? clipped->capacity : clipped->padded_total - 2;
  if (cap < P.cols) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "clip_scene: clipped set smaller than canvas_cols");
  if ((int) (sizeof(u64) * (size_t) P.cols) > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "clip_scene: canvas does not fit LDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  cloudset_drop_grids(clipped);
  { const int rc0 = flush_pending(scene); if (rc0) return rc0; }
  clipped->unpack_pending = false; clipped->prep_pending = false;      // whatever was staged for the output set is replaced
  const size_t cols = (size_t) P.cols, o_src = cols * 8, o_cnt = o_src + cols * 4, bytes = o_cnt + 16;
  int rc = ensure_scratch(ctx, bytes); if (rc) return rc;
  rc = ensure_stage(ctx, bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  float cam[3], cam_inv[3];
  compose_host(robot_in_local_map, sensor_in_robot, cam); inverse_host(cam, cam_inv);
  const Iso T = make_iso(cam_inv);
  u64* d_canvas = (u64*) L.d_scratch;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  const bool small = scene->h_count[si] <= 32768;            // one workgroup, LDS canvas, one launch
  if (!small) { rc = project_split(ctx, scene->d_xy + scene->h_start[si], scene->h_count[si], T, P, d_canvas); if (rc) return rc; }
  ClipEmitArgs A;
  A.gcanvas = d_canvas; A.cols = P.cols; A.xy = scene->d_xy + scene->h_start[si]; A.nrm = scene->d_nrm + scene->h_start[si];
  A.T = T; A.S = make_iso(sensor_in_robot);
  const bool s_ident = sensor_in_robot[0] == 0.0f && sensor_in_robot[1] == 0.0f && sensor_in_robot[2] == 0.0f;
  A.s_identity = s_ident || vox;                  // voxelisation happens in the sensor frame
  // synchronous form: source indices and the count go straight to the pinned staging buffer (no device-to-host copy)
  char* dvo = (char*) (out_n ? L.h_stage.dev() : L.d_scratch);
  if (out_n) *(int32_t*) ((char*) L.h_stage + o_cnt) = kStatusNotWritten;
  A.out_xy = clipped->d_xy; A.out_nrm = clipped->d_nrm; A.out_src = (int32_t*) (dvo + o_src);
  A.out_count = vox ? (int32_t*) ((char*) L.d_scratch + o_cnt) : (int32_t*) (dvo + o_cnt);      // with voxelisation the final count is k_voxelize_clipped's
  A.out_count_dev = clipped->d_count; A.host_polls = out_n != nullptr && !vox;
  if (small) {
    ClipSmallArgs CS; CS.xy = A.xy; CS.nrm = A.nrm; CS.n = scene->h_count[si]; CS.n_dev = scene->count_pending ? scene->d_count : nullptr; CS.proj = P; CS.emit = A;
    hipLaunchKernelGGL(k_clip_small, dim3(1), dim3(kFindBlock), sizeof(u64) * (size_t) P.cols, ctx->stream, CS);
  } else {
    hipLaunchKernelGGL(k_clip_emit, dim3(1), dim3(kFindBlock), 0, ctx->stream, A);
  }
  HIPCHK(ctx, hipGetLastError());
  if (vox) {
    VoxArgs V;
    V.xy = clipped->d_xy; V.nrm = clipped->d_nrm; V.count_dev = clipped->d_count;
    V.inv_rx = 1.0f / vox_res; V.inv_rn = 1.0f / 0.1f;      // coefficients (res, res, 0.1, 0.1): scene_clipper_projective_2d.cpp:46
    V.S = make_iso(sensor_in_robot); V.s_identity = s_ident;
    V.out_count = out_n ? (int32_t*) (dvo + o_cnt) : nullptr; V.host_polls = out_n != nullptr;
    hipLaunchKernelGGL(k_voxelize_clipped, dim3(1), dim3(kVoxBlock), 0, ctx->stream, V);
    HIPCHK(ctx, hipGetLastError());
  }
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  if (!out_n) {                               // at most one point per column
    clipped->h_count[0] = P.cols; clipped->total = P.cols; clipped->count_pending = true;
    return LSM2D_SUCCESS;
  }
  HIPCHK(ctx, wait_for_statuses(ctx, (const int32_t*) ((char*) L.h_stage + o_cnt), 1));      // the kernel writes the count last
  const int32_t n = *(const int32_t*) ((char*) L.h_stage + o_cnt);
  clipped->h_count[0] = n; clipped->total = n; clipped->count_pending = false; *out_n = n;
  if (out_src) memcpy(out_src, (char*) L.h_stage + o_src, sizeof(int32_t) * (size_t) n);
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_clip_scene(lsm2d_context* ctx, const lsm2d_projector* pr, const lsm2d_cloudset* scene, int32_t si,
                                const float robot_in_local_map[3], const float sensor_in_robot[3], lsm2d_cloudset* clipped,
                                int32_t* out_n, int32_t* out_src) {
  return clip_scene_impl(ctx, pr, scene, si, robot_in_local_map, sensor_in_robot, 0.0f, clipped, out_n, out_src);
}
extern "C" int lsm2d_clip_scene_voxelized(lsm2d_context* ctx, const lsm2d_projector* pr, const lsm2d_cloudset* scene, int32_t si,
                                          const float robot_in_local_map[3], const float sensor_in_robot[3], float voxelize_resolution,
                                          lsm2d_cloudset* clipped, int32_t* out_n, int32_t* out_src) {
  return clip_scene_impl(ctx, pr, scene, si, robot_in_local_map, sensor_in_robot, voxelize_resolution, clipped, out_n, out_src);
}

// ---- MergerProjective2D ----------------------------------------------------------------------------------------
extern "C" int lsm2d_merge_scene(lsm2d_context* ctx, const lsm2d_projector* pr, lsm2d_cloudset* scene, const lsm2d_cloudset* meas,
                                 int32_t mi, const float measurement_in_scene[3], float merge_threshold, int32_t* out_size,
                                 int32_t* out_counts) {
  if (!ctx || !pr || !scene || !measurement_in_scene || !valid_cloud_index(meas, mi) || scene->n_clouds != 1 || scene->many || scene == meas || (!out_size && out_counts))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene: bad argument");
  ProjK P;
  if (!make_projk(*pr, &P)) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene: bad projector");
  const int64_t cap = scene->capacity > 0 ? scene->capacity : scene->padded_total - 2;
  // out_size == NULL: asynchronous.  Sizes only the device knows are upper bounds here; when a bound no longer settles a
  // decision (room left, single-workgroup path) it is replaced by the real number (one synchronisation)
  if (scene->count_pending && (int64_t) scene->h_count[0] + P.cols > cap) { const int rc0 = resolve_count(scene); if (rc0) return rc0; }
  // The single-workgroup path reads device-side sizes; the multi-launch path takes BOTH sizes by value (k_transform_cloud,
  // project_split, k_merge_apply), so whenever the bounds do not settle for the small path -- either set above 32 768 points, or
  // canvases beyond LDS -- every pending size is replaced by the real number first: an upper bound there would run stale slots of the
  // reserved set through the merge.
  const bool small_by_bounds = scene->h_count[0] <= 32768 && meas->h_count[mi] <= 32768 && (int) (sizeof(u64) * 2 * (size_t) P.cols) <= ctx->max_dyn_lds;
  if (!small_by_bounds) {
    int rc0 = resolve_count(scene); if (rc0) return rc0;
    rc0 = resolve_count(meas); if (rc0) return rc0;
  }
  const int n_scene = scene->h_count[0], n_meas = meas->h_count[mi];
  if ((int64_t) n_scene + P.cols > cap) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "merge_scene: scene set has no room for canvas_cols more points");
  if ((int) (sizeof(u64) * (size_t) P.cols) > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "merge_scene: canvas does not fit LDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  cloudset_drop_grids(scene);
  { int rc0 = flush_pending(scene); if (rc0) return rc0; rc0 = flush_pending(meas); if (rc0) return rc0; }
  const size_t cols = (size_t) P.cols, nm = (size_t) (n_meas > 0 ? n_meas : 1);
  const size_t o_mcan = cols * 8, o_out = o_mcan + cols * 8, o_txy = o_out + 64, o_tn = o_txy + ((nm * 8 + 15) & ~(size_t) 15) + 16, bytes = o_tn + nm * 8 + 16;
  int rc = ensure_scratch(ctx, bytes); if (rc) return rc;
  rc = ensure_stage(ctx, o_out + 64); if (rc) return rc;
  Lane& L = lane(ctx);
  float cam_inv[3]; inverse_host(measurement_in_scene, cam_inv);
  const Iso Tinv = make_iso(cam_inv), M = make_iso(measurement_in_scene);
  char* ds = (char*) L.d_scratch;
  char* dvo = out_size ? (char*) L.h_stage.dev() : ds;      // synchronous form: the four counters go straight to the pinned staging buffer
  if (out_size) *(int32_t*) ((char*) L.h_stage + o_out) = kStatusNotWritten;
  u64* d_scan = (u64*) ds; u64* d_mcan = (u64*) (ds + o_mcan);
  float2* d_txy = (float2*) (ds + o_txy); float2* d_tn = (float2*) (ds + o_tn);
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  const bool small = n_scene <= 32768 && n_meas <= 32768 && (int) (sizeof(u64) * 2 * (size_t) P.cols) <= ctx->max_dyn_lds;
  if (small) {                                               // one workgroup does the transform, both z-buffers and the column walk
    MergeSmallArgs MS;
    MS.m.scanvas = nullptr; MS.m.mcanvas = nullptr; MS.m.cols = P.cols; MS.m.sxy = scene->d_xy; MS.m.snrm = scene->d_nrm; MS.m.n_scene = n_scene;
    MS.m.mxy = meas->d_xy + meas->h_start[mi]; MS.m.mnrm = meas->d_nrm + meas->h_start[mi];
    MS.m.far_limit = 0.9f * pr->range_max; MS.m.merge_threshold = merge_threshold;
    MS.m.out = (int32_t*) (dvo + o_out); MS.m.count_dev = scene->d_count; MS.m.host_polls = out_size != nullptr;
    MS.proj = P; MS.Tinv = Tinv; MS.M = M; MS.n_meas = n_meas;
    MS.n_scene_dev = scene->count_pending ? scene->d_count : nullptr; MS.n_meas_dev = meas->count_pending ? meas->d_count + mi : nullptr;
    hipLaunchKernelGGL(k_merge_small, dim3(1), dim3(kFindBlock), sizeof(u64) * 2 * (size_t) P.cols, ctx->stream, MS);
    HIPCHK(ctx, hipGetLastError());
  } else {
  if (n_meas > 0) {
    hipLaunchKernelGGL(k_transform_cloud, dim3((unsigned) ((n_meas + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const float2*) (meas->d_xy + meas->h_start[mi]), (const float2*) (meas->d_nrm + meas->h_start[mi]), n_meas, M, d_txy, d_tn);
    HIPCHK(ctx, hipGetLastError());
  }
  rc = project_split(ctx, scene->d_xy, n_scene, Tinv, P, d_scan); if (rc) return rc;
  rc = project_split(ctx, d_txy, n_meas, Tinv, P, d_mcan); if (rc) return rc;
  MergeArgs A;
  A.scanvas = d_scan; A.mcanvas = d_mcan; A.cols = P.cols; A.sxy = scene->d_xy; A.snrm = scene->d_nrm; A.n_scene = n_scene;
  A.mxy = d_txy; A.mnrm = d_tn; A.far_limit = 0.9f * pr->range_max; A.merge_threshold = merge_threshold;
  A.out = (int32_t*) (dvo + o_out); A.count_dev = scene->d_count; A.host_polls = out_size != nullptr;
  hipLaunchKernelGGL(k_merge_apply, dim3(1), dim3(kFindBlock), 0, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  }
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  if (!out_size) {                            // a merge appends at most one point per column
    scene->h_count[0] = n_scene + P.cols; scene->total = scene->h_count[0]; scene->count_pending = true;
    return LSM2D_SUCCESS;
  }
  HIPCHK(ctx, wait_for_statuses(ctx, (const int32_t*) ((char*) L.h_stage + o_out), 1));      // the kernel writes the new size last
  const int32_t* h = (const int32_t*) ((char*) L.h_stage + o_out);
  scene->h_count[0] = h[0]; scene->total = h[0]; scene->count_pending = false; *out_size = h[0];
  if (out_counts) { out_counts[0] = h[1]; out_counts[1] = h[2]; out_counts[2] = h[3]; }
  return LSM2D_SUCCESS;
}


// several measurements into one scene, in order: ONE launch when everything is small (the live tracker's two scans), else the
// calls one by one -- the same result either way
extern "C" int lsm2d_merge_scenes(lsm2d_context* ctx, const lsm2d_projector* pr, lsm2d_cloudset* scene, int32_t n_measurements,
                                  const lsm2d_cloudset* const* meas, const int32_t* meas_index, const float* measurement_in_scene,
                                  float merge_threshold, int32_t* out_size, int32_t* out_counts) {
  if (!ctx || !pr || !scene || !meas || !measurement_in_scene || n_measurements < 1 || scene->n_clouds != 1 || scene->many || (!out_size && out_counts))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scenes: bad argument");
  for (int k = 0; k < n_measurements; ++k)
    if (!valid_cloud_index(meas[k], meas_index ? meas_index[k] : 0) || meas[k] == scene) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scenes: bad measurement");
  ProjK P;
  if (!make_projk(*pr, &P)) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scenes: bad projector");
  const int64_t cap = scene->capacity > 0 ? scene->capacity : scene->padded_total - 2;
  const int n = n_measurements;
  bool together = n >= 2 && n <= kMergeMulti && (int) (sizeof(u64) * 2 * (size_t) P.cols) <= ctx->max_dyn_lds && !ctx->kernel_timing;
  if (together && scene->count_pending && (int64_t) scene->h_count[0] + (int64_t) n * P.cols > cap) { const int rc0 = resolve_count(scene); if (rc0) return rc0; }
  together = together && (int64_t) scene->h_count[0] + (int64_t) n * P.cols <= cap && (int64_t) scene->h_count[0] + (int64_t) (n - 1) * P.cols <= 32768;
  for (int k = 0; k < n && together; ++k) together = meas[k]->h_count[meas_index ? meas_index[k] : 0] <= 32768;
  if (!together) {                            // one by one (large scenes, one measurement, timed launches)
    for (int k = 0; k < n; ++k) {
      int32_t size = 0;
      const int rc = lsm2d_merge_scene(ctx, pr, scene, meas[k], meas_index ? meas_index[k] : 0, measurement_in_scene + 3 * k, merge_threshold,
                                       out_size ? &size : nullptr, out_counts ? out_counts + 3 * k : nullptr);
      if (rc) return rc;
      if (out_size) *out_size = size;
    }
    return LSM2D_SUCCESS;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  cloudset_drop_grids(scene);
  { const int rc0 = flush_pending(scene); if (rc0) return rc0; }
  for (int k = 0; k < n; ++k) { const int rc0 = flush_pending(meas[k]); if (rc0) return rc0; }
  const size_t cols = (size_t) P.cols, o_out = 0, bytes = 16 * (size_t) n + 64;
  int rc = ensure_scratch(ctx, bytes); if (rc) return rc;
  rc = ensure_stage(ctx, bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  char* dvo = (char*) (out_size ? L.h_stage.dev() : L.d_scratch);         // synchronous form: the counters go straight to the pinned staging buffer, the last size last
  if (out_size) { *(int32_t*) ((char*) L.h_stage + o_out + 16 * (size_t) (n - 1)) = kStatusNotWritten; }
  MergeMultiArgs MM; MM.n = n;
  for (int k = 0; k < n; ++k) {
    const lsm2d_cloudset* ms = meas[k]; const int mi = meas_index ? meas_index[k] : 0;
    const float* mis = measurement_in_scene + 3 * k;
    float cam_inv[3]; inverse_host(mis, cam_inv);
    MergeSmallArgs& MS = MM.a[k];
    MS.m.scanvas = nullptr; MS.m.mcanvas = nullptr; MS.m.cols = P.cols; MS.m.sxy = scene->d_xy; MS.m.snrm = scene->d_nrm; MS.m.n_scene = scene->h_count[0];
    MS.m.mxy = ms->d_xy + ms->h_start[mi]; MS.m.mnrm = ms->d_nrm + ms->h_start[mi];
    MS.m.far_limit = 0.9f * pr->range_max; MS.m.merge_threshold = merge_threshold;
    MS.m.out = (int32_t*) (dvo + o_out + 16 * (size_t) k); MS.m.count_dev = scene->d_count; MS.m.host_polls = out_size != nullptr && k == n - 1;
    MS.proj = P; MS.Tinv = make_iso(cam_inv); MS.M = make_iso(mis); MS.n_meas = ms->h_count[mi];
    MS.n_scene_dev = scene->count_pending ? scene->d_count : nullptr; MS.n_meas_dev = ms->count_pending ? ms->d_count + mi : nullptr;
  }
  for (int k = n; k < kMergeMulti; ++k) MM.a[k] = MM.a[0];
  hipLaunchKernelGGL(k_merge_multi, dim3(1), dim3(kFindBlock), sizeof(u64) * 2 * cols, ctx->stream, MM);
  HIPCHK(ctx, hipGetLastError());
  ctx->have_timing = false;
  if (!out_size) {                            // every merge appends at most one point per column
    scene->h_count[0] = scene->h_count[0] + n * P.cols; scene->total = scene->h_count[0]; scene->count_pending = true;
    return LSM2D_SUCCESS;
  }
  HIPCHK(ctx, wait_for_statuses(ctx, (const int32_t*) ((char*) L.h_stage + o_out + 16 * (size_t) (n - 1)), 1));
  const int32_t* h = (const int32_t*) ((char*) L.h_stage + o_out);
  scene->h_count[0] = h[4 * (n - 1)]; scene->total = scene->h_count[0]; scene->count_pending = false; *out_size = scene->h_count[0];
  if (out_counts) for (int k = 0; k < n; ++k) { out_counts[3 * k] = h[4 * k + 1]; out_counts[3 * k + 1] = h[4 * k + 2]; out_counts[3 * k + 2] = h[4 * k + 3]; }
  return LSM2D_SUCCESS;
}

// ---- N independent trackers per call: batched clipper and merger ------------------------------------------------------------------
// The per-tracker arguments go to the OUTPUT set's own pinned buffer (acquire_upload_stage: it waits only when the set's previous batch has not
// been waited for since -- in a tracker step the aligner's wait comes in between), which the kernel reads directly: nothing else is staged, so
// an asynchronous call leaves nothing behind in the context's staging buffer that a later call could overwrite under it.
// vox_res > 0: the voxelize_resolution branch (mapping/scene_clipper_projective_2d.cpp:36-48) inside the same launch -- k_clip_vox_batch keeps the clipped
// cloud in LDS, voxelises it in the SENSOR frame and writes only the voxels, moved to the robot frame
static int clip_scene_batch_impl(lsm2d_context* ctx, const lsm2d_projector* pr, const lsm2d_cloudset* scenes, int32_t n,
                                 const int32_t* scene_index, const float* robot_in_local_map, const float sensor_in_robot[3],
                                 float vox_res, lsm2d_cloudset* clipped, int32_t* out_n) {
  if (!ctx || !pr || !scenes || !robot_in_local_map || !sensor_in_robot || !clipped || n < 1 || scenes == clipped ||
      scenes->ctx != ctx || clipped->ctx != ctx || !clipped->many || clipped->n_clouds < n)
    return fail(ctx, LSM2D_BAD_ARGUMENT, "clip_scene_batch: bad argument (clipped: a reserved-many set of >= n_trackers clouds, not the scenes' set)");
  for (int i = 0; i < n; ++i)
    if (!valid_cloud_index(scenes, scene_index ? scene_index[i] : i)) return fail(ctx, LSM2D_BAD_ARGUMENT, "clip_scene_batch: scene index out of range");
  ProjK P;
  if (!make_projk(*pr, &P)) return fail(ctx, LSM2D_BAD_ARGUMENT, "clip_scene_batch: bad projector");
  const bool vox = vox_res > 0.0f;
  if (vox && P.cols > kVoxMax) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "clip_scene_batch: voxelisation takes at most 2048 columns");
  if (clipped->capacity < P.cols) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "clip_scene_batch: clipped clouds smaller than canvas_cols");
  if ((int) (sizeof(u64) * (size_t) P.cols) + 512 > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "clip_scene_batch: canvas does not fit LDS");
  // (k_clip_vox_batch's LDS is static: points, normals and keys at kVoxMax entries, the canvas aliased onto the keys)
  if (vox && (int) (3 * sizeof(u64) * (size_t) kVoxMax) + 512 > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "clip_scene_batch: the voxelising workgroup does not fit LDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  { const int rc0 = flush_pending(scenes); if (rc0) return rc0; }
  HIPCHK(ctx, join_refill_stream(ctx, ctx->stream));
  int rc = acquire_upload_stage(clipped, sizeof(ClipBatchItem) * (size_t) n + 16); if (rc) return rc;
  if (out_n) { rc = ensure_stage(ctx, sizeof(int32_t) * (size_t) n + 16); if (rc) return rc; }
  cloudset_drop_grids(clipped);
  ClipBatchItem* items = (ClipBatchItem*) clipped->h_upload;
  for (int i = 0; i < n; ++i) {      // the single call's transform (clip_scene_impl), per tracker
    const int si = scene_index ? scene_index[i] : i;
    float cam[3], cam_inv[3];
    compose_host(robot_in_local_map + 3 * i, sensor_in_robot, cam); inverse_host(cam, cam_inv);
    items[i].T = make_iso(cam_inv); items[i].start = scenes->h_start[si]; items[i].n = scenes->count_pending ? -1 : scenes->h_count[si]; items[i].si = si; items[i].pad = 0;
  }
  ClipBatchArgs A;
  A.xy = scenes->d_xy; A.nrm = scenes->d_nrm; A.scene_count_dev = scenes->d_count; A.items = (const ClipBatchItem*) clipped->h_upload.dev();
  A.proj = P; A.S = make_iso(sensor_in_robot);
  A.s_identity = sensor_in_robot[0] == 0.0f && sensor_in_robot[1] == 0.0f && sensor_in_robot[2] == 0.0f;
  A.out_xy = clipped->d_xy; A.out_nrm = clipped->d_nrm; A.out_stride = clipped->n_clouds > 1 ? clipped->h_start[1] : 0; A.out_count_dev = clipped->d_count;
  A.host_polls = out_n != nullptr; A.out_count = nullptr;
  Lane& L = lane(ctx);
  int32_t* h_out = (int32_t*) L.h_stage;
  if (out_n) {
    A.out_count = (int32_t*) L.h_stage.dev();
    for (int i = 0; i < n; ++i) h_out[i] = kStatusNotWritten;
  }
  if (vox) {
    ClipVoxBatchArgs V; V.c = A;
    V.inv_rx = 1.0f / vox_res; V.inv_rn = 1.0f / 0.1f;      // coefficients (res, res, 0.1, 0.1): scene_clipper_projective_2d.cpp:46
    hipLaunchKernelGGL(k_clip_vox_batch, dim3((unsigned) n), dim3(kVoxBlock), 0, ctx->stream, V);
  } else {
    hipLaunchKernelGGL(k_clip_batch, dim3((unsigned) n), dim3(kFindBlock), sizeof(u64) * (size_t) P.cols, ctx->stream, A);
  }
  HIPCHK(ctx, hipGetLastError());
  clipped->staged_epoch = ctx->sync_epoch;
  ctx->have_timing = false;
  if (!out_n) {                               // at most one point per column (a voxelised cloud never grows)
    for (int i = 0; i < n; ++i) { clipped->total += (int64_t) P.cols - clipped->h_count[i]; clipped->h_count[i] = P.cols; }
    clipped->count_pending = true;
    return LSM2D_SUCCESS;
  }
  HIPCHK(ctx, wait_for_statuses(ctx, h_out, n));      // every workgroup writes its count last
  // (exact sizes now for clouds 0 .. n; a set whose other clouds' sizes were pending stays pending: their numbers are still upper bounds)
  for (int i = 0; i < n; ++i) { clipped->total += (int64_t) h_out[i] - clipped->h_count[i]; clipped->h_count[i] = h_out[i]; out_n[i] = h_out[i]; }
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_clip_scene_batch(lsm2d_context* ctx, const lsm2d_projector* pr, const lsm2d_cloudset* scenes, int32_t n,
                                      const int32_t* scene_index, const float* robot_in_local_map, const float sensor_in_robot[3],
                                      lsm2d_cloudset* clipped, int32_t* out_n) {
  return clip_scene_batch_impl(ctx, pr, scenes, n, scene_index, robot_in_local_map, sensor_in_robot, 0.0f, clipped, out_n);
}
// voxelize_resolution <= 0: lsm2d_clip_scene_batch itself
extern "C" int lsm2d_clip_scene_voxelized_batch(lsm2d_context* ctx, const lsm2d_projector* pr, const lsm2d_cloudset* scenes, int32_t n,
                                                const int32_t* scene_index, const float* robot_in_local_map, const float sensor_in_robot[3],
                                                float voxelize_resolution, lsm2d_cloudset* clipped, int32_t* out_n) {
  return clip_scene_batch_impl(ctx, pr, scenes, n, scene_index, robot_in_local_map, sensor_in_robot, voxelize_resolution, clipped, out_n);
}

extern "C" int lsm2d_merge_scene_batch(lsm2d_context* ctx, const lsm2d_projector* pr, lsm2d_cloudset* scenes, int32_t n,
                                       const int32_t* scene_index, int32_t n_measurements, const lsm2d_cloudset* const* meas,
                                       const int32_t* meas_index, const float* measurement_in_scene, float merge_threshold,
                                       int32_t* out_sizes, int32_t* out_counts) {
  if (!ctx || !pr || !scenes || !meas || !measurement_in_scene || n < 1 || n_measurements < 1 || n_measurements > kMergeMulti ||
      scenes->ctx != ctx || !scenes->many || (!out_sizes && out_counts))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene_batch: bad argument (scenes: a reserved-many set; 1 <= n_measurements <= 4)");
  const int nm = n_measurements;
  for (int k = 0; k < nm; ++k) {
    if (!meas[k] || meas[k] == scenes || meas[k]->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene_batch: bad measurement set");
    for (int i = 0; i < n; ++i)
      if (!valid_cloud_index(meas[k], meas_index ? meas_index[(size_t) k * n + i] : i)) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene_batch: measurement index out of range");
  }
  {   // every scene once
    std::vector<char> seen((size_t) scenes->n_clouds, 0);
    for (int i = 0; i < n; ++i) {
      const int si = scene_index ? scene_index[i] : i;
      if (!valid_cloud_index(scenes, si)) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene_batch: scene index out of range");
      if (seen[(size_t) si]) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene_batch: a scene index appears twice");
      seen[(size_t) si] = 1;
    }
  }
  ProjK P;
  if (!make_projk(*pr, &P)) return fail(ctx, LSM2D_BAD_ARGUMENT, "merge_scene_batch: bad projector");
  if ((int) (sizeof(u64) * 2 * (size_t) P.cols) + 512 > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "merge_scene_batch: canvases do not fit LDS");
  // all or nothing: upper bounds first, the real sizes (one wait) only when a bound does not settle it
  const int64_t cap = scenes->capacity, grow = (int64_t) nm * P.cols;
  for (int pass = 0; pass < 2; ++pass) {
    int short_of_room = -1;
    for (int i = 0; i < n && short_of_room < 0; ++i) if ((int64_t) scenes->h_count[scene_index ? scene_index[i] : i] + grow > cap) short_of_room = i;
    if (short_of_room < 0) break;
    if (pass == 0 && scenes->count_pending) { const int rc0 = resolve_count(scenes); if (rc0) return rc0; continue; }
    char msg[160];
    snprintf(msg, sizeof msg, "merge_scene_batch: the scene of tracker %d (cloud %d) has no room for n_measurements * canvas_cols more points", short_of_room,
             scene_index ? scene_index[short_of_room] : short_of_room);
    return fail(ctx, LSM2D_CAPACITY_EXCEEDED, msg);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (int k = 0; k < nm; ++k) { const int rc0 = flush_pending(meas[k]); if (rc0) return rc0; }
  HIPCHK(ctx, join_refill_stream(ctx, ctx->stream));
  const size_t o_items = ((sizeof(int4) * (size_t) n) + 15) & ~(size_t) 15;
  int rc = acquire_upload_stage(scenes, o_items + sizeof(MergeBatchItem) * (size_t) n * nm + 16); if (rc) return rc;
  const size_t out_bytes = sizeof(int32_t) * 4 * (size_t) n * nm;
  rc = ensure_scratch(ctx, out_bytes + 16); if (rc) return rc;
  if (out_sizes) { rc = ensure_stage(ctx, out_bytes + 16); if (rc) return rc; }
  cloudset_drop_grids(scenes);
  int4* hs = (int4*) scenes->h_upload;
  MergeBatchItem* items = (MergeBatchItem*) ((char*) scenes->h_upload + o_items);
  for (int i = 0; i < n; ++i) {
    const int si = scene_index ? scene_index[i] : i;
    hs[i] = make_int4(scenes->h_start[si], scenes->count_pending ? -1 : scenes->h_count[si], si, 0);
    for (int k = 0; k < nm; ++k) {      // lsm2d_merge_scenes' transforms, per tracker and measurement
      const lsm2d_cloudset* ms = meas[k]; const int mi = meas_index ? meas_index[(size_t) k * n + i] : i;
      const float* mis = measurement_in_scene + 3 * ((size_t) i * nm + k);
      float cam_inv[3]; inverse_host(mis, cam_inv);
      MergeBatchItem& it = items[(size_t) i * nm + k];
      it.Tinv = make_iso(cam_inv); it.M = make_iso(mis); it.mstart = ms->h_start[mi]; it.n_meas = ms->count_pending ? -1 : ms->h_count[mi]; it.mc = mi; it.pad = 0;
    }
  }
  MergeBatchArgs A;
  A.sxy = scenes->d_xy; A.snrm = scenes->d_nrm; A.scene_count_dev = scenes->d_count;
  A.scenes = (const int4*) scenes->h_upload.dev(); A.items = (const MergeBatchItem*) ((char*) scenes->h_upload.dev() + o_items);
  for (int k = 0; k < kMergeMulti; ++k) {
    const lsm2d_cloudset* ms = meas[k < nm ? k : 0];
    A.mxy[k] = ms->d_xy; A.mnrm[k] = ms->d_nrm; A.mcount_dev[k] = ms->d_count;
  }
  A.proj = P; A.far_limit = 0.9f * pr->range_max; A.merge_threshold = merge_threshold; A.n_meas = nm;
  A.host_polls = out_sizes != nullptr;
  Lane& L = lane(ctx);
  const int32_t* h_out = (const int32_t*) L.h_stage;
  if (out_sizes) {
    A.out = (int32_t*) L.h_stage.dev();
    for (int i = 0; i < n; ++i) ((int32_t*) L.h_stage)[4 * ((size_t) i * nm + nm - 1)] = kStatusNotWritten;
  } else {
    A.out = (int32_t*) L.d_scratch;
  }
  hipLaunchKernelGGL(k_merge_batch, dim3((unsigned) n), dim3(kFindBlock), sizeof(u64) * 2 * (size_t) P.cols, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  scenes->staged_epoch = ctx->sync_epoch;
  ctx->have_timing = false;
  if (!out_sizes) {                           // every merge appends at most one point per column
    for (int i = 0; i < n; ++i) { const int si = scene_index ? scene_index[i] : i; scenes->h_count[si] += (int32_t) grow; scenes->total += grow; }
    scenes->count_pending = true;
    return LSM2D_SUCCESS;
  }
  // every tracker's last new size, each written last by its workgroup: polled one after the other (a stride of n_measurements counters)
  for (int i = 0; i < n; ++i) HIPCHK(ctx, wait_for_statuses(ctx, h_out + 4 * ((size_t) i * nm + nm - 1), 1));
  // (exact sizes now for the scenes merged into; a set whose other clouds' sizes were pending stays pending)
  for (int i = 0; i < n; ++i) {
    const int si = scene_index ? scene_index[i] : i;
    const int32_t* h = h_out + 4 * ((size_t) i * nm);
    scenes->total += (int64_t) h[4 * (nm - 1)] - scenes->h_count[si]; scenes->h_count[si] = h[4 * (nm - 1)]; out_sizes[i] = h[4 * (nm - 1)];
    if (out_counts) for (int k = 0; k < nm; ++k) { out_counts[3 * ((size_t) i * nm + k)] = h[4 * k + 1]; out_counts[3 * ((size_t) i * nm + k) + 1] = h[4 * k + 2]; out_counts[3 * ((size_t) i * nm + k) + 2] = h[4 * k + 3]; }
  }
  return LSM2D_SUCCESS;
}

// ---- a3 ------------------------------------------------------------------------------------------------
extern "C" int lsm2d_project(lsm2d_context* ctx, const lsm2d_projector* pr, const lsm2d_cloudset* cloud, int32_t ci,
                             const float pose[3], int32_t* out_src, float* out_depth, float* out_xynn) {
  if (!ctx || !pr || !pose || !valid_cloud_index(cloud, ci)) return fail(ctx, LSM2D_BAD_ARGUMENT, "project: bad argument");
  { int rc0 = resolve_count(cloud); if (rc0) return rc0; rc0 = flush_pending(cloud); if (rc0) return rc0; }
  ProjectArgs A;
  if (!make_projk(*pr, &A.proj)) return fail(ctx, LSM2D_BAD_ARGUMENT, "project: bad projector");
  const size_t lds = sizeof(u64) * (size_t) A.proj.cols;
  if ((int) lds > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "project: canvas does not fit LDS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t cols = (size_t) A.proj.cols, bytes = cols * (4 + 4 + 16);
  int rc = ensure_scratch(ctx, bytes); if (rc) return rc;
  rc = ensure_stage(ctx, bytes); if (rc) return rc;
  Lane& L = lane(ctx);
  A.cloud = cloud_dev(cloud, nullptr); A.ci = ci; A.T = make_iso(pose);
  char* dv = (char*) L.h_stage.dev();       // the canvas rows go straight to pinned host memory
  A.out_xynn = (float4*) dv;
  A.out_src = (int32_t*) (dv + cols * 16);
  A.out_depth = (float*) (dv + cols * 20);
  hipLaunchKernelGGL(k_project_canvas, dim3(1), dim3(kFindBlock), lds, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, stream_sync(ctx));
  if (out_xynn) memcpy(out_xynn, L.h_stage, cols * 16);
  if (out_src) memcpy(out_src, (char*) L.h_stage + cols * 16, cols * 4);
  if (out_depth) memcpy(out_depth, (char*) L.h_stage + cols * 20, cols * 4);
  return LSM2D_SUCCESS;
}
