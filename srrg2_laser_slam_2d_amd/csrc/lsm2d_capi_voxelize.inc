// lsm2d_capi_voxelize.inc -- PointCloud::voxelize over device-resident clouds of any size: several inputs, each moved by a pose, voxelised per group into
// the clouds of a reserved set in ONE call (lsm2d_voxelize, include/lsm2d.h; PARITY.md section 3, item 17b).  Part of lsm2d_capi.hip.
//
//   up          the call's tables -- per input (transform, start, group), the concatenation offsets, per group (destination start, room, cloud) -- through the
//               lane's pinned staging buffer into its scratch: one copy
//   the chain   k_vox_keys; per digit k_vox_hist, k_vox_scan, k_vox_scatter; k_vox_head_count, k_vox_scan, k_vox_head_write; k_vox_sum; k_vox_verdict;
//               k_vox_write; k_vox_finish -- on the context's stream in order, every dependency a launch boundary
//   down        [counts | dropped | verdict, heads]: ONE copy, ONE wait
// The lane's scratch is sized ONCE before the first launch.  The source clouds are read by k_vox_keys alone and the destination clouds are written by
// k_vox_write / k_vox_finish alone, behind the verdict: dst may be src, and a refused result leaves every destination cloud as it was.  What the destination
// set carries derived from its points is dropped with cloudset_drop_grids, the call lsm2d_merge_scene makes -- but AFTER the wait and only when the call has
// succeeded, where lsm2d_merge_scene drops before it launches: a result that does not fit changes no point, so it must not cost the set its search structures
// either, and the call is synchronous, so nobody can see the difference in order.

struct VoxelizeLayout {
  size_t n = 0, n_tiles = 0, n_inputs = 0, n_groups = 0;
  // the block that travels up (the same offsets in the staging buffer and in the scratch)
  size_t u_inputs = 0, u_offset = 0, u_groups = 0, up_bytes = 0;
  // the block that travels down, and the words cleared with it
  size_t o_down = 0, d_counts = 0, d_dropped = 0, d_misc = 0, down_bytes = 0;
  size_t o_first = 0, o_last = 0, o_txy = 0, o_tn = 0, o_key[2] = {}, o_idx[2] = {}, o_hist = 0, o_tile_heads = 0, o_head_pos = 0, o_vxy = 0, o_vn = 0, bytes = 0;
  VoxelizeLayout(size_t n_, size_t n_inputs_, size_t n_groups_) {
    n = n_; n_inputs = n_inputs_; n_groups = n_groups_;
    n_tiles = n ? (n + kVoxTile - 1) / kVoxTile : 1;
    const size_t np = n ? n : 1;
    u_inputs = 0; u_offset = up256(sizeof(VoxInput) * n_inputs); u_groups = up256(u_offset + sizeof(int32_t) * (n_inputs + 1));
    up_bytes = up256(u_groups + sizeof(VoxGroup) * n_groups);
    o_down = up_bytes;
    d_counts = 0; d_dropped = sizeof(int32_t) * n_groups; d_misc = 2 * sizeof(int32_t) * n_groups; down_bytes = d_misc + 4 * sizeof(int32_t);
    size_t o = up256(o_down + down_bytes);
    o_first = o; o = up256(o + sizeof(int32_t) * n_groups);
    o_last = o; o = up256(o + sizeof(int32_t) * n_groups);
    o_txy = o; o = up256(o + sizeof(float2) * np);
    o_tn = o; o = up256(o + sizeof(float2) * np);
    for (int p = 0; p < 2; ++p) { o_key[p] = o; o = up256(o + sizeof(u64) * np); o_idx[p] = o; o = up256(o + sizeof(uint32_t) * np); }
    o_hist = o; o = up256(o + sizeof(uint32_t) * 256 * n_tiles);
    o_tile_heads = o; o = up256(o + sizeof(uint32_t) * n_tiles);
    o_head_pos = o; o = up256(o + sizeof(uint32_t) * np);
    o_vxy = o; o = up256(o + sizeof(float2) * np);
    o_vn = o; o = up256(o + sizeof(float2) * np);
    bytes = o;
  }
};

extern "C" int lsm2d_voxelize(lsm2d_context* ctx, const lsm2d_voxelize_params* params, const lsm2d_cloudset* src, int32_t n_inputs, const int32_t* src_index,
                              const float* pose, const int32_t* group, int32_t n_groups, lsm2d_cloudset* dst, const int32_t* dst_index, int32_t* out_counts,
                              int32_t* out_dropped) {
  static_assert(LSM2D_VOXELIZE_MAX_POINTS == kVoxMaxPoints && LSM2D_VOXELIZE_MAX_GROUPS == kVoxMaxGroups, "the ABI's limits are the kernels'");
  // ---- refusals: nothing is launched or written before the last of them
  if (!ctx || !params || !src || !dst || !out_counts) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: null argument");
  if (src->ctx != ctx || dst->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: cloud set from another (or a destroyed) context");
  if (!(params->resolution > 0.0f) || !std::isfinite(params->resolution) || !(params->normal_resolution > 0.0f) || !std::isfinite(params->normal_resolution))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: resolution and normal_resolution must be finite and > 0");
  if (n_inputs < 1) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: n_inputs must be >= 1");
  if (n_groups < 1) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: n_groups must be >= 1");
  if (n_groups > kVoxMaxGroups) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: more groups than LSM2D_VOXELIZE_MAX_GROUPS");
  if (dst->capacity <= 0) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: dst must be a reserved set (lsm2d_cloudset_create_reserved / _reserved_many)");
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  for (int32_t k = 0; k < n_inputs; ++k) {
    if (!valid_cloud_index(src, src_index ? src_index[k] : k)) return failf(ctx, LSM2D_BAD_ARGUMENT, "voxelize: input %d: cloud index outside the source set", (int) k);
    if (group && (group[k] < 0 || group[k] >= n_groups)) return failf(ctx, LSM2D_BAD_ARGUMENT, "voxelize: input %d: group outside [0, n_groups)", (int) k);
  }
  {   // every destination cloud once
    std::vector<char> seen((size_t) dst->n_clouds, 0);
    for (int32_t g = 0; g < n_groups; ++g) {
      const int32_t ci = dst_index ? dst_index[g] : g;
      if (!valid_cloud_index(dst, ci)) return failf(ctx, LSM2D_BAD_ARGUMENT, "voxelize: group %d: cloud index outside the destination set", (int) g);
      if (seen[(size_t) ci]) return failf(ctx, LSM2D_BAD_ARGUMENT, "voxelize: group %d: its destination cloud appears twice", (int) g);
      seen[(size_t) ci] = 1;
    }
  }
  // sizes the device alone knows are upper bounds on the host: a sum of bounds within the limit settles it, else the real sizes are fetched (the one wait
  // lsm2d_merge_scene_batch allows itself) -- and they are fetched anyway before the tables are made, which hold exact offsets
  long long total = 0;
  for (int32_t k = 0; k < n_inputs; ++k) total += src->h_count[(size_t) (src_index ? src_index[k] : k)];
  if (total > kVoxMaxPoints && !src->count_pending) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: more input points than LSM2D_VOXELIZE_MAX_POINTS");
  { int rc0 = resolve_count(src); if (rc0) return rc0; rc0 = resolve_count(dst); if (rc0) return rc0; }
  total = 0;
  for (int32_t k = 0; k < n_inputs; ++k) total += src->h_count[(size_t) (src_index ? src_index[k] : k)];
  if (total > kVoxMaxPoints) return fail(ctx, LSM2D_BAD_ARGUMENT, "voxelize: more input points than LSM2D_VOXELIZE_MAX_POINTS");
  // ---- from here on the call launches
  HIPCHK(ctx, hipSetDevice(ctx->device));
  { int rc0 = flush_pending(src); if (rc0) return rc0; rc0 = flush_pending(dst); if (rc0) return rc0; }      // an upload still in its pinned buffer would land on top of the result
  HIPCHK(ctx, join_refill_stream(ctx, ctx->stream));
  const VoxelizeLayout Y((size_t) total, (size_t) n_inputs, (size_t) n_groups);
  { int rc = ensure_scratch(ctx, Y.bytes); if (rc) return rc; rc = ensure_stage(ctx, std::max(Y.up_bytes, Y.down_bytes)); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const ds = (char*) L.d_scratch; char* const hs = (char*) L.h_stage;
  {
    VoxInput* hin = (VoxInput*) (hs + Y.u_inputs); int32_t* hoff = (int32_t*) (hs + Y.u_offset); VoxGroup* hg = (VoxGroup*) (hs + Y.u_groups);
    int32_t o = 0;
    for (int32_t k = 0; k < n_inputs; ++k) {
      const int32_t ci = src_index ? src_index[k] : k;
      VoxInput& in = hin[k];
      if (pose) in.T = make_iso(pose + 3 * (size_t) k); else { in.T.c = 1.0f; in.T.s = 0.0f; in.T.tx = 0.0f; in.T.ty = 0.0f; }
      in.start = src->h_start[(size_t) ci]; in.group = group ? group[k] : 0; in.has_pose = pose != nullptr; in.pad = 0;
      hoff[k] = o; o += src->h_count[(size_t) ci];
    }
    hoff[n_inputs] = o;
    for (int32_t g = 0; g < n_groups; ++g) {
      const int32_t ci = dst_index ? dst_index[g] : g;
      hg[g].start = dst->h_start[(size_t) ci]; hg[g].cap = (int32_t) std::min<int64_t>(dst->capacity, 0x7fffffff); hg[g].cloud = ci; hg[g].pad = 0;
    }
  }
  const int n = (int) total, n_tiles = (int) Y.n_tiles;
  int gb = 0; while ((1 << gb) < n_groups) ++gb;
  const int sort_bits = kVoxKeyBits + gb + 1, n_digits = (sort_bits + 7) / 8;      // (+ 1: the dropped points' all-ones key sorts behind every group)
  const unsigned pt_blocks = (unsigned) ((std::max(n, 1) + 255) / 256), tile_blocks = (unsigned) ((n_tiles + kVoxSortBlock / 64 - 1) / (kVoxSortBlock / 64));
  const unsigned group_blocks = (unsigned) ((n_groups + 255) / 256);
  int32_t* const d_misc = (int32_t*) (ds + Y.o_down + Y.d_misc);      // [verdict, heads, fault, 0]
  // ---- the timing bracket of the whole call
  ctx->have_timing = false;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ds, hs, Y.up_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ds + Y.o_down, 0, (Y.o_last - Y.o_down), ctx->stream));      // counts, dropped, verdict, heads, group_first: 0
  HIPCHK(ctx, hipMemsetAsync(ds + Y.o_last, 0xFF, sizeof(int32_t) * (size_t) n_groups, ctx->stream));      // group_last: -1
  int final_buf = 0;
  if (n > 0) {
    VoxKeysArgs K;
    K.xy = src->d_xy; K.nrm = src->d_nrm; K.inputs = (const VoxInput*) (ds + Y.u_inputs); K.offset = (const int32_t*) (ds + Y.u_offset);
    K.n_inputs = n_inputs; K.n = n; K.inv_res = 1.0f / params->resolution; K.inv_rn = 1.0f / params->normal_resolution;
    K.txy = (float2*) (ds + Y.o_txy); K.tn = (float2*) (ds + Y.o_tn); K.key = (u64*) (ds + Y.o_key[0]); K.idx = (uint32_t*) (ds + Y.o_idx[0]);
    K.dropped = (int32_t*) (ds + Y.o_down + Y.d_dropped);
    hipLaunchKernelGGL(k_vox_keys, dim3(pt_blocks), dim3(256), 0, ctx->stream, K);
    HIPCHK(ctx, hipGetLastError());
    for (int d = 0; d < n_digits; ++d) {
      VoxSortArgs S;
      S.key_in = (const u64*) (ds + Y.o_key[final_buf]); S.idx_in = (const uint32_t*) (ds + Y.o_idx[final_buf]);
      S.key_out = (u64*) (ds + Y.o_key[final_buf ^ 1]); S.idx_out = (uint32_t*) (ds + Y.o_idx[final_buf ^ 1]);
      S.hist = (uint32_t*) (ds + Y.o_hist); S.n = n; S.n_tiles = n_tiles; S.shift = 8 * d; S.fault = d_misc + 2;
      hipLaunchKernelGGL(k_vox_hist, dim3(tile_blocks), dim3(kVoxSortBlock), 0, ctx->stream, S);
      VoxScanArgs C; C.data = S.hist; C.n = 256 * n_tiles; C.total = nullptr;
      hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(kVoxScanBlock), 0, ctx->stream, C);
      hipLaunchKernelGGL(k_vox_scatter, dim3(tile_blocks), dim3(kVoxSortBlock), 0, ctx->stream, S);
      HIPCHK(ctx, hipGetLastError());
      final_buf ^= 1;
    }
    VoxHeadArgs H;
    H.key = (const u64*) (ds + Y.o_key[final_buf]); H.tile_heads = (uint32_t*) (ds + Y.o_tile_heads); H.n = n; H.n_tiles = n_tiles;
    H.head_pos = (uint32_t*) (ds + Y.o_head_pos); H.group_first = (int32_t*) (ds + Y.o_first); H.fault = d_misc + 2;
    hipLaunchKernelGGL(k_vox_head_count, dim3(tile_blocks), dim3(kVoxSortBlock), 0, ctx->stream, H);
    VoxScanArgs C; C.data = H.tile_heads; C.n = n_tiles; C.total = d_misc + 1;
    hipLaunchKernelGGL(k_vox_scan, dim3(1), dim3(kVoxScanBlock), 0, ctx->stream, C);
    hipLaunchKernelGGL(k_vox_head_write, dim3(tile_blocks), dim3(kVoxSortBlock), 0, ctx->stream, H);
    HIPCHK(ctx, hipGetLastError());
    VoxSumArgs U;
    U.key = H.key; U.idx = (const uint32_t*) (ds + Y.o_idx[final_buf]); U.txy = (const float2*) (ds + Y.o_txy); U.tn = (const float2*) (ds + Y.o_tn);
    U.head_pos = H.head_pos; U.n_heads = d_misc + 1; U.n = n; U.n_groups = n_groups;
    U.vxy = (float2*) (ds + Y.o_vxy); U.vn = (float2*) (ds + Y.o_vn); U.group_last = (int32_t*) (ds + Y.o_last); U.fault = d_misc + 2;
    hipLaunchKernelGGL(k_vox_sum, dim3(pt_blocks), dim3(256), 0, ctx->stream, U);
    HIPCHK(ctx, hipGetLastError());
  }
  VoxOutArgs O;
  O.groups = (const VoxGroup*) (ds + Y.u_groups); O.n_groups = n_groups; O.n = n;
  O.group_first = (const int32_t*) (ds + Y.o_first); O.group_last = (const int32_t*) (ds + Y.o_last);
  O.counts = (int32_t*) (ds + Y.o_down + Y.d_counts); O.verdict = d_misc;
  O.key = (const u64*) (ds + Y.o_key[final_buf]); O.head_pos = (const uint32_t*) (ds + Y.o_head_pos); O.n_heads = d_misc + 1;
  O.vxy = (const float2*) (ds + Y.o_vxy); O.vn = (const float2*) (ds + Y.o_vn);
  O.dst_xy = dst->d_xy; O.dst_nrm = dst->d_nrm; O.dst_count = dst->d_count; O.fault = d_misc + 2;
  hipLaunchKernelGGL(k_vox_verdict, dim3(group_blocks), dim3(256), 0, ctx->stream, O);
  if (n > 0) hipLaunchKernelGGL(k_vox_write, dim3(pt_blocks), dim3(256), 0, ctx->stream, O);
  hipLaunchKernelGGL(k_vox_finish, dim3(group_blocks), dim3(256), 0, ctx->stream, O);
  HIPCHK(ctx, hipGetLastError());
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  HIPCHK(ctx, hipMemcpyAsync(hs, ds + Y.o_down, Y.down_bytes, hipMemcpyDeviceToHost, ctx->stream));      // the one copy down
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  const int32_t* const h_counts = (const int32_t*) (hs + Y.d_counts); const int32_t* const h_dropped = (const int32_t*) (hs + Y.d_dropped);
  const int32_t* const h_misc = (const int32_t*) (hs + Y.d_misc);
  if (h_misc[2]) return fail(ctx, LSM2D_DEVICE_ERROR, "voxelize: an index left its array on the device (the destination clouds' counts are unchanged, their points may not be)");
  long long sum = 0;
  for (int32_t g = 0; g < n_groups; ++g) {
    if (h_counts[g] < 0 || h_counts[g] > n || h_dropped[g] < 0 || h_dropped[g] > n) return fail(ctx, LSM2D_DEVICE_ERROR, "voxelize: the counters are inconsistent");
    sum += h_counts[g];
  }
  if (sum != h_misc[1]) return fail(ctx, LSM2D_DEVICE_ERROR, "voxelize: the counters are inconsistent");
  for (int32_t g = 0; g < n_groups; ++g) { out_counts[g] = h_counts[g]; if (out_dropped) out_dropped[g] = h_dropped[g]; }
  if (h_misc[0]) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "voxelize: a group has more voxels than its destination cloud has room (out_counts: what is needed); nothing was written");
  cloudset_drop_grids(dst);
  dst->unpack_pending = false; dst->prep_pending = false;
  for (int32_t g = 0; g < n_groups; ++g) {
    const int32_t ci = dst_index ? dst_index[g] : g;
    dst->total += (int64_t) h_counts[g] - dst->h_count[(size_t) ci]; dst->h_count[(size_t) ci] = h_counts[g];
  }
  return LSM2D_SUCCESS;
}
