// lsm2d_capi_score_grid.inc -- a grid of pose hypotheses scored coarse to fine in ONE call (lsm2d_score_grid_select, include/lsm2d.h): the hypotheses are
// made on the device from the grid descriptor, every level is lsm2d_score_aligner_select's scoring and selection, and a level's selection becomes the next
// level's hypotheses without leaving the device.  Part of lsm2d_capi.hip, included behind the scoring's and the selection's parts.
//
//   per level   k_grid_level0 (level 0) or k_grid_children (below it) writes the level's pose block and origins; score_aligner_queue in its device-poses
//               mode runs the scoring over them -- no staging, no copy up, no pass over the items; k_grid_mask_pads (below level 0) takes the pads out of
//               the ranking; select_launches<CombRow> leaves [header | index | rows] on the device.
//   the end     k_grid_finish gathers the levels' headers and the selected poses and origins next to the last level's selection; the timing bracket begun
//               in front of the first launch is closed; ONE copy, ONE wait.
// Everything runs on the context's stream in order, on the current lane, which is never switched.  The lane's scratch and staging are sized ONCE, for the
// largest level, before the first launch (ensure_scratch may reallocate, and earlier levels' kernels are still queued): every level lays its arrays out for
// n_cap items, and the sets' search structures are found or built before that as well.  What must outlive a level -- its poses, its origins and its
// selection, which the next level's generation reads -- lies in the caller's region behind the scoring's layout (d_extra); poses and origins are
// double-buffered, so k_grid_children never writes what it reads.

// the caller's region behind the scoring's layout, relative to ScoreAlignerLayout::o_extra, and the region that goes down (x_final, final_bytes):
// [headers[n_levels][4] | the last level's header, index[k], rows[k][kCombWords] | pose[k][3] | origin[k]]
struct ScoreGridLayout {
  int levels = 0; size_t n[kGridMaxLevels] = {}, K[kGridMaxLevels] = {}; size_t n_cap = 0;
  size_t x_down[kGridMaxLevels] = {}, x_pose[2] = {}, x_origin[2] = {}, x_final = 0, f_last = 0, f_pose = 0, f_origin = 0, final_bytes = 0, bytes = 0;
  ScoreGridLayout(const lsm2d_pose_grid& g, size_t k) {
    levels = g.n_levels;
    const size_t R = (size_t) g.refine[0] * (size_t) g.refine[1] * (size_t) g.refine[2];
    size_t sel = 0;
    for (int l = 0; l < levels; ++l) {
      n[l] = l == 0 ? (size_t) g.count[0] * (size_t) g.count[1] * (size_t) g.count[2] : (size_t) g.k_parents * R;
      K[l] = l == levels - 1 ? k : (size_t) g.k_parents;
      n_cap = std::max(n_cap, n[l]);
      sel = std::max(sel, SelectLayout(n[l], K[l], kCombWords).e_down);      // the selection's own arrays and its counter; where its answer goes is ours to say
    }
    size_t o = up256(sel);
    for (int l = 0; l + 1 < levels; ++l) { x_down[l] = o; o = up256(o + SelectLayout(n[l], K[l], kCombWords).down_bytes); }
    for (int p = 0; p < 2; ++p) { x_pose[p] = o; o = up256(o + sizeof(float) * 3 * n_cap); x_origin[p] = o; o = up256(o + sizeof(int32_t) * n_cap); }
    x_final = o;
    f_last = sizeof(int32_t) * kSelectHeaderWords * (size_t) levels;
    f_pose = f_last + SelectLayout(n[levels - 1], k, kCombWords).down_bytes;
    f_origin = f_pose + sizeof(float) * 3 * k;
    final_bytes = f_origin + sizeof(int32_t) * k;
    x_down[levels - 1] = x_final + f_last;
    bytes = x_final + final_bytes;
  }
};

extern "C" int lsm2d_score_grid_select(lsm2d_context* ctx, int32_t n_slices, const lsm2d_slice_params* slices, const lsm2d_cloudset* const* fixed,
                                       const int32_t* fixed_cloud, const lsm2d_cloudset* const* moving, const int32_t* moving_cloud, const lsm2d_pose_grid* grid,
                                       const lsm2d_select_params* coarse_select, const lsm2d_select_params* select, int32_t k, float* out_pose,
                                       int32_t* out_origin, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats, int32_t* out_active,
                                       int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_level_counts) {
  static const char who[] = "score_grid_select";
  static_assert(LSM2D_GRID_MAX_LEVELS == kGridMaxLevels && LSM2D_GRID_MAX_ITEMS == kGridMaxItems, "the ABI's limits are the kernels'");
  if (!ctx || !slices || !fixed || !moving || !grid || !select || !out_pose || !out_n_selected || !out_n_accepted)
    return fail(ctx, LSM2D_BAD_ARGUMENT, "score_grid_select: null argument");
  if (n_slices < 1 || n_slices > kMaxSlices) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: n_slices outside [1, %d]", who, kMaxSlices);
  const lsm2d_pose_grid& g = *grid;
  if (g.n_levels < 1 || g.n_levels > kGridMaxLevels) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_grid_select: n_levels outside [1, LSM2D_GRID_MAX_LEVELS]");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_grid_select: k outside [1, LSM2D_SELECT_MAX_K]");
  long long n0 = 1, R = 1;
  for (int a = 0; a < 3; ++a) {
    if (g.count[a] < 1 || g.count[a] > kGridMaxItems) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: count[%d] outside [1, LSM2D_GRID_MAX_ITEMS]", who, a);
    if (g.refine[a] < 1 || g.refine[a] > kGridMaxItems) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: refine[%d] outside [1, LSM2D_GRID_MAX_ITEMS]", who, a);
    if (!(g.step[a] >= 0.0f) || !std::isfinite(g.step[a])) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: step[%d] must be finite and >= 0", who, a);
    if (!std::isfinite(g.center[a])) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: center[%d] must be finite", who, a);
    n0 *= g.count[a]; R *= g.refine[a];      // (at most 2^54 each)
  }
  if (n0 > kGridMaxItems) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_grid_select: the level-0 grid holds more than LSM2D_GRID_MAX_ITEMS cells");
  if (g.n_levels > 1) {
    if (!coarse_select) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_grid_select: null argument (coarse_select with n_levels > 1)");
    if (g.k_parents < 1 || g.k_parents > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_grid_select: k_parents outside [1, LSM2D_SELECT_MAX_K]");
    if ((long long) g.k_parents * R > kGridMaxItems) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_grid_select: k_parents x children per parent above LSM2D_GRID_MAX_ITEMS");
  }
  // the sets, the lane and the slices' finders as lsm2d_score_aligner_select checks them, on a batch of ONE item that uses the call's clouds: the cloud
  // indices are checked once per slice ("item 0, slice s")
  static const float present_pose[3] = {0.0f, 0.0f, 0.0f}; static const int32_t cloud0[kMaxSlices] = {0, 0, 0, 0};
  lsm2d_batch b;
  memset(&b, 0, sizeof b);
  b.n_alignments = 1; b.n_slices = n_slices; b.slices = slices; b.fixed = fixed; b.moving = moving;
  b.fixed_index = fixed_cloud ? fixed_cloud : cloud0; b.moving_index = moving_cloud ? moving_cloud : cloud0; b.init_pose = present_pose;
  { const int rc = score_aligner_head(ctx, who, &b); if (rc) return rc; }
  { const int rc = score_aligner_refusals(ctx, who, &b); if (rc) return rc; }
  const ScoreGridLayout G(g, (size_t) k);
  const int L = G.levels; const size_t n_cap = G.n_cap;
  // the scoring's layout for n_cap items, as every level's score_aligner_queue will make it -- and the sets' search structures, found or built now: a
  // build stages through the lane and may wait, neither of which may happen once the first level is queued
  bool f_tab = false, m_tab = false; int32_t slot_max = 1;
  for (int s = 0; s < n_slices; ++s) {
    long long need = 0;
    { const int rc0 = find_batch_need(slices + s, moving[s], &need); if (rc0) return rc0; }
    if (need < 0 || need > 0x7fffffffll) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: bad projector", who);
    slot_max = std::max(slot_max, (int32_t) need);
    FindBatchLaunch P;
    { const int rc = find_batch_prepare(ctx, slices + s, fixed[s], moving[s], 0.0f, (int32_t) need, who, P); if (rc) return rc; }
    f_tab = f_tab || fixed[s]->n_clouds != 1; m_tab = m_tab || moving[s]->n_clouds != 1;
  }
  const ScoreAlignerLayout Y0(n_cap, (size_t) n_slices, false, f_tab, m_tab, items_per_launch((size_t) slot_max, n_cap, kLinBatchMaxItems), (size_t) slot_max, G.bytes,
                              G.final_bytes);
  { int rc = ensure_scratch(ctx, Y0.d_bytes); if (rc) return rc; rc = ensure_stage(ctx, Y0.h_bytes); if (rc) return rc; }
  Lane& Ln = lane(ctx);
  char* const ds = (char*) Ln.d_scratch; char* const hs = (char*) Ln.h_stage;
  char* const dx = ds + Y0.o_extra;
  // the levels' batch: the index arrays are "present" where a set holds several clouds (the tables are on the device), none of them is read by the host
  static const int32_t present_index = 0;
  b.fixed_index = f_tab ? &present_index : nullptr; b.moving_index = m_tab ? &present_index : nullptr;
  // spacings: fp32 division on the host, once per level
  float spacing[kGridMaxLevels][3];
  for (int a = 0; a < 3; ++a) { spacing[0][a] = g.step[a]; for (int l = 1; l < L; ++l) spacing[l][a] = spacing[l - 1][a] / (float) g.refine[a]; }
  // ---- the timing bracket of the whole call: from in front of the first launch to behind the last selection
  ctx->have_timing = false;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(Ln.ev0, ctx->stream));
  for (int l = 0; l < L; ++l) {
    const size_t n = G.n[l];
    float* const d_pose = (float*) (dx + G.x_pose[l & 1]); int32_t* const d_origin = (int32_t*) (dx + G.x_origin[l & 1]);
    if (l == 0) {
      GridLevel0Args A;
      memset(&A, 0, sizeof A);
      for (int a = 0; a < 3; ++a) { A.center[a] = g.center[a]; A.step[a] = g.step[a]; }
      A.nx = g.count[0]; A.ny = g.count[1]; A.nt = g.count[2]; A.n0 = (int32_t) n; A.n_cap = (int32_t) n_cap; A.n_slices = n_slices;
      A.pose = d_pose; A.origin = d_origin;
      for (int s = 0; s < n_slices; ++s) {
        A.f_table[s] = f_tab ? (int32_t*) (ds + Y0.o_fidx) + (size_t) s * n_cap : nullptr; A.m_table[s] = m_tab ? (int32_t*) (ds + Y0.o_midx) + (size_t) s * n_cap : nullptr;
        A.f_cloud[s] = fixed_cloud ? fixed_cloud[s] : 0; A.m_cloud[s] = moving_cloud ? moving_cloud[s] : 0;
      }
      hipLaunchKernelGGL(k_grid_level0, dim3((unsigned) ((n_cap + 255) / 256)), dim3(256), 0, ctx->stream, A);
    } else {
      GridChildrenArgs A;
      memset(&A, 0, sizeof A);
      A.sel = (const int32_t*) (dx + G.x_down[l - 1]);
      A.pose_in = (const float*) (dx + G.x_pose[(l - 1) & 1]); A.origin_in = (const int32_t*) (dx + G.x_origin[(l - 1) & 1]);
      A.n_in = (int32_t) G.n[l - 1]; A.k_parents = g.k_parents; A.rx = g.refine[0]; A.ry = g.refine[1]; A.rt = g.refine[2]; A.R = (int32_t) R;
      for (int a = 0; a < 3; ++a) { A.spacing[a] = spacing[l][a]; A.center[a] = g.center[a]; }
      A.pose = d_pose; A.origin = d_origin;
      hipLaunchKernelGGL(k_grid_children, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    }
    HIPCHK(ctx, hipGetLastError());
    b.n_alignments = (int32_t) n;
    const ScoreDevicePoses dev = {n_cap, G.x_pose[l & 1]};
    ScoreAlignerLayout Y;
    { const int rc = score_aligner_queue(ctx, who, &b, G.bytes, G.final_bytes, Y, nullptr, 0, /* chained */ true, &dev); if (rc) return rc; }
    HIPCHK(ctx, hipGetLastError());      // (k_score_combine's launch)
    if ((char*) Ln.d_scratch != ds || Y.o_extra != Y0.o_extra || Y.o_comb != Y0.o_comb || Y.h_out != Y0.h_out)
      return fail(ctx, LSM2D_DEVICE_ERROR, "score_grid_select: a level laid its scratch out differently from the first");
    if (l > 0) {
      GridMaskArgs M;
      M.sel = (const int32_t*) (dx + G.x_down[l - 1]); M.k_parents = g.k_parents; M.R = (int32_t) R; M.rows = (int32_t*) (ds + Y.o_comb);
      hipLaunchKernelGGL(k_grid_mask_pads<CombRow>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, M);
      HIPCHK(ctx, hipGetLastError());
    }
    const lsm2d_select_params* const sp = l == L - 1 ? select : coarse_select;
    const SelectLayout E(n, G.K[l], kCombWords);
    { const int rc = select_launches<CombRow>(ctx, select_args(ds + Y.o_comb, (int32_t) n, (int32_t) G.K[l], sp), E, dx, (int32_t*) (dx + G.x_down[l])); if (rc) return rc; }
    HIPCHK(ctx, hipGetLastError());
  }
  {
    GridFinishArgs F;
    memset(&F, 0, sizeof F);
    for (int l = 0; l < L; ++l) F.sel[l] = (const int32_t*) (dx + G.x_down[l]);
    F.n_levels = L; F.k = k; F.n_last = (int32_t) G.n[L - 1];
    F.pose_in = (const float*) (dx + G.x_pose[(L - 1) & 1]); F.origin_in = (const int32_t*) (dx + G.x_origin[(L - 1) & 1]);
    F.headers = (int32_t*) (dx + G.x_final); F.pose = (float*) (dx + G.x_final + G.f_pose); F.origin = (int32_t*) (dx + G.x_final + G.f_origin);
    const size_t threads = std::max((size_t) k, (size_t) (L * kSelectHeaderWords));
    hipLaunchKernelGGL(k_grid_finish, dim3((unsigned) ((threads + 255) / 256)), dim3(256), 0, ctx->stream, F);
    HIPCHK(ctx, hipGetLastError());
  }
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(Ln.ev1, ctx->stream));
  ctx->have_timing = ctx->kernel_timing != 0; ctx->timed_lane = ctx->cur;
  char* const h_down = hs + Y0.h_out;
  HIPCHK(ctx, hipMemcpyAsync(h_down, dx + G.x_final, G.final_bytes, hipMemcpyDeviceToHost, ctx->stream));      // the one copy down
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  const int32_t* const hh = (const int32_t*) h_down;
  for (int l = 0; l < L; ++l)
    if (!select_header_ok(hh + kSelectHeaderWords * l, (int32_t) G.n[l], (int32_t) G.K[l], false))
      return fail(ctx, LSM2D_DEVICE_ERROR, "score_grid_select: the selection's counters are inconsistent");
  const int32_t* const h_last = (const int32_t*) (h_down + G.f_last);
  const int32_t n_acc = h_last[0], n_sel = h_last[1];
  if (n_acc != hh[kSelectHeaderWords * (L - 1)] || n_sel != hh[kSelectHeaderWords * (L - 1) + 1])
    return fail(ctx, LSM2D_DEVICE_ERROR, "score_grid_select: the selection's counters are inconsistent");
  memcpy(out_pose, h_down + G.f_pose, sizeof(float) * 3 * (size_t) n_sel);
  if (out_origin) memcpy(out_origin, h_down + G.f_origin, sizeof(int32_t) * (size_t) n_sel);
  comb_block_out(h_last, (size_t) k, 0, nullptr, out_H, out_b, out_stats, out_active);
  if (out_level_counts) for (int l = 0; l < L; ++l) { out_level_counts[2 * l] = hh[kSelectHeaderWords * l]; out_level_counts[2 * l + 1] = hh[kSelectHeaderWords * l + 1]; }
  *out_n_selected = n_sel; *out_n_accepted = n_acc;
  return LSM2D_SUCCESS;
}
