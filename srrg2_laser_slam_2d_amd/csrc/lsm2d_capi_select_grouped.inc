// lsm2d_capi_select_grouped.inc -- the three grouped select entry points (include/lsm2d.h, 0.7.8): each its ungrouped sibling up to the selection -- the same
// checks, score_batch_queue / score_aligner_queue / AlignBatch's select mode, with the groups' table riding up behind the arguments -- ending in
// select_queue_grouped (lsm2d_capi_finder.inc).  Included LAST by lsm2d_capi.hip: the grouped kernels are instantiated here, behind every kernel the library
// had before them, so that those keep their places (and their labels) in the code object.

extern "C" int lsm2d_score_select_grouped(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                          const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses,
                                          const lsm2d_select_params* select, int32_t k, int32_t n_groups, const int32_t* group_offsets, int32_t* out_index,
                                          float* out_H, float* out_b, lsm2d_iteration_stats* out_stats, int32_t* out_n_selected, int32_t* out_n_accepted) {
  static const char who[] = "score_select_grouped";
  if (!select || !out_index || !out_n_selected || !out_n_accepted) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select_grouped: null argument");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select_grouped: k outside [1, LSM2D_SELECT_MAX_K]");
  { const int rc = batch_head(ctx, who, sp, fixed, moving, n_items, 0); if (rc) return rc; }
  { const int rc = check_groups(ctx, who, n_groups, group_offsets, n_items, k); if (rc) return rc; }
  if (n_items == 0) { groups_report_empty(n_groups, out_n_selected, out_n_accepted, nullptr); return LSM2D_SUCCESS; }
  if (!poses) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select_grouped: null argument");
  const size_t K = (size_t) k;
  const SelectGroupedLayout E(group_offsets, (size_t) n_groups, K, kLinOutWords);
  ScoreLayout Y;
  { const int rc = score_batch_queue(ctx, who, sp, fixed, fixed_index, moving, moving_index, n_items, poses, E.d_bytes, E.down_bytes, Y, E.table.data(), E.table_bytes()); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  SelectArgs A;
  A.rows = (const float*) (ds + Y.o_out); A.n_items = n_items; A.k = k;
  A.min_inliers = select->min_inliers; A.max_chi_per_inlier = select->max_chi_per_inlier; A.min_inlier_ratio = select->min_inlier_ratio;
  { const int rc = select_queue_grouped<ScoreRow>(ctx, who, A, E, ds + Y.o_extra, (const int32_t*) (ds + Y.o_up), hs + Y.h_out); if (rc) return rc; }
  float H[9], b[3];
  for (size_t g = 0; g < E.G; ++g) {
    const int32_t* h = (const int32_t*) (hs + Y.h_out) + E.group_words * g;
    const int32_t* h_index = h + kSelectHeaderWords; const float* h_rows = (const float*) (h + kSelectHeaderWords + K);
    for (int32_t j = 0; j < h[1]; ++j) {
      const size_t slot = g * K + (size_t) j;
      out_index[slot] = h_index[j];
      lin_row_out(h_rows + kLinOutWords * (size_t) j, out_H ? out_H + 9 * slot : H, out_b ? out_b + 3 * slot : b, out_stats ? out_stats + slot : nullptr);
    }
    out_n_selected[g] = h[1]; out_n_accepted[g] = h[0];
  }
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_score_aligner_select_grouped(lsm2d_context* ctx, const lsm2d_batch* batch, const lsm2d_select_params* select, int32_t k, int32_t n_groups,
                                                  const int32_t* group_offsets, int32_t* out_index, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats,
                                                  int32_t* out_active, int32_t* out_n_selected, int32_t* out_n_accepted) {
  static const char who[] = "score_aligner_select_grouped";
  if (!select || !out_index || !out_n_selected || !out_n_accepted) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_aligner_select_grouped: null argument");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_aligner_select_grouped: k outside [1, LSM2D_SELECT_MAX_K]");
  { const int rc = score_aligner_head(ctx, who, batch); if (rc) return rc; }
  { const int rc = check_groups(ctx, who, n_groups, group_offsets, batch->n_alignments, k); if (rc) return rc; }
  if (batch->n_alignments == 0) { groups_report_empty(n_groups, out_n_selected, out_n_accepted, nullptr); return LSM2D_SUCCESS; }
  const size_t K = (size_t) k;
  const SelectGroupedLayout E(group_offsets, (size_t) n_groups, K, kCombWords);
  ScoreAlignerLayout Y;
  { const int rc = score_aligner_queue(ctx, who, batch, E.d_bytes, E.down_bytes, Y, E.table.data(), E.table_bytes()); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  HIPCHK(ctx, hipGetLastError());
  SelectArgs A;
  A.rows = (const float*) (ds + Y.o_comb); A.n_items = batch->n_alignments; A.k = k;
  A.min_inliers = select->min_inliers; A.max_chi_per_inlier = select->max_chi_per_inlier; A.min_inlier_ratio = select->min_inlier_ratio;
  { const int rc = select_queue_grouped<CombRow>(ctx, who, A, E, ds + Y.o_extra, (const int32_t*) (ds + Y.o_up_extra), hs + Y.h_out); if (rc) return rc; }
  for (size_t g = 0; g < E.G; ++g) {
    const int32_t* h = (const int32_t*) (hs + Y.h_out) + E.group_words * g;
    const int32_t* h_index = h + kSelectHeaderWords; const float* h_rows = (const float*) (h + kSelectHeaderWords + K);
    for (int32_t j = 0; j < h[1]; ++j) {
      const size_t slot = g * K + (size_t) j;
      out_index[slot] = h_index[j];
      comb_row_out(h_rows + kCombWords * (size_t) j, out_H ? out_H + 9 * slot : nullptr, out_b ? out_b + 3 * slot : nullptr, out_stats ? out_stats + slot : nullptr,
                   out_active ? out_active + slot : nullptr);
    }
    out_n_selected[g] = h[1]; out_n_accepted[g] = h[0];
  }
  return LSM2D_SUCCESS;
}

// ... and per group of the batch: the fleet's candidate loop (include/lsm2d.h).  lsm2d_align_select up to the selection, with the groups' table in the input block.
extern "C" int lsm2d_align_select_grouped(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, const lsm2d_select_params* select, int32_t k,
                                          int32_t n_groups, const int32_t* group_offsets, int32_t* out_index, float* out_pose, float* out_H, int32_t* out_its,
                                          lsm2d_iteration_stats* out_last_stats, int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  static const char who[] = "align_select_grouped";
  if (!ctx || !ap || !b || !select || !out_index || !out_pose || !out_n_selected || !out_n_accepted) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_select_grouped: null argument");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_select_grouped: k outside [1, LSM2D_SELECT_MAX_K]");
  if (lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: two batches are in flight on this context: wait for the older one first (lsm2d_align_batch_wait)");
  { const int rc = check_groups(ctx, who, n_groups, group_offsets, b->n_alignments, k); if (rc) return rc; }
  static int32_t wanted_status; static lsm2d_iteration_stats wanted_stats;      // (as in lsm2d_align_select)
  const SelectGroupedLayout E(group_offsets, (size_t) n_groups, (size_t) k, AlignRow::kWords);
  AlignBatch B;
  B.ctx = ctx; B.L = &lane(ctx); B.ap = ap; B.b = b; B.out_pose = out_pose; B.out_H = out_H; B.out_status = &wanted_status; B.out_its = out_its;
  B.out_stats = &wanted_stats; B.out_last_pose = nullptr; B.out_work = nullptr; B.pend = nullptr;
  B.select = select; B.select_k = k; B.sel_index = out_index; B.sel_last_stats = out_last_stats; B.sel_n_selected = out_n_selected; B.sel_n_accepted = out_n_accepted;
  B.sel_n_success = out_n_success; B.groups = &E;
  if (b->n_alignments == 0) {      // an empty batch: its descriptor is checked as ever, every group's counts are zeros
    const int rc = B.validate_and_lay_out_scratch();
    if (rc != kEmptyBatch) return rc;
    groups_report_empty(n_groups, out_n_selected, out_n_accepted, out_n_success);
    return LSM2D_SUCCESS;
  }
  return align_batch_run(B);
}
