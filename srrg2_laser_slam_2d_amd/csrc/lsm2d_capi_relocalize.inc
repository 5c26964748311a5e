// lsm2d_capi_relocalize.inc -- the relocaliser / loop detector's candidate loop in ONE call (lsm2d_relocalize_select, include/lsm2d.h; MULTI.json:749-769,
// :964-986): lsm2d_score_aligner_select's scoring and selection, then lsm2d_align_select over the selected hypotheses, with nothing coming down in between.
// Part of lsm2d_capi.hip, included behind the aligner's and the selection's parts, whose stages it chains.
//
//   stage 1   score_aligner_queue and the selection's launches (select_launches<CombRow>) on the context's CURRENT lane, exactly as lsm2d_score_aligner_select
//             queues them -- but the region that goes down is written into the OTHER lane's scratch, and nothing is copied or waited for.
//   stage 2   AlignBatch in select mode on the other lane, n = k_score, with its inputs on the device (AlignBatch::reloc): k_reloc_items writes
//             [init_pose | prior | fidx | midx] from stage 1's selection and upload, k_cull_estimate (n > 256) and the aligner read them in stream order,
//             k_align_rows_live packs the rows with the pads' ok = 0, select_launches<AlignRow> ranks them into the region next to stage 1's.
//   the end   the timing bracket begun in front of stage 1's first launch is closed on stage 1's lane; ONE copy of [stage 1's header | index | rows || stage 2's header | index | rows], ONE wait.
// Two lanes, so neither stage's layout knows of the other and no scratch is reallocated between the stages: stage 2's checks, layout, scratch and set
// preparation (AlignBatch's stages up to lay_out_lds) run BEFORE stage 1 queues anything; stage 1's own allocation comes ahead of its first launch as ever.
// The context's current lane stays what it is throughout: AlignBatch is handed its lane (ensure_scratch / ensure_stage take one), nothing is switched.
// The path rule decides for n = k_score, not for the number selected: the two-call route may take another launch form; the bits are the same across forms.
// A call in which nothing passes stage 1 still runs k_score alignments of hypothesis 0.

// what stage 1 left on the device, as stage 2 needs it
struct RelocStage {
  Lane* L1 = nullptr;                // stage 1's lane: its scratch holds the upload, its events the timing bracket
  ScoreAlignerLayout Y;              // where the upload lies there
  const lsm2d_batch* batch = nullptr; // the caller's descriptor (the hypotheses)
  int32_t k_score = 0;
  size_t down1_bytes = 0, o_down2 = 0;      // stage 1's region that goes down, and where stage 2's begins behind it (both relative to AlignBatch::o_reloc_down)
  // the caller's outputs for stage 1
  int32_t* out_scored_index = nullptr; lsm2d_iteration_stats* out_scored_stats = nullptr; int32_t* out_n_scored_selected = nullptr; int32_t* out_n_scored_accepted = nullptr;
};

int AlignBatch::reloc_stage_inputs() {
  const RelocStage& R = *reloc;
  const lsm2d_batch* hb = R.batch;
  const char* const d1 = (const char*) R.L1->d_scratch;
  const size_t n_items = (size_t) hb->n_alignments;
  RelocItemsArgs I;
  memset(&I, 0, sizeof I);
  I.sel = (const int32_t*) (ds + o_reloc_down);
  I.poses = (const float*) d1; I.prior = hb->prior ? (const PriorDev*) (d1 + R.Y.o_prior) : nullptr;
  I.n_items = hb->n_alignments; I.n_slices = ns; I.k_score = n;
  I.pose_out = (float*) (ds + o_pose_in); I.prior_out = hb->prior ? (PriorDev*) (ds + o_prior) : nullptr;
  for (int s = 0; s < ns; ++s) {
    RelocSlice& S = I.s[s];
    S.f_index = hb->fixed_index ? (const int32_t*) (d1 + R.Y.o_fidx) + (size_t) s * n_items : nullptr;
    S.m_index = hb->moving_index ? (const int32_t*) (d1 + R.Y.o_midx) + (size_t) s * n_items : nullptr;
    S.f_clouds = hb->fixed[s]->n_clouds; S.m_clouds = hb->moving[s]->n_clouds;
    S.f_out = (int32_t*) (ds + o_fidx[s]); S.m_out = (int32_t*) (ds + o_midx[s]);
  }
  hipLaunchKernelGGL(k_reloc_items, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, pre, I);
  HIPCHK(ctx, hipGetLastError());
  return LSM2D_SUCCESS;
}

// select_finish for the chained call: the live count comes from stage 1's header on the device, the rows' selection lands next to stage 1's region, the
// bracket stage 1 began is ended, and ONE copy and ONE wait hand both stages' answers over.
int AlignBatch::reloc_finish() {
  RelocStage& R = *reloc;
  const SelectLayout E((size_t) n, (size_t) select_k, AlignRow::kWords);
  char* const d = (char*) L->d_scratch;
  char* const de = d + o_sel;
  int32_t* const d_down1 = (int32_t*) (d + o_reloc_down);
  int32_t* const d_down2 = (int32_t*) (d + o_reloc_down + R.o_down2);
  HIPCHK(ctx, hipMemsetAsync(de + E.e_acc, 0, sizeof(int32_t) * 3, ks));      // accepted | Success | never written
  AlignRowsLiveArgs RL;
  AlignRowsArgs& RA = RL.R;
  RA.pose = (const float*) (d + o_pose); RA.H = (const float*) (d + o_H); RA.status = (const int32_t*) (d + o_status); RA.its = (const int32_t*) (d + o_its);
  RA.stats = (const StatsDev*) (d + o_stats); RA.n = n; RA.stats_stride = stats_stride; RA.not_written = kStatusNotWritten;
  RA.rows = (float*) (d + o_rows); RA.counts = (int32_t*) (de + E.e_acc) + 1;
  RL.n_live = d_down1 + 1;      // stage 1's n_selected
  hipLaunchKernelGGL(k_align_rows_live<AlignRow>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ks, RL);
  HIPCHK(ctx, hipGetLastError());
  { const int rc = select_launches<AlignRow>(ctx, select_args(RA.rows, n, select_k, select), E, de, d_down2); if (rc) return rc; }
  // the bracket: from in front of stage 1's first launch (its lane's ev0, recorded by the entry point) to here
  HIPCHK(ctx, hipGetLastError());
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(R.L1->ev1, ks));
  ctx->have_timing = ctx->kernel_timing != 0; ctx->timed_lane = (int) (R.L1 - ctx->lanes);
  char* const h_down = hs + o_reloc_down;
  HIPCHK(ctx, hipMemcpyAsync(h_down, d_down1, R.o_down2 + E.down_bytes, hipMemcpyDeviceToHost, ks));      // the one copy down
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  // ---- stage 1's answer, as lsm2d_score_aligner_select hands it over
  const int32_t* h1 = (const int32_t*) h_down;
  const int32_t n_sel1 = h1[1];
  if (!select_header_ok(h1, R.batch->n_alignments, R.k_score, false)) return fail(ctx, LSM2D_DEVICE_ERROR, "relocalize_select: the selection's counters are inconsistent");
  const int32_t* h1_index = h1 + kSelectHeaderWords;
  // ---- stage 2's, as lsm2d_align_select hands it over, with the indices taken through stage 1's
  const int32_t* h2 = (const int32_t*) (h_down + R.o_down2);
  if (h2[3] != 0) { for (Lane& any : ctx->lanes) any.order_valid = false; return fail(ctx, LSM2D_DEVICE_ERROR, "align_batch: an alignment's workgroup never reported (placement or launch fault)"); }
  if (!select_header_ok(h2, n_sel1, select_k, true)) return fail(ctx, LSM2D_DEVICE_ERROR, "relocalize_select: the selection's counters are inconsistent");
  const int32_t* h2_index = h2 + kSelectHeaderWords;
  for (int32_t j = 0; j < h2[1]; ++j) if (h2_index[j] < 0 || h2_index[j] >= n_sel1) return fail(ctx, LSM2D_DEVICE_ERROR, "relocalize_select: a pad was selected");
  if (R.out_scored_stats) comb_block_out(h1, (size_t) R.k_score, 0, nullptr, nullptr, nullptr, R.out_scored_stats, nullptr);
  memcpy(R.out_scored_index, h1_index, sizeof(int32_t) * (size_t) n_sel1);
  groups_report(h1, 0, 1, R.out_n_scored_selected, R.out_n_scored_accepted, nullptr);
  align_block_out(h2, (size_t) select_k, 0, h1_index, sel_index, out_pose, out_H, out_its, sel_last_stats);
  groups_report(h2, 0, 1, sel_n_selected, sel_n_accepted, sel_n_success);
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_relocalize_select(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* batch,
                                       const lsm2d_select_params* score_select, int32_t k_score, const lsm2d_select_params* align_select, int32_t k,
                                       int32_t* out_scored_index, lsm2d_iteration_stats* out_scored_stats, int32_t* out_n_scored_selected, int32_t* out_n_scored_accepted,
                                       int32_t* out_index, float* out_pose, float* out_H, int32_t* out_its, lsm2d_iteration_stats* out_last_stats,
                                       int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  static const char who[] = "relocalize_select";
  if (!ctx || !ap || !batch || !score_select || !out_scored_index || !out_n_scored_selected || !out_n_scored_accepted || !out_index || !out_pose || !out_n_selected ||
      !out_n_accepted)
    return fail(ctx, LSM2D_BAD_ARGUMENT, "relocalize_select: null argument");
  if (!align_select) align_select = score_select;
  if (k_score < 1 || k_score > kSelectMaxK || k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "relocalize_select: k_score or k outside [1, LSM2D_SELECT_MAX_K]");
  // the call takes BOTH lanes: not with a batch in flight on the context
  if (ctx->inflight > 0 || ctx->lanes[0].busy || ctx->lanes[1].busy)
    return fail(ctx, LSM2D_BAD_ARGUMENT, "relocalize_select: a batch is in flight on this context: wait for it first (lsm2d_align_batch_wait)");
  { const int rc = score_aligner_head(ctx, who, batch); if (rc) return rc; }
  static int32_t wanted_status; static lsm2d_iteration_stats wanted_stats;      // (as lsm2d_align_select: the stages ask "is this output wanted?" of the pointers)
  static const float present_pose[3] = {0.0f, 0.0f, 0.0f}; static const lsm2d_prior present_prior = {{0.0f, 0.0f, 0.0f}, {0.0f}}; static const int32_t present_index = 0;
  RelocStage R;
  R.L1 = &lane(ctx); R.batch = batch; R.k_score = k_score;
  R.out_scored_index = out_scored_index; R.out_scored_stats = out_scored_stats; R.out_n_scored_selected = out_n_scored_selected; R.out_n_scored_accepted = out_n_scored_accepted;
  // stage 2's batch: k_score slots over the same slices and sets; prior and index arrays "present" (every slot's clouds are spelled out), none of them read
  lsm2d_batch b2 = *batch;
  b2.init_pose = present_pose; b2.prior = batch->prior ? &present_prior : nullptr; b2.fixed_index = &present_index; b2.moving_index = &present_index;
  AlignBatch B;
  B.ctx = ctx; B.L = &ctx->lanes[ctx->cur ^ 1]; B.ap = ap; B.b = &b2; B.out_pose = out_pose; B.out_H = out_H; B.out_status = &wanted_status; B.out_its = out_its;
  B.out_stats = &wanted_stats; B.out_last_pose = nullptr; B.out_work = nullptr; B.pend = nullptr;
  B.select = align_select; B.select_k = k; B.sel_index = out_index; B.sel_last_stats = out_last_stats; B.sel_n_selected = out_n_selected; B.sel_n_accepted = out_n_accepted;
  B.sel_n_success = out_n_success;
  if (batch->n_alignments == 0) {      // no hypotheses: the aligner's side of the descriptor is checked as lsm2d_align_select checks it, the counts are zeros
    const int rc = B.validate_and_lay_out_scratch();
    if (rc != kEmptyBatch) return rc;
    *out_n_scored_selected = 0; *out_n_scored_accepted = 0; *out_n_selected = 0; *out_n_accepted = 0; if (out_n_success) *out_n_success = 0;
    return LSM2D_SUCCESS;
  }
  { const int rc = score_aligner_refusals(ctx, who, batch); if (rc) return rc; }      // (stage 1's, ahead of stage 2's preparation: score_aligner_queue is told not to repeat them)
  b2.n_alignments = k_score;
  const SelectLayout E1((size_t) batch->n_alignments, (size_t) k_score, kCombWords);
  const SelectLayout E2((size_t) k_score, (size_t) k, AlignRow::kWords);
  R.down1_bytes = E1.down_bytes; R.o_down2 = up256(E1.down_bytes);
  B.reloc = &R; B.reloc_down_bytes = R.o_down2 + E2.down_bytes;
  // ---- stage 2's refusals, layout, scratch and set preparation, before anything of stage 1 is queued.  AlignBatch asks for ITS lane's scratch and staging
  // (B.L: the other lane); set preparation stages through the current lane, which stage 1 lays out only afterwards.
  {
    int rc = B.validate_and_lay_out_scratch();
    if (!rc) rc = B.choose_path();
    if (!rc) rc = B.prepare_slices();
    if (!rc) rc = B.lay_out_lds();
    if (rc) return rc;
  }
  // ---- stage 1 on the current lane; its selection writes what goes down into stage 2's lane.
  // The timing bracket of the WHOLE call begins here, in front of stage 1's first launch, on stage 1's lane; reloc_finish ends it behind the final selection.
  // Until then there is no finished bracket: a call that fails from here on must not leave lsm2d_last_kernel_ms pairing this ev0 with an older ev1.
  ctx->have_timing = false;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(R.L1->ev0, ctx->stream));
  { const int rc = score_aligner_queue(ctx, who, batch, E1.d_bytes, 0, R.Y, nullptr, 0, /* chained */ true); if (rc) return rc; }
  {
    char* const d1 = (char*) R.L1->d_scratch;
    HIPCHK(ctx, hipGetLastError());      // (k_score_combine's launch, as lsm2d_score_aligner_select checks it)
    const int rc = select_launches<CombRow>(ctx, select_args(d1 + R.Y.o_comb, batch->n_alignments, k_score, score_select), E1, d1 + R.Y.o_extra, (int32_t*) ((char*) B.L->d_scratch + B.o_reloc_down)); if (rc) return rc;
    HIPCHK(ctx, hipGetLastError());
  }
  // ---- stage 2: inputs made on the device, placement, launch, rows, selection, the copy and the wait
  int rc = B.stage_inputs();
  if (!rc) rc = B.make_placement();
  if (!rc) rc = B.launch();
  if (!rc) rc = B.hand_over();
  // the other lane's device block and placement were made from data the host never saw: a later lsm2d_align_batch there must not believe it knows them
  B.L->inputs_shadow.clear(); B.L->inputs_valid = false; B.L->order_valid = false;
  return rc;
}
