// lsm2d_capi_aligner.inc -- plugin interface #2: MultiAligner2D::compute over a batch (lsm2d_align_batch and its begin / wait / pairs / estimate forms).
// Part of lsm2d_capi.hip (included there); not a translation unit of its own.
//
// A call runs through the STAGES of AlignBatch, in this order (round 6: one 550-line function before; the statements are the same):
//   validate_and_lay_out_scratch  the arguments, the kernel's scalar parameters, where inputs / results / statistics live in the lane's scratch and staging
//   choose_path                   one workgroup per alignment (k_align), the split path, zero-copy arguments
//   prepare_slices                per slice: ownership, pending preprocessing / uploads, the finder's structure (grid, distance map, KD-tree), the derived layouts
//   lay_out_lds                   dynamic LDS of the launch: canvases, reduction, the finders' staged tables, culling state, unit lists, sum_order's records; the latency kernel's
//   stage_inputs                  start poses / priors / index arrays into staging and (unless kept) onto the device; where the results go; status words armed
//   estimate_only | make_placement  lsm2d_estimate_work's answer | the balanced placement of a culled batch (k_cull_estimate), kept for an unchanged batch
//   launch                        the kernels, the events, the copies of the results
//   hand_over                     a lsm2d_pending for an asynchronous begin, or the wait and the results (align_batch_finish)
// SELECT mode (lsm2d_align_select: AlignBatch::select != NULL) runs the same stages with the results kept on the device -- no zero-copy form, no results written
// to pinned host memory, no copy of them queued -- and hand_over ends in k_align_rows and select_queue<AlignRow>: k rows come down (select_finish).
// ... and with its INPUTS ON THE DEVICE (lsm2d_relocalize_select: AlignBatch::reloc != NULL, lsm2d_capi_relocalize.inc) select mode takes a batch whose start
// poses, priors and index arrays a kernel writes from an earlier stage's selection: stage_inputs copies nothing and queues no upload (reloc_stage_inputs),
// every shortcut that assumes the host knows the inputs is off, the timing bracket is the earlier stage's, and hand_over ends in reloc_finish.
// ---- plugin interface #2 ----------------------------------------------------------------------------------------
extern "C" uint64_t lsm2d_pair_hash(uint32_t slice, uint32_t fixed_idx, uint32_t moving_idx) {      // the kernels' pair_hash_dev, on the host
  const uint32_t a = fixed_idx * 0x9E3779B1u, b = (moving_idx ^ (slice * 0x632BE5ABu)) * 0x85EBCA77u;
  uint32_t lo = a ^ ((b << 13) | (b >> 19)), hi = b ^ ((a << 19) | (a >> 13));
  lo += ((lo << 17) | (lo >> 15)) ^ b;
  hi += ((hi << 11) | (hi >> 21)) ^ a;
  return ((uint64_t) hi << 32) | (uint64_t) lo;
}

extern "C" int32_t lsm2d_stats_capacity(const lsm2d_aligner_params* ap) {
  if (!ap) return 1;
  const long long c = (long long) (ap->max_iterations > 0 ? ap->max_iterations : 0) * (ap->enable_inlier_only_runs ? 2 : 1);
  return (int32_t) (c < 1 ? 1 : (c > 0x7fffffff ? 0x7fffffff : c));
}

// What a batch that has been LAUNCHED keeps until its results are asked for (lsm2d_align_batch_begin / _wait; the synchronous calls go through the same two halves)
struct lsm2d_pending {
  lsm2d_context* ctx = nullptr;
  Lane* lane = nullptr;                     // the lane the batch was launched on: its pinned staging buffer is where the results are (or are copied to), its ev_done what a wait waits for
  size_t o_pose = 0, o_H = 0, o_status = 0, o_its = 0, o_stats = 0, o_last_pose = 0, o_clock = 0, o_cand = 0;
  int n = 0, stats_stride = 0, n_clock = 0, clock_stride = 0;
  bool zero_copy = false, want_stats = false, want_last_pose = false, stamps = false, timed = false, async = false;
};
static int align_batch_finish(lsm2d_pending& P, float* out_pose, float* out_H, int32_t* out_status, int32_t* out_its, lsm2d_iteration_stats* out_stats, float* out_last_pose);

// out_last_pose [n][3] (may be NULL): the pose the last iteration every alignment started began at (what lsm2d_align_batch_pairs re-derives
// that iteration's correspondences from)
// out_work [n] (may be NULL): ONLY the work estimate of lsm2d_estimate_work is produced -- no alignment runs, the other outputs are not touched
// pend != NULL: lsm2d_align_batch_begin -- the call returns once everything is queued; the output pointers only say WHICH outputs are wanted (non-null), nothing is
// written through them; lsm2d_align_batch_wait -> align_batch_finish hands the results over.
static constexpr int kEmptyBatch = 0x7e7e7e7e;      // validate_and_lay_out_scratch: n_alignments == 0, nothing to do, LSM2D_SUCCESS

// Threads per workgroup of a culled projective batch of n alignments whose workgroups ask for `lds` bytes of dynamic LDS ("align_width": 0 = this rule; 512 or 256
// forces one; results never depend on it).  One workgroup per alignment: 512 threads (8 waves) fill a CU's 32 wave slots with four workgroups -- 1024 alignments
// resident on 256 CUs; 256 threads (4 waves: one per SIMD) leave room for eight, of which the canvases' LDS admits six -- 1536 resident, each alignment slower, the
// same rate for a full chip (1536 alignments in 1.10 ms against 1024 in 0.745 on configs[1]'s geometry).  A batch just above a multiple of 1024 at 512 threads
// leaves its last few alignments to a round of their own on an emptying chip: 1100 alignments 1.02 ms, 1536 1.27 ms (profiles/r06/batch_size_sweep_widths_r06k.txt).
// (Widths that are not a multiple of 256 threads spread their waves unevenly over the four SIMDs and gain no residency: 384 threads measured -- four per CU, not five.)
// The rule: the cheaper width under a model of a launch's time in units of one full round of the width, fitted to that sweep: full rounds, plus a partly filled
// last round g(f) of a full one (f = its fill); a lone partly filled round of narrow workgroups is bounded below by one alignment's lifetime at 256 threads.
static int align_width_for(const lsm2d_context* ctx, int n, size_t lds) {
  if (ctx->align_width == 512 || ctx->align_width == 256) return ctx->align_width;
  if (n <= 1024 || n > 4096) return kAlignBlock;      // (many rounds fill their last one's gaps by themselves: 65 536 candidates ran 2.6 % SLOWER in narrow workgroups)
  const int n_cu = ctx->n_cu > 0 ? ctx->n_cu : 256;
  const size_t per_wg = lds + 1536 + 512;      // + the kernel's static LDS and the allocation's granule
  const int by_lds = (int) ((160u << 10) / per_wg);
  auto launch_cost = [&](int width) -> double {
    int per_cu = 32 / (width / 64); if (by_lds < per_cu) per_cu = by_lds;
    if (per_cu < 1) return 1e30;
    const int slots = per_cu * n_cu, full = n / slots;
    const double f = (double) (n - full * slots) / (double) slots;
    double g = 0.0;
    if (f > 0.0) {
      if (width == 512) { g = 0.33 + 0.65 * f; if (0.14 + 8.5 * f < g) g = 0.14 + 8.5 * f; }    // (a handful of stragglers: their own lifetime on an emptying chip, 0.15 of a round for one, 0.27 for sixteen)
      else if (full == 0) { g = 0.79 + 0.75 * (f - 0.72); if (g < 0.79) g = 0.79; }            // (one alignment's lifetime at 256 threads: 0.79 of a full narrow round)
      else g = 0.40 + 0.62 * f;
      if (g > 1.0) g = 1.0;
    }
    return (double) per_cu * ((double) full + g) * (width == 512 ? 1.0 : 0.985);      // a full round of either width: the same time per resident alignment, to 1.5 %
  };
  return launch_cost(256) < 0.97 * launch_cost(512) ? 256 : kAlignBlock;      // (the model is good to a few per cent: the wide kernel on near-ties)
}

// Round 6 (late): PACKED batches.  A few alignments more than one round of wide workgroups holds -- or more than one round of NARROW ones -- used to start another
// dispatch round on an emptying chip.  Instead the batch runs in exactly one round of 4 x n_cu workgroups, its lightest alignments two to a workgroup, one after the
// other (k_align_two; the pairs are made where the placement is made: balance_order).  A light alignment still pays the phases outside its stream, so pairs are
// heavy items and the form pays only where few are needed or where the alternative is two wide rounds -- measured (profiles/r06/order_pairs_ab_r06Q.txt, us per
// alignment, k_align alone): 1025: 0.840 -> 0.734, 1040: 0.833 (narrow) -> 0.815, 1100: 0.808 (narrow) -> 0.863, 1536: 0.724 (narrow) -> 0.751, 1700: 0.775 -> 0.731.
// Hence: packed for slots < n <= slots + 24 and for narrow capacity < n < 2 x slots; "align_width" 1024 forces it, 512 / 256 exclude it.  Above 2048: the same with 2048 or 3072 workgroups in two or three rounds.
static bool pack_two_for(const lsm2d_context* ctx, int n, size_t lds) {
  const int n_cu = ctx->n_cu > 0 ? ctx->n_cu : 256, slots = 4 * n_cu;
  const int rounds = n / slots, extra = n - rounds * slots;      // whole rounds the batch fills, and what is left over
  if (slots != 1024 || rounds < 1 || rounds > kPackMaxRounds || extra == 0 || n >= 4096) return false;      // (balance_order deals 1024 first-round items; the seconds' numbers have 12 bits)
  if (ctx->align_width == 1024) return true;
  if (ctx->align_width != 0) return false;
  if (rounds > 1) return extra <= ctx->pack_extra_max;
  if (ctx->sum_order) return n <= slots + slots / 2 + 64;      // (no narrow kernel in the reference's order of summation; whole step, us per alignment, packed / wide: 1025 1.08 / 1.23, 1100 1.25 / 1.29,
                                                             //  1536 1.05 / 1.09, 1700 1.05 / 1.02, 2047 0.95 / 0.91: profiles/r06/packed_seq_ab_r06X.txt)      // (a few alignments more than two or three rounds hold; whole step, us per alignment, packed / wide: 2049 0.742 / 0.778, 2064 0.827 / 0.868,
                                                            //  2080 0.855 / 0.868, 2100 0.836 / 0.836, 3073 0.723 / 0.745, 3088 0.805 / 0.816: profiles/r06/packed_ab_r06U.txt)
  const size_t per_wg = lds + 1536 + 512;
  int narrow_per_cu = (int) ((160u << 10) / per_wg); if (narrow_per_cu > 8) narrow_per_cu = 8;
  return n <= slots + 24 || n > narrow_per_cu * n_cu;      // (against the narrow kernel, whole step, us per alignment: 1041 0.876 vs 0.895, 1050 0.892 vs 0.888, 1060 0.905 vs 0.882: profiles/r06/packed_ab_r06S.txt)
}

struct RelocStage;      // what the first stage of lsm2d_relocalize_select left on the device (lsm2d_capi_relocalize.inc)
// Everything the stages of one lsm2d_align_batch call share.  The members carry the names the statements below always used.
struct AlignBatch {
  // ---- the call
  lsm2d_context* ctx; const lsm2d_aligner_params* ap; const lsm2d_batch* b;
  Lane* L;      // the lane the call works on: the context's current one when it began (hand_over moves the context on to the other lane, not this)
  float* out_pose; float* out_H; int32_t* out_status; int32_t* out_its; lsm2d_iteration_stats* out_stats; float* out_last_pose; int32_t* out_work; lsm2d_pending* pend;
  bool async; hipStream_t pre, ks;      // begun asynchronously; the stream of what goes AHEAD of k_align (start poses, estimate); the stream of the batch's own operations
  int n, ns, stats_stride, it_cap;
  AlignArgs A;
  // ---- scratch / staging layout: [init_pose | prior | indices | out_pose | out_H | status | its | stats | last_pose | clock | work | ff_rows]
  size_t off, o_pose_in, o_prior, o_fidx[kMaxSlices], o_midx[kMaxSlices], in_bytes, o_pose, o_H, o_status, o_its, o_stats, o_last_pose, o_clock, o_cand, out_bytes, o_work, o_ff_rows, total_bytes;
  int clock_stride, n_clock;
  bool had_inputs; char* hs; char* ds;
  // ---- which path
  bool has_proj, has_nn, has_dist, has_kd, proj_only /* projective slices and no others */, split_ok, use_split, zero_copy;
  bool pair_eligible /* the latency kernel may take the call, its LDS and the split path aside */, use_pair;
  int max_moving;
  // ---- slices, LDS
  int cols_max, fcan_total, max_fixed_rows; const KdCache* kd_cache0;
  size_t lds, pq_bytes, lds_budget, lds_pair0, lds_mov, lds_fix, lds_pair;
  bool proj_culled_for_all, nn_lds_for_all;
  // ---- inputs, results
  bool same_inputs, host_results, stamps;
  // ---- select mode (lsm2d_align_select): the thresholds and k (NULL: every other call), where the rows and the selection's part of the scratch lie, what it hands back
  const lsm2d_select_params* select = nullptr; int32_t select_k = 0;
  size_t o_rows = 0, o_sel = 0;
  lsm2d_iteration_stats* sel_last_stats = nullptr;      // [k] or NULL (out_stats only says that statistics are wanted, as for a begun batch)
  int32_t* sel_index = nullptr; int32_t* sel_n_selected = nullptr; int32_t* sel_n_accepted = nullptr; int32_t* sel_n_success = nullptr;
  // ---- ... per group (lsm2d_align_select_grouped): the groups' layout (NULL: one pool), whose table rides up at the end of the input block; the counts above are [n_groups] then
  const SelectGroupedLayout* groups = nullptr; size_t o_gtab = 0;
  // ---- ... with the inputs ON THE DEVICE (lsm2d_relocalize_select, lsm2d_capi_relocalize.inc): the batch's n slots are filled by a kernel from an earlier
  // stage's selection (reloc_stage_inputs), not from the host.  The descriptor's init_pose / prior / index pointers then only say "there is one" and are never
  // read, every shortcut that assumes the host knows the inputs is off (inline_n1, defer_unpack, the inputs' shadow, the kept placement), the timing bracket is
  // the earlier stage's, and reloc_down_bytes of the scratch and the staging at o_reloc_down hold what the call copies down (reloc_finish)
  RelocStage* reloc = nullptr; size_t reloc_down_bytes = 0, o_reloc_down = 0;

  size_t take(size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t) 255; return o; }
  int reloc_stage_inputs();
  int reloc_finish();
  int validate_and_lay_out_scratch();
  int choose_path();
  int prepare_slices();
  int lay_out_lds();
  int stage_inputs();
  int estimate_only();
  int make_placement();
  int launch();
  int hand_over();
  int select_finish();
};

int AlignBatch::validate_and_lay_out_scratch() {
  async = pend != nullptr; off = 0;
  // what goes AHEAD of k_align (start poses, the placement's estimate): on the second stream while another batch is in flight
  pre = (async && !out_work) ? pre_stream(ctx) : ctx->stream;
  HIPCHK(ctx, join_refill_stream(ctx, pre));      // scans refilled while a batch was in flight: their preprocessing comes before anything this call queues
  n = b->n_alignments, ns = b->n_slices;
  if (n < 0 || ns < 1 || ns > kMaxSlices || ap->max_iterations < 0 || !b->slices || !b->fixed || !b->moving || (n > 0 && !b->init_pose))
    return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: bad batch descriptor");
  if (n == 0) return kEmptyBatch;
  static_assert(sizeof(StatsDev) == sizeof(lsm2d_iteration_stats), "stats layout");
  HIPCHK(ctx, hipSetDevice(ctx->device));

  memset(&A, 0, sizeof A);
  A.n_align = n; A.n_slices = ns; A.max_it = ap->max_iterations; A.min_inliers = ap->min_num_inliers; A.damping = ap->damping;
  if (!(ap->termination_chi_epsilon >= 0.0f)) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: termination_chi_epsilon must be >= 0");
  A.term_eps = ap->termination_chi_epsilon;
  if (ap->max_iterations > 0x3fffffff) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: max_iterations out of range");
  A.inlier_runs = ap->enable_inlier_only_runs != 0;
  stats_stride = lsm2d_stats_capacity(ap), it_cap = A.inlier_runs ? 2 * ap->max_iterations : ap->max_iterations;
  A.stats_stride = stats_stride;
  // ---- device scratch layout: [init_pose | prior | indices | out_pose | out_H | status | its | stats]
  o_pose_in = take(sizeof(float) * 3 * (size_t) n);
  o_prior = b->prior ? take(sizeof(PriorDev) * (size_t) n) : 0;
  for (int s = 0; s < kMaxSlices; ++s) o_fidx[s] = o_midx[s] = 0;
  for (int s = 0; s < ns; ++s) {
    if (b->fixed_index) o_fidx[s] = take(sizeof(int32_t) * (size_t) n);
    if (b->moving_index) o_midx[s] = take(sizeof(int32_t) * (size_t) n);
  }
  if (groups) o_gtab = take(groups->table_bytes());
  in_bytes = off;
  o_pose = take(sizeof(float) * 3 * (size_t) n), o_H = take(sizeof(float) * 9 * (size_t) n);
  o_status = take(sizeof(int32_t) * (size_t) n), o_its = take(sizeof(int32_t) * (size_t) n);
  o_stats = out_stats ? take(sizeof(StatsDev) * (size_t) n * (size_t) stats_stride) : 0;
  o_last_pose = out_last_pose ? take(sizeof(float) * 3 * (size_t) n) : 0;
  // in-kernel clock stamps of ~32 workgroups spread over the grid (timed k_align launches only)
  clock_stride = ctx->clock_stride > 0 ? ctx->clock_stride : (n / 32 > 1 ? n / 32 : 1), n_clock = (n + clock_stride - 1) / clock_stride;
  o_clock = ctx->kernel_timing ? take(sizeof(unsigned long long) * 4 * (size_t) n_clock) : 0;
  o_cand = out_stats ? take(sizeof(int32_t) * 2 * (size_t) n) : 0;      // the candidate lists' books, [2][n] words (AlignArgs::cand_out: every alignment's books, then its builds that fell back from the queue): with the statistics only
  out_bytes = off - o_pose;      // what travels back to the host
  o_work = take(sizeof(int32_t) * (size_t) n);                                                     // balanced placement: the estimate's counts (device only)
  // "fast_forward" 2: H and inlier count of every alignment's last kFfRing iterations (device only; 640 bytes per alignment; needs no clearing: a row is read only after its alignment wrote it)
  o_ff_rows = (ctx->fast_forward == 2 && !out_work) ? take(sizeof(uint32_t) * kFfRowWords * kFfRing * (size_t) n) : 0;
  if (select) {      // the candidates' rows and the selection's own arrays, behind everything the aligner uses (the staging buffer takes the region that comes down at the same offset)
    o_rows = take(sizeof(float) * AlignRow::kWords * (size_t) n);
    o_sel = take(groups ? groups->d_bytes : SelectLayout((size_t) n, (size_t) select_k, AlignRow::kWords).d_bytes);
  }
  if (reloc) o_reloc_down = take(reloc_down_bytes);
  total_bytes = off;
  had_inputs = L->inputs_valid;      // (the lane's scratch still holds the previous batch's input block: ensure_scratch below clears the flag)
  int rc = ensure_scratch(ctx, *L, total_bytes); if (rc) return rc;
  rc = ensure_stage(ctx, *L, total_bytes); if (rc) return rc;
  hs = (char*) L->h_stage; ds = (char*) L->d_scratch;
  return LSM2D_SUCCESS;
}

// Which calls the latency kernel may take, as far as the order of summation goes: every one in the tree order; with "sum_order" 1 (k_align_pair<true>)
// an explicit align_path 3, and -- automatically -- a single alignment (the live tracker's and the standalone aligner's call: DESIGN section 5, the
// tracker step in the reference's order).  Batches of two and more keep k_align_seq, one workgroup per alignment.
static bool pair_order_ok(const lsm2d_context* ctx, int n) {
  return !ctx->sum_order || ctx->align_path == 3 || (ctx->align_path == 0 && n == 1);
}

int AlignBatch::choose_path() {
  // ---- which path: few alignments against a big cloud are spread over many workgroups each (projective slices only)
  has_proj = false, has_nn = false, has_dist = false, has_kd = false;
  max_moving = 0;
  for (int s = 0; s < ns; ++s) {
    const int fd = b->slices[s].finder;
    if (fd == LSM2D_FINDER_PROJECTIVE) has_proj = true; else if (fd == LSM2D_FINDER_NN) has_nn = true; else if (fd == LSM2D_FINDER_KDTREE) has_kd = true; else has_dist = true;
    const lsm2d_cloudset* m = b->moving[s];
    if (m) max_moving = std::max(max_moving, max_cloud_count(m));
  }
  proj_only = has_proj && !has_nn && !has_dist && !has_kd;
  split_ok = proj_only && ap->max_iterations > 0 && n <= 32768;
  // measured (tools/small_batch_bench.py, profiles/r01/small_batch*.jsonl): the split path costs two launches per iteration per
  // alignment call and wins whenever one workgroup per alignment would leave most of the chip idle for long enough
  use_split = split_ok && (ctx->align_path == 2 ||
                                      (ctx->align_path == 0 && n <= 192 && (long long) max_moving * ap->max_iterations >= 400000));
  // A handful of alignments in one launch (the live tracker: one): the kernel reads its few hundred bytes of arguments from, and
  // writes its results to, the PINNED staging buffer directly -- no host-to-device copy, no memset, no device-to-host copy, i.e.
  // three small transfers and their launch latencies off the critical path of the call.
  // (Not for big batches: with 1000 alignments reading their start poses and writing their results over the host link the step takes 1.485 ms
  // against 1.467 with the three small transfers; tools/zero_copy_ab.py.)
  // ("zero_copy_max" bounds every batch, so the A/B knob works below 256 too; batches that carry index arrays stay on the transfers above 256)
  zero_copy = !select && !out_work && !use_split && n <= ctx->zero_copy_max && (n <= 256 || (!b->fixed_index && !b->moving_index));
  pair_eligible = pair_order_ok(ctx, n) && ctx->align_path != 1 && (ns == 1 || ns == 2) && proj_only && (n <= 256 || ctx->align_path == 3) && ap->max_iterations > 0;
  if (zero_copy) ds = (char*) L->h_stage.dev();
  return LSM2D_SUCCESS;
}

int AlignBatch::prepare_slices() {
  // ---- slices
  for (int s = 0; s < ns; ++s)        // ownership first: nothing is launched for a set that is not this context's (or is orphaned)
    if (!b->fixed[s] || !b->moving[s] || b->fixed[s]->ctx != ctx || b->moving[s]->ctx != ctx)
      return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: cloud set missing or from another context");
  {   // scans whose preprocessing is still pending (lsm2d_preprocess_scan_into): one launch for all of them
    const lsm2d_cloudset* rd[2 * kMaxSlices]; int nr = 0;
    for (int s = 0; s < ns; ++s) { rd[nr++] = b->fixed[s]; rd[nr++] = b->moving[s]; }
    const int prc = flush_preprocessing_together(ctx, rd, nr); if (prc) return prc;
  }
  {   // KD-tree slices over scan-sized fixed sets whose trees are not there yet (the live tracker: a new scan per laser and step -- the reference's reset(),
      // correspondence_finder_kd_tree_2d.cpp:6-8,31-38): ALL of them in one launch, side by side, with one wait (kd_scan_launch)
    KdScanPrep preps[kMaxSlices]; int np_ = 0;
    for (int s = 0; s < ns; ++s) {
      const lsm2d_slice_params& sp = b->slices[s];
      if (sp.finder != LSM2D_FINDER_KDTREE) continue;
      const lsm2d_cloudset* f = b->fixed[s];
      float mlr = sp.kd_max_leaf_range; int mlp = sp.kd_min_leaf_points; kd_defaults(mlr, mlp);
      int rc0 = resolve_count(f); if (rc0) return rc0;
      if (kd_cached(f, mlr, mlp) || !kd_scan_eligible(ctx, f)) continue;
      bool dup = false;
      for (int i = 0; i < np_; ++i) dup = dup || preps[i].cs == f;
      if (dup) continue;      // (one set in two slices: built once here; with other parameters the second goes through ensure_kdtree)
      rc0 = flush_pending(f); if (rc0) return rc0;
      rc0 = kd_scan_prepare(ctx, f, mlr, mlp, preps[np_]); if (rc0) return rc0;
      ++np_;
    }
    if (np_ >= 2) { const int rc0 = kd_scan_launch(ctx, preps, np_); if (rc0) return rc0; }
    else if (np_ == 1) { const int rc0 = kd_scan_launch(ctx, preps, 1); if (rc0) return rc0; }
  }
  cols_max = 0, fcan_total = 0;
  kd_cache0 = nullptr;      // the KD-tree set of the (last) KD-tree slice
  for (int s = 0; s < ns; ++s) {
    const lsm2d_slice_params& sp = b->slices[s];
    SliceDev& S = A.s[s];
    const lsm2d_cloudset* f = b->fixed[s]; const lsm2d_cloudset* m = b->moving[s];
    if (!f || !m || f->ctx != ctx || m->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: cloud set missing or from another context");
    // sizes that only the device knows yet (asynchronous clip / merge) are fine for the projective finder -- the kernels read the
    // device-side counts and the host needs upper bounds only; the search structures of the other finders need the numbers
    if (sp.finder != LSM2D_FINDER_PROJECTIVE) { int rc0 = resolve_count(f); if (rc0) return rc0; rc0 = resolve_count(m); if (rc0) return rc0; }
    if (sp.finder != LSM2D_FINDER_PROJECTIVE && sp.finder != LSM2D_FINDER_NN && sp.finder != LSM2D_FINDER_DISTMAP && sp.finder != LSM2D_FINDER_KDTREE)
      return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: unknown finder");
    if (sp.finder == LSM2D_FINDER_PROJECTIVE) {
      if (!make_projk(sp.projector, &S.proj)) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: bad projector");
    } else {
      if ((sp.finder == LSM2D_FINDER_NN || sp.finder == LSM2D_FINDER_KDTREE) && !(sp.max_distance > 0.0f)) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: max_distance must be > 0");
      memset(&S.proj, 0, sizeof S.proj);
    }
    if (!b->fixed_index && f->n_clouds != 1 && f->n_clouds != n) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: fixed set must hold 1 or n_alignments clouds");
    if (!b->moving_index && m->n_clouds != 1 && m->n_clouds != n) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: moving set must hold 1 or n_alignments clouds");
    const int32_t* d_fi = nullptr; const int32_t* d_mi = nullptr;
    if (reloc) {
      // inputs on the device: both index arrays are written there (reloc_stage_inputs) from tables the earlier stage checked against the sets; the
      // descriptor's pointers are not read
      d_fi = (const int32_t*) (ds + o_fidx[s]); d_mi = (const int32_t*) (ds + o_midx[s]);
    } else {
      if (b->fixed_index) {
        const int32_t* src = b->fixed_index + (size_t) s * n;
        for (int i = 0; i < n; ++i) if (src[i] < 0 || src[i] >= f->n_clouds) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: fixed_index out of range");
        memcpy(hs + o_fidx[s], src, sizeof(int32_t) * (size_t) n); d_fi = (const int32_t*) (ds + o_fidx[s]);
      }
      if (b->moving_index) {
        const int32_t* src = b->moving_index + (size_t) s * n;
        for (int i = 0; i < n; ++i) if (src[i] < 0 || src[i] >= m->n_clouds) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: moving_index out of range");
        memcpy(hs + o_midx[s], src, sizeof(int32_t) * (size_t) n); d_mi = (const int32_t*) (ds + o_midx[s]);
      }
    }
    // a fixed set whose upload still sits in its pinned buffer: single-alignment projective calls unpack it in the kernel's prologue
    // (decided once the kernel is known, below); every other reader gets it unpacked by a launch of its own, here (inputs on the device: always here)
    const bool defer_unpack = !reloc && f->unpack_pending && n == 1 && !use_split && proj_only && f != m;
    if (!defer_unpack) { const int urc = flush_pending(f); if (urc) return urc; }
    { const int urc = flush_pending(m); if (urc) return urc; }
    if (sp.finder == LSM2D_FINDER_PROJECTIVE) { const int lrc = ensure_lane_layout(ctx, m); if (lrc) return lrc; }
    // k_align's bin walk gathers both z-buffer winners as 16-byte rows of the sets' AoS copies (not for the calls the latency kernel or the split
    // path will take: the live tracker's sets change every step)
    if (sp.finder == LSM2D_FINDER_PROJECTIVE && !use_split && !pair_eligible && !defer_unpack) {
      int arc = ensure_aos(ctx, f); if (arc) return arc;
      arc = ensure_aos(ctx, m); if (arc) return arc;
    }
    S.fixed = cloud_dev(f, d_fi); S.moving = cloud_dev(m, d_mi);
    S.unpack_src = defer_unpack ? (const float4*) f->h_upload.dev() : nullptr; S.unpack_n = defer_unpack ? f->h_count[0] : 0;
    if (sp.finder == LSM2D_FINDER_NN) { const int grc = ensure_grid(ctx, f, sp.max_distance, &S.fixed.grid); if (grc) return grc; }
    if (sp.finder == LSM2D_FINDER_DISTMAP) { const int grc = ensure_distmap(ctx, f, sp.max_distance, sp.resolution, &S.fixed.dist); if (grc) return grc; }
    if (sp.finder == LSM2D_FINDER_KDTREE) { const int grc = ensure_kdtree(ctx, f, sp.kd_max_leaf_range, sp.kd_min_leaf_points, &S.fixed.kd, &kd_cache0); if (grc) return grc; }
    {   // cooperative NN search pays when the fixed cloud is much denser than the queries (map as fixed, scans as queries)
      const int64_t mf = max_cloud_count(f), mm = std::max(1, max_cloud_count(m));
      S.nn_group = mf >= 4 * mm ? kNNGroup : 1;
    }
    S.finder = sp.finder; S.point_distance = sp.point_distance; S.normal_cos = sp.normal_cos; S.max_distance = sp.max_distance;
    S.cauchy = sp.robustifier == LSM2D_ROBUST_CAUCHY; S.tau = sp.chi_threshold; S.min_corr = sp.min_num_correspondences;
    if (S.cauchy && !(S.tau > 0.0f)) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: chi_threshold must be > 0");
    S.has_sensor = !(sp.sensor_in_robot[0] == 0.0f && sp.sensor_in_robot[1] == 0.0f && sp.sensor_in_robot[2] == 0.0f);
    inverse_host(sp.sensor_in_robot, S.Sinv); sincos_fixed(S.Sinv[2], S.sSinv, S.cSinv);
    S.fcan_offset = fcan_total; fcan_total += S.proj.cols; if (S.proj.cols > cols_max) cols_max = S.proj.cols;
  }
  A.cols_max = cols_max; A.fcan_total = fcan_total;
  A.cull = ctx->cull;      // (the test's column loop wraps once: canvases below 64 columns are not worth it and would need a second wrap)
  for (int s = 0; s < ns; ++s) if (b->slices[s].finder == LSM2D_FINDER_PROJECTIVE && A.s[s].proj.cols < 64) A.cull = 0;
  return LSM2D_SUCCESS;
}

int AlignBatch::lay_out_lds() {
  lds = sizeof(u64) * (size_t) (cols_max + fcan_total + ((cols_max + fcan_total) & 1)) +
               sizeof(float) * kAccumWords * (kAlignBlock / 64);      // moving canvas, fixed canvases (padded to 16 bytes), reduction
  // one NN slice whose fixed clouds are scan-sized (one lane per query): stage each cloud's search tables in LDS.  Budget 38 KB
  // per workgroup keeps four workgroups on a CU; bigger clouds / grids search in global memory as before.  (Measured on configs[1]
  // role A: 3 sqrt(n) cells per side in 38 KB 9.6 ms; 4 sqrt(n) in 50 KB -- three workgroups per CU -- 12.2; 2 sqrt(n) 12.3.)
  // one NN, KD-tree or distance-map slice in the tracker's wiring (scan-sized fixed clouds, a big moving cloud): exact culling of the queries (k_align,
  // "point-query finders"): an occupancy bitmap of the fixed cloud (2 KB) and one keep bit per tile of 64 moving points, out of the same budget
  A.pq_cull_off = 0; A.pq_keep_words = 0;
  pq_bytes = 0;
  if (ns == 1 && ctx->cull && (b->slices[0].finder == LSM2D_FINDER_NN || b->slices[0].finder == LSM2D_FINDER_KDTREE || b->slices[0].finder == LSM2D_FINDER_DISTMAP) &&
      !b->moving[0]->count_pending) {
    const lsm2d_cloudset* f = b->fixed[0]; const lsm2d_cloudset* m = b->moving[0];
    const int mf = max_cloud_count(f), mm = max_cloud_count(m);
    const int keep_words = (((mm + 63) / 64 + kAlignBlock - 1) / kAlignBlock) * (kAlignBlock / 64);
    if (mf <= 16384 && mm >= 4096 && mm > 2 * mf && keep_words <= 512) {
      const int trc = ensure_tile_bounds(ctx, m); if (trc) return trc;
      if (m->derived.d_tile_bounds) { A.pq_keep_words = keep_words; pq_bytes = 128 * 5 * 4 + sizeof(u64) * (size_t) keep_words + 16; A.s[0].moving = cloud_dev_with_tiles(A.s[0].moving, m); }
    }
  }
  lds_budget = 38 * 1024 - pq_bytes;
  A.nn_lds_points = 0; A.nn_lds_cells = 0;
  if (ns == 1 && b->slices[0].finder == LSM2D_FINDER_NN && A.s[0].nn_group == 1) {
    const lsm2d_cloudset* f = b->fixed[0];
    const int mf = max_cloud_count(f);
    int cap = (int) ceil((mf >= 16384 ? 6.0 : 3.0) * sqrt((double) (mf > 0 ? mf : 1))); cap = cap < 16 ? 16 : cap;      // ensure_grid's rule
    const size_t need = sizeof(float2) * (size_t) mf + sizeof(uint16_t) * ((size_t) cap * cap + 4) + sizeof(uint16_t) * ((size_t) mf + 2);
    if (mf > 0 && mf <= 65535 && lds + need <= lds_budget) { A.nn_lds_points = mf; A.nn_lds_cells = cap * cap + 1; lds += need + 16; }
  }
  // one NN slice whose tables stay in global memory (the map is the fixed cloud): every query's cell and the candidate ranges of its 3 x 3 block are
  // cached in LDS from one iteration to the next (32 bytes per query of the biggest moving cloud), same budget
  A.nn_qcache = 0;
  if (ns == 1 && b->slices[0].finder == LSM2D_FINDER_NN && A.nn_lds_points == 0 && ctx->nn_qcache) {
    const lsm2d_cloudset* m = b->moving[0];
    const int mm = max_cloud_count(m);
    lds = (lds + 15) & ~(size_t) 15;
    if (mm > 0 && lds + 32 * (size_t) mm + 16 <= lds_budget) { A.nn_qcache = mm; lds += 32 * (size_t) mm + 16; }
  }
  // one KD-tree slice: the top of the fixed cloud's tree (up to "kd_lds_nodes" nodes, 24 bytes each) rides in LDS -- same 38 KB budget
  A.kd_lds_nodes = 0; A.kd_lds_points = 0;
  if (ns == 1 && b->slices[0].finder == LSM2D_FINDER_KDTREE && kd_cache0 && ctx->kd_lds_nodes > 0) {
    int k = kd_cache0->max_nodes_per_cloud < ctx->kd_lds_nodes ? kd_cache0->max_nodes_per_cloud : ctx->kd_lds_nodes;
    const size_t room = lds < lds_budget ? (lds_budget - lds) / (sizeof(float4) + sizeof(int2)) : 0;
    if ((size_t) k > room) k = (int) room;
    if (k > 0) { A.kd_lds_nodes = k; lds += (size_t) k * (sizeof(float4) + sizeof(int2)) + 16; }
    // scan-sized fixed clouds whose whole tree fits: the leaf arrays too (coordinates and normals: 16 bytes per point)
    const lsm2d_cloudset* f = b->fixed[0];
    const int mf = max_cloud_count(f);
    const size_t need = (size_t) (mf + 2) * (sizeof(float2) + sizeof(float2)) + 32;
    if (k > 0 && k == kd_cache0->max_nodes_per_cloud && mf > 0 && mf <= 65535 && lds + need <= lds_budget) { A.kd_lds_points = mf; lds += need; }
  }
  if (pq_bytes) { lds = (lds + 15) & ~(size_t) 15; A.pq_cull_off = (int32_t) lds; lds += pq_bytes; }
  ctx->last_query_cull = A.pq_cull_off > 0;
  // the projective instantiation with the culled stream only: every slice's moving set has its lane-chunked copy and chunk circles, and culling is on
  // (its unit lists -- kCullBlocks x 512 16-bit entries per slice, kept across iterations -- sit behind everything else in dynamic LDS)
  proj_culled_for_all = proj_only && A.cull == 1 && ctx->proj_modes;
  for (int s = 0; s < ns && proj_culled_for_all; ++s)
    proj_culled_for_all = A.s[s].moving.lane_xy != nullptr && A.s[s].moving.lane_bounds != nullptr && A.s[s].moving.block_bounds != nullptr;
  A.units_off = 0; A.cull_keep = ctx->cull_keep; A.fast_forward = ctx->fast_forward;
  A.ff_rows = (ctx->fast_forward == 2 && !out_work) ? (uint32_t*) ((char*) L->d_scratch + o_ff_rows) : nullptr;      // (the lane's DEVICE scratch whatever path the call takes: a zero-copy launch does not fast-forward)
  A.cull_mt = ctx->cull_keep ? 1e-6f * (float) ctx->cull_margin_um : 0.0f; A.cull_mth = ctx->cull_keep ? 1e-6f * (float) ctx->cull_margin_urad : 0.0f; A.cull_mt2 = A.cull_mt * A.cull_mt;      // (lists rebuilt every iteration: no margins)
  if (proj_culled_for_all) {
    int nb_max = kCullBlocks;
    for (int s = 0; s < ns; ++s) if (b->moving[s]->block_stride > nb_max) nb_max = b->moving[s]->block_stride;
    A.units_stride = nb_max * kAlignBlock;
    const size_t at = (lds + 15) & ~(size_t) 15, need = sizeof(uint16_t) * (size_t) ns * (size_t) A.units_stride;
    if ((int) (at + need) + 2048 <= ctx->max_dyn_lds && at + need + 2048 <= 40 * 1024) { A.units_off = (int32_t) at; lds = at + need; }      // four workgroups per CU must still fit (160 KB)
    else proj_culled_for_all = false;
  }
  // Round 20: a single slice's candidate list (lsm2d_device.h) behind the unit lists -- a word per column, then up to "cand_cap" 32-bit entries -- for the batches it pays for
  // and by room, launched as k_align_cand; every other batch runs the kernel it always ran.  The rules, each from a measurement (DESIGN section 5):
  //  - room: four workgroups per CU must still fit, and only the wide unpacked form carries the code: not with "sum_order" 1, and not where the batch takes the narrow or
  //    the packed form with or without the list's bytes (they are chosen by the workgroups a CU holds: align_width_for, pack_two_for);
  //  - at most ONE dispatch round (4 workgroups x the CUs): what the lists shorten is the tail a few long alignments leave on an emptying chip.  A batch of many rounds
  //    has no such tail -- the next round fills the slots -- and there the builds of the many alignments that are done after three to five iterations are pure cost
  //    (65 536 candidates: 15.2 -> 19.6 ms per step with lists);
  //  - a moving cloud whose lists can fit: the candidates grow with the cloud's density -- about 2 % of a 100k-point map's points -- and a list that outgrows its room is a
  //    wasted build (1M points: every list overflowed, 3.9 -> 6.6 ms per step).  48 points of cloud per entry of room is the bound; the kernel, for its part, does not
  //    build a second list for an alignment whose first one was too long;
  //  - no other batch in flight: a batch begun while another one runs has its tail under that one's launch or the next one's, so there is nothing to shorten, while the
  //    build's passes and the list's LDS -- room the next batch's pre-kernels would have found free -- are paid (the streamed pipeline: 0.362 - 0.368 -> 0.381 - 0.384 ms per
  //    step with lists, profiles/r20/stream_ab.txt).  A batch begun alone and waited for gets its lists.
  A.cand_off = 0;
  const int one_round = 4 * (ctx->n_cu > 0 ? ctx->n_cu : 256);
  if (proj_culled_for_all && ns == 1 && ctx->cand_lists && ctx->cull_keep && !ctx->sum_order && cols_max <= 16384 && n <= one_round && !(async && ctx->inflight >= 1)) {
    const size_t at = (lds + 15) & ~(size_t) 15, bits = sizeof(uint32_t) * (size_t) cand_blocker_words(cols_max);
    const size_t limit = std::min((size_t) 40 * 1024, (size_t) (ctx->max_dyn_lds > 0 ? ctx->max_dyn_lds : 0));
    long long cap = at + bits + 2048 < limit ? (long long) ((limit - 2048 - at - bits) / sizeof(uint32_t)) : 0;
    const bool cloud_fits = (long long) max_moving <= 48ll * cap;      // (against the room, not against a capacity the caller lowered)
    if (cap > ctx->cand_cap) cap = ctx->cand_cap;
    if (cap >= 64 && cloud_fits) {
      const size_t with = at + bits + sizeof(uint32_t) * (size_t) cap;
      const bool wide = align_width_for(ctx, n, lds) == kAlignBlock && align_width_for(ctx, n, with) == kAlignBlock;
      const bool balanced = !use_split && !zero_copy && A.cull && ctx->balance && n > 256 && n <= 4096;      // (make_placement's condition for a placement, hence for packing)
      const bool packed = balanced && (pack_two_for(ctx, n, lds) || pack_two_for(ctx, n, with));
      if (wide && !packed) {
        A.cand_off = (int32_t) at; A.cand_cap = (int32_t) cap; lds = with;
        A.cand_first_it = ctx->cand_first_it; A.cand_max_builds = ctx->cand_max_builds;
        A.cand_mt = 1e-6f * (float) ctx->cand_margin_um; A.cand_mth = 1e-6f * (float) ctx->cand_margin_urad;
        // Round 30: the queue of maybes, "cand_queue_cap" entries per alignment in device memory of the lane's (at most one dispatch round of 16 384: 64 MB); "cand_queue" 0: none
        A.cand_qcap = ctx->cand_queue ? ctx->cand_queue_cap : -1;
        if (A.cand_qcap > 0) {
          const size_t qbytes = sizeof(uint32_t) * (size_t) n * (size_t) A.cand_qcap;      // (grown on demand like the scratch, to the byte; never cleared: a region is read only up to what its alignment has just written)
          HIPCHK(ctx, L->d_cand_queue.ensure(qbytes, qbytes, wait_for_stream(ctx)));
          A.cand_queue = (uint32_t*) L->d_cand_queue;
        }
      }
    }
  }
  // "sum_order" 1: the trip's pair records (lsm2d_device.h), behind everything else -- three workgroups per CU instead of four
  A.seq_off = 0;
  if (ctx->sum_order) { lds = (lds + 15) & ~(size_t) 15; A.seq_off = (int32_t) lds; lds += kSeqLdsBytes; }
  // the NN instantiation without the search in global memory: the staging holds every alignment's tables (sized for the largest fixed cloud above), and no
  // alignment takes the cooperative loop, which searches in global memory (the kernel's rule: fixed cloud >= 4 x moving cloud) -- whatever the pairing
  nn_lds_for_all = false;
  if (A.nn_lds_points > 0 && ctx->nn_lds_only && !b->moving[0]->count_pending && !b->fixed[0]->count_pending) {
    const lsm2d_cloudset* f = b->fixed[0]; const lsm2d_cloudset* m = b->moving[0];
    const long long mf = max_cloud_count(f); long long mn = 0x7fffffff;
    for (int c = 0; c < m->n_clouds; ++c) if (m->h_count[c] < mn) mn = m->h_count[c];
    nn_lds_for_all = m->n_clouds > 0 && mf < 4 * mn;
  }
  if ((int) lds + 512 > ctx->max_dyn_lds) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "align_batch: canvases do not fit LDS");
  // one or two projective slices and too few alignments to fill the chip (the live tracker: one alignment per scan): the latency
  // kernel (k_align_pair; bit-identical sums) -- 512 threads per slice, two slices' passes side by side instead of one after the
  // other, registers to spare for the serial solve step.  Measured against k_align on single-slice calls (tools/latency_kernel_ab.py):
  // 1 scan vs 10k points 0.163 -> 0.146 ms, vs a 700-point clipped scene with prior 0.063 -> 0.045, 256 candidates 0.172 -> 0.154
  // its LDS: fixed winners and canvases as k_align, a moving canvas and a block of wave totals per slice, and -- room permitting --
  // the moving clouds themselves (kPairMovCap points of 16 bytes per slice)
  lds_pair0 = sizeof(float4) * (size_t) fcan_total + sizeof(u64) * (size_t) fcan_total +
                           (size_t) ns * (sizeof(u64) * (size_t) cols_max + sizeof(float) * kPairRedStride * (kAlignBlock / 64));
  // ("sum_order" 1, k_align_pair<true>: a buffer of pair records per slice behind the canvases -- counted before the clouds, which are staged only if there is room)
  if (ctx->sum_order) lds_pair0 += (size_t) ns * kSeqLdsBytes;
  lds_mov = (size_t) ns * kPairMovCap * sizeof(float4);
  A.pair_mov_cap = (int) (lds_pair0 + lds_mov) + 512 <= ctx->max_dyn_lds ? kPairMovCap : 0;
  // ... and the fixed clouds (sizes the host knows, or upper bounds of sizes only the device knows: the kernel compares the real ones)
  max_fixed_rows = 0;
  for (int s = 0; s < ns; ++s) max_fixed_rows = std::max(max_fixed_rows, max_cloud_count(b->fixed[s]));
  max_fixed_rows = (max_fixed_rows + 63) & ~63;
  lds_fix = (size_t) ns * (size_t) max_fixed_rows * sizeof(float4);
  A.pair_fix_cap = max_fixed_rows <= 4096 && (int) (lds_pair0 + (A.pair_mov_cap ? lds_mov : 0) + lds_fix) + 512 <= ctx->max_dyn_lds ? max_fixed_rows : 0;
  lds_pair = lds_pair0 + (A.pair_mov_cap ? lds_mov : 0) + (A.pair_fix_cap ? lds_fix : 0);
  // ("sum_order" 1: the latency kernel's reference-order form, k_align_pair<true>, for the calls pair_order_ok admits; the others take k_align_seq)
  use_pair = pair_eligible && !use_split && (int) lds_pair + 512 <= ctx->max_dyn_lds;
  return LSM2D_SUCCESS;
}

int AlignBatch::stage_inputs() {
  // ---- inputs
  if (reloc) {
    // inputs on the device: the host stages nothing -- b->init_pose / b->prior only say "there is one" -- and a single slot's start pose and prior cannot ride
    // in the kernel arguments, which the host would have to know
    if (b->prior) A.prior = (const PriorDev*) (ds + o_prior);
    A.inline_n1 = 0;
  } else {
    memcpy(hs + o_pose_in, b->init_pose, sizeof(float) * 3 * (size_t) n);
    if (b->prior) {
      PriorDev* p = (PriorDev*) (hs + o_prior);
      for (int i = 0; i < n; ++i) {
        inverse_host(b->prior[i].z, p[i].z_inv); sincos_fixed(p[i].z_inv[2], p[i].sz, p[i].cz);
        memcpy(p[i].omega, b->prior[i].omega, sizeof(float) * 9);
      }
      A.prior = (const PriorDev*) (ds + o_prior);
    }
    // one alignment (the live tracker's call): start pose and prior ride in the kernel arguments, so the kernel's prologue does not
    // wait for a read of host memory
    A.inline_n1 = n == 1 && !use_split;
    if (A.inline_n1) { memcpy(A.pose1, b->init_pose, sizeof A.pose1); if (b->prior) memcpy(&A.prior1, hs + o_prior, sizeof A.prior1); }
  }
  if (groups) memcpy(hs + o_gtab, groups->table.data(), groups->table_bytes());
  // the stream this batch's own operations go to: its lane's when it was begun asynchronously (lane_stream) -- not for the split path (one workspace per context).
  // Everything queued so far went to the context's stream (set preparation: pending preprocessing, trees, lane copies): an
  // event behind it orders the lane's stream and the pre-kernels' stream
  ks = (async && !out_work && !use_split) ? lane_stream(ctx) : ctx->stream;
  if (ks != ctx->stream && pre != ctx->stream) {
    HIPCHK(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(pre, ctx->ev_main, 0));
  }
  // Round 5: a batch that comes again with the SAME input block (start poses, index arrays; no priors) while nothing else has touched the lane's scratch needs no
  // upload: the blit and the wait behind it are 8 us of a 0.77 ms step (kernel trace: copy 2.4 us + 5.6 us until k_align starts).  Compared byte for byte against a
  // host-side shadow of what was uploaded last -- up to 64 KB; a sweep's index arrays beyond that are uploaded as before.
  if (reloc) {
    // inputs on the device: the block is written where it lies, on the stream of what goes ahead of the estimate and the aligner.  The host holds no copy of it:
    // nothing to compare, nothing to upload, and no shadow for a later batch to compare against
    same_inputs = false;
    L->inputs_shadow.clear();
    const int rrc = reloc_stage_inputs(); if (rrc) return rrc;
  } else {
    same_inputs = !zero_copy && !out_work && !b->prior && had_inputs && in_bytes <= (64u << 10) && L->inputs_shadow.size() == in_bytes &&
                             !memcmp(L->inputs_shadow.data(), hs, in_bytes);
    if (!zero_copy && !same_inputs) {
      HIPCHK(ctx, hipMemcpyAsync(ds, hs, in_bytes, hipMemcpyHostToDevice, pre));
      if (!out_work && !b->prior && in_bytes <= (64u << 10)) L->inputs_shadow.assign((const unsigned char*) hs, (const unsigned char*) hs + in_bytes); else L->inputs_shadow.clear();
    }
  }
  L->inputs_valid = !zero_copy && !L->inputs_shadow.empty();
  A.init_pose = (const float*) (ds + o_pose_in);
  // the SMALL results of a batch that travels by copies (56 bytes per alignment + the clock stamps) are written by the kernels straight into the pinned
  // staging buffer: the device-to-host copy behind the launch -- a hand-over to the copy engine, 9 us of gap + 6 us of copy on the timeline of a
  // 1000-alignment step -- is gone, the stream wait ends with the kernel.  The statistics (28 bytes per iteration and alignment) stay on the device and are copied.
  host_results = !select && !zero_copy && !use_split && ctx->results_to_host && n > 0;      // (select mode: k_align_rows reads them where the kernels leave them, on the device)
  char* const ro = host_results ? (char*) L->h_stage.dev() : ds;
  A.out_pose = (float*) (ro + o_pose); A.out_H = (float*) (ro + o_H); A.out_status = (int32_t*) (ro + o_status); A.out_its = (int32_t*) (ro + o_its);
  A.out_stats = out_stats ? (StatsDev*) (ds + o_stats) : nullptr;
  A.out_last_pose = out_last_pose ? (float*) (ro + o_last_pose) : nullptr;
  A.cand_out = out_stats ? (int32_t*) (ro + o_cand) : nullptr;

  ctx->last_clock_khz = 0; ctx->last_wg_lifetime_ns = 0;
  stamps = ctx->kernel_timing && !use_split && !use_pair;
  if (stamps) { A.clock_out = (unsigned long long*) ((host_results ? (char*) L->h_stage.dev() : ds) + o_clock); A.clock_stride = clock_stride; }
  A.host_polls = zero_copy;
  if (zero_copy) {
    memset(hs + o_pose, 0, out_bytes);
    int32_t* st = (int32_t*) (hs + o_status);
    for (int i = 0; i < n; ++i) st[i] = kStatusNotWritten;          // the kernels write an alignment's status last (release, system scope)
  }
  else {
    // every alignment's pose, information matrix, status and iteration count are written by its workgroup whatever happens to it; what a kernel may leave
    // untouched are the statistics of iterations that never started: only those are cleared (the clock stamps of a timed launch are written by every
    // stamping workgroup -- each alignment runs exactly once, wherever the placement puts it)
    if (out_stats) HIPCHK(ctx, hipMemsetAsync(ds + o_stats, 0, sizeof(StatsDev) * (size_t) n * (size_t) stats_stride, ks));
    // ... and "exactly once" is checked, not assumed (round-4 advisor): the status words start as kStatusNotWritten -- in the pinned buffer the kernels write to, a
    // host memset of 4 n bytes; on the device for the paths that copy -- and one that is still unwritten after the wait turns the call into LSM2D_DEVICE_ERROR
    if (host_results) memset(hs + o_status, 0xFF, sizeof(int32_t) * (size_t) n);
    else HIPCHK(ctx, hipMemsetAsync(ds + o_status, 0xFF, sizeof(int32_t) * (size_t) n, ks));
    if (out_stats) { if (host_results) memset(hs + o_cand, 0, sizeof(int32_t) * 2 * (size_t) n); else HIPCHK(ctx, hipMemsetAsync(ds + o_cand, 0, sizeof(int32_t) * 2 * (size_t) n, ks)); }      // (the paths without lists write nothing there)
  }
  ctx->last_align_path = use_split ? 2 : (use_pair ? 3 : 1);
  return LSM2D_SUCCESS;
}

// (A.order / A.wg_place and the estimate's margins: set for every batch, read by both forms below)
int AlignBatch::estimate_only() {      // lsm2d_estimate_work: the chunks of the moving cloud each alignment's FIRST iteration will stream (k_cull_estimate), or 1 everywhere
  int bs = -1;
  for (int s = 0; s < ns && bs < 0; ++s) if (A.s[s].finder == LSM2D_FINDER_PROJECTIVE && A.s[s].moving.lane_xy && A.s[s].moving.lane_bounds && A.cull) bs = s;
  if (bs < 0) { for (int i = 0; i < n; ++i) out_work[i] = 1; return LSM2D_SUCCESS; }
  int32_t* d_work = (int32_t*) ((char*) L->d_scratch + o_work);
  hipLaunchKernelGGL(k_cull_estimate, dim3((unsigned) n), dim3(kAlignBlock), sizeof(u64) * (size_t) A.s[bs].proj.cols, ctx->stream, A, bs, d_work, (int32_t*) nullptr, (const int32_t*) nullptr, ctx->n_cu, (unsigned int*) nullptr);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(hs + o_work, d_work, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  memcpy(out_work, hs + o_work, sizeof(int32_t) * (size_t) n);
  return LSM2D_SUCCESS;
}

int AlignBatch::make_placement() {
  // culled batches that run in about one dispatch round: balanced placement (one small launch ahead of k_align; see k_cull_estimate)
  A.order = nullptr; A.wg_place = nullptr;
  A.cull_est_mt = 1e-6f * (float) ctx->cull_est_um; A.cull_est_mth = 1e-6f * (float) ctx->cull_est_urad;
  if (out_work) return LSM2D_SUCCESS;
  // (a batch of many dispatch rounds balances itself, and the estimate of 65 536 alignments costs more than its heaviest-first order saves:
  // configs[3] 47.6 vs 47.2 ms per step -- the placement is for batches of up to four rounds)
  ctx->last_cull_estimate = 0;
  if (!use_split && !use_pair && !zero_copy && A.cull && ctx->balance && n > 256 && n <= 4096 && has_proj) {
    int bs = -1;
    for (int s = 0; s < ns && bs < 0; ++s) if (A.s[s].finder == LSM2D_FINDER_PROJECTIVE && A.s[s].moving.lane_xy && A.s[s].moving.lane_bounds) bs = s;
    if (bs >= 0) {
      int32_t* d_work = (int32_t*) ((char*) L->d_scratch + o_work);
      // the workgroups of the previous launch of the same shape noted the CU they ran on (AlignArgs::wg_place): the placement groups by those notes
      // (round 6) packed: one dispatch round of 4 n_cu workgroups, the lightest alignments two to a workgroup (pack_two_for; the pairs are made by balance_order)
      const bool packed = proj_culled_for_all && pack_two_for(ctx, n, lds);
      const unsigned long long shape = ((unsigned long long) (unsigned) n << 32) ^ ((unsigned long long) lds << 8) ^ (unsigned long long) (proj_culled_for_all ? 5 : 0) ^ (packed ? 0x80ull : 0ull);
      if (!ctx->d_wg_place) {      // 1024 notes + the estimate's ticket counter
        HIPCHK(ctx, ctx->d_wg_place.alloc(sizeof(int32_t) * 1025)); ctx->wg_place_shape = 0;
        HIPCHK(ctx, hipMemsetAsync(ctx->d_wg_place, 0, sizeof(int32_t) * 1025, pre));      // (on the stream the estimate that reads the ticket is queued on)
      }
      if (!L->d_order) { HIPCHK(ctx, L->d_order.alloc(sizeof(int32_t) * kOrderInts)); L->order_valid = false; }
      const bool notes = ctx->balance_notes && ctx->wg_place_shape == shape;
      // Round 5: the order lives in a buffer of its own and is KEPT.  A caller that runs the same batch again -- the same sets (uid and version), index arrays,
      // slice parameters, launch shape and START POSES: a candidate sweep re-scored, bench.py's resident step -- gets the placement made for it the first time
      // with notes, and no estimate launch (33 us of a 0.8 ms step).  Anything that differs makes it afresh; only where alignments run depends on it, never a result.
      unsigned long long key = 1469598103934665603ull;
      auto mix = [&](const void* p, size_t bytes) { const unsigned char* q = (const unsigned char*) p; for (size_t i = 0; i < bytes; ++i) { key ^= q[i]; key *= 1099511628211ull; } };
      mix(&shape, sizeof shape); mix(&bs, sizeof bs); mix(&A.cull_est_mt, 4); mix(&A.cull_est_mth, 4); mix(&ns, sizeof ns); mix(&packed, sizeof packed);
      for (int s = 0; s < ns; ++s) {
        const unsigned long long id[4] = {b->fixed[s]->uid, b->fixed[s]->version, b->moving[s]->uid, b->moving[s]->version};
        mix(id, sizeof id); mix(&b->slices[s], sizeof(lsm2d_slice_params));
        if (b->fixed_index && !reloc) mix(b->fixed_index + (size_t) s * n, sizeof(int32_t) * (size_t) n);
        if (b->moving_index && !reloc) mix(b->moving_index + (size_t) s * n, sizeof(int32_t) * (size_t) n);
      }
      // (inputs made on the device: the host cannot tell whether they are a batch it has placed before -- the estimate runs, behind the kernel that writes the
      // poses on the same stream, and what it leaves in d_order is nobody's to keep)
      const bool reuse = !reloc && ctx->estimate_reuse && notes && L->order_valid && L->order_key == key && L->order_poses.size() == 3 * (size_t) n &&
                         !memcmp(L->order_poses.data(), b->init_pose, sizeof(float) * 3 * (size_t) n);
      // A batch begun while another one is in flight starts on the slots that one's tail leaves free -- wherever they are: the launch balances itself as a batch
      // of many dispatch rounds does, and what is left of the placement's gain (2 % with a kept order) is less than the estimate's own chip time when it has to be made
      // afresh (streamed pipeline 0.685 against 0.696 ms per step): no estimate then, workgroup b = alignment b.  A kept order is still used -- and a batch this
      // lane has seen before (same sets, versions, parameters: a caller that runs it again and again) gets its estimate once, to be kept from then on.
      const bool joins_a_batch_in_flight = ks != ctx->stream && ctx->inflight >= 1 && ctx->lane_streams;
      if (!reuse && joins_a_batch_in_flight && !(ctx->estimate_reuse && L->order_key == key)) { L->order_valid = false; L->order_key = key; }
      else {
      if (!reuse) {
        size_t est_lds = sizeof(u64) * (size_t) A.s[bs].proj.cols; if (est_lds < sizeof(BalanceLds)) est_lds = sizeof(BalanceLds);
        // (estimates share ONE ticket counter: one queued on the second stream waits for the latest one queued on the first)
        if (pre != ctx->stream && ctx->a_est_recorded) HIPCHK(ctx, hipStreamWaitEvent(pre, ctx->ev_a_est, 0));
        if (pre == ctx->stream && ctx->side_pre.recorded) HIPCHK(ctx, hipStreamWaitEvent(pre, ctx->side_pre.ev, 0));      // (... and the other way round: a synchronous call while a begun batch's estimate may still be running)
        hipLaunchKernelGGL(k_cull_estimate, dim3((unsigned) n), dim3(kAlignBlock), est_lds, pre, A, bs, d_work, L->d_order,
                           notes ? (const int32_t*) ctx->d_wg_place : (const int32_t*) nullptr, ctx->n_cu, (unsigned int*) (ctx->d_wg_place + 1024),
                           packed ? L->d_order + kPackOrder2At : (int32_t*) nullptr);
        const hipError_t le = hipGetLastError();
        if (le == hipSuccess && pre == ctx->stream) { HIPCHK(ctx, hipEventRecord(ctx->ev_a_est, ctx->stream)); ctx->a_est_recorded = true; }
        if (le != hipSuccess) {      // (round-4 advisor) a launch that failed may have left the ticket counter mid-count: the next call must not start mis-counted
          (void) hipMemsetAsync(ctx->d_wg_place + 1024, 0, sizeof(int32_t), ctx->stream); L->order_valid = false;
          HIPCHK(ctx, le);
        }
        ctx->last_cull_estimate = 1;
        // (kept only once it was made WITH notes: the first call of a shape orders by the round-3 assumption, the second by what the first really did)
        L->order_valid = notes && !reloc; L->order_key = key;
        if (notes && !reloc) L->order_poses.assign(b->init_pose, b->init_pose + 3 * (size_t) n);
      }
      A.order = L->d_order;
      if (packed) A.order2 = L->d_order + kPackOrder2At;      // (kept with the order: a batch that comes again with the same start poses finds both)
      if (ctx->balance_notes && ((packed && n < 2048) || n <= 1024)) { A.wg_place = ctx->d_wg_place; ctx->wg_place_shape = shape; }      // (one note per workgroup of a launch of at most 1024)
      }
    }
  }
  return LSM2D_SUCCESS;
}

int AlignBatch::launch() {
  if (ks != ctx->stream) {      // ... and the lane's stream behind everything the context's own stream was given up to here (set preparation; with nothing in flight also this batch's start poses and estimate)
    HIPCHK(ctx, hipEventRecord(ctx->ev_main, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ks, ctx->ev_main, 0));
  }
  HIPCHK(ctx, join_pre_stream(ctx, ks));      // whatever the second stream holds for this batch (its start poses, its estimate) comes first
  if (ctx->kernel_timing && !reloc) HIPCHK(ctx, hipEventRecord(L->ev0, ks));      // (lsm2d_relocalize_select: the bracket was begun by the stage in front, on its lane)
  if (use_split) {
    // workspace: global canvases + running pose / flags, grown on demand and kept by the context
    const size_t can_bytes = sizeof(u64) * 2 * (size_t) fcan_total * (size_t) n;
    const size_t w_pose = (can_bytes + 255) & ~(size_t) 255, w_done = w_pose + (((sizeof(float) * 3 * (size_t) n) + 255) & ~(size_t) 255);
    const size_t w_H = w_done + (((sizeof(int32_t) * (size_t) n) + 255) & ~(size_t) 255), w_last = w_H + (((sizeof(float) * 9 * (size_t) n) + 255) & ~(size_t) 255);
    const size_t w_phase = w_last + ((sizeof(StatsDev) * (size_t) n + 255) & ~(size_t) 255);
    const size_t w_total = w_phase + sizeof(int32_t) * 3 * (size_t) n;
    HIPCHK(ctx, ctx->d_split.ensure(w_total, w_total + w_total / 2, wait_for_stream(ctx)));
    char* w = (char*) ctx->d_split;
    SplitArgs SA; SA.A = A;
    SA.gcan = (u64*) w; SA.pose = (float*) (w + w_pose); SA.done = (int32_t*) (w + w_done); SA.H_last = (float*) (w + w_H); SA.last = (StatsDev*) (w + w_last);
    SA.phase = (int32_t*) (w + w_phase);
    HIPCHK(ctx, hipMemsetAsync(SA.gcan, 0xFF, can_bytes, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(SA.done, 0, sizeof(int32_t) * (size_t) n, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(SA.phase, 0, sizeof(int32_t) * 3 * (size_t) n, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(SA.pose, A.init_pose, sizeof(float) * 3 * (size_t) n, hipMemcpyDeviceToDevice, ctx->stream));
    int max_fixed = 0;
    for (int s = 0; s < ns; ++s) max_fixed = std::max(max_fixed, max_cloud_count(b->fixed[s]));
    auto chunks_for = [&](int max_points) {
      int c = (max_points / 2 + 2047) / 2048;                 // >= 4 pairs per thread and chunk
      const int budget = 2048 / (n * ns) > 1 ? 2048 / (n * ns) : 1;
      if (c > budget) c = budget;
      return c < 1 ? 1 : c;
    };
    const size_t clds = sizeof(u64) * (size_t) cols_max;
    SA.it = 0;
    hipLaunchKernelGGL((k_split_project<true>), dim3((unsigned) chunks_for(max_fixed), (unsigned) n, (unsigned) ns), dim3(512), clds, ctx->stream, SA);
    const int mchunks = chunks_for(max_moving);
    for (int it = 0; it < it_cap; ++it) {      // (alignments that are done leave their launches at once: S.done)
      SA.it = it;
      hipLaunchKernelGGL((k_split_project<false>), dim3((unsigned) mchunks, (unsigned) n, (unsigned) ns), dim3(512), clds, ctx->stream, SA);
      if (ctx->sum_order) hipLaunchKernelGGL(k_split_finish<true>, dim3((unsigned) n), dim3(kAlignBlock), 0, ctx->stream, SA);
      else hipLaunchKernelGGL(k_split_finish<false>, dim3((unsigned) n), dim3(kAlignBlock), 0, ctx->stream, SA);
    }
  } else {
    const dim3 grid((unsigned) n), block(kAlignBlock);
    if (use_pair) hipLaunchKernelGGL(ctx->sum_order ? k_align_pair<true> : k_align_pair<false>, grid, dim3((unsigned) (kAlignBlock * ns)), lds_pair, ks, A);
    else {
      // which instantiation: the finders the batch's slices use, and -- for a batch of ONE finder kind -- the form of its inner loop the host could prove
      // serves every alignment (kNNMode of align_body).  One table (round 5; a 12-way ladder before); the mixed instantiations take whatever is left.
      const unsigned finders = (has_proj ? kFProj : 0u) | (has_nn ? kFNN : 0u) | (has_dist ? kFDist : 0u) | (has_kd ? kFKd : 0u);
      int mode = 0;
      if (finders == kFProj) mode = proj_culled_for_all ? 5 : 0;                                                                       // every slice: the culled stream over kept unit lists
      else if (finders == kFNN) mode = A.nn_lds_points == 0 ? 1 : (nn_lds_for_all ? 2 : 0);                        // tables in global memory / in LDS for every alignment
      else if (finders == kFKd && ns == 1 && ctx->kd_modes) mode = A.kd_lds_points > 0 ? 3 : 4;                    // whole trees in LDS / only their tops
      AlignKernel fn = nullptr;
      if (ctx->sum_order) {      // the reference's order of summation: k_align_seq, the culled projective stream or the finder kind's general form
        if (mode != 5) mode = 0;
        for (const AlignVariant& v : kAlignVariantsSeq) if (v.finders == finders && v.mode == mode) { fn = v.fn; break; }
        if (!fn) fn = has_kd ? (AlignKernel) k_align_seq<true, true, true, true> : (AlignKernel) k_align_seq<true, true, true>;
      }
      else
      for (const AlignVariant& v : kAlignVariants) if (v.finders == finders && v.mode == mode) { fn = v.fn; break; }
      if (!fn) fn = has_kd ? (AlignKernel) k_align<true, true, true, true> : (AlignKernel) k_align<true, true, true>;      // mixed finders
      // Round 6: the culled projective stream in NARROW workgroups for batches that would otherwise leave a dispatch round nearly empty (align_width_for)
      const int width = (mode == 5 && !ctx->sum_order) ? align_width_for(ctx, n, lds) : kAlignBlock;
      ctx->last_align_width = width;
      if (A.order2) { ctx->last_align_width = 1024; hipLaunchKernelGGL(ctx->sum_order ? k_align_seq_two : k_align_two, dim3((unsigned) ((n / (4 * ctx->n_cu)) * (4 * ctx->n_cu))), block, lds, ks, A); }      // (packed: two alignments in some workgroups, one dispatch round: make_placement)
      else
      if (width == 256) hipLaunchKernelGGL(k_align_narrow<256>, grid, dim3(256), lds, ks, A);
      else
      hipLaunchKernelGGL(A.cand_off > 0 && mode == 5 && !ctx->sum_order ? (AlignKernel) k_align_cand : fn, grid, block, lds, ks, A);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  for (int s = 0; s < ns; ++s)                  // sets the kernel's prologue unpacks (SliceDev::unpack_src)
    if (A.s[s].unpack_src) { b->fixed[s]->unpack_pending = false; b->fixed[s]->staged_epoch = ctx->sync_epoch; }
  if (select) return LSM2D_SUCCESS;      // the results stay where they are; the timing bracket ends behind the selection (select_finish)
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L->ev1, ks));
  ctx->have_timing = ctx->kernel_timing;
  if (host_results) { if (out_stats) HIPCHK(ctx, hipMemcpyAsync(hs + o_stats, ds + o_stats, sizeof(StatsDev) * (size_t) n * (size_t) stats_stride, hipMemcpyDeviceToHost, ks)); }
  else if (!zero_copy) HIPCHK(ctx, hipMemcpyAsync(hs + o_pose, ds + o_pose, out_bytes, hipMemcpyDeviceToHost, ks));
  return LSM2D_SUCCESS;
}

int AlignBatch::hand_over() {
  if (select) return reloc ? reloc_finish() : select_finish();
  // ---- the batch is queued.  What its results need: kept in a lsm2d_pending (the caller's for an asynchronous begin, a local one otherwise)
  lsm2d_pending local; lsm2d_pending& P = pend ? *pend : local;
  P.ctx = ctx; P.lane = L;
  P.o_pose = o_pose; P.o_H = o_H; P.o_status = o_status; P.o_its = o_its; P.o_stats = o_stats; P.o_last_pose = o_last_pose; P.o_clock = o_clock; P.o_cand = o_cand;
  P.n = n; P.stats_stride = stats_stride; P.n_clock = n_clock; P.clock_stride = clock_stride;
  P.zero_copy = zero_copy; P.want_stats = out_stats != nullptr; P.want_last_pose = out_last_pose != nullptr; P.stamps = stamps; P.timed = ctx->kernel_timing != 0; P.async = async;
  if (async) {
    HIPCHK(ctx, hipEventRecord(L->ev_done, ks));      // (zero-copy batches too: what their wait falls back to when the statuses do not arrive within the spin budget)
    L->busy = true; ++ctx->inflight;
    ctx->cur ^= 1;      // whatever is called next works on the other lane (L stays this batch's)
    return LSM2D_SUCCESS;
  }
  return align_batch_finish(P, out_pose, out_H, out_status, out_its, out_stats, out_last_pose);
}

// Select mode's second half.  Behind the aligner's launch on the same stream: k_align_rows packs every candidate's results and the LAST statistics row it
// started into an AlignRow and counts the Success and the never-written statuses of the whole batch; select_queue / select_queue_grouped (lsm2d_capi_select.inc)
// rank the rows, end the timing bracket (the aligner's launch PLUS the selection), copy the blocks [n_accepted, n_selected, n_success, n_unwritten | index[k] |
// rows[k]] down -- one, or one per group with the group's n_success and the batch's n_unwritten -- and wait: the one copy and the one wait of the call.  Group
// g's rows land in slots g * k + j.  The never-reported check of align_batch_finish is the first block's fourth header word.
int AlignBatch::select_finish() {
  const SelectLayout E1((size_t) n, (size_t) select_k, AlignRow::kWords);      // (the ungrouped call's; `groups` is the grouped one's)
  char* const d = (char*) L->d_scratch;      // (== ds: select mode never takes the zero-copy form)
  char* const de = d + o_sel;
  // the counters: ungrouped [accepted | Success | never written], three words; grouped [Success | never written | accepted[G]], of which select_queue_grouped
  // zeroes the accepted words where its launches add to them.  k_align_rows counts into the two words [Success | never written] either way.
  int32_t* const counts = (int32_t*) (de + (groups ? groups->e_acc : E1.e_acc + sizeof(int32_t)));
  if (groups) HIPCHK(ctx, hipMemsetAsync(counts, 0, sizeof(int32_t) * 2, ks));
  else HIPCHK(ctx, hipMemsetAsync(counts - 1, 0, sizeof(int32_t) * 3, ks));
  AlignRowsArgs R;
  R.pose = (const float*) (d + o_pose); R.H = (const float*) (d + o_H); R.status = (const int32_t*) (d + o_status); R.its = (const int32_t*) (d + o_its);
  R.stats = (const StatsDev*) (d + o_stats); R.n = n; R.stats_stride = stats_stride; R.not_written = kStatusNotWritten;
  R.rows = (float*) (d + o_rows); R.counts = counts;
  hipLaunchKernelGGL(k_align_rows<AlignRow>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ks, R);
  HIPCHK(ctx, hipGetLastError());
  const SelectArgs S = select_args(R.rows, n, select_k, select);
  const int32_t* const h = (const int32_t*) (hs + o_sel);
  {
    const int rc = groups ? select_queue_grouped<AlignRow>(ctx, "align_select_grouped", S, *groups, de, (const int32_t*) (d + o_gtab), hs + o_sel)
                          : select_queue<AlignRow>(ctx, "align_select", S, E1, de, hs + o_sel);
    if (rc) return rc;
  }
  if (h[3] != 0) { for (Lane& any : ctx->lanes) any.order_valid = false; return fail(ctx, LSM2D_DEVICE_ERROR, "align_batch: an alignment's workgroup never reported (placement or launch fault)"); }
  if (!groups && !select_header_ok(h, n, select_k, true)) return fail(ctx, LSM2D_DEVICE_ERROR, "align_select: the selection's counters are inconsistent");
  const size_t G = groups ? groups->G : 1, K = (size_t) select_k, words = select_block_words(K, AlignRow::kWords);
  for (size_t g = 0; g < G; ++g) align_block_out(h + words * g, K, g * K, nullptr, sel_index, out_pose, out_H, out_its, sel_last_stats);
  groups_report(h, words, G, sel_n_selected, sel_n_accepted, sel_n_success);
  return LSM2D_SUCCESS;
}

static int align_batch_run(AlignBatch& B) {
  int rc = B.validate_and_lay_out_scratch();
  if (rc == kEmptyBatch) return LSM2D_SUCCESS;
  if (!rc) rc = B.choose_path();
  if (!rc) rc = B.prepare_slices();
  if (!rc) rc = B.lay_out_lds();
  if (!rc) rc = B.stage_inputs();
  if (!rc) rc = B.make_placement();
  if (rc) return rc;
  if (B.out_work) return B.estimate_only();
  rc = B.launch();
  return rc ? rc : B.hand_over();
}

static int align_batch_impl(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, float* out_pose,
                            float* out_H, int32_t* out_status, int32_t* out_its, lsm2d_iteration_stats* out_stats, float* out_last_pose,
                            int32_t* out_work = nullptr, lsm2d_pending* pend = nullptr) {
  if (!ctx || !ap || !b || ((!out_pose || !out_status) && !out_work)) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: null argument");
  if (lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: two batches are in flight on this context: wait for the older one first (lsm2d_align_batch_wait)");
  AlignBatch B;
  B.ctx = ctx; B.L = &lane(ctx); B.ap = ap; B.b = b; B.out_pose = out_pose; B.out_H = out_H; B.out_status = out_status; B.out_its = out_its; B.out_stats = out_stats;
  B.out_last_pose = out_last_pose; B.out_work = out_work; B.pend = pend;
  return align_batch_run(B);
}

// the second half: wait for the batch, check that every alignment reported, hand the results over
static int align_batch_finish(lsm2d_pending& P, float* out_pose, float* out_H, int32_t* out_status, int32_t* out_its, lsm2d_iteration_stats* out_stats, float* out_last_pose) {
  lsm2d_context* ctx = P.ctx; Lane& L = *P.lane;
  char* hs = (char*) L.h_stage; const int n = P.n;
  const size_t o_pose = P.o_pose, o_H = P.o_H, o_status = P.o_status, o_its = P.o_its, o_stats = P.o_stats, o_last_pose = P.o_last_pose, o_clock = P.o_clock;
  const int stats_stride = P.stats_stride, n_clock = P.n_clock, clock_stride = P.clock_stride;
  const bool zero_copy = P.zero_copy, stamps = P.stamps;
  if (P.async) {
    // (an event of the batch's own, not a wait for the stream: the NEXT batch may be queued behind it already.  The stream's epoch does not move: work queued
    // after this batch has not necessarily run)
    hipError_t we = hipSuccess;
    if (zero_copy) { const unsigned long long epoch = ctx->sync_epoch; we = wait_for_statuses(ctx, (const int32_t*) (hs + o_status), n, L.ev_done); ctx->sync_epoch = epoch; }
    else we = hipEventSynchronize(L.ev_done);
    L.busy = false;
    if (ctx->inflight > 0) --ctx->inflight;
    HIPCHK(ctx, we);
  }
  else if (zero_copy) HIPCHK(ctx, wait_for_statuses(ctx, (const int32_t*) (hs + o_status), n));
  else HIPCHK(ctx, stream_sync(ctx));
  ctx->timed_lane = (int) (&L - ctx->lanes); ctx->have_timing = P.timed;
  {
    static_assert(kStatusNotWritten == -1, "the memsets above write 0xFF bytes");
    const int32_t* st = (const int32_t*) (hs + o_status);
    for (int i = 0; i < n; ++i) if (st[i] == kStatusNotWritten) { for (Lane& any : ctx->lanes) any.order_valid = false; return fail(ctx, LSM2D_DEVICE_ERROR, "align_batch: an alignment's workgroup never reported (placement or launch fault)"); }
  }
  memcpy(out_pose, hs + o_pose, sizeof(float) * 3 * (size_t) n);
  if (out_H) memcpy(out_H, hs + o_H, sizeof(float) * 9 * (size_t) n);
  memcpy(out_status, hs + o_status, sizeof(int32_t) * (size_t) n);
  if (out_its) memcpy(out_its, hs + o_its, sizeof(int32_t) * (size_t) n);
  if (out_stats) memcpy(out_stats, hs + o_stats, sizeof(StatsDev) * (size_t) n * (size_t) stats_stride);
  if (out_last_pose) memcpy(out_last_pose, hs + o_last_pose, sizeof(float) * 3 * (size_t) n);
  if (P.want_stats) {      // the candidate lists' books of this batch (align_body's s_cand_stat: iterations served | lists built << 16 | of which too long << 24)
    const uint32_t* cw = (const uint32_t*) (hs + P.o_cand);
    long long its = 0, builds = 0, over = 0, fell = 0;
    for (int i = 0; i < n; ++i) { its += cw[i] & 0xFFFFu; builds += (cw[i] >> 16) & 0xFFu; over += cw[i] >> 24; fell += cw[n + i]; }
    ctx->last_cand_fallbacks = (int) std::min(fell, (long long) 0x7fffffff);
    ctx->last_cand_iterations = (int) std::min(its, (long long) 0x7fffffff); ctx->last_cand_builds = (int) std::min(builds, (long long) 0x7fffffff); ctx->last_cand_overflows = (int) std::min(over, (long long) 0x7fffffff);
  }
  if (stamps) {     // median over the stamped workgroups: shader cycles per 10 ns tick of the constant 100 MHz counter
    const unsigned long long* ck = (const unsigned long long*) (hs + o_clock);
    std::vector<double> khz; std::vector<unsigned long long> life;
    for (int i = 0; i < n_clock; ++i) if (ck[4 * i + 1] > 0) { khz.push_back((double) ck[4 * i] / (double) ck[4 * i + 1] * 1e5); life.push_back(ck[4 * i + 1] * 10ull); }
    if (const char* dump = getenv("LSM2D_DUMP_STAMPS")) {      // diagnostics: one line per stamped workgroup (tools/occupancy_probe.py reads them)
      if (FILE* f = fopen(dump, "a")) {
        unsigned long long t0 = ~0ull; for (int i = 0; i < n_clock; ++i) if (ck[4 * i + 1] > 0 && ck[4 * i + 2] < t0) t0 = ck[4 * i + 2];
        fprintf(f, "# launch n=%d stride=%d t0=%llu\n", n, clock_stride, t0);      // (t0: what the third column is relative to)
        for (int i = 0; i < n_clock; ++i)
          fprintf(f, "%d %llu %llu %llu 0x%llx\n", i * clock_stride, ck[4 * i], ck[4 * i + 1], ck[4 * i + 2] - t0, ck[4 * i + 3]);
        fclose(f);
      }
    }
    if (!khz.empty()) {
      std::nth_element(khz.begin(), khz.begin() + khz.size() / 2, khz.end()); ctx->last_clock_khz = (long long) khz[khz.size() / 2];
      std::nth_element(life.begin(), life.begin() + life.size() / 2, life.end()); ctx->last_wg_lifetime_ns = (long long) life[life.size() / 2];
    }
  }
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_align_batch(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, float* out_pose,
                                 float* out_H, int32_t* out_status, int32_t* out_its, lsm2d_iteration_stats* out_stats) {
  return align_batch_impl(ctx, ap, b, out_pose, out_H, out_status, out_its, out_stats, nullptr);
}

// ---- aligned, accepted and ranked: the candidate loops' verdict with k rows coming down (include/lsm2d.h).  The alignment is lsm2d_align_batch's with statistics
// (the same stages, path rule, kernels and launch forms); synchronous, on the context's current lane like every other call.
// (grouped: the fleet's candidate loop, ranked per group of the batch -- the groups' table rides up in the input block; lsm2d_capi_select.inc)
static int align_select_impl(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, const lsm2d_select_params* select, int32_t k, bool grouped,
                             int32_t n_groups, const int32_t* group_offsets, int32_t* out_index, float* out_pose, float* out_H, int32_t* out_its,
                             lsm2d_iteration_stats* out_last_stats, int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  const char* const who = grouped ? "align_select_grouped" : "align_select";
  if (!ctx || !ap || !b || !select || !out_index || !out_pose || !out_n_selected || !out_n_accepted) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: null argument", who);
  if (k < 1 || k > kSelectMaxK) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: k outside [1, LSM2D_SELECT_MAX_K]", who);
  if (lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch: two batches are in flight on this context: wait for the older one first (lsm2d_align_batch_wait)");
  std::optional<SelectGroupedLayout> E;
  if (grouped) {
    const int rc = check_groups(ctx, who, n_groups, group_offsets, b->n_alignments, k); if (rc) return rc;
    E.emplace(group_offsets, (size_t) n_groups, (size_t) k, (size_t) AlignRow::kWords);
  }
  static int32_t wanted_status; static lsm2d_iteration_stats wanted_stats;      // (the stages ask "is this output wanted?" of the pointers: statuses and statistics are, on the device)
  AlignBatch B;
  B.ctx = ctx; B.L = &lane(ctx); B.ap = ap; B.b = b; B.out_pose = out_pose; B.out_H = out_H; B.out_status = &wanted_status; B.out_its = out_its;
  B.out_stats = &wanted_stats; B.out_last_pose = nullptr; B.out_work = nullptr; B.pend = nullptr;
  B.select = select; B.select_k = k; B.sel_index = out_index; B.sel_last_stats = out_last_stats; B.sel_n_selected = out_n_selected; B.sel_n_accepted = out_n_accepted;
  B.sel_n_success = out_n_success; B.groups = E ? &*E : nullptr;
  if (b->n_alignments == 0) {      // an empty batch: its descriptor is checked as ever, the counts (every group's) are zeros
    const int rc = B.validate_and_lay_out_scratch();
    if (rc != kEmptyBatch) return rc;
    groups_report(nullptr, 0, E ? E->G : 1, out_n_selected, out_n_accepted, out_n_success);
    return LSM2D_SUCCESS;
  }
  return align_batch_run(B);
}

extern "C" int lsm2d_align_select(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, const lsm2d_select_params* select, int32_t k,
                                  int32_t* out_index, float* out_pose, float* out_H, int32_t* out_its, lsm2d_iteration_stats* out_last_stats,
                                  int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  return align_select_impl(ctx, ap, b, select, k, false, 1, nullptr, out_index, out_pose, out_H, out_its, out_last_stats, out_n_selected, out_n_accepted, out_n_success);
}

extern "C" int lsm2d_align_select_grouped(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, const lsm2d_select_params* select, int32_t k,
                                          int32_t n_groups, const int32_t* group_offsets, int32_t* out_index, float* out_pose, float* out_H, int32_t* out_its,
                                          lsm2d_iteration_stats* out_last_stats, int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  return align_select_impl(ctx, ap, b, select, k, true, n_groups, group_offsets, out_index, out_pose, out_H, out_its, out_last_stats, out_n_selected, out_n_accepted,
                           out_n_success);
}

// ---- a batch in flight: MultiAligner2D::compute over a batch, split where the host would otherwise sleep.  begin() queues everything -- inputs, placement,
// kernels, the copies of the results -- and returns; wait() blocks until THAT batch's last operation has run (an event of its own: a younger batch may be
// queued behind it) and hands the results over.  While one batch is in flight, the next one's pre-kernels go to a second stream (pre_stream) and fill the
// slots its tail leaves free.  Two lanes of staging / scratch: at most two batches in flight, waited for in the order they were begun.
extern "C" int lsm2d_align_batch_begin(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, int32_t want_stats, lsm2d_pending** out_pending) {
  if (!ctx || !out_pending) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch_begin: null argument");
  *out_pending = nullptr;
  lsm2d_pending* P = new (std::nothrow) lsm2d_pending;
  if (!P) return LSM2D_OUT_OF_MEMORY;
  static float dummy_pose; static int32_t dummy_status; static lsm2d_iteration_stats dummy_stats;      // (only their being non-null is looked at)
  const int rc = align_batch_impl(ctx, ap, b, &dummy_pose, nullptr, &dummy_status, nullptr, want_stats ? &dummy_stats : nullptr, nullptr, nullptr, P);
  if (rc != LSM2D_SUCCESS || !P->ctx) { const bool empty = rc == LSM2D_SUCCESS; delete P; if (!empty) return rc; P = new (std::nothrow) lsm2d_pending; if (!P) return LSM2D_OUT_OF_MEMORY; }      // (n == 0: an empty batch, nothing in flight)
  *out_pending = P;
  return LSM2D_SUCCESS;
}
extern "C" int lsm2d_align_batch_wait(lsm2d_pending* pending, float* out_pose, float* out_H, int32_t* out_status, int32_t* out_its, lsm2d_iteration_stats* out_stats) {
  if (!pending) return LSM2D_BAD_ARGUMENT;
  if (!pending->ctx) { delete pending; return LSM2D_SUCCESS; }      // an empty batch
  lsm2d_context* ctx = pending->ctx;
  int rc = LSM2D_SUCCESS;
  if (!out_pose || !out_status || (out_stats && !pending->want_stats)) {
    // the batch must still be retired: its lane stays busy otherwise
    float* p = (float*) malloc(sizeof(float) * 3 * (size_t) (pending->n > 0 ? pending->n : 1)); int32_t* st = (int32_t*) malloc(sizeof(int32_t) * (size_t) (pending->n > 0 ? pending->n : 1));
    if (p && st) (void) align_batch_finish(*pending, p, nullptr, st, nullptr, nullptr, nullptr);
    free(p); free(st);
    rc = fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch_wait: out_pose / out_status missing, or statistics asked for that the batch was not begun with");
  }
  else rc = align_batch_finish(*pending, out_pose, out_H, out_status, out_its, out_stats, nullptr);
  delete pending;
  return rc;
}

extern "C" int lsm2d_estimate_work(lsm2d_context* ctx, const lsm2d_batch* b, int32_t* out_work) {
  if (!out_work) return fail(ctx, LSM2D_BAD_ARGUMENT, "estimate_work: null argument");
  lsm2d_aligner_params ap; memset(&ap, 0, sizeof ap); ap.max_iterations = 1;
  return align_batch_impl(ctx, &ap, b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out_work);
}

// MultiAligner2D::compute + what it leaves in the slices' correspondence vectors (apps/visual_test_aligner_2d.cpp:129-143).  The aligner kernels keep
// no pair lists (their pairs live for one bin walk / one query); the vectors are re-derived from the pose the last started iteration began at by
// the finder-level kernels -- the same arithmetic, hence the same pairs (tests: their digest equals the in-kernel one).  A batch takes ONE batched finder
// pass per slice over the alignments that started an iteration (k_find_*_batch: a workgroup per alignment, one wait per launch), so the pairs of a thousand
// alignments cost a launch and a copy, not a thousand waits.
// Routing: a call with ONE alignment keeps the single calls, one per slice (lsm2d_find_correspondences: pairs written straight to pinned host memory, no
// argument upload, no result copy) -- for one slice by definition, for the tracker's two slices because it is the faster of the two: the batched pass is a
// launch and a wait per slice as well and adds an upload and a copy to each.  Measured on the MI355X (tests/bench/pairs_batch_bench.py part c: one alignment, two
// 721-column slices, a prior, with pairs; medians of 300 calls, three runs each, alternated in one job; profiles/r10/pairs_ab_r10.jsonl): single calls 83.2 / 84.1 /
// 91.5 us per call (the parent commit: 84.2 / 84.2 / 84.3), the batched pass (a build with -DLSM2D_PAIRS_BATCH_MIN=1) 106.6 / 108.2 / 108.5.  From two alignments on
// the batched pass: at n = 1000 it costs 0.53 - 0.65 ms where 1000 single calls cost 31.3 - 31.6 ms.
static constexpr int kPairsBatchMinAlignments =
#ifdef LSM2D_PAIRS_BATCH_MIN
    LSM2D_PAIRS_BATCH_MIN;      // (A/B builds of tests/bench/pairs_batch_bench.py only)
#else
    2;
#endif
extern "C" int lsm2d_align_batch_pairs(lsm2d_context* ctx, const lsm2d_aligner_params* ap, const lsm2d_batch* b, float* out_pose, float* out_H,
                                       int32_t* out_status, int32_t* out_its, lsm2d_iteration_stats* out_stats,
                                       lsm2d_correspondence* out_pairs, int32_t pair_capacity, int32_t* out_n_pairs) {
  if (!out_pairs) return align_batch_impl(ctx, ap, b, out_pose, out_H, out_status, out_its, out_stats, nullptr);
  if (!ctx || !ap || !b || !out_n_pairs || pair_capacity < 0) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch_pairs: bad argument");
  const int n = b->n_alignments, ns = b->n_slices;
  if (n < 0 || ns < 1 || ns > kMaxSlices || !b->slices || !b->fixed || !b->moving) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch_pairs: bad batch descriptor");
  for (int s = 0; s < ns; ++s) {      // a slice's largest possible vector must fit
    const lsm2d_cloudset* m = b->moving[s];
    if (!m || !b->fixed[s]) return fail(ctx, LSM2D_BAD_ARGUMENT, "align_batch_pairs: cloud set missing");
    long long need = 0;
    { const int rc0 = find_batch_need(&b->slices[s], m, &need); if (rc0) return rc0; }
    if (need > pair_capacity) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "align_batch_pairs: pair_capacity below a slice's largest possible correspondence vector");
  }
  std::vector<float> last_pose((size_t) 3 * (size_t) (n > 0 ? n : 1));
  std::vector<int32_t> its_local;
  int32_t* its = out_its;
  if (!its) { its_local.assign((size_t) (n > 0 ? n : 1), 0); its = its_local.data(); }
  int rc = align_batch_impl(ctx, ap, b, out_pose, out_H, out_status, its, out_stats, last_pose.data());
  if (rc) return rc;
  const bool batched = n >= kPairsBatchMinAlignments;
  std::vector<int32_t> slots, fcs, mcs; std::vector<float> poses;
  if (batched) { slots.reserve((size_t) n); fcs.reserve((size_t) n); mcs.reserve((size_t) n); poses.reserve((size_t) 3 * (size_t) n); }
  for (int s = 0; s < ns; ++s) {
    const lsm2d_slice_params& sp = b->slices[s];
    const lsm2d_cloudset* f = b->fixed[s]; const lsm2d_cloudset* m = b->moving[s];
    const bool has_sensor = !(sp.sensor_in_robot[0] == 0.0f && sp.sensor_in_robot[1] == 0.0f && sp.sensor_in_robot[2] == 0.0f);
    const float inl_tau = (ap->keep_only_inlier_correspondences && sp.robustifier == LSM2D_ROBUST_CAUCHY) ? sp.chi_threshold : 0.0f;
    float Sinv[3] = {0.0f, 0.0f, 0.0f};
    if (has_sensor) inverse_host(sp.sensor_in_robot, Sinv);
    slots.clear(); fcs.clear(); mcs.clear(); poses.clear();
    for (int i = 0; i < n; ++i) {
      int32_t* cnt = out_n_pairs + (size_t) i * ns + s;
      lsm2d_correspondence* dst = out_pairs + ((size_t) i * ns + s) * (size_t) pair_capacity;
      *cnt = 0;
      if (its[i] < 1) continue;      // no iteration started: the vectors stay empty
      const int fc = b->fixed_index ? b->fixed_index[(size_t) s * n + i] : (f->n_clouds == 1 ? 0 : i);
      const int mc = b->moving_index ? b->moving_index[(size_t) s * n + i] : (m->n_clouds == 1 ? 0 : i);
      float Xe[3] = {last_pose[3 * (size_t) i], last_pose[3 * (size_t) i + 1], last_pose[3 * (size_t) i + 2]};
      if (has_sensor) { float X[3] = {Xe[0], Xe[1], Xe[2]}; compose_host(Sinv, X, Xe); }      // X_eff = S^-1 X, the kernels' operations
      if (!batched) {
        rc = find_correspondences_impl(ctx, &sp, f, fc, m, mc, Xe, dst, pair_capacity, cnt, inl_tau);
        if (rc) return rc;
        continue;
      }
      slots.push_back(i); fcs.push_back(fc); mcs.push_back(mc); poses.push_back(Xe[0]); poses.push_back(Xe[1]); poses.push_back(Xe[2]);
    }
    if (batched && !slots.empty()) {      // the slice's pass: destination strided into [n][n_slices][pair_capacity]
      rc = find_batch_impl(ctx, &sp, f, fcs.data(), m, mcs.data(), (int32_t) slots.size(), poses.data(), inl_tau, out_pairs + (size_t) s * (size_t) pair_capacity,
                           pair_capacity, out_n_pairs + s, slots.data(), (size_t) ns * (size_t) pair_capacity, (size_t) ns);
      if (rc) return rc;
    }
  }
  return LSM2D_SUCCESS;
}
