// lsm2d_capi_select.inc -- scored rows ranked on the device: the acceptance test and the best k, for the whole batch or per GROUP of it (lsm2d_k_select.h).
// Part of lsm2d_capi.hip, included behind lsm2d_capi_finder.inc (the scoring's queues and row formats) and in front of lsm2d_capi_aligner.inc (lsm2d_align_select
// and its grouped sibling rank AlignRow rows with the layouts, queues and unpacking below).
//
// Whole batch.  Behind the last launch group, on the same stream: keys and the accepted count (k_select_keys), passes of k_select_tile over two ping-pong
// arrays of (key, index) entries until one tile is left -- a pass turns m entries into ceil(m / tile) x k, less than half of them while m > tile -- and
// k_select_gather, which fills the one region that comes down: a BLOCK [n_accepted, n_selected, c2, c3 | index[k] | rows[k][row words]], 16 + 68 k bytes of
// ScoreRow rows whatever n_items is.  A batch of at most one tile does all three in ONE launch (k_select_tile_one: four launches and a memset less, which is
// what counts at 1000 items).
// Per group.  Group g is items [off[g], off[g + 1]); every group gets the block the ungrouped call returns for its sub-batch, indices shifted by off[g]: the
// region that comes down is n_groups blocks, the ungrouped calls' ONE.  The host knows every group's size, so it lays out every launch: a table [offsets | one
// closing descriptor per group | keys descriptors | the passes' descriptors] rides up with the call's arguments, in the same copy.  Every group at most one
// tile: ONE launch, a workgroup per group, and the table is the offsets alone.  Otherwise: keys over (group, chunk) descriptors, passes of k_select_tile_seg
// over the groups that are still larger than a tile -- group g's m entries become ceil(m / tile) x k, in its own stretch of the other array -- and
// k_select_gather_group, which sorts what is left of every group and gathers.

static constexpr size_t select_block_words(size_t K, size_t row_words) { return kSelectHeaderWords + K + K * row_words; }

// where the selection's own part of the scratch lies: [keys A | index A] of n entries, [keys B | index B] of what the first pass leaves, the accepted count,
// the region that goes down (one block: down_bytes)
struct SelectLayout {
  size_t n, K, e_idx_a, e_key_b, e_idx_b, e_acc, e_down, down_bytes, d_bytes;
  SelectLayout(size_t n_, size_t K_, size_t row_words) : n(n_), K(K_) {
    const size_t n_first = ((n + kSelectTile - 1) / kSelectTile) * K;      // what the first pass leaves
    e_idx_a = up256(sizeof(u64) * n); e_key_b = up256(e_idx_a + sizeof(int32_t) * n); e_idx_b = up256(e_key_b + sizeof(u64) * n_first);
    e_acc = up256(e_idx_b + sizeof(int32_t) * n_first); e_down = e_acc + 256;
    down_bytes = sizeof(int32_t) * select_block_words(K, row_words);
    d_bytes = e_down + down_bytes;
  }
};

// The table that rides up (words), where the selection's own part of the scratch lies -- [keys A | index A] of n entries, [keys B | index B] of what the first
// pass leaves, [Success, never written | accepted[G]], the region that goes down (G blocks) -- and every launch of the segmented form.
struct SelectGroupedLayout {
  struct Pass { size_t t_off, count; };
  size_t n, G, K, group_words, n_b = 0;
  bool one_tile = true;
  std::vector<int32_t> table; size_t t_fin = 0, t_keys = 0, n_keys = 0; std::vector<Pass> passes;      // (t_*: word offsets of SelectSeg arrays in the table)
  size_t e_idx_a = 0, e_key_b = 0, e_idx_b = 0, e_acc = 0, e_down = 0, down_bytes = 0, d_bytes = 0;
  size_t table_bytes() const { return sizeof(int32_t) * table.size(); }
  SelectGroupedLayout(const int32_t* off, size_t G_, size_t K_, size_t row_words) : n((size_t) off[G_]), G(G_), K(K_), group_words(select_block_words(K_, row_words)) {
    static_assert(sizeof(SelectSeg) == 4 * sizeof(int32_t), "a descriptor is four words of the table");
    for (size_t g = 0; g < G; ++g) if (off[g + 1] - off[g] > kSelectTile) one_tile = false;
    table.assign(off, off + G + 1);
    if (!one_tile) {
      const auto push = [this](int32_t a, int32_t b, int32_t c, int32_t d) { table.push_back(a); table.push_back(b); table.push_back(c); table.push_back(d); };
      while (table.size() % 4) table.push_back(0);
      t_fin = table.size(); table.resize(t_fin + 4 * G, 0);      // filled once the passes are known
      t_keys = table.size();
      for (size_t g = 0; g < G; ++g)
        for (int32_t c = off[g]; c < off[g + 1]; c += 256) { push(c, std::min<int32_t>(256, off[g + 1] - c), 0, (int32_t) g); ++n_keys; }
      std::vector<int32_t> base(off, off + G), cnt(G), b_base(G, 0);
      for (size_t g = 0; g < G; ++g) {
        cnt[g] = off[g + 1] - off[g];
        if (cnt[g] > kSelectTile) { b_base[g] = (int32_t) n_b; n_b += (size_t) ((cnt[g] + kSelectTile - 1) / kSelectTile) * K; }      // (< cnt[g]: n_b < n)
      }
      for (int src = 0;; src ^= 1) {      // a pass reads array `src` and writes the other: a group's stretch of A is its items', of B what its first pass left
        Pass P = {table.size(), 0};
        for (size_t g = 0; g < G; ++g) {
          if (cnt[g] <= kSelectTile) continue;
          const int32_t tiles = (cnt[g] + kSelectTile - 1) / kSelectTile, out = src ? off[g] : b_base[g];
          for (int32_t j = 0; j < tiles; ++j) push(base[g] + j * kSelectTile, std::min<int32_t>(kSelectTile, cnt[g] - j * kSelectTile), out + j * (int32_t) K, 0);
          P.count += (size_t) tiles; base[g] = out; cnt[g] = tiles * (int32_t) K;      // (tiles >= 2: tiles x k <= tiles x tile / 2 < the entries that came in)
          table[t_fin + 4 * g + 3] = src ^ 1;
        }
        if (!P.count) break;
        passes.push_back(P);
      }
      for (size_t g = 0; g < G; ++g) { table[t_fin + 4 * g] = base[g]; table[t_fin + 4 * g + 1] = cnt[g]; }
      e_idx_a = up256(sizeof(u64) * n); e_key_b = up256(e_idx_a + sizeof(int32_t) * n); e_idx_b = up256(e_key_b + sizeof(u64) * n_b);
      e_acc = up256(e_idx_b + sizeof(int32_t) * n_b);
    }
    e_down = up256(e_acc + sizeof(int32_t) * (2 + G));
    down_bytes = sizeof(int32_t) * group_words * G;
    d_bytes = e_down + down_bytes;
  }
};

// what every selection is asked: the rows where the scoring left them, their number, k and the thresholds (keys, index and n_accepted are the launches' to say)
static SelectArgs select_args(const void* rows, int32_t n_items, int32_t k, const lsm2d_select_params* p) {
  SelectArgs A;
  memset(&A, 0, sizeof A);
  A.rows = (const float*) rows; A.n_items = n_items; A.k = k;
  A.min_inliers = p->min_inliers; A.max_chi_per_inlier = p->max_chi_per_inlier; A.min_inlier_ratio = p->min_inlier_ratio;
  return A;
}

// is a block's header, as it came down, one the kernels can have written for `size` items?  0 <= n_accepted <= size, n_selected = min(n_accepted, k), and
// for a format that carries counts n_accepted <= n_success <= size
static bool select_header_ok(const int32_t* h, int32_t size, int32_t k, bool counts) {
  const int32_t n_acc = h[0], n_sel = h[1];
  return n_acc >= 0 && n_acc <= size && n_sel == (n_acc < k ? n_acc : k) && (!counts || (h[2] >= n_acc && h[2] <= size));
}

// A block that came down, unpacked: row j < n_selected of block h goes to slot base + j of the caller's outputs (an ungrouped call: its one block, base 0;
// group g: base g * k).  One per row format.
static void score_block_out(const int32_t* h, size_t K, size_t base, int32_t* out_index, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats) {      // ScoreRow
  const int32_t* h_index = h + kSelectHeaderWords; const float* h_rows = (const float*) (h_index + K);
  float H[9], b[3];
  for (int32_t j = 0; j < h[1]; ++j) {
    const size_t slot = base + (size_t) j;
    out_index[slot] = h_index[j];
    lin_row_out(h_rows + kLinOutWords * (size_t) j, out_H ? out_H + 9 * slot : H, out_b ? out_b + 3 * slot : b, out_stats ? out_stats + slot : nullptr);
  }
}
static void comb_block_out(const int32_t* h, size_t K, size_t base, int32_t* out_index, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats,
                           int32_t* out_active) {      // CombRow; out_index NULL: the caller has the indices from elsewhere
  const int32_t* h_index = h + kSelectHeaderWords; const float* h_rows = (const float*) (h_index + K);
  for (int32_t j = 0; j < h[1]; ++j) {
    const size_t slot = base + (size_t) j;
    if (out_index) out_index[slot] = h_index[j];
    comb_row_out(h_rows + kCombWords * (size_t) j, out_H ? out_H + 9 * slot : nullptr, out_b ? out_b + 3 * slot : nullptr, out_stats ? out_stats + slot : nullptr,
                 out_active ? out_active + slot : nullptr);
  }
}
// AlignRow; `through`: an index table the block's indices are taken through (lsm2d_relocalize_select: the first stage's selection), or NULL
static void align_block_out(const int32_t* h, size_t K, size_t base, const int32_t* through, int32_t* out_index, float* out_pose, float* out_H, int32_t* out_its,
                            lsm2d_iteration_stats* out_last_stats) {
  const int32_t* h_index = h + kSelectHeaderWords; const int32_t* h_rows = h_index + K;
  for (int32_t j = 0; j < h[1]; ++j) {
    const int32_t* row = h_rows + AlignRow::kWords * (size_t) j;
    const size_t slot = base + (size_t) j;
    out_index[slot] = through ? through[h_index[j]] : h_index[j];
    memcpy(out_pose + 3 * slot, row + AlignRow::kPose, sizeof(float) * 3);
    if (out_H) memcpy(out_H + 9 * slot, row + AlignRow::kH, sizeof(float) * 9);
    if (out_its) out_its[slot] = row[AlignRow::kIts];
    if (out_last_stats) memcpy(out_last_stats + slot, row + AlignRow::kStats, sizeof(lsm2d_iteration_stats));
  }
}

// The selection's launches over rows of format Row, behind the scoring on the same stream; `de`: the selection's part of the scratch; `down`: where the
// block that goes down is written (select_queue: de + E.e_down; lsm2d_relocalize_select: next to the second stage's, so that one copy takes both).  Waits
// for nothing, copies nothing.  A (select_args) is the caller's.
template <class Row>
static int select_launches(lsm2d_context* ctx, SelectArgs A, const SelectLayout& E, char* de, int32_t* down) {
  const size_t n = E.n, K = E.K;
  u64* key[2] = {(u64*) de, (u64*) (de + E.e_key_b)}; int32_t* idx[2] = {(int32_t*) (de + E.e_idx_a), (int32_t*) (de + E.e_idx_b)};
  A.keys = key[0]; A.index = idx[0]; A.n_accepted = (int32_t*) (de + E.e_acc);
  if (n <= (size_t) kSelectTile) {      // one tile: keys, sort and gather in one launch of one workgroup
    hipLaunchKernelGGL(k_select_tile_one<Row>, dim3(1), dim3(kSelectBlock), 0, ctx->stream, A, (int32_t) select_sort_size((int) n), down);
  } else {
    HIPCHK(ctx, hipMemsetAsync(A.n_accepted, 0, sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(k_select_keys<Row>, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, A);
    size_t m = n; int src = 0;
    for (;;) {      // array A has room for n entries, B for n_first: pass p writes fewer than pass p - 2 read
      const size_t tiles = (m + kSelectTile - 1) / kSelectTile;
      hipLaunchKernelGGL(k_select_tile, dim3((unsigned) tiles), dim3(kSelectBlock), 0, ctx->stream, (const u64*) key[src], (const int32_t*) idx[src], (int32_t) m,
                         A.k, key[src ^ 1], idx[src ^ 1]);
      src ^= 1; m = tiles * K;
      if (tiles == 1) break;
    }
    hipLaunchKernelGGL(k_select_gather<Row>, dim3(1), dim3(256), 0, ctx->stream, A, (const u64*) key[src], (const int32_t*) idx[src], down);
  }
  return LSM2D_SUCCESS;
}

// what ends every select call: the end of the timing bracket (the last launch group and the selection), the one copy down, the one wait
static int select_come_down(lsm2d_context* ctx, const char* d_down, size_t down_bytes, char* h_down) {
  HIPCHK(ctx, TimedLaunch(ctx, lane(ctx), ctx->stream).end());
  HIPCHK(ctx, hipMemcpyAsync(h_down, d_down, down_bytes, hipMemcpyDeviceToHost, ctx->stream));      // the one copy down
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  return LSM2D_SUCCESS;
}

// ... and the rest of a select call: the launches above, select_come_down to `h_down` and the check of the counters.
template <class Row>
static int select_queue(lsm2d_context* ctx, const char* who, SelectArgs A, const SelectLayout& E, char* de, char* h_down) {
  { const int rc = select_launches<Row>(ctx, A, E, de, (int32_t*) (de + E.e_down)); if (rc) return rc; }
  { const int rc = select_come_down(ctx, de + E.e_down, E.down_bytes, h_down); if (rc) return rc; }
  if (!select_header_ok((const int32_t*) h_down, A.n_items, A.k, false)) return failf(ctx, LSM2D_DEVICE_ERROR, "%s: the selection's counters are inconsistent", who);
  return LSM2D_SUCCESS;
}

// select_queue for groups; every group's counters checked.  `d_table`: where the layout's table lies on the device.  (A format that carries counts: the
// caller has zeroed the two words at de + e_acc and queued the kernel that counts into them.)
template <class Row>
static int select_queue_grouped(lsm2d_context* ctx, const char* who, SelectArgs S, const SelectGroupedLayout& E, char* de, const int32_t* d_table, char* h_down) {
  int32_t* const acc = (int32_t*) (de + E.e_acc);
  u64* const key_b = (u64*) (de + E.e_key_b); int32_t* const idx_b = (int32_t*) (de + E.e_idx_b);
  S.keys = (u64*) de; S.index = (int32_t*) (de + E.e_idx_a); S.n_accepted = acc + 2;
  SelectGroupedArgs A;
  A.S = S; A.offsets = d_table; A.unwritten = SelectCarriesCounts<Row>::value ? acc + 1 : nullptr; A.down = (int32_t*) (de + E.e_down);
  if (E.one_tile) hipLaunchKernelGGL(k_select_group_one<Row>, dim3((unsigned) E.G), dim3(kSelectBlock), 0, ctx->stream, A);
  else {
    HIPCHK(ctx, hipMemsetAsync(S.n_accepted, 0, sizeof(int32_t) * E.G, ctx->stream));
    hipLaunchKernelGGL(k_select_keys_seg<Row>, dim3((unsigned) E.n_keys), dim3(256), 0, ctx->stream, A, (const SelectSeg*) (d_table + E.t_keys));
    int src = 0;
    for (const SelectGroupedLayout::Pass& P : E.passes) {
      hipLaunchKernelGGL(k_select_tile_seg, dim3((unsigned) P.count), dim3(kSelectBlock), 0, ctx->stream, (const u64*) (src ? key_b : S.keys),
                         (const int32_t*) (src ? idx_b : S.index), src ? S.keys : key_b, src ? S.index : idx_b, (const SelectSeg*) (d_table + P.t_off), S.k);
      src ^= 1;
    }
    hipLaunchKernelGGL(k_select_gather_group<Row>, dim3((unsigned) E.G), dim3(kSelectBlock), 0, ctx->stream, A, (const SelectSeg*) (d_table + E.t_fin),
                       (const u64*) key_b, (const int32_t*) idx_b);
  }
  HIPCHK(ctx, hipGetLastError());
  { const int rc = select_come_down(ctx, de + E.e_down, E.down_bytes, h_down); if (rc) return rc; }
  for (size_t g = 0; g < E.G; ++g)
    if (!select_header_ok((const int32_t*) h_down + E.group_words * g, E.table[g + 1] - E.table[g], S.k, SelectCarriesCounts<Row>::value))
      return failf(ctx, LSM2D_DEVICE_ERROR, "%s: the selection's counters are inconsistent (group %d)", who, (int) g);
  return LSM2D_SUCCESS;
}

// offsets: n_groups + 1 values, non-decreasing, from 0 to n; n_groups x k within LSM2D_SELECT_MAX_GROUP_ROWS
static int check_groups(lsm2d_context* ctx, const char* who, int32_t n_groups, const int32_t* off, int32_t n, int32_t k) {
  static_assert(LSM2D_SELECT_MAX_GROUP_ROWS == (1 << 18), "the ABI's cap");
  if (!off) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: null argument", who);
  if (n_groups < 1) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: n_groups must be >= 1", who);
  if ((long long) n_groups * (long long) k > (long long) LSM2D_SELECT_MAX_GROUP_ROWS)
    return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: n_groups x k above LSM2D_SELECT_MAX_GROUP_ROWS", who);
  if (off[0] != 0 || off[n_groups] != n) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: group_offsets must start at 0 and end at the batch's size", who);
  for (int32_t g = 0; g < n_groups; ++g)
    if (off[g + 1] < off[g]) return failf(ctx, LSM2D_BAD_ARGUMENT, "%s: group_offsets decrease at group %d", who, (int) g);
  return LSM2D_SUCCESS;
}

// every group's counts as the caller reads them: from the blocks that came down, or (h NULL: an empty batch) 0 accepted and 0 selected
static void groups_report(const int32_t* h, size_t group_words, size_t n_groups, int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  for (size_t g = 0; g < n_groups; ++g, h += h ? group_words : 0) {
    out_n_selected[g] = h ? h[1] : 0; out_n_accepted[g] = h ? h[0] : 0;
    if (out_n_success) out_n_success[g] = h ? h[2] : 0;
  }
}

// ---- one slice's hypotheses (lsm2d_score_batch's scoring: score_batch_queue) ---------------------------------------------------------------------------------------
extern "C" int lsm2d_score_select(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                  const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses,
                                  const lsm2d_select_params* select, int32_t k, int32_t* out_index, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats,
                                  int32_t* out_n_selected, int32_t* out_n_accepted) {
  static_assert(LSM2D_SELECT_MAX_K == kSelectMaxK, "the ABI's limit is the kernels'");
  if (!select || !out_index || !out_n_selected || !out_n_accepted) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select: null argument");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select: k outside [1, LSM2D_SELECT_MAX_K]");
  { const int rc = batch_head(ctx, "score_select", sp, fixed, moving, n_items, 0); if (rc) return rc; }
  if (n_items == 0) { *out_n_selected = 0; *out_n_accepted = 0; return LSM2D_SUCCESS; }
  if (!poses) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select: null argument");
  const SelectLayout E((size_t) n_items, (size_t) k, kLinOutWords);
  ScoreLayout Y;
  { const int rc = score_batch_queue(ctx, "score_select", sp, fixed, fixed_index, moving, moving_index, n_items, poses, E.d_bytes, E.down_bytes, Y); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  { const int rc = select_queue<ScoreRow>(ctx, "score_select", select_args(ds + Y.o_out, n_items, k, select), E, ds + Y.o_extra, hs + Y.h_out); if (rc) return rc; }
  const int32_t* h = (const int32_t*) (hs + Y.h_out);
  score_block_out(h, E.K, 0, out_index, out_H, out_b, out_stats);
  groups_report(h, 0, 1, out_n_selected, out_n_accepted, nullptr);
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_score_select_grouped(lsm2d_context* ctx, const lsm2d_slice_params* sp, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                          const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* poses,
                                          const lsm2d_select_params* select, int32_t k, int32_t n_groups, const int32_t* group_offsets, int32_t* out_index,
                                          float* out_H, float* out_b, lsm2d_iteration_stats* out_stats, int32_t* out_n_selected, int32_t* out_n_accepted) {
  static const char who[] = "score_select_grouped";
  if (!select || !out_index || !out_n_selected || !out_n_accepted) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select_grouped: null argument");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select_grouped: k outside [1, LSM2D_SELECT_MAX_K]");
  { const int rc = batch_head(ctx, who, sp, fixed, moving, n_items, 0); if (rc) return rc; }
  { const int rc = check_groups(ctx, who, n_groups, group_offsets, n_items, k); if (rc) return rc; }
  if (n_items == 0) { groups_report(nullptr, 0, (size_t) n_groups, out_n_selected, out_n_accepted, nullptr); return LSM2D_SUCCESS; }
  if (!poses) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_select_grouped: null argument");
  const SelectGroupedLayout E(group_offsets, (size_t) n_groups, (size_t) k, kLinOutWords);
  ScoreLayout Y;
  { const int rc = score_batch_queue(ctx, who, sp, fixed, fixed_index, moving, moving_index, n_items, poses, E.d_bytes, E.down_bytes, Y, E.table.data(), E.table_bytes()); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  { const int rc = select_queue_grouped<ScoreRow>(ctx, who, select_args(ds + Y.o_out, n_items, k, select), E, ds + Y.o_extra, (const int32_t*) (ds + Y.o_up), hs + Y.h_out); if (rc) return rc; }
  const int32_t* h = (const int32_t*) (hs + Y.h_out);
  for (size_t g = 0; g < E.G; ++g) score_block_out(h + E.group_words * g, E.K, g * E.K, out_index, out_H, out_b, out_stats);
  groups_report(h, E.group_words, E.G, out_n_selected, out_n_accepted, nullptr);
  return LSM2D_SUCCESS;
}

// ---- hypotheses scored against an aligner (lsm2d_score_aligner_batch's scoring: score_aligner_queue) ---------------------------------------------------------------
extern "C" int lsm2d_score_aligner_select(lsm2d_context* ctx, const lsm2d_batch* batch, const lsm2d_select_params* select, int32_t k, int32_t* out_index,
                                          float* out_H, float* out_b, lsm2d_iteration_stats* out_stats, int32_t* out_active, int32_t* out_n_selected,
                                          int32_t* out_n_accepted) {
  static const char who[] = "score_aligner_select";
  if (!select || !out_index || !out_n_selected || !out_n_accepted) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_aligner_select: null argument");
  if (k < 1 || k > kSelectMaxK) return fail(ctx, LSM2D_BAD_ARGUMENT, "score_aligner_select: k outside [1, LSM2D_SELECT_MAX_K]");
  { const int rc = score_aligner_head(ctx, who, batch); if (rc) return rc; }
  if (batch->n_alignments == 0) { *out_n_selected = 0; *out_n_accepted = 0; return LSM2D_SUCCESS; }
  const SelectLayout E((size_t) batch->n_alignments, (size_t) k, kCombWords);
  ScoreAlignerLayout Y;
  { const int rc = score_aligner_queue(ctx, who, batch, E.d_bytes, E.down_bytes, Y); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  HIPCHK(ctx, hipGetLastError());
  { const int rc = select_queue<CombRow>(ctx, who, select_args(ds + Y.o_comb, batch->n_alignments, k, select), E, ds + Y.o_extra, hs + Y.h_out); if (rc) return rc; }
  const int32_t* h = (const int32_t*) (hs + Y.h_out);
  comb_block_out(h, E.K, 0, out_index, out_H, out_b, out_stats, out_active);
  groups_report(h, 0, 1, out_n_selected, out_n_accepted, nullptr);
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
  if (batch->n_alignments == 0) { groups_report(nullptr, 0, (size_t) n_groups, out_n_selected, out_n_accepted, nullptr); return LSM2D_SUCCESS; }
  const SelectGroupedLayout E(group_offsets, (size_t) n_groups, (size_t) k, kCombWords);
  ScoreAlignerLayout Y;
  { const int rc = score_aligner_queue(ctx, who, batch, E.d_bytes, E.down_bytes, Y, E.table.data(), E.table_bytes()); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const hs = (char*) L.h_stage; char* const ds = (char*) L.d_scratch;
  HIPCHK(ctx, hipGetLastError());
  { const int rc = select_queue_grouped<CombRow>(ctx, who, select_args(ds + Y.o_comb, batch->n_alignments, k, select), E, ds + Y.o_extra, (const int32_t*) (ds + Y.o_up_extra), hs + Y.h_out); if (rc) return rc; }
  const int32_t* h = (const int32_t*) (hs + Y.h_out);
  for (size_t g = 0; g < E.G; ++g) comb_block_out(h + E.group_words * g, E.K, g * E.K, out_index, out_H, out_b, out_stats, out_active);
  groups_report(h, E.group_words, E.G, out_n_selected, out_n_accepted, nullptr);
  return LSM2D_SUCCESS;
}
