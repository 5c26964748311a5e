// lsm2d_capi_structures.inc -- parameter packing and what a set caches per finder: the NN grid, the KD-tree (level loop, one-launch and LDS forms), the lane-chunked copy with its circles, AoS rows, tile bounds, the distance map.
// Part of lsm2d_capi.hip (included there); not a translation unit of its own.
static bool valid_cloud_index(const lsm2d_cloudset* cs, int32_t i) { return cs && i >= 0 && i < cs->n_clouds; }
static bool valid_cloud_index_fwd(const lsm2d_cloudset* cs, int32_t i) { return valid_cloud_index(cs, i); }
// the set's largest cloud, in points (sizes the host knows, or upper bounds of sizes only the device knows); 0 for a set without clouds
static int max_cloud_count(const lsm2d_cloudset* cs) {
  int mx = 0;
  for (int c = 0; c < cs->n_clouds; ++c) if (cs->h_count[c] > mx) mx = cs->h_count[c];
  return mx;
}
// ---- parameter packing -------------------------------------------------------------------------------
// Depths are compared through r2: sqrtf is correctly rounded and monotone, so
//   rmin <= sqrtf(r2)  <=>  r2 >= r2lo,  r2lo = smallest float whose sqrtf reaches rmin   (same for rmax).
// Ranges are clamped to [1e-15, 1e18] m so r2 stays a normal fp32 number (the oracle applies the same clamp).
static float r2_lower_threshold(float rmin) {
  float v = rmin * rmin;
  while (sqrtf(v) >= rmin) v = nextafterf(v, 0.0f);
  while (sqrtf(v) < rmin) v = nextafterf(v, INFINITY);
  return v;
}
static float r2_upper_threshold(float rmax) {
  float v = rmax * rmax;
  while (sqrtf(v) <= rmax) v = nextafterf(v, INFINITY);
  while (sqrtf(v) > rmax) v = nextafterf(v, 0.0f);
  return v;
}
static bool make_projk(const lsm2d_projector& p, ProjK* k) {
  if (p.canvas_cols <= 0 || !(p.angle_max > p.angle_min) || !(p.range_max >= p.range_min) || !(p.range_min >= 0.0f)) return false;
  k->cols = p.canvas_cols;
  k->K00 = (float) p.canvas_cols / (p.angle_max - p.angle_min);
  k->K01 = (float) p.canvas_cols * 0.5f + p.col_offset;
  k->rmin = fmaxf(p.range_min, 1e-15f); k->rmax = fminf(p.range_max, 1e18f); k->colsf = (float) p.canvas_cols;
  if (!(k->rmax >= k->rmin)) return false;
  k->r2lo = r2_lower_threshold(k->rmin); k->r2hi = r2_upper_threshold(k->rmax);
  // The stream's short quotient min(|x|,|y|) / r (div_by_depth) is exact for min >= 1e-12; below that its result is merely SOME value
  // t' with |t'| <= A = 2.1e-12 / r, r >= rmin.  That cannot move a column when (i) pi/2 - t' and pi - t' round back to pi/2 and pi
  // (A below a quarter ulp of pi/2) and (ii) K00 * (+-t') + K01 rounds to K01 (K00 A below a quarter ulp of K01): then the kernels
  // drop the guard branch in front of the quotient.  True for every sane projector (cols 1081, 2 pi: K00 A ~ 2e-9 vs 1.5e-5).
  const double A = 2.1e-12 / (0.7 * (double) k->rmin);
  k->tiny_ok = (A < 2.5e-8 && k->K01 >= 0.25f && (double) k->K00 * A < (double) k->K01 * 1.4e-8) ? 1 : 0;
  return true;
}
static CloudDev cloud_dev(const lsm2d_cloudset* cs, const int32_t* d_index) {
  CloudDev c; c.xy = cs->d_xy; c.nrm = cs->d_nrm; c.start = cs->d_start; c.count = cs->d_count; c.index = d_index; c.n_clouds = cs->n_clouds;
  c.lane_xy = cs->derived.d_lane_xy; c.lane_start = cs->derived.d_lane_start; c.lane_T = cs->derived.d_lane_T; c.lane_bounds = cs->derived.d_lane_bounds;
  c.block_bounds = cs->derived.d_block_bounds; c.block_stride = cs->block_stride; c.aos = cs->derived.d_aos;
  c.tile_bounds = cs->derived.d_tile_bounds; c.tile_start = cs->derived.d_tile_start;
  c.grid = GridDev{nullptr, nullptr, nullptr, nullptr, nullptr};
  c.dist = DistDev{nullptr, nullptr};
  c.kd = KdDev{nullptr, nullptr, nullptr, nullptr, nullptr};
  return c;
}
// NN finder: uniform grid over every cloud of the (fixed) set, cached per max_distance.  Replaces
// CorrespondenceFinderKDTree2D::reset() (registration/correspondence_finder_kd_tree_2d.cpp:31-38).
static int ensure_grid(lsm2d_context* ctx, const lsm2d_cloudset* cs, float max_distance, GridDev* out) {
  for (const auto& g : cs->derived.grids)
    if (g.max_distance == max_distance) { *out = GridDev{g.d_meta, g.d_cell_start, g.d_sorted_idx, g.d_sorted_xy, g.d_sorted_nrm}; return LSM2D_SUCCESS; }
  const int nc = cs->n_clouds;
  std::vector<int32_t> cell_base(nc), gcap(nc);
  int64_t cells = 0;
  for (int c = 0; c < nc; ++c) {
    // cells per side: ~3 sqrt(n) for scan-sized clouds (their queries mostly find empty blocks; finer cells only add block
    // levels), ~6 sqrt(n) for map-sized ones (dense walls: the 3x3 block of a converged query holds 3x fewer candidates).
    // Measured on configs[1], role B: 3 sqrt(n) 3.12 ms, 6 sqrt(n) 2.95 ms, 12 sqrt(n) 3.24 ms (cell table out of L2).
    int cap = (int) ceil((cs->h_count[c] >= 16384 ? 0.1 * (double) ctx->grid_big_cells_x10 : 3.0) * sqrt((double) cs->h_count[c]));
    cap = cap < 16 ? 16 : (cap > 2048 ? 2048 : cap);       // 4096 buys 13 % on a 1M-point map for 4x the cell table: not taken
    gcap[c] = cap; cell_base[c] = (int32_t) cells; cells += (int64_t) cap * cap + 1;
    if (cells > 0x7fffffff) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "grid: too many cells");
  }
  GridCache g; g.max_distance = max_distance;      // (published to the set only once built: an early return takes the block with it)
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t) 255; return o; };
  const size_t o_meta = take(sizeof(GridMeta) * (size_t) nc), o_start = take(sizeof(int32_t) * (size_t) cells), o_cursor = take(sizeof(int32_t) * (size_t) cells);
  const size_t o_sidx = take(sizeof(int32_t) * (size_t) cs->padded_total), o_sxy = take(sizeof(float2) * (size_t) cs->padded_total), o_snr = take(sizeof(float2) * (size_t) cs->padded_total);
  const size_t o_base = take(sizeof(int32_t) * (size_t) nc), o_gcap = take(sizeof(int32_t) * (size_t) nc), o_tiles = take(sizeof(int32_t) * 2048);
  HIPCHK(ctx, g.d_block.alloc(off));
  char* blk = (char*) g.d_block;
  g.d_meta = (GridMeta*) (blk + o_meta); g.d_cell_start = (int32_t*) (blk + o_start); g.d_cursor = (int32_t*) (blk + o_cursor);
  g.d_sorted_idx = (int32_t*) (blk + o_sidx); g.d_sorted_xy = (float2*) (blk + o_sxy); g.d_sorted_nrm = (float2*) (blk + o_snr);
  int32_t* d_base = (int32_t*) (blk + o_base); int32_t* d_gcap = (int32_t*) (blk + o_gcap); int32_t* d_tiles = (int32_t*) (blk + o_tiles);
  HIPCHK(ctx, hipMemcpyAsync(d_base, cell_base.data(), sizeof(int32_t) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_gcap, gcap.data(), sizeof(int32_t) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  GridBuildArgs A;
  A.xy = cs->d_xy; A.start = cs->d_start; A.count = cs->d_count; A.n_clouds = nc; A.h_min = max_distance * 0.015625f;
  A.cell_base = d_base; A.gcap = d_gcap; A.meta = g.d_meta; A.cell_start = g.d_cell_start; A.cursor = g.d_cursor;
  A.sorted_idx = g.d_sorted_idx; A.sorted_xy = g.d_sorted_xy; A.nrm = cs->d_nrm; A.sorted_nrm = g.d_sorted_nrm;
  A.big_threshold = ctx->grid_big_threshold;
  hipLaunchKernelGGL(k_grid_build, dim3((unsigned) nc), dim3(1024), 0, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  // map-sized clouds: k_grid_build left them with their meta only; the counting sort runs over the whole chip, one cloud after the other
  for (int c = 0; c < nc; ++c) {
    if (cs->h_count[c] < ctx->grid_big_threshold) continue;
    const int64_t cells_max = (int64_t) gcap[c] * gcap[c] + 1;
    const int n_tiles = (int) ((cells_max + kGridTile - 1) / kGridTile);            // <= 1025: gcap <= 2048
    HIPCHK(ctx, hipMemsetAsync(g.d_cursor + cell_base[c], 0, sizeof(int32_t) * (size_t) cells_max, ctx->stream));
    GridBigArgs B;
    B.xy = cs->d_xy; B.start = cs->d_start; B.count = cs->d_count; B.cloud = c; B.meta = g.d_meta; B.cell_start = g.d_cell_start; B.cursor = g.d_cursor;
    B.tile_sums = d_tiles; B.sorted_idx = g.d_sorted_idx; B.sorted_xy = g.d_sorted_xy; B.nrm = cs->d_nrm; B.sorted_nrm = g.d_sorted_nrm;
    int pb = (cs->h_count[c] + 1023) / 1024; pb = pb < 1 ? 1 : (pb > 2048 ? 2048 : pb);
    hipLaunchKernelGGL(k_grid_big_hist, dim3((unsigned) pb), dim3(256), 0, ctx->stream, B);
    hipLaunchKernelGGL(k_grid_big_scan<0>, dim3((unsigned) n_tiles), dim3(1024), 0, ctx->stream, B);
    hipLaunchKernelGGL(k_grid_big_scan_tiles, dim3(1), dim3(1024), 0, ctx->stream, B.tile_sums, n_tiles);
    hipLaunchKernelGGL(k_grid_big_scan<1>, dim3((unsigned) n_tiles), dim3(1024), 0, ctx->stream, B);
    hipLaunchKernelGGL(k_grid_big_scatter, dim3((unsigned) pb), dim3(256), 0, ctx->stream, B);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, stream_sync(ctx));      // host vectors above must outlive the copies
  *out = GridDev{g.d_meta, g.d_cell_start, g.d_sorted_idx, g.d_sorted_xy, g.d_sorted_nrm};
  cs->derived.grids.push_back(std::move(g));
  return LSM2D_SUCCESS;
}

// KD-tree finder: CorrespondenceFinderKDTree2D::reset() (registration/correspondence_finder_kd_tree_2d.cpp:31-38) for every cloud of the
// (fixed) set, cached per (max_leaf_range, min_leaf_points).  Built on the device, level by level (k_kd_level: one wave per node); the
// host only learns, after each level, how many nodes the next one has.
// ---- the latency form of the KD-tree build (k_kd_build_scan): a handful of scan-sized clouds, working set in LDS.  Nothing is uploaded or cleared ahead of
// the kernel (it writes the set's KdMeta itself), and the fixed sets of an aligner call's KD-tree slices -- the live tracker: one scan per laser -- are built
// side by side by ONE launch with ONE wait for the trees' sizes (kd_scan_launch).
static constexpr int kKdScanCap = 1280;      // points per cloud the LDS layout is sized for (58 KB)
struct KdScanPrep {
  const lsm2d_cloudset* cs = nullptr; KdCache kc; KdBuildScanArgs W;      // (kc owns the block until kd_scan_launch publishes it)
  std::vector<KdMeta> h_meta;
};
static void kd_defaults(float& max_leaf_range, int& min_leaf_points) {      // the class defaults (correspondence_finder_kd_tree_2d.h:26-33), as the oracle applies them
  if (!(max_leaf_range > 0.0f)) max_leaf_range = 1e-2f;
  if (min_leaf_points <= 0) min_leaf_points = 20;
}
static const KdCache* kd_cached(const lsm2d_cloudset* cs, float max_leaf_range, int min_leaf_points) {
  for (const auto& k : cs->derived.kds) if (k.valid && k.max_leaf_range == max_leaf_range && k.min_leaf_points == min_leaf_points) return &k;
  return nullptr;
}
static bool kd_scan_eligible(const lsm2d_context* ctx, const lsm2d_cloudset* cs) {
  const int nc = cs->n_clouds;
  if (nc < 1 || nc > ctx->kd_scan_max_clouds || nc > 8 || cs->count_pending || (int) kd_scan_lds_bytes(kKdScanCap) > ctx->max_dyn_lds) return false;
  for (int c = 0; c < nc; ++c) if (cs->h_count[c] > kKdScanCap || cs->h_count[c] > ctx->kd_wg_max_points) return false;
  return true;
}
// The block the trees of a set are built into (meta, `nodes` nodes, the leaf-order arrays), owned by `kc` until the build has succeeded, and kc's views into it:
// the block a reserved single-cloud set kept across a change of its contents (cloudset_drop_grids) moves out of the set when it is large enough, else it goes
// and a new one is allocated
static int kd_take_block(lsm2d_context* ctx, const lsm2d_cloudset* cs, long long nodes, KdCache& kc) {
  const size_t np = (size_t) cs->padded_total;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t) 255; return o; };
  const size_t o_meta = take(sizeof(KdMeta) * (size_t) cs->n_clouds), o_nodes = take(sizeof(KdNode) * (size_t) nodes);
  const size_t o_lxy = take(sizeof(float2) * np), o_lidx = take(sizeof(int32_t) * np), o_lnr = take(sizeof(float2) * np);
  std::vector<KdCache>& kds = cs->derived.kds;
  kc.block_bytes = off;
  if (kds.size() == 1 && !kds[0].valid) {
    if (kds[0].d_block && kds[0].block_bytes >= off) { kc.d_block = std::move(kds[0].d_block); kc.block_bytes = kds[0].block_bytes; }
    kds.clear();
  }
  if (!kc.d_block) HIPCHK(ctx, kc.d_block.alloc(off));
  char* blk = (char*) kc.d_block;
  kc.d_meta = (KdMeta*) (blk + o_meta); kc.d_nodes = (KdNode*) (blk + o_nodes);
  kc.d_leaf_xy = (float2*) (blk + o_lxy); kc.d_leaf_idx = (int32_t*) (blk + o_lidx); kc.d_leaf_nrm = (float2*) (blk + o_lnr);
  return LSM2D_SUCCESS;
}
// the set's block (recycled for a reserved single-cloud set) and the kernel's arguments; no GPU work
static int kd_scan_prepare(lsm2d_context* ctx, const lsm2d_cloudset* cs, float max_leaf_range, int min_leaf_points, KdScanPrep& P) {
  const int nc = cs->n_clouds;
  P.cs = cs; P.kc = KdCache(); P.kc.max_leaf_range = max_leaf_range; P.kc.min_leaf_points = min_leaf_points;
  long long nodes = 0;
  for (int c = 0; c < nc; ++c) {
    P.W.node_base[c] = (int32_t) nodes;
    const long long room = cs->capacity > 0 ? cs->capacity : cs->h_count[c];      // (a reserved set: for whatever it may hold later -- its allocation is recycled)
    nodes += 2ll * room > 2 ? 2ll * room : 2;
  }
  KdCache& kc = P.kc;
  { const int rc = kd_take_block(ctx, cs, nodes, kc); if (rc) return rc; }
  KdBuildArgs B;
  B.start = cs->d_start; B.meta = kc.d_meta; B.nodes = kc.d_nodes; B.n_nodes = nullptr;
  B.leaf_xy = kc.d_leaf_xy; B.leaf_idx = kc.d_leaf_idx; B.max_leaf_range = max_leaf_range; B.min_leaf_points = min_leaf_points;
  B.xy_in = nullptr; B.idx_in = nullptr; B.xy_out = nullptr; B.idx_out = nullptr; B.q_in = nullptr; B.q_out = nullptr; B.q_out_count = nullptr; B.n_items = 0; B.n_items_ptr = nullptr; B.local_io = 0; B.io_base = 0; B.io_node_base = 0;
  P.W.B = B; P.W.count = cs->d_count; P.W.xy0 = cs->d_xy; P.W.nrm0 = cs->d_nrm; P.W.leaf_nrm = kc.d_leaf_nrm; P.W.meta_rw = kc.d_meta; P.W.cap = kKdScanCap; P.W.n_clouds = nc;
  P.h_meta.resize((size_t) nc);
  return LSM2D_SUCCESS;
}
// one launch for all prepared sets, one wait for their trees' sizes; the caches are published to their sets
static int kd_scan_launch(lsm2d_context* ctx, KdScanPrep* P, int count) {
  if (count <= 0) return LSM2D_SUCCESS;
  const size_t lds = kd_scan_lds_bytes(kKdScanCap);
  if (count == 1) {
    if (ctx->kd_chain == 1) hipLaunchKernelGGL(k_kd_build_scan<1>, dim3((unsigned) P[0].W.n_clouds), dim3(kKdScanThreads), lds, ctx->stream, P[0].W);
    else hipLaunchKernelGGL(k_kd_build_scan<0>, dim3((unsigned) P[0].W.n_clouds), dim3(kKdScanThreads), lds, ctx->stream, P[0].W);
  } else {
    KdBuildScanMulti M; int widest = 1;
    for (int i = 0; i < kMaxSlices; ++i) { M.w[i] = P[i < count ? i : 0].W; if (i >= count) M.w[i].n_clouds = 0; }
    for (int i = 0; i < count; ++i) if (P[i].W.n_clouds > widest) widest = P[i].W.n_clouds;
    if (ctx->kd_chain == 1) hipLaunchKernelGGL(k_kd_build_scan_multi<1>, dim3((unsigned) widest, (unsigned) count), dim3(kKdScanThreads), lds, ctx->stream, M);
    else hipLaunchKernelGGL(k_kd_build_scan_multi<0>, dim3((unsigned) widest, (unsigned) count), dim3(kKdScanThreads), lds, ctx->stream, M);
  }
  HIPCHK(ctx, hipGetLastError());
  for (int i = 0; i < count; ++i)
    HIPCHK(ctx, hipMemcpyAsync(P[i].h_meta.data(), P[i].kc.d_meta, sizeof(KdMeta) * P[i].h_meta.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  for (int i = 0; i < count; ++i) {
    KdCache& kc = P[i].kc;
    kc.levels = 0; kc.total_nodes = 0; kc.max_nodes_per_cloud = 0;
    for (const KdMeta& m : P[i].h_meta) { kc.total_nodes += m.n_nodes; if (m.n_nodes > kc.max_nodes_per_cloud) kc.max_nodes_per_cloud = m.n_nodes; if (m.pad0 > kc.levels) kc.levels = m.pad0; }
    ctx->last_kd_levels = kc.levels; ctx->last_kd_nodes = kc.total_nodes;
    P[i].cs->derived.kds.push_back(std::move(kc));
  }
  return LSM2D_SUCCESS;
}

static int ensure_kdtree(lsm2d_context* ctx, const lsm2d_cloudset* cs, float max_leaf_range, int min_leaf_points, KdDev* out, const KdCache** out_cache = nullptr) {
  kd_defaults(max_leaf_range, min_leaf_points);
  if (const KdCache* k = kd_cached(cs, max_leaf_range, min_leaf_points)) {
    *out = KdDev{k->d_meta, k->d_nodes, k->d_leaf_xy, k->d_leaf_idx, k->d_leaf_nrm}; if (out_cache) *out_cache = k; return LSM2D_SUCCESS;
  }
  if (kd_scan_eligible(ctx, cs)) {      // a handful of scan-sized clouds: the latency form
    KdScanPrep P;
    int rc = kd_scan_prepare(ctx, cs, max_leaf_range, min_leaf_points, P); if (rc) return rc;
    rc = kd_scan_launch(ctx, &P, 1); if (rc) return rc;
    const KdCache& k = cs->derived.kds.back();
    *out = KdDev{k.d_meta, k.d_nodes, k.d_leaf_xy, k.d_leaf_idx, k.d_leaf_nrm}; if (out_cache) *out_cache = &k;
    return LSM2D_SUCCESS;
  }
  const int nc = cs->n_clouds;
  // a cloud of n points has at most 2 n - 1 nodes (every split leaves both children non-empty); an empty cloud still has its root
  std::vector<KdMeta> meta((size_t) nc);
  long long nodes = 0;
  for (int c = 0; c < nc; ++c) {
    meta[(size_t) c].node_base = (int32_t) nodes; meta[(size_t) c].n_nodes = 0; meta[(size_t) c].pad0 = meta[(size_t) c].pad1 = 0;
    const long long room = cs->capacity > 0 ? cs->capacity : cs->h_count[c];      // (a reserved set: for whatever it may hold later -- its allocation is recycled)
    nodes += 2ll * room > 2 ? 2ll * room : 2;
    if (nodes > 0x7ffffff0ll) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "kdtree: too many nodes");
  }
  const size_t np = (size_t) cs->padded_total, nq = np / 2 + (size_t) nc + 2;
  constexpr int kMaxLevels = 8192;
  KdCache kc; kc.max_leaf_range = max_leaf_range; kc.min_leaf_points = min_leaf_points;
  { const int rc = kd_take_block(ctx, cs, nodes, kc); if (rc) return rc; }
  // working set of the build: two ping-pong copies of (xy, idx), two queues, per-cloud node counters, one queue counter per level
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t) 255; return o; };
  const size_t w_xy0 = take(sizeof(float2) * np), w_xy1 = take(sizeof(float2) * np), w_ix0 = take(sizeof(int32_t) * np), w_ix1 = take(sizeof(int32_t) * np);
  const size_t w_q0 = take(sizeof(int4) * nq), w_q1 = take(sizeof(int4) * nq), w_nn = take(sizeof(int32_t) * (size_t) nc), w_cnt = take(sizeof(int32_t) * (size_t) (kMaxLevels + 1));
  HIPCHK(ctx, ctx->d_kd_work.ensure(off, off + off / 2, wait_for_stream(ctx)));
  char* wk = (char*) ctx->d_kd_work;
  float2* xyb[2] = {(float2*) (wk + w_xy0), (float2*) (wk + w_xy1)}; int32_t* ixb[2] = {(int32_t*) (wk + w_ix0), (int32_t*) (wk + w_ix1)};
  int4* qb[2] = {(int4*) (wk + w_q0), (int4*) (wk + w_q1)};
  int32_t* d_nn = (int32_t*) (wk + w_nn); int32_t* d_cnt = (int32_t*) (wk + w_cnt);
  HIPCHK(ctx, hipMemcpyAsync(kc.d_meta, meta.data(), sizeof(KdMeta) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * (size_t) (kMaxLevels + 1), ctx->stream));
  KdBuildArgs B;
  B.start = cs->d_start; B.meta = kc.d_meta; B.nodes = kc.d_nodes; B.n_nodes = d_nn;
  B.leaf_xy = kc.d_leaf_xy; B.leaf_idx = kc.d_leaf_idx; B.max_leaf_range = max_leaf_range; B.min_leaf_points = min_leaf_points;
  B.xy_in = nullptr; B.idx_in = nullptr; B.xy_out = nullptr; B.idx_out = nullptr; B.q_in = nullptr; B.q_out = nullptr; B.q_out_count = nullptr; B.n_items = 0; B.n_items_ptr = nullptr; B.local_io = 0; B.io_base = 0; B.io_node_base = 0;
  // Scan-sized clouds: ONE launch builds every such tree, a workgroup per cloud walking its levels itself (k_kd_build_wg) -- no host round trip per level.
  // Map-sized clouds keep the level loop (a level of theirs fills the chip): their roots are queued here, the host learns every level's node count.
  const int wg_max = ctx->kd_wg_max_points;
  std::vector<int4> roots; std::vector<int32_t> ones((size_t) nc, 1);
  int n_small = 0;
  for (int c = 0; c < nc; ++c) { if (cs->h_count[c] <= wg_max) ++n_small; else roots.push_back(make_int4(c, 0, 0, cs->h_count[c])); }
  HIPCHK(ctx, hipMemcpyAsync(d_nn, ones.data(), sizeof(int32_t) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  if (n_small > 0) {
    KdBuildWgArgs W; W.B = B; W.count = cs->d_count; W.xy0 = cs->d_xy; W.nrm0 = cs->d_nrm;
    W.xy_buf[0] = xyb[0]; W.xy_buf[1] = xyb[1]; W.idx_buf[0] = ixb[0]; W.idx_buf[1] = ixb[1]; W.q_buf[0] = qb[0]; W.q_buf[1] = qb[1];
    W.leaf_nrm = kc.d_leaf_nrm; W.meta_rw = kc.d_meta; W.max_points = wg_max;
    if (ctx->kd_chain == 1) hipLaunchKernelGGL(k_kd_build_wg<1>, dim3((unsigned) nc), dim3(256), 0, ctx->stream, W);
    else hipLaunchKernelGGL(k_kd_build_wg<0>, dim3((unsigned) nc), dim3(256), 0, ctx->stream, W);
    HIPCHK(ctx, hipGetLastError());
  }
  long long n_items = (long long) roots.size(); int level = 0;
  std::vector<KdMeta> h_meta((size_t) nc);
  if (n_items > 0) {
    // (the big clouds' items use the queue buffers from position 0: the small clouds' stretches -- start / 2 + c -- are theirs alone only while the
    // workgroup build runs, and the stream orders the two)
    HIPCHK(ctx, hipMemcpyAsync(qb[0], roots.data(), sizeof(int4) * roots.size(), hipMemcpyHostToDevice, ctx->stream));
    // Levels are launched back to back with an UPPER BOUND of their item count (a level cannot hold more items than roots x 2^level, nor more than
    // there are groups of max(min_leaf_points, 2) points); the kernel reads the true count where the previous level left it, waves beyond it leave at
    // once, a level with no items does nothing.  The host reads the counts after as many levels as a balanced tree would have, then every four levels.
    long long big_points = 0; for (const int4& r : roots) big_points += r.w;
    const long long per_item = min_leaf_points > 2 ? min_leaf_points : 2;
    const long long cap_items = big_points / per_item + (long long) roots.size();
    const int32_t n_roots = (int32_t) roots.size();
    HIPCHK(ctx, hipMemcpyAsync(d_cnt, &n_roots, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));      // (pageable source: copied before the call returns)
    int expect = 4; for (long long m = cap_items; m > 1; m >>= 1) ++expect;      // (a 100k-point map with 20-point leaves: 16 launches for its 15 levels)
    std::vector<int32_t> h_counts;
    bool more = true;
    while (more) {
      const int until = level == 0 ? expect : level + 4;
      for (; level < until; ++level) {
        if (level >= kMaxLevels) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "kdtree: deeper than 8192 levels");
        B.xy_in = level == 0 ? cs->d_xy : xyb[level & 1]; B.idx_in = level == 0 ? nullptr : ixb[level & 1];
        B.xy_out = xyb[(level + 1) & 1]; B.idx_out = ixb[(level + 1) & 1];
        B.q_in = qb[level & 1]; B.q_out = qb[(level + 1) & 1]; B.q_out_count = d_cnt + level + 1; B.n_items = 0; B.n_items_ptr = d_cnt + level;
        long long bound = level < 40 ? ((long long) n_roots << level) : cap_items; if (bound > cap_items) bound = cap_items;
        // the top levels of a map-sized cloud -- while an evenly split node would still hold "kd_wide_min_points" points --: a workgroup per node (kd_node_wide)
        const bool wide = ctx->kd_wide_min_points > 0 && level < 40 && (big_points / n_roots) >> level >= ctx->kd_wide_min_points;
        if (wide) {
          if (ctx->kd_chain == 1) hipLaunchKernelGGL(k_kd_level_wide<1>, dim3((unsigned) bound), dim3(256), 0, ctx->stream, B);
          else hipLaunchKernelGGL(k_kd_level_wide<0>, dim3((unsigned) bound), dim3(256), 0, ctx->stream, B);
        } else {
          const unsigned blocks = (unsigned) ((bound + 3) / 4);
          if (ctx->kd_chain == 1) hipLaunchKernelGGL(k_kd_level<1>, dim3(blocks), dim3(256), 0, ctx->stream, B);
          else hipLaunchKernelGGL(k_kd_level<0>, dim3(blocks), dim3(256), 0, ctx->stream, B);
        }
      }
      // the big clouds' sizes and leaf-order normals (the workgroup build wrote its own clouds') go out with every batch of levels -- they are right as soon
      // as the last level has run, which is nearly always the first batch -- and the counts and the sizes come back with ONE wait
      hipLaunchKernelGGL(k_kd_finish, dim3((unsigned) ((nc + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t*) d_nn, nc, kc.d_meta);
      for (int c = 0; c < nc; ++c) {
        if (cs->h_count[c] <= wg_max) continue;
        int gx = (cs->h_count[c] + 255) / 256; if (gx > 1024) gx = 1024;
        hipLaunchKernelGGL(k_kd_permute_normals, dim3((unsigned) gx, 1u), dim3(256), 0, ctx->stream, (const float2*) cs->d_nrm,
                           (const int32_t*) cs->d_start, (const int32_t*) cs->d_count, (const int32_t*) kc.d_leaf_idx, kc.d_leaf_nrm, c);
      }
      HIPCHK(ctx, hipGetLastError());
      h_counts.resize((size_t) level + 1);
      HIPCHK(ctx, hipMemcpyAsync(h_counts.data(), d_cnt, sizeof(int32_t) * ((size_t) level + 1), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipMemcpyAsync(h_meta.data(), kc.d_meta, sizeof(KdMeta) * (size_t) nc, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, stream_sync(ctx));
      more = h_counts[(size_t) level] > 0;
    }
    level = 0; while ((size_t) level < h_counts.size() && h_counts[(size_t) level] > 0) ++level;      // levels that held items: what the level-by-level loop counted
  }
  else {      // what the host needs of the result: every tree's node count (and, of the workgroup builds, the depth): one read, one wait
    HIPCHK(ctx, hipMemcpyAsync(h_meta.data(), kc.d_meta, sizeof(KdMeta) * (size_t) nc, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_sync(ctx));
  }
  kc.levels = level; kc.total_nodes = 0; kc.max_nodes_per_cloud = 0;
  for (int c = 0; c < nc; ++c) {
    const int nn = h_meta[(size_t) c].n_nodes;
    kc.total_nodes += nn; if (nn > kc.max_nodes_per_cloud) kc.max_nodes_per_cloud = nn;
    if (cs->h_count[c] <= wg_max && h_meta[(size_t) c].pad0 > kc.levels) kc.levels = h_meta[(size_t) c].pad0;
  }
  ctx->last_kd_levels = kc.levels; ctx->last_kd_nodes = kc.total_nodes;
  *out = KdDev{kc.d_meta, kc.d_nodes, kc.d_leaf_xy, kc.d_leaf_idx, kc.d_leaf_nrm};
  cs->derived.kds.push_back(std::move(kc));
  if (out_cache) *out_cache = &cs->derived.kds.back();
  return LSM2D_SUCCESS;
}

static CloudDev cloud_dev_with_tiles(CloudDev c, const lsm2d_cloudset* cs) { c.tile_bounds = cs->derived.d_tile_bounds; c.tile_start = cs->derived.d_tile_start; return c; }

// lane-chunked copy of every cloud for k_align's projective streaming pass (project_cloud_lanes in lsm2d_device.h), with the bounding circles of
// every thread's chunk and of every block of it (the exact culling).  Everything is built into guarded temporaries and PUBLISHED to the set only
// after the last launch has finished (round-3 advisor: a failure half-way used to leave d_lane_xy set and never filled -- the next call streamed
// uninitialised memory).
static int ensure_lane_layout(lsm2d_context* ctx, const lsm2d_cloudset* cs) {
  if (cs->derived.d_lane_xy || cs->count_pending) return LSM2D_SUCCESS;     // a size-pending set is a clipped scene: small, and building needs a sync
  const int nc = cs->n_clouds;
  bool any_big = false;                       // every cloud <= one pair per thread: the plain layout already is lane-chunked
  for (int c = 0; c < nc; ++c) if (((long long) cs->h_count[c] + 1) / 2 > kAlignBlock) { any_big = true; break; }
  if (!any_big) return LSM2D_SUCCESS;
  // project_cloud_lanes walks a cloud's rows with a 32-bit scalar byte offset: a cloud beyond 2^31 bytes of slots
  // (> 2.6e8 points) keeps the plain layout and project_cloud
  for (int c = 0; c < nc; ++c) if ((((long long) cs->h_count[c] + 1) / 2 + kAlignBlock) * (long long) sizeof(float4) >= (1ll << 31)) return LSM2D_SUCCESS;
  std::vector<long long> lstart((size_t) nc); std::vector<int32_t> lT((size_t) nc);
  long long slots = 0; int maxT = 1;
  for (int c = 0; c < nc; ++c) {
    const long long npairs = ((long long) cs->h_count[c] + 1) / 2;
    const int T = (int) ((npairs + kAlignBlock - 1) / kAlignBlock);
    lstart[c] = slots; lT[c] = T; slots += (long long) T * kAlignBlock; if (T > maxT) maxT = T;
  }
  if (slots == 0) slots = 1;
  slots += 2 * kAlignBlock;      // two spare rows behind the last cloud: project_cloud_units' look-ahead load may read one row past a cloud's last
  // block circles: 57 KB per cloud.  They are what the kept unit lists are built from -- worth it for a map or a few thousand big clouds, not for tens of
  // thousands of scan-sized moving clouds (round-4 advisor: several GB there): beyond 256 MB the set goes without them and its batches run the chunk-level
  // stream of the shared instantiation (proj_culled_for_all needs block_bounds)
  const int nbs = kCullBlocks;      // blocks per chunk (lsm2d_kernels.h)
  const bool want_blocks = sizeof(float4) * (size_t) nc * nbs * kAlignBlock <= ((size_t) 256 << 20);
  DevBuf<float4> d_xy, d_bounds, d_blocks; DevBuf<long long> d_start; DevBuf<int32_t> d_T;
  HIPCHK(ctx, d_xy.alloc(sizeof(float4) * (size_t) slots));
  HIPCHK(ctx, d_bounds.alloc(sizeof(float4) * (size_t) nc * kAlignBlock));
  if (want_blocks) HIPCHK(ctx, d_blocks.alloc(sizeof(float4) * (size_t) nc * nbs * kAlignBlock));
  HIPCHK(ctx, d_start.alloc(sizeof(long long) * (size_t) nc));
  HIPCHK(ctx, d_T.alloc(sizeof(int32_t) * (size_t) nc));
  HIPCHK(ctx, hipMemsetAsync(d_xy + (slots - 2 * kAlignBlock), 0x7f, sizeof(float4) * 2 * kAlignBlock, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_start, lstart.data(), sizeof(long long) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_T, lT.data(), sizeof(int32_t) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  long long per = (long long) maxT * kAlignBlock; int gx = (int) ((per + 255) / 256); if (gx > 2048) gx = 2048; if (gx < 1) gx = 1;
  for (int c0 = 0; c0 < nc; c0 += 32768) {         // gridDim.y is limited to 65535
    const int ny = nc - c0 < 32768 ? nc - c0 : 32768;
    hipLaunchKernelGGL(k_lane_layout, dim3((unsigned) gx, (unsigned) ny), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy,
                       (const int32_t*) cs->d_start, (const int32_t*) cs->d_count, (const long long*) d_start,
                       (const int32_t*) d_T, (int) kAlignBlock, d_xy, c0);
    hipLaunchKernelGGL(k_lane_bounds, dim3((unsigned) (kAlignBlock / 4), (unsigned) ny), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy,
                       (const int32_t*) cs->d_start, (const int32_t*) cs->d_count, (const int32_t*) d_T, (int) kAlignBlock, d_bounds, c0);
    if (want_blocks)
      hipLaunchKernelGGL(k_block_bounds, dim3((unsigned) (kAlignBlock * nbs / 4), (unsigned) ny), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy,
                         (const int32_t*) cs->d_start, (const int32_t*) cs->d_count, (const int32_t*) d_T, (int) kAlignBlock, d_blocks, c0, nbs);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, stream_sync(ctx));        // the host vectors above back the async copies; and only a finished build is published
  cs->derived.d_lane_xy = std::move(d_xy); cs->derived.d_lane_bounds = std::move(d_bounds); cs->derived.d_block_bounds = std::move(d_blocks);
  cs->derived.d_lane_start = std::move(d_start); cs->derived.d_lane_T = std::move(d_T);
  cs->block_stride = nbs;
  return LSM2D_SUCCESS;
}

// (x, y, nx, ny) rows of the whole set: k_align's bin walk gathers a z-buffer winner's point and normal as one 16-byte row
static int ensure_aos(lsm2d_context* ctx, const lsm2d_cloudset* cs) {
  if (cs->derived.d_aos || cs->count_pending || cs->unpack_pending || cs->prep_pending) return LSM2D_SUCCESS;      // (a set still changing on the device is gathered from its split arrays)
  DevBuf<float4> t;
  HIPCHK(ctx, t.alloc(sizeof(float4) * (size_t) cs->padded_total));
  long long blocks = (cs->padded_total + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_aos_rows, dim3((unsigned) blocks), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy, (const float2*) cs->d_nrm, (long long) cs->padded_total, t);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, stream_sync(ctx));
  cs->derived.d_aos = std::move(t);
  return LSM2D_SUCCESS;
}

// bounding circles of every cloud's tiles of 64 consecutive points: what k_align's point-query branch tests before it runs a tile's queries
static int ensure_tile_bounds(lsm2d_context* ctx, const lsm2d_cloudset* cs) {
  if (cs->derived.d_tile_bounds || cs->count_pending) return LSM2D_SUCCESS;
  const int nc = cs->n_clouds;
  std::vector<int32_t> tstart((size_t) nc);
  long long tiles = 0; int max_tiles = 1;
  for (int c = 0; c < nc; ++c) {
    const int t = (cs->h_count[c] + 63) / 64;
    tstart[c] = (int32_t) tiles; tiles += t; if (t > max_tiles) max_tiles = t;
    if (tiles > 0x7fffffff) return LSM2D_SUCCESS;          // (no culling for such a set)
  }
  DevBuf<float4> t_bounds; DevBuf<int32_t> t_start;      // published only when complete (see ensure_lane_layout)
  HIPCHK(ctx, t_bounds.alloc(sizeof(float4) * (size_t) (tiles > 0 ? tiles : 1)));
  HIPCHK(ctx, t_start.alloc(sizeof(int32_t) * (size_t) nc));
  HIPCHK(ctx, hipMemcpyAsync(t_start, tstart.data(), sizeof(int32_t) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  int gx = (max_tiles + 3) / 4; if (gx > 4096) gx = 4096; if (gx < 1) gx = 1;
  for (int c0 = 0; c0 < nc; c0 += 32768) {
    const int ny = nc - c0 < 32768 ? nc - c0 : 32768;
    hipLaunchKernelGGL(k_tile_bounds, dim3((unsigned) gx, (unsigned) ny), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy, (const int32_t*) cs->d_start,
                       (const int32_t*) cs->d_count, (const int32_t*) t_start, t_bounds, c0);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, stream_sync(ctx));        // the host vector above backs the async copy
  cs->derived.d_tile_bounds = std::move(t_bounds); cs->derived.d_tile_start = std::move(t_start);
  return LSM2D_SUCCESS;
}

// Distance-map finder: CorrespondenceFinderNN2D::reset() (registration/correspondence_finder_nn_2d.cpp:10-52,84-97) for every
// cloud of the (fixed) set, cached per (max_distance, resolution).
static int ensure_distmap(lsm2d_context* ctx, const lsm2d_cloudset* cs, float max_distance, float resolution, DistDev* out) {
  for (const auto& d : cs->derived.dists)
    if (d.max_distance == max_distance && d.resolution == resolution) { *out = DistDev{d.d_meta, d.d_parent}; return LSM2D_SUCCESS; }
  if (!(resolution > 0.0f) || max_distance < 0.0f) return fail(ctx, LSM2D_BAD_ARGUMENT, "distmap: resolution must be > 0 and max_distance >= 0");
  const int nc = cs->n_clouds;
  DevBuf<float4> d_bbox;
  HIPCHK(ctx, d_bbox.alloc(sizeof(float4) * (size_t) nc));
  hipLaunchKernelGGL(k_cloud_bbox, dim3((unsigned) nc), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy, (const int32_t*) cs->d_start,
                     (const int32_t*) cs->d_count, d_bbox);
  HIPCHK(ctx, hipGetLastError());
  std::vector<float4> bbox((size_t) nc);
  HIPCHK(ctx, hipMemcpyAsync(bbox.data(), d_bbox, sizeof(float4) * (size_t) nc, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  const float inv_res = 1.0f / resolution;
  const float mds_px = max_distance * max_distance * inv_res * inv_res;
  const int padding = (int) (sqrtf(mds_px) + 75.5f);
  const int R = (int) floor(sqrt((double) mds_px));
  std::vector<DistMeta> meta((size_t) nc);
  long long total = 0; int max_rows_cols = 0;
  for (int c = 0; c < nc; ++c) {
    const float lx = bbox[c].x, ly = bbox[c].y, ux = bbox[c].z, uy = bbox[c].w;
    const double rows = ceil((double) ((ux - lx) * inv_res + (float) padding)), cols = ceil((double) ((uy - ly) * inv_res + (float) padding));
    if (!(rows >= 1 && cols >= 1) || rows * cols > 400e6) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "distmap: grid too large");
    DistMeta& m = meta[c];
    m.lx = lx; m.ly = ly; m.inv_res = inv_res; m.half_pad = (float) padding * 0.5f; m.rows = (int) rows; m.cols = (int) cols; m.base = total;
    total += (long long) m.rows * m.cols;
    if (m.rows * (long long) m.cols > max_rows_cols) max_rows_cols = (int) (m.rows * (long long) m.cols > 0x7fffffff ? 0x7fffffff : m.rows * (long long) m.cols);
    if (total > (1ll << 33)) return fail(ctx, LSM2D_CAPACITY_EXCEEDED, "distmap: more than 8 Gi pixels in one set");
  }
  // scatter build (every point stamps its disc, k_distmap_stamp) whenever (d2, index) packs into 31 bits; else the gather build
  const int max_pts = std::max(1, max_cloud_count(cs));
  int gbits = 1; while (gbits < 31 && (1ll << gbits) < (long long) max_pts) ++gbits;
  const bool scatter = ctx->distmap_build != 1 && R <= 511 && (((long long) R * R + 1) << gbits) <= (1ll << 31);
  for (auto& m : meta) { m.gbits = scatter ? gbits : 31; m.gmask = scatter ? (int32_t) ((1u << gbits) - 1u) : 0x7fffffff; }
  DistCache d; d.max_distance = max_distance; d.resolution = resolution;
  DevBuf<int32_t> d_cellgoal;      // (the gather build's working set: goes with this call)
  HIPCHK(ctx, d.d_meta.alloc(sizeof(DistMeta) * (size_t) nc));
  HIPCHK(ctx, d.d_parent.alloc(sizeof(int32_t) * (size_t) total));
  HIPCHK(ctx, hipMemcpyAsync(d.d_meta, meta.data(), sizeof(DistMeta) * (size_t) nc, hipMemcpyHostToDevice, ctx->stream));
  if (scatter) {
    HIPCHK(ctx, hipMemsetAsync(d.d_parent, 0xff, sizeof(int32_t) * (size_t) total, ctx->stream));
    int sb = (max_pts + 3) / 4; if (sb > 16384) sb = 16384;
    for (int c0 = 0; c0 < nc; c0 += 32768) {         // gridDim.y is limited to 65535
      const int ny = nc - c0 < 32768 ? nc - c0 : 32768;
      hipLaunchKernelGGL(k_distmap_stamp, dim3((unsigned) sb, (unsigned) ny), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy,
                         (const int32_t*) cs->d_start, (const int32_t*) cs->d_count, (const DistMeta*) d.d_meta, (uint32_t*) d.d_parent.get(), mds_px, R, c0);      // (the stamps are unsigned minima over the map's int32 cells)
    }
  } else {
    HIPCHK(ctx, d_cellgoal.alloc(sizeof(int32_t) * (size_t) total));
    HIPCHK(ctx, hipMemsetAsync(d_cellgoal, 0x7f, sizeof(int32_t) * (size_t) total, ctx->stream));
    int gb = (max_pts + 255) / 256; if (gb > 1024) gb = 1024;
    int fb = (max_rows_cols + 255) / 256; if (fb > 4096) fb = 4096; if (fb < 1) fb = 1;
    for (int c0 = 0; c0 < nc; c0 += 32768) {
      const int ny = nc - c0 < 32768 ? nc - c0 : 32768;
      hipLaunchKernelGGL(k_distmap_goals, dim3((unsigned) gb, (unsigned) ny), dim3(256), 0, ctx->stream, (const float2*) cs->d_xy,
                         (const int32_t*) cs->d_start, (const int32_t*) cs->d_count, (const DistMeta*) d.d_meta, d_cellgoal, c0);
    }
    for (int c0 = 0; c0 < nc; c0 += 32768) {
      const int ny = nc - c0 < 32768 ? nc - c0 : 32768;
      hipLaunchKernelGGL(k_distmap_fill, dim3((unsigned) fb, (unsigned) ny), dim3(256), 0, ctx->stream, (const DistMeta*) d.d_meta,
                         (const int32_t*) d_cellgoal, d.d_parent, mds_px, R, c0);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, stream_sync(ctx));
  *out = DistDev{d.d_meta, d.d_parent};
  cs->derived.dists.push_back(std::move(d));
  return LSM2D_SUCCESS;
}

static Iso make_iso(const float pose[3]) { Iso T; sincos_fixed(pose[2], T.s, T.c); T.tx = pose[0]; T.ty = pose[1]; return T; }
static float wrap_host(float a) {
  if (!(fabsf(a) < 3.0e7f)) return NAN;      // (wrap_angle: the loops below would never end)
  while (a > 3.14159274101257324f) a -= 6.28318548202514648f;
  while (a <= -3.14159274101257324f) a += 6.28318548202514648f;
  return a;
}
static void inverse_host(const float a[3], float out[3]) {   // (R,t)^-1 = (R^T, -R^T t)
  float s, c; sincos_fixed(a[2], s, c);
  out[0] = -(fmaf(c, a[0], s * a[1]));
  out[1] = -(fmaf(-s, a[0], c * a[1]));
  out[2] = wrap_host(-a[2]);
}
static void compose_host(const float a[3], const float b[3], float out[3]) {   // v2t(a) * v2t(b)
  float s, c; sincos_fixed(a[2], s, c);
  out[0] = fmaf(c, b[0], fmaf(-s, b[1], a[0]));
  out[1] = fmaf(s, b[0], fmaf(c, b[1], a[1]));
  out[2] = wrap_host(a[2] + b[2]);
}

// z-buffer of one cloud spread over many workgroups into a global canvas (d_canvas: cols u64 cells)
static int project_split(lsm2d_context* ctx, const float2* d_xy, int n, const Iso& T, const ProjK& P, u64* d_canvas) {
  HIPCHK(ctx, hipMemsetAsync(d_canvas, 0xFF, sizeof(u64) * (size_t) P.cols, ctx->stream));
  if (n <= 0) return LSM2D_SUCCESS;
  ProjectSplitArgs A; A.xy = d_xy; A.n = n; A.T = T; A.proj = P; A.gcanvas = d_canvas;
  int blocks = (n + 8191) / 8192; if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(k_project_split, dim3(blocks), dim3(512), sizeof(u64) * (size_t) P.cols, ctx->stream, A);
  HIPCHK(ctx, hipGetLastError());
  return LSM2D_SUCCESS;
}

// a BATCH of scans: the small form of the kernel (512 threads, 37 KB: the footprint of one k_align workgroup) whenever the beams fit it -- it runs beside a launch in
// flight in single slots as they come free, four to a CU when the chip is idle; a handful of scans keep one beam per thread (a scan's latency, the tracker's concern)
