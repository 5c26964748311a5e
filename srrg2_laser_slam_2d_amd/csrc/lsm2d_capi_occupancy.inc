// lsm2d_capi_occupancy.inc -- occupancy grids on the device: grid sets (create, clear, upload, download, destroy), lsm2d_occupancy_update (the points of
// device-resident clouds ray-traced from their sensor poses into hit / miss counters) and lsm2d_occupancy_render (include/lsm2d.h; PARITY.md section 3,
// item 17c; not in the reference, which has no grid mapper).  Part of lsm2d_capi.hip.
//
// lsm2d_occupancy_update:
//   up          the call's tables -- per input (transform, ray start, where its points begin, its grid), the concatenation offsets, the inputs' boxes as
//               {max, max, min, min}, per grid the range of its inputs -- through the lane's pinned staging buffer into its scratch: one copy.  The inputs are
//               listed grid by grid (a stable counting sort on the host): a tile's workgroup loops over its own grid's inputs only.
//   the chain   k_occ_rays, k_occ_tiles<false> -- on the context's stream in order
//   down        [rays | dropped | fault]: ONE copy, ONE wait.  With kernel timing on the tile workgroups' clock stamps follow in a copy of their own
//               (diagnostics: "last_occupancy_wg_median_ns" / "last_occupancy_wg_max_ns").
// lsm2d_occupancy_update_scans (0.7.13; item 17d): the same shape from raw range scans, no cloud set and no size fetch:
//   up          the tables as above -- a row per scan, the regular offsets j * n_beams, boxes, per grid its scans -- and, behind them in the same staging
//               block, pageable ranges: one copy.  Pinned ranges are copied from directly; device-resident ranges are read in place.
//   the chain   k_occ_beams, k_occ_tiles<true>
//   down        [hit | clear | dropped | fault]: ONE copy, ONE wait; the stamps as above.
// Into a log-odds set the second kernel of either chain is k_occ_tiles_logodds<kKinds>.  The two calls differ in their refusals, in the first kernel and in
// what travels up; the layout, the geometry, the tables, the tile launch and the finish are one function each, and the two render calls share their tail.

struct lsm2d_gridset {
  lsm2d_context* ctx = nullptr;
  lsm2d_grid_geometry geo = {};
  int32_t n_grids = 0;
  size_t cells_per_grid = 0;
  DevBuf<uint2> d_cells;         // [n_grids][height][width] = {hits, misses}: a cell is one 8-byte access
  bool logodds = false;          // 0.7.14: a set of the second kind, a cell is {int32 value, uint32 observed} (item 17e)
  lsm2d_logodds_params lp = {};  // ... and the votes and clamps of its updates
};

static void orphan_gridsets(lsm2d_context* ctx) { for (lsm2d_gridset* gs : ctx->live_gridsets) gs->ctx = nullptr; }

extern "C" int lsm2d_gridset_create(lsm2d_context* ctx, const lsm2d_grid_geometry* geo, int32_t n_grids, lsm2d_gridset** out) {
  static_assert(LSM2D_OCCUPANCY_MAX_SIDE == kOccMaxSide && LSM2D_OCCUPANCY_MAX_CELLS == kOccMaxCells && LSM2D_OCCUPANCY_MAX_RAYS == kOccMaxRays &&
                LSM2D_OCCUPANCY_MAX_RAY_CELLS == kOccMaxRayCells, "the ABI's limits are the kernels'");
  if (out) *out = nullptr;
  if (!ctx || !geo || !out) return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_create: null argument");
  if (!(geo->resolution > 0.0f) || !std::isfinite(geo->resolution)) return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_create: resolution must be finite and > 0");
  if (!std::isfinite(geo->origin_x) || !std::isfinite(geo->origin_y)) return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_create: the origin must be finite");
  if (geo->width < 1 || geo->height < 1 || geo->width > kOccMaxSide || geo->height > kOccMaxSide)
    return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_create: a side must lie in 1 .. LSM2D_OCCUPANCY_MAX_SIDE");
  if (n_grids < 1) return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_create: n_grids must be >= 1");
  const long long per = (long long) geo->width * geo->height;
  if (per * n_grids > (long long) kOccMaxCells) return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_create: more cells than LSM2D_OCCUPANCY_MAX_CELLS");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  struct Destroy { void operator()(lsm2d_gridset* g) const { lsm2d_gridset_destroy(g); } };
  std::unique_ptr<lsm2d_gridset, Destroy> gs(new (std::nothrow) lsm2d_gridset);      // (as a cloud set: registered at once, destroyed by any return before it is released into *out)
  if (!gs) return LSM2D_OUT_OF_MEMORY;
  gs->ctx = ctx; ctx->live_gridsets.push_back(gs.get());
  gs->geo = *geo; gs->n_grids = n_grids; gs->cells_per_grid = (size_t) per;
  HIPCHK(ctx, gs->d_cells.alloc(sizeof(uint2) * gs->cells_per_grid * (size_t) n_grids));
  HIPCHK(ctx, hipMemsetAsync(gs->d_cells, 0, sizeof(uint2) * gs->cells_per_grid * (size_t) n_grids, ctx->stream));
  *out = gs.release();
  return LSM2D_SUCCESS;
}

extern "C" void lsm2d_gridset_destroy(lsm2d_gridset* gs) {
  if (!gs) return;
  if (gs->ctx) {
    (void) hipSetDevice(gs->ctx->device);
    (void) stream_sync(gs->ctx);      // a queued clear or update may still write the cells
    auto& v = gs->ctx->live_gridsets;
    for (size_t i = 0; i < v.size(); ++i) if (v[i] == gs) { v[i] = v.back(); v.pop_back(); break; }
  }
  delete gs;      // (its cells go with it)
}

static bool valid_grid_index(const lsm2d_gridset* gs, int32_t i) { return gs && i >= 0 && i < gs->n_grids; }

extern "C" int lsm2d_gridset_clear(lsm2d_gridset* gs, int32_t n, const int32_t* grid_index) {
  if (!gs || !gs->ctx) return fail(gs ? gs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "gridset_clear: null argument (or the set's context is gone)");
  lsm2d_context* ctx = gs->ctx;
  if (grid_index && n < 0) return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_clear: n must be >= 0");
  if (grid_index) for (int32_t j = 0; j < n; ++j) if (!valid_grid_index(gs, grid_index[j])) return failf(ctx, LSM2D_BAD_ARGUMENT, "gridset_clear: entry %d: grid index outside the set", (int) j);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(uint2) * gs->cells_per_grid;
  if (!grid_index) { HIPCHK(ctx, hipMemsetAsync(gs->d_cells, 0, bytes * (size_t) gs->n_grids, ctx->stream)); return LSM2D_SUCCESS; }
  for (int32_t j = 0; j < n; ++j) HIPCHK(ctx, hipMemsetAsync(gs->d_cells + gs->cells_per_grid * (size_t) grid_index[j], 0, bytes, ctx->stream));
  return LSM2D_SUCCESS;
}

// the two words of a cell from planar host arrays, whatever they mean: the counts upload and the log-odds upload behind their own checks
static int gridset_put(lsm2d_gridset* gs, int32_t grid_index, const uint32_t* hits, const uint32_t* misses);

extern "C" int lsm2d_gridset_upload(lsm2d_gridset* gs, int32_t grid_index, const uint32_t* hits, const uint32_t* misses) {
  if (!gs || !gs->ctx) return fail(gs ? gs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "gridset_upload: null argument (or the set's context is gone)");
  if (gs->logodds) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_upload: a log-odds set (lsm2d_gridset_upload_logodds)");
  if (!valid_grid_index(gs, grid_index)) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_upload: grid index outside the set");
  return gridset_put(gs, grid_index, hits, misses);
}

static int gridset_put(lsm2d_gridset* gs, int32_t grid_index, const uint32_t* hits, const uint32_t* misses) {
  lsm2d_context* ctx = gs->ctx;
  if (!hits && !misses) return LSM2D_SUCCESS;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = gs->cells_per_grid;
  DevBuf<uint32_t> planar;      // the host arrays as they are; k_occ_put interleaves them (a NULL array leaves its counter)
  HIPCHK(ctx, planar.alloc(sizeof(uint32_t) * n * 2));
  uint32_t* const dh = planar; uint32_t* const dm = dh + n;
  if (hits) HIPCHK(ctx, hipMemcpyAsync(dh, hits, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
  if (misses) HIPCHK(ctx, hipMemcpyAsync(dm, misses, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
  OccPutArgs P; P.cells = gs->d_cells + n * (size_t) grid_index; P.hits = hits ? dh : nullptr; P.misses = misses ? dm : nullptr; P.n = (long long) n;
  hipLaunchKernelGGL(k_occ_put, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, P);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, stream_sync(ctx));
  return LSM2D_SUCCESS;
}

static int gridset_get(const lsm2d_gridset* gs, int32_t grid_index, uint32_t* out_hits, uint32_t* out_misses);

extern "C" int lsm2d_gridset_download(const lsm2d_gridset* gs, int32_t grid_index, uint32_t* out_hits, uint32_t* out_misses) {
  if (!gs || !gs->ctx) return fail(gs ? gs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "gridset_download: null argument (or the set's context is gone)");
  if (gs->logodds) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_download: a log-odds set (lsm2d_gridset_download_logodds)");
  if (!valid_grid_index(gs, grid_index)) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_download: grid index outside the set");
  return gridset_get(gs, grid_index, out_hits, out_misses);
}

static int gridset_get(const lsm2d_gridset* gs, int32_t grid_index, uint32_t* out_hits, uint32_t* out_misses) {
  lsm2d_context* ctx = gs->ctx;
  if (!out_hits && !out_misses) return LSM2D_SUCCESS;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = gs->cells_per_grid;
  std::vector<uint2> cells(n);
  HIPCHK(ctx, hipMemcpyAsync(cells.data(), gs->d_cells + n * (size_t) grid_index, sizeof(uint2) * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, stream_sync(ctx));
  for (size_t c = 0; c < n; ++c) { if (out_hits) out_hits[c] = cells[c].x; if (out_misses) out_misses[c] = cells[c].y; }
  return LSM2D_SUCCESS;
}

// ---- what both update calls share: the layout, the geometry, the tables, the tile launch and the finish -----------------------------------------------------
// count_rows: the per-grid count rows that come down, [rays | dropped] or [hit | clear | dropped]; ranges_bytes: the ranges that travel up (0: the cloud
// call, and device-resident ranges)
struct OccupancyLayout {
  size_t u_inputs = 0, u_offset = 0, u_box = 0, u_first = 0, up_bytes = 0;      // the tables that travel up (the same offsets in the staging buffer and in the scratch) ...
  size_t u_ranges = 0, ranges_bytes = 0;                                        // ... and, right behind them, the ranges
  size_t o_down = 0, count_rows = 0, d_row = 0, d_fault = 0, down_bytes = 0;    // the block that travels down, cleared before the chain: count row r at r * d_row, then the fault word
  size_t o_rays = 0, o_stamps = 0, bytes = 0;
  OccupancyLayout(size_t n, size_t n_inputs, size_t n_grids, size_t n_workgroups, size_t count_rows_, size_t ranges_bytes_) {
    u_inputs = 0; u_offset = up256(sizeof(OccInput) * n_inputs); u_box = up256(u_offset + sizeof(int32_t) * (n_inputs + 1));
    u_first = up256(u_box + sizeof(int32_t) * 4 * n_inputs); up_bytes = up256(u_first + sizeof(int32_t) * (n_grids + 1));
    u_ranges = up_bytes; ranges_bytes = ranges_bytes_;
    o_down = up256(u_ranges + ranges_bytes);
    count_rows = count_rows_; d_row = sizeof(int32_t) * n_grids; d_fault = count_rows * d_row; down_bytes = d_fault + 4 * sizeof(int32_t);
    o_rays = up256(o_down + down_bytes);
    o_stamps = up256(o_rays + sizeof(int4) * (n ? n : 1));
    bytes = up256(o_stamps + sizeof(unsigned long long) * n_workgroups);
  }
};

static OccGeo occupancy_geo(const lsm2d_gridset* grids) {
  OccGeo G;
  G.ox = grids->geo.origin_x; G.oy = grids->geo.origin_y; G.inv = 1.0f / grids->geo.resolution; G.w = grids->geo.width; G.h = grids->geo.height; G.n_grids = grids->n_grids;
  G.tiles_x = (G.w + kOccTile - 1) / kOccTile; G.tiles_y = (G.h + kOccTile - 1) / kOccTile;
  return G;
}
static size_t occupancy_workgroups(const OccGeo& G) { return (size_t) G.tiles_x * (size_t) G.tiles_y * (size_t) G.n_grids; }      // (<= LSM2D_OCCUPANCY_MAX_CELLS: a tile holds a cell at least)

// the call's tables into the staging buffer: the inputs grid by grid, list order kept inside a grid (a counting sort); per input its row, its offset in the
// records and an empty box; per grid the range of its inputs.  start(k), count(k): where the caller's input k begins in what the first kernel reads and how
// many records it gives
template <class Start, class Count>
static void occupancy_tables(char* hs, const OccupancyLayout& Y, int32_t n_inputs, int32_t n_grids, const float* pose, const int32_t* grid, Start start, Count count) {
  OccInput* hin = (OccInput*) (hs + Y.u_inputs); int32_t* hoff = (int32_t*) (hs + Y.u_offset); int32_t* hbox = (int32_t*) (hs + Y.u_box);
  int32_t* hfirst = (int32_t*) (hs + Y.u_first);
  for (int32_t g = 0; g <= n_grids; ++g) hfirst[g] = 0;
  for (int32_t k = 0; k < n_inputs; ++k) ++hfirst[(grid ? grid[k] : 0) + 1];
  for (int32_t g = 0; g < n_grids; ++g) hfirst[g + 1] += hfirst[g];
  std::vector<int32_t> cursor(hfirst, hfirst + n_grids), order((size_t) n_inputs);
  for (int32_t k = 0; k < n_inputs; ++k) order[(size_t) cursor[(size_t) (grid ? grid[k] : 0)]++] = k;
  int32_t o = 0;
  for (int32_t j = 0; j < n_inputs; ++j) {
    const int32_t k = order[(size_t) j];
    OccInput& in = hin[j];
    if (pose) { in.T = make_iso(pose + 3 * (size_t) k); in.sx = pose[3 * (size_t) k]; in.sy = pose[3 * (size_t) k + 1]; }
    else { in.T.c = 1.0f; in.T.s = 0.0f; in.T.tx = 0.0f; in.T.ty = 0.0f; in.sx = 0.0f; in.sy = 0.0f; }
    in.start = start(k); in.grid = grid ? grid[k] : 0; in.has_pose = pose != nullptr; in.pad = 0;
    hoff[j] = o; o += count(k);
    hbox[4 * j] = hbox[4 * j + 1] = 0x7fffffff; hbox[4 * j + 2] = hbox[4 * j + 3] = kOccDropped;
  }
  hoff[n_inputs] = o;
}

// the second kernel of either chain over the first one's records: the set's kind and the records' (kinds: k_occ_beams') pick it
static int occupancy_launch_tiles(lsm2d_context* ctx, const lsm2d_gridset* grids, char* ds, const OccupancyLayout& Y, int32_t n_inputs, int n, const OccGeo& G, bool stamps, bool kinds) {
  const size_t n_wg = occupancy_workgroups(G);
  OccTilesArgs T;
  T.rays = (const int4*) (ds + Y.o_rays); T.offset = (const int32_t*) (ds + Y.u_offset); T.box = (const int32_t*) (ds + Y.u_box);
  T.grid_first = (const int32_t*) (ds + Y.u_first); T.n_inputs = n_inputs; T.n = n; T.G = G;
  T.cells = grids->d_cells; T.fault = (int32_t*) (ds + Y.o_down + Y.d_fault); T.stamps = stamps ? (unsigned long long*) (ds + Y.o_stamps) : nullptr;
  if (stamps) HIPCHK(ctx, hipMemsetAsync(ds + Y.o_stamps, 0, sizeof(unsigned long long) * n_wg, ctx->stream));
  const OccLogoddsArgs P = {T, grids->lp.l_hit, grids->lp.l_miss, grids->lp.l_min, grids->lp.l_max};
  const dim3 wgs((unsigned) n_wg), block(kOccBlock);
  if (grids->logodds && kinds) hipLaunchKernelGGL(k_occ_tiles_logodds<true>, wgs, block, 0, ctx->stream, P);
  else if (grids->logodds) hipLaunchKernelGGL(k_occ_tiles_logodds<false>, wgs, block, 0, ctx->stream, P);
  else if (kinds) hipLaunchKernelGGL(k_occ_tiles<true>, wgs, block, 0, ctx->stream, T);
  else hipLaunchKernelGGL(k_occ_tiles<false>, wgs, block, 0, ctx->stream, T);
  HIPCHK(ctx, hipGetLastError());
  return LSM2D_SUCCESS;
}

// diagnostics: how unevenly the tiles' work is spread (a copy and a wait of its own, with kernel timing on only)
static int occupancy_read_stamps(lsm2d_context* ctx, const char* d_stamps, size_t n_wg) {
  std::vector<unsigned long long> t(n_wg);
  HIPCHK(ctx, hipMemcpy(t.data(), d_stamps, sizeof(unsigned long long) * n_wg, hipMemcpyDeviceToHost));
  t.erase(std::remove(t.begin(), t.end(), 0ull), t.end());
  if (!t.empty()) {
    std::sort(t.begin(), t.end());
    ctx->last_occ_wg_median_ns = (long long) t[t.size() / 2] * 10; ctx->last_occ_wg_max_ns = (long long) t.back() * 10;      // (s_memrealtime: 100 MHz)
  }
  return LSM2D_SUCCESS;
}

// the end of both update calls, `who` for the messages: the one copy down and the one wait; the fault word, the counts' signs and their sum against
// `total`; out[r] (or NULL), one per count row; the stamps of the n_wg_stamped workgroups (0: none were written)
static int occupancy_finish(lsm2d_context* ctx, const char* who, const OccupancyLayout& Y, int32_t n_grids, long long total, int32_t* const* out, size_t n_wg_stamped) {
  Lane& L = lane(ctx);
  char* const ds = (char*) L.d_scratch; char* const hs = (char*) L.h_stage;
  HIPCHK(ctx, hipMemcpyAsync(hs, ds + Y.o_down, Y.down_bytes, hipMemcpyDeviceToHost, ctx->stream));      // the one copy down
  HIPCHK(ctx, stream_sync(ctx));      // the one wait of the call
  if (*(const int32_t*) (hs + Y.d_fault)) return failf(ctx, LSM2D_DEVICE_ERROR, "%s: an index left its array on the device (the counters may be partly updated)", who);
  long long sum = 0;
  for (int32_t g = 0; g < n_grids; ++g)
    for (size_t r = 0; r < Y.count_rows; ++r) {
      const int32_t c = ((const int32_t*) (hs + r * Y.d_row))[g];
      if (c < 0) return failf(ctx, LSM2D_DEVICE_ERROR, "%s: the counters are inconsistent", who);
      sum += c;
    }
  if (sum != total) return failf(ctx, LSM2D_DEVICE_ERROR, "%s: the counters are inconsistent", who);
  for (size_t r = 0; r < Y.count_rows; ++r) if (out[r]) memcpy(out[r], hs + r * Y.d_row, Y.d_row);
  ctx->last_occ_wg_median_ns = 0; ctx->last_occ_wg_max_ns = 0;
  if (n_wg_stamped) return occupancy_read_stamps(ctx, ds + Y.o_stamps, n_wg_stamped);
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_occupancy_update(lsm2d_context* ctx, lsm2d_gridset* grids, const lsm2d_cloudset* src, int32_t n_inputs, const int32_t* src_index,
                                      const float* pose, const int32_t* grid, int32_t* out_rays, int32_t* out_dropped) {
  // ---- refusals: nothing is launched or written before the last of them
  if (!ctx || !grids || !src) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update: null argument");
  if (src->ctx != ctx || grids->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update: a set from another (or a destroyed) context");
  if (n_inputs < 1) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update: n_inputs must be >= 1");
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  const int32_t n_grids = grids->n_grids;
  for (int32_t k = 0; k < n_inputs; ++k) {
    if (!valid_cloud_index(src, src_index ? src_index[k] : k)) return failf(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update: input %d: cloud index outside the source set", (int) k);
    if (grid && (grid[k] < 0 || grid[k] >= n_grids)) return failf(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update: input %d: grid outside [0, n_grids)", (int) k);
  }
  // sizes the device alone knows are upper bounds on the host: a sum of bounds within the limit settles it, else the real sizes are fetched -- and they are
  // fetched anyway before the tables are made, which hold exact offsets (as in lsm2d_voxelize)
  long long total = 0;
  for (int32_t k = 0; k < n_inputs; ++k) total += src->h_count[(size_t) (src_index ? src_index[k] : k)];
  if (total > kOccMaxRays && !src->count_pending) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update: more input points than LSM2D_OCCUPANCY_MAX_RAYS");
  { const int rc0 = resolve_count(src); if (rc0) return rc0; }
  total = 0;
  for (int32_t k = 0; k < n_inputs; ++k) total += src->h_count[(size_t) (src_index ? src_index[k] : k)];
  if (total > kOccMaxRays) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update: more input points than LSM2D_OCCUPANCY_MAX_RAYS");
  // ---- from here on the call launches
  HIPCHK(ctx, hipSetDevice(ctx->device));
  { const int rc0 = flush_pending(src); if (rc0) return rc0; }
  HIPCHK(ctx, join_refill_stream(ctx, ctx->stream));
  const OccGeo G = occupancy_geo(grids);
  const bool stamps = ctx->kernel_timing != 0;
  const OccupancyLayout Y((size_t) total, (size_t) n_inputs, (size_t) n_grids, stamps ? occupancy_workgroups(G) : 0, 2, 0);      // [rays | dropped]
  { int rc = ensure_scratch(ctx, Y.bytes); if (rc) return rc; rc = ensure_stage(ctx, std::max(Y.up_bytes, Y.down_bytes)); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const ds = (char*) L.d_scratch; char* const hs = (char*) L.h_stage;
  occupancy_tables(hs, Y, n_inputs, n_grids, pose, grid, [&](int32_t k) { return src->h_start[(size_t) (src_index ? src_index[k] : k)]; },
                   [&](int32_t k) { return src->h_count[(size_t) (src_index ? src_index[k] : k)]; });
  const int n = (int) total;
  // ---- the timing bracket of the whole call
  ctx->have_timing = false;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ds, hs, Y.up_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ds + Y.o_down, 0, Y.down_bytes, ctx->stream));
  if (n > 0) {
    OccRaysArgs R;
    R.xy = src->d_xy; R.inputs = (const OccInput*) (ds + Y.u_inputs); R.offset = (const int32_t*) (ds + Y.u_offset); R.n_inputs = n_inputs; R.n = n; R.G = G;
    R.rays = (int4*) (ds + Y.o_rays); R.box = (int32_t*) (ds + Y.u_box);
    R.n_rays = (int32_t*) (ds + Y.o_down); R.n_dropped = (int32_t*) (ds + Y.o_down + Y.d_row); R.fault = (int32_t*) (ds + Y.o_down + Y.d_fault);
    hipLaunchKernelGGL(k_occ_rays, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, R);
    HIPCHK(ctx, hipGetLastError());
    { const int rc = occupancy_launch_tiles(ctx, grids, ds, Y, n_inputs, n, G, stamps, false); if (rc) return rc; }
  }
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  int32_t* const out[] = {out_rays, out_dropped};
  return occupancy_finish(ctx, "occupancy_update", Y, n_grids, total, out, stamps && n > 0 ? occupancy_workgroups(G) : 0);
}

// the tail of both render calls, R holding what is the kernel's own: the grid's cells rendered into the lane's scratch inside the timing bracket, then the copy and the wait
template <class Args>
static int occupancy_render_grid(lsm2d_context* ctx, const lsm2d_gridset* grids, int32_t grid_index, void (*kernel)(Args), Args& R, int8_t* out) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = grids->cells_per_grid;
  { const int rc = ensure_scratch(ctx, up256(n)); if (rc) return rc; }
  Lane& L = lane(ctx);
  R.cells = grids->d_cells + n * (size_t) grid_index; R.n = (long long) n; R.out = (int8_t*) L.d_scratch;
  ctx->have_timing = false;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  hipLaunchKernelGGL(kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, R);
  HIPCHK(ctx, hipGetLastError());
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  HIPCHK(ctx, hipMemcpyAsync(out, L.d_scratch, n, hipMemcpyDeviceToHost, ctx->stream));      // one byte per cell comes down instead of eight
  HIPCHK(ctx, stream_sync(ctx));
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_occupancy_render(lsm2d_context* ctx, const lsm2d_gridset* grids, int32_t grid_index, const lsm2d_occupancy_render_params* params,
                                      int8_t* out) {
  if (!ctx || !grids || !params || !out) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render: null argument");
  if (grids->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render: a grid set from another (or a destroyed) context");
  if (grids->logodds) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render: a log-odds set (lsm2d_occupancy_render_logodds)");
  if (!valid_grid_index(grids, grid_index)) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render: grid index outside the set");
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  OccRenderArgs R; R.min_visits = params->min_visits;
  return occupancy_render_grid(ctx, grids, grid_index, k_occ_render, R, out);
}

// ---- from raw scans (0.7.13) ------------------------------------------------------------------------------------------------------------------------------
extern "C" int lsm2d_occupancy_update_scans(lsm2d_context* ctx, lsm2d_gridset* grids, const lsm2d_occupancy_scan_params* params, const float* ranges,
                                            int32_t n_scans, const float* pose, const int32_t* grid, int32_t* out_hit_rays, int32_t* out_clear_rays,
                                            int32_t* out_dropped) {
  // ---- refusals: nothing is launched or written before the last of them
  if (!ctx || !grids || !params || !ranges) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: null argument");
  if (grids->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: a grid set from another (or a destroyed) context");
  if (n_scans < 1) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: n_scans must be >= 1");
  lsm2d_preprocessor geometry = {};      // the sensor geometry as the preprocessor states it: the same check, the same direction table, the same cache
  geometry.n_beams = params->n_beams; geometry.angle_min = params->angle_min; geometry.angle_max = params->angle_max;
  geometry.range_min = params->range_min; geometry.range_max = params->range_max; geometry.normal_min_points = 1;
  { const int rc0 = check_preprocessor(ctx, &geometry, "occupancy_update_scans"); if (rc0) return rc0; }
  const int nb = params->n_beams;
  const long long total = (long long) nb * n_scans;
  if (total > kOccMaxRays) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: more beams than LSM2D_OCCUPANCY_MAX_RAYS");
  const float rmin = params->range_min, rmax = params->range_max, trace = params->trace_range;
  if (!std::isfinite(rmin) || !std::isfinite(rmax) || !std::isfinite(trace)) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: range_min, range_max and trace_range must be finite");
  if (rmin < 0.0f || rmin > rmax || !(trace > 0.0f) || trace < rmin || trace > rmax)
    return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: need 0 <= range_min <= trace_range <= range_max and trace_range > 0");
  if (params->clear_no_return != 0 && params->clear_no_return != 1) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: clear_no_return must be 0 or 1");
  const int32_t n_grids = grids->n_grids;
  if (grid) for (int32_t k = 0; k < n_scans; ++k) if (grid[k] < 0 || grid[k] >= n_grids) return failf(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: scan %d: grid outside [0, n_grids)", (int) k);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rdev = -1;
  const PtrKind kind = pointer_kind(ranges, &rdev);
  if (kind == PtrKind::device && rdev != ctx->device) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_update_scans: device-resident ranges must live on the context's device");
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  // ---- from here on the call launches
  const float2* d_dir = nullptr;
  { const int rc0 = beam_dirs_device(ctx, &geometry, &d_dir); if (rc0) return rc0; }      // (made and uploaded once per sensor geometry)
  HIPCHK(ctx, join_refill_stream(ctx, ctx->stream));
  const OccGeo G = occupancy_geo(grids);
  const bool stamps = ctx->kernel_timing != 0;
  const OccupancyLayout Y((size_t) total, (size_t) n_scans, (size_t) n_grids, stamps ? occupancy_workgroups(G) : 0, 3,      // [hit | clear | dropped]
                          kind == PtrKind::device ? 0 : sizeof(float) * (size_t) total);
  const size_t staged_bytes = Y.up_bytes + (kind == PtrKind::pageable ? Y.ranges_bytes : 0);      // pageable ranges ride behind the tables in the one copy up
  { int rc = ensure_scratch(ctx, Y.bytes); if (rc) return rc; rc = ensure_stage(ctx, std::max(staged_bytes, Y.down_bytes)); if (rc) return rc; }
  Lane& L = lane(ctx);
  char* const ds = (char*) L.d_scratch; char* const hs = (char*) L.h_stage;
  occupancy_tables(hs, Y, n_scans, n_grids, pose, grid, [&](int32_t k) { return k * nb; }, [&](int32_t) { return nb; });      // (the ranges stay in the caller's order)
  if (kind == PtrKind::pageable) memcpy(hs + Y.u_ranges, ranges, Y.ranges_bytes);
  const int n = (int) total;
  ++ctx->uploads; ctx->last_h2d_bytes = (long long) Y.ranges_bytes;
  // ---- the timing bracket of the whole call
  ctx->have_timing = false;
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev0, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ds, hs, staged_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (kind == PtrKind::pinned) HIPCHK(ctx, hipMemcpyAsync(ds + Y.u_ranges, ranges, Y.ranges_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ds + Y.o_down, 0, Y.down_bytes, ctx->stream));
  OccBeamsArgs B;
  B.ranges = kind == PtrKind::device ? ranges : (const float*) (ds + Y.u_ranges); B.beam_dir = d_dir; B.inputs = (const OccInput*) (ds + Y.u_inputs);
  B.n_inputs = n_scans; B.n_beams = nb; B.n = n; B.n_ranges = n; B.rmin = rmin; B.rmax = rmax; B.trace = trace; B.clear_no_return = params->clear_no_return; B.G = G;
  B.rays = (int4*) (ds + Y.o_rays); B.box = (int32_t*) (ds + Y.u_box);
  B.n_hit = (int32_t*) (ds + Y.o_down); B.n_clear = (int32_t*) (ds + Y.o_down + Y.d_row); B.n_dropped = (int32_t*) (ds + Y.o_down + 2 * Y.d_row);
  B.fault = (int32_t*) (ds + Y.o_down + Y.d_fault);
  hipLaunchKernelGGL(k_occ_beams, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, ctx->stream, B);
  HIPCHK(ctx, hipGetLastError());
  { const int rc = occupancy_launch_tiles(ctx, grids, ds, Y, n_scans, n, G, stamps, true); if (rc) return rc; }
  if (ctx->kernel_timing) HIPCHK(ctx, hipEventRecord(L.ev1, ctx->stream));
  note_timed(ctx, ctx->kernel_timing);
  int32_t* const out[] = {out_hit_rays, out_clear_rays, out_dropped};
  return occupancy_finish(ctx, "occupancy_update_scans", Y, n_grids, total, out, stamps ? occupancy_workgroups(G) : 0);
}

// ---- log-odds grid sets (0.7.14; PARITY.md section 3, item 17e) -------------------------------------------------------------------------------------------
static const char* logodds_params_fault(const lsm2d_logodds_params* p) {
  if (p->l_hit < 1 || p->l_hit > (1 << 20)) return "l_hit must lie in 1 .. 2^20";
  if (p->l_miss > -1 || p->l_miss < -(1 << 20)) return "l_miss must lie in -2^20 .. -1";
  if (p->l_min > 0 || p->l_min < -(1 << 30)) return "l_min must lie in -2^30 .. 0";
  if (p->l_max < 0 || p->l_max > (1 << 30)) return "l_max must lie in 0 .. 2^30";
  return nullptr;
}

extern "C" int lsm2d_gridset_create_logodds(lsm2d_context* ctx, const lsm2d_grid_geometry* geo, int32_t n_grids, const lsm2d_logodds_params* params,
                                            lsm2d_gridset** out) {
  if (out) *out = nullptr;
  if (!ctx || !geo || !params || !out) return fail(ctx, LSM2D_BAD_ARGUMENT, "gridset_create_logodds: null argument");
  if (const char* why = logodds_params_fault(params)) return failf(ctx, LSM2D_BAD_ARGUMENT, "gridset_create_logodds: %s", why);
  const int rc = lsm2d_gridset_create(ctx, geo, n_grids, out);      // (all cells zero: value 0, observed 0 = unknown)
  if (rc) return rc;
  (*out)->logodds = true; (*out)->lp = *params;
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_gridset_set_logodds(lsm2d_gridset* gs, const lsm2d_logodds_params* params) {
  if (!gs || !gs->ctx || !params) return fail(gs ? gs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "gridset_set_logodds: null argument (or the set's context is gone)");
  if (!gs->logodds) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_set_logodds: a counts set");
  if (const char* why = logodds_params_fault(params)) return failf(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_set_logodds: %s", why);
  gs->lp = *params;      // host-side only: an update queued earlier took its copy at its launch
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_gridset_upload_logodds(lsm2d_gridset* gs, int32_t grid_index, const int32_t* value, const uint32_t* observed) {
  if (!gs || !gs->ctx) return fail(gs ? gs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "gridset_upload_logodds: null argument (or the set's context is gone)");
  if (!gs->logodds) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_upload_logodds: a counts set (lsm2d_gridset_upload)");
  if (!valid_grid_index(gs, grid_index)) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_upload_logodds: grid index outside the set");
  return gridset_put(gs, grid_index, (const uint32_t*) value, observed);      // (k_occ_put moves words: a value outside the clamps is legal, item 17e)
}

extern "C" int lsm2d_gridset_download_logodds(const lsm2d_gridset* gs, int32_t grid_index, int32_t* out_value, uint32_t* out_observed) {
  if (!gs || !gs->ctx) return fail(gs ? gs->ctx : nullptr, LSM2D_BAD_ARGUMENT, "gridset_download_logodds: null argument (or the set's context is gone)");
  if (!gs->logodds) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_download_logodds: a counts set (lsm2d_gridset_download)");
  if (!valid_grid_index(gs, grid_index)) return fail(gs->ctx, LSM2D_BAD_ARGUMENT, "gridset_download_logodds: grid index outside the set");
  return gridset_get(gs, grid_index, (uint32_t*) out_value, out_observed);
}

extern "C" int lsm2d_occupancy_decay(lsm2d_context* ctx, lsm2d_gridset* gs, int32_t n, const int32_t* grid_index, int32_t amount) {
  if (!ctx || !gs) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_decay: null argument");
  if (gs->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_decay: a grid set from another (or a destroyed) context");
  if (!gs->logodds) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_decay: a counts set");
  if (amount < 0) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_decay: amount must be >= 0");
  if (grid_index && n < 0) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_decay: n must be >= 0");
  if (grid_index) for (int32_t j = 0; j < n; ++j) if (!valid_grid_index(gs, grid_index[j])) return failf(ctx, LSM2D_BAD_ARGUMENT, "occupancy_decay: entry %d: grid index outside the set", (int) j);
  if (amount == 0) return LSM2D_SUCCESS;      // (nothing moves)
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t per = gs->cells_per_grid;
  const int32_t launches = grid_index ? n : 1;      // queued, no wait: every grid in one launch, or a launch per listed grid (a grid listed twice decays twice)
  for (int32_t j = 0; j < launches; ++j) {
    OccDecayArgs D; D.cells = gs->d_cells + (grid_index ? per * (size_t) grid_index[j] : 0); D.n = (long long) (grid_index ? per : per * (size_t) gs->n_grids); D.amount = amount;
    hipLaunchKernelGGL(k_occ_decay, dim3((unsigned) ((D.n + 255) / 256)), dim3(256), 0, ctx->stream, D);
    HIPCHK(ctx, hipGetLastError());
  }
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_logodds_render_table(float unit, int32_t* out_threshold) {
  if (!out_threshold || !(unit > 0.0f) || !std::isfinite(unit)) return LSM2D_BAD_ARGUMENT;
  for (int j = 1; j <= 100; ++j) {      // the smallest integer value whose probability rounds to j percent or more: p >= (j - 0.5) / 100
    const double t = std::ceil(std::log(((double) j - 0.5) / (100.5 - (double) j)) / (double) unit);
    out_threshold[j - 1] = t < -2147483648.0 ? INT32_MIN : t > 2147483647.0 ? INT32_MAX : (int32_t) t;
  }
  return LSM2D_SUCCESS;
}

extern "C" int lsm2d_occupancy_render_logodds(lsm2d_context* ctx, const lsm2d_gridset* grids, int32_t grid_index, const lsm2d_logodds_render_params* params,
                                              int8_t* out) {
  if (!ctx || !grids || !params || !out) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render_logodds: null argument");
  if (grids->ctx != ctx) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render_logodds: a grid set from another (or a destroyed) context");
  if (!grids->logodds) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render_logodds: a counts set (lsm2d_occupancy_render)");
  if (!valid_grid_index(grids, grid_index)) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render_logodds: grid index outside the set");
  OccRenderLogoddsArgs R;
  if (lsm2d_logodds_render_table(params->unit, R.threshold)) return fail(ctx, LSM2D_BAD_ARGUMENT, "occupancy_render_logodds: unit must be finite and > 0");
  if (ctx->inflight >= 2 || lane(ctx).busy) return fail(ctx, LSM2D_BAD_ARGUMENT, kBothLanesBusy);
  R.min_scans = params->min_scans;
  return occupancy_render_grid(ctx, grids, grid_index, k_occ_render_logodds, R, out);      // (the 100 thresholds ride in the arguments)
}
