// lsm2d_capi_sweep.inc -- the loop-closure / relocalisation sweep over several devices in one process (MultiLoopDetectorBruteForce2D's candidate loop, configurations/stage_segway_double_config_MULTI.json:964-986).
// Part of lsm2d_capi.hip (included there); not a translation unit of its own.
// ---- loop-closure / relocalisation sweep over several devices in ONE process (no Python, no MPI) ------------------------------
// What MultiLoopDetectorBruteForce2D's candidate loop (MULTI.json:964-986) becomes on a node of MI355Xs: every device gets its own
// context, a replica of the submap (device-to-device copies from the first device) and of the distinct candidate scans; the
// candidates are block-sharded, one host thread drives each device, results land in candidate order.  No collective on the data
// path; several entries of device_ids may name the same device (rehearsal on a one-GPU box).
struct lsm2d_sweep {
  std::vector<lsm2d_context*> ctx;
  std::vector<lsm2d_cloudset*> map, scans;
  std::string last_error;
  int peer_copy = 0;                                                  // 0 automatic, 1 replicas always filled from the host buffer
  long long by_peer = 0, through_host = 0, same_device = 0;           // how the replicas of the last set_map / set_scans were filled
};
static int sweep_fail(lsm2d_sweep* sw, int code, const std::string& msg) { if (sw) sw->last_error = msg; g_last_error = msg; return code; }
static void sweep_drop(std::vector<lsm2d_cloudset*>& v) { for (auto* s : v) lsm2d_cloudset_destroy(s); v.clear(); }

extern "C" int lsm2d_sweep_create(const int32_t* device_ids, int32_t n_devices, lsm2d_sweep** out) {
  if (!device_ids || n_devices < 1 || n_devices > 64 || !out) return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_create: bad argument");
  lsm2d_sweep* sw = new (std::nothrow) lsm2d_sweep;
  if (!sw) return fail(nullptr, LSM2D_OUT_OF_MEMORY, "sweep_create: out of memory");
  for (int r = 0; r < n_devices; ++r) {
    lsm2d_context* c = nullptr;
    const int rc = lsm2d_create(device_ids[r], nullptr, &c);
    if (rc) { for (auto* k : sw->ctx) lsm2d_destroy(k); delete sw; return rc; }
    sw->ctx.push_back(c);
  }
  *out = sw;
  return LSM2D_SUCCESS;
}
extern "C" void lsm2d_sweep_destroy(lsm2d_sweep* sw) {
  if (!sw) return;
  sweep_drop(sw->map); sweep_drop(sw->scans);
  for (auto* c : sw->ctx) lsm2d_destroy(c);
  delete sw;
}
extern "C" int32_t lsm2d_sweep_num_devices(const lsm2d_sweep* sw) { return sw ? (int32_t) sw->ctx.size() : 0; }
extern "C" int lsm2d_sweep_set_option(lsm2d_sweep* sw, const char* key, int64_t value) {
  if (!sw || !key) return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_set_option: bad argument");
  if (!strcmp(key, "peer_copy")) { if (value < 0 || value > 1) return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "peer_copy must be 0 or 1"); sw->peer_copy = (int) value; return LSM2D_SUCCESS; }
  return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "sweep_set_option: unknown option");
}
extern "C" int lsm2d_sweep_get_option(const lsm2d_sweep* sw, const char* key, int64_t* out) {
  if (!sw || !key || !out) return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_get_option: bad argument");
  if (!strcmp(key, "peer_copy")) { *out = sw->peer_copy; return LSM2D_SUCCESS; }
  if (!strcmp(key, "replicas_by_peer_copy")) { *out = sw->by_peer; return LSM2D_SUCCESS; }
  if (!strcmp(key, "replicas_through_host")) { *out = sw->through_host; return LSM2D_SUCCESS; }
  if (!strcmp(key, "replicas_same_device")) { *out = sw->same_device; return LSM2D_SUCCESS; }
  return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_get_option: unknown option");
}
extern "C" const char* lsm2d_sweep_last_error(const lsm2d_sweep* sw) { return sw ? sw->last_error.c_str() : g_last_error.c_str(); }

// one host cloud set replicated on every device of the sweep: host -> first device once, then device -> device
static int sweep_replicate(lsm2d_sweep* sw, const float* pts, const int32_t* offsets, int32_t n_clouds, int64_t total, std::vector<lsm2d_cloudset*>* out) {
  sweep_drop(*out);
  if (!pts || total < 0 || n_clouds < 1) return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "sweep: bad cloud");
  const size_t bytes = sizeof(float) * 4 * (size_t) (total > 0 ? total : 1);
  lsm2d_context* c0 = sw->ctx[0];
  void* d0 = nullptr;
  if (hipSetDevice(c0->device) != hipSuccess || hipMalloc(&d0, bytes) != hipSuccess) return sweep_fail(sw, LSM2D_OUT_OF_MEMORY, "sweep: staging allocation failed");
  if (total > 0 && hipMemcpy(d0, pts, sizeof(float) * 4 * (size_t) total, hipMemcpyHostToDevice) != hipSuccess) { (void) hipFree(d0); return sweep_fail(sw, LSM2D_DEVICE_ERROR, "sweep: upload failed"); }
  int rc = LSM2D_SUCCESS;
  sw->by_peer = sw->through_host = sw->same_device = 0;
  for (size_t r = 0; r < sw->ctx.size() && rc == LSM2D_SUCCESS; ++r) {
    lsm2d_context* c = sw->ctx[r];
    void* dr = d0;
    if (r > 0) {      // a replica of its own: over the fabric (xGMI between the GPUs of a node) where the two devices reach each other, else from the host buffer
      if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&dr, bytes) != hipSuccess) { rc = sweep_fail(sw, LSM2D_OUT_OF_MEMORY, "sweep: replica allocation failed"); break; }
      const size_t nbytes = sizeof(float) * 4 * (size_t) total;
      bool done = total == 0;
      if (!done && sw->peer_copy == 0) {
        if (c->device == c0->device) {                        // a rehearsal of several shards on one device: a plain device-to-device copy
          done = hipMemcpy(dr, d0, nbytes, hipMemcpyDeviceToDevice) == hipSuccess;
          if (done) ++sw->same_device;
        } else {
          int can = 0;
          if (hipDeviceCanAccessPeer(&can, c->device, c0->device) == hipSuccess && can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(c0->device, 0);      // current device: c->device; once per pair
            if (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled) done = hipMemcpyPeer(dr, c->device, d0, c0->device, nbytes) == hipSuccess;
            if (done) ++sw->by_peer;
          }
        }
        (void) hipGetLastError();                             // a refused peer path is not an error: the host path follows
      }
      if (!done) {                                            // no peer access (or switched off, or the peer copy failed): the caller's host buffer is the source
        if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(dr, pts, nbytes, hipMemcpyHostToDevice) != hipSuccess) { (void) hipFree(dr); rc = sweep_fail(sw, LSM2D_DEVICE_ERROR, "sweep: replica upload failed"); break; }
        ++sw->through_host;
      }
    }
    lsm2d_cloudset* set = nullptr;
    rc = lsm2d_cloudset_create_from_device(c, dr, offsets, n_clouds, total, &set);
    if (rc == LSM2D_SUCCESS) { rc = lsm2d_synchronize(c); out->push_back(set); }      // the split of the AoS staging buffer has run before it is freed
    if (r > 0) { (void) hipSetDevice(c->device); (void) hipFree(dr); }
  }
  (void) hipSetDevice(c0->device); (void) hipFree(d0);
  if (rc != LSM2D_SUCCESS) { sweep_drop(*out); return rc; }
  return LSM2D_SUCCESS;
}
extern "C" int lsm2d_sweep_set_map(lsm2d_sweep* sw, const float* map_xynn, int64_t n_points) {
  if (!sw) return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_set_map: null sweep");
  return sweep_replicate(sw, map_xynn, nullptr, 1, n_points, &sw->map);
}
extern "C" int lsm2d_sweep_set_scans(lsm2d_sweep* sw, const float* scans_xynn, const int32_t* offsets, int32_t n_scans) {
  if (!sw || !offsets || n_scans < 1) return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_set_scans: bad argument");
  return sweep_replicate(sw, scans_xynn, offsets, n_scans, offsets[n_scans], &sw->scans);
}

extern "C" int lsm2d_sweep_align(lsm2d_sweep* sw, const lsm2d_aligner_params* ap, const lsm2d_slice_params* slice, int32_t n_candidates,
                                 const int32_t* scan_index, const float* init_pose, float* out_pose, float* out_H, int32_t* out_status,
                                 int32_t* out_iterations, lsm2d_iteration_stats* out_last_stats) {
  if (!sw || !ap || !slice || n_candidates < 0 || (n_candidates > 0 && (!init_pose || !out_pose || !out_status)))
    return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_align: bad argument");
  if (sw->map.size() != sw->ctx.size() || sw->scans.size() != sw->ctx.size()) return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "sweep_align: set_map / set_scans first");
  if (n_candidates == 0) return LSM2D_SUCCESS;      // an empty candidate list is a no-op, as an empty batch is for lsm2d_align_batch
  const int G = (int) sw->ctx.size();
  const int n_scans = lsm2d_cloudset_num_clouds(sw->scans[0]);
  if (!scan_index && n_scans != n_candidates && n_scans != 1) return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "sweep_align: scan_index needed unless there is one scan per candidate");
  // no exception crosses the C ABI: allocation failures inside a worker become that device's status, a failure to start a thread joins
  // the ones already running and returns LSM2D_OUT_OF_MEMORY
  std::vector<int> rcs; std::vector<std::thread> workers;
  try { rcs.assign((size_t) G, LSM2D_SUCCESS); workers.reserve((size_t) G); } catch (...) { return sweep_fail(sw, LSM2D_OUT_OF_MEMORY, "sweep_align: out of memory"); }
  bool spawn_failed = false;
  for (int r = 0; r < G && !spawn_failed; ++r) {
    const long long lo = (long long) n_candidates * r / G, hi = (long long) n_candidates * (r + 1) / G;
    if (hi <= lo) continue;
    try {
    workers.emplace_back([=, &rcs]() {
      try {
      const int n = (int) (hi - lo);
      // without an index array candidate i uses scan i: the shard needs an explicit index then (its scans start at lo)
      std::vector<int32_t> own_index;
      const int32_t* idx = scan_index ? scan_index + lo : nullptr;
      if (!idx && n_scans != 1) { own_index.resize((size_t) n); for (int i = 0; i < n; ++i) own_index[(size_t) i] = (int32_t) (lo + i); idx = own_index.data(); }
      const lsm2d_cloudset* fx = sw->scans[(size_t) r]; const lsm2d_cloudset* mv = sw->map[(size_t) r];
      lsm2d_batch b; memset(&b, 0, sizeof b);
      b.n_alignments = n; b.n_slices = 1; b.slices = slice; b.fixed = &fx; b.moving = &mv; b.fixed_index = idx; b.init_pose = init_pose + 3 * lo;
      std::vector<lsm2d_iteration_stats> stats;
      if (out_last_stats) stats.resize((size_t) n * (size_t) lsm2d_stats_capacity(ap));
      std::vector<int32_t> its((size_t) n);
      const int rc = lsm2d_align_batch(sw->ctx[(size_t) r], ap, &b, out_pose + 3 * lo, out_H ? out_H + 9 * lo : nullptr, out_status + lo, its.data(),
                                       out_last_stats ? stats.data() : nullptr);
      rcs[(size_t) r] = rc;
      if (rc != LSM2D_SUCCESS) return;
      if (out_iterations) memcpy(out_iterations + lo, its.data(), sizeof(int32_t) * (size_t) n);
      if (out_last_stats)
        for (int i = 0; i < n; ++i) {
          lsm2d_iteration_stats z; memset(&z, 0, sizeof z);
          out_last_stats[lo + i] = its[(size_t) i] > 0 ? stats[(size_t) i * (size_t) lsm2d_stats_capacity(ap) + (size_t) (its[(size_t) i] - 1)] : z;
        }
      } catch (const std::bad_alloc&) { rcs[(size_t) r] = LSM2D_OUT_OF_MEMORY; } catch (...) { rcs[(size_t) r] = LSM2D_DEVICE_ERROR; }
    });
    } catch (...) { spawn_failed = true; }      // std::system_error from the thread constructor, bad_alloc from the vector
  }
  for (auto& w : workers) w.join();
  if (spawn_failed) return sweep_fail(sw, LSM2D_OUT_OF_MEMORY, "sweep_align: could not start a worker thread");
  for (int r = 0; r < G; ++r) if (rcs[(size_t) r] != LSM2D_SUCCESS) return sweep_fail(sw, rcs[(size_t) r], std::string("sweep_align: device ") + std::to_string(r) + ": " + lsm2d_last_error(sw->ctx[(size_t) r]));
  return LSM2D_SUCCESS;
}

// ---- ... with the verdict made on the devices: every shard runs lsm2d_align_select with the caller's k on its block of candidates, and the host merges the
// <= G x k rows by the selection's own key over GLOBAL candidate indices -- n_inliers descending, chi_inliers ascending on its bit pattern, index ascending.
// A candidate among the best k of all is among the best k of its shard, and the order is total: the result is lsm2d_align_select's on one device, whatever G is.
extern "C" int lsm2d_sweep_align_select(lsm2d_sweep* sw, const lsm2d_aligner_params* ap, const lsm2d_slice_params* slice, int32_t n_candidates,
                                        const int32_t* scan_index, const float* init_pose, const lsm2d_select_params* select, int32_t k,
                                        int32_t* out_index, float* out_pose, float* out_H, int32_t* out_iterations, lsm2d_iteration_stats* out_last_stats,
                                        int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  if (!sw || !ap || !slice || !select || !out_index || !out_pose || !out_n_selected || !out_n_accepted || n_candidates < 0 || (n_candidates > 0 && !init_pose))
    return fail(nullptr, LSM2D_BAD_ARGUMENT, "sweep_align_select: bad argument");
  if (k < 1 || k > LSM2D_SELECT_MAX_K) return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "sweep_align_select: k outside [1, LSM2D_SELECT_MAX_K]");
  if (sw->map.size() != sw->ctx.size() || sw->scans.size() != sw->ctx.size()) return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "sweep_align_select: set_map / set_scans first");
  if (n_candidates == 0) { *out_n_selected = 0; *out_n_accepted = 0; if (out_n_success) *out_n_success = 0; return LSM2D_SUCCESS; }
  const int G = (int) sw->ctx.size();
  const int n_scans = lsm2d_cloudset_num_clouds(sw->scans[0]);
  if (!scan_index && n_scans != n_candidates && n_scans != 1) return sweep_fail(sw, LSM2D_BAD_ARGUMENT, "sweep_align_select: scan_index needed unless there is one scan per candidate");
  struct Shard { std::vector<int32_t> index, its; std::vector<float> pose, H; std::vector<lsm2d_iteration_stats> stats; int32_t n_sel = 0, n_acc = 0, n_success = 0; };
  std::vector<int> rcs; std::vector<std::thread> workers; std::vector<Shard> shards;
  try {
    rcs.assign((size_t) G, LSM2D_SUCCESS); workers.reserve((size_t) G); shards.resize((size_t) G);
    for (Shard& s : shards) { s.index.resize((size_t) k); s.its.resize((size_t) k); s.pose.resize(3 * (size_t) k); s.H.resize(9 * (size_t) k); s.stats.resize((size_t) k); }
  } catch (...) { return sweep_fail(sw, LSM2D_OUT_OF_MEMORY, "sweep_align_select: out of memory"); }
  bool spawn_failed = false;
  for (int r = 0; r < G && !spawn_failed; ++r) {
    const long long lo = (long long) n_candidates * r / G, hi = (long long) n_candidates * (r + 1) / G;
    if (hi <= lo) continue;
    try {
    workers.emplace_back([=, &rcs, &shards]() {
      try {
      const int n = (int) (hi - lo);
      Shard& s = shards[(size_t) r];
      std::vector<int32_t> own_index;      // (without an index array candidate i uses scan i: the shard's scans start at lo)
      const int32_t* idx = scan_index ? scan_index + lo : nullptr;
      if (!idx && n_scans != 1) { own_index.resize((size_t) n); for (int i = 0; i < n; ++i) own_index[(size_t) i] = (int32_t) (lo + i); idx = own_index.data(); }
      const lsm2d_cloudset* fx = sw->scans[(size_t) r]; const lsm2d_cloudset* mv = sw->map[(size_t) r];
      lsm2d_batch b; memset(&b, 0, sizeof b);
      b.n_alignments = n; b.n_slices = 1; b.slices = slice; b.fixed = &fx; b.moving = &mv; b.fixed_index = idx; b.init_pose = init_pose + 3 * lo;
      rcs[(size_t) r] = lsm2d_align_select(sw->ctx[(size_t) r], ap, &b, select, k, s.index.data(), s.pose.data(), s.H.data(), s.its.data(), s.stats.data(),
                                           &s.n_sel, &s.n_acc, &s.n_success);
      for (int32_t j = 0; j < s.n_sel; ++j) s.index[(size_t) j] += (int32_t) lo;      // global candidate indices from here on
      } catch (const std::bad_alloc&) { rcs[(size_t) r] = LSM2D_OUT_OF_MEMORY; } catch (...) { rcs[(size_t) r] = LSM2D_DEVICE_ERROR; }
    });
    } catch (...) { spawn_failed = true; }
  }
  for (auto& w : workers) w.join();
  if (spawn_failed) return sweep_fail(sw, LSM2D_OUT_OF_MEMORY, "sweep_align_select: could not start a worker thread");
  for (int r = 0; r < G; ++r) if (rcs[(size_t) r] != LSM2D_SUCCESS) return sweep_fail(sw, rcs[(size_t) r], std::string("sweep_align_select: device ") + std::to_string(r) + ": " + lsm2d_last_error(sw->ctx[(size_t) r]));
  struct Entry { uint64_t key; int32_t index; int shard, row; };
  std::vector<Entry> all;
  long long n_acc = 0, n_success = 0;
  try {
    for (int r = 0; r < G; ++r) {
      const Shard& s = shards[(size_t) r];
      n_acc += s.n_acc; n_success += s.n_success;
      for (int32_t j = 0; j < s.n_sel; ++j) {
        uint32_t chi_bits; memcpy(&chi_bits, &s.stats[(size_t) j].chi_inliers, sizeof chi_bits);
        all.push_back({((uint64_t) (uint32_t) (0x7fffffff - s.stats[(size_t) j].n_inliers) << 32) | (uint64_t) chi_bits, s.index[(size_t) j], r, (int) j});
      }
    }
  } catch (...) { return sweep_fail(sw, LSM2D_OUT_OF_MEMORY, "sweep_align_select: out of memory"); }
  std::sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.key < b.key || (a.key == b.key && a.index < b.index); });
  const int32_t n_sel = (int32_t) std::min<long long>((long long) k, n_acc);      // (every shard handed back min(k, its accepted): all.size() >= n_sel)
  for (int32_t j = 0; j < n_sel && (size_t) j < all.size(); ++j) {
    const Entry& e = all[(size_t) j]; const Shard& s = shards[(size_t) e.shard];
    out_index[j] = e.index;
    memcpy(out_pose + 3 * (size_t) j, s.pose.data() + 3 * (size_t) e.row, sizeof(float) * 3);
    if (out_H) memcpy(out_H + 9 * (size_t) j, s.H.data() + 9 * (size_t) e.row, sizeof(float) * 9);
    if (out_iterations) out_iterations[j] = s.its[(size_t) e.row];
    if (out_last_stats) out_last_stats[j] = s.stats[(size_t) e.row];
  }
  *out_n_selected = n_sel; *out_n_accepted = (int32_t) n_acc;
  if (out_n_success) *out_n_success = (int32_t) n_success;
  return LSM2D_SUCCESS;
}
