// lsm2d_standin.cpp -- stands in for liblsm2d_hip.so under host/lsm2d.hpp, without a device: every lsm2d_* symbol the header references, each writing
// one line per call to stdout -- the symbol and every argument -- and answering success with only what the header reads back.  Plain C++, no HIP.
//   scalars by value; NULL as "NULL"; a context / set / pending / sweep handle by its order of creation ("h3"); a struct passed by pointer and an input array
//   by their bytes ("x:<hex>", the length from the call's own counts); a lsm2d_batch by its counts and what each non-null member points to; an output
//   pointer as "out".  The destroy calls are not in the record (when an object dies is the program's affair) but are counted: a handle that arrives in a
//   call after its destroy, or is destroyed twice, ends the run with a message and exit status 3; standin_leak_check() reports what was made and never
//   destroyed.  tests/test_cpp_mirror_calls_cpu.py builds this file with tests/cpp/mirror_trace_driver.cpp.
#include <lsm2d.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Handle { int id; const char* made_by; bool alive, reported; int32_t n_clouds; int64_t n_points; };
std::vector<Handle*> g_handles;
std::string g_fail_symbol; int g_fail_in = 0;
std::vector<int32_t> g_selected;

[[noreturn]] void die(const std::string& what) { fflush(stdout); fprintf(stderr, "lsm2d_standin: %s\n", what.c_str()); exit(3); }

Handle* lookup(const void* p, const char* sym) {
  for (Handle* h : g_handles) if (h == p) return h;
  die(std::string(sym) + ": a pointer that is no handle of this library");
}
std::string H(const void* p, const char* sym) {
  if (!p) return "NULL";
  Handle* h = lookup(p, sym);
  if (!h->alive) die(std::string(sym) + ": handle h" + std::to_string(h->id) + " used after its destroy");
  return "h" + std::to_string(h->id);
}
template <class T> T* fresh(const char* sym, int32_t n_clouds = 0, int64_t n_points = 0) {
  g_handles.push_back(new Handle{(int) g_handles.size(), sym, true, false, n_clouds, n_points});
  return reinterpret_cast<T*>(g_handles.back());
}
void destroy(void* p, const char* sym) {
  if (!p) return;
  Handle* h = lookup(p, sym);
  if (!h->alive) die(std::string(sym) + ": handle h" + std::to_string(h->id) + " destroyed twice");
  h->alive = false;
}
const Handle* peek(const void* p) { return reinterpret_cast<const Handle*>(p); }

std::string X(const void* p, size_t bytes) {            // input bytes
  if (!p) return "NULL";
  static const char* d = "0123456789abcdef";
  std::string s = "x:";
  for (size_t i = 0; i < bytes; ++i) { const unsigned char c = ((const unsigned char*) p)[i]; s += d[c >> 4]; s += d[c & 15]; }
  return s;
}
template <class T> std::string S(const T* p) { return X(p, sizeof(T)); }
std::string O(const void* p) { return p ? "out" : "NULL"; }
std::string I(long long v) { return std::to_string(v); }
std::string F(float v) { char b[40]; snprintf(b, sizeof b, "%.9g", (double) v); return b; }
std::string T(const char* s) { return s ? std::string("\"") + s + "\"" : "NULL"; }
std::string HS(const lsm2d_cloudset* const* p, size_t n, const char* sym) {
  if (!p) return "NULL";
  std::string s = "[";
  for (size_t i = 0; i < n; ++i) s += (i ? "," : "") + H(p[i], sym);
  return s + "]";
}
std::string B(const lsm2d_batch* b, const char* sym) {
  if (!b) return "NULL";
  const size_t n = (size_t) b->n_alignments, ns = (size_t) b->n_slices;
  return "{n_alignments=" + I(b->n_alignments) + " n_slices=" + I(b->n_slices) + " slices=" + X(b->slices, ns * sizeof(lsm2d_slice_params)) +
         " fixed=" + HS(b->fixed, ns, sym) + " moving=" + HS(b->moving, ns, sym) + " fixed_index=" + X(b->fixed_index, 4 * ns * n) +
         " moving_index=" + X(b->moving_index, 4 * ns * n) + " init_pose=" + X(b->init_pose, 12 * n) + " prior=" + X(b->prior, n * sizeof(lsm2d_prior)) + "}";
}

// one line of the record; the status to answer with: LSM2D_DEVICE_ERROR where the driver asked for it
int rec(const char* sym, std::initializer_list<std::string> args) {
  std::string line = sym;
  for (const auto& a : args) line += " " + a;
  const bool fail = g_fail_symbol == sym && g_fail_in > 0 && --g_fail_in == 0;
  if (fail) { line += " -> LSM2D_DEVICE_ERROR"; g_fail_symbol.clear(); }
  puts(line.c_str());
  return fail ? LSM2D_DEVICE_ERROR : LSM2D_SUCCESS;
}

// rows any reader can tell apart: row i holds H = 100 i + 0..8, b = 100 i + 50 + 0..2, n_correspondences 10 + i, n_inliers 5 + i, active i + 1
void rows(size_t m, float* Hm, float* b, lsm2d_iteration_stats* st, int32_t* active) {
  for (size_t i = 0; i < m; ++i) {
    for (size_t k = 0; k < 9; ++k) Hm[9 * i + k] = (float) (100 * i + k);
    for (size_t k = 0; k < 3; ++k) b[3 * i + k] = (float) (100 * i + 50 + k);
    st[i] = lsm2d_iteration_stats{(int32_t) (10 + i), (int32_t) (5 + i), 5, 0.25f * (float) (i + 1), 1.5f, (uint32_t) i, 7u};
    if (active) active[i] = (int32_t) i + 1;
  }
}
// the scripted answer of a selecting call: the indices standin_select() gave, at most k of them
int32_t select(int32_t k, int32_t* out_index, int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success = nullptr) {
  const int32_t m = std::min<int32_t>((int32_t) g_selected.size(), k > 0 ? k : 0);
  for (int32_t j = 0; j < m; ++j) out_index[j] = g_selected[(size_t) j];
  *out_n_selected = m; *out_n_accepted = (int32_t) g_selected.size();
  if (out_n_success) *out_n_success = (int32_t) g_selected.size() + 1;
  g_selected.clear();
  return m;
}
// an aligner's outputs: zero poses, an information matrix of 1..9, status success, 2 iterations, statistics row r of item i with n_inliers 5 + r
void aligned(size_t n, float* pose, float* Hm, int32_t* status, int32_t* iterations, lsm2d_iteration_stats* st, size_t cap) {
  for (size_t i = 0; i < n; ++i) {
    if (pose) for (size_t k = 0; k < 3; ++k) pose[3 * i + k] = 0.0f;
    if (Hm) for (size_t k = 0; k < 9; ++k) Hm[9 * i + k] = (float) (k + 1);
    if (status) status[i] = LSM2D_SUCCESS;
    if (iterations) iterations[i] = 2;
    if (st) for (size_t r = 0; r < cap; ++r) st[i * cap + r] = lsm2d_iteration_stats{(int32_t) (10 + i), (int32_t) (5 + r), 5, 0.25f, 1.5f, (uint32_t) i, (uint32_t) r};
  }
}
constexpr int32_t STATS_CAPACITY = 4;

}  // namespace

extern "C" {

// what the driver tells the stand-in: fail the kth call of `symbol` from now; the indices the next selecting call hands out; a line of its own for the record;
// report every handle made and not destroyed (each once), returning how many
void standin_fail_at(const char* symbol, int kth) { g_fail_symbol = symbol; g_fail_in = kth; }
void standin_select(int32_t n, const int32_t* index) { g_selected.assign(index, index + n); }
void standin_note(const char* text) { puts(text); }
int standin_leak_check(const char* where) {
  int leaks = 0;
  fflush(stdout);
  for (Handle* h : g_handles)
    if (h->alive && !h->reported) { h->reported = true; ++leaks; fprintf(stderr, "lsm2d_standin: leak at %s: h%d (%s) was never destroyed\n", where, h->id, h->made_by); }
  return leaks;
}

// (the three text lookups are not in the record: an error message calls two of them in one expression, in an order the compiler chooses)
const char* lsm2d_status_string(int status) { return status == LSM2D_DEVICE_ERROR ? "device error" : "status"; }
const char* lsm2d_last_error(const lsm2d_context* ctx) { H(ctx, "lsm2d_last_error"); return "(stand-in)"; }
int32_t lsm2d_stats_capacity(const lsm2d_aligner_params* aligner) { rec("lsm2d_stats_capacity", {S(aligner)}); return STATS_CAPACITY; }

int lsm2d_create(int device_id, void* hip_stream, lsm2d_context** out_ctx) {
  const int rc = rec("lsm2d_create", {I(device_id), O(hip_stream), O(out_ctx)});
  if (!rc) *out_ctx = fresh<lsm2d_context>("lsm2d_create");
  return rc;
}
void lsm2d_destroy(lsm2d_context* ctx) { destroy(ctx, "lsm2d_destroy"); }
int lsm2d_synchronize(lsm2d_context* ctx) { return rec("lsm2d_synchronize", {H(ctx, "lsm2d_synchronize")}); }
int lsm2d_set_option(lsm2d_context* ctx, const char* key, int64_t value) { return rec("lsm2d_set_option", {H(ctx, "lsm2d_set_option"), T(key), I(value)}); }
int lsm2d_get_option(lsm2d_context* ctx, const char* key, int64_t* out_value) {
  const int rc = rec("lsm2d_get_option", {H(ctx, "lsm2d_get_option"), T(key), O(out_value)});
  if (!rc) *out_value = 3;
  return rc;
}
int lsm2d_last_kernel_ms(lsm2d_context* ctx, float* out_ms) {
  const int rc = rec("lsm2d_last_kernel_ms", {H(ctx, "lsm2d_last_kernel_ms"), O(out_ms)});
  if (!rc) *out_ms = 0.5f;
  return rc;
}

int lsm2d_cloudset_create(lsm2d_context* ctx, const float* points_xynn, const int32_t* offsets, int32_t n_clouds, int64_t total_points, lsm2d_cloudset** out_set) {
  const char* sym = "lsm2d_cloudset_create";
  const int rc = rec(sym, {H(ctx, sym), X(points_xynn, 16 * (size_t) total_points), X(offsets, 4 * ((size_t) n_clouds + 1)), I(n_clouds), I(total_points), O(out_set)});
  if (!rc) *out_set = fresh<lsm2d_cloudset>(sym, n_clouds, total_points);
  return rc;
}
int lsm2d_cloudset_create_reserved(lsm2d_context* ctx, int64_t capacity_points, lsm2d_cloudset** out_set) {
  const char* sym = "lsm2d_cloudset_create_reserved";
  const int rc = rec(sym, {H(ctx, sym), I(capacity_points), O(out_set)});
  if (!rc) *out_set = fresh<lsm2d_cloudset>(sym, 1, 0);
  return rc;
}
int lsm2d_cloudset_create_reserved_many(lsm2d_context* ctx, int32_t n_clouds, int64_t capacity_per_cloud, lsm2d_cloudset** out_set) {
  const char* sym = "lsm2d_cloudset_create_reserved_many";
  const int rc = rec(sym, {H(ctx, sym), I(n_clouds), I(capacity_per_cloud), O(out_set)});
  if (!rc) *out_set = fresh<lsm2d_cloudset>(sym, n_clouds, 0);
  return rc;
}
int lsm2d_cloudset_clear_clouds(lsm2d_cloudset* set, int32_t n, const int32_t* cloud_index) {
  const char* sym = "lsm2d_cloudset_clear_clouds";
  return rec(sym, {H(set, sym), I(n), X(cloud_index, 4 * (size_t) n)});
}
int lsm2d_cloudset_upload(lsm2d_cloudset* set, const float* points_xynn, int64_t n_points) {
  const char* sym = "lsm2d_cloudset_upload";
  const int rc = rec(sym, {H(set, sym), X(points_xynn, 16 * (size_t) n_points), I(n_points)});
  if (!rc) reinterpret_cast<Handle*>(set)->n_points = n_points;
  return rc;
}
int lsm2d_cloudset_download(const lsm2d_cloudset* set, int32_t cloud_index, float* out_points_xynn, int64_t capacity, int64_t* out_n) {
  const char* sym = "lsm2d_cloudset_download";
  const int rc = rec(sym, {H(set, sym), I(cloud_index), O(out_points_xynn), I(capacity), O(out_n)});
  if (!rc) *out_n = capacity > 0 ? capacity - 1 : 0;      // one fewer than the room made: the caller has to shrink to it
  return rc;
}
void lsm2d_cloudset_destroy(lsm2d_cloudset* set) { destroy(set, "lsm2d_cloudset_destroy"); }
int32_t lsm2d_cloudset_num_clouds(const lsm2d_cloudset* set) { rec("lsm2d_cloudset_num_clouds", {H(set, "lsm2d_cloudset_num_clouds")}); return peek(set)->n_clouds; }
int64_t lsm2d_cloudset_num_points(const lsm2d_cloudset* set) { rec("lsm2d_cloudset_num_points", {H(set, "lsm2d_cloudset_num_points")}); return peek(set)->n_points; }
int32_t lsm2d_cloudset_cloud_sizes(const lsm2d_cloudset* set, int32_t* out_sizes, int32_t capacity) {
  const int rc = rec("lsm2d_cloudset_cloud_sizes", {H(set, "lsm2d_cloudset_cloud_sizes"), O(out_sizes), I(capacity)});
  if (rc) return rc;
  for (int32_t i = 0; i < capacity && i < peek(set)->n_clouds; ++i) out_sizes[i] = 3 + i;
  return peek(set)->n_clouds;
}

int lsm2d_preprocess_scans(lsm2d_context* ctx, const lsm2d_preprocessor* params, const float* ranges, int32_t n_scans, lsm2d_cloudset** out_set) {
  const char* sym = "lsm2d_preprocess_scans";
  const int rc = rec(sym, {H(ctx, sym), S(params), X(ranges, 4 * (size_t) n_scans * (size_t) params->n_beams), I(n_scans), O(out_set)});
  if (!rc) *out_set = fresh<lsm2d_cloudset>(sym, n_scans, 7);
  return rc;
}
int lsm2d_preprocess_scans_refill(lsm2d_context* ctx, const lsm2d_preprocessor* params, const float* ranges, int32_t n_scans, lsm2d_cloudset* set) {
  const char* sym = "lsm2d_preprocess_scans_refill";
  return rec(sym, {H(ctx, sym), S(params), X(ranges, 4 * (size_t) n_scans * (size_t) params->n_beams), I(n_scans), H(set, sym)});
}
int lsm2d_clip_scene_voxelized(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* full_scene, int32_t scene_index,
                               const float robot_in_local_map[3], const float sensor_in_robot[3], float voxelize_resolution, lsm2d_cloudset* clipped,
                               int32_t* out_n_points, int32_t* out_source_idx) {
  const char* sym = "lsm2d_clip_scene_voxelized";
  const int rc = rec(sym, {H(ctx, sym), S(projector), H(full_scene, sym), I(scene_index), X(robot_in_local_map, 12), X(sensor_in_robot, 12), F(voxelize_resolution),
                           H(clipped, sym), O(out_n_points), O(out_source_idx)});
  if (!rc && out_n_points) *out_n_points = 3;
  return rc;
}
int lsm2d_merge_scene(lsm2d_context* ctx, const lsm2d_projector* projector, lsm2d_cloudset* scene, const lsm2d_cloudset* measurement, int32_t measurement_index,
                      const float measurement_in_scene[3], float merge_threshold, int32_t* out_scene_size, int32_t* out_counts) {
  const char* sym = "lsm2d_merge_scene";
  const int rc = rec(sym, {H(ctx, sym), S(projector), H(scene, sym), H(measurement, sym), I(measurement_index), X(measurement_in_scene, 12), F(merge_threshold),
                           O(out_scene_size), O(out_counts)});
  if (!rc && out_scene_size) *out_scene_size = 5;
  if (!rc && out_counts) { out_counts[0] = 1; out_counts[1] = 2; out_counts[2] = 3; }
  return rc;
}
int lsm2d_merge_scenes(lsm2d_context* ctx, const lsm2d_projector* projector, lsm2d_cloudset* scene, int32_t n_measurements, const lsm2d_cloudset* const* measurements,
                       const int32_t* meas_index, const float* measurement_in_scene, float merge_threshold, int32_t* out_size, int32_t* out_counts) {
  const char* sym = "lsm2d_merge_scenes";
  const size_t n = (size_t) n_measurements;
  const int rc = rec(sym, {H(ctx, sym), S(projector), H(scene, sym), I(n_measurements), HS(measurements, n, sym), X(meas_index, 4 * n), X(measurement_in_scene, 12 * n),
                           F(merge_threshold), O(out_size), O(out_counts)});
  if (!rc && out_size) *out_size = 6;
  return rc;
}
int lsm2d_clip_scene_batch(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* scenes, int32_t n_trackers, const int32_t* scene_index,
                           const float* robot_in_local_map, const float sensor_in_robot[3], lsm2d_cloudset* clipped, int32_t* out_n_points) {
  const char* sym = "lsm2d_clip_scene_batch";
  const size_t n = (size_t) n_trackers;
  return rec(sym, {H(ctx, sym), S(projector), H(scenes, sym), I(n_trackers), X(scene_index, 4 * n), X(robot_in_local_map, 12 * n), X(sensor_in_robot, 12),
                   H(clipped, sym), O(out_n_points)});
}
int lsm2d_clip_scene_voxelized_batch(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* scenes, int32_t n_trackers, const int32_t* scene_index,
                                     const float* robot_in_local_map, const float sensor_in_robot[3], float voxelize_resolution, lsm2d_cloudset* clipped,
                                     int32_t* out_n_points) {
  const char* sym = "lsm2d_clip_scene_voxelized_batch";
  const size_t n = (size_t) n_trackers;
  return rec(sym, {H(ctx, sym), S(projector), H(scenes, sym), I(n_trackers), X(scene_index, 4 * n), X(robot_in_local_map, 12 * n), X(sensor_in_robot, 12),
                   F(voxelize_resolution), H(clipped, sym), O(out_n_points)});
}
int lsm2d_merge_scene_batch(lsm2d_context* ctx, const lsm2d_projector* projector, lsm2d_cloudset* scenes, int32_t n_trackers, const int32_t* scene_index,
                            int32_t n_measurements, const lsm2d_cloudset* const* measurements, const int32_t* meas_index, const float* measurement_in_scene,
                            float merge_threshold, int32_t* out_sizes, int32_t* out_counts) {
  const char* sym = "lsm2d_merge_scene_batch";
  const size_t n = (size_t) n_trackers, nm = (size_t) n_measurements;
  return rec(sym, {H(ctx, sym), S(projector), H(scenes, sym), I(n_trackers), X(scene_index, 4 * n), I(n_measurements), HS(measurements, nm, sym), X(meas_index, 4 * n * nm),
                   X(measurement_in_scene, 12 * n * nm), F(merge_threshold), O(out_sizes), O(out_counts)});
}

int lsm2d_find_correspondences(lsm2d_context* ctx, const lsm2d_slice_params* slice, const lsm2d_cloudset* fixed, int32_t fixed_index, const lsm2d_cloudset* moving,
                               int32_t moving_index, const float local_map_in_sensor[3], lsm2d_correspondence* out_pairs, int32_t capacity, int32_t* out_n_pairs) {
  const char* sym = "lsm2d_find_correspondences";
  const int rc = rec(sym, {H(ctx, sym), S(slice), H(fixed, sym), I(fixed_index), H(moving, sym), I(moving_index), X(local_map_in_sensor, 12), O(out_pairs), I(capacity),
                           O(out_n_pairs)});
  if (rc) return rc;
  *out_n_pairs = std::min<int32_t>(capacity, 2);
  for (int32_t j = 0; j < *out_n_pairs; ++j) out_pairs[j] = lsm2d_correspondence{j, j + 1};
  return rc;
}
int lsm2d_find_correspondences_batch(lsm2d_context* ctx, const lsm2d_slice_params* slice, const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                     const lsm2d_cloudset* moving, const int32_t* moving_index, int32_t n_items, const float* local_map_in_sensor,
                                     lsm2d_correspondence* out_pairs, int32_t pair_capacity, int32_t* out_n_pairs) {
  const char* sym = "lsm2d_find_correspondences_batch";
  const size_t n = (size_t) n_items;
  const int rc = rec(sym, {H(ctx, sym), S(slice), H(fixed, sym), X(fixed_index, 4 * n), H(moving, sym), X(moving_index, 4 * n), I(n_items), X(local_map_in_sensor, 12 * n),
                           O(out_pairs), I(pair_capacity), O(out_n_pairs)});
  if (rc) return rc;
  for (int32_t i = 0; i < n_items; ++i) {         // item i: min(i + 1, capacity) pairs (10 i + j, j)
    out_n_pairs[i] = std::min<int32_t>(pair_capacity, i + 1);
    for (int32_t j = 0; j < out_n_pairs[i]; ++j) out_pairs[(size_t) i * (size_t) pair_capacity + (size_t) j] = lsm2d_correspondence{10 * i + j, j};
  }
  return rc;
}
int lsm2d_linearize(lsm2d_context* ctx, const lsm2d_slice_params* slice, const lsm2d_cloudset* fixed, int32_t fixed_index, const lsm2d_cloudset* moving,
                    int32_t moving_index, const lsm2d_correspondence* pairs, int32_t n_pairs, const float pose[3], float out_H[9], float out_b[3],
                    lsm2d_iteration_stats* out_stats) {
  const char* sym = "lsm2d_linearize";
  const int rc = rec(sym, {H(ctx, sym), S(slice), H(fixed, sym), I(fixed_index), H(moving, sym), I(moving_index), X(pairs, 8 * (size_t) n_pairs), I(n_pairs), X(pose, 12),
                           O(out_H), O(out_b), O(out_stats)});
  if (!rc) rows(1, out_H, out_b, out_stats, nullptr);
  return rc;
}
int lsm2d_linearize_batch(lsm2d_context* ctx, const lsm2d_slice_params* slice, const lsm2d_cloudset* fixed, const int32_t* fixed_index, const lsm2d_cloudset* moving,
                          const int32_t* moving_index, int32_t n_items, const lsm2d_correspondence* pairs, int32_t pair_capacity, const int32_t* n_pairs,
                          const float* poses, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats) {
  const char* sym = "lsm2d_linearize_batch";
  const size_t n = (size_t) n_items;
  const int rc = rec(sym, {H(ctx, sym), S(slice), H(fixed, sym), X(fixed_index, 4 * n), H(moving, sym), X(moving_index, 4 * n), I(n_items),
                           X(pairs, 8 * n * (size_t) pair_capacity), I(pair_capacity), X(n_pairs, 4 * n), X(poses, 12 * n), O(out_H), O(out_b), O(out_stats)});
  if (!rc) rows(n, out_H, out_b, out_stats, nullptr);
  return rc;
}
int lsm2d_score_batch(lsm2d_context* ctx, const lsm2d_slice_params* slice, const lsm2d_cloudset* fixed, const int32_t* fixed_index, const lsm2d_cloudset* moving,
                      const int32_t* moving_index, int32_t n_items, const float* poses, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats) {
  const char* sym = "lsm2d_score_batch";
  const size_t n = (size_t) n_items;
  const int rc = rec(sym, {H(ctx, sym), S(slice), H(fixed, sym), X(fixed_index, 4 * n), H(moving, sym), X(moving_index, 4 * n), I(n_items), X(poses, 12 * n), O(out_H),
                           O(out_b), O(out_stats)});
  if (!rc) rows(n, out_H, out_b, out_stats, nullptr);
  return rc;
}
int lsm2d_score_select(lsm2d_context* ctx, const lsm2d_slice_params* slice, const lsm2d_cloudset* fixed, const int32_t* fixed_index, const lsm2d_cloudset* moving,
                       const int32_t* moving_index, int32_t n_items, const float* poses, const lsm2d_select_params* select_params, int32_t k, int32_t* out_index,
                       float* out_H, float* out_b, lsm2d_iteration_stats* out_stats, int32_t* out_n_selected, int32_t* out_n_accepted) {
  const char* sym = "lsm2d_score_select";
  const size_t n = (size_t) n_items;
  const int rc = rec(sym, {H(ctx, sym), S(slice), H(fixed, sym), X(fixed_index, 4 * n), H(moving, sym), X(moving_index, 4 * n), I(n_items), X(poses, 12 * n),
                           S(select_params), I(k), O(out_index), O(out_H), O(out_b), O(out_stats), O(out_n_selected), O(out_n_accepted)});
  if (!rc) rows((size_t) select(k, out_index, out_n_selected, out_n_accepted), out_H, out_b, out_stats, nullptr);
  return rc;
}

int lsm2d_align_batch(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch, float* out_pose, float* out_H, int32_t* out_status,
                      int32_t* out_iterations, lsm2d_iteration_stats* out_stats) {
  const char* sym = "lsm2d_align_batch";
  const int rc = rec(sym, {H(ctx, sym), S(aligner), B(batch, sym), O(out_pose), O(out_H), O(out_status), O(out_iterations), O(out_stats)});
  if (!rc) aligned((size_t) batch->n_alignments, out_pose, out_H, out_status, out_iterations, out_stats, STATS_CAPACITY);
  return rc;
}
int lsm2d_align_batch_pairs(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch, float* out_pose, float* out_H, int32_t* out_status,
                            int32_t* out_iterations, lsm2d_iteration_stats* out_stats, lsm2d_correspondence* out_pairs, int32_t pair_capacity, int32_t* out_n_pairs) {
  const char* sym = "lsm2d_align_batch_pairs";
  const int rc = rec(sym, {H(ctx, sym), S(aligner), B(batch, sym), O(out_pose), O(out_H), O(out_status), O(out_iterations), O(out_stats), O(out_pairs), I(pair_capacity),
                           O(out_n_pairs)});
  if (rc) return rc;
  aligned((size_t) batch->n_alignments, out_pose, out_H, out_status, out_iterations, out_stats, STATS_CAPACITY);
  for (int32_t s = 0; s < batch->n_alignments * batch->n_slices; ++s) {       // slice s: min(s + 1, capacity) pairs (s, j)
    out_n_pairs[s] = std::min<int32_t>(pair_capacity, s + 1);
    for (int32_t j = 0; j < out_n_pairs[s]; ++j) out_pairs[(size_t) s * (size_t) pair_capacity + (size_t) j] = lsm2d_correspondence{s, j};
  }
  return rc;
}
int lsm2d_align_select(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch, const lsm2d_select_params* select_params, int32_t k,
                       int32_t* out_index, float* out_pose, float* out_H, int32_t* out_iterations, lsm2d_iteration_stats* out_last_stats, int32_t* out_n_selected,
                       int32_t* out_n_accepted, int32_t* out_n_success) {
  const char* sym = "lsm2d_align_select";
  const int rc = rec(sym, {H(ctx, sym), S(aligner), B(batch, sym), S(select_params), I(k), O(out_index), O(out_pose), O(out_H), O(out_iterations), O(out_last_stats),
                           O(out_n_selected), O(out_n_accepted), O(out_n_success)});
  if (!rc) aligned((size_t) select(k, out_index, out_n_selected, out_n_accepted, out_n_success), out_pose, out_H, nullptr, out_iterations, out_last_stats, 1);
  return rc;
}
int lsm2d_score_aligner_batch(lsm2d_context* ctx, const lsm2d_batch* batch, float* out_H, float* out_b, lsm2d_iteration_stats* out_stats, int32_t* out_active) {
  const char* sym = "lsm2d_score_aligner_batch";
  const int rc = rec(sym, {H(ctx, sym), B(batch, sym), O(out_H), O(out_b), O(out_stats), O(out_active)});
  if (!rc) rows((size_t) batch->n_alignments, out_H, out_b, out_stats, out_active);
  return rc;
}
int lsm2d_score_aligner_select(lsm2d_context* ctx, const lsm2d_batch* batch, const lsm2d_select_params* select_params, int32_t k, int32_t* out_index, float* out_H,
                               float* out_b, lsm2d_iteration_stats* out_stats, int32_t* out_active, int32_t* out_n_selected, int32_t* out_n_accepted) {
  const char* sym = "lsm2d_score_aligner_select";
  const int rc = rec(sym, {H(ctx, sym), B(batch, sym), S(select_params), I(k), O(out_index), O(out_H), O(out_b), O(out_stats), O(out_active), O(out_n_selected),
                           O(out_n_accepted)});
  if (!rc) rows((size_t) select(k, out_index, out_n_selected, out_n_accepted), out_H, out_b, out_stats, out_active);
  return rc;
}
int lsm2d_align_batch_begin(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch, int32_t want_stats, lsm2d_pending** out_pending) {
  const char* sym = "lsm2d_align_batch_begin";
  const int rc = rec(sym, {H(ctx, sym), S(aligner), B(batch, sym), I(want_stats), O(out_pending)});
  if (!rc) *out_pending = fresh<lsm2d_pending>(sym, batch->n_alignments);
  return rc;
}
int lsm2d_align_batch_wait(lsm2d_pending* pending, float* out_pose, float* out_H, int32_t* out_status, int32_t* out_iterations, lsm2d_iteration_stats* out_stats) {
  const char* sym = "lsm2d_align_batch_wait";
  const int rc = rec(sym, {H(pending, sym), O(out_pose), O(out_H), O(out_status), O(out_iterations), O(out_stats)});
  const size_t n = (size_t) peek(pending)->n_clouds;          // (the batch's n_alignments)
  destroy(pending, sym);                                      // wait() consumes the handle whatever it returns
  if (!rc) aligned(n, out_pose, out_H, out_status, out_iterations, out_stats, STATS_CAPACITY);
  return rc;
}

int lsm2d_sweep_create(const int32_t* device_ids, int32_t n_devices, lsm2d_sweep** out_sweep) {
  const int rc = rec("lsm2d_sweep_create", {X(device_ids, 4 * (size_t) n_devices), I(n_devices), O(out_sweep)});
  if (!rc) *out_sweep = fresh<lsm2d_sweep>("lsm2d_sweep_create", n_devices);
  return rc;
}
void lsm2d_sweep_destroy(lsm2d_sweep* sweep) { destroy(sweep, "lsm2d_sweep_destroy"); }
int32_t lsm2d_sweep_num_devices(const lsm2d_sweep* sweep) { rec("lsm2d_sweep_num_devices", {H(sweep, "lsm2d_sweep_num_devices")}); return peek(sweep)->n_clouds; }
const char* lsm2d_sweep_last_error(const lsm2d_sweep* sweep) { H(sweep, "lsm2d_sweep_last_error"); return "(stand-in sweep)"; }
int lsm2d_sweep_set_map(lsm2d_sweep* sweep, const float* map_xynn, int64_t n_points) {
  return rec("lsm2d_sweep_set_map", {H(sweep, "lsm2d_sweep_set_map"), X(map_xynn, 16 * (size_t) n_points), I(n_points)});
}
int lsm2d_sweep_set_scans(lsm2d_sweep* sweep, const float* scans_xynn, const int32_t* offsets, int32_t n_scans) {
  const char* sym = "lsm2d_sweep_set_scans";
  return rec(sym, {H(sweep, sym), X(scans_xynn, offsets ? 16 * (size_t) offsets[n_scans] : 0), X(offsets, 4 * ((size_t) n_scans + 1)), I(n_scans)});
}
int lsm2d_sweep_align(lsm2d_sweep* sweep, const lsm2d_aligner_params* aligner, const lsm2d_slice_params* slice, int32_t n_candidates, const int32_t* scan_index,
                      const float* init_pose, float* out_pose, float* out_H, int32_t* out_status, int32_t* out_iterations, lsm2d_iteration_stats* out_last_stats) {
  const char* sym = "lsm2d_sweep_align";
  const size_t n = (size_t) n_candidates;
  const int rc = rec(sym, {H(sweep, sym), S(aligner), S(slice), I(n_candidates), X(scan_index, 4 * n), X(init_pose, 12 * n), O(out_pose), O(out_H), O(out_status),
                           O(out_iterations), O(out_last_stats)});
  if (!rc) aligned(n, out_pose, out_H, out_status, out_iterations, out_last_stats, 1);
  return rc;
}
int lsm2d_sweep_align_select(lsm2d_sweep* sweep, const lsm2d_aligner_params* aligner, const lsm2d_slice_params* slice, int32_t n_candidates, const int32_t* scan_index,
                             const float* init_pose, const lsm2d_select_params* select_params, int32_t k, int32_t* out_index, float* out_pose, float* out_H,
                             int32_t* out_iterations, lsm2d_iteration_stats* out_last_stats, int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success) {
  const char* sym = "lsm2d_sweep_align_select";
  const size_t n = (size_t) n_candidates;
  const int rc = rec(sym, {H(sweep, sym), S(aligner), S(slice), I(n_candidates), X(scan_index, 4 * n), X(init_pose, 12 * n), S(select_params), I(k), O(out_index),
                           O(out_pose), O(out_H), O(out_iterations), O(out_last_stats), O(out_n_selected), O(out_n_accepted), O(out_n_success)});
  if (!rc) aligned((size_t) select(k, out_index, out_n_selected, out_n_accepted, out_n_success), out_pose, out_H, nullptr, out_iterations, out_last_stats, 1);
  return rc;
}

}  // extern "C"
