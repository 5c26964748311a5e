// lsm2d.hpp -- header-only C++ host mirror of the reference's finder / aligner surface over the C ABI
// (include/lsm2d.h).  Same method names, argument meaning and error behaviour as the reference classes:
//   CorrespondenceFinderProjective2f   registration/correspondence_finder_projective_2d.{h,cpp}
//       setFixed / setMoving / setLocalMapInSensor / setCorrespondences / compute
//       (apps/visual_test_correspondence_finder_projective_2d.cpp:74-79); throws std::runtime_error on a
//       missing projector / fixed / moving exactly where the reference does (.cpp:21-31)
//   MultiAligner2D                     upstream, driven as in apps/visual_test_aligner_2d.cpp:123-156
//       param_slice_processors / setFixed / setMoving / setMovingInFixed / compute / movingInFixed /
//       iterationStats / status
//   LaserMessageBatchStream            batches of fresh LaserMessages through preprocessor + aligner, pipelined over three scan sets
//       (lsm2d_preprocess_scans_refill, lsm2d_align_batch_begin / _wait)
//   TrackerBatch                       N independent live trackers stepped together: one batched clip, align and merge per step
//       (lsm2d_clip_scene_batch or, with Params::clip_voxelize_resolution > 0, lsm2d_clip_scene_voxelized_batch; lsm2d_align_batch, lsm2d_merge_scene_batch), each tracker's bits those of the single-tracker calls
// This header depends on nothing but the C ABI and the standard library, so it compiles with plain g++;
// the SRRG-side adapter (adapters/srrg/) is the same code expressed with srrg2_core types.
#pragma once
#include <lsm2d.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace lsm2d_host {

struct PointNormal2f { float x, y, nx, ny; };                 // srrg2_core::PointNormal2f payload
using PointNormal2fVectorCloud = std::vector<PointNormal2f>;
using Correspondence = lsm2d_correspondence;                  // {fixed_idx, moving_idx}
using CorrespondenceVector = std::vector<Correspondence>;
using Vector3f = std::array<float, 3>;                        // geometry2d::t2v(Isometry2f) = (x, y, theta)

inline void check(int rc, const char* where, const lsm2d_context* ctx = nullptr) {
  if (rc < 0) throw std::runtime_error(std::string(where) + ": " + lsm2d_status_string(rc) + " " + lsm2d_last_error(ctx));
}

class Context {
 public:
  explicit Context(int device = 0, void* hip_stream = nullptr) { check(lsm2d_create(device, hip_stream, &_h), "lsm2d_create"); }
  ~Context() { lsm2d_destroy(_h); }
  Context(const Context&) = delete; Context& operator=(const Context&) = delete;
  lsm2d_context* get() const { return _h; }
  void setKernelTiming(bool on) { check(lsm2d_set_option(_h, "kernel_timing", on ? 1 : 0), "lsm2d_set_option", _h); }   // needed before lastKernelMs()
  // "align_path": 0 automatic, 1 k_align, 2 split over many workgroups, 3 two projective slices side by side (include/lsm2d.h)
  void setOption(const char* key, int64_t value) { check(lsm2d_set_option(_h, key, value), "lsm2d_set_option", _h); }
  int64_t getOption(const char* key) const { int64_t v = 0; check(lsm2d_get_option(_h, key, &v), "lsm2d_get_option", _h); return v; }
  float lastKernelMs() const { float ms = 0; check(lsm2d_last_kernel_ms(_h, &ms), "lsm2d_last_kernel_ms", _h); return ms; }
 private:
  lsm2d_context* _h = nullptr;
};

namespace detail {
// what the C ABI takes for a vector: its first element, NULL when there is none (a cloud as its floats x, y, nx, ny; poses as their floats)
template <class T> const T* ptrOrNull(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
inline const float* ptrOrNull(const PointNormal2fVectorCloud& c) { return c.empty() ? nullptr : &c[0].x; }
inline const float* ptrOrNull(const std::vector<Vector3f>& v) { return v.empty() ? nullptr : v[0].data(); }

// the one owner of a lsm2d_cloudset*: every set this header makes lives in one of these, so that a throw anywhere gives it back; reads as the pointer
class CloudSetHandle {
 public:
  CloudSetHandle() = default; ~CloudSetHandle() { lsm2d_cloudset_destroy(_h); }
  CloudSetHandle(const CloudSetHandle&) = delete; CloudSetHandle& operator=(const CloudSetHandle&) = delete;
  operator lsm2d_cloudset*() const { return _h; }
  lsm2d_cloudset** out() { return &_h; }      // where a creating call puts the set: only while this handle is empty
 private:
  lsm2d_cloudset* _h = nullptr;
};
}  // namespace detail
using detail::ptrOrNull;

// device-resident copy of one cloud or of a ragged batch of clouds
class CloudSet {
 public:
  CloudSet(Context& ctx, const PointNormal2fVectorCloud& cloud) {
    check(lsm2d_cloudset_create(ctx.get(), ptrOrNull(cloud), nullptr, 1, (int64_t) cloud.size(), _h.out()), "lsm2d_cloudset_create", ctx.get());
  }
  CloudSet(Context& ctx, const std::vector<PointNormal2fVectorCloud>& clouds) {
    std::vector<int32_t> offs(1, 0); PointNormal2fVectorCloud packed;
    for (const auto& c : clouds) { packed.insert(packed.end(), c.begin(), c.end()); offs.push_back((int32_t) packed.size()); }
    check(lsm2d_cloudset_create(ctx.get(), ptrOrNull(packed), offs.data(), (int32_t) clouds.size(), (int64_t) packed.size(), _h.out()),
          "lsm2d_cloudset_create", ctx.get());
  }
  lsm2d_cloudset* get() const { return _h; }
  int32_t numClouds() const { return lsm2d_cloudset_num_clouds(_h); }
 private:
  detail::CloudSetHandle _h;
};

// PointNormal2fProjectorPolar parameters (apps/synthetic_scene_generator.cpp:69-75, MULTI.json:71-97)
struct PointNormal2fProjectorPolar {
  int   param_canvas_cols = 721;
  float param_angle_col_min = -3.14159f, param_angle_col_max = 3.14159f;
  float param_range_min = 0.3f, param_range_max = 20.f;
  float col_offset = 0.f;
  lsm2d_projector abi() const { return {param_canvas_cols, param_angle_col_min, param_angle_col_max, param_range_min, param_range_max, col_offset}; }
};
using PointNormal2fProjectorPolarPtr = std::shared_ptr<PointNormal2fProjectorPolar>;

// what the factor returns for one item: H (row-major 3x3), b and the statistics; with the slices of a whole aligner, how many of them contributed
struct Linearization { std::array<float, 9> H{}; std::array<float, 3> b{}; lsm2d_iteration_stats stats{}; };
struct AlignerScore { Linearization row; int32_t active = 0; };

namespace detail {
template <class T> bool emptyOrHolds(const std::vector<T>& v, size_t n) { return v.empty() || v.size() == n; }
// an index vector is left out (empty) or holds `n` entries; `rule` is the caller's wording of that, `others` what its wording covers besides
inline void checkIndexVectors(const char* who, const char* rule, const std::vector<int32_t>& fixed_index, const std::vector<int32_t>& moving_index, size_t n,
                              bool others = true) {
  if (!emptyOrHolds(fixed_index, n) || !emptyOrHolds(moving_index, n) || !others) throw std::runtime_error(std::string(who) + "| " + rule);
}
constexpr const char* ONE_PER_POSE = "an index vector is empty or holds one entry per pose";

// the flat rows a scoring call fills -- H[9 m], b[3 m], stats[m] and, for a whole aligner, active[m] -- with room for at least one
struct RowBuffer {
  std::vector<float> H, b; std::vector<lsm2d_iteration_stats> stats; std::vector<int32_t> active;
  explicit RowBuffer(size_t m, bool with_active = false)
      : H(9 * std::max<size_t>(m, 1)), b(3 * std::max<size_t>(m, 1)), stats(std::max<size_t>(m, 1)), active(with_active ? std::max<size_t>(m, 1) : 0, 0) {}
  void fill(Linearization& r, size_t i) const {
    std::copy(H.begin() + (ptrdiff_t) (9 * i), H.begin() + (ptrdiff_t) (9 * i + 9), r.H.begin());
    std::copy(b.begin() + (ptrdiff_t) (3 * i), b.begin() + (ptrdiff_t) (3 * i + 3), r.b.begin());
    r.stats = stats[i];
  }
  void fill(AlignerScore& r, size_t i) const { fill(r.row, i); r.active = active[i]; }
  template <class Row> std::vector<Row> rows(size_t m) const { std::vector<Row> out(m); for (size_t i = 0; i < m; ++i) fill(out[i], i); return out; }
};

// a lsm2d_batch and the two handle arrays it points into: slices[s] reads fixed[s] / moving[s]; everything else stays the caller's
struct BatchDescriptor {
  std::vector<const lsm2d_cloudset*> fx, mv; lsm2d_batch b{};
  BatchDescriptor(size_t n, const lsm2d_slice_params* slices, std::vector<const lsm2d_cloudset*> fixed, std::vector<const lsm2d_cloudset*> moving,
                  const float* init_pose, const lsm2d_prior* prior = nullptr, const int32_t* fixed_index = nullptr, const int32_t* moving_index = nullptr)
      : fx(std::move(fixed)), mv(std::move(moving)) {
    b.n_alignments = (int32_t) n; b.n_slices = (int32_t) fx.size(); b.slices = slices; b.fixed = fx.data(); b.moving = mv.data();
    b.fixed_index = fixed_index; b.moving_index = moving_index; b.init_pose = init_pose; b.prior = prior;
  }
  BatchDescriptor(const BatchDescriptor&) = delete; BatchDescriptor& operator=(const BatchDescriptor&) = delete;
};
inline std::vector<const lsm2d_cloudset*> handles(const std::vector<const CloudSet*>& sets) {
  std::vector<const lsm2d_cloudset*> out;
  for (const CloudSet* cs : sets) out.push_back(cs ? cs->get() : nullptr);
  return out;
}
inline void checkSetsPerSlice(const char* who, size_t n_slices, const std::vector<const CloudSet*>& fixed, const std::vector<const CloudSet*>& moving) {
  if (fixed.size() != n_slices || moving.size() != n_slices) throw std::runtime_error(std::string(who) + "| one fixed and one moving set per slice");
}
// the batch of the aligner-scoring calls, refusing what they refuse
inline BatchDescriptor alignerBatch(const char* who, const std::vector<lsm2d_slice_params>& slices, const std::vector<const CloudSet*>& fixed,
                                    const std::vector<const CloudSet*>& moving, const std::vector<Vector3f>& poses, const std::vector<lsm2d_prior>& priors,
                                    const std::vector<int32_t>& fixed_index, const std::vector<int32_t>& moving_index) {
  const size_t n = poses.size(), ns = slices.size();
  checkSetsPerSlice(who, ns, fixed, moving);
  checkIndexVectors(who, "an index vector is empty or holds n_slices x n entries", fixed_index, moving_index, ns * n);
  if (!emptyOrHolds(priors, n)) throw std::runtime_error(std::string(who) + "| priors is empty or holds one per pose");
  return BatchDescriptor(n, slices.data(), handles(fixed), handles(moving), ptrOrNull(poses), ptrOrNull(priors), ptrOrNull(fixed_index), ptrOrNull(moving_index));
}
}  // namespace detail

// compute() of a finder for poses.size() independent (fixed, moving, pose) triples in one launch (lsm2d_find_correspondences_batch): item i matches cloud
// fixed_index[i] of `fixed` against cloud moving_index[i] of `moving` (an empty index vector: cloud i, or the only cloud of a one-cloud set) under poses[i];
// per item the vector compute() fills, in the same order
inline std::vector<CorrespondenceVector> findCorrespondencesBatch(Context& ctx, const lsm2d_slice_params& sp, const CloudSet& fixed, const CloudSet& moving,
                                                                  const std::vector<Vector3f>& poses, const std::vector<int32_t>& fixed_index,
                                                                  const std::vector<int32_t>& moving_index) {
  const size_t n = poses.size();
  detail::checkIndexVectors("findCorrespondencesBatch", detail::ONE_PER_POSE, fixed_index, moving_index, n);
  size_t cap = 0;
  if (sp.finder == LSM2D_FINDER_PROJECTIVE) cap = (size_t) (sp.projector.canvas_cols > 0 ? sp.projector.canvas_cols : 0);
  else {      // one pair per point of the largest moving cloud
    std::vector<int32_t> sizes((size_t) moving.numClouds(), 0);
    check(std::min(lsm2d_cloudset_cloud_sizes(moving.get(), sizes.data(), (int32_t) sizes.size()), 0), "lsm2d_cloudset_cloud_sizes", ctx.get());
    for (int32_t v : sizes) cap = std::max(cap, (size_t) v);
  }
  std::vector<Correspondence> buf(std::max<size_t>(cap * n, 1)); std::vector<int32_t> cnt(std::max<size_t>(n, 1), 0);
  check(lsm2d_find_correspondences_batch(ctx.get(), &sp, fixed.get(), ptrOrNull(fixed_index), moving.get(), ptrOrNull(moving_index), (int32_t) n, ptrOrNull(poses),
                                         buf.data(), (int32_t) cap, cnt.data()),
        "lsm2d_find_correspondences_batch", ctx.get());
  std::vector<CorrespondenceVector> out(n);
  for (size_t i = 0; i < n; ++i) out[i].assign(buf.begin() + (ptrdiff_t) (i * cap), buf.begin() + (ptrdiff_t) (i * cap + (size_t) cnt[i]));
  return out;
}

// SE2Plane2PlaneErrorFactor + robustifier over a correspondence vector (lsm2d_linearize; registration/aligner_slice_processor_laser_2d.h:4,8): H, b and the
// statistics of cloud fixed_index of `fixed` against cloud moving_index of `moving` at `pose`.  The slice parameters' robustifier and chi_threshold are the
// ones that matter here.
inline Linearization linearize(Context& ctx, const lsm2d_slice_params& sp, const CloudSet& fixed, const CloudSet& moving, const CorrespondenceVector& pairs,
                               const Vector3f& pose, int32_t fixed_index = 0, int32_t moving_index = 0) {
  Linearization r;
  check(lsm2d_linearize(ctx.get(), &sp, fixed.get(), fixed_index, moving.get(), moving_index, ptrOrNull(pairs), (int32_t) pairs.size(), pose.data(),
                        r.H.data(), r.b.data(), &r.stats),
        "lsm2d_linearize", ctx.get());
  return r;
}
// ... and over poses.size() vectors in one launch (lsm2d_linearize_batch): item i is pairs[i] between cloud fixed_index[i] of `fixed` and cloud
// moving_index[i] of `moving` (an empty index vector: cloud i, or the only cloud of a one-cloud set) at poses[i]; per item what linearize() returns, bit for
// bit.  `pairs` is what findCorrespondencesBatch returns.
inline std::vector<Linearization> linearizeBatch(Context& ctx, const lsm2d_slice_params& sp, const CloudSet& fixed, const CloudSet& moving,
                                                 const std::vector<CorrespondenceVector>& pairs, const std::vector<Vector3f>& poses,
                                                 const std::vector<int32_t>& fixed_index = {}, const std::vector<int32_t>& moving_index = {}) {
  const size_t n = poses.size();
  if (pairs.size() != n) throw std::runtime_error("linearizeBatch| one correspondence vector per pose");
  detail::checkIndexVectors("linearizeBatch", detail::ONE_PER_POSE, fixed_index, moving_index, n);
  size_t cap = 1;
  for (const auto& v : pairs) cap = std::max(cap, v.size());
  std::vector<Correspondence> buf(std::max<size_t>(cap * n, 1)); std::vector<int32_t> cnt(std::max<size_t>(n, 1), 0);
  for (size_t i = 0; i < n; ++i) { std::copy(pairs[i].begin(), pairs[i].end(), buf.begin() + (ptrdiff_t) (i * cap)); cnt[i] = (int32_t) pairs[i].size(); }
  detail::RowBuffer rows(n);
  check(lsm2d_linearize_batch(ctx.get(), &sp, fixed.get(), ptrOrNull(fixed_index), moving.get(), ptrOrNull(moving_index), (int32_t) n, buf.data(), (int32_t) cap,
                              cnt.data(), ptrOrNull(poses), rows.H.data(), rows.b.data(), rows.stats.data()),
        "lsm2d_linearize_batch", ctx.get());
  return rows.rows<Linearization>(n);
}

// Finder, then factor, for poses.size() pose hypotheses with the pairs kept on the device (lsm2d_score_batch): item i matches cloud fixed_index[i] of
// `fixed` against cloud moving_index[i] of `moving` (an empty index vector: cloud i, or the only cloud of a one-cloud set) at poses[i] with the finder `sp`
// names and linearises what it found there; per item what findCorrespondencesBatch (a finder's computeBatch) followed by linearizeBatch returns, bit for
// bit, with one copy down and one wait.
inline std::vector<Linearization> scoreBatch(Context& ctx, const lsm2d_slice_params& sp, const CloudSet& fixed, const CloudSet& moving,
                                             const std::vector<Vector3f>& poses, const std::vector<int32_t>& fixed_index = {},
                                             const std::vector<int32_t>& moving_index = {}) {
  const size_t n = poses.size();
  detail::checkIndexVectors("scoreBatch", detail::ONE_PER_POSE, fixed_index, moving_index, n);
  detail::RowBuffer rows(n);
  check(lsm2d_score_batch(ctx.get(), &sp, fixed.get(), ptrOrNull(fixed_index), moving.get(), ptrOrNull(moving_index), (int32_t) n, ptrOrNull(poses), rows.H.data(),
                          rows.b.data(), rows.stats.data()),
        "lsm2d_score_batch", ctx.get());
  return rows.rows<Linearization>(n);
}

// scoreBatch's scoring, then the acceptance test and the best k accepted hypotheses ranked on the device (lsm2d_score_select): only k rows come down, with
// one copy and one wait.  index[j] is the j-th best hypothesis -- inliers descending, chi_inliers ascending, index ascending -- and rows[j] what scoreBatch
// returns for it, bit for bit; n_accepted counts the hypotheses that pass among all of them.
struct Selection { std::vector<int32_t> index; std::vector<Linearization> rows; int32_t n_accepted = 0; };
inline Selection scoreSelect(Context& ctx, const lsm2d_slice_params& sp, const CloudSet& fixed, const CloudSet& moving, const std::vector<Vector3f>& poses,
                             const lsm2d_select_params& select, int32_t k, const std::vector<int32_t>& fixed_index = {},
                             const std::vector<int32_t>& moving_index = {}) {
  const size_t n = poses.size();
  detail::checkIndexVectors("scoreSelect", detail::ONE_PER_POSE, fixed_index, moving_index, n);
  const size_t cap = (size_t) std::max<int32_t>(k, 1);
  detail::RowBuffer rows(cap);
  int32_t n_sel = 0; Selection out;
  out.index.resize(cap);
  check(lsm2d_score_select(ctx.get(), &sp, fixed.get(), ptrOrNull(fixed_index), moving.get(), ptrOrNull(moving_index), (int32_t) n, ptrOrNull(poses), &select, k,
                           out.index.data(), rows.H.data(), rows.b.data(), rows.stats.data(), &n_sel, &out.n_accepted),
        "lsm2d_score_select", ctx.get());
  out.index.resize((size_t) n_sel); out.rows = rows.rows<Linearization>((size_t) n_sel);
  return out;
}

// lsm2d_score_select's acceptance test on one item's statistics (fp32, IEEE division)
inline bool selectAccept(const lsm2d_iteration_stats& st, const lsm2d_select_params& p) {
  const float n_in = (float) st.n_inliers, n_c = (float) (st.n_correspondences > 1 ? st.n_correspondences : 1);
  return st.n_inliers >= p.min_inliers && st.chi_inliers / (n_in > 1.f ? n_in : 1.f) <= p.max_chi_per_inlier && n_in / n_c >= p.min_inlier_ratio;
}

// What both relocalize() add to their selection: the selected hypotheses aligned from their own poses (lsm2d_align_batch), row j for selection.index[j];
// last_stats[j] the statistics of the last iteration it started and accepted[j] whether the aligner succeeded and those pass the acceptance test.
struct AlignedSelection {
  std::vector<Vector3f> pose; std::vector<std::array<float, 9>> information; std::vector<int32_t> status, iterations;
  std::vector<lsm2d_iteration_stats> last_stats; std::vector<char> accepted;
};
namespace detail {
// the tail of both relocalize(): the selected items' poses and priors (their clouds come spelled out, `fi` / `mi`: NULL means "cloud i" only while the batch
// is the whole set), the aligner on them, each one's last started iteration, the acceptance test on it
inline void alignSelected(Context& ctx, const lsm2d_aligner_params& aligner, const lsm2d_slice_params* slices, std::vector<const lsm2d_cloudset*> fixed,
                          std::vector<const lsm2d_cloudset*> moving, const std::vector<int32_t>& selected, const std::vector<Vector3f>& poses,
                          const std::vector<lsm2d_prior>& priors, const std::vector<int32_t>& fi, const std::vector<int32_t>& mi,
                          const lsm2d_select_params& select, AlignedSelection& r) {
  const size_t m = selected.size();
  std::vector<Vector3f> x0(m); std::vector<lsm2d_prior> pr;
  for (size_t j = 0; j < m; ++j) { x0[j] = poses[(size_t) selected[j]]; if (!priors.empty()) pr.push_back(priors[(size_t) selected[j]]); }
  const BatchDescriptor d(m, slices, std::move(fixed), std::move(moving), ptrOrNull(x0), ptrOrNull(pr), ptrOrNull(fi), ptrOrNull(mi));
  const size_t cap = (size_t) lsm2d_stats_capacity(&aligner);
  std::vector<lsm2d_iteration_stats> st(m * cap);
  r.pose.resize(m); r.information.resize(m); r.status.resize(m); r.iterations.resize(m); r.last_stats.resize(m); r.accepted.resize(m);
  check(lsm2d_align_batch(ctx.get(), &aligner, &d.b, r.pose[0].data(), r.information[0].data(), r.status.data(), r.iterations.data(), st.data()),
        "lsm2d_align_batch", ctx.get());
  for (size_t j = 0; j < m; ++j) {
    const size_t it = (size_t) std::min<long>(std::max<long>((long) r.iterations[j] - 1, 0), (long) cap - 1);
    r.last_stats[j] = st[j * cap + it];
    r.accepted[j] = r.status[j] == LSM2D_SUCCESS && selectAccept(r.last_stats[j], select);
  }
}
}  // namespace detail

// The candidate loop of the relocaliser / loop detector (MULTI.json:749-769, :964-986) over poses.size() hypotheses of one laser slice: scoreSelect, then
// lsm2d_align_batch on the selected hypotheses from their own poses, then the acceptance test on the statistics of the last iteration each started.  Pure
// composition: the same as calling the two entry points by hand.
struct Relocalization : AlignedSelection { Selection selection; };
inline Relocalization relocalize(Context& ctx, const lsm2d_aligner_params& aligner, const lsm2d_slice_params& sp, const CloudSet& fixed, const CloudSet& moving,
                                 const std::vector<Vector3f>& poses, const lsm2d_select_params& select, int32_t k,
                                 const std::vector<int32_t>& fixed_index = {}, const std::vector<int32_t>& moving_index = {}) {
  Relocalization r;
  r.selection = scoreSelect(ctx, sp, fixed, moving, poses, select, k, fixed_index, moving_index);
  if (r.selection.index.empty()) return r;
  auto chosen = [&](const CloudSet& cs, const std::vector<int32_t>& idx) {
    std::vector<int32_t> out;
    if (idx.empty() && cs.numClouds() == 1) return out;
    for (int32_t i : r.selection.index) out.push_back(idx.empty() ? i : idx[(size_t) i]);
    return out;
  };
  const std::vector<int32_t> fi = chosen(fixed, fixed_index), mi = chosen(moving, moving_index);
  detail::alignSelected(ctx, aligner, &sp, {fixed.get()}, {moving.get()}, r.selection.index, poses, {}, fi, mi, select, r);
  return r;
}

// lsm2d_align_batch's alignment of init_pose.size() candidates, then the candidate loops' verdict made on the device (lsm2d_align_select): aligner
// succeeded, the last iteration started passes `select`, the best k of those ranked -- inliers descending, chi_inliers ascending, index ascending.  Only k
// rows come down: row j is what lsm2d_align_batch returns for candidate index[j], last_stats[j] its statistics row iterations - 1.  slices[s] reads
// fixed[s] / moving[s]; the index vectors are empty or [n_slices][n] flat and priors is empty or holds one per candidate, as lsm2d_batch takes them.
struct AlignSelection {
  std::vector<int32_t> index; std::vector<Vector3f> pose; std::vector<std::array<float, 9>> information; std::vector<int32_t> iterations;
  std::vector<lsm2d_iteration_stats> last_stats; int32_t n_accepted = 0, n_success = 0;
};
inline AlignSelection alignSelect(Context& ctx, const lsm2d_aligner_params& aligner, const std::vector<lsm2d_slice_params>& slices,
                                  const std::vector<const CloudSet*>& fixed, const std::vector<const CloudSet*>& moving, const std::vector<Vector3f>& init_pose,
                                  const lsm2d_select_params& select, int32_t k, const std::vector<lsm2d_prior>& priors = {},
                                  const std::vector<int32_t>& fixed_index = {}, const std::vector<int32_t>& moving_index = {}) {
  const size_t n = init_pose.size(), ns = slices.size();
  detail::checkSetsPerSlice("alignSelect", ns, fixed, moving);
  detail::checkIndexVectors("alignSelect", "an index vector is empty or [n_slices][n]; priors is empty or holds one per candidate", fixed_index, moving_index, ns * n,
                            detail::emptyOrHolds(priors, n));
  const detail::BatchDescriptor d(n, slices.data(), detail::handles(fixed), detail::handles(moving), ptrOrNull(init_pose), ptrOrNull(priors), ptrOrNull(fixed_index),
                                  ptrOrNull(moving_index));
  const size_t cap = (size_t) std::max<int32_t>(k, 1);
  AlignSelection out; int32_t n_sel = 0;
  out.index.resize(cap); out.pose.resize(cap); out.information.resize(cap); out.iterations.resize(cap); out.last_stats.resize(cap);
  static_assert(sizeof(Vector3f) == 3 * sizeof(float) && sizeof(std::array<float, 9>) == 9 * sizeof(float), "rows are packed");
  check(lsm2d_align_select(ctx.get(), &aligner, &d.b, &select, k, out.index.data(), out.pose[0].data(), out.information[0].data(), out.iterations.data(),
                           out.last_stats.data(), &n_sel, &out.n_accepted, &out.n_success),
        "lsm2d_align_select", ctx.get());
  out.index.resize((size_t) n_sel); out.pose.resize((size_t) n_sel); out.information.resize((size_t) n_sel); out.iterations.resize((size_t) n_sel);
  out.last_stats.resize((size_t) n_sel);
  return out;
}

// ---- pose hypotheses scored against a whole aligner: its slices with their sensor offsets and skip thresholds, an optional prior per hypothesis ----
// (lsm2d_score_aligner_batch / lsm2d_score_aligner_select).  slices[s] reads fixed[s] / moving[s]; the index vectors are empty or [n_slices][n] flat, as
// lsm2d_batch takes them; priors is empty or holds one per pose.  A row is what the first iteration of lsm2d_align_batch holds just before its solve;
// active counts the slices that contributed (0: zeros, the hypothesis the aligner would end with LSM2D_NOT_ENOUGH_CORRESPONDENCES).
struct AlignerSelection { std::vector<int32_t> index; std::vector<AlignerScore> rows; int32_t n_accepted = 0; };
inline std::vector<AlignerScore> scoreAligner(Context& ctx, const std::vector<lsm2d_slice_params>& slices, const std::vector<const CloudSet*>& fixed,
                                              const std::vector<const CloudSet*>& moving, const std::vector<Vector3f>& poses,
                                              const std::vector<lsm2d_prior>& priors = {}, const std::vector<int32_t>& fixed_index = {},
                                              const std::vector<int32_t>& moving_index = {}) {
  const detail::BatchDescriptor d = detail::alignerBatch("scoreAligner", slices, fixed, moving, poses, priors, fixed_index, moving_index);
  detail::RowBuffer rows(poses.size(), true);
  check(lsm2d_score_aligner_batch(ctx.get(), &d.b, rows.H.data(), rows.b.data(), rows.stats.data(), rows.active.data()), "lsm2d_score_aligner_batch", ctx.get());
  return rows.rows<AlignerScore>(poses.size());
}
// ... then the acceptance test and the best k accepted hypotheses ranked on the device, as scoreSelect ranks; a hypothesis with active == 0 is rejected
inline AlignerSelection scoreAlignerSelect(Context& ctx, const std::vector<lsm2d_slice_params>& slices, const std::vector<const CloudSet*>& fixed,
                                           const std::vector<const CloudSet*>& moving, const std::vector<Vector3f>& poses, const lsm2d_select_params& select,
                                           int32_t k, const std::vector<lsm2d_prior>& priors = {}, const std::vector<int32_t>& fixed_index = {},
                                           const std::vector<int32_t>& moving_index = {}) {
  const detail::BatchDescriptor d = detail::alignerBatch("scoreAlignerSelect", slices, fixed, moving, poses, priors, fixed_index, moving_index);
  const size_t cap = (size_t) std::max<int32_t>(k, 1);
  detail::RowBuffer rows(cap, true);
  int32_t n_sel = 0; AlignerSelection out;
  out.index.resize(cap);
  check(lsm2d_score_aligner_select(ctx.get(), &d.b, &select, k, out.index.data(), rows.H.data(), rows.b.data(), rows.stats.data(), rows.active.data(), &n_sel,
                                   &out.n_accepted),
        "lsm2d_score_aligner_select", ctx.get());
  out.index.resize((size_t) n_sel); out.rows = rows.rows<AlignerScore>((size_t) n_sel);
  return out;
}

// relocalize for the two-laser robot (MULTI.json:700-732: two WithSensor slices and the odometry prior; the relocaliser's own aligner is unset, :749-769,
// and falls back on it): scoreAlignerSelect, then lsm2d_align_batch on the selected hypotheses from their own poses with their own priors, then the
// acceptance test on the statistics of the last iteration each started.  Pure composition.
struct AlignerRelocalization : AlignedSelection { AlignerSelection selection; };
inline AlignerRelocalization relocalize(Context& ctx, const lsm2d_aligner_params& aligner, const std::vector<lsm2d_slice_params>& slices,
                                        const std::vector<const CloudSet*>& fixed, const std::vector<const CloudSet*>& moving,
                                        const std::vector<Vector3f>& poses, const lsm2d_select_params& select, int32_t k,
                                        const std::vector<lsm2d_prior>& priors = {}, const std::vector<int32_t>& fixed_index = {},
                                        const std::vector<int32_t>& moving_index = {}) {
  AlignerRelocalization r;
  r.selection = scoreAlignerSelect(ctx, slices, fixed, moving, poses, select, k, priors, fixed_index, moving_index);
  const size_t n = poses.size(), ns = slices.size();
  if (r.selection.index.empty()) return r;
  // (for every slice; not the one-slice relocalize's lambda, which asks a set for its number of clouds once: the calls a program makes stay what they were)
  auto chosen = [&](const std::vector<const CloudSet*>& sets, const std::vector<int32_t>& idx) {
    std::vector<int32_t> out;
    bool all_single = idx.empty();
    for (const CloudSet* cs : sets) all_single = all_single && cs->numClouds() == 1;
    if (all_single) return out;
    for (size_t s = 0; s < ns; ++s)
      for (int32_t i : r.selection.index) out.push_back(!idx.empty() ? idx[s * n + (size_t) i] : (sets[s]->numClouds() == 1 ? 0 : i));
    return out;
  };
  const std::vector<int32_t> fi = chosen(fixed, fixed_index), mi = chosen(moving, moving_index);
  detail::alignSelected(ctx, aligner, slices.data(), detail::handles(fixed), detail::handles(moving), r.selection.index, poses, priors, fi, mi, select, r);
  return r;
}

// what every finder class has: the two clouds (uploaded when set; the reference keeps raw pointers and a _fixed_changed_flag), the pose, where the pairs
// go, and the one lsm2d_find_correspondences call.  A finder kind adds its parameters, how many pairs to make room for and what it refuses.
class CorrespondenceFinderBase {
 public:
  void setFixed(const PointNormal2fVectorCloud* fixed) { _fixed.reset(fixed ? new CloudSet(_ctx, *fixed) : nullptr); }
  void setMoving(const PointNormal2fVectorCloud* moving) { _moving.reset(moving ? new CloudSet(_ctx, *moving) : nullptr); _n_moving = moving ? moving->size() : 0; }
  void setLocalMapInSensor(const Vector3f& pose) { _local_map_in_sensor = pose; }
  void setCorrespondences(CorrespondenceVector* c) { _correspondences = c; }
 protected:
  explicit CorrespondenceFinderBase(Context& ctx) : _ctx(ctx) {}
  // room for `capacity` pairs, then as many as were found (projective .cpp:49,76; kd .cpp:10; nn .cpp:60)
  void find(const lsm2d_slice_params& sp, size_t capacity) {
    _correspondences->resize(capacity);
    int32_t k = 0;
    check(lsm2d_find_correspondences(_ctx.get(), &sp, _fixed->get(), 0, _moving->get(), 0, _local_map_in_sensor.data(), _correspondences->data(),
                                     (int32_t) _correspondences->size(), &k),
          "lsm2d_find_correspondences", _ctx.get());
    _correspondences->resize((size_t) k);
  }
  Context& _ctx;
  std::unique_ptr<CloudSet> _fixed, _moving; size_t _n_moving = 0;
  Vector3f _local_map_in_sensor{{0.f, 0.f, 0.f}};
  CorrespondenceVector* _correspondences = nullptr;
};

class CorrespondenceFinderProjective2f : public CorrespondenceFinderBase {
 public:
  explicit CorrespondenceFinderProjective2f(Context& ctx) : CorrespondenceFinderBase(ctx) {}
  float param_point_distance = 0.5f;   // .h:16-20
  float param_normal_cos = 0.8f;       // .h:21
  PointNormal2fProjectorPolarPtr param_projector{new PointNormal2fProjectorPolar};

  lsm2d_slice_params sliceParams() const {
    lsm2d_slice_params sp{};
    sp.finder = LSM2D_FINDER_PROJECTIVE; sp.projector = param_projector->abi();
    sp.point_distance = param_point_distance; sp.normal_cos = param_normal_cos;
    return sp;
  }

  void compute() {
    if (!param_projector) throw std::runtime_error("CorrespondenceFinderProjective2f::compute| Missing Projector");
    if (!_fixed) throw std::runtime_error("CorrespondenceFinderProjective2f::compute| Missing fixed!");
    if (!_moving) throw std::runtime_error("CorrespondenceFinderProjective2f::compute| Missing moving!");
    if (!_correspondences) throw std::runtime_error("CorrespondenceFinderProjective2f::compute| Missing correspondences!");
    const lsm2d_slice_params sp = sliceParams();
    find(sp, (size_t) sp.projector.canvas_cols);
  }
  // compute() for a whole batch of (fixed, moving, pose) triples in one launch: see findCorrespondencesBatch
  std::vector<CorrespondenceVector> computeBatch(const CloudSet& fixed, const CloudSet& moving, const std::vector<Vector3f>& poses,
                                                 const std::vector<int32_t>& fixed_index = {}, const std::vector<int32_t>& moving_index = {}) {
    if (!param_projector) throw std::runtime_error("CorrespondenceFinderProjective2f::computeBatch| Missing Projector");
    return findCorrespondencesBatch(_ctx, sliceParams(), fixed, moving, poses, fixed_index, moving_index);
  }
};

// CorrespondenceFinderKDTree2D (registration/correspondence_finder_kd_tree_2d.{h,cpp}) and CorrespondenceFinderNN2D
// (registration/correspondence_finder_nn_2d.{h,cpp}): same surface, different lsm2d_finder.
class CorrespondenceFinderPointQuery : public CorrespondenceFinderBase {
 public:
  CorrespondenceFinderPointQuery(Context& ctx, int finder) : CorrespondenceFinderBase(ctx), _finder(finder) {}
  float param_max_distance_m = 1e-2f;   // kd .h:23 (nn .h:20-24 defaults to 1)
  float param_resolution = 5e-2f;       // nn .h:25-29
  float param_normal_cos = 0.8f;
  float param_max_leaf_range = 1e-2f;   // kd .h:26-28 -- honoured by LSM2D_FINDER_KDTREE (search "kdtree")
  unsigned param_min_leaf_points = 20;  // kd .h:29-33
  lsm2d_slice_params sliceParams() const {
    lsm2d_slice_params sp{};
    sp.finder = _finder; sp.projector = PointNormal2fProjectorPolar().abi();
    sp.max_distance = param_max_distance_m; sp.resolution = param_resolution; sp.normal_cos = param_normal_cos;
    sp.kd_max_leaf_range = param_max_leaf_range; sp.kd_min_leaf_points = (int32_t) param_min_leaf_points;
    return sp;
  }
  void compute() {
    refuseBadResolution();
    if (!_fixed || !_moving || !_correspondences) throw std::runtime_error("CorrespondenceFinder::compute| missing fixed, moving or correspondences");
    find(sliceParams(), _n_moving);
  }
  // compute() for a whole batch of (fixed, moving, pose) triples in one launch: see findCorrespondencesBatch
  std::vector<CorrespondenceVector> computeBatch(const CloudSet& fixed, const CloudSet& moving, const std::vector<Vector3f>& poses,
                                                 const std::vector<int32_t>& fixed_index = {}, const std::vector<int32_t>& moving_index = {}) {
    refuseBadResolution();
    return findCorrespondencesBatch(_ctx, sliceParams(), fixed, moving, poses, fixed_index, moving_index);
  }
 protected:
  int _finder;
 private:
  void refuseBadResolution() const {      // nn .cpp:11-14
    if (_finder == LSM2D_FINDER_DISTMAP && !(param_resolution > 0.f)) throw std::runtime_error("resolution must be > 0");
  }
};
// search "kdtree" (default): the reference's own tree and single-leaf descent (approximate, honours max_leaf_range / min_leaf_points);
// "exact": an exact nearest-neighbour search on a uniform grid (LSM2D_FINDER_NN), for which the two leaf parameters have no meaning
struct CorrespondenceFinderKDTree2D : CorrespondenceFinderPointQuery {
  explicit CorrespondenceFinderKDTree2D(Context& ctx, const std::string& search = "kdtree") : CorrespondenceFinderPointQuery(ctx, finderOf(search)) {}
  void setSearch(const std::string& search) { _finder = finderOf(search); }
  static int finderOf(const std::string& search) {
    if (search == "kdtree") return LSM2D_FINDER_KDTREE;
    if (search == "exact") return LSM2D_FINDER_NN;
    throw std::runtime_error("CorrespondenceFinderKDTree2D| search must be \"kdtree\" or \"exact\"");
  }
};
struct CorrespondenceFinderNN2D : CorrespondenceFinderPointQuery {
  explicit CorrespondenceFinderNN2D(Context& ctx) : CorrespondenceFinderPointQuery(ctx, LSM2D_FINDER_DISTMAP) { param_max_distance_m = 1.f; }
};

// a single growable device cloud: the tracker's local map / the clipped scene
class ReservedCloud {
 public:
  ReservedCloud(Context& ctx, int64_t capacity) : _ctx(ctx) { check(lsm2d_cloudset_create_reserved(ctx.get(), capacity, _h.out()), "lsm2d_cloudset_create_reserved", ctx.get()); }
  lsm2d_cloudset* get() const { return _h; }
  void upload(const PointNormal2fVectorCloud& c) { check(lsm2d_cloudset_upload(get(), ptrOrNull(c), (int64_t) c.size()), "lsm2d_cloudset_upload", _ctx.get()); }
  PointNormal2fVectorCloud download() const {
    PointNormal2fVectorCloud c((size_t) size()); int64_t n = 0;
    check(lsm2d_cloudset_download(get(), 0, c.empty() ? nullptr : &c[0].x, (int64_t) c.size(), &n), "lsm2d_cloudset_download", _ctx.get());
    c.resize((size_t) n); return c;
  }
  int64_t size() const { return lsm2d_cloudset_num_points(get()); }
 private:
  Context& _ctx; detail::CloudSetHandle _h;
};

// SceneClipperProjective2D (mapping/scene_clipper_projective_2d.{h,cpp})
class SceneClipperProjective2D {
 public:
  explicit SceneClipperProjective2D(Context& ctx) : _ctx(ctx) {}
  PointNormal2fProjectorPolarPtr param_projector{new PointNormal2fProjectorPolar};
  void setFullScene(const ReservedCloud* scene) { _scene = scene; }
  void setClippedSceneInRobot(ReservedCloud* clipped) { _clipped = clipped; }
  void setRobotInLocalMap(const Vector3f& p) { _robot_in_local_map = p; }
  void setSensorInRobot(const Vector3f& p) { _sensor_in_robot = p; }
  int compute() {
    if (!_scene || !_clipped) throw std::runtime_error("SceneClipperProjective2D::compute| missing local OR global scene");     // .cpp:12-17
    if (!param_projector) throw std::runtime_error("SceneClipperProjective2D::compute| Missing Projector");                     // .cpp:19-21
    const lsm2d_projector pr = param_projector->abi(); int32_t n = -1;
    // asynchronous: the call only queues the work; the clipped set's size stays on the device until somebody asks (returns -1)
    check(lsm2d_clip_scene_voxelized(_ctx.get(), &pr, _scene->get(), 0, _robot_in_local_map.data(), _sensor_in_robot.data(),
                                     param_voxelize_resolution, _clipped->get(), asynchronous ? nullptr : &n, nullptr),
          "lsm2d_clip_scene", _ctx.get());
    return n;
  }
  bool asynchronous = false;
  float param_voxelize_resolution = 0.1f;                                  // the class default (.h:21-25); both shipped configurations set 0 (MULTI.json:673-683); > 0: .cpp:36-48
 private:
  Context& _ctx; const ReservedCloud* _scene = nullptr; ReservedCloud* _clipped = nullptr;
  Vector3f _robot_in_local_map{{0.f, 0.f, 0.f}}, _sensor_in_robot{{0.f, 0.f, 0.f}};
};

// MergerProjective2D (mapping/merger_projective_2d.{h,cpp})
class MergerProjective2D {
 public:
  explicit MergerProjective2D(Context& ctx) : _ctx(ctx) {}
  float param_merge_threshold = 0.2f;                                      // .h:12-16
  PointNormal2fProjectorPolarPtr param_projector{new PointNormal2fProjectorPolar};
  void setScene(ReservedCloud* scene) { _scene = scene; }
  void setMeasurement(const PointNormal2fVectorCloud* m) { _measurement.reset(m ? new CloudSet(_ctx, *m) : nullptr); _device_measurement = nullptr; }
  void setMeasurement(const ReservedCloud* m) { _measurement.reset(); _device_measurement = m; }     // a measurement that already lives on the device
  void setMeasurementInScene(const Vector3f& p) { _measurement_in_scene = p; }
  int compute() {
    if (!param_projector) throw std::runtime_error("MergerProjective2D::compute| Missing Projector");                            // .cpp:10-12
    const lsm2d_cloudset* meas = _device_measurement ? _device_measurement->get() : (_measurement ? _measurement->get() : nullptr);
    if (!_scene || !meas) throw std::runtime_error("MergerProjective2D::compute| missing scene or measurement");
    const lsm2d_projector pr = param_projector->abi(); int32_t size = -1;
    // asynchronous: queue only; the scene's new size (and the counts) stay on the device (returns -1)
    check(lsm2d_merge_scene(_ctx.get(), &pr, _scene->get(), meas, 0, _measurement_in_scene.data(), param_merge_threshold,
                            asynchronous ? nullptr : &size, asynchronous ? nullptr : counts.data()),
          "lsm2d_merge_scene", _ctx.get());
    return size;
  }
  // several device-resident measurements, each at its own pose, in order: one call (one launch when everything is small)
  int computeAll(const std::vector<const ReservedCloud*>& measurements, const std::vector<Vector3f>& poses) {
    if (!param_projector) throw std::runtime_error("MergerProjective2D::compute| Missing Projector");
    if (!_scene || measurements.empty() || measurements.size() != poses.size()) throw std::runtime_error("MergerProjective2D::compute| missing scene or measurement");
    std::vector<const lsm2d_cloudset*> sets; std::vector<float> p;
    for (size_t k = 0; k < measurements.size(); ++k) { sets.push_back(measurements[k]->get()); p.insert(p.end(), poses[k].begin(), poses[k].end()); }
    const lsm2d_projector pr = param_projector->abi(); int32_t size = -1;
    check(lsm2d_merge_scenes(_ctx.get(), &pr, _scene->get(), (int32_t) sets.size(), sets.data(), nullptr, p.data(), param_merge_threshold,
                             asynchronous ? nullptr : &size, nullptr), "lsm2d_merge_scenes", _ctx.get());
    return size;
  }
  bool asynchronous = false;
  std::array<int32_t, 3> counts{{0, 0, 0}};                                // new, merged, replaced
 private:
  Context& _ctx; ReservedCloud* _scene = nullptr; std::unique_ptr<CloudSet> _measurement; const ReservedCloud* _device_measurement = nullptr;
  Vector3f _measurement_in_scene{{0.f, 0.f, 0.f}};
};

struct RobustifierCauchy { float param_chi_threshold = 0.01f; };     // MULTI.json:153-158

// AlignerSliceProcessorLaser2D[WithSensor] (registration/aligner_slice_processor_laser_2d.h:7-42; MULTI.json:160-188)
struct AlignerSliceProcessorLaser2D {
  std::string param_fixed_slice_name = "points", param_moving_slice_name = "points";
  int param_min_num_correspondences = 0;
  std::shared_ptr<CorrespondenceFinderProjective2f> param_finder;
  std::shared_ptr<RobustifierCauchy> param_robustifier;
  Vector3f sensor_in_robot{{0.f, 0.f, 0.f}};                           // WithSensor: from the tf Platform
  lsm2d_slice_params sliceParams() const {
    if (!param_finder) throw std::runtime_error("AlignerSliceProcessorLaser2D| Missing finder");
    lsm2d_slice_params sp = param_finder->sliceParams();
    sp.robustifier = param_robustifier ? LSM2D_ROBUST_CAUCHY : LSM2D_ROBUST_NONE;
    sp.chi_threshold = param_robustifier ? param_robustifier->param_chi_threshold : 0.f;
    sp.min_num_correspondences = param_min_num_correspondences;
    for (int i = 0; i < 3; ++i) sp.sensor_in_robot[i] = sensor_in_robot[i];
    return sp;
  }
};
using AlignerSliceProcessorLaser2DPtr = std::shared_ptr<AlignerSliceProcessorLaser2D>;

class MultiAligner2D {
 public:
  enum Status { Success = 0, NotEnoughCorrespondences = 1, NotEnoughInliers = 2, Fail = 3 };
  using PropertyContainer = std::map<std::string, const PointNormal2fVectorCloud*>;   // slice name -> cloud
  explicit MultiAligner2D(Context& ctx) : _ctx(ctx) {}
  int param_max_iterations = 10, param_min_num_inliers = 10;             // MULTI.json:711,714
  float param_damping = 0.f;                                             // MULTI.json:254-259
  // the options the shipped aligners carry at their defaults (MULTI.json:606-610,627-630); semantics in include/lsm2d.h (restated from the
  // parameters' doc strings: the upstream class is not in the reference tree); the termination criterion exists as an epsilon (lsm2d.h)
  bool param_enable_inlier_only_runs = false, param_keep_only_inlier_correspondences = false;
  bool store_correspondences = false;      // compute() also fetches what the reference leaves in slice->correspondences() (a finder pass per slice)
  float param_termination_chi_epsilon = 0.f;                             // 0 = "termination_criteria" not set = max_iterations
  std::vector<AlignerSliceProcessorLaser2DPtr> param_slice_processors;

  void setFixed(const PropertyContainer* f) { _fixed = f; }
  void setMoving(const PropertyContainer* m) { _moving = m; }
  void setMovingInFixed(const Vector3f& x) { _moving_in_fixed = x; }
  void setPrior(const Vector3f& z, const std::array<float, 9>& omega) { _has_prior = true; for (int i = 0; i < 3; ++i) _prior.z[i] = z[i]; for (int i = 0; i < 9; ++i) _prior.omega[i] = omega[i]; }

  void compute() {
    if (!_fixed || !_moving) throw std::runtime_error("MultiAligner2D::compute| fixed or moving not set");
    const int ns = (int) param_slice_processors.size();
    if (ns < 1) throw std::runtime_error("MultiAligner2D::compute| no slice processors");
    std::vector<lsm2d_slice_params> sp; std::vector<std::unique_ptr<CloudSet>> own;
    std::vector<const lsm2d_cloudset*> fx, mv;
    for (const auto& s : param_slice_processors) {
      sp.push_back(s->sliceParams());
      auto fi = _fixed->find(s->param_fixed_slice_name); auto mi = _moving->find(s->param_moving_slice_name);
      if (fi == _fixed->end() || mi == _moving->end() || !fi->second || !mi->second) throw std::runtime_error("MultiAligner2D::compute| slice cloud missing");
      own.emplace_back(new CloudSet(_ctx, *fi->second)); fx.push_back(own.back()->get());
      own.emplace_back(new CloudSet(_ctx, *mi->second)); mv.push_back(own.back()->get());
    }
    const detail::BatchDescriptor d(1, sp.data(), std::move(fx), std::move(mv), _moving_in_fixed.data(), _has_prior ? &_prior : nullptr);
    lsm2d_aligner_params ap{param_max_iterations, param_min_num_inliers, param_damping, param_termination_chi_epsilon,
                            param_enable_inlier_only_runs ? 1 : 0, param_keep_only_inlier_correspondences ? 1 : 0};
    _stats.assign((size_t) lsm2d_stats_capacity(&ap), lsm2d_iteration_stats{});
    int32_t st = 0, its = 0;
    _pairs.assign((size_t) ns, {});
    if (store_correspondences) {
      size_t cap = 1;
      for (int s = 0; s < ns; ++s) {
        const size_t need = sp[(size_t) s].finder == LSM2D_FINDER_PROJECTIVE ? (size_t) sp[(size_t) s].projector.canvas_cols : (size_t) lsm2d_cloudset_num_points(d.mv[(size_t) s]);
        cap = need > cap ? need : cap;
      }
      std::vector<lsm2d_correspondence> buf(cap * (size_t) ns); std::vector<int32_t> cnt((size_t) ns, 0);
      check(lsm2d_align_batch_pairs(_ctx.get(), &ap, &d.b, _moving_in_fixed.data(), _information.data(), &st, &its, _stats.data(), buf.data(), (int32_t) cap, cnt.data()),
            "lsm2d_align_batch_pairs", _ctx.get());
      for (int s = 0; s < ns; ++s) _pairs[(size_t) s].assign(buf.begin() + (long) (cap * (size_t) s), buf.begin() + (long) (cap * (size_t) s) + cnt[(size_t) s]);
    } else {
      check(lsm2d_align_batch(_ctx.get(), &ap, &d.b, _moving_in_fixed.data(), _information.data(), &st, &its, _stats.data()), "lsm2d_align_batch", _ctx.get());
    }
    _stats.resize((size_t) its); _status = st;
  }
  // slice->correspondences() after compute() (apps/visual_test_aligner_2d.cpp:129-143); needs store_correspondences
  const std::vector<lsm2d_correspondence>& correspondences(size_t slice = 0) const { return _pairs.at(slice); }
  const Vector3f& movingInFixed() const { return _moving_in_fixed; }
  const std::array<float, 9>& informationMatrix() const { return _information; }
  const std::vector<lsm2d_iteration_stats>& iterationStats() const { return _stats; }
  int status() const { return _status; }
 private:
  Context& _ctx;
  const PropertyContainer* _fixed = nullptr; const PropertyContainer* _moving = nullptr;
  Vector3f _moving_in_fixed{{0.f, 0.f, 0.f}};
  std::array<float, 9> _information{};
  std::vector<lsm2d_iteration_stats> _stats;
  std::vector<std::vector<lsm2d_correspondence>> _pairs;
  lsm2d_prior _prior{}; bool _has_prior = false; int _status = 0;
};

// Batches of FRESH LaserMessages against one device-resident map, pipelined: per incoming message RawDataPreprocessorProjective2D::compute
// (sensor_processing/raw_data_preprocessor_projective_2d.cpp:13-51) feeding MultiAligner2D::compute (apps/visual_test_aligner_2d.cpp:123-156), for n_scans
// messages per push().  THREE scan sets in rotation, the order include/lsm2d.h recommends at lsm2d_align_batch_begin:  push(k) begins batch k - 1 (whose scans
// were preprocessed by the previous push), refills a set with the ranges of batch k (lsm2d_preprocess_scans_refill: their preprocessing has the whole launch of
// batch k - 1 to hide under), and waits for batch k - 2.  It returns true when pose / information / status / iterations hold a finished batch's results --
// retired() says which push they belong to -- bit for bit those of lsm2d_preprocess_scans + lsm2d_align_batch on the same ranges.
// At the end of the sequence:  while (stream.flush()) { ...results of one more batch... }.
// The caller keeps a pushed `ranges` buffer untouched until the results of ITS batch have come out (pinned memory is fetched asynchronously).
class LaserMessageBatchStream {
 public:
  LaserMessageBatchStream(Context& ctx, const lsm2d_preprocessor& pre, const CloudSet& map, const lsm2d_slice_params& slice, const lsm2d_aligner_params& aligner, int n_scans)
      : _ctx(ctx), _pre(pre), _map(map), _slice(slice), _aligner(aligner), _n(n_scans) {
    if (n_scans < 1) throw std::runtime_error("LaserMessageBatchStream| n_scans < 1");
    pose.resize((size_t) n_scans); information.resize((size_t) n_scans); status.resize((size_t) n_scans); iterations.resize((size_t) n_scans);
    _start.resize((size_t) n_scans);
  }
  ~LaserMessageBatchStream() { try { while (flush()) {} } catch (...) {} }
  LaserMessageBatchStream(const LaserMessageBatchStream&) = delete; LaserMessageBatchStream& operator=(const LaserMessageBatchStream&) = delete;
  bool push(const float* ranges /* [n_scans][n_beams] */, const Vector3f* init_pose /* [n_scans] */) {
    if (_pushed > _begun) begin_next();                                   // batch k - 1: its scans are on the device (or on their way)
    if (!_sets[0])                                                        // the first push makes the three sets (allocation; nothing is in flight yet), every later one refills
      for (auto& s : _sets) check(lsm2d_preprocess_scans(_ctx.get(), &_pre, ranges, _n, s.out()), "lsm2d_preprocess_scans", _ctx.get());
    else                                                                  // (the set batch k - 3 read: retired by the previous push)
      check(lsm2d_preprocess_scans_refill(_ctx.get(), &_pre, ranges, _n, _sets[_pushed % 3]), "lsm2d_preprocess_scans_refill", _ctx.get());
    _start.assign(init_pose, init_pose + _n);
    ++_pushed;
    return _begun - _retired >= 2 ? retire() : false;                     // batch k - 2
  }
  bool flush() {                      // ONE more batch per call, oldest first; false when none is left
    if (_pushed > _begun) begin_next();
    return _begun > _retired ? retire() : false;
  }
  long retired() const { return _retired - 1; }                           // the push (0-based) whose results the members hold; -1: none yet
  std::vector<Vector3f> pose; std::vector<std::array<float, 9>> information; std::vector<int32_t> status, iterations;
 private:
  void begin_next() {      // (a plain descriptor on the stack: detail::BatchDescriptor would allocate its two handle arrays on every step)
    const lsm2d_cloudset* fx[1] = {_sets[_begun % 3]}; const lsm2d_cloudset* mv[1] = {_map.get()};
    lsm2d_batch b{}; b.n_alignments = _n; b.n_slices = 1; b.slices = &_slice; b.fixed = fx; b.moving = mv; b.init_pose = _start[0].data();
    check(lsm2d_align_batch_begin(_ctx.get(), &_aligner, &b, 0, &_pending[_begun & 1]), "lsm2d_align_batch_begin", _ctx.get());
    ++_begun;
  }
  bool retire() {
    lsm2d_pending* p = _pending[_retired & 1]; _pending[_retired & 1] = nullptr;     // wait() consumes the handle whatever it returns
    ++_retired;
    check(lsm2d_align_batch_wait(p, pose[0].data(), information[0].data(), status.data(), iterations.data(), nullptr), "lsm2d_align_batch_wait", _ctx.get());
    return true;
  }
  Context& _ctx; lsm2d_preprocessor _pre; const CloudSet& _map; lsm2d_slice_params _slice; lsm2d_aligner_params _aligner; int _n;
  detail::CloudSetHandle _sets[3]; lsm2d_pending* _pending[2] = {nullptr, nullptr};
  std::vector<Vector3f> _start;                                             // the start poses of the batch pushed last (begun by the next push)
  long _pushed = 0, _begun = 0, _retired = 0;
};

// The candidate loop of MultiLoopDetectorBruteForce2D / MultiRelocalizer2D (MULTI.json:964-986, :749-769) over the GPUs of one node,
// in this process: one context and one host thread per device, the submap replicated device to device, candidates block-sharded,
// results in candidate order (lsm2d_sweep_* in include/lsm2d.h).  accept() is the reference's acceptance test (MULTI.json:979-985).
class LoopClosureSweep {
 public:
  explicit LoopClosureSweep(const std::vector<int>& device_ids) {
    std::vector<int32_t> ids(device_ids.begin(), device_ids.end());
    const int rc = lsm2d_sweep_create(ids.data(), (int32_t) ids.size(), &_sw);
    if (rc < 0) throw std::runtime_error(std::string("LoopClosureSweep| ") + lsm2d_status_string(rc) + ": " + lsm2d_sweep_last_error(nullptr));
  }
  ~LoopClosureSweep() { lsm2d_sweep_destroy(_sw); }
  LoopClosureSweep(const LoopClosureSweep&) = delete; LoopClosureSweep& operator=(const LoopClosureSweep&) = delete;
  int numDevices() const { return lsm2d_sweep_num_devices(_sw); }
  // relocalize_aligner's parameters (MULTI.json:602-630) and its one laser slice (MULTI.json:572-600,771-784: projective finder,
  // point_distance 1.414, normal_cos 0.8, Cauchy 0.05, min_num_correspondences 10)
  int param_max_iterations = 30, param_min_num_inliers = 10;
  lsm2d_slice_params param_slice = projectiveSlice(PointNormal2fProjectorPolar(), 1.414f, 0.8f, 0.05f, 10);
  static lsm2d_slice_params projectiveSlice(const PointNormal2fProjectorPolar& projector, float point_distance, float normal_cos,
                                            float cauchy_chi_threshold /* <= 0: no robustifier */, int min_num_correspondences) {
    lsm2d_slice_params sp{};
    sp.finder = LSM2D_FINDER_PROJECTIVE; sp.projector = projector.abi(); sp.point_distance = point_distance; sp.normal_cos = normal_cos;
    sp.robustifier = cauchy_chi_threshold > 0.f ? LSM2D_ROBUST_CAUCHY : LSM2D_ROBUST_NONE; sp.chi_threshold = cauchy_chi_threshold > 0.f ? cauchy_chi_threshold : 0.f;
    sp.min_num_correspondences = min_num_correspondences;
    return sp;
  }
  // acceptance thresholds (MULTI.json:964-986)
  int param_relocalize_min_inliers = 500; float param_relocalize_max_chi_inliers = 0.1f, param_relocalize_min_inliers_ratio = 0.8f;

  void setMap(const PointNormal2fVectorCloud& map) { checkSweep(lsm2d_sweep_set_map(_sw, ptrOrNull(map), (int64_t) map.size()), "set_map"); }
  void setScans(const std::vector<PointNormal2fVectorCloud>& scans) {
    std::vector<float> packed; std::vector<int32_t> offs(1, 0);
    for (const auto& c : scans) { for (const auto& p : c) { packed.push_back(p.x); packed.push_back(p.y); packed.push_back(p.nx); packed.push_back(p.ny); } offs.push_back((int32_t) (packed.size() / 4)); }
    checkSweep(lsm2d_sweep_set_scans(_sw, packed.data(), offs.data(), (int32_t) scans.size()), "set_scans");
  }
  void setScansPacked(const float* xynn, const int32_t* offsets, int n_scans) { checkSweep(lsm2d_sweep_set_scans(_sw, xynn, offsets, n_scans), "set_scans"); }
  // candidates: (scan index, initial guess of moving-in-fixed); results in candidate order
  void compute(const std::vector<int32_t>& scan_index, const std::vector<Vector3f>& init_pose) {
    const lsm2d_aligner_params ap = alignerParams("LoopClosureSweep::compute| one scan index per candidate", scan_index, init_pose);
    const size_t n = init_pose.size();
    pose.assign(n, Vector3f{{0.f, 0.f, 0.f}}); information.assign(n, std::array<float, 9>{});
    status.assign(n, 0); iterations.assign(n, 0); last_stats.assign(n, lsm2d_iteration_stats{});
    static_assert(sizeof(Vector3f) == 3 * sizeof(float), "poses are packed");
    checkSweep(lsm2d_sweep_align(_sw, &ap, &param_slice, (int) n, scan_index.data(), ptrOrNull(init_pose), n ? pose[0].data() : nullptr,
                                 n ? information[0].data() : nullptr, status.data(), iterations.data(), last_stats.data()), "align");
  }
  bool accept(size_t i) const { return status[i] == LSM2D_SUCCESS && selectAccept(last_stats[i], selectParams()); }
  // compute + accept + "take the best k" on the devices (lsm2d_sweep_align_select): every shard ranks its candidates where they lie, k rows per shard come
  // down and are merged by the same key.  selected[j] is the j-th best accepted candidate (param_relocalize_* are the thresholds) and row j of pose /
  // information / iterations / last_stats its results -- the bits compute() gives for that candidate; status is left empty (every selected candidate
  // succeeded).  n_accepted / n_success count among all candidates.
  void computeSelect(const std::vector<int32_t>& scan_index, const std::vector<Vector3f>& init_pose, int32_t k) {
    const lsm2d_aligner_params ap = alignerParams("LoopClosureSweep::computeSelect| one scan index per candidate", scan_index, init_pose);
    const lsm2d_select_params sel = selectParams();
    const size_t cap = (size_t) std::max<int32_t>(k, 1);
    selected.assign(cap, 0); pose.assign(cap, Vector3f{{0.f, 0.f, 0.f}}); information.assign(cap, std::array<float, 9>{});
    status.clear(); iterations.assign(cap, 0); last_stats.assign(cap, lsm2d_iteration_stats{});
    int32_t n_sel = 0; n_accepted = 0; n_success = 0;
    checkSweep(lsm2d_sweep_align_select(_sw, &ap, &param_slice, (int) init_pose.size(), scan_index.data(), ptrOrNull(init_pose), &sel, k, selected.data(),
                                        pose[0].data(), information[0].data(), iterations.data(), last_stats.data(), &n_sel, &n_accepted, &n_success), "align_select");
    selected.resize((size_t) n_sel); pose.resize((size_t) n_sel); information.resize((size_t) n_sel); iterations.resize((size_t) n_sel);
    last_stats.resize((size_t) n_sel);
  }
  std::vector<Vector3f> pose; std::vector<std::array<float, 9>> information;
  std::vector<int32_t> status, iterations; std::vector<lsm2d_iteration_stats> last_stats;
  std::vector<int32_t> selected; int32_t n_accepted = 0, n_success = 0;      // computeSelect
 private:
  // what both candidate calls start from: one scan index per candidate, and the aligner the parameters describe
  lsm2d_aligner_params alignerParams(const char* refusal, const std::vector<int32_t>& scan_index, const std::vector<Vector3f>& init_pose) const {
    if (scan_index.size() != init_pose.size()) throw std::runtime_error(refusal);
    return {param_max_iterations, param_min_num_inliers, 0.f, 0.f, 0, 0};
  }
  lsm2d_select_params selectParams() const { return {param_relocalize_min_inliers, param_relocalize_max_chi_inliers, param_relocalize_min_inliers_ratio}; }
  void checkSweep(int rc, const char* where) const {
    if (rc < 0) throw std::runtime_error(std::string("LoopClosureSweep::") + where + "| " + lsm2d_status_string(rc) + ": " + lsm2d_sweep_last_error(_sw));
  }
  lsm2d_sweep* _sw = nullptr;
};

// N independent live trackers with one robot model (MULTI.json:464-482 for each of them): clip the local map around the odometry guess, align the
// front and the rear scan (two projective slices with their sensor offsets) with the odometry prior, merge both scans at the corrected pose --
// one call of each batched entry point per step, ONE wait (the aligner's poses).  Poses compose in double on the host, per tracker.
class TrackerBatch {
 public:
  struct Params {
    lsm2d_projector projector{721, -(float) M_PI, (float) M_PI, 0.3f, 20.0f, 0.0f};
    lsm2d_preprocessor preprocessor{721, -2.34747f, 2.35619f, 0.3f, 20.0f, 0.3f, 5, 0.02f};
    std::array<lsm2d_slice_params, 2> slices{};          // front, rear: projective, sensor_in_robot set (the first one's is also the clip's)
    lsm2d_aligner_params aligner{10, 10, 0.0f, 0.0f, 0, 0};
    std::array<float, 9> prior_omega{{100, 0, 0, 0, 100, 0, 0, 0, 100}};
    float merge_threshold = 0.2f;
    int64_t map_capacity = 50000;
    float clip_voxelize_resolution = 0.0f;               // > 0: the clipper voxelises what it clipped (scene_clipper_projective_2d.cpp:36-48; the class default is 0.1)
  };
  TrackerBatch(Context& ctx, int32_t n_trackers, const Params& p) : _ctx(ctx), _n(n_trackers), _p(p), _est((size_t) n_trackers * 3, 0.0),
                                                                       _prior((size_t) n_trackers), _x((size_t) n_trackers * 3), _H((size_t) n_trackers * 9),
                                                                       _status((size_t) n_trackers) {
    check(lsm2d_cloudset_create_reserved_many(ctx.get(), _n, p.map_capacity, _maps.out()), "lsm2d_cloudset_create_reserved_many", ctx.get());
    check(lsm2d_cloudset_create_reserved_many(ctx.get(), _n, p.projector.canvas_cols, _clipped.out()), "lsm2d_cloudset_create_reserved_many", ctx.get());
    for (auto& q : _prior) { for (float& z : q.z) z = 0.0f; for (int k = 0; k < 9; ++k) q.omega[k] = p.prior_omega[(size_t) k]; }
  }
  TrackerBatch(const TrackerBatch&) = delete; TrackerBatch& operator=(const TrackerBatch&) = delete;
  int32_t size() const { return _n; }
  // trackers idx[0 .. m) start a new local map at robot pose poses[m][3] from their scans front / rear [m][n_beams]
  void reset(int32_t m, const int32_t* idx, const float* front, const float* rear, const double* poses) {
    detail::CloudSetHandle meas[2];       // (they go when reset() returns or throws: by then the merge has read them)
    const float* r[2] = {front, rear};
    for (int s = 0; s < 2; ++s) check(lsm2d_preprocess_scans(_ctx.get(), &_p.preprocessor, r[s], m, meas[s].out()), "lsm2d_preprocess_scans", _ctx.get());
    std::vector<float> mis((size_t) m * 6);
    for (int32_t i = 0; i < m; ++i) { std::copy(poses + 3 * i, poses + 3 * i + 3, &_est[(size_t) idx[i] * 3]); sensorPoses(idx[i], &mis[(size_t) i * 6]); }
    int rc = lsm2d_cloudset_clear_clouds(_maps, m, idx);
    const lsm2d_cloudset* ms[2] = {meas[0], meas[1]};
    if (rc == LSM2D_SUCCESS) rc = lsm2d_merge_scene_batch(_ctx.get(), &_p.projector, _maps, m, idx, 2, ms, nullptr, mis.data(), _p.merge_threshold, nullptr, nullptr);
    if (rc == LSM2D_SUCCESS) rc = lsm2d_synchronize(_ctx.get());
    check(rc, "TrackerBatch::reset", _ctx.get());
  }
  // one step of every tracker: front / rear [N][n_beams] raw ranges (kept untouched until step() returns), odometry [N][3]
  void step(const float* front, const float* rear, const double* odometry) {
    const float* r[2] = {front, rear};
    for (int s = 0; s < 2; ++s) {
      if (!_scans[s]) check(lsm2d_preprocess_scans(_ctx.get(), &_p.preprocessor, r[s], _n, _scans[s].out()), "lsm2d_preprocess_scans", _ctx.get());
      else check(lsm2d_preprocess_scans_refill(_ctx.get(), &_p.preprocessor, r[s], _n, _scans[s]), "lsm2d_preprocess_scans_refill", _ctx.get());
    }
    std::vector<float> guess((size_t) _n * 3), x0((size_t) _n * 3, 0.0f), mis((size_t) _n * 6);
    for (int32_t i = 0; i < _n; ++i) { double g[3]; compose(&_est[(size_t) i * 3], odometry + 3 * i, g); for (int c = 0; c < 3; ++c) guess[(size_t) i * 3 + c] = (float) g[c]; }
    if (_p.clip_voxelize_resolution > 0.0f)
      check(lsm2d_clip_scene_voxelized_batch(_ctx.get(), &_p.projector, _maps, _n, nullptr, guess.data(), _p.slices[0].sensor_in_robot, _p.clip_voxelize_resolution, _clipped, nullptr),
            "lsm2d_clip_scene_voxelized_batch", _ctx.get());
    else
      check(lsm2d_clip_scene_batch(_ctx.get(), &_p.projector, _maps, _n, nullptr, guess.data(), _p.slices[0].sensor_in_robot, _clipped, nullptr), "lsm2d_clip_scene_batch", _ctx.get());
    const lsm2d_cloudset* fx[2] = {_scans[0], _scans[1]}; const lsm2d_cloudset* mv[2] = {_clipped, _clipped};
    lsm2d_batch b{};      // (on the stack, as in the stream: detail::BatchDescriptor would add two allocations to the three above)
    b.n_alignments = _n; b.n_slices = 2; b.slices = _p.slices.data(); b.fixed = fx; b.moving = mv; b.init_pose = x0.data(); b.prior = _prior.data();
    check(lsm2d_align_batch(_ctx.get(), &_p.aligner, &b, _x.data(), _H.data(), _status.data(), nullptr, nullptr), "lsm2d_align_batch", _ctx.get());
    for (int32_t i = 0; i < _n; ++i) {          // estimate = guess * x^-1, then both scans at the corrected pose
      const double xd[3] = {_x[(size_t) i * 3], _x[(size_t) i * 3 + 1], _x[(size_t) i * 3 + 2]}, gd[3] = {guess[(size_t) i * 3], guess[(size_t) i * 3 + 1], guess[(size_t) i * 3 + 2]};
      double xi[3]; inverse(xd, xi); compose(gd, xi, &_est[(size_t) i * 3]); sensorPoses(i, &mis[(size_t) i * 6]);
    }
    check(lsm2d_merge_scene_batch(_ctx.get(), &_p.projector, _maps, _n, nullptr, 2, fx, nullptr, mis.data(), _p.merge_threshold, nullptr, nullptr), "lsm2d_merge_scene_batch", _ctx.get());
  }
  const std::vector<float>& movingInFixed() const { return _x; }         // [N][3]: the aligner's result of the last step
  const std::vector<float>& informationMatrix() const { return _H; }     // [N][9]
  const std::vector<int32_t>& status() const { return _status; }         // [N]
  const std::vector<double>& robotInLocalMap() const { return _est; }    // [N][3]: every tracker's corrected pose
  lsm2d_cloudset* localMaps() const { return _maps; }
  lsm2d_cloudset* clippedScenes() const { return _clipped; }
 private:
  static void compose(const double a[3], const double b[3], double o[3]) {
    const double c = std::cos(a[2]), s = std::sin(a[2]);
    // the angle is brought back into [-pi, pi) with the operations of api.TrackerBatch's composition (synth.compose_poses: a floored modulo), so that
    // both classes hand the same float32 guesses and sensor poses to the library
    double th = std::fmod(a[2] + b[2] + M_PI, 2.0 * M_PI); if (th < 0.0) th += 2.0 * M_PI;
    o[0] = a[0] + c * b[0] - s * b[1]; o[1] = a[1] + s * b[0] + c * b[1]; o[2] = th - M_PI;
  }
  static void inverse(const double a[3], double o[3]) {
    const double c = std::cos(a[2]), s = std::sin(a[2]);
    o[0] = -(c * a[0] + s * a[1]); o[1] = -(-s * a[0] + c * a[1]); o[2] = -a[2];
  }
  void sensorPoses(int32_t i, float* out) const {
    for (int s = 0; s < 2; ++s) {
      const double S[3] = {_p.slices[(size_t) s].sensor_in_robot[0], _p.slices[(size_t) s].sensor_in_robot[1], _p.slices[(size_t) s].sensor_in_robot[2]};
      double m[3]; compose(&_est[(size_t) i * 3], S, m); for (int c = 0; c < 3; ++c) out[3 * s + c] = (float) m[c];
    }
  }
  Context& _ctx; int32_t _n; Params _p;
  std::vector<double> _est; std::vector<lsm2d_prior> _prior;
  std::vector<float> _x, _H; std::vector<int32_t> _status;
  detail::CloudSetHandle _maps, _clipped, _scans[2];
};

}  // namespace lsm2d_host
