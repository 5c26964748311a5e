// lsm2d_grouped.hpp -- the select calls PER GROUP of a batch over the C ABI (include/lsm2d.h, 0.7.8): scoreSelectGrouped, scoreAlignerSelectGrouped,
// alignSelectGrouped.  An extension of lsm2d.hpp (which it includes and whose types it returns): a fleet server lays its N robots' candidates one robot
// behind the other in one batch, group_offsets[g] .. group_offsets[g + 1] being robot g's, and gets every robot's own verdict -- what the ungrouped call
// returns for that robot's candidates alone, with BATCH indices -- from one call with one copy down and one wait.
#pragma once

#include "lsm2d.hpp"

namespace lsm2d_host {

namespace detail {
// group_offsets as the calls take it: at least one group (the calls check the rest and name what is wrong)
inline size_t groupCount(const char* who, const std::vector<int32_t>& group_offsets) {
  if (group_offsets.size() < 2) throw std::runtime_error(std::string(who) + "| group_offsets holds n_groups + 1 entries, n_groups >= 1");
  return group_offsets.size() - 1;
}
inline size_t groupedRows(size_t n_groups, int32_t k) { return n_groups * (size_t) std::max<int32_t>(k, 1); }
}  // namespace detail

// scoreSelect per group (lsm2d_score_select_grouped): entry g is the Selection scoreSelect returns for hypotheses group_offsets[g] .. group_offsets[g + 1]
// alone -- its best k, its accepted count -- with batch indices.
inline std::vector<Selection> scoreSelectGrouped(Context& ctx, const lsm2d_slice_params& sp, const CloudSet& fixed, const CloudSet& moving,
                                                 const std::vector<Vector3f>& poses, const std::vector<int32_t>& group_offsets,
                                                 const lsm2d_select_params& select, int32_t k, const std::vector<int32_t>& fixed_index = {},
                                                 const std::vector<int32_t>& moving_index = {}) {
  const size_t n = poses.size(), G = detail::groupCount("scoreSelectGrouped", group_offsets), K = (size_t) std::max<int32_t>(k, 1);
  detail::checkIndexVectors("scoreSelectGrouped", detail::ONE_PER_POSE, fixed_index, moving_index, n);
  detail::RowBuffer rows(detail::groupedRows(G, k));
  std::vector<int32_t> index(detail::groupedRows(G, k)), n_sel(G, 0), n_acc(G, 0);
  check(lsm2d_score_select_grouped(ctx.get(), &sp, fixed.get(), detail::ptrOrNull(fixed_index), moving.get(), detail::ptrOrNull(moving_index), (int32_t) n,
                                   detail::ptrOrNull(poses), &select, k, (int32_t) G, group_offsets.data(), index.data(), rows.H.data(), rows.b.data(),
                                   rows.stats.data(), n_sel.data(), n_acc.data()),
        "lsm2d_score_select_grouped", ctx.get());
  std::vector<Selection> out(G);
  for (size_t g = 0; g < G; ++g) {
    const size_t m = (size_t) n_sel[g];
    out[g].n_accepted = n_acc[g];
    out[g].index.assign(index.begin() + (ptrdiff_t) (g * K), index.begin() + (ptrdiff_t) (g * K + m));
    out[g].rows.resize(m);
    for (size_t j = 0; j < m; ++j) rows.fill(out[g].rows[j], g * K + j);
  }
  return out;
}

// scoreAlignerSelect per group (lsm2d_score_aligner_select_grouped)
inline std::vector<AlignerSelection> scoreAlignerSelectGrouped(Context& ctx, const std::vector<lsm2d_slice_params>& slices, const std::vector<const CloudSet*>& fixed,
                                                               const std::vector<const CloudSet*>& moving, const std::vector<Vector3f>& poses,
                                                               const std::vector<int32_t>& group_offsets, const lsm2d_select_params& select, int32_t k,
                                                               const std::vector<lsm2d_prior>& priors = {}, const std::vector<int32_t>& fixed_index = {},
                                                               const std::vector<int32_t>& moving_index = {}) {
  const size_t G = detail::groupCount("scoreAlignerSelectGrouped", group_offsets), K = (size_t) std::max<int32_t>(k, 1);
  const detail::BatchDescriptor d = detail::alignerBatch("scoreAlignerSelectGrouped", slices, fixed, moving, poses, priors, fixed_index, moving_index);
  detail::RowBuffer rows(detail::groupedRows(G, k), true);
  std::vector<int32_t> index(detail::groupedRows(G, k)), n_sel(G, 0), n_acc(G, 0);
  check(lsm2d_score_aligner_select_grouped(ctx.get(), &d.b, &select, k, (int32_t) G, group_offsets.data(), index.data(), rows.H.data(), rows.b.data(),
                                           rows.stats.data(), rows.active.data(), n_sel.data(), n_acc.data()),
        "lsm2d_score_aligner_select_grouped", ctx.get());
  std::vector<AlignerSelection> out(G);
  for (size_t g = 0; g < G; ++g) {
    const size_t m = (size_t) n_sel[g];
    out[g].n_accepted = n_acc[g];
    out[g].index.assign(index.begin() + (ptrdiff_t) (g * K), index.begin() + (ptrdiff_t) (g * K + m));
    out[g].rows.resize(m);
    for (size_t j = 0; j < m; ++j) rows.fill(out[g].rows[j], g * K + j);
  }
  return out;
}

// alignSelect per group (lsm2d_align_select_grouped): the fleet's loop-closure verdict, entry g robot g's AlignSelection with batch indices
inline std::vector<AlignSelection> alignSelectGrouped(Context& ctx, const lsm2d_aligner_params& aligner, const std::vector<lsm2d_slice_params>& slices,
                                                      const std::vector<const CloudSet*>& fixed, const std::vector<const CloudSet*>& moving,
                                                      const std::vector<Vector3f>& init_pose, const std::vector<int32_t>& group_offsets,
                                                      const lsm2d_select_params& select, int32_t k, const std::vector<lsm2d_prior>& priors = {},
                                                      const std::vector<int32_t>& fixed_index = {}, const std::vector<int32_t>& moving_index = {}) {
  const size_t n = init_pose.size(), ns = slices.size(), G = detail::groupCount("alignSelectGrouped", group_offsets), K = (size_t) std::max<int32_t>(k, 1);
  detail::checkSetsPerSlice("alignSelectGrouped", ns, fixed, moving);
  detail::checkIndexVectors("alignSelectGrouped", "an index vector is empty or [n_slices][n]; priors is empty or holds one per candidate", fixed_index, moving_index,
                            ns * n, detail::emptyOrHolds(priors, n));
  const detail::BatchDescriptor d(n, slices.data(), detail::handles(fixed), detail::handles(moving), detail::ptrOrNull(init_pose), detail::ptrOrNull(priors),
                                  detail::ptrOrNull(fixed_index), detail::ptrOrNull(moving_index));
  const size_t cap = detail::groupedRows(G, k);
  std::vector<int32_t> index(cap), its(cap), n_sel(G, 0), n_acc(G, 0), n_suc(G, 0);
  std::vector<Vector3f> pose(cap); std::vector<std::array<float, 9>> H(cap); std::vector<lsm2d_iteration_stats> last(cap);
  check(lsm2d_align_select_grouped(ctx.get(), &aligner, &d.b, &select, k, (int32_t) G, group_offsets.data(), index.data(), pose[0].data(), H[0].data(), its.data(),
                                   last.data(), n_sel.data(), n_acc.data(), n_suc.data()),
        "lsm2d_align_select_grouped", ctx.get());
  std::vector<AlignSelection> out(G);
  for (size_t g = 0; g < G; ++g) {
    const ptrdiff_t lo = (ptrdiff_t) (g * K), hi = lo + (ptrdiff_t) n_sel[g];
    AlignSelection& r = out[g];
    r.n_accepted = n_acc[g]; r.n_success = n_suc[g];
    r.index.assign(index.begin() + lo, index.begin() + hi); r.pose.assign(pose.begin() + lo, pose.begin() + hi);
    r.information.assign(H.begin() + lo, H.begin() + hi); r.iterations.assign(its.begin() + lo, its.begin() + hi);
    r.last_stats.assign(last.begin() + lo, last.begin() + hi);
  }
  return out;
}

}  // namespace lsm2d_host
