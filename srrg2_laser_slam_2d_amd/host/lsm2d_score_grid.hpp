// lsm2d_score_grid.hpp -- a grid of pose hypotheses scored coarse to fine on the device over the C ABI (include/lsm2d.h, 0.7.10): scoreGridSelect and
// relocalizeGrid.  An extension of lsm2d.hpp (which it includes and whose types it returns).  The hypotheses are made on the device from a lsm2d_pose_grid;
// every level is scoreAlignerSelect's scoring and selection, a level's selection becomes the next level's hypotheses without leaving the device; one copy
// down, one wait, no upload of hypotheses.  NOT upstream (the reference does not say how its relocaliser chooses hypotheses) and NOT the exhaustive fine grid:
// the search finds that grid's winner only if its coarse cell is among the parents kept.
#pragma once

#include "lsm2d.hpp"

namespace lsm2d_host {

// row j is the j-th best hypothesis of the LAST level: pose[j] the pose it was scored at, origin[j] the level-0 cell it descends from, rows[j] what
// scoreAlignerSelect returns for it; level_counts[l] = {accepted, selected} of level l.  Pads (slots of parents that were not selected) are never in any of it.
struct GridSelection {
  std::vector<Vector3f> pose; std::vector<int32_t> origin; std::vector<AlignerScore> rows; int32_t n_accepted = 0;
  std::vector<std::array<int32_t, 2>> level_counts;
};

// slices[s] reads cloud fixed_cloud[s] of fixed[s] and cloud moving_cloud[s] of moving[s] for every hypothesis (an empty vector: cloud 0).  coarse_select
// judges the levels below the last (may be NULL when grid.n_levels == 1), select and k the last.
inline GridSelection scoreGridSelect(Context& ctx, const std::vector<lsm2d_slice_params>& slices, const std::vector<const CloudSet*>& fixed,
                                     const std::vector<const CloudSet*>& moving, const lsm2d_pose_grid& grid, const lsm2d_select_params* coarse_select,
                                     const lsm2d_select_params& select, int32_t k, const std::vector<int32_t>& fixed_cloud = {},
                                     const std::vector<int32_t>& moving_cloud = {}) {
  const size_t ns = slices.size();
  detail::checkSetsPerSlice("scoreGridSelect", ns, fixed, moving);
  detail::checkIndexVectors("scoreGridSelect", "a cloud vector is empty or holds one entry per slice", fixed_cloud, moving_cloud, ns);
  const std::vector<const lsm2d_cloudset*> fx = detail::handles(fixed), mv = detail::handles(moving);
  const size_t cap = (size_t) std::max<int32_t>(k, 1), levels = (size_t) std::max<int32_t>(grid.n_levels, 1);
  detail::RowBuffer rows(cap, true);
  GridSelection out; int32_t n_sel = 0;
  out.pose.resize(cap); out.origin.resize(cap); out.level_counts.assign(levels, std::array<int32_t, 2>{{0, 0}});
  static_assert(sizeof(Vector3f) == 3 * sizeof(float) && sizeof(std::array<int32_t, 2>) == 2 * sizeof(int32_t), "rows are packed");
  check(lsm2d_score_grid_select(ctx.get(), (int32_t) ns, slices.data(), fx.data(), ptrOrNull(fixed_cloud), mv.data(), ptrOrNull(moving_cloud), &grid, coarse_select,
                                &select, k, out.pose[0].data(), out.origin.data(), rows.H.data(), rows.b.data(), rows.stats.data(), rows.active.data(), &n_sel,
                                &out.n_accepted, out.level_counts[0].data()),
        "lsm2d_score_grid_select", ctx.get());
  out.pose.resize((size_t) n_sel); out.origin.resize((size_t) n_sel); out.rows = rows.rows<AlignerScore>((size_t) n_sel);
  return out;
}

// The relocaliser's candidate loop over a pose grid: scoreGridSelect(..., k_score), then the existing alignSelect from the returned poses (align_select NULL:
// `select` judges the aligned candidates too).  TWO calls and TWO waits, on purpose: chaining the aligned stage behind the scoring on the device was
// measured at 0.4 % in 0.7.9 (relocalizeSelect).  aligned.index points into scored.  Where the grid search selects nothing, no alignment is run.
struct GridRelocalization { GridSelection scored; AlignSelection aligned; };
inline GridRelocalization relocalizeGrid(Context& ctx, const lsm2d_aligner_params& aligner, const std::vector<lsm2d_slice_params>& slices,
                                         const std::vector<const CloudSet*>& fixed, const std::vector<const CloudSet*>& moving, const lsm2d_pose_grid& grid,
                                         const lsm2d_select_params* coarse_select, const lsm2d_select_params& select, int32_t k_score,
                                         const lsm2d_select_params* align_select, int32_t k, const std::vector<int32_t>& fixed_cloud = {},
                                         const std::vector<int32_t>& moving_cloud = {}) {
  GridRelocalization out;
  out.scored = scoreGridSelect(ctx, slices, fixed, moving, grid, coarse_select, select, k_score, fixed_cloud, moving_cloud);
  const size_t m = out.scored.pose.size(), ns = slices.size();
  if (m == 0) return out;
  // every candidate's cloud in every slice, spelled out: [n_slices][m]
  std::vector<int32_t> fi(ns * m, 0), mi(ns * m, 0);
  for (size_t s = 0; s < ns; ++s)
    for (size_t j = 0; j < m; ++j) { fi[s * m + j] = fixed_cloud.empty() ? 0 : fixed_cloud[s]; mi[s * m + j] = moving_cloud.empty() ? 0 : moving_cloud[s]; }
  out.aligned = alignSelect(ctx, aligner, slices, fixed, moving, out.scored.pose, align_select ? *align_select : select, k, {}, fi, mi);
  return out;
}

}  // namespace lsm2d_host
