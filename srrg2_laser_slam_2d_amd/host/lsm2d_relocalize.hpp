// lsm2d_relocalize.hpp -- the relocaliser / loop detector's candidate loop in ONE call over the C ABI (include/lsm2d.h, 0.7.9): relocalizeSelect.  An
// extension of lsm2d.hpp (which it includes and whose types it returns).  lsm2d.hpp's relocalize() composes two calls with the host in the middle --
// scoreAlignerSelect, a gather of the selected hypotheses, lsm2d_align_batch; here the selection stays on the device, the aligner's inputs are written there,
// and both stages' answers come down in one copy after one wait (MULTI.json:749-769, :964-986).
#pragma once

#include "lsm2d.hpp"

namespace lsm2d_host {

// scored: what scoreAlignerSelect(..., score_select, k_score) returns but for the rows' H and b (index, statistics, n_accepted; rows[j].row.stats is filled,
// the other members of a row are zeros).  aligned: what alignSelect(..., align_select, k) returns for the scored.index.size() selected hypotheses, each
// started from its own pose with its own prior and clouds -- with index holding BATCH indices (hypothesis numbers), not positions in the selection.
struct RelocalizeSelection { AlignerSelection scored; AlignSelection aligned; };

// slices[s] reads fixed[s] / moving[s]; the index vectors are empty or [n_slices][n] flat and priors is empty or holds one per hypothesis, as lsm2d_batch
// takes them.  align_select NULL: score_select's thresholds judge the aligned hypotheses as well.  The aligner always runs k_score alignments -- slots for
// which nothing was selected repeat a selected hypothesis and are never returned -- so where mostly nothing passes the scoring, relocalize() is cheaper.
inline RelocalizeSelection relocalizeSelect(Context& ctx, const lsm2d_aligner_params& aligner, const std::vector<lsm2d_slice_params>& slices,
                                            const std::vector<const CloudSet*>& fixed, const std::vector<const CloudSet*>& moving,
                                            const std::vector<Vector3f>& poses, const lsm2d_select_params& score_select, int32_t k_score,
                                            const lsm2d_select_params* align_select, int32_t k, const std::vector<lsm2d_prior>& priors = {},
                                            const std::vector<int32_t>& fixed_index = {}, const std::vector<int32_t>& moving_index = {}) {
  const detail::BatchDescriptor d = detail::alignerBatch("relocalizeSelect", slices, fixed, moving, poses, priors, fixed_index, moving_index);
  const size_t cap1 = (size_t) std::max<int32_t>(k_score, 1), cap2 = (size_t) std::max<int32_t>(k, 1);
  RelocalizeSelection out;
  std::vector<lsm2d_iteration_stats> scored_stats(cap1);
  int32_t n_scored = 0, n_sel = 0;
  out.scored.index.resize(cap1);
  AlignSelection& a = out.aligned;
  a.index.resize(cap2); a.pose.resize(cap2); a.information.resize(cap2); a.iterations.resize(cap2); a.last_stats.resize(cap2);
  static_assert(sizeof(Vector3f) == 3 * sizeof(float) && sizeof(std::array<float, 9>) == 9 * sizeof(float), "rows are packed");
  check(lsm2d_relocalize_select(ctx.get(), &aligner, &d.b, &score_select, k_score, align_select, k, out.scored.index.data(), scored_stats.data(), &n_scored,
                                &out.scored.n_accepted, a.index.data(), a.pose[0].data(), a.information[0].data(), a.iterations.data(), a.last_stats.data(),
                                &n_sel, &a.n_accepted, &a.n_success),
        "lsm2d_relocalize_select", ctx.get());
  out.scored.index.resize((size_t) n_scored); out.scored.rows.resize((size_t) n_scored);
  for (size_t j = 0; j < (size_t) n_scored; ++j) out.scored.rows[j].row.stats = scored_stats[j];
  a.index.resize((size_t) n_sel); a.pose.resize((size_t) n_sel); a.information.resize((size_t) n_sel); a.iterations.resize((size_t) n_sel);
  a.last_stats.resize((size_t) n_sel);
  return out;
}

}  // namespace lsm2d_host
