// Drives relocalizeSelect of the C++ host mirror (host/lsm2d_relocalize.hpp) against the existing relocalize() on the same inputs:
//   relocalize_select_driver scan.bin map.bin poses.bin cols tau iterations min_num_inliers sum_order min_inliers max_chi_bits min_ratio_bits k_score k
// One projective slice with a Cauchy robustifier, min_num_correspondences 10; the same thresholds judge both stages.  relocalize() scores, gathers on the host
// and aligns every selected hypothesis (lsm2d_align_batch); its verdict is restated here -- accepted rows ranked by inliers descending, chi_inliers ascending
// on its bits, position in the selection ascending, cut at k -- and compared with relocalizeSelect's answer byte for byte.  Prints JSON (floats as bits).
#include <algorithm>
#include <lsm2d_relocalize.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

int main(int argc, char** argv) {
  if (argc < 14) { fprintf(stderr, "usage: %s scan.bin map.bin poses.bin cols tau iterations min_num_inliers sum_order min_inliers max_chi_bits min_ratio_bits k_score k\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    ctx.setOption("sum_order", atoi(argv[8]));
    const std::vector<float> pf = read_all<float>(argv[3]);
    const size_t n = pf.size() / 3;
    std::vector<Vector3f> poses(n);
    for (size_t i = 0; i < n; ++i) poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}};
    CloudSet scan(ctx, read_all<PointNormal2f>(argv[1])), map(ctx, read_all<PointNormal2f>(argv[2]));
    CorrespondenceFinderProjective2f cf(ctx);
    cf.param_projector->param_canvas_cols = atoi(argv[4]); cf.param_projector->param_range_max = 30.f;
    cf.param_projector->param_angle_col_min = -(float) M_PI; cf.param_projector->param_angle_col_max = (float) M_PI;
    lsm2d_slice_params sp = cf.sliceParams();
    sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = (float) atof(argv[5]); sp.min_num_correspondences = 10;
    const std::vector<lsm2d_slice_params> slices = {sp};
    const std::vector<const CloudSet*> fixed = {&scan}, moving = {&map};
    const lsm2d_aligner_params ap{atoi(argv[6]), atoi(argv[7]), 0.f, 0.f, 0, 0};
    const lsm2d_select_params select{atoi(argv[9]), from_bits_arg(argv[10]), from_bits_arg(argv[11])};
    const int32_t k_score = atoi(argv[12]), k = atoi(argv[13]);

    const AlignerRelocalization rel = relocalize(ctx, ap, slices, fixed, moving, poses, select, k_score);
    const RelocalizeSelection rs = relocalizeSelect(ctx, ap, slices, fixed, moving, poses, select, k_score, nullptr, k);

    const size_t m = rel.selection.index.size();
    int scored_equal = rs.scored.index == rel.selection.index && rs.scored.n_accepted == rel.selection.n_accepted && rs.scored.rows.size() == m;
    for (size_t j = 0; j < m && scored_equal; ++j)
      scored_equal = !memcmp(&rs.scored.rows[j].row.stats, &rel.selection.rows[j].row.stats, sizeof(lsm2d_iteration_stats));
    // relocalize()'s verdict, ranked
    std::vector<std::pair<uint64_t, size_t>> keyed; int32_t n_success = 0;
    for (size_t j = 0; j < rel.pose.size(); ++j) {
      n_success += rel.status[j] == LSM2D_SUCCESS;
      if (!rel.accepted[j] || rel.iterations[j] < 1) continue;
      keyed.emplace_back(key_of(rel.last_stats[j]), j);
    }
    std::sort(keyed.begin(), keyed.end());
    const size_t r = std::min(keyed.size(), (size_t) k);
    const AlignSelection& a = rs.aligned;
    int aligned_equal = a.n_accepted == (int32_t) keyed.size() && a.n_success == n_success && a.index.size() == r && a.pose.size() == r;
    for (size_t q = 0; q < r && aligned_equal; ++q) {
      const size_t j = keyed[q].second;
      aligned_equal = a.index[q] == rel.selection.index[j] && !memcmp(a.pose[q].data(), rel.pose[j].data(), 12) &&
                      !memcmp(a.information[q].data(), rel.information[j].data(), 36) && a.iterations[q] == rel.iterations[j] &&
                      !memcmp(&a.last_stats[q], &rel.last_stats[j], sizeof(lsm2d_iteration_stats));
    }
    const RelocalizeSelection none = relocalizeSelect(ctx, ap, slices, fixed, moving, std::vector<Vector3f>(), select, k_score, nullptr, k);

    printf("{\"n\": %zu, \"scored_equal\": %d, \"aligned_equal\": %d, \"n_empty\": %zu, \"n_scored_accepted\": %d, \"n_accepted\": %d, \"n_success\": %d, ",
           n, scored_equal, aligned_equal, none.scored.index.size() + none.aligned.index.size() + (size_t) none.scored.n_accepted + (size_t) none.aligned.n_accepted,
           rs.scored.n_accepted, a.n_accepted, a.n_success);
    print_int_list("scored_index", rs.scored.index, ", "); print_int_list("index", a.index, ", ");
    printf("\"rows\": [");
    for (size_t q = 0; q < a.index.size(); ++q) {
      printf("%s{", q ? "," : "");
      print_bits_list("pose", a.pose[q].data(), 3, ", "); print_bits_list("H", a.information[q].data(), 9, ", ");
      printf("\"iterations\": %d, ", a.iterations[q]);
      print_stats(a.last_stats[q]);
      printf("}");
    }
    printf("]}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
