// Drives alignSelect and LoopClosureSweep::computeSelect of the C++ host mirror (lsm2d_align_select, lsm2d_sweep_align_select):
//   align_select_driver scan.bin map.bin poses.bin cols tau iterations min_num_inliers sum_order min_inliers max_chi_bits min_ratio_bits k
// reads one float32 [N,4] scan (fixed), one map (moving) and n float32 start poses, aligns every candidate (projective finder, a Cauchy robustifier of threshold
// tau), has the device accept and rank them, and prints both results as JSON (floats as their bit patterns; the two float thresholds come as their bit
// patterns).  The sweep names device 0 twice: two shards whose rows the host merges; it runs in the default order of summation only (a sweep's contexts
// take no option).
#include <lsm2d.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

static void print_rows(const std::vector<int32_t>& index, const std::vector<Vector3f>& pose, const std::vector<std::array<float, 9>>& H,
                       const std::vector<int32_t>& its, const std::vector<lsm2d_iteration_stats>& st, int32_t n_accepted, int32_t n_success) {
  printf("{\"n_accepted\": %d, \"n_success\": %d, ", n_accepted, n_success);
  print_int_list("index", index, ", ");
  printf("\"rows\": [");
  for (size_t j = 0; j < index.size(); ++j) {
    printf("%s{", j ? "," : "");
    print_bits_list("pose", pose[j].data(), 3, ", "); print_bits_list("H", H[j].data(), 9, ", ");
    printf("\"iterations\": %d, ", its[j]);
    print_stats(st[j]);
    printf("}");
  }
  printf("]}");
}

int main(int argc, char** argv) {
  if (argc < 13) { fprintf(stderr, "usage: %s scan.bin map.bin poses.bin cols tau iterations min_num_inliers sum_order min_inliers max_chi_bits min_ratio_bits k\n", argv[0]); return 2; }
  try {
    const PointNormal2fVectorCloud scan = read_all<PointNormal2f>(argv[1]);
    const PointNormal2fVectorCloud map = read_all<PointNormal2f>(argv[2]);
    const std::vector<float> pf = read_all<float>(argv[3]);
    const int cols = atoi(argv[4]); const float tau = (float) atof(argv[5]);
    const int iterations = atoi(argv[6]), min_num_inliers = atoi(argv[7]), order = atoi(argv[8]);
    const lsm2d_select_params select{atoi(argv[9]), from_bits_arg(argv[10]), from_bits_arg(argv[11])};
    const int32_t k = atoi(argv[12]);
    const size_t n = pf.size() / 3;
    std::vector<Vector3f> poses(n);
    for (size_t i = 0; i < n; ++i) poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}};

    PointNormal2fProjectorPolar projector;
    projector.param_canvas_cols = cols; projector.param_range_max = 30.f; projector.param_angle_col_min = -(float) M_PI; projector.param_angle_col_max = (float) M_PI;
    const lsm2d_slice_params sp = LoopClosureSweep::projectiveSlice(projector, 0.5f, 0.8f, tau, 10);
    const lsm2d_aligner_params ap{iterations, min_num_inliers, 0.f, 0.f, 0, 0};

    printf("{\"n\": %zu, \"align_select\": ", n);
    {
      Context ctx(0);
      ctx.setOption("sum_order", order);
      CloudSet scan_set(ctx, scan), map_set(ctx, map);
      const AlignSelection s = alignSelect(ctx, ap, {sp}, {&scan_set}, {&map_set}, poses, select, k);
      print_rows(s.index, s.pose, s.information, s.iterations, s.last_stats, s.n_accepted, s.n_success);
      const AlignSelection none = alignSelect(ctx, ap, {sp}, {&scan_set}, {&map_set}, std::vector<Vector3f>(), select, k);
      printf(", \"n_empty\": %zu", none.index.size() + (size_t) none.n_accepted + (size_t) none.n_success);
    }
    printf(", \"compute_select\": ");
    if (order == 0) {
      LoopClosureSweep sweep({0, 0});
      sweep.param_max_iterations = iterations; sweep.param_min_num_inliers = min_num_inliers; sweep.param_slice = sp;
      sweep.param_relocalize_min_inliers = select.min_inliers; sweep.param_relocalize_max_chi_inliers = select.max_chi_per_inlier;
      sweep.param_relocalize_min_inliers_ratio = select.min_inlier_ratio;
      sweep.setMap(map); sweep.setScans({scan});
      sweep.computeSelect(std::vector<int32_t>(n, 0), poses, k);
      print_rows(sweep.selected, sweep.pose, sweep.information, sweep.iterations, sweep.last_stats, sweep.n_accepted, sweep.n_success);
    } else printf("null");
    printf("}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
