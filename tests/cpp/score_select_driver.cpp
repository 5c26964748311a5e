// Drives scoreSelect and relocalize of the C++ host mirror (lsm2d_score_select):
//   score_select_driver scan.bin map.bin poses.bin cols tau sum_order min_inliers max_chi_bits min_ratio_bits k
// reads one float32 [N,4] scan (fixed), one map (moving) and n float32 poses, selects the best k hypotheses that pass the acceptance test (projective finder,
// a Cauchy robustifier of threshold tau; the two float thresholds come as their bit patterns), checks every selected row byte for byte against scoreBatch
// on the same poses, runs relocalize with an aligner of 8 iterations and prints everything as JSON (floats as their bit patterns).
#include <lsm2d.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

int main(int argc, char** argv) {
  if (argc < 11) { fprintf(stderr, "usage: %s scan.bin map.bin poses.bin cols tau sum_order min_inliers max_chi_bits min_ratio_bits k\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    const PointNormal2fVectorCloud scan = read_all<PointNormal2f>(argv[1]);
    const PointNormal2fVectorCloud map = read_all<PointNormal2f>(argv[2]);
    const std::vector<float> pf = read_all<float>(argv[3]);
    const int cols = atoi(argv[4]); const float tau = (float) atof(argv[5]);
    ctx.setOption("sum_order", atoi(argv[6]));
    const lsm2d_select_params select{atoi(argv[7]), from_bits_arg(argv[8]), from_bits_arg(argv[9])};
    const int32_t k = atoi(argv[10]);
    const size_t n = pf.size() / 3;
    std::vector<Vector3f> poses(n);
    for (size_t i = 0; i < n; ++i) poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}};
    CloudSet scan_set(ctx, scan), map_set(ctx, map);

    CorrespondenceFinderProjective2f cf(ctx);
    cf.param_projector->param_canvas_cols = cols; cf.param_projector->param_range_max = 30.f;
    cf.param_projector->param_angle_col_min = -(float) M_PI; cf.param_projector->param_angle_col_max = (float) M_PI;
    lsm2d_slice_params sp = cf.sliceParams();
    sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = tau; sp.min_num_correspondences = 10;

    const Selection sel = scoreSelect(ctx, sp, scan_set, map_set, poses, select, k);
    const std::vector<Linearization> all = scoreBatch(ctx, sp, scan_set, map_set, poses);
    int rows_equal_score_batch = sel.index.size() == sel.rows.size();
    for (size_t j = 0; j < sel.index.size() && rows_equal_score_batch; ++j)
      if (sel.index[j] < 0 || (size_t) sel.index[j] >= n || !same_bytes(sel.rows[j], all[(size_t) sel.index[j]])) rows_equal_score_batch = 0;
    const Selection none = scoreSelect(ctx, sp, scan_set, map_set, std::vector<Vector3f>(), select, k);

    const lsm2d_aligner_params ap{8, 10, 0.f, 0.f, 0, 0};
    const Relocalization rel = relocalize(ctx, ap, sp, scan_set, map_set, poses, select, k);

    printf("{\"n\": %zu, \"n_accepted\": %d, \"rows_equal_score_batch\": %d, \"n_empty\": %zu, ", n, sel.n_accepted, rows_equal_score_batch,
           none.index.size() + (size_t) none.n_accepted);
    print_int_list("index", sel.index, ", ");
    printf("\"rows\": [");
    for (size_t j = 0; j < sel.rows.size(); ++j) {
      const Linearization& r = sel.rows[j];
      printf("%s{", j ? "," : "");
      print_bits_list("H", r.H.data(), 9, ", "); print_bits_list("b", r.b.data(), 3, ", ");
      print_stats(r.stats);
      printf("}");
    }
    printf("], \"relocalize\": {\"n_accepted\": %d, ", rel.selection.n_accepted);
    print_int_list("index", rel.selection.index, ", ");
    printf("\"items\": [");
    for (size_t j = 0; j < rel.pose.size(); ++j) {
      printf("%s{", j ? "," : "");
      print_bits_list("pose", rel.pose[j].data(), 3, ", ");
      printf("\"status\": %d, \"iterations\": %d, \"accepted\": %d, ", rel.status[j], rel.iterations[j], (int) rel.accepted[j]);
      print_stats(rel.last_stats[j]);
      printf("}");
    }
    printf("]}}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
