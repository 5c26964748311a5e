// Drives scoreGridSelect and relocalizeGrid of the C++ host mirror (host/lsm2d_score_grid.hpp):
//   score_grid_driver scan.bin map.bin cols tau sum_order  c0 c1 c2 s0 s1 s2 (float bits)  nx ny nt n_levels rx ry rt k_parents
//                     coarse: min_inliers max_chi_bits min_ratio_bits  last: min_inliers max_chi_bits min_ratio_bits  k  iterations k_align
// One projective slice with a Cauchy robustifier, min_num_correspondences 10.  Prints what the two calls return as JSON (floats as bits): the Python test
// compares it with api.score_grid_select / api.relocalize_grid on the same inputs.
#include <lsm2d_score_grid.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

int main(int argc, char** argv) {
  if (argc < 29) { fprintf(stderr, "usage: %s scan.bin map.bin cols tau sum_order <6 float bits> <8 grid integers> <3 coarse> <3 last> k iterations k_align\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    ctx.setOption("sum_order", atoi(argv[5]));
    CloudSet scan(ctx, read_all<PointNormal2f>(argv[1])), map(ctx, read_all<PointNormal2f>(argv[2]));
    CorrespondenceFinderProjective2f cf(ctx);
    cf.param_projector->param_canvas_cols = atoi(argv[3]); cf.param_projector->param_range_max = 30.f;
    cf.param_projector->param_angle_col_min = -(float) M_PI; cf.param_projector->param_angle_col_max = (float) M_PI;
    lsm2d_slice_params sp = cf.sliceParams();
    sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = (float) atof(argv[4]); sp.min_num_correspondences = 10;
    const std::vector<lsm2d_slice_params> slices = {sp};
    const std::vector<const CloudSet*> fixed = {&scan}, moving = {&map};
    lsm2d_pose_grid g;
    for (int a = 0; a < 3; ++a) { g.center[a] = from_bits_arg(argv[6 + a]); g.step[a] = from_bits_arg(argv[9 + a]); g.count[a] = atoi(argv[12 + a]); g.refine[a] = atoi(argv[16 + a]); }
    g.n_levels = atoi(argv[15]); g.k_parents = atoi(argv[19]);
    const lsm2d_select_params coarse{atoi(argv[20]), from_bits_arg(argv[21]), from_bits_arg(argv[22])}, last{atoi(argv[23]), from_bits_arg(argv[24]), from_bits_arg(argv[25])};
    const int32_t k = atoi(argv[26]), k_align = atoi(argv[28]);
    const lsm2d_aligner_params ap{atoi(argv[27]), 0, 0.f, 0.f, 0, 0};

    const GridSelection s = scoreGridSelect(ctx, slices, fixed, moving, g, &coarse, last, k);
    const GridRelocalization r = relocalizeGrid(ctx, ap, slices, fixed, moving, g, &coarse, last, k, nullptr, k_align);

    int again = r.scored.pose.size() == s.pose.size() && r.scored.origin == s.origin && r.scored.n_accepted == s.n_accepted && r.scored.level_counts == s.level_counts;
    for (size_t j = 0; j < s.pose.size() && again; ++j)
      again = !memcmp(r.scored.pose[j].data(), s.pose[j].data(), 12) && !memcmp(&r.scored.rows[j].row.stats, &s.rows[j].row.stats, sizeof(lsm2d_iteration_stats));
    printf("{\"n_accepted\": %d, \"scored_again_equal\": %d, \"level_counts\": [", s.n_accepted, again);
    for (size_t l = 0; l < s.level_counts.size(); ++l) printf("%s[%d,%d]", l ? "," : "", s.level_counts[l][0], s.level_counts[l][1]);
    printf("], ");
    print_int_list("origin", s.origin, ", ");
    printf("\"rows\": [");
    for (size_t j = 0; j < s.pose.size(); ++j) {
      const AlignerScore& w = s.rows[j];
      printf("%s{", j ? "," : "");
      print_bits_list("pose", s.pose[j].data(), 3, ", "); print_bits_list("H", w.row.H.data(), 9, ", "); print_bits_list("b", w.row.b.data(), 3, ", ");
      printf("\"active\": %d, ", w.active);
      print_stats(w.row.stats);
      printf("}");
    }
    const AlignSelection& a = r.aligned;
    printf("], \"aligned\": {\"n_accepted\": %d, \"n_success\": %d, ", a.n_accepted, a.n_success);
    print_int_list("index", a.index, ", ");
    printf("\"pose\": [");
    for (size_t q = 0; q < a.pose.size(); ++q) printf("%s[%u,%u,%u]", q ? "," : "", bits(a.pose[q][0]), bits(a.pose[q][1]), bits(a.pose[q][2]));
    printf("]}}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
