// Drives the aligner scoring through the bare C ABI and through the C++ host mirror (lsm2d_score_aligner_batch / lsm2d_score_aligner_select):
//   score_aligner_driver dir sum_order min_inliers max_chi_bits min_ratio_bits k with_prior
// `dir` holds, for the two slices s = 0, 1: fixed<s>.bin (float32 [N,4], the clouds back to back), off<s>.bin (int32 offsets), moving<s>.bin (one cloud),
// and poses.bin (float32 [n,3]), priors.bin (float32 [n,12]: z, omega).  Slice 0: projective 1081 columns, Cauchy 0.05, sensor (0.1, -0.05, 0.3); slice 1:
// projective 721 columns, Cauchy 0.01, sensor (-0.2, 0, 3.0); min_num_correspondences 10.  Scores every hypothesis through the ABI and through scoreAligner
// (checked equal byte for byte here), selects the best k (scoreAlignerSelect; rows checked against scoreAligner's), runs the two-slice relocalize with an
// aligner of 8 iterations and checks it against the entry points called by hand; prints everything as JSON (floats as their bit patterns).
#include <lsm2d.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

static void print_score(const AlignerScore& r) {
  printf("{");
  print_bits_list("H", r.row.H.data(), 9, ", "); print_bits_list("b", r.row.b.data(), 3, ", ");
  printf("\"active\": %d, ", r.active);
  print_stats(r.row.stats);
  printf("}");
}

static std::vector<PointNormal2fVectorCloud> split(const PointNormal2fVectorCloud& packed, const std::vector<int32_t>& off) {
  std::vector<PointNormal2fVectorCloud> out;
  for (size_t c = 0; c + 1 < off.size(); ++c) out.emplace_back(packed.begin() + off[c], packed.begin() + off[c + 1]);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 8) { fprintf(stderr, "usage: %s dir sum_order min_inliers max_chi_bits min_ratio_bits k with_prior\n", argv[0]); return 2; }
  try {
    const std::string dir = std::string(argv[1]) + "/";
    Context ctx(0);
    ctx.setOption("sum_order", atoi(argv[2]));
    const lsm2d_select_params select{atoi(argv[3]), from_bits_arg(argv[4]), from_bits_arg(argv[5])};
    const int32_t k = atoi(argv[6]); const bool with_prior = atoi(argv[7]) != 0;
    const std::vector<float> pf = read_all<float>(dir + "poses.bin"), prf = read_all<float>(dir + "priors.bin");
    const size_t n = pf.size() / 3;
    std::vector<Vector3f> poses(n); std::vector<lsm2d_prior> priors;
    for (size_t i = 0; i < n; ++i) poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}};
    if (with_prior) { priors.resize(n); for (size_t i = 0; i < n; ++i) { memcpy(priors[i].z, &prf[12 * i], sizeof(float) * 3); memcpy(priors[i].omega, &prf[12 * i + 3], sizeof(float) * 9); } }
    CloudSet f0(ctx, split(read_all<PointNormal2f>(dir + "fixed0.bin"), read_all<int32_t>(dir + "off0.bin")));
    CloudSet f1(ctx, split(read_all<PointNormal2f>(dir + "fixed1.bin"), read_all<int32_t>(dir + "off1.bin")));
    CloudSet m0(ctx, read_all<PointNormal2f>(dir + "moving0.bin")), m1(ctx, read_all<PointNormal2f>(dir + "moving1.bin"));

    std::vector<lsm2d_slice_params> slices;
    const int cols[2] = {1081, 721}; const float tau[2] = {0.05f, 0.01f}; const float S[2][3] = {{0.1f, -0.05f, 0.3f}, {-0.2f, 0.f, 3.0f}};
    for (int s = 0; s < 2; ++s) {
      CorrespondenceFinderProjective2f cf(ctx);
      cf.param_projector->param_canvas_cols = cols[s]; cf.param_projector->param_range_max = 30.f;
      cf.param_projector->param_angle_col_min = -(float) M_PI; cf.param_projector->param_angle_col_max = (float) M_PI;
      lsm2d_slice_params sp = cf.sliceParams();
      sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = tau[s]; sp.min_num_correspondences = 10; memcpy(sp.sensor_in_robot, S[s], sizeof(float) * 3);
      slices.push_back(sp);
    }
    const std::vector<const CloudSet*> fixed = {&f0, &f1}, moving = {&m0, &m1};

    // the bare ABI
    const lsm2d_cloudset* fx[2] = {f0.get(), f1.get()}; const lsm2d_cloudset* mv[2] = {m0.get(), m1.get()};
    lsm2d_batch b{}; b.n_alignments = (int32_t) n; b.n_slices = 2; b.slices = slices.data(); b.fixed = fx; b.moving = mv; b.init_pose = poses[0].data();
    b.prior = with_prior ? priors.data() : nullptr;
    std::vector<float> H(9 * n), bb(3 * n); std::vector<lsm2d_iteration_stats> st(n); std::vector<int32_t> active(n);
    check(lsm2d_score_aligner_batch(ctx.get(), &b, H.data(), bb.data(), st.data(), active.data()), "lsm2d_score_aligner_batch", ctx.get());
    // the mirror
    const std::vector<AlignerScore> all = scoreAligner(ctx, slices, fixed, moving, poses, priors);
    int mirror_equals_abi = all.size() == n;
    for (size_t i = 0; i < n && mirror_equals_abi; ++i)
      if (memcmp(all[i].row.H.data(), &H[9 * i], sizeof(float) * 9) || memcmp(all[i].row.b.data(), &bb[3 * i], sizeof(float) * 3) ||
          memcmp(&all[i].row.stats, &st[i], sizeof(lsm2d_iteration_stats)) || all[i].active != active[i]) mirror_equals_abi = 0;
    const AlignerSelection sel = scoreAlignerSelect(ctx, slices, fixed, moving, poses, select, k, priors);
    int rows_equal_score_aligner = sel.index.size() == sel.rows.size();
    for (size_t j = 0; j < sel.index.size() && rows_equal_score_aligner; ++j)
      if (sel.index[j] < 0 || (size_t) sel.index[j] >= n || !same_bytes(sel.rows[j].row, all[(size_t) sel.index[j]].row) ||
          sel.rows[j].active != all[(size_t) sel.index[j]].active) rows_equal_score_aligner = 0;
    const AlignerSelection none = scoreAlignerSelect(ctx, slices, fixed, moving, std::vector<Vector3f>(), select, k);

    // relocalize, and the entry points called by hand
    const lsm2d_aligner_params ap{8, 10, 0.f, 0.f, 0, 0};
    const AlignerRelocalization rel = relocalize(ctx, ap, slices, fixed, moving, poses, select, k, priors);
    const size_t m = sel.index.size();
    int relocalize_equals_by_hand = rel.selection.index == sel.index && rel.pose.size() == m;
    if (m && relocalize_equals_by_hand) {
      std::vector<int32_t> fi; std::vector<Vector3f> x0(m); std::vector<lsm2d_prior> pr;
      for (int s = 0; s < 2; ++s) for (int32_t i : sel.index) fi.push_back(i);
      for (size_t j = 0; j < m; ++j) { x0[j] = poses[(size_t) sel.index[j]]; if (with_prior) pr.push_back(priors[(size_t) sel.index[j]]); }
      lsm2d_batch a = b; a.n_alignments = (int32_t) m; a.fixed_index = fi.data(); a.init_pose = x0[0].data(); a.prior = with_prior ? pr.data() : nullptr;
      std::vector<Vector3f> pose(m); std::vector<std::array<float, 9>> info(m); std::vector<int32_t> status(m), its(m);
      check(lsm2d_align_batch(ctx.get(), &ap, &a, pose[0].data(), info[0].data(), status.data(), its.data(), nullptr), "lsm2d_align_batch", ctx.get());
      relocalize_equals_by_hand = !memcmp(pose.data(), rel.pose.data(), sizeof(Vector3f) * m) && !memcmp(info.data(), rel.information.data(), sizeof(float) * 9 * m) &&
                                  status == rel.status && its == rel.iterations;
    }

    printf("{\"n\": %zu, \"mirror_equals_abi\": %d, \"rows_equal_score_aligner\": %d, \"relocalize_equals_by_hand\": %d, \"n_empty\": %zu, \"n_accepted\": %d, ",
           n, mirror_equals_abi, rows_equal_score_aligner, relocalize_equals_by_hand, none.index.size() + (size_t) none.n_accepted, sel.n_accepted);
    print_int_list("index", sel.index, ", ");
    printf("\"all\": [");
    for (size_t i = 0; i < n; ++i) { if (i) printf(","); print_score(all[i]); }
    printf("], \"rows\": [");
    for (size_t j = 0; j < sel.rows.size(); ++j) { if (j) printf(","); print_score(sel.rows[j]); }
    printf("], \"relocalize\": {\"n_accepted\": %d, \"items\": [", rel.selection.n_accepted);
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
