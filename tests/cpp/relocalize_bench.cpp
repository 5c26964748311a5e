// Times lsm2d_relocalize_select against the route a caller had before it -- lsm2d_score_aligner_select, the host's gather of the selected hypotheses' poses
// and cloud indices, lsm2d_align_select -- through the bare C ABI, both in this process, alternating call by call:
//   relocalize_bench scans.bin offsets.bin map.bin poses.bin cols tau iterations min_inliers max_chi_bits min_ratio_bits k_score k steps warmup
// n float32 hypotheses; scans.bin holds ragged float32 [N,4] scans (int32 offsets): ONE scan every hypothesis is scored against, or n scans, hypothesis i
// against scan i; one map.  Projective finder, Cauchy robustifier of threshold tau, `iterations` Gauss-Newton iterations, the aligner's min_num_inliers 10;
// the same thresholds judge both stages; the two float thresholds come as their bit patterns.  Prints one JSON line: medians, minima and maxima of the wall
// clock around each route in ms, lsm2d_last_kernel_ms of one more call of each (the two-call route: the sum of its two calls'), the counts, and whether every
// output of the two routes is equal byte for byte (the caller's parity gate: tests/bench/relocalize_bench.py).
#include <cstddef>

#include "driver_common.h"

// everything the call returns
struct Answer {
  std::vector<int32_t> scored_index, index, its; std::vector<lsm2d_iteration_stats> scored_stats, last; std::vector<float> pose, H;
  int32_t n_scored = 0, n_scored_acc = 0, n_sel = 0, n_acc = 0, n_suc = 0;
  Answer(size_t k_score, size_t k) : scored_index(k_score), index(k), its(k), scored_stats(k_score), last(k), pose(3 * k), H(9 * k) {}
  bool equals(const Answer& o) const {
    if (n_scored != o.n_scored || n_scored_acc != o.n_scored_acc || n_sel != o.n_sel || n_acc != o.n_acc || n_suc != o.n_suc) return false;
    const size_t m = (size_t) n_scored, r = (size_t) n_sel;
    return !memcmp(scored_index.data(), o.scored_index.data(), 4 * m) && !memcmp(scored_stats.data(), o.scored_stats.data(), sizeof(lsm2d_iteration_stats) * m) &&
           !memcmp(index.data(), o.index.data(), 4 * r) && !memcmp(its.data(), o.its.data(), 4 * r) && !memcmp(pose.data(), o.pose.data(), 12 * r) &&
           !memcmp(H.data(), o.H.data(), 36 * r) && !memcmp(last.data(), o.last.data(), sizeof(lsm2d_iteration_stats) * r);
  }
};

int main(int argc, char** argv) {
  if (argc < 15) { fprintf(stderr, "usage: %s scans.bin offsets.bin map.bin poses.bin cols tau iterations min_inliers max_chi_bits min_ratio_bits k_score k steps warmup\n", argv[0]); return 2; }
  const std::vector<float> scans = read_all<float>(argv[1]);
  const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
  const std::vector<float> map = read_all<float>(argv[3]);
  const std::vector<float> poses = read_all<float>(argv[4]);
  const int cols = atoi(argv[5]); const float tau = (float) atof(argv[6]); const int iterations = atoi(argv[7]);
  const lsm2d_select_params select{atoi(argv[8]), from_bits_arg(argv[9]), from_bits_arg(argv[10])};
  const int32_t k_score = atoi(argv[11]), k = atoi(argv[12]); const int steps = atoi(argv[13]), warmup = atoi(argv[14]);
  const int32_t n = (int32_t) (poses.size() / 3), n_scans = (int32_t) offs.size() - 1;
  if (n_scans != 1 && n_scans != n) { fprintf(stderr, "offsets.bin: one scan, or one per hypothesis\n"); return 2; }

  lsm2d_context* ctx = nullptr;
  must(lsm2d_create(0, nullptr, &ctx), "lsm2d_create", nullptr);
  lsm2d_cloudset *fixed = nullptr, *moving = nullptr;
  must(lsm2d_cloudset_create(ctx, scans.data(), offs.data(), n_scans, (int64_t) (scans.size() / 4), &fixed), "scans", ctx);
  must(lsm2d_cloudset_create(ctx, map.data(), nullptr, 1, (int64_t) (map.size() / 4), &moving), "map", ctx);
  lsm2d_slice_params sp{};
  sp.finder = LSM2D_FINDER_PROJECTIVE; sp.projector = lsm2d_projector{cols, -3.14159265358979f, 3.14159265358979f, 0.3f, 30.0f, 0.0f};
  sp.point_distance = 0.5f; sp.normal_cos = 0.8f; sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = tau; sp.min_num_correspondences = 10;
  const lsm2d_aligner_params ap{iterations, 10, 0.f, 0.f, 0, 0};
  const lsm2d_cloudset* fx[1] = {fixed}; const lsm2d_cloudset* mv[1] = {moving};
  lsm2d_batch b{}; b.n_alignments = n; b.n_slices = 1; b.slices = &sp; b.fixed = fx; b.moving = mv; b.init_pose = poses.data();

  Answer fused((size_t) k_score, (size_t) k), two((size_t) k_score, (size_t) k);
  auto route_fused = [&] {
    Answer& a = fused;
    must(lsm2d_relocalize_select(ctx, &ap, &b, &select, k_score, nullptr, k, a.scored_index.data(), a.scored_stats.data(), &a.n_scored, &a.n_scored_acc,
                                 a.index.data(), a.pose.data(), a.H.data(), a.its.data(), a.last.data(), &a.n_sel, &a.n_acc, &a.n_suc), "lsm2d_relocalize_select", ctx);
  };
  std::vector<float> x0(3 * (size_t) k_score); std::vector<int32_t> fi((size_t) k_score), sub((size_t) k);
  float kernel_two[2] = {0.f, 0.f}; bool timed = false;
  auto route_two = [&] {
    Answer& a = two;
    must(lsm2d_score_aligner_select(ctx, &b, &select, k_score, a.scored_index.data(), nullptr, nullptr, a.scored_stats.data(), nullptr, &a.n_scored, &a.n_scored_acc),
         "lsm2d_score_aligner_select", ctx);
    if (timed) must(lsm2d_last_kernel_ms(ctx, &kernel_two[0]), "lsm2d_last_kernel_ms", ctx);
    a.n_sel = a.n_acc = a.n_suc = 0; kernel_two[1] = 0.f;
    if (a.n_scored == 0) return;
    for (int32_t j = 0; j < a.n_scored; ++j) {      // the host's gather
      const size_t i = (size_t) a.scored_index[(size_t) j];
      memcpy(&x0[3 * (size_t) j], &poses[3 * i], 12); fi[(size_t) j] = n_scans == 1 ? 0 : (int32_t) i;
    }
    lsm2d_batch b2 = b; b2.n_alignments = a.n_scored; b2.init_pose = x0.data(); b2.fixed_index = fi.data();
    must(lsm2d_align_select(ctx, &ap, &b2, &select, k, sub.data(), a.pose.data(), a.H.data(), a.its.data(), a.last.data(), &a.n_sel, &a.n_acc, &a.n_suc),
         "lsm2d_align_select", ctx);
    if (timed) must(lsm2d_last_kernel_ms(ctx, &kernel_two[1]), "lsm2d_last_kernel_ms", ctx);
    for (int32_t r = 0; r < a.n_sel; ++r) a.index[(size_t) r] = a.scored_index[(size_t) sub[(size_t) r]];
  };

  must(lsm2d_set_option(ctx, "kernel_timing", 0), "kernel_timing", ctx);
  for (int w = 0; w < warmup; ++w) { route_fused(); route_two(); }
  std::vector<double> t_fused, t_two;
  using clk = std::chrono::steady_clock;
  for (int s = 0; s < steps; ++s) {
    auto t0 = clk::now(); route_fused(); auto t1 = clk::now(); route_two(); auto t2 = clk::now();
    t_fused.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); t_two.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
  }
  const int outputs_equal = fused.equals(two) ? 1 : 0;
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "kernel_timing", ctx);
  timed = true;
  float k_fused = 0.f;
  route_fused(); must(lsm2d_last_kernel_ms(ctx, &k_fused), "lsm2d_last_kernel_ms", ctx);
  route_two();
  double sf[3], st[3]; summary(t_fused, sf); summary(t_two, st);
  printf("{\"n_hypotheses\": %d, \"k_score\": %d, \"k\": %d, \"steps\": %d, \"fused_ms\": [%.4f, %.4f, %.4f], \"two_call_ms\": [%.4f, %.4f, %.4f], "
         "\"fused_kernel_ms\": %.4f, \"two_call_kernel_ms\": [%.4f, %.4f], \"outputs_equal\": %d, \"n_scored_accepted\": %d, \"n_scored_selected\": %d, "
         "\"n_success\": %d, \"n_accepted\": %d, \"n_selected\": %d, \"best\": %d}\n",
         n, k_score, k, steps, sf[0], sf[1], sf[2], st[0], st[1], st[2], k_fused, kernel_two[0], kernel_two[1], outputs_equal, fused.n_scored_acc, fused.n_scored,
         fused.n_suc, fused.n_acc, fused.n_sel, fused.n_sel ? fused.index[0] : -1);
  lsm2d_cloudset_destroy(fixed); lsm2d_cloudset_destroy(moving); lsm2d_destroy(ctx);
  return 0;
}
