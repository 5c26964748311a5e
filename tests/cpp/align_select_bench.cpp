// Times lsm2d_align_select against the route a caller had before it -- lsm2d_align_batch with every iteration's statistics, then the acceptance test on each
// candidate's last row and the ranking on the host -- through the bare C ABI, both in this process, alternating call by call:
//   align_select_bench scans.bin offsets.bin map.bin poses.bin index.bin cols tau iterations min_inliers max_chi_bits min_ratio_bits k steps warmup out.bin
// n float32 start poses; scans.bin holds ragged float32 [N,4] scans (int32 offsets), index.bin one int32 scan index per candidate (an empty file: candidate i
// uses scan i); one map every candidate is aligned against.  Projective finder, Cauchy robustifier of threshold tau, `iterations` Gauss-Newton iterations, the
// aligner's min_num_inliers 10; the two float thresholds come as their bit patterns.  Prints one JSON line -- medians, minima and maxima of the wall clock
// around each route in ms, lsm2d_last_kernel_ms of one more call of each, both routes' verdicts -- and writes the baseline's status, iteration count and last
// statistics row of all n candidates to out.bin ([n] int32, [n] int32, [n] rows) for the caller's parity gate (tests/bench/align_select_bench.py).
#include <cstddef>

#include "driver_common.h"

int main(int argc, char** argv) {
  if (argc < 16) { fprintf(stderr, "usage: %s scans.bin offsets.bin map.bin poses.bin index.bin cols tau iterations min_inliers max_chi_bits min_ratio_bits k steps warmup out.bin\n", argv[0]); return 2; }
  const std::vector<float> scans = read_all<float>(argv[1]);
  const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
  const std::vector<float> map = read_all<float>(argv[3]);
  const std::vector<float> poses = read_all<float>(argv[4]);
  const std::vector<int32_t> index = read_all<int32_t>(argv[5]);
  const int cols = atoi(argv[6]); const float tau = (float) atof(argv[7]); const int iterations = atoi(argv[8]);
  const lsm2d_select_params select{atoi(argv[9]), from_bits_arg(argv[10]), from_bits_arg(argv[11])};
  const int32_t k = atoi(argv[12]); const int steps = atoi(argv[13]), warmup = atoi(argv[14]);
  const int32_t n = (int32_t) (poses.size() / 3), n_scans = (int32_t) offs.size() - 1;
  if (!index.empty() && (int32_t) index.size() != n) { fprintf(stderr, "index.bin: one entry per candidate, or none\n"); return 2; }

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
  lsm2d_batch b{}; b.n_alignments = n; b.n_slices = 1; b.slices = &sp; b.fixed = fx; b.moving = mv; b.fixed_index = index.empty() ? nullptr : index.data();
  b.init_pose = poses.data();
  const size_t cap = (size_t) lsm2d_stats_capacity(&ap);

  // the new route: k rows come down
  std::vector<int32_t> idx_new((size_t) k), its_new((size_t) k); std::vector<float> pose_new(3 * (size_t) k), H_new(9 * (size_t) k);
  std::vector<lsm2d_iteration_stats> st_new((size_t) k);
  int32_t n_sel_new = 0, n_acc_new = 0, n_suc_new = 0;
  auto route_new = [&] {
    must(lsm2d_align_select(ctx, &ap, &b, &select, k, idx_new.data(), pose_new.data(), H_new.data(), its_new.data(), st_new.data(), &n_sel_new, &n_acc_new,
                            &n_suc_new), "lsm2d_align_select", ctx);
  };
  // the baseline: every candidate's results and every iteration's statistics come down, the host tests each candidate's last row and ranks (the same fp32
  // test, the same total order; a partial sort of the accepted candidates)
  std::vector<float> pose((size_t) n * 3), H((size_t) n * 9); std::vector<int32_t> status((size_t) n), its((size_t) n);
  std::vector<lsm2d_iteration_stats> st((size_t) n * cap);
  std::vector<std::pair<uint64_t, int32_t>> keyed; keyed.reserve((size_t) n);
  std::vector<int32_t> idx_base; int32_t n_acc_base = 0, n_suc_base = 0;
  auto route_base = [&] {
    must(lsm2d_align_batch(ctx, &ap, &b, pose.data(), H.data(), status.data(), its.data(), st.data()), "lsm2d_align_batch", ctx);
    keyed.clear(); n_suc_base = 0;
    for (int32_t i = 0; i < n; ++i) {
      if (status[(size_t) i] != LSM2D_SUCCESS) continue;
      ++n_suc_base;
      if (its[(size_t) i] < 1) continue;
      const lsm2d_iteration_stats& s = st[(size_t) i * cap + (size_t) (its[(size_t) i] - 1)];
      if (accept(s, select)) keyed.emplace_back(key_of(s), i);
    }
    n_acc_base = (int32_t) keyed.size();
    const size_t m = std::min((size_t) k, keyed.size());
    std::partial_sort(keyed.begin(), keyed.begin() + (std::ptrdiff_t) m, keyed.end());
    idx_base.resize(m);
    for (size_t j = 0; j < m; ++j) idx_base[j] = keyed[j].second;
  };

  must(lsm2d_set_option(ctx, "kernel_timing", 0), "kernel_timing", ctx);
  for (int w = 0; w < warmup; ++w) { route_new(); route_base(); }
  std::vector<double> t_new, t_base;
  using clk = std::chrono::steady_clock;
  for (int s = 0; s < steps; ++s) {
    auto t0 = clk::now(); route_new(); auto t1 = clk::now(); route_base(); auto t2 = clk::now();
    t_new.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); t_base.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
  }
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "kernel_timing", ctx);
  float k_new = 0.f, k_base = 0.f;
  route_new(); must(lsm2d_last_kernel_ms(ctx, &k_new), "lsm2d_last_kernel_ms", ctx);
  route_base(); must(lsm2d_last_kernel_ms(ctx, &k_base), "lsm2d_last_kernel_ms", ctx);

  // the new route's rows are the baseline's rows of the selected candidates
  int rows_equal = 1;
  for (int32_t j = 0; j < n_sel_new && rows_equal; ++j) {
    const size_t i = (size_t) idx_new[(size_t) j];
    if (i >= (size_t) n || its[i] < 1 || memcmp(&pose_new[3 * (size_t) j], &pose[3 * i], 12) || memcmp(&H_new[9 * (size_t) j], &H[9 * i], 36) ||
        its_new[(size_t) j] != its[i] || memcmp(&st_new[(size_t) j], &st[i * cap + (size_t) (its[i] - 1)], sizeof(lsm2d_iteration_stats)))
      rows_equal = 0;
  }
  std::vector<lsm2d_iteration_stats> last((size_t) n);
  for (int32_t i = 0; i < n; ++i) {
    lsm2d_iteration_stats z; memset(&z, 0, sizeof z);
    last[(size_t) i] = its[(size_t) i] >= 1 ? st[(size_t) i * cap + (size_t) (its[(size_t) i] - 1)] : z;
  }
  FILE* f = fopen(argv[15], "wb");
  if (!f || fwrite(status.data(), sizeof(int32_t), (size_t) n, f) != (size_t) n || fwrite(its.data(), sizeof(int32_t), (size_t) n, f) != (size_t) n ||
      fwrite(last.data(), sizeof(lsm2d_iteration_stats), (size_t) n, f) != (size_t) n) { perror(argv[15]); return 2; }
  fclose(f);
  double sn[3], sb[3]; summary(t_new, sn); summary(t_base, sb);
  printf("{\"n_candidates\": %d, \"k\": %d, \"steps\": %d, \"stats_rows_per_candidate\": %zu, \"select_ms\": [%.4f, %.4f, %.4f], \"baseline_ms\": [%.4f, %.4f, %.4f], "
         "\"select_kernel_ms\": %.4f, \"baseline_kernel_ms\": %.4f, \"rows_equal\": %d, \"n_accepted\": [%d, %d], \"n_success\": [%d, %d], ",
         n, k, steps, cap, sn[0], sn[1], sn[2], sb[0], sb[1], sb[2], k_new, k_base, rows_equal, n_acc_new, n_acc_base, n_suc_new, n_suc_base);
  idx_new.resize((size_t) n_sel_new);
  print_int_list("index_select", idx_new, ", "); print_int_list("index_baseline", idx_base, "}\n");
  lsm2d_cloudset_destroy(fixed); lsm2d_cloudset_destroy(moving); lsm2d_destroy(ctx);
  return 0;
}
