// Times lsm2d_score_aligner_batch / lsm2d_score_aligner_select against the route a caller had before them for an aligner with two slices -- one
// lsm2d_score_batch per slice at the effective pose the caller composes itself, the rows added and the skip rule applied on the host, and for the select form
// the acceptance test and a partial sort on the host -- through the bare C ABI, all in this process, the routes alternating call by call:
//   score_aligner_bench fixed0.bin off0.bin fixed1.bin off1.bin map.bin poses.bin sinv.bin cols tau sum_order min_corr min_inliers max_chi_bits min_ratio_bits k steps warmup
// n float32 poses; fixed<s>.bin holds n ragged float32 [N,4] scans (int32 offsets [n+1]) or ONE scan every pose is matched against; sinv.bin holds per slice
// S (3 floats), S^-1 (3 floats) and cos / sin of S^-1's angle as the library forms them (the caller's composition is then the library's, bit for bit).
// Projective finders, Cauchy robustifier of threshold tau.  Prints one JSON line: medians, minima and maxima of the wall clock around each route in ms,
// lsm2d_last_kernel_ms of one more call of each, whether the routes agree (rows byte for byte but for the digest, which the old route cannot salt; selections).
#include <lsm2d.h>

#include <cmath>
#include <cstddef>

#include "driver_common.h"

static float wrap(float a) {
  while (a > 3.14159274101257324f) a -= 6.28318548202514648f;
  while (a <= -3.14159274101257324f) a += 6.28318548202514648f;
  return a;
}

int main(int argc, char** argv) {
  if (argc < 18) { fprintf(stderr, "usage: %s fixed0 off0 fixed1 off1 map poses sinv cols tau sum_order min_corr min_inliers max_chi_bits min_ratio_bits k steps warmup\n", argv[0]); return 2; }
  const std::vector<float> fx0 = read_all<float>(argv[1]), fx1 = read_all<float>(argv[3]), map = read_all<float>(argv[5]), poses = read_all<float>(argv[6]);
  const std::vector<int32_t> off0 = read_all<int32_t>(argv[2]), off1 = read_all<int32_t>(argv[4]);
  const std::vector<float> sinv = read_all<float>(argv[7]);      // [2][8]
  const int cols = atoi(argv[8]); const float tau = (float) atof(argv[9]); const int order = atoi(argv[10]); const int min_corr = atoi(argv[11]);
  const lsm2d_select_params select{atoi(argv[12]), from_bits_arg(argv[13]), from_bits_arg(argv[14])};
  const int32_t k = atoi(argv[15]); const int steps = atoi(argv[16]), warmup = atoi(argv[17]);
  const int32_t n = (int32_t) (poses.size() / 3);

  lsm2d_context* ctx = nullptr;
  must(lsm2d_create(0, nullptr, &ctx), "lsm2d_create", nullptr);
  must(lsm2d_set_option(ctx, "sum_order", order), "sum_order", ctx);
  lsm2d_cloudset *fixed[2] = {nullptr, nullptr}, *moving = nullptr;
  must(lsm2d_cloudset_create(ctx, fx0.data(), off0.data(), (int32_t) off0.size() - 1, (int64_t) (fx0.size() / 4), &fixed[0]), "fixed0", ctx);
  must(lsm2d_cloudset_create(ctx, fx1.data(), off1.data(), (int32_t) off1.size() - 1, (int64_t) (fx1.size() / 4), &fixed[1]), "fixed1", ctx);
  must(lsm2d_cloudset_create(ctx, map.data(), nullptr, 1, (int64_t) (map.size() / 4), &moving), "map", ctx);
  lsm2d_slice_params sp[2];
  for (int s = 0; s < 2; ++s) {
    sp[s] = lsm2d_slice_params{};
    sp[s].finder = LSM2D_FINDER_PROJECTIVE; sp[s].projector = lsm2d_projector{cols, -3.14159265358979f, 3.14159265358979f, 0.3f, 30.0f, 0.0f};
    sp[s].point_distance = 0.5f; sp[s].normal_cos = 0.8f; sp[s].robustifier = LSM2D_ROBUST_CAUCHY; sp[s].chi_threshold = tau;
    sp[s].min_num_correspondences = min_corr; memcpy(sp[s].sensor_in_robot, &sinv[8 * (size_t) s], sizeof(float) * 3);
  }
  const lsm2d_cloudset* fxp[2] = {fixed[0], fixed[1]}; const lsm2d_cloudset* mvp[2] = {moving, moving};
  lsm2d_batch B{}; B.n_alignments = n; B.n_slices = 2; B.slices = sp; B.fixed = fxp; B.moving = mvp; B.init_pose = poses.data();

  const size_t N = (size_t) n, K = (size_t) k;
  // ---- the new routes
  std::vector<float> H_new(9 * N), b_new(3 * N); std::vector<lsm2d_iteration_stats> st_new(N); std::vector<int32_t> act_new(N);
  auto new_batch = [&] { must(lsm2d_score_aligner_batch(ctx, &B, H_new.data(), b_new.data(), st_new.data(), act_new.data()), "lsm2d_score_aligner_batch", ctx); };
  std::vector<int32_t> idx_new(K), act_sel(K); std::vector<float> H_sel(9 * K), b_sel(3 * K); std::vector<lsm2d_iteration_stats> st_sel(K);
  int32_t n_sel_new = 0, n_acc_new = 0;
  auto new_select = [&] {
    must(lsm2d_score_aligner_select(ctx, &B, &select, k, idx_new.data(), H_sel.data(), b_sel.data(), st_sel.data(), act_sel.data(), &n_sel_new, &n_acc_new),
         "lsm2d_score_aligner_select", ctx);
  };
  // ---- the old route: per slice the caller's own effective poses and one lsm2d_score_batch (two waits, two full copies), then the combination on the host
  std::vector<float> Xe(3 * N), Hs[2], bs[2]; std::vector<lsm2d_iteration_stats> sts[2];
  for (int s = 0; s < 2; ++s) { Hs[s].resize(9 * N); bs[s].resize(3 * N); sts[s].resize(N); }
  std::vector<float> H_old(9 * N), b_old(3 * N); std::vector<lsm2d_iteration_stats> st_old(N); std::vector<int32_t> act_old(N);
  auto old_batch = [&] {
    for (int s = 0; s < 2; ++s) {
      const float* a = &sinv[8 * (size_t) s + 3]; const float c = sinv[8 * (size_t) s + 6], sn = sinv[8 * (size_t) s + 7];
      for (size_t i = 0; i < N; ++i) {
        const float* x = &poses[3 * i];
        Xe[3 * i] = fmaf(c, x[0], fmaf(-sn, x[1], a[0])); Xe[3 * i + 1] = fmaf(sn, x[0], fmaf(c, x[1], a[1])); Xe[3 * i + 2] = wrap(a[2] + x[2]);
      }
      must(lsm2d_score_batch(ctx, &sp[s], fixed[s], nullptr, moving, nullptr, n, Xe.data(), Hs[s].data(), bs[s].data(), sts[s].data()), "lsm2d_score_batch", ctx);
    }
    for (size_t i = 0; i < N; ++i) {
      float H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}; lsm2d_iteration_stats t{}; int32_t active = 0;
      for (int s = 0; s < 2; ++s) {
        const lsm2d_iteration_stats& r = sts[s][i];
        t.n_correspondences += r.n_correspondences;
        if (r.n_correspondences <= min_corr) continue;
        for (int c = 0; c < 9; ++c) H[c] += Hs[s][9 * i + (size_t) c];
        for (int c = 0; c < 3; ++c) b[c] += bs[s][3 * i + (size_t) c];
        t.n_inliers += r.n_inliers; t.n_outliers += r.n_outliers; t.chi_inliers += r.chi_inliers; t.chi_outliers += r.chi_outliers; ++active;
      }
      memcpy(&H_old[9 * i], H, sizeof H); memcpy(&b_old[3 * i], b, sizeof b); st_old[i] = t; act_old[i] = active;
    }
  };
  std::vector<std::pair<uint64_t, int32_t>> keyed; keyed.reserve(N);
  std::vector<int32_t> idx_old; int32_t n_acc_old = 0;
  auto old_select = [&] {
    old_batch();
    keyed.clear();
    for (int32_t i = 0; i < n; ++i) {
      const lsm2d_iteration_stats& s = st_old[(size_t) i];
      if (act_old[(size_t) i] > 0 && accept(s, select)) keyed.emplace_back(key_of(s), i);
    }
    n_acc_old = (int32_t) keyed.size();
    const size_t m = std::min(K, keyed.size());
    std::partial_sort(keyed.begin(), keyed.begin() + (std::ptrdiff_t) m, keyed.end());
    idx_old.resize(m);
    for (size_t j = 0; j < m; ++j) idx_old[j] = keyed[j].second;
  };

  must(lsm2d_set_option(ctx, "kernel_timing", 0), "kernel_timing", ctx);
  for (int w = 0; w < warmup; ++w) { new_batch(); old_batch(); new_select(); old_select(); }
  std::vector<double> t[4];
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  for (int s = 0; s < steps; ++s) {
    auto t0 = clk::now(); new_batch(); auto t1 = clk::now(); old_batch(); auto t2 = clk::now(); new_select(); auto t3 = clk::now(); old_select(); auto t4 = clk::now();
    t[0].push_back(ms(t0, t1)); t[1].push_back(ms(t1, t2)); t[2].push_back(ms(t2, t3)); t[3].push_back(ms(t3, t4));
  }
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "kernel_timing", ctx);
  float km[3] = {0.f, 0.f, 0.f};
  new_batch(); must(lsm2d_last_kernel_ms(ctx, &km[0]), "lsm2d_last_kernel_ms", ctx);
  new_select(); must(lsm2d_last_kernel_ms(ctx, &km[1]), "lsm2d_last_kernel_ms", ctx);
  old_batch(); must(lsm2d_last_kernel_ms(ctx, &km[2]), "lsm2d_last_kernel_ms", ctx);      // (the old route's second slice, last group)
  old_select();

  // ---- the routes agree: every row but for the digest (the old route's is salted with slice 0 in both slices), and the selections
  int rows_equal = 1;
  for (size_t i = 0; i < N && rows_equal; ++i)
    if (memcmp(&H_new[9 * i], &H_old[9 * i], 36) || memcmp(&b_new[3 * i], &b_old[3 * i], 12) || memcmp(&st_new[i], &st_old[i], 20) || act_new[i] != act_old[i]) rows_equal = 0;
  int select_equal = n_acc_new == n_acc_old && (size_t) n_sel_new == idx_old.size();
  for (int32_t j = 0; j < n_sel_new && select_equal; ++j) {
    const size_t i = (size_t) idx_new[(size_t) j];
    if (idx_new[(size_t) j] != idx_old[(size_t) j] || memcmp(&H_sel[9 * (size_t) j], &H_new[9 * i], 36) || memcmp(&st_sel[(size_t) j], &st_new[i], sizeof(lsm2d_iteration_stats)))
      select_equal = 0;
  }
  double s0[3], s1[3], s2[3], s3[3]; summary(t[0], s0); summary(t[1], s1); summary(t[2], s2); summary(t[3], s3);
  int32_t n_inactive = 0; for (size_t i = 0; i < N; ++i) n_inactive += act_new[i] == 0;
  printf("{\"n_items\": %d, \"n_slices\": 2, \"k\": %d, \"steps\": %d, \"batch_ms\": [%.4f, %.4f, %.4f], \"baseline_batch_ms\": [%.4f, %.4f, %.4f], "
         "\"select_ms\": [%.4f, %.4f, %.4f], \"baseline_select_ms\": [%.4f, %.4f, %.4f], \"batch_kernel_ms\": %.4f, \"select_kernel_ms\": %.4f, "
         "\"baseline_kernel_ms\": %.4f, \"rows_equal\": %d, \"select_equal\": %d, \"n_accepted\": %d, \"n_selected\": %d, \"n_inactive\": %d, \"best_item\": %d}\n",
         n, k, steps, s0[0], s0[1], s0[2], s1[0], s1[1], s1[2], s2[0], s2[1], s2[2], s3[0], s3[1], s3[2], km[0], km[1], km[2], rows_equal, select_equal,
         n_acc_new, n_sel_new, n_inactive, n_sel_new ? idx_new[0] : -1);
  lsm2d_cloudset_destroy(fixed[0]); lsm2d_cloudset_destroy(fixed[1]); lsm2d_cloudset_destroy(moving); lsm2d_destroy(ctx);
  return 0;
}
