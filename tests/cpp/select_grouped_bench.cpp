// Times the grouped select calls against the two routes a fleet server had before them, through the bare C ABI, all three in this process, alternating call by
// call:
//   select_grouped_bench MODE scans.bin offsets.bin map.bin poses.bin index.bin groups.bin cols tau iterations min_inliers max_chi_bits min_ratio_bits k steps warmup out.bin
// MODE align:  (a) lsm2d_align_select_grouped   (b) one lsm2d_align_select per group   (c) lsm2d_align_batch with statistics, the test and a partial sort
//              per group on the host.
// MODE score:  (a) lsm2d_score_select_grouped   (b) one lsm2d_score_select per group   (c) lsm2d_score_batch, the same on the host.
// n float32 poses; scans.bin holds ragged float32 [N,4] scans (int32 offsets), index.bin one int32 scan index per item, groups.bin the n_groups + 1 int32
// group offsets; one map every item is matched against.  Projective finder, Cauchy robustifier of threshold tau; the two float thresholds come as their bit
// patterns.  Parity is checked inside the run: per group, routes (a) and (b) name the items and counts route (c) names, and route (a)'s rows are route (c)'s
// rows of those items, byte for byte.  Prints one JSON line -- median, minimum and maximum of the wall clock around each route in ms, lsm2d_last_kernel_ms of
// one more grouped call -- and writes route (c)'s verdict inputs of all n items to out.bin (align: status [n], iterations [n], last rows [n]; score: rows
// [n]) followed by route (a)'s counts and indices ([G] accepted, [G] selected, [G x k] index) for the caller's own gate (tests/bench/select_grouped_bench.py).
#include <cstddef>

#include "driver_common.h"

// one route's verdict: per group the accepted and selected counts, the selected items in slots g * k + j
struct Verdict {
  std::vector<int32_t> n_acc, n_sel, index;
  Verdict(size_t G, size_t k) : n_acc(G, 0), n_sel(G, 0), index(G * k, -1) {}
  bool agrees(const Verdict& o, size_t k) const {
    if (n_acc != o.n_acc || n_sel != o.n_sel) return false;
    for (size_t g = 0; g < n_sel.size(); ++g)
      for (int32_t j = 0; j < n_sel[g]; ++j) if (index[g * k + (size_t) j] != o.index[g * k + (size_t) j]) return false;
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc < 18) { fprintf(stderr, "usage: %s align|score scans.bin offsets.bin map.bin poses.bin index.bin groups.bin cols tau iterations min_inliers max_chi_bits min_ratio_bits k steps warmup out.bin\n", argv[0]); return 2; }
  const bool align = std::string(argv[1]) == "align";
  const std::vector<float> scans = read_all<float>(argv[2]);
  const std::vector<int32_t> offs = read_all<int32_t>(argv[3]);
  const std::vector<float> map = read_all<float>(argv[4]);
  const std::vector<float> poses = read_all<float>(argv[5]);
  const std::vector<int32_t> index = read_all<int32_t>(argv[6]);
  const std::vector<int32_t> groups = read_all<int32_t>(argv[7]);
  const int cols = atoi(argv[8]); const float tau = (float) atof(argv[9]); const int iterations = atoi(argv[10]);
  const lsm2d_select_params select{atoi(argv[11]), from_bits_arg(argv[12]), from_bits_arg(argv[13])};
  const int32_t k = atoi(argv[14]); const int steps = atoi(argv[15]), warmup = atoi(argv[16]);
  const int32_t n = (int32_t) (poses.size() / 3), n_scans = (int32_t) offs.size() - 1, G = (int32_t) groups.size() - 1;
  if ((int32_t) index.size() != n || G < 1 || groups[(size_t) G] != n || k < 1) { fprintf(stderr, "index.bin: one entry per item; groups.bin: offsets from 0 to n\n"); return 2; }
  const size_t K = (size_t) k, rows = (size_t) G * K;

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
  lsm2d_batch b{}; b.n_alignments = n; b.n_slices = 1; b.slices = &sp; b.fixed = fx; b.moving = mv; b.fixed_index = index.data(); b.init_pose = poses.data();
  const size_t cap = align ? (size_t) lsm2d_stats_capacity(&ap) : 1;

  // (a) the grouped call: n_groups x k rows come down
  Verdict va((size_t) G, K), vb((size_t) G, K), vc((size_t) G, K);
  std::vector<int32_t> its_a(rows), suc_a((size_t) G, 0); std::vector<float> pose_a(3 * rows), H_a(9 * rows), b_a(3 * rows); std::vector<lsm2d_iteration_stats> st_a(rows);
  auto route_a = [&] {
    if (align) must(lsm2d_align_select_grouped(ctx, &ap, &b, &select, k, G, groups.data(), va.index.data(), pose_a.data(), H_a.data(), its_a.data(), st_a.data(),
                                               va.n_sel.data(), va.n_acc.data(), suc_a.data()), "lsm2d_align_select_grouped", ctx);
    else must(lsm2d_score_select_grouped(ctx, &sp, fixed, index.data(), moving, nullptr, n, poses.data(), &select, k, G, groups.data(), va.index.data(), H_a.data(),
                                         b_a.data(), st_a.data(), va.n_sel.data(), va.n_acc.data()), "lsm2d_score_select_grouped", ctx);
  };
  // (b) one ungrouped select call per group, one after another: G copies down, G waits
  std::vector<int32_t> its_b(K), idx_b(K); std::vector<float> pose_b(3 * K), H_b(9 * K), b_b(3 * K); std::vector<lsm2d_iteration_stats> st_b(K);
  auto route_b = [&] {
    for (int32_t g = 0; g < G; ++g) {
      const int32_t lo = groups[(size_t) g], m = groups[(size_t) g + 1] - lo;
      int32_t n_sel = 0, n_acc = 0, n_suc = 0;
      if (align) {
        lsm2d_batch s = b; s.n_alignments = m; s.fixed_index = index.data() + lo; s.init_pose = poses.data() + 3 * (size_t) lo;
        must(lsm2d_align_select(ctx, &ap, &s, &select, k, idx_b.data(), pose_b.data(), H_b.data(), its_b.data(), st_b.data(), &n_sel, &n_acc, &n_suc), "lsm2d_align_select", ctx);
      } else
        must(lsm2d_score_select(ctx, &sp, fixed, index.data() + lo, moving, nullptr, m, poses.data() + 3 * (size_t) lo, &select, k, idx_b.data(), H_b.data(), b_b.data(),
                                st_b.data(), &n_sel, &n_acc), "lsm2d_score_select", ctx);
      vb.n_sel[(size_t) g] = n_sel; vb.n_acc[(size_t) g] = n_acc;
      for (int32_t j = 0; j < n_sel; ++j) vb.index[(size_t) g * K + (size_t) j] = idx_b[(size_t) j] + lo;
    }
  };
  // (c) one batch call with everything coming down, then the same fp32 test and the same total order per group on the host (a partial sort of each group's
  // accepted items)
  std::vector<float> pose((size_t) n * 3), H((size_t) n * 9), bb((size_t) n * 3); std::vector<int32_t> status((size_t) n, 0), its((size_t) n, 1);
  std::vector<lsm2d_iteration_stats> st((size_t) n * cap);
  std::vector<std::pair<uint64_t, int32_t>> keyed; keyed.reserve((size_t) n);
  auto last_row = [&](int32_t i) -> const lsm2d_iteration_stats& { return st[(size_t) i * cap + (size_t) (align ? its[(size_t) i] - 1 : 0)]; };
  auto route_c = [&] {
    if (align) must(lsm2d_align_batch(ctx, &ap, &b, pose.data(), H.data(), status.data(), its.data(), st.data()), "lsm2d_align_batch", ctx);
    else must(lsm2d_score_batch(ctx, &sp, fixed, index.data(), moving, nullptr, n, poses.data(), H.data(), bb.data(), st.data()), "lsm2d_score_batch", ctx);
    for (int32_t g = 0; g < G; ++g) {
      keyed.clear();
      for (int32_t i = groups[(size_t) g]; i < groups[(size_t) g + 1]; ++i) {
        if (align && (status[(size_t) i] != LSM2D_SUCCESS || its[(size_t) i] < 1)) continue;
        if (accept(last_row(i), select)) keyed.emplace_back(key_of(last_row(i)), i);
      }
      const size_t m = std::min(K, keyed.size());
      std::partial_sort(keyed.begin(), keyed.begin() + (std::ptrdiff_t) m, keyed.end());
      vc.n_acc[(size_t) g] = (int32_t) keyed.size(); vc.n_sel[(size_t) g] = (int32_t) m;
      for (size_t j = 0; j < m; ++j) vc.index[(size_t) g * K + j] = keyed[j].second;
    }
  };

  must(lsm2d_set_option(ctx, "kernel_timing", 0), "kernel_timing", ctx);
  for (int w = 0; w < warmup; ++w) { route_a(); route_b(); route_c(); }
  std::vector<double> ta, tb, tc;
  using clk = std::chrono::steady_clock;
  for (int s = 0; s < steps; ++s) {
    auto t0 = clk::now(); route_a(); auto t1 = clk::now(); route_b(); auto t2 = clk::now(); route_c(); auto t3 = clk::now();
    ta.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); tb.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    tc.push_back(std::chrono::duration<double, std::milli>(t3 - t2).count());
  }
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "kernel_timing", ctx);
  float k_a = 0.f;
  route_c(); route_b(); route_a(); must(lsm2d_last_kernel_ms(ctx, &k_a), "lsm2d_last_kernel_ms", ctx);

  // parity: the three verdicts agree, and the grouped call's rows are the batch call's rows of the selected items
  const int a_is_c = va.agrees(vc, K), b_is_c = vb.agrees(vc, K);
  int rows_equal = 1; long long n_acc_all = 0, n_sel_all = 0;
  for (int32_t g = 0; g < G && rows_equal; ++g) {
    n_acc_all += va.n_acc[(size_t) g]; n_sel_all += va.n_sel[(size_t) g];
    for (int32_t j = 0; j < va.n_sel[(size_t) g] && rows_equal; ++j) {
      const size_t slot = (size_t) g * K + (size_t) j; const int32_t i = va.index[slot];
      if (i < groups[(size_t) g] || i >= groups[(size_t) g + 1] || memcmp(&H_a[9 * slot], &H[9 * (size_t) i], 36) || memcmp(&st_a[slot], &last_row(i), sizeof(lsm2d_iteration_stats))) rows_equal = 0;
      else if (align && (memcmp(&pose_a[3 * slot], &pose[3 * (size_t) i], 12) || its_a[slot] != its[(size_t) i])) rows_equal = 0;
      else if (!align && memcmp(&b_a[3 * slot], &bb[3 * (size_t) i], 12)) rows_equal = 0;
    }
  }
  std::vector<lsm2d_iteration_stats> last((size_t) n);
  for (int32_t i = 0; i < n; ++i) {
    lsm2d_iteration_stats z; memset(&z, 0, sizeof z);
    last[(size_t) i] = (!align || its[(size_t) i] >= 1) ? last_row(i) : z;
  }
  FILE* f = fopen(argv[17], "wb");
  bool ok = f != nullptr;
  if (ok && align) ok = fwrite(status.data(), sizeof(int32_t), (size_t) n, f) == (size_t) n && fwrite(its.data(), sizeof(int32_t), (size_t) n, f) == (size_t) n;
  ok = ok && fwrite(last.data(), sizeof(lsm2d_iteration_stats), (size_t) n, f) == (size_t) n && fwrite(va.n_acc.data(), sizeof(int32_t), (size_t) G, f) == (size_t) G &&
       fwrite(va.n_sel.data(), sizeof(int32_t), (size_t) G, f) == (size_t) G && fwrite(va.index.data(), sizeof(int32_t), rows, f) == rows;
  if (!ok) { perror(argv[17]); return 2; }
  fclose(f);
  double sa[3], sb[3], sc[3]; summary(ta, sa); summary(tb, sb); summary(tc, sc);
  printf("{\"mode\": \"%s\", \"n_items\": %d, \"n_groups\": %d, \"k\": %d, \"steps\": %d, \"stats_rows_per_item\": %zu, \"grouped_ms\": [%.4f, %.4f, %.4f], "
         "\"per_group_calls_ms\": [%.4f, %.4f, %.4f], \"batch_and_host_ms\": [%.4f, %.4f, %.4f], \"grouped_kernel_ms\": %.4f, \"grouped_is_host\": %d, "
         "\"per_group_calls_is_host\": %d, \"rows_equal\": %d, \"n_accepted\": %lld, \"n_selected\": %lld}\n",
         argv[1], n, G, k, steps, cap, sa[0], sa[1], sa[2], sb[0], sb[1], sb[2], sc[0], sc[1], sc[2], k_a, a_is_c, b_is_c, rows_equal, n_acc_all, n_sel_all);
  lsm2d_cloudset_destroy(fixed); lsm2d_cloudset_destroy(moving); lsm2d_destroy(ctx);
  return 0;
}
