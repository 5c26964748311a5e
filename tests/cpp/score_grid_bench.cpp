// Times lsm2d_score_grid_select against the same pyramid made of existing calls, through the bare C ABI, all routes in this process, alternating call by call:
//   score_grid_bench scan.bin map.bin cols tau c0 c1 c2 s0 s1 s2 (float bits) min_inliers max_chi_bits min_ratio_bits nobody steps warmup
// ONE scan against one map, projective finder, Cauchy robustifier of threshold tau.  (c0 c1 c2) is the grid's centre, (s0 s1 s2) the spacing of the COARSE
// grid of 16 x 16 x 16 cells.  Two pyramids of the same final resolution: "two" = refine (4, 4, 1) once, "three" = refine (2, 2, 1) twice; k_parents 64, k 64.
//   route a  lsm2d_score_grid_select
//   route b  the same pyramid from lsm2d_score_aligner_select per level, the children made on the host by the header's formulas (the yardstick: existing
//            entry points); it stops at the first level that selects nothing
//   route c  the exhaustive 64 x 64 x 16 grid through lsm2d_score_aligner_select, its poses made once outside the timing (for context)
// nobody = 1: the coarse thresholds pass nobody -- what the pads cost when route b stops after level 0.  Prints one JSON line: medians, minima and maxima of
// the wall clock in ms, lsm2d_last_kernel_ms of one more call of route a, whether routes a and b agree byte for byte, and how far a's best pose lies from c's.
#include <cmath>
#include <cstddef>

#include "driver_common.h"

// base + (o * s): two roundings (volatile keeps the compiler from contracting them)
static float coord(float base, int i, int n, float s) { volatile float o = (float) i - 0.5f * (float) (n - 1); volatile float p = o * s; volatile float r = base + p; return r; }

struct Answer {
  std::vector<float> pose, H, b; std::vector<int32_t> origin, active, counts; std::vector<lsm2d_iteration_stats> stats; int32_t n_sel = 0, n_acc = 0;
  explicit Answer(size_t k) : pose(3 * k), H(9 * k), b(3 * k), origin(k), active(k), counts(2 * LSM2D_GRID_MAX_LEVELS, 0), stats(k) {}
  bool equals(const Answer& o, int levels) const {
    if (n_sel != o.n_sel || n_acc != o.n_acc || memcmp(counts.data(), o.counts.data(), 8 * (size_t) levels)) return false;
    const size_t m = (size_t) n_sel;
    return !memcmp(pose.data(), o.pose.data(), 12 * m) && !memcmp(H.data(), o.H.data(), 36 * m) && !memcmp(b.data(), o.b.data(), 12 * m) &&
           !memcmp(origin.data(), o.origin.data(), 4 * m) && !memcmp(active.data(), o.active.data(), 4 * m) &&
           !memcmp(stats.data(), o.stats.data(), sizeof(lsm2d_iteration_stats) * m);
  }
};

int main(int argc, char** argv) {
  if (argc < 17) { fprintf(stderr, "usage: %s scan.bin map.bin cols tau <6 float bits> min_inliers max_chi_bits min_ratio_bits nobody steps warmup\n", argv[0]); return 2; }
  const std::vector<float> scan = read_all<float>(argv[1]), map = read_all<float>(argv[2]);
  const int cols = atoi(argv[3]); const float tau = (float) atof(argv[4]);
  float center[3], step[3];
  for (int a = 0; a < 3; ++a) { center[a] = from_bits_arg(argv[5 + a]); step[a] = from_bits_arg(argv[8 + a]); }
  const lsm2d_select_params select{atoi(argv[11]), from_bits_arg(argv[12]), from_bits_arg(argv[13])};
  const bool nobody = atoi(argv[14]) != 0; const int steps = atoi(argv[15]), warmup = atoi(argv[16]);
  const lsm2d_select_params none{1000000000, 0.0f, 2.0f};
  const lsm2d_select_params coarse = nobody ? none : select;
  const int32_t K = 64;

  lsm2d_context* ctx = nullptr;
  must(lsm2d_create(0, nullptr, &ctx), "lsm2d_create", nullptr);
  lsm2d_cloudset *fixed = nullptr, *moving = nullptr;
  must(lsm2d_cloudset_create(ctx, scan.data(), nullptr, 1, (int64_t) (scan.size() / 4), &fixed), "scan", ctx);
  must(lsm2d_cloudset_create(ctx, map.data(), nullptr, 1, (int64_t) (map.size() / 4), &moving), "map", ctx);
  lsm2d_slice_params sp{};
  sp.finder = LSM2D_FINDER_PROJECTIVE; sp.projector = lsm2d_projector{cols, -3.14159265358979f, 3.14159265358979f, 0.3f, 30.0f, 0.0f};
  sp.point_distance = 0.5f; sp.normal_cos = 0.8f; sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = tau; sp.min_num_correspondences = 10;
  const lsm2d_cloudset* fx[1] = {fixed}; const lsm2d_cloudset* mv[1] = {moving};

  lsm2d_pose_grid grids[2];
  for (int p = 0; p < 2; ++p) {
    lsm2d_pose_grid& g = grids[p];
    for (int a = 0; a < 3; ++a) { g.center[a] = center[a]; g.step[a] = step[a]; g.count[a] = 16; }
    g.n_levels = p == 0 ? 2 : 3; g.refine[0] = g.refine[1] = p == 0 ? 4 : 2; g.refine[2] = 1; g.k_parents = K;
  }
  // the exhaustive grid: 64 x 64 x 16 at the pyramids' final spacing
  const int ex[3] = {64, 64, 16}; const float es[3] = {step[0] / 4.0f, step[1] / 4.0f, step[2]};
  std::vector<float> all((size_t) 3 * 64 * 64 * 16);
  for (int it = 0; it < ex[2]; ++it) for (int iy = 0; iy < ex[1]; ++iy) for (int ix = 0; ix < ex[0]; ++ix) {
    float* q = &all[3 * (((size_t) it * 64 + (size_t) iy) * 64 + (size_t) ix)];
    q[0] = coord(center[0], ix, 64, es[0]); q[1] = coord(center[1], iy, 64, es[1]); q[2] = coord(center[2], it, 16, es[2]);
  }

  Answer A[2] = {Answer((size_t) K), Answer((size_t) K)}, B[2] = {Answer((size_t) K), Answer((size_t) K)};
  auto route_a = [&](int p) {
    Answer& a = A[p];
    must(lsm2d_score_grid_select(ctx, 1, &sp, fx, nullptr, mv, nullptr, &grids[p], &coarse, &select, K, a.pose.data(), a.origin.data(), a.H.data(), a.b.data(),
                                 a.stats.data(), a.active.data(), &a.n_sel, &a.n_acc, a.counts.data()), "lsm2d_score_grid_select", ctx);
  };
  std::vector<float> poses, next; std::vector<int32_t> origins, next_origins, index((size_t) K);
  auto route_b = [&](int p) {
    Answer& a = B[p]; const lsm2d_pose_grid& g = grids[p];
    std::fill(a.counts.begin(), a.counts.end(), 0); a.n_sel = a.n_acc = 0;
    const int n0 = g.count[0] * g.count[1] * g.count[2], R = g.refine[0] * g.refine[1] * g.refine[2];
    poses.resize(3 * (size_t) n0); origins.resize((size_t) n0);
    for (int i = 0; i < n0; ++i) {
      const int ix = i % g.count[0], iy = (i / g.count[0]) % g.count[1], it = i / (g.count[0] * g.count[1]);
      poses[3 * (size_t) i] = coord(g.center[0], ix, g.count[0], g.step[0]); poses[3 * (size_t) i + 1] = coord(g.center[1], iy, g.count[1], g.step[1]);
      poses[3 * (size_t) i + 2] = coord(g.center[2], it, g.count[2], g.step[2]); origins[(size_t) i] = i;
    }
    float s[3] = {g.step[0], g.step[1], g.step[2]};
    for (int l = 0; l < g.n_levels; ++l) {
      const bool last = l == g.n_levels - 1;
      lsm2d_batch b{}; b.n_alignments = (int32_t) (poses.size() / 3); b.n_slices = 1; b.slices = &sp; b.fixed = fx; b.moving = mv; b.init_pose = poses.data();
      int32_t n_sel = 0, n_acc = 0;
      must(lsm2d_score_aligner_select(ctx, &b, last ? &select : &coarse, K, index.data(), a.H.data(), a.b.data(), a.stats.data(), a.active.data(), &n_sel, &n_acc),
           "lsm2d_score_aligner_select", ctx);
      a.counts[2 * (size_t) l] = n_acc; a.counts[2 * (size_t) l + 1] = n_sel;
      if (last) {
        a.n_sel = n_sel; a.n_acc = n_acc;
        for (int32_t j = 0; j < n_sel; ++j) { memcpy(&a.pose[3 * (size_t) j], &poses[3 * (size_t) index[(size_t) j]], 12); a.origin[(size_t) j] = origins[(size_t) index[(size_t) j]]; }
        break;
      }
      if (n_sel == 0) break;      // the host can stop early
      for (int a3 = 0; a3 < 3; ++a3) s[a3] = s[a3] / (float) g.refine[a3];
      next.resize(3 * (size_t) n_sel * (size_t) R); next_origins.resize((size_t) n_sel * (size_t) R);
      for (int32_t j = 0; j < n_sel; ++j) {
        const float* base = &poses[3 * (size_t) index[(size_t) j]];
        for (int c = 0; c < R; ++c) {
          const int cx = c % g.refine[0], cy = (c / g.refine[0]) % g.refine[1], ct = c / (g.refine[0] * g.refine[1]);
          float* q = &next[3 * ((size_t) j * (size_t) R + (size_t) c)];
          q[0] = coord(base[0], cx, g.refine[0], s[0]); q[1] = coord(base[1], cy, g.refine[1], s[1]); q[2] = coord(base[2], ct, g.refine[2], s[2]);
          next_origins[(size_t) j * (size_t) R + (size_t) c] = origins[(size_t) index[(size_t) j]];
        }
      }
      poses.swap(next); origins.swap(next_origins);
    }
  };
  Answer Cx((size_t) K); std::vector<int32_t> c_index((size_t) K);
  auto route_c = [&] {
    lsm2d_batch b{}; b.n_alignments = 64 * 64 * 16; b.n_slices = 1; b.slices = &sp; b.fixed = fx; b.moving = mv; b.init_pose = all.data();
    must(lsm2d_score_aligner_select(ctx, &b, &select, K, c_index.data(), Cx.H.data(), Cx.b.data(), Cx.stats.data(), Cx.active.data(), &Cx.n_sel, &Cx.n_acc),
         "lsm2d_score_aligner_select", ctx);
  };

  must(lsm2d_set_option(ctx, "kernel_timing", 0), "kernel_timing", ctx);
  for (int w = 0; w < warmup; ++w) { for (int p = 0; p < 2; ++p) { route_a(p); route_b(p); } route_c(); }
  std::vector<double> ta[2], tb[2], tc;
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  for (int s = 0; s < steps; ++s) {
    for (int p = 0; p < 2; ++p) {
      auto t0 = clk::now(); route_a(p); auto t1 = clk::now(); route_b(p); auto t2 = clk::now();
      ta[p].push_back(ms(t0, t1)); tb[p].push_back(ms(t1, t2));
    }
    auto t0 = clk::now(); route_c(); auto t1 = clk::now(); tc.push_back(ms(t0, t1));
  }
  const int equal[2] = {A[0].equals(B[0], 2) ? 1 : 0, A[1].equals(B[1], 3) ? 1 : 0};
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "kernel_timing", ctx);
  float ka[2] = {0.f, 0.f}, kc = 0.f;
  for (int p = 0; p < 2; ++p) { route_a(p); must(lsm2d_last_kernel_ms(ctx, &ka[p]), "lsm2d_last_kernel_ms", ctx); }
  route_c(); must(lsm2d_last_kernel_ms(ctx, &kc), "lsm2d_last_kernel_ms", ctx);
  double sa[2][3], sb[2][3], sc[3];
  for (int p = 0; p < 2; ++p) { summary(ta[p], sa[p]); summary(tb[p], sb[p]); }
  summary(tc, sc);
  // a's best against c's best
  printf("{\"steps\": %d, \"nobody\": %d, \"exhaustive_ms\": [%.4f, %.4f, %.4f], \"exhaustive_kernel_ms\": %.4f, \"exhaustive_accepted\": %d, \"pyramids\": [", steps,
         nobody ? 1 : 0, sc[0], sc[1], sc[2], kc, Cx.n_acc);
  for (int p = 0; p < 2; ++p) {
    const Answer& a = A[p];
    double dist = -1.0, dth = -1.0; int same_cell = -1;
    if (a.n_sel > 0 && Cx.n_sel > 0) {
      const int32_t ci = c_index[0]; const float* q = &all[3 * (size_t) ci];
      dist = std::hypot((double) a.pose[0] - (double) q[0], (double) a.pose[1] - (double) q[1]); dth = std::fabs((double) a.pose[2] - (double) q[2]);
      const int ix = ci % 64, iy = (ci / 64) % 64, it = ci / (64 * 64);
      same_cell = a.origin[0] == (it * 16 + iy / 4) * 16 + ix / 4 ? 1 : 0;
    }
    printf("%s{\"n_levels\": %d, \"refine\": [%d, %d, %d], \"grid_ms\": [%.4f, %.4f, %.4f], \"per_level_ms\": [%.4f, %.4f, %.4f], \"grid_kernel_ms\": %.4f, "
           "\"outputs_equal\": %d, \"level_counts\": [", p ? ", " : "", grids[p].n_levels, grids[p].refine[0], grids[p].refine[1], grids[p].refine[2], sa[p][0], sa[p][1],
           sa[p][2], sb[p][0], sb[p][1], sb[p][2], ka[p], equal[p]);
    for (int l = 0; l < grids[p].n_levels; ++l) printf("%s[%d, %d]", l ? ", " : "", a.counts[2 * (size_t) l], a.counts[2 * (size_t) l + 1]);
    printf("], \"best_to_exhaustive_best_m\": %.6f, \"best_to_exhaustive_best_rad\": %.6f, \"same_level0_cell\": %d}", dist, dth, same_cell);
  }
  printf("]}\n");
  lsm2d_cloudset_destroy(fixed); lsm2d_cloudset_destroy(moving); lsm2d_destroy(ctx);
  return 0;
}
