// N independent live trackers through the bare C ABI, two ways in the same process: ONE batched step for all of them
// (lsm2d_preprocess_scans_refill x 2, lsm2d_clip_scene_batch, lsm2d_align_batch with n = N, lsm2d_merge_scene_batch) and the same trackers
// stepped one after another with the single-tracker calls (lsm2d_preprocess_scan_into x 2, lsm2d_clip_scene, lsm2d_align_batch with n = 1,
// lsm2d_merge_scenes: tests/cpp/track_step_bench.cpp's mode 2).  Every pose of every step must be the same bits on both sides.
//   track_batch_driver dir n_scenarios steps n_beams angle_min angle_max n_trackers episodes
// dir holds ranges.bin (float32 [n_scenarios][steps + 1][2][n_beams]), odo.bin (float64 [n_scenarios][steps][3]), start.bin (float64 [n_scenarios][3]);
// tracker j runs scenario j % n_scenarios.  An episode starts every tracker's local map from step 0's scans and runs steps 1 .. steps; episodes
// alternate between the two sides, the first of each side is a warm-up.  Prints one JSON line.
#include <cmath>

#include "driver_common.h"

static void compose(const double a[3], const double b[3], double o[3]) {
  const double c = cos(a[2]), s = sin(a[2]);
  o[0] = a[0] + c * b[0] - s * b[1]; o[1] = a[1] + s * b[0] + c * b[1]; o[2] = a[2] + b[2];
}
static void inverse(const double a[3], double o[3]) {
  const double c = cos(a[2]), s = sin(a[2]);
  o[0] = -(c * a[0] + s * a[1]); o[1] = -(-s * a[0] + c * a[1]); o[2] = -a[2];
}
#define CK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s -> %d (%s)\n", #x, rc_, lsm2d_last_error(ctx)); exit(1); } } while (0)

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s dir n_scenarios steps n_beams angle_min angle_max n_trackers episodes\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const int M = atoi(argv[2]), S = atoi(argv[3]), nb = atoi(argv[4]), N = atoi(argv[7]), episodes = atoi(argv[8]);
  const std::vector<float> ranges = read_all<float>(dir + "/ranges.bin");
  const std::vector<double> odo = read_all<double>(dir + "/odo.bin"), start = read_all<double>(dir + "/start.bin");
  if ((long) ranges.size() != (long) M * (S + 1) * 2 * nb || (long) odo.size() != (long) M * S * 3 || (long) start.size() != (long) M * 3) { fprintf(stderr, "bad inputs\n"); return 2; }
  auto rng = [&](int scen, int k, int sensor) { return ranges.data() + (((size_t) scen * (S + 1) + k) * 2 + sensor) * nb; };
  lsm2d_preprocessor pp; memset(&pp, 0, sizeof pp);
  pp.n_beams = nb; pp.angle_min = (float) atof(argv[5]); pp.angle_max = (float) atof(argv[6]);
  pp.range_min = 0.3f; pp.range_max = 20.0f; pp.normal_point_distance = 0.3f; pp.normal_min_points = 5; pp.voxelize_resolution = 0.02f;
  const lsm2d_projector pr = {721, -(float) M_PI, (float) M_PI, 0.3f, 20.0f, 0.0f};
  const float S0[3] = {0.2f, 0.1f, 0.1f}, S1[3] = {-0.3f, 0.0f, (float) M_PI};
  const double Sd[2][3] = {{S0[0], S0[1], S0[2]}, {S1[0], S1[1], S1[2]}};
  lsm2d_slice_params sl[2]; memset(sl, 0, sizeof sl);
  for (int i = 0; i < 2; ++i) {
    sl[i].finder = LSM2D_FINDER_PROJECTIVE; sl[i].projector = pr; sl[i].point_distance = 0.5f; sl[i].normal_cos = i ? 0.8f : 0.9f;
    sl[i].robustifier = i ? LSM2D_ROBUST_NONE : LSM2D_ROBUST_CAUCHY; sl[i].chi_threshold = 0.01f; sl[i].min_num_correspondences = 5;
    memcpy(sl[i].sensor_in_robot, i ? S1 : S0, sizeof S0);
  }
  const lsm2d_aligner_params ap = {10, 10, 0.0f, 0.0f, 0, 0};
  lsm2d_context* ctx = nullptr;
  CK(lsm2d_create(0, nullptr, &ctx));
  std::vector<lsm2d_prior> prior((size_t) N);
  for (auto& p : prior) { memset(&p, 0, sizeof p); p.omega[0] = p.omega[4] = p.omega[8] = 100.0f; }
  const int map_cap = 50000;
  // ---- the batched side's sets
  lsm2d_cloudset *maps = nullptr, *clipped = nullptr, *front = nullptr, *rear = nullptr;
  CK(lsm2d_cloudset_create_reserved_many(ctx, N, map_cap, &maps));
  CK(lsm2d_cloudset_create_reserved_many(ctx, N, pr.canvas_cols, &clipped));
  std::vector<std::vector<float>> rk((size_t) (S + 1) * 2, std::vector<float>((size_t) N * nb));      // [step][sensor]: every tracker's ranges, tracker-major
  for (int k = 0; k <= S; ++k) for (int s = 0; s < 2; ++s) for (int j = 0; j < N; ++j) memcpy(rk[(size_t) k * 2 + s].data() + (size_t) j * nb, rng(j % M, k, s), sizeof(float) * nb);
  CK(lsm2d_preprocess_scans(ctx, &pp, rk[0].data(), N, &front)); CK(lsm2d_preprocess_scans(ctx, &pp, rk[1].data(), N, &rear));
  // ---- the sequential side's sets: one tracker's worth each
  std::vector<lsm2d_cloudset*> smap((size_t) N), sclip((size_t) N), sm0((size_t) N), sm1((size_t) N);
  for (int j = 0; j < N; ++j) {
    CK(lsm2d_cloudset_create_reserved(ctx, map_cap, &smap[j])); CK(lsm2d_cloudset_create_reserved(ctx, pr.canvas_cols, &sclip[j]));
    CK(lsm2d_cloudset_create_reserved(ctx, 1024, &sm0[j])); CK(lsm2d_cloudset_create_reserved(ctx, 1024, &sm1[j]));
  }
  std::vector<float> pose_b((size_t) S * N * 3), pose_s((size_t) S * N * 3);
  std::vector<int32_t> st_b((size_t) S * N), st_s((size_t) S * N);
  std::vector<double> est((size_t) N * 3);
  std::vector<float> g32((size_t) N * 3), mis((size_t) N * 6), x((size_t) N * 3);
  auto sensor_poses = [&](int j, float* out) {
    for (int s = 0; s < 2; ++s) { double m[3]; compose(&est[(size_t) j * 3], Sd[s], m); for (int c = 0; c < 3; ++c) out[3 * s + c] = (float) m[c]; }
  };
  double t_batch = 0, t_seq = 0; int n_batch = 0, n_seq = 0;
  for (int e = 0; e < 2 * episodes; ++e) {
    const bool batched = (e & 1) == 0, timed = e >= 2;
    for (int j = 0; j < N; ++j) memcpy(&est[(size_t) j * 3], &start[(size_t) (j % M) * 3], sizeof(double) * 3);
    if (batched) {           // a new local map for every tracker: clear, both step-0 scans merged at the start pose
      CK(lsm2d_cloudset_clear_clouds(maps, 0, nullptr));
      CK(lsm2d_preprocess_scans_refill(ctx, &pp, rk[0].data(), N, front)); CK(lsm2d_preprocess_scans_refill(ctx, &pp, rk[1].data(), N, rear));
      for (int j = 0; j < N; ++j) sensor_poses(j, &mis[(size_t) j * 6]);
      const lsm2d_cloudset* ms[2] = {front, rear};
      CK(lsm2d_merge_scene_batch(ctx, &pr, maps, N, nullptr, 2, ms, nullptr, mis.data(), 0.2f, nullptr, nullptr));
    } else {
      for (int j = 0; j < N; ++j) {
        CK(lsm2d_cloudset_upload(smap[j], nullptr, 0));
        CK(lsm2d_preprocess_scan_into(ctx, &pp, rng(j % M, 0, 0), sm0[j])); CK(lsm2d_preprocess_scan_into(ctx, &pp, rng(j % M, 0, 1), sm1[j]));
        sensor_poses(j, &mis[(size_t) j * 6]);
        const lsm2d_cloudset* ms[2] = {sm0[j], sm1[j]};
        CK(lsm2d_merge_scenes(ctx, &pr, smap[j], 2, ms, nullptr, &mis[(size_t) j * 6], 0.2f, nullptr, nullptr));
      }
    }
    CK(lsm2d_synchronize(ctx));
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 1; k <= S; ++k) {
      for (int j = 0; j < N; ++j) {
        double g[3]; compose(&est[(size_t) j * 3], &odo[((size_t) (j % M) * S + (k - 1)) * 3], g);
        for (int c = 0; c < 3; ++c) g32[(size_t) j * 3 + c] = (float) g[c];
      }
      float* xo = (batched ? pose_b : pose_s).data() + (size_t) (k - 1) * N * 3;
      int32_t* so = (batched ? st_b : st_s).data() + (size_t) (k - 1) * N;
      if (batched) {
        CK(lsm2d_preprocess_scans_refill(ctx, &pp, rk[(size_t) k * 2].data(), N, front)); CK(lsm2d_preprocess_scans_refill(ctx, &pp, rk[(size_t) k * 2 + 1].data(), N, rear));
        CK(lsm2d_clip_scene_batch(ctx, &pr, maps, N, nullptr, g32.data(), S0, clipped, nullptr));
        const lsm2d_cloudset* fixed[2] = {front, rear}; const lsm2d_cloudset* moving[2] = {clipped, clipped};
        std::vector<float> x0((size_t) N * 3, 0.0f);
        lsm2d_batch b; memset(&b, 0, sizeof b);
        b.n_alignments = N; b.n_slices = 2; b.slices = sl; b.fixed = fixed; b.moving = moving; b.init_pose = x0.data(); b.prior = prior.data();
        CK(lsm2d_align_batch(ctx, &ap, &b, xo, nullptr, so, nullptr, nullptr));
        for (int j = 0; j < N; ++j) {
          const double xd[3] = {xo[3 * j], xo[3 * j + 1], xo[3 * j + 2]}, gd[3] = {g32[3 * j], g32[3 * j + 1], g32[3 * j + 2]};
          double xi[3]; inverse(xd, xi); compose(gd, xi, &est[(size_t) j * 3]); sensor_poses(j, &mis[(size_t) j * 6]);
        }
        const lsm2d_cloudset* ms[2] = {front, rear};
        CK(lsm2d_merge_scene_batch(ctx, &pr, maps, N, nullptr, 2, ms, nullptr, mis.data(), 0.2f, nullptr, nullptr));
      } else {
        for (int j = 0; j < N; ++j) {
          CK(lsm2d_clip_scene(ctx, &pr, smap[j], 0, &g32[(size_t) j * 3], S0, sclip[j], nullptr, nullptr));
          CK(lsm2d_preprocess_scan_into(ctx, &pp, rng(j % M, k, 0), sm0[j])); CK(lsm2d_preprocess_scan_into(ctx, &pp, rng(j % M, k, 1), sm1[j]));
          const lsm2d_cloudset* fixed[2] = {sm0[j], sm1[j]}; const lsm2d_cloudset* moving[2] = {sclip[j], sclip[j]};
          const float x0[3] = {0, 0, 0};
          lsm2d_batch b; memset(&b, 0, sizeof b);
          b.n_alignments = 1; b.n_slices = 2; b.slices = sl; b.fixed = fixed; b.moving = moving; b.init_pose = x0; b.prior = &prior[0];
          CK(lsm2d_align_batch(ctx, &ap, &b, xo + 3 * j, nullptr, so + j, nullptr, nullptr));
          const double xd[3] = {xo[3 * j], xo[3 * j + 1], xo[3 * j + 2]}, gd[3] = {g32[3 * j], g32[3 * j + 1], g32[3 * j + 2]};
          double xi[3]; inverse(xd, xi); compose(gd, xi, &est[(size_t) j * 3]); sensor_poses(j, &mis[(size_t) j * 6]);
          const lsm2d_cloudset* ms[2] = {sm0[j], sm1[j]};
          CK(lsm2d_merge_scenes(ctx, &pr, smap[j], 2, ms, nullptr, &mis[(size_t) j * 6], 0.2f, nullptr, nullptr));
        }
      }
    }
    CK(lsm2d_synchronize(ctx));
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (timed) { if (batched) { t_batch += dt; n_batch += S; } else { t_seq += dt; n_seq += S; } }
  }
  // bitwise: every pose and status of the last episode of each side
  long diff = 0;
  for (size_t i = 0; i < pose_b.size(); ++i) { uint32_t a, b; memcpy(&a, &pose_b[i], 4); memcpy(&b, &pose_s[i], 4); diff += a != b; }
  for (size_t i = 0; i < st_b.size(); ++i) diff += st_b[i] != st_s[i];
  long ok = 0; for (int32_t s : st_b) ok += s == 0;
  // the local maps, tracker by tracker
  std::vector<float> a((size_t) map_cap * 4), bb((size_t) map_cap * 4);
  long map_diff = 0;
  for (int j = 0; j < N; ++j) {
    int64_t na = 0, nb2 = 0;
    CK(lsm2d_cloudset_download(maps, j, a.data(), map_cap, &na)); CK(lsm2d_cloudset_download(smap[j], 0, bb.data(), map_cap, &nb2));
    map_diff += na != nb2 || memcmp(a.data(), bb.data(), sizeof(float) * 4 * (size_t) na) != 0;
  }
  const double ms_b = n_batch ? 1e3 * t_batch / n_batch : 0, ms_s = n_seq ? 1e3 * t_seq / n_seq : 0;
  printf("{\"n_trackers\": %d, \"steps_per_episode\": %d, \"timed_episodes\": %d, \"ms_per_batched_step\": %.5f, \"ms_per_sequential_step\": %.5f, "
         "\"tracker_steps_per_s_batched\": %.1f, \"tracker_steps_per_s_sequential\": %.1f, \"speedup\": %.3f, \"bitwise_equal\": %s, \"differing_words\": %ld, "
         "\"differing_maps\": %ld, \"status_ok\": %ld}\n",
         N, S, episodes - 1, ms_b, ms_s, ms_b > 0 ? 1e3 * N / ms_b : 0.0, ms_s > 0 ? 1e3 * N / ms_s : 0.0, ms_b > 0 ? ms_s / ms_b : 0.0,
         diff == 0 && map_diff == 0 ? "true" : "false", diff, map_diff, ok);
  for (int j = 0; j < N; ++j) { lsm2d_cloudset_destroy(smap[j]); lsm2d_cloudset_destroy(sclip[j]); lsm2d_cloudset_destroy(sm0[j]); lsm2d_cloudset_destroy(sm1[j]); }
  lsm2d_cloudset_destroy(maps); lsm2d_cloudset_destroy(clipped); lsm2d_cloudset_destroy(front); lsm2d_cloudset_destroy(rear);
  lsm2d_destroy(ctx);
  return diff == 0 && map_diff == 0 ? 0 : 3;
}
