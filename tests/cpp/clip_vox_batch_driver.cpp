// lsm2d_host::TrackerBatch (srrg2_laser_slam_2d_amd/host/lsm2d.hpp) with a clipper that voxelises: Params::clip_voxelize_resolution > 0 makes
// step() clip through lsm2d_clip_scene_voxelized_batch.  N trackers start their local maps from step 0's scans and run steps 1 .. steps.
//   clip_vox_batch_driver dir n_scenarios steps n_beams angle_min angle_max n_trackers resolution
// dir holds ranges.bin (float32 [n_scenarios][steps + 1][2][n_beams]), odo.bin (float64 [n_scenarios][steps][3]), start.bin (float64 [n_scenarios][3])
// (tests/bench/track_batch_bench.py write_inputs); tracker j runs scenario j % n_scenarios.  Prints one JSON object: per step and tracker the pose's
// three words, the status, the clipped cloud's size and the local map's size, all as hex strings.
#include <cmath>
#include <lsm2d.hpp>

#include "driver_common.h"

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s dir n_scenarios steps n_beams angle_min angle_max n_trackers resolution\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const int M = atoi(argv[2]), S = atoi(argv[3]), nb = atoi(argv[4]), N = atoi(argv[7]);
  const std::vector<float> ranges = read_all<float>(dir + "/ranges.bin");
  const std::vector<double> odo = read_all<double>(dir + "/odo.bin"), start = read_all<double>(dir + "/start.bin");
  if ((long) ranges.size() != (long) M * (S + 1) * 2 * nb || (long) odo.size() != (long) M * S * 3 || (long) start.size() != (long) M * 3) { fprintf(stderr, "bad inputs\n"); return 2; }
  auto rng = [&](int scen, int k, int sensor) { return ranges.data() + (((size_t) scen * (S + 1) + k) * 2 + sensor) * nb; };
  try {
    lsm2d_host::Context ctx(0);
    lsm2d_host::TrackerBatch::Params p;
    p.projector = lsm2d_projector{721, -(float) M_PI, (float) M_PI, 0.3f, 20.0f, 0.0f};
    memset(&p.preprocessor, 0, sizeof p.preprocessor);
    p.preprocessor.n_beams = nb; p.preprocessor.angle_min = (float) atof(argv[5]); p.preprocessor.angle_max = (float) atof(argv[6]);
    p.preprocessor.range_min = 0.3f; p.preprocessor.range_max = 20.0f; p.preprocessor.normal_point_distance = 0.3f; p.preprocessor.normal_min_points = 5;
    p.preprocessor.voxelize_resolution = 0.02f;
    const float S0[3] = {0.2f, 0.1f, 0.1f}, S1[3] = {-0.3f, 0.0f, (float) M_PI};
    for (int i = 0; i < 2; ++i) {
      lsm2d_slice_params& sl = p.slices[(size_t) i]; memset(&sl, 0, sizeof sl);
      sl.finder = LSM2D_FINDER_PROJECTIVE; sl.projector = p.projector; sl.point_distance = 0.5f; sl.normal_cos = i ? 0.8f : 0.9f;
      sl.robustifier = i ? LSM2D_ROBUST_NONE : LSM2D_ROBUST_CAUCHY; sl.chi_threshold = i ? 0.0f : 0.01f; sl.min_num_correspondences = 5;
      memcpy(sl.sensor_in_robot, i ? S1 : S0, sizeof S0);
    }
    p.aligner = lsm2d_aligner_params{10, 10, 0.0f, 0.0f, 0, 0};
    p.merge_threshold = 0.2f;
    p.clip_voxelize_resolution = (float) atof(argv[8]);
    lsm2d_host::TrackerBatch tb(ctx, N, p);
    std::vector<float> front((size_t) N * nb), rear((size_t) N * nb);
    std::vector<double> od((size_t) N * 3), st((size_t) N * 3);
    std::vector<int32_t> idx((size_t) N), clip_n((size_t) N), map_n((size_t) N);
    auto gather = [&](int k) {
      for (int j = 0; j < N; ++j) { memcpy(&front[(size_t) j * nb], rng(j % M, k, 0), sizeof(float) * nb); memcpy(&rear[(size_t) j * nb], rng(j % M, k, 1), sizeof(float) * nb); }
    };
    for (int j = 0; j < N; ++j) { idx[(size_t) j] = j; memcpy(&st[(size_t) j * 3], &start[(size_t) (j % M) * 3], sizeof(double) * 3); }
    gather(0);
    tb.reset(N, idx.data(), front.data(), rear.data(), st.data());
    printf("{\"n_trackers\": %d, \"steps\": [", N);
    for (int k = 1; k <= S; ++k) {
      gather(k);
      for (int j = 0; j < N; ++j) memcpy(&od[(size_t) j * 3], &odo[((size_t) (j % M) * S + (k - 1)) * 3], sizeof(double) * 3);
      tb.step(front.data(), rear.data(), od.data());
      if (lsm2d_cloudset_cloud_sizes(tb.clippedScenes(), clip_n.data(), N) != N || lsm2d_cloudset_cloud_sizes(tb.localMaps(), map_n.data(), N) != N) { fprintf(stderr, "sizes\n"); return 1; }
      printf("%s[", k > 1 ? ", " : "");
      for (int j = 0; j < N; ++j) {
        uint32_t w[3]; memcpy(w, &tb.movingInFixed()[(size_t) j * 3], sizeof w);
        printf("%s{\"pose\": [\"%08x\", \"%08x\", \"%08x\"], \"status\": \"%x\", \"clip_points\": \"%x\", \"map_points\": \"%x\"}", j ? ", " : "", w[0], w[1], w[2],
               (unsigned) tb.status()[(size_t) j], (unsigned) clip_n[(size_t) j], (unsigned) map_n[(size_t) j]);
      }
      printf("]");
    }
    printf("]}\n");
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
