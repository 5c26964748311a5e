// lsm2d_occupancy_update and lsm2d_occupancy_render against the routes a caller had before them, through the bare C ABI, alternating call by call:
//   occupancy_bench points.bin offsets.bin poses.bin grid.bin|- n_grids ox_bits oy_bits res_bits width height steps warmup
// update   device route: ONE lsm2d_occupancy_update.  Host route: lsm2d_cloudset_download per cloud, the definition's loops on one host core
//          (tests/cpp/occupancy_ref.cpp, linked in, -O2) and the grid kept on the host.  Both accumulate from zero, call after call.
// render   device route: lsm2d_occupancy_render of grid 0 (one byte per cell comes down).  Host route: lsm2d_gridset_download of its counters (eight bytes per
//          cell) and the same rule on the host.
// Wall clock round calls that end in their wait, kernel timing off; medians over `steps` after `warmup`.  The two routes' outputs are compared byte for byte
// after the first call of each AND after the last.  One more update with kernel timing on gives lsm2d_last_kernel_ms and the tile workgroups' median and
// longest lifetime.  Prints one JSON line.
#include <cmath>

#include "driver_common.h"

extern "C" void occref_update(const float* points, const int32_t* offsets, int n_inputs, const float* pose, const int32_t* grid, int n_grids, float ox, float oy,
                              float resolution, int width, int height, uint32_t* hits, uint32_t* misses, int32_t* rays, int32_t* dropped);

int main(int argc, char** argv) {
  if (argc < 13) { fprintf(stderr, "usage: %s points.bin offsets.bin poses.bin grid.bin|- n_grids ox_bits oy_bits res_bits width height steps warmup\n", argv[0]); return 2; }
  const std::vector<float> pts = read_all<float>(argv[1]);
  const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
  const std::vector<float> poses = read_all<float>(argv[3]);
  const std::vector<int32_t> grid = read_all_or_empty<int32_t>(argv[4]);
  const int32_t G = atoi(argv[5]);
  const lsm2d_grid_geometry geo{from_bits_arg(argv[6]), from_bits_arg(argv[7]), from_bits_arg(argv[8]), atoi(argv[9]), atoi(argv[10])};
  const int steps = atoi(argv[11]), warmup = atoi(argv[12]);
  const int32_t K = (int32_t) offs.size() - 1; const int64_t N = offs[(size_t) K];
  const size_t cells = (size_t) geo.width * (size_t) geo.height;
  lsm2d_context* ctx = nullptr; must(lsm2d_create(0, nullptr, &ctx), "lsm2d_create", ctx);
  lsm2d_cloudset* src = nullptr; must(lsm2d_cloudset_create(ctx, pts.data(), K > 1 ? offs.data() : nullptr, K, N, &src), "lsm2d_cloudset_create", ctx);
  lsm2d_gridset* gs = nullptr; must(lsm2d_gridset_create(ctx, &geo, G, &gs), "lsm2d_gridset_create", ctx);
  std::vector<uint32_t> h_hits(cells * (size_t) G, 0u), h_misses(cells * (size_t) G, 0u), d_hits(cells), d_misses(cells);
  std::vector<int32_t> rays((size_t) G), dropped((size_t) G), h_rays((size_t) G), h_dropped((size_t) G), h_offs((size_t) K + 1, 0);
  std::vector<float> down((size_t) 4 * (size_t) N);
  const int32_t* gp = grid.empty() ? nullptr : grid.data();
  auto device_route = [&]() { must(lsm2d_occupancy_update(ctx, gs, src, K, nullptr, poses.data(), gp, rays.data(), dropped.data()), "lsm2d_occupancy_update", ctx); };
  auto host_route = [&]() {
    for (int32_t k = 0; k < K; ++k) {
      int64_t n = 0;
      must(lsm2d_cloudset_download(src, k, down.data() + 4 * (size_t) h_offs[(size_t) k], N - h_offs[(size_t) k], &n), "lsm2d_cloudset_download", ctx);
      h_offs[(size_t) k + 1] = h_offs[(size_t) k] + (int32_t) n;
    }
    occref_update(down.data(), h_offs.data(), K, poses.data(), gp, G, geo.origin_x, geo.origin_y, geo.resolution, geo.width, geo.height, h_hits.data(), h_misses.data(),
                  h_rays.data(), h_dropped.data());
  };
  auto grids_equal = [&]() {
    bool eq = rays == h_rays && dropped == h_dropped;
    for (int32_t g = 0; g < G && eq; ++g) {
      must(lsm2d_gridset_download(gs, g, d_hits.data(), d_misses.data()), "lsm2d_gridset_download", ctx);
      eq = !memcmp(d_hits.data(), h_hits.data() + cells * (size_t) g, sizeof(uint32_t) * cells) && !memcmp(d_misses.data(), h_misses.data() + cells * (size_t) g, sizeof(uint32_t) * cells);
    }
    return eq;
  };
  // ---- parity first
  device_route(); host_route();
  int equal = grids_equal();
  long long n_rays = 0, n_dropped = 0; for (int32_t g = 0; g < G; ++g) { n_rays += rays[(size_t) g]; n_dropped += dropped[(size_t) g]; }
  // ---- times, the routes alternating call by call
  std::vector<double> td, th;
  for (int i = 0; i < warmup + steps; ++i) {
    double t0 = now_ms(); device_route(); double t1 = now_ms();
    double t2 = now_ms(); host_route(); double t3 = now_ms();
    if (i >= warmup) { td.push_back(t1 - t0); th.push_back(t3 - t2); }
  }
  equal = equal && grids_equal();
  // ---- the render of grid 0 against a download of its counters and the rule on the host
  const lsm2d_occupancy_render_params rp{2};
  std::vector<int8_t> r_dev(cells), r_host(cells);
  auto render_device = [&]() { must(lsm2d_occupancy_render(ctx, gs, 0, &rp, r_dev.data()), "lsm2d_occupancy_render", ctx); };
  auto render_host = [&]() {
    must(lsm2d_gridset_download(gs, 0, d_hits.data(), d_misses.data()), "lsm2d_gridset_download", ctx);
    for (size_t c = 0; c < cells; ++c) {
      const unsigned long long v = (unsigned long long) d_hits[c] + d_misses[c];
      r_host[c] = v < 2ull ? (int8_t) -1 : (int8_t) rintf(100.0f * ((float) d_hits[c] / (float) v));
    }
  };
  std::vector<double> rd, rh;
  for (int i = 0; i < warmup + steps; ++i) {
    double t0 = now_ms(); render_device(); double t1 = now_ms();
    double t2 = now_ms(); render_host(); double t3 = now_ms();
    if (i >= warmup) { rd.push_back(t1 - t0); rh.push_back(t3 - t2); }
  }
  const int render_equal = r_dev == r_host;
  double d[3], h[3], r1[3], r2[3]; summary(td, d, true); summary(th, h, true); summary(rd, r1, true); summary(rh, r2, true);      // the upper middle element, as ever
  float kernel_ms = 0.0f; int64_t wg_median = 0, wg_max = 0;
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "lsm2d_set_option", ctx);
  device_route();
  must(lsm2d_last_kernel_ms(ctx, &kernel_ms), "lsm2d_last_kernel_ms", ctx);
  must(lsm2d_get_option(ctx, "last_occupancy_wg_median_ns", &wg_median), "lsm2d_get_option", ctx);
  must(lsm2d_get_option(ctx, "last_occupancy_wg_max_ns", &wg_max), "lsm2d_get_option", ctx);
  printf("{\"inputs\": %d, \"points\": %lld, \"grids\": %d, \"width\": %d, \"height\": %d, \"rays\": %lld, \"dropped\": %lld, \"outputs_equal\": %d, \"render_equal\": %d, "
         "\"device_ms\": [%.4f, %.4f, %.4f], \"host_route_ms\": [%.4f, %.4f, %.4f], \"render_ms\": [%.4f, %.4f, %.4f], \"render_download_route_ms\": [%.4f, %.4f, %.4f], "
         "\"device_kernel_ms\": %.4f, \"tile_workgroup_median_us\": %.2f, \"tile_workgroup_longest_us\": %.2f}\n",
         K, (long long) N, G, geo.width, geo.height, n_rays, n_dropped, equal, render_equal, d[0], d[1], d[2], h[0], h[1], h[2], r1[0], r1[1], r1[2], r2[0], r2[1], r2[2],
         kernel_ms, wg_median / 1000.0, wg_max / 1000.0);
  lsm2d_gridset_destroy(gs); lsm2d_cloudset_destroy(src);
  lsm2d_destroy(ctx);
  return equal && render_equal ? 0 : 3;
}
