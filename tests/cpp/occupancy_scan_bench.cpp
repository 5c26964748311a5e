// lsm2d_occupancy_update_scans against the routes a caller had before it, through the bare C ABI, alternating call by call:
//   occupancy_scan_bench ranges.bin poses.bin grid.bin|- n_grids n_beams amin_bits amax_bits rmin_bits rmax_bits trace_bits clear ox_bits oy_bits res_bits
//                        width height steps warmup two_call
// new call   ONE lsm2d_occupancy_update_scans over the ranges in pageable host memory.
// host       the definition's loops on one host core (tests/cpp/occupancy_scan_ref.cpp, linked in, -O2) and the grid kept on the host.
// two calls  (two_call = 1, meaningful where no beam is without a return) lsm2d_preprocess_scans_refill into a set made once, then lsm2d_occupancy_update,
//            into a grid set of its own: the device route of 0.7.12.  The preprocessor is the default one but for normal_min_points 1 and no voxelisation,
//            so it still drops the beams whose window has no direction: its ray count is reported, its counters are not compared.
// All accumulate from zero, call after call.  Wall clock round calls that end in their wait, kernel timing off; medians over `steps` after `warmup`.  The
// new call's counters and counts are compared with the host route's byte for byte after the first call of each AND after the last.  One more new call with
// kernel timing on gives lsm2d_last_kernel_ms and the tile workgroups' median and longest lifetime.  Prints one JSON line.
#include <cmath>

#include "driver_common.h"

extern "C" void occsref_update(const lsm2d_occupancy_scan_params* P, const float* ranges, int n_scans, const float* pose, const int32_t* grid, int n_grids, float ox,
                               float oy, float resolution, int width, int height, uint32_t* hits, uint32_t* misses, int32_t* hit_rays, int32_t* clear_rays,
                               int32_t* dropped);

static long long total(const std::vector<int32_t>& v) { long long s = 0; for (int32_t x : v) s += x; return s; }

int main(int argc, char** argv) {
  if (argc < 20) { fprintf(stderr, "usage: %s ranges.bin poses.bin grid.bin|- n_grids n_beams amin amax rmin rmax trace (bits) clear ox oy res (bits) width height steps warmup two_call\n", argv[0]); return 2; }
  const std::vector<float> ranges = read_all<float>(argv[1]);
  const std::vector<float> poses = read_all<float>(argv[2]);
  const std::vector<int32_t> grid = read_all_or_empty<int32_t>(argv[3]);
  const int32_t G = atoi(argv[4]);
  const lsm2d_occupancy_scan_params prm{atoi(argv[5]), from_bits_arg(argv[6]), from_bits_arg(argv[7]), from_bits_arg(argv[8]), from_bits_arg(argv[9]), from_bits_arg(argv[10]), atoi(argv[11])};
  const lsm2d_grid_geometry geo{from_bits_arg(argv[12]), from_bits_arg(argv[13]), from_bits_arg(argv[14]), atoi(argv[15]), atoi(argv[16])};
  const int steps = atoi(argv[17]), warmup = atoi(argv[18]), two_call = atoi(argv[19]);
  const int32_t K = (int32_t) (ranges.size() / (size_t) prm.n_beams);
  const size_t cells = (size_t) geo.width * (size_t) geo.height;
  lsm2d_context* ctx = nullptr; must(lsm2d_create(0, nullptr, &ctx), "lsm2d_create", ctx);
  lsm2d_gridset* gs = nullptr; must(lsm2d_gridset_create(ctx, &geo, G, &gs), "lsm2d_gridset_create", ctx);
  std::vector<uint32_t> h_hits(cells * (size_t) G, 0u), h_misses(cells * (size_t) G, 0u), d_hits(cells), d_misses(cells);
  std::vector<int32_t> hit((size_t) G), clear((size_t) G), dropped((size_t) G), h_hit((size_t) G), h_clear((size_t) G), h_dropped((size_t) G), rays2((size_t) G), dropped2((size_t) G);
  const int32_t* gp = grid.empty() ? nullptr : grid.data();
  auto new_call = [&]() {
    must(lsm2d_occupancy_update_scans(ctx, gs, &prm, ranges.data(), K, poses.data(), gp, hit.data(), clear.data(), dropped.data()), "lsm2d_occupancy_update_scans", ctx);
  };
  auto host_route = [&]() {
    occsref_update(&prm, ranges.data(), K, poses.data(), gp, G, geo.origin_x, geo.origin_y, geo.resolution, geo.width, geo.height, h_hits.data(), h_misses.data(),
                   h_hit.data(), h_clear.data(), h_dropped.data());
  };
  // the two-call route of 0.7.12: a cloud set kept alive, refilled, then traced
  lsm2d_preprocessor pp{prm.n_beams, prm.angle_min, prm.angle_max, prm.range_min, prm.range_max, 0.3f, 1, 0.0f};
  lsm2d_cloudset* set = nullptr; lsm2d_gridset* gs2 = nullptr;
  if (two_call) {
    must(lsm2d_preprocess_scans(ctx, &pp, ranges.data(), K, &set), "lsm2d_preprocess_scans", ctx);
    must(lsm2d_gridset_create(ctx, &geo, G, &gs2), "lsm2d_gridset_create", ctx);
  }
  auto two_calls = [&]() {
    must(lsm2d_preprocess_scans_refill(ctx, &pp, ranges.data(), K, set), "lsm2d_preprocess_scans_refill", ctx);
    must(lsm2d_occupancy_update(ctx, gs2, set, K, nullptr, poses.data(), gp, rays2.data(), dropped2.data()), "lsm2d_occupancy_update", ctx);
  };
  auto grids_equal = [&]() {
    bool eq = hit == h_hit && clear == h_clear && dropped == h_dropped;
    for (int32_t g = 0; g < G && eq; ++g) {
      must(lsm2d_gridset_download(gs, g, d_hits.data(), d_misses.data()), "lsm2d_gridset_download", ctx);
      eq = !memcmp(d_hits.data(), h_hits.data() + cells * (size_t) g, sizeof(uint32_t) * cells) && !memcmp(d_misses.data(), h_misses.data() + cells * (size_t) g, sizeof(uint32_t) * cells);
    }
    return eq;
  };
  // ---- parity first
  new_call(); host_route();
  int equal = grids_equal();
  if (two_call) two_calls();
  // ---- times, the routes alternating call by call
  std::vector<double> tn, th, t2;
  for (int i = 0; i < warmup + steps; ++i) {
    double a0 = now_ms(); new_call(); double a1 = now_ms();
    double b0 = now_ms(); host_route(); double b1 = now_ms();
    double c0 = now_ms(); if (two_call) two_calls(); double c1 = now_ms();
    if (i >= warmup) { tn.push_back(a1 - a0); th.push_back(b1 - b0); if (two_call) t2.push_back(c1 - c0); }
  }
  equal = equal && grids_equal();
  double n[3], h[3], w[3]; summary(tn, n, true); summary(th, h, true); summary(t2, w, true);      // the upper middle element, as ever
  float kernel_ms = 0.0f; int64_t wg_median = 0, wg_max = 0;
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "lsm2d_set_option", ctx);
  new_call();
  must(lsm2d_last_kernel_ms(ctx, &kernel_ms), "lsm2d_last_kernel_ms", ctx);
  must(lsm2d_get_option(ctx, "last_occupancy_wg_median_ns", &wg_median), "lsm2d_get_option", ctx);
  must(lsm2d_get_option(ctx, "last_occupancy_wg_max_ns", &wg_max), "lsm2d_get_option", ctx);
  float kernel2_ms = 0.0f; int64_t wg2_median = 0, wg2_max = 0;
  if (two_call) {      // (the bracket of lsm2d_occupancy_update alone: the refill's launch is outside it)
    two_calls();
    must(lsm2d_last_kernel_ms(ctx, &kernel2_ms), "lsm2d_last_kernel_ms", ctx);
    must(lsm2d_get_option(ctx, "last_occupancy_wg_median_ns", &wg2_median), "lsm2d_get_option", ctx);
    must(lsm2d_get_option(ctx, "last_occupancy_wg_max_ns", &wg2_max), "lsm2d_get_option", ctx);
  }
  printf("{\"scans\": %d, \"beams\": %lld, \"grids\": %d, \"width\": %d, \"height\": %d, \"hit_rays\": %lld, \"clear_rays\": %lld, \"dropped\": %lld, \"outputs_equal\": %d, "
         "\"new_call_ms\": [%.4f, %.4f, %.4f], \"host_route_ms\": [%.4f, %.4f, %.4f], \"two_call_ms\": [%.4f, %.4f, %.4f], \"two_call_rays\": %lld, "
         "\"new_call_kernel_ms\": %.4f, \"tile_workgroup_median_us\": %.2f, \"tile_workgroup_longest_us\": %.2f, "
         "\"two_call_update_kernel_ms\": %.4f, \"two_call_tile_workgroup_median_us\": %.2f, \"two_call_tile_workgroup_longest_us\": %.2f}\n",
         K, (long long) K * prm.n_beams, G, geo.width, geo.height, total(hit), total(clear), total(dropped), equal, n[0], n[1], n[2], h[0], h[1], h[2], w[0], w[1], w[2],
         two_call ? total(rays2) : 0ll, kernel_ms, wg_median / 1000.0, wg_max / 1000.0, kernel2_ms, wg2_median / 1000.0, wg2_max / 1000.0);
  if (two_call) { lsm2d_gridset_destroy(gs2); lsm2d_cloudset_destroy(set); }
  lsm2d_gridset_destroy(gs);
  lsm2d_destroy(ctx);
  return equal ? 0 : 3;
}
