// lsm2d_occupancy_update_scans into a LOG-ODDS grid set against (a) the definition on one host core and (b) the same call into a COUNTS set -- what the
// once-per-scan rule costs --, through the bare C ABI, alternating call by call:
//   occupancy_logodds_bench ranges.bin poses.bin grid.bin|- n_grids n_beams amin_bits amax_bits rmin_bits rmax_bits trace_bits clear ox_bits oy_bits res_bits
//                           width height steps warmup l_hit l_miss l_min l_max
// log-odds   ONE lsm2d_occupancy_update_scans over the ranges in pageable host memory, into a log-odds set.
// counts     the same call, the same ranges, into a counts set of the same geometry, in the same process.
// host       the definition's loops on one host core (-O2), the grid kept on the host: the rays of each scan by tests/cpp/occupancy_scan_ref.cpp, the votes by
//            tests/cpp/occupancy_logodds_ref.cpp (both linked in).
// All accumulate from zero, call after call.  Wall clock round calls that end in their wait, kernel timing off; medians over `steps` after `warmup`.  The
// log-odds set's cells are compared with the host route's byte for byte after the first call of each AND after the last.  One more call of each device route
// with kernel timing on gives lsm2d_last_kernel_ms and the tile workgroups' median and longest lifetime under both kinds of set.  Prints one JSON line.
#include <lsm2d_logodds.h>

#include "driver_common.h"

extern "C" void occsref_rays(const lsm2d_occupancy_scan_params* P, const float* ranges, const float* pose, float ox, float oy, float resolution, int32_t* rays, int32_t* kind);
extern "C" void occlref_update(const lsm2d_logodds_params* P, const int32_t* rays, const int32_t* kind, const int32_t* first, int n_scans, const int32_t* grid, int n_grids,
                               int width, int height, int32_t* value, uint32_t* observed);

static long long total(const std::vector<int32_t>& v) { long long s = 0; for (int32_t x : v) s += x; return s; }

int main(int argc, char** argv) {
  if (argc < 23) { fprintf(stderr, "usage: %s ranges.bin poses.bin grid.bin|- n_grids n_beams amin amax rmin rmax trace (bits) clear ox oy res (bits) width height steps warmup l_hit l_miss l_min l_max\n", argv[0]); return 2; }
  const std::vector<float> ranges = read_all<float>(argv[1]);
  const std::vector<float> poses = read_all<float>(argv[2]);
  const std::vector<int32_t> grid = read_all_or_empty<int32_t>(argv[3]);
  const int32_t G = atoi(argv[4]);
  const lsm2d_occupancy_scan_params prm{atoi(argv[5]), from_bits_arg(argv[6]), from_bits_arg(argv[7]), from_bits_arg(argv[8]), from_bits_arg(argv[9]), from_bits_arg(argv[10]), atoi(argv[11])};
  const lsm2d_grid_geometry geo{from_bits_arg(argv[12]), from_bits_arg(argv[13]), from_bits_arg(argv[14]), atoi(argv[15]), atoi(argv[16])};
  const int steps = atoi(argv[17]), warmup = atoi(argv[18]);
  const lsm2d_logodds_params lp{atoi(argv[19]), atoi(argv[20]), atoi(argv[21]), atoi(argv[22])};
  const int32_t K = (int32_t) (ranges.size() / (size_t) prm.n_beams), nb = prm.n_beams;
  const size_t cells = (size_t) geo.width * (size_t) geo.height;
  lsm2d_context* ctx = nullptr; must(lsm2d_create(0, nullptr, &ctx), "lsm2d_create", ctx);
  lsm2d_gridset* lo = nullptr; must(lsm2d_gridset_create_logodds(ctx, &geo, G, &lp, &lo), "lsm2d_gridset_create_logodds", ctx);
  lsm2d_gridset* cs = nullptr; must(lsm2d_gridset_create(ctx, &geo, G, &cs), "lsm2d_gridset_create", ctx);
  std::vector<int32_t> h_value(cells * (size_t) G, 0), d_value(cells);
  std::vector<uint32_t> h_observed(cells * (size_t) G, 0u), d_observed(cells);
  std::vector<int32_t> hit((size_t) G), clear((size_t) G), dropped((size_t) G), c_hit((size_t) G), c_clear((size_t) G), c_dropped((size_t) G);
  std::vector<int32_t> rays(4 * (size_t) K * nb), kind((size_t) K * nb), first((size_t) K + 1);
  for (int32_t k = 0; k <= K; ++k) first[(size_t) k] = k * nb;
  const int32_t* gp = grid.empty() ? nullptr : grid.data();
  auto logodds_call = [&]() {
    must(lsm2d_occupancy_update_scans(ctx, lo, &prm, ranges.data(), K, poses.data(), gp, hit.data(), clear.data(), dropped.data()), "lsm2d_occupancy_update_scans (log-odds)", ctx);
  };
  auto counts_call = [&]() {
    must(lsm2d_occupancy_update_scans(ctx, cs, &prm, ranges.data(), K, poses.data(), gp, c_hit.data(), c_clear.data(), c_dropped.data()), "lsm2d_occupancy_update_scans (counts)", ctx);
  };
  auto host_route = [&]() {
    for (int32_t k = 0; k < K; ++k)
      occsref_rays(&prm, ranges.data() + (size_t) k * nb, poses.data() + 3 * (size_t) k, geo.origin_x, geo.origin_y, geo.resolution, rays.data() + 4 * (size_t) k * nb, kind.data() + (size_t) k * nb);
    occlref_update(&lp, rays.data(), kind.data(), first.data(), K, gp, G, geo.width, geo.height, h_value.data(), h_observed.data());
  };
  auto grids_equal = [&]() {
    bool eq = hit == c_hit && clear == c_clear && dropped == c_dropped;      // the counts count rays, whatever the kind of set
    for (int32_t g = 0; g < G && eq; ++g) {
      must(lsm2d_gridset_download_logodds(lo, g, d_value.data(), d_observed.data()), "lsm2d_gridset_download_logodds", ctx);
      eq = !memcmp(d_value.data(), h_value.data() + cells * (size_t) g, sizeof(int32_t) * cells) && !memcmp(d_observed.data(), h_observed.data() + cells * (size_t) g, sizeof(uint32_t) * cells);
    }
    return eq;
  };
  // ---- parity first
  logodds_call(); counts_call(); host_route();
  int equal = grids_equal();
  // ---- times, the routes alternating call by call
  std::vector<double> tl, tc, th;
  for (int i = 0; i < warmup + steps; ++i) {
    double a0 = now_ms(); logodds_call(); double a1 = now_ms();
    double b0 = now_ms(); counts_call(); double b1 = now_ms();
    double c0 = now_ms(); host_route(); double c1 = now_ms();
    if (i >= warmup) { tl.push_back(a1 - a0); tc.push_back(b1 - b0); th.push_back(c1 - c0); }
  }
  equal = equal && grids_equal();
  double l[3], c[3], h[3]; summary(tl, l, true); summary(tc, c, true); summary(th, h, true);      // the upper middle element, as ever
  float k_ms[2] = {0.0f, 0.0f}; int64_t wg_median[2] = {0, 0}, wg_max[2] = {0, 0};
  must(lsm2d_set_option(ctx, "kernel_timing", 1), "lsm2d_set_option", ctx);
  for (int which = 0; which < 2; ++which) {
    if (which == 0) logodds_call(); else counts_call();
    must(lsm2d_last_kernel_ms(ctx, &k_ms[which]), "lsm2d_last_kernel_ms", ctx);
    must(lsm2d_get_option(ctx, "last_occupancy_wg_median_ns", &wg_median[which]), "lsm2d_get_option", ctx);
    must(lsm2d_get_option(ctx, "last_occupancy_wg_max_ns", &wg_max[which]), "lsm2d_get_option", ctx);
  }
  printf("{\"scans\": %d, \"beams\": %lld, \"grids\": %d, \"width\": %d, \"height\": %d, \"hit_rays\": %lld, \"clear_rays\": %lld, \"dropped\": %lld, \"outputs_equal\": %d, "
         "\"logodds_call_ms\": [%.4f, %.4f, %.4f], \"counts_call_ms\": [%.4f, %.4f, %.4f], \"host_route_ms\": [%.4f, %.4f, %.4f], "
         "\"logodds_kernel_ms\": %.4f, \"logodds_tile_workgroup_median_us\": %.2f, \"logodds_tile_workgroup_longest_us\": %.2f, "
         "\"counts_kernel_ms\": %.4f, \"counts_tile_workgroup_median_us\": %.2f, \"counts_tile_workgroup_longest_us\": %.2f}\n",
         K, (long long) K * nb, G, geo.width, geo.height, total(hit), total(clear), total(dropped), equal, l[0], l[1], l[2], c[0], c[1], c[2], h[0], h[1], h[2],
         k_ms[0], wg_median[0] / 1000.0, wg_max[0] / 1000.0, k_ms[1], wg_median[1] / 1000.0, wg_max[1] / 1000.0);
  lsm2d_gridset_destroy(cs); lsm2d_gridset_destroy(lo);
  lsm2d_destroy(ctx);
  return equal ? 0 : 3;
}
