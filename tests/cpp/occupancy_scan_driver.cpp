// Drives occupancyUpdateScans of the C++ host mirror (host/lsm2d_occupancy.hpp):
//   occupancy_scan_driver ranges.bin poses.bin|- grid.bin|- n_grids n_beams amin_bits amax_bits rmin_bits rmax_bits trace_bits clear ox_bits oy_bits res_bits
//                         width height min_visits out.bin
// The scans (float ranges [n_scans][n_beams], float poses [n_scans][3], int32 grid [n_scans]) are ray-traced TWICE into a set of n_grids grids (the counters
// accumulate); out.bin receives, per grid, hits [h][w] uint32, misses [h][w] uint32 and the render [h][w] int8; the three counts of the second call are
// printed as JSON.  The Python test compares the bytes with api.occupancy_update_scans / occupancy_render on the same inputs.
#include <lsm2d_occupancy.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

int main(int argc, char** argv) {
  if (argc < 19) { fprintf(stderr, "usage: %s ranges.bin poses.bin|- grid.bin|- n_grids n_beams amin amax rmin rmax trace (bits) clear ox oy res (bits) width height min_visits out.bin\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    const std::vector<float> ranges = read_all<float>(argv[1]);
    const std::vector<Vector3f> poses = read_all_or_empty<Vector3f>(argv[2]);
    const std::vector<int32_t> grid = read_all_or_empty<int32_t>(argv[3]);
    const int32_t n_grids = atoi(argv[4]), n_beams = atoi(argv[5]);
    const OccupancyScanParams params(n_beams, from_bits_arg(argv[6]), from_bits_arg(argv[7]), from_bits_arg(argv[8]), from_bits_arg(argv[9]), from_bits_arg(argv[10]), atoi(argv[11]) != 0);
    const lsm2d_grid_geometry geo{from_bits_arg(argv[12]), from_bits_arg(argv[13]), from_bits_arg(argv[14]), atoi(argv[15]), atoi(argv[16])};
    const int32_t n_scans = (int32_t) (ranges.size() / (size_t) n_beams);
    GridSet grids(ctx, geo, n_grids);
    occupancyUpdateScans(ctx, grids, params, ranges.data(), n_scans, poses, grid);
    const OccupancyScanUpdate u = occupancyUpdateScans(ctx, grids, params, ranges.data(), n_scans, poses, grid);
    FILE* out = fopen(argv[18], "wb"); if (!out) { perror(argv[18]); return 2; }
    for (int32_t g = 0; g < n_grids; ++g) {
      const GridSet::Counters c = grids.download(g);
      const std::vector<int8_t> r = occupancyRender(ctx, grids, g, atoi(argv[17]));
      fwrite(c.hits.data(), sizeof(uint32_t), c.hits.size(), out); fwrite(c.misses.data(), sizeof(uint32_t), c.misses.size(), out); fwrite(r.data(), 1, r.size(), out);
    }
    fclose(out);
    printf("{");
    print_int_list("hit_rays", u.hit_rays, ", "); print_int_list("clear_rays", u.clear_rays, ", "); print_int_list("dropped", u.dropped, "}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
