// Drives the log-odds grid set of the C++ host mirror (host/lsm2d_occupancy.hpp):
//   occupancy_logodds_driver ranges.bin poses.bin|- grid.bin|- n_grids n_beams amin_bits amax_bits rmin_bits rmax_bits trace_bits clear ox_bits oy_bits res_bits
//                            width height l_hit l_miss l_min l_max l_hit2 l_miss2 l_min2 l_max2 decay unit_bits min_scans out.bin
// The scans are ray-traced into a log-odds set of n_grids grids with the first parameters, once more after setLogOdds with the second ones, then the set
// decays by `decay`, grid 0 is downloaded and uploaded again (a round trip) and out.bin receives, per grid, value [h][w] int32, observed [h][w] uint32 and
// the render [h][w] int8; the three counts of the second call are printed as JSON.  The Python test compares the bytes with the Python mirror's.
#include <lsm2d_occupancy.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

int main(int argc, char** argv) {
  if (argc < 29) { fprintf(stderr, "usage: %s ranges.bin poses.bin|- grid.bin|- n_grids n_beams (sensor, 6) (geometry, 5) (params, 4) (params, 4) decay unit_bits min_scans out.bin\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    const std::vector<float> ranges = read_all<float>(argv[1]);
    const std::vector<Vector3f> poses = read_all_or_empty<Vector3f>(argv[2]);
    const std::vector<int32_t> grid = read_all_or_empty<int32_t>(argv[3]);
    const int32_t n_grids = atoi(argv[4]), n_beams = atoi(argv[5]);
    const OccupancyScanParams params(n_beams, from_bits_arg(argv[6]), from_bits_arg(argv[7]), from_bits_arg(argv[8]), from_bits_arg(argv[9]), from_bits_arg(argv[10]), atoi(argv[11]) != 0);
    const lsm2d_grid_geometry geo{from_bits_arg(argv[12]), from_bits_arg(argv[13]), from_bits_arg(argv[14]), atoi(argv[15]), atoi(argv[16])};
    const LogOddsParams first(atoi(argv[17]), atoi(argv[18]), atoi(argv[19]), atoi(argv[20])), second(atoi(argv[21]), atoi(argv[22]), atoi(argv[23]), atoi(argv[24]));
    const int32_t n_scans = (int32_t) (ranges.size() / (size_t) n_beams);
    GridSet grids(ctx, geo, n_grids, first);
    if (!grids.isLogOdds()) return 3;
    occupancyUpdateScans(ctx, grids, params, ranges.data(), n_scans, poses, grid);
    grids.setLogOdds(second);
    const OccupancyScanUpdate u = occupancyUpdateScans(ctx, grids, params, ranges.data(), n_scans, poses, grid);
    occupancyDecay(ctx, grids, atoi(argv[25]));
    { const GridSet::LogOdds c = grids.downloadLogOdds(0); grids.clear({0}); grids.uploadLogOdds(0, c.value, c.observed); }
    FILE* out = fopen(argv[28], "wb"); if (!out) { perror(argv[28]); return 2; }
    for (int32_t g = 0; g < n_grids; ++g) {
      const GridSet::LogOdds c = grids.downloadLogOdds(g);
      const std::vector<int8_t> r = occupancyRenderLogOdds(ctx, grids, g, from_bits_arg(argv[26]), atoi(argv[27]));
      fwrite(c.value.data(), sizeof(int32_t), c.value.size(), out); fwrite(c.observed.data(), sizeof(uint32_t), c.observed.size(), out); fwrite(r.data(), 1, r.size(), out);
    }
    fclose(out);
    printf("{");
    print_int_list("hit_rays", u.hit_rays, ", "); print_int_list("clear_rays", u.clear_rays, ", "); print_int_list("dropped", u.dropped, "}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
