// Drives the occupancy calls of the C++ host mirror (host/lsm2d_occupancy.hpp):
//   occupancy_driver points.bin offsets.bin poses.bin|- grid.bin|- n_grids ox_bits oy_bits res_bits width height min_visits out.bin
// The inputs (float [n][4], int32 offsets [n_inputs + 1], float poses [n_inputs][3], int32 grid [n_inputs]) are ray-traced TWICE into a set of n_grids grids
// (the counters accumulate); out.bin receives, per grid, hits [h][w] uint32, misses [h][w] uint32 and the render [h][w] int8; rays and dropped counts of
// the second call are printed as JSON.  The Python test compares the bytes with api.occupancy_update / occupancy_render on the same inputs.
#include <lsm2d_occupancy.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

int main(int argc, char** argv) {
  if (argc < 13) { fprintf(stderr, "usage: %s points.bin offsets.bin poses.bin|- grid.bin|- n_grids ox_bits oy_bits res_bits width height min_visits out.bin\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    const std::vector<PointNormal2f> pts = read_all<PointNormal2f>(argv[1]);
    const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
    std::vector<PointNormal2fVectorCloud> clouds;
    for (size_t k = 0; k + 1 < offs.size(); ++k) clouds.emplace_back(pts.begin() + offs[k], pts.begin() + offs[k + 1]);
    const std::vector<Vector3f> poses = read_all_or_empty<Vector3f>(argv[3]);
    const std::vector<int32_t> grid = read_all_or_empty<int32_t>(argv[4]);
    const int32_t n_grids = atoi(argv[5]);
    const lsm2d_grid_geometry geo{from_bits_arg(argv[6]), from_bits_arg(argv[7]), from_bits_arg(argv[8]), atoi(argv[9]), atoi(argv[10])};
    CloudSet src(ctx, clouds);
    GridSet grids(ctx, geo, n_grids);
    occupancyUpdate(ctx, grids, src.get(), {}, poses, grid);
    const OccupancyUpdate u = occupancyUpdate(ctx, grids, src.get(), {}, poses, grid);
    FILE* out = fopen(argv[12], "wb"); if (!out) { perror(argv[12]); return 2; }
    for (int32_t g = 0; g < n_grids; ++g) {
      const GridSet::Counters c = grids.download(g);
      const std::vector<int8_t> r = occupancyRender(ctx, grids, g, atoi(argv[11]));
      fwrite(c.hits.data(), sizeof(uint32_t), c.hits.size(), out); fwrite(c.misses.data(), sizeof(uint32_t), c.misses.size(), out); fwrite(r.data(), 1, r.size(), out);
    }
    fclose(out);
    printf("{");
    print_int_list("rays", u.rays, ", "); print_int_list("dropped", u.dropped, "}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
