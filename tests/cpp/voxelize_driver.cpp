// Drives voxelize of the C++ host mirror (host/lsm2d_voxelize.hpp):
//   voxelize_driver points.bin offsets.bin poses.bin|- groups.bin|- n_groups capacity res_bits nres_bits res2_bits
// The inputs (float [n][4], int32 offsets [n_inputs + 1], float poses [n_inputs][3], int32 groups [n_inputs]) are voxelised into a reserved set of n_groups
// clouds; with res2_bits != 0 that set is then voxelised IN PLACE (cloud g to cloud g, no poses) at the second resolution.  Prints counts, dropped counts and
// the clouds of each pass as JSON (floats as bits): the Python test compares it with api.voxelize on the same inputs.
#include <lsm2d_voxelize.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

static void print_pass(const char* name, const Voxelization& v, const ReservedClouds& dst) {
  printf("\"%s\": {\"fits\": %d, ", name, v.fits ? 1 : 0);
  print_int_list("counts", v.counts, ", "); print_int_list("dropped", v.dropped, ", ");
  printf("\"clouds\": [");
  for (int32_t g = 0; g < dst.numClouds(); ++g) {
    const PointNormal2fVectorCloud c = dst.download(g);
    printf("%s[", g ? "," : "");
    for (size_t i = 0; i < c.size(); ++i) printf("%s%u,%u,%u,%u", i ? "," : "", bits(c[i].x), bits(c[i].y), bits(c[i].nx), bits(c[i].ny));
    printf("]");
  }
  printf("]}");
}

int main(int argc, char** argv) {
  if (argc < 10) { fprintf(stderr, "usage: %s points.bin offsets.bin poses.bin|- groups.bin|- n_groups capacity res_bits nres_bits res2_bits\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    const std::vector<PointNormal2f> pts = read_all<PointNormal2f>(argv[1]);
    const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
    std::vector<PointNormal2fVectorCloud> clouds;
    for (size_t k = 0; k + 1 < offs.size(); ++k) clouds.emplace_back(pts.begin() + offs[k], pts.begin() + offs[k + 1]);
    const std::vector<Vector3f> poses = read_all_or_empty<Vector3f>(argv[3]);
    const std::vector<int32_t> groups = read_all_or_empty<int32_t>(argv[4]);
    const int32_t n_groups = atoi(argv[5]);
    CloudSet src(ctx, clouds);
    ReservedClouds dst(ctx, n_groups, atoll(argv[6]));
    const lsm2d_voxelize_params p1{from_bits_arg(argv[7]), from_bits_arg(argv[8])};
    const Voxelization a = voxelize(ctx, p1, src.get(), dst.get(), n_groups, {}, poses, groups);
    printf("{");
    print_pass("first", a, dst);
    if (strtoul(argv[9], nullptr, 10) != 0) {
      const lsm2d_voxelize_params p2{from_bits_arg(argv[9]), from_bits_arg(argv[8])};
      std::vector<int32_t> each((size_t) n_groups);
      for (int32_t g = 0; g < n_groups; ++g) each[(size_t) g] = g;
      const Voxelization b = voxelize(ctx, p2, dst.get(), dst.get(), n_groups, {}, {}, each);
      printf(", ");
      print_pass("in_place", b, dst);
    }
    printf("}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
