// Drives linearize / linearizeBatch of the C++ host mirror (lsm2d_linearize, lsm2d_linearize_batch):
//   linearize_batch_driver scans.bin offsets.bin map.bin poses.bin cols tau sum_order
// reads n ragged float32 [N,4] scans (int32 offsets [n+1]), one map and n float32 poses, finds every item's pairs with the projective finder's batch form
// (scan i fixed, the map moving), linearises the whole batch under a Cauchy robustifier of threshold tau -- once as it is and once through a reversed index
// array -- compares every item byte for byte with linearize() on that item alone, and prints the batch's results as JSON (floats as their bit patterns).
#include <lsm2d.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

int main(int argc, char** argv) {
  if (argc < 8) { fprintf(stderr, "usage: %s scans.bin offsets.bin map.bin poses.bin cols tau sum_order\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    const PointNormal2fVectorCloud all = read_all<PointNormal2f>(argv[1]);
    const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
    PointNormal2fVectorCloud map = read_all<PointNormal2f>(argv[3]);
    const std::vector<float> pf = read_all<float>(argv[4]);
    const int cols = atoi(argv[5]); const float tau = (float) atof(argv[6]);
    ctx.setOption("sum_order", atoi(argv[7]));
    const size_t n = offs.size() - 1;
    std::vector<PointNormal2fVectorCloud> scans(n);
    std::vector<Vector3f> poses(n);
    for (size_t i = 0; i < n; ++i) {
      scans[i].assign(all.begin() + offs[i], all.begin() + offs[i + 1]);
      poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}};
    }
    CloudSet scan_set(ctx, scans), map_set(ctx, map);

    CorrespondenceFinderProjective2f cf(ctx);
    cf.param_projector->param_canvas_cols = cols; cf.param_projector->param_range_max = 30.f;
    cf.param_projector->param_angle_col_min = -(float) M_PI; cf.param_projector->param_angle_col_max = (float) M_PI;
    std::vector<CorrespondenceVector> pairs = cf.computeBatch(scan_set, map_set, poses);
    pairs[n - 1].clear();      // an item without pairs
    lsm2d_slice_params sp = cf.sliceParams();
    sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = tau;

    const std::vector<Linearization> batch = linearizeBatch(ctx, sp, scan_set, map_set, pairs, poses);
    // ... a reversed index array: item i is scan n-1-i
    std::vector<int32_t> rev(n); std::vector<Vector3f> rposes(n); std::vector<CorrespondenceVector> rpairs(n);
    for (size_t i = 0; i < n; ++i) { rev[i] = (int32_t) (n - 1 - i); rposes[i] = poses[n - 1 - i]; rpairs[i] = pairs[n - 1 - i]; }
    const std::vector<Linearization> batch_rev = linearizeBatch(ctx, sp, scan_set, map_set, rpairs, rposes, rev);

    int equal_single = 1, equal_reversed = 1;
    for (size_t i = 0; i < n; ++i) {
      const Linearization one = linearize(ctx, sp, scan_set, map_set, pairs[i], poses[i], (int32_t) i, 0);
      if (!same_bytes(one, batch[i])) equal_single = 0;
      if (!same_bytes(batch[i], batch_rev[n - 1 - i])) equal_reversed = 0;
    }
    const size_t n_empty = linearizeBatch(ctx, sp, scan_set, map_set, std::vector<CorrespondenceVector>(), std::vector<Vector3f>()).size();

    printf("{\"n\": %zu, \"equal_single\": %d, \"equal_reversed\": %d, \"n_empty\": %zu, \"items\": [", n, equal_single, equal_reversed, n_empty);
    for (size_t i = 0; i < n; ++i) {
      const Linearization& r = batch[i];
      printf("%s{", i ? "," : "");
      print_bits_list("H", r.H.data(), 9, ", "); print_bits_list("b", r.b.data(), 3, ", ");
      print_stats(r.stats);
      printf(", \"pairs\": [");
      for (size_t k = 0; k < pairs[i].size(); ++k) printf("%s[%d,%d]", k ? "," : "", pairs[i][k].fixed_idx, pairs[i][k].moving_idx);
      printf("]}");
    }
    printf("]}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
