// Drives computeBatch of the C++ host mirror's finders (lsm2d_find_correspondences_batch):
//   find_batch_driver scans.bin offsets.bin map.bin poses.bin cols max_distance
// reads n ragged float32 [N,4] scans (int32 offsets [n+1]), one map and n float32 poses, runs the projective finder (scan i fixed, the map moving) and the
// exact point-query finder (the map fixed, scan i moving under the inverse pose) over the whole batch, compares every item with the same finder's compute()
// on that item alone, and prints the batches' pairs as JSON.
#include <lsm2d.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

static Vector3f x_inv(const Vector3f& a) {
  const float c = cosf(a[2]), s = sinf(a[2]);
  return Vector3f{{-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), -a[2]}};
}

static bool same_pairs(const CorrespondenceVector& a, const CorrespondenceVector& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) if (a[i].fixed_idx != b[i].fixed_idx || a[i].moving_idx != b[i].moving_idx) return false;
  return true;
}

static void print_batch(const char* key, const std::vector<CorrespondenceVector>& v) {
  printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) {
    printf("%s[", i ? "," : "");
    for (size_t k = 0; k < v[i].size(); ++k) printf("%s[%d,%d]", k ? "," : "", v[i][k].fixed_idx, v[i][k].moving_idx);
    printf("]");
  }
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: %s scans.bin offsets.bin map.bin poses.bin cols max_distance\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    const PointNormal2fVectorCloud all = read_all<PointNormal2f>(argv[1]);
    const std::vector<int32_t> offs = read_all<int32_t>(argv[2]);
    PointNormal2fVectorCloud map = read_all<PointNormal2f>(argv[3]);
    const std::vector<float> pf = read_all<float>(argv[4]);
    const int cols = atoi(argv[5]); const float md = (float) atof(argv[6]);
    const size_t n = offs.size() - 1;
    std::vector<PointNormal2fVectorCloud> scans(n);
    std::vector<Vector3f> poses(n), inv(n);
    for (size_t i = 0; i < n; ++i) {
      scans[i].assign(all.begin() + offs[i], all.begin() + offs[i + 1]);
      poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}}; inv[i] = x_inv(poses[i]);
    }
    CloudSet scan_set(ctx, scans), map_set(ctx, map);

    CorrespondenceFinderProjective2f cf(ctx);
    cf.param_projector->param_canvas_cols = cols; cf.param_projector->param_range_max = 25.f;
    cf.param_projector->param_angle_col_min = -(float) M_PI; cf.param_projector->param_angle_col_max = (float) M_PI;
    const std::vector<CorrespondenceVector> proj = cf.computeBatch(scan_set, map_set, poses);
    // ... a reversed index array: item i is scan n-1-i
    std::vector<int32_t> rev(n); std::vector<Vector3f> rposes(n);
    for (size_t i = 0; i < n; ++i) { rev[i] = (int32_t) (n - 1 - i); rposes[i] = poses[n - 1 - i]; }
    const std::vector<CorrespondenceVector> proj_rev = cf.computeBatch(scan_set, map_set, rposes, rev);

    CorrespondenceFinderKDTree2D kd(ctx, "exact"); kd.param_max_distance_m = md; kd.param_normal_cos = 0.7f;
    const std::vector<CorrespondenceVector> nn = kd.computeBatch(map_set, scan_set, inv);

    int equal_single = 1, equal_reversed = 1;
    for (size_t i = 0; i < n; ++i) {
      CorrespondenceVector one;
      cf.setFixed(&scans[i]); cf.setMoving(&map); cf.setLocalMapInSensor(poses[i]); cf.setCorrespondences(&one); cf.compute();
      if (!same_pairs(one, proj[i])) equal_single = 0;
      if (!same_pairs(proj[i], proj_rev[n - 1 - i])) equal_reversed = 0;
      CorrespondenceVector one_nn;
      kd.setFixed(&map); kd.setMoving(&scans[i]); kd.setLocalMapInSensor(inv[i]); kd.setCorrespondences(&one_nn); kd.compute();
      if (!same_pairs(one_nn, nn[i])) equal_single = 0;
    }
    const size_t n_empty = cf.computeBatch(scan_set, map_set, std::vector<Vector3f>()).size();

    printf("{\"n\": %zu, \"equal_single\": %d, \"equal_reversed\": %d, \"n_empty\": %zu, \"inv\": [", n, equal_single, equal_reversed, n_empty);
    for (size_t i = 0; i < n; ++i) printf("%s[%.9g,%.9g,%.9g]", i ? "," : "", inv[i][0], inv[i][1], inv[i][2]);
    printf("], ");
    print_batch("projective", proj); printf(", "); print_batch("nn", nn);
    printf("}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
