// Drives relocalizeSelect of the C++ host mirror (host/lsm2d_relocalize.hpp) against the existing relocalize() on the same inputs:
//   relocalize_select_driver scan.bin map.bin poses.bin cols tau iterations min_num_inliers sum_order min_inliers max_chi_bits min_ratio_bits k_score k
// One projective slice with a Cauchy robustifier, min_num_correspondences 10; the same thresholds judge both stages.  relocalize() scores, gathers on the host
// and aligns every selected hypothesis (lsm2d_align_batch); its verdict is restated here -- accepted rows ranked by inliers descending, chi_inliers ascending
// on its bits, position in the selection ascending, cut at k -- and compared with relocalizeSelect's answer byte for byte.  Prints JSON (floats as bits).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <lsm2d_relocalize.hpp>

using namespace lsm2d_host;

template <class T> static std::vector<T> read_all(const char* path) {
  FILE* f = fopen(path, "rb"); if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END); long n = ftell(f) / (long) sizeof(T); fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t) n);
  if (n && fread(v.data(), sizeof(T), (size_t) n, f) != (size_t) n) exit(2);
  fclose(f); return v;
}
static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, sizeof u); return u; }
static float from_bits(uint32_t u) { float v; memcpy(&v, &u, sizeof v); return v; }

int main(int argc, char** argv) {
  if (argc < 14) { fprintf(stderr, "usage: %s scan.bin map.bin poses.bin cols tau iterations min_num_inliers sum_order min_inliers max_chi_bits min_ratio_bits k_score k\n", argv[0]); return 2; }
  try {
    Context ctx(0);
    ctx.setOption("sum_order", atoi(argv[8]));
    const std::vector<float> pf = read_all<float>(argv[3]);
    const size_t n = pf.size() / 3;
    std::vector<Vector3f> poses(n);
    for (size_t i = 0; i < n; ++i) poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}};
    CloudSet scan(ctx, read_all<PointNormal2f>(argv[1])), map(ctx, read_all<PointNormal2f>(argv[2]));
    CorrespondenceFinderProjective2f cf(ctx);
    cf.param_projector->param_canvas_cols = atoi(argv[4]); cf.param_projector->param_range_max = 30.f;
    cf.param_projector->param_angle_col_min = -(float) M_PI; cf.param_projector->param_angle_col_max = (float) M_PI;
    lsm2d_slice_params sp = cf.sliceParams();
    sp.robustifier = LSM2D_ROBUST_CAUCHY; sp.chi_threshold = (float) atof(argv[5]); sp.min_num_correspondences = 10;
    const std::vector<lsm2d_slice_params> slices = {sp};
    const std::vector<const CloudSet*> fixed = {&scan}, moving = {&map};
    const lsm2d_aligner_params ap{atoi(argv[6]), atoi(argv[7]), 0.f, 0.f, 0, 0};
    const lsm2d_select_params select{atoi(argv[9]), from_bits((uint32_t) strtoul(argv[10], nullptr, 10)), from_bits((uint32_t) strtoul(argv[11], nullptr, 10))};
    const int32_t k_score = atoi(argv[12]), k = atoi(argv[13]);

    const AlignerRelocalization rel = relocalize(ctx, ap, slices, fixed, moving, poses, select, k_score);
    const RelocalizeSelection rs = relocalizeSelect(ctx, ap, slices, fixed, moving, poses, select, k_score, nullptr, k);

    const size_t m = rel.selection.index.size();
    int scored_equal = rs.scored.index == rel.selection.index && rs.scored.n_accepted == rel.selection.n_accepted && rs.scored.rows.size() == m;
    for (size_t j = 0; j < m && scored_equal; ++j)
      scored_equal = !memcmp(&rs.scored.rows[j].row.stats, &rel.selection.rows[j].row.stats, sizeof(lsm2d_iteration_stats));
    // relocalize()'s verdict, ranked
    std::vector<std::pair<uint64_t, size_t>> keyed; int32_t n_success = 0;
    for (size_t j = 0; j < rel.pose.size(); ++j) {
      n_success += rel.status[j] == LSM2D_SUCCESS;
      if (!rel.accepted[j] || rel.iterations[j] < 1) continue;
      keyed.emplace_back(((uint64_t) (uint32_t) (0x7fffffff - rel.last_stats[j].n_inliers) << 32) | bits(rel.last_stats[j].chi_inliers), j);
    }
    std::sort(keyed.begin(), keyed.end());
    const size_t r = std::min(keyed.size(), (size_t) k);
    const AlignSelection& a = rs.aligned;
    int aligned_equal = a.n_accepted == (int32_t) keyed.size() && a.n_success == n_success && a.index.size() == r && a.pose.size() == r;
    for (size_t q = 0; q < r && aligned_equal; ++q) {
      const size_t j = keyed[q].second;
      aligned_equal = a.index[q] == rel.selection.index[j] && !memcmp(a.pose[q].data(), rel.pose[j].data(), 12) &&
                      !memcmp(a.information[q].data(), rel.information[j].data(), 36) && a.iterations[q] == rel.iterations[j] &&
                      !memcmp(&a.last_stats[q], &rel.last_stats[j], sizeof(lsm2d_iteration_stats));
    }
    const RelocalizeSelection none = relocalizeSelect(ctx, ap, slices, fixed, moving, std::vector<Vector3f>(), select, k_score, nullptr, k);

    printf("{\"n\": %zu, \"scored_equal\": %d, \"aligned_equal\": %d, \"n_empty\": %zu, \"n_scored_accepted\": %d, \"n_accepted\": %d, \"n_success\": %d, \"scored_index\": [",
           n, scored_equal, aligned_equal, none.scored.index.size() + none.aligned.index.size() + (size_t) none.scored.n_accepted + (size_t) none.aligned.n_accepted,
           rs.scored.n_accepted, a.n_accepted, a.n_success);
    for (size_t j = 0; j < rs.scored.index.size(); ++j) printf("%s%d", j ? "," : "", rs.scored.index[j]);
    printf("], \"index\": [");
    for (size_t q = 0; q < a.index.size(); ++q) printf("%s%d", q ? "," : "", a.index[q]);
    printf("], \"rows\": [");
    for (size_t q = 0; q < a.index.size(); ++q) {
      const lsm2d_iteration_stats& s = a.last_stats[q];
      printf("%s{\"pose\": [%u,%u,%u], \"H\": [", q ? "," : "", bits(a.pose[q][0]), bits(a.pose[q][1]), bits(a.pose[q][2]));
      for (int c = 0; c < 9; ++c) printf("%s%u", c ? "," : "", bits(a.information[q][(size_t) c]));
      printf("], \"iterations\": %d, \"counts\": [%d,%d,%d], \"chi\": [%u,%u], \"digest\": [%u,%u]}", a.iterations[q], s.n_correspondences, s.n_inliers, s.n_outliers,
             bits(s.chi_inliers), bits(s.chi_outliers), s.pair_digest_lo, s.pair_digest_hi);
    }
    printf("]}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
