// Drives the three grouped select calls twice each -- through the bare C ABI (include/lsm2d.h) and through the C++ host mirror's extension header
// (lsm2d_grouped.hpp: scoreSelectGrouped, scoreAlignerSelectGrouped, alignSelectGrouped):
//   select_grouped_driver scan.bin map.bin poses.bin groups.bin cols tau iterations min_num_inliers min_inliers max_chi_bits min_ratio_bits k
//                         score_min_inliers score_max_chi_bits score_min_ratio_bits
// reads one float32 [N,4] scan (fixed), one map (moving), n float32 poses and the n_groups + 1 int32 group offsets; one projective slice with a Cauchy
// robustifier of threshold tau (the aligner forms: that slice alone, no sensor offset, no prior).  Prints one JSON object: per call and route a list with one
// entry per group -- n_accepted, n_success (-1 where the call has none), the selected batch indices, and the selected rows' words as unsigned integers
// (score: H 9, b 3, statistics 7; score_aligner: the same and active; align: pose 3, H 9, iterations, statistics 7).  The two float thresholds come as
// their bit patterns; the first triple is the align form's, the second the two score forms' (unaligned hypotheses pass other thresholds than aligned ones).
#include <lsm2d_grouped.hpp>

#include "driver_common.h"

using namespace lsm2d_host;

// one group's block as words
struct Block { int32_t n_accepted = 0, n_success = -1; std::vector<int32_t> index; std::vector<uint32_t> words; };
static void put(Block& b, const void* p, size_t n_words) { const uint32_t* w = (const uint32_t*) p; b.words.insert(b.words.end(), w, w + n_words); }
static void print_blocks(const char* name, const std::vector<Block>& blocks) {
  printf("\"%s\": [", name);
  for (size_t g = 0; g < blocks.size(); ++g) {
    const Block& b = blocks[g];
    printf("%s{\"n_accepted\": %d, \"n_success\": %d, ", g ? "," : "", b.n_accepted, b.n_success);
    print_int_list("index", b.index, ", ");
    printf("\"words\": [");
    for (size_t j = 0; j < b.words.size(); ++j) printf("%s%u", j ? "," : "", b.words[j]);
    printf("]}");
  }
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 16) { fprintf(stderr, "usage: %s scan.bin map.bin poses.bin groups.bin cols tau iterations min_num_inliers min_inliers max_chi_bits min_ratio_bits k score_min_inliers score_max_chi_bits score_min_ratio_bits\n", argv[0]); return 2; }
  try {
    const PointNormal2fVectorCloud scan = read_all<PointNormal2f>(argv[1]);
    const PointNormal2fVectorCloud map = read_all<PointNormal2f>(argv[2]);
    const std::vector<float> pf = read_all<float>(argv[3]);
    const std::vector<int32_t> groups = read_all<int32_t>(argv[4]);
    const int cols = atoi(argv[5]); const float tau = (float) atof(argv[6]);
    const int iterations = atoi(argv[7]), min_num_inliers = atoi(argv[8]);
    const lsm2d_select_params select{atoi(argv[9]), from_bits_arg(argv[10]), from_bits_arg(argv[11])};
    const int32_t k = atoi(argv[12]);
    const lsm2d_select_params select_score{atoi(argv[13]), from_bits_arg(argv[14]), from_bits_arg(argv[15])};
    const size_t n = pf.size() / 3, G = groups.size() - 1, K = (size_t) k, rows = G * K;
    std::vector<Vector3f> poses(n);
    for (size_t i = 0; i < n; ++i) poses[i] = Vector3f{{pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]}};

    PointNormal2fProjectorPolar projector;
    projector.param_canvas_cols = cols; projector.param_range_max = 30.f; projector.param_angle_col_min = -(float) M_PI; projector.param_angle_col_max = (float) M_PI;
    const lsm2d_slice_params sp = LoopClosureSweep::projectiveSlice(projector, 0.5f, 0.8f, tau, 10);
    const lsm2d_aligner_params ap{iterations, min_num_inliers, 0.f, 0.f, 0, 0};

    Context ctx(0);
    CloudSet scan_set(ctx, scan), map_set(ctx, map);
    const lsm2d_cloudset* fx[1] = {scan_set.get()}; const lsm2d_cloudset* mv[1] = {map_set.get()};
    lsm2d_batch b{}; b.n_alignments = (int32_t) n; b.n_slices = 1; b.slices = &sp; b.fixed = fx; b.moving = mv; b.init_pose = pf.data();
    std::vector<int32_t> index(rows), n_sel(G), n_acc(G), n_suc(G), its(rows), active(rows);
    std::vector<float> H(9 * rows), bb(3 * rows), pose(3 * rows); std::vector<lsm2d_iteration_stats> st(rows);
    std::vector<Block> blocks;
    printf("{\"n\": %zu, \"n_groups\": %zu, ", n, G);

    // ---- the score form
    must(lsm2d_score_select_grouped(ctx.get(), &sp, scan_set.get(), nullptr, map_set.get(), nullptr, (int32_t) n, pf.data(), &select_score, k, (int32_t) G, groups.data(),
                                    index.data(), H.data(), bb.data(), st.data(), n_sel.data(), n_acc.data()), "lsm2d_score_select_grouped", ctx.get());
    blocks.assign(G, Block());
    for (size_t g = 0; g < G; ++g) {
      blocks[g].n_accepted = n_acc[g];
      for (size_t s = g * K; s < g * K + (size_t) n_sel[g]; ++s) { blocks[g].index.push_back(index[s]); put(blocks[g], &H[9 * s], 9); put(blocks[g], &bb[3 * s], 3); put(blocks[g], &st[s], 7); }
    }
    print_blocks("score_abi", blocks); printf(", ");
    const std::vector<Selection> ss = scoreSelectGrouped(ctx, sp, scan_set, map_set, poses, groups, select_score, k);
    blocks.assign(G, Block());
    for (size_t g = 0; g < G; ++g) {
      blocks[g].n_accepted = ss[g].n_accepted; blocks[g].index = ss[g].index;
      for (const Linearization& r : ss[g].rows) { put(blocks[g], r.H.data(), 9); put(blocks[g], r.b.data(), 3); put(blocks[g], &r.stats, 7); }
    }
    print_blocks("score_mirror", blocks); printf(", ");

    // ---- the score-aligner form
    must(lsm2d_score_aligner_select_grouped(ctx.get(), &b, &select_score, k, (int32_t) G, groups.data(), index.data(), H.data(), bb.data(), st.data(), active.data(),
                                            n_sel.data(), n_acc.data()), "lsm2d_score_aligner_select_grouped", ctx.get());
    blocks.assign(G, Block());
    for (size_t g = 0; g < G; ++g) {
      blocks[g].n_accepted = n_acc[g];
      for (size_t s = g * K; s < g * K + (size_t) n_sel[g]; ++s) {
        blocks[g].index.push_back(index[s]); put(blocks[g], &H[9 * s], 9); put(blocks[g], &bb[3 * s], 3); put(blocks[g], &st[s], 7); put(blocks[g], &active[s], 1);
      }
    }
    print_blocks("score_aligner_abi", blocks); printf(", ");
    const std::vector<AlignerSelection> as = scoreAlignerSelectGrouped(ctx, {sp}, {&scan_set}, {&map_set}, poses, groups, select_score, k);
    blocks.assign(G, Block());
    for (size_t g = 0; g < G; ++g) {
      blocks[g].n_accepted = as[g].n_accepted; blocks[g].index = as[g].index;
      for (const AlignerScore& r : as[g].rows) { put(blocks[g], r.row.H.data(), 9); put(blocks[g], r.row.b.data(), 3); put(blocks[g], &r.row.stats, 7); put(blocks[g], &r.active, 1); }
    }
    print_blocks("score_aligner_mirror", blocks); printf(", ");

    // ---- the align form
    must(lsm2d_align_select_grouped(ctx.get(), &ap, &b, &select, k, (int32_t) G, groups.data(), index.data(), pose.data(), H.data(), its.data(), st.data(), n_sel.data(),
                                    n_acc.data(), n_suc.data()), "lsm2d_align_select_grouped", ctx.get());
    blocks.assign(G, Block());
    for (size_t g = 0; g < G; ++g) {
      blocks[g].n_accepted = n_acc[g]; blocks[g].n_success = n_suc[g];
      for (size_t s = g * K; s < g * K + (size_t) n_sel[g]; ++s) {
        blocks[g].index.push_back(index[s]); put(blocks[g], &pose[3 * s], 3); put(blocks[g], &H[9 * s], 9); put(blocks[g], &its[s], 1); put(blocks[g], &st[s], 7);
      }
    }
    print_blocks("align_abi", blocks); printf(", ");
    const std::vector<AlignSelection> al = alignSelectGrouped(ctx, ap, {sp}, {&scan_set}, {&map_set}, poses, groups, select, k);
    blocks.assign(G, Block());
    for (size_t g = 0; g < G; ++g) {
      blocks[g].n_accepted = al[g].n_accepted; blocks[g].n_success = al[g].n_success; blocks[g].index = al[g].index;
      for (size_t j = 0; j < al[g].index.size(); ++j) {
        put(blocks[g], al[g].pose[j].data(), 3); put(blocks[g], al[g].information[j].data(), 9); put(blocks[g], &al[g].iterations[j], 1); put(blocks[g], &al[g].last_stats[j], 7);
      }
    }
    print_blocks("align_mirror", blocks);
    printf("}\n");
  } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
  return 0;
}
