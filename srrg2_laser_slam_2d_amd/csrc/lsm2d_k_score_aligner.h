// lsm2d_k_score_aligner.h -- pose hypotheses scored against an ALIGNER: all its slices, their sensor offsets, the skip rule and the optional prior
// (lsm2d_score_aligner_batch / lsm2d_score_aligner_select).  Part of lsm2d_kernels.h (included there, inside namespace lsm2d).
//
// A scored item is what the first iteration of MultiAligner2D::compute holds just before its solve.  Per slice the finder's kernels and k_score_*_batch run
// as they are (lsm2d_k_split_finder.h), on that slice's own item table, counts, digests and rows; two small kernels stand round them:
//   k_score_aligner_items   a thread per (item, slice): the slice's FindItem table from the poses uploaded once -- the item's clouds by lsm2d_batch's rule,
//                           T = make_iso(Xe), Xe = X bit for bit for a slice without sensor offset, else S^-1 X in k_align's own operations (slice_iso_of:
//                           the host's compose_host, fma for fma), nn_group by find_batch_fill_items' rule on the sets' device-side sizes.
//   k_score_combine         a thread per item: counts and digests of every slice, skipped ones included; the sums of the slices with more than
//                           min_num_correspondences pairs added in fp32 in slice order from +0; the prior (prior_apply, the aligner's own) last, when one is
//                           given and a slice contributed; one combined row of kCombWords words.
// No float atomic, no workgroup waits for another, no scratch memory.
#pragma once

// a combined row: H[9] row-major, b[3], chi_inliers, chi_outliers, n_inliers, n_outliers, n_correspondences, active, the 64-bit pair digest (8-byte aligned)
static constexpr int kCombWords = 20;
struct CombRow { static constexpr int kWords = kCombWords, kChi = 12, kNin = 14, kNcorr = 16, kActive = 17; };
static constexpr int kCombB = 9, kCombChiOut = 13, kCombNout = 15, kCombDigest = 18;
static_assert(kCombDigest % 2 == 0 && kCombWords % 2 == 0, "the digest of every row is 8-byte aligned");

struct ScoreAlignerSlice {
  // k_score_aligner_items
  const int32_t* f_count; const int32_t* m_count;      // the fixed / moving set's sizes (CloudDev::count)
  const int32_t* f_index; const int32_t* m_index;      // [n_items] the item's cloud in either set, or nullptr: cloud i, or cloud 0 of a one-cloud set
  int32_t f_clouds, m_clouds;
  int32_t has_sensor; float Sinv[3], cSinv, sSinv;     // as SliceDev's
  FindItem* items;                                     // [n_items], written
  // k_score_combine
  const int32_t* count;                                // [n_items] what the slice's finder wrote
  const float* rows;                                   // [n_items][kLinOutWords] what k_score_final_batch / k_score_seq_batch wrote
  int32_t slot, min_corr;
};

struct ScoreAlignerArgs {
  const float* poses;            // [n_items][3]
  const PriorDev* prior;         // [n_items] or nullptr
  int32_t n_items, n_slices;
  float* out;                    // [n_items][kCombWords]
  ScoreAlignerSlice s[kMaxSlices];
};

// grid: (ceil(n_items / 256), n_slices)
__global__ __launch_bounds__(256) void k_score_aligner_items(const ScoreAlignerArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_items) return;
  const ScoreAlignerSlice& S = A.s[blockIdx.y];
  const float pose[3] = {A.poses[3 * (size_t) i], A.poses[3 * (size_t) i + 1], A.poses[3 * (size_t) i + 2]};
  FindItem it;
  it.fc = S.f_index ? S.f_index[i] : (S.f_clouds == 1 ? 0 : i);      // (checked against the sets by the host before the launch)
  it.mc = S.m_index ? S.m_index[i] : (S.m_clouds == 1 ? 0 : i);
  it.T = slice_iso_of(S.has_sensor, S.cSinv, S.sSinv, S.Sinv, pose);
  it.nn_group = (long long) S.f_count[it.fc] >= 4ll * (long long) S.m_count[it.mc] ? kNNGroup : 1;
  it.pad = 0;
  S.items[i] = it;
}

__global__ __launch_bounds__(256) void k_score_combine(const ScoreAlignerArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_items) return;
  float sum[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) sum[k] = 0.0f;
  int n_in = 0, n_out = 0, n_corr = 0, active = 0;
  u64 dig = 0ull;
  for (int s = 0; s < A.n_slices; ++s) {
    const ScoreAlignerSlice& S = A.s[s];
    int n = S.count[i];
    n = n < 0 ? 0 : (n > S.slot ? S.slot : n);      // score_count's clamp
    const float* row = S.rows + (size_t) i * kLinOutWords;
    n_corr += n;
    dig += *reinterpret_cast<const unsigned long long*>(row + kAccumWords);
    if (n > S.min_corr) {
#pragma unroll
      for (int k = 0; k < 11; ++k) sum[k] += row[k];
      n_in += __float_as_int(row[11]); n_out += __float_as_int(row[12]);
      ++active;
    }
  }
  float H[9] = {sum[0], sum[1], sum[2], sum[1], sum[3], sum[4], sum[2], sum[4], sum[5]};
  float b[3] = {sum[6], sum[7], sum[8]};
  if (active && A.prior) {
    const float pose[3] = {A.poses[3 * (size_t) i], A.poses[3 * (size_t) i + 1], A.poses[3 * (size_t) i + 2]};
    add_prior_inline(A.prior[i], pose, H, b);
  }
  float* o = A.out + (size_t) i * kCombWords;
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = H[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) o[kCombB + k] = b[k];
  o[CombRow::kChi] = sum[9]; o[kCombChiOut] = sum[10];
  o[CombRow::kNin] = __int_as_float(n_in); o[kCombNout] = __int_as_float(n_out); o[CombRow::kNcorr] = __int_as_float(n_corr);
  o[CombRow::kActive] = __int_as_float(active);
  *reinterpret_cast<unsigned long long*>(o + kCombDigest) = (unsigned long long) dig;
}
