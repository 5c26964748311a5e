// lsm2d_k_align_select.h -- the row an ALIGNED candidate shows to the selection of lsm2d_k_select.h, and the kernel that packs it (lsm2d_align_select).
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d).
//
// The candidate loops of the loop detector and the relocaliser (MULTI.json:964-986, :749-769) align every candidate, keep those whose aligner succeeded and
// whose LAST iteration passes the thresholds, and take the best.  The aligner kernels leave pose, H, status, iteration count and every iteration's statistics
// in the batch's device scratch; k_align_rows turns them into one row per candidate -- the last started iteration's statistics only -- and the selection's
// kernels rank those rows where they lie: k rows travel, whatever n and the iteration count are.
//   AlignRow      [pose 3 | H 9 | status | iterations | n_corr n_in n_out chi_in chi_out dig_lo dig_hi | ok | 2 words of padding]: 24 words, 96 bytes.
//   ok            status == 0 && iterations >= 1: select_key's kActive rule ("0 rejects whatever the thresholds are") is the status term of the test.
//   k_align_rows  a thread per candidate; Success and never-written statuses are counted by ballot and popcount, one integer atomicAdd per workgroup each.
// No float atomics and no order among workgroups enters a row or a count.
#pragma once

struct AlignRow { static constexpr int kWords = 24, kPose = 0, kH = 3, kStatus = 12, kIts = 13, kStats = 14, kNcorr = 14, kNin = 15, kChi = 17, kActive = 21; };
static_assert(AlignRow::kWords % 4 == 0 && AlignRow::kActive < AlignRow::kWords && AlignRow::kStats + (int) (sizeof(StatsDev) / 4) == AlignRow::kActive, "row layout");
static_assert(sizeof(StatsDev) == 7 * sizeof(int32_t), "seven words of statistics");
// the two spare header words of the region that goes down carry k_align_rows' counts: select_gather copies them from behind the accepted count
template <> struct SelectCarriesCounts<AlignRow> { static constexpr bool value = true; };

struct AlignRowsArgs {
  const float* pose; const float* H; const int32_t* status; const int32_t* its; const StatsDev* stats;      // the batch's results in device scratch ([n][3], [n][9], [n], [n], [n][stats_stride])
  int32_t n, stats_stride, not_written;                                                                  // not_written: the value a status word holds until its workgroup reports
  float* rows;              // [n][Row::kWords]
  int32_t* counts;          // [0] Success, [1] never written: zeroed by the host
};

// (the row format is a template argument, as it is for the selection's kernels that read the rows)
template <class Row>
__global__ __launch_bounds__(256) void k_align_rows(const AlignRowsArgs A) {
  __shared__ int32_t s_cnt[8];
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool success = false, unwritten = false;
  if (i < A.n) {
    int32_t* row = reinterpret_cast<int32_t*>(A.rows) + (size_t) i * Row::kWords;      // words are moved as bits
    const int32_t st = A.status[i], its = A.its[i];
    success = st == 0; unwritten = st == A.not_written;
    const int32_t* p = reinterpret_cast<const int32_t*>(A.pose) + 3 * (size_t) i;
    const int32_t* h = reinterpret_cast<const int32_t*>(A.H) + 9 * (size_t) i;
    for (int w = 0; w < 3; ++w) row[Row::kPose + w] = p[w];
    for (int w = 0; w < 9; ++w) row[Row::kH + w] = h[w];
    row[Row::kStatus] = st; row[Row::kIts] = its;
    // the last iteration the candidate started; none (or a count outside the rows there are): zeros, and the candidate is rejected
    const bool has_row = its >= 1 && its <= A.stats_stride;
    const int32_t* s = reinterpret_cast<const int32_t*>(A.stats + (size_t) i * (size_t) A.stats_stride + (size_t) (has_row ? its - 1 : 0));
    for (int w = 0; w < 7; ++w) row[Row::kStats + w] = has_row ? s[w] : 0;
    row[Row::kActive] = (success && has_row) ? 1 : 0;
    row[Row::kActive + 1] = 0; row[Row::kActive + 2] = 0;
  }
  const unsigned long long ms = __ballot(success), mu = __ballot(unwritten);
  if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6] = __popcll(ms); s_cnt[4 + (threadIdx.x >> 6)] = __popcll(mu); }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t cs = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3], cu = s_cnt[4] + s_cnt[5] + s_cnt[6] + s_cnt[7];
    if (cs) atomicAdd(A.counts, cs);
    if (cu) atomicAdd(A.counts + 1, cu);
  }
}
