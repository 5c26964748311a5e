// lsm2d_k_relocalize.h -- the glue that chains the hypothesis scoring to the aligner without the host (lsm2d_relocalize_select).
// Part of lsm2d_kernels.h (included there inside namespace lsm2d, behind the selection and k_align_rows).
//
// The relocaliser / loop detector (MULTI.json:749-769, :964-986) scores n hypotheses, keeps the best k_score that pass the acceptance test, aligns those and
// judges the aligned ones.  The scoring's selection leaves [n_accepted, n_selected, 0, 0 | index[k_score] | rows] in device memory; the hypotheses' poses,
// priors and cloud index tables lie where the scoring's ONE upload put them.  Two small kernels stand between the two stages:
//   k_reloc_items      a thread per slot j < k_score of the aligner's input block: slot j is hypothesis index[j] -- its pose, its PriorDev, its cloud in
//                      every slice's sets (lsm2d_batch's rule spelled out: the table's entry, else cloud i, else the only cloud).  A slot j >= n_selected, a
//                      PAD, repeats slot 0's hypothesis (hypothesis 0 when nothing was selected): a real alignment of valid inputs, so every workgroup of the
//                      aligner's launch reports and the never-written check stays meaningful.
//   k_align_rows_live  k_align_rows with the number of LIVE candidates read from the device: rows of pads get ok = 0 -- never ranked, never counted as
//                      Success, never in an output; never-written statuses are counted over all slots.
// Words are moved as bits.  No float atomics, no workgroup waits for another, no scratch memory.
#pragma once

struct RelocSlice {
  const int32_t* f_index; const int32_t* m_index;      // [n_items] the scoring's tables for this slice, or nullptr: cloud i, or cloud 0 of a one-cloud set
  int32_t f_clouds, m_clouds;
  int32_t* f_out; int32_t* m_out;                      // [k_score] the aligner's index arrays for this slice (CloudDev::index)
};

struct RelocItemsArgs {
  const int32_t* sel;            // the scoring's selection as it goes down: [n_accepted, n_selected, 0, 0 | index[k_score] | ...]
  const float* poses;            // [n_items][3] the scoring's upload
  const PriorDev* prior;         // [n_items] or nullptr
  int32_t n_items, n_slices, k_score;
  float* pose_out;               // [k_score][3]  AlignArgs::init_pose
  PriorDev* prior_out;           // [k_score]     AlignArgs::prior (nullptr when there is none)
  RelocSlice s[kMaxSlices];
};

static_assert(sizeof(PriorDev) % sizeof(int32_t) == 0, "a prior is moved word by word");

__global__ __launch_bounds__(256) void k_reloc_items(const RelocItemsArgs A) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= A.k_score) return;
  int n_sel = A.sel[1];
  n_sel = n_sel < 0 ? 0 : (n_sel > A.k_score ? A.k_score : n_sel);
  int h = n_sel > 0 ? A.sel[kSelectHeaderWords + (j < n_sel ? j : 0)] : 0;
  if ((uint32_t) h >= (uint32_t) A.n_items) h = 0;      // (cannot be: the selection's indices are item indices)
  const int32_t* p = reinterpret_cast<const int32_t*>(A.poses) + 3 * (size_t) h;
  int32_t* po = reinterpret_cast<int32_t*>(A.pose_out) + 3 * (size_t) j;
  for (int w = 0; w < 3; ++w) po[w] = p[w];
  if (A.prior) {
    constexpr int kPriorWords = (int) (sizeof(PriorDev) / sizeof(int32_t));
    const int32_t* q = reinterpret_cast<const int32_t*>(A.prior + h);
    int32_t* qo = reinterpret_cast<int32_t*>(A.prior_out + j);
    for (int w = 0; w < kPriorWords; ++w) qo[w] = q[w];
  }
  for (int s = 0; s < A.n_slices; ++s) {
    const RelocSlice& S = A.s[s];
    S.f_out[j] = S.f_index ? S.f_index[h] : (S.f_clouds == 1 ? 0 : h);
    S.m_out[j] = S.m_index ? S.m_index[h] : (S.m_clouds == 1 ? 0 : h);
  }
}

struct AlignRowsLiveArgs {
  AlignRowsArgs R;
  const int32_t* n_live;         // one word on the device: candidates i < *n_live are real, the others pads
};

// A COPY of k_align_rows (lsm2d_k_align_select.h) in which one statement differs: `success` also asks for i < n_live.  Keep the two in step by hand.  A body
// shared by both kernels -- a force-inlined device function template taking the live flag as a template argument and the LDS words as a pointer -- was tried:
// k_align_rows<AlignRow> then came out with 263 instruction lines against the parent's 261 and tools/isa_diff.py reported it `different`, and the existing
// instantiation has to keep its instructions.
template <class Row>
__global__ __launch_bounds__(256) void k_align_rows_live(const AlignRowsLiveArgs L) {
  __shared__ int32_t s_cnt[8];
  const AlignRowsArgs& A = L.R;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n_live = *L.n_live;
  bool success = false, unwritten = false;
  if (i < A.n) {
    int32_t* row = reinterpret_cast<int32_t*>(A.rows) + (size_t) i * Row::kWords;      // words are moved as bits
    const int32_t st = A.status[i], its = A.its[i];
    success = st == 0 && i < n_live; unwritten = st == A.not_written;      // (the one difference: a pad is never a Success, whatever its alignment ended with)
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
