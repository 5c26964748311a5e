// lsm2d_k_select.h -- acceptance test and best-k ranking over the result rows lsm2d_score_batch's kernels leave on the device (lsm2d_score_select).
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d).
//
// The candidate loops of the loop detector and the relocaliser (MULTI.json:964-986, :749-769) ask of n scored hypotheses "which pass the acceptance test, and
// which of those are best?".  Three kernels answer on the device, behind the last launch group of the scoring, so that only k rows travel:
//   k_select_keys    a thread per item: the acceptance test on its row, a 64-bit sort key, the number of accepted items.
//   k_select_tile    a workgroup per tile of kSelectTile (key, index) entries: a bitonic sort in LDS by (key, index), the k smallest written out.  Queued
//                    again and again over the survivors until one tile is left: ceil(n / tile) x k entries per pass, less than half of what came in.
//   k_select_gather  the selected rows, their indices and the two counters into ONE contiguous region: what the host copies down.
//   k_select_tile_one  a batch of at most one tile: the three steps above in ONE launch of one workgroup (the same device functions; the count needs no atomic).
// The order is total -- n_inliers descending, chi_inliers ascending on its bit pattern, item index ascending -- so the selection is unique; every entry's
// place after a pass is a function of the entries alone, never of the order in which workgroups run.  The only atomic is one integer add per workgroup of
// k_select_keys.  The same device functions, over a base offset and a size, make the selection per GROUP of a batch: lsm2d_k_select_grouped.h.
#pragma once

static constexpr int kSelectMaxK = 1024;               // LSM2D_SELECT_MAX_K
static constexpr int kSelectTile = 2 * kSelectMaxK;    // entries a workgroup of k_select_tile sorts: a power of two, 2 x the largest k, 24 KB of LDS
static constexpr int kSelectBlock = kSelectTile / 2;   // one compare-exchange per thread and step
static constexpr u64 kSelectRejected = ~(u64) 0;       // the key of a rejected item and of the padding: above every accepted key, never selected
static constexpr int kSelectHeaderWords = 4;           // a block that goes down: [n_accepted, n_selected, c2, c3 | index[k] | rows[k][Row::kWords]]
static_assert((kSelectTile & (kSelectTile - 1)) == 0 && kSelectTile >= 2 * kSelectMaxK, "the tile is a power of two holding two selections");
static_assert(kSelectTile * (sizeof(u64) + sizeof(int32_t)) < 64 * 1024, "static LDS stays below 64 KB");
static_assert(kSelectBlock <= 1024, "one workgroup");

// What a result row looks like to the selection: its length in words and where the three statistics of the acceptance test lie in it.  ScoreRow: the rows
// k_score_final_batch / k_score_seq_batch leave (linearize_final_body's words).  The kernels that read rows take the format as a template argument; a format
// with kActive >= 0 names a word that counts the aligner slices that contributed: an item whose count is 0 is rejected whatever the thresholds are
// (lsm2d_k_score_aligner.h: it has no aligner status to pass).  k_select_tile and k_select_tile_seg see keys and indices only.
struct ScoreRow { static constexpr int kWords = kLinOutWords, kChi = 9, kNin = 11, kNcorr = 13, kActive = -1; };
// A format may say that the two spare header words of a block carry two counts of its own (AlignRow, lsm2d_k_align_select.h: Success and never-written
// statuses); for every other format they are zeros.  Ungrouped, the kernel that wrote the rows made both, into the two words BEHIND SelectArgs::n_accepted.
template <class Row> struct SelectCarriesCounts { static constexpr bool value = false; };

struct SelectArgs {
  const float* rows;          // [n_items][Row::kWords]: where the scoring's last kernel left them
  int32_t n_items, k;
  int32_t min_inliers; float max_chi_per_inlier, min_inlier_ratio;
  u64* keys; int32_t* index;  // [n_items]: k_select_keys writes, the first pass of k_select_tile reads
  int32_t* n_accepted;        // one word, zeroed by the host (grouped: [n_groups])
};

// the smallest power of two >= max(m, 2), m <= kSelectTile: the entries the sort's network runs over
LSM2D_HD int select_sort_size(int m) { return m <= 2 ? 2 : 1 << (32 - __builtin_clz((unsigned) (m - 1))); }

// The acceptance test of LoopClosureSweep::accept (host/lsm2d.hpp) without its status term, in fp32.  The divisions are IEEE: the library is built without
// any fast-math flag and hipcc's fp32 divide is correctly rounded by default, so numpy's float32 quotients (api.score_rank) are the same bits.  A NaN on
// either side of a comparison makes it false: the item is rejected.
LSM2D_DEV bool select_accept(int32_t n_inliers, int32_t n_correspondences, float chi_inliers, int32_t min_inliers, float max_chi_per_inlier,
                             float min_inlier_ratio) {
  const float n_in = (float) n_inliers;
  const float per_inlier = chi_inliers / fmaxf(n_in, 1.0f);
  const float ratio = n_in / (float) (n_correspondences > 1 ? n_correspondences : 1);
  return n_inliers >= min_inliers && per_inlier <= max_chi_per_inlier && ratio >= min_inlier_ratio;
}

// item i's sort key: (0x7fffffff - n_inliers, chi_inliers' bits) when it is accepted, all ones when it is not
template <class Row>
LSM2D_DEV u64 select_key(const SelectArgs& A, int i, bool* ok) {
  const float* row = A.rows + (size_t) i * Row::kWords;
  const float chi = row[Row::kChi];
  const int32_t n_in = __float_as_int(row[Row::kNin]), n_c = __float_as_int(row[Row::kNcorr]);
  *ok = select_accept(n_in, n_c, chi, A.min_inliers, A.max_chi_per_inlier, A.min_inlier_ratio);
  if constexpr (Row::kActive >= 0) *ok = *ok && __float_as_int(row[Row::kActive]) > 0;
  return *ok ? ((u64) (uint32_t) (0x7fffffff - n_in) << 32) | (u64) __float_as_uint(chi) : kSelectRejected;
}

// is item i's status Success?  (formats that carry counts only: a group's n_success is counted from the rows)
template <class Row>
LSM2D_DEV bool select_row_success(const SelectArgs& A, int i) {
  if constexpr (SelectCarriesCounts<Row>::value) return __float_as_int(A.rows[(size_t) i * Row::kWords + Row::kStatus]) == 0;
  else return false;
}

// A workgroup of 256 threads: the keys of batch items [first, first + count), count <= 256; entry i of (A.keys, A.index) is item i.  The accepted ones are
// counted by ballot and popcount through LDS and added to *counter with ONE integer atomic.
template <class Row>
LSM2D_DEV void select_keys_chunk(const SelectArgs& A, int first, int count, int32_t* counter) {
  __shared__ int32_t s_cnt[4];
  const int i = first + (int) threadIdx.x;
  bool ok = false;
  if ((int) threadIdx.x < count && i < A.n_items) {
    A.keys[i] = select_key<Row>(A, i, &ok);
    A.index[i] = i;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (c) atomicAdd(counter, c);
  }
}

template <class Row>
__global__ __launch_bounds__(256) void k_select_keys(const SelectArgs A) { select_keys_chunk<Row>(A, (int) blockIdx.x * 256, 256, A.n_accepted); }

LSM2D_DEV bool select_before(u64 ka, int32_t ia, u64 kb, int32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// The first `size_all` entries (a power of two, at most the tile) of (s_key, s_idx) in LDS sorted ascending by (key, index): a bitonic network, one
// compare-exchange per thread and step, a barrier after every step (and in front of the first).  All pairs (key, index) are distinct -- item indices are --
// but for the padding, which is equal in both words: the network's result does not depend on how it treats equals.
LSM2D_DEV void select_sort(u64* s_key, int32_t* s_idx, int size_all) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int size = 2; size <= size_all; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;      // the t-th pair of this step
      if (hi < size_all) {
        const bool up = (lo & size) == 0;                              // ascending stretch (the last merge: all of it)
        const u64 ka = s_key[lo], kb = s_key[hi];
        const int32_t ia = s_idx[lo], ib = s_idx[hi];
        if (select_before(kb, ib, ka, ia) == up) { s_key[lo] = kb; s_key[hi] = ka; s_idx[lo] = ib; s_idx[hi] = ia; }
      }
      __syncthreads();
    }
  }
}

// n_in entries from `base` of (keys, index) into the first `fill` entries of the LDS arrays, padded with (all ones, INT32_MAX): nothing beyond the n_in
// entries is read -- the arrays end there, or a neighbouring group's entries lie there.  (A workgroup of kSelectBlock threads, as the sort's.)
LSM2D_DEV void select_load_seg(u64* s_key, int32_t* s_idx, const u64* keys, const int32_t* index, size_t base, int n_in, int fill) {
  for (int e = threadIdx.x; e < fill; e += kSelectBlock) {
    const bool in = e < n_in;
    s_key[e] = in ? keys[base + (size_t) e] : kSelectRejected;
    s_idx[e] = in ? index[base + (size_t) e] : 0x7fffffff;
  }
}

// a pass's workgroup: n_in <= tile entries from in_base sorted, the first k of them to entries [out_base, out_base + k) of (keys_out, index_out)
LSM2D_DEV void select_tile_pass(const u64* keys_in, const int32_t* index_in, size_t in_base, int n_in, int k, u64* keys_out, int32_t* index_out, size_t out_base) {
  __shared__ u64 s_key[kSelectTile];
  __shared__ int32_t s_idx[kSelectTile];
  select_load_seg(s_key, s_idx, keys_in, index_in, in_base, n_in, kSelectTile);
  select_sort(s_key, s_idx, kSelectTile);
  for (int e = threadIdx.x; e < k; e += kSelectBlock) {
    keys_out[out_base + (size_t) e] = s_key[e];
    index_out[out_base + (size_t) e] = s_idx[e];
  }
}

// Workgroup b sorts entries [b * tile, min((b + 1) * tile, n_in)) of (keys_in, index_in) and writes the first k of them to entries [b * k, (b + 1) * k) of
// (keys_out, index_out).
__global__ __launch_bounds__(kSelectBlock) void k_select_tile(const u64* keys_in, const int32_t* index_in, int32_t n_in, int32_t k, u64* keys_out,
                                                              int32_t* index_out) {
  const long long base = (long long) blockIdx.x * kSelectTile, left = (long long) n_in - base;
  select_tile_pass(keys_in, index_in, (size_t) base, left < kSelectTile ? (int) left : kSelectTile, k, keys_out, index_out, (size_t) blockIdx.x * (size_t) k);
}

// A block of the region that goes down: n_selected = min(k, n_accepted); the header with its two spare words c2, c3, then the indices and the rows of the
// first n_selected entries of the sorted (keys, index).  Positions >= n_selected are left alone (the host does not read them).
template <class Row>
LSM2D_DEV void select_gather(const SelectArgs& A, int n_acc, int32_t c2, int32_t c3, const u64* keys, const int32_t* index, int32_t* down) {
  const int n_sel = n_acc < A.k ? n_acc : A.k;
  if (threadIdx.x == 0) { down[0] = n_acc; down[1] = n_sel; down[2] = c2; down[3] = c3; }
  int32_t* d_index = down + kSelectHeaderWords;
  int32_t* d_rows = down + kSelectHeaderWords + A.k;
  const int32_t* rows = reinterpret_cast<const int32_t*>(A.rows);      // words are moved as bits: counts and the digest lie among the sums
  for (int e = threadIdx.x; e < n_sel * Row::kWords; e += (int) blockDim.x) {
    const int j = e / Row::kWords, w = e % Row::kWords;
    const int32_t i = index[j];
    if (keys[j] == kSelectRejected || (uint32_t) i >= (uint32_t) A.n_items) continue;      // (cannot be: the n_accepted smallest entries are accepted items)
    if (w == 0) d_index[j] = i;
    d_rows[e] = rows[(size_t) i * Row::kWords + w];
  }
}

// the ungrouped calls' one block: its spare words are the two counts behind the accepted count for a format that carries counts, zeros otherwise
template <class Row>
LSM2D_DEV void select_gather_all(const SelectArgs& A, int n_acc, const u64* keys, const int32_t* index, int32_t* down) {
  int32_t c2 = 0, c3 = 0;
  if constexpr (SelectCarriesCounts<Row>::value) { c2 = A.n_accepted[1]; c3 = A.n_accepted[2]; }
  select_gather<Row>(A, n_acc, c2, c3, keys, index, down);
}

template <class Row>
__global__ __launch_bounds__(256) void k_select_gather(const SelectArgs A, const u64* keys, const int32_t* index, int32_t* down) {
  select_gather_all<Row>(A, *A.n_accepted, keys, index, down);
}

// At most one tile of items in ONE workgroup: the keys of batch items [base, base + m) into LDS (entry e is item base + e), padded to `sort_size` (the
// smallest power of two >= max(m, 2): the network runs over that many entries only), and the sort.  The accepted items -- and with kSuccess, which a caller
// sets for a format that carries counts only, the Success statuses -- are counted through LDS (s_cnt: kSelectBlock / 64 words each): no atomic, A.keys,
// A.index and A.n_accepted are not used.
template <class Row, bool kSuccess>
LSM2D_DEV void select_sort_items(const SelectArgs& A, int base, int m, int sort_size, u64* s_key, int32_t* s_idx, int32_t* s_cnt, int* n_acc, int* n_suc) {
  const int t = threadIdx.x;
  int mine = 0, mine_s = 0;
  for (int e = t; e < sort_size; e += kSelectBlock) {
    bool ok = false;
    const bool in = e < m;
    s_key[e] = in ? select_key<Row>(A, base + e, &ok) : kSelectRejected;
    s_idx[e] = in ? base + e : 0x7fffffff;
    mine += __popcll(__ballot(ok));      // (over the lanes that are in the loop; lane 0 of a wave is whenever one of its lanes is)
    if constexpr (kSuccess) mine_s += __popcll(__ballot(in && select_row_success<Row>(A, base + e)));
  }
  if ((t & 63) == 0) { s_cnt[t >> 6] = mine; if constexpr (kSuccess) s_cnt[kSelectBlock / 64 + (t >> 6)] = mine_s; }
  select_sort(s_key, s_idx, sort_size);
  *n_acc = 0; *n_suc = 0;
  for (int w = 0; w < kSelectBlock / 64; ++w) { *n_acc += s_cnt[w]; if constexpr (kSuccess) *n_suc += s_cnt[kSelectBlock / 64 + w]; }
}

// n_items <= tile: keys, sort and gather by ONE workgroup in one launch.  `sort_size`: select_sort_size(n_items), from the host.
template <class Row>
__global__ __launch_bounds__(kSelectBlock) void k_select_tile_one(const SelectArgs A, int32_t sort_size, int32_t* down) {
  __shared__ u64 s_key[kSelectTile];
  __shared__ int32_t s_idx[kSelectTile];
  __shared__ int32_t s_cnt[kSelectBlock / 64];
  int n_acc, n_suc;
  select_sort_items<Row, false>(A, 0, A.n_items, sort_size, s_key, s_idx, s_cnt, &n_acc, &n_suc);
  select_gather_all<Row>(A, n_acc, s_key, s_idx, down);
}
