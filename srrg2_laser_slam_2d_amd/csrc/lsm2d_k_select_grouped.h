// lsm2d_k_select_grouped.h -- the selection of lsm2d_k_select.h PER GROUP of a batch (lsm2d_score_select_grouped, lsm2d_score_aligner_select_grouped,
// lsm2d_align_select_grouped).  Part of lsm2d_kernels.h (included there, inside namespace lsm2d).
//
// A fleet server's batch is N robots' candidates one behind the other: group g is items [off[g], off[g + 1]) of the batch, and every group gets its own
// acceptance count and its own best k -- the block the ungrouped selection returns for the sub-batch of g's items, with the item indices shifted by off[g].
// What goes down is one block per group, [n_accepted, n_selected, c2, c3 | index[k] | rows[k][Row::kWords]], group g's at word g * select_group_words.
//   k_select_group_one   every group fits one tile: ONE launch, a workgroup per group -- keys, count, sort and gather (k_select_tile_one with a base offset).
//   k_select_keys_seg    some group is larger than a tile: a workgroup per (group, chunk of 256 items) descriptor; one integer atomicAdd into n_accepted[g].
//   k_select_tile_seg    k_select_tile over per-workgroup descriptors {in_base, n_in, out_base}: passes over the groups that are still larger than a tile.
//   k_select_gather_group  a workgroup per group: the group's last (at most one tile of) entries sorted, its header, indices and rows gathered.
// The entries' index word is the BATCH item index: the order inside a group -- n_inliers descending, chi_inliers ascending on its bits, index ascending --
// is the ungrouped one, and no entry of one group is ever compared with an entry of another.  No workgroup waits for another; the only atomic is the one
// integer add per workgroup of k_select_keys_seg; every descriptor is read at blockIdx.x, so the sort's size is uniform in the workgroup.
#pragma once

// one workgroup's part of a launch, read from a table the host lays out (it knows every group's size) and uploads once with the call's arguments
struct SelectSeg {
  int32_t in_base, n_in;      // entries [in_base, in_base + n_in) of the pass's input arrays (k_select_keys_seg: batch items)
  int32_t out_base;           // k_select_tile_seg: the first of the k entries this workgroup writes
  int32_t aux;                // k_select_keys_seg: the group; k_select_gather_group: 1 when the group's entries lie in the second array
};

struct SelectGroupedArgs {
  SelectArgs S;                  // rows, n_items, k, thresholds as ever; keys / index: the first array, [n_items]; n_accepted: [n_groups], zeroed by the host
  const int32_t* offsets;        // [n_groups + 1], on the device
  const int32_t* unwritten;      // formats that carry counts (AlignRow): the ONE global never-written count of k_align_rows; NULL otherwise
  int32_t* down;                 // [n_groups][select_group_words]
};

template <class Row>
LSM2D_HD constexpr int select_group_words(int k) { return kSelectHeaderWords + k + k * Row::kWords; }

// the smallest power of two >= max(m, 2), m <= kSelectTile
LSM2D_DEV int select_sort_size(int m) { return m <= 2 ? 2 : 1 << (32 - __clz(m - 1)); }

// select_gather with the header's two spare words handed in and the block's place in the region the caller's: header, then the indices and the rows of the
// first n_selected entries of the sorted (keys, index).  Positions >= n_selected are left alone.
template <class Row>
LSM2D_DEV void select_gather_block(const SelectArgs& A, int n_acc, int32_t c2, int32_t c3, const u64* keys, const int32_t* index, int32_t* down) {
  const int n_sel = n_acc < A.k ? n_acc : A.k;
  if (threadIdx.x == 0) { down[0] = n_acc; down[1] = n_sel; down[2] = c2; down[3] = c3; }
  int32_t* d_index = down + kSelectHeaderWords;
  int32_t* d_rows = down + kSelectHeaderWords + A.k;
  const int32_t* rows = reinterpret_cast<const int32_t*>(A.rows);      // words are moved as bits
  for (int e = threadIdx.x; e < n_sel * Row::kWords; e += (int) blockDim.x) {
    const int j = e / Row::kWords, w = e % Row::kWords;
    const int32_t i = index[j];
    if (keys[j] == kSelectRejected || (uint32_t) i >= (uint32_t) A.n_items) continue;      // (cannot be: the n_accepted smallest entries are accepted items)
    if (w == 0) d_index[j] = i;
    d_rows[e] = rows[(size_t) i * Row::kWords + w];
  }
}

// is item i's status Success?  (formats that carry counts only: the group's n_success is counted from the rows)
template <class Row>
LSM2D_DEV bool select_row_success(const SelectArgs& A, int i) {
  if constexpr (SelectCarriesCounts<Row>::value) return __float_as_int(A.rows[(size_t) i * Row::kWords + Row::kStatus]) == 0;
  else return false;
}

// Every group is at most one tile.  Workgroup g: keys of its items into LDS (entry e is batch item off[g] + e), the accepted (and Success) counts through
// LDS, the sort over the smallest power of two >= max(size, 2), the gather into its own block.  An empty group writes its header and leaves before the sort.
template <class Row>
__global__ __launch_bounds__(kSelectBlock) void k_select_group_one(const SelectGroupedArgs A) {
  __shared__ u64 s_key[kSelectTile];
  __shared__ int32_t s_idx[kSelectTile];
  __shared__ int32_t s_cnt[2 * (kSelectBlock / 64)];
  const int t = threadIdx.x, g = blockIdx.x;
  const int o0 = A.offsets[g], m = A.offsets[g + 1] - o0;      // (uniform: read at blockIdx.x)
  int32_t* down = A.down + (size_t) g * (size_t) select_group_words<Row>(A.S.k);
  const int32_t unwritten = SelectCarriesCounts<Row>::value ? *A.unwritten : 0;
  if (m <= 0 || m > kSelectTile) {      // (larger than a tile cannot be: the host takes the segmented passes then)
    if (t == 0) { down[0] = 0; down[1] = 0; down[2] = 0; down[3] = unwritten; }
    return;
  }
  const int sort_size = select_sort_size(m);
  int mine = 0, mine_s = 0;
  for (int e = t; e < sort_size; e += kSelectBlock) {
    bool ok = false, suc = false;
    const bool in = e < m;
    s_key[e] = in ? select_key<Row>(A.S, o0 + e, &ok) : kSelectRejected;
    s_idx[e] = in ? o0 + e : 0x7fffffff;
    if (in) suc = select_row_success<Row>(A.S, o0 + e);
    mine += __popcll(__ballot(ok));      // (over the lanes that are in the loop; lane 0 of a wave is whenever one of its lanes is)
    if constexpr (SelectCarriesCounts<Row>::value) mine_s += __popcll(__ballot(suc));
  }
  if ((t & 63) == 0) { s_cnt[t >> 6] = mine; s_cnt[kSelectBlock / 64 + (t >> 6)] = mine_s; }
  select_sort(s_key, s_idx, sort_size);
  int n_acc = 0, n_suc = 0;
  for (int w = 0; w < kSelectBlock / 64; ++w) { n_acc += s_cnt[w]; n_suc += s_cnt[kSelectBlock / 64 + w]; }
  select_gather_block<Row>(A.S, n_acc, n_suc, unwritten, s_key, s_idx, down);
}

// Workgroup b: the keys of batch items [in_base, in_base + n_in), n_in <= 256, all of group `aux`; entry i of the first array is item i.
template <class Row>
__global__ __launch_bounds__(256) void k_select_keys_seg(const SelectGroupedArgs A, const SelectSeg* segs) {
  __shared__ int32_t s_cnt[4];
  const SelectSeg d = segs[blockIdx.x];
  const int i = d.in_base + (int) threadIdx.x;
  bool ok = false;
  if ((int) threadIdx.x < d.n_in && i < A.S.n_items) {
    A.S.keys[i] = select_key<Row>(A.S, i, &ok);
    A.S.index[i] = i;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int32_t c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (c) atomicAdd(A.S.n_accepted + d.aux, c);
  }
}

// n_in entries from `base` of (keys, index) into the first `fill` entries of the LDS arrays, padded with (all ones, INT32_MAX): nothing beyond the segment's
// n_in is read -- a neighbouring group's entries lie there
LSM2D_DEV void select_load_seg(u64* s_key, int32_t* s_idx, const u64* keys, const int32_t* index, int base, int n_in, int fill) {
  for (int e = threadIdx.x; e < fill; e += (int) blockDim.x) {
    const bool in = e < n_in;
    s_key[e] = in ? keys[(size_t) base + (size_t) e] : kSelectRejected;
    s_idx[e] = in ? index[(size_t) base + (size_t) e] : 0x7fffffff;
  }
}

// k_select_tile with a descriptor per workgroup: entries [in_base, in_base + n_in), n_in <= tile, sorted; the first k of them to [out_base, out_base + k).
// (A template, of one instantiation: a kernel that is no template is emitted among the library's first kernels and moves every later one's labels in the
// code object; as a template it comes behind them, with its siblings.)
template <int kTile>
__global__ __launch_bounds__(kSelectBlock) void k_select_tile_seg(const u64* keys_in, const int32_t* index_in, u64* keys_out, int32_t* index_out,
                                                                  const SelectSeg* segs, int32_t k) {
  static_assert(kTile == kSelectTile, "the one instantiation");
  __shared__ u64 s_key[kTile];
  __shared__ int32_t s_idx[kTile];
  const SelectSeg d = segs[blockIdx.x];
  const int n_in = d.n_in < kTile ? d.n_in : kTile;
  select_load_seg(s_key, s_idx, keys_in, index_in, d.in_base, n_in, kTile);
  select_sort(s_key, s_idx, kTile);
  for (int e = threadIdx.x; e < k; e += kSelectBlock) {
    keys_out[(size_t) d.out_base + (size_t) e] = s_key[e];
    index_out[(size_t) d.out_base + (size_t) e] = s_idx[e];
  }
}

// Workgroup g: group g's remaining entries -- its own keys where the group was one tile from the start, what its last pass left otherwise; at most one tile
// -- sorted, then its block gathered.  The accepted count is k_select_keys_seg's; a format that carries counts has its group's Success statuses counted
// here, from the rows, by ballot and popcount through LDS.
template <class Row>
__global__ __launch_bounds__(kSelectBlock) void k_select_gather_group(const SelectGroupedArgs A, const SelectSeg* fin, const u64* keys_b, const int32_t* index_b) {
  __shared__ u64 s_key[kSelectTile];
  __shared__ int32_t s_idx[kSelectTile];
  __shared__ int32_t s_cnt[kSelectBlock / 64];
  const int t = threadIdx.x, g = blockIdx.x;
  const SelectSeg d = fin[g];
  int32_t* down = A.down + (size_t) g * (size_t) select_group_words<Row>(A.S.k);
  const int32_t unwritten = SelectCarriesCounts<Row>::value ? *A.unwritten : 0;
  const int o0 = A.offsets[g], m = A.offsets[g + 1] - o0;
  if (m <= 0 || d.n_in <= 0 || d.n_in > kSelectTile) {
    if (t == 0) { down[0] = 0; down[1] = 0; down[2] = 0; down[3] = unwritten; }
    return;
  }
  int n_suc = 0;
  if constexpr (SelectCarriesCounts<Row>::value) {
    int mine = 0;
    for (int e0 = 0; e0 < m; e0 += kSelectBlock) {      // (a uniform trip count: every lane takes the ballot)
      const int e = e0 + t;
      mine += __popcll(__ballot(e < m && select_row_success<Row>(A.S, o0 + e)));
    }
    if ((t & 63) == 0) s_cnt[t >> 6] = mine;
  }
  const int sort_size = select_sort_size(d.n_in);
  select_load_seg(s_key, s_idx, d.aux ? keys_b : A.S.keys, d.aux ? index_b : A.S.index, d.in_base, d.n_in, sort_size);
  select_sort(s_key, s_idx, sort_size);
  if constexpr (SelectCarriesCounts<Row>::value) for (int w = 0; w < kSelectBlock / 64; ++w) n_suc += s_cnt[w];
  select_gather_block<Row>(A.S, A.S.n_accepted[g], n_suc, unwritten, s_key, s_idx, down);
}
