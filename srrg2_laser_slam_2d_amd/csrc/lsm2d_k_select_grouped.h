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

// Every group is at most one tile.  Workgroup g: keys of its items into LDS (entry e is batch item off[g] + e), the accepted (and Success) counts through
// LDS, the sort over the smallest power of two >= max(size, 2) (select_sort_items, k_select_tile_one's), the gather into its own block.  An empty group
// writes its header and leaves before the sort.
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
  int n_acc, n_suc;
  select_sort_items<Row, SelectCarriesCounts<Row>::value>(A.S, o0, m, select_sort_size(m), s_key, s_idx, s_cnt, &n_acc, &n_suc);
  select_gather<Row>(A.S, n_acc, n_suc, unwritten, s_key, s_idx, down);
}

// Workgroup b: the keys of batch items [in_base, in_base + n_in), n_in <= 256, all of group `aux`; entry i of the first array is item i.
template <class Row>
__global__ __launch_bounds__(256) void k_select_keys_seg(const SelectGroupedArgs A, const SelectSeg* segs) {
  const SelectSeg d = segs[blockIdx.x];
  select_keys_chunk<Row>(A.S, d.in_base, d.n_in, A.S.n_accepted + d.aux);
}

// k_select_tile with a descriptor per workgroup: entries [in_base, in_base + n_in), n_in <= tile, sorted; the first k of them to [out_base, out_base + k).
__global__ __launch_bounds__(kSelectBlock) void k_select_tile_seg(const u64* keys_in, const int32_t* index_in, u64* keys_out, int32_t* index_out,
                                                                  const SelectSeg* segs, int32_t k) {
  const SelectSeg d = segs[blockIdx.x];
  select_tile_pass(keys_in, index_in, (size_t) d.in_base, d.n_in < kSelectTile ? d.n_in : kSelectTile, k, keys_out, index_out, (size_t) d.out_base);
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
  select_load_seg(s_key, s_idx, d.aux ? keys_b : A.S.keys, d.aux ? index_b : A.S.index, (size_t) d.in_base, d.n_in, sort_size);
  select_sort(s_key, s_idx, sort_size);
  if constexpr (SelectCarriesCounts<Row>::value) for (int w = 0; w < kSelectBlock / 64; ++w) n_suc += s_cnt[w];
  select_gather<Row>(A.S, A.S.n_accepted[g], n_suc, unwritten, s_key, s_idx, down);
}
