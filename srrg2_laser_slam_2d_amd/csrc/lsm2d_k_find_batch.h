// lsm2d_k_find_batch.h -- the finder-level kernels for a whole batch: CorrespondenceFinder_::compute for n_items independent (fixed, moving, pose) triples in ONE launch.
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d, behind lsm2d_k_split_finder.h); not a translation unit of its own.
// One workgroup of kFindBlock threads owns one item (blockIdx.x) from its z-buffers / its first query to its last pair: nobody waits for another workgroup,
// nothing polls.  The device functions and the ballot compaction are k_find_projective's and k_find_nn's, statement for statement, so an item's pairs and
// their order are the single call's by construction (tests/test_gpu_find_batch.py compares them bit for bit).
struct FindItem {
  int32_t fc, mc;        // the item's clouds in the fixed / moving set
  Iso T;                 // local_map_in_sensor
  int32_t nn_group;      // exact NN: lanes per query (kNNGroup when the item's fixed cloud holds >= 4 x its moving cloud's points, else 1)
  int32_t pad;
};
static_assert(sizeof(FindItem) == 32, "the host fills an array of these");

struct FindBatchArgs {
  CloudDev fixed, moving;
  ProjK proj; float point_distance, normal_cos;
  const FindItem* items;      // [gridDim.x]
  int32_t* out_pairs;         // [gridDim.x][pair_capacity][2]
  int32_t* out_count;         // [gridDim.x]
  int32_t pair_capacity;
  float inl_tau;              // as FindArgs::inl_tau
};

// A cloud of any size is z-buffered by the item's own workgroup (project_cloud): the canvas is a 64-bit minimum over the cloud's keys, so it is the canvas
// k_project_split folds together from many workgroups for the single call.
__global__ __launch_bounds__(kFindBlock) void k_find_projective_batch(const FindBatchArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* mcan = reinterpret_cast<u64*>(smem);
  u64* fcan = mcan + A.proj.cols;
  __shared__ int s_wave_tot[kFindBlock / 64];
  __shared__ int s_base;
  const int tid = threadIdx.x;
  const FindItem it = A.items[blockIdx.x];
  int32_t* const out_pairs = A.out_pairs + 2 * (size_t) blockIdx.x * (size_t) A.pair_capacity;
  for (int i = tid; i < A.proj.cols; i += kFindBlock) { mcan[i] = kEmptyCell; fcan[i] = kEmptyCell; }
  if (tid == 0) s_base = 0;
  __syncthreads();
  const Iso ident = {1.0f, 0.0f, 0.0f, 0.0f};
  const int fbase = A.fixed.start[it.fc], mbase = A.moving.start[it.mc];
  project_cloud(A.fixed.xy + fbase, A.fixed.count[it.fc], ident, A.proj, fcan, tid, kFindBlock);
  project_cloud(A.moving.xy + mbase, A.moving.count[it.mc], it.T, A.proj, mcan, tid, kFindBlock);
  __syncthreads();
  SliceDev S; S.point_distance = A.point_distance; S.normal_cos = A.normal_cos;
  const int lane = tid & 63, wave = tid >> 6;
  for (int c0 = 0; c0 < A.proj.cols; c0 += kFindBlock) {
    const int col = c0 + tid;
    int fi = -1, mi = -1; float2 nf, nm; bool ok = false;
    if (col < A.proj.cols) ok = match_bin(fcan[col], mcan[col], S, it.T, A.fixed.nrm + fbase, A.moving.nrm + mbase, fi, mi, nf, nm);
    if (ok && A.inl_tau > 0.0f) ok = pair_chi(it.T, A.fixed.xy[fbase + fi], nf, A.moving.xy[mbase + mi], nm) < A.inl_tau;
    // order-preserving compaction: ballot prefix inside the wave, wave totals through LDS.  At most one pair per column and
    // pair_capacity >= cols (checked by the host before the launch), and the write is guarded besides: nothing leaves the item's slot
    const u64 bal = __ballot(ok);
    const int prefix = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int before = s_base, total = 0;
    for (int w = 0; w < kFindBlock / 64; ++w) { const int t = s_wave_tot[w]; if (w < wave) before += t; total += t; }
    if (ok && before + prefix < A.pair_capacity) { out_pairs[2 * (before + prefix)] = fi; out_pairs[2 * (before + prefix) + 1] = mi; }
    __syncthreads();
    if (tid == 0) s_base += total;
    __syncthreads();
  }
  if (tid == 0) A.out_count[blockIdx.x] = s_base;
}

struct FindNNBatchArgs {
  CloudDev fixed, moving; int32_t use_distmap; int32_t use_kd;      // at most one of the two set; neither: the exact grid search
  float max_distance, normal_cos;
  const FindItem* items;      // [gridDim.x]
  int32_t* out_pairs;         // [gridDim.x][pair_capacity][2]
  int32_t* out_count;         // [gridDim.x]
  int32_t pair_capacity;
  float inl_tau;              // as FindArgs::inl_tau
};

// An item's queries in trips of kFindBlock / group, however many there are (the single call spreads more than two trips over many workgroups and ranks the
// pairs in a second launch: the same matches in the same ascending order).  The group width is the ITEM's: one launch may hold both forms.
__global__ __launch_bounds__(kFindBlock) void k_find_nn_batch(const FindNNBatchArgs A) {
  __shared__ int s_wave_tot[kFindBlock / 64];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FindItem it = A.items[blockIdx.x];
  int32_t* const out_pairs = A.out_pairs + 2 * (size_t) blockIdx.x * (size_t) A.pair_capacity;
  if (tid == 0) s_base = 0;
  __syncthreads();
  const int fbase = A.fixed.start[it.fc], mbase = A.moving.start[it.mc], n = A.moving.count[it.mc];
  GridMeta g; DistMeta dm;
  const int32_t* cst = nullptr; const int32_t* sidx = nullptr; const float2* sxy = nullptr;
  const KdNode* knd = nullptr;
  if (A.use_distmap) dm = A.fixed.dist.meta[it.fc];
  else if (A.use_kd) { knd = A.fixed.kd.nodes + A.fixed.kd.meta[it.fc].node_base; sxy = A.fixed.kd.leaf_xy + fbase; sidx = A.fixed.kd.leaf_idx + fbase; }
  else {
    g = A.fixed.grid.meta[it.fc]; cst = A.fixed.grid.cell_start + g.cell_base;
    sidx = A.fixed.grid.sorted_idx + fbase; sxy = A.fixed.grid.sorted_xy + fbase;
  }
  const float md2 = A.max_distance * A.max_distance;
  const int group = (A.use_distmap || A.use_kd) ? 1 : it.nn_group, sub = tid & (group - 1);
  const int per_step = kFindBlock / group;
  auto query = [&](float qx, float qy) {
    if (A.use_kd) return kd_query(knd, sxy, sidx, qx, qy, md2);
    return group == kNNGroup ? nn_query<kNNGroup>(g, cst, sidx, sxy, qx, qy, A.max_distance, md2, sub)
                             : nn_query<1>(g, cst, sidx, sxy, qx, qy, A.max_distance, md2, sub);
  };
  for (int j0 = 0; j0 < n; j0 += per_step) {
    const int j = j0 + tid / group;
    int best = -1; bool ok = false;
    if (j < n) {
      const float2 pm = A.moving.xy[mbase + j];
      float qx, qy; xf_point(it.T, pm.x, pm.y, qx, qy);
      best = A.use_distmap ? distmap_lookup(dm, A.fixed.dist.parent, qx, qy) : query(qx, qy);
      if (best >= 0 && sub == 0) {
        const float2 nm = A.moving.nrm[mbase + j], nf = A.fixed.nrm[fbase + best];
        float nqx, nqy; xf_normal(it.T, nm.x, nm.y, nqx, nqy);
        ok = !(__builtin_fmaf(nqx, nf.x, nqy * nf.y) < A.normal_cos);
        if (ok && A.inl_tau > 0.0f) ok = pair_chi(it.T, A.fixed.xy[fbase + best], nf, pm, nm) < A.inl_tau;
      }
    }
    // lanes are in ascending query order (tid / group), so the ballot compaction keeps ascending moving index.  At most one pair per query and
    // pair_capacity >= the largest moving cloud (checked by the host before the launch), and the write is guarded besides: nothing leaves the item's slot
    const u64 bal = __ballot(ok);
    const int prefix = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int before = s_base, total = 0;
    for (int w = 0; w < kFindBlock / 64; ++w) { const int t = s_wave_tot[w]; if (w < wave) before += t; total += t; }
    if (ok && before + prefix < A.pair_capacity) { out_pairs[2 * (before + prefix)] = best; out_pairs[2 * (before + prefix) + 1] = j; }
    __syncthreads();
    if (tid == 0) s_base += total;
    __syncthreads();
  }
  if (tid == 0) A.out_count[blockIdx.x] = s_base;
}
