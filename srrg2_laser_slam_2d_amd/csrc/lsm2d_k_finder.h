// lsm2d_k_finder.h -- the finder-level kernels (CorrespondenceFinder_::compute): one (fixed, moving, pose) per call, or n_items independent triples in ONE launch.
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d, behind lsm2d_k_split_finder.h); not a translation unit of its own.
// In a batch launch one workgroup of kFindBlock threads owns one item (blockIdx.x) from its z-buffers / its first query to its last pair: nobody waits for
// another workgroup, nothing polls.  The single-call and the batch kernels share their bodies (find_projective_body, find_nn_body, nn_match), so an item's pairs
// and their order are the single call's (tests/test_gpu_find_batch.py compares them bit for bit).
// (FindItem, the arguments of one item: lsm2d_k_split_finder.h, where the factor over the batch finder's slots reads it too)

// ---- projective: (fixed, moving, pose) -> pairs in ascending column ------------------------------
struct FindArgs {
  CloudDev fixed, moving; int32_t fc, mc;
  ProjK proj; float point_distance, normal_cos;
  Iso T;
  int32_t* out_pairs;  // [cols][2]
  int32_t* out_count;
  const u64* fcan_global; const u64* mcan_global;      // a map-sized cloud's canvas, projected over many workgroups beforehand (k_project_split), or nullptr
  float inl_tau;         // > 0: only pairs whose factor is an inlier under a Cauchy robustifier of this threshold (chi^2 < tau) are emitted -- the aligner's
                         // keep_only_inlier_correspondences (lsm2d_align_batch_pairs); 0: every pair
};

struct FindBatchArgs {
  CloudDev fixed, moving;
  ProjK proj; float point_distance, normal_cos;
  const FindItem* items;      // [gridDim.x]
  int32_t* out_pairs;         // [gridDim.x][pair_capacity][2]
  int32_t* out_count;         // [gridDim.x]
  int32_t pair_capacity;
  float inl_tau;              // as FindArgs::inl_tau
};

// One workgroup, one (cloud fc of A.fixed, cloud mc of A.moving, T); Args: FindArgs or FindBatchArgs (the sets, the projector and the gates are read from it).
// Both clouds are z-buffered into `can` (2 x cols keys of dynamic LDS) unless a canvas comes pre-projected: a cloud of any size can be done by the workgroup
// itself, the canvas is a 64-bit minimum over the cloud's keys, so it is the canvas k_project_split folds together from many workgroups.
// At most one pair per column and capacity >= cols (the single call's buffer is cols pairs; a batch's pair_capacity is checked by the host before the launch),
// and the write is guarded besides: nothing leaves the caller's slot.
template <typename Args>
LSM2D_DEV void find_projective_body(const Args& A, int fc, int mc, const Iso& T, const u64* fcan_global, const u64* mcan_global, int32_t* out_pairs,
                                    int32_t* out_count, int capacity, u64* can, int* s_wave_tot, int* s_base) {
  u64* mcan = can; u64* fcan = mcan + A.proj.cols;
  const int tid = threadIdx.x;
  for (int i = tid; i < A.proj.cols; i += kFindBlock) { mcan[i] = kEmptyCell; fcan[i] = kEmptyCell; }
  if (tid == 0) *s_base = 0;
  __syncthreads();
  const Iso ident = {1.0f, 0.0f, 0.0f, 0.0f};
  const int fbase = A.fixed.start[fc], mbase = A.moving.start[mc];
  if (fcan_global) { for (int i = tid; i < A.proj.cols; i += kFindBlock) fcan[i] = fcan_global[i]; }
  else project_cloud(A.fixed.xy + fbase, A.fixed.count[fc], ident, A.proj, fcan, tid, kFindBlock);
  if (mcan_global) { for (int i = tid; i < A.proj.cols; i += kFindBlock) mcan[i] = mcan_global[i]; }
  else project_cloud(A.moving.xy + mbase, A.moving.count[mc], T, A.proj, mcan, tid, kFindBlock);
  __syncthreads();
  SliceDev S; S.point_distance = A.point_distance; S.normal_cos = A.normal_cos;
  for (int c0 = 0; c0 < A.proj.cols; c0 += kFindBlock) {
    const int col = c0 + tid;
    int fi = -1, mi = -1; float2 nf, nm; bool ok = false;
    if (col < A.proj.cols) ok = match_bin(fcan[col], mcan[col], S, T, A.fixed.nrm + fbase, A.moving.nrm + mbase, fi, mi, nf, nm);
    if (ok && A.inl_tau > 0.0f) ok = pair_chi(T, A.fixed.xy[fbase + fi], nf, A.moving.xy[mbase + mi], nm) < A.inl_tau;
    const int pos = block_compact_offset(ok, s_wave_tot, s_base, tid, kFindBlock / 64);      // threads are in ascending column
    if (ok && pos < capacity) { out_pairs[2 * pos] = fi; out_pairs[2 * pos + 1] = mi; }
  }
  if (tid == 0) *out_count = *s_base;
}

__global__ __launch_bounds__(kFindBlock) void k_find_projective(const FindArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int s_wave_tot[kFindBlock / 64];
  __shared__ int s_base;
  find_projective_body(A, A.fc, A.mc, A.T, A.fcan_global, A.mcan_global, A.out_pairs, A.out_count, A.proj.cols, reinterpret_cast<u64*>(smem), s_wave_tot, &s_base);
}

__global__ __launch_bounds__(kFindBlock) void k_find_projective_batch(const FindBatchArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ int s_wave_tot[kFindBlock / 64];
  __shared__ int s_base;
  const FindItem it = A.items[blockIdx.x];
  find_projective_body(A, it.fc, it.mc, it.T, nullptr, nullptr, A.out_pairs + 2 * (size_t) blockIdx.x * (size_t) A.pair_capacity, A.out_count + blockIdx.x,
                       A.pair_capacity, reinterpret_cast<u64*>(smem), s_wave_tot, &s_base);
}

// ---- point queries (exact grid NN, KD-tree, distance map): pairs in ascending moving index (correspondence_finder_kd_tree_2d.cpp:12-27) ------
struct FindNNArgs {
  CloudDev fixed, moving; int32_t fc, mc; int32_t use_distmap; int32_t use_kd;      // at most one of the two set; neither: the exact grid search
  float max_distance, normal_cos; Iso T; int32_t nn_group;
  int32_t* out_pairs; int32_t* out_count;
  int32_t* match; int32_t* block_count;      // k_find_nn_multi: per query the matched fixed index or -1; pairs per workgroup
  float inl_tau;                              // as FindArgs::inl_tau
};

struct FindNNBatchArgs {
  CloudDev fixed, moving; int32_t use_distmap; int32_t use_kd;      // at most one of the two set; neither: the exact grid search
  float max_distance, normal_cos;
  const FindItem* items;      // [gridDim.x]
  int32_t* out_pairs;         // [gridDim.x][pair_capacity][2]
  int32_t* out_count;         // [gridDim.x]
  int32_t pair_capacity;
  float inl_tau;              // as FindArgs::inl_tau
};

// what a point query against cloud fc of the fixed set reads: the search structure in use, resolved to that cloud, and the cloud's points and normals
struct NNView {
  int32_t use_distmap, use_kd;
  DistMeta dm; const int32_t* parent = nullptr;      // (dm, g: set for the structure in use only)
  GridMeta g; const int32_t* cst = nullptr;
  const KdNode* knd = nullptr;
  const int32_t* sidx = nullptr; const float2* sxy = nullptr;      // the grid's sorted points or the tree's leaves
  const float2* xy; const float2* nrm;
  LSM2D_DEV NNView(const CloudDev& fixed, int fc, int use_distmap_, int use_kd_) : use_distmap(use_distmap_), use_kd(use_kd_) {
    const int fbase = fixed.start[fc];
    xy = fixed.xy + fbase; nrm = fixed.nrm + fbase;
    if (use_distmap) { dm = fixed.dist.meta[fc]; parent = fixed.dist.parent; }
    else if (use_kd) { knd = fixed.kd.nodes + fixed.kd.meta[fc].node_base; sxy = fixed.kd.leaf_xy + fbase; sidx = fixed.kd.leaf_idx + fbase; }
    else {
      g = fixed.grid.meta[fc]; cst = fixed.grid.cell_start + g.cell_base;
      sidx = fixed.grid.sorted_idx + fbase; sxy = fixed.grid.sorted_xy + fbase;
    }
  }
};

// Query j of a moving cloud (mxy / mnrm: its points and normals): transformed by T, searched in the view, then the normal gate and the inlier gate.
// group lanes (sub = 0 .. group - 1, kNNGroup or 1; 1 for the tree and the map) work on one query.  best: the nearest fixed point within max_distance
// or -1; returns whether (best, j) is a pair -- true in the group's lane sub == 0 only.
LSM2D_DEV bool nn_match(const NNView& V, const float2* mxy, const float2* mnrm, int j, const Iso& T, int group, int sub, float max_distance, float normal_cos,
                        float inl_tau, int& best) {
  const float2 pm = mxy[j];
  float qx, qy; xf_point(T, pm.x, pm.y, qx, qy);
  const float md2 = max_distance * max_distance;
  if (V.use_distmap) best = distmap_lookup(V.dm, V.parent, qx, qy);
  else if (V.use_kd) best = kd_query(V.knd, V.sxy, V.sidx, qx, qy, md2);
  else best = group == kNNGroup ? nn_query<kNNGroup>(V.g, V.cst, V.sidx, V.sxy, qx, qy, max_distance, md2, sub)
                                : nn_query<1>(V.g, V.cst, V.sidx, V.sxy, qx, qy, max_distance, md2, sub);
  bool ok = false;
  if (best >= 0 && sub == 0) {
    const float2 nm = mnrm[j], nf = V.nrm[best];
    float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
    ok = !(__builtin_fmaf(nqx, nf.x, nqy * nf.y) < normal_cos);
    if (ok && inl_tau > 0.0f) ok = pair_chi(T, V.xy[best], nf, pm, nm) < inl_tau;
  }
  return ok;
}

// One workgroup, one (cloud fc of A.fixed, cloud mc of A.moving, T); Args: FindNNArgs or FindNNBatchArgs (the sets, the finder kind and the gates are read
// from it).  The cloud's queries go in trips of kFindBlock / group, however many there are.  Lanes are in ascending query order (tid / group), so the
// compaction keeps ascending moving index.  At most one pair per query and capacity >= the moving cloud (the single call's buffer is that many pairs; a
// batch's pair_capacity is checked by the host before the launch), and the write is guarded besides: nothing leaves the caller's slot.
template <typename Args>
LSM2D_DEV void find_nn_body(const Args& A, int fc, int mc, const Iso& T, int nn_group, int32_t* out_pairs, int32_t* out_count, int capacity, int* s_wave_tot,
                            int* s_base) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_base = 0;
  __syncthreads();
  const NNView V(A.fixed, fc, A.use_distmap, A.use_kd);
  const int mbase = A.moving.start[mc], n = A.moving.count[mc];
  const int group = (A.use_distmap || A.use_kd) ? 1 : nn_group, sub = tid & (group - 1);
  const int per_step = kFindBlock / group;
  for (int j0 = 0; j0 < n; j0 += per_step) {
    const int j = j0 + tid / group;
    int best = -1; bool ok = false;
    if (j < n) ok = nn_match(V, A.moving.xy + mbase, A.moving.nrm + mbase, j, T, group, sub, A.max_distance, A.normal_cos, A.inl_tau, best);
    const int pos = block_compact_offset(ok, s_wave_tot, s_base, tid, kFindBlock / 64);
    if (ok && pos < capacity) { out_pairs[2 * pos] = best; out_pairs[2 * pos + 1] = j; }
  }
  if (tid == 0) *out_count = *s_base;
}

__global__ __launch_bounds__(kFindBlock) void k_find_nn(const FindNNArgs A) {
  __shared__ int s_wave_tot[kFindBlock / 64];
  __shared__ int s_base;
  find_nn_body(A, A.fc, A.mc, A.T, A.nn_group, A.out_pairs, A.out_count, A.moving.count[A.mc], s_wave_tot, &s_base);
}

// The group width is the ITEM's: one launch may hold both forms.  (The single call spreads more than two trips over many workgroups and ranks the pairs in a
// second launch, k_find_nn_multi: the same matches in the same ascending order.)
__global__ __launch_bounds__(kFindBlock) void k_find_nn_batch(const FindNNBatchArgs A) {
  __shared__ int s_wave_tot[kFindBlock / 64];
  __shared__ int s_base;
  const FindItem it = A.items[blockIdx.x];
  find_nn_body(A, it.fc, it.mc, it.T, it.nn_group, A.out_pairs + 2 * (size_t) blockIdx.x * (size_t) A.pair_capacity, A.out_count + blockIdx.x, A.pair_capacity,
               s_wave_tot, &s_base);
}

// The same finder over many workgroups (more queries than one workgroup takes in one trip: a map-sized moving cloud against a scan's
// structure is 98 trips of one workgroup otherwise).  Workgroup b owns the queries [b * per_step, (b + 1) * per_step), ascending.
// Phase 0: search, normal gate, match[j] = fixed index or -1, pairs per workgroup.  Phase 1 (a second launch of the same shape): every
// workgroup adds up the counts in front of it, ranks its own pairs by ballot and writes them -- ascending moving index, as the
// reference emits them (correspondence_finder_kd_tree_2d.cpp:12-27, correspondence_finder_nn_2d.cpp:63-80).
template <int kPhase>
__global__ __launch_bounds__(kFindBlock) void k_find_nn_multi(const FindNNArgs A) {
  __shared__ int s_wave_tot[kFindBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = A.moving.count[A.mc];
  const int group = (A.use_distmap || A.use_kd) ? 1 : A.nn_group, sub = tid & (group - 1);
  const int per_step = kFindBlock / group;
  const int j = blockIdx.x * per_step + tid / group;
  if (kPhase == 0) {
    const NNView V(A.fixed, A.fc, A.use_distmap, A.use_kd);
    const int mbase = A.moving.start[A.mc];
    int best = -1; bool ok = false;
    if (j < n) {
      ok = nn_match(V, A.moving.xy + mbase, A.moving.nrm + mbase, j, A.T, group, sub, A.max_distance, A.normal_cos, A.inl_tau, best);
      if (sub == 0) A.match[j] = ok ? best : -1;
    }
    const u64 bal = __ballot(ok);
    if (lane == 0) s_wave_tot[wave] = __popcll(bal);
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < kFindBlock / 64; ++w) t += s_wave_tot[w]; A.block_count[blockIdx.x] = t; }
  } else {
    // the base comes from the counts of the workgroups in front and there is one pass: its own few lines rather than block_compact_offset's three barriers
    __shared__ int s_before;
    if (tid == 0) s_before = 0;
    __syncthreads();
    int mine = 0;
    for (int b = tid; b < (int) blockIdx.x; b += kFindBlock) mine += A.block_count[b];
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&s_before, mine);
    const int best = (j < n && sub == 0) ? A.match[j] : -1;
    const bool ok = best >= 0;
    const u64 bal = __ballot(ok);
    const int prefix = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int before = s_before, total = 0;
    for (int w = 0; w < kFindBlock / 64; ++w) { const int t = s_wave_tot[w]; if (w < wave) before += t; total += t; }
    if (ok) { A.out_pairs[2 * (before + prefix)] = best; A.out_pairs[2 * (before + prefix) + 1] = j; }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *A.out_count = s_before + total;
  }
}

