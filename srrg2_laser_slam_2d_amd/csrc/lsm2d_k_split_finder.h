// lsm2d_k_split_finder.h -- the split aligner path (k_split_project / k_split_finish), the projector and the factor over a correspondence vector (the finder-level kernels: lsm2d_k_finder.h).
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d, in this order); not a translation unit of its own.
// ---- split path: the same alignment spread over many workgroups -------------------------------------------------
// For a handful of alignments against a big cloud one workgroup per alignment leaves the chip empty, so each iteration
// becomes two launches: k_split_project z-buffers slices of the cloud in LDS and folds them into a global canvas
// (atomicMin u64 is order independent), k_split_finish does the bin walk, the reduction (same thread <-> column mapping,
// same order as k_align, hence bit-identical sums), the 3x3 solve and the pose update.  Projective slices only.
struct SplitArgs {
  AlignArgs A;
  u64* gcan;             // [n_align][2 * fcan_total]: fixed canvases then moving canvases, pre-filled with kEmptyCell
  float* pose;           // [n_align][3] current estimate
  int32_t* done;         // [n_align] 0 = running
  float* H_last;         // [n_align][9]
  StatsDev* last;        // [n_align]
  int32_t* phase;        // [n_align][3]: phase (0 regular, 1 inlier-only runs), its first iteration, its end -- zero-filled means (0, 0, max_it)
  int32_t it;            // iteration this launch belongs to
};


template <bool kFixed>
__global__ __launch_bounds__(512) void k_split_project(const SplitArgs S) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* can = reinterpret_cast<u64*>(smem);
  __shared__ Iso s_T;
  const int a = blockIdx.y, sl = blockIdx.z, tid = threadIdx.x;
  if (S.done[a]) return;
  const SliceDev& SL = S.A.s[sl];
  const CloudDev& C = kFixed ? SL.fixed : SL.moving;
  const int ci = pick_cloud(C, a), n = C.count[ci];
  const int npairs = (n + 1) >> 1;
  const int per = (npairs + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = lo + per < npairs ? lo + per : npairs;
  if (lo >= hi) return;
  if (tid == 0) {
    if (kFixed) { s_T.c = 1.0f; s_T.s = 0.0f; s_T.tx = 0.0f; s_T.ty = 0.0f; }
    else { const float p[3] = {S.pose[3 * a], S.pose[3 * a + 1], S.pose[3 * a + 2]}; s_T = slice_iso(SL, p); }
  }
  const ProjK P = SL.proj;
  for (int i = tid; i < P.cols; i += 512) can[i] = kEmptyCell;
  __syncthreads();
  const Iso T = s_T;
  const float4* xy4 = reinterpret_cast<const float4*>(C.xy + C.start[ci]);
  for (int j = lo + tid; j < hi; j += 512) {
    const float4 v = xy4[j];
    project_point(T, P, v.x, v.y, 2 * j, can);
    if (2 * j + 1 < n) project_point(T, P, v.z, v.w, 2 * j + 1, can);
  }
  __syncthreads();
  u64* g = S.gcan + (size_t) a * 2 * S.A.fcan_total + (kFixed ? 0 : S.A.fcan_total) + SL.fcan_offset;
  for (int i = tid; i < P.cols; i += 512) { const u64 k = can[i]; if (k != kEmptyCell) atomicMin(&g[i], k); }
}

// kSeq: "sum_order" 1 -- the sums pair after pair in ascending column (lsm2d_device.h: pair_terms / seq_walk), as k_align_seq forms them
template <bool kSeq>
__global__ __launch_bounds__(kAlignBlock) void k_split_finish(const SplitArgs S) {
  const AlignArgs& A = S.A;
  __shared__ float red[(kAlignBlock / 64) * kAccumWords];
  __shared__ __attribute__((aligned(16))) float s_rec[kSeq ? kSeqHalf * kSeqFields : 4];
  __shared__ Iso s_iso[kMaxSlices];
  // as in k_align: the iteration's sums are added in LDS by the lanes that gathered them, the matrix is assembled, given its prior and
  // solved where it lies (no private arrays, no scratch on the serial stretch)
  __shared__ float s_H[9], s_rhs[3], s_sum[kAccumWords + 2], s_pose[3];
  __shared__ int s_n_corr, s_active;
  __shared__ u64 s_dig;
  const int a = blockIdx.x, tid = threadIdx.x;
  constexpr int nwaves = kAlignBlock / 64;
  if (S.done[a]) return;
  const bool want_dig = A.out_stats != nullptr;
  const bool inl_only = A.inlier_runs && S.phase[3 * a] != 0;
  if (tid == 0) {
    s_dig = 0ull;
    s_pose[0] = S.pose[3 * a]; s_pose[1] = S.pose[3 * a + 1]; s_pose[2] = S.pose[3 * a + 2];
    if (A.out_last_pose) { A.out_last_pose[3 * a] = s_pose[0]; A.out_last_pose[3 * a + 1] = s_pose[1]; A.out_last_pose[3 * a + 2] = s_pose[2]; }
    for (int s = 0; s < A.n_slices; ++s) s_iso[s] = slice_iso(A.s[s], s_pose);
    for (int k = 0; k < 11; ++k) s_sum[k] = 0.0f;
    s_sum[11] = s_sum[12] = __int_as_float(0);
    s_n_corr = s_active = 0;
  }
  __syncthreads();
  u64* gF = S.gcan + (size_t) a * 2 * A.fcan_total; u64* gM = gF + A.fcan_total;
  for (int s = 0; s < A.n_slices; ++s) {
    const SliceDev& SL = A.s[s];
    const Iso T = s_iso[s];
    const int fc = pick_cloud(SL.fixed, a), mc = pick_cloud(SL.moving, a);
    const int mbase = SL.moving.start[mc], fbase = SL.fixed.start[fc];
    const float2* fn = SL.fixed.nrm + fbase; const float2* mn = SL.moving.nrm + mbase;
    const float2* fp = SL.fixed.xy + fbase;  const float2* mp = SL.moving.xy + mbase;
    Accum acc; accum_zero(acc);
    float seq_acc = 0.0f;
    if constexpr (kSeq) {
      for (int col0 = 0; col0 < SL.proj.cols; col0 += kAlignBlock) {      // trips of kAlignBlock consecutive columns, every thread in every trip (barriers)
        const int col = col0 + tid;
        float t[kSeqFields]; seq_zero(t);
        if (col < SL.proj.cols) {
          const u64 mk = gM[SL.fcan_offset + col];
          gM[SL.fcan_offset + col] = kEmptyCell;
          int fi, mi; float2 nf, nm;
          if (match_bin(gF[SL.fcan_offset + col], mk, SL, T, fn, mn, fi, mi, nf, nm)) {
            if (want_dig) digest_add(&s_dig, (uint32_t) s * 0x632BE5ABu, fi, mi);
            bool inl; pair_terms(T, fp[fi], nf, mp[mi], nm, SL.cauchy != 0, SL.tau, inl_only, t, inl);
            ++acc.n_corr; acc.n_in += inl ? 1 : 0; acc.n_out += inl ? 0 : 1;
          }
        }
        const int n_rec = SL.proj.cols - col0 < kAlignBlock ? SL.proj.cols - col0 : kAlignBlock;
        for (int h0 = 0; h0 < n_rec; h0 += kSeqHalf) {      // the trip's records in two halves
          if (tid >= h0 && tid < h0 + kSeqHalf) seq_store(s_rec, tid - h0, t);
          __syncthreads();
          const int left = n_rec - h0;
          if (tid < 64) seq_acc = seq_walk(s_rec, left < kSeqHalf ? left : kSeqHalf, tid, seq_acc);
          __syncthreads();
        }
      }
    } else
    for (int col = tid; col < SL.proj.cols; col += kAlignBlock) {
      const u64 mk = gM[SL.fcan_offset + col];
      gM[SL.fcan_offset + col] = kEmptyCell;                  // ready for the next iteration's projection
      int fi, mi; float2 nf, nm;
      if (match_bin(gF[SL.fcan_offset + col], mk, SL, T, fn, mn, fi, mi, nf, nm)) {
        if (want_dig) digest_add(&s_dig, (uint32_t) s * 0x632BE5ABu, fi, mi);
        accumulate_pair(T, fp[fi], nf, mp[mi], nm, SL.cauchy != 0, SL.tau, acc, inl_only);
      }
    }
    block_reduce_store(acc, red, tid);
    __syncthreads();
    if (tid < 64) {
      float v; int vi; block_reduce_gather_lane(red, nwaves, tid, v, vi);
      if constexpr (kSeq) v = seq_total(seq_acc, tid);
      const int n_corr = __builtin_amdgcn_readlane(vi, 13);
      if (tid == 0) s_n_corr += n_corr;
      if (n_corr > SL.min_corr) {
        if (tid < 11) s_sum[tid] += v;
        else if (tid < 13) s_sum[tid] = __int_as_float(__float_as_int(s_sum[tid]) + vi);
        if (tid == 0) ++s_active;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    StatsDev last; last.n_corr = s_n_corr; last.n_in = __float_as_int(s_sum[11]); last.n_out = __float_as_int(s_sum[12]); last.chi_in = s_sum[9]; last.chi_out = s_sum[10];
    if (A.out_stats) { const u64 dg = s_dig; last.dig_lo = (uint32_t) dg; last.dig_hi = (uint32_t) (dg >> 32); A.out_stats[(size_t) a * A.stats_stride + S.it] = last; }
    int status = LSM2D_RUNNING;
    bool stop_now = false;
    const int ph = A.inlier_runs ? S.phase[3 * a] : 0, ph_start = ph ? S.phase[3 * a + 1] : 0, ph_end = ph ? S.phase[3 * a + 2] : A.max_it;
    if (!s_active) {
      status = LSM2D_NOT_ENOUGH_CORRESPONDENCES;
      for (int k = 0; k < 9; ++k) s_H[k] = S.it == 0 ? 0.0f : S.H_last[9 * a + k];      // the information matrix stays the last solved iteration's
    } else {
      s_H[0] = s_sum[0]; s_H[1] = s_sum[1]; s_H[2] = s_sum[2]; s_H[3] = s_sum[1]; s_H[4] = s_sum[3]; s_H[5] = s_sum[4];
      s_H[6] = s_sum[2]; s_H[7] = s_sum[4]; s_H[8] = s_sum[5];
      s_rhs[0] = s_sum[6]; s_rhs[1] = s_sum[7]; s_rhs[2] = s_sum[8];
      if (A.prior) add_prior(A.prior[a], s_pose, s_H, s_rhs);
      for (int k = 0; k < 9; ++k) S.H_last[9 * a + k] = s_H[k];
      if (!solve_update(s_H, s_rhs, A.damping, s_pose)) status = LSM2D_SINGULAR_H;
      else {
        S.pose[3 * a] = s_pose[0]; S.pose[3 * a + 1] = s_pose[1]; S.pose[3 * a + 2] = s_pose[2];
        if (A.term_eps > 0.0f) {       // as in k_align; the previous iteration's statistics wait in S.last
          const float chi_now = last.chi_in + last.chi_out;
          if (S.it > ph_start) { const StatsDev pv = S.last[a]; stop_now = __builtin_fabsf((pv.chi_in + pv.chi_out) - chi_now) < A.term_eps * chi_now; }
          S.last[a] = last;
        }
      }
    }
    bool last_it = S.it + 1 >= ph_end || stop_now;
    if (status == LSM2D_RUNNING && last_it && A.inlier_runs && ph == 0 && last.n_in >= A.min_inliers) {      // as in k_align: on to the inlier-only runs
      S.phase[3 * a] = 1; S.phase[3 * a + 1] = S.it + 1; S.phase[3 * a + 2] = S.it + 1 + A.max_it; last_it = false;
    }
    if (status == LSM2D_RUNNING && last_it) status = last.n_in < A.min_inliers ? LSM2D_NOT_ENOUGH_INLIERS : LSM2D_SUCCESS;
    if (status != LSM2D_RUNNING) {
      S.done[a] = 1;
      A.out_status[a] = status;
      A.out_pose[3 * a] = s_pose[0]; A.out_pose[3 * a + 1] = s_pose[1]; A.out_pose[3 * a + 2] = s_pose[2];
      if (A.out_H) for (int k = 0; k < 9; ++k) A.out_H[9 * a + k] = S.it == 0 && !s_active ? 0.0f : S.H_last[9 * a + k];
      if (A.out_its) A.out_its[a] = S.it + 1;
    }
  }
}

// ---- projector-level: canvas of one cloud --------------------------------------------------------
struct ProjectArgs {
  CloudDev cloud; int32_t ci; ProjK proj; Iso T;
  int32_t* out_src; float* out_depth; float4* out_xynn;
};

__global__ __launch_bounds__(kFindBlock) void k_project_canvas(const ProjectArgs A) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* can = reinterpret_cast<u64*>(smem);
  const int tid = threadIdx.x;
  for (int i = tid; i < A.proj.cols; i += kFindBlock) can[i] = kEmptyCell;
  __syncthreads();
  const int base = A.cloud.start[A.ci];
  project_cloud(A.cloud.xy + base, A.cloud.count[A.ci], A.T, A.proj, can, tid, kFindBlock);
  __syncthreads();
  for (int col = tid; col < A.proj.cols; col += kFindBlock) {
    const u64 k = can[col];
    int src = -1; float depth = 3.402823466e+38f; float4 t = {0.0f, 0.0f, 0.0f, 0.0f};
    if (k != kEmptyCell) {
      src = (int) (uint32_t) k; depth = __uint_as_float((uint32_t) (k >> 32));
      const float2 p = A.cloud.xy[base + src], n = A.cloud.nrm[base + src];
      xf_point(A.T, p.x, p.y, t.x, t.y);
      xf_normal(A.T, n.x, n.y, t.z, t.w);
    }
    if (A.out_src) A.out_src[col] = src;
    if (A.out_depth) A.out_depth[col] = depth;
    if (A.out_xynn) A.out_xynn[col] = t;
  }
}

// ---- factor-level: H, b, stats for a given correspondence vector ----------------------------------
struct LinArgs {
  CloudDev fixed, moving; int32_t fc, mc;
  const int32_t* pairs; int32_t n_pairs;
  Iso T; int32_t cauchy; float tau;
  float* partial;     // [n_blocks][kAccumWords]
  float* out;         // [kAccumWords]
  unsigned long long* dig;      // the pairs' digest (lsm2d_iteration_stats.pair_digest, slice 0), zeroed by the host: every workgroup adds its share
};

// The three bodies below ARE the factor's reduction: the single-call kernels (k_linearize_*) and the batch kernels (k_linearize_*_batch) both call them, so an
// item of a batch gets the single call's bits by construction (tests/test_gpu_linearize_batch.py compares them bit for bit, in both orders of summation).
// Workgroup `blk` of the `nblk` workgroups of 256 threads that share one correspondence vector: a grid-stride walk over the pairs, the thread's sums through the
// wave tree and the workgroup's four waves, one row of kAccumWords to `row`; the workgroup's share of the pair digest is added to *dig (zeroed beforehand).
// slice_salt: slice * 0x632BE5AB of the digest's hash (pair_hash_dev) -- 0 from every caller that linearises a lone slice; the aligner scoring passes its slice's.
LSM2D_DEV void linearize_partial_body(const CloudDev& fixed, const CloudDev& moving, int fc, int mc, const int32_t* pairs, int n_pairs, const Iso& T, bool cauchy,
                                      float tau, uint32_t slice_salt, int blk, int nblk, float* row, unsigned long long* dig, float* red /* [4 * kAccumWords] */, u64* s_dig) {
  const int tid = threadIdx.x;
  const int fbase = fixed.start[fc], mbase = moving.start[mc];
  Accum acc; accum_zero(acc);
  if (tid == 0) *s_dig = 0ull;
  __syncthreads();
  u64 dg = 0ull;
  for (int k = blk * 256 + tid; k < n_pairs; k += nblk * 256) {
    const int fi = pairs[2 * k], mi = pairs[2 * k + 1];
    dg += pair_hash_dev(slice_salt, (uint32_t) fi, (uint32_t) mi);
    accumulate_pair(T, fixed.xy[fbase + fi], fixed.nrm[fbase + fi], moving.xy[mbase + mi], moving.nrm[mbase + mi], cauchy, tau, acc);
  }
  if (dg) atomicAdd(reinterpret_cast<unsigned long long*>(s_dig), (unsigned long long) dg);
  block_reduce_store(acc, red, tid);
  __syncthreads();
  if (tid == 0) {
    if (dig && *s_dig) atomicAdd(dig, (unsigned long long) *s_dig);
    Accum t; block_reduce_gather(red, 4, t);
    float* p = row;
    p[0] = t.h00; p[1] = t.h01; p[2] = t.h02; p[3] = t.h11; p[4] = t.h12; p[5] = t.h22; p[6] = t.b0; p[7] = t.b1; p[8] = t.b2;
    p[9] = t.chi_in; p[10] = t.chi_out; p[11] = __int_as_float(t.n_in); p[12] = __int_as_float(t.n_out); p[13] = __int_as_float(t.n_corr);
  }
}

// ONE thread: the rows of a vector's workgroups added in ascending block order (fixed order => deterministic)
LSM2D_DEV void linearize_final_body(const float* partial, int n_blocks, float* out) {
  Accum t; block_reduce_gather(partial, n_blocks, t);
  out[0] = t.h00; out[1] = t.h01; out[2] = t.h02; out[3] = t.h11; out[4] = t.h12; out[5] = t.h22; out[6] = t.b0; out[7] = t.b1; out[8] = t.b2;
  out[9] = t.chi_in; out[10] = t.chi_out; out[11] = __int_as_float(t.n_in); out[12] = __int_as_float(t.n_out); out[13] = __int_as_float(t.n_corr);
}

// "sum_order" 1: ONE workgroup of kAlignBlock threads owns the vector: trips of kAlignBlock consecutive pairs, their terms as records in LDS, eleven lanes of
// wave 0 adding them in ascending position (lsm2d_device.h).  The totals go to out[kAccumWords], the digest to *dig (written, not added).
LSM2D_DEV void linearize_seq_body(const CloudDev& fixed, const CloudDev& moving, int fc, int mc, const int32_t* pairs, int n_pairs, const Iso& T, bool cauchy,
                                  float tau, uint32_t slice_salt, float* out, unsigned long long* dig, float* s_rec /* [kSeqHalf * kSeqFields], 16-byte aligned */,
                                  float* red /* [(kAlignBlock / 64) * kAccumWords] */, u64* s_dig) {
  const int tid = threadIdx.x;
  const int fbase = fixed.start[fc], mbase = moving.start[mc];
  Accum acc; accum_zero(acc);
  float seq_acc = 0.0f;
  if (tid == 0) *s_dig = 0ull;
  __syncthreads();
  u64 dg = 0ull;
  for (int k0 = 0; k0 < n_pairs; k0 += kAlignBlock) {
    const int k = k0 + tid;
    float t[kSeqFields]; seq_zero(t);
    if (k < n_pairs) {
      const int fi = pairs[2 * k], mi = pairs[2 * k + 1];
      dg += pair_hash_dev(slice_salt, (uint32_t) fi, (uint32_t) mi);
      bool inl; pair_terms(T, fixed.xy[fbase + fi], fixed.nrm[fbase + fi], moving.xy[mbase + mi], moving.nrm[mbase + mi], cauchy, tau, false, t, inl);
      ++acc.n_corr; acc.n_in += inl ? 1 : 0; acc.n_out += inl ? 0 : 1;
    }
    const int n_rec = n_pairs - k0 < kAlignBlock ? n_pairs - k0 : kAlignBlock;
    for (int h0 = 0; h0 < n_rec; h0 += kSeqHalf) {
      if (tid >= h0 && tid < h0 + kSeqHalf) seq_store(s_rec, tid - h0, t);
      __syncthreads();
      const int left = n_rec - h0;
      if (tid < 64) seq_acc = seq_walk(s_rec, left < kSeqHalf ? left : kSeqHalf, tid, seq_acc);
      __syncthreads();
    }
  }
  if (dg) atomicAdd(reinterpret_cast<unsigned long long*>(s_dig), (unsigned long long) dg);
  block_reduce_store(acc, red, tid);
  __syncthreads();
  if (tid < 64) {
    float v; int vi; block_reduce_gather_lane(red, kAlignBlock / 64, tid, v, vi);
    const float tot = seq_total(seq_acc, tid);
    if (tid < 11) out[tid] = tot;
    else if (tid < kAccumWords) out[tid] = __int_as_float(vi);
    if (tid == 0 && dig) *dig = (unsigned long long) *s_dig;
  }
}

__global__ __launch_bounds__(256) void k_linearize_partial(const LinArgs A) {
  __shared__ float red[4 * kAccumWords];
  __shared__ u64 s_dig;
  linearize_partial_body(A.fixed, A.moving, A.fc, A.mc, A.pairs, A.n_pairs, A.T, A.cauchy != 0, A.tau, 0u, (int) blockIdx.x, (int) gridDim.x,
                         A.partial + (size_t) blockIdx.x * kAccumWords, A.dig, red, &s_dig);
}

// "sum_order" 1: the same factor with the sums formed pair after pair in the order of the correspondence vector (the reference's loop): ONE workgroup
__global__ __launch_bounds__(kAlignBlock) void k_linearize_seq(const LinArgs A) {
  __shared__ __attribute__((aligned(16))) float s_rec[kSeqHalf * kSeqFields];
  __shared__ float red[(kAlignBlock / 64) * kAccumWords];
  __shared__ u64 s_dig;
  linearize_seq_body(A.fixed, A.moving, A.fc, A.mc, A.pairs, A.n_pairs, A.T, A.cauchy != 0, A.tau, 0u, A.out, A.dig, s_rec, red, &s_dig);
}

__global__ void k_linearize_final(const float* partial, int n_blocks, float* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  linearize_final_body(partial, n_blocks, out);
}

// ---- the factor for a whole batch of correspondence vectors (lsm2d_linearize_batch) -----------------------------------------------------
// Item i = (cloud fc of the fixed set, cloud mc of the moving set, T, n_pairs pairs from pair_base on in one packed array).  Tree order: the item owns
// `blocks` = clamp(ceil(n_pairs / 256), 1, 1024) consecutive workgroups of ONE flat launch, from block_base on -- the single call's launch shape, so its
// workgroups stride over its pairs exactly as the single call's do; wg_item (host-built, one int per workgroup) says whose workgroup this is.  A second
// launch gathers every item's rows, one thread per item.  Reference order: one workgroup of kAlignBlock threads per item.  Nobody waits for another
// workgroup; the only atomics are the digest's 64-bit wrapping adds.
struct LinItem {
  int32_t fc, mc, n_pairs, blocks;
  Iso T;
  int32_t block_base, pair_base, pad0, pad1;
};
static_assert(sizeof(LinItem) == 48, "the host fills an array of these");
static constexpr int kLinOutWords = 16;      // an item's results: the kAccumWords sums and counts, then the 64-bit pair digest

struct LinBatchArgs {
  CloudDev fixed, moving;
  const LinItem* items;       // [n_items]
  const int32_t* wg_item;     // [sum of blocks]: the item a workgroup of k_linearize_partial_batch works for
  const int32_t* pairs;       // the items' vectors one after the other, [sum of n_pairs][2]
  int32_t n_items; int32_t cauchy; float tau;
  float* partial;             // [sum of blocks][kAccumWords]
  unsigned long long* dig;    // [n_items], zeroed by the host (tree order only)
  float* out;                 // [n_items][kLinOutWords]
};

// (the item's values are the same in every lane: fetched through a uniform index they stay in scalar registers, like the single call's kernel arguments)
__global__ __launch_bounds__(256) void k_linearize_partial_batch(const LinBatchArgs A) {
  __shared__ float red[4 * kAccumWords];
  __shared__ u64 s_dig;
  const int i = __builtin_amdgcn_readfirstlane(A.wg_item[blockIdx.x]);
  const LinItem it = A.items[i];
  linearize_partial_body(A.fixed, A.moving, it.fc, it.mc, A.pairs + 2 * (size_t) it.pair_base, it.n_pairs, it.T, A.cauchy != 0, A.tau, 0u,
                         (int) blockIdx.x - it.block_base, it.blocks, A.partial + (size_t) blockIdx.x * kAccumWords, A.dig + i, red, &s_dig);
}

__global__ __launch_bounds__(256) void k_linearize_final_batch(const LinBatchArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_items) return;
  const LinItem it = A.items[i];
  float* row = A.out + (size_t) i * kLinOutWords;
  linearize_final_body(A.partial + (size_t) it.block_base * kAccumWords, it.blocks, row);
  *reinterpret_cast<unsigned long long*>(row + kAccumWords) = A.dig[i];
}

__global__ __launch_bounds__(kAlignBlock) void k_linearize_seq_batch(const LinBatchArgs A) {
  __shared__ __attribute__((aligned(16))) float s_rec[kSeqHalf * kSeqFields];
  __shared__ float red[(kAlignBlock / 64) * kAccumWords];
  __shared__ u64 s_dig;
  const LinItem it = A.items[blockIdx.x];
  float* row = A.out + (size_t) blockIdx.x * kLinOutWords;
  linearize_seq_body(A.fixed, A.moving, it.fc, it.mc, A.pairs + 2 * (size_t) it.pair_base, it.n_pairs, it.T, A.cauchy != 0, A.tau, 0u, row,
                     reinterpret_cast<unsigned long long*>(row + kAccumWords), s_rec, red, &s_dig);
}

// ---- the factor over the batch finder's own slots (lsm2d_score_batch) --------------------------------------------------------------------
// k_find_projective_batch / k_find_nn_batch leave item i's pairs in slot i of `slot` pairs and its count in count[i], both in device memory; the three kernels
// below linearise them where they lie, so the pairs never travel.  An item's count is read from the device (clamped to [0, slot]: nothing outside the slot is
// read, whatever the word holds) instead of from a host-built table, and the bodies are linearize_*_body unchanged: item i has the bits of lsm2d_linearize on
// the pairs lsm2d_find_correspondences_batch returns.  Tree order: ONE flat launch of n_items x B workgroups, B = lin_blocks(slot); workgroup w is virtual
// block w % B of item w / B, and of an item's B workgroups the first lin_blocks(count) -- the single call's launch shape for that count -- do its work while
// the others return before their first barrier.  A second launch, a thread per item, gathers those rows in block order and appends the digest.  Reference
// order: one workgroup of kAlignBlock threads per item.  Nobody waits for another workgroup; the only atomics are the digest's 64-bit wrapping adds.
struct FindItem {
  int32_t fc, mc;        // the item's clouds in the fixed / moving set
  Iso T;                 // local_map_in_sensor
  int32_t nn_group;      // exact NN: lanes per query (kNNGroup when the item's fixed cloud holds >= 4 x its moving cloud's points, else 1)
  int32_t pad;
};
static_assert(sizeof(FindItem) == 32, "the host fills an array of these");

LSM2D_HD int lin_blocks(int n_pairs) { const int b = (n_pairs + 255) / 256; return b < 1 ? 1 : (b > 1024 ? 1024 : b); }      // lsm2d_linearize's launch shape

struct ScoreBatchArgs {
  CloudDev fixed, moving;
  const FindItem* items;      // [n_items]: the finder's own arguments (clouds and T)
  const int32_t* count;       // [n_items]: what the finder wrote
  const int32_t* pairs;       // [n_items][slot][2]: what the finder wrote
  int32_t n_items, slot, blocks_per_item;      // blocks_per_item = lin_blocks(slot)
  int32_t cauchy; float tau;
  uint32_t slice_salt;        // slice * 0x632BE5AB of the pairs' digest (pair_hash_dev): 0 for a lone slice, the aligner's salt when the items are slice `slice` of one (lsm2d_score_aligner_batch)
  float* partial;             // [n_items][blocks_per_item][kAccumWords]
  unsigned long long* dig;    // [n_items], zeroed by the host (tree order only)
  float* out;                 // [n_items][kLinOutWords]
};

LSM2D_DEV int score_count(const ScoreBatchArgs& A, int i) { const int n = A.count[i]; return n < 0 ? 0 : (n > A.slot ? A.slot : n); }

// (item and virtual block are the same in every lane: through readfirstlane they and what is fetched by them stay in scalar registers)
__global__ __launch_bounds__(256) void k_score_partial_batch(const ScoreBatchArgs A) {
  __shared__ float red[4 * kAccumWords];
  __shared__ u64 s_dig;
  const int i = __builtin_amdgcn_readfirstlane((int) (blockIdx.x / (unsigned) A.blocks_per_item));
  const int blk = __builtin_amdgcn_readfirstlane((int) (blockIdx.x % (unsigned) A.blocks_per_item));
  const int n = __builtin_amdgcn_readfirstlane(score_count(A, i));
  const int nblk = lin_blocks(n);
  if (blk >= nblk) return;      // the whole workgroup, before any barrier
  const FindItem it = A.items[i];
  linearize_partial_body(A.fixed, A.moving, it.fc, it.mc, A.pairs + 2 * (size_t) i * (size_t) A.slot, n, it.T, A.cauchy != 0, A.tau, A.slice_salt, blk, nblk,
                         A.partial + (size_t) blockIdx.x * kAccumWords, A.dig + i, red, &s_dig);
}

__global__ __launch_bounds__(256) void k_score_final_batch(const ScoreBatchArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_items) return;
  float* row = A.out + (size_t) i * kLinOutWords;
  linearize_final_body(A.partial + (size_t) i * (size_t) A.blocks_per_item * kAccumWords, lin_blocks(score_count(A, i)), row);
  *reinterpret_cast<unsigned long long*>(row + kAccumWords) = A.dig[i];
}

__global__ __launch_bounds__(kAlignBlock) void k_score_seq_batch(const ScoreBatchArgs A) {
  __shared__ __attribute__((aligned(16))) float s_rec[kSeqHalf * kSeqFields];
  __shared__ float red[(kAlignBlock / 64) * kAccumWords];
  __shared__ u64 s_dig;
  const FindItem it = A.items[blockIdx.x];
  const int n = __builtin_amdgcn_readfirstlane(score_count(A, (int) blockIdx.x));
  float* row = A.out + (size_t) blockIdx.x * kLinOutWords;
  linearize_seq_body(A.fixed, A.moving, it.fc, it.mc, A.pairs + 2 * (size_t) blockIdx.x * (size_t) A.slot, n, it.T, A.cauchy != 0, A.tau, A.slice_salt, row,
                     reinterpret_cast<unsigned long long*>(row + kAccumWords), s_rec, red, &s_dig);
}
