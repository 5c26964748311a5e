// lsm2d_k_align_args.h -- what an aligner launch is handed (SliceDev, AlignArgs) and the small pieces every aligner kernel shares: the bin gates, X_eff = S^-1 X, the odometry prior (MultiAligner2D, registration/aligner_slice_processor_laser_2d.h:7-42).
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d, in this order); not a translation unit of its own.
struct SliceDev {
  CloudDev fixed, moving;
  int32_t finder;
  ProjK   proj;
  float   point_distance, normal_cos, max_distance;
  int32_t nn_group;          // host hint (largest fixed vs largest moving cloud of the sets): 1 = scan-sized fixed clouds, worth staging their tables in LDS
  int32_t cauchy;
  float   tau;
  int32_t min_corr;
  int32_t has_sensor;        // X_eff = S^-1 * X
  float   Sinv[3], cSinv, sSinv;
  int32_t fcan_offset;       // start of this slice's fixed canvas, in cells
  // single-alignment calls whose fixed set still sits in its pinned upload buffer (lsm2d_cloudset_upload defers the unpacking):
  // the kernel's prologue reads the host's AoS points over the bus itself, writes the set's arrays and count (later consumers
  // find them there) and goes on -- no separate k_upload_unpack launch in front of the alignment
  const float4* unpack_src;  // device view of the pinned AoS points, or nullptr
  int32_t unpack_n;
};

struct PriorDev { float z_inv[3], cz, sz, omega[9]; };   // Z^-1 and cos/sin of its angle, host-computed
struct StatsDev { int32_t n_corr, n_in, n_out; float chi_in, chi_out; uint32_t dig_lo, dig_hi; };

// lsm2d_pair_hash (include/lsm2d.h) on the device: the per-pair term of lsm2d_iteration_stats.pair_digest.  slice_salt = slice * 0x632BE5AB
// (wave-uniform).  Integer arithmetic only; tests hold the two definitions against each other through the oracle's digest.
LSM2D_DEV u64 pair_hash_dev(uint32_t slice_salt, uint32_t f, uint32_t m) {
  const uint32_t a = f * 0x9E3779B1u, b = (m ^ slice_salt) * 0x85EBCA77u;
  uint32_t lo = a ^ __builtin_rotateleft32(b, 13), hi = b ^ __builtin_rotateleft32(a, 19);
  lo += __builtin_rotateleft32(lo, 17) ^ b;
  hi += __builtin_rotateleft32(hi, 11) ^ a;
  return ((u64) hi << 32) | (u64) lo;
}
// one pair into the iteration's digest: a fire-and-forget 64-bit LDS add (order-independent: the sum wraps mod 2^64), no register held across the loops
LSM2D_DEV void digest_add(u64* s_dig, uint32_t slice_salt, int f, int m) { atomicAdd(reinterpret_cast<unsigned long long*>(s_dig), (unsigned long long) pair_hash_dev(slice_salt, (uint32_t) f, (uint32_t) m)); }

struct AlignArgs {
  int32_t n_align, n_slices, max_it, min_inliers;
  float   damping;
  float   term_eps;                         // lsm2d_aligner_params.termination_chi_epsilon (0 = run all iterations)
  int32_t inlier_runs;                      // lsm2d_aligner_params.enable_inlier_only_runs: a second loop of up to max_it iterations over inliers only (lsm2d.h)
  int32_t stats_stride;                     // iterations an alignment may run = row length of out_stats: max_it * (1 + inlier_runs), at least 1
  float*  out_last_pose;                    // [n][3] or nullptr: the pose the LAST started iteration began at (lsm2d_align_batch_pairs re-derives that iteration's pairs from it)
  int32_t cols_max, fcan_total;
  int32_t nn_lds_points, nn_lds_cells;      // > 0: single NN slice over scan-sized fixed clouds -- their search tables are staged in LDS (room for this many)
  int32_t nn_qcache;                        // > 0: single NN slice with its tables in global memory (kNNGlobal): room in LDS for this many queries' cached cell ranges (32 bytes each)
  int32_t kd_lds_nodes;                     // > 0: single KD-tree slice -- room in LDS for this many nodes of the fixed cloud's tree (its top levels)
  int32_t kd_lds_points;                    // > 0: ... and, for scan-sized fixed clouds, for this many leaf points (whole trees on chip)
  const int32_t* order;                     // alignment handled by workgroup b (nullptr: b itself) -- the balanced placement of k_balance_order
  float cull_est_mt, cull_est_mth;          // margins of k_cull_estimate's chunk test (metres, radians)
  float cull_mt2;                           // cull_mt squared (host)
  int32_t* wg_place;                        // [grid] or nullptr: every workgroup notes the CU it ran on (place_key) for the next call's placement
  int32_t cull;                             // 1: projective slices drop the chunks of the moving cloud that cannot yield a pair (chunk_may_matter), results unchanged
  // kProjCulled (round 4): every slice keeps a LIST of the (block, chunk) units that survive the test at block level, in dynamic LDS at units_off
  // (kCullBlocks * kAlignBlock 16-bit entries per slice), built with margins (cull_mt metres, cull_mth radians) and kept while the slice's transform
  // stays within them of the one it was built at (cull_keep 0: rebuilt every iteration, zero margins -- A/B knob)
  int32_t units_off, cull_keep;
  int32_t units_stride;                     // entries per slice of the unit lists: the largest block_stride of the batch's moving sets x kAlignBlock
  float   cull_mt, cull_mth;
  int32_t pq_cull_off;                      // > 0: byte offset in dynamic LDS of the point-query finders' culling state (occupancy bitmap of the fixed cloud, then
  int32_t pq_keep_words;                    //   pq_keep_words 64-bit words of per-tile keep bits); single-slice NN / KD-tree batches with scan-sized fixed clouds
  int32_t pair_mov_cap;                     // latency kernel: moving points per slice it may keep in LDS (kPairMovCap, or 0: no room)
  int32_t pair_fix_cap;                     // latency kernel: fixed points per slice it may keep in LDS (0: no room)
  const float* init_pose;
  const PriorDev* prior;
  int32_t  host_polls;                      // results go to pinned host memory and the host polls the status words: release them to the system
  int32_t  inline_n1;                       // 1: a single alignment whose start pose / prior travel in the kernel arguments (pose1, prior1)
  float    pose1[3];
  PriorDev prior1;
  float* out_pose; float* out_H; int32_t* out_status; int32_t* out_its; StatsDev* out_stats;
  // kernel timing on (lsm2d_set_option "kernel_timing"): thread 0 of every clock_stride-th workgroup stamps s_memtime (shader
  // cycles) and s_memrealtime (100 MHz) once at its start and once at its end -- [a / clock_stride][4] = {cycles, 10 ns ticks, start tick, hardware id} of
  // the workgroup's lifetime, from which the host reads the clock the chip held under THIS load (MI355X_MICROARCH.md, DVFS note 6)
  unsigned long long* clock_out; int32_t clock_stride;
  // "sum_order" 1 (the k_align_seq / k_split_finish<true> instantiations): byte offset in dynamic LDS of the trip's pair records, kAlignBlock x kSeqFields floats
  // (lsm2d_device.h, "sum_order"); sits in what was padding, so the other fields keep their offsets
  int32_t seq_off;
  const int32_t* order2;                    // (round 6, k_align_two) a SECOND alignment for workgroup b to run after its first (-1: none), or nullptr: a batch of a few alignments more than
                                            // the chip holds packs its lightest ones two to a workgroup instead of starting another dispatch round (balance_order, "packed")
  // "fast_forward" (align_body): an iteration is a pure function of the pose it starts at, so once the pose after an iteration equals, bit for bit, the
  // start pose of one of the last kFfRing iterations, the rest of the phase is that cycle again and again.  1: whole periods of it are skipped and the
  // remainder runs; 2: the alignment finishes at once, from what the twin of its last iteration left -- poses in the ring (LDS), H and inlier count in ff_rows;
  // results unchanged (0: every iteration runs; A/B switch.  Ignored with term_eps > 0, inlier_runs and host_polls)
  uint32_t* ff_rows;                        // [n_align][kFfRing][kFfRowWords] device scratch, written and read by the alignment's thread 0 only; nullptr unless fast_forward == 2
  int32_t fast_forward;
  SliceDev s[kMaxSlices];
  // kProjCulled, round 20: the candidate list of a single-slice batch (lsm2d_device.h, "candidate lists").  cand_off > 0: byte offset in dynamic LDS of a word per
  // column (its blocker's depth: cand_blocker_words) and behind them cand_cap 32-bit point indices -- given only where both fit behind the unit
  // lists without changing the launch form or the workgroups a CU holds; 0: no lists.  cand_mt / cand_mth: the margins a list serves (metres, radians); cand_first_it: the first iteration that may build
  // one; cand_max_builds: lists per alignment.  cand_out [n_align] or nullptr: every alignment's books (align_body's s_cand_stat), summed by the host
  int32_t cand_off, cand_cap, cand_first_it, cand_max_builds;
  float   cand_mt, cand_mth;
  int32_t* cand_out;                        // (behind everything else: the kernels without lists read every older field at the offset it always had)
  // Round 30, the queue of maybes (lsm2d_device_cand.h): cand_qcap entries of room per alignment, region a at cand_queue + a * cand_qcap (32-bit point indices, device
  // memory the host keeps per lane, for batches with lists only); cand_qcap < 0: "cand_queue" 0.  With the queue, cand_out has a second word per alignment, at
  // [n_align + a]: the builds that outgrew the room and made their list from the unit list.  Behind cand_out, for the reason given there
  uint32_t* cand_queue; int32_t cand_qcap;
};

LSM2D_DEV int pick_cloud(const CloudDev& c, int a) {
  return c.index ? c.index[a] : (c.n_clouds == 1 ? 0 : a);
}

// bin walk of one column: gates of correspondence_finder_projective_2d.cpp:61-69
LSM2D_DEV bool match_bin(u64 fk, u64 mk, const SliceDev& S, const Iso& T, const float2* fn, const float2* mn,
                         int& fi, int& mi, float2& nf, float2& nm) {
  if (mk == kEmptyCell || fk == kEmptyCell) return false;
  const float fd = __uint_as_float((uint32_t) (fk >> 32)), md = __uint_as_float((uint32_t) (mk >> 32));
  if (__builtin_fabsf(fd - md) > S.point_distance) return false;
  fi = (int) (uint32_t) fk; mi = (int) (uint32_t) mk;
  nf = fn[fi]; nm = mn[mi];
  float nqx, nqy;
  xf_normal(T, nm.x, nm.y, nqx, nqy);
  const float dot = __builtin_fmaf(nqx, nf.x, nqy * nf.y);
  return !(dot < S.normal_cos);
}

LSM2D_DEV Iso slice_iso_of(int has_sensor, float cSinv, float sSinv, const float Sinv[3], const float pose[3]) {
  float Xe[3] = {pose[0], pose[1], pose[2]};
  if (has_sensor) compose(cSinv, sSinv, Sinv, pose, Xe);
  Iso T; sincos_fixed(Xe[2], T.s, T.c); T.tx = Xe[0]; T.ty = Xe[1];
  return T;
}
LSM2D_DEV Iso slice_iso(const SliceDev& S, const float pose[3]) {      // X_eff = S^-1 X (AlignerSliceProcessorLaser2DWithSensor) as rotation + translation
  return slice_iso_of(S.has_sensor, S.cSinv, S.sSinv, S.Sinv, pose);
}
// prologue of the single-alignment kernels: unpack the slices' freshly uploaded fixed sets (see SliceDev::unpack_src)
LSM2D_DEV void unpack_fixed_set(const SliceDev& S, int tid, int nthreads) {
  float2* xy = const_cast<float2*>(S.fixed.xy); float2* nrm = const_cast<float2*>(S.fixed.nrm);
  for (int i = tid; i < S.unpack_n; i += nthreads) {
    const float4 v = S.unpack_src[i];
    xy[i] = make_float2(v.x, v.y); nrm[i] = make_float2(v.z, v.w);
  }
  if (tid == 0) *const_cast<int32_t*>(S.fixed.count) = S.unpack_n;
}
#ifndef LSM2D_ALIGN_MIN_WAVES
#define LSM2D_ALIGN_MIN_WAVES 8      // waves per SIMD the register allocator must leave room for (tools/variant_bench.sh builds with other values; the other kernels' budgets: lsm2d_k_align_kernels.h)
#endif
// SE2 odometry prior (AlignerSliceOdom2DPrior, MULTI.json:402-422): e = t2v(Z^-1 X), J = blkdiag(R_e, 1) for the right perturbation;
// adds J^T Omega J to H and J^T Omega e to b.  One definition for k_align and the split path: the same operation order in both.
// prior_terms: the nine and three values that go into H and b -- they do not depend on H or b, so whoever has the pose can have them ready
// (the latency kernel's thread 0 computes them while it would otherwise wait at the barrier for the slowest wave)
// (kAdd: the terms are added to H and b as they come -- the form k_align's out-of-line call takes: twelve registers fewer)
template <bool kAdd>
LSM2D_DEV void prior_apply(const PriorDev& Pz, const float pose[3], float Hp[9], float bp[3]) {
  float E[3]; compose(Pz.cz, Pz.sz, Pz.z_inv, pose, E);
  float c, s_; sincos_fixed(E[2], s_, c);
  const float Jp[9] = {c, -s_, 0.0f, s_, c, 0.0f, 0.0f, 0.0f, 1.0f};
  float OJ[9], Oe[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Oe[r] = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) Oe[r] += Pz.omega[3 * r + k] * E[k];
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      OJ[3 * r + cc] = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) OJ[3 * r + cc] += Pz.omega[3 * r + k] * Jp[3 * k + cc];
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      float v = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; ++k) v += Jp[3 * k + r] * OJ[3 * k + cc];
      if (kAdd) Hp[3 * r + cc] += v; else Hp[3 * r + cc] = v;
    }
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) v += Jp[3 * k + r] * Oe[k];
    if (kAdd) bp[r] += v; else bp[r] = v;
  }
}
LSM2D_DEV void prior_terms(const PriorDev& Pz, const float pose[3], float Hp[9], float bp[3]) { prior_apply<false>(Pz, pose, Hp, bp); }
LSM2D_DEV void add_prior_inline(const PriorDev& Pz, const float pose[3], float H[9], float b[3]) { prior_apply<true>(Pz, pose, H, b); }
// ONE entry of the odometry prior's J^T Omega [J | e] (prior_apply's operations for that entry, in its order): row r in 0..2, column c in
// 0..2 of the H term, c == 3 the b term.  J = [[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]].
LSM2D_DEV float prior_term_lane(const PriorDev& Pz, const float pose[3], int r, int c) {
  float E[3]; compose(Pz.cz, Pz.sz, Pz.z_inv, pose, E);
  float cs, sn; sincos_fixed(E[2], sn, cs);
  const float msn = -sn;
  const float x0 = c == 0 ? cs : (c == 1 ? msn : (c == 2 ? 0.0f : E[0]));
  const float x1 = c == 0 ? sn : (c == 1 ? cs : (c == 2 ? 0.0f : E[1]));
  const float x2 = c == 2 ? 1.0f : (c == 3 ? E[2] : 0.0f);
  const float j0 = r == 0 ? cs : (r == 1 ? msn : 0.0f);
  const float j1 = r == 0 ? sn : (r == 1 ? cs : 0.0f);
  const float j2 = r == 2 ? 1.0f : 0.0f;
  float oj[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { float v = 0.0f; v += Pz.omega[3 * k + 0] * x0; v += Pz.omega[3 * k + 1] * x1; v += Pz.omega[3 * k + 2] * x2; oj[k] = v; }
  float v = 0.0f; v += j0 * oj[0]; v += j1 * oj[1]; v += j2 * oj[2];
  return v;
}
// k_align's wave 0 calls it (one entry per lane), out of line like add_prior below: its temporaries stay out of the register allocation of the kernel's loops
__device__ __noinline__ float prior_term_lane_call(const PriorDev& Pz, float px, float py, float pth, int r, int c) { const float pose[3] = {px, py, pth}; return prior_term_lane(Pz, pose, r, c); }
// k_align (64 VGPRs) and the split path call it: rarely taken, and out of the register allocation of their loops
__device__ __noinline__ void add_prior(const PriorDev& Pz, const float pose[3], float H[9], float b[3]) { add_prior_inline(Pz, pose, H, b); }

// kHasProj / kHasNN: which finders the batch's slices use -- the unused one is compiled out so the
// projective hot loop does not carry the NN path's register pressure (and vice versa).
// kHasDist: a slice uses the distance-map finder (compiled out otherwise so the NN search keeps its registers).
// kHasKd: a slice uses the KD-tree finder (LSM2D_FINDER_KDTREE); compiled out otherwise.
// kNNGlobal: a pure grid-NN batch whose search tables stay in global memory (the map is the fixed cloud: BASELINE's wording with the exact search) --
// an instantiation of its own, so that its position-keeping search (nn_query_pos) does not share 64 registers with the LDS-table path of the
// tracker's wiring (both forms in one kernel: scratch 16 -> 80 bytes, role A 7.2 -> 10.6 ms)
// kNNMode 2: the counterpart -- a pure grid-NN batch whose tables the host has PROVED to fit the LDS staging for every alignment (nn_lds_points is the
// largest fixed cloud, nn_lds_cells the grid ensure_grid() gives that size): the search in global memory and the cooperative loop are compiled out
// where a workgroup runs: the key the balanced placement groups workgroup ids by (see k_balance_order)
static constexpr int kPlaceKeys = 4096;      // XCC (4 bits) | SE (3) | SH (1) | CU (4)
LSM2D_DEV int place_key() {
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20);      // HW_REG_HW_ID, HW_REG_XCC_ID
  return (int) (((xcc & 15u) << 8) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u));
}
