// lsm2d_k_align.h -- k_align: one workgroup owns one alignment for all its iterations -- the moving cloud streamed through the LDS z-buffer, the bin walk, the point-query passes, the reduction, the 3x3 solve as a vector over wave 0 (MultiAligner2D::compute; registration/correspondence_finder_projective_2d.cpp:35-74; octave/solver/nicp_post.m:69-97); k_align_seq: the same with the reference's order of summation.
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d, in this order); not a translation unit of its own.  This file is align_body, the one device function all of them share;
// the __global__ kernels that instantiate it are in lsm2d_k_align_kernels.h, its phase-probe macros in lsm2d_k_align_probe.h.
// kSeq: "sum_order" 1 -- H, b and the chi^2 statistics are added pair after pair in the reference's order (lsm2d_device.h: pair_terms / seq_walk) instead of
// in trees; instantiations of their own (k_align_seq), so the default kernels do not carry the records' code
// kW: threads of the workgroup (round 6).  512 = kAlignBlock everywhere but in the NARROW instantiation of the culled projective stream (k_align_narrow<256>):
// four waves per workgroup, one per SIMD, so six workgroups fit a CU (the canvases' LDS bounds it: 1536 resident alignments instead of 1024) -- for batches just
// above a multiple of 1024, whose last alignments would otherwise run a second, nearly empty dispatch round (tools/batch_size_sweep.py: 1100 .. 1536 alignments
// lost 17-25 % per alignment).  The z-buffer does not care who streams which point; the bin walk and the sums keep the 512 VIRTUAL threads of the wide kernel --
// thread t plays virtual threads t, t + kW, ... one after the other, each with its own partial sums, its waves' trees written to the same eight rows of `red` --
// so every result keeps its bits (tests: 256 against 512).
// kCandLists: the instantiation carries the candidate lists of round 20 (lsm2d_device.h) -- k_align_cand, the wide culled projective kernel, alone: with their code the
// narrow, the packed and the reference-order forms, which share this body, needed private memory (16 .. 32 bytes of scratch; the packed ones a copy of the
// arguments), and in the shapes those forms are chosen for the lists' room in LDS runs out anyway; and inside k_align<1,0,0,0,5> it
// would change the kernel of every batch that gets no list.  The host gives a list an offset only to a batch it launches as k_align_cand.
template <bool kHasProj, bool kHasNN, bool kHasDist, bool kHasKd = false, int kNNMode = 0, bool kSeq = false, int kW = kAlignBlock, bool kCandLists = false>
LSM2D_DEV void align_body(const AlignArgs& A, int a_given = -1) {
  static_assert(kW == kAlignBlock || (kNNMode == 5 && !kSeq && kW % 64 == 0 && kW >= 256 && kW < kAlignBlock), "narrow workgroups: the culled projective stream only");
  __builtin_assume(A.n_slices >= 1 && A.n_slices <= kMaxSlices);      // (the host refuses anything else: the slice loops need no guard -- which, as a flag, was kept in a vector register and spilled)
  constexpr bool kNNGlobal = kNNMode == 1, kNNLds = kNNMode == 2;
  // the same for a pure KD-tree batch: 3 = every alignment's whole tree, leaf arrays included, is in LDS (the tracker's wiring: a tree per scan); 4 = only the
  // top of the tree is (the map is the fixed cloud): the other form of the descent and of the leaf scan is compiled out
  constexpr bool kKdAllLds = kNNMode == 3, kKdTop = kNNMode == 4;
  // ... and for a pure projective batch: 5 = every slice streams a lane-chunked moving cloud through the exact culling in units (what a batch against a map
  // does): the plain lane stream and the per-pair stream of small clouds are compiled out
  constexpr bool kProjCulled = kNNMode == 5;
  constexpr bool kCand = kCandLists && kProjCulled && !kSeq && kW == kAlignBlock;
  static_assert(kNNMode == 0 || ((kNNMode <= 2) && kHasNN && !kHasProj && !kHasDist && !kHasKd) || ((kNNMode == 3 || kNNMode == 4) && kHasKd && !kHasProj && !kHasDist && !kHasNN) ||
                (kNNMode == 5 && kHasProj && !kHasNN && !kHasDist && !kHasKd), "kNNMode: one finder only");
  extern __shared__ __align__(16) unsigned char smem[];
  // (round 4: the fixed winners' payload no longer sits in LDS -- 16 bytes per column, 17 KB at 1081 -- the bin walk gathers it like the moving winner's,
  // one 16-byte row of the cloud's AoS copy each, both in flight together; the room holds the culled stream's unit lists)
  u64* mcan = reinterpret_cast<u64*>(smem);
  u64* fcan = mcan + A.cols_max;
  float* red = reinterpret_cast<float*>(fcan + A.fcan_total + ((A.cols_max + A.fcan_total) & 1));     // [nwaves][kAccumWords], 16-byte aligned
  // NN finder over a scan-sized fixed cloud (the tracker wiring: tree over the scan, every map point a query): the cloud's search
  // tables live in LDS for the whole alignment -- 20 iterations x N_m queries then touch global memory only for the query stream
  float2* l_sxy = reinterpret_cast<float2*>(red + (kAlignBlock / 64) * kAccumWords);
  int* l_qc = reinterpret_cast<int*>(red + (kAlignBlock / 64) * kAccumWords);      // kNNGlobal: [nn_qcache][8] cached cell ranges per query (16-byte aligned: the host pads)
  uint16_t* l_cst = reinterpret_cast<uint16_t*>(l_sxy + A.nn_lds_points);
  uint16_t* l_sidx = l_cst + ((A.nn_lds_cells + 2) & ~1);
  // KD-tree finder: the top levels of the fixed cloud's tree (its first kd_lds_nodes nodes) live in LDS for the whole alignment -- every
  // descent starts there (the host offers this only to pure KD-tree batches, where the region behind `red` is 16-byte aligned and free)
  float4* l_kpl = reinterpret_cast<float4*>(red + (kAlignBlock / 64) * kAccumWords);
  int2* l_klk = reinterpret_cast<int2*>(l_kpl + A.kd_lds_nodes);
  float2* l_kxy = reinterpret_cast<float2*>(l_klk + A.kd_lds_nodes + (A.kd_lds_nodes & 1));      // 16-byte aligned: pairs of points are read as one
  float2* l_knr = l_kxy + A.kd_lds_points + (A.kd_lds_points & 1);
  __shared__ float s_pose[3];
  __shared__ Iso   s_iso[kMaxSlices];
  // s_H: information matrix (H of the last solved iteration, prior included), stored by the nine lanes of wave 0 that hold its entries;
  // s_sum: this iteration's sums in the order of Accum (h00 h01 h02 h11 h12 h22 b0 b1 b2 chi_in chi_out | n_in n_out as integers), then the pairs of
  // all slices and the number of active slices (integers: kSumPairs, kSumActive), each added by the lane of wave 0 that gathered it
  __shared__ float s_H[9], s_sum[kAccumWords + 2];
  constexpr int kSumPairs = 13, kSumActive = 14, kSumWords = 15;
  static_assert(kSumWords <= kAccumWords + 2 && kAccumWords + 2 == 16, "s_sum: one word per lane of a row of sixteen");
  __shared__ int   s_done, s_status, s_last_n_in;
  __shared__ float s_prev_chi;      // total chi^2 of the previous iteration (termination_chi_epsilon)
  __shared__ u64 s_dig;             // this iteration's pair digest (lsm2d_iteration_stats.pair_digest): every matched pair adds its hash; only when statistics go out
  __shared__ int s_it0;            // the iteration this launch starts at (always 0 now; kept so that the kernels' LDS layout and code stay as they were)
  __shared__ int s_phase, s_phase_start, s_phase_end;      // 0: the regular loop, 1: the inlier-only runs (enable_inlier_only_runs); iterations [start, end) belong to the phase
  __shared__ uint16_t s_surv[kAlignBlock];      // culling: the chunks of the moving cloud that survived this iteration's test, compacted in thread order
  __shared__ int s_wcnt[2 * (kAlignBlock / 64)];
  __shared__ int s_nunits[kMaxSlices], s_rebuild[kMaxSlices];      // kProjCulled: entries in a slice's unit list; the list must be rebuilt before it is streamed again
  __shared__ Iso s_list_iso[kMaxSlices];                             // ... and the transform it was built at
  // kProjCulled, round 20: the slice's CANDIDATE list (lsm2d_device.h, "candidate lists"; AlignArgs::cand_off > 0: a single slice, and room in LDS).  The transform
  // it was built at; its entries (counted by the build's waves, past the capacity if they must); what the coming iteration does about it -- 0: streams the
  // unit list, 1: gathers the list's points instead, 2: streams the unit list and builds a list behind it; and what happened so far: iterations served by a
  // list (bits 0..15, saturating), lists built (16..23), of which too long to be used (24..31).  Wave 0's, like s_rebuild: no register is held across the loops.
  __shared__ Iso s_cand_iso;
  __shared__ int s_cand_n, s_cand_state, s_cand_stat;
  // ... and the launch's arguments for it, read back from here by whoever needs them: as kernel arguments they were loop invariants, scalar registers held -- and
  // spilled into vector registers -- across the loops.  Words: offset (0: no lists), capacity, first iteration, lists per alignment | margins (floats) | the room
  // of the queue of maybes in entries (-1: "cand_queue" 0, the collect pass over the unit list)
  __shared__ int s_cand_par[7];
  // Round 30, the queue of maybes (lsm2d_device_cand.h): this alignment's region of AlignArgs::cand_queue, the maybes the build's stream counted (past the room if
  // it must: the build then falls back to the pass over the unit list), and the builds that fell back -- thread 0's, handed over with the books
  __shared__ uint32_t* s_cand_q;
  __shared__ int s_cand_qn, s_cand_fb;
  uint16_t* l_units = reinterpret_cast<uint16_t*>(smem + A.units_off);      // [n_slices][kCullBlocks * kAlignBlock]
  float* l_rec = reinterpret_cast<float*>(smem + (kSeq ? A.seq_off : 0));   // kSeq: [kSeqHalf][kSeqFields]: half a trip's pair records
  // "fast_forward" (AlignArgs::fast_forward): the poses the last kFfRing iterations STARTED at, as bit patterns, in a ring (slot = pushes & (kFfRing - 1)); how
  // many were pushed; the iterations wave 0 found it may skip behind the current one (0: none), read by everybody after the iteration's closing barrier.  In
  // LDS like the rest of wave 0's serial state: no register held across the loops.  (What else "fast_forward" 2 keeps of those iterations -- H and the
  // inlier count -- lies in device memory: AlignArgs::ff_rows)
  __shared__ uint32_t s_ring[3 * kFfRing];
  __shared__ int s_ring_n, s_skip;
  __shared__ uint32_t* s_ff_rows;      // this alignment's row of A.ff_rows, or nullptr ("fast_forward" 2 only: the host hands the rows over for that value alone).  Wave 0 reads it back with the rest of its state: as a kernel argument and a product with `a` it was four scalar registers held across the loops -- in the narrow kernel, spills
  __shared__ PriorDev s_prior;      // read once: with zero-copy arguments A.prior is host memory, a PCIe round trip per access

  // (the alignment's index is wave-uniform: said so, or everything indexed by it would live in vector registers)
  const int a = a_given >= 0 ? a_given : (A.order ? __builtin_amdgcn_readfirstlane(A.order[blockIdx.x]) : (int) blockIdx.x), tid = threadIdx.x;
  constexpr int nwaves = kW / 64;      // physical waves (the rows of `red` stay kAlignBlock / 64: one per VIRTUAL wave)
  constexpr int kPriorWords = (int) (sizeof(PriorDev) / sizeof(float));
  __shared__ unsigned long long s_clk[2];      // start stamps wait in LDS: no register is held across the kernel for them
#ifdef LSM2D_PHASE_PROBE      // diagnostics build: thread 0 sums the cycles it spends in the query / projection phase, at the barrier + reduction, and in the solve (the LSM2D_PH* macros: lsm2d_k_align_probe.h)
  __shared__ unsigned long long s_ph[4];
  if (tid == 0) { s_ph[0] = s_ph[1] = s_ph[2] = 0; s_ph[3] = __builtin_amdgcn_s_memtime(); }
#endif
  if (A.wg_place && tid == 0) A.wg_place[blockIdx.x] = place_key();
  const bool stamp = A.clock_out && tid == 0 && a % A.clock_stride == 0;
  if (stamp) { s_clk[0] = __builtin_amdgcn_s_memtime(); s_clk[1] = __builtin_amdgcn_s_memrealtime(); }
  if (A.prior && tid >= 64 && tid < 64 + kPriorWords)
    ((float*) &s_prior)[tid - 64] = A.inline_n1 ? ((const float*) &A.prior1)[tid - 64] : ((const float*) (A.prior + a))[tid - 64];

  // ---- point-query finders, tracker wiring (a scan-sized fixed cloud, every point of a big moving cloud a query): EXACT culling of the queries.
  // A pair needs a fixed point within max_distance of the transformed moving point (the grid search's gate d2 <= md2, the tree's d2 < md2, the
  // distance map's parent pixel within max_distance of the query's pixel), so a TILE of 64 consecutive moving points -- what one wave handles in
  // one trip of the query loop -- can be skipped when no fixed point lies within rho + max_distance of its bounding circle's centre
  // (k_tile_bounds: centre, rho).  The fixed cloud is rasterised ONCE per alignment into a 128 x 128 occupancy bitmap (cell side g: its extent
  // / 125, at least a sixth of the reach); the test looks at the (2k + 1)^2 cells around the centre's, k = floor(reach / g) + 1: if they are
  // clear, every fixed point is more than `reach` away.  The queries keep their threads and a skipped query could not have paired: every sum
  // keeps its bits.  (Measured on configs[1], role A: 49 % of the tiles survive where an exact distance test would keep 32 %.)
  constexpr int kPqRowWords = 5, kPqOccWords = 128 * kPqRowWords;      // rows of 128 bits and one word that stays zero: a row's window is read as two words
  __shared__ unsigned s_pqbb[4];      // the fixed cloud's bounding box as order-preserving integers: min x, min y, max x, max y
  __shared__ float s_pq[4];           // bitmap origin x, y, 1 / g, the reach beyond a tile's own radius (< 0: culling off for this alignment)
  const bool pq_on = (kHasNN || kHasKd || kHasDist) && A.pq_cull_off > 0;
  uint32_t* l_occ = reinterpret_cast<uint32_t*>(smem + (pq_on ? A.pq_cull_off : 0));
  u64* l_keep = reinterpret_cast<u64*>(l_occ + kPqOccWords);
  auto ordered = [](float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
  auto unordered = [](unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); };
  if (pq_on) {
    for (int i = tid; i < kPqOccWords; i += kAlignBlock) l_occ[i] = 0u;
    if (tid < 4) s_pqbb[tid] = tid < 2 ? 0xFFFFFFFFu : 0u;
  }

  if (kHasProj && !kHasNN && !kHasDist && !kHasKd && A.inline_n1)
    for (int s = 0; s < A.n_slices; ++s) if (A.s[s].unpack_src) unpack_fixed_set(A.s[s], tid, kW);      // visible after the barrier below
  // ---- prologue: fixed canvases, camera at identity (correspondence_finder_projective_2d.cpp:37-44)
  for (int i = tid; i < A.fcan_total; i += kW) fcan[i] = kEmptyCell;
  for (int i = tid; i < A.cols_max; i += kW) mcan[i] = kEmptyCell;      // afterwards the bin walk resets what it reads
  // per-iteration set-up by lane 0: X_eff = S^-1 X per slice (AlignerSliceProcessorLaser2DWithSensor), cos/sin once per
  // slice, zeroed sums.  Done here for iteration 0; at the end of every solve wave 0 does the same for the next one, a slice per lane (no extra barrier).
  auto begin_iteration = [&]() {
    for (int s = 0; s < A.n_slices; ++s) {
      float Xe[3] = {s_pose[0], s_pose[1], s_pose[2]};
      if (A.s[s].has_sensor) compose(A.s[s].cSinv, A.s[s].sSinv, A.s[s].Sinv, s_pose, Xe);
      sincos_fixed(Xe[2], s_iso[s].s, s_iso[s].c); s_iso[s].tx = Xe[0]; s_iso[s].ty = Xe[1];
    }
    // (the zero is made HERE, every time: a constant the compiler may hoist becomes a zero quad that every thread keeps -- and spills --
    // across the whole kernel for thread 0's sake)
    float zf = 0.0f; int zi = 0;
    asm volatile("" : "+v"(zf), "+v"(zi));
    for (int k = 0; k < 11; ++k) s_sum[k] = zf;
    for (int k = 11; k < kSumWords; ++k) s_sum[k] = __int_as_float(zi);
    s_dig = (u64) (unsigned) zi;
    if (kProjCulled) for (int s = 0; s < A.n_slices; ++s) {
      // has the slice's transform left the neighbourhood its unit list serves?  Seen from the sensor the change is a rotation by dth about the origin
      // and a translation d = t - R(dth) t0 (chunk_may_matter): the list holds while |d| <= cull_mt and |dth| <= cull_mth
      const Iso N = s_iso[s], L = s_list_iso[s];
      const float cd = N.c * L.c + N.s * L.s, sd = N.s * L.c - N.c * L.s;
      const float dx = N.tx - (cd * L.tx - sd * L.ty), dy = N.ty - (sd * L.tx + cd * L.ty);
      s_rebuild[s] = (A.cull_keep && cd > 0.5f && __builtin_fabsf(sd) <= A.cull_mth && dx * dx + dy * dy <= A.cull_mt2) ? zi : 1;      // (the square comes with the arguments: formed here it was a
      // loop invariant in a vector register, kept -- and spilled -- across the whole iteration for thread 0's sake)
    }
    if (A.out_last_pose) { A.out_last_pose[3 * a + 0] = s_pose[0]; A.out_last_pose[3 * a + 1] = s_pose[1]; A.out_last_pose[3 * a + 2] = s_pose[2]; }
  };
  if (tid == 0) {
    if (A.inline_n1) { s_pose[0] = A.pose1[0]; s_pose[1] = A.pose1[1]; s_pose[2] = A.pose1[2]; }
    else { s_pose[0] = A.init_pose[3 * a + 0]; s_pose[1] = A.init_pose[3 * a + 1]; s_pose[2] = A.init_pose[3 * a + 2]; }
    s_done = 0; s_status = LSM2D_RUNNING; s_last_n_in = 0;
    s_phase = 0; s_phase_start = 0; s_phase_end = A.max_it; s_it0 = 0;
    for (int k = 0; k < 9; ++k) s_H[k] = 0.0f;
    s_ring_n = 0; s_skip = 0;
    s_ff_rows = A.ff_rows ? A.ff_rows + (size_t) a * (kFfRing * kFfRowWords) : nullptr;
    for (int s = 0; s < kMaxSlices; ++s) { s_list_iso[s].c = 1.0f; s_list_iso[s].s = 0.0f; s_list_iso[s].tx = 0.0f; s_list_iso[s].ty = 0.0f; }
    if (!s_done) begin_iteration();
    for (int s = 0; s < kMaxSlices; ++s) s_rebuild[s] = 1;      // no list yet
    if (kCand) {
    s_cand_n = 0; s_cand_state = 0; s_cand_stat = 0;
    s_cand_qn = 0; s_cand_fb = 0; s_cand_par[6] = A.cand_qcap;
    s_cand_q = A.cand_queue ? A.cand_queue + (size_t) a * (size_t) (A.cand_qcap > 0 ? A.cand_qcap : 0) : nullptr;
    s_cand_par[0] = A.cand_off; s_cand_par[1] = A.cand_cap; s_cand_par[2] = A.cand_first_it; s_cand_par[3] = A.cand_max_builds;
    s_cand_par[4] = __float_as_int(A.cand_mt); s_cand_par[5] = __float_as_int(A.cand_mth);
    }
  }
  __syncthreads();
  if (kNNGlobal) for (int i = tid; i < A.nn_qcache; i += kAlignBlock) l_qc[8 * i] = 0x7fffffff;      // no cell cached yet (visible after the barriers below)
  bool nn_lds = false;
  if (kHasNN && !kNNGlobal && A.nn_lds_points > 0) {
    const SliceDev& S = A.s[0];
    const int fc = pick_cloud(S.fixed, a), nf = S.fixed.count[fc];
    const GridMeta g0 = S.fixed.grid.meta[fc];
    const int ncell = g0.gw * g0.gh;
    nn_lds = nf <= A.nn_lds_points && ncell + 1 <= A.nn_lds_cells;     // workgroup-uniform; else this alignment searches in global memory
    if (nn_lds) {
      const int32_t* cst = S.fixed.grid.cell_start + g0.cell_base;
      const int fbase = S.fixed.start[fc];
      for (int i = tid; i <= ncell; i += kAlignBlock) l_cst[i] = (uint16_t) cst[i];
      for (int i = tid; i < nf; i += kAlignBlock) { l_sxy[i] = S.fixed.grid.sorted_xy[fbase + i]; l_sidx[i] = (uint16_t) S.fixed.grid.sorted_idx[fbase + i]; }
    }
  }
  if (kNNLds && !nn_lds) {      // cannot happen (the host sized the staging for the set's largest cloud): refuse loudly rather than search tables that are not there
    if (tid == 0) {
      A.out_pose[3 * a + 0] = s_pose[0]; A.out_pose[3 * a + 1] = s_pose[1]; A.out_pose[3 * a + 2] = s_pose[2];
      if (A.out_H) for (int k = 0; k < 9; ++k) A.out_H[9 * a + k] = 0.0f;      // (no iteration ran: the information matrix is the zero the regular path would hand back)
      if (A.out_its) A.out_its[a] = 0;
      if (A.host_polls) { __threadfence_system(); __hip_atomic_store(&A.out_status[a], (int) LSM2D_CAPACITY_EXCEEDED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
      else A.out_status[a] = LSM2D_CAPACITY_EXCEEDED;
    }
    return;
  }
  int kd_lds = 0;                            // nodes of this alignment's tree that were staged (workgroup-uniform)
  bool kd_leaves_lds = false;                // ... and its leaf arrays
  if (kHasKd && A.kd_lds_nodes > 0) {
    const SliceDev& S = A.s[0];
    const KdMeta km = S.fixed.kd.meta[pick_cloud(S.fixed, a)];
    kd_lds = km.n_nodes < A.kd_lds_nodes ? km.n_nodes : A.kd_lds_nodes;
    const KdNode* nd = S.fixed.kd.nodes + km.node_base;
    for (int i = tid; i < kd_lds; i += kAlignBlock) {
      l_kpl[i] = reinterpret_cast<const float4*>(nd)[2 * i];
      const int4 w = reinterpret_cast<const int4*>(nd)[2 * i + 1]; l_klk[i] = make_int2(w.x, w.y);
    }
    // a scan-sized fixed cloud (the tracker wiring: a tree per scan, every map point a query): its leaf arrays ride in LDS too -- the whole
    // tree is on chip and 20 iterations x N_m queries touch global memory for the query stream only
    if (A.kd_lds_points > 0) {
      const int fc = pick_cloud(S.fixed, a), nf = S.fixed.count[fc], fb = S.fixed.start[fc];
      kd_leaves_lds = !kKdTop && nf <= A.kd_lds_points && kd_lds == km.n_nodes;      // workgroup-uniform
      if (kd_leaves_lds) for (int i = tid; i < nf; i += kAlignBlock) { l_kxy[i] = S.fixed.kd.leaf_xy[fb + i]; l_knr[i] = S.fixed.kd.leaf_nrm[fb + i]; }
    }
  }
  if (pq_on) {      // bounding box of the fixed cloud (finite points only)
    const SliceDev& S = A.s[0];
    const int fc = pick_cloud(S.fixed, a), nf = S.fixed.count[fc];
    const float2* fp = S.fixed.xy + S.fixed.start[fc];
    for (int i = tid; i < nf; i += kAlignBlock) {
      const float2 p = fp[i];
      if (__builtin_fabsf(p.x) < 1e30f && __builtin_fabsf(p.y) < 1e30f) {
        atomicMin(&s_pqbb[0], ordered(p.x)); atomicMin(&s_pqbb[1], ordered(p.y)); atomicMax(&s_pqbb[2], ordered(p.x)); atomicMax(&s_pqbb[3], ordered(p.y));
      }
    }
  }
  if (kKdAllLds && !kd_leaves_lds) {      // cannot happen (the host sized the staging for the set's largest tree): refuse loudly, as above
    if (tid == 0) {
      A.out_pose[3 * a + 0] = s_pose[0]; A.out_pose[3 * a + 1] = s_pose[1]; A.out_pose[3 * a + 2] = s_pose[2];
      if (A.out_H) for (int k = 0; k < 9; ++k) A.out_H[9 * a + k] = 0.0f;      // (no iteration ran: the information matrix is the zero the regular path would hand back)
      if (A.out_its) A.out_its[a] = 0;
      if (A.host_polls) { __threadfence_system(); __hip_atomic_store(&A.out_status[a], (int) LSM2D_CAPACITY_EXCEEDED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
      else A.out_status[a] = LSM2D_CAPACITY_EXCEEDED;
    }
    return;
  }
  const Iso ident = {1.0f, 0.0f, 0.0f, 0.0f};
  for (int s = 0; s < A.n_slices; ++s) {
    const SliceDev& S = A.s[s];
    if (!kHasProj || S.finder != LSM2D_FINDER_PROJECTIVE) continue;
    const int fc = pick_cloud(S.fixed, a);
    // (a set unpacked by this launch: its size comes with the arguments -- the scalar cache may not have seen the count written above)
    project_cloud(S.fixed.xy + S.fixed.start[fc], (A.inline_n1 && S.unpack_src) ? S.unpack_n : S.fixed.count[fc], ident, S.proj, fcan + S.fcan_offset, tid, kW);
  }
  __syncthreads();
  if (pq_on) {      // the occupancy bitmap: every thread derives the same cell size and origin from the box, then stamps its points
    const SliceDev& S = A.s[0];
    const int fc = pick_cloud(S.fixed, a), nf = S.fixed.count[fc];
    const float2* fp = S.fixed.xy + S.fixed.start[fc];
    const unsigned k0 = s_pqbb[0], k1 = s_pqbb[1], k2 = s_pqbb[2], k3 = s_pqbb[3];
    const float minx = unordered(k0), miny = unordered(k1), maxx = unordered(k2), maxy = unordered(k3);
    const bool have = k0 <= k2 && k1 <= k3;                           // at least one finite point
    // a skipped tile's points stay farther than max_distance from every fixed point; the distance map pairs a query with the point of a PIXEL whose
    // centre is within max_distance of the query's pixel centre: two pixel diagonals more
    float reach = S.max_distance * 1.002f + 2e-3f;
    if (kHasDist && S.finder == LSM2D_FINDER_DISTMAP) reach += 3.0f / S.fixed.dist.meta[fc].inv_res;
    const float ext = __builtin_fmaxf(maxx - minx, maxy - miny);
    const float g = __builtin_fmaxf((reach + 0.1f) * (1.0f / 6.0f), ext * (1.0f / 125.0f));
    const float ox = minx - g, oy = miny - g, inv_g = 1.0f / g;
    const bool usable = have && g > 0.0f && g < 1e30f && S.max_distance >= 0.0f;
    if (tid == 0) { s_pq[0] = ox; s_pq[1] = oy; s_pq[2] = inv_g; s_pq[3] = usable ? reach : -1.0f; }
    if (usable) for (int i = tid; i < nf; i += kAlignBlock) {
      const float2 p = fp[i];
      if (!(__builtin_fabsf(p.x) < 1e30f && __builtin_fabsf(p.y) < 1e30f)) continue;
      const int cx = (int) ((p.x - ox) * inv_g), cy = (int) ((p.y - oy) * inv_g);       // 1 .. 126 by construction
      if ((unsigned) cx < 128u && (unsigned) cy < 128u) atomicOr(&l_occ[cy * kPqRowWords + (cx >> 5)], 1u << (cx & 31));
    }
  }
  __syncthreads();

  int it = __builtin_amdgcn_readfirstlane(s_it0);
  const int it_cap = __builtin_amdgcn_readfirstlane(A.inlier_runs ? 2 * A.max_it : A.max_it);      // (a scalar: as a select and a shift it lived in a vector register, spilled for the loop's back edge)
  const bool want_dig = A.out_stats != nullptr;      // the digest leaves the kernel through the statistics only
  // Fast-forward.  One iteration is a pure function of the pose it starts at (begin_iteration makes s_iso from s_pose; the stream, the bin walk and the sums
  // depend on s_iso alone -- the z-buffer's minimum and the fixed trees are deterministic, a kept or rebuilt unit list changes no bit; the prior, the damping
  // and the solve depend on the sums and s_pose).  So when the pose AFTER iteration `it` equals, bit for bit, the pose iteration it - p + 1 started at, the
  // poses repeat with period p from there on, and with R iterations of the phase left, skipping (R / p) * p of them leaves s_pose, s_H, s_last_n_in,
  // out_last_pose and the status exactly what the full run would have left; the R mod p others run ("fast_forward" 1).  They need not either ("fast_forward"
  // 2): the LAST iteration, it + R, is the twin of iteration t = s + ((R - 1) mod p), s = it - p + 1 <= t <= it, which has been executed -- its start pose and
  // the pose it ended on (the start of t + 1, or the pose just solved if t == it) are in the ring, and its H (as solve_update was given it: prior included,
  // damping not, which the solve applies to a copy) and inlier count wait in the alignment's row of A.ff_rows, stored by wave 0 iteration by iteration without
  // waiting and read once here.  The alignment finishes from those, R iterations counted and no iteration run.  Off where an iteration depends on more than the pose:
  // the chi^2 termination test (s_prev_chi; a fixed point ends itself there one iteration later anyway), the inlier-only runs (s_phase); and in a zero-copy launch (host_polls: at most
  // "zero_copy_max" alignments, results and statistics rows in pinned HOST memory -- a skipped row copied from the row one period back would be a read across
  // the host link on thread 0's serial path; the small calls, most of which the latency kernel and the split path take anyway, are the follow-up: DESIGN section 9)
  const bool ff_on = A.fast_forward && !(A.term_eps > 0.0f) && !A.inlier_runs && !A.host_polls;      // (wave-uniform: kernel arguments)
  for (; it < it_cap; ++it) {
    const bool inl_only = A.inlier_runs && __builtin_amdgcn_readfirstlane(s_phase) != 0;
    // wave priority by progress (lsm2d_kernels.h): halving intervals -- 1/2, 3/4, 7/8 of the iterations (configs[1]: 1.65 ms; off 1.86, quarters 1.69)
    { if (2 * it < A.max_it) __builtin_amdgcn_s_setprio(3); else if (4 * it < 3 * A.max_it) __builtin_amdgcn_s_setprio(2); else if (8 * it < 7 * A.max_it) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
    for (int s = 0; s < A.n_slices; ++s) {
      const SliceDev& S = A.s[s];
      const Iso T = s_iso[s];
      const uint32_t salt = (uint32_t) s * 0x632BE5ABu;
      Accum acc; accum_zero(acc);
      float seq_acc = 0.0f;      // kSeq: wave 0's lanes carry the slice's eleven running sums (in Accum's order) from trip to trip: seq_walk / seq_total; the counts stay in acc
      // kSeq: a matched pair becomes a record instead of being added into the thread's partial sums
      bool seq_have = false;      // kSeq: this thread holds a pair of the current trip
      auto seq_pair = [&](float2 pf, float2 nf, float2 pm, float2 nm, float (&t)[kSeqFields]) {
        bool inl; pair_terms(T, pf, nf, pm, nm, S.cauchy != 0, S.tau, inl_only, t, inl);
        ++acc.n_corr; acc.n_in += inl ? 1 : 0; acc.n_out += inl ? 0 : 1;
        seq_have = true;
      };
      // kSeq: the end of a trip.  The trip's PAIRS are compacted in thread order -- ascending column for the projective walk, ascending moving index for the queries: the
      // reference's order (a slot without a pair would add fma(+0, +0, h) == h: leaving it out changes no bit, and on the tracker's wiring of the point-query finders a
      // trip of 512 queries holds a handful of pairs) -- and APPENDED to the records in LDS (kSeqHalf of them: 14 KB); wave 0 walks them, in ascending position, whenever
      // the buffer is full and once more at the end of the slice (seq_flush): a walk costs two barriers, and the queries' 196 trips per iteration on configs[1] fill
      // the buffer three or four times.  One barrier per trip (the compaction's); the stores of later trips go to other slots than those of earlier ones, and every walk
      // stands between two barriers of its own.
      int seq_fill = 0;      // records waiting in LDS (the same in every thread)
      auto seq_walk_buffer = [&](int n) {      // n records in LDS, "no pair" records up to the next multiple of eight (seq_walk takes eight at a time)
        if (tid < ((n + 7) & ~7) - n) { float z[kSeqFields]; seq_zero(z); seq_store(l_rec, n + tid, z); }
        __syncthreads();
        // (seq_walk<true>: the walking wave at top priority while it walks, ahead of the other workgroups' streams on its SIMD -- its workgroup's other seven waves wait for it, and for the
        // solve, which is wave 0's: the wave keeps the priority until the next iteration sets the one its progress earns)
        if (tid < 64) seq_acc = seq_walk<true>(l_rec, n, tid, seq_acc);
        __syncthreads();
      };
      auto seq_trip = [&](const float (&t)[kSeqFields], int parity /* 0, 1, 0, ... from trip to trip: s_wcnt's two buffers */) {
        int n_rec = 0;
        const int pos = block_compact_pos(seq_have, s_wcnt, parity, n_rec, tid, kAlignBlock / 64);      // (one barrier; n_rec: the trip's pairs, the same in every thread)
        for (int done = 0; done < n_rec; ) {
          const int room = kSeqHalf - seq_fill, take = n_rec - done < room ? n_rec - done : room;
          if (seq_have && pos >= done && pos < done + take) seq_store(l_rec, seq_fill + pos - done, t);
          seq_fill += take; done += take;
          if (seq_fill == kSeqHalf) { seq_walk_buffer(kSeqHalf); seq_fill = 0; }
        }
        seq_have = false;
      };
      auto seq_flush = [&]() { if (seq_fill > 0) { seq_walk_buffer(seq_fill); seq_fill = 0; } };      // the end of the slice's pairs: what is still waiting
      LSM2D_PH(2);
      if (kHasProj && ((!kHasNN && !kHasDist && !kHasKd) || S.finder == LSM2D_FINDER_PROJECTIVE)) {
        {
          // HOT: every moving point, every iteration (correspondence_finder_projective_2d.cpp:47-48)
          const int mc = pick_cloud(S.moving, a);
          // clouds of at most one pair per thread (the tracker's clipped scenes) need no lane-chunked copy
          if (kProjCulled) {
            // Round 4: the survivors of the BLOCK-level test as a list in LDS, kept across iterations (see AlignArgs::units_off).  Build, when thread 0 found the
            // slice's transform outside the list's neighbourhood: (A) every thread tests the chunk it owns -- as the per-iteration test of round 3 did, with the
            // margins -- and the surviving chunks are compacted; (B) the nb blocks of every surviving chunk are tested the same way, dealt to the threads in
            // block-major order and compacted in that order: the list.  2 + ceil(nb s / 512) + 1 barriers, a few times per alignment.
            const int lane = tid & 63, wave = tid >> 6;
            uint16_t* units = l_units + s * A.units_stride;
            const int Tm = S.moving.lane_T[mc];
            const int nbs = __builtin_amdgcn_readfirstlane(S.moving.block_stride);
            const int B = cull_block_steps(Tm, nbs), nb = (Tm + B - 1) / B;
            // Round 20: what wave 0 decided about the slice's candidate list when it prepared this iteration (s_cand_state; a single slice: s == 0)
            const int cst = kCand ? __builtin_amdgcn_readfirstlane(s_cand_state) : 0;      // (stays 0 where the launch has no room for lists)
            LSM2D_PH_CAND(-1);
            if (kCand && cst == 1) {      // the list serves this transform: its points alone -- the unit list is neither rebuilt (s_rebuild is 0: wave 0 saw to that) nor read
              const float2* mxy = S.moving.xy + S.moving.start[mc];
              const uint32_t* cand = reinterpret_cast<const uint32_t*>(smem + __builtin_amdgcn_readfirstlane(s_cand_par[0])) + cand_blocker_words(S.proj.cols);
              const int n_cand = __builtin_amdgcn_readfirstlane(s_cand_n);
              if (S.proj.tiny_ok) project_candidates_t<false, kW>(mxy, T, S.proj, mcan, tid, cand, n_cand);
              else project_candidates_t<true, kW>(mxy, T, S.proj, mcan, tid, cand, n_cand);
              LSM2D_PH_CAND(2);
            } else {
            if (__builtin_amdgcn_readfirstlane(s_rebuild[s])) {
              typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
              const float m_t = A.cull_mt, m_th = A.cull_mth;      // (0 when the lists are not kept: the host sees to that -- a select made here was a vector register held across the iteration)
              const unsigned long long bb = reinterpret_cast<unsigned long long>(S.moving.lane_bounds + (size_t) mc * kAlignBlock);
              float4* bbase = reinterpret_cast<float4*>(((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (bb >> 32)) << 32) |
                                                        (unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) bb));
              int n_surv = 0;
              if constexpr (kW == kAlignBlock) {
              const u32x4 bw = __builtin_amdgcn_raw_buffer_load_b128(__builtin_amdgcn_make_buffer_rsrc(bbase, (short) 0, kAlignBlock * 16, 0x00020000), tid * 16, 0, 0);
              const bool keep = chunk_may_matter(T, S.proj, make_float4(__uint_as_float(bw.x), __uint_as_float(bw.y), __uint_as_float(bw.z), 0.0f), fcan + S.fcan_offset, S.point_distance, m_t, m_th);
              const u64 bal = __ballot(keep);
              { int wv = tid >> 6; asm volatile("" : "+v"(wv)); if (lane == 0) s_wcnt[wv] = __popcll(bal); }      // (the address made here, not in front of the iteration loop and kept)
              __syncthreads();
              int before = 0;
#pragma unroll
              for (int w = 0; w < nwaves; ++w) { const int cw = s_wcnt[w]; before += w < wave ? cw : 0; n_surv += cw; }
              n_surv = __builtin_amdgcn_readfirstlane(n_surv);
              if (keep) s_surv[before + (int) __builtin_amdgcn_mbcnt_hi((unsigned) (bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) bal, 0u))] = (uint16_t) tid;
              __syncthreads();
              } else {      // narrow workgroup: the 512 chunks in rounds of kW, compacted round by round (any order of the survivors serves: the z-buffer's minimum is the same)
                const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(bbase, (short) 0, kAlignBlock * 16, 0x00020000);
                int par = 0;
                for (int v0 = 0; v0 < kAlignBlock; v0 += kW, par ^= 1) {
                  const int v = v0 + tid; bool keep = false;
                  if (v < kAlignBlock) {
                    const u32x4 bw = __builtin_amdgcn_raw_buffer_load_b128(brs, v * 16, 0, 0);
                    keep = chunk_may_matter(T, S.proj, make_float4(__uint_as_float(bw.x), __uint_as_float(bw.y), __uint_as_float(bw.z), 0.0f), fcan + S.fcan_offset, S.point_distance, m_t, m_th);
                  }
                  const int pos = block_compact_pos(keep, s_wcnt, par, n_surv, tid, nwaves);
                  if (keep) s_surv[pos] = (uint16_t) v;
                }
                __syncthreads();
              }
              // (B) test v = (block v / n_surv, survivor v mod n_surv), v = tid, tid + 512, ...; block_compact_pos: one barrier per round, buffers alternating
              const unsigned long long kb = reinterpret_cast<unsigned long long>(S.moving.block_bounds + (size_t) mc * nbs * kAlignBlock);
              float4* kbase = reinterpret_cast<float4*>(((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (kb >> 32)) << 32) |
                                                        (unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) kb));
              const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(kbase, (short) 0, nbs * kAlignBlock * 16, 0x00020000);
              int n_units = 0, parity = 1, i = tid, blk = 0;
              while (n_surv > 0 && i >= n_surv && blk < nb) { i -= n_surv; ++blk; }
              const int n_tests = nb * n_surv;
              for (int v0 = 0; v0 < n_tests; v0 += kW, parity ^= 1) {
                bool k2 = false; int code = 0;
                if (blk < nb) {
                  const int g = (int) s_surv[i];
                  code = (blk << 9) | g;
                  const u32x4 w4 = __builtin_amdgcn_raw_buffer_load_b128(krs, code * 16, 0, 0);      // entry (blk * 512 + g) of the cloud's block circles
                  k2 = chunk_may_matter(T, S.proj, make_float4(__uint_as_float(w4.x), __uint_as_float(w4.y), __uint_as_float(w4.z), 0.0f), fcan + S.fcan_offset, S.point_distance, m_t, m_th);
                }
                const int pos = block_compact_pos(k2, s_wcnt, parity, n_units, tid, nwaves);
                if (k2) units[pos] = (uint16_t) code;
                i += kW;
                while (n_surv > 0 && i >= n_surv && blk < nb) { i -= n_surv; ++blk; }
              }
              if (tid == 0) { s_nunits[s] = n_units; s_list_iso[s] = T; }
              __syncthreads();
            }
            LSM2D_PH_LISTS();
            const int n_units = __builtin_amdgcn_readfirstlane(s_nunits[s]);
            if (kCand && cst == 2) {
              // Build: (a) every column's blocker, made by the stream itself from the r, th, u and column it has just computed for the canvas (the blockers
              // cleared in front of it); (b) behind it, the unit list's points once more, against the rule (lsm2d_device.h); wave 0 looks at the count behind
              // the sums' barrier (too long: not used, the alignment goes on streaming units)
              uint32_t* blk = reinterpret_cast<uint32_t*>(smem + __builtin_amdgcn_readfirstlane(s_cand_par[0]));
              cand_clear_blockers<kW>(S.proj, tid, blk);
              __syncthreads();
              // Round 30 ("cand_queue" 1: qcap >= 0): the stream also queues the points its provisional blockers could not settle, and (b) looks at those
              // alone -- unless they outgrew the queue's room (a wave-uniform read behind the barrier): then (b) is the pass over the unit list, as with "cand_queue" 0
              const int qcap = __builtin_amdgcn_readfirstlane(s_cand_par[6]);
              if (qcap < 0) { if (n_units > 0) project_cloud_list_blk<kW>(S.moving.lane_xy + S.moving.lane_start[mc], Tm, T, S.proj, mcan, tid, kAlignBlock, units, n_units, B, blk, s_cand_par); }
              else if (n_units > 0) project_cloud_list_blkq<kW>(S.moving.lane_xy + S.moving.lane_start[mc], Tm, T, S.proj, mcan, tid, kAlignBlock, units, n_units, B, blk, s_cand_par, &s_cand_qn, &s_cand_q);
              __syncthreads();
              LSM2D_PH_CAND(1);
              const int nq = __builtin_amdgcn_readfirstlane(s_cand_qn);
              if (qcap > 0 && nq <= qcap) {
                const unsigned long long qb = reinterpret_cast<unsigned long long>(s_cand_q);
                const uint32_t* queue = reinterpret_cast<const uint32_t*>(((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (qb >> 32)) << 32) |
                                                                          (unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) qb));
                cand_collect_queue<kW>(S.moving.xy + S.moving.start[mc], T, S.proj, tid, queue, nq, blk, s_cand_par, &s_cand_n);
              } else {
                if (qcap >= 0 && tid == 0) ++s_cand_fb;
                cand_collect<kW, kAlignBlock>(S.moving.lane_xy + S.moving.lane_start[mc], Tm, T, S.proj, tid, units, n_units, B, blk, s_cand_par, &s_cand_n);
              }
              LSM2D_PH_CAND(4);
            } else {
              if (n_units > 0) project_cloud_list<kW>(S.moving.lane_xy + S.moving.lane_start[mc], Tm, T, S.proj, mcan, tid, kAlignBlock, units, n_units, B);
              LSM2D_PH_CAND(0);
            }
            }
          }
          else if (S.moving.lane_xy && S.moving.lane_bounds && A.cull) {
            // exact culling against the fixed canvas (chunk_may_matter): every thread tests the chunk it would stream, the survivors are
            // compacted (two barriers: counts, then the list) and their points spread evenly over the workgroup (project_cloud_units)
            const int lane = tid & 63, wave = tid >> 6;
            // (the chunk's circle through a buffer resource: base in SGPRs, one 32-bit lane offset -- a per-thread 64-bit pointer would be
            // hoisted out of the iteration loop and spilled: 64 registers)
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const unsigned long long bb = reinterpret_cast<unsigned long long>(S.moving.lane_bounds + (size_t) mc * kAlignBlock);
            float4* bbase = reinterpret_cast<float4*>(((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (bb >> 32)) << 32) |
                                                      (unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) bb));
            const u32x4 bw = __builtin_amdgcn_raw_buffer_load_b128(__builtin_amdgcn_make_buffer_rsrc(bbase, (short) 0, kAlignBlock * 16, 0x00020000), tid * 16, 0, 0);
            const bool keep = chunk_may_matter(T, S.proj, make_float4(__uint_as_float(bw.x), __uint_as_float(bw.y), __uint_as_float(bw.z), 0.0f), fcan + S.fcan_offset, S.point_distance);
            const u64 bal = __ballot(keep);
            if (lane == 0) s_wcnt[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, n_surv = 0;
#pragma unroll
            for (int w = 0; w < nwaves; ++w) { const int cw = s_wcnt[w]; before += w < wave ? cw : 0; n_surv += cw; }
            // (rank below the lane by v_mbcnt: a hoisted 64-bit lane mask would be two more registers held -- and spilled -- across the loops)
            if (keep) s_surv[before + (int) __builtin_amdgcn_mbcnt_hi((unsigned) (bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) bal, 0u))] = (uint16_t) tid;
            __syncthreads();
            const int Tm = S.moving.lane_T[mc];
            // blocks of an even number of steps, 7 per chunk (measured on configs[1], T = 98: blocks of 2 / 4 / 6 / 8 / 14 steps 1.098 / 1.017 /
            // 0.991 / 0.983 / 0.969 ms -- what a unit costs to set up outweighs the better balance of smaller ones; element-wise row-major
            // order, balanced to one step, 1.066: docs/REJECTED.md)
            const int B = cull_block_steps(Tm), nb = (Tm + B - 1) / B;
            if (n_surv > 0) project_cloud_units(S.moving.lane_xy + S.moving.lane_start[mc], Tm, T, S.proj, mcan, tid, kAlignBlock, s_surv, n_surv, B, nb);
          }
          else if (S.moving.lane_xy) project_cloud_lanes(S.moving.lane_xy + S.moving.lane_start[mc], S.moving.lane_T[mc], T, S.proj, mcan, tid, kAlignBlock);
          else project_cloud(S.moving.xy + S.moving.start[mc], S.moving.count[mc], T, S.proj, mcan, tid, kAlignBlock);
        }
        __syncthreads();
        LSM2D_PH_STREAM();
        // bin walk (correspondence_finder_projective_2d.cpp:55-74): the fixed side comes from LDS, the two gathers of the
        // moving winner are issued together, and every cell read is reset for the next projection
        const int mbase = S.moving.start[pick_cloud(S.moving, a)], fbase = S.fixed.start[pick_cloud(S.fixed, a)];
        const float2* mn = S.moving.nrm + mbase; const float2* mp = S.moving.xy + mbase;
        const float2* fnr = S.fixed.nrm + fbase; const float2* fpp = S.fixed.xy + fbase;
        const float4* maos = S.moving.aos ? S.moving.aos + mbase : nullptr;      // (a set without its AoS copy -- sizes still pending on the device, or
        const float4* faos = S.fixed.aos ? S.fixed.aos + fbase : nullptr;        //  unpacked by this launch -- is gathered from its split arrays)
        const u64* fcs = fcan + S.fcan_offset;
        if constexpr (kSeq) {
          // "sum_order" 1: trips of kAlignBlock consecutive columns (every thread takes part in every trip: the barriers), slot = column - first column of the trip
          for (int col0 = 0; col0 < S.proj.cols; col0 += kAlignBlock) {
            const int col = col0 + tid;
            float t[kSeqFields]; seq_zero(t);
            if (col < S.proj.cols) {
              const u64 fk = fcs[col], mk = mcan[col];
              mcan[col] = kEmptyCell;
              const float fd = __uint_as_float((uint32_t) (fk >> 32)), md = __uint_as_float((uint32_t) (mk >> 32));
              if (mk != kEmptyCell && fk != kEmptyCell && !(__builtin_fabsf(fd - md) > S.point_distance)) {
                const int mi = (int) (uint32_t) mk, fi = (int) (uint32_t) fk;
                float2 nm, pm; float4 f;
                if (maos) { const float4 m4 = maos[mi]; pm = make_float2(m4.x, m4.y); nm = make_float2(m4.z, m4.w); } else { nm = mn[mi]; pm = mp[mi]; }
                if (faos) f = faos[fi]; else { const float2 p2 = fpp[fi], n2 = fnr[fi]; f = make_float4(p2.x, p2.y, n2.x, n2.y); }
                float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
                if (!(__builtin_fmaf(nqx, f.z, nqy * f.w) < S.normal_cos)) {
                  if (want_dig) digest_add(&s_dig, salt, fi, mi);
                  seq_pair(make_float2(f.x, f.y), make_float2(f.z, f.w), pm, nm, t);
                }
              }
            }
            seq_trip(t, (col0 / kAlignBlock) & 1);
          }
        }
        else if constexpr (kW != kAlignBlock) {
          // narrow workgroup: this thread plays the VIRTUAL threads tid, tid + kW, ... (< 512) of the wide kernel one after the other -- each with its own partial sums
          // over the wide kernel's columns (vt, vt + 512, ...) in its order, each virtual wave's tree into that wave's row of `red` (kW is a multiple of 64: a
          // physical wave plays whole virtual waves)
          const int bits = 32 - __builtin_clz(((S.proj.cols + kAlignBlock - 1) / kAlignBlock) | 1);
          for (int vt = tid; vt < kAlignBlock; vt += kW) {
            Accum av; accum_zero(av);
            for (int col = vt; col < S.proj.cols; col += kAlignBlock) {
              const u64 fk = fcs[col], mk = mcan[col];
              mcan[col] = kEmptyCell;
              if (mk == kEmptyCell || fk == kEmptyCell) continue;
              const float fd = __uint_as_float((uint32_t) (fk >> 32)), md = __uint_as_float((uint32_t) (mk >> 32));
              if (__builtin_fabsf(fd - md) > S.point_distance) continue;
              const int mi = (int) (uint32_t) mk, fi = (int) (uint32_t) fk;
              float2 nm, pm; float4 f;
              if (maos) { const float4 m4 = maos[mi]; pm = make_float2(m4.x, m4.y); nm = make_float2(m4.z, m4.w); } else { nm = mn[mi]; pm = mp[mi]; }
              if (faos) f = faos[fi]; else { const float2 p2 = fpp[fi], n2 = fnr[fi]; f = make_float4(p2.x, p2.y, n2.x, n2.y); }
              float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
              if (__builtin_fmaf(nqx, f.z, nqy * f.w) < S.normal_cos) continue;
              if (want_dig) digest_add(&s_dig, salt, fi, mi);
              accumulate_pair(T, make_float2(f.x, f.y), make_float2(f.z, f.w), pm, nm, S.cauchy != 0, S.tau, av, inl_only);
            }
            block_reduce_store(av, red, vt, bits);
          }
        }
        else
        if (kProjCulled && maos && faos) {
          // Round 5: the walk as a two-deep pipeline -- the NEXT column's cells are read and gated (LDS) and its winners' two 16-byte rows asked for BEFORE this
          // column's factor terms are formed; the terms are added in the same column order as before (the sums keep their bits).  A trip used to end in two
          // dependent gathers from L2 that nothing covered: three exposed round trips per thread, iteration and slice; now the second and third travel under
          // the arithmetic of the one before.  (All three trips asked for up front needed 24 registers more than the kernel has: 96 bytes of scratch.)
          auto gate = [&](int col, int& fi, int& mi) -> bool {
            if (col >= S.proj.cols) return false;
            const u64 fk = fcs[col], mk = mcan[col];
            mcan[col] = kEmptyCell;
            if (mk == kEmptyCell || fk == kEmptyCell) return false;
            const float fd = __uint_as_float((uint32_t) (fk >> 32)), md = __uint_as_float((uint32_t) (mk >> 32));
            if (__builtin_fabsf(fd - md) > S.point_distance) return false;
            mi = (int) (uint32_t) mk; fi = (int) (uint32_t) fk;
            return true;
          };
          int fi_a = 0, mi_a = 0, fi_b = 0, mi_b = 0;
          float4 m_a = make_float4(0.f, 0.f, 0.f, 0.f), f_a = m_a, m_b = m_a, f_b = m_a;
          bool ok_a = gate(tid, fi_a, mi_a);
          if (ok_a) { m_a = maos[mi_a]; f_a = faos[fi_a]; }
          for (int col = tid; col < S.proj.cols; col += kAlignBlock) {
            const bool ok_b = gate(col + kAlignBlock, fi_b, mi_b);
            if (ok_b) { m_b = maos[mi_b]; f_b = faos[fi_b]; }
            if (ok_a) {
              const float2 pm = make_float2(m_a.x, m_a.y), nm = make_float2(m_a.z, m_a.w);
              float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
              if (!(__builtin_fmaf(nqx, f_a.z, nqy * f_a.w) < S.normal_cos)) {
                if (want_dig) digest_add(&s_dig, salt, fi_a, mi_a);
                accumulate_pair(T, make_float2(f_a.x, f_a.y), make_float2(f_a.z, f_a.w), pm, nm, S.cauchy != 0, S.tau, acc, inl_only);
              }
            }
            ok_a = ok_b; fi_a = fi_b; mi_a = mi_b; m_a = m_b; f_a = f_b;
          }
        }
        else
        for (int col = tid; col < S.proj.cols; col += kAlignBlock) {
          const u64 fk = fcs[col], mk = mcan[col];
          mcan[col] = kEmptyCell;
          if (mk == kEmptyCell || fk == kEmptyCell) continue;
          const float fd = __uint_as_float((uint32_t) (fk >> 32)), md = __uint_as_float((uint32_t) (mk >> 32));
          if (__builtin_fabsf(fd - md) > S.point_distance) continue;
          const int mi = (int) (uint32_t) mk, fi = (int) (uint32_t) fk;
          float2 nm, pm; float4 f;
          if (maos) { const float4 m4 = maos[mi]; pm = make_float2(m4.x, m4.y); nm = make_float2(m4.z, m4.w); } else { nm = mn[mi]; pm = mp[mi]; }
          if (faos) f = faos[fi]; else { const float2 p2 = fpp[fi], n2 = fnr[fi]; f = make_float4(p2.x, p2.y, n2.x, n2.y); }
          float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
          if (__builtin_fmaf(nqx, f.z, nqy * f.w) < S.normal_cos) continue;
          if (want_dig) digest_add(&s_dig, salt, fi, mi);
          accumulate_pair(T, make_float2(f.x, f.y), make_float2(f.z, f.w), pm, nm, S.cauchy != 0, S.tau, acc, inl_only);
        }
      } else if (kHasNN || kHasDist || kHasKd) {
        // NN finder fused with the factor (correspondence_finder_kd_tree_2d.cpp:12-27): every moving point is
        // transformed, matched to its exact nearest fixed point within max_distance, normal-gated, accumulated
        const int fc = pick_cloud(S.fixed, a), mc = pick_cloud(S.moving, a);
        // (the clouds' first indices declared wave-uniform -- they are -- so that the six pointers formed from them live in scalar registers: round 6, k_align<0,1,0,0,1>
        // 48 B of scratch -> none, role B / exact NN 1.608 -> 1.393 ms on configs[1]; the other point-query modes unchanged: profiles/r06/pq_uniform_bases_ab_r06o.txt)
        const int mbase = __builtin_amdgcn_readfirstlane(S.moving.start[mc]), fbase = __builtin_amdgcn_readfirstlane(S.fixed.start[fc]);
        const float2* fn = S.fixed.nrm + fbase; const float2* mn = S.moving.nrm + mbase;
        const float2* fp = S.fixed.xy + fbase;  const float2* mp = S.moving.xy + mbase;
        const bool use_grid = kHasNN && ((!kHasDist && !kHasKd) || S.finder == LSM2D_FINDER_NN);
        const bool use_kd = kHasKd && ((!kHasNN && !kHasDist) || S.finder == LSM2D_FINDER_KDTREE);
        GridMeta g; DistMeta dm;
        const int32_t* cst = nullptr; const int32_t* sidx = nullptr; const float2* sxy = nullptr;
        const KdNode* knd = nullptr; const float2* knr = nullptr;
        if (use_kd) {      // the reference's tree over the fixed cloud (correspondence_finder_kd_tree_2d.cpp:18-19): one descent + one leaf per query
          knd = S.fixed.kd.nodes + __builtin_amdgcn_readfirstlane(S.fixed.kd.meta[fc].node_base);
          sxy = S.fixed.kd.leaf_xy + fbase; knr = S.fixed.kd.leaf_nrm + fbase;
        } else if (use_grid) {
          g = S.fixed.grid.meta[fc];
          // the meta comes through a vector load: tell the compiler it is wave-uniform -- seven VGPRs fewer across the query loops, which
          // takes the last spills out of them (NN role B 2.27 -> 2.06 ms, role A 7.91 -> 7.82; variants_r02v_nn_scalar_meta.log)
          g.minx = uniform_f(g.minx); g.miny = uniform_f(g.miny); g.h = uniform_f(g.h); g.inv_h = uniform_f(g.inv_h);
          g.gw = __builtin_amdgcn_readfirstlane(g.gw); g.gh = __builtin_amdgcn_readfirstlane(g.gh); g.cell_base = __builtin_amdgcn_readfirstlane(g.cell_base);
          cst = S.fixed.grid.cell_start + g.cell_base;
          sidx = S.fixed.grid.sorted_idx + fbase; sxy = S.fixed.grid.sorted_xy + fbase;
          if (kNNGlobal) knr = S.fixed.grid.sorted_nrm + fbase;
        } else {
          dm = S.fixed.dist.meta[fc];       // distance-map finder: one lookup per query (correspondence_finder_nn_2d.cpp:63-80)
        }
        const float md2 = S.max_distance * S.max_distance;
        const int nm_pts = S.moving.count[mc];
        // cooperative search (kNNGroup lanes per query) when THIS alignment's fixed cloud is at least four times its moving one --
        // decided per alignment from the device-side counts, so ragged batches get the right loop for each cloud (the oracle's
        // device-order mode applies the same rule)
        const bool coop = use_grid && (long long) S.fixed.count[fc] >= 4ll * nm_pts;
        // this iteration's keep bits, one per tile of 64 moving points (see the prologue): bit t of l_keep <-> tile t
        const int n_tiles = (nm_pts + 63) >> 6;
        const bool pq_cull = pq_on && S.moving.tile_bounds && !coop && ((n_tiles + kAlignBlock - 1) / kAlignBlock) * (kAlignBlock / 64) <= A.pq_keep_words;
        if (pq_cull) {
          const float4* tb = S.moving.tile_bounds + S.moving.tile_start[mc];
          const float ox = s_pq[0], oy = s_pq[1], inv_g = s_pq[2], reach = s_pq[3];
          for (int t0 = 0; t0 < n_tiles; t0 += kAlignBlock) {
            const int t = t0 + tid; bool keep = false;
            if (t < n_tiles) {
              const float4 b = tb[t];
              keep = true;
              const float kf = (b.z * 1.002f + reach) * inv_g;      // cells the tile's reach spans (rho = +inf, a tile with a non-finite point: no claim)
              if (reach >= 0.0f && kf < 10.0f) {
                float qx, qy; xf_point(T, b.x, b.y, qx, qy);
                const float fx = __builtin_floorf((qx - ox) * inv_g), fy = __builtin_floorf((qy - oy) * inv_g);
                if (fx > -64.0f && fx < 192.0f && fy > -64.0f && fy < 192.0f) {
                  const int k = (int) kf + 1, cx = (int) fx, cy = (int) fy;
                  const int x0 = cx - k < 0 ? 0 : cx - k, x1 = cx + k > 127 ? 127 : cx + k, y0 = cy - k < 0 ? 0 : cy - k, y1 = cy + k > 127 ? 127 : cy + k;
                  keep = false;
                  if (x0 <= x1) {
                    const u64 mask = (~0ull >> (63 - (x1 - x0))) << (x0 & 31);      // at most 21 bits, from bit x0 of the two-word window
                    for (int y = y0; y <= y1; ++y) {
                      const uint32_t* row = l_occ + y * kPqRowWords + (x0 >> 5);
                      if ((((u64) row[1] << 32) | (u64) row[0]) & mask) { keep = true; break; }
                    }
                  }
                }
                else keep = !(fx == fx && fy == fy);      // far beyond the bitmap: nothing within reach; not a number: no claim
              }
            }
            const u64 bal = __ballot(keep);
            if ((tid & 63) == 0) l_keep[(t0 >> 6) + (tid >> 6)] = bal;
          }
          __syncthreads();
        }
        // the grid search is cooperative on dense fixed clouds (kNNGroup lanes per query); the distance map is one lookup
        auto query_loop = [&](auto group_tag) {
          constexpr int group = decltype(group_tag)::value;
          const int sub = tid & (group - 1);
          constexpr int per_step = kAlignBlock / group;
          for (int j0 = 0; j0 < nm_pts; j0 += per_step) {
            bool skip = false;                       // kSeq: a culled tile's wave still takes part in the trip (its records are zeros, the barriers are everybody's)
            float t[kSeqFields];                     // kSeq: this thread's record of the trip
            if constexpr (kSeq) seq_zero(t);
            if (group == 1 && pq_cull) {             // this wave's 64 queries of the trip are one tile
              const int tile = (j0 >> 6) + __builtin_amdgcn_readfirstlane(tid >> 6);
              const u64 w = l_keep[tile >> 6];
              const unsigned half = (tile & 32) ? (unsigned) (w >> 32) : (unsigned) w;
              if (!((__builtin_amdgcn_readfirstlane((int) half) >> (tile & 31)) & 1)) { if constexpr (kSeq) skip = true; else continue; }
            }
            const int j = j0 + tid / group;
            const bool live = j < nm_pts && !skip;           // whole groups are live or not: the shuffles inside stay uniform
            const float2 pm = live ? mp[j] : make_float2(0.0f, 0.0f);
            float qx, qy; xf_point(T, pm.x, pm.y, qx, qy);
            int best = -1;
            if (use_kd) {      // the match's point and normal come from the leaf arrays, where the scan found it: the original index is never needed
              if (live) {
                float2 bxy;
                const int pos = kKdAllLds ? kd_query_pos<true>(knd, l_kxy, qx, qy, md2, bxy, l_kpl, l_klk, kd_lds)
                              : kKdTop ? kd_query_pos(knd, sxy, qx, qy, md2, bxy, l_kpl, l_klk, kd_lds)
                              : kd_leaves_lds ? kd_query_pos<true>(knd, l_kxy, qx, qy, md2, bxy, l_kpl, l_klk, kd_lds) : kd_query_pos(knd, sxy, qx, qy, md2, bxy, l_kpl, l_klk, kd_lds);
                if (pos >= 0) {
                  const float2 nm = mn[j], nf = kKdAllLds ? l_knr[pos] : (kKdTop ? knr[pos] : (kd_leaves_lds ? l_knr[pos] : knr[pos]));
                  float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
                  const float dot = __builtin_fmaf(nqx, nf.x, nqy * nf.y);
                  if (!(dot < S.normal_cos)) {
                    if (want_dig) digest_add(&s_dig, salt, S.fixed.kd.leaf_idx[fbase + pos], j);      // the original index: only the digest asks for it
                    if constexpr (kSeq) seq_pair(bxy, nf, pm, nm, t); else
                    accumulate_pair(T, bxy, nf, pm, nm, S.cauchy != 0, S.tau, acc, inl_only);
                  }
                }
              }
            } else
            if (kNNGlobal) {      // the match's point and normal come from where the search found it: no detour through the original index
              const int pos = live ? nn_query_pos<group>(g, cst, sidx, sxy, qx, qy, S.max_distance, md2, sub, j < A.nn_qcache ? l_qc + 8 * j : nullptr) : -1;
              if (pos >= 0 && sub == 0) {                    // one lane per query accumulates
                const float2 nm = mn[j], nf = knr[pos], pf = sxy[pos];
                float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
                const float dot = __builtin_fmaf(nqx, nf.x, nqy * nf.y);
                if (!(dot < S.normal_cos)) {
                  if (want_dig) digest_add(&s_dig, salt, sidx[pos], j);
                  if constexpr (kSeq) seq_pair(pf, nf, pm, nm, t); else
                  accumulate_pair(T, pf, nf, pm, nm, S.cauchy != 0, S.tau, acc, inl_only);
                }
              }
            } else
            if (kNNLds) { if (live) best = nn_query<1, uint16_t, uint16_t>(g, l_cst, l_sidx, l_sxy, qx, qy, S.max_distance, md2, 0); }
            else
            if (use_grid) {
              if (live) best = (group == 1 && nn_lds) ? nn_query<1, uint16_t, uint16_t>(g, l_cst, l_sidx, l_sxy, qx, qy, S.max_distance, md2, 0)
                                                      : nn_query<group>(g, cst, sidx, sxy, qx, qy, S.max_distance, md2, sub);
            }
            else if (live) best = distmap_lookup(dm, S.fixed.dist.parent, qx, qy);
            if (best >= 0 && sub == 0) {                     // one lane per query accumulates
              const float2 nm = mn[j], nf = fn[best];
              float nqx, nqy; xf_normal(T, nm.x, nm.y, nqx, nqy);
              const float dot = __builtin_fmaf(nqx, nf.x, nqy * nf.y);
              if (!(dot < S.normal_cos)) {
                if (want_dig) digest_add(&s_dig, salt, best, j);
                if constexpr (kSeq) seq_pair(fp[best], nf, pm, nm, t); else
                accumulate_pair(T, fp[best], nf, pm, nm, S.cauchy != 0, S.tau, acc, inl_only);
              }
            }
            if constexpr (kSeq) seq_trip(t, (j0 / per_step) & 1);      // "sum_order" 1: the trip's queries are per_step consecutive moving indices (one lane per query holds its pair: ascending thread = ascending query)
          }
        };
        // (the cooperative search on a scan-sized fixed cloud with its tables in LDS: 2 / 4 / 8 lanes per query take 21 / 41 / 90 ms against
        // 8.1 ms with one lane per query -- the time goes with the number of wave-queries, i.e. into the fixed cost of a query, not its candidates)
        // (several queries of a thread in flight together -- all points, then all pixels, then all parents -- measured with the registers
        // for it: 4 waves per SIMD and 3-4 trips tie with this loop at 8 waves per SIMD on role B and lose 10-50 % elsewhere; at 8 waves per SIMD
        // with only the parents' indices kept live, 2 / 3 trips take 0.29 / 0.38 ms against 0.21 on role B and lose on role A too; DESIGN App. A)
        // (matched pairs queued per wave in LDS and added up 64 at a time with every lane busy, instead of ~70 instructions of accumulate_pair on
        // every trip for the quarter of the lanes that matched: slower everywhere -- distance map role A 5.21 -> 5.87 ms, NN role A 7.95 -> 8.61,
        // distance map role B 0.21 -> 0.30: the ballot, the queue and the reloads cost more than the idle lanes; DESIGN App. A)
        if (!kNNLds && coop) query_loop(std::integral_constant<int, kNNGroup>{});
        else query_loop(std::integral_constant<int, 1>{});
      }
      if constexpr (kSeq) seq_flush();
      LSM2D_PH(0);
      // (a projective slice's thread accumulates at most ceil(cols / block) pairs: its counts are a few bits, summed by ballots)
      if constexpr (kW == kAlignBlock)      // (the narrow workgroups' virtual waves have written their rows in the walk)
      block_reduce_store(acc, red, tid, (kHasProj && !kHasNN && !kHasDist && !kHasKd) ? 32 - __builtin_clz(((S.proj.cols + kAlignBlock - 1) / kAlignBlock) | 1) : 0);
      __syncthreads();
      LSM2D_PH_SUMS();
      if (tid < 64) {
        // lanes 0..13 of wave 0 each add one quantity over the waves and then into the iteration's sum themselves; lane 13 the pairs, lane 14 counts the active slices
        int ln = tid; asm volatile("" : "+v"(ln));      // (s_sum's and red's addresses for this lane made here: hoisted, they were spilled across the iteration)
        const float cur = s_sum[ln & 15];
        // (wave order, from +0: block_reduce_gather's sums; float and integer sum of the same words, each lane uses its own kind)
        float v = 0.0f; int vi = 0;
        {
          const float* rr = red + (ln < kAccumWords ? ln : 0);
          float g[kAlignBlock / 64];
#pragma unroll
          for (int w = 0; w < kAlignBlock / 64; ++w) g[w] = rr[w * kAccumWords];
#pragma unroll
          for (int w = 0; w < kAlignBlock / 64; ++w) { v += g[w]; vi += __float_as_int(g[w]); }
        }
        if constexpr (kSeq) v = seq_total(seq_acc, tid);      // (the partial sums' floats were never touched: the eleven quantities are the walker's)
        const int n_corr_s = __builtin_amdgcn_readlane(vi, 13);
        const bool act = n_corr_s > S.min_corr;     // slices with #pairs <= min_num_correspondences are skipped (their pairs still count)
        float tot = cur;
        if (act || ln == kSumPairs) tot = ln < 11 ? cur + v : __int_as_float(__float_as_int(cur) + (ln == kSumPairs ? n_corr_s : (ln == kSumActive ? 1 : vi)));
        if (ln < kSumWords) s_sum[ln] = tot;
      }
      LSM2D_PH(1);
      // pure projective kernels need no barrier here: the other waves go on to the next slice's projection (the cells it
      // writes were reset by the bin walk) and touch `red` again only after the barrier that follows it, which lane 0
      // joins once it is done with the partials.  The point-query branches write `red` without such a barrier in between.
      if (kHasNN || kHasDist || kHasKd) __syncthreads();
    }
    if (tid < 64) {
      // Wave 0's stretch, as a VECTOR over the wave: behind the fast-forward the launch waits for a few lone workgroups, and nobody issues under this stretch.
      // The operations on every value and their order are block_reduce_gather's, solve_update's, add_prior's, begin_iteration's and the ring rule's; what
      // changed is who holds what.  Lane q < 15 owns word q of s_sum; lanes 32..40 the nine entries of the information matrix, lane 41 the inlier count beside
      // them; decisions are taken by every lane alike from v_readlane broadcasts.  The serial state still lives in LDS from one iteration to the next --
      // no register is held across the loops for it -- and EVERYTHING the stretch reads there is asked for here, at once: one round trip instead of one per value.
      // (the lane made HERE: every per-lane address and constant below derives from it -- hoisted in front of the loops they would be registers all threads keep)
      int ln = tid; asm volatile("" : "+v"(ln));
      const int l16 = ln & (kFfRing - 1);
      static_assert(kFfRing == 16 && kMaxSlices == 4, "lane masks below");
      const float p0 = s_pose[0], p1 = s_pose[1], p2 = s_pose[2];
      const int n = s_ring_n, phase_end = s_phase_end;
      uint32_t* const ffw = s_ff_rows;
      const Iso iso0 = s_iso[0], Ll = s_list_iso[ln & 3];
      const uint32_t e0 = s_ring[3 * l16], e1 = s_ring[3 * l16 + 1], e2 = s_ring[3 * l16 + 2];      // lane j < 16: slot j of the ring
      const float tot = s_sum[l16];      // lane q < 15: word q of the sums
#define LSM2D_RL_F(x, k) __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), k))
      const int hk = ln - 32;
      const bool h_lane = (unsigned) hk < 9u;
      const int n_corr = __builtin_amdgcn_readlane(__float_as_int(tot), kSumPairs), active = __builtin_amdgcn_readlane(__float_as_int(tot), kSumActive);
      const int n_in = __builtin_amdgcn_readlane(__float_as_int(tot), 11);
      const float chi_in = LSM2D_RL_F(tot, 9), chi_out = LSM2D_RL_F(tot, 10);
      if (ln == 0) s_last_n_in = n_in;
      int skip = 0;      // fast-forward: iterations to jump over behind this one
      if (A.out_stats) {      // the statistics row: one word per lane
        static_assert(sizeof(StatsDev) == 28, "seven words: n_corr n_in n_out chi_in chi_out dig_lo dig_hi");
        int n_out = __builtin_amdgcn_readlane(__float_as_int(tot), 12); float chi_o = chi_out;
#ifdef LSM2D_DEBUG_UNITS      // diagnostics build: the culled stream's list length and whether it was rebuilt, in place of the outlier statistics
        if (kProjCulled) { n_out = s_nunits[0]; chi_o = (float) s_rebuild[0]; }
#endif
        u64 dg = s_dig;
#ifdef LSM2D_DEBUG_CAND      // diagnostics build: what the iteration did about the candidate list (s_cand_state) and the list's entries, in place of the pair digest
        if (kCand) dg = ((u64) (unsigned) s_cand_n << 32) | (u64) (unsigned) s_cand_state;
        // ... and, of a build iteration, the maybes its stream queued (bits 2.. of the low word; none with "cand_queue" 0)
        if (kCand && s_cand_state == 2) dg |= (u64) (unsigned) s_cand_qn << 2;
#endif
        const int w = ln == 0 ? n_corr : ln == 1 ? n_in : ln == 2 ? n_out : ln == 3 ? __float_as_int(chi_in) : ln == 4 ? __float_as_int(chi_o) : ln == 5 ? (int) (uint32_t) dg : (int) (uint32_t) (dg >> 32);
        if (ln < 7) reinterpret_cast<int32_t*>(A.out_stats + (size_t) a * A.stats_stride + it)[ln] = w;
      }
      bool done = false;
      float np0 = 0.0f, np1 = 0.0f, np2 = 0.0f;      // the pose the next iteration starts at
      if (!active) { if (ln == 0) { s_status = LSM2D_NOT_ENOUGH_CORRESPONDENCES; s_done = 1; } done = true; }
      else {
        // the solve's nine inputs as broadcasts; information matrix = H of the last iteration (h00 h01 h02 / h01 h11 h12 / h02 h12 h22), prior included: one store by its nine lanes
        float x0 = LSM2D_RL_F(tot, 0), x1 = LSM2D_RL_F(tot, 1), x2 = LSM2D_RL_F(tot, 2), x3 = LSM2D_RL_F(tot, 3), x4 = LSM2D_RL_F(tot, 4), x5 = LSM2D_RL_F(tot, 5),
              x6 = LSM2D_RL_F(tot, 6), x7 = LSM2D_RL_F(tot, 7), x8 = LSM2D_RL_F(tot, 8);
        float Hq = (hk == 0) ? x0 : (hk == 1 || hk == 3) ? x1 : (hk == 2 || hk == 6) ? x2 : (hk == 4) ? x3 : (hk == 5 || hk == 7) ? x4 : x5;      // (lane 41: the inlier count, below)
        if (A.prior) {      // add_prior's terms: lane q < 9 that of its solve input (the upper triangle's and b's), lane 32 + k that of H's entry k
          const int pr = h_lane ? hk / 3 : (int) ((0x210211000ull >> (4 * l16)) & 15), pc = h_lane ? hk - 3 * (hk / 3) : (int) ((0x333221210ull >> (4 * l16)) & 15);
          float P = 0.0f;
          if (ln < 9 || h_lane) P = prior_term_lane_call(s_prior, p0, p1, p2, pr, pc);
          Hq += P;
          const float tp = tot + P;
          x0 = LSM2D_RL_F(tp, 0); x1 = LSM2D_RL_F(tp, 1); x2 = LSM2D_RL_F(tp, 2); x3 = LSM2D_RL_F(tp, 3); x4 = LSM2D_RL_F(tp, 4); x5 = LSM2D_RL_F(tp, 5);
          x6 = LSM2D_RL_F(tp, 6); x7 = LSM2D_RL_F(tp, 7); x8 = LSM2D_RL_F(tp, 8);
        }
        if (h_lane) s_H[hk] = Hq;
        if (ff_on) {      // the pose this iteration started at: into the ring (slot = pushes so far & 15)
          if (ln < 3) s_ring[3 * (n & (kFfRing - 1)) + ln] = __float_as_uint(ln == 0 ? p0 : (ln == 1 ? p1 : p2));
          if (ln == 0) s_ring_n = n + 1;
        }
        float dmp = A.damping;
        asm volatile("" : "+v"(dmp));      // (not a loop invariant to hoist -- as a double it was kept, and spilled, across the whole kernel)
        float dx, dy, dth;
        const bool ok = solve_flat(x0, x1, x2, x3, x4, x5, x6, x7, x8, dmp, dx, dy, dth);
        if (!ok) { if (ln == 0) { s_status = LSM2D_SINGULAR_H; s_done = 1; } done = true; }      // (nothing of the step has been written: s_pose stays the start pose)
        else {
          // cos / sin of the heading the iteration started at: slice 0's, the same function of the same float, unless a sensor offset stands between them
          float sn = iso0.s, cs = iso0.c;
          if (A.s[0].has_sensor) sincos_fixed(p2, sn, cs);
          np0 = __builtin_fmaf(cs, dx, __builtin_fmaf(-sn, dy, p0));
          np1 = __builtin_fmaf(sn, dx, __builtin_fmaf(cs, dy, p1));
          np2 = wrap_angle(p2 + dth);
          if (ln < 3) s_pose[ln] = ln == 0 ? np0 : (ln == 1 ? np1 : np2);
          if (ff_on) {
            // the new pose against the ring, as integers (-0 is not +0, a NaN is its pattern).  Slot j holds the start of iteration it - k, k = (n - j) & 15, if
            // that many were pushed; slot n & 15 is this iteration's own start pose, on its way there.  The hit with the smallest k is the newest entry, the
            // smallest period: the sixteen hits rotated into the order of k, lowest bit first.
            const int kb = (n - ln) & (kFfRing - 1);
            const bool own = kb == 0;
            const bool hit = ln < kFfRing && kb <= n && (own ? __float_as_uint(p0) : e0) == __float_as_uint(np0) && (own ? __float_as_uint(p1) : e1) == __float_as_uint(np1) &&
                             (own ? __float_as_uint(p2) : e2) == __float_as_uint(np2);
            const uint32_t bal = (uint32_t) __ballot(hit) & 0xFFFFu;
            if (bal) {      // once per alignment: lane 0 alone, as it always was
              const uint32_t rev = __builtin_bitreverse32(bal) >> 16;      // bit i: slot 15 - i, i.e. k = (i + n + 1) & 15
              const int rot = (n + 1) & (kFfRing - 1);
              const uint32_t byk = ((rev << rot) | (rev >> (kFfRing - rot))) & 0xFFFFu;
              const int k = __builtin_amdgcn_readfirstlane(__builtin_ctz(byk)), n1 = n + 1;
              if (ln == 0) {
                const unsigned p = (unsigned) (k + 1), left = (unsigned) (phase_end - (it + 1));
                skip = (int) ((left / p) * p);
                const uint32_t* const rows = ffw;
                if (rows && left > 0) {      // finish from the ring: the last iteration's twin is `back` entries back (0: this very iteration), 0 <= back <= k
                  const int back = k - (int) ((left - 1) % p);
                  if (back > 0) {      // (back == 0: it is its own twin -- s_H, s_last_n_in, the pose just solved and out_last_pose are what they must be)
                    const uint32_t* et = s_ring + 3 * ((n1 - 1 - back) & (kFfRing - 1));      // the pose the twin started at,
                    const uint32_t* en = s_ring + 3 * ((n1 - back) & (kFfRing - 1));          // the pose it ended on: the start of the iteration behind it
                    const uint32_t* w = rows + ((n1 - 1 - back) & (kFfRing - 1)) * kFfRowWords;
                    _Pragma("nounroll") for (int j = 0; j < 9; ++j) s_H[j] = __uint_as_float(w[j]);      // (once per alignment: word by word, no registers for a row)
                    s_last_n_in = (int) w[9];
                    if (A.out_last_pose) { A.out_last_pose[3 * a + 0] = __uint_as_float(et[0]); A.out_last_pose[3 * a + 1] = __uint_as_float(et[1]); A.out_last_pose[3 * a + 2] = __uint_as_float(et[2]); }
                    s_pose[0] = __uint_as_float(en[0]); s_pose[1] = __uint_as_float(en[1]); s_pose[2] = __uint_as_float(en[2]);
                  }
                  skip = (int) left;      // all of them: phase_over below, and ff_on excludes a second phase -- s_done, the status decided at the exit
                }
                if (A.out_stats) {      // the skipped iterations' rows are the cycle's: written by this wave, read back by it in program order
                  StatsDev* row = A.out_stats + (size_t) a * A.stats_stride;
                  for (int j = it + 1; j <= it + skip; ++j) {
                    StatsDev r = row[j - (int) p];
#ifdef LSM2D_DEBUG_UNITS      // diagnostics build: a skipped row says so, and with which period (tools/units_probe.py)
                    r.chi_out = (rows ? -0.5f : 0.0f) - (float) p;      // (... and a row filled in by "fast_forward" 2 -- nothing runs behind it -- by the half)
#endif
                    row[j] = r;
                  }
                }
              }
              skip = __builtin_amdgcn_readfirstlane(skip);      // lane 0's
            }
          }
          bool phase_over = it + skip + 1 >= phase_end;
          if (ff_on && !phase_over && ffw)      // another iteration follows: what a twin of THIS one would leave behind besides its poses -- H as the solve was given it, the inlier count: one store by ten lanes
            if ((unsigned) hk < (unsigned) kFfRowWords) ffw[(n & (kFfRing - 1)) * kFfRowWords + hk] = hk == 9 ? (uint32_t) n_in : __float_as_uint(Hq);
          if (A.term_eps > 0.0f) {      // the aligner's termination criterion: relative decay of the total chi^2 (lsm2d.h), afresh in every phase
            const float chi_now = chi_in + chi_out;
            if (it > s_phase_start && __builtin_fabsf(s_prev_chi - chi_now) < A.term_eps * chi_now) phase_over = true;      // status stays RUNNING: decided below as after max_iterations
            if (ln == 0) s_prev_chi = chi_now;
          }
          if (phase_over) {
            // enable_inlier_only_runs (lsm2d.h): the regular loop ended without a failure and with enough inliers -> up to max_it iterations over inliers only
            if (A.inlier_runs && s_phase == 0 && n_in >= A.min_inliers) { if (ln == 0) { s_phase = 1; s_phase_start = it + 1; s_phase_end = it + 1 + A.max_it; } }
            else { if (ln == 0) s_done = 1; done = true; }
          }
        }
      }
#undef LSM2D_RL_F
      if (ff_on && ln == 0) s_skip = skip;      // every iteration, whichever way it went: nobody adds a stale one
      if (!done) {      // begin_iteration for the next one, under the same barrier: lane j prepares slice j (its constants through the scalar cache, picked by lane)
        int hs = 0; float cS = 1.0f, sS = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f;
        for (int j = 0; j < A.n_slices; ++j) {
          const SliceDev& Sj = A.s[__builtin_amdgcn_readfirstlane(j)];      // (said to be wave-uniform: the loop over lanes is not to become one load with a per-lane address -- a trip to the L2)
          if (ln == j) { hs = Sj.has_sensor; cS = Sj.cSinv; sS = Sj.sSinv; S0 = Sj.Sinv[0]; S1 = Sj.Sinv[1]; S2 = Sj.Sinv[2]; }
        }
        if (ln < A.n_slices) {
          const float Sv[3] = {S0, S1, S2}, X[3] = {np0, np1, np2};
          float Xe[3] = {np0, np1, np2};
          if (hs) compose(cS, sS, Sv, X, Xe);
          Iso N; sincos_fixed(Xe[2], N.s, N.c); N.tx = Xe[0]; N.ty = Xe[1];
          const Iso cur0 = s_iso[0];      // (kProjCulled, the candidate list: the transform the iteration that ends here had)
          s_iso[ln] = N;
          if (kProjCulled) {      // (see begin_iteration)
            const float cd = N.c * Ll.c + N.s * Ll.s, sd = N.s * Ll.c - N.c * Ll.s;
            const float ddx = N.tx - (cd * Ll.tx - sd * Ll.ty), ddy = N.ty - (sd * Ll.tx + cd * Ll.ty);
            const int rb = (A.cull_keep && cd > 0.5f && __builtin_fabsf(sd) <= A.cull_mth && ddx * ddx + ddy * ddy <= A.cull_mt2) ? 0 : 1;
            s_rebuild[ln] = rb;
            if (kCand && s_cand_par[0] > 0 && ln == 0) {
              // Round 20, the candidate list (a single slice: lane 0's).  First the books of the iteration that has just ended: a list
              // it built (the sums' barrier stands behind the build's counting) is the list from here on if it fits, built at the transform this iteration had --
              // asked for in `cur0` before s_iso[0] was overwritten.  Then the policy for the coming iteration.  The list serves N while the unit list it was taken
              // from does (a list whose pose was left is dropped) and N is within the tight margins of the transform it was built at.  A new one is built from
              // iteration cand_first_it on, while fewer than cand_max_builds were (a test of the step just taken against a fraction of the margins, so that
              // only settled poses build, measured slower than building at cand_first_it whatever the step was: docs/REJECTED.md).  Everything is read here and now, from LDS: nothing of it lives in a register anywhere else in the kernel.
              int st = s_cand_state, stat = s_cand_stat;
              const int n_built = s_cand_n, cap = s_cand_par[1], first_it = s_cand_par[2], max_builds = s_cand_par[3];
              const float mt = __int_as_float(s_cand_par[4]), mth = __int_as_float(s_cand_par[5]);
              Iso Lc = s_cand_iso;
              if (st == 2) {
                const bool fits = n_built <= cap;
                // (as arithmetic, not `fits ? 0x10000 : 0x1010000`: hipcc 6.x turned that select into an s_cselect_b32 on a stale SCC behind a v_cmp that sets VCC --
                // every list was booked as too long; seen in the assembly, the counters of tests/test_gpu_candidate_lists.py are what guards it)
                int over = fits ? 0 : 1; asm volatile("" : "+v"(over));
                stat += 0x10000 + (over << 24);
                st = fits ? 1 : 0;
                if (fits) { Lc = cur0; s_cand_iso = cur0; }
              }
              const bool serves = st == 1 && !rb && cand_pose_within(N, Lc, mt, mth);
              const bool build = !serves && it + 1 >= first_it && ((stat >> 16) & 0xFF) < max_builds && (stat >> 24) == 0;      // (a list that was too long once will be again: no second try)
              if (serves && (stat & 0xFFFF) != 0xFFFF) ++stat;      // counted where it is decided: the alignment's last iteration too
              s_cand_state = serves ? 1 : (build ? 2 : 0);
              s_cand_stat = stat;
              if (build) { s_cand_n = 0; s_cand_qn = 0; }
            }
          }
        }
        int zi = 0; asm volatile("" : "+v"(zi));      // (made here, every time: see begin_iteration)
        if (ln < kSumWords) s_sum[ln] = __int_as_float(zi);
        if (ln == 0) s_dig = (u64) (unsigned) zi;
        if (A.out_last_pose && ln < 3) A.out_last_pose[3 * a + ln] = ln == 0 ? np0 : (ln == 1 ? np1 : np2);
      } else if (kCand && ln == 0 && s_cand_par[0] > 0) {
        // The alignment ends with this iteration.  If it built a list, the build is booked all the same, behind the iteration that made its blockers (as
        // arithmetic, like the books above: no select on a condition code)
        int built = s_cand_state == 2 ? 1 : 0, over = s_cand_n > s_cand_par[1] ? 1 : 0;
        asm volatile("" : "+v"(built), "+v"(over));
        s_cand_stat += (built << 16) + ((built & over) << 24);
      }
    }
    LSM2D_PH(2);
    LSM2D_PH_TAIL();
    __syncthreads();
    if (ff_on) it += __builtin_amdgcn_readfirstlane(s_skip);      // (every thread alike: `it` stays a scalar, and the exit below counts the skipped iterations in)
    if (s_done) { ++it; break; }
  }
  if (tid == 0) {
    int st = s_status;
    if (st == LSM2D_RUNNING) st = (A.max_it > 0 && s_last_n_in < A.min_inliers) ? LSM2D_NOT_ENOUGH_INLIERS : LSM2D_SUCCESS;
    A.out_pose[3 * a + 0] = s_pose[0]; A.out_pose[3 * a + 1] = s_pose[1]; A.out_pose[3 * a + 2] = s_pose[2];
    if (A.out_H) for (int k = 0; k < 9; ++k) A.out_H[9 * a + k] = s_H[k];
    if (A.out_its) A.out_its[a] = it;
    if (kCand && A.cand_out) { A.cand_out[a] = s_cand_stat; A.cand_out[A.n_align + a] = s_cand_fb; }      // (handed over only when the caller asked for statistics: the timed launch does not pay for it.  The second word per alignment: its builds that fell back from the queue)
    // the status goes last, behind a system-scope release: with results written straight to pinned host memory the host polls
    // this word instead of waiting for the stream (lsm2d_align_batch), and whoever sees it sees everything above
    if (stamp) {
      unsigned long long* co = A.clock_out + 4 * (a / A.clock_stride);
      co[0] = __builtin_amdgcn_s_memtime() - s_clk[0];
      co[1] = __builtin_amdgcn_s_memrealtime() - s_clk[1];
      co[2] = s_clk[1];                                                            // when it started (100 MHz ticks): which dispatch round it was in
#ifdef LSM2D_PHASE_PROBE
      co[1] = s_ph[0]; co[2] = s_ph[1]; co[3] = s_ph[2];      // cycles: query phase, barrier + reduction, solve + the rest (co[0] stays the lifetime)
      if (A.host_polls) { __threadfence_system(); __hip_atomic_store(&A.out_status[a], st, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); } else A.out_status[a] = st;
      return;
#endif
      co[3] = (unsigned long long) __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4) |      // HW_REG_HW_ID (id 4): wave / SIMD / CU / SE it ran on
              ((unsigned long long) __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20) << 32);  // HW_REG_XCC_ID (id 20)
    }
    if (A.host_polls) { __threadfence_system(); __hip_atomic_store(&A.out_status[a], st, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }
    else A.out_status[a] = st;
  }
}
