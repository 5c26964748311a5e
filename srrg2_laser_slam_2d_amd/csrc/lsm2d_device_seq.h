// lsm2d_device_seq.h -- "sum_order" 1: the factor's terms as records (pair_terms, seq_store) and the walk that adds them pair after pair in the reference's order (seq_walk, seq_total).
// Part of lsm2d_device.h (included there, inside namespace lsm2d, at the place this text was cut from); not a header of its own.
// ---- "sum_order" 1: H, b and the chi^2 statistics added PAIR AFTER PAIR, the reference's order --------------------------------------
// The reference adds one factor after the other into H and b (octave/solver/nicp_post.m:69-90: H += J'*J; b += J'*e inside the loop over the
// correspondences; the correspondence vector is in ascending column for the projective finder, correspondence_finder_projective_2d.cpp:55-74, and
// in ascending moving index for the point-query finders, correspondence_finder_kd_tree_2d.cpp:12-27).  The default kernels add in trees (a thread's
// pairs, then 64 lanes, then 8 waves): the same terms, another association.  With the option on, every thread that holds a pair writes the pair's
// TERMS -- accumulate_pair's operations up to the sums, in its order -- as a record of kSeqFields floats into LDS, slot = the pair's position in the
// reference's order within the current trip of the workgroup (a trip: 512 consecutive columns / moving indices, handed over in two halves); after the barrier
// eleven lanes of wave 0 walk the records in ascending slot, lane q adding quantity q with exactly the fused operations the sequential CPU restatement of the factor
// uses (the tests hold the two against each other bit for bit): h = fma(w a_i, a_j, h), two of them chained for h22 and b2, chi sums by plain adds.  A slot without a pair holds zeros:
// fma(+0, +0, h) == h and h + 0 == h bit for bit (no sum here is ever -0: they start at +0).  The counts are integers and keep their ballots.
// Record = 14 floats, 56 bytes: a0 a1 a2 e0 | wa0 wa1 wa2 w | dd de chi_in chi_out | 1 0 (wa_i = w * a_i, rounded by the thread that holds the pair: the
// reference's `wa` temporaries; the two constants travel with every record).  The records of HALF a trip (kSeqHalf = 256) sit in LDS; lane q of the walking wave
// reads, per record, the four operands of ITS two fused adds straight from LDS -- acc = fma(x1, y1, acc); acc = fma(x2, y2, acc) -- at four per-lane FIELD
// offsets and one stride for all: an operand that is a constant for this lane (1 for the chi sums' y1; 0, 0 for the second add of the nine quantities that have
// none) reads the record's constant fields.  So a record costs the walk four LDS reads with immediate offsets (the compiler pairs them: ds_read2_b32) and two
// dependent FMAs, nothing else.  (Round 6, measured in isolation -- tools/seq_walk_probe.py: a first form that selected and multiplied in the loop and waited for
// each record's loads 135 cycles per record; per-lane strides for the constants -- sixteen address adds per four records -- 65; this one: see DESIGN section 5.)
static constexpr int kSeqFields = 14, kSeqHalf = 256;
static constexpr int kSeqLdsBytes = kSeqHalf * kSeqFields * 4;
template <bool kInlineLog = false>
LSM2D_DEV void pair_terms(const Iso& T, float2 pf, float2 nf, float2 pm, float2 nm, bool cauchy, float tau, bool inl_only,
                          float (&t)[kSeqFields], bool& inlier) {
  float qx, qy, nqx, nqy;
  xf_point(T, pm.x, pm.y, qx, qy);
  xf_normal(T, nm.x, nm.y, nqx, nqy);
  const float dx = qx - pf.x, dy = qy - pf.y;
  const float e0 = __builtin_fmaf(nf.x, dx, nf.y * dy);
  const float e1 = nqx - nf.x, e2 = nqy - nf.y;
  const float a0 = __builtin_fmaf(T.c, nf.x, T.s * nf.y);
  const float a1 = __builtin_fmaf(-T.s, nf.x, T.c * nf.y);
  const float a2 = __builtin_fmaf(a1, pm.x, -(a0 * pm.y));
  const float d0 = -nqy, d1 = nqx;
  const float chi = __builtin_fmaf(e0, e0, __builtin_fmaf(e1, e1, e2 * e2));
  float w = 1.0f, kern = 0.0f;
  inlier = true;
  if (cauchy) {
    const float q = chi / tau;
    w = 1.0f / (1.0f + q);
    inlier = chi < tau;
    if (!inlier) kern = tau * (kInlineLog ? log_fixed_inline(1.0f + q) : log_fixed(1.0f + q));
    if (inl_only) w = inlier ? 1.0f : 0.0f;
  }
  t[0] = a0; t[1] = a1; t[2] = a2; t[3] = e0;
  t[4] = w * a0; t[5] = w * a1; t[6] = w * a2; t[7] = w;
  t[8] = __builtin_fmaf(d0, d0, d1 * d1);
  t[9] = __builtin_fmaf(d0, e1, d1 * e2);
  t[10] = inlier ? chi : 0.0f;
  t[11] = inlier ? 0.0f : kern;
}
// "no pair in this slot": zeros and the constants
LSM2D_DEV void seq_zero(float (&t)[kSeqFields]) {
#pragma unroll
  for (int f = 0; f < 12; ++f) t[f] = 0.0f;
  t[12] = 1.0f; t[13] = 0.0f;
}
// `rec`: the region's start; record `slot` (0 .. kSeqHalf - 1) as seven 8-byte stores
LSM2D_DEV void seq_store(float* rec, int slot, const float (&t)[kSeqFields]) {
  float2* r = reinterpret_cast<float2*>(rec + slot * kSeqFields);
#pragma unroll
  for (int f = 0; f < kSeqFields / 2; ++f) r[f] = make_float2(t[2 * f], t[2 * f + 1]);
}
// The walk, one wave.  The chain of a quantity is serial -- acc = fma(x1, y1, acc); acc = fma(x2, y2, acc), record after record -- and what a single lane walking
// it pays per record is the LDS round trip of the record's operands as far as nothing covers it: the first form of this round (lane q < 11 walks quantity q, two
// groups of two records in flight: all the registers the kernel has for it) took 44 cycles per record.  Now a QUAD of lanes walks a quantity: lane j of quad q
// (lane 4 q + j) holds the operands of records 8 b + 2 j and 8 b + 2 j + 1 of batch b, so ONE pair of LDS reads per operand brings eight records, and the running
// sum travels round the quad -- quad_perm:[3,0,1,2], one DPP move -- picking up each lane's two records in ascending record order: lane 0 takes it from lane 3
// (the previous batch's end), adds records 8 b and 8 b + 1, lane 1 takes it from lane 0, ...  Every lane executes every step; the value that counts is in lane s
// after step s, what the other lanes compute meanwhile is overwritten before it is ever read on the chain.  Per record: two fused adds + half a move = 2.5
// vector instructions on the chain and an eighth of the LDS reads, the next batch's loads in flight under this batch's twenty instructions.  The same fused operations on
// the same values in the same order as before: the same bits (the tests hold the kernel against the sequential CPU restatement bit for bit).
// `acc`: the caller keeps it per lane between calls (zero at first, in all lanes); the running sum of quantity q is lane 4 q + 3's after every call -- seq_total()
// brings it to lane q.  Records n .. 8 ceil(n / 8) - 1 of the buffer must hold "no pair" records (k_align_seq, which walks its pairs only, pads them; the split path's kernels write every slot of a half-trip).
// Measured (tools/seq_walk_probe.py: cycles per record in isolation; configs[1] with "sum_order" 1: k_align_seq ms; profiles/r06/sum_order_walker_quads_ab_r06.txt):
//   single lane 44 / 1.123;  quads, R records per lane and batch, B batches in registers: R 1 B 4: 44 / 1.114;  R 2 B 2 (shipped): 30 / 0.955-0.961;  R 2 B 3: 28 / 0.971;
//   R 4 B 2: 23 / 0.944 with 48 bytes of scratch in the headline instantiation.  The cost is ~14 cycles for a record's two dependent fused adds + ~30 per move of the
//   sum to the next lane (a DPP result feeding the chain), i.e. per R records.  Bringing the OPERANDS to the sum instead (quad broadcasts, the x operand as
//   v_fmac_f32_dpp's own): 33-37 / 1.04-1.06 -- four DPP instructions per record cost more than half a move.  Loads pinned ahead of the chain (sched_barrier): slower.
//   (The single-lane walk's code is gone: 44 cycles per record and 1.123 ms against the quads' 30 and 0.955-0.961; docs/REJECTED.md, "alternatives whose code is gone".)
LSM2D_DEV float seq_quad_prev(float v) {      // lane 4 q + j <- lane 4 q + (j + 3) % 4
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x93 /* quad_perm:[3,0,1,2] */, 0xF, 0xF, true));
}
template <bool kTopPriority = false>      // kTopPriority: s_setprio 3 once the walk's addresses are made (k_align_seq: the caller says when it ends)
LSM2D_DEV float seq_walk(const float* rec, int n, int lane, float acc) {
  asm volatile("" : "+v"(lane));      // (the lane's field offsets are made HERE, every time: as loop invariants of the iteration loop they are registers held -- and spilled -- across the whole kernel)
  const int q = (lane >> 2) < 11 ? (lane >> 2) : 0, j = lane & 3;      // (quads 11 .. 15 walk along like quad 0 and hold nothing of value)
  const bool chi = q >= 9, has2 = q == 5 || q == 8;
  const int fx1 = (int) ((0xBA654655444ull >> (4 * q)) & 15), fy1 = chi ? 12 : (int) ((0x00333221210ull >> (4 * q)) & 15);      // field of x1 (wa_i, or the chi term) and of y1 (a_j, e0, or the constant 1)
  const int fx2 = has2 ? 7 : 13, fy2 = has2 ? (q == 5 ? 8 : 9) : 13;                                                             // w and dd / de; elsewhere the constant 0 twice
  constexpr int kR = 2, kBufs = 2;      // records per lane and batch; batches in registers (the R 2 B 2 row above)
  const float* r0 = rec + kR * j * kSeqFields;      // this lane's first record of batch 0
  const float* px1 = r0 + fx1; const float* py1 = r0 + fy1; const float* px2 = r0 + fx2; const float* py2 = r0 + fy2;
  constexpr int kBatch = 4 * kR * kSeqFields;      // floats from one batch to the next
  struct Ops { float x1[kR], y1[kR], x2[kR], y2[kR]; };
  auto load = [&](int b) {
    Ops o; const int off = b * kBatch;
#pragma unroll
    for (int r = 0; r < kR; ++r) { o.x1[r] = px1[off + r * kSeqFields]; o.y1[r] = py1[off + r * kSeqFields]; o.x2[r] = px2[off + r * kSeqFields]; o.y2[r] = py2[off + r * kSeqFields]; }
    return o;
  };
  auto chain = [&](const Ops& o) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float t = seq_quad_prev(acc);
#pragma unroll
      for (int r = 0; r < kR; ++r) { t = __builtin_fmaf(o.x1[r], o.y1[r], t); t = __builtin_fmaf(o.x2[r], o.y2[r], t); }
      acc = t;
    }
  };
  const int nb = (n + 4 * kR - 1) / (4 * kR);
  if (nb <= 0) return acc;
  Ops buf[kBufs];
  if constexpr (kTopPriority) __builtin_amdgcn_s_setprio(3);
#pragma unroll
  for (int i = 0; i + 1 < kBufs; ++i) buf[i] = load(i < nb ? i : nb - 1);
  for (int b = 0; b < nb; b += kBufs) {      // buf[i] holds batch b + i; the free buffer takes batch b + i + kBufs - 1 (past the end: the last batch again, never used)
#pragma unroll
    for (int i = 0; i < kBufs; ++i) {
      if (b + i < nb) {
        const int nxt = b + i + kBufs - 1;
        buf[(i + kBufs - 1) % kBufs] = load(nxt < nb ? nxt : nb - 1);
        chain(buf[i]);
      }
    }
  }
  return acc;
}
// the walk's result for lane q < 11 of the walking wave: the running sum of quantity q (every lane of the wave calls)
LSM2D_DEV float seq_total(float acc, int lane) {
  const int src = lane < 11 ? 4 * lane + 3 : lane;
  return __int_as_float(__builtin_amdgcn_ds_bpermute(4 * src, __float_as_int(acc)));
}
