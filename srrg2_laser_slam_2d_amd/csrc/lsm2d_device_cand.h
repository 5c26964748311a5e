// lsm2d_device_cand.h -- the candidate lists of the culled projective stream (k_align_cand): the rule and its proof, the build iteration's stream with its blockers, the collect pass over the unit list and the one over the queue of maybes, the gather that serves a list, and the test that a list still holds.
// Part of lsm2d_device.h (included there, inside namespace lsm2d, at the place this text was cut from); not a header of its own.
// ---- Round 20: CANDIDATE lists -- the second, tighter level of the kept lists ----------------------------------------------------------------
// Once the pose has settled an iteration still streams the whole unit list (some 41 k points on configs[1]) to keep one winner per column.  A candidate list,
// built in an iteration that has just streamed its unit list at the slice transform T0, holds the INDICES of the streamed points that can still be, or beat, a
// winner under any transform T near T0; while it is valid the iteration gathers those points alone (project_candidates).  The moving canvas such an iteration
// makes equals the unit list's canvas at T cell for cell -- the unit list's own proof (chunk_may_matter) carries the rest: every pair, sum and pose keeps its bits.
//
// What "near" means.  T applies M = [[c, -s], [s, c]] with the fp32 outputs of sincos_fixed (abs error 9.3e-8 each: M is a rotation scaled by rho, |rho - 1| <=
// 1.4e-7), so in exact arithmetic q_T = A q_0 + d with A = M_T M_0^-1 a rotation by dth = atan2(sd, cd) scaled by kappa, |kappa - 1| <= 2.8e-7, and d = t_T - A t_0:
// cd, sd, dx, dy are the quantities begin_iteration forms for s_rebuild.  The list serves every T with |d| <= m_t and |dth| <= 1.001 m_th; k_align's validity
// test leaves room for what its own fp32 evaluation of cd, sd, d can be off by (cand_pose_within).  Where T and T0 have the SAME rotation bits A is the identity
// and d = t_T - t_0, one subtraction of two nearby floats: nothing to allow for.  Otherwise: the factor 1 / rho_0^2 the expression leaves out, 2.8e-7 |t_0|; the
// roundings of cd (two products of at most 3e-8 and a sum of 6e-8) and sd (6e-8), 1.4e-7 |t_0| together; the roundings of the two products and the sum per
// component, 1.7e-7 |t_0|_1: 4e-7 (|t_0|_1 + |t_T|_1) covers them; 3e-7 on |sd|; asin(x) <= 1.0005 x for x <= 0.05, the largest margin the option table admits.
//
// Depth.  The stream computes qx = fl(c px + a), a = fl(-s py + tx) (and qy alike): each rounding is at most 6e-8 of its result, |a| <= |py| + |t| and |q| = r, so
// the computed q is within eq = 6e-8 (|p| + |t| + 1.42 r) of M p + t; a point at depth r has |p| <= (r + |t|) / rho, hence eq <= eq(r) = 1.5e-7 r + 1.25e-7 |t|_1: a
// bound from the depth alone, which a column's winner carries in its key.  r2 = fma(qx, qx, qy qy) and r = sqrt_rn(r2) add 1.2e-7 r.  Exactly, | |q_T| - |q_0| | <=
// |kappa - 1| |q_0| + |d|.  So the depths the stream computes for ONE point under T0 and under any served T differ by at most
//   md(r) = m_t + 2 eq(r) + (2 x 1.2e-7 + 2.8e-7) r  <=  m_t + 1.0e-6 r + 2.6e-7 (|t|_1 + 2 m_t) + 1e-7      (cand_depth_margin; |t_T|_1 <= |t_0|_1 + 2 m_t)
// with 1.8e-7 r to spare for the two roundings (6e-8 r each) of the comparison that uses it.
// Column.  The bearing of A q_0 is that of q_0 plus dth; adding d turns it by at most asin(|d| / (|q_0| - |d|)); the computed q is off by eq on either side, i.e.
// by eq / r of bearing each; bearing()'s polynomial (5e-8 rad), its octant fix-ups (three roundings of at most 1.2e-7 rad) and the rounding of u = fma(K00, th,
// K01) (half an ulp of 16 384: 4.9e-4 columns) add at most 1.3e-3 columns per evaluation at up to 16 384 columns (the host offers no list to a wider canvas).
// With asin(x) <= 1.048 x on [0, 1/2] the computed u of one point under T0 and under a served T differ by at most
//   cs(r) = K00 (1.001 m_th + 1.06 md / (r - md)) + 4e-3   columns, claimed only where md <= r / 4      (cand_classify; md >= m_t + 2 eq covers the numerator)
// -- unless the bearing WRAPS between -pi and pi: a point within cs of either end makes no claim.
// The rule.  Call a streamed point INTERIOR when, at T0, its depth is inside [rmin, rmax] by more than md and its u is farther than cs from both edges of a valid
// column: under every served T it passes the gates and falls into that same column.  A column's BLOCKER is the nearest of its interior points (project_point_stream_blk:
// the minimum of r + md(r) per column, an array of its own -- not the canvas's winner: along a wall seen at an angle the nearest point of a column sits at the
// column's edge, and on configs[1] a quarter of the winners are no interior points).  A streamed point p is DROPPED when it cannot pass the gates under any served
// T -- coordinates that are not finite (padding slots), a depth beyond a range gate by more than md, a column beyond either end of the canvas by more than cs -- or
// when it is interior and its column's blocker b has r_b + md(r_b) < r_p - md(r_p): under every served T both are in the column and b is strictly nearer, so p is
// not the winner; b itself is in the list (the inequality fails for b against itself, and for every interior point at most as deep -- an interior winner among
// them).  Everything else is kept: points near a column edge or a range gate (from either side), points just outside the field of view, the points of a column
// without a blocker, every winner.  Keeping a point that could have gone is always harmless.
LSM2D_DEV float cand_depth_margin(float r, float m_t, float tn2 /* |tx| + |ty| + 2 m_t */) { return m_t + __builtin_fmaf(1.0e-6f, r, __builtin_fmaf(2.6e-7f, tn2, 1e-7f)); }
// 0: p passes the gates under no served transform; 1: no claim; 2: interior (column `col`, depth r, margin md) under every served transform.  ONE statement of the
// rule in two steps: from the point to what the stream makes of it (r, th, u, col: project_point_stream's operations, one for one), and from there to the class.
// The build iteration's stream (project_point_stream_blk) enters at the second step with the r, th, u and col it has just made for the canvas.
LSM2D_DEV int cand_classify_polar(const ProjK& P, float r, float th, float u, int col /* v_cvt_flr_i32_f32 of u */, float m_t, float m_th, float tn2, float& md) {
  md = cand_depth_margin(r, m_t, tn2);
  if (r < P.rmin - md || r > P.rmax + md) return 0;
  if (!(md <= 0.25f * r)) return 1;
  const float aK = __builtin_fabsf(P.K00);
  const float cs = __builtin_fmaf(aK, __builtin_fmaf(1.06f, md / (r - md), 1.001f * m_th), 4e-3f);
  if ((3.14159274101257324f - __builtin_fabsf(th)) * aK <= cs) return 1;      // the bearing may wrap
  if (u < -cs || u > P.colsf + cs) return 0;
  if ((unsigned) col >= (unsigned) P.cols) return 1;
  if (!(r >= P.rmin + md && r <= P.rmax - md)) return 1;
  const float f = u - (float) col;      // (exact: u and its floor are within one of each other)
  return (f > cs && 1.0f - f > cs) ? 2 : 1;
}
template <bool kGuarded>
LSM2D_DEV int cand_classify(const Iso& T, const ProjK& P, float px, float py, float m_t, float m_th, float tn2, float& r, float& md, int& col) {
  r = 0.0f; md = 0.0f; col = -1;
  if (!(__builtin_fabsf(px) < __builtin_huge_valf() && __builtin_fabsf(py) < __builtin_huge_valf())) return 0;      // q is infinite or not a number under every T: r2 fails the gate
  float qx, qy;
  xf_point(T, px, py, qx, qy);
  const float r2 = __builtin_fmaf(qx, qx, qy * qy);
  if (!(r2 >= 1e-30f && r2 <= 1e37f)) return 1;
  float y0;
  r = sqrt_rn_seed(r2, y0);
  const float th = bearing<kGuarded>(qy, qx, r, y0);      // (pure functions of their operands: made in front of the depth tests instead of behind them, the class is the same)
  const float u = __builtin_fmaf(P.K00, th, P.K01);
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(col) : "v"(u));
  const int cl = cand_classify_polar(P, r, th, u, col, m_t, m_th, tn2, md);
  if ((unsigned) col >= (unsigned) P.cols) col = -1;
  return cl;
}
// One point of the BUILD iteration's stream: project_point_stream's operation sequence for the canvas -- and, inside the gate's branch, the point's entry in the
// blockers from the r, th, u and col just made.  blk[] comes out word for word what a pass of its own over the same points with cand_classify made of it:
//  * an interior point (class 2) has rmin + md <= r <= rmax - md with md > 0 (cand_depth_margin: at least 1e-7), so rmin <= r <= rmax for r = sqrt_rn(r2) --
//    which IS r2lo <= r2 <= r2hi (make_projk: the smallest / largest float whose correctly rounded root reaches rmin / stays within rmax; sqrt_rn is monotone) --
//    and a column inside the canvas: every interior point is inside both branches below.  Where rmin + md rounds to rmin (md below half an ulp of it) the point
//    at r == rmin is interior and r2 >= r2lo holds with equality of the roots; the same at rmax.  [r2lo, r2hi] lies inside cand_classify's own [1e-30, 1e37]
//    (ranges are clamped to [1e-15, 1e18] m), and a point with a coordinate that is not finite has an r2 that fails the gate here and class 0 there;
//  * inside the branches r, th, u and col are made by the functions cand_classify calls, on the same operands, with the same kGuarded, and T is the slice's T0;
//  * a point outside them was never interior, so it never touched blk[].
// kQueue (the build with "cand_queue" 1): the PROVISIONAL test.  The function says whether the point is a MAYBE -- whether the collect still has to look at it --
// and everything it does not call a maybe is SETTLED: dropped by the rule (above) whatever the rest of the stream brings.
//  * a class-2 point whose column held, before this point's own entry, a blocker `old` with old < r - md (`old` is what the atomic minimum returns; the all-ones
//    start word is a NaN, the comparison fails, the point stays a maybe).  Blockers only fall: the word the collect reads behind the barrier is the minimum over
//    every entry, `old` among them, and positive floats order like their patterns, so final <= old < r - md in float order -- the very comparison cand_collect_t
//    makes, on the same r and md (made by the same functions on the same operands: the list above), with a smaller left side: the point is dropped there too;
//  * a point with a coordinate that is not finite: class 0 by cand_classify's first line.  (It also keeps the padding slots' indices, which lie behind the
//    cloud's last point, out of the queue: the collect over the queue gathers its points from the cloud itself.)
// Every other streamed point is a maybe: class 2 against a blocker that does not beat it yet, class 1 inside the gates, and every point outside the stream's own
// gates, whose class the stream does not know.  A maybe gets the full rule from cand_collect_queue_t -- cand_classify and the final blocker, as cand_collect_t
// applies them -- so kept = (maybes the rule keeps) = (streamed points the rule keeps): the list is the same SET as the pass over the unit list makes.
template <bool kGuarded, bool kQueue>
LSM2D_DEV bool project_point_stream_blk(const Iso& T, const ProjK& P, float px, float py, int idx, u64* canvas, uint32_t* blk, const int* par) {
  float qx, qy;
  xf_point(T, px, py, qx, qy);
  const float r2 = __builtin_fmaf(qx, qx, qy * qy);
  if (r2 >= P.r2lo && r2 <= P.r2hi) {
    float y0;
    const float r  = sqrt_rn_seed(r2, y0);
    const float th = bearing<kGuarded>(qy, qx, r, y0);
    const float u  = __builtin_fmaf(P.K00, th, P.K01);
    int col;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(col) : "v"(u));
    if ((unsigned) col < (unsigned) P.cols) {
      atomicMin(&canvas[col], ((u64) __float_as_uint(r) << 32) | (u64) (uint32_t) idx);
      // (the margins from k_align's s_cand_par, here and now: as arguments they were loop invariants held in registers across the stream)
      const float m_t = __int_as_float(par[4]), m_th = __int_as_float(par[5]);
      const float tn2 = __builtin_fabsf(T.tx) + __builtin_fabsf(T.ty) + 2.0f * m_t;
      float md;
      if (cand_classify_polar(P, r, th, u, col, m_t, m_th, tn2, md) == 2) {
        const uint32_t old = atomicMin(&blk[col], __float_as_uint(r + md));
        if (kQueue) return !(__uint_as_float(old) < r - md);
      }
    }
    return kQueue;
  }
  return kQueue && __builtin_fabsf(px) < __builtin_huge_valf() && __builtin_fabsf(py) < __builtin_huge_valf();
}
// project_cloud_list_t for the build iteration: the same loads, the same two-buffer look-ahead, project_point_stream_blk for project_point_stream
template <bool kGuarded, int kStride>
LSM2D_DEV void project_cloud_list_blk_t(const float4* __restrict__ lane_xy, int T_steps, const Iso& Tin, const ProjK& Pin, u64* canvas, int tid, int nthreads,
                                        const uint16_t* units, int n_units, int B, uint32_t* blk, const int* par) {
  const Iso T = Tin; ProjK P = Pin;
  asm volatile("" : "+v"(P.K01));
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const unsigned long long pb = reinterpret_cast<unsigned long long>(lane_xy);
  const unsigned pb_hi = (unsigned) __builtin_amdgcn_readfirstlane((int) (pb >> 32));
  const unsigned pb_lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) pb);
  float4* ubase = reinterpret_cast<float4*>(((unsigned long long) pb_hi << 32) | (unsigned long long) pb_lo);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(ubase, (short) 0, 0x7fffffff, 0x00020000);
  const int row_bytes = nthreads * (int) sizeof(float4);
  for (int k = tid; k < n_units; k += kStride) {
    const int code = (int) units[k];
    const int g = code & 511, t0 = (code >> 9) * B;
    const int nsteps = T_steps - t0 < B ? T_steps - t0 : B;
    const int voff = g * (int) sizeof(float4) + t0 * row_bytes;
    int idx = 2 * (g * T_steps + t0);
    auto load = [&](int soff) {
      const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
      return make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
    };
    auto pair = [&](const float4& v, int i) {
      project_point_stream_blk<kGuarded, false>(T, P, v.x, v.y, i, canvas, blk, par);
      project_point_stream_blk<kGuarded, false>(T, P, v.z, v.w, i + 1, canvas, blk, par);
    };
    int t = 0, soff = 0;
    float4 va = load(0);
    for (; t + 2 <= nsteps; t += 2) {
      const float4 vb = load(soff + row_bytes);
      pair(va, idx);
      soff += 2 * row_bytes;
      va = load(soff);
      pair(vb, idx + 2);
      idx += 4;
    }
    if (t < nsteps) pair(va, idx);
  }
}
// The build's pass over the unit list's points: project_cloud_list_t's loads, index arithmetic and two-buffer look-ahead (two steps per trip, the buffers swapping
// roles, the scalar offset advancing unconditionally); every step's pair of points is handed to f(ax, ay, bx, by, t), t the step inside the unit (points 2 t and
// 2 t + 1 of it), and behind a unit's last step end(index of the unit's first point) is called.  The last trip's look-ahead reads one row past the block -- the next
// block's, the next cloud's, or one of the two spare rows ensure_lane_layout() keeps behind the last cloud: the addresses the stream of the same unit has just read,
// and nothing past them -- and is never used.
// The loop over units is the WAVE's, not the lane's: the lanes of a wave hold consecutive entries, so the wave runs trips while its first lane has one, and a lane
// without an entry takes an empty unit (no step, so f is never called for it; its first load reads the cloud's first row, which exists: the list is not empty) and
// arrives at end() with the others.  end() is therefore reached by all 64 lanes of a wave together, once per trip, behind the reconvergence of the step loop: it may
// use cross-lane operations over the full wave.  No barrier stands inside, so waves with different trip counts cannot wait for each other.
static constexpr int kCandSegSteps = 16;      // steps between two end()s: two bits per step fill the 32-bit mask cand_collect_t keeps per lane (B is 14 at 100k points)
template <int kStride, bool kIdx = false, class F, class E>
LSM2D_DEV void cand_for_each_pair(const float4* __restrict__ lane_xy, int T_steps, int tid, int nthreads, const uint16_t* units, int n_units, int B, F f, E end) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const unsigned long long pb = reinterpret_cast<unsigned long long>(lane_xy);
  const unsigned pb_hi = (unsigned) __builtin_amdgcn_readfirstlane((int) (pb >> 32));
  const unsigned pb_lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) pb);
  float4* ubase = reinterpret_cast<float4*>(((unsigned long long) pb_hi << 32) | (unsigned long long) pb_lo);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(ubase, (short) 0, 0x7fffffff, 0x00020000);
  const int row_bytes = nthreads * (int) sizeof(float4);
  const int lane = tid & 63;
  for (int kw = __builtin_amdgcn_readfirstlane(tid - lane); kw < n_units; kw += kStride) {
    const bool have = kw + lane < n_units;
    const int code = have ? (int) units[kw + lane] : 0;
    const int g = code & 511, t0 = (code >> 9) * B;
    const int usteps = !have ? 0 : T_steps - t0 < B ? T_steps - t0 : B;
    // (a unit of more than kCandSegSteps steps -- a cloud of more than 7 x 16 x 1024 points -- is taken in segments, each with its own end(): B is the wave's, so is the trip count)
    for (int s0 = 0; s0 < B; s0 += kCandSegSteps) {
      const int nsteps = usteps - s0 < kCandSegSteps ? usteps - s0 : kCandSegSteps;      // <= 0: nothing of this lane's, the first row again
      const int voff = nsteps > 0 ? g * (int) sizeof(float4) + (t0 + s0) * row_bytes : 0;
      auto load = [&](int soff) { return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0); };
      auto pair = [&](const u32x4& w, int t) {
        if constexpr (kIdx) f(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w), t, 2 * (g * T_steps + t0 + s0));      // (kIdx: and the index end() will get)
        else f(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w), t);
      };
      int t = 0, soff = 0;
      u32x4 va = load(0);
      for (; t + 2 <= nsteps; t += 2) {
        const u32x4 vb = load(soff + row_bytes);
        pair(va, t);
        soff += 2 * row_bytes;
        va = load(soff);
        pair(vb, t + 1);
      }
      if (t < nsteps) pair(va, t);
      end(2 * (g * T_steps + t0 + s0));
    }
  }
}
// Build, the pass behind the stream: every point against the rule; the kept indices are appended to `cand` (any order serves: the z-buffer's minimum does not depend on it) through
// one LDS counter, a wave's keeps of a unit in one add.  The counter goes on counting past `cap`: the caller sees the overflow there and does not use the list.
// Inside a unit a lane only notes what it keeps -- bit 2 t + j of its mask for point j of step t, no cross-lane operation in the step (a lane keeps about 3 of its
// 80 points) -- and behind the unit's last step the wave appends once: cand_for_each_pair brings all 64 lanes to end() together (a lane without a unit with an empty
// mask), so the inclusive scan of the lanes' popcounts (wave_sum63_i's DPP tree: every lane is its source's equal in EXEC) has the wave's total in lane 63, lane 0
// adds it to the counter when it is not zero -- a wave-uniform branch -- and every lane writes the indices of its set bits from base + (its scan - its popcount) on,
// while the position is inside the capacity.  Every kept point is counted exactly once, in the total of its own wave and unit.
LSM2D_DEV int wave_sum63_i(int v);      // (with the wave reductions, further down lsm2d_device.h)
template <bool kGuarded, int kStride>
LSM2D_DEV void cand_collect_t(const float4* __restrict__ lane_xy, int T_steps, const Iso& Tin, const ProjK& Pin, int tid, int nthreads, const uint16_t* units, int n_units, int B,
                              const uint32_t* blk, uint32_t* cand, int cap, int* count, float m_t, float m_th) {
  const Iso T = Tin; const ProjK P = Pin;
  const float tn2 = __builtin_fabsf(T.tx) + __builtin_fabsf(T.ty) + 2.0f * m_t;
  // (a step's two points are classified first and their columns' blockers read side by side, one LDS round trip for the pair instead of one inside each point's
  // branch; a point that is not interior reads word 0 -- blk[] has a word per column -- and does not look at it: the rule's comparison as before)
  unsigned mask = 0;
  cand_for_each_pair<kStride>(lane_xy, T_steps, tid, nthreads, units, n_units, B, [&](float ax, float ay, float bx, float by, int t) {
    float r0, md0, r1, md1; int col0, col1;
    const int cl0 = cand_classify<kGuarded>(T, P, ax, ay, m_t, m_th, tn2, r0, md0, col0);
    const int cl1 = cand_classify<kGuarded>(T, P, bx, by, m_t, m_th, tn2, r1, md1, col1);
    const float b0 = __uint_as_float(blk[cl0 == 2 ? col0 : 0]), b1 = __uint_as_float(blk[cl1 == 2 ? col1 : 0]);
    const bool k0 = cl0 == 2 ? !(b0 < r0 - md0) : cl0 == 1, k1 = cl1 == 2 ? !(b1 < r1 - md1) : cl1 == 1;
    mask |= ((k0 ? 1u : 0u) | (k1 ? 2u : 0u)) << (2 * t);
  }, [&](int idx0) {
    const int n = __popc(mask);
    const int incl = wave_sum63_i(n);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    if (total) {
      int base = 0;
      if ((tid & 63) == 0) base = atomicAdd(count, total);
      int pos = __builtin_amdgcn_readfirstlane(base) + incl - n;
      for (unsigned m = mask; m; m &= m - 1, ++pos)
        if (pos < cap) cand[pos] = (uint32_t) (idx0 + __builtin_ctz(m));
    }
    mask = 0;
  });
}
// Use: the iteration's stream while the list is valid.  Thread t takes entries t, t + kStride, ...: the 8-byte point gathered from the cloud by its index (the
// key's index is that index), the next entry's on its way while this one is projected; project_point_stream as ever.
template <bool kGuarded, int kStride>
LSM2D_DEV void project_candidates_t(const float2* __restrict__ mxy, const Iso& Tin, const ProjK& Pin, u64* canvas, int tid, const uint32_t* cand, int n) {
  const Iso T = Tin; ProjK P = Pin;
  asm volatile("" : "+v"(P.K01));
  int k = tid;
  if (k >= n) return;
  int idx = (int) cand[k];
  float2 p = mxy[idx];
  for (; k < n; k += kStride) {
    const int kn = k + kStride;
    const int idn = (int) cand[kn < n ? kn : k];
    const float2 pn = mxy[idn];
    project_point_stream<kGuarded>(T, P, p.x, p.y, idx, canvas);
    idx = idn; p = pn;
  }
}
// The build as k_align calls it.  `blk`: a word per column -- all ones (a NaN: no blocker, and no comparison with it holds) before the stream, then the minimum over
// the column's interior points of r + md(r), as bits (positive floats order like their patterns) -- the list behind them; capacity and margins are read from
// k_align's s_cand_par (LDS) here and now.  The barriers are everybody's: cand_clear_blockers and one in front of the stream; the stream (made in the same pass
// as the canvas: project_cloud_list_blk), one more, then cand_collect (it does not look at the canvas, so it may stand in front of the bin walk).
// With "cand_queue" 1 the stream is project_cloud_list_blkq and the pass behind the barrier cand_collect_queue (round 30, further down); cand_collect is then the fallback.
LSM2D_HD int cand_blocker_words(int cols) { return (cols + 3) & ~3; }
template <int kStride>
LSM2D_DEV void cand_clear_blockers(const ProjK& P, int tid, uint32_t* blk) { for (int c = tid; c < P.cols; c += kStride) blk[c] = 0xFFFFFFFFu; }
template <int kStride>
LSM2D_DEV void project_cloud_list_blk(const float4* __restrict__ lane_xy, int T_steps, const Iso& T, const ProjK& P, u64* canvas, int tid, int nthreads,
                                      const uint16_t* units, int n_units, int B, uint32_t* blk, const int* par) {
  if (P.tiny_ok) project_cloud_list_blk_t<false, kStride>(lane_xy, T_steps, T, P, canvas, tid, nthreads, units, n_units, B, blk, par);
  else project_cloud_list_blk_t<true, kStride>(lane_xy, T_steps, T, P, canvas, tid, nthreads, units, n_units, B, blk, par);
}
template <int kStride, int kChunks>
LSM2D_DEV void cand_collect(const float4* lane_xy, int T_steps, const Iso& T, const ProjK& P, int tid, const uint16_t* units, int n_units, int B, uint32_t* blk, const int* par, int* count) {
  const int cap = __builtin_amdgcn_readfirstlane(par[1]);
  const float m_t = __int_as_float(__builtin_amdgcn_readfirstlane(par[4])), m_th = __int_as_float(__builtin_amdgcn_readfirstlane(par[5]));
  uint32_t* cand = blk + cand_blocker_words(P.cols);
  if (P.tiny_ok) cand_collect_t<false, kStride>(lane_xy, T_steps, T, P, tid, kChunks, units, n_units, B, blk, cand, cap, count, m_t, m_th);
  else cand_collect_t<true, kStride>(lane_xy, T_steps, T, P, tid, kChunks, units, n_units, B, blk, cand, cap, count, m_t, m_th);
}
// ---- Round 30: the QUEUE of maybes ("cand_queue" 1) -- the collect looks at the points the build's stream could not settle, not at the unit list again ----
// The build iteration's stream on cand_for_each_pair's wave-owned unit loop (the units a lane takes are the ones project_cloud_list_blk_t gives it: entry tid, tid +
// kStride, ...; the canvas and the blockers are minima, no order matters).  A lane notes its maybes (project_point_stream_blk<., true>) in its mask, bit 2 t + j as
// cand_collect_t notes its keeps, and behind the unit the wave appends their indices to the alignment's region of the queue in device memory with cand_collect_t's
// end(): one scan, one add to the LDS counter `qcount`, stores while the position is below `qcap`.  The counter runs on past qcap: the caller sees it there and lets
// cand_collect make the list from the unit list (what the queue holds then is never read).  `queue` and `qcap` are read from LDS here and now, once per unit.
template <bool kGuarded, int kStride>
LSM2D_DEV void project_cloud_list_blkq_t(const float4* __restrict__ lane_xy, int T_steps, const Iso& Tin, const ProjK& Pin, u64* canvas, int tid, int nthreads,
                                         const uint16_t* units, int n_units, int B, uint32_t* blk, const int* par, int* qcount, uint32_t* const* qptr) {
  const Iso T = Tin; ProjK P = Pin;
  asm volatile("" : "+v"(P.K01));
  unsigned mask = 0;
  cand_for_each_pair<kStride, true>(lane_xy, T_steps, tid, nthreads, units, n_units, B, [&](float ax, float ay, float bx, float by, int t, int idx0) {
    const bool m0 = project_point_stream_blk<kGuarded, true>(T, P, ax, ay, idx0 + 2 * t, canvas, blk, par);
    const bool m1 = project_point_stream_blk<kGuarded, true>(T, P, bx, by, idx0 + 2 * t + 1, canvas, blk, par);
    mask |= ((m0 ? 1u : 0u) | (m1 ? 2u : 0u)) << (2 * t);
  }, [&](int idx0) {
    const int n = __popc(mask);
    const int incl = wave_sum63_i(n);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    if (total) {
      int base = 0;
      if ((tid & 63) == 0) base = atomicAdd(qcount, total);
      const int qcap = __builtin_amdgcn_readfirstlane(par[6]);
      const unsigned long long qb = reinterpret_cast<unsigned long long>(*qptr);
      uint32_t* queue = reinterpret_cast<uint32_t*>(((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (qb >> 32)) << 32) |
                                                    (unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) qb));
      // (through a buffer resource over the region's qcap words: the pointer read back from LDS has no address space the compiler knows, a plain store through
      // it is a FLAT one -- and with a flat access pending the stream's loads lose their look-ahead, every wait for one becomes a wait for all)
      const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(queue, (short) 0, qcap > 0 ? qcap * (int) sizeof(uint32_t) : 0, 0x00020000);
      int pos = __builtin_amdgcn_readfirstlane(base) + incl - n;
      for (unsigned m = mask; m; m &= m - 1, ++pos)
        if (pos < qcap) __builtin_amdgcn_raw_buffer_store_b32((unsigned) (idx0 + __builtin_ctz(m)), qrs, pos * (int) sizeof(uint32_t), 0, 0);
    }
    mask = 0;
  });
}
template <int kStride>
LSM2D_DEV void project_cloud_list_blkq(const float4* __restrict__ lane_xy, int T_steps, const Iso& T, const ProjK& P, u64* canvas, int tid, int nthreads,
                                       const uint16_t* units, int n_units, int B, uint32_t* blk, const int* par, int* qcount, uint32_t* const* qptr) {
  if (P.tiny_ok) project_cloud_list_blkq_t<false, kStride>(lane_xy, T_steps, T, P, canvas, tid, nthreads, units, n_units, B, blk, par, qcount, qptr);
  else project_cloud_list_blkq_t<true, kStride>(lane_xy, T_steps, T, P, canvas, tid, nthreads, units, n_units, B, blk, par, qcount, qptr);
}
// The collect over the queue's nq <= qcap <= 32 kStride entries (behind the barrier that ends the stream: the blockers are final, the queue is written).  Thread t
// takes entries t, t + kStride, ... -- project_candidates_t's shape: the 8-byte point gathered from the cloud by its index, the next entry's on its way -- and applies
// cand_collect_t's rule word for word: cand_classify, the column's blocker for a class-2 point, the same comparison.  The keep of trip i is bit i of ONE mask (at
// most 32 trips: the host bounds qcap), and behind the loop the wave appends once, as cand_collect_t's end() does: scan, one add to the counter, which goes on
// counting past `cap`, guarded stores -- of the entries themselves, read back from the queue (a lane keeps about three).  Every lane of the wave reaches the scan.
template <bool kGuarded, int kStride>
LSM2D_DEV void cand_collect_queue_t(const float2* __restrict__ mxy, const Iso& Tin, const ProjK& Pin, int tid, const uint32_t* queue, int nq,
                                    const uint32_t* blk, uint32_t* cand, int cap, int* count, float m_t, float m_th) {
  const Iso T = Tin; const ProjK P = Pin;
  const float tn2 = __builtin_fabsf(T.tx) + __builtin_fabsf(T.ty) + 2.0f * m_t;
  // (the queue through a buffer resource over its nq entries, as the stream wrote it: no flat access)
  const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(queue), (short) 0, nq * (int) sizeof(uint32_t), 0x00020000);
  auto entry = [&](int k) { return (int) __builtin_amdgcn_raw_buffer_load_b32(qrs, k * (int) sizeof(uint32_t), 0, 0); };
  unsigned mask = 0;
  if (tid < nq) {
    int k = tid;
    float2 p = mxy[entry(k)];
    for (unsigned bit = 1u; k < nq; k += kStride, bit <<= 1) {
      const int kn = k + kStride;
      const float2 pn = mxy[entry(kn < nq ? kn : k)];
      float r, md; int col;
      const int cl = cand_classify<kGuarded>(T, P, p.x, p.y, m_t, m_th, tn2, r, md, col);
      const float b = __uint_as_float(blk[cl == 2 ? col : 0]);
      if (cl == 2 ? !(b < r - md) : cl == 1) mask |= bit;
      p = pn;
    }
  }
  const int n = __popc(mask);
  const int incl = wave_sum63_i(n);
  const int total = __builtin_amdgcn_readlane(incl, 63);
  if (total) {
    int base = 0;
    if ((tid & 63) == 0) base = atomicAdd(count, total);
    int pos = __builtin_amdgcn_readfirstlane(base) + incl - n;
    for (unsigned m = mask; m; m &= m - 1, ++pos)
      if (pos < cap) cand[pos] = (uint32_t) entry(tid + kStride * __builtin_ctz(m));
  }
}
template <int kStride>
LSM2D_DEV void cand_collect_queue(const float2* mxy, const Iso& T, const ProjK& P, int tid, const uint32_t* queue, int nq, uint32_t* blk, const int* par, int* count) {
  const int cap = __builtin_amdgcn_readfirstlane(par[1]);
  const float m_t = __int_as_float(__builtin_amdgcn_readfirstlane(par[4])), m_th = __int_as_float(__builtin_amdgcn_readfirstlane(par[5]));
  uint32_t* cand = blk + cand_blocker_words(P.cols);
  if (P.tiny_ok) cand_collect_queue_t<false, kStride>(mxy, T, P, tid, queue, nq, blk, cand, cap, count, m_t, m_th);
  else cand_collect_queue_t<true, kStride>(mxy, T, P, tid, queue, nq, blk, cand, cap, count, m_t, m_th);
}
// has the transform N stayed within (m_t, m_th) of L, with room for what this fp32 evaluation can be off by?  (begin_iteration's expression for s_rebuild; the proof above)
LSM2D_DEV bool cand_pose_within(const Iso& N, const Iso& L, float m_t, float m_th) {
  if (__float_as_uint(N.c) == __float_as_uint(L.c) && __float_as_uint(N.s) == __float_as_uint(L.s)) {      // the same rotation, bit for bit: d = t - t0
    const float ex = N.tx - L.tx, ey = N.ty - L.ty;
    return ex * ex + ey * ey <= m_t * m_t * 0.999999f;
  }
  const float cd = N.c * L.c + N.s * L.s, sd = N.s * L.c - N.c * L.s;
  const float dx = N.tx - (cd * L.tx - sd * L.ty), dy = N.ty - (sd * L.tx + cd * L.ty);
  const float lim = m_t - 4e-7f * (__builtin_fabsf(N.tx) + __builtin_fabsf(N.ty) + __builtin_fabsf(L.tx) + __builtin_fabsf(L.ty));
  return cd > 0.5f && __builtin_fabsf(sd) <= m_th - 3e-7f && lim > 0.0f && dx * dx + dy * dy <= lim * lim * 0.999999f;
}
