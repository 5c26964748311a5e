// lsm2d_k_occupancy.h -- occupancy grids on the device: the points of device-resident clouds ray-traced from their sensor poses into per-cell hit / miss
// counters (lsm2d_occupancy_update), and the counters rendered to what a map consumer reads (lsm2d_occupancy_render).
// Part of lsm2d_kernels.h (included there inside namespace lsm2d).
//
// A capability of this build, not of the reference: the reference tree has no grid mapper.  Meaning: PARITY.md section 3, item 17c; everything behind the
// transform is integer arithmetic, so the result is unique whatever the order of the sums.  The chain, every step a launch of its own on the lane's stream:
//   k_occ_rays    a thread per concatenated point: its input by binary search in the call's offset table (as k_vox_keys), the point moved by the input's pose
//                 (xf_point: lsm2d_merge_scene's transform; no pose: the bits copied), the four cell coordinates floorf((v - o) * inv) with the difference and
//                 the product rounded separately, and a 16-byte ray record {x0, y0, x1, y1} to scratch -- or a marker for a point that gives no ray (a
//                 coordinate outside [-2^20, 2^20), NaN and Inf among them, or a ray longer than kOccMaxRayCells).  Per (wave, input) the bounding box of the
//                 live rays and the live / dropped counts are reduced over the wave and added with ONE integer atomic each to the input's box and the
//                 grid's counts.
//   k_occ_tiles   a workgroup of 256 threads per (grid, tile of kOccTile x kOccTile cells).  The host lists a grid's inputs contiguously; the workgroup tests
//                 256 input boxes a round against its tile and keeps the inputs that can touch it.  A workgroup no box touches leaves before it zeroes
//                 anything.  For a kept input the threads stride over its ray records: reject by the ray's own box, the step interval [i_lo, i_hi] whose major
//                 coordinate lies in the tile in O(1), the minor coordinate started from the closed form (ONE 32-bit division per (ray, tile)) and carried by
//                 its remainder, at most kOccTile steps, each a no-return LDS atomic into one of two kOccTile x kOccTile uint32 arrays (32 KB).  After one
//                 barrier a thread per cell adds the non-zero LDS counts into the grid: a plain 8-byte load, a saturating add in 64 bits, a plain store -- a
//                 tile has exactly ONE owner per launch.
//   k_occ_render  a thread per cell: -1 below min_visits, else rintf(100 * hits / (hits + misses)).
//   k_occ_put     a thread per cell: host counters (planar) into the interleaved cells, a NULL array leaving its counter (lsm2d_gridset_upload).
// The walk (item 17c.3): with L the major extent and a the minor extent, step i = 0 .. L is the cell (m0 + s i, n0 + s' ((2 i a + L) / (2 L))), the division
// integer; 2 * 32767^2 + 32767 < 2^31.  Steps 0 .. L - 1 are misses, step L is the hit; a cell outside the grid adds nothing and the ray goes on.
// The walk stands ONCE, in occ_walk; every tile kernel calls it and says only what a hit and a miss do to its LDS.  k_occ_tiles is k_occ_tiles<false>.
// From raw scans (lsm2d_occupancy_update_scans, PARITY.md section 3, item 17d) the chain is
//   k_occ_beams        a thread per (scan, beam), i = j * n_beams + c over the scans in the host's grid-by-grid order (regular offsets: no search).  The beam's
//                      class from its range (dropped / HIT of length r / CLEAR of length trace_range), the end point as ONE fp32 product per coordinate with
//                      the host's direction table (k_preprocess_scans' product), then k_occ_rays' transform, cells and tests (occ_ray_cells).  The 16-byte
//                      record carries the ray's kind in bit 22 of its last word: y1 is stored as (y1 & 0x3fffff) | kind << 22 and sign-extended from 22 bits
//                      on read (a cell coordinate needs 21).  Per (wave, scan) -- a wave straddles scans whenever n_beams is no multiple of 64 -- the box of
//                      the live rays of BOTH kinds (occ_wave_box, as in k_occ_rays) and the three counts are reduced over the wave and added by the leader lane.
//   k_occ_tiles<true>  the same kernel over records that carry a kind: a step is a hit iff i == L and the ray is a HIT ray; a CLEAR ray adds a miss on every
//                      step 0 .. L.
// Into a log-odds grid set (0.7.14, PARITY.md section 3, item 17e: a cell is {int32 value, uint32 observed}) the second kernel of either chain is
//   k_occ_tiles_logodds<kKinds>  the same workgroup per (grid, tile), the same box rounds and the same walk, but the scans are applied ONE AFTER THE OTHER in
//                      ascending input order and every cell gets ONE vote per scan.  The kept list is compacted in order (a ballot per wave, the four waves'
//                      counts through LDS).  On the first kept input the tile's value / observed words come from the grid into LDS (the 2 x 16 KB of the
//                      two count arrays).  Per kept scan the walk sets the cell's bit in a hit mask or a miss mask (4096 bits each, no-return LDS OR); after a
//                      barrier each thread takes 16 bits of both masks, applies the clamped vote to the set bits (a hit bit wins) and clears its bits; a
//                      second barrier ends the scan.  At the end a cell of the cut tile whose bits differ from the grid's is stored, 8 bytes, plain.
//   k_occ_decay        a thread per cell: an observed cell's value moves toward 0 by `amount`, never past it (lsm2d_occupancy_decay).
//   k_occ_render_logodds  a thread per cell: -1 below min_scans, else how many of the 100 thresholds in the kernel's arguments are <= value (branch-free).
// The typed upload goes through k_occ_put with the words reinterpreted: the kernel is untouched.
// Every index is checked against its array; a failed check sets the fault word and the host answers LSM2D_DEVICE_ERROR.  No global atomics on the grid, no
// workgroup waits for another, no float atomics, no scratch memory.  Tiles overlapped by many scans work longest: the known imbalance, measured in DESIGN.md
// section 8, not engineered around.
#pragma once

static constexpr int kOccTile = 64;                    // cells per side of a tile: what ONE workgroup owns ("occupancy_tile")
static constexpr int kOccBlock = 256;                  // threads of a tile's workgroup = input boxes tested per round
static constexpr int kOccMaxSide = 16384;              // LSM2D_OCCUPANCY_MAX_SIDE
static constexpr int kOccMaxCells = 1 << 28;           // LSM2D_OCCUPANCY_MAX_CELLS
static constexpr int kOccMaxRays = 1 << 24;            // LSM2D_OCCUPANCY_MAX_RAYS
static constexpr int kOccMaxRayCells = 32767;          // LSM2D_OCCUPANCY_MAX_RAY_CELLS
static constexpr int kOccDropped = -0x7fffffff - 1;    // x0 of a record whose point gave no ray (no cell coordinate reaches it)
static constexpr int kOccKindShift = 22;               // a record with kinds (k_occ_beams): w = (y1 & 0x3fffff) | kind << 22
static constexpr int kOccHit = 0, kOccClear = 1;       // a ray's kind: its last step is a hit / every step is a miss

struct OccInput { Iso T; float sx, sy; int32_t start, grid, has_pose, pad; };      // per input, in the host's order (grid by grid): transform, ray start, where its points begin
struct OccGeo { float ox, oy, inv; int32_t w, h, n_grids, tiles_x, tiles_y; };

struct OccRaysArgs {
  const float2* xy;                                 // the source set
  const OccInput* inputs; const int32_t* offset;    // [n_inputs], [n_inputs + 1] concatenation offsets
  int32_t n_inputs, n;                              // n: concatenated points
  OccGeo G;
  int4* rays;                                       // [n]
  int32_t* box;                                     // [n_inputs][4] = {xmin, ymin, xmax, ymax} of the input's live rays, uploaded as {max, max, min, min}
  int32_t* n_rays; int32_t* n_dropped;              // [n_grids]
  int32_t* fault;
};

LSM2D_DEV float occ_cell(float v, float o, float inv) { return __builtin_floorf(__fmul_rn(__fsub_rn(v, o), inv)); }
LSM2D_DEV bool occ_in_range(float c) { return c >= -1048576.0f && c < 1048576.0f; }      // (NaN fails)

// the cells of a ray from (sx, sy) to (x, y), and whether it is live: all four coordinates in range and no more than kOccMaxRayCells steps
LSM2D_DEV bool occ_ray_cells(const OccGeo& G, float sx, float sy, float x, float y, int& x0, int& y0, int& x1, int& y1) {
  const float fx0 = occ_cell(sx, G.ox, G.inv), fy0 = occ_cell(sy, G.oy, G.inv);
  const float fx1 = occ_cell(x, G.ox, G.inv), fy1 = occ_cell(y, G.oy, G.inv);
  bool live = false;
  if (occ_in_range(fx0) && occ_in_range(fy0) && occ_in_range(fx1) && occ_in_range(fy1)) {
    x0 = (int) fx0; y0 = (int) fy0; x1 = (int) fx1; y1 = (int) fy1;
    const int ax = x1 > x0 ? x1 - x0 : x0 - x1, ay = y1 > y0 ? y1 - y0 : y0 - y1;
    live = (ax > ay ? ax : ay) <= kOccMaxRayCells;
  }
  return live;
}

// the box {xmin, ymin, xmax, ymax} of the rays of the wave's lanes with `lv` set, in every lane ({max, max, min, min} if there is none)
LSM2D_DEV int4 occ_wave_box(bool lv, int x0, int y0, int x1, int y1) {
  int bx0 = lv ? (x0 < x1 ? x0 : x1) : 0x7fffffff, by0 = lv ? (y0 < y1 ? y0 : y1) : 0x7fffffff;
  int bx1 = lv ? (x0 > x1 ? x0 : x1) : kOccDropped, by1 = lv ? (y0 > y1 ? y0 : y1) : kOccDropped;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(bx0, o), b = __shfl_xor(by0, o), c = __shfl_xor(bx1, o), d = __shfl_xor(by1, o);
    bx1 = c > bx1 ? c : bx1; by1 = d > by1 ? d : by1; bx0 = a < bx0 ? a : bx0; by0 = b < by0 ? b : by0;      // (the maxima first: two instructions fewer per kernel)
  }
  return make_int4(bx0, by0, bx1, by1);
}

LSM2D_DEV void occ_box_add(int32_t* box, int4 b) { atomicMin(box, b.x); atomicMin(box + 1, b.y); atomicMax(box + 2, b.z); atomicMax(box + 3, b.w); }

__global__ __launch_bounds__(256) void k_occ_rays(const OccRaysArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool in_range = i < A.n;
  int k = -1, grid = -1, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  bool live = false;
  if (in_range) {
    int lo = 0, hi = A.n_inputs;      // the last input k with offset[k] <= i (empty inputs share their successor's offset and lose)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.offset[mid] <= i) lo = mid; else hi = mid; }
    const OccInput in = A.inputs[lo];
    k = lo; grid = in.grid;
    const float2 p = A.xy[(size_t) in.start + (size_t) (i - A.offset[lo])];
    float x = p.x, y = p.y;
    if (in.has_pose) xf_point(in.T, p.x, p.y, x, y);
    live = occ_ray_cells(A.G, in.sx, in.sy, x, y, x0, y0, x1, y1);
    A.rays[i] = live ? make_int4(x0, y0, x1, y1) : make_int4(kOccDropped, 0, 0, 0);
  }
  // per (wave, input): the box of the live rays and the two counts, reduced over the wave; one lane adds them
  u64 todo = __ballot(in_range);
  while (todo) {
    const int leader = __ffsll((long long) todo) - 1;
    const int kk = __shfl(k, leader);
    const bool mine = in_range && k == kk, lv = mine && live;
    const int4 box = occ_wave_box(lv, x0, y0, x1, y1);
    const u64 m_mine = __ballot(mine);
    const int nl = __popcll(__ballot(lv)), nd = __popcll(m_mine) - nl;
    if (lane == leader) {
      if (kk < 0 || kk >= A.n_inputs || grid < 0 || grid >= A.G.n_grids) *A.fault = 1;
      else {
        if (nl) { occ_box_add(A.box + 4 * (size_t) kk, box); atomicAdd(A.n_rays + grid, nl); }
        if (nd) atomicAdd(A.n_dropped + grid, nd);
      }
    }
    todo &= ~m_mine;
  }
}

struct OccBeamsArgs {
  const float* ranges; const float2* beam_dir;      // [n_ranges] the scans' ranges as the caller laid them out, [n_beams] the host's direction table
  const OccInput* inputs;                           // [n_inputs] scans in the host's order; start: where the scan's ranges begin
  int32_t n_inputs, n_beams, n, n_ranges;           // n = n_inputs * n_beams
  float rmin, rmax, trace; int32_t clear_no_return;
  OccGeo G;
  int4* rays;                                       // [n]: {x0, y0, x1, (y1 & 0x3fffff) | kind << 22}, or {kOccDropped, 0, 0, 0}
  int32_t* box;                                     // [n_inputs][4], as OccRaysArgs
  int32_t* n_hit; int32_t* n_clear; int32_t* n_dropped;      // [n_grids]
  int32_t* fault;
};

__global__ __launch_bounds__(256) void k_occ_beams(const OccBeamsArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool in_range = i < A.n;
  int k = -1, grid = -1, kind = -1, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  bool live = false, bad = false;
  if (in_range) {
    k = (int) ((unsigned) i / (unsigned) A.n_beams);
    const int c = i - k * A.n_beams;
    if (k >= A.n_inputs) bad = true;
    else {
      const OccInput in = A.inputs[k];
      grid = in.grid;
      if (in.start < 0 || in.start > A.n_ranges - A.n_beams) bad = true;
      else {
        const float r = A.ranges[(size_t) in.start + (size_t) c];
        const float2 d = A.beam_dir[c];
        float len = 0.0f;      // item 17d: the beam's class, the tests in this order
        if (!(r >= A.rmin)) kind = -1;
        else if (r <= A.trace) { kind = kOccHit; len = r; }
        else if (r <= A.rmax || A.clear_no_return) { kind = kOccClear; len = A.trace; }
        if (kind >= 0) {
          const float px = __fmul_rn(len, d.x), py = __fmul_rn(len, d.y);
          float x = px, y = py;
          if (in.has_pose) xf_point(in.T, px, py, x, y);
          live = occ_ray_cells(A.G, in.sx, in.sy, x, y, x0, y0, x1, y1);
        }
      }
    }
    A.rays[i] = live ? make_int4(x0, y0, x1, (int) (((uint32_t) y1 & 0x3fffffu) | ((uint32_t) kind << kOccKindShift))) : make_int4(kOccDropped, 0, 0, 0);
  }
  // per (wave, scan): the box of the live rays of both kinds and the three counts, reduced over the wave; one lane adds them
  u64 todo = __ballot(in_range);
  while (todo) {
    const int leader = __ffsll((long long) todo) - 1;
    const int kk = __shfl(k, leader);
    const bool mine = in_range && k == kk, lv = mine && live;
    const int4 box = occ_wave_box(lv, x0, y0, x1, y1);
    const u64 m_mine = __ballot(mine);
    const bool any_bad = __ballot(mine && bad) != 0;
    const int nh = __popcll(__ballot(lv && kind == kOccHit)), nc = __popcll(__ballot(lv && kind == kOccClear)), nd = __popcll(m_mine) - nh - nc;
    if (lane == leader) {
      if (any_bad || kk < 0 || kk >= A.n_inputs || grid < 0 || grid >= A.G.n_grids) *A.fault = 1;
      else {
        if (nh + nc) occ_box_add(A.box + 4 * (size_t) kk, box);
        if (nh) atomicAdd(A.n_hit + grid, nh);
        if (nc) atomicAdd(A.n_clear + grid, nc);
        if (nd) atomicAdd(A.n_dropped + grid, nd);
      }
    }
    todo &= ~m_mine;
  }
}

struct OccTilesArgs {
  const int4* rays; const int32_t* offset; const int32_t* box;      // [n], [n_inputs + 1], [n_inputs][4]
  const int32_t* grid_first;                                        // [n_grids + 1]: grid g's inputs are grid_first[g] .. grid_first[g + 1]
  int32_t n_inputs, n;
  OccGeo G;
  uint2* cells;                                                     // [n_grids][h][w] = {hits, misses}
  int32_t* fault;
  unsigned long long* stamps;                                       // [workgroups] or NULL: 10 ns ticks a workgroup that had work lived (kernel timing on: diagnostics)
};

// The walk of ONE ray record over ONE tile [cx0, cx1] x [cy0, cy1] (both ends inclusive, cut to the grid): hit(c) or miss(c) for every step whose cell c (row-major
// in the uncut tile) lies in it.  The only place that knows item 17c.3's step arithmetic and, with kKinds, the record's kind bits (k_occ_beams).  Measured when
// the three copies became this one: at equal size and resources the compiler states the box reject's compare chain in its complementary form, commutes the
// operands of one v_mad_u64_u32 and swaps two registers of the remainder carry (profiles/r38).
template <bool kKinds, class Hit, class Miss>
LSM2D_DEV void occ_walk(int4 R, const int cx0, const int cy0, const int cx1, const int cy1, int32_t* const fault, Hit hit, Miss miss) {
  if (R.x == kOccDropped) return;
  bool hit_ray = true;
  if (kKinds) {
    hit_ray = ((uint32_t) R.w >> kOccKindShift) == (uint32_t) kOccHit;      // (a CLEAR ray: a miss on every step)
    R.w = (int) ((uint32_t) R.w << (32 - kOccKindShift)) >> (32 - kOccKindShift);      // y1, sign-extended from 22 bits
  }
  if ((R.x > R.z ? R.x : R.z) < cx0 || (R.x < R.z ? R.x : R.z) > cx1 || (R.y > R.w ? R.y : R.w) < cy0 || (R.y < R.w ? R.y : R.w) > cy1) return;
  const int dx = R.z - R.x, dy = R.w - R.y;
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  const bool xm = ax >= ay;      // a tie is x-major
  const int L = xm ? ax : ay, a = xm ? ay : ax;
  const int m0 = xm ? R.x : R.y, n0 = xm ? R.y : R.x;
  const int sm = (xm ? dx : dy) < 0 ? -1 : 1, sn = (xm ? dy : dx) < 0 ? -1 : 1;
  const int mlo = xm ? cx0 : cy0, mhi = xm ? cx1 : cy1, nlo = xm ? cy0 : cx0, nhi = xm ? cy1 : cx1;
  int ilo = sm > 0 ? mlo - m0 : m0 - mhi, ihi = sm > 0 ? mhi - m0 : m0 - mlo;      // the steps whose major coordinate lies in the tile
  ilo = ilo > 0 ? ilo : 0; ihi = ihi < L ? ihi : L;
  if (ilo > ihi) return;
  const uint32_t den = L ? 2u * (uint32_t) L : 1u;      // (L == 0: a == 0, the one step has the minor offset 0)
  const uint32_t num = 2u * (uint32_t) ilo * (uint32_t) a + (uint32_t) L;
  uint32_t q = num / den, rem = num - q * den;
  for (int i = ilo; i <= ihi; ++i) {      // at most kOccTile steps
    const int nn = n0 + sn * (int) q;
    if (nn >= nlo && nn <= nhi) {
      const int mm = m0 + sm * i;
      const int c = ((xm ? nn : mm) - cy0) * kOccTile + ((xm ? mm : nn) - cx0);
      if (c < 0 || c >= kOccTile * kOccTile) *fault = 1;
      else if (i == L && hit_ray) hit(c);
      else miss(c);
    }
    rem += 2u * (uint32_t) a;      // (2 a <= den: one carry at the most)
    if (rem >= den) { rem -= den; ++q; }
  }
}

// kKinds: the records carry a kind (k_occ_beams'), else every ray is a HIT ray (k_occ_rays')
template <bool kKinds>
__global__ __launch_bounds__(kOccBlock) void k_occ_tiles(const OccTilesArgs A) {
  __shared__ uint32_t s_hits[kOccTile * kOccTile];
  __shared__ uint32_t s_miss[kOccTile * kOccTile];
  __shared__ int32_t s_list[kOccBlock];
  __shared__ int32_t s_n;
  const int tid = threadIdx.x;
  const unsigned long long t_start = A.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;
  const int tpg = A.G.tiles_x * A.G.tiles_y;
  const int g = (int) (blockIdx.x / (unsigned) tpg), t = (int) (blockIdx.x - (unsigned) g * (unsigned) tpg);
  if (g >= A.G.n_grids) { if (tid == 0) *A.fault = 1; return; }
  const int ty = t / A.G.tiles_x, tx = t - ty * A.G.tiles_x;
  const int cx0 = tx * kOccTile, cy0 = ty * kOccTile;      // the tile's cells, both ends inclusive, cut to the grid
  const int cx1 = (cx0 + kOccTile < A.G.w ? cx0 + kOccTile : A.G.w) - 1, cy1 = (cy0 + kOccTile < A.G.h ? cy0 + kOccTile : A.G.h) - 1;
  const int first = A.grid_first[g], last = A.grid_first[g + 1];
  if (first < 0 || last > A.n_inputs || first > last) { if (tid == 0) *A.fault = 1; return; }
  bool zeroed = false;
  for (int base = first; base < last; base += kOccBlock) {
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int k = base + tid;
    if (k < last) {
      const int4 B = *(const int4*) (A.box + 4 * (size_t) k);
      if (B.x <= cx1 && B.z >= cx0 && B.y <= cy1 && B.w >= cy0) s_list[atomicAdd(&s_n, 1)] = k;      // (an input without a live ray keeps {max, max, min, min})
    }
    __syncthreads();
    const int m = s_n;
    if (m > 0 && !zeroed) {
      for (int c = tid; c < kOccTile * kOccTile; c += kOccBlock) { s_hits[c] = 0u; s_miss[c] = 0u; }
      __syncthreads();
      zeroed = true;
    }
    for (int j = 0; j < m; ++j) {
      const int kk = s_list[j];
      const int b = A.offset[kk], e = A.offset[kk + 1];
      if (b < 0 || e > A.n || b > e) { *A.fault = 1; continue; }
      for (int r = b + tid; r < e; r += kOccBlock)
        occ_walk<kKinds>(A.rays[r], cx0, cy0, cx1, cy1, A.fault, [&](int c) { atomicAdd(&s_hits[c], 1u); }, [&](int c) { atomicAdd(&s_miss[c], 1u); });
    }
    __syncthreads();
  }
  if (!zeroed) return;
  for (int c = tid; c < kOccTile * kOccTile; c += kOccBlock) {
    const uint32_t hh = s_hits[c], mm = s_miss[c];
    if (!(hh | mm)) continue;
    const int cx = cx0 + (c % kOccTile), cy = cy0 + (c / kOccTile);
    if (cx > cx1 || cy > cy1) { *A.fault = 1; continue; }      // (the walk adds inside the cut tile only)
    uint2* const cell = A.cells + (((size_t) g * (size_t) A.G.h + (size_t) cy) * (size_t) A.G.w + (size_t) cx);
    const uint2 v = *cell;
    const u64 nh = (u64) v.x + hh, nm = (u64) v.y + mm;
    *cell = make_uint2(nh > 0xffffffffull ? 0xffffffffu : (uint32_t) nh, nm > 0xffffffffull ? 0xffffffffu : (uint32_t) nm);
  }
  if (A.stamps && tid == 0) A.stamps[blockIdx.x] = __builtin_amdgcn_s_memrealtime() - t_start;
}

struct OccRenderArgs { const uint2* cells; long long n; int32_t min_visits; int8_t* out; };

__global__ __launch_bounds__(256) void k_occ_render(const OccRenderArgs A) {
  const long long c = (long long) blockIdx.x * 256 + threadIdx.x;
  if (c >= A.n) return;
  const uint2 v = A.cells[c];
  const u64 visits = (u64) v.x + (u64) v.y;
  const u64 need = A.min_visits > 1 ? (u64) A.min_visits : 1ull;
  int8_t o = -1;
  if (visits >= need) {
    const float p = (float) v.x / (float) visits;
    o = (int8_t) __builtin_rintf(__fmul_rn(100.0f, p));
  }
  A.out[c] = o;
}

struct OccPutArgs { uint2* cells; const uint32_t* hits; const uint32_t* misses; long long n; };

__global__ __launch_bounds__(256) void k_occ_put(const OccPutArgs A) {
  const long long c = (long long) blockIdx.x * 256 + threadIdx.x;
  if (c >= A.n) return;
  uint2 v = A.cells[c];
  if (A.hits) v.x = A.hits[c];
  if (A.misses) v.y = A.misses[c];
  A.cells[c] = v;
}

// ---- log-odds grid sets (0.7.14; PARITY.md section 3, item 17e) -----------------------------------------------------------------------------------------
struct OccLogoddsArgs { OccTilesArgs T; int32_t l_hit, l_miss, l_min, l_max; };      // T.cells: {value (int32 bits), observed}

static constexpr int kOccMaskWords = kOccTile * kOccTile / 32;      // a tile's cells as bits

// The walk is occ_walk, as in k_occ_tiles<kKinds>.  What differs is the accumulation: a step sets a bit, and the bits of ONE scan become one clamped vote per
// cell before the next scan's walk begins.
template <bool kKinds>
__global__ __launch_bounds__(kOccBlock) void k_occ_tiles_logodds(const OccLogoddsArgs P) {
  __shared__ int32_t s_val[kOccTile * kOccTile];
  __shared__ uint32_t s_obs[kOccTile * kOccTile];
  __shared__ uint32_t s_hitm[kOccMaskWords];
  __shared__ uint32_t s_missm[kOccMaskWords];
  __shared__ int32_t s_list[kOccBlock];
  __shared__ int32_t s_wcnt[kOccBlock / 64];
  const OccTilesArgs& A = P.T;
  const int tid = threadIdx.x, wave = tid >> 6;
  const unsigned long long t_start = A.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;
  const int tpg = A.G.tiles_x * A.G.tiles_y;
  const int g = (int) (blockIdx.x / (unsigned) tpg), t = (int) (blockIdx.x - (unsigned) g * (unsigned) tpg);
  if (g >= A.G.n_grids) { if (tid == 0) *A.fault = 1; return; }
  const int ty = t / A.G.tiles_x, tx = t - ty * A.G.tiles_x;
  const int cx0 = tx * kOccTile, cy0 = ty * kOccTile;      // the tile's cells, both ends inclusive, cut to the grid
  const int cx1 = (cx0 + kOccTile < A.G.w ? cx0 + kOccTile : A.G.w) - 1, cy1 = (cy0 + kOccTile < A.G.h ? cy0 + kOccTile : A.G.h) - 1;
  const int first = A.grid_first[g], last = A.grid_first[g + 1];
  if (first < 0 || last > A.n_inputs || first > last) { if (tid == 0) *A.fault = 1; return; }
  uint2* const grid_cells = A.cells + (size_t) g * (size_t) A.G.h * (size_t) A.G.w;
  bool loaded = false;
  for (int base = first; base < last; base += kOccBlock) {
    // the kept inputs of this round in ASCENDING order: a ballot per wave, the waves' counts through LDS (rounds ascend by themselves)
    const int k = base + tid;
    bool keep = false;
    if (k < last) {
      const int4 B = *(const int4*) (A.box + 4 * (size_t) k);
      keep = B.x <= cx1 && B.z >= cx0 && B.y <= cy1 && B.w >= cy0;      // (an input without a live ray keeps {max, max, min, min})
    }
    const u64 bal = __ballot(keep);
    if ((tid & 63) == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, m = 0;
#pragma unroll
    for (int w = 0; w < kOccBlock / 64; ++w) { const int c = s_wcnt[w]; before += w < wave ? c : 0; m += c; }
    if (keep) s_list[before + __popcll(bal & ((1ull << (tid & 63)) - 1ull))] = k;      // (before + rank < m <= kOccBlock)
    if (m > 0 && !loaded) {
      for (int c = tid; c < kOccTile * kOccTile; c += kOccBlock) {
        const int cx = cx0 + (c % kOccTile), cy = cy0 + (c / kOccTile);
        uint2 v = make_uint2(0u, 0u);      // (outside the cut tile: never voted on, never stored)
        if (cx <= cx1 && cy <= cy1) v = grid_cells[(size_t) cy * (size_t) A.G.w + (size_t) cx];
        s_val[c] = (int32_t) v.x; s_obs[c] = v.y;
      }
      if (tid < kOccMaskWords) { s_hitm[tid] = 0u; s_missm[tid] = 0u; }
      loaded = true;
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const int kk = s_list[j];
      const int b = A.offset[kk], e = A.offset[kk + 1];
      if (b < 0 || e > A.n || b > e) { *A.fault = 1; continue; }      // (the same for every thread: no barrier is left out by some)
      for (int r = b + tid; r < e; r += kOccBlock)
        occ_walk<kKinds>(A.rays[r], cx0, cy0, cx1, cy1, A.fault, [&](int c) { atomicOr(&s_hitm[c >> 5], 1u << (c & 31)); }, [&](int c) { atomicOr(&s_missm[c >> 5], 1u << (c & 31)); });
      __syncthreads();
      // one vote per cell: thread tid owns cells 16 tid .. 16 tid + 15, half a word of each mask, reads it, votes and clears it -- nobody else touches them
      {
        const uint32_t sh = (uint32_t) (tid & 1) * 16u;
        const uint32_t hw = s_hitm[tid >> 1], mw = s_missm[tid >> 1];
        const uint32_t hb = (hw >> sh) & 0xffffu;
        uint32_t any = hb | ((mw >> sh) & 0xffffu);
        if (any) {
          atomicAnd(&s_hitm[tid >> 1], ~(0xffffu << sh)); atomicAnd(&s_missm[tid >> 1], ~(0xffffu << sh));      // (the word's other half is its neighbour's)
          while (any) {
            const int bit = __ffs((int) any) - 1;
            any &= any - 1u;
            const int c = tid * 16 + bit;
            long long v = (long long) s_val[c] + (long long) (((hb >> bit) & 1u) ? P.l_hit : P.l_miss);      // the hit wins
            v = v < (long long) P.l_min ? (long long) P.l_min : v; v = v > (long long) P.l_max ? (long long) P.l_max : v;
            s_val[c] = (int32_t) v;
            const uint32_t o = s_obs[c];
            s_obs[c] = o == 0xffffffffu ? o : o + 1u;
          }
        }
      }
      __syncthreads();
    }
  }
  if (!loaded) return;
  for (int c = tid; c < kOccTile * kOccTile; c += kOccBlock) {
    const int cx = cx0 + (c % kOccTile), cy = cy0 + (c / kOccTile);
    if (cx > cx1 || cy > cy1) continue;
    uint2* const cell = grid_cells + ((size_t) cy * (size_t) A.G.w + (size_t) cx);
    const uint2 was = *cell, now = make_uint2((uint32_t) s_val[c], s_obs[c]);
    if (was.x != now.x || was.y != now.y) *cell = now;      // (a voted cell whose bits did not move -- clamped and saturated -- needs no store)
  }
  if (A.stamps && tid == 0) A.stamps[blockIdx.x] = __builtin_amdgcn_s_memrealtime() - t_start;
}

struct OccDecayArgs { uint2* cells; long long n; int32_t amount; };

__global__ __launch_bounds__(256) void k_occ_decay(const OccDecayArgs A) {
  const long long c = (long long) blockIdx.x * 256 + threadIdx.x;
  if (c >= A.n) return;
  const uint2 cell = A.cells[c];
  if (cell.y == 0u) return;      // unknown: keeps its bits
  const long long v = (long long) (int32_t) cell.x;
  const long long w = v > 0 ? (v - A.amount > 0 ? v - A.amount : 0) : (v < 0 ? (v + A.amount < 0 ? v + A.amount : 0) : 0);
  if (w != v) A.cells[c] = make_uint2((uint32_t) (int32_t) w, cell.y);
}

struct OccRenderLogoddsArgs { const uint2* cells; long long n; int32_t min_scans; int8_t* out; int32_t threshold[100]; };

__global__ __launch_bounds__(256) void k_occ_render_logodds(const OccRenderLogoddsArgs A) {
  const long long c = (long long) blockIdx.x * 256 + threadIdx.x;
  if (c >= A.n) return;
  const uint2 cell = A.cells[c];
  const int32_t v = (int32_t) cell.x;
  const uint32_t need = A.min_scans > 1 ? (uint32_t) A.min_scans : 1u;
  int count = 0;
#pragma unroll
  for (int j = 0; j < 100; ++j) count += A.threshold[j] <= v ? 1 : 0;      // the table IS the rendering: no exponential here
  A.out[c] = cell.y >= need ? (int8_t) count : (int8_t) -1;
}
