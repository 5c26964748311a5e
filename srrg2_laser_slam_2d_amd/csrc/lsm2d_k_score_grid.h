// lsm2d_k_score_grid.h -- a grid of pose hypotheses made, refined and ranked level by level without the host (lsm2d_score_grid_select).
// Part of lsm2d_kernels.h (included there inside namespace lsm2d, behind the selection).
//
// The hypotheses of a level lie in device memory as a pose block [n][3] and an origin array [n] (the level-0 cell every descendant came from); the scoring
// (k_score_aligner_items ... k_score_combine) and the selection (k_select_*) run over them as they are.  Four small kernels stand round those:
//   k_grid_level0     a thread per slot of the call's LARGEST level: thread i < n0 writes cell i's pose and origin; every thread writes entry i of the
//                     constant cloud index tables of the sets that hold several clouds, where k_score_aligner_items reads them at every level.
//   k_grid_children   a thread per slot of a level l >= 1: slot j * R + c is child c of parent j, the j-th best of the previous level's selection, read from
//                     the region that selection left on the device.  A slot of a parent j >= n_selected, a PAD, repeats parent 0's child (the grid's centre
//                     when nothing was selected): valid inputs for the scoring, so every workgroup of its launches has work of the usual kind.
//   k_grid_mask_pads  behind k_score_combine: the `active` word of every pad's combined row becomes 0, which the selection rejects whatever the thresholds
//                     are (select_key<CombRow>) -- a pad is never accepted, counted, ranked or returned.
//   k_grid_finish     the per-level headers, and the poses and origins of the last level's selection, into the region that goes down.
// A coordinate is base + (o * s), o = i - 0.5 (n - 1): the product rounded to fp32, then the sum (__fmul_rn / __fadd_rn: never an fma, whatever the
// contraction flags are).  Words that are only moved are moved as bits.  No float atomics, no workgroup waits for another, no scratch memory.
#pragma once

static constexpr int kGridMaxLevels = 4;          // LSM2D_GRID_MAX_LEVELS
static constexpr int kGridMaxItems = 1 << 18;     // LSM2D_GRID_MAX_ITEMS

// o(i, n) = i - 0.5 (n - 1): exact in fp32 for every n the ABI admits (n <= 2^18: halves below 2^17)
LSM2D_DEV float grid_offset(int i, int n) { return __fsub_rn((float) i, __fmul_rn(0.5f, (float) (n - 1))); }
LSM2D_DEV float grid_coord(float base, float o, float s) { return __fadd_rn(base, __fmul_rn(o, s)); }

struct GridLevel0Args {
  float center[3], step[3];
  int32_t nx, ny, nt, n0;        // n0 = nx ny nt
  int32_t n_cap, n_slices;       // slots of the largest level: the index tables' length
  float* pose; int32_t* origin;  // [n0][3], [n0]
  int32_t* f_table[kMaxSlices]; int32_t* m_table[kMaxSlices];      // [n_cap] per slice, or nullptr (a one-cloud set needs none)
  int32_t f_cloud[kMaxSlices], m_cloud[kMaxSlices];
};

__global__ __launch_bounds__(256) void k_grid_level0(const GridLevel0Args A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_cap) return;
  for (int s = 0; s < A.n_slices; ++s) {
    if (A.f_table[s]) A.f_table[s][i] = A.f_cloud[s];
    if (A.m_table[s]) A.m_table[s][i] = A.m_cloud[s];
  }
  if (i >= A.n0) return;
  const int ix = i % A.nx, iy = (i / A.nx) % A.ny, it = i / (A.nx * A.ny);
  float* p = A.pose + 3 * (size_t) i;
  p[0] = grid_coord(A.center[0], grid_offset(ix, A.nx), A.step[0]);
  p[1] = grid_coord(A.center[1], grid_offset(iy, A.ny), A.step[1]);
  p[2] = grid_coord(A.center[2], grid_offset(it, A.nt), A.step[2]);
  A.origin[i] = i;
}

struct GridChildrenArgs {
  const int32_t* sel;            // the previous level's selection: [n_accepted, n_selected, 0, 0 | index[k_parents] | ...]
  const float* pose_in; const int32_t* origin_in;      // the previous level's hypotheses, n_in slots
  int32_t n_in, k_parents;
  int32_t rx, ry, rt, R;         // R = rx ry rt
  float spacing[3];              // this level's, divided on the host
  float center[3];
  float* pose; int32_t* origin;  // [k_parents R][3], [k_parents R]
};

__global__ __launch_bounds__(256) void k_grid_children(const GridChildrenArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.k_parents * A.R) return;
  const int j = t / A.R, c = t % A.R;
  int m = A.sel[1];
  m = m < 0 ? 0 : (m > A.k_parents ? A.k_parents : m);
  int32_t* po = reinterpret_cast<int32_t*>(A.pose) + 3 * (size_t) t;
  if (m == 0) {      // nothing was selected: every slot is a pad at the grid's centre
    for (int w = 0; w < 3; ++w) po[w] = __float_as_int(A.center[w]);
    A.origin[t] = 0;
    return;
  }
  int h = A.sel[kSelectHeaderWords + (j < m ? j : 0)];
  if ((uint32_t) h >= (uint32_t) A.n_in) h = 0;      // (cannot be: the selection's indices are slot indices of the previous level)
  const float* base = A.pose_in + 3 * (size_t) h;
  const int cx = c % A.rx, cy = (c / A.rx) % A.ry, ct = c / (A.rx * A.ry);
  A.pose[3 * (size_t) t] = grid_coord(base[0], grid_offset(cx, A.rx), A.spacing[0]);
  A.pose[3 * (size_t) t + 1] = grid_coord(base[1], grid_offset(cy, A.ry), A.spacing[1]);
  A.pose[3 * (size_t) t + 2] = grid_coord(base[2], grid_offset(ct, A.rt), A.spacing[2]);
  A.origin[t] = A.origin_in[h];
}

struct GridMaskArgs {
  const int32_t* sel;            // the previous level's selection (its n_selected is the number of live parents)
  int32_t k_parents, R;
  int32_t* rows;                 // [k_parents R][Row::kWords] this level's combined rows
};

template <class Row>
__global__ __launch_bounds__(256) void k_grid_mask_pads(const GridMaskArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= A.k_parents * A.R) return;
  int m = A.sel[1];
  m = m < 0 ? 0 : (m > A.k_parents ? A.k_parents : m);
  if (t >= m * A.R) A.rows[(size_t) t * Row::kWords + Row::kActive] = 0;
}

struct GridFinishArgs {
  const int32_t* sel[kGridMaxLevels];      // every level's selection; the last one's lies in the region that goes down already
  int32_t n_levels, k, n_last;             // n_last: slots of the last level
  const float* pose_in; const int32_t* origin_in;      // the last level's hypotheses
  int32_t* headers;              // [n_levels][kSelectHeaderWords]
  float* pose; int32_t* origin;  // [k][3], [k]
};

__global__ __launch_bounds__(256) void k_grid_finish(const GridFinishArgs A) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < A.n_levels * kSelectHeaderWords) A.headers[j] = A.sel[j / kSelectHeaderWords][j % kSelectHeaderWords];
  if (j >= A.k) return;
  const int32_t* last = A.sel[A.n_levels - 1];
  int m = last[1];
  m = m < 0 ? 0 : (m > A.k ? A.k : m);
  if (j >= m) return;      // positions beyond the count are not written
  const int32_t h = last[kSelectHeaderWords + j];
  if ((uint32_t) h >= (uint32_t) A.n_last) return;      // (cannot be)
  const int32_t* p = reinterpret_cast<const int32_t*>(A.pose_in) + 3 * (size_t) h;
  int32_t* po = reinterpret_cast<int32_t*>(A.pose) + 3 * (size_t) j;
  for (int w = 0; w < 3; ++w) po[w] = p[w];
  A.origin[j] = A.origin_in[h];
}
