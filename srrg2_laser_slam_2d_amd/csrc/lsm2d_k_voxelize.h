// lsm2d_k_voxelize.h -- PointCloud::voxelize over device-resident clouds of any size, several inputs and several outputs per call (lsm2d_voxelize).
// Part of lsm2d_kernels.h (included there inside namespace lsm2d).
//
// What voxelize_lds (lsm2d_k_mapping.h) does for at most kVoxMax points of one workgroup in LDS, for a batch of any size: the same key, the same order, the
// same sums (PARITY.md section 3, item 17b).  The chain, every step a launch of its own on the lane's stream:
//   k_vox_keys        a thread per concatenated point: its input by binary search in the call's offset table, the point moved by the input's pose (xf_point /
//                     xf_normal: lsm2d_merge_scene's transform; no pose: the bits copied), the transformed values written ONCE to scratch -- nothing reads the
//                     source clouds after this launch, which is what makes dst == src legal -- and the sort key (dropped | group | voxel key) with the
//                     concatenation index as its value.  A point without a key gets the all-ones key and is counted per group.
//   per digit of 8 bits, lowest first, over the bits in use (42 key bits + the group bits the call needs + the dropped bit):
//     k_vox_hist      a WAVE per tile of kVoxTile keys: the tile's 256 digit counts, to hist[digit][tile]
//     k_vox_scan      ONE workgroup: the exclusive prefix sum over hist in that order (digit-major), in place, kVoxScanTiles tiles' counters (4096 words) a pass,
//                     the running sum carried from pass to pass
//     k_vox_scatter   a wave per tile again: 64 keys a round, a key's rank among the equal digits of its round by wave64 ballots, the digit's running position
//                     in LDS; ranks follow the lane order, tiles follow the scan: the sort is STABLE, equal keys stay in ascending concatenation index
//   k_vox_head_count  a wave per tile: positions whose key differs from their predecessor's (heads), counted; k_vox_scan over the tiles' counts
//   k_vox_head_write  the heads' positions compacted in order; the first head of a group notes its rank (group_first)
//   k_vox_sum         a thread per head walks its run in sorted order and forms the reference's sums over the transformed values: four fp32 sums from +0,
//                     times 1.0f / (float) count, the normal divided by sqrtf(fmaf(anx, anx, any * any)) when that is > 0.  The voxel goes to scratch; the last
//                     head of a group notes its rank (group_last).  A run may be ARBITRARILY long -- a million points in one voxel is one thread adding a
//                     million times: legal and slow; the sums cannot be split and keep their bits.
//   k_vox_verdict     a thread per group: its voxel count, and whether it fits its destination cloud -- decided on the device ahead of the first write
//   k_vox_write       a thread per head: the voxel to its destination cloud, unless some group did not fit (then NO destination cloud is touched)
//   k_vox_finish      a thread per group: the destination clouds' device-side counts, last
// Every index is checked against its array before it is used; a check that fails -- it cannot, while the chain is right -- sets a fault word, nothing more is
// written to the destination set's counts, and the host answers LSM2D_DEVICE_ERROR: a fault is never a wrong answer.
// No workgroup waits for another: every dependency is a launch boundary.  No float atomics; integer atomics count (the tiles' digits in LDS, the dropped
// points per group).
#pragma once

static constexpr int kVoxTile = 1024;              // keys per sort tile: what ONE wave ranks ("voxelize_tile")
static constexpr int kVoxScanBlock = 1024;
static constexpr int kVoxScanTiles = 4 * kVoxScanBlock / 256;      // tiles whose 256 counters ONE pass of the scan's workgroup takes; the running sum is carried from pass to pass ("voxelize_scan_tiles": 16)
static constexpr int kVoxSortBlock = 256;          // 4 waves, 4 tiles per workgroup
static constexpr int kVoxKeyBits = 42;             // the voxel key: 16 + 16 + 5 + 5 bits (PARITY.md section 3, item 17b)
static constexpr int kVoxMaxPoints = 1 << 24;      // LSM2D_VOXELIZE_MAX_POINTS
static constexpr int kVoxMaxGroups = 1 << 16;      // LSM2D_VOXELIZE_MAX_GROUPS
static constexpr u64 kVoxDropped = ~0ull;

struct VoxInput { Iso T; int32_t start, group, has_pose, pad; };      // per input of the call's list: where its points begin in the source arrays
struct VoxGroup { int32_t start, cap, cloud, pad; };                  // per group: where its destination cloud begins, its room, its index in the set

struct VoxKeysArgs {
  const float2* xy; const float2* nrm;            // the source set
  const VoxInput* inputs; const int32_t* offset;  // [n_inputs], [n_inputs + 1] concatenation offsets
  int32_t n_inputs, n;                            // n: concatenated points
  float inv_res, inv_rn;
  float2* txy; float2* tn;                        // [n] transformed values
  u64* key; uint32_t* idx;                        // [n]
  int32_t* dropped;                               // [n_groups]
};

__global__ __launch_bounds__(256) void k_vox_keys(const VoxKeysArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  int lo = 0, hi = A.n_inputs;      // the last input k with offset[k] <= i (empty inputs share their successor's offset and lose)
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.offset[mid] <= i) lo = mid; else hi = mid; }
  const VoxInput in = A.inputs[lo];
  const size_t s = (size_t) in.start + (size_t) (i - A.offset[lo]);
  const float2 p = A.xy[s], q = A.nrm[s];
  float x = p.x, y = p.y, nx = q.x, ny = q.y;
  if (in.has_pose) { xf_point(in.T, p.x, p.y, x, y); xf_normal(in.T, q.x, q.y, nx, ny); }
  A.txy[i] = make_float2(x, y); A.tn[i] = make_float2(nx, ny);
  const float kx = __builtin_floorf(x * A.inv_res), ky = __builtin_floorf(y * A.inv_res);
  const float knx = __builtin_floorf(nx * A.inv_rn), kny = __builtin_floorf(ny * A.inv_rn);
  u64 key = kVoxDropped;
  if (kx >= -32768.0f && kx < 32768.0f && ky >= -32768.0f && ky < 32768.0f && knx >= -16.0f && knx <= 15.0f && kny >= -16.0f && kny <= 15.0f) {
    const u64 v = ((u64) ((int) kx + 32768) << 26) | ((u64) ((int) ky + 32768) << 10) | ((u64) ((int) knx + 16) << 5) | (u64) ((int) kny + 16);
    key = ((u64) (uint32_t) in.group << kVoxKeyBits) | v;
  } else {
    atomicAdd(A.dropped + in.group, 1);
  }
  A.key[i] = key; A.idx[i] = (uint32_t) i;
}

// a wave's LDS words are its own here: its operations complete in order, only the compiler must keep them in order
LSM2D_DEV void vox_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

struct VoxSortArgs {
  const u64* key_in; const uint32_t* idx_in; u64* key_out; uint32_t* idx_out;
  uint32_t* hist;                 // [256][n_tiles]
  int32_t n, n_tiles, shift;
  int32_t* fault;                 // set when an index leaves its array (cannot be; the host turns it into LSM2D_DEVICE_ERROR)
};

__global__ __launch_bounds__(kVoxSortBlock) void k_vox_hist(const VoxSortArgs A) {
  __shared__ uint32_t s_cnt[kVoxSortBlock / 64][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (kVoxSortBlock / 64) + wave;
  uint32_t* cnt = s_cnt[wave];
  for (int d = lane; d < 256; d += 64) cnt[d] = 0;
  vox_wave_sync();
  if (tile >= A.n_tiles) return;
  const int b = tile * kVoxTile, e = b + kVoxTile < A.n ? b + kVoxTile : A.n;
  for (int i = b + lane; i < e; i += 64) atomicAdd(&cnt[(uint32_t) (A.key_in[i] >> A.shift) & 255u], 1u);
  vox_wave_sync();
  for (int d = lane; d < 256; d += 64) A.hist[(size_t) d * A.n_tiles + tile] = cnt[d];
}

// exclusive prefix sum of data[0 .. n) in place, ONE workgroup; the sum of all goes to *total when that is given
struct VoxScanArgs { uint32_t* data; int32_t n; int32_t* total; };

__global__ __launch_bounds__(kVoxScanBlock) void k_vox_scan(const VoxScanArgs A) {
  __shared__ uint32_t s_wave[kVoxScanBlock / 64];
  __shared__ uint32_t s_carry;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int c0 = 0; c0 < A.n; c0 += 4 * kVoxScanBlock) {
    const int i0 = c0 + 4 * tid;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = i0 + j < A.n ? A.data[i0 + j] : 0u; sum += v[j]; }
    uint32_t inc = sum;      // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = s_carry, all = 0;
    for (int w = 0; w < kVoxScanBlock / 64; ++w) { const uint32_t t = s_wave[w]; if (w < wave) before += t; all += t; }
    uint32_t run = before + inc - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) { if (i0 + j < A.n) A.data[i0 + j] = run; run += v[j]; }
    __syncthreads();
    if (tid == 0) s_carry += all;
    __syncthreads();
  }
  if (tid == 0 && A.total) *A.total = (int32_t) s_carry;
}

__global__ __launch_bounds__(kVoxSortBlock) void k_vox_scatter(const VoxSortArgs A) {
  __shared__ uint32_t s_run[kVoxSortBlock / 64][256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (kVoxSortBlock / 64) + wave;
  if (tile >= A.n_tiles) return;
  uint32_t* run = s_run[wave];
  for (int d = lane; d < 256; d += 64) run[d] = A.hist[(size_t) d * A.n_tiles + tile];
  vox_wave_sync();
  const int b = tile * kVoxTile, e = b + kVoxTile < A.n ? b + kVoxTile : A.n;
  const u64 below = (1ull << lane) - 1ull;
  for (int i0 = b; i0 < e; i0 += 64) {
    const int i = i0 + lane;
    const bool live = i < e;
    u64 key = 0; uint32_t idx = 0;
    if (live) { key = A.key_in[i]; idx = A.idx_in[i]; }
    const uint32_t d = (uint32_t) (key >> A.shift) & 255u;
    u64 same = __ballot(live);      // the live lanes of this round with my digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) { const u64 m = __ballot(live && ((d >> bit) & 1u)); same &= ((d >> bit) & 1u) ? m : ~m; }
    const uint32_t base = run[d];
    vox_wave_sync();
    if (live && (same & below) == 0) run[d] = base + (uint32_t) __popcll(same);      // the digit's first lane moves its position on
    vox_wave_sync();
    if (live) {
      const uint32_t pos = base + (uint32_t) __popcll(same & below);
      if (pos < (uint32_t) A.n) { A.key_out[pos] = key; A.idx_out[pos] = idx; }      // (the positions are a permutation of 0 .. n)
      else *A.fault = 1;
    }
  }
}

struct VoxHeadArgs {
  const u64* key;                 // [n] sorted
  uint32_t* tile_heads;           // [n_tiles]: k_vox_head_count writes the counts, k_vox_scan turns them into the tiles' first ranks
  int32_t n, n_tiles;
  uint32_t* head_pos;             // [n] the heads' positions, in order
  int32_t* group_first;           // [n_groups] the rank of a group's first head
  int32_t* fault;
};

LSM2D_DEV bool vox_is_head(const u64* key, int p) {
  const u64 k = key[p];
  return k != kVoxDropped && (p == 0 || key[p - 1] != k);
}

__global__ __launch_bounds__(kVoxSortBlock) void k_vox_head_count(const VoxHeadArgs A) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (kVoxSortBlock / 64) + wave;
  if (tile >= A.n_tiles) return;
  const int b = tile * kVoxTile, e = b + kVoxTile < A.n ? b + kVoxTile : A.n;
  uint32_t c = 0;
  for (int i0 = b; i0 < e; i0 += 64) { const int i = i0 + lane; c += (uint32_t) __popcll(__ballot(i < e && vox_is_head(A.key, i))); }
  if (lane == 0) A.tile_heads[tile] = c;
}

__global__ __launch_bounds__(kVoxSortBlock) void k_vox_head_write(const VoxHeadArgs A) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = blockIdx.x * (kVoxSortBlock / 64) + wave;
  if (tile >= A.n_tiles) return;
  const int b = tile * kVoxTile, e = b + kVoxTile < A.n ? b + kVoxTile : A.n;
  const u64 below = (1ull << lane) - 1ull;
  uint32_t h0 = A.tile_heads[tile];
  for (int i0 = b; i0 < e; i0 += 64) {
    const int i = i0 + lane;
    const bool head = i < e && vox_is_head(A.key, i);
    const u64 m = __ballot(head);
    if (head) {
      const uint32_t h = h0 + (uint32_t) __popcll(m & below);
      if (h < (uint32_t) A.n) A.head_pos[h] = (uint32_t) i; else *A.fault = 1;
      const uint32_t g = (uint32_t) (A.key[i] >> kVoxKeyBits);
      if (i == 0 || (uint32_t) (A.key[i - 1] >> kVoxKeyBits) != g) A.group_first[g] = (int32_t) h;      // (g < n_groups: a head is not a dropped point, and the host checked every group)
    }
    h0 += (uint32_t) __popcll(m);
  }
}

struct VoxSumArgs {
  const u64* key; const uint32_t* idx;        // [n] sorted
  const float2* txy; const float2* tn;        // [n] transformed values, by concatenation index
  const uint32_t* head_pos; const int32_t* n_heads;
  int32_t n, n_groups;
  float2* vxy; float2* vn;                    // [n_heads] the voxels, in order
  int32_t* group_last;                        // [n_groups] the rank of a group's last head
  int32_t* fault;
};

__global__ __launch_bounds__(256) void k_vox_sum(const VoxSumArgs A) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  int nh = *A.n_heads; if (nh > A.n) nh = A.n;
  if (h >= nh) return;
  const int p = (int) A.head_pos[h];
  if (p < 0 || p >= A.n) { *A.fault = 1; return; }
  const u64 key = A.key[p];
  float ax = 0.0f, ay = 0.0f, anx = 0.0f, any_ = 0.0f; int cnt = 0;
  int e = p;
  for (; e < A.n && A.key[e] == key; ++e) {
    const uint32_t i = A.idx[e];
    if (i >= (uint32_t) A.n) { *A.fault = 1; return; }
    const float2 q = A.txy[i], m = A.tn[i];
    ax += q.x; ay += q.y; anx += m.x; any_ += m.y; ++cnt;
  }
  const float inv = 1.0f / (float) cnt;
  ax *= inv; ay *= inv; anx *= inv; any_ *= inv;
  const float nn = __builtin_sqrtf(__builtin_fmaf(anx, anx, any_ * any_));
  if (nn > 0.0f) { anx = anx / nn; any_ = any_ / nn; }
  A.vxy[h] = make_float2(ax, ay); A.vn[h] = make_float2(anx, any_);
  const uint32_t g = (uint32_t) (key >> kVoxKeyBits);
  if (g >= (uint32_t) A.n_groups) { *A.fault = 1; return; }
  if (e >= A.n || (uint32_t) (A.key[e] >> kVoxKeyBits) != g) A.group_last[g] = h;
}

struct VoxOutArgs {
  const VoxGroup* groups; int32_t n_groups, n;
  const int32_t* group_first; const int32_t* group_last;      // (first 0, last -1: a group without heads)
  int32_t* counts;                // [n_groups] voxels per group, as needed -- written whatever the verdict is
  int32_t* verdict;               // 0: every group fits its destination cloud
  const u64* key; const uint32_t* head_pos; const int32_t* n_heads;
  const float2* vxy; const float2* vn;
  float2* dst_xy; float2* dst_nrm; int32_t* dst_count;
  int32_t* fault;
};

__global__ __launch_bounds__(256) void k_vox_verdict(const VoxOutArgs A) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= A.n_groups) return;
  const int c = A.group_last[g] - A.group_first[g] + 1;
  A.counts[g] = c;
  if (c > A.groups[g].cap) *A.verdict = 1;      // (every writer writes the same word)
}

__global__ __launch_bounds__(256) void k_vox_write(const VoxOutArgs A) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (*A.verdict || *A.fault) return;
  int nh = *A.n_heads; if (nh > A.n) nh = A.n;
  if (h >= nh) return;
  const uint32_t p = A.head_pos[h];
  if (p >= (uint32_t) A.n) { *A.fault = 1; return; }
  const uint32_t g = (uint32_t) (A.key[p] >> kVoxKeyBits);
  if (g >= (uint32_t) A.n_groups) { *A.fault = 1; return; }
  const VoxGroup G = A.groups[g];
  const int j = h - A.group_first[g];
  if (j < 0 || j >= G.cap) { *A.fault = 1; return; }      // (the verdict said it fits)
  A.dst_xy[(size_t) G.start + j] = A.vxy[h]; A.dst_nrm[(size_t) G.start + j] = A.vn[h];
}

__global__ __launch_bounds__(256) void k_vox_finish(const VoxOutArgs A) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= A.n_groups || *A.verdict || *A.fault) return;
  A.dst_count[A.groups[g].cloud] = A.counts[g];
}
