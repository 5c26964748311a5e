// placement_deal_driver.hip -- balance_order (csrc/lsm2d_k_placement.h) alone, on chosen inputs.
//
// The deal of a culled batch's alignments to workgroup ids is a pure device function: it reads work[] and place[], writes order[], order2[] and the
// seconds scratch.  Through the library its inputs are whatever the dispatcher and the workload make them; here a test chooses them
// (tests/placement_cases.py: every size around the dispatch rounds, chosen work counts, chosen notes -- also the ones that take the two fallback
// branches, which no launch on this chip produces) and reads the whole order block back.  The header is included unchanged; the launch is the one
// k_cull_estimate's last workgroup makes: one workgroup of kAlignBlock threads, sizeof(BalanceLds) of dynamic LDS, per_cu 4, nt = kAlignBlock, the
// library's buffer layout (one block of kOrderInts words, order2 = order + kPackOrder2At).
//
// usage:  placement_deal_driver <cases file> <output file>
//
// cases file (int32, little endian):
//   'P','D','C','1'  n_cases
//   per case:  n  n_cu  n_place  has_order2   work[n]   place[n_place]
//     n_place 0: no notes (place = nullptr), otherwise at least first = min(n, 4 n_cu, 1024) and at most 1024 entries; has_order2 0 / 1.
// output file: per case the whole block of kOrderInts int32 as the device left it; every word was kSentinel (-7) before the launch.
//
// A case outside what the host guarantees the function (1 <= n <= 4096, every count in [0, kAlignBlock], n_cu >= 1, notes for the whole first round)
// is refused before anything is launched: exit code 3.  The first HIP error ends the run (exit code 2, the case's number on stderr): nothing is
// launched behind a fault.
//
// build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-function \
//               -Isrrg2_laser_slam_2d_amd/csrc -Iinclude -o placement_deal_driver tests/cpp/placement_deal_driver.hip
#include <hip/hip_runtime.h>
#include "lsm2d.h"
namespace lsm2d { static constexpr int LSM2D_RUNNING = -99; }
#include "lsm2d_kernels.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static constexpr int32_t kSentinel = -7;
static constexpr int kMaxN = 4096;

__global__ __launch_bounds__(lsm2d::kAlignBlock) void k_deal(const int32_t* work, int n, int n_cu, int32_t* order, const int32_t* place, int32_t* order2) {
  extern __shared__ __align__(16) unsigned char smem[];
  lsm2d::balance_order(*reinterpret_cast<lsm2d::BalanceLds*>(smem), work, n, n_cu, 4, order, place, (int) threadIdx.x, lsm2d::kAlignBlock, order2);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "case %d: HIP error %s at %s:%d\n", c, hipGetErrorString(e_), __FILE__, __LINE__); return 2; } } while (0)

static bool get(FILE* f, int32_t* p, size_t count) { return fread(p, sizeof(int32_t), count, f) == count; }

int main(int argc, char** argv) {
  using namespace lsm2d;
  static_assert(kPackOrder2At + kPackMaxRounds * 1024 == kPackSecondsAt && kPackSecondsAt + 1024 == kOrderInts && kMaxN <= kPackOrder2At, "the order block's layout");
  if (argc != 3) { fprintf(stderr, "usage: %s <cases file> <output file>\n", argv[0]); return 3; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 3; }
  int32_t head[2];
  if (!get(in, head, 2) || memcmp(&head[0], "PDC1", 4) != 0 || head[1] < 0) { fprintf(stderr, "%s: not a cases file\n", argv[1]); return 3; }
  const int n_cases = head[1];
  struct Case { int n, n_cu, n_place, has_order2; std::vector<int32_t> work, place; };
  std::vector<Case> cases((size_t) n_cases);
  // every case is read and held to the contract before the GPU is opened
  for (int c = 0; c < n_cases; ++c) {
    Case& k = cases[(size_t) c];
    int32_t h[4];
    if (!get(in, h, 4)) { fprintf(stderr, "case %d: truncated\n", c); return 3; }
    k.n = h[0]; k.n_cu = h[1]; k.n_place = h[2]; k.has_order2 = h[3];
    if (k.n < 1 || k.n > kMaxN || k.n_cu < 1 || k.n_cu > (1 << 20) || (k.has_order2 != 0 && k.has_order2 != 1)) { fprintf(stderr, "case %d: n %d, n_cu %d, has_order2 %d outside the contract\n", c, k.n, k.n_cu, k.has_order2); return 3; }
    int first = k.n < 4 * k.n_cu ? k.n : 4 * k.n_cu;
    if (first > kBalMaxFirst) first = kBalMaxFirst;
    if (k.n_place != 0 && (k.n_place < first || k.n_place > kBalMaxFirst)) { fprintf(stderr, "case %d: %d notes for a first round of %d\n", c, k.n_place, first); return 3; }
    k.work.resize((size_t) k.n); k.place.resize((size_t) k.n_place);
    if (!get(in, k.work.data(), (size_t) k.n) || !get(in, k.place.data(), (size_t) k.n_place)) { fprintf(stderr, "case %d: truncated\n", c); return 3; }
    for (int i = 0; i < k.n; ++i) if (k.work[(size_t) i] < 0 || k.work[(size_t) i] > kAlignBlock) { fprintf(stderr, "case %d: count %d of alignment %d outside [0, %d]\n", c, k.work[(size_t) i], i, kAlignBlock); return 3; }
  }
  fclose(in);
  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 3; }

  int c = -1;
  int32_t *d_work = nullptr, *d_place = nullptr, *d_order = nullptr;
  CK(hipMalloc(&d_work, sizeof(int32_t) * kMaxN));
  CK(hipMalloc(&d_place, sizeof(int32_t) * kBalMaxFirst));
  CK(hipMalloc(&d_order, sizeof(int32_t) * kOrderInts));
  const std::vector<int32_t> sentinel((size_t) kOrderInts, kSentinel);
  std::vector<int32_t> block((size_t) kOrderInts);
  for (c = 0; c < n_cases; ++c) {
    const Case& k = cases[(size_t) c];
    CK(hipMemcpy(d_work, k.work.data(), sizeof(int32_t) * (size_t) k.n, hipMemcpyHostToDevice));
    if (k.n_place) CK(hipMemcpy(d_place, k.place.data(), sizeof(int32_t) * (size_t) k.n_place, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_order, sentinel.data(), sizeof(int32_t) * kOrderInts, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_deal, dim3(1), dim3(kAlignBlock), sizeof(BalanceLds), 0, (const int32_t*) d_work, k.n, k.n_cu, d_order,
                       k.n_place ? (const int32_t*) d_place : (const int32_t*) nullptr, k.has_order2 ? d_order + kPackOrder2At : (int32_t*) nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(block.data(), d_order, sizeof(int32_t) * kOrderInts, hipMemcpyDeviceToHost));
    if (fwrite(block.data(), sizeof(int32_t), (size_t) kOrderInts, out) != (size_t) kOrderInts) { fprintf(stderr, "case %d: cannot write the output\n", c); return 3; }
  }
  if (fclose(out) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 3; }
  CK(hipFree(d_work)); CK(hipFree(d_place)); CK(hipFree(d_order));
  printf("%d cases\n", n_cases);
  return 0;
}
