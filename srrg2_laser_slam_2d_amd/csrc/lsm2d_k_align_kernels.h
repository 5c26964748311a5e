// lsm2d_k_align_kernels.h -- the kernels that instantiate align_body (lsm2d_k_align.h): k_align, k_align_cand, k_align_two, k_align_seq_two, k_align_narrow, k_align_seq, and the register budget each is given.
// Part of lsm2d_kernels.h (included there, inside namespace lsm2d, right behind lsm2d_k_align.h); not a translation unit of its own.
// Registers: 8 waves per SIMD (64 VGPRs, four workgroups per CU) for every single-finder instantiation.  The MIXED instantiations (a projective slice next to a
// point-query slice in one aligner: all forms of all finders in one body) spilled 176 bytes per thread at that budget; they are given 4 waves per SIMD
// (128 VGPRs, two workgroups per CU) and have no private segment -- a configuration no BASELINE workload uses (round 5; tools/isa_dump.sh prints every kernel's frame).
// LSM2D_ALIGN_MIN_WAVES (lsm2d_k_align_args.h) is the one budget a tool still sets (tools/variant_bench.sh); the others are constants:
static constexpr int kMixedMinWaves = 4;
static constexpr int kQueryMinWaves = 8;                     // the instantiations without a projective slice (point-query finders); 6 and 4 measured 15-50 % slower
static constexpr int kNNGlobalMinWaves = kQueryMinWaves;     // k_align<0,1,0,0,1>: the A/B's other side was 6 (80 VGPRs, no frame, three workgroups per CU)
static constexpr int kSeqMinWaves = 8;
template <bool kHasProj, bool kHasNN, bool kHasDist, bool kHasKd, int kNNMode>
constexpr int align_min_waves() {
  return (kHasProj && (kHasNN || kHasDist || kHasKd)) ? kMixedMinWaves : kHasProj ? LSM2D_ALIGN_MIN_WAVES : kNNMode == 1 ? kNNGlobalMinWaves : kQueryMinWaves;
}
template <bool kHasProj, bool kHasNN, bool kHasDist, bool kHasKd = false, int kNNMode = 0>
__global__ __launch_bounds__(kAlignBlock, (align_min_waves<kHasProj, kHasNN, kHasDist, kHasKd, kNNMode>())) void k_align(const AlignArgs A) {
  align_body<kHasProj, kHasNN, kHasDist, kHasKd, kNNMode>(A);
}
// Round 20: k_align<1,0,0,0,5> WITH the candidate lists (align_body's kCandLists) -- a kernel of its own, launched only for a batch the host has given a list's room
// (AlignArgs::cand_off > 0); every other batch runs the kernel it always ran, instruction for instruction.
__global__ __launch_bounds__(kAlignBlock, LSM2D_ALIGN_MIN_WAVES) void k_align_cand(const AlignArgs A) {
  align_body<true, false, false, false, 5, false, kAlignBlock, true>(A);
}
// The culled projective stream with up to TWO alignments per workgroup, one after the other (AlignArgs::order2): the whole body again, from its prologue -- an
// instantiation of its own (two copies of the body), so that the headline's kernel does not carry a loop around it (in one kernel: 80 bytes of scratch).
__global__ __launch_bounds__(kAlignBlock, LSM2D_ALIGN_MIN_WAVES) void k_align_two(const AlignArgs A) {
  align_body<true, false, false, false, 5>(A, __builtin_amdgcn_readfirstlane(A.order[blockIdx.x]));
  const int a2 = __builtin_amdgcn_readfirstlane(A.order2[blockIdx.x]);
  if (a2 < 0) return;
  __syncthreads();      // (thread 0 is done with the first one's results before anybody overwrites the state they came from)
  align_body<true, false, false, false, 5>(A, a2);
}
// ... and the same with the reference's order of summation ("sum_order" 1: no narrow form exists for it, so every batch between one and two rounds is packed)
__global__ __launch_bounds__(kAlignBlock, kSeqMinWaves) void k_align_seq_two(const AlignArgs A) {
  align_body<true, false, false, false, 5, true>(A, __builtin_amdgcn_readfirstlane(A.order[blockIdx.x]));
  const int a2 = __builtin_amdgcn_readfirstlane(A.order2[blockIdx.x]);
  if (a2 < 0) return;
  __syncthreads();
  align_body<true, false, false, false, 5, true>(A, a2);
}
// The culled projective stream in NARROW workgroups (align_body's kW): 256 threads, six workgroups -- 1536 alignments -- resident per round where the wide kernel
// holds 1024.  The same results as k_align<1,0,0,0,5>, bit for bit; chosen by the host (align_width_for) for batches just above a multiple of 1024 alignments.
template <int kW>
__global__ __launch_bounds__(kW, LSM2D_ALIGN_MIN_WAVES) void k_align_narrow(const AlignArgs A) {
  align_body<true, false, false, false, 5, false, kW>(A);
}
// "sum_order" 1: the same kernel with the reference's order of summation (align_body<.., kSeq = true>).  14 KB of pair records per workgroup beside the canvases (four workgroups per CU still fit the headline's shape):
// the register budget stays that of 8 waves per SIMD -- 4 for the mixed instantiations, as above
template <bool kHasProj, bool kHasNN, bool kHasDist, bool kHasKd = false, int kNNMode = 0>
__global__ __launch_bounds__(kAlignBlock, ((kHasProj && (kHasNN || kHasDist || kHasKd)) ? kMixedMinWaves : kSeqMinWaves)) void k_align_seq(const AlignArgs A) {
  align_body<kHasProj, kHasNN, kHasDist, kHasKd, kNNMode, true>(A);
}
