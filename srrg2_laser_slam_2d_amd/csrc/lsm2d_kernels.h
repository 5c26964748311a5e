// lsm2d_kernels.h -- HIP kernels of the scan-matching hot path for gfx950 (CDNA4, wave64).
//
//   k_align            the product kernel: ONE workgroup owns ONE alignment for all max_iterations
//                      (MultiAligner2D::compute restated): per iteration and slice it
//                      streams the moving cloud through an LDS polar z-buffer (64-bit ds_min keys),
//                      walks the two canvases bin by bin (registration/correspondence_finder_projective_2d.cpp:55-74),
//                      accumulates the plane-to-plane factor (octave/solver/nicp_post.m:4-26,69-90) in
//                      registers, reduces with wave shuffles + one LDS hop, and wave 0 solves the 3x3
//                      system and right-updates the pose -- no host round trip, no global atomics.
//   k_find_projective  CorrespondenceFinderProjective2f::compute for one (fixed, moving, pose): ordered pairs (lsm2d_k_finder.h).
//   k_find_nn[_multi]  the point-query finders (exact grid NN, KD-tree, distance map) for one (fixed, moving, pose): pairs in ascending moving index.
//   k_find_*_batch     the same finders for n_items (fixed, moving, pose) triples in one launch, a workgroup per item: the single kernels' bodies.
//   k_project_canvas   PointNormal2fProjectorPolar::compute: source index / depth / transformed point per column.
//   k_linearize_*      SE2Plane2PlaneErrorFactor over a correspondence vector (two-stage deterministic reduce).
//   k_linearize_*_batch  the same factor over a batch of vectors: the same device functions, an item keeps the single call's launch shape.
//   k_score_*_batch    the same factor over the slots k_find_*_batch has just filled, counts read from the device: the pairs never leave it (lsm2d_score_batch).
//   k_select_*         the acceptance test and the best k of those rows, ranked on the device: only k rows travel (lsm2d_score_select; lsm2d_k_select.h).
//   k_align_rows       one row per ALIGNED candidate (pose, H, status, iterations, its last iteration's statistics) for the same selection, and the counts of
//                      Success and never-written statuses (lsm2d_align_select; lsm2d_k_align_select.h).
//   k_select_group_one / k_select_*_seg / k_select_gather_group  the same selection per GROUP of the batch: a fleet's candidates, the best k per robot
//                      (lsm2d_*_select_grouped; lsm2d_k_select_grouped.h).
//   k_score_aligner_items / k_score_combine  hypotheses scored against a whole aligner: per-slice item tables from the poses, and the slices' rows combined with
//                      the skip rule and the prior into one row per item (lsm2d_score_aligner_batch / _select; lsm2d_k_score_aligner.h).
//   k_reloc_items / k_align_rows_live  the scoring's selection turned into the aligner's input block on the device, and k_align_rows for a batch whose tail
//                      is padding (lsm2d_relocalize_select; lsm2d_k_relocalize.h).
//   k_grid_level0 / k_grid_children / k_grid_mask_pads / k_grid_finish  a grid of pose hypotheses made on the device, a level's selection turned into the next
//                      level's hypotheses, pads kept out of the ranking (lsm2d_score_grid_select; lsm2d_k_score_grid.h).
//   k_vox_keys / k_vox_hist / k_vox_scan / k_vox_scatter / k_vox_head_count / k_vox_head_write / k_vox_sum / k_vox_verdict / k_vox_write / k_vox_finish
//                      PointCloud::voxelize over device-resident clouds of any size: keys, a stable radix sort, the runs' sums in the reference's order, the
//                      voxels to the clouds of a reserved set behind a capacity verdict made on the device (lsm2d_voxelize; lsm2d_k_voxelize.h).
//   k_occ_rays / k_occ_tiles / k_occ_render / k_occ_put
//                      occupancy grids: device-resident clouds ray-traced from their sensor poses into per-cell hit / miss counters, a workgroup per tile
//                      summing in LDS, and the counters rendered to 0 .. 100 / -1 (lsm2d_occupancy_update / _render; lsm2d_k_occupancy.h; not in the reference).
//   k_repack_cloud    AoS float4 (x,y,nx,ny) -> split xy / normal arrays with even-aligned cloud starts.
#pragma once
#include "lsm2d_device.h"

#include <type_traits>

namespace lsm2d {

static constexpr int kMaxSlices = 4;
static constexpr int kFfRing = 16;     // align_body's fast-forward: iteration-start poses remembered = the longest period it finds (a power of two)
static constexpr int kFfRowWords = 10; // ... and per remembered iteration, for "fast_forward" 2, in device memory (AlignArgs::ff_rows): H's nine words and the inlier count
// (A -DLSM2D_EXPERIMENTS build of the library differs on the host side only: lsm2d_capi.hip's A/B option keys, switches for alternatives that are always on in the
// product.  Its kernels are the shipped ones; the code of the measured-and-rejected launch forms is gone from the tree: docs/REJECTED.md.)
// exact culling of a projective slice's moving cloud (k_align): a thread's chunk of T steps is cut into at most kCullBlocks blocks of B steps
static constexpr int kCullBlocks = 7;
LSM2D_HD int cull_block_steps(int T, int nbs = kCullBlocks) { return 2 * ((T + 2 * nbs - 1) / (2 * nbs)); }      // even; ceil(T / B) <= nbs for every T >= 1
// Wave priority by progress.  The SIMD arbitrates by priority, then AGE: with equal priorities the oldest two waves of a SIMD run
// at full single-wave speed and the younger workgroups of a CU wait (tools/occupancy_probe.py: lifetimes 0.97 .. 2.19 ms in one
// launch), so the last workgroup of a CU ends up alone, with nobody to issue under its barriers, bin walks and solves.  A
// workgroup that lowers its priority as it advances lets the ones behind it catch up: all of a CU's workgroups finish together.
// The schedule is align_body's: halving intervals -- priority 3 for the first 1/2 of the iterations, 2 up to 3/4, 1 up to 7/8, then 0 (1.65 ms on configs[1]; off 1.86,
// quarters of the iterations 1.69; those two and the schedule rising with the iteration are gone from the tree: docs/REJECTED.md).
// k_align_seq's walking wave is at top priority while it walks (seq_walk<true>; configs[1], "sum_order" 1: 0.954 -> 0.937 ms; profiles/r06/sum_order_walker_quads_ab_r06.txt).
static constexpr int kAlignBlock = 512;
static constexpr int kFindBlock = 1024;

#include "lsm2d_k_search.h"
#include "lsm2d_k_structures.h"
#include "lsm2d_k_kdbuild.h"
#include "lsm2d_k_align_args.h"
#include "lsm2d_k_align_probe.h"
#include "lsm2d_k_align.h"
#include "lsm2d_k_align_kernels.h"
#include "lsm2d_k_placement.h"
#include "lsm2d_k_align_pair.h"
#include "lsm2d_k_split_finder.h"
#include "lsm2d_k_select.h"
#include "lsm2d_k_align_select.h"
#include "lsm2d_k_select_grouped.h"
#include "lsm2d_k_score_aligner.h"
#include "lsm2d_k_finder.h"
#include "lsm2d_k_mapping.h"
#include "lsm2d_k_layout.h"
#include "lsm2d_k_relocalize.h"
#include "lsm2d_k_score_grid.h"
#include "lsm2d_k_voxelize.h"
#include "lsm2d_k_occupancy.h"

}  // namespace lsm2d
