/*
 * lsm2d.h -- C ABI of the MI355X-native 2D scan-matching core (liblsm2d_hip.so).
 *
 * Drop-in boundary for ONE hot path of rvp-group/srrg2_laser_slam_2d: the per-scan inner loop
 * "correspondence search + plane-to-plane ICP Gauss-Newton step" that the reference runs through
 *   - CorrespondenceFinder_<Isometry2f, PointNormal2fVectorCloud, PointNormal2fVectorCloud>
 *     (srrg2_laser_slam_2d/src/srrg2_laser_slam_2d/registration/correspondence_finder_normal_2f.h:9-13),
 *   - AlignerSliceProcessorLaser2D[WithSensor]  (registration/aligner_slice_processor_laser_2d.h:7-42),
 *   - MultiAligner2D (upstream; driven as in apps/visual_test_aligner_2d.cpp:123-156).
 * Paths below are relative to srrg2_laser_slam_2d/src/srrg2_laser_slam_2d/ unless they start
 * with apps/ or configurations/.
 *
 * Conventions (apps/visual_test_aligner_2d.cpp:126,145):
 *   - a point is the PointNormal2f payload: 4 x fp32 (x, y, nx, ny), array-of-structs on the host side;
 *   - a pose is float[3] = (x, y, theta) = geometry2d::t2v(Isometry2f), metres / radians;
 *   - the estimate maps MOVING into FIXED (setMovingInFixed / setLocalMapInSensor);
 *   - H is row-major 3x3 in the right-perturbation basis X <- X * v2t(dx).
 * Plain pointers and sizes only; no exceptions cross this boundary: every entry point returns an
 * lsm2d_status (0 = ok, < 0 = call-level error); per-alignment outcomes go to out_status[].
 * One lsm2d_context = one device + one HIP stream; a context is not thread-safe, different contexts
 * may be used concurrently.  Host buffers are borrowed for the duration of a call only.
 */
#ifndef LSM2D_H
#define LSM2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSM2D_VERSION 160 /* 0.1.1: + lsm2d_preprocess_scan_into, asynchronous clip / merge (NULL size outputs), non-blocking upload;
                             0.1.11: + lsm2d_get_option, align_path 3; 0.1.12: + lsm2d_merge_scenes;
                             0.2.0: + lsm2d_clip_scene_voxelized, lsm2d_sweep_* (multi-device loop-closure sweep), in-kernel clock options;
                             0.2.1: + lsm2d_cloudset_cloud_sizes, pinned / device-resident ranges in lsm2d_preprocess_scans, options
                                    "distmap_build", "grid_big_threshold", "find_path", "zero_copy_max";
                             0.3.0: + LSM2D_FINDER_KDTREE (the reference KD-tree's own build and single-leaf descent, honouring max_leaf_range /
                                    min_leaf_points: lsm2d_slice_params grew two fields), lsm2d_aligner_params.termination_chi_epsilon,
                                    sweep option "peer_copy";
                             0.4.0: lsm2d_iteration_stats grew the order-independent digest of the iteration's correspondence set (pair_digest_lo / _hi);
                                    lsm2d_aligner_params grew enable_inlier_only_runs / keep_only_inlier_correspondences (no longer refused);
                                    + lsm2d_align_batch_pairs (the correspondences the aligner leaves in its slices), lsm2d_stats_capacity,
                                    lsm2d_pair_hash, lsm2d_estimate_work (work-aware sharding of a candidate sweep);
                             0.5.0: + lsm2d_align_batch_begin / _wait (a batch in flight while the host prepares the next one), lsm2d_preprocess_scans_refill
                                    (fresh scans into an existing set: no allocation, nothing waits); the option keys below are the WHOLE public set (the A/B
                                    knobs of rounds 1-4 exist only in a -DLSM2D_EXPERIMENTS build); read-only keys "uploads", "last_cull_estimate", "experiments";
                             0.6.0: + option "sum_order" (1: H, b and the chi^2 statistics are added pair after pair in the reference's order -- the ONE option
                                    results depend on: with it the aligner is bitwise the sequential fp32 restatement of nicp_post.m:69-90);
                             (0.7.0, number unchanged: additions only) + lsm2d_cloudset_create_reserved_many / lsm2d_cloudset_clear_clouds, lsm2d_clip_scene_batch,
                                    lsm2d_merge_scene_batch (N independent trackers per call: one workgroup per tracker, the single-tracker calls' bits);
                             (0.7.1, number unchanged: an addition only) + lsm2d_find_correspondences_batch (plugin interface #1 for n_items triples in one
                                    launch, the single call's bits); lsm2d_align_batch_pairs of more than one alignment derives its pairs through it;
                             (0.7.2, number unchanged: an addition only) + lsm2d_linearize_batch (the factor over n_items correspondence vectors in one
                                    launch, the single call's bits in both orders of summation);
                             (0.7.3, number unchanged: an addition only) + lsm2d_score_batch (finder, then factor, for n_items pose hypotheses with the
                                    pairs kept on the device: one copy down and one wait per call, the bits of the two batch calls in sequence);
                             (0.7.4, number unchanged: an addition only) + lsm2d_score_select, lsm2d_select_params, LSM2D_SELECT_MAX_K (lsm2d_score_batch's
                                    scoring, then the acceptance test and the best k hypotheses ranked on the device: only k rows come down);
                             (0.7.5, number unchanged: an addition only) + lsm2d_score_aligner_batch, lsm2d_score_aligner_select (hypotheses scored against an
                                    ALIGNER -- all its slices, sensor offsets, the skip rule and the optional prior -- in one call with one wait, and ranked
                                    on the device);
                             (0.7.6, number unchanged: an addition only) + lsm2d_clip_scene_voxelized_batch (lsm2d_clip_scene_batch with the clipper's
                                    voxelize_resolution > 0 branch inside the same launch, the single voxelised call's bits per tracker);
                             (0.7.7, number unchanged: an addition only) + lsm2d_align_select, lsm2d_sweep_align_select (lsm2d_align_batch's alignment, then
                                    the candidate loops' acceptance test -- status term included -- and the best k aligned candidates ranked on the device:
                                    only k rows come down, whatever the iteration count is);
                             (0.7.8, number unchanged: an addition only) + lsm2d_score_select_grouped, lsm2d_score_aligner_select_grouped,
                                    lsm2d_align_select_grouped, LSM2D_SELECT_MAX_GROUP_ROWS (the three select calls per GROUP of the batch -- a fleet's
                                    candidates, the best k per robot: one call, one wait, n_groups x k rows come down);
                             (0.7.9, number unchanged: an addition only) + lsm2d_relocalize_select (lsm2d_score_aligner_select, then lsm2d_align_select
                                    over the selected hypotheses, chained on the device: one upload, one copy down, one wait);
                             (0.7.10, number unchanged: an addition only) + lsm2d_score_grid_select, lsm2d_pose_grid, LSM2D_GRID_MAX_LEVELS,
                                    LSM2D_GRID_MAX_ITEMS (a grid of pose hypotheses made on the device from a descriptor and scored coarse to fine:
                                    a level's selection becomes the next level's hypotheses there; no upload of items, one copy down, one wait);
                             (0.7.11, number unchanged: an addition only) + lsm2d_voxelize, lsm2d_voxelize_params, LSM2D_VOXELIZE_MAX_POINTS,
                                    LSM2D_VOXELIZE_MAX_GROUPS (PointCloud::voxelize over device-resident clouds of any size: several inputs, each moved
                                    by a pose, voxelised per group into the clouds of a reserved set; one copy down, one wait); read-only option keys
                                    "voxelize_tile", "voxelize_scan_tiles";
                             (0.7.12, number unchanged: an addition only) + lsm2d_gridset (create / clear / upload / download / destroy),
                                    lsm2d_grid_geometry, lsm2d_occupancy_update, lsm2d_occupancy_render, lsm2d_occupancy_render_params,
                                    LSM2D_OCCUPANCY_MAX_SIDE / _MAX_CELLS / _MAX_RAYS / _MAX_RAY_CELLS (occupancy grids on the device: clouds ray-traced
                                    from their sensor poses into hit / miss counts, rendered to 0 .. 100 / -1; not in the reference); read-only option
                                    keys "occupancy_tile", "last_occupancy_wg_median_ns", "last_occupancy_wg_max_ns";
                             (0.7.13, number unchanged: an addition only) + read-only option key "live_handles"; lsm2d_occupancy_update_scans,
                                    lsm2d_occupancy_scan_params (occupancy grids from raw range scans: maximum-range truncation and clearing along
                                    beams without a return);
                             (0.7.14, number unchanged: an addition only) + log-odds grid sets: lsm2d_logodds_params, lsm2d_logodds_render_params,
                                    lsm2d_gridset_create_logodds / _set_logodds / _upload_logodds / _download_logodds, lsm2d_occupancy_decay,
                                    lsm2d_logodds_render_table, lsm2d_occupancy_render_logodds (occupancy as clamped log-odds, one vote per scan and
                                    cell, the hit winning; both update calls accept either kind of set) */

/* ---- status codes -------------------------------------------------------------------------
 * Replace: std::runtime_error throws of the finders (registration/correspondence_finder_projective_2d.cpp:21-31,
 * registration/correspondence_finder_nn_2d.cpp:11-18) and the upstream aligner status enum. */
typedef enum {
  LSM2D_SUCCESS                    = 0,
  LSM2D_NOT_ENOUGH_CORRESPONDENCES = 1,  /* per-alignment */
  LSM2D_NOT_ENOUGH_INLIERS         = 2,  /* per-alignment */
  LSM2D_SINGULAR_H                 = 3,  /* per-alignment */
  LSM2D_BAD_ARGUMENT               = -1,
  LSM2D_DEVICE_ERROR               = -2, /* a HIP call failed; lsm2d_last_error() has the text */
  LSM2D_OUT_OF_MEMORY              = -3,
  LSM2D_CAPACITY_EXCEEDED          = -4, /* output buffer too small / canvas too large for LDS */
  LSM2D_NO_DEVICE                  = -5
} lsm2d_status;

/* ---- parameter blocks ----------------------------------------------------------------------
 * PointNormal2fProjectorPolar parameters as the reference sets them
 * (apps/synthetic_scene_generator.cpp:69-75; configurations/stage_segway_double_config_MULTI.json:71-97).
 * Camera matrix convention [[cols/(angle_max-angle_min), cols/2],[0,1]]
 * (apps/synthetic_scene_generator.cpp:59-66, sensor_processing/raw_data_preprocessor_projective_2d.cpp:83-90). */
typedef struct {
  int32_t canvas_cols;
  float   angle_min, angle_max;  /* angle_col_min / angle_col_max [rad] */
  float   range_min, range_max;  /* [m] */
  float   col_offset;            /* column = floor(K00*atan2(y,x) + K01 + col_offset); 0 = truncate, 0.5 = nearest */
} lsm2d_projector;

typedef enum {
  LSM2D_FINDER_PROJECTIVE = 0, /* CorrespondenceFinderProjective2f  (registration/correspondence_finder_projective_2d.cpp:18-77) */
  LSM2D_FINDER_NN         = 1, /* CorrespondenceFinderKDTree2D      (registration/correspondence_finder_kd_tree_2d.cpp:5-38) with an EXACT
                                  nearest-neighbour search (uniform grid): a superset-quality substitute, max_leaf_range / min_leaf_points unused */
  LSM2D_FINDER_DISTMAP    = 2, /* CorrespondenceFinderNN2D          (registration/correspondence_finder_nn_2d.cpp:54-97) */
  LSM2D_FINDER_KDTREE     = 3  /* CorrespondenceFinderKDTree2D as the reference runs it: reset() builds KDTree2D(coordinates, max_leaf_range,
                                  min_leaf_points) (.cpp:31-38, .h:36-39), compute() calls findNeighbor per moved point (.cpp:12-27).  Upstream's
                                  tree (srrg2_core, not in the reference tree) is restated as SURVEY.md App. A.4 believes it: split through the
                                  mean along the principal eigenvector until a node holds fewer than min_leaf_points points or is smaller than
                                  max_leaf_range; descent to the single leaf on the query's side, no backtracking -- hence APPROXIMATE: it may
                                  return a farther neighbour than LSM2D_FINDER_NN, or none */
} lsm2d_finder;

typedef enum { LSM2D_ROBUST_NONE = 0, LSM2D_ROBUST_CAUCHY = 1 } lsm2d_robustifier;

/* One aligner slice = finder + factor + robustifier, i.e. one AlignerSliceProcessorLaser2D[WithSensor]
 * (registration/aligner_slice_processor_laser_2d.h:7-42) with the config fields of MULTI.json:160-188. */
typedef struct {
  int32_t         finder;                  /* lsm2d_finder */
  lsm2d_projector projector;               /* projective finder: param_projector (.h:22-26) */
  float           point_distance;          /* projective: param_point_distance, default 0.5 (.h:16-20) */
  float           normal_cos;              /* all finders: param_normal_cos, default 0.8 */
  float           max_distance;            /* NN / DISTMAP: param_max_distance_m (kd .h:23, nn .h:20-24) */
  float           resolution;              /* DISTMAP: param_resolution [m/pixel] (nn .h:25-29) */
  int32_t         robustifier;             /* lsm2d_robustifier (RobustifierCauchy, MULTI.json:153-158) */
  float           chi_threshold;           /* Cauchy tau */
  int32_t         min_num_correspondences; /* slice skipped when #pairs <= this (MULTI.json:179,391,591) */
  float           sensor_in_robot[3];      /* WithSensor variant (registration/aligner_slice_processor_laser_2d_impl.cpp:7-10); zeros = plain */
  float           kd_max_leaf_range;       /* KDTREE: param_max_leaf_range  (kd .h:26-28); <= 0: the class default 1e-2 */
  int32_t         kd_min_leaf_points;      /* KDTREE: param_min_leaf_points (kd .h:29-33); <= 0: the class default 20 */
} lsm2d_slice_params;

/* MultiAligner2D parameters (MULTI.json:700-732, :602-630) + GN damping (MULTI.json:254-259). */
typedef struct {
  int32_t max_iterations;
  int32_t min_num_inliers;
  float   damping;
  /* device-side counterpart of the aligner's "termination_criteria" (MULTI.json:627-630,729-731: unset in both shipped aligners = always
   * max_iterations; the solver's SimpleTerminationCriteria, MULTI.json:218-223, documents epsilon as the "ratio of decay of chi2 between
   * iteration"): 0 = off; > 0: the loop stops after an iteration whose total chi^2 (inliers + kernelised outliers) differs from the
   * previous iteration's by less than epsilon times itself.  The iteration that triggers the stop is still solved and applied. */
  float   termination_chi_epsilon;
  /* MultiAligner2D's two remaining options (MULTI.json:606-610,704-708; both 0 in the shipped configurations).  The upstream class is not in
   * the reference tree, so their semantics are RESTATED from the parameters' own doc strings (PARITY.md section 2, [UPSTREAM-MEMORY]):
   * enable_inlier_only_runs ("toggles additional inlier only runs if sufficient inliers are available"): when the regular loop ended without
   *   a failure and its last iteration counted n_inliers >= min_num_inliers, a second loop of up to max_iterations iterations follows in which
   *   a pair whose factor is not an inlier under its slice's robustifier (chi^2 >= chi_threshold) contributes nothing and an inlier contributes
   *   with weight 1 (no kernel); finders, gates, statistics, the termination criterion (afresh) and the status rules are those of the regular
   *   loop.  An alignment then runs up to 2 * max_iterations iterations: see lsm2d_stats_capacity.
   * keep_only_inlier_correspondences ("toggles removal of correspondences which factors are not inliers in the last iteration"): the
   *   correspondences the aligner leaves in its slices (lsm2d_align_batch_pairs) hold only the pairs whose factor was an inlier in the last
   *   iteration; poses, information matrices and statistics do not depend on it. */
  int32_t enable_inlier_only_runs;
  int32_t keep_only_inlier_correspondences;
} lsm2d_aligner_params;
/* iterations one alignment may run under `aligner`, i.e. the row length of out_stats: max_iterations, doubled with enable_inlier_only_runs (>= 1) */
int32_t lsm2d_stats_capacity(const lsm2d_aligner_params* aligner);

/* Optional odometry-prior cue (AlignerSliceOdom2DPrior, MULTI.json:402-422): e = t2v(Z^-1 X), information omega. */
typedef struct {
  float z[3];
  float omega[9];
} lsm2d_prior;

/* Correspondence(fixed_idx, moving_idx) (registration/correspondence_finder_kd_tree_2d.cpp:25) */
typedef struct { int32_t fixed_idx, moving_idx; } lsm2d_correspondence;

/* per-iteration statistics = what aligner->iterationStats() prints (apps/visual_test_aligner_2d.cpp:156) */
typedef struct {
  int32_t n_correspondences, n_inliers, n_outliers;
  float   chi_inliers, chi_outliers;
  /* order-independent digest of the iteration's correspondence SET -- the pairs the reference aligner exposes per slice
   * (apps/visual_test_aligner_2d.cpp:129-143): the wrapping 64-bit sum of lsm2d_pair_hash(slice, fixed_idx, moving_idx) over every pair counted
   * in n_correspondences (all slices, skipped ones included).  Equal digests <=> the same pairs went into the iteration (up to a 2^-64 hash
   * collision); tests use it to tell "same pairs, different summation order" from "different pairs".  Computed only when statistics are asked for. */
  uint32_t pair_digest_lo, pair_digest_hi;
} lsm2d_iteration_stats;
/* the per-pair hash behind pair_digest -- plain 32-bit integer arithmetic, the same on the host, in the kernels and in the CPU oracle:
 *   a = fixed_idx * 0x9E3779B1;  b = (moving_idx ^ (slice * 0x632BE5AB)) * 0x85EBCA77;
 *   lo = a ^ rotl(b, 13);  hi = b ^ rotl(a, 19);  lo += rotl(lo, 17) ^ b;  hi += rotl(hi, 11) ^ a;  hash = hi << 32 | lo
 * (so a caller holding a correspondence vector can form the digest it should see) */
uint64_t lsm2d_pair_hash(uint32_t slice, uint32_t fixed_idx, uint32_t moving_idx);

typedef struct lsm2d_context  lsm2d_context;
typedef struct lsm2d_cloudset lsm2d_cloudset;

/* ---- library / context ------------------------------------------------------------------------ */
int         lsm2d_version(void);
const char* lsm2d_status_string(int status);
/* text of the last HIP failure seen by this context (or by the library when ctx == NULL) */
const char* lsm2d_last_error(const lsm2d_context* ctx);
/* hip_stream: an existing hipStream_t to launch on (e.g. the caller's torch stream), or NULL to own one */
int  lsm2d_create(int device_id, void* hip_stream, lsm2d_context** out_ctx);
/* waits for the stream, frees the context.  Cloud sets still alive on it stay the caller's to destroy (any time), but no call takes them any more. */
/* (batches begun with lsm2d_align_batch_begin must have been waited for: the call brings every stream of the context to rest before it frees anything, but a
 * lsm2d_pending that is still outstanding refers to the context and must not be used afterwards) */
void lsm2d_destroy(lsm2d_context* ctx);
/* blocks until everything queued on the context's stream has finished */
int  lsm2d_synchronize(lsm2d_context* ctx);
/* Options: the WHOLE public set (16 keys; anything else is LSM2D_BAD_ARGUMENT "unknown option").  Results never depend on any of them but "sum_order".
 * "sum_order": 0 (default) = H, b and the chi^2 statistics of an iteration are added in TREES (a thread's pairs, then the 64 lanes of a wave, then the eight
 *   waves): the fast order.  1 = added PAIR AFTER PAIR in the order of the reference's correspondence vector -- ascending canvas column for the projective
 *   finder (registration/correspondence_finder_projective_2d.cpp:55-74), ascending moving index for the point-query finders
 *   (registration/correspondence_finder_kd_tree_2d.cpp:12-27) -- one factor after the other into H and b as octave/solver/nicp_post.m:69-90 does, slice
 *   totals added in slice order.  Both orders use the same per-pair terms and the same fused operations; they differ in the association of fp32 sums,
 *   i.e. in the last bits of H and b, which a pair sitting on a gate can turn into another correspondence set a few iterations later (PARITY.md section 0).
 *   With 1 the aligner (lsm2d_align_batch and its begin / wait / pairs forms, every finder kind, priors, sensor offsets, the split path) and
 *   lsm2d_linearize equal the sequential fp32 oracle (oracle/: lsmo_align_f, lsmo_linearize_f) BIT FOR BIT.  Cost: the pairs' terms go through LDS (14 KB
 *   more per workgroup) and one wave adds them one after the other (a quad of lanes per quantity): configs[1] (1000 scans vs a 100k-point map) takes
 *   about 1.2 x the default order's step (1.03 M against 1.24 M alignments/s: DESIGN.md section 5; the point-query finders in the tracker's wiring, whose 100 000
 *   queries per iteration all pass a barrier per 512, 3 - 5 x).  The latency kernel has a reference-order form too (k_align_pair<true>: both slices' pairs
 *   added at once, one wave per slice): with "sum_order" 1 it takes every SINGLE-alignment call with one or two projective slices (the live tracker's and the
 *   standalone aligner's call) and every call with align_path 3, whenever its LDS layout fits ("last_align_path" reads 3); batches of two and more alignments
 *   take k_align_seq by themselves (one workgroup per alignment).  The tracker's step (two 721-column slices + prior): 0.114 ms asynchronous against 0.204 on
 *   k_align_seq and 0.059 in the tree order.
 * "align_width": the launch form of a culled projective batch (k_align): 0 = automatic (default: workgroups of 512 threads; of 256 -- six alignments per CU round instead
 *   of four -- for batches just above a multiple of 1024 alignments, where the last few would otherwise run a round of their own on an empty chip; PACKED -- one round
 *   of 1024 workgroups, the lightest alignments two to a workgroup, one after the other -- for 1025 .. 1048 and 1537 .. 2047 alignments, and for up to 32 more than 2048 or 3072; with "sum_order" 1, which has no narrow form: 1025 .. 1600), 512 / 256 = always that
 *   width, 1024 = packed whenever the batch has more than 1024 and fewer than 4096 alignments and is not a multiple of 1024.  The narrow workgroups keep the wide kernel's 512 virtual threads in the bin walk and the
 *   sums, a packed workgroup runs the same kernel body twice: bit-identical results (get: "last_align_width": 512, 256, or 1024 for a packed launch).
 *   Only 0, 256, 512 and 1024 are accepted; any other value is LSM2D_BAD_ARGUMENT and leaves the option as it was.
 * "align_path": 0 = automatic (default), 1 = always one workgroup per alignment (k_align), 2 = always the split path (k_split_project +
 *   k_split_finish per iteration; projective slices only), 3 = the latency kernel whenever the batch has one or two projective slices
 *   (k_align_pair: 512 threads per slice, two slices' passes side by side in one workgroup; automatic for <= 256 alignments -- with "sum_order" 1 for
 *   single alignments only, see there).  All paths return
 *   bit-identical results; the split path is for a handful of alignments against a large cloud, the latency kernel for calls that cannot fill
 *   the chip (the live tracker).
 * "kernel_timing": 1 records HIP events around the hot-path launches so that lsm2d_last_kernel_ms can report them; 0 (default) does not -- the
 *   two timed events per operation cost a latency-critical caller such as the live tracker ~20 % of its step -- and lsm2d_last_kernel_ms
 *   returns LSM2D_BAD_ARGUMENT.  "clock_stride" (default 0 = ~32 per launch): with kernel timing on, every clock_stride-th workgroup of a k_align
 *   launch stamps its shader-cycle and 100 MHz counters (get: "last_kernel_clock_khz", "last_workgroup_lifetime_ns").
 * "find_path": 0 = automatic (default: a point-query lsm2d_find_correspondences call with more queries than one workgroup takes in a trip runs on
 *   many workgroups, two launches; the projective finder z-buffers a cloud of more than 32768 points over many workgroups first), 1 = always one
 *   workgroup; same pairs, same order.
 * "zero_copy_max" (default 256): batches of at most this many alignments read their arguments from, and write their results to, pinned host memory
 *   directly (no transfers, status words polled) -- above 256 alignments only when the batch carries no index arrays; measured slower than the
 *   transfers at 1000 alignments.  0 switches the zero-copy form off.
 * "cull" (default 1): the aligner's projective slices drop, exactly, the parts of a map-sized moving cloud that cannot yield a pair (and its
 *   point-query slices the tiles of queries nobody is near); 0 streams everything.  "cull_margin_um" (10000) / "cull_margin_urad" (2000, at most
 *   50000): how far a pose may move before the kept survivor lists of the projective culling are rebuilt.
 * "cand_lists" (default 1): k_align on a single-slice culled projective batch keeps, once an alignment has run "cand_first_it" (default 3) iterations, a CANDIDATE
 *   list: the indices of the streamed map points that can still win, or beat the winner of, a z-buffer column under any transform within "cand_margin_um" (default
 *   30, at most 100000) micrometres / "cand_margin_urad" (default 3, at most 50000) microradians of the one the list was built at.  While the pose stays there an
 *   iteration gathers those points (a few thousand where it would stream 41 000 on a 100k-point map) instead of streaming the kept survivor list; a pose that leaves
 *   drops the list, and up to "cand_max_builds" (default 2) lists are built per alignment.  "cand_cap" (default 3328; lowered to the room in LDS): entries a list
 *   may hold -- a longer one is not used and the alignment goes on streaming.  The moving canvas keeps its bits, hence every result does, whatever the values.  A
 *   batch gets lists (and the kernel that carries them, k_align_cand) only where they pay and fit: one slice, "sum_order" 0, the wide unpacked launch form, at most one
 *   dispatch round of alignments (4 x the CUs: what the lists shorten is the tail a few long alignments leave on an emptying chip), a moving cloud of at most 48 points
 *   per entry of room (a denser map's lists do not fit), no other batch in flight when it is begun, and room in LDS beside four workgroups per CU.  Every other batch
 *   runs exactly as without the option.  0: no lists.
 * "cand_queue" (default 1): how a list is built.  1: the iteration that builds it tests every point it streams against the blocker its column has at that moment and
 *   notes the points that test cannot drop yet -- about a quarter of them on a 100k-point map -- in a queue in device memory; the list is then collected from the
 *   queue.  0: from the streamed points once more.  The list is the same set, and every result keeps its bits.  "cand_queue_cap" (default and largest value 16384;
 *   0 .. 16384): the queue's entries per alignment (4 bytes each, allocated for batches that get lists only); a build that notes more falls back to 0's pass.
 * "balance" (default 1): batches of 257 .. 4096 culled alignments are placed on the chip by estimated work (one small launch ahead of k_align; a
 *   batch run again with unchanged sets and start poses keeps its placement: get "last_cull_estimate"); 0: workgroup i runs alignment i.
 * "fast_forward" (0, 1 or 2; default 2): k_align and its packed, narrow and reference-order forms stop iterating once the pose repeats.  One Gauss-Newton
 *   iteration is a pure function of the pose it starts at, so when the pose after an iteration equals, BIT FOR BIT, the pose one of the last sixteen iterations
 *   started at, the remaining iterations only go round that cycle (period 1: a fixed point of the fp32 arithmetic).
 *     2: the alignment finishes there.  Its last iteration would repeat one the cycle has already been through: that one's start and end pose, information
 *        matrix and inlier count were kept, and the results are written from them; no iteration runs behind the match.
 *     1: whole periods are skipped and the remainder of a period runs again (the rule before 2 existed; kept as the A/B switch inside one library).
 *     0: every iteration runs.
 *   Pose, information matrix, status, iteration count (skipped iterations are counted) and every iteration's statistics row are those of the full run whatever
 *   the value.  Without effect -- every iteration runs -- with termination_chi_epsilon > 0, with enable_inlier_only_runs, in zero-copy batches (at most
 *   "zero_copy_max" alignments: their results and statistics live in pinned host memory), on the split path and in the latency kernel.
 * "grid_big_threshold" (default 16384): fixed clouds of at least this many points get the NN finder's search grid built by chip-wide kernels
 *   (histogram / scan / scatter over many workgroups) instead of one workgroup per cloud.
 * "distmap_build": 0 = automatic (default: the distance maps of CorrespondenceFinderNN2D are built from the points' side, one disc of atomic minima
 *   per point, whenever squared pixel distance and point index pack into 31 bits), 1 = always the per-pixel gather build; identical maps.
 * "kd_lds_nodes" (default 1536): nodes of the fixed cloud's KD-tree a k_align workgroup keeps in LDS (its top levels).
 * Read-only (lsm2d_get_option): "last_align_path" (1 k_align, 2 split, 3 slice pair), "last_query_cull", "last_cull_estimate", "last_cand_builds" / "last_cand_iterations" /
 *   "last_cand_overflows" / "last_cand_fallbacks" (the latest aligner call that asked for statistics: candidate lists built, iterations a list served, lists too long
 *   to be used, builds whose queue was too short; a call without statistics hands no counter over and leaves them as they were), "last_kd_levels",
 *   "last_kd_nodes", "last_kernel_clock_khz", "last_workgroup_lifetime_ns", "max_dyn_lds", "uploads" (host-to-device cloud uploads queued so far:
 *   lsm2d_cloudset_create / _upload / lsm2d_preprocess_scans_refill), "last_h2d_bytes", "experiments" (1: this library was built with
 *   -DLSM2D_EXPERIMENTS and also knows the A/B knobs of DESIGN.md App. A; the shipped library: 0), "live_handles" (device buffers, pinned host
 *   buffers, events and streams the library holds at this moment, over ALL contexts and sets of the process -- a set may outlive its context; whatever
 *   a context and its sets acquired is gone from the count once both are destroyed, in either order: what a leak test on a shared GPU can assert). */
int  lsm2d_set_option(lsm2d_context* ctx, const char* key, int64_t value);
/* reads a knob back; also "last_align_path": what the most recent lsm2d_align_batch ran (1 k_align, 2 split, 3 slice pair) */
int  lsm2d_get_option(lsm2d_context* ctx, const char* key, int64_t* out_value);
/* device time [ms] of the hot-path kernel launches of the most recent call (HIP events on the context's stream);
 * needs lsm2d_set_option(ctx, "kernel_timing", 1) */
int  lsm2d_last_kernel_ms(lsm2d_context* ctx, float* out_ms);

/* ---- clouds: device-resident ragged sets of PointNormal2fVectorCloud ---------------------------
 * Replace: the raw non-owning PointNormal2fVectorCloud* the reference hands to setFixed / setMoving
 * (apps/visual_test_correspondence_finder_projective_2d.cpp:74-75).  A set holds n_clouds clouds
 * packed back to back; offsets[n_clouds+1] delimit them (NULL when n_clouds == 1).  The local map
 * shared by a batch is a set with ONE cloud. */
int  lsm2d_cloudset_create(lsm2d_context* ctx, const float* points_xynn, const int32_t* offsets,
                           int32_t n_clouds, int64_t total_points, lsm2d_cloudset** out_set);
/* same, from points already in device memory on ctx's device (float4 per point); offsets stay host.
 * ORDERING: the points are read on the CONTEXT's stream.  Whatever produced them (another stream, e.g. torch's current stream) must have
 * finished -- synchronise that stream or make it wait-for -- or the context must have been created on that very stream
 * (lsm2d_create's hip_stream); the library cannot know the producer.  The same holds for device-resident `ranges` below. */
int  lsm2d_cloudset_create_from_device(lsm2d_context* ctx, const void* d_points_xynn, const int32_t* offsets,
                                       int32_t n_clouds, int64_t total_points, lsm2d_cloudset** out_set);
/* a single growable cloud (count 0) with room for capacity_points: the device-resident local map / clipped scene */
int  lsm2d_cloudset_create_reserved(lsm2d_context* ctx, int64_t capacity_points, lsm2d_cloudset** out_set);
/* n_clouds growable clouds (count 0 each), each with room for capacity_per_cloud points: the local maps of N trackers, or their clipped
 * scenes (lsm2d_clip_scene_batch / lsm2d_merge_scene_batch).  Cloud i occupies the fixed slot that starts at point i * capacity_per_cloud,
 * rounded up to an even point.  Sizes written by the batched calls stay on the device until asked for (lsm2d_cloudset_cloud_sizes: one
 * wait for all of them).  lsm2d_align_batch, lsm2d_find_correspondences, lsm2d_project and lsm2d_cloudset_download read such a set
 * like any multi-cloud set; the single-cloud calls (lsm2d_cloudset_upload, lsm2d_clip_scene[_voxelized], lsm2d_merge_scene[s],
 * lsm2d_preprocess_scan_into, lsm2d_preprocess_scans_refill) refuse it (LSM2D_BAD_ARGUMENT), even with n_clouds = 1. */
int  lsm2d_cloudset_create_reserved_many(lsm2d_context* ctx, int32_t n_clouds, int64_t capacity_per_cloud, lsm2d_cloudset** out_set);
/* empties clouds cloud_index[0 .. n) of a set of lsm2d_cloudset_create_reserved_many (cloud_index NULL: every cloud, n is not read) --
 * a tracker that starts a new local map.  Asynchronous: queued on the context's stream, nothing waits. */
int  lsm2d_cloudset_clear_clouds(lsm2d_cloudset* set, int32_t n, const int32_t* cloud_index);
/* refill an existing SINGLE-cloud set in place (no allocation); LSM2D_CAPACITY_EXCEEDED when it does not fit.  The points are
 * copied into the set's pinned staging buffer before the call returns and travel asynchronously on the context's stream:
 * for scan-sized sets (<= 16 384 points) whoever reads the set first queues their unpacking, and a single-alignment projective
 * lsm2d_align_batch unpacks its fixed sets inside the aligner kernel -- the live tracker's scans cost no launch of their own. */
int  lsm2d_cloudset_upload(lsm2d_cloudset* set, const float* points_xynn, int64_t n_points);
/* copy cloud `cloud_index` back to the host as (x, y, nx, ny) rows; *out_n = its size */
int  lsm2d_cloudset_download(const lsm2d_cloudset* set, int32_t cloud_index, float* out_points_xynn, int64_t capacity, int64_t* out_n);
void lsm2d_cloudset_destroy(lsm2d_cloudset* set);
int32_t lsm2d_cloudset_num_clouds(const lsm2d_cloudset* set);
int64_t lsm2d_cloudset_num_points(const lsm2d_cloudset* set);
/* points in cloud `cloud_index` (-1 when out of range).  After an asynchronous lsm2d_clip_scene / lsm2d_merge_scene the size
 * of the set they wrote is known to the device only; the size queries (and lsm2d_cloudset_download) then wait for the stream. */
int64_t lsm2d_cloudset_cloud_size(const lsm2d_cloudset* set, int32_t cloud_index);
/* all sizes at once (a preprocessed batch holds thousands of clouds): fills out_sizes[0 .. min(capacity, num_clouds)), returns the number written or a negative status */
int32_t lsm2d_cloudset_cloud_sizes(const lsm2d_cloudset* set, int32_t* out_sizes, int32_t capacity);

/* ---- a3: PointNormal2fProjectorPolar::compute -------------------------------------------------
 * One polar z-buffer pass of cloud `cloud_index` seen through `pose` (points are mapped by pose,
 * i.e. pose = camera_pose^-1).  Outputs (host, each canvas_cols long; any may be NULL):
 * source index or -1, depth, transformed point (x, y, nx, ny). */
int lsm2d_project(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* cloud,
                  int32_t cloud_index, const float pose[3], int32_t* out_source_idx, float* out_depth,
                  float* out_transformed_xynn);

/* ---- RawDataPreprocessorProjective2D::compute, batched (sensor_processing/raw_data_preprocessor_projective_2d.cpp:13-51,
 * :77-104): ranges of n_scans LaserMessages -> one cloud set of n_scans PointNormal2fVectorClouds that never leaves the
 * device (ready to be the aligner's `fixed`).  Per scan: polar unprojection with the reference's sensor matrix
 * [[n/(angle_max-angle_min), n/2]], sliding-window normals (NormalComputator1DSlidingWindow: normal_point_distance,
 * normal_min_points; MULTI.json:845-853), voxelisation at voxelize_resolution (.h:41-45; <= 0 keeps every valid point).
 * n_beams <= 2048.  The upstream pieces are not in the reference tree: semantics as restated in oracle/lsm2d_oracle.c F2.1-F2.3. */
typedef struct {
  int32_t n_beams;
  float   angle_min, angle_max;    /* LaserMessage angle_min / angle_max [rad] */
  float   range_min, range_max;    /* max(message, param) / min(message, param), .cpp:83-84 */
  float   normal_point_distance;
  int32_t normal_min_points;
  float   voxelize_resolution;
} lsm2d_preprocessor;
/* `ranges` [n_scans][n_beams] may live in pageable host memory (staged through the context's pinned buffer), in pinned / registered host
 * memory (copied from directly) or in device memory of the context's device (read in place: nothing crosses the host link; see the
 * ORDERING note at lsm2d_cloudset_create_from_device: the producer's stream must have been synchronised with). */
int lsm2d_preprocess_scans(lsm2d_context* ctx, const lsm2d_preprocessor* params, const float* ranges,
                           int32_t n_scans, lsm2d_cloudset** out_set);
/* The same operation INTO a set that lsm2d_preprocess_scans made for the same number of scans and beams: no allocation, nothing waits (RawDataPreprocessorProjective2D::compute
 * per incoming message, sensor_processing/raw_data_preprocessor_projective_2d.cpp:13-51, for a BATCH of fresh messages per step).  Pinned `ranges` are fetched by an
 * asynchronous copy, pageable ones staged first, device-resident ones read in place; the clouds' sizes stay on the device (lsm2d_cloudset_cloud_size asks for them: a wait).
 * Same kernel, same bits as lsm2d_preprocess_scans.  The caller keeps `ranges` untouched until the batch that reads the set has been waited for.
 * While a batch is in flight the refill runs on a stream of its own, ordered before the next aligner call on this context (and before lsm2d_cloudset_cloud_size /
 * lsm2d_synchronize); other entry points that read a set refilled while a batch was in flight: lsm2d_synchronize first. */
int lsm2d_preprocess_scans_refill(lsm2d_context* ctx, const lsm2d_preprocessor* params, const float* ranges, int32_t n_scans, lsm2d_cloudset* set);
/* The live tracker's form of the same operation: ONE scan into an existing reserved single-cloud set (capacity >= n_beams) --
 * no allocation, nothing waits: the ranges are staged in the set's pinned buffer, the cloud's size stays on the device until
 * somebody asks (see lsm2d_clip_scene).  Same kernel, same bits as lsm2d_preprocess_scans with n_scans = 1.  Unless kernel timing is
 * on, the launch itself is queued by the set's first reader, and an lsm2d_align_batch that reads several such sets (front and rear
 * scanner) queues them as one launch, one workgroup per scan. */
int lsm2d_preprocess_scan_into(lsm2d_context* ctx, const lsm2d_preprocessor* params, const float* ranges /* host [n_beams] */,
                               lsm2d_cloudset* out_reserved_set);

/* ---- SceneClipperProjective2D::compute (mapping/scene_clipper_projective_2d.cpp:11-65, voxelize_resolution = 0
 * as in both shipped configs, MULTI.json:673-683): what the sensor at robot_in_local_map * sensor_in_robot sees of
 * `full_scene` -- at most one point per projector column, ascending column, expressed in the ROBOT frame.
 * `clipped` is a reserved single-cloud set (capacity >= canvas_cols) that is overwritten and stays on the device,
 * ready to be the aligner's moving cloud.  out_source_idx (host, canvas_cols entries) may be NULL.
 * out_n_points == NULL (then out_source_idx must be NULL too): ASYNCHRONOUS -- the call only queues the work on the context's
 * stream and nothing is copied back; lsm2d_align_batch (projective slices), lsm2d_merge_scene and another lsm2d_clip_scene accept
 * the sets as they are, so a tracker step (clip -> upload -> align -> merge) synchronises once, for the aligner's pose. */
int lsm2d_clip_scene(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* full_scene,
                     int32_t scene_index, const float robot_in_local_map[3], const float sensor_in_robot[3],
                     lsm2d_cloudset* clipped, int32_t* out_n_points, int32_t* out_source_idx);

/* The same with the clipper's voxelize_resolution > 0 branch (mapping/scene_clipper_projective_2d.cpp:36-48): the clipped points, still
 * in the sensor frame, are voxelised with coefficients (res, res, 0.1, 0.1) -- equal keys averaged, ascending key order (assumption
 * F2.3, oracle/lsm2d_oracle.c) -- and then moved to the robot frame.  out_source_idx must be NULL (a voxel has no source point);
 * canvas_cols <= 2048; voxelize_resolution <= 0 is lsm2d_clip_scene. */
int lsm2d_clip_scene_voxelized(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* full_scene,
                               int32_t scene_index, const float robot_in_local_map[3], const float sensor_in_robot[3],
                               float voxelize_resolution, lsm2d_cloudset* clipped, int32_t* out_n_points, int32_t* out_source_idx);

/* ---- MergerProjective2D::compute (mapping/merger_projective_2d.cpp:9-100): folds `measurement` (cloud
 * measurement_index, in its own sensor/robot frame) into the single-cloud reserved set `scene`, in place: per projector
 * column seen from measurement_in_scene a measurement point is merged into (|depth difference| < merge_threshold),
 * replaces (it lies behind) or is appended next to the scene's nearest point; measurement depths beyond
 * 0.9*range_max are ignored.  out_counts[3] = {new, merged, replaced} (may be NULL).
 * out_scene_size == NULL (then out_counts must be NULL too): ASYNCHRONOUS, see lsm2d_clip_scene. */
int lsm2d_merge_scene(lsm2d_context* ctx, const lsm2d_projector* projector, lsm2d_cloudset* scene,
                      const lsm2d_cloudset* measurement, int32_t measurement_index, const float measurement_in_scene[3],
                      float merge_threshold, int32_t* out_scene_size, int32_t* out_counts);
/* Several measurements merged into the scene one after the other, exactly as n calls of lsm2d_merge_scene in this order would (the live
 * tracker merges the front and the rear scan at the corrected pose) -- but as ONE launch when the scene and the measurements are small
 * (<= 4 measurements, scene + (n-1) canvas_cols <= 32 768 points, kernel timing off).  meas_index NULL: cloud 0 of every set;
 * measurement_in_scene: [n][3]; out_size NULL: asynchronous (see lsm2d_clip_scene); out_counts: [n][3] (new, merged, replaced) or NULL. */
int lsm2d_merge_scenes(lsm2d_context* ctx, const lsm2d_projector* projector, lsm2d_cloudset* scene, int32_t n_measurements,
                       const lsm2d_cloudset* const* measurements, const int32_t* meas_index, const float* measurement_in_scene,
                       float merge_threshold, int32_t* out_size, int32_t* out_counts);

/* ---- N independent trackers per call (one robot model: one projector and one sensor_in_robot for all of them) ----------------------
 * Each tracker's result is the bits the single-tracker call gives for it; one workgroup per tracker, no workgroup waits for another.
 * lsm2d_clip_scene for n_trackers at once (voxelize_resolution 0): tracker i clips cloud scene_index[i] (NULL: i) of `scenes` at
 * robot_in_local_map[i] * sensor_in_robot into cloud i of `clipped`, a set of lsm2d_cloudset_create_reserved_many with >= n_trackers
 * clouds of >= canvas_cols points.  Any scene size, sizes known to the device only included, is clipped without a wait.
 * out_n_points [n_trackers] or NULL (ASYNCHRONOUS: nothing waits, the sizes stay on the device). */
int lsm2d_clip_scene_batch(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* scenes, int32_t n_trackers,
                           const int32_t* scene_index, const float* robot_in_local_map /* [n_trackers][3] */, const float sensor_in_robot[3],
                           lsm2d_cloudset* clipped, int32_t* out_n_points);
/* lsm2d_clip_scene_voxelized for n_trackers at once -- the clipper's voxelize_resolution > 0 branch (mapping/scene_clipper_projective_2d.cpp:36-48;
 * the class default is 0.1) in the SAME single launch: each tracker's workgroup keeps its clipped points in LDS, in the sensor frame, voxelises
 * them with coefficients (res, res, 0.1, 0.1) and writes only the voxels, moved to the robot frame, to cloud i of `clipped`.  Each tracker has the
 * bits and the count of lsm2d_clip_scene_voxelized for the same scene, pose, offset and resolution.  No source indices (a voxel has no source
 * point).  Arguments, set requirements and the asynchronous form (out_n_points NULL; the host's bound per cloud is canvas_cols: a voxelised cloud
 * never grows) as lsm2d_clip_scene_batch; canvas_cols <= 2048, more is LSM2D_CAPACITY_EXCEEDED and nothing is launched.
 * voxelize_resolution <= 0 is lsm2d_clip_scene_batch. */
int lsm2d_clip_scene_voxelized_batch(lsm2d_context* ctx, const lsm2d_projector* projector, const lsm2d_cloudset* scenes, int32_t n_trackers,
                                     const int32_t* scene_index, const float* robot_in_local_map /* [n_trackers][3] */, const float sensor_in_robot[3],
                                     float voxelize_resolution, lsm2d_cloudset* clipped, int32_t* out_n_points);
/* lsm2d_merge_scenes for n_trackers at once: cloud scene_index[i] (NULL: i) of `scenes` (a set of lsm2d_cloudset_create_reserved_many;
 * no index twice) gets cloud meas_index[k * n_trackers + i] (NULL: i) of measurements[k], k = 0 .. n_measurements - 1 (1 .. 4), merged
 * one after the other at measurement_in_scene[i][k] ([n_trackers][n_measurements][3]).  All or nothing: when a scene may lack room for
 * n_measurements * canvas_cols more points by the host's upper bounds, the sizes are fetched (one wait); a scene that really lacks it is
 * LSM2D_CAPACITY_EXCEEDED (lsm2d_last_error names the tracker) and nothing is launched.  out_sizes [n_trackers] and
 * out_counts [n_trackers][n_measurements][3] (new, merged, replaced) or NULL (then both: ASYNCHRONOUS). */
int lsm2d_merge_scene_batch(lsm2d_context* ctx, const lsm2d_projector* projector, lsm2d_cloudset* scenes, int32_t n_trackers,
                            const int32_t* scene_index, int32_t n_measurements, const lsm2d_cloudset* const* measurements,
                            const int32_t* meas_index, const float* measurement_in_scene, float merge_threshold,
                            int32_t* out_sizes, int32_t* out_counts);

/* ---- plugin interface #1: CorrespondenceFinder_::compute ---------------------------------------
 * Replaces compute() of the three finders (registration/correspondence_finder_projective_2d.cpp:18-77,
 * registration/correspondence_finder_kd_tree_2d.cpp:5-38, registration/correspondence_finder_nn_2d.cpp:54-97)
 * after setFixed / setMoving / setLocalMapInSensor / setCorrespondences.  Pairs come out in the
 * reference's order (ascending column for PROJECTIVE, ascending moving index otherwise). */
int lsm2d_find_correspondences(lsm2d_context* ctx, const lsm2d_slice_params* slice,
                               const lsm2d_cloudset* fixed, int32_t fixed_index,
                               const lsm2d_cloudset* moving, int32_t moving_index,
                               const float local_map_in_sensor[3],
                               lsm2d_correspondence* out_pairs, int32_t capacity, int32_t* out_n_pairs);
/* CorrespondenceFinder_::compute for n_items independent (fixed, moving, pose) triples in ONE launch: item i matches cloud
 * fixed_index[i] of `fixed` against cloud moving_index[i] of `moving` under local_map_in_sensor[i].  All four finder kinds; per item the
 * pairs and their order are those of lsm2d_find_correspondences, bit for bit (one workgroup per item runs the single call's device
 * functions; a cloud of any size is z-buffered by the item's own workgroup).
 * Indices: the rule of lsm2d_batch -- NULL means cloud i, or cloud 0 of a set that holds one cloud (the set must then hold 1 or n_items
 * clouds); indices may repeat.  Sets in any state (sizes known to the device only, unpacking / preprocessing pending) are read: counts are
 * resolved and pending work is flushed once for the whole batch, and the set's search structure is built or reused once.
 * pair_capacity must hold the largest possible vector -- canvas_cols for the projective finder, the largest cloud of `moving` otherwise --
 * or the call returns LSM2D_CAPACITY_EXCEEDED before anything is launched and writes nothing.  n_items == 0 is a successful no-op.
 * The pairs pass through a device buffer of fixed size (2^21 pairs): a batch whose n_items x pair_capacity exceeds it runs as several
 * launches over consecutive items.  The call waits once per launch.  With one batch in flight (lsm2d_align_batch_begin) it works; with
 * two it is refused (LSM2D_BAD_ARGUMENT), like every call that moves data. */
int lsm2d_find_correspondences_batch(lsm2d_context* ctx, const lsm2d_slice_params* slice,
                                     const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                                     const lsm2d_cloudset* moving, const int32_t* moving_index,
                                     int32_t n_items, const float* local_map_in_sensor /* [n_items][3] */,
                                     lsm2d_correspondence* out_pairs /* [n_items][pair_capacity] */,
                                     int32_t pair_capacity, int32_t* out_n_pairs /* [n_items] */);

/* ---- factor: SE2Plane2PlaneErrorFactor over a correspondence vector ----------------------------
 * Replaces the per-correspondence errorAndJacobian + robustifier + H/b accumulation of the
 * correspondence-driven factor bound at registration/aligner_slice_processor_laser_2d.h:4,8
 * (math: octave/solver/nicp_post.m:4-26,69-90). */
int lsm2d_linearize(lsm2d_context* ctx, const lsm2d_slice_params* slice,
                    const lsm2d_cloudset* fixed, int32_t fixed_index,
                    const lsm2d_cloudset* moving, int32_t moving_index,
                    const lsm2d_correspondence* pairs, int32_t n_pairs, const float pose[3],
                    float out_H[9], float out_b[3], lsm2d_iteration_stats* out_stats);
/* The same factor over n_items correspondence vectors in ONE launch (two in the tree order): what a caller with n_items pose hypotheses needs after
 * lsm2d_find_correspondences_batch -- the candidate loop of MultiLoopDetectorBruteForce2D (MULTI.json:964-986) reads exactly these statistics, and a
 * host with its own solver gets H AND b at the poses it chooses (registration/aligner_slice_processor_laser_2d.h:4,8; octave/solver/nicp_post.m:4-26,69-90).
 * Item i linearises pairs[i * pair_capacity .. + n_pairs[i]) between cloud fixed_index[i] of `fixed` and cloud moving_index[i] of `moving` at poses[i];
 * pairs / pair_capacity / n_pairs are laid out as lsm2d_find_correspondences_batch writes them, so its output feeds this call untouched.  Only the first
 * n_pairs[i] entries of a row are read or checked: the tails may be uninitialised.
 * Per item H, b, the counts, the chi^2 sums and the pair digest (slice 0) are those of lsm2d_linearize, bit for bit, in both orders of summation (option
 * "sum_order"): the single call's kernels and the batch's share their device functions and the item keeps the single call's launch shape.
 * Indices: the rule of lsm2d_batch (NULL: cloud i, or cloud 0 of a one-cloud set; the set then holds 1 or n_items clouds; indices may repeat).  Sets in any
 * state are read; counts are resolved and pending work is flushed once for the whole batch (one wait at most: the checks need the sizes).
 * n_items == 0 is a successful no-op; n_pairs[i] == 0 gives zeros and n_correspondences == 0.
 * Checked before anything is launched or written: n_pairs[i] outside [0, pair_capacity] and a pair index outside its item's clouds are
 * LSM2D_BAD_ARGUMENT, and lsm2d_last_error names the item.
 * The pairs pass through a device buffer of fixed size (2^21 pairs, an item counting with its pair_capacity; at most 65536 items): a batch beyond it runs as
 * several launches over consecutive items, one wait each -- the items are independent, no bit changes.  With one batch in flight (lsm2d_align_batch_begin) the call works;
 * with two it is refused (LSM2D_BAD_ARGUMENT).  "kernel_timing" / lsm2d_last_kernel_ms cover the (last) launch as they cover lsm2d_linearize's. */
int lsm2d_linearize_batch(lsm2d_context* ctx, const lsm2d_slice_params* slice,
                          const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                          const lsm2d_cloudset* moving, const int32_t* moving_index,
                          int32_t n_items,
                          const lsm2d_correspondence* pairs /* [n_items][pair_capacity] */, int32_t pair_capacity,
                          const int32_t* n_pairs /* [n_items] */, const float* poses /* [n_items][3] */,
                          float* out_H /* [n_items][9] */, float* out_b /* [n_items][3] */,
                          lsm2d_iteration_stats* out_stats /* [n_items] or NULL */);
/* Finder, then factor, for n_items pose hypotheses, with the pairs kept on the device: what the candidate loops of the loop detector and the relocaliser
 * (MULTI.json:964-986, :749-769) read of a candidate -- inlier / outlier counts, chi^2 sums -- and what a particle filter weighs by or a host with its own
 * solver needs at poses it chooses: H AND b (registration/aligner_slice_processor_laser_2d.h:4,8; octave/solver/nicp_post.m:4-26,69-90).  Item i matches
 * cloud fixed_index[i] of `fixed` against cloud moving_index[i] of `moving` at poses[i] with the slice's finder and linearises what it found at the same pose.
 * Per item H, b, the counts, the chi^2 sums and the pair digest (slice 0) are, bit for bit, those of lsm2d_find_correspondences_batch at poses[i] followed
 * by lsm2d_linearize_batch on what it wrote -- in both orders of summation (option "sum_order"), for all four finder kinds, with and without the Cauchy
 * robustifier; hence also those of the single calls.  An item that finds no pair returns zeros and n_correspondences == 0.
 * The pairs never leave the device: the finder's kernels write them into the lane's scratch and the factor's kernels (linearize_*_body, the single call's)
 * read them there, an item's count included.  There is no pair_capacity argument: every item's slot is the slice's largest possible vector (canvas_cols,
 * or the largest moving cloud).  There is no host-side check of pair indices (the pairs are the finder's own); the count is clamped to the slot on the device.
 * Indices: the rule of lsm2d_batch (NULL: cloud i, or cloud 0 of a one-cloud set; the set then holds 1 or n_items clouds; indices may repeat).  Sets in any
 * state are read; counts are resolved and pending work is flushed once for the whole batch; the fixed set's search structure is built or reused once.
 * A batch whose n_items x slot exceeds the 2^21-pair buffer runs as several launch groups over consecutive items, queued one behind the other and reusing
 * the same pair scratch; the items' arguments go up once, the results (16 words per item) come down in one copy, and the call waits ONCE, at its end.
 * n_items == 0 is a successful no-op.  A cloud index out of range is LSM2D_BAD_ARGUMENT, lsm2d_last_error names the item, nothing is launched or written.
 * Canvases that do not fit LDS are LSM2D_CAPACITY_EXCEEDED, as in lsm2d_find_correspondences_batch.  With one batch in flight (lsm2d_align_batch_begin) the
 * call works; with two it is refused (LSM2D_BAD_ARGUMENT).  "kernel_timing" / lsm2d_last_kernel_ms cover the last launch group, finder and factor together. */
int lsm2d_score_batch(lsm2d_context* ctx, const lsm2d_slice_params* slice,
                      const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                      const lsm2d_cloudset* moving, const int32_t* moving_index,
                      int32_t n_items, const float* poses /* [n_items][3] */,
                      float* out_H /* [n_items][9] */, float* out_b /* [n_items][3] */,
                      lsm2d_iteration_stats* out_stats /* [n_items] or NULL */);

/* lsm2d_score_batch's scoring, then the acceptance test of the candidate loops and the best k of the accepted hypotheses, ranked on the device: what the
 * loop detector's and the relocaliser's candidate loops (MULTI.json:964-986, :749-769) ask of n_items scored hypotheses -- "which pass, and which of those
 * are best?" -- without n_items result rows travelling to the host and being scanned there.
 * Scoring: every item is scored exactly as lsm2d_score_batch scores it -- the same kernels, the same launch groups, the same bits in both values of
 * "sum_order" -- and its row stays on the device.
 * Acceptance, in fp32 with IEEE division (LoopClosureSweep::accept of host/lsm2d.hpp without its status term): item i is accepted when
 *     n_inliers >= min_inliers,   chi_inliers / max((float) n_inliers, 1.f) <= max_chi_per_inlier,
 *     (float) n_inliers / (float) max(n_correspondences, 1) >= min_inlier_ratio.
 * A NaN on either side of a comparison rejects the item; {0, +Inf, 0} accepts every item whose chi_inliers is not NaN.
 * Ranking of the accepted items, a total order (the result is unique): n_inliers descending, then chi_inliers ascending compared on its bit pattern as
 * uint32 (its order as a value: the sum is non-negative and not NaN), then item index ascending.  What the reference's relocaliser ranks by is not in its
 * tree: the order is an assumption of this build (PARITY.md section 3).
 * Outputs: *out_n_accepted the number of accepted items among all n_items; *out_n_selected = min(k, n_accepted); out_index[0 .. n_selected) the item
 * indices, best first; rows j < n_selected of out_H / out_b / out_stats (each may be NULL) the bits lsm2d_score_batch returns for item out_index[j].
 * Entries at positions >= n_selected are not written.
 * 1 <= k <= LSM2D_SELECT_MAX_K: another k, a NULL select, out_index or count pointer is LSM2D_BAD_ARGUMENT, returned before anything is launched or
 * written.  n_items == 0 succeeds and sets both counts to 0.  Cloud-index and capacity errors and the refusal with two batches in flight are those of
 * lsm2d_score_batch; nothing is written then, the counts included.
 * Up: the items' arguments, once.  Down: ONE copy of the two counts, k indices and k rows (16 + 68 k bytes, whatever n_items is).  ONE wait, at the end of
 * the call, however many launch groups the batch needs.  "kernel_timing" / lsm2d_last_kernel_ms cover the last launch group plus the selection. */
#define LSM2D_SELECT_MAX_K 1024
typedef struct {
  int32_t min_inliers;          /* relocalize_min_inliers        (MULTI.json:982 / :765) */
  float   max_chi_per_inlier;   /* relocalize_max_chi_inliers    (:979 / :762) */
  float   min_inlier_ratio;     /* relocalize_min_inliers_ratio  (:985 / :768) */
} lsm2d_select_params;

int lsm2d_score_select(lsm2d_context* ctx, const lsm2d_slice_params* slice,
                       const lsm2d_cloudset* fixed, const int32_t* fixed_index,
                       const lsm2d_cloudset* moving, const int32_t* moving_index,
                       int32_t n_items, const float* poses /* [n_items][3] */,
                       const lsm2d_select_params* select, int32_t k,
                       int32_t* out_index /* [k] */,
                       float* out_H /* [k][9] or NULL */, float* out_b /* [k][3] or NULL */,
                       lsm2d_iteration_stats* out_stats /* [k] or NULL */,
                       int32_t* out_n_selected, int32_t* out_n_accepted);

/* ---- plugin interface #2: MultiAligner2D::compute, batched --------------------------------------
 * Replaces aligner->setFixed / setMoving / setMovingInFixed / compute / movingInFixed /
 * iterationStats (apps/visual_test_aligner_2d.cpp:123-156) for n_alignments independent alignments
 * (the tracker uses 1; MultiLoopDetectorBruteForce2D's candidate loop, MULTI.json:964-986, uses many).
 * Each alignment runs max_iterations x { every slice: finder + factor ; one 3x3 solve ; right update }
 * entirely on the device.  Cloud selection for alignment i, slice s: fixed[s] cloud
 * fixed_index[s*n+i] (or i when fixed_index == NULL, or 0 when the set holds one cloud); same for moving. */
typedef struct {
  int32_t                       n_alignments;
  int32_t                       n_slices;
  const lsm2d_slice_params*     slices;        /* [n_slices] */
  const lsm2d_cloudset* const*  fixed;         /* [n_slices] */
  const lsm2d_cloudset* const*  moving;        /* [n_slices] */
  const int32_t*                fixed_index;   /* [n_slices][n_alignments] or NULL */
  const int32_t*                moving_index;  /* [n_slices][n_alignments] or NULL */
  const float*                  init_pose;     /* [n_alignments][3]  setMovingInFixed */
  const lsm2d_prior*            prior;         /* [n_alignments] or NULL */
} lsm2d_batch;

int lsm2d_align_batch(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch,
                      float* out_pose,                  /* [n][3]  movingInFixed() */
                      float* out_H,                     /* [n][9]  information matrix = H of the last iteration; may be NULL */
                      int32_t* out_status,              /* [n]     lsm2d_status >= 0 */
                      int32_t* out_iterations,          /* [n]     iterations started; may be NULL */
                      lsm2d_iteration_stats* out_stats  /* [n][lsm2d_stats_capacity(aligner)]; may be NULL */);

/* lsm2d_align_batch's alignment, then the verdict of the candidate loops (MultiLoopDetectorBruteForce2D, MultiRelocalizer2D: MULTI.json:964-986, :749-769)
 * made on the device: which candidates' aligner succeeded AND whose last iteration passes the thresholds, and which k of those are best.  What a caller
 * otherwise gets by asking lsm2d_align_batch for every iteration's statistics (lsm2d_stats_capacity x 28 bytes per candidate: 55 MB for 65 536 candidates
 * of a 30-iteration aligner) and scanning them on the host.
 * Alignment: candidate i is aligned exactly as lsm2d_align_batch(..., out_stats != NULL) aligns it -- the same path rule, kernels and launch forms, the
 * same bits in both values of "sum_order" and every value of "fast_forward" -- with ONE exception: the results stay in device memory, so the zero-copy
 * form (results written to pinned host memory) is not taken, whatever "zero_copy_max" says.
 * Acceptance (PARITY.md section 3, items 18 and 18c): candidate i is accepted when status[i] == LSM2D_SUCCESS, iterations[i] >= 1 and lsm2d_score_select's
 * fp32 test passes on row iterations[i] - 1 of its statistics -- the last iteration it started.  A candidate that started no iteration is rejected.
 * Ranking: lsm2d_score_select's total order on that last row -- n_inliers descending, chi_inliers ascending on its bit pattern, candidate index ascending.
 * Outputs: *out_n_accepted the accepted candidates among all n_alignments; *out_n_selected = min(k, n_accepted); *out_n_success (may be NULL) the candidates
 * with status LSM2D_SUCCESS; out_index[0 .. n_selected) the selected candidates, best first; rows j < n_selected of out_pose / out_H / out_iterations
 * (the last two may be NULL) the bits lsm2d_align_batch returns for candidate out_index[j], out_last_stats[j] (may be NULL) its statistics row
 * iterations - 1.  Positions >= n_selected are not written.
 * Refused before anything is launched or written: a NULL the call needs (ctx, aligner, batch, select, out_index, out_pose, the two count pointers) or k
 * outside [1, LSM2D_SELECT_MAX_K] (LSM2D_BAD_ARGUMENT), and whatever lsm2d_align_batch refuses: a bad descriptor, cloud indices out of range, canvases
 * that do not fit LDS, two batches in flight.  n_alignments == 0 succeeds with all counts 0.
 * Up: what lsm2d_align_batch sends up.  Down: ONE copy of [n_accepted, n_selected, n_success, never-reported | k indices | k rows of 96 bytes].  ONE wait.
 * The check that every alignment's workgroup reported is made on the device (the fourth header word): non-zero is LSM2D_DEVICE_ERROR, as for
 * lsm2d_align_batch.  The call is synchronous (there is no begin / wait form); with one batch in flight it works on the free lane like every other call.
 * "kernel_timing" / lsm2d_last_kernel_ms cover the aligner's launch PLUS the packing and the selection behind it.  The read-only options
 * "last_cand_builds" / "last_cand_iterations" / "last_cand_overflows" / "last_cand_fallbacks" are derived from arrays that stay on the device here: after this call they keep
 * the previous call's values. */
int lsm2d_align_select(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch,
                       const lsm2d_select_params* select, int32_t k,
                       int32_t* out_index /* [k] */, float* out_pose /* [k][3] */, float* out_H /* [k][9] or NULL */,
                       int32_t* out_iterations /* [k] or NULL */, lsm2d_iteration_stats* out_last_stats /* [k] or NULL */,
                       int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success /* or NULL */);

/* ---- pose hypotheses scored against an ALIGNER (the two-laser robot's relocaliser, MULTI.json:700-732 with the slices at :715-721 and the odometry
 * prior of :402-422; its relocaliser's own aligner is unset, :749-769, so it falls back on this one): lsm2d_score_batch / lsm2d_score_select for a
 * lsm2d_batch -- up to 4 slices, WithSensor offsets, min_num_correspondences, an optional prior per hypothesis -- in ONE call with ONE wait.
 * batch: n_alignments = the hypotheses, init_pose = their poses X, prior = [n] or NULL; cloud selection is lsm2d_batch's rule per slice (fixed_index /
 * moving_index are [n_slices][n] or NULL; indices may repeat; a set without index holds 1 or n clouds).
 * A scored item is what the first iteration of MultiAligner2D::compute holds just before its solve.  For slices s = 0 .. n_slices - 1, in order:
 *   1. effective pose: Xe = X bit for bit when sensor_in_robot[s] compares equal to (0, 0, 0) (so (-0, 0, 0) too), else Xe = S^-1 X, in the aligner's
 *      own fp32 operations;
 *   2. pairs: the slice's finder at Xe -- lsm2d_find_correspondences_batch's pairs;
 *   3. the pairs enter n_correspondences and the pair digest WHETHER OR NOT the slice is skipped, and the digest uses lsm2d_pair_hash(s, ...): the
 *      slice index, as the aligner's digest does (lsm2d_score_batch hashes with slice 0);
 *   4. a slice with n_pairs <= min_num_correspondences contributes nothing else;
 *   5. otherwise its H, b, n_inliers, n_outliers and chi^2 sums are the bits lsm2d_score_batch gives for that slice at Xe, in both values of "sum_order";
 *   6. the slices' values are added in fp32, in slice order, starting from +0 (a -0 therefore becomes +0);
 *   7. the prior, when one is given AND at least one slice contributed, is added last (the aligner's own device function: omega is taken as given,
 *      symmetric or not, and all nine entries of H are kept as summed);
 *   8. out_active[i] is the number of slices that contributed.  0: H and b are zeros, no prior is added, n_correspondences and the digest are still
 *      reported -- the hypothesis an aligner would end with LSM2D_NOT_ENOUGH_CORRESPONDENCES.
 * Consequences.  With "sum_order" 1 an item equals the sequential oracle's align(max_iterations = 1) bit for bit -- its H, its first statistics row, its
 * NOT_ENOUGH_CORRESPONDENCES status -- and the oracle's solve_update(H, b, X, damping) on the item's H and b gives that alignment's pose bit for bit.
 * In the default order a slice's tree is lsm2d_linearize's (256-thread workgroups), NOT k_align's 512-thread tree: lsm2d_align_batch's first iteration is
 * not the yardstick there; the combination above over lsm2d_linearize per slice is.
 * Refused before anything is launched or written: n_slices outside [1, 4] or a NULL the call needs (LSM2D_BAD_ARGUMENT); a cloud index out of range
 * (LSM2D_BAD_ARGUMENT; lsm2d_last_error names item and slice); canvases that do not fit LDS (LSM2D_CAPACITY_EXCEEDED); two batches in flight (as
 * lsm2d_score_batch); for the select form k outside [1, LSM2D_SELECT_MAX_K].  n_alignments == 0 succeeds (the select form sets both counts to 0).
 * Up: poses, priors and index tables, once; the slices' item tables are made on the device.  Down: ONE copy -- n combined rows (80 bytes each), or for the
 * select form 16 bytes + k indices and rows.  ONE wait, however many slices and launch groups there are; a launch group is sized by the largest slot
 * among the slices.  "kernel_timing" / lsm2d_last_kernel_ms cover the last launch group of the last slice, the combination and the selection.
 * lsm2d_score_aligner_select ranks as lsm2d_score_select does (same test, same total order) on the combined statistics; an item with active == 0 is
 * rejected whatever the thresholds are: it has no aligner status to pass.  Rows j < n_selected of out_H / out_b / out_stats / out_active (each may be
 * NULL) are lsm2d_score_aligner_batch's for item out_index[j]. */
int lsm2d_score_aligner_batch(lsm2d_context* ctx, const lsm2d_batch* batch,
                              float* out_H /* [n][9] */, float* out_b /* [n][3] */,
                              lsm2d_iteration_stats* out_stats /* [n] or NULL */, int32_t* out_active /* [n] or NULL */);
int lsm2d_score_aligner_select(lsm2d_context* ctx, const lsm2d_batch* batch, const lsm2d_select_params* select, int32_t k,
                               int32_t* out_index /* [k] */, float* out_H /* [k][9] or NULL */, float* out_b /* [k][3] or NULL */,
                               lsm2d_iteration_stats* out_stats /* [k] or NULL */, int32_t* out_active /* [k] or NULL */,
                               int32_t* out_n_selected, int32_t* out_n_accepted);

/* ---- the three select calls PER GROUP of the batch (0.7.8): a fleet server's N robots each have their own loop-closure candidates or relocalisation
 * hypotheses, laid one robot behind the other in ONE batch, and each robot wants ITS best k -- not the best k of the pool, which a robot with many good
 * candidates would fill.  Each call is its ungrouped sibling plus groups: the same arguments, scoring / alignment, thresholds and k (shared by all groups).
 * Groups: group_offsets is a host array of n_groups + 1 int32 values, non-decreasing, group_offsets[0] == 0, group_offsets[n_groups] == n_items
 * (n_alignments for the batch forms); group g is items [group_offsets[g], group_offsets[g + 1]).  Empty groups are legal: 0 accepted, 0 selected.
 * Outputs: every per-row output has n_groups x k rows; group g's j-th best lands in slot g * k + j, j < out_n_selected[g]; other slots are not written.
 * out_index holds BATCH item indices, not positions within the group.  out_n_selected, out_n_accepted (and lsm2d_align_select_grouped's out_n_success, which
 * may be NULL) are [n_groups].
 * Meaning: group g's block is bit for bit what the ungrouped call returns for the sub-batch of g's items, with the indices shifted by group_offsets[g]: the
 * same fp32 acceptance test, the same total order (n_inliers descending, chi_inliers ascending on its bits, index ascending; PARITY.md section 3, 18d).  The
 * result is unique and does not depend on the order in which workgroups run.
 * Refused before anything is launched or written: everything the ungrouped sibling refuses; a NULL group_offsets, n_groups < 1, offsets that decrease, do
 * not start at 0 or do not end at the batch's size; n_groups x k above LSM2D_SELECT_MAX_GROUP_ROWS (all LSM2D_BAD_ARGUMENT).
 * LSM2D_SELECT_MAX_GROUP_ROWS = 2^18 rows: what comes down is n_groups x (16 + 4 k + 4 k row_words) bytes -- row_words 17 (score), 20 (score_aligner), 24
 * (align) -- so the cap bounds the one copy, and the pinned staging behind it, at about 25 MB of 96-byte aligned-candidate rows.
 * Cost: ONE upload of the sibling's arguments with the group table behind them in the same copy, ONE copy down, ONE wait, whatever n_groups and the groups'
 * sizes are.  While every group holds at most 2048 items the selection is ONE launch of a workgroup per group; a larger group takes segmented passes (a keys
 * launch, a tile pass per halving, a gather), small groups of the same call riding along.  "kernel_timing" / lsm2d_last_kernel_ms cover what they cover for
 * the sibling.  The never-reported check of lsm2d_align_select stays one global count and one LSM2D_DEVICE_ERROR.  The calls are synchronous. */
#define LSM2D_SELECT_MAX_GROUP_ROWS (1 << 18)
int lsm2d_score_select_grouped(lsm2d_context* ctx, const lsm2d_slice_params* slice,
                               const lsm2d_cloudset* fixed, const int32_t* fixed_index /* [n_items] or NULL */,
                               const lsm2d_cloudset* moving, const int32_t* moving_index /* [n_items] or NULL */,
                               int32_t n_items, const float* poses /* [n_items][3] */,
                               const lsm2d_select_params* select, int32_t k,
                               int32_t n_groups, const int32_t* group_offsets /* [n_groups + 1] */,
                               int32_t* out_index /* [n_groups * k] */, float* out_H /* [n_groups * k][9] or NULL */, float* out_b /* [n_groups * k][3] or NULL */,
                               lsm2d_iteration_stats* out_stats /* [n_groups * k] or NULL */,
                               int32_t* out_n_selected /* [n_groups] */, int32_t* out_n_accepted /* [n_groups] */);
int lsm2d_score_aligner_select_grouped(lsm2d_context* ctx, const lsm2d_batch* batch, const lsm2d_select_params* select, int32_t k,
                                       int32_t n_groups, const int32_t* group_offsets /* [n_groups + 1] */,
                                       int32_t* out_index /* [n_groups * k] */, float* out_H /* [n_groups * k][9] or NULL */, float* out_b /* [n_groups * k][3] or NULL */,
                                       lsm2d_iteration_stats* out_stats /* [n_groups * k] or NULL */, int32_t* out_active /* [n_groups * k] or NULL */,
                                       int32_t* out_n_selected /* [n_groups] */, int32_t* out_n_accepted /* [n_groups] */);
int lsm2d_align_select_grouped(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch,
                               const lsm2d_select_params* select, int32_t k,
                               int32_t n_groups, const int32_t* group_offsets /* [n_groups + 1] */,
                               int32_t* out_index /* [n_groups * k] */, float* out_pose /* [n_groups * k][3] */, float* out_H /* [n_groups * k][9] or NULL */,
                               int32_t* out_iterations /* [n_groups * k] or NULL */, lsm2d_iteration_stats* out_last_stats /* [n_groups * k] or NULL */,
                               int32_t* out_n_selected /* [n_groups] */, int32_t* out_n_accepted /* [n_groups] */, int32_t* out_n_success /* [n_groups] or NULL */);

/* ---- relocalise in ONE call (0.7.9): the candidate loop of the relocaliser / loop detector (MultiRelocalizer2D, MultiLoopDetectorBruteForce2D:
 * MULTI.json:749-769, :964-986) scores its hypotheses, keeps the best that pass the acceptance test, aligns those and judges the aligned ones.  That is
 * lsm2d_score_aligner_select followed by lsm2d_align_select, with the host in the middle only to gather the selected hypotheses' poses, priors and cloud
 * indices and send them up again.  Here the selection's answer stays on the device, a kernel writes the aligner's input block from it, and both answers come
 * down together.
 * batch: the descriptor lsm2d_score_aligner_select takes -- 1 .. 4 slices, optional per-hypothesis priors, optional [n_slices][n] index arrays, init_pose
 * holding the hypotheses.
 * Meaning (PARITY.md section 3, item 18e).  Every output is bit for bit what the two existing calls give, made in this order:
 *   1. lsm2d_score_aligner_select(batch, score_select, k_score) returns m = n_scored_selected indices idx[0 .. m), best first;
 *   2. lsm2d_align_select(aligner, batch', align_select, k), where batch' has m candidates and candidate j is hypothesis idx[j]: its pose, its prior, its
 *      cloud in every slice (where batch has no index array, lsm2d_batch's rule spelled out: cloud idx[j], or cloud 0 of a one-cloud set);
 *   3. out_index[r] = idx[the second call's index]: out_index holds BATCH indices;
 *   4. the counts are the second call's; n_success counts the m real candidates only;
 *   5. ties in the second ranking break by slot j, i.e. by stage-1 rank;
 *   6. m == 0: the second stage's counts are zeros and the call succeeds.
 * in both values of "sum_order", every "fast_forward" and every "align_path".  align_select == NULL: score_select's thresholds judge the aligned candidates too.
 * Outputs: out_scored_index / out_scored_stats (may be NULL) / the two scored counts as lsm2d_score_aligner_select gives index, statistics and counts;
 * out_index .. out_n_success as lsm2d_align_select gives them.  Positions beyond the counts are not written.
 * Refused before anything is launched or written: everything either sibling refuses; k_score or k outside [1, LSM2D_SELECT_MAX_K]; a batch in flight on
 * the context (the call uses both lanes).  n_alignments == 0 succeeds with all counts 0.
 * Cost: ONE upload (stage 1's), ONE copy down -- [16 bytes | k_score indices | k_score rows of 80 bytes] and [16 bytes | k indices | k rows of 96 bytes],
 * adjacent -- and ONE wait.  The aligner always runs k_score alignments: slots beyond m are PADS that repeat idx[0] (hypothesis 0 when m == 0); their rows
 * are never ranked, counted or returned.  So a call in which nothing passes stage 1 still pays k_score alignments: a caller who expects mostly empty
 * selections is better served by the two calls.  The path rule ("align_path" 0) decides for k_score candidates, not for m: the launch form may differ from
 * the two-call route's, the bits do not.  "kernel_timing" / lsm2d_last_kernel_ms cover the whole chain, from in front of stage 1's first launch (its upload
 * included -- more than lsm2d_score_aligner_select's own bracket, which begins at the last launch group) to the final selection.  The call is synchronous. */
int lsm2d_relocalize_select(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch,
                            const lsm2d_select_params* score_select, int32_t k_score,     /* stage 1: lsm2d_score_aligner_select's test and k */
                            const lsm2d_select_params* align_select, int32_t k,           /* stage 2: lsm2d_align_select's; NULL = score_select */
                            int32_t* out_scored_index /* [k_score] */, lsm2d_iteration_stats* out_scored_stats /* [k_score] or NULL */,
                            int32_t* out_n_scored_selected, int32_t* out_n_scored_accepted,
                            int32_t* out_index /* [k] */, float* out_pose /* [k][3] */, float* out_H /* [k][9] or NULL */,
                            int32_t* out_iterations /* [k] or NULL */, lsm2d_iteration_stats* out_last_stats /* [k] or NULL */,
                            int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success /* or NULL */);

/* ---- a pose grid scored coarse to fine in ONE call (0.7.10).  The hypotheses of ONE scan against one map are not sent up: they are made on the device
 * from a grid descriptor -- six floats and a few integers in the kernel arguments -- scored and ranked as lsm2d_score_aligner_select scores and ranks; the
 * k_parents best cells of a level are refined into refine[0] x refine[1] x refine[2] children each, which are the next level's hypotheses, without leaving
 * the device; the best k of the LAST level come down.  16 x 16 x 16 cells, 64 parents and 4 x 4 x 1 children reach the resolution of a 64 x 64 x 16 grid
 * with 5 120 scored hypotheses instead of 65 536.
 * NOT upstream: nothing in the reference says how its relocaliser chooses hypotheses (MultiRelocalizer2D, MULTI.json:749-769).  A coarse-to-fine search is
 * NOT the exhaustive grid: it finds the fine grid's winner only if that winner's coarse cell is among the parents kept, and can miss it.
 * Meaning (PARITY.md section 3, item 18f), fixed by the existing calls:
 *   spacings   s_0 = step; s_l[a] = s_(l-1)[a] / (float) refine[a]: fp32 IEEE division, made on the host once per level.
 *   offsets    o(i, n) = (float) i - 0.5f * (float) (n - 1), exact in fp32.
 *   coordinate base[a] + (o * s_l[a]): the product rounded to fp32, then the sum rounded to fp32 -- never fused into an fma.  theta is not wrapped.
 *   level 0    item i = (it * ny + iy) * nx + ix, base = center, n = count; its origin is i.
 *   level l>0  with R = rx * ry * rt, item j * R + c is child c = (ct * ry + cy) * rx + cx of parent j; parents are the previous level's selection, best
 *              first; base = the parent's pose bit for bit as it was scored, n = refine; its origin is the parent's (the level-0 cell it descends from).
 *   scoring    level l is, bit for bit, lsm2d_score_aligner_select over a batch of the level's REAL items (n0 at level 0, m_(l-1) * R below it), with the
 *              generated poses as init_pose, no prior and the same cloud in every slice for every item; coarse_select and k_parents below the last level,
 *              select and k at the last; m_l is that call's n_selected and out_level_counts[l] its {n_accepted, n_selected} -- in both values of
 *              "sum_order", for every finder kind, for 1 .. 4 slices with sensor offsets.  n_levels == 1 is lsm2d_score_aligner_select on the level-0 grid.
 *   pads       the device runs k_parents * R slots at every level l >= 1; the slots of parents j >= m_(l-1) are PADS that repeat parent 0's children (the
 *              grid's centre when nothing was selected).  They are scored and paid for, as lsm2d_relocalize_select pays for its pads, and are never
 *              accepted, counted, ranked or returned.  When m_l == 0 every deeper level still runs its slots, reports {0, 0}, the final counts are 0 and
 *              the call succeeds: a caller who expects mostly empty selections is better served by a loop over lsm2d_score_aligner_select.
 * fixed_cloud / moving_cloud: the ONE cloud of every slice's set that all hypotheses use (the sets may hold more: a fleet's scans and the index of the
 * robot being relocalised); NULL: cloud 0.
 * Outputs: row j < *out_n_selected is the j-th best hypothesis of the last level: out_pose the pose it was scored at, out_origin its level-0 cell, out_H /
 * out_b / out_stats / out_active what lsm2d_score_aligner_select returns for it.  Positions beyond the count are not written.
 * Refused with LSM2D_BAD_ARGUMENT before anything is launched or written: a NULL the call needs; n_slices outside [1, 4]; a cloud index out of range (the
 * message names the slice); a count or refine below 1; k_parents outside [1, LSM2D_SELECT_MAX_K] or coarse_select NULL when n_levels > 1; n_levels outside
 * [1, LSM2D_GRID_MAX_LEVELS]; k outside [1, LSM2D_SELECT_MAX_K]; a step that is negative, NaN or Inf; a centre that is not finite; nx * ny * nt or
 * k_parents * R above LSM2D_GRID_MAX_ITEMS; whatever lsm2d_score_aligner_select refuses for the slices (canvases that do not fit LDS:
 * LSM2D_CAPACITY_EXCEEDED); a batch in flight on both lanes.
 * Cost: NO upload of items; ONE copy down -- the per-level headers, then the last level's header, k indices, k rows of 80 bytes, k poses and k origins --
 * and ONE wait, however many levels and launch groups there are.  "kernel_timing" / lsm2d_last_kernel_ms cover everything from the first launch to the
 * last selection.  The call is synchronous and runs on the context's stream in order. */
#define LSM2D_GRID_MAX_LEVELS 4
#define LSM2D_GRID_MAX_ITEMS  (1 << 18)      /* hypotheses of one level, pads included */
typedef struct {
  float   center[3];    /* x, y, theta of the grid's centre */
  float   step[3];      /* level 0's spacing per axis; finite, >= 0 (0 with count > 1 is legal: duplicates) */
  int32_t count[3];     /* level 0: nx, ny, nt, each >= 1 */
  int32_t n_levels;     /* 1 .. LSM2D_GRID_MAX_LEVELS; level 0 is the grid, each further level refines the parents kept */
  int32_t refine[3];    /* children per parent and axis at every further level, each >= 1; child spacing = parent spacing / refine */
  int32_t k_parents;    /* parents kept per level below the last, 1 .. LSM2D_SELECT_MAX_K (ignored when n_levels == 1) */
} lsm2d_pose_grid;

int lsm2d_score_grid_select(lsm2d_context* ctx, int32_t n_slices, const lsm2d_slice_params* slices,
                            const lsm2d_cloudset* const* fixed,  const int32_t* fixed_cloud  /* [n_slices] or NULL: cloud 0 */,
                            const lsm2d_cloudset* const* moving, const int32_t* moving_cloud /* [n_slices] or NULL: cloud 0 */,
                            const lsm2d_pose_grid* grid,
                            const lsm2d_select_params* coarse_select /* levels below the last; may be NULL when n_levels == 1 */,
                            const lsm2d_select_params* select, int32_t k /* the last level's test and k */,
                            float* out_pose /* [k][3] */, int32_t* out_origin /* [k] or NULL */,
                            float* out_H /* [k][9] or NULL */, float* out_b /* [k][3] or NULL */,
                            lsm2d_iteration_stats* out_stats /* [k] or NULL */, int32_t* out_active /* [k] or NULL */,
                            int32_t* out_n_selected, int32_t* out_n_accepted,
                            int32_t* out_level_counts /* [n_levels][2] = {accepted, selected} per level, or NULL */);

/* ---- voxelise and assemble device-resident clouds of any size in ONE call (0.7.11).  PointCloud::voxelize as the reference uses it --
 * sensor_processing/raw_data_preprocessor_projective_2d.cpp:38-41 with coefficients (res, res, 1, 1), mapping/scene_clipper_projective_2d.cpp:44-48 with
 * (res, res, 0.1, 0.1) -- which the older entry points reach only for the at most 2048 points of one scan or one clipped canvas.  Here the inputs are any
 * clouds of a set, as large as they are: output cloud g of `dst` becomes the voxelisation of the CONCATENATION of every input k with group[k] == g, taken
 * in the order of the call's list, each first moved by its pose.  Three uses:
 *   a map assembled       every input in group 0, poses = the local maps' optimised poses: K local maps as one decimated cloud, no download
 *   a fleet's maps bounded group[k] = k, dst == src, no poses: every cloud of a reserved-many set decimated in place (what keeps lsm2d_merge_scene* away
 *                         from LSM2D_CAPACITY_EXCEEDED without a round trip through the host)
 *   a smaller map         one input, one group: a 1M-point map made a 100k-point map -- every aligner and scoring call is linear in the map's points
 * Meaning (PARITY.md section 3, item 17b; nothing here is new arithmetic):
 *   transform  input k's point i becomes what lsm2d_merge_scene appends for it at measurement_in_scene = pose[k]: the point and the normal under the
 *              isometry made from the pose, cosine and sine the deterministic ones of item 11b, no renormalisation.  pose == NULL copies the bits.
 *   key        the four floors of x * inv_res, y * inv_res, nx * inv_rn, ny * inv_rn on the transformed values, inv = 1.0f / coefficient divided once on
 *              the host.  The x and y floors must lie in [-32768, 32768) and the normal floors in [-16, 15]; a point that fails (NaN and Inf fail) has no
 *              key, is dropped and is counted in out_dropped per group.
 *   order      ascending key, then ascending concatenation index (list position, then point index).
 *   voxel      four fp32 sums from +0 in that order, times 1.0f / (float) count; nn = sqrtf(fmaf(anx, anx, any * any)), both normal components divided
 *              by nn when nn > 0.  Voxels come out in ascending key order.
 *   groups     equal keys in different groups are never merged; an empty group, or one whose points were all dropped, writes a count of 0.
 * All or nothing: if any group's voxel count exceeds its destination cloud's capacity NO destination cloud is changed, the call returns
 * LSM2D_CAPACITY_EXCEEDED and out_counts holds the counts that would have been needed (the device decides ahead of its first write to dst).
 * Aliasing: dst may be src and a destination cloud may be one of the inputs; the result is as if every input were read before anything is written.
 * Refused with LSM2D_BAD_ARGUMENT before anything is launched or written: a NULL the call needs (ctx, params, src, dst, out_counts); a resolution that is
 * not > 0 or not finite; n_inputs < 1; n_groups < 1 or above LSM2D_VOXELIZE_MAX_GROUPS; an index outside its set (with dst_index == NULL: n_groups above
 * dst's clouds); a group value outside [0, n_groups); a destination index given twice; dst not a reserved set; more input points in all than
 * LSM2D_VOXELIZE_MAX_POINTS; a batch in flight on the lane.
 * Cost: the call is synchronous; the call's small tables go up, ONE copy comes down (the counts) and there is ONE wait -- plus the one fetch of sizes
 * when a set's sizes are known to the device only (after an asynchronous clip / merge).  "kernel_timing" / lsm2d_last_kernel_ms cover the whole chain.  A
 * voxel's sum is one thread's walk: a million points in ONE voxel is legal and slow.  Whatever dst carries derived from its points (row copies, search
 * grids, KD-trees, distance maps, tile bounds) is invalidated as lsm2d_merge_scene invalidates it.  Read-only options "voxelize_tile" (keys per sort
 * tile, 1024) and "voxelize_scan_tiles" (16: the tiles whose digit counters one pass of the scan's single workgroup takes; beyond 16 tiles -- 16 384 points -- the
 * scan carries its running sum from pass to pass) describe the device side's tiling. */
#define LSM2D_VOXELIZE_MAX_POINTS (1 << 24)      /* input points of one call, all inputs together */
#define LSM2D_VOXELIZE_MAX_GROUPS (1 << 16)
typedef struct lsm2d_voxelize_params {
  float resolution;          /* x and y coefficient, > 0 (the preprocessor's / clipper's `res`) */
  float normal_resolution;   /* nx and ny coefficient, > 0: 1 = the preprocessor's (res,res,1,1), 0.1 = the clipper's (res,res,0.1,0.1) */
} lsm2d_voxelize_params;

int lsm2d_voxelize(lsm2d_context* ctx, const lsm2d_voxelize_params* params,
                   const lsm2d_cloudset* src, int32_t n_inputs,
                   const int32_t* src_index,   /* [n_inputs] or NULL: cloud k */
                   const float* pose,          /* [n_inputs][3] (x, y, theta) or NULL: no transform at all */
                   const int32_t* group,       /* [n_inputs], values in [0, n_groups), or NULL: all 0 */
                   int32_t n_groups,
                   lsm2d_cloudset* dst,
                   const int32_t* dst_index,   /* [n_groups] or NULL: cloud g; no index twice */
                   int32_t* out_counts,        /* [n_groups] voxels written */
                   int32_t* out_dropped);      /* [n_groups] points that had no key, or NULL */

/* ---- occupancy grids on the device (0.7.12): scans ray-traced into hit / miss counts, and the counts rendered.  A capability of THIS build: the reference
 * tree has no grid mapper (like the ranking order of PARITY.md section 3, item 18a and the pose pyramid of item 18f); what a planner, a fleet UI or a map
 * server reads of a 2D laser SLAM is which cells the beams passed through and which they ended in, and the clouds and the poses are already on the device.
 * A grid set is n_grids grids of ONE geometry; cell (cx, cy) covers [origin + c * resolution, origin + (c + 1) * resolution) on each axis and carries two
 * uint32 counters, hits and misses, stored side by side (a cell is one 8-byte access).  Host arrays are row-major: row = cy, column = cx.
 * lsm2d_occupancy_update mirrors lsm2d_voxelize's argument list.  Meaning (PARITY.md section 3, item 17c); everything after the transform is integers:
 *   transform  input k's point i becomes what lsm2d_merge_scene appends for it at measurement_in_scene = pose[k]: xf_point (csrc/lsm2d_device.h) under the
 *              isometry the host makes from the pose, cosine and sine the deterministic ones of item 11b.  pose == NULL copies the bits.  The ray starts
 *              at the pose's translation (pose[k][0], pose[k][1]) -- (0, 0) when pose == NULL.  Normals are not read.              [item 17c.1; 17b.1; 11b]
 *   cells      inv = 1.0f / resolution, divided once on the host; a coordinate v on an axis with origin o has the cell floorf((v - o) * inv), the
 *              difference and the product rounded separately (never an fma).  All four cell coordinates of a ray must lie in [-2^20, 2^20) (NaN and Inf
 *              fail) and L = max(|x1 - x0|, |y1 - y0|) must be <= LSM2D_OCCUPANCY_MAX_RAY_CELLS; a point that fails either test gives no ray and is counted
 *              in out_dropped of its grid.                                                                                        [item 17c.2]
 *   walk       with ax = |x1 - x0|, ay = |y1 - y0| and the signs s, s': x-major iff ax >= ay (a tie is x-major); step i = 0 .. L is the cell with the major
 *              coordinate m0 + s i and the minor coordinate n0 + s' ((2 i a + L) / (2 L)), a the minor extent, the division integer and non-negative
 *              (2 * 32767^2 + 32767 < 2^31); L = 0 is the single cell (x0, y0).  Steps 0 .. L - 1 add 1 to `misses` of their cell, step L adds 1 to
 *              `hits`.  A step whose cell lies outside the grid adds nothing and the ray goes on: there is no clipping rule.  This is the incremental
 *              error-term (Bresenham) walk: L + 1 cells, 8-connected, never more than half a cell from the ideal line on the minor axis
 *              (tests/test_occupancy_abi.py checks all three in exact rationals).                                                [item 17c.3]
 *   sums       counters accumulate over calls, and within a call over every input sent to the grid; they saturate at 2^32 - 1.  Integer sums have no
 *              order: the result is unique.                                                                                       [item 17c.4]
 * Refused with LSM2D_BAD_ARGUMENT before anything is launched or written: a NULL the call needs; a resolution that is not > 0 or not finite; a non-finite
 * origin; a side < 1 or above LSM2D_OCCUPANCY_MAX_SIDE; n_grids < 1, or the cells of the set above LSM2D_OCCUPANCY_MAX_CELLS; n_inputs < 1; an index
 * outside its set; a grid value outside [0, n_grids); more input points than LSM2D_OCCUPANCY_MAX_RAYS; a set of another context; a batch in flight on
 * the lane.
 * Cost: the call is synchronous; the small tables go up, ONE copy comes down (rays, dropped, fault word) and there is ONE wait -- plus the one fetch of
 * sizes when the source set's sizes are known to the device only (as in lsm2d_voxelize).  "kernel_timing" / lsm2d_last_kernel_ms cover the chain; with it
 * on, the tile workgroups' clock stamps come down in a second copy and "last_occupancy_wg_median_ns" / "last_occupancy_wg_max_ns" read them
 * (diagnostics).  Two launches: k_occ_rays (a thread per point) and k_occ_tiles (a workgroup per grid and tile of "occupancy_tile" = 64 x 64 cells,
 * read-only, summing in LDS; no global atomics on the grid).  Tiles overlapped by many scans work longest (measured: DESIGN.md section 8).
 * lsm2d_occupancy_render: v = hits + misses in 64 bits; v < max(min_visits, 1) gives -1 (unknown); else p = (float) hits / (float) v (IEEE division, both
 * conversions round to nearest) and the value is (int8) rintf(100.0f * p), the product rounded once, ties to even: 0 .. 100.  One byte per cell comes down
 * instead of eight.                                                                                                               [item 17c.6]
 * NOT BUILT (item 17c.5): an asynchronous form; per-grid geometry; maximum-range truncation and clearing along beams without a return
 * (a cloud holds returns only: a beam without a return clears nothing); a once-per-scan rule for counts sets (every ray counts); splitting a tile's work
 * over several workgroups.  (0.7.13 builds the truncation and the clearing from raw ranges: lsm2d_occupancy_update_scans, below.  0.7.14 builds the
 * once-per-scan rule and log-odds with decay as a second kind of set, which this call accepts as it accepts a counts set: log-odds grid sets, below.) */
#define LSM2D_OCCUPANCY_MAX_SIDE      16384
#define LSM2D_OCCUPANCY_MAX_CELLS     (1 << 28)   /* all grids of a set together: 2 GB of counters */
#define LSM2D_OCCUPANCY_MAX_RAYS      (1 << 24)   /* input points of one update, all inputs together */
#define LSM2D_OCCUPANCY_MAX_RAY_CELLS 32767       /* longest ray, in cells along its major axis */
typedef struct lsm2d_grid_geometry { float origin_x, origin_y, resolution; int32_t width, height; } lsm2d_grid_geometry;
typedef struct lsm2d_gridset lsm2d_gridset;

int  lsm2d_gridset_create(lsm2d_context* ctx, const lsm2d_grid_geometry* geometry, int32_t n_grids, lsm2d_gridset** out);   /* counters zero */
int  lsm2d_gridset_clear(lsm2d_gridset* grids, int32_t n, const int32_t* grid_index /* [n] or NULL: every grid */);           /* queued, no wait */
int  lsm2d_gridset_upload(lsm2d_gridset* grids, int32_t grid_index, const uint32_t* hits, const uint32_t* misses);   /* host [height][width]; a NULL array leaves that counter */
int  lsm2d_gridset_download(const lsm2d_gridset* grids, int32_t grid_index, uint32_t* out_hits, uint32_t* out_misses); /* either may be NULL */
void lsm2d_gridset_destroy(lsm2d_gridset* grids);

int lsm2d_occupancy_update(lsm2d_context* ctx, lsm2d_gridset* grids,
                           const lsm2d_cloudset* src, int32_t n_inputs,
                           const int32_t* src_index,  /* [n_inputs] or NULL: cloud k */
                           const float* pose,         /* [n_inputs][3] sensor in the grid's frame, or NULL: no transform, origin (0, 0) */
                           const int32_t* grid,       /* [n_inputs] in [0, n_grids), or NULL: all 0 */
                           int32_t* out_rays,         /* [n_grids] rays walked, or NULL */
                           int32_t* out_dropped);     /* [n_grids] points that gave no ray, or NULL */

typedef struct lsm2d_occupancy_render_params { int32_t min_visits; } lsm2d_occupancy_render_params;
int lsm2d_occupancy_render(lsm2d_context* ctx, const lsm2d_gridset* grids, int32_t grid_index,
                           const lsm2d_occupancy_render_params* params, int8_t* out /* host [height][width] */);

/* ---- occupancy grids from raw scans (0.7.13): the beams of range scans ray-traced into the counters of a grid set -- the returns as lsm2d_occupancy_update
 * traces a cloud's points, and the beams WITHOUT a return, which no cloud holds, cleared out to a cut.  A door that opens onto a corridor, a person who
 * walked away: the beams that now pass through return nothing, and only the scan knows of them.  Like 0.7.12 a capability of this build (the reference tree
 * has no grid mapper); the definition is the contract (PARITY.md section 3, item 17d), everything behind the transform is integer arithmetic.
 *   classes    beam c of scan k, r = ranges[k][c], by these tests in this order:
 *                1. !(r >= range_min)   NaN, -Inf, too close: no ray, counted in out_dropped;
 *                2. r <= trace_range    a HIT ray of length l = r;
 *                3. r <= range_max      a return beyond the cut: a CLEAR ray of length l = trace_range;
 *                4. otherwise           no return (+Inf included): a CLEAR ray of length trace_range when clear_no_return, else dropped.        [item 17d.1]
 *   end point  in the sensor frame (l * dir[c].x, l * dir[c].y), each ONE fp32 product (lsm2d_preprocess_scans' product, oracle F2.1); dir[c] is the cosine
 *              and sine of the bearing (c - n_beams / 2) * (angle_max - angle_min) / n_beams from the host's libm, made once per sensor geometry (the
 *              preprocessor's table and cache).  With a pose the end point is moved by xf_point under the isometry of pose[k] (item 17c.1 / 11b) and the
 *              ray starts at the pose's translation; pose == NULL copies the bits and the ray starts at (0, 0).                                [item 17d.2]
 *   cells      item 17c.2 unchanged: floorf((v - o) * inv), all four cells in [-2^20, 2^20), L <= LSM2D_OCCUPANCY_MAX_RAY_CELLS; a ray that fails is
 *              dropped and counted.                                                                                                            [item 17d.3]
 *   walk       item 17c.3 unchanged.  A HIT ray adds misses on steps 0 .. L - 1 and a hit on step L; a CLEAR ray adds a miss on EVERY step 0 .. L and no hit
 *              (its end cell is known free: trace_range <= range_max is required, the beam had no return before l).  Cells outside the grid add nothing
 *              and the ray goes on; counters saturate at 2^32 - 1.  Per grid out_hit_rays + out_clear_rays + out_dropped = the beams sent to it. [item 17d.4]
 * Refused before anything is launched or written, with LSM2D_CAPACITY_EXCEEDED for n_beams outside 1 .. 2048 (as the preprocessor) and LSM2D_BAD_ARGUMENT
 * for: a NULL the call needs; a set of another or a destroyed context; n_scans < 1; n_scans * n_beams > LSM2D_OCCUPANCY_MAX_RAYS; !(angle_max > angle_min);
 * a non-finite range_min, range_max or trace_range; range_min < 0; range_min > range_max; !(trace_range > 0); trace_range < range_min; trace_range >
 * range_max; clear_no_return outside {0, 1}; a grid value outside [0, n_grids); device-resident ranges on another device; both lanes busy.
 * Cost: synchronous.  ONE upload of the call's tables (with pageable ranges in the same copy; pinned ranges are copied from directly; device-resident
 * ranges are read in place), TWO launches -- k_occ_beams (a thread per beam) and k_occ_tiles<true> (k_occ_tiles over records that carry the ray's
 * kind) --, ONE copy down (hit rays, clear rays, dropped, fault word) and ONE wait.  No size fetch: nothing has a size the host does not know.
 * "kernel_timing" / lsm2d_last_kernel_ms bracket the chain and "last_occupancy_wg_median_ns" / "last_occupancy_wg_max_ns" work as in 0.7.12.
 * NOT BUILT (item 17d.5): an asynchronous form; per-grid geometry or per-scan sensor parameters; a once-per-scan rule for counts sets; splitting a tile's
 * work over several workgroups; intensity or multi-echo.  (0.7.14: into a log-odds set -- below -- this call gives every cell one clamped vote per scan.) */
typedef struct lsm2d_occupancy_scan_params {
  int32_t n_beams;               /* 1 .. 2048, as lsm2d_preprocessor */
  float   angle_min, angle_max;  /* as lsm2d_preprocessor: bearing of beam c = (c - n/2) * (angle_max - angle_min) / n */
  float   range_min, range_max;  /* a return: range_min <= r <= range_max (F2.1's gate) */
  float   trace_range;           /* no ray is traced farther than this [m] */
  int32_t clear_no_return;       /* 1: a beam with r > range_max (+Inf included) clears out to trace_range; 0: it is dropped */
} lsm2d_occupancy_scan_params;

int lsm2d_occupancy_update_scans(lsm2d_context* ctx, lsm2d_gridset* grids, const lsm2d_occupancy_scan_params* params,
                                 const float* ranges,     /* [n_scans][n_beams]: pageable, pinned or device memory of the context's device */
                                 int32_t n_scans,
                                 const float* pose,       /* [n_scans][3] sensor in the grid's frame, or NULL */
                                 const int32_t* grid,     /* [n_scans] or NULL: all 0 */
                                 int32_t* out_hit_rays, int32_t* out_clear_rays, int32_t* out_dropped /* each [n_grids] or NULL */);

/* Log-odds grid sets (0.7.14) -- a second kind of lsm2d_gridset that both update calls above accept, with its own entry points -- are declared in
 * lsm2d_logodds.h, an extension of this header (as host/lsm2d_occupancy.hpp extends host/lsm2d.hpp); this header keeps its set of symbols. */

/* What an alignment of `batch` will cost relative to the others, WITHOUT running it: for projective slices against a map-sized moving cloud the
 * number of chunks of that cloud (of 512) that survive the exact culling against the alignment's fixed canvas at its start pose -- what its first
 * iteration streams (k_cull_estimate: the quantity lsm2d_align_batch itself places a batch on the chip by); 1 for every alignment when there is
 * no such slice.  A caller that shards a candidate sweep over several devices or processes (MultiLoopDetectorBruteForce2D's loop, MULTI.json:964-986)
 * balances the shards by the SUM of these numbers instead of by candidate count: with the culling an alignment's time follows it (33-59 % of the
 * chunks survive on configs[1]).  out_work: [n_alignments]. */
int lsm2d_estimate_work(lsm2d_context* ctx, const lsm2d_batch* batch, int32_t* out_work);

/* lsm2d_align_batch in two halves: what a host that feeds the aligner batch after batch does between launching one and needing its poses
 * (the reference's candidate loop, MULTI.json:964-986, and its per-scan tracker, apps/visual_test_aligner_2d.cpp:123-156, are synchronous: this is
 * what a pipelined host puts in their place).  begin() queues everything -- start poses, placement, kernels, the copies of the results -- and returns;
 * the batch descriptor and what it points to may be reused as soon as it has.  wait() blocks until THAT batch is done (a younger one may be queued
 * behind it) and fills the outputs exactly as lsm2d_align_batch would have: begin + wait == lsm2d_align_batch, bit for bit.  While a batch is in flight,
 * the NEXT batch's lsm2d_preprocess_scans_refill and the pre-kernels of its begin() run on side streams, in the slots the launch in flight leaves
 * free; and each asynchronously begun batch launches on a stream of its LANE's own, so the younger of two batches in flight starts on the slots the older one's
 * tail leaves free instead of waiting for its last workgroup (configs[1], the same resident batch begun again and again: 0.69 ms per batch against 0.76 one at a time).  At most two batches are in flight per context; they are waited for in the order they were begun; every begun batch must be waited for.
 * While TWO are in flight the context's staging buffers are theirs: lsm2d_preprocess_scans_refill, lsm2d_align_batch_wait, the option calls and
 * lsm2d_synchronize work, every other call that moves data returns LSM2D_BAD_ARGUMENT (with one in flight everything works).
 * The cloud sets a batch in flight reads must not be modified: a pipeline alternates between two scan sets -- or, better, between THREE, refilling a step
 * ahead: per step  begin(i) ; refill(set of step i + 1) ; wait(i - 1).  The launch in flight holds every wave slot of the chip, so a preprocessing launch
 * queued beside it finishes only after it; queued a step ahead it is done before begin(i + 1) queues the estimate that reads its clouds, and batch i + 1
 * starts where batch i ends (tests/cpp/stream_step_bench.cpp, bench.py --stream).
 * want_stats != 0: the batch keeps per-iteration statistics (wait's out_stats may then be non-NULL). */
typedef struct lsm2d_pending lsm2d_pending;
int lsm2d_align_batch_begin(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch, int32_t want_stats, lsm2d_pending** out_pending);
int lsm2d_align_batch_wait(lsm2d_pending* pending, float* out_pose, float* out_H, int32_t* out_status, int32_t* out_iterations, lsm2d_iteration_stats* out_stats);

/* The same call, additionally handing back what aligner->compute() leaves in every slice's correspondence vector (the reference's
 * slice->correspondences(), apps/visual_test_aligner_2d.cpp:129-143): the pairs of the LAST iteration each alignment started, in the finder's
 * order (ascending column / ascending moving index) -- with keep_only_inlier_correspondences only those whose factor was an inlier in that
 * iteration.  out_pairs: [n][n_slices][pair_capacity]; out_n_pairs: [n][n_slices].  pair_capacity must hold a slice's largest possible vector
 * (canvas_cols of a projective slice, the largest moving cloud of a point-query slice) or the call returns LSM2D_CAPACITY_EXCEEDED.  The
 * pairs are re-derived after the aligner kernel from the pose its last iteration started at: ONE batched finder pass per slice over the
 * alignments that started an iteration (lsm2d_find_correspondences_batch's kernels: a workgroup per alignment, one wait per launch; a call
 * with a single alignment keeps one lsm2d_find_correspondences pass per slice) -- the same arithmetic, hence the same pairs: tests compare
 * their digest with the in-kernel one.  out_pairs == NULL is lsm2d_align_batch. */
int lsm2d_align_batch_pairs(lsm2d_context* ctx, const lsm2d_aligner_params* aligner, const lsm2d_batch* batch,
                            float* out_pose, float* out_H, int32_t* out_status, int32_t* out_iterations, lsm2d_iteration_stats* out_stats,
                            lsm2d_correspondence* out_pairs, int32_t pair_capacity, int32_t* out_n_pairs);

/* ---- the candidate loop of MultiLoopDetectorBruteForce2D / MultiRelocalizer2D (MULTI.json:964-986, :749-769) over the GPUs of one
 * node, in ONE process and without Python: a context per device, the submap uploaded to device_ids[0] once and replicated device to
 * device (xGMI), the distinct candidate scans replicated likewise, candidates block-sharded [r N / G, (r + 1) N / G) over the
 * devices, one host thread per device, results in candidate order.  Alignments are independent, so there is no collective on the
 * data path and the result of a candidate does not depend on G (tests: bit-identical to one lsm2d_align_batch).  Role assignment of
 * the reference tracker / loop detector: fixed = the candidate's scan, moving = the submap; one laser slice.
 * device_ids may name a device more than once (a rehearsal of G > 1 on a one-GPU box). */
typedef struct lsm2d_sweep lsm2d_sweep;
int     lsm2d_sweep_create(const int32_t* device_ids, int32_t n_devices, lsm2d_sweep** out_sweep);
void    lsm2d_sweep_destroy(lsm2d_sweep* sweep);
int32_t lsm2d_sweep_num_devices(const lsm2d_sweep* sweep);
const char* lsm2d_sweep_last_error(const lsm2d_sweep* sweep);
/* "peer_copy": 0 = automatic (default): a replica on another device is filled device to device when hipDeviceCanAccessPeer says the two
 * devices reach each other (peer access is enabled for the pair once), else -- and whenever a peer copy fails -- straight from the caller's
 * host buffer; 1 = always from the host buffer (what a node without xGMI / with peer access disabled gets; results do not depend on it).
 * Read-only: "replicas_by_peer_copy", "replicas_through_host", "replicas_same_device" -- how the replicas of the most recent
 * lsm2d_sweep_set_map / lsm2d_sweep_set_scans were filled. */
int     lsm2d_sweep_set_option(lsm2d_sweep* sweep, const char* key, int64_t value);
int     lsm2d_sweep_get_option(const lsm2d_sweep* sweep, const char* key, int64_t* out_value);
int     lsm2d_sweep_set_map(lsm2d_sweep* sweep, const float* map_xynn, int64_t n_points);
/* the distinct scans the candidates refer to: packed back to back, offsets[n_scans + 1] */
int     lsm2d_sweep_set_scans(lsm2d_sweep* sweep, const float* scans_xynn, const int32_t* offsets, int32_t n_scans);
/* candidate i = (scan scan_index[i] -- or scan i when scan_index is NULL -- , init_pose[i]); out_last_stats: the statistics of the last
 * iteration each candidate started (what the acceptance test of MULTI.json:979-985 reads); out_H / out_iterations / out_last_stats may be NULL */
int     lsm2d_sweep_align(lsm2d_sweep* sweep, const lsm2d_aligner_params* aligner, const lsm2d_slice_params* slice, int32_t n_candidates,
                          const int32_t* scan_index, const float* init_pose, float* out_pose, float* out_H, int32_t* out_status,
                          int32_t* out_iterations, lsm2d_iteration_stats* out_last_stats);
/* ... with the verdict made on the devices: every shard runs lsm2d_align_select with the same k on its block of candidates, the host merges the <= G x k
 * rows by the same key over GLOBAL candidate indices and sums the counts.  The order is total, so the result does not depend on G: it is
 * lsm2d_align_select's on one device, bit for bit.  Outputs and refusals as there (out_H / out_iterations / out_last_stats / out_n_success may be NULL). */
int     lsm2d_sweep_align_select(lsm2d_sweep* sweep, const lsm2d_aligner_params* aligner, const lsm2d_slice_params* slice, int32_t n_candidates,
                                 const int32_t* scan_index, const float* init_pose, const lsm2d_select_params* select, int32_t k,
                                 int32_t* out_index, float* out_pose, float* out_H, int32_t* out_iterations, lsm2d_iteration_stats* out_last_stats,
                                 int32_t* out_n_selected, int32_t* out_n_accepted, int32_t* out_n_success);

#ifdef __cplusplus
}
#endif
#endif /* LSM2D_H */
