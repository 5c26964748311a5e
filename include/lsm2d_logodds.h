/* lsm2d_logodds.h -- log-odds grid sets (ABI 0.7.14): an extension of lsm2d.h, which it includes and whose types it uses; the symbols are exported by the
 * same library (liblsm2d_hip.so).  lsm2d.h keeps its set of symbols; a caller that wants occupancy as clamped log-odds includes this header instead. */
#ifndef LSM2D_LOGODDS_H
#define LSM2D_LOGODDS_H

#include "lsm2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- log-odds grid sets (0.7.14): occupancy as clamped log-odds, a scan counts ONCE per cell.  A grid set of a second kind: the allocation and geometry
 * of a counts set, a cell still one 8-byte access, {int32 value, uint32 observed}: value is the log-odds in integer units of the caller's choice,
 * observed the number of scans that voted on the cell, saturating at 2^32 - 1; observed == 0 is unknown.  Like 0.7.12 / 0.7.13 a capability of this build
 * (the reference tree has no grid mapper); the definition is the contract (PARITY.md section 3, item 17e) and is integers throughout.
 *   update     lsm2d_occupancy_update and lsm2d_occupancy_update_scans accept either kind of set; the set's kind picks the tile kernel, everything else
 *              of the call is unchanged.  Into a log-odds set the scans sent to a grid (an input cloud / a row of ranges) are applied ONE AFTER THE OTHER
 *              in ascending position in the call's list.  For scan s, with rays, classes, transform, cells and walk those of items 17c / 17d:
 *                H_s = the grid cells that are step L of a HIT ray of s; M_s = the grid cells that are a miss step of any ray of s and not in H_s (the hit
 *                wins, also over a CLEAR ray of the same scan that passes through);
 *                c in H_s: value = clamp((int64) value + l_hit, l_min, l_max); c in M_s: the same with l_miss; c in either: observed += 1, saturating;
 *                every other cell keeps its bits.
 *              The clamp makes the order of the scans matter, hence the fixed order; within a scan there is none.  ONE call over scans 0 .. n - 1 equals
 *              n calls of one scan each.  out_rays / out_hit_rays / out_clear_rays / out_dropped keep their meaning: they count rays, not votes.
 *   params     1 <= l_hit <= 2^20; -2^20 <= l_miss <= -1; -2^30 <= l_min <= 0 <= l_max <= 2^30.  lsm2d_gridset_set_logodds is host-side only.  Uploaded
 *              values outside the clamps are legal (the sum is taken in 64 bits and pulled in by the next vote).
 *   decay      lsm2d_occupancy_decay: a cell with observed > 0 moves toward 0 by amount >= 0, never past it: v > 0 -> max(v - amount, 0), v < 0 ->
 *              min(v + amount, 0); observed is unchanged.  Queued, no wait, like lsm2d_gridset_clear; grid_index NULL: every grid.
 *   render     lsm2d_logodds_render_table (host only, launches nothing): entry j - 1, j = 1 .. 100, is ceil(log((j - 0.5) / (100.5 - j)) / unit) in
 *              double, clamped to int32; unit > 0 and finite, in log-odds per integer unit.  THE TABLE IS THE DEFINITION OF THE RENDERING: the rendered
 *              value of v is the number of thresholds <= v, 0 .. 100 (50 for v == 0).  lsm2d_occupancy_render_logodds gives -1 where observed <
 *              max(min_scans, 1), else that number; the 100 thresholds ride in the kernel's arguments, no exponential runs on the device; one copy down
 *              and one wait, as lsm2d_occupancy_render.
 * lsm2d_gridset_clear and lsm2d_gridset_destroy serve both kinds.  lsm2d_gridset_upload, lsm2d_gridset_download and lsm2d_occupancy_render refuse a
 * log-odds set; the _logodds calls and lsm2d_occupancy_decay refuse a counts set.  Refused with LSM2D_BAD_ARGUMENT before anything is launched or written:
 * a parameter outside the constraints; a NULL the call needs; the wrong kind of set; amount < 0; a unit that is not > 0 or not finite; an index outside
 * the set.
 * Kernels: k_occ_tiles_logodds (the launch shape and the tile walk of k_occ_tiles: a workgroup per grid and 64 x 64 tile, one owner per tile, no global
 * atomics on the grid; the kept inputs in ascending order, the tile's words in LDS, two 4096-bit masks per scan, two barriers per kept scan), k_occ_decay and
 * k_occ_render_logodds (a thread per cell).  No older kernel changed.
 * NOT BUILT (item 17e.6): an asynchronous form; per-grid geometry; per-scan sensor parameters; splitting a tile's work over several workgroups; intensity
 * or multi-echo; a once-per-scan rule for counts sets. */
typedef struct lsm2d_logodds_params { int32_t l_hit, l_miss, l_min, l_max; } lsm2d_logodds_params;
typedef struct lsm2d_logodds_render_params { int32_t min_scans; float unit; } lsm2d_logodds_render_params;

int lsm2d_gridset_create_logodds(lsm2d_context* ctx, const lsm2d_grid_geometry* geometry, int32_t n_grids, const lsm2d_logodds_params* params,
                                 lsm2d_gridset** out);                                                              /* all cells zero: unknown */
int lsm2d_gridset_set_logodds(lsm2d_gridset* grids, const lsm2d_logodds_params* params);                            /* for later updates */
int lsm2d_gridset_upload_logodds(lsm2d_gridset* grids, int32_t grid_index, const int32_t* value, const uint32_t* observed);   /* a NULL array leaves that word */
int lsm2d_gridset_download_logodds(const lsm2d_gridset* grids, int32_t grid_index, int32_t* out_value, uint32_t* out_observed); /* either may be NULL */
int lsm2d_occupancy_decay(lsm2d_context* ctx, lsm2d_gridset* grids, int32_t n, const int32_t* grid_index /* [n] or NULL: every grid */, int32_t amount);
int lsm2d_logodds_render_table(float unit, int32_t out_threshold[100]);
int lsm2d_occupancy_render_logodds(lsm2d_context* ctx, const lsm2d_gridset* grids, int32_t grid_index,
                                   const lsm2d_logodds_render_params* params, int8_t* out /* host [height][width] */);

#ifdef __cplusplus
}
#endif
#endif /* LSM2D_LOGODDS_H */
