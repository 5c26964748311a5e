// lsm2d_occupancy.hpp -- occupancy grids on the device over the C ABI (include/lsm2d.h, 0.7.12): GridSet, the owner of a lsm2d_gridset, occupancyUpdate
// (the points of device-resident clouds ray-traced from their sensor poses into hit / miss counters) and occupancyRender (the counters as a map consumer
// reads them); from 0.7.13 occupancyUpdateScans (raw range scans, the beams without a return cleared).  An extension of lsm2d.hpp (which it includes and whose types it uses; lsm2d.hpp itself keeps its set of C calls).  A capability of this
// build: the reference tree has no grid mapper (PARITY.md section 3, item 17c).
#pragma once

#include "lsm2d.hpp"
#include <lsm2d_logodds.h>      // log-odds grid sets (0.7.14): the extension header of the C ABI

namespace lsm2d_host {

// lsm2d_logodds_params in integer units of the caller's choice: the votes of a hit and of a miss, and the clamps
struct LogOddsParams : lsm2d_logodds_params {
  LogOddsParams(int32_t l_hit_, int32_t l_miss_, int32_t l_min_, int32_t l_max_) : lsm2d_logodds_params{l_hit_, l_miss_, l_min_, l_max_} {}
};

// n_grids device-resident grids of one geometry, two uint32 counters per cell (hits, misses), zero at creation; host arrays are [height][width]
class GridSet {
 public:
  struct Counters { std::vector<uint32_t> hits, misses; };
  struct LogOdds { std::vector<int32_t> value; std::vector<uint32_t> observed; };
  GridSet(Context& ctx, const lsm2d_grid_geometry& geometry, int32_t n_grids = 1) : _ctx(ctx), _geometry(geometry), _n_grids(n_grids) {
    check(lsm2d_gridset_create(ctx.get(), &geometry, n_grids, &_h), "lsm2d_gridset_create", ctx.get());
  }
  // a log-odds set (0.7.14): a cell is {int32 value, uint32 observed}; every scan of an update gives a cell ONE clamped vote, the scans in list order
  GridSet(Context& ctx, const lsm2d_grid_geometry& geometry, int32_t n_grids, const lsm2d_logodds_params& logodds)
      : _ctx(ctx), _geometry(geometry), _n_grids(n_grids), _logodds(true) {
    check(lsm2d_gridset_create_logodds(ctx.get(), &geometry, n_grids, &logodds, &_h), "lsm2d_gridset_create_logodds", ctx.get());
  }
  bool isLogOdds() const { return _logodds; }
  // the votes and clamps of LATER updates; host-side only
  void setLogOdds(const lsm2d_logodds_params& p) { check(lsm2d_gridset_set_logodds(_h, &p), "lsm2d_gridset_set_logodds", _ctx.get()); }
  // an empty vector leaves that word as it is; values outside the clamps are legal
  void uploadLogOdds(int32_t grid_index, const std::vector<int32_t>& value, const std::vector<uint32_t>& observed) {
    if ((!value.empty() && value.size() != cells()) || (!observed.empty() && observed.size() != cells()))
      throw std::runtime_error("GridSet::uploadLogOdds| value and observed are empty or hold height x width cells");
    check(lsm2d_gridset_upload_logodds(_h, grid_index, detail::ptrOrNull(value), detail::ptrOrNull(observed)), "lsm2d_gridset_upload_logodds", _ctx.get());
  }
  LogOdds downloadLogOdds(int32_t grid_index) const {
    LogOdds c; c.value.resize(cells()); c.observed.resize(cells());
    check(lsm2d_gridset_download_logodds(_h, grid_index, c.value.data(), c.observed.data()), "lsm2d_gridset_download_logodds", _ctx.get());
    return c;
  }
  ~GridSet() { lsm2d_gridset_destroy(_h); }
  GridSet(const GridSet&) = delete; GridSet& operator=(const GridSet&) = delete;
  lsm2d_gridset* get() const { return _h; }
  int32_t numGrids() const { return _n_grids; }
  const lsm2d_grid_geometry& geometry() const { return _geometry; }
  size_t cells() const { return (size_t) _geometry.width * (size_t) _geometry.height; }
  // indices empty: every grid
  void clear(const std::vector<int32_t>& indices = {}) {
    check(lsm2d_gridset_clear(_h, (int32_t) indices.size(), detail::ptrOrNull(indices)), "lsm2d_gridset_clear", _ctx.get());
  }
  // an empty vector leaves that counter as it is
  void upload(int32_t grid_index, const std::vector<uint32_t>& hits, const std::vector<uint32_t>& misses) {
    if ((!hits.empty() && hits.size() != cells()) || (!misses.empty() && misses.size() != cells()))
      throw std::runtime_error("GridSet::upload| hits and misses are empty or hold height x width counters");
    check(lsm2d_gridset_upload(_h, grid_index, detail::ptrOrNull(hits), detail::ptrOrNull(misses)), "lsm2d_gridset_upload", _ctx.get());
  }
  Counters download(int32_t grid_index) const {
    Counters c; c.hits.resize(cells()); c.misses.resize(cells());
    check(lsm2d_gridset_download(_h, grid_index, c.hits.data(), c.misses.data()), "lsm2d_gridset_download", _ctx.get());
    return c;
  }
 private:
  Context& _ctx; lsm2d_grid_geometry _geometry; int32_t _n_grids; bool _logodds = false; lsm2d_gridset* _h = nullptr;
};

// rays[g]: rays walked into grid g; dropped[g]: its points that gave no ray
struct OccupancyUpdate { std::vector<int32_t> rays, dropped; };

// src_index empty: input k is cloud k of src (n_inputs = its clouds); poses empty: no transform at all, every ray starts at (0, 0); grid empty: every
// input into grid 0.  Throws on every refusal of the call.
inline OccupancyUpdate occupancyUpdate(Context& ctx, GridSet& grids, const lsm2d_cloudset* src, const std::vector<int32_t>& src_index = {},
                                       const std::vector<Vector3f>& poses = {}, const std::vector<int32_t>& grid = {}) {
  const int32_t n_inputs = src_index.empty() ? lsm2d_cloudset_num_clouds(src) : (int32_t) src_index.size();
  const size_t n = (size_t) (n_inputs > 0 ? n_inputs : 0);
  if ((!poses.empty() && poses.size() != n) || (!grid.empty() && grid.size() != n))
    throw std::runtime_error("occupancyUpdate| poses and grid are empty or hold one entry per input");
  OccupancyUpdate out;
  out.rays.assign((size_t) grids.numGrids(), 0); out.dropped.assign((size_t) grids.numGrids(), 0);
  check(lsm2d_occupancy_update(ctx.get(), grids.get(), src, n_inputs, ptrOrNull(src_index), ptrOrNull(poses), ptrOrNull(grid), out.rays.data(), out.dropped.data()),
        "lsm2d_occupancy_update", ctx.get());
  return out;
}

// lsm2d_occupancy_update_scans' parameters, with the defaults a caller most often keeps
struct OccupancyScanParams : lsm2d_occupancy_scan_params {
  OccupancyScanParams(int32_t n_beams_, float angle_min_, float angle_max_, float range_min_ = 0.0f, float range_max_ = 30.0f, float trace_range_ = 30.0f,
                      bool clear_no_return_ = true)
      : lsm2d_occupancy_scan_params{n_beams_, angle_min_, angle_max_, range_min_, range_max_, trace_range_, clear_no_return_ ? 1 : 0} {}
};

// hit_rays[g] / clear_rays[g]: rays walked into grid g that end in a hit / that only clear; dropped[g]: its beams that gave no ray
struct OccupancyScanUpdate { std::vector<int32_t> hit_rays, clear_rays, dropped; };

// ranges: [n_scans][n_beams] in pageable, pinned or device memory of the context's device; poses empty: no transform, every ray starts at (0, 0); grid
// empty: every scan into grid 0.  Throws on every refusal of the call.
inline OccupancyScanUpdate occupancyUpdateScans(Context& ctx, GridSet& grids, const lsm2d_occupancy_scan_params& params, const float* ranges, int32_t n_scans,
                                                const std::vector<Vector3f>& poses = {}, const std::vector<int32_t>& grid = {}) {
  const size_t n = (size_t) (n_scans > 0 ? n_scans : 0);
  if ((!poses.empty() && poses.size() != n) || (!grid.empty() && grid.size() != n))
    throw std::runtime_error("occupancyUpdateScans| poses and grid are empty or hold one entry per scan");
  OccupancyScanUpdate out;
  out.hit_rays.assign((size_t) grids.numGrids(), 0); out.clear_rays.assign((size_t) grids.numGrids(), 0); out.dropped.assign((size_t) grids.numGrids(), 0);
  check(lsm2d_occupancy_update_scans(ctx.get(), grids.get(), &params, ranges, n_scans, ptrOrNull(poses), ptrOrNull(grid), out.hit_rays.data(),
                                     out.clear_rays.data(), out.dropped.data()),
        "lsm2d_occupancy_update_scans", ctx.get());
  return out;
}

// [height][width]: -1 where hits + misses < max(min_visits, 1), else the share of hits in percent, 0 .. 100
inline std::vector<int8_t> occupancyRender(Context& ctx, const GridSet& grids, int32_t grid_index = 0, int32_t min_visits = 1) {
  const lsm2d_occupancy_render_params p{min_visits};
  std::vector<int8_t> out(grids.cells());
  check(lsm2d_occupancy_render(ctx.get(), grids.get(), grid_index, &p, out.data()), "lsm2d_occupancy_render", ctx.get());
  return out;
}

// every observed cell of grids `indices` (empty: every grid) of a log-odds set moves toward 0 by amount >= 0, never past it; queued, no wait
inline void occupancyDecay(Context& ctx, GridSet& grids, int32_t amount, const std::vector<int32_t>& indices = {}) {
  check(lsm2d_occupancy_decay(ctx.get(), grids.get(), (int32_t) indices.size(), detail::ptrOrNull(indices), amount), "lsm2d_occupancy_decay", ctx.get());
}

// the 100 thresholds of `unit` (log-odds per integer unit): entry j - 1 is the smallest value that renders as j percent or more.  Host only.
inline std::vector<int32_t> logOddsRenderTable(float unit) {
  std::vector<int32_t> t(100);
  if (lsm2d_logodds_render_table(unit, t.data()) != LSM2D_SUCCESS) throw std::runtime_error("logOddsRenderTable| unit must be finite and > 0");
  return t;
}

// [height][width] of a log-odds set: -1 where observed < max(min_scans, 1), else the probability in percent, 0 .. 100, by the table of `unit`
inline std::vector<int8_t> occupancyRenderLogOdds(Context& ctx, const GridSet& grids, int32_t grid_index, float unit, int32_t min_scans = 1) {
  const lsm2d_logodds_render_params p{min_scans, unit};
  std::vector<int8_t> out(grids.cells());
  check(lsm2d_occupancy_render_logodds(ctx.get(), grids.get(), grid_index, &p, out.data()), "lsm2d_occupancy_render_logodds", ctx.get());
  return out;
}

}  // namespace lsm2d_host
