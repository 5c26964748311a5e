// lsm2d_voxelize.hpp -- device-resident clouds voxelised and assembled in one call over the C ABI (include/lsm2d.h, 0.7.11): voxelize, and ReservedClouds, the
// set of growable clouds it writes into.  An extension of lsm2d.hpp (which it includes and whose types it uses).  Output cloud g is PointCloud::voxelize
// (raw_data_preprocessor_projective_2d.cpp:38-41, scene_clipper_projective_2d.cpp:44-48) of the concatenation of every input with group[k] == g, each first
// moved by its pose; dst may be src (a fleet's maps decimated in place).
#pragma once

#include "lsm2d.hpp"

namespace lsm2d_host {

// n_clouds growable device clouds with room for `capacity` points each (lsm2d_cloudset_create_reserved_many)
class ReservedClouds {
 public:
  ReservedClouds(Context& ctx, int32_t n_clouds, int64_t capacity) : _ctx(ctx) {
    check(lsm2d_cloudset_create_reserved_many(ctx.get(), n_clouds, capacity, _h.out()), "lsm2d_cloudset_create_reserved_many", ctx.get());
  }
  lsm2d_cloudset* get() const { return _h; }
  int32_t numClouds() const { return lsm2d_cloudset_num_clouds(get()); }
  int64_t size(int32_t i) const { return lsm2d_cloudset_cloud_size(get(), i); }
  PointNormal2fVectorCloud download(int32_t i) const {
    const int64_t m = size(i);
    PointNormal2fVectorCloud c((size_t) (m > 0 ? m : 0)); int64_t n = 0;
    check(lsm2d_cloudset_download(get(), i, c.empty() ? nullptr : &c[0].x, (int64_t) c.size(), &n), "lsm2d_cloudset_download", _ctx.get());
    c.resize((size_t) n); return c;
  }
 private:
  Context& _ctx; detail::CloudSetHandle _h;
};

// counts[g]: voxels written to group g's cloud; dropped[g]: its points that had no key.  `fits` is false when some group had more voxels than its cloud
// has room for: then NOTHING was written and counts holds what would have been needed.
struct Voxelization { std::vector<int32_t> counts, dropped; bool fits = true; };

// src_index empty: input k is cloud k of src (n_inputs = its clouds); poses empty: no transform at all; groups empty: every input in group 0;
// dst_index empty: group g goes to cloud g of dst.  Throws on every refusal of the call; a group that does not fit is reported, not thrown.
inline Voxelization voxelize(Context& ctx, const lsm2d_voxelize_params& params, const lsm2d_cloudset* src, lsm2d_cloudset* dst, int32_t n_groups = 1,
                             const std::vector<int32_t>& src_index = {}, const std::vector<Vector3f>& poses = {}, const std::vector<int32_t>& groups = {},
                             const std::vector<int32_t>& dst_index = {}) {
  const int32_t n_inputs = src_index.empty() ? lsm2d_cloudset_num_clouds(src) : (int32_t) src_index.size();
  const size_t n = (size_t) (n_inputs > 0 ? n_inputs : 0), ng = (size_t) (n_groups > 0 ? n_groups : 0);
  if ((!poses.empty() && poses.size() != n) || (!groups.empty() && groups.size() != n) || (!dst_index.empty() && dst_index.size() != ng))
    throw std::runtime_error("voxelize| poses and groups are empty or hold one entry per input, dst_index is empty or holds one per group");
  Voxelization out;
  out.counts.assign(ng ? ng : 1, 0); out.dropped.assign(ng ? ng : 1, 0);
  const int rc = lsm2d_voxelize(ctx.get(), &params, src, n_inputs, ptrOrNull(src_index), ptrOrNull(poses), ptrOrNull(groups), n_groups, dst, ptrOrNull(dst_index),
                                out.counts.data(), out.dropped.data());
  out.counts.resize(ng); out.dropped.resize(ng);
  if (rc == LSM2D_CAPACITY_EXCEEDED) { out.fits = false; return out; }
  check(rc, "lsm2d_voxelize", ctx.get());
  return out;
}

}  // namespace lsm2d_host
