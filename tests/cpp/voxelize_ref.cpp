// voxelize_ref.cpp -- the definition of lsm2d_voxelize (PARITY.md section 3, item 17b), restated on the host in fp32: test infrastructure, built as a shared
// object by tests/voxelize_cases.py through tests/cpp_build.py.  Every fused multiply-add is libm's fmaf (a true one); compiled with -ffp-contract=off, so no
// other operation is fused.  tests/test_voxelize_abi.py pins it to the CPU oracle bit for bit.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace {
struct Iso { float c, s, tx, ty; };

// item 11b: cosine and sine of a pose angle as a fixed sequence of fp32 operations
void sincos_fixed(float x, float& sn, float& cs) {
  const float kf = rintf(x * 6.3661974669e-01f);
  float r = fmaf(-kf, 1.5707963705e+00f, x);
  r = fmaf(-kf, -4.3711388287e-08f, r);
  const float z = r * r;
  float ps = -1.9495635934e-04f; ps = fmaf(ps, z, 8.3319786936e-03f); ps = fmaf(ps, z, -1.6666650772e-01f);
  const float s = fmaf(r * z, ps, r);
  float pc = 2.4438450055e-05f; pc = fmaf(pc, z, -1.3887367677e-03f); pc = fmaf(pc, z, 4.1666645557e-02f);
  const float c = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
  const int q = (int) kf & 3;
  sn = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
  cs = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
}

// item 1: the point and the normal under the isometry of a pose, no renormalisation
void transform(const Iso& T, const float* p, float* q) {
  q[0] = fmaf(T.c, p[0], fmaf(-T.s, p[1], T.tx));
  q[1] = fmaf(T.s, p[0], fmaf(T.c, p[1], T.ty));
  q[2] = fmaf(T.c, p[2], (-T.s) * p[3]);
  q[3] = fmaf(T.s, p[2], T.c * p[3]);
}

// item 2: the 42-bit key, or -1
long long vox_key(const float* q, float inv_res, float inv_rn) {
  const float kx = floorf(q[0] * inv_res), ky = floorf(q[1] * inv_res), knx = floorf(q[2] * inv_rn), kny = floorf(q[3] * inv_rn);
  if (!(kx >= -32768.0f && kx < 32768.0f && ky >= -32768.0f && ky < 32768.0f && knx >= -16.0f && knx <= 15.0f && kny >= -16.0f && kny <= 15.0f)) return -1;
  return ((long long) ((int) kx + 32768) << 26) | ((long long) ((int) ky + 32768) << 10) | ((long long) ((int) knx + 16) << 5) | (long long) ((int) kny + 16);
}

struct Rec { int group; long long key; int idx; };
}  // namespace

extern "C" {

// out[i] = points[i] moved by pose (x, y, theta)
void voxref_transform(const float* points, int n, const float* pose, float* out) {
  Iso T; sincos_fixed(pose[2], T.s, T.c); T.tx = pose[0]; T.ty = pose[1];
  for (int i = 0; i < n; ++i) transform(T, points + 4 * (size_t) i, out + 4 * (size_t) i);
}

// keys[i] of the points as they are (no transform): the 42-bit key or -1
void voxref_keys(const float* points, int n, float resolution, float normal_resolution, long long* keys) {
  const float inv_res = 1.0f / resolution, inv_rn = 1.0f / normal_resolution;
  for (int i = 0; i < n; ++i) keys[i] = vox_key(points + 4 * (size_t) i, inv_res, inv_rn);
}

// points: the inputs back to back, offsets[n_inputs + 1]; pose [n_inputs][3] or NULL; group [n_inputs] or NULL.  out: [n][4], the groups' voxels back to
// back in group order; counts / dropped: [n_groups].  Returns the number of voxels in all.
int voxref_voxelize(const float* points, const int32_t* offsets, int n_inputs, const float* pose, const int32_t* group, int n_groups, float resolution,
                    float normal_resolution, float* out, int32_t* counts, int32_t* dropped) {
  const int n = offsets[n_inputs];
  const float inv_res = 1.0f / resolution, inv_rn = 1.0f / normal_resolution;
  std::vector<float> t((size_t) 4 * (n > 0 ? n : 1));
  std::vector<Rec> recs;
  for (int g = 0; g < n_groups; ++g) { counts[g] = 0; dropped[g] = 0; }
  for (int k = 0; k < n_inputs; ++k) {
    const int g = group ? group[k] : 0;
    Iso T = {1.0f, 0.0f, 0.0f, 0.0f};
    if (pose) { sincos_fixed(pose[3 * k + 2], T.s, T.c); T.tx = pose[3 * k]; T.ty = pose[3 * k + 1]; }
    for (int i = offsets[k]; i < offsets[k + 1]; ++i) {
      if (pose) transform(T, points + 4 * (size_t) i, &t[4 * (size_t) i]); else memcpy(&t[4 * (size_t) i], points + 4 * (size_t) i, sizeof(float) * 4);
      const long long key = vox_key(&t[4 * (size_t) i], inv_res, inv_rn);
      if (key < 0) { ++dropped[g]; continue; }
      recs.push_back(Rec{g, key, i});
    }
  }
  // item 3 (and 5): ascending (group, key), then ascending concatenation index
  std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.group != b.group ? a.group < b.group : (a.key != b.key ? a.key < b.key : a.idx < b.idx); });
  int n_out = 0;
  for (size_t b = 0; b < recs.size();) {      // item 4
    size_t e = b; float ax = 0.0f, ay = 0.0f, anx = 0.0f, any_ = 0.0f;
    while (e < recs.size() && recs[e].group == recs[b].group && recs[e].key == recs[b].key) {
      const float* q = &t[4 * (size_t) recs[e].idx];
      ax += q[0]; ay += q[1]; anx += q[2]; any_ += q[3]; ++e;
    }
    const float inv = 1.0f / (float) (e - b);
    ax *= inv; ay *= inv; anx *= inv; any_ *= inv;
    const float nn = sqrtf(fmaf(anx, anx, any_ * any_));
    if (nn > 0.0f) { anx = anx / nn; any_ = any_ / nn; }
    float* o = out + 4 * (size_t) n_out;
    o[0] = ax; o[1] = ay; o[2] = anx; o[3] = any_;
    ++n_out; ++counts[recs[b].group];
    b = e;
  }
  return n_out;
}

}  // extern "C"
