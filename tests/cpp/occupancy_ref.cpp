// occupancy_ref.cpp -- the definition of lsm2d_occupancy_update (PARITY.md section 3, item 17c), restated on the host as plain loops: test infrastructure,
// built as a shared object by tests/occupancy_cases.py through tests/cpp_build.py (and compiled into tests/cpp/occupancy_bench.cpp as the host route).
// Every fused multiply-add is libm's fmaf (a true one); compiled with -ffp-contract=off, so no other operation is fused.  tests/test_occupancy_abi.py pins
// the transform to voxelize_cases.transform (itself pinned to the oracle's merger) and the walk to an independent incremental one.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

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

// item 17c.1: the point under the isometry of a pose (normals are not read)
void transform(const Iso& T, const float* p, float* q) {
  q[0] = fmaf(T.c, p[0], fmaf(-T.s, p[1], T.tx));
  q[1] = fmaf(T.s, p[0], fmaf(T.c, p[1], T.ty));
}

// item 17c.2: the cell of a coordinate; the difference and the product are rounded separately
float cell_of(float v, float o, float inv) { return floorf((v - o) * inv); }
bool in_range(float c) { return c >= -1048576.0f && c < 1048576.0f; }

// -> true and the four cell coordinates, or false: no ray
bool make_ray(float sx, float sy, float px, float py, float ox, float oy, float inv, int32_t* r) {
  const float fx0 = cell_of(sx, ox, inv), fy0 = cell_of(sy, oy, inv), fx1 = cell_of(px, ox, inv), fy1 = cell_of(py, oy, inv);
  if (!(in_range(fx0) && in_range(fy0) && in_range(fx1) && in_range(fy1))) return false;
  r[0] = (int32_t) fx0; r[1] = (int32_t) fy0; r[2] = (int32_t) fx1; r[3] = (int32_t) fy1;
  const long long ax = llabs((long long) r[2] - r[0]), ay = llabs((long long) r[3] - r[1]);
  return (ax > ay ? ax : ay) <= 32767;
}

// item 17c.3: step i of the ray, from the closed form
void step_cell(const int32_t* r, int i, int32_t* cx, int32_t* cy) {
  const int dx = r[2] - r[0], dy = r[3] - r[1];
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
  const bool xm = ax >= ay;
  const int L = xm ? ax : ay, a = xm ? ay : ax;
  const int off = L ? (int) ((2ll * i * a + L) / (2ll * L)) : 0;
  if (xm) { *cx = r[0] + sx * i; *cy = r[1] + sy * off; } else { *cy = r[1] + sy * i; *cx = r[0] + sx * off; }
}

void add_sat(uint32_t* c) { if (*c != 0xffffffffu) ++*c; }
}  // namespace

extern "C" {

// out[i] = (x, y) of points[i] (rows of 4 floats) moved by pose (x, y, theta); the normals are copied
void occref_transform(const float* points, int n, const float* pose, float* out) {
  Iso T; sincos_fixed(pose[2], T.s, T.c); T.tx = pose[0]; T.ty = pose[1];
  for (int i = 0; i < n; ++i) { transform(T, points + 4 * (size_t) i, out + 4 * (size_t) i); out[4 * (size_t) i + 2] = points[4 * (size_t) i + 2]; out[4 * (size_t) i + 3] = points[4 * (size_t) i + 3]; }
}

// rays[i] = {x0, y0, x1, y1} and live[i] = 1, or live[i] = 0, for the points of ONE input as item 17c.1-2 make them
void occref_rays(const float* points, int n, const float* pose /* [3] or NULL */, float ox, float oy, float resolution, int32_t* rays, int32_t* live) {
  const float inv = 1.0f / resolution;
  Iso T = {1.0f, 0.0f, 0.0f, 0.0f}; float sx = 0.0f, sy = 0.0f;
  if (pose) { sincos_fixed(pose[2], T.s, T.c); T.tx = pose[0]; T.ty = pose[1]; sx = pose[0]; sy = pose[1]; }
  for (int i = 0; i < n; ++i) {
    float q[2] = {points[4 * (size_t) i], points[4 * (size_t) i + 1]};
    if (pose) transform(T, points + 4 * (size_t) i, q);
    int32_t r[4] = {0, 0, 0, 0};
    live[i] = make_ray(sx, sy, q[0], q[1], ox, oy, inv, r) ? 1 : 0;
    memcpy(rays + 4 * (size_t) i, r, sizeof r);
  }
}

// the L + 1 cells of a ray, in step order: cells [L + 1][2]
void occref_walk(const int32_t* ray, int32_t* cells) {
  const int ax = abs(ray[2] - ray[0]), ay = abs(ray[3] - ray[1]);
  const int L = ax > ay ? ax : ay;
  for (int i = 0; i <= L; ++i) step_cell(ray, i, cells + 2 * (size_t) i, cells + 2 * (size_t) i + 1);
}

// points: the inputs back to back (rows of 4 floats), offsets[n_inputs + 1]; pose [n_inputs][3] or NULL; grid [n_inputs] or NULL.  hits / misses:
// [n_grids][height][width], ACCUMULATED into (saturating); rays / dropped: [n_grids], set.
void occref_update(const float* points, const int32_t* offsets, int n_inputs, const float* pose, const int32_t* grid, int n_grids, float ox, float oy,
                   float resolution, int width, int height, uint32_t* hits, uint32_t* misses, int32_t* rays, int32_t* dropped) {
  const float inv = 1.0f / resolution;
  for (int g = 0; g < n_grids; ++g) { rays[g] = 0; dropped[g] = 0; }
  for (int k = 0; k < n_inputs; ++k) {
    const int g = grid ? grid[k] : 0;
    uint32_t* const H = hits + (size_t) g * width * height; uint32_t* const M = misses + (size_t) g * width * height;
    Iso T = {1.0f, 0.0f, 0.0f, 0.0f}; float sx = 0.0f, sy = 0.0f;
    if (pose) { sincos_fixed(pose[3 * k + 2], T.s, T.c); T.tx = pose[3 * k]; T.ty = pose[3 * k + 1]; sx = T.tx; sy = T.ty; }
    for (int i = offsets[k]; i < offsets[k + 1]; ++i) {
      float q[2] = {points[4 * (size_t) i], points[4 * (size_t) i + 1]};
      if (pose) transform(T, points + 4 * (size_t) i, q);
      int32_t r[4];
      if (!make_ray(sx, sy, q[0], q[1], ox, oy, inv, r)) { ++dropped[g]; continue; }
      ++rays[g];
      const int ax = abs(r[2] - r[0]), ay = abs(r[3] - r[1]);
      const int L = ax > ay ? ax : ay;
      for (int s = 0; s <= L; ++s) {
        int32_t cx, cy; step_cell(r, s, &cx, &cy);
        if (cx < 0 || cy < 0 || cx >= width || cy >= height) continue;
        add_sat((s == L ? H : M) + (size_t) cy * width + cx);
      }
    }
  }
}

}  // extern "C"
