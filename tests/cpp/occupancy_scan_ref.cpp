// occupancy_scan_ref.cpp -- the definition of lsm2d_occupancy_update_scans (PARITY.md section 3, item 17d), restated on the host as plain loops: test
// infrastructure, built as a shared object by tests/occupancy_scan_cases.py through tests/cpp_build.py (and compiled into tests/cpp/occupancy_scan_bench.cpp
// as the host route).  Written independently of the kernels and of occupancy_ref.cpp: the walk here is the incremental error-term one, not the closed form.
// Every fused multiply-add is libm's fmaf (a true one); compiled with -ffp-contract=off, so no other operation is fused.  tests/test_occupancy_scan_abi.py
// pins it to occupancy_cases.reference (clouds made of its end points) and its end points to the oracle's preprocessor.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace occsref {
// lsm2d_occupancy_scan_params, field by field (the test passes the ABI's struct)
struct Params { int32_t n_beams; float angle_min, angle_max, range_min, range_max, trace_range; int32_t clear_no_return; };
struct Iso { float c, s, tx, ty; };
enum { DROPPED = -1, HIT = 0, CLEAR = 1 };

// item 11b: cosine and sine of a pose angle as a fixed sequence of fp32 operations
inline void sincos_fixed(float x, float& sn, float& cs) {
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

// the direction of beam c: host libm at the bearing (c - n / 2) * (angle_max - angle_min) / n
inline void beam_dir(const Params& P, int c, float* d) {
  const float sensor_res = (P.angle_max - P.angle_min) / (float) P.n_beams, half = (float) P.n_beams * 0.5f;
  const float a = ((float) c - half) * sensor_res;
  d[0] = cosf(a); d[1] = sinf(a);
}

// item 17d.1: the class 1 .. 4 of a range, the tests in this order; -> the ray's kind and its length
inline int classify(const Params& P, float r, int* kind, float* len) {
  *kind = DROPPED; *len = 0.0f;
  if (!(r >= P.range_min)) return 1;
  if (r <= P.trace_range) { *kind = HIT; *len = r; return 2; }
  if (r <= P.range_max) { *kind = CLEAR; *len = P.trace_range; return 3; }
  if (P.clear_no_return) { *kind = CLEAR; *len = P.trace_range; }
  return 4;
}

inline float cell_of(float v, float o, float inv) { return floorf((v - o) * inv); }
inline bool in_range(float c) { return c >= -1048576.0f && c < 1048576.0f; }

// items 17d.2-3 for one beam that has a ray by its class: -> true and the four cells, or false (dropped by the cell tests)
inline bool make_ray(const float* dir, float len, const float* pose, const Iso& T, float ox, float oy, float inv, int32_t* r) {
  const float px = len * dir[0], py = len * dir[1];      // ONE product each
  float x = px, y = py, sx = 0.0f, sy = 0.0f;
  if (pose) { x = fmaf(T.c, px, fmaf(-T.s, py, T.tx)); y = fmaf(T.s, px, fmaf(T.c, py, T.ty)); sx = pose[0]; sy = pose[1]; }
  const float fx0 = cell_of(sx, ox, inv), fy0 = cell_of(sy, oy, inv), fx1 = cell_of(x, ox, inv), fy1 = cell_of(y, oy, inv);
  if (!(in_range(fx0) && in_range(fy0) && in_range(fx1) && in_range(fy1))) return false;
  r[0] = (int32_t) fx0; r[1] = (int32_t) fy0; r[2] = (int32_t) fx1; r[3] = (int32_t) fy1;
  const long long ax = llabs((long long) r[2] - r[0]), ay = llabs((long long) r[3] - r[1]);
  return (ax > ay ? ax : ay) <= 32767;
}

inline void add_sat(uint32_t* c) { if (*c != 0xffffffffu) ++*c; }

// item 17d.4: the error-term walk; a HIT ray's last step is a hit, every other step of either kind a miss
inline void walk(const int32_t* r, int kind, int width, int height, uint32_t* H, uint32_t* M) {
  const int dx = r[2] - r[0], dy = r[3] - r[1];
  const int ax = abs(dx), ay = abs(dy), sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
  const bool xm = ax >= ay;      // a tie is x-major
  const int L = xm ? ax : ay, a = xm ? ay : ax;
  int x = r[0], y = r[1];
  long long err = L;
  for (int i = 0; i <= L; ++i) {
    if (x >= 0 && y >= 0 && x < width && y < height) add_sat(((i == L && kind == HIT) ? H : M) + (size_t) y * width + x);
    if (xm) x += sx; else y += sy;
    err += 2ll * a;
    if (L && err >= 2ll * L) { err -= 2ll * L; if (xm) y += sy; else x += sx; }
  }
}
}  // namespace occsref

extern "C" {

// dirs [n_beams][2]
void occsref_dirs(const occsref::Params* P, float* dirs) { for (int c = 0; c < P->n_beams; ++c) occsref::beam_dir(*P, c, dirs + 2 * (size_t) c); }

// ONE scan: cls [n_beams] the class 1 .. 4, kind [n_beams] -1 / 0 / 1 by the class alone, xy [n_beams][2] the sensor-frame end point (0, 0 without a ray)
void occsref_points(const occsref::Params* P, const float* ranges, int32_t* cls, int32_t* kind, float* xy) {
  for (int c = 0; c < P->n_beams; ++c) {
    float d[2], len; int k;
    occsref::beam_dir(*P, c, d);
    cls[c] = occsref::classify(*P, ranges[c], &k, &len); kind[c] = k;
    xy[2 * c] = k == occsref::DROPPED ? 0.0f : len * d[0]; xy[2 * c + 1] = k == occsref::DROPPED ? 0.0f : len * d[1];
  }
}

// ONE scan: rays [n_beams][4] and kind [n_beams] = -1 (no ray, by its class or by the cell tests) / 0 HIT / 1 CLEAR
void occsref_rays(const occsref::Params* P, const float* ranges, const float* pose /* [3] or NULL */, float ox, float oy, float resolution, int32_t* rays,
                  int32_t* kind) {
  const float inv = 1.0f / resolution;
  occsref::Iso T = {1.0f, 0.0f, 0.0f, 0.0f};
  if (pose) { occsref::sincos_fixed(pose[2], T.s, T.c); T.tx = pose[0]; T.ty = pose[1]; }
  for (int c = 0; c < P->n_beams; ++c) {
    float d[2], len; int k; int32_t r[4] = {0, 0, 0, 0};
    occsref::beam_dir(*P, c, d);
    occsref::classify(*P, ranges[c], &k, &len);
    if (k != occsref::DROPPED && !occsref::make_ray(d, len, pose, T, ox, oy, inv, r)) { k = occsref::DROPPED; memset(r, 0, sizeof r); }
    kind[c] = k; memcpy(rays + 4 * (size_t) c, r, sizeof r);
  }
}

// ranges [n_scans][n_beams]; pose [n_scans][3] or NULL; grid [n_scans] or NULL.  hits / misses: [n_grids][height][width], ACCUMULATED into (saturating);
// hit_rays / clear_rays / dropped: [n_grids], set.
void occsref_update(const occsref::Params* P, const float* ranges, int n_scans, const float* pose, const int32_t* grid, int n_grids, float ox, float oy,
                    float resolution, int width, int height, uint32_t* hits, uint32_t* misses, int32_t* hit_rays, int32_t* clear_rays, int32_t* dropped) {
  const float inv = 1.0f / resolution;
  const int nb = P->n_beams;
  float* dirs = (float*) malloc(sizeof(float) * 2 * (size_t) nb);      // the table, once per geometry
  occsref_dirs(P, dirs);
  for (int g = 0; g < n_grids; ++g) { hit_rays[g] = 0; clear_rays[g] = 0; dropped[g] = 0; }
  for (int k = 0; k < n_scans; ++k) {
    const int g = grid ? grid[k] : 0;
    uint32_t* const H = hits + (size_t) g * width * height; uint32_t* const M = misses + (size_t) g * width * height;
    const float* ps = pose ? pose + 3 * (size_t) k : nullptr;
    occsref::Iso T = {1.0f, 0.0f, 0.0f, 0.0f};
    if (ps) { occsref::sincos_fixed(ps[2], T.s, T.c); T.tx = ps[0]; T.ty = ps[1]; }
    for (int c = 0; c < nb; ++c) {
      float len; int kind; int32_t r[4];
      occsref::classify(*P, ranges[(size_t) k * nb + c], &kind, &len);
      if (kind == occsref::DROPPED || !occsref::make_ray(dirs + 2 * (size_t) c, len, ps, T, ox, oy, inv, r)) { ++dropped[g]; continue; }
      ++(kind == occsref::HIT ? hit_rays : clear_rays)[g];
      occsref::walk(r, kind, width, height, H, M);
    }
  }
  free(dirs);
}

}  // extern "C"
