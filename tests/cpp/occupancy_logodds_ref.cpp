// occupancy_logodds_ref.cpp -- the accumulation of a log-odds grid set (PARITY.md section 3, item 17e), restated on the host as plain loops: test
// infrastructure, built as a shared object by tests/occupancy_logodds_cases.py through tests/cpp_build.py.  Written independently of the kernels: scan after
// scan, each ray walked by the closed form of item 17c.3 evaluated afresh at every step (no carried remainder) into a per-scan MARK array (0 nothing,
// 1 miss, 2 hit: the larger mark stays), then one clamped vote per marked cell.  Its input is integer rays with a kind, as occupancy_cases.rays_of and
// occupancy_scan_cases.rays_of make them (both pinned by the CPU suites): the two update calls differ in how a ray comes to be, not in what it adds.
// tests/test_occupancy_logodds_abi.py pins it to occupancy_cases.reference / occupancy_scan_cases.reference run on each scan alone.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace occlref {
enum { DROPPED = -1, HIT = 0, CLEAR = 1 };
struct Params { int32_t l_hit, l_miss, l_min, l_max; };      // lsm2d_logodds_params, field by field

// item 17c.3: step i of the ray, i = 0 .. L, from the closed form
inline void step_cell(const int32_t* r, int i, int* x, int* y) {
  const long long dx = (long long) r[2] - r[0], dy = (long long) r[3] - r[1];
  const long long ax = llabs(dx), ay = llabs(dy);
  const bool xm = ax >= ay;      // a tie is x-major
  const long long L = xm ? ax : ay, a = xm ? ay : ax;
  const long long minor = L ? (2ll * i * a + L) / (2ll * L) : 0;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
  *x = (int) (r[0] + (xm ? sx * (long long) i : sx * minor));
  *y = (int) (r[1] + (xm ? sy * minor : sy * (long long) i));
}

inline void vote(int32_t* value, uint32_t* observed, long long l, const Params& P) {
  long long v = (long long) *value + l;      // 64 bits: an uploaded value may stand anywhere in int32
  if (v < P.l_min) v = P.l_min;
  if (v > P.l_max) v = P.l_max;
  *value = (int32_t) v;
  if (*observed != 0xffffffffu) ++*observed;
}
}  // namespace occlref

extern "C" {

// rays [n][4] and kind [n] (-1 no ray / 0 HIT / 1 CLEAR) of the scans one after the other, scan s holding rays first[s] .. first[s + 1]; grid [n_scans] or
// NULL.  value / observed: [n_grids][height][width], voted on in place, the scans in the order given.
void occlref_update(const occlref::Params* P, const int32_t* rays, const int32_t* kind, const int32_t* first, int n_scans, const int32_t* grid, int n_grids,
                    int width, int height, int32_t* value, uint32_t* observed) {
  const size_t cells = (size_t) width * height;
  uint8_t* mark = (uint8_t*) calloc(cells, 1);
  size_t* marked = (size_t*) malloc(sizeof(size_t) * cells);      // the cells a scan marked, so that a scan costs its rays and not the grid
  for (int s = 0; s < n_scans; ++s) {
    const int g = grid ? grid[s] : 0;
    if (g < 0 || g >= n_grids) continue;
    size_t n_marked = 0;
    for (int k = first[s]; k < first[s + 1]; ++k) {
      if (kind[k] == occlref::DROPPED) continue;
      const int32_t* r = rays + 4 * (size_t) k;
      const long long ax = llabs((long long) r[2] - r[0]), ay = llabs((long long) r[3] - r[1]);
      const int L = (int) (ax > ay ? ax : ay);
      for (int i = 0; i <= L; ++i) {
        int x, y;
        occlref::step_cell(r, i, &x, &y);
        if (x < 0 || y < 0 || x >= width || y >= height) continue;
        const uint8_t m = (i == L && kind[k] == occlref::HIT) ? 2 : 1;
        uint8_t* const c = mark + (size_t) y * width + x;
        if (!*c) marked[n_marked++] = (size_t) y * width + x;
        if (m > *c) *c = m;      // the hit wins
      }
    }
    for (size_t j = 0; j < n_marked; ++j) {      // one vote per marked cell, and the mark array is clean for the next scan
      const size_t c = marked[j];
      occlref::vote(value + g * cells + c, observed + g * cells + c, mark[c] == 2 ? P->l_hit : P->l_miss, *P);
      mark[c] = 0;
    }
  }
  free(marked); free(mark);
}

// lsm2d_occupancy_decay over n cells
void occlref_decay(int32_t* value, const uint32_t* observed, long long n, int32_t amount) {
  for (long long c = 0; c < n; ++c) {
    if (!observed[c]) continue;
    const long long v = value[c];
    if (v > 0) value[c] = (int32_t) (v - amount > 0 ? v - amount : 0);
    else if (v < 0) value[c] = (int32_t) (v + amount < 0 ? v + amount : 0);
  }
}

}  // extern "C"
