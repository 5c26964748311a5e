/*
 * lsm2d_oracle_impl.inc -- precision-generic body of the CPU ORACLE (test infrastructure; PARITY
 * UNPINNED, see lsm2d_oracle.h).  Included twice by lsm2d_oracle.c with
 *   REAL=float  SFX(x)=x##_f  (fp32 mirror: the exact IEEE operation sequence of the HIP kernels)
 *   REAL=double SFX(x)=x##_d  (fp64 truth)
 * No -ffast-math, -ffp-contract=off: every fused multiply-add below is an explicit R_FMA.
 */

/* ---- SE(2) helpers: geometry2d::v2t / t2v (visual_test_correspondence_finder_projective_2d.cpp:71,
 *      octave/solver/geometry_helpers_3d.m:56-60 restricted to rotation about z) ------------- */
typedef struct { REAL c, s, tx, ty; } SFX(iso);

static inline SFX(iso) SFX(v2t)(const REAL v[3]) {
  SFX(iso) T;
  T.c = R_COS(v[2]); T.s = R_SIN(v[2]); T.tx = v[0]; T.ty = v[1];
  return T;
}

static inline REAL SFX(wrap_angle)(REAL a) {
  if (!(fabs((double) a) < 3.0e7)) return (REAL) NAN;      /* not a number, or beyond where 2 pi changes it: the loops below would never end (the device's wrap_angle) */
  while (a > R_PI) a -= R_TWO_PI;
  while (a <= -R_PI) a += R_TWO_PI;
  return a;
}

void SFX(lsmo_compose)(const REAL a[3], const REAL b[3], REAL out[3]) {
  SFX(iso) A = SFX(v2t)(a);
  REAL x = R_FMA(A.c, b[0], R_FMA(-A.s, b[1], A.tx));
  REAL y = R_FMA(A.s, b[0], R_FMA(A.c, b[1], A.ty));
  out[0] = x; out[1] = y; out[2] = SFX(wrap_angle)(a[2] + b[2]);
}

void SFX(lsmo_inverse)(const REAL a[3], REAL out[3]) {
  SFX(iso) A = SFX(v2t)(a);
  /* (R,t)^-1 = (R^T, -R^T t) */
  REAL x = -(R_FMA(A.c, a[0], A.s * a[1]));
  REAL y = -(R_FMA(-A.s, a[0], A.c * a[1]));
  out[0] = x; out[1] = y; out[2] = SFX(wrap_angle)(-a[2]);
}

/* PointNormal2f::transform<Isometry>: coordinates -> R p + t, normal -> R n
 * (use at correspondence_finder_kd_tree_2d.cpp:15-16; SURVEY App. A.1) */
static inline void SFX(xf_point)(const SFX(iso)* T, REAL px, REAL py, REAL* qx, REAL* qy) {
#ifdef LSMO_REFERENCE_PASS      /* Eigen: linear() * p first, then + translation() */
  *qx = (T->c * px + (-T->s) * py) + T->tx;
  *qy = (T->s * px + T->c * py) + T->ty;
#else
  *qx = R_FMA(T->c, px, R_FMA(-T->s, py, T->tx));
  *qy = R_FMA(T->s, px, R_FMA(T->c, py, T->ty));
#endif
}
static inline void SFX(xf_normal)(const SFX(iso)* T, REAL nx, REAL ny, REAL* ox, REAL* oy) {
  *ox = R_FMA(T->c, nx, (-T->s) * ny);
  *oy = R_FMA(T->s, nx, T->c * ny);
}

/* ---- projector ---------------------------------------------------------------------------
 * Restates PointNormal2fProjectorPolar::compute as the reference uses it
 * (correspondence_finder_projective_2d.cpp:40-41,47-48; camera matrix [[1/res, cols/2],[0,1]] at
 * synthetic_scene_generator.cpp:59-66 and raw_data_preprocessor_projective_2d.cpp:83-90).
 * SURVEY App. A.3 / D.1: per point in index order: q = T p; r = |q|; skip unless
 * range_min <= r <= range_max; col = floor(K00*atan2(qy,qx) + K01 [+ col_offset]); skip unless
 * 0 <= col < cols; strict r < depth[col] replaces the cell (first point wins ties). */
typedef struct { int src; REAL depth, x, y, nx, ny; } SFX(cell);

static void SFX(project_cells)(const lsmo_projector* pr, const lsmo_point* cloud, int n,
                               const SFX(iso)* T, SFX(cell)* cells) {
  const int cols = pr->canvas_cols;
  const REAL K00 = (REAL) cols / ((REAL) pr->angle_max - (REAL) pr->angle_min);
  const REAL K01 = (REAL) cols * (REAL) 0.5 + (REAL) pr->col_offset;
  /* ranges clamped to [1e-15, 1e18] m: keeps r*r a normal fp32 number (same clamp in the HIP library) */
  const REAL rmin = (REAL) (pr->range_min > 1e-15f ? pr->range_min : 1e-15f), rmax = (REAL) (pr->range_max < 1e18f ? pr->range_max : 1e18f);
  for (int c = 0; c < cols; ++c) {
    cells[c].src = -1; cells[c].depth = R_MAX;
    cells[c].x = cells[c].y = cells[c].nx = cells[c].ny = 0;
  }
  for (int i = 0; i < n; ++i) {
    REAL qx, qy;
    SFX(xf_point)(T, (REAL) cloud[i].x, (REAL) cloud[i].y, &qx, &qy);
    const REAL r = R_SQRT(R_FMA(qx, qx, qy * qy));
    if (!(r >= rmin && r <= rmax)) continue;
    const REAL th = R_ATAN2(qy, qx);
    const REAL u  = R_FMA(K00, th, K01);
    if (!(u >= 0 && u < (REAL) cols)) continue;
    const int col = (int) R_FLOOR(u);
    if (r < cells[col].depth) {
      cells[col].src = i; cells[col].depth = r;
      cells[col].x = qx; cells[col].y = qy;
      SFX(xf_normal)(T, (REAL) cloud[i].nx, (REAL) cloud[i].ny, &cells[col].nx, &cells[col].ny);
    }
  }
}

int SFX(lsmo_project)(const lsmo_projector* pr, const lsmo_point* cloud, int n, const REAL pose[3],
                      int* out_src, REAL* out_depth, REAL* out_xyn) {
  if (!pr || pr->canvas_cols <= 0 || !(pr->angle_max > pr->angle_min)) return LSMO_BAD_ARGUMENT;
  SFX(cell)* cells = (SFX(cell)*) malloc(sizeof(SFX(cell)) * (size_t) pr->canvas_cols);
  SFX(iso) T = SFX(v2t)(pose);
  SFX(project_cells)(pr, cloud, n, &T, cells);
  for (int c = 0; c < pr->canvas_cols; ++c) {
    out_src[c] = cells[c].src;
    if (out_depth) out_depth[c] = cells[c].depth;
    if (out_xyn) {
      out_xyn[4 * c + 0] = cells[c].x;  out_xyn[4 * c + 1] = cells[c].y;
      out_xyn[4 * c + 2] = cells[c].nx; out_xyn[4 * c + 3] = cells[c].ny;
    }
  }
  free(cells);
  return LSMO_SUCCESS;
}

/* ---- projective finder: correspondence_finder_projective_2d.cpp:18-77 ----------------------
 * fixed projected with the camera at identity (:40-41), moving with camera pose =
 * local_map_in_sensor^-1, i.e. moving points mapped by `pose` (:47-48); lock-step walk over the two
 * canvases (:55-74): skip empty cells (:61), |depth_f - depth_m| > point_distance (:65),
 * transformed-normal dot < normal_cos (:69); emit (fixed src, moving src) in ascending column (:73). */
static int SFX(match_cells_cols)(const lsmo_slice_params* sp, const SFX(cell)* fc, const SFX(cell)* mc,
                                 lsmo_corr* out, int* out_col /* column of every pair, or NULL */) {
  int k = 0;
  const REAL pd = (REAL) sp->point_distance, nc = (REAL) sp->normal_cos;
  for (int c = 0; c < sp->projector.canvas_cols; ++c) {
    if (mc[c].src < 0 || fc[c].src < 0) continue;
    if (R_FABS(fc[c].depth - mc[c].depth) > pd) continue;
    const REAL dot = R_FMA(mc[c].nx, fc[c].nx, mc[c].ny * fc[c].ny);
    if (dot < nc) continue;
    out[k].fixed_idx = fc[c].src; out[k].moving_idx = mc[c].src;
    if (out_col) out_col[k] = c;
    ++k;
  }
  return k;
}
static int SFX(match_cells)(const lsmo_slice_params* sp, const SFX(cell)* fc, const SFX(cell)* mc, lsmo_corr* out) {
  return SFX(match_cells_cols)(sp, fc, mc, out, NULL);
}

int SFX(lsmo_find_projective)(const lsmo_slice_params* sp, const lsmo_point* fixed, int n_fixed,
                              const lsmo_point* moving, int n_moving, const REAL pose[3],
                              lsmo_corr* out) {
  const int cols = sp->projector.canvas_cols;
  if (cols <= 0 || !(sp->projector.angle_max > sp->projector.angle_min)) return LSMO_BAD_ARGUMENT;
  SFX(cell)* fc = (SFX(cell)*) malloc(sizeof(SFX(cell)) * (size_t) cols * 2);
  SFX(cell)* mc = fc + cols;
  const REAL ident[3] = {0, 0, 0};
  SFX(iso) I = SFX(v2t)(ident), T = SFX(v2t)(pose);
  SFX(project_cells)(&sp->projector, fixed, n_fixed, &I, fc);
  SFX(project_cells)(&sp->projector, moving, n_moving, &T, mc);
  int k = SFX(match_cells)(sp, fc, mc, out);
  free(fc);
  return k;
}

/* ---- NN finder: correspondence_finder_kd_tree_2d.cpp:5-38 -----------------------------------
 * per moving point in ascending index (:12): moved = T m (:15-16); nearest fixed point within
 * max_distance (:18-19) else none (:21); gate moved.normal . fixed.normal >= normal_cos (:22);
 * emit (fixed_idx, moving_idx) (:25).  SURVEY App. D.2: the search is EXACT here (upstream
 * KDTree::findNeighbor is believed approximate, App. A.4); ties -> lowest fixed index;
 * "within" = squared distance <= max_distance^2. */
static inline int SFX(nn_gate_emit)(const lsmo_slice_params* sp, const lsmo_point* fixed, int best,
                                    REAL nqx, REAL nqy) {
  if (best < 0) return 0;
  const REAL dot = R_FMA(nqx, (REAL) fixed[best].nx, nqy * (REAL) fixed[best].ny);
  return !(dot < (REAL) sp->normal_cos);
}

int SFX(lsmo_find_nn_brute)(const lsmo_slice_params* sp, const lsmo_point* fixed, int n_fixed,
                            const lsmo_point* moving, int n_moving, const REAL pose[3],
                            lsmo_corr* out) {
  SFX(iso) T = SFX(v2t)(pose);
  const REAL md2 = (REAL) sp->max_distance * (REAL) sp->max_distance;
  int k = 0;
  for (int j = 0; j < n_moving; ++j) {
    REAL qx, qy, nqx, nqy;
    SFX(xf_point)(&T, (REAL) moving[j].x, (REAL) moving[j].y, &qx, &qy);
    SFX(xf_normal)(&T, (REAL) moving[j].nx, (REAL) moving[j].ny, &nqx, &nqy);
    int best = -1; REAL bd = R_MAX;
    for (int i = 0; i < n_fixed; ++i) {
      const REAL dx = (REAL) fixed[i].x - qx, dy = (REAL) fixed[i].y - qy;
      const REAL d2 = R_FMA(dx, dx, dy * dy);
      if (d2 <= md2 && d2 < bd) { bd = d2; best = i; }
    }
    if (SFX(nn_gate_emit)(sp, fixed, best, nqx, nqy)) { out[k].fixed_idx = best; out[k].moving_idx = j; ++k; }
  }
  return k;
}

/* uniform-grid acceleration of the same exact search (cell = max_distance*(1+1e-5), 3x3 cells);
 * points are visited per cell in ascending index so (d2, idx) lexicographic min == brute force */
typedef struct {
  REAL minx, miny, inv_h; int gw, gh; int* start; int* items;
} SFX(grid);

static int SFX(grid_build)(SFX(grid)* g, const lsmo_point* fixed, int n, REAL h) {
  REAL minx = R_MAX, miny = R_MAX, maxx = -R_MAX, maxy = -R_MAX;
  for (int i = 0; i < n; ++i) {
    REAL x = (REAL) fixed[i].x, y = (REAL) fixed[i].y;
    if (x < minx) minx = x; if (x > maxx) maxx = x;
    if (y < miny) miny = y; if (y > maxy) maxy = y;
  }
  if (n == 0) { minx = miny = 0; maxx = maxy = 0; }
  g->minx = minx; g->miny = miny; g->inv_h = (REAL) 1 / h;
  double gw = floor((double) (maxx - minx) * (double) g->inv_h) + 1, gh = floor((double) (maxy - miny) * (double) g->inv_h) + 1;
  if (gw * gh > 64e6) return -1;
  g->gw = (int) gw; g->gh = (int) gh;
  const int nc = g->gw * g->gh;
  g->start = (int*) calloc((size_t) nc + 1, sizeof(int));
  g->items = (int*) malloc(sizeof(int) * (size_t) (n > 0 ? n : 1));
  int* cell_of = (int*) malloc(sizeof(int) * (size_t) (n > 0 ? n : 1));
  for (int i = 0; i < n; ++i) {
    int cx = (int) R_FLOOR(((REAL) fixed[i].x - minx) * g->inv_h);
    int cy = (int) R_FLOOR(((REAL) fixed[i].y - miny) * g->inv_h);
    if (cx < 0) cx = 0; if (cx >= g->gw) cx = g->gw - 1;
    if (cy < 0) cy = 0; if (cy >= g->gh) cy = g->gh - 1;
    cell_of[i] = cy * g->gw + cx;
    g->start[cell_of[i] + 1]++;
  }
  for (int c = 0; c < nc; ++c) g->start[c + 1] += g->start[c];
  int* fill = (int*) malloc(sizeof(int) * (size_t) (nc > 0 ? nc : 1));
  memcpy(fill, g->start, sizeof(int) * (size_t) nc);
  for (int i = 0; i < n; ++i) g->items[fill[cell_of[i]]++] = i;   /* ascending index inside a cell */
  free(fill); free(cell_of);
  return 0;
}
static void SFX(grid_free)(SFX(grid)* g) { free(g->start); free(g->items); }

int SFX(lsmo_find_nn)(const lsmo_slice_params* sp, const lsmo_point* fixed, int n_fixed,
                      const lsmo_point* moving, int n_moving, const REAL pose[3], lsmo_corr* out) {
  if (!(sp->max_distance > 0)) return LSMO_BAD_ARGUMENT;
  SFX(grid) g;
  const REAL h = (REAL) sp->max_distance * (REAL) 1.00001 + (REAL) 1e-30;
  if (SFX(grid_build)(&g, fixed, n_fixed, h) != 0)
    return SFX(lsmo_find_nn_brute)(sp, fixed, n_fixed, moving, n_moving, pose, out);
  SFX(iso) T = SFX(v2t)(pose);
  const REAL md2 = (REAL) sp->max_distance * (REAL) sp->max_distance;
  int k = 0;
  for (int j = 0; j < n_moving; ++j) {
    REAL qx, qy, nqx, nqy;
    SFX(xf_point)(&T, (REAL) moving[j].x, (REAL) moving[j].y, &qx, &qy);
    SFX(xf_normal)(&T, (REAL) moving[j].nx, (REAL) moving[j].ny, &nqx, &nqy);
    const double fx = floor((double) ((qx - g.minx) * g.inv_h)), fy = floor((double) ((qy - g.miny) * g.inv_h));
    int best = -1; REAL bd = R_MAX;
    if (fx >= -1 && fy >= -1 && fx <= g.gw && fy <= g.gh) {
      const int cx = (int) fx, cy = (int) fy;
      for (int yy = cy - 1; yy <= cy + 1; ++yy) {
        if (yy < 0 || yy >= g.gh) continue;
        for (int xx = cx - 1; xx <= cx + 1; ++xx) {
          if (xx < 0 || xx >= g.gw) continue;
          const int c = yy * g.gw + xx;
          for (int t = g.start[c]; t < g.start[c + 1]; ++t) {
            const int i = g.items[t];
            const REAL dx = (REAL) fixed[i].x - qx, dy = (REAL) fixed[i].y - qy;
            const REAL d2 = R_FMA(dx, dx, dy * dy);
            if (d2 <= md2 && (d2 < bd || (d2 == bd && i < best))) { bd = d2; best = i; }
          }
        }
      }
    }
    if (SFX(nn_gate_emit)(sp, fixed, best, nqx, nqy)) { out[k].fixed_idx = best; out[k].moving_idx = j; ++k; }
  }
  SFX(grid_free)(&g);
  return k;
}

/* ---- the KD-tree as upstream is BELIEVED to build and search it (SURVEY App. A.4; ctor and call shape at
 * correspondence_finder_kd_tree_2d.h:36-39, .cpp:18-19,36-37) -- oracle only, LSMO_FINDER_KDTREE_APPROX ------------------
 * build: a node becomes a leaf when it holds fewer than min_leaf_points points or when its extent along both principal axes
 * (half the spread of the projections on the covariance's eigenvectors) is below max_leaf_range; otherwise it is split by the
 * plane through the mean whose normal is the principal eigenvector (largest eigenvalue) -- points with (p - mean).n < 0 go left.
 * search: descend to the ONE leaf on the query's side of every plane (no backtracking => approximate), scan it for the nearest
 * point with squared distance < max_distance^2 (first point wins ties: the stable partition keeps ascending indices); none -> -1
 * (correspondence_finder_kd_tree_2d.cpp:21).  UNVERIFIABLE: the upstream sources are not in the tree. */
typedef struct { int leaf, begin, end, left, right; REAL mx, my, nx, ny; } SFX(kdnode);
typedef struct { SFX(kdnode)* nodes; int n_nodes, cap; int* idx; int* tmp; REAL max_leaf_range; int min_leaf_points; } SFX(kdtree);

static int SFX(kd_build_node)(SFX(kdtree)* t, const lsmo_point* pts, int begin, int end) {
  if (t->n_nodes == t->cap) { t->cap *= 2; t->nodes = (SFX(kdnode)*) realloc(t->nodes, sizeof(SFX(kdnode)) * (size_t) t->cap); }
  const int me = t->n_nodes++;
  SFX(kdnode) nd; nd.leaf = 1; nd.begin = begin; nd.end = end; nd.left = nd.right = -1; nd.mx = nd.my = nd.nx = nd.ny = 0;
  const int n = end - begin;
  if (n >= t->min_leaf_points && n >= 2) {
    REAL mx = 0, my = 0;
    for (int k = begin; k < end; ++k) { mx += (REAL) pts[t->idx[k]].x; my += (REAL) pts[t->idx[k]].y; }
    mx /= (REAL) n; my /= (REAL) n;
    REAL sxx = 0, sxy = 0, syy = 0;
    for (int k = begin; k < end; ++k) {
      const REAL dx = (REAL) pts[t->idx[k]].x - mx, dy = (REAL) pts[t->idx[k]].y - my;
      sxx += dx * dx; sxy += dx * dy; syy += dy * dy;
    }
    /* principal eigenvector of [[sxx, sxy], [sxy, syy]] (closed form) */
    const REAL tr = sxx + syy, df = sxx - syy;
    const REAL disc = R_SQRT(df * df + (REAL) 4 * sxy * sxy);
    const REAL l1 = (tr + disc) / (REAL) 2;
    REAL vx, vy;
    if (R_FABS(sxy) > (REAL) 0) { vx = l1 - syy; vy = sxy; } else if (sxx >= syy) { vx = 1; vy = 0; } else { vx = 0; vy = 1; }
    const REAL vn = R_SQRT(vx * vx + vy * vy);
    if (vn > (REAL) 0) {
      vx /= vn; vy /= vn;
      REAL lo1 = R_MAX, hi1 = -R_MAX, lo2 = R_MAX, hi2 = -R_MAX;
      for (int k = begin; k < end; ++k) {
        const REAL dx = (REAL) pts[t->idx[k]].x - mx, dy = (REAL) pts[t->idx[k]].y - my;
        const REAL a = dx * vx + dy * vy, b = -dx * vy + dy * vx;
        if (a < lo1) lo1 = a; if (a > hi1) hi1 = a; if (b < lo2) lo2 = b; if (b > hi2) hi2 = b;
      }
      const REAL e1 = (hi1 - lo1) / (REAL) 2, e2 = (hi2 - lo2) / (REAL) 2;
      if ((e1 > e2 ? e1 : e2) >= t->max_leaf_range) {
        /* stable partition: left = (p - mean).v < 0 */
        int nl = 0, nr = 0;
        for (int k = begin; k < end; ++k) {
          const REAL dx = (REAL) pts[t->idx[k]].x - mx, dy = (REAL) pts[t->idx[k]].y - my;
          if (dx * vx + dy * vy < (REAL) 0) t->idx[begin + nl++] = t->idx[k]; else t->tmp[nr++] = t->idx[k];
        }
        for (int k = 0; k < nr; ++k) t->idx[begin + nl + k] = t->tmp[k];
        if (nl > 0 && nr > 0) {
          nd.leaf = 0; nd.mx = mx; nd.my = my; nd.nx = vx; nd.ny = vy;
          t->nodes[me] = nd;
          const int l = SFX(kd_build_node)(t, pts, begin, begin + nl);
          const int r = SFX(kd_build_node)(t, pts, begin + nl, end);
          t->nodes[me].left = l; t->nodes[me].right = r;
          return me;
        }
      }
    }
  }
  t->nodes[me] = nd;
  return me;
}
static void SFX(kd_build)(SFX(kdtree)* t, const lsmo_point* pts, int n, REAL max_leaf_range, int min_leaf_points) {
  t->cap = 64; t->n_nodes = 0; t->nodes = (SFX(kdnode)*) malloc(sizeof(SFX(kdnode)) * (size_t) t->cap);
  t->idx = (int*) malloc(sizeof(int) * (size_t) (n > 0 ? n : 1)); t->tmp = (int*) malloc(sizeof(int) * (size_t) (n > 0 ? n : 1));
  t->max_leaf_range = max_leaf_range; t->min_leaf_points = min_leaf_points;
  for (int i = 0; i < n; ++i) t->idx[i] = i;
  SFX(kd_build_node)(t, pts, 0, n);
}
static void SFX(kd_free)(SFX(kdtree)* t) { free(t->nodes); free(t->idx); free(t->tmp); }
static int SFX(kd_find)(const SFX(kdtree)* t, const lsmo_point* pts, REAL qx, REAL qy, REAL md2) {
  int k = 0;
  while (!t->nodes[k].leaf) {
    const SFX(kdnode)* nd = &t->nodes[k];
    k = ((qx - nd->mx) * nd->nx + (qy - nd->my) * nd->ny < (REAL) 0) ? nd->left : nd->right;
  }
  int best = -1; REAL bd = md2;
  for (int j = t->nodes[k].begin; j < t->nodes[k].end; ++j) {
    const int i = t->idx[j];
    const REAL dx = (REAL) pts[i].x - qx, dy = (REAL) pts[i].y - qy;
    const REAL d2 = R_FMA(dx, dx, dy * dy);
    if (d2 < bd) { bd = d2; best = i; }
  }
  return best;
}
static int SFX(kd_find_all)(const SFX(kdtree)* t, const lsmo_slice_params* sp, const lsmo_point* fixed,
                            const lsmo_point* moving, int n_moving, const REAL pose[3], lsmo_corr* out) {
  SFX(iso) T = SFX(v2t)(pose);
  const REAL md2 = (REAL) sp->max_distance * (REAL) sp->max_distance;
  int k = 0;
  for (int j = 0; j < n_moving; ++j) {
    REAL qx, qy, nqx, nqy;
    SFX(xf_point)(&T, (REAL) moving[j].x, (REAL) moving[j].y, &qx, &qy);
    SFX(xf_normal)(&T, (REAL) moving[j].nx, (REAL) moving[j].ny, &nqx, &nqy);
    const int best = SFX(kd_find)(t, fixed, qx, qy, md2);
    if (SFX(nn_gate_emit)(sp, fixed, best, nqx, nqy)) { out[k].fixed_idx = best; out[k].moving_idx = j; ++k; }
  }
  return k;
}
int SFX(lsmo_find_kdtree)(const lsmo_slice_params* sp, const lsmo_point* fixed, int n_fixed,
                          const lsmo_point* moving, int n_moving, const REAL pose[3], lsmo_corr* out) {
  if (!(sp->max_distance > 0)) return LSMO_BAD_ARGUMENT;
  SFX(kdtree) t;
  SFX(kd_build)(&t, fixed, n_fixed, (REAL) (sp->kd_max_leaf_range > 0 ? sp->kd_max_leaf_range : 1e-2f), sp->kd_min_leaf_points > 0 ? sp->kd_min_leaf_points : 20);
  const int k = SFX(kd_find_all)(&t, sp, fixed, moving, n_moving, pose, out);
  SFX(kd_free)(&t);
  return k;
}

/* ---- distance-map finder: correspondence_finder_nn_2d.cpp:10-97 ----------------------------------------
 * reset(): inv_res = 1/resolution, mds_px = (max_distance*inv_res)^2, padding = (int)(sqrt(mds_px) + 75.5) (:20-25);
 * bounding box of the fixed cloud with the upper bounds INITIALISED TO numeric_limits<float>::min() (smallest positive,
 * :31-32, SURVEY App. C.4); rows = ceil(bb.x*inv_res + padding), cols likewise (:44-46); goal f sits at pixel
 * trunc((p_f - lowest)*inv_res + padding/2) (.h:38-41); the path search fills, for every pixel within mds_px (squared
 * pixel distance) of a goal pixel, the index of a nearest goal (:92-94).
 * compute(): moved = T m; pixel = trunc(pointInMapCoords(moved)); outside -> skip (:67-69); parent -1 -> skip (:71-73);
 * normal gate (:75); emit (parent, m) in ascending m (:79).
 * ASSUMED (upstream PathMatrixDistanceSearch is not in the tree): the parent is the EXACT nearest goal pixel in squared
 * integer pixel distance, ties -> lowest goal index, several goals in one pixel -> lowest index; negative pixel
 * coordinates are rejected (the reference casts to size_t, which wraps and fails inside()). */
typedef struct { int rows, cols; REAL lx, ly, inv_res, half_pad; int* parent; } SFX(distmap);

static int SFX(distmap_build)(SFX(distmap)* dm, const lsmo_slice_params* sp, const lsmo_point* fixed, int n) {
  if (!(sp->resolution > 0) || sp->max_distance < 0) return LSMO_BAD_ARGUMENT;
  const REAL inv_res = (REAL) 1 / (REAL) sp->resolution;
  const REAL mdm = (REAL) sp->max_distance;
  const REAL mds_px = mdm * mdm * inv_res * inv_res;
  const int padding = (int) (R_SQRT(mds_px) + (REAL) 75.5);
  REAL lx = R_MAX, ly = R_MAX, ux = R_TINY, uy = R_TINY;
  for (int i = 0; i < n; ++i) {
    const REAL px = (REAL) fixed[i].x, py = (REAL) fixed[i].y;
    if (px < lx) lx = px; if (py < ly) ly = py; if (px > ux) ux = px; if (py > uy) uy = py;
  }
  if (n == 0) { lx = ly = 0; }
  const double rows = ceil((double) ((ux - lx) * inv_res + (REAL) padding)), cols = ceil((double) ((uy - ly) * inv_res + (REAL) padding));
  if (!(rows >= 1 && cols >= 1) || rows * cols > 400e6) return LSMO_BAD_ARGUMENT;
  dm->rows = (int) rows; dm->cols = (int) cols; dm->lx = lx; dm->ly = ly; dm->inv_res = inv_res; dm->half_pad = (REAL) padding * (REAL) 0.5;
  const size_t npx = (size_t) dm->rows * (size_t) dm->cols;
  dm->parent = (int*) malloc(sizeof(int) * npx);
  int* best_d = (int*) malloc(sizeof(int) * npx);
  for (size_t i = 0; i < npx; ++i) { dm->parent[i] = -1; best_d[i] = 0x7fffffff; }
  const int R = (int) floor(sqrt((double) mds_px));
  for (int f = 0; f < n; ++f) {
    const REAL gx = ((REAL) fixed[f].x - lx) * inv_res + dm->half_pad, gy = ((REAL) fixed[f].y - ly) * inv_res + dm->half_pad;
    if (!(gx >= 0 && gy >= 0 && gx < (REAL) dm->rows && gy < (REAL) dm->cols)) continue;
    const int gr = (int) gx, gc = (int) gy;
    for (int dr = -R; dr <= R; ++dr) {
      const int r = gr + dr; if (r < 0 || r >= dm->rows) continue;
      for (int dc = -R; dc <= R; ++dc) {
        const int c = gc + dc; if (c < 0 || c >= dm->cols) continue;
        const int d2 = dr * dr + dc * dc;
        if ((REAL) d2 > mds_px) continue;
        const size_t k = (size_t) r * (size_t) dm->cols + (size_t) c;
        if (d2 < best_d[k] || (d2 == best_d[k] && f < dm->parent[k])) { best_d[k] = d2; dm->parent[k] = f; }
      }
    }
  }
  free(best_d);
  return LSMO_SUCCESS;
}

static inline int SFX(distmap_lookup)(const SFX(distmap)* dm, REAL qx, REAL qy) {
  const REAL gx = (qx - dm->lx) * dm->inv_res + dm->half_pad, gy = (qy - dm->ly) * dm->inv_res + dm->half_pad;
  if (!(gx >= 0 && gy >= 0 && gx < (REAL) dm->rows && gy < (REAL) dm->cols)) return -1;
  return dm->parent[(size_t) (int) gx * (size_t) dm->cols + (size_t) (int) gy];
}

static int SFX(distmap_find)(const SFX(distmap)* dm, const lsmo_slice_params* sp, const lsmo_point* fixed,
                             const lsmo_point* moving, int n_moving, const REAL pose[3], lsmo_corr* out) {
  SFX(iso) T = SFX(v2t)(pose);
  int k = 0;
  for (int j = 0; j < n_moving; ++j) {
    REAL qx, qy, nqx, nqy;
    SFX(xf_point)(&T, (REAL) moving[j].x, (REAL) moving[j].y, &qx, &qy);
    SFX(xf_normal)(&T, (REAL) moving[j].nx, (REAL) moving[j].ny, &nqx, &nqy);
    const int best = SFX(distmap_lookup)(dm, qx, qy);
    if (SFX(nn_gate_emit)(sp, fixed, best, nqx, nqy)) { out[k].fixed_idx = best; out[k].moving_idx = j; ++k; }
  }
  return k;
}

int SFX(lsmo_find_distmap)(const lsmo_slice_params* sp, const lsmo_point* fixed, int n_fixed,
                           const lsmo_point* moving, int n_moving, const REAL pose[3], lsmo_corr* out) {
  SFX(distmap) dm;
  const int rc = SFX(distmap_build)(&dm, sp, fixed, n_fixed);
  if (rc != LSMO_SUCCESS) return rc;
  const int k = SFX(distmap_find)(&dm, sp, fixed, moving, n_moving, pose, out);
  free(dm.parent);
  return k;
}

/* ---- factor: SE2Plane2PlaneErrorFactor restated from octave/solver/nicp_post.m:4-26 ----------
 * (directErrorAndJacobian, 3-D -> rotation about z, translation in x,y; right-multiplicative
 * increment X <- X*v2t(dx), nicp_post.m:92-97).  SURVEY App. D.3:
 *   q = R p_m + t, n_q = R n_m
 *   e = [ n_f.(q - p_f) ; n_q - n_f ]
 *   J = [[ (R^T n_f)^T , n_f.(R J2 p_m) ], [ 0 , R J2 n_m ]],  J2 p = (-p_y, p_x)
 * Information matrix = I3 (App. A.5).  RobustifierCauchy (App. A.7): w = 1/(1+chi2/tau), inlier <=>
 * chi2 < tau, kernelised chi = tau ln(1+chi2/tau). */
static inline void SFX(err_jac)(const SFX(iso)* T, const lsmo_point* f, const lsmo_point* m,
                                REAL e[3], REAL J0[3], REAL d[2]) {
  REAL qx, qy, nqx, nqy;
  const REAL pmx = (REAL) m->x, pmy = (REAL) m->y;
  SFX(xf_point)(T, pmx, pmy, &qx, &qy);
  SFX(xf_normal)(T, (REAL) m->nx, (REAL) m->ny, &nqx, &nqy);
  const REAL nfx = (REAL) f->nx, nfy = (REAL) f->ny;
  const REAL dx = qx - (REAL) f->x, dy = qy - (REAL) f->y;
  e[0] = R_FMA(nfx, dx, nfy * dy);
  e[1] = nqx - nfx;
  e[2] = nqy - nfy;
  /* a = R^T n_f */
  J0[0] = R_FMA(T->c, nfx, T->s * nfy);
  J0[1] = R_FMA(-T->s, nfx, T->c * nfy);
  /* g = n_f . (R J2 p_m) = (R^T n_f) . (J2 p_m) = a0*(-pmy) + a1*pmx */
  J0[2] = R_FMA(J0[1], pmx, -(J0[0] * pmy));
  /* d = R J2 n_m = J2 (R n_m) */
  d[0] = -nqy; d[1] = nqx;
}

/* inl_only: an iteration of the aligner's inlier-only runs (lsmo_aligner_params.enable_inlier_only_runs): a pair that is not an inlier under the
 * slice's robustifier gets weight 0, an inlier weight 1; the statistics are the regular iteration's */
static int SFX(linearize_core)(const lsmo_slice_params* sp, const lsmo_point* fixed, const lsmo_point* moving,
                               const lsmo_corr* corr, int n_corr, const REAL pose[3],
                               REAL H[9], REAL b[3], lsmo_iter_stats* st, int inl_only) {
  SFX(iso) T = SFX(v2t)(pose);
  REAL h00 = 0, h01 = 0, h02 = 0, h11 = 0, h12 = 0, h22 = 0, b0 = 0, b1 = 0, b2 = 0;
  REAL chi_in = 0, chi_out = 0; int n_in = 0, n_out = 0;
  const int cauchy = sp->robustifier == LSMO_ROBUST_CAUCHY;
  const REAL tau = (REAL) sp->chi_threshold;
  for (int k = 0; k < n_corr; ++k) {
    REAL e[3], a[3], d[2];
    SFX(err_jac)(&T, &fixed[corr[k].fixed_idx], &moving[corr[k].moving_idx], e, a, d);
    const REAL chi = R_FMA(e[0], e[0], R_FMA(e[1], e[1], e[2] * e[2]));
    REAL w = 1;
    if (cauchy) {
      const REAL q = chi / tau;
      w = (REAL) 1 / ((REAL) 1 + q);
      if (chi < tau) { ++n_in; chi_in += chi; }
      else { ++n_out; chi_out += tau * R_LOG((REAL) 1 + q); }
      if (inl_only) w = chi < tau ? (REAL) 1 : (REAL) 0;
    } else { ++n_in; chi_in += chi; }
    const REAL dd = R_FMA(d[0], d[0], d[1] * d[1]);
    const REAL de = R_FMA(d[0], e[1], d[1] * e[2]);
    const REAL wa0 = w * a[0], wa1 = w * a[1], wa2 = w * a[2];
    h00 = R_FMA(wa0, a[0], h00); h01 = R_FMA(wa0, a[1], h01); h02 = R_FMA(wa0, a[2], h02);
    h11 = R_FMA(wa1, a[1], h11); h12 = R_FMA(wa1, a[2], h12);
    h22 = R_FMA(wa2, a[2], h22); h22 = R_FMA(w, dd, h22);
    b0 = R_FMA(wa0, e[0], b0); b1 = R_FMA(wa1, e[0], b1);
    b2 = R_FMA(wa2, e[0], b2); b2 = R_FMA(w, de, b2);
  }
  H[0] = h00; H[1] = h01; H[2] = h02; H[3] = h01; H[4] = h11; H[5] = h12; H[6] = h02; H[7] = h12; H[8] = h22;
  b[0] = b0; b[1] = b1; b[2] = b2;
  if (st) {
    st->n_corr = n_corr; st->n_in = n_in; st->n_out = n_out; st->chi_in = (float) chi_in; st->chi_out = (float) chi_out;
    unsigned long long dg = 0;
    for (int k = 0; k < n_corr; ++k) dg += lsmo_pair_hash(0u, (unsigned) corr[k].fixed_idx, (unsigned) corr[k].moving_idx);
    st->pair_digest_lo = (unsigned) dg; st->pair_digest_hi = (unsigned) (dg >> 32);
  }
  return LSMO_SUCCESS;
}
int SFX(lsmo_linearize)(const lsmo_slice_params* sp, const lsmo_point* fixed, const lsmo_point* moving,
                        const lsmo_corr* corr, int n_corr, const REAL pose[3],
                        REAL H[9], REAL b[3], lsmo_iter_stats* st) {
  return SFX(linearize_core)(sp, fixed, moving, corr, n_corr, pose, H, b, st, 0);
}

#ifdef LSMO_FLOAT_PASS
/* ---- the same sums in the device's order (lsmo_aligner_params.device_order) ------------------------------------------
 * srrg2_laser_slam_2d_amd/csrc: k_align / k_split_finish give the pair of slot t (column or moving index, see lsmo_align) to
 * thread t mod 512; a thread adds its pairs in ascending slot (accumulate_pair: the operations of the loop body above, with the
 * inlier / outlier sums written branch-free, i.e. adding +0); the 64 partial sums of a wave are combined by wave_sum63 -- an
 * inclusive scan inside each row of 16 lanes (row_shr 1, 2, 4, 8), lane 15 -> row 1 and lane 47 -> row 3 (row_bcast:15), lane 31 ->
 * rows 2, 3 (row_bcast:31), total in lane 63 -- and the 8 wave totals are added in wave order (block_reduce_gather_wave0). */
#define LSMO_DEV_BLOCK 512
static float lsmo_wave_sum63(const float* x) {
  float v[64], t[64];
  for (int i = 0; i < 64; ++i) v[i] = x[i];
  for (int sh = 1; sh <= 8; sh <<= 1) {
    for (int i = 0; i < 64; ++i) t[i] = v[i] + ((i & 15) >= sh ? v[i - sh] : 0.0f);
    for (int i = 0; i < 64; ++i) v[i] = t[i];
  }
  for (int i = 0; i < 64; ++i) t[i] = v[i] + (((i >> 4) & 1) ? v[(i & ~15) - 1] : 0.0f);      /* row_bcast:15, rows 1 and 3 */
  for (int i = 0; i < 64; ++i) v[i] = t[i];
  for (int i = 0; i < 64; ++i) t[i] = v[i] + ((i >> 5) ? v[31] : 0.0f);                       /* row_bcast:31, rows 2 and 3 */
  return t[63];
}

/* Generic over the launch shape: `threads` threads in workgroups of `block` (multiples of 64); pair k goes to thread slot[k] mod
 * threads (slot == NULL: k); a workgroup's wave totals are added in wave order starting from 0, the workgroup totals in workgroup
 * order starting from 0.  The aligner kernels are one workgroup of 512; lsm2d_linearize launches ceil(n / 256) <= 1024 workgroups
 * of 256 (k_linearize_partial / k_linearize_final). */
static int linearize_device_order_core(const lsmo_slice_params* sp, const lsmo_point* fixed, const lsmo_point* moving,
                                       const lsmo_corr* corr, const int* slot, int n_corr, const float pose[3], int threads, int block,
                                       float H[9], float b[3], lsmo_iter_stats* st, int inl_only) {
  enum { NQ = 11 };
  if (threads < 64 || block < 64 || threads % block || block % 64) return LSMO_BAD_ARGUMENT;
  float (*acc)[NQ] = (float (*)[NQ]) calloc((size_t) threads, sizeof *acc);      /* h00 h01 h02 h11 h12 h22 b0 b1 b2 chi_in chi_out */
  int n_in = 0, n_out = 0;
  SFX(iso) T = SFX(v2t)(pose);
  const int cauchy = sp->robustifier == LSMO_ROBUST_CAUCHY;
  const float tau = sp->chi_threshold;
  for (int k = 0; k < n_corr; ++k) {
    float* A = acc[(slot ? slot[k] : k) % threads];
    float e[3], a[3], d[2];
    SFX(err_jac)(&T, &fixed[corr[k].fixed_idx], &moving[corr[k].moving_idx], e, a, d);
    const float chi = fmaf(e[0], e[0], fmaf(e[1], e[1], e[2] * e[2]));
    float w = 1.0f, kern = 0.0f; int inlier = 1;
    if (cauchy) { const float q = chi / tau; w = 1.0f / (1.0f + q); inlier = chi < tau; kern = tau * lsmo_logf_fixed(1.0f + q); if (inl_only) w = inlier ? 1.0f : 0.0f; }
    n_in += inlier; n_out += !inlier;
    A[9] += inlier ? chi : 0.0f;
    A[10] += inlier ? 0.0f : kern;
    const float dd = fmaf(d[0], d[0], d[1] * d[1]);
    const float de = fmaf(d[0], e[1], d[1] * e[2]);
    const float wa0 = w * a[0], wa1 = w * a[1], wa2 = w * a[2];
    A[0] = fmaf(wa0, a[0], A[0]); A[1] = fmaf(wa0, a[1], A[1]); A[2] = fmaf(wa0, a[2], A[2]);
    A[3] = fmaf(wa1, a[1], A[3]); A[4] = fmaf(wa1, a[2], A[4]);
    A[5] = fmaf(wa2, a[2], A[5]); A[5] = fmaf(w, dd, A[5]);
    A[6] = fmaf(wa0, e[0], A[6]); A[7] = fmaf(wa1, e[0], A[7]);
    A[8] = fmaf(wa2, e[0], A[8]); A[8] = fmaf(w, de, A[8]);
  }
  float tot[NQ];
  for (int q = 0; q < NQ; ++q) {
    float v = 0.0f;
    for (int wg = 0; wg < threads / block; ++wg) {
      float vb = 0.0f;
      for (int wv = 0; wv < block / 64; ++wv) {
        float lane[64];
        for (int l = 0; l < 64; ++l) lane[l] = acc[wg * block + wv * 64 + l][q];
        vb += lsmo_wave_sum63(lane);
      }
      v += vb;
    }
    tot[q] = v;
  }
  free(acc);
  H[0] = tot[0]; H[1] = tot[1]; H[2] = tot[2]; H[3] = tot[1]; H[4] = tot[3]; H[5] = tot[4]; H[6] = tot[2]; H[7] = tot[4]; H[8] = tot[5];
  b[0] = tot[6]; b[1] = tot[7]; b[2] = tot[8];
  if (st) {
    st->n_corr = n_corr; st->n_in = n_in; st->n_out = n_out; st->chi_in = tot[9]; st->chi_out = tot[10];
    unsigned long long dg = 0;
    for (int k = 0; k < n_corr; ++k) dg += lsmo_pair_hash(0u, (unsigned) corr[k].fixed_idx, (unsigned) corr[k].moving_idx);
    st->pair_digest_lo = (unsigned) dg; st->pair_digest_hi = (unsigned) (dg >> 32);
  }
  return LSMO_SUCCESS;
}
int lsmo_linearize_device_order_f(const lsmo_slice_params* sp, const lsmo_point* fixed, const lsmo_point* moving,
                                  const lsmo_corr* corr, const int* slot, int n_corr, const float pose[3], int threads, int block,
                                  float H[9], float b[3], lsmo_iter_stats* st) {
  return linearize_device_order_core(sp, fixed, moving, corr, slot, n_corr, pose, threads, block, H, b, st, 0);
}
#endif /* LSMO_FLOAT_PASS */

/* ---- step: nicp_post.m:92-97 (dx = -H\b; T = T*v2t(dx)); GN damping (MULTI.json:254-259) -----
 * The 3x3 solve runs in fp64 in both instantiations (the reference hands the block to Cholmod,
 * which is double precision -- SURVEY section 8 row a9); LDL^T, pivot <= 0 or non-finite -> SingularH. */
int SFX(lsmo_solve_update)(const REAL H[9], const REAL b[3], REAL damping, REAL pose[3], REAL dx_out[3]) {
  const double a00 = (double) H[0] + (double) damping, a01 = H[1], a02 = H[2];
  const double a11 = (double) H[4] + (double) damping, a12 = H[5], a22 = (double) H[8] + (double) damping;
  const double r0 = -(double) b[0], r1 = -(double) b[1], r2 = -(double) b[2];
  const double d0 = a00;
  if (!(d0 > 0) || !isfinite(d0)) return LSMO_SINGULAR_H;
  const double l10 = a01 / d0, l20 = a02 / d0;
  const double d1 = a11 - l10 * a01;
  if (!(d1 > 0) || !isfinite(d1)) return LSMO_SINGULAR_H;
  const double l21 = (a12 - l20 * a01) / d1;
  const double d2 = a22 - l20 * a02 - l21 * l21 * d1;
  if (!(d2 > 0) || !isfinite(d2)) return LSMO_SINGULAR_H;
  const double y0 = r0, y1 = r1 - l10 * y0, y2 = r2 - l20 * y0 - l21 * y1;
  const double z2 = y2 / d2;
  const double z1 = y1 / d1 - l21 * z2;
  const double z0 = y0 / d0 - l10 * z1 - l20 * z2;
  if (!isfinite(z0) || !isfinite(z1) || !isfinite(z2)) return LSMO_SINGULAR_H;
  const REAL dx = (REAL) z0, dy = (REAL) z1, dth = (REAL) z2;
  SFX(iso) T = SFX(v2t)(pose);
  pose[0] = R_FMA(T.c, dx, R_FMA(-T.s, dy, T.tx));
  pose[1] = R_FMA(T.s, dx, R_FMA(T.c, dy, T.ty));
  pose[2] = SFX(wrap_angle)(pose[2] + dth);
  if (dx_out) { dx_out[0] = dx; dx_out[1] = dy; dx_out[2] = dth; }
  return LSMO_SUCCESS;
}

/* ---- aligner: MultiAligner2D::compute restated (SURVEY section 3.2, App. D.5) ------------------
 * for it < max_iterations: every laser slice runs its finder at X_eff = S^-1 X, then its factor;
 * slices with #pairs <= min_num_correspondences are skipped, all skipped -> NotEnoughCorrespondences;
 * H, b, statistics are SUMMED over slices (+ the odometry prior) before ONE solve and right update;
 * after the loop: n_in(last) < min_num_inliers -> NotEnoughInliers; information matrix = last H. */
int SFX(lsmo_align_pairs)(const lsmo_aligner_params* ap, int n_slices, const lsmo_slice_params* sp,
                          const lsmo_point* const* fixed, const int* n_fixed,
                          const lsmo_point* const* moving, const int* n_moving,
                          const REAL x0[3], REAL x_out[3], REAL H_out[9],
                          lsmo_iter_stats* stats, int* iterations_done, lsmo_corr* const* out_pairs, int* out_n_pairs) {
  if (!ap || n_slices < 1 || ap->max_iterations < 0) return LSMO_BAD_ARGUMENT;
  REAL X[3] = {x0[0], x0[1], x0[2]};
  int status = LSMO_SUCCESS, it = 0;
  lsmo_iter_stats last; memset(&last, 0, sizeof last);
  float chi_prev = 0.0f;
  /* the regular loop is phase 0; enable_inlier_only_runs may add phase 1 (see lsmo_aligner_params) */
  int phase = 0, phase_start = 0, phase_end = ap->max_iterations;
  const int it_cap = ap->enable_inlier_only_runs ? 2 * ap->max_iterations : ap->max_iterations;
  if (out_n_pairs) for (int s = 0; s < n_slices; ++s) out_n_pairs[s] = 0;
  for (int i = 0; i < 9; ++i) H_out[i] = 0;

  /* per-slice scratch: correspondence buffers + cached fixed canvas (projected once:
   * correspondence_finder_projective_2d.cpp:37-44) */
  lsmo_corr** corr = (lsmo_corr**) calloc((size_t) n_slices, sizeof(lsmo_corr*));
  int** slot = (int**) calloc((size_t) n_slices, sizeof(int*));      /* device_order: which thread of the device's workgroup sums a pair */
  SFX(cell)** fcan = (SFX(cell)**) calloc((size_t) n_slices, sizeof(SFX(cell)*));
  SFX(cell)** mcan = (SFX(cell)**) calloc((size_t) n_slices, sizeof(SFX(cell)*));
  SFX(distmap)* dmap = (SFX(distmap)*) calloc((size_t) n_slices, sizeof(SFX(distmap)));
  SFX(kdtree)* kdt = (SFX(kdtree)*) calloc((size_t) n_slices, sizeof(SFX(kdtree)));
  int* have_kd = (int*) calloc((size_t) n_slices, sizeof(int));
  const REAL ident[3] = {0, 0, 0};
  SFX(iso) I = SFX(v2t)(ident);
  for (int s = 0; s < n_slices; ++s) {
    int cap = n_moving[s];
    if (sp[s].finder == LSMO_FINDER_PROJECTIVE) {
      const int cols = sp[s].projector.canvas_cols;
      if (cols <= 0 || !(sp[s].projector.angle_max > sp[s].projector.angle_min)) { status = LSMO_BAD_ARGUMENT; goto done; }
      cap = cols;
      fcan[s] = (SFX(cell)*) malloc(sizeof(SFX(cell)) * (size_t) cols);
      mcan[s] = (SFX(cell)*) malloc(sizeof(SFX(cell)) * (size_t) cols);
      SFX(project_cells)(&sp[s].projector, fixed[s], n_fixed[s], &I, fcan[s]);
    } else if (sp[s].finder == LSMO_FINDER_DISTMAP) {
      if (SFX(distmap_build)(&dmap[s], &sp[s], fixed[s], n_fixed[s]) != LSMO_SUCCESS) { status = LSMO_BAD_ARGUMENT; goto done; }
    } else if (sp[s].finder == LSMO_FINDER_KDTREE_APPROX) {
      if (!(sp[s].max_distance > 0)) { status = LSMO_BAD_ARGUMENT; goto done; }
      SFX(kd_build)(&kdt[s], fixed[s], n_fixed[s], (REAL) (sp[s].kd_max_leaf_range > 0 ? sp[s].kd_max_leaf_range : 1e-2f),
                    sp[s].kd_min_leaf_points > 0 ? sp[s].kd_min_leaf_points : 20);
      have_kd[s] = 1;
    } else if (sp[s].finder != LSMO_FINDER_NN) { status = LSMO_BAD_ARGUMENT; goto done; }
    corr[s] = (lsmo_corr*) malloc(sizeof(lsmo_corr) * (size_t) (cap > 0 ? cap : 1));
    slot[s] = (int*) malloc(sizeof(int) * (size_t) (cap > 0 ? cap : 1));
  }

  for (it = 0; it < it_cap; ++it) {
    REAL H[9] = {0}, b[3] = {0};
    lsmo_iter_stats tot; memset(&tot, 0, sizeof tot);
    unsigned long long dig = 0;
    int active = 0;
    for (int s = 0; s < n_slices; ++s) {
      /* X_eff = S^-1 * X */
      REAL S[3] = {(REAL) sp[s].sensor_in_robot[0], (REAL) sp[s].sensor_in_robot[1], (REAL) sp[s].sensor_in_robot[2]};
      REAL Xe[3];
      if (S[0] == 0 && S[1] == 0 && S[2] == 0) { Xe[0] = X[0]; Xe[1] = X[1]; Xe[2] = X[2]; }
      else { REAL Si[3]; SFX(lsmo_inverse)(S, Si); SFX(lsmo_compose)(Si, X, Xe); }
      int n = 0;
      if (sp[s].finder == LSMO_FINDER_PROJECTIVE) {
        SFX(iso) T = SFX(v2t)(Xe);
        SFX(project_cells)(&sp[s].projector, moving[s], n_moving[s], &T, mcan[s]);
        n = SFX(match_cells_cols)(&sp[s], fcan[s], mcan[s], corr[s], slot[s]);               /* slot = column */
      } else if (sp[s].finder == LSMO_FINDER_DISTMAP) {
        n = SFX(distmap_find)(&dmap[s], &sp[s], fixed[s], moving[s], n_moving[s], Xe, corr[s]);
      } else if (sp[s].finder == LSMO_FINDER_KDTREE_APPROX) {
        n = SFX(kd_find_all)(&kdt[s], &sp[s], fixed[s], moving[s], n_moving[s], Xe, corr[s]);
      } else {
        n = SFX(lsmo_find_nn)(&sp[s], fixed[s], n_fixed[s], moving[s], n_moving[s], Xe, corr[s]);
        if (n < 0) { status = LSMO_BAD_ARGUMENT; goto done; }
      }
      tot.n_corr += n;
      for (int k = 0; k < n; ++k) dig += lsmo_pair_hash((unsigned) s, (unsigned) corr[s][k].fixed_idx, (unsigned) corr[s][k].moving_idx);
      if (out_pairs && out_n_pairs) {      /* what the slice's correspondence vector holds after this iteration (the last one started wins) */
        SFX(iso) Tk = SFX(v2t)(Xe);
        const int filter = ap->keep_only_inlier_correspondences && sp[s].robustifier == LSMO_ROBUST_CAUCHY;
        int m = 0;
        for (int k = 0; k < n; ++k) {
          if (filter) {
            REAL e[3], a[3], d[2];
            SFX(err_jac)(&Tk, &fixed[s][corr[s][k].fixed_idx], &moving[s][corr[s][k].moving_idx], e, a, d);
            const REAL chi = R_FMA(e[0], e[0], R_FMA(e[1], e[1], e[2] * e[2]));
            if (!(chi < (REAL) sp[s].chi_threshold)) continue;
          }
          out_pairs[s][m++] = corr[s][k];
        }
        out_n_pairs[s] = m;
      }
      if (n <= sp[s].min_num_correspondences) continue;
      ++active;
      REAL Hs[9], bs[3]; lsmo_iter_stats st;
#ifdef LSMO_FLOAT_PASS
      if (ap->device_order) {
        if (sp[s].finder != LSMO_FINDER_PROJECTIVE) {
          /* point-query finders: moving point j is matched by thread j mod 512 -- or, when the fixed cloud is at least four times
           * the moving one (the NN finder's cooperative search, four lanes per query), by thread 4 * (j mod 128) */
          const int coop = sp[s].finder == LSMO_FINDER_NN && (long long) n_fixed[s] >= 4ll * n_moving[s];
          for (int k = 0; k < n; ++k) slot[s][k] = coop ? 4 * (corr[s][k].moving_idx % 128) : corr[s][k].moving_idx % LSMO_DEV_BLOCK;
        }
        linearize_device_order_core(&sp[s], fixed[s], moving[s], corr[s], slot[s], n, Xe, LSMO_DEV_BLOCK, LSMO_DEV_BLOCK, Hs, bs, &st, phase);
      } else
#endif
      SFX(linearize_core)(&sp[s], fixed[s], moving[s], corr[s], n, Xe, Hs, bs, &st, phase);
      for (int i = 0; i < 9; ++i) H[i] += Hs[i];
      for (int i = 0; i < 3; ++i) b[i] += bs[i];
      tot.n_in += st.n_in; tot.n_out += st.n_out; tot.chi_in += st.chi_in; tot.chi_out += st.chi_out;
    }
    tot.pair_digest_lo = (unsigned) dig; tot.pair_digest_hi = (unsigned) (dig >> 32);
    if (!active) { status = LSMO_NOT_ENOUGH_CORRESPONDENCES; if (stats) stats[it] = tot; last = tot; ++it; break; }
    if (ap->has_prior) {
      /* SE2 prior: e = t2v(Z^-1 X); right-perturbation Jacobian J = blkdiag(R_e, 1) */
      REAL Z[3] = {(REAL) ap->prior_z[0], (REAL) ap->prior_z[1], (REAL) ap->prior_z[2]}, Zi[3], E[3];
      SFX(lsmo_inverse)(Z, Zi); SFX(lsmo_compose)(Zi, X, E);
      const REAL c = R_COS(E[2]), s_ = R_SIN(E[2]);
      const REAL Jp[9] = {c, -s_, 0, s_, c, 0, 0, 0, 1};
      REAL OJ[9], Oe[3];
      for (int r = 0; r < 3; ++r) {
        Oe[r] = 0;
        for (int k = 0; k < 3; ++k) Oe[r] += (REAL) ap->prior_omega[3 * r + k] * E[k];
        for (int cc = 0; cc < 3; ++cc) {
          OJ[3 * r + cc] = 0;
          for (int k = 0; k < 3; ++k) OJ[3 * r + cc] += (REAL) ap->prior_omega[3 * r + k] * Jp[3 * k + cc];
        }
      }
      for (int r = 0; r < 3; ++r) {
        for (int cc = 0; cc < 3; ++cc) { REAL a = 0; for (int k = 0; k < 3; ++k) a += Jp[3 * k + r] * OJ[3 * k + cc]; H[3 * r + cc] += a; }
        REAL a = 0; for (int k = 0; k < 3; ++k) a += Jp[3 * k + r] * Oe[k]; b[r] += a;
      }
    }
    for (int i = 0; i < 9; ++i) H_out[i] = H[i];
    if (stats) stats[it] = tot;
    last = tot;
    const int rc = SFX(lsmo_solve_update)(H, b, (REAL) ap->damping, X, NULL);
    if (rc != LSMO_SUCCESS) { status = rc; ++it; break; }
    int phase_over = it + 1 >= phase_end;
    if (ap->termination_chi_epsilon > 0) {        /* see lsmo_aligner_params.termination_chi_epsilon (the sums are the statistics' fp32 values); afresh in every phase */
      const float chi_now = tot.chi_in + tot.chi_out;
      if (it > phase_start && fabsf(chi_prev - chi_now) < ap->termination_chi_epsilon * chi_now) phase_over = 1;
      chi_prev = chi_now;
    }
    if (phase_over) {
      if (ap->enable_inlier_only_runs && phase == 0 && tot.n_in >= ap->min_num_inliers) { phase = 1; phase_start = it + 1; phase_end = it + 1 + ap->max_iterations; }
      else { ++it; break; }
    }
  }
  if (status == LSMO_SUCCESS && ap->max_iterations > 0 && last.n_in < ap->min_num_inliers) status = LSMO_NOT_ENOUGH_INLIERS;
done:
  for (int s = 0; s < n_slices; ++s) { free(corr[s]); free(slot[s]); free(fcan[s]); free(mcan[s]); free(dmap[s].parent); if (have_kd[s]) SFX(kd_free)(&kdt[s]); }
  free(corr); free(slot); free(fcan); free(mcan); free(dmap); free(kdt); free(have_kd);
  x_out[0] = X[0]; x_out[1] = X[1]; x_out[2] = X[2];
  if (iterations_done) *iterations_done = it;
  return status;
}
int SFX(lsmo_align)(const lsmo_aligner_params* ap, int n_slices, const lsmo_slice_params* sp,
                    const lsmo_point* const* fixed, const int* n_fixed,
                    const lsmo_point* const* moving, const int* n_moving,
                    const REAL x0[3], REAL x_out[3], REAL H_out[9],
                    lsmo_iter_stats* stats, int* iterations_done) {
  return SFX(lsmo_align_pairs)(ap, n_slices, sp, fixed, n_fixed, moving, n_moving, x0, x_out, H_out, stats, iterations_done, NULL, NULL);
}

/* ---- scene clipper: mapping/scene_clipper_projective_2d.cpp:11-65 ---------------------------------
 * sensor_in_local_map = robot_in_local_map * sensor_in_robot (:29); the full scene is projected with the
 * camera at that pose (:31-32); every filled cell's TRANSFORMED point (in the sensor frame), in ascending
 * column, becomes a clipped point (:53-59, voxelize_resolution <= 0 branch); the clipped cloud is then moved
 * to the robot frame by sensor_in_robot unless that is the identity (:61-63).  Returns the number of points. */
int SFX(lsmo_clip_scene)(const lsmo_projector* pr, const lsmo_point* scene, int n_scene,
                         const REAL robot_in_local_map[3], const REAL sensor_in_robot[3],
                         lsmo_point* out /* capacity canvas_cols */, int* out_src /* capacity canvas_cols or NULL */) {
  if (!pr || pr->canvas_cols <= 0 || !(pr->angle_max > pr->angle_min)) return LSMO_BAD_ARGUMENT;
  const int cols = pr->canvas_cols;
  REAL cam[3], cam_inv[3];
  SFX(lsmo_compose)(robot_in_local_map, sensor_in_robot, cam);
  SFX(lsmo_inverse)(cam, cam_inv);
  SFX(iso) T = SFX(v2t)(cam_inv);
  SFX(cell)* cells = (SFX(cell)*) malloc(sizeof(SFX(cell)) * (size_t) cols);
  SFX(project_cells)(pr, scene, n_scene, &T, cells);
  const int ident = sensor_in_robot[0] == 0 && sensor_in_robot[1] == 0 && sensor_in_robot[2] == 0;
  SFX(iso) S = SFX(v2t)(sensor_in_robot);
  int k = 0;
  for (int c = 0; c < cols; ++c) {
    if (cells[c].src < 0) continue;
    REAL x = cells[c].x, y = cells[c].y, nx = cells[c].nx, ny = cells[c].ny;
    if (!ident) {
      REAL tx, ty, tnx, tny;
      SFX(xf_point)(&S, x, y, &tx, &ty); SFX(xf_normal)(&S, nx, ny, &tnx, &tny);
      x = tx; y = ty; nx = tnx; ny = tny;
    }
    out[k].x = (float) x; out[k].y = (float) y; out[k].nx = (float) nx; out[k].ny = (float) ny;
    if (out_src) out_src[k] = cells[c].src;
    ++k;
  }
  free(cells);
  return k;
}

/* ---- merger: mapping/merger_projective_2d.cpp:9-100 ---------------------------------------------------
 * camera at measurement_in_scene for BOTH projections (:19-25): the scene as it is, the measurement after
 * being moved into the scene frame (:22-23).  Column by column (:39-95): a measurement cell deeper than
 * 0.9*range_max is dropped (:46-48); no scene point in the column -> append the measurement point (:56-61);
 * |dr| < merge_threshold -> scene point = normalised average (:71-76); measurement behind -> replace
 * (:79-83); scene behind -> append (:86-87).  `scene` must have room for n_scene + canvas_cols points.
 * PointNormal2f += / *= act on coordinates and normal, normalize() renormalises the normal
 * (SURVEY.md App. A.1).  Returns the new scene size; counts[3] = {new, merged, replaced}. */
int SFX(lsmo_merge_scene)(const lsmo_projector* pr, lsmo_point* scene, int n_scene, const lsmo_point* meas, int n_meas,
                          const REAL measurement_in_scene[3], REAL merge_threshold, int counts[3]) {
  if (!pr || pr->canvas_cols <= 0 || !(pr->angle_max > pr->angle_min)) return LSMO_BAD_ARGUMENT;
  const int cols = pr->canvas_cols;
  REAL cam_inv[3];
  SFX(lsmo_inverse)(measurement_in_scene, cam_inv);
  SFX(iso) Tinv = SFX(v2t)(cam_inv), M = SFX(v2t)(measurement_in_scene);
  lsmo_point* tm = (lsmo_point*) malloc(sizeof(lsmo_point) * (size_t) (n_meas > 0 ? n_meas : 1));
  for (int i = 0; i < n_meas; ++i) {
    REAL x, y, nx, ny;
    SFX(xf_point)(&M, (REAL) meas[i].x, (REAL) meas[i].y, &x, &y);
    SFX(xf_normal)(&M, (REAL) meas[i].nx, (REAL) meas[i].ny, &nx, &ny);
    tm[i].x = (float) x; tm[i].y = (float) y; tm[i].nx = (float) nx; tm[i].ny = (float) ny;
  }
  SFX(cell)* sc = (SFX(cell)*) malloc(sizeof(SFX(cell)) * (size_t) cols * 2);
  SFX(cell)* mc = sc + cols;
  SFX(project_cells)(pr, scene, n_scene, &Tinv, sc);
  SFX(project_cells)(pr, tm, n_meas, &Tinv, mc);
  const REAL far_limit = (REAL) 0.9f * (REAL) pr->range_max;
  int size = n_scene, n_new = 0, n_merged = 0, n_replaced = 0;
  for (int c = 0; c < cols; ++c) {
    if (mc[c].depth > far_limit) mc[c].src = -1;
    if (mc[c].src < 0) continue;
    const lsmo_point mp = tm[mc[c].src];
    if (sc[c].src < 0) { scene[size++] = mp; ++n_new; continue; }
    lsmo_point* sp = &scene[sc[c].src];
    const REAL dr = mc[c].depth - sc[c].depth;
    if (R_FABS(dr) < merge_threshold) {
      const float x = (sp->x + mp.x) * 0.5f, y = (sp->y + mp.y) * 0.5f;
      const float nx = (sp->nx + mp.nx) * 0.5f, ny = (sp->ny + mp.ny) * 0.5f;
      const float nn = sqrtf(fmaf(nx, nx, ny * ny));
      sp->x = x; sp->y = y;
      if (nn > 0.0f) { sp->nx = nx / nn; sp->ny = ny / nn; } else { sp->nx = nx; sp->ny = ny; }
      ++n_merged; continue;
    }
    if (dr > 0) { *sp = mp; ++n_replaced; continue; }
    scene[size++] = mp;
  }
  free(sc); free(tm);
  if (counts) { counts[0] = n_new; counts[1] = n_merged; counts[2] = n_replaced; }
  return size;
}
