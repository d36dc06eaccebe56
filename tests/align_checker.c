/*
 * tests/align_checker.c -- CPU restatement of the global alignment, with the dense colour term optional (DESIGN.md sections 4e "Global alignment"
 * and 4f "The colour term of the global alignment"; scannet_amd/csrc/align.hip and align_colour.hip are the GPU side).
 *
 * K keyframes (u16 depth, RGB8 colour or none, camera-to-world poses) and P directed pairs.  Each frame becomes a vertex map, a normal map and, with
 * pictures, a map of {intensity, gx, gy} at one level; each pair gives 31 numbers, reduced in the kernel's order; the host loop drops thin pairs, keeps
 * the frames connected to the fixed frame, assembles and solves by Cholesky on the first 29 values, and updates the poses.  The rules themselves are
 * tests/solver_rules.h's; what is here is the alignment's own: its arguments, its maps and its host loop, sf_align_pairs and sf_align_spread.
 * The pictures may be NULL: no colour rows are formed, values 29 and 30 are 0 and the first 29 are the depth term's, as they are at colour_weight 0.
 */
#include "solver_rules.h"

#define AL_MAX_FRAMES 256
#define AL_MAX_PAIRS 4096

/* sf_align_params */
typedef struct al_params {
  int32_t level, down_width, down_height, max_iters;
  float dist_thres, normal_thres, depth_min, depth_max, early_out;
  int32_t min_pair_correspondences, fixed_frame;
  float pair_max_dist, pair_max_angle, max_translation, max_rotation;
  float colour_weight, colour_thres, colour_gradient_min;
  int32_t reserved[6];
} al_params;

/* sf_align_result */
typedef struct al_result {
  int32_t status, iterations, pairs_used, frames_unconnected, frames_rejected, reserved0;
  int64_t correspondences;
  float rms_first, rms_last;
  int64_t colour_correspondences;
  float colour_rms_first, colour_rms_last;
  int32_t reserved[2];
} al_result;

/* the level the parameters choose on a W x H integration image and its camera; -1: none */
static int pick_level(const sr_frame* fr, const al_params* a, cam_t* c) {
  int l = a->level;
  if (l < 0 || l > 3) return -1;
  if ((a->down_width == 0) != (a->down_height == 0) || a->down_width < 0 || a->down_height < 0) return -1;
  if (a->down_width > 0) {
    l = -1;
    for (int k = 0; k < 4 && l < 0; k++)
      if ((fr->W >> k) == a->down_width && (fr->H >> k) == a->down_height) l = k;
    if (l < 0) return -1;
  }
  return level_cam(fr, l, c) ? l : -1;
}

static int check_args(int64_t K, const int32_t* pairs, int64_t P, const al_params* a, const uint8_t* rgb) {
  if (a->max_iters < 1 || a->max_iters > 100) return -1;
  if (!isfinite(a->dist_thres) || !(a->dist_thres > 0.0f)) return -1;
  if (!(a->normal_thres >= -1.0f && a->normal_thres <= 1.0f)) return -1;
  if (!isfinite(a->depth_min) || !isfinite(a->depth_max) || a->depth_min < 0.0f || a->depth_max < a->depth_min) return -1;
  if (!isfinite(a->early_out) || !(a->early_out >= 0.0f)) return -1;
  if (a->min_pair_correspondences < 1) return -1;
  if (!isfinite(a->max_translation) || !(a->max_translation > 0.0f) || !isfinite(a->max_rotation) || !(a->max_rotation > 0.0f)) return -1;
  if (!colour_args_ok(rgb != NULL, a->colour_weight, a->colour_thres, a->colour_gradient_min)) return -1;
  if (K < 2 || K > AL_MAX_FRAMES) return -1;
  if (a->fixed_frame < 0 || a->fixed_frame >= K) return -1;
  if (P < 1 || P > AL_MAX_PAIRS) return -1;
  for (int64_t p = 0; p < P; p++) {
    const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
    if (i < 0 || j < 0 || i >= K || j >= K || i == j) return -1;
  }
  return 0;
}

typedef struct {
  int K, npx;
  cam_t cam;
  f3 *v, *n;   /* [K][npx]; x = -inf: invalid */
  f3* ph;      /* [K][npx] {I, gx, gy}; NULL: no colour pictures */
} maps_t;

/* one frame's vertex and normal map at level l: the pre-pass rule, l reductions, the solver's own depth gate */
static void frame_maps(const sr_frame* fr, const uint16_t* depth, int l, const cam_t* c, float dmin, float dmax, f3* vmap, f3* nmap) {
  float* d = prepass_depth(fr, depth);
  for (int k = 0; k < l; k++) {
    float* e = down4(d, fr->W >> k, fr->H >> k);
    free(d);
    d = e;
  }
  for (int i = 0; i < c->W * c->H; i++)
    if (!(d[i] >= dmin && d[i] <= dmax)) d[i] = -INFINITY;
  vertex_normal_maps(c, d, vmap, nmap);
  free(d);
}

/* one frame's {I, gx, gy} at level l from its RGB8 picture */
static void frame_photo(const sr_frame* fr, const uint8_t* rgb, int l, const cam_t* c, f3* pmap) {
  float* d = prepass_intensity(fr, rgb);
  for (int k = 0; k < l; k++) {
    float* e = photo_down(d, fr->W >> k, fr->H >> k);
    free(d);
    d = e;
  }
  photo_map(c, d, pmap);
  free(d);
}

static int maps_build(maps_t* m, const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, int K, const al_params* a) {
  memset(m, 0, sizeof(*m));
  const int l = pick_level(fr, a, &m->cam);
  if (l < 0) return -1;
  const int own = a->depth_min == 0.0f && a->depth_max == 0.0f;
  const float dmin = own ? fr->depth_min : a->depth_min, dmax = own ? fr->depth_max : a->depth_max;
  m->K = K;
  m->npx = m->cam.W * m->cam.H;
  m->v = (f3*)malloc(sizeof(f3) * (size_t)K * m->npx);
  m->n = (f3*)malloc(sizeof(f3) * (size_t)K * m->npx);
  for (int k = 0; k < K; k++)
    frame_maps(fr, depth + (size_t)k * fr->in_w * fr->in_h, l, &m->cam, dmin, dmax, m->v + (size_t)k * m->npx, m->n + (size_t)k * m->npx);
  if (rgb) {
    const size_t cpx = fr->color_w > 0 ? (size_t)fr->color_w * fr->color_h : (size_t)fr->W * fr->H;
    m->ph = (f3*)malloc(sizeof(f3) * (size_t)K * m->npx);
    for (int k = 0; k < K; k++) frame_photo(fr, rgb + 3 * cpx * k, l, &m->cam, m->ph + (size_t)k * m->npx);
  }
  return 0;
}
static void maps_free(maps_t* m) {
  free(m->v);
  free(m->n);
  free(m->ph);
}

/* one source pixel's 31 values for the pair (i, j); 1 when it is a (depth) correspondence.  rc, Jc (may be NULL): the colour row, when acc[30] is 1 */
static int pixel_row(const maps_t* m, int i, int j, int px, const float* Ti, const float* Tj, const float* M, const al_params* a, float* acc, float* rc_out,
                     float* Jc_out) {
  const cam_t* c = &m->cam;
  const f3 v = m->v[(size_t)i * m->npx + px], nc = m->n[(size_t)i * m->npx + px];
  if (!(v.z > 0.0f && nc.x > -INFINITY)) return 0;
  const f3 p = xf(Ti, v), n = rot(Ti, nc), pc = xf(M, v);
  int ux, uy;
  if (!project_nearest(c, pc, &ux, &uy)) return 0;
  const size_t t = (size_t)j * m->npx + (size_t)(uy * c->W + ux);
  const f3 vj = m->v[t], nj = m->n[t];
  if (!(vj.z > 0.0f && nj.x > -INFINITY)) return 0;
  if (!plane_row(p, n, xf(Tj, vj), rot(Tj, nj), a->dist_thres, a->normal_thres, acc)) return 0;
  float rc, Jc[6];
  if (m->ph && colour_row(m->ph[(size_t)i * m->npx + px].x, m->ph + (size_t)j * m->npx, c, pc, p, Tj, a->colour_thres, a->colour_gradient_min, &rc, Jc)) {
    add_colour_row(acc, a->colour_weight, rc, Jc);
    if (rc_out) { *rc_out = rc; memcpy(Jc_out, Jc, sizeof(Jc)); }
  }
  return 1;
}

/* the P systems at the poses T (K x 12 doubles) */
static void systems_at(const maps_t* m, const double* T, const uint8_t* valid, const int32_t* pairs, int P, const al_params* a, double* sys) {
  const int nb = (m->npx + 255) / 256;
  static float lane[256][SR_NSYS];
  for (int p = 0; p < P; p++) {
    double* tot = sys + (size_t)p * SR_NSYS;
    for (int k = 0; k < SR_NSYS; k++) tot[k] = 0.0;
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    if (!valid[i] || !valid[j]) continue;
    float Ti[12], Tj[12], M[12];
    for (int k = 0; k < 12; k++) { Ti[k] = (float)T[12 * i + k]; Tj[k] = (float)T[12 * j + k]; }
    compose_ref(T + 12 * j, T + 12 * i, M);
    for (int b = 0; b < nb; b++) {
      memset(lane, 0, sizeof(lane));
      for (int tid = 0; tid < 256; tid++) {
        const int px = b * 256 + tid;
        if (px < m->npx) pixel_row(m, i, j, px, Ti, Tj, M, a, lane[tid], NULL, NULL);
      }
      reduce_block(lane, tot);
    }
  }
}

static int uf_find(int* parent, int k) {
  while (parent[k] != k) k = parent[k];
  return k;
}

/* The P per-pair systems at the given poses, 31 doubles each (the library's sf_fuser_align_system and sf_fuser_align_rgbd_system).  rgb: K pictures
 * or NULL.  -1: an argument the library refuses. */
int al_system(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, const float* poses, const int32_t* pairs, int64_t P, const al_params* a,
              double* sys) {
  if (check_args(K, pairs, P, a, rgb) != 0) return -1;
  maps_t m;
  if (maps_build(&m, fr, depth, rgb, (int)K, a) != 0) return -1;
  double* T = (double*)calloc((size_t)K * 12, sizeof(double));
  uint8_t* valid = (uint8_t*)calloc((size_t)K, 1);
  for (int k = 0; k < K; k++) {
    valid[k] = (uint8_t)finite12(poses + 16 * k);
    for (int i = 0; i < 12 && valid[k]; i++) T[12 * k + i] = poses[16 * k + i];
  }
  systems_at(&m, T, valid, pairs, (int)P, a, sys);
  free(T);
  free(valid);
  maps_free(&m);
  return 0;
}

/* The maps of frame k at the solver's level for the tests: vmap npx x 3 floats, pmap npx x 3 floats {I, gx, gy}; cam_out: W, H as floats, fx, fy, mx, my */
int al_maps(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, int64_t k, const al_params* a, float* vmap, float* pmap, float* cam_out) {
  maps_t m;
  if (!rgb || k < 0 || k >= K || maps_build(&m, fr, depth, rgb, (int)K, a) != 0) return -1;
  memcpy(vmap, m.v + (size_t)k * m.npx, sizeof(f3) * m.npx);
  memcpy(pmap, m.ph + (size_t)k * m.npx, sizeof(f3) * m.npx);
  cam_out[0] = (float)m.cam.W; cam_out[1] = (float)m.cam.H; cam_out[2] = m.cam.fx; cam_out[3] = m.cam.fy; cam_out[4] = m.cam.mx; cam_out[5] = m.cam.my;
  maps_free(&m);
  return 0;
}

/* The colour rows of pair (i, j) at the given poses for the tests: rows npx x 8 floats {has a colour row, r_c, J_c[6]}, zeros elsewhere */
int al_rows(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, const float* poses, int32_t i, int32_t j, const al_params* a, float* rows) {
  maps_t m;
  if (!rgb || i < 0 || j < 0 || i >= K || j >= K || maps_build(&m, fr, depth, rgb, (int)K, a) != 0) return -1;
  double Td[2][12];
  float Ti[12], Tj[12], M[12];
  for (int k = 0; k < 12; k++) { Td[0][k] = Ti[k] = poses[16 * i + k]; Td[1][k] = Tj[k] = poses[16 * j + k]; }
  compose_ref(Td[1], Td[0], M);
  memset(rows, 0, sizeof(float) * 8 * m.npx);
  for (int px = 0; px < m.npx; px++) {
    float acc[SR_NSYS] = {0};
    float* o = rows + 8 * (size_t)px;
    if (pixel_row(&m, i, j, px, Ti, Tj, M, a, acc, o + 1, o + 2)) o[0] = acc[30];
  }
  maps_free(&m);
  return 0;
}

/* The whole alignment (sf_fuser_align and sf_fuser_align_rgbd).  -1: an argument the library refuses. */
int al_align(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, const float* poses_in, const int32_t* pairs, int64_t P, const al_params* a,
             float* poses_out, al_result* res) {
  if (check_args(K, pairs, P, a, rgb) != 0) return -1;
  maps_t m;
  if (maps_build(&m, fr, depth, rgb, (int)K, a) != 0) return -1;
  al_result r;
  memset(&r, 0, sizeof(r));
  memcpy(poses_out, poses_in, sizeof(float) * 16 * (size_t)K);
  double* T0 = (double*)calloc((size_t)K * 12, sizeof(double));
  double* T = (double*)calloc((size_t)K * 12, sizeof(double));
  double* sys = (double*)calloc((size_t)P * SR_NSYS, sizeof(double));
  uint8_t* valid = (uint8_t*)calloc((size_t)K, 1);
  uint8_t* kept = (uint8_t*)calloc((size_t)P, 1);
  uint8_t* conn = (uint8_t*)calloc((size_t)K, 1);
  int* parent = (int*)calloc((size_t)K, sizeof(int));
  int* slot = (int*)calloc((size_t)K, sizeof(int));
  for (int k = 0; k < K; k++) {
    valid[k] = (uint8_t)finite12(poses_in + 16 * k);
    for (int i = 0; i < 12 && valid[k]; i++) T0[12 * k + i] = T[12 * k + i] = poses_in[16 * k + i];
  }
  const int fixed = a->fixed_frame;
  for (int it = 0; it < a->max_iters; it++) {
    systems_at(&m, T, valid, pairs, (int)P, a, sys);
    /* pairs with enough correspondences; the frames they connect to the fixed frame */
    for (int k = 0; k < K; k++) parent[k] = k;
    for (int p = 0; p < P; p++) {
      const int i = pairs[2 * p], j = pairs[2 * p + 1];
      kept[p] = valid[i] && valid[j] && sys[(size_t)p * SR_NSYS + 28] >= (double)a->min_pair_correspondences;
      if (!kept[p]) continue;
      const int ra = uf_find(parent, i), rb = uf_find(parent, j);
      if (ra < rb) parent[rb] = ra;
      else if (rb < ra) parent[ra] = rb;
    }
    const int rf = uf_find(parent, fixed);
    int n = 0, nconn = 0;
    for (int k = 0; k < K; k++) {
      conn[k] = valid[k] && uf_find(parent, k) == rf;
      slot[k] = -1;
      if (conn[k]) {
        nconn++;
        if (k != fixed) slot[k] = n++;
      }
    }
    if (!valid[fixed] || nconn < 2) { r.status = 2; break; }
    const int N = 6 * n;
    double* A = (double*)calloc((size_t)N * N, sizeof(double));
    double* b = (double*)calloc((size_t)N, sizeof(double));
    double* xi = (double*)calloc((size_t)N, sizeof(double));
    int used = 0;
    double corr = 0.0, r2 = 0.0, ccorr = 0.0, cr2 = 0.0;
    for (int p = 0; p < P; p++) {
      const int i = pairs[2 * p], j = pairs[2 * p + 1];
      if (!kept[p] || !conn[i]) continue;
      const double* s = sys + (size_t)p * SR_NSYS;
      double H[6][6];
      unpack_sym6(s, H);
      const int si = slot[i], sj = slot[j];
      for (int u = 0; u < 6; u++) {
        for (int v = 0; v < 6; v++) {
          if (si >= 0) A[(size_t)(6 * si + u) * N + 6 * si + v] += H[u][v];
          if (sj >= 0) A[(size_t)(6 * sj + u) * N + 6 * sj + v] += H[u][v];
          if (si >= 0 && sj >= 0) {
            A[(size_t)(6 * si + u) * N + 6 * sj + v] -= H[u][v];
            A[(size_t)(6 * sj + u) * N + 6 * si + v] -= H[u][v];
          }
        }
        if (si >= 0) b[6 * si + u] += s[21 + u];
        if (sj >= 0) b[6 * sj + u] -= s[21 + u];
      }
      used++;
      r2 += s[27];
      corr += s[28];
      cr2 += s[29];
      ccorr += s[30];
    }
    r.pairs_used = used;
    r.correspondences = (int64_t)corr;
    r.rms_last = rms_of(r2, corr);
    r.colour_correspondences = (int64_t)ccorr;
    r.colour_rms_last = rms_of(cr2, ccorr);
    if (it == 0) { r.rms_first = r.rms_last; r.colour_rms_first = r.colour_rms_last; }
    const int ok = cholesky_solve(A, b, N, xi);
    if (ok)
      for (int k = 0; k < K; k++)
        if (slot[k] >= 0) apply_update(xi + 6 * slot[k], T + 12 * k);
    const double mx = ok ? max_abs(xi, N) : 0.0;
    free(A);
    free(b);
    free(xi);
    if (!ok) { r.status = 1; break; }
    r.iterations++;
    if (mx < (double)a->early_out) break;
  }
  for (int k = 0; k < K; k++) {
    if (!valid[k] || k == fixed) continue;
    if (!conn[k]) { r.frames_unconnected++; continue; }
    if (r.status != 0) continue;
    if (!motion_ok(T0 + 12 * k, T + 12 * k, a->max_translation, a->max_rotation)) { r.frames_rejected++; continue; }
    write_pose(T + 12 * k, poses_out + 16 * k);
  }
  *res = r;
  free(T0); free(T); free(sys); free(valid); free(kept); free(conn); free(parent); free(slot);
  maps_free(&m);
  return 0;
}

/* sf_align_pairs */
int al_pairs(const float* poses, int64_t K, const al_params* a, int32_t* pairs_out, uint64_t capacity, uint64_t* n_out) {
  uint64_t n = 0;
  for (int64_t i = 0; i < K; i++) {
    const float* pa = poses + 16 * i;
    if (!finite12(pa)) continue;
    for (int64_t j = i + 1; j < K; j++) {
      const float* pb = poses + 16 * j;
      if (!finite12(pb)) continue;
      int take = j == i + 1;
      if (!take) {
        double d2 = 0.0, M[3][3];
        for (int r = 0; r < 3; r++) {
          const double dt = (double)pb[4 * r + 3] - (double)pa[4 * r + 3];
          d2 += dt * dt;
        }
        for (int u = 0; u < 3; u++)
          for (int v = 0; v < 3; v++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)pa[4 * k + u] * (double)pb[4 * k + v];
            M[u][v] = s;
          }
        const double x = M[2][1] - M[1][2], y = M[0][2] - M[2][0], z = M[1][0] - M[0][1];
        const double sn = 0.5 * sqrt((x * x + y * y) + z * z);
        const double cs = 0.5 * (((M[0][0] + M[1][1]) + M[2][2]) - 1.0);
        take = sqrt(d2) <= (double)a->pair_max_dist && atan2(sn, cs) <= (double)a->pair_max_angle;
      }
      if (!take) continue;
      if (n < capacity) { pairs_out[2 * n] = (int32_t)i; pairs_out[2 * n + 1] = (int32_t)j; }
      n++;
      if (n < capacity) { pairs_out[2 * n] = (int32_t)j; pairs_out[2 * n + 1] = (int32_t)i; }
      n++;
    }
  }
  *n_out = n;
  return 0;
}

/* sf_align_spread */
int al_spread(const float* poses, uint64_t n, const uint64_t* keyframes, uint64_t K, const float* new_key_poses, float* poses_out) {
  for (uint64_t f = 0; f < n; f++) {
    const float* Tf = poses + 16 * f;
    /* the usable keyframe at or before f nearest to it; else the first usable one */
    int64_t k = -1, first = -1;
    int is_key = 0;
    for (uint64_t q = 0; q < K; q++) {
      if (!finite12(poses + 16 * keyframes[q]) || !finite12(new_key_poses + 16 * q)) continue;
      if (first < 0) first = (int64_t)q;
      if (keyframes[q] <= f) { k = (int64_t)q; is_key = keyframes[q] == f; }
    }
    if (k < 0) k = first;
    float* o = poses_out + 16 * f;
    if (is_key) { memcpy(o, new_key_poses + 16 * k, 16 * sizeof(float)); continue; }
    if (k < 0 || !finite12(Tf)) { memmove(o, Tf, 16 * sizeof(float)); continue; }
    const float* To = poses + 16 * keyframes[k];
    const float* Tn = new_key_poses + 16 * k;
    double Tod[12], inv[9], D[12];
    for (int q = 0; q < 12; q++) Tod[q] = To[q];
    inverse3(Tod, inv);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) D[4 * r + c] = ((double)Tn[4 * r] * inv[c] + (double)Tn[4 * r + 1] * inv[3 + c]) + (double)Tn[4 * r + 2] * inv[6 + c];
      D[4 * r + 3] = (double)Tn[4 * r + 3] - ((D[4 * r] * (double)To[3] + D[4 * r + 1] * (double)To[7]) + D[4 * r + 2] * (double)To[11]);
    }
    float out[16];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) {
        double s = (D[4 * r] * (double)Tf[c] + D[4 * r + 1] * (double)Tf[4 + c]) + D[4 * r + 2] * (double)Tf[8 + c];
        if (c == 3) s += D[4 * r + 3];
        out[4 * r + c] = (float)s;
      }
    out[12] = out[13] = out[14] = 0.0f;
    out[15] = 1.0f;
    memcpy(o, out, sizeof(out));
  }
  return 0;
}
