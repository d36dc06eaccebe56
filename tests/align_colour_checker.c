/*
 * tests/align_colour_checker.c -- CPU restatement of the global alignment with the dense colour term (DESIGN.md section 4f "The colour term of the
 * global alignment"; scannet_amd/csrc/align_colour.hip is the GPU side).  It stands alone: the depth term of section 4e is restated here as
 * tests/align_checker.c states it, and the photometric row is added to it.
 *
 * K keyframes (u16 depth, RGB8 colour, camera-to-world poses) and P directed pairs.  Each frame becomes a vertex map, a normal map and a map of
 * {intensity, gx, gy} at one level; each pair gives 31 numbers -- the 27 of the weighted normal equations, the depth term's sum r^2 and count, the
 * colour term's sum r^2 and count -- reduced in the kernel's order (256-pixel workgroups, xor butterfly per 64-lane wave, (w0 + w1) + (w2 + w3),
 * partials summed in index order in double); the host loop is section 4e's on the first 29 of them.
 * Every operation is written out as the specification states it; build with -ffp-contract=off (and -mfma, so that fmaf is one instruction).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define AL_NSYS 31
#define AL_DOWN_THRES 0.03f
#define AL_PIVOT_REL 1e-5
#define AL_MAX_FRAMES 256
#define AL_MAX_PAIRS 4096

typedef struct al_frame {
  int32_t in_w, in_h;            /* input depth size                                  */
  int32_t W, H;                  /* integration size                                  */
  float fx, fy, mx, my;          /* integration intrinsics                            */
  float depth_shift, depth_min, depth_max;
  int32_t color_w, color_h;      /* colour picture size; 0: the integration size      */
  float cfx, cfy, cmx, cmy;      /* colour intrinsics (read when color_w > 0)         */
} al_frame;

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

typedef struct { float x, y, z; } f3;
typedef struct { int W, H; float fx, fy, mx, my; } cam_t;

static f3 xf(const float* T, f3 v) {
  f3 o = {fmaf(T[2], v.z, fmaf(T[1], v.y, fmaf(T[0], v.x, T[3]))), fmaf(T[6], v.z, fmaf(T[5], v.y, fmaf(T[4], v.x, T[7]))),
          fmaf(T[10], v.z, fmaf(T[9], v.y, fmaf(T[8], v.x, T[11])))};
  return o;
}
static f3 rot(const float* T, f3 n) {
  f3 o = {fmaf(T[2], n.z, fmaf(T[1], n.y, T[0] * n.x)), fmaf(T[6], n.z, fmaf(T[5], n.y, T[4] * n.x)), fmaf(T[10], n.z, fmaf(T[9], n.y, T[8] * n.x))};
  return o;
}
static float dot3(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static f3 cross3(f3 a, f3 b) {
  f3 o = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
  return o;
}
static f3 sub3(f3 a, f3 b) {
  f3 o = {a.x - b.x, a.y - b.y, a.z - b.z};
  return o;
}
static f3 unproject(const cam_t* c, int x, int y, float d) {
  f3 o = {((float)x - c->mx) / c->fx * d, ((float)y - c->my) / c->fy * d, d};
  return o;
}
static int finite12(const float* T) {
  for (int i = 0; i < 12; i++)
    if (!isfinite(T[i])) return 0;
  return 1;
}

/* the level the parameters choose on a W x H integration image and its camera; -1: none */
static int pick_level(const al_frame* fr, const al_params* a, cam_t* c) {
  int l = a->level;
  if (l < 0 || l > 3) return -1;
  if ((a->down_width == 0) != (a->down_height == 0) || a->down_width < 0 || a->down_height < 0) return -1;
  if (a->down_width > 0) {
    l = -1;
    for (int k = 0; k < 4 && l < 0; k++)
      if ((fr->W >> k) == a->down_width && (fr->H >> k) == a->down_height) l = k;
    if (l < 0) return -1;
  }
  c->W = fr->W >> l;
  c->H = fr->H >> l;
  if (c->W < 8 || c->H < 8) return -1;
  const float sx = (float)c->W / (float)fr->W, sy = (float)c->H / (float)fr->H;
  c->fx = fr->fx * sx; c->mx = fr->mx * sx;
  c->fy = fr->fy * sy; c->my = fr->my * sy;
  return l;
}

static int check_args(int64_t K, const int32_t* pairs, int64_t P, const al_params* a) {
  if (a->max_iters < 1 || a->max_iters > 100) return -1;
  if (!isfinite(a->dist_thres) || !(a->dist_thres > 0.0f)) return -1;
  if (!(a->normal_thres >= -1.0f && a->normal_thres <= 1.0f)) return -1;
  if (!isfinite(a->depth_min) || !isfinite(a->depth_max) || a->depth_min < 0.0f || a->depth_max < a->depth_min) return -1;
  if (!isfinite(a->early_out) || !(a->early_out >= 0.0f)) return -1;
  if (a->min_pair_correspondences < 1) return -1;
  if (!isfinite(a->max_translation) || !(a->max_translation > 0.0f) || !isfinite(a->max_rotation) || !(a->max_rotation > 0.0f)) return -1;
  if (!isfinite(a->colour_weight) || !(a->colour_weight >= 0.0f)) return -1;
  if (!isfinite(a->colour_thres) || !(a->colour_thres >= 0.0f)) return -1;
  if (!isfinite(a->colour_gradient_min) || !(a->colour_gradient_min >= 0.0f)) return -1;
  if (K < 2 || K > AL_MAX_FRAMES) return -1;
  if (a->fixed_frame < 0 || a->fixed_frame >= K) return -1;
  if (P < 1 || P > AL_MAX_PAIRS) return -1;
  for (int64_t p = 0; p < P; p++) {
    const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
    if (i < 0 || j < 0 || i >= K || j >= K || i == j) return -1;
  }
  return 0;
}

/* one frame's vertex and normal map at level l (x = -inf: invalid) */
static void frame_maps(const al_frame* fr, const uint16_t* depth, int l, const cam_t* c, float dmin, float dmax, f3* vmap, f3* nmap) {
  int Wc = fr->W, Hc = fr->H;
  float* d = (float*)malloc(sizeof(float) * Wc * Hc);
  const int resample = fr->in_w != fr->W || fr->in_h != fr->H;
  const float rsx = resample ? (float)(fr->in_w - 1) / (float)(fr->W - 1) : 1.0f, rsy = resample ? (float)(fr->in_h - 1) / (float)(fr->H - 1) : 1.0f;
  for (int i = 0; i < Wc * Hc; i++) {   /* the pre-pass rule */
    uint16_t u;
    if (resample) {
      const unsigned xi = (unsigned)((float)(i % fr->W) * rsx + 0.5f), yi = (unsigned)((float)(i / fr->W) * rsy + 0.5f);
      u = (xi < (unsigned)fr->in_w && yi < (unsigned)fr->in_h) ? depth[(size_t)yi * fr->in_w + xi] : 0;
    } else {
      u = depth[i];
    }
    float v = (float)u / fr->depth_shift;
    if (u == 0 || v < fr->depth_min || v > fr->depth_max) v = -INFINITY;
    d[i] = v;
  }
  for (int k = 0; k < l; k++) {   /* l reductions */
    const int Wd = Wc >> 1, Hd = Hc >> 1;
    float* e = (float*)malloc(sizeof(float) * Wd * Hd);
    for (int y = 0; y < Hd; y++)
      for (int x = 0; x < Wd; x++) {
        const float* p = d + (size_t)(2 * y) * Wc + 2 * x;
        const float r = p[0];
        float out = -INFINITY;
        if (r > 0.0f) {
          const float v[4] = {p[0], p[1], p[Wc], p[Wc + 1]};
          float sum = 0.0f, cnt = 0.0f;
          for (int q = 0; q < 4; q++)
            if (v[q] > 0.0f && fabsf(v[q] - r) <= AL_DOWN_THRES) {
              sum = sum + v[q];
              cnt = cnt + 1.0f;
            }
          out = sum / cnt;
        }
        e[y * Wd + x] = out;
      }
    free(d);
    d = e;
    Wc = Wd;
    Hc = Hd;
  }
  for (int i = 0; i < Wc * Hc; i++)   /* the solver's own gate */
    if (!(d[i] >= dmin && d[i] <= dmax)) d[i] = -INFINITY;
  for (int y = 0; y < c->H; y++)
    for (int x = 0; x < c->W; x++) {
      const int i = y * c->W + x;
      const f3 inv = {-INFINITY, -INFINITY, -INFINITY};
      f3 vo = inv, no = inv;
      const float dz = d[i];
      if (dz > 0.0f) {
        const f3 v = unproject(c, x, y, dz);
        vo = v;
        if (x + 1 < c->W && y + 1 < c->H) {
          const float dr = d[i + 1], dd = d[i + c->W];
          if (dr > 0.0f && dd > 0.0f) {
            const f3 n = cross3(sub3(unproject(c, x, y + 1, dd), v), sub3(unproject(c, x + 1, y, dr), v));
            const float len = sqrtf(dot3(n, n));
            if (len > 0.0f) { no.x = n.x / len; no.y = n.y / len; no.z = n.z / len; }
          }
        }
      }
      vmap[i] = vo;
      nmap[i] = no;
    }
  free(d);
}

/* one frame's {I, gx, gy} at level l (-inf: invalid) from its RGB8 picture */
static void frame_photo(const al_frame* fr, const uint8_t* rgb, int l, const cam_t* c, f3* pmap) {
  int Wc = fr->W, Hc = fr->H;
  float* d = (float*)malloc(sizeof(float) * Wc * Hc);
  for (int y = 0; y < Hc; y++)
    for (int x = 0; x < Wc; x++) {   /* the pre-pass's colour look-up */
      int cx = x, cy = y, cw = fr->W, ok = 1;
      if (fr->color_w > 0) {
        const float u = fmaf(((float)x - fr->mx) / fr->fx, fr->cfx, fr->cmx) + 0.5f;
        const float v = fmaf(((float)y - fr->my) / fr->fy, fr->cfy, fr->cmy) + 0.5f;
        ok = u >= 0.0f && u < (float)fr->color_w && v >= 0.0f && v < (float)fr->color_h;
        cx = ok ? (int)u : 0;
        cy = ok ? (int)v : 0;
        cw = fr->color_w;
      }
      float I = -INFINITY;
      if (ok) {
        const uint8_t* q = rgb + 3 * ((size_t)cy * cw + cx);
        I = ((0.299f * (float)q[0] + 0.587f * (float)q[1]) + 0.114f * (float)q[2]) / 255.0f;
      }
      d[y * Wc + x] = I;
    }
  for (int k = 0; k < l; k++) {   /* l reductions: the mean of the 2x2 block, invalid if one of the four is */
    const int Wd = Wc >> 1, Hd = Hc >> 1;
    float* e = (float*)malloc(sizeof(float) * Wd * Hd);
    for (int y = 0; y < Hd; y++)
      for (int x = 0; x < Wd; x++) {
        const float* p = d + (size_t)(2 * y) * Wc + 2 * x;
        const float s00 = p[0], s10 = p[1], s01 = p[Wc], s11 = p[Wc + 1];
        e[y * Wd + x] = (s00 >= 0.0f && s10 >= 0.0f && s01 >= 0.0f && s11 >= 0.0f) ? (((s00 + s10) + s01) + s11) * 0.25f : -INFINITY;
      }
    free(d);
    d = e;
    Wc = Wd;
    Hc = Hd;
  }
  for (int y = 0; y < c->H; y++)
    for (int x = 0; x < c->W; x++) {
      const int i = y * c->W + x;
      f3 o = {d[i], -INFINITY, -INFINITY};
      if (x >= 1 && x + 1 < c->W && y >= 1 && y + 1 < c->H) {
        const float xl = d[i - 1], xr = d[i + 1], yu = d[i - c->W], yd = d[i + c->W];
        if (xl >= 0.0f && xr >= 0.0f && yu >= 0.0f && yd >= 0.0f) {
          o.y = (xr - xl) * 0.5f;
          o.z = (yd - yu) * 0.5f;
        }
      }
      pmap[i] = o;
    }
  free(d);
}

typedef struct {
  int K, npx;
  cam_t cam;
  f3 *v, *n;   /* [K][npx] */
  f3* ph;      /* [K][npx] {I, gx, gy}; NULL: no colour pictures */
} maps_t;

static int maps_build(maps_t* m, const al_frame* fr, const uint16_t* depth, const uint8_t* rgb, int K, const al_params* a) {
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

/* T_j^-1 T_i: the inverse by cofactors over the determinant, the product and the translation in double, rounded to float once */
static void compose_ref(const double* Tref, const double* T, float* M) {
  const double a00 = Tref[0], a01 = Tref[1], a02 = Tref[2], a10 = Tref[4], a11 = Tref[5], a12 = Tref[6], a20 = Tref[8], a21 = Tref[9], a22 = Tref[10];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  double inv[9];
  inv[0] = c00 / det; inv[1] = (a02 * a21 - a01 * a22) / det; inv[2] = (a01 * a12 - a02 * a11) / det;
  inv[3] = c01 / det; inv[4] = (a00 * a22 - a02 * a20) / det; inv[5] = (a02 * a10 - a00 * a12) / det;
  inv[6] = c02 / det; inv[7] = (a01 * a20 - a00 * a21) / det; inv[8] = (a00 * a11 - a01 * a10) / det;
  const double dt[3] = {T[3] - Tref[3], T[7] - Tref[7], T[11] - Tref[11]};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[4 * r + c] = (float)((inv[3 * r] * T[c] + inv[3 * r + 1] * T[4 + c]) + inv[3 * r + 2] * T[8 + c]);
    M[4 * r + 3] = (float)((inv[3 * r] * dt[0] + inv[3 * r + 1] * dt[1]) + inv[3 * r + 2] * dt[2]);
  }
}

/* bilinear sample of one component: the two rows along x, then along y */
static float bilin(float t00, float t10, float t01, float t11, float ax, float ay) {
  const float top = fmaf(ax, t10 - t00, t00), bot = fmaf(ax, t11 - t01, t01);
  return fmaf(ay, bot - top, top);
}

/* the colour row of a depth correspondence: source pixel px of frame i, c = M v in frame j's camera, p = T_i v.  1 and (r_c, J_c) when the pixel has one */
static int colour_row(const maps_t* m, int i, int j, int px, f3 pc, f3 p, const float* Tj, const al_params* a, float* rc, float* J) {
  const cam_t* c = &m->cam;
  const float Is = m->ph[(size_t)i * m->npx + px].x;
  if (!(Is >= 0.0f)) return 0;
  const float uf = fmaf(pc.x / pc.z, c->fx, c->mx), vf = fmaf(pc.y / pc.z, c->fy, c->my);
  if (!(uf >= 0.0f && uf < (float)(c->W - 1) && vf >= 0.0f && vf < (float)(c->H - 1))) return 0;
  const float xf0 = floorf(uf), yf0 = floorf(vf);
  const int x0 = (int)xf0, y0 = (int)yf0;
  const f3* t = m->ph + (size_t)j * m->npx + (size_t)(y0 * c->W + x0);
  const f3 t00 = t[0], t10 = t[1], t01 = t[c->W], t11 = t[c->W + 1];
  if (!(t00.x >= 0.0f && t00.y > -INFINITY && t10.x >= 0.0f && t10.y > -INFINITY && t01.x >= 0.0f && t01.y > -INFINITY && t11.x >= 0.0f && t11.y > -INFINITY))
    return 0;
  const float ax = uf - xf0, ay = vf - yf0;
  const float It = bilin(t00.x, t10.x, t01.x, t11.x, ax, ay);
  const float gx = bilin(t00.y, t10.y, t01.y, t11.y, ax, ay), gy = bilin(t00.z, t10.z, t01.z, t11.z, ax, ay);
  const float r = It - Is;
  if (fabsf(r) > a->colour_thres || sqrtf(gx * gx + gy * gy) < a->colour_gradient_min) return 0;
  const float gxf = gx * c->fx, gyf = gy * c->fy;
  const f3 g = {gxf / pc.z, gyf / pc.z, -((gxf * pc.x + gyf * pc.y) / (pc.z * pc.z))};
  const f3 av = rot(Tj, g);
  const f3 cr = cross3(p, av);
  J[0] = cr.x; J[1] = cr.y; J[2] = cr.z; J[3] = av.x; J[4] = av.y; J[5] = av.z;
  *rc = r;
  return 1;
}

/* one source pixel's 31 values for the pair (i, j); 1 when it is a (depth) correspondence */
static int pixel_row(const maps_t* m, int i, int j, int px, const float* Ti, const float* Tj, const float* M, const al_params* prm, float* acc) {
  const float dthr = prm->dist_thres, nthr = prm->normal_thres;
  const cam_t* c = &m->cam;
  const f3 v = m->v[(size_t)i * m->npx + px], nc = m->n[(size_t)i * m->npx + px];
  if (!(v.z > 0.0f && nc.x > -INFINITY)) return 0;
  const f3 p = xf(Ti, v), n = rot(Ti, nc), pc = xf(M, v);
  if (!(pc.z > 0.0f)) return 0;
  const float ux = floorf(fmaf(pc.x / pc.z, c->fx, c->mx) + 0.5f), uy = floorf(fmaf(pc.y / pc.z, c->fy, c->my) + 0.5f);
  if (!(ux >= 0.0f && ux < (float)c->W && uy >= 0.0f && uy < (float)c->H)) return 0;
  const size_t t = (size_t)j * m->npx + (size_t)((int)uy * c->W + (int)ux);
  const f3 vj = m->v[t], nj = m->n[t];
  if (!(vj.z > 0.0f && nj.x > -INFINITY)) return 0;
  const f3 q = xf(Tj, vj), nm = rot(Tj, nj);
  const f3 d = sub3(p, q);
  if (!(sqrtf(dot3(d, d)) <= dthr && dot3(nm, n) >= nthr)) return 0;
  const float r = dot3(nm, d);
  const f3 cr = cross3(p, nm);
  const float J[6] = {cr.x, cr.y, cr.z, nm.x, nm.y, nm.z};
  int k = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) acc[k++] = J[a] * J[b];
  for (int a = 0; a < 6; a++) acc[21 + a] = J[a] * r;
  acc[27] = r * r;
  acc[28] = 1.0f;
  float rc, Jc[6];
  if (m->ph && colour_row(m, i, j, px, pc, p, Tj, prm, &rc, Jc)) {
    const float w = prm->colour_weight;
    if (w != 0.0f) {   /* weight 0: the depth term's sums stay as they are */
      k = 0;
      for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++, k++) acc[k] = acc[k] + w * (Jc[a] * Jc[b]);
      for (int a = 0; a < 6; a++) acc[21 + a] = acc[21 + a] + w * (Jc[a] * rc);
    }
    acc[29] = rc * rc;
    acc[30] = 1.0f;
  }
  return 1;
}

/* the P systems at the poses T (K x 12 doubles) */
static void systems_at(const maps_t* m, const double* T, const uint8_t* valid, const int32_t* pairs, int P, const al_params* a, double* sys) {
  const int nb = (m->npx + 255) / 256;
  static float lane[256][AL_NSYS];
  for (int p = 0; p < P; p++) {
    double* tot = sys + (size_t)p * AL_NSYS;
    for (int k = 0; k < AL_NSYS; k++) tot[k] = 0.0;
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    if (!valid[i] || !valid[j]) continue;
    float Ti[12], Tj[12], M[12];
    for (int k = 0; k < 12; k++) { Ti[k] = (float)T[12 * i + k]; Tj[k] = (float)T[12 * j + k]; }
    compose_ref(T + 12 * j, T + 12 * i, M);
    for (int b = 0; b < nb; b++) {
      memset(lane, 0, sizeof(lane));
      for (int tid = 0; tid < 256; tid++) {
        const int px = b * 256 + tid;
        if (px < m->npx) pixel_row(m, i, j, px, Ti, Tj, M, a, lane[tid]);
      }
      float wsum[4][AL_NSYS];
      for (int w = 0; w < 4; w++)
        for (int k = 0; k < AL_NSYS; k++) {
          float x[64];
          for (int q = 0; q < 64; q++) x[q] = lane[64 * w + q][k];
          for (int off = 32; off >= 1; off >>= 1)   /* the xor butterfly: lane 0 keeps x0 + x_off at every step */
            for (int q = 0; q < off; q++) x[q] = x[q] + x[q + off];
          wsum[w][k] = x[0];
        }
      for (int k = 0; k < AL_NSYS; k++) tot[k] += (double)((wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]));
    }
  }
}

static void apply_update(const double* xi, double* T) {
  const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
  const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  double a = 1.0, b = 0.5;
  if (th >= 1e-8) {
    a = sin(th) / th;
    b = (1.0 - cos(th)) / (th * th);
  }
  const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  double R[3][3], out[12];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
      R[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + b * k2;
    }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 4; j++) out[4 * i + j] = (R[i][0] * T[j] + R[i][1] * T[4 + j]) + R[i][2] * T[8 + j];
    out[4 * i + 3] += xi[3 + i];
  }
  memcpy(T, out, sizeof(out));
}

static int uf_find(int* parent, int k) {
  while (parent[k] != k) k = parent[k];
  return k;
}

/* A x = -b, A symmetric N x N: Cholesky, sums in index order; 0 at a pivot <= AL_PIVOT_REL x its diagonal entry */
static int solve_dense(const double* A, const double* b, int N, double* x) {
  double* L = (double*)calloc((size_t)N * N, sizeof(double));
  double* y = (double*)calloc((size_t)N, sizeof(double));
  int ok = 1;
  for (int j = 0; j < N && ok; j++) {
    double s = A[(size_t)j * N + j];
    for (int m = 0; m < j; m++) s -= L[(size_t)j * N + m] * L[(size_t)j * N + m];
    if (!(s > AL_PIVOT_REL * A[(size_t)j * N + j])) { ok = 0; break; }
    L[(size_t)j * N + j] = sqrt(s);
    for (int i = j + 1; i < N; i++) {
      double e = A[(size_t)i * N + j];
      for (int m = 0; m < j; m++) e -= L[(size_t)i * N + m] * L[(size_t)j * N + m];
      L[(size_t)i * N + j] = e / L[(size_t)j * N + j];
    }
  }
  if (ok) {
    for (int i = 0; i < N; i++) {
      double e = -b[i];
      for (int m = 0; m < i; m++) e -= L[(size_t)i * N + m] * y[m];
      y[i] = e / L[(size_t)i * N + i];
    }
    for (int i = N - 1; i >= 0; i--) {
      double e = y[i];
      for (int m = i + 1; m < N; m++) e -= L[(size_t)m * N + i] * x[m];
      x[i] = e / L[(size_t)i * N + i];
    }
  }
  free(L);
  free(y);
  return ok;
}

/* The P per-pair systems at the given poses, 31 doubles each (the library's sf_fuser_align_rgbd_system).  rgb: K pictures or NULL.
 * -1: an argument the library refuses. */
int alc_system(const al_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, const float* poses, const int32_t* pairs, int64_t P, const al_params* a,
               double* sys) {
  if (check_args(K, pairs, P, a) != 0 || (!rgb && a->colour_weight > 0.0f)) return -1;
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
int alc_maps(const al_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, int64_t k, const al_params* a, float* vmap, float* pmap, float* cam_out) {
  maps_t m;
  if (!rgb || k < 0 || k >= K || maps_build(&m, fr, depth, rgb, (int)K, a) != 0) return -1;
  memcpy(vmap, m.v + (size_t)k * m.npx, sizeof(f3) * m.npx);
  memcpy(pmap, m.ph + (size_t)k * m.npx, sizeof(f3) * m.npx);
  cam_out[0] = (float)m.cam.W; cam_out[1] = (float)m.cam.H; cam_out[2] = m.cam.fx; cam_out[3] = m.cam.fy; cam_out[4] = m.cam.mx; cam_out[5] = m.cam.my;
  maps_free(&m);
  return 0;
}

/* The colour rows of pair (i, j) at the given poses for the tests: rows npx x 8 floats {has a colour row, r_c, J_c[6]}, zeros elsewhere */
int alc_rows(const al_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, const float* poses, int32_t i, int32_t j, const al_params* a, float* rows) {
  maps_t m;
  if (!rgb || maps_build(&m, fr, depth, rgb, (int)K, a) != 0) return -1;
  double Td[2][12];
  float Ti[12], Tj[12], M[12];
  for (int k = 0; k < 12; k++) { Td[0][k] = Ti[k] = poses[16 * i + k]; Td[1][k] = Tj[k] = poses[16 * j + k]; }
  compose_ref(Td[1], Td[0], M);
  memset(rows, 0, sizeof(float) * 8 * m.npx);
  for (int px = 0; px < m.npx; px++) {
    float acc[AL_NSYS] = {0};
    if (!pixel_row(&m, i, j, px, Ti, Tj, M, a, acc) || acc[30] == 0.0f) continue;
    const f3 v = m.v[(size_t)i * m.npx + px];
    float* o = rows + 8 * (size_t)px;
    o[0] = 1.0f;
    colour_row(&m, i, j, px, xf(M, v), xf(Ti, v), Tj, a, o + 1, o + 2);
  }
  maps_free(&m);
  return 0;
}

/* The whole alignment (sf_fuser_align_rgbd).  -1: an argument the library refuses. */
int alc_align(const al_frame* fr, const uint16_t* depth, const uint8_t* rgb, int64_t K, const float* poses_in, const int32_t* pairs, int64_t P, const al_params* a,
              float* poses_out, al_result* res) {
  if (check_args(K, pairs, P, a) != 0 || (!rgb && a->colour_weight > 0.0f)) return -1;
  maps_t m;
  if (maps_build(&m, fr, depth, rgb, (int)K, a) != 0) return -1;
  al_result r;
  memset(&r, 0, sizeof(r));
  memcpy(poses_out, poses_in, sizeof(float) * 16 * (size_t)K);
  double* T0 = (double*)calloc((size_t)K * 12, sizeof(double));
  double* T = (double*)calloc((size_t)K * 12, sizeof(double));
  double* sys = (double*)calloc((size_t)P * AL_NSYS, sizeof(double));
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
      kept[p] = valid[i] && valid[j] && sys[(size_t)p * AL_NSYS + 28] >= (double)a->min_pair_correspondences;
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
      const double* s = sys + (size_t)p * AL_NSYS;
      double H[6][6];
      int k = 0;
      for (int u = 0; u < 6; u++)
        for (int v = u; v < 6; v++) H[u][v] = H[v][u] = s[k++];
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
    r.rms_last = corr > 0.0 ? (float)sqrt(r2 / corr) : 0.0f;
    if (it == 0) r.rms_first = r.rms_last;
    r.colour_correspondences = (int64_t)ccorr;
    r.colour_rms_last = ccorr > 0.0 ? (float)sqrt(cr2 / ccorr) : 0.0f;
    if (it == 0) r.colour_rms_first = r.colour_rms_last;
    const int ok = solve_dense(A, b, N, xi);
    double mx = 0.0;
    if (ok) {
      for (int k = 0; k < K; k++)
        if (slot[k] >= 0) apply_update(xi + 6 * slot[k], T + 12 * k);
      for (int k = 0; k < N; k++) mx = fmax(mx, fabs(xi[k]));
    }
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
    const double* G = T0 + 12 * k;
    const double* Tk = T + 12 * k;
    const double dt[3] = {Tk[3] - G[3], Tk[7] - G[7], Tk[11] - G[11]};
    const double dist = sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
    double tr = 0.0;
    for (int i = 0; i < 3; i++) tr += (G[i] * Tk[i] + G[4 + i] * Tk[4 + i]) + G[8 + i] * Tk[8 + i];
    const double ang = acos(fmin(1.0, fmax(-1.0, (tr - 1.0) * 0.5)));
    int fin = 1;
    for (int i = 0; i < 12; i++) fin = fin && isfinite(Tk[i]);
    if (!fin || !(dist <= (double)a->max_translation) || !(ang <= (double)a->max_rotation)) { r.frames_rejected++; continue; }
    float* o = poses_out + 16 * k;
    for (int i = 0; i < 12; i++) o[i] = (float)Tk[i];
    o[12] = o[13] = o[14] = 0.0f;
    o[15] = 1.0f;
  }
  *res = r;
  free(T0); free(T); free(sys); free(valid); free(kept); free(conn); free(parent); free(slot);
  maps_free(&m);
  return 0;
}
