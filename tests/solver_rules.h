/*
 * tests/solver_rules.h -- the rules the camera tracker and the global alignment share, each stated once for their two CPU restatements
 * (tests/track_checker.c and tests/align_checker.c; DESIGN.md sections 4c, 4e, 4f, 4g).  The device side has them once in
 * scannet_amd/csrc/track_math.h and photo_math.h.
 *
 * Every operation is written out as the specification states it, in the specification's order; build with -ffp-contract=off (and -mfma, so that
 * fmaf is one instruction).  Plain C99, nothing beyond libm.  The rows take their inputs as values and plain maps, so neither checker's own state
 * enters a rule.
 */
#ifndef SOLVER_RULES_H
#define SOLVER_RULES_H
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SR_NSYS 31   /* the 27 of the normal equations, the depth term's sum r^2 and count, the colour term's sum r^2 and count */
#define SR_DOWN_THRES 0.03f
#define SR_PIVOT_REL 1e-5

/* one frame description for both checkers */
typedef struct sr_frame {
  int32_t in_w, in_h;            /* input depth size                                  */
  int32_t W, H;                  /* integration size                                  */
  float fx, fy, mx, my;          /* integration intrinsics                            */
  float depth_shift, depth_min, depth_max;
  int32_t color_w, color_h;      /* colour picture size; 0: the integration size      */
  float cfx, cfy, cmx, cmy;      /* colour intrinsics (read when color_w > 0)         */
} sr_frame;

typedef struct { int W, H; float fx, fy, mx, my; } cam_t;
typedef struct { float x, y, z; } f3;

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

/* the camera of level l of the integration image; 0: the level is smaller than 8 x 8 */
static int level_cam(const sr_frame* fr, int l, cam_t* c) {
  c->W = fr->W >> l;
  c->H = fr->H >> l;
  if (c->W < 8 || c->H < 8) return 0;
  const float sx = (float)c->W / (float)fr->W, sy = (float)c->H / (float)fr->H;
  c->fx = fr->fx * sx; c->mx = fr->mx * sx;
  c->fy = fr->fy * sy; c->my = fr->my * sy;
  return 1;
}

/* ---- depth: the pre-pass rule, the 2x2 reduction, vertices and normals ---------------------------------------------------------------------- */

/* level 0 depth in metres at the integration size (-inf: invalid), malloc'ed */
static float* prepass_depth(const sr_frame* fr, const uint16_t* depth) {
  const int resample = fr->in_w != fr->W || fr->in_h != fr->H;
  const float rsx = resample ? (float)(fr->in_w - 1) / (float)(fr->W - 1) : 1.0f, rsy = resample ? (float)(fr->in_h - 1) / (float)(fr->H - 1) : 1.0f;
  float* d = (float*)malloc(sizeof(float) * fr->W * fr->H);
  for (int i = 0; i < fr->W * fr->H; i++) {
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
  return d;
}

/* the next level of a Ws-wide depth map, (Ws >> 1) x (Hs >> 1), malloc'ed: the mean of the block's valid values within SR_DOWN_THRES of its first */
static float* down4(const float* src, int Ws, int Hs) {
  const int Wd = Ws >> 1, Hd = Hs >> 1;
  float* dst = (float*)malloc(sizeof(float) * Wd * Hd);
  for (int y = 0; y < Hd; y++)
    for (int x = 0; x < Wd; x++) {
      const float* p = src + (size_t)(2 * y) * Ws + 2 * x;
      const float r = p[0];
      float out = -INFINITY;
      if (r > 0.0f) {
        const float v[4] = {p[0], p[1], p[Ws], p[Ws + 1]};
        float sum = 0.0f, cnt = 0.0f;
        for (int k = 0; k < 4; k++)
          if (v[k] > 0.0f && fabsf(v[k] - r) <= SR_DOWN_THRES) {
            sum = sum + v[k];
            cnt = cnt + 1.0f;
          }
        out = sum / cnt;
      }
      dst[y * Wd + x] = out;
    }
  return dst;
}

/* camera-space vertices and normals of a depth map at camera c (x = -inf: invalid) */
static void vertex_normal_maps(const cam_t* c, const float* d, f3* vmap, f3* nmap) {
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
}

/* ---- intensity: the rule, the pre-pass's colour look-up, the 2x2 means, the central differences ---------------------------------------------- */

static float intensity_rgb8(const uint8_t* q) { return ((0.299f * (float)q[0] + 0.587f * (float)q[1]) + 0.114f * (float)q[2]) / 255.0f; }

/* level 0 intensity of a frame's picture at the integration size (nearest colour pixel under the depth pixel's ray; -inf: outside), malloc'ed */
static float* prepass_intensity(const sr_frame* fr, const uint8_t* rgb) {
  const int W = fr->W, H = fr->H;
  float* d = (float*)malloc(sizeof(float) * W * H);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      int cx = x, cy = y, cw = fr->W, ok = 1;
      if (fr->color_w > 0) {
        const float u = fmaf(((float)x - fr->mx) / fr->fx, fr->cfx, fr->cmx) + 0.5f;
        const float v = fmaf(((float)y - fr->my) / fr->fy, fr->cfy, fr->cmy) + 0.5f;
        ok = u >= 0.0f && u < (float)fr->color_w && v >= 0.0f && v < (float)fr->color_h;
        cx = ok ? (int)u : 0;
        cy = ok ? (int)v : 0;
        cw = fr->color_w;
      }
      d[y * W + x] = ok ? intensity_rgb8(rgb + 3 * ((size_t)cy * cw + cx)) : -INFINITY;
    }
  return d;
}

/* the next level of a Ws-wide intensity map, malloc'ed: the mean of the 2x2 block, invalid if one of the four is */
static float* photo_down(const float* src, int Ws, int Hs) {
  const int Wd = Ws >> 1, Hd = Hs >> 1;
  float* dst = (float*)malloc(sizeof(float) * Wd * Hd);
  for (int y = 0; y < Hd; y++)
    for (int x = 0; x < Wd; x++) {
      const float* p = src + (size_t)(2 * y) * Ws + 2 * x;
      const float s00 = p[0], s10 = p[1], s01 = p[Ws], s11 = p[Ws + 1];
      dst[y * Wd + x] = (s00 >= 0.0f && s10 >= 0.0f && s01 >= 0.0f && s11 >= 0.0f) ? (((s00 + s10) + s01) + s11) * 0.25f : -INFINITY;
    }
  return dst;
}

/* {I, gx, gy} of an intensity map at camera c: central differences, invalid (-inf) on the border and where one of the four neighbours is */
static void photo_map(const cam_t* c, const float* d, f3* out) {
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
      out[i] = o;
    }
}

/* ---- the two rows ------------------------------------------------------------------------------------------------------------------------------ */

/* the inverse of a pose's 3 x 3 block (rows of 4 doubles) by cofactors over the determinant */
static void inverse3(const double* A, double* inv) {
  const double a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[4], a11 = A[5], a12 = A[6], a20 = A[8], a21 = A[9], a22 = A[10];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  inv[0] = c00 / det; inv[1] = (a02 * a21 - a01 * a22) / det; inv[2] = (a01 * a12 - a02 * a11) / det;
  inv[3] = c01 / det; inv[4] = (a00 * a22 - a02 * a20) / det; inv[5] = (a02 * a10 - a00 * a12) / det;
  inv[6] = c02 / det; inv[7] = (a01 * a20 - a00 * a21) / det; inv[8] = (a00 * a11 - a01 * a10) / det;
}

/* Tref^-1 T: the inverse, the product and the translation in double, rounded to float once */
static void compose_ref(const double* Tref, const double* T, float* M) {
  double inv[9];
  inverse3(Tref, inv);
  const double dt[3] = {T[3] - Tref[3], T[7] - Tref[7], T[11] - Tref[11]};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[4 * r + c] = (float)((inv[3 * r] * T[c] + inv[3 * r + 1] * T[4 + c]) + inv[3 * r + 2] * T[8 + c]);
    M[4 * r + 3] = (float)((inv[3 * r] * dt[0] + inv[3 * r + 1] * dt[1]) + inv[3 * r + 2] * dt[2]);
  }
}

/* the target pixel a source vertex projects to: pc = M v in the target's camera, rounded to the nearest pixel.  1 and (ux, uy) when it is inside */
static int project_nearest(const cam_t* c, f3 pc, int* ux_out, int* uy_out) {
  if (!(pc.z > 0.0f)) return 0;
  const float ux = floorf(fmaf(pc.x / pc.z, c->fx, c->mx) + 0.5f), uy = floorf(fmaf(pc.y / pc.z, c->fy, c->my) + 0.5f);
  if (!(ux >= 0.0f && ux < (float)c->W && uy >= 0.0f && uy < (float)c->H)) return 0;
  *ux_out = (int)ux;
  *uy_out = (int)uy;
  return 1;
}

/* the point-to-plane row: source point p and normal n, target point q and normal nm, all in the world.  1 and the first 29 values of acc when the
 * two gates pass */
static int plane_row(f3 p, f3 n, f3 q, f3 nm, float dthr, float nthr, float* acc) {
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
  return 1;
}

/* bilinear sample of one component: the two rows along x, then along y */
static float bilin(float t00, float t10, float t01, float t11, float ax, float ay) {
  const float top = fmaf(ax, t10 - t00, t00), bot = fmaf(ax, t11 - t01, t01);
  return fmaf(ay, bot - top, top);
}

/* the colour row of a depth correspondence: source intensity Is, the target's {I, gx, gy} map at camera c, pc = M v in the target's camera, p = T v in
 * the world, Tt the target's pose.  1 and (r_c, J_c) when the pixel has one */
static int colour_row(float Is, const f3* tmap, const cam_t* c, f3 pc, f3 p, const float* Tt, float thres, float gradient_min, float* rc, float* J) {
  if (!(Is >= 0.0f)) return 0;
  const float uf = fmaf(pc.x / pc.z, c->fx, c->mx), vf = fmaf(pc.y / pc.z, c->fy, c->my);
  if (!(uf >= 0.0f && uf < (float)(c->W - 1) && vf >= 0.0f && vf < (float)(c->H - 1))) return 0;
  const float xf0 = floorf(uf), yf0 = floorf(vf);
  const int x0 = (int)xf0, y0 = (int)yf0;
  const f3* t = tmap + (size_t)(y0 * c->W + x0);
  const f3 t00 = t[0], t10 = t[1], t01 = t[c->W], t11 = t[c->W + 1];
  if (!(t00.x >= 0.0f && t00.y > -INFINITY && t10.x >= 0.0f && t10.y > -INFINITY && t01.x >= 0.0f && t01.y > -INFINITY && t11.x >= 0.0f && t11.y > -INFINITY))
    return 0;
  const float ax = uf - xf0, ay = vf - yf0;
  const float It = bilin(t00.x, t10.x, t01.x, t11.x, ax, ay);
  const float gx = bilin(t00.y, t10.y, t01.y, t11.y, ax, ay), gy = bilin(t00.z, t10.z, t01.z, t11.z, ax, ay);
  const float r = It - Is;
  if (fabsf(r) > thres || sqrtf(gx * gx + gy * gy) < gradient_min) return 0;
  const float gxf = gx * c->fx, gyf = gy * c->fy;
  const f3 g = {gxf / pc.z, gyf / pc.z, -((gxf * pc.x + gyf * pc.y) / (pc.z * pc.z))};
  const f3 av = rot(Tt, g);
  const f3 cr = cross3(p, av);
  J[0] = cr.x; J[1] = cr.y; J[2] = cr.z; J[3] = av.x; J[4] = av.y; J[5] = av.z;
  *rc = r;
  return 1;
}

/* a colour row joins a correspondence's values with weight w; weight 0 leaves the depth term's sums as they are */
static void add_colour_row(float* acc, float w, float rc, const float* Jc) {
  if (w != 0.0f) {
    int k = 0;
    for (int a = 0; a < 6; a++)
      for (int b = a; b < 6; b++, k++) acc[k] = acc[k] + w * (Jc[a] * Jc[b]);
    for (int a = 0; a < 6; a++) acc[21 + a] = acc[21 + a] + w * (Jc[a] * rc);
  }
  acc[29] = rc * rc;
  acc[30] = 1.0f;
}

/* what the library refuses of the colour term's arguments; it looks at them only when pictures or a non-zero weight are given */
static int colour_args_ok(int has_pictures, float weight, float thres, float gradient_min) {
  if (!has_pictures && weight == 0.0f) return 1;
  if (!isfinite(weight) || !(weight >= 0.0f)) return 0;
  if (!isfinite(thres) || !(thres >= 0.0f)) return 0;
  if (!isfinite(gradient_min) || !(gradient_min >= 0.0f)) return 0;
  return has_pictures || !(weight > 0.0f);
}

/* ---- the reduction and the solve ------------------------------------------------------------------------------------------------------------- */

/* one 256-pixel workgroup: the xor butterfly of each 64-lane wave, (w0 + w1) + (w2 + w3), added to the totals in double */
static void reduce_block(float lane[256][SR_NSYS], double* tot) {
  float wsum[4][SR_NSYS];
  for (int w = 0; w < 4; w++)
    for (int k = 0; k < SR_NSYS; k++) {
      float x[64];
      for (int i = 0; i < 64; i++) x[i] = lane[64 * w + i][k];
      for (int off = 32; off >= 1; off >>= 1)   /* the xor butterfly: lane 0 keeps x0 + x_off at every step */
        for (int i = 0; i < off; i++) x[i] = x[i] + x[i + off];
      wsum[w][k] = x[0];
    }
  for (int k = 0; k < SR_NSYS; k++) tot[k] += (double)((wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]));
}

/* A x = -b, A symmetric N x N: Cholesky, sums in index order; 0 at a pivot <= SR_PIVOT_REL x its diagonal entry.  The tracker's 6 x 6 solve and the
 * alignment's dense one are this loop: the operations and their order do not depend on N. */
static int cholesky_solve(const double* A, const double* b, int N, double* x) {
  double* L = (double*)calloc((size_t)N * N, sizeof(double));
  double* y = (double*)calloc((size_t)N, sizeof(double));
  int ok = 1;
  for (int j = 0; j < N && ok; j++) {
    double s = A[(size_t)j * N + j];
    for (int m = 0; m < j; m++) s -= L[(size_t)j * N + m] * L[(size_t)j * N + m];
    if (!(s > SR_PIVOT_REL * A[(size_t)j * N + j])) { ok = 0; break; }
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

/* the 6 x 6 blocks of a system's 21 upper-triangle values */
static void unpack_sym6(const double* sys, double H[6][6]) {
  int k = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) H[a][b] = H[b][a] = sys[k++];
}

/* T <- exp(xi) T: Rodrigues on xi's first three, the translation added */
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

static double max_abs(const double* x, int n) {
  double mx = 0.0;
  for (int k = 0; k < n; k++) mx = fmax(mx, fabs(x[k]));
  return mx;
}

static float rms_of(double r2, double count) { return count > 0.0 ? (float)sqrt(r2 / count) : 0.0f; }

/* 1 when the solved pose T is finite and within the motion limits of its start G */
static int motion_ok(const double* G, const double* T, float max_translation, float max_rotation) {
  const double dt[3] = {T[3] - G[3], T[7] - G[7], T[11] - G[11]};
  const double dist = sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
  double tr = 0.0;
  for (int i = 0; i < 3; i++) tr += (G[i] * T[i] + G[4 + i] * T[4 + i]) + G[8 + i] * T[8 + i];
  const double ang = acos(fmin(1.0, fmax(-1.0, (tr - 1.0) * 0.5)));
  int fin = 1;
  for (int i = 0; i < 12; i++) fin = fin && isfinite(T[i]);
  return fin && dist <= (double)max_translation && ang <= (double)max_rotation;
}

static void write_pose(const double* T, float* o) {
  for (int i = 0; i < 12; i++) o[i] = (float)T[i];
  o[12] = o[13] = o[14] = 0.0f;
  o[15] = 1.0f;
}

#endif
