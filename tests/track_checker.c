/*
 * tests/track_checker.c -- CPU restatement of the camera tracker (DESIGN.md "Camera tracking"; scannet_amd/csrc/track.hip is the GPU side).
 *
 * Takes the model as the ray caster makes it (depth and world normals at the integration size, cast at T_ref: tests/raycast_checker.c on the CPU),
 * builds the input pyramid, associates, reduces in the kernel's order (256-pixel workgroups, xor butterfly per 64-lane wave, (w0 + w1) + (w2 + w3),
 * partials summed in index order in double) and solves on the host as the library does.  Every operation is written out as the specification
 * states it; build with -ffp-contract=off (and -mfma, so that fmaf is one instruction).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TK_MAX_LEVELS 4
#define TK_NSYS 29
#define TK_DOWN_THRES 0.03f
#define TK_PIVOT_REL 1e-5

typedef struct tk_frame {
  int32_t in_w, in_h;            /* input depth size                                  */
  int32_t W, H;                  /* integration size                                  */
  float fx, fy, mx, my;          /* integration intrinsics                            */
  float depth_shift, depth_min, depth_max;
} tk_frame;

/* the leading fields of sf_track_params */
typedef struct tk_params {
  int32_t levels;
  int32_t max_iters[4];
  float dist_thres[4];
  float normal_thres[4];
  float early_out;
  int32_t min_correspondences;
  float max_translation, max_rotation;
} tk_params;

typedef struct tk_result {
  int32_t tracked, iterations[4], correspondences;
  float rms_residual;
  int32_t lost_reason;
} tk_result;

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

typedef struct {
  int levels;
  cam_t cam[TK_MAX_LEVELS];
  f3 *v[TK_MAX_LEVELS], *n[TK_MAX_LEVELS];   /* x = -inf: invalid */
  f3 *mq, *mn;                                /* the model, level 0 */
} state_t;

static void state_free(state_t* s) {
  for (int l = 0; l < TK_MAX_LEVELS; l++) { free(s->v[l]); free(s->n[l]); }
  free(s->mq);
  free(s->mn);
}

/* -1: a level smaller than 8 x 8 */
static int state_build(state_t* s, const tk_frame* fr, const uint16_t* depth, const float* md, const float* mnrm, const tk_params* t, const float* Tref) {
  memset(s, 0, sizeof(*s));
  s->levels = t->levels;
  for (int l = 0; l < t->levels; l++) {
    cam_t* c = &s->cam[l];
    c->W = fr->W >> l;
    c->H = fr->H >> l;
    if (c->W < 8 || c->H < 8) return -1;
    const float sx = (float)c->W / (float)fr->W, sy = (float)c->H / (float)fr->H;
    c->fx = fr->fx * sx; c->mx = fr->mx * sx;
    c->fy = fr->fy * sy; c->my = fr->my * sy;
  }
  /* level 0 depth: the pre-pass rule */
  float* d[TK_MAX_LEVELS] = {0};
  const int resample = fr->in_w != fr->W || fr->in_h != fr->H;
  const float rsx = resample ? (float)(fr->in_w - 1) / (float)(fr->W - 1) : 1.0f, rsy = resample ? (float)(fr->in_h - 1) / (float)(fr->H - 1) : 1.0f;
  d[0] = (float*)malloc(sizeof(float) * fr->W * fr->H);
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
    d[0][i] = v;
  }
  for (int l = 1; l < t->levels; l++) {
    const int Ws = s->cam[l - 1].W, Wd = s->cam[l].W, Hd = s->cam[l].H;
    d[l] = (float*)malloc(sizeof(float) * Wd * Hd);
    for (int y = 0; y < Hd; y++)
      for (int x = 0; x < Wd; x++) {
        const float* p = d[l - 1] + (size_t)(2 * y) * Ws + 2 * x;
        const float r = p[0];
        float out = -INFINITY;
        if (r > 0.0f) {
          const float v[4] = {p[0], p[1], p[Ws], p[Ws + 1]};
          float sum = 0.0f, cnt = 0.0f;
          for (int k = 0; k < 4; k++)
            if (v[k] > 0.0f && fabsf(v[k] - r) <= TK_DOWN_THRES) {
              sum = sum + v[k];
              cnt = cnt + 1.0f;
            }
          out = sum / cnt;
        }
        d[l][y * Wd + x] = out;
      }
  }
  for (int l = 0; l < t->levels; l++) {
    const cam_t* c = &s->cam[l];
    s->v[l] = (f3*)malloc(sizeof(f3) * c->W * c->H);
    s->n[l] = (f3*)malloc(sizeof(f3) * c->W * c->H);
    for (int y = 0; y < c->H; y++)
      for (int x = 0; x < c->W; x++) {
        const int i = y * c->W + x;
        const f3 inv = {-INFINITY, -INFINITY, -INFINITY};
        f3 vo = inv, no = inv;
        const float dz = d[l][i];
        if (dz > 0.0f) {
          const f3 v = unproject(c, x, y, dz);
          vo = v;
          if (x + 1 < c->W && y + 1 < c->H) {
            const float dr = d[l][i + 1], dd = d[l][i + c->W];
            if (dr > 0.0f && dd > 0.0f) {
              const f3 n = cross3(sub3(unproject(c, x, y + 1, dd), v), sub3(unproject(c, x + 1, y, dr), v));
              const float len = sqrtf(dot3(n, n));
              if (len > 0.0f) { no.x = n.x / len; no.y = n.y / len; no.z = n.z / len; }
            }
          }
        }
        s->v[l][i] = vo;
        s->n[l][i] = no;
      }
  }
  for (int l = 0; l < t->levels; l++) free(d[l]);
  const cam_t* c0 = &s->cam[0];
  s->mq = (f3*)malloc(sizeof(f3) * c0->W * c0->H);
  s->mn = (f3*)malloc(sizeof(f3) * c0->W * c0->H);
  for (int i = 0; i < c0->W * c0->H; i++) {
    const f3 inv = {-INFINITY, -INFINITY, -INFINITY};
    s->mq[i] = inv;
    s->mn[i] = inv;
    if (md[i] > 0.0f && mnrm[3 * i] > -INFINITY) {
      s->mq[i] = xf(Tref, unproject(c0, i % c0->W, i / c0->W, md[i]));
      s->mn[i].x = mnrm[3 * i]; s->mn[i].y = mnrm[3 * i + 1]; s->mn[i].z = mnrm[3 * i + 2];
    }
  }
  return 0;
}

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

/* one pixel's 29 values; 1 when it is a correspondence */
static int pixel_row(const state_t* s, int l, int i, const float* Tf, const float* M, float dthr, float nthr, float* acc) {
  const cam_t* c = &s->cam[l];
  const f3 v = s->v[l][i], nc = s->n[l][i];
  if (!(v.z > 0.0f && nc.x > -INFINITY)) return 0;
  const f3 p = xf(Tf, v), n = rot(Tf, nc), pc = xf(M, v);
  if (!(pc.z > 0.0f)) return 0;
  const float ux = floorf(fmaf(pc.x / pc.z, c->fx, c->mx) + 0.5f), uy = floorf(fmaf(pc.y / pc.z, c->fy, c->my) + 0.5f);
  if (!(ux >= 0.0f && ux < (float)c->W && uy >= 0.0f && uy < (float)c->H)) return 0;
  const size_t j = (size_t)((int)uy << l) * s->cam[0].W + ((int)ux << l);
  const f3 q = s->mq[j];
  if (!(q.x > -INFINITY)) return 0;
  const f3 nm = s->mn[j];
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

static void system_at(const state_t* s, int l, const double* T, const double* Tref, const tk_params* t, double* sys, uint8_t* mask) {
  float Tf[12], M[12];
  for (int i = 0; i < 12; i++) Tf[i] = (float)T[i];
  compose_ref(Tref, T, M);
  const int npx = s->cam[l].W * s->cam[l].H, nb = (npx + 255) / 256;
  double tot[TK_NSYS] = {0};
  static float lane[256][TK_NSYS];
  for (int b = 0; b < nb; b++) {
    memset(lane, 0, sizeof(lane));
    for (int tid = 0; tid < 256; tid++) {
      const int i = b * 256 + tid;
      if (i >= npx) continue;
      const int ok = pixel_row(s, l, i, Tf, M, t->dist_thres[l], t->normal_thres[l], lane[tid]);
      if (mask) mask[i] = (uint8_t)ok;
    }
    float wsum[4][TK_NSYS];
    for (int w = 0; w < 4; w++)
      for (int k = 0; k < TK_NSYS; k++) {
        float x[64];
        for (int i = 0; i < 64; i++) x[i] = lane[64 * w + i][k];
        for (int off = 32; off >= 1; off >>= 1)   /* the xor butterfly: lane 0 keeps x0 + x_off at every step */
          for (int i = 0; i < off; i++) x[i] = x[i] + x[i + off];
        wsum[w][k] = x[0];
      }
    for (int k = 0; k < TK_NSYS; k++) tot[k] += (double)((wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]));
  }
  memcpy(sys, tot, sizeof(tot));
}

static int solve6(const double* sys, double* xi) {
  double A[6][6], L[6][6];
  memset(L, 0, sizeof(L));
  int k = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) A[a][b] = A[b][a] = sys[k++];
  for (int j = 0; j < 6; j++) {
    double s = A[j][j];
    for (int m = 0; m < j; m++) s -= L[j][m] * L[j][m];
    if (!(s > TK_PIVOT_REL * A[j][j])) return 0;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; i++) {
      double e = A[i][j];
      for (int m = 0; m < j; m++) e -= L[i][m] * L[j][m];
      L[i][j] = e / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; i++) {
    double e = -sys[21 + i];
    for (int m = 0; m < i; m++) e -= L[i][m] * y[m];
    y[i] = e / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double e = y[i];
    for (int m = i + 1; m < 6; m++) e -= L[m][i] * xi[m];
    xi[i] = e / L[i][i];
  }
  return 1;
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

static int finite12(const float* T) {
  for (int i = 0; i < 12; i++)
    if (!isfinite(T[i])) return 0;
  return 1;
}

/* One level's system at T (the library's sf_fuser_track_system).  -1: a level below 8 x 8. */
int tk_system(const tk_frame* fr, const uint16_t* depth, const float* md, const float* mnrm, const tk_params* t, int level, const float* T,
              const float* Tref, double* sys, uint8_t* mask) {
  state_t s;
  if (state_build(&s, fr, depth, md, mnrm, t, Tref) != 0) { state_free(&s); return -1; }
  double Td[12], Rd[12];
  for (int i = 0; i < 12; i++) { Td[i] = T[i]; Rd[i] = Tref[i]; }
  system_at(&s, level, Td, Rd, t, sys, mask);
  state_free(&s);
  return 0;
}

/* The whole track (sf_fuser_track) with the model ray-cast at ref (NULL: the guess).  -1: a level below 8 x 8. */
int tk_track(const tk_frame* fr, const uint16_t* depth, const float* md, const float* mnrm, const tk_params* t, const float* guess, const float* ref,
             float* pose_out, tk_result* res) {
  tk_result r;
  memset(&r, 0, sizeof(r));
  for (int i = 0; i < 16; i++) pose_out[i] = -INFINITY;
  if (!ref) ref = guess;
  if (!finite12(guess) || !finite12(ref)) {
    r.lost_reason = 1;
    *res = r;
    return 0;
  }
  state_t s;
  if (state_build(&s, fr, depth, md, mnrm, t, ref) != 0) { state_free(&s); return -1; }
  double T[12], Tref[12], G[12], sys[TK_NSYS];
  for (int i = 0; i < 12; i++) { T[i] = guess[i]; G[i] = guess[i]; Tref[i] = ref[i]; }
  for (int l = t->levels - 1; l >= 0 && r.lost_reason == 0; l--) {
    for (int it = 0; it < t->max_iters[l]; it++) {
      system_at(&s, l, T, Tref, t, sys, NULL);
      if (l == 0) {
        r.correspondences = (int32_t)sys[28];
        r.rms_residual = sys[28] > 0.0 ? (float)sqrt(sys[27] / sys[28]) : 0.0f;
        if (sys[28] < (double)t->min_correspondences) { r.lost_reason = 2; break; }
      }
      double xi[6];
      if (!solve6(sys, xi)) { r.lost_reason = 3; break; }
      apply_update(xi, T);
      r.iterations[l]++;
      double mx = 0.0;
      for (int k = 0; k < 6; k++) mx = fmax(mx, fabs(xi[k]));
      if (mx < (double)t->early_out) break;
    }
  }
  state_free(&s);
  if (r.lost_reason == 0) {
    const double dt[3] = {T[3] - G[3], T[7] - G[7], T[11] - G[11]};
    const double dist = sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
    double tr = 0.0;
    for (int i = 0; i < 3; i++) tr += (G[i] * T[i] + G[4 + i] * T[4 + i]) + G[8 + i] * T[8 + i];
    const double ang = acos(fmin(1.0, fmax(-1.0, (tr - 1.0) * 0.5)));
    int fin = 1;
    for (int i = 0; i < 12; i++) fin = fin && isfinite(T[i]);
    if (!fin || !(dist <= (double)t->max_translation) || !(ang <= (double)t->max_rotation)) r.lost_reason = 4;
  }
  if (r.lost_reason == 0) {
    r.tracked = 1;
    for (int i = 0; i < 12; i++) pose_out[i] = (float)T[i];
    pose_out[12] = pose_out[13] = pose_out[14] = 0.0f;
    pose_out[15] = 1.0f;
  }
  *res = r;
  return 0;
}
