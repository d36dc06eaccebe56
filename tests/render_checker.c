/* render_checker.c -- DESIGN.md section 4j restated in plain C, without a product header and WITHOUT A TREE: every ray is tested against every
 * triangle of the mesh, in index order.  Built by the tests with `gcc -O2 -mfma -ffp-contract=off -shared`: nothing fuses but fmaf(); `/` and
 * sqrtf are IEEE.  The product's host path and kernels must give these bits. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>

#define RK_NONE 0xFFFFFFFFu
#define RK_FLT_MAX 3.402823466e38f

typedef struct { const float* xyz; const uint8_t* rgba; int64_t nv; const uint32_t* tris; int64_t nf; float guard; } rk_mesh;

static float rk_guard(const float* xyz, int64_t nv) {   /* 2^-14 x the largest |coordinate| */
  float big = 0.f;
  for (int64_t i = 0; i < 3 * nv; i++) {
    const float a = xyz[i] < 0.f ? -xyz[i] : xyz[i];
    if (a > big) big = a;
  }
  return big * 6.103515625e-05f;
}

static float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static void cross3(const float* a, const float* b, float* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
static float lo3(float a, float b, float c) { float m = a < b ? a : b; return m < c ? m : c; }
static float hi3(float a, float b, float c) { float m = a > b ? a : b; return m > c ? m : c; }

/* the ray-triangle test of 4j: 1 and t, u, v when it accepts */
static int rk_triangle(const rk_mesh* m, int64_t f, const float* o, const float* d, float* t, float* u, float* v) {
  const float *v0 = m->xyz + 3 * (int64_t)m->tris[3 * f], *v1 = m->xyz + 3 * (int64_t)m->tris[3 * f + 1], *v2 = m->xyz + 3 * (int64_t)m->tris[3 * f + 2];
  float e1[3], e2[3], p[3], s[3], q[3];
  for (int a = 0; a < 3; a++) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; }
  cross3(d, e2, p);
  const float det = dot3(e1, p);
  if (!(det > 0.f || det < 0.f)) return 0;
  const float inv = 1.f / det;
  for (int a = 0; a < 3; a++) s[a] = o[a] - v0[a];
  *u = dot3(s, p) * inv;
  if (!(*u >= 0.f && *u <= 1.f)) return 0;
  cross3(s, e1, q);
  *v = dot3(d, q) * inv;
  if (!(*v >= 0.f && *u + *v <= 1.f)) return 0;
  *t = dot3(e2, q) * inv;
  if (!(*t > 0.f && *t <= RK_FLT_MAX)) return 0;
  for (int a = 0; a < 3; a++) {   /* the guard band */
    const float x = fmaf(*t, d[a], o[a]);
    if (!(x >= lo3(v0[a], v1[a], v2[a]) - m->guard && x <= hi3(v0[a], v1[a], v2[a]) + m->guard)) return 0;
  }
  return 1;
}

/* closest hit: the smallest t over all accepting triangles but `exclude`; in index order with a strict "<", the lowest index wins a tie */
static uint32_t rk_closest(const rk_mesh* m, const float* o, const float* d, uint32_t exclude, float* t, float* u, float* v) {
  uint32_t best = RK_NONE;
  *t = 0.f; *u = 0.f; *v = 0.f;
  for (int64_t f = 0; f < m->nf; f++) {
    float tt, uu, vv;
    if ((uint32_t)f == exclude || !rk_triangle(m, f, o, d, &tt, &uu, &vv)) continue;
    if (best == RK_NONE || tt < *t) { best = (uint32_t)f; *t = tt; *u = uu; *v = vv; }
  }
  return best;
}

static uint32_t rk_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
static float rk_uniform(uint32_t pixel, uint32_t sample, uint32_t bounce, uint32_t dim, uint32_t try_) {
  uint32_t h = rk_mix(pixel + 0x9e3779b9u);
  h = rk_mix(h + sample);
  h = rk_mix(h + ((bounce << 8) | (dim << 4) | try_));
  return (float)(h >> 8) * 5.9604644775390625e-8f;
}

void rk_sample(const float* n, uint32_t pixel, uint32_t sample, uint32_t bounce, float* dir) {
  float s[3] = {n[0], n[1], n[2]};
  for (uint32_t k = 0; k < 8; k++) {
    const float u1 = rk_uniform(pixel, sample, bounce, 0, k), u2 = rk_uniform(pixel, sample, bounce, 1, k);
    const float a = (u1 + u1) - 1.f, b = (u2 + u2) - 1.f;
    const float q = a * a + b * b;
    if (q < 1.f) {
      const float r = sqrtf(1.f - q);
      s[0] = (a + a) * r; s[1] = (b + b) * r; s[2] = 1.f - (q + q);
      break;
    }
  }
  const float w[3] = {n[0] + s[0], n[1] + s[1], n[2] + s[2]};
  const float len2 = dot3(w, w);
  if (!(len2 > 0.f && len2 <= RK_FLT_MAX)) { dir[0] = n[0]; dir[1] = n[1]; dir[2] = n[2]; return; }
  const float len = sqrtf(len2);
  for (int a = 0; a < 3; a++) dir[a] = w[a] / len;
}

static float rk_byte(const rk_mesh* m, uint32_t vertex, int c) { return (float)(m->rgba ? m->rgba[4 * (int64_t)vertex + c] : 128) / 255.f; }

/* cam: origin, right, up, forward (3 floats each), tan(fov / 2), aspect */
static void rk_path(const rk_mesh* m, const float* cam, int W, int H, int x, int y, uint32_t sample, int bounces, int ao, int pixel_centre, float* out) {
  const uint32_t pixel = (uint32_t)y * (uint32_t)W + (uint32_t)x;
  const float jx = pixel_centre ? 0.5f : rk_uniform(pixel, sample, 0, 0, 0), jy = pixel_centre ? 0.5f : rk_uniform(pixel, sample, 0, 1, 0);
  const float px = (float)x + jx, py = (float)y + jy;
  const float a = (px + px) / (float)W - 1.f, b = 1.f - (py + py) / (float)H;
  const float sx = a * cam[12], sy = b * (cam[12] / cam[13]);
  float o[3], d[3], w[3], thr[3] = {1.f, 1.f, 1.f};
  for (int k = 0; k < 3; k++) { o[k] = cam[k]; w[k] = fmaf(sy, cam[6 + k], fmaf(sx, cam[3 + k], cam[9 + k])); }
  const float wl = sqrtf(dot3(w, w));
  for (int k = 0; k < 3; k++) d[k] = w[k] / wl;
  uint32_t exclude = RK_NONE;
  out[0] = out[1] = out[2] = 0.f; out[3] = 1.f;
  for (int k = 0; k <= bounces; k++) {
    float t, u, v;
    const uint32_t f = rk_closest(m, o, d, exclude, &t, &u, &v);
    if (f == RK_NONE) {
      out[0] = thr[0]; out[1] = thr[1]; out[2] = thr[2];
      if (k == 0) out[3] = 0.f;
      return;
    }
    if (k == bounces) return;
    const uint32_t i0 = m->tris[3 * (int64_t)f], i1 = m->tris[3 * (int64_t)f + 1], i2 = m->tris[3 * (int64_t)f + 2];
    const float *v0 = m->xyz + 3 * (int64_t)i0, *v1 = m->xyz + 3 * (int64_t)i1, *v2 = m->xyz + 3 * (int64_t)i2;
    float e1[3], e2[3], g[3], n[3];
    for (int c = 0; c < 3; c++) { e1[c] = v1[c] - v0[c]; e2[c] = v2[c] - v0[c]; }
    cross3(e1, e2, g);
    if (!(dot3(d, g) < 0.f)) return;
    const float len2 = dot3(g, g);
    if (!(len2 > 0.f && len2 <= RK_FLT_MAX)) return;
    const float len = sqrtf(len2);
    for (int c = 0; c < 3; c++) n[c] = g[c] / len;
    if (!ao) {
      const float w0 = (1.f - u) - v;
      for (int c = 0; c < 3; c++) thr[c] = thr[c] * ((w0 * rk_byte(m, i0, c) + u * rk_byte(m, i1, c)) + v * rk_byte(m, i2, c));
    }
    for (int c = 0; c < 3; c++) o[c] = fmaf(t, d[c], o[c]);
    rk_sample(n, pixel, sample, (uint32_t)k + 1u, d);
    exclude = f;
  }
}

/* rows y0, y0 + step, ... of one picture: pixels do not depend on each other, so the rows are dealt to a few threads */
typedef struct { const rk_mesh* m; const float* cam; int W, H, samples, max_depth, ao, pixel_centre, y0, step; float* out; } rk_job;

static void* rk_rows(void* arg) {
  const rk_job* j = (const rk_job*)arg;
  for (int y = j->y0; y < j->H; y += j->step)
    for (int x = 0; x < j->W; x++) {
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < j->samples; s++) {   /* in sample order */
        float val[4];
        rk_path(j->m, j->cam, j->W, j->H, x, y, (uint32_t)s, j->ao ? 1 : j->max_depth, j->ao, j->pixel_centre, val);
        for (int c = 0; c < 4; c++) sum[c] = sum[c] + val[c];
      }
      for (int c = 0; c < 4; c++) j->out[4 * ((int64_t)y * j->W + x) + c] = sum[c] / (float)j->samples;
    }
  return 0;
}

/* rgba: 4 bytes per vertex or NULL (every byte 128); out: H x W x 4 floats */
void rk_render(const float* xyz, const uint8_t* rgba, int64_t nv, const uint32_t* tris, int64_t nf, const float* cam, int W, int H, int samples,
               int max_depth, int ao, int pixel_centre, float* out) {
  const rk_mesh m = {xyz, rgba, nv, tris, nf, rk_guard(xyz, nv)};
  enum { THREADS = 8 };
  pthread_t th[THREADS];
  rk_job job[THREADS];
  int started[THREADS];
  for (int k = 0; k < THREADS; k++) {
    const rk_job j = {&m, cam, W, H, samples, max_depth, ao, pixel_centre, k, THREADS, out};
    job[k] = j;
    started[k] = k > 0 && pthread_create(&th[k], 0, rk_rows, &job[k]) == 0;
  }
  rk_rows(&job[0]);
  for (int k = 1; k < THREADS; k++) {
    if (started[k]) pthread_join(th[k], 0);
    else rk_rows(&job[k]);
  }
}

/* rays: origin and direction (6 floats each); tri_out: the triangle or 0xFFFFFFFF; tuv_out: t, u, v (0 on a miss) */
typedef struct { const rk_mesh* m; int64_t n, i0, step; const float* rays; uint32_t* tri_out; float* tuv_out; } rk_ray_job;

static void* rk_ray_rows(void* arg) {
  const rk_ray_job* j = (const rk_ray_job*)arg;
  for (int64_t i = j->i0; i < j->n; i += j->step)
    j->tri_out[i] = rk_closest(j->m, j->rays + 6 * i, j->rays + 6 * i + 3, RK_NONE, j->tuv_out + 3 * i, j->tuv_out + 3 * i + 1, j->tuv_out + 3 * i + 2);
  return 0;
}

void rk_rays(const float* xyz, int64_t nv, const uint32_t* tris, int64_t nf, int64_t n, const float* rays, uint32_t* tri_out, float* tuv_out) {
  const rk_mesh m = {xyz, 0, nv, tris, nf, rk_guard(xyz, nv)};
  enum { THREADS = 8 };
  pthread_t th[THREADS];
  rk_ray_job job[THREADS];
  int started[THREADS];
  for (int k = 0; k < THREADS; k++) {
    const rk_ray_job j = {&m, n, k, THREADS, rays, tri_out, tuv_out};
    job[k] = j;
    started[k] = k > 0 && pthread_create(&th[k], 0, rk_ray_rows, &job[k]) == 0;
  }
  rk_ray_rows(&job[0]);
  for (int k = 1; k < THREADS; k++) {
    if (started[k]) pthread_join(th[k], 0);
    else rk_ray_rows(&job[k]);
  }
}
