/* oracle/calib_oracle.c -- TEST INFRASTRUCTURE ONLY (never linked into the product).
 *
 * CPU restatement of the `calibrate` stage's per-frame image operations, /root/reference/Calibrate:
 *   or_calib_undistort_rgb / _f32   Calibration::undistort               src/calibration.h:185-223
 *   or_calib_undistort_distance     Calibration::undistortDistance       src/calibration.h:226-250, Grid3D::GetValue src/grid3d.cpp:119-151
 *   or_calib_depth_to_color         Aligner::depthToColor                src/aligner.h:21-87 + shaders/aligner.hlsl:52-166
 *   or_calib_depth_to_color_splat   Aligner::depthToColorDebug           src/aligner.h:90-117 (the reference's own CPU variant)
 *   or_calib_frame                  the frame body of calibrateScan      src/calibration.h:262-304
 * PARITY UNPINNED: the reference cannot be built here (mLib + Direct3D 11), holds no test or fixture for this stage, and its
 * depthToColor is a D3D11 draw call whose result depends on the rasteriser of the GPU it ran on.  What is restated:
 *   - every arithmetic statement of the C++ / HLSL source, operation by operation in binary32 (-ffp-contract=off);
 *   - mLib's math::round (the submodule is empty) is taken as floor(x + 0.5);
 *   - the draw call as a software rasteriser with the Direct3D 11 rules: viewport = target size, pixel centres at +0.5,
 *     vertex positions snapped to 1/256 pixel, top-left fill rule, no culling, LESS depth test on a float depth buffer
 *     cleared to 1.0, z interpolated affinely (w = 1) from the three vertices' projected z.
 *   - the table cell coordinate of a pixel is i / bin and, where it reaches the table's resolution (a resolution that does not divide the image: the
 *     reference's GetValue asserts there), the last cell's, the rule calibrate_depth's apply mode states;
 *   - the draw's depth test writes a strictly smaller z; the stages (or_calib_stage_prepare / _raster / _finalize, or_calib_undistort_rgb) are the
 *     four launches of the HIP path, and or_calib_frame / or_calib_depth_to_color are their composition.
 * The HIP path (scannet_amd/csrc/calibrate.hip) implements the same statements; tests compare them bit for bit and
 * cross-check the rasterised result against the reference's point-splat variant. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  uint32_t color_width, color_height, depth_width, depth_height;
  float color_intrinsic[16], depth_intrinsic[16], depth_extrinsic[16]; /* row-major; depth_extrinsic = depthToColorExtrinsics */
  float color_dist[5], depth_dist[5];
} or_calib;

typedef struct {
  int32_t xres, yres, zres;
  float max_dist;
  const float* data; /* z-major: (z * yres + y) * xres + x  (grid3d.cpp:67-71) */
} or_lut;

static int round_i(float x) { return (int)floorf(x + 0.5f); }

/* calibration.h:192-212: where output pixel (x, y) samples the distorted source */
static void sample_loc(const float* K, const float* c, unsigned x, unsigned y, int* sx, int* sy) {
  const float nx = ((float)x - K[2]) / K[0];
  const float ny = ((float)y - K[6]) / K[5];
  const float r2 = nx * nx + ny * ny;
  const float radial = 1.0f + r2 * c[0] + r2 * r2 * c[1] + r2 * r2 * r2 * c[4];
  float lx = nx * radial, ly = ny * radial;
  lx += 2.0f * c[2] * nx * ny + c[3] * (r2 + 2.0f * nx * nx);
  ly += c[2] * (r2 + 2.0f * ny * ny) + 2.0f * c[3] * nx * ny;
  lx = lx * K[0] + K[2];
  ly = ly * K[5] + K[6];
  *sx = round_i(lx);
  *sy = round_i(ly);
}

void or_calib_undistort_rgb(const uint8_t* src, uint8_t* dst, int w, int h, const float* K, const float* coeff) {
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      int sx, sy;
      sample_loc(K, coeff, (unsigned)x, (unsigned)y, &sx, &sy);
      uint8_t* o = dst + 3 * ((size_t)y * w + x);
      if (sx >= 0 && sx < w && sy >= 0 && sy < h) memcpy(o, src + 3 * ((size_t)sy * w + sx), 3);
      else o[0] = o[1] = o[2] = 0; /* invalid value of the colour image: (0,0,0), calibration.h:265 */
    }
}

void or_calib_undistort_f32(const float* src, float* dst, int w, int h, const float* K, const float* coeff, float invalid) {
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      int sx, sy;
      sample_loc(K, coeff, (unsigned)x, (unsigned)y, &sx, &sy);
      dst[(size_t)y * w + x] = (sx >= 0 && sx < w && sy >= 0 && sy < h) ? src[(size_t)sy * w + sx] : invalid;
    }
}

/* grid3d.cpp:119-151 */
static float lut_value(const or_lut* t, float x, float y, float z) {
  int x1 = (int)x, y1 = (int)y, z1 = (int)z;
  int x2 = x1 + 1, y2 = y1 + 1, z2 = z1 + 1;
  if (x2 >= t->xres) x2 = x1;
  if (y2 >= t->yres) y2 = y1;
  if (z2 >= t->zres) z2 = z1;
  const float dx = x - (float)x1, dy = y - (float)y1, dz = z - (float)z1;
#define G(a, b, c) t->data[((size_t)(c) * t->yres + (b)) * t->xres + (a)]
  float v = 0.0f;
  v += G(x1, y1, z1) * (1.0f - dx) * (1.0f - dy) * (1.0f - dz);
  v += G(x1, y1, z2) * (1.0f - dx) * (1.0f - dy) * dz;
  v += G(x1, y2, z1) * (1.0f - dx) * dy * (1.0f - dz);
  v += G(x1, y2, z2) * (1.0f - dx) * dy * dz;
  v += G(x2, y1, z1) * dx * (1.0f - dy) * (1.0f - dz);
  v += G(x2, y1, z2) * dx * (1.0f - dy) * dz;
  v += G(x2, y2, z1) * dx * dy * (1.0f - dz);
  v += G(x2, y2, z2) * dx * dy * dz;
#undef G
  return v;
}

/* the table cell coordinate of pixel i: i / bin, the last cell's where it reaches res (a resolution that does not divide the image) */
static float lut_cell(int i, float bin, int res) {
  const float x = (float)i / bin;
  return x >= (float)res ? (float)res - 1.0f : x;
}

/* calibration.h:226-250, one pixel: u16 in, u16 out (truncating conversion) */
static uint16_t undistort_distance_px(uint16_t raw, int i, int j, int w, int h, const or_lut* t, float shift) {
  const float xbin = (float)(w / t->xres), ybin = (float)(h / t->yres);
  const float zbin = (float)t->zres / t->max_dist;
  const float depth = (float)raw / shift;
  const float zidx = fminf(depth * zbin, (float)t->zres - 1.0f);
  const float multiplier = 1.0f / lut_value(t, lut_cell(i, xbin, t->xres), lut_cell(j, ybin, t->yres), zidx);
  const float nd = depth * multiplier * shift;
  if (!(nd >= 0.0f)) return 0;            /* NaN / negative: the reference's cast is undefined there */
  return nd >= 65535.0f ? 65535 : (uint16_t)nd;
}

void or_calib_undistort_distance(uint16_t* depth, int w, int h, const or_lut* t, float shift) {
  for (int j = 0; j < h; j++)
    for (int i = 0; i < w; i++) depth[(size_t)j * w + i] = undistort_distance_px(depth[(size_t)j * w + i], i, j, w, h, t, shift);
}

/* ---- depthToColor ------------------------------------------------------------------------------------------------ */
static void invert_intrinsic(const float* K, float* inv) { /* mat4f::getInverse of an upper-triangular pinhole matrix, in double */
  const double fx = K[0], sk = K[1], mx = K[2], fy = K[5], my = K[6];
  memset(inv, 0, 64);
  inv[0] = (float)(1.0 / fx);
  inv[1] = (float)(-sk / (fx * fy));
  inv[2] = (float)((sk * my - mx * fy) / (fx * fy));
  inv[5] = (float)(1.0 / fy);
  inv[6] = (float)(-my / fy);
  inv[10] = 1.0f;
  inv[15] = 1.0f;
}

typedef struct { float px, py, z; int ok; } vert_t;

#define DEPTH_WORLD_MIN 0.1f
#define DEPTH_WORLD_MAX 10.0f

/* aligner.hlsl:52-103 ComputeQuadVertex + the viewport transform: target pixel coordinates and projected z */
static vert_t quad_vertex(float d, int w, int h, const float* Kinv, const float* E, const float* Kc, unsigned wnew, unsigned hnew, int x, int y) {
  vert_t v;
  const float ax = (float)x * d, ay = (float)y * d;
  /* posCam = Kinv * (x d, y d, d, d), w forced to 1 (:55-56) */
  const float cx = Kinv[0] * ax + Kinv[1] * ay + Kinv[2] * d + Kinv[3] * d;
  const float cy = Kinv[4] * ax + Kinv[5] * ay + Kinv[6] * d + Kinv[7] * d;
  const float cz = Kinv[8] * ax + Kinv[9] * ay + Kinv[10] * d + Kinv[11] * d;
  /* posWorld = E * posCam, / w (:58-59) */
  float wx = E[0] * cx + E[1] * cy + E[2] * cz + E[3];
  float wy = E[4] * cx + E[5] * cy + E[6] * cz + E[7];
  float wz = E[8] * cx + E[9] * cy + E[10] * cz + E[11];
  const float ww = E[12] * cx + E[13] * cy + E[14] * cz + E[15];
  wx /= ww; wy /= ww; wz /= ww;
  /* posClip = Kc * posWorld, x and y divided by z (:78-79) */
  const float qx = Kc[0] * wx + Kc[1] * wy + Kc[2] * wz + Kc[3];
  const float qy = Kc[4] * wx + Kc[5] * wy + Kc[6] * wz + Kc[7];
  const float qz = Kc[8] * wx + Kc[9] * wy + Kc[10] * wz + Kc[11];
  const float ux = qx / qz, uy = qy / qz;
  const float fx = (ux / (float)(wnew - 1)) * 2.0f - 1.0f;               /* :82 */
  const float fy = 1.0f - (uy / ((float)hnew - 1.0f)) * 2.0f;            /* :84 */
  const float fz = (qz - DEPTH_WORLD_MIN) / (DEPTH_WORLD_MAX - DEPTH_WORLD_MIN); /* :85, :6-9 */
  v.ok = !(fx < -1.0f || fx > 1.0f) && !(fy < -1.0f || fy > 1.0f) && !(fz < 0.0f || fz > 1.0f); /* isValidVertex :123-129 (NaN passes, as in HLSL) */
  /* viewport: NDC -> target pixels (x right, y down) */
  v.px = (fx + 1.0f) * 0.5f * (float)w;
  v.py = (1.0f - fy) * 0.5f * (float)h;
  v.z = fz;
  return v;
}

static int64_t snap(float p) { /* 1/256 pixel, round to nearest */
  const float s = p * 256.0f;
  if (!(s > -1.0e9f && s < 1.0e9f)) return INT64_MIN; /* NaN / huge: the triangle is dropped */
  return (int64_t)floorf(s + 0.5f);
}

/* one triangle, top-left rule, no culling; z = affine interpolation of the vertices' z */
static void raster_tri(float* zbuf, int w, int h, const vert_t* a, const vert_t* b, const vert_t* c) {
  int64_t x0 = snap(a->px), y0 = snap(a->py), x1 = snap(b->px), y1 = snap(b->py), x2 = snap(c->px), y2 = snap(c->py);
  if (x0 == INT64_MIN || y0 == INT64_MIN || x1 == INT64_MIN || y1 == INT64_MIN || x2 == INT64_MIN || y2 == INT64_MIN) return;
  float z0 = a->z, z1 = b->z, z2 = c->z;
  int64_t area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
  if (area == 0) return;
  if (area < 0) { /* make it counter-clockwise in the (x right, y down) integer frame: swap two vertices */
    int64_t t;
    float tz;
    t = x1; x1 = x2; x2 = t;
    t = y1; y1 = y2; y2 = t;
    tz = z1; z1 = z2; z2 = tz;
    area = -area;
  }
  int64_t minx = x0 < x1 ? x0 : x1, maxx = x0 > x1 ? x0 : x1, miny = y0 < y1 ? y0 : y1, maxy = y0 > y1 ? y0 : y1;
  if (x2 < minx) minx = x2;
  if (x2 > maxx) maxx = x2;
  if (y2 < miny) miny = y2;
  if (y2 > maxy) maxy = y2;
  /* pixel (i, j) has its centre at (256 i + 128, 256 j + 128) */
  int64_t i0 = (minx - 128 + 255) >> 8, i1 = (maxx - 128) >> 8, j0 = (miny - 128 + 255) >> 8, j1 = (maxy - 128) >> 8;
  if (i0 < 0) i0 = 0;
  if (j0 < 0) j0 = 0;
  if (i1 > w - 1) i1 = w - 1;
  if (j1 > h - 1) j1 = h - 1;
  for (int64_t j = j0; j <= j1; j++)
    for (int64_t i = i0; i <= i1; i++) {
      const int64_t px = 256 * i + 128, py = 256 * j + 128;
      /* edge functions of the positively oriented triangle (v0, v1, v2): inside = all >= 0; an edge value of 0 counts only on a
       * top edge (horizontal, interior below it) or a left edge (interior to its right) */
      const int64_t ex[3] = {x1 - x0, x2 - x1, x0 - x2}, ey[3] = {y1 - y0, y2 - y1, y0 - y2};
      const int64_t e0 = ex[0] * (py - y0) - ey[0] * (px - x0);
      const int64_t e1 = ex[1] * (py - y1) - ey[1] * (px - x1);
      const int64_t e2 = ex[2] * (py - y2) - ey[2] * (px - x2);
      const int64_t e[3] = {e0, e1, e2};
      int inside = 1;
      for (int k = 0; k < 3 && inside; k++) {
        if (e[k] < 0) inside = 0;
        else if (e[k] == 0) {
          /* with y down and positive orientation: interior lies to the side where the edge function grows.  top edge: ey == 0 and
           * ex > 0;  left edge: ey < 0 */
          const int top_left = (ey[k] == 0 && ex[k] > 0) || (ey[k] < 0);
          if (!top_left) inside = 0;
        }
      }
      if (!inside) continue;
      /* barycentric weights: e1 belongs to v0, e2 to v1, e0 to v2 */
      const float fa = (float)area;
      const float z = ((float)e1 * z0 + (float)e2 * z1 + (float)e0 * z2) / fa;
      float* zb = &zbuf[(size_t)j * w + i];
      if (z < *zb) *zb = z;
    }
}

/* The draw on caller-given data: und = the depth image in metres (the quad tests read it), vert = 4 floats per pixel {target x, target y, projected z,
 * valid}, zbuf = the depth buffer, initial contents in, result out.  aligner.hlsl:131-173 */
void or_calib_stage_raster(int w, int h, const float* depth, const float* vert, float* zbuf) {
  const float thresh_lin = 0.05f, thresh_off = 0.01f; /* aligner.h:31-32 */
  for (int y = 0; y < h - 1; y++)      /* aligner.hlsl:139-140 */
    for (int x = 0; x < w - 1; x++) {
      const float d0 = depth[(size_t)y * w + x], d1 = depth[(size_t)(y + 1) * w + x], d2 = depth[(size_t)y * w + x + 1], d3 = depth[(size_t)(y + 1) * w + x + 1];
      if (d0 <= DEPTH_WORLD_MIN || d1 <= DEPTH_WORLD_MIN || d2 <= DEPTH_WORLD_MIN || d3 <= DEPTH_WORLD_MIN) continue;  /* :147 */
      if (d0 == -INFINITY || d1 == -INFINITY || d2 == -INFINITY || d3 == -INFINITY) continue;                        /* :148 */
      const float dmax = fmaxf(fmaxf(d0, d1), fmaxf(d2, d3)), dmin = fminf(fminf(d0, d1), fminf(d2, d3));
      const float dm = 0.5f * (dmax + dmin);
      if (dmax - dmin > thresh_off + thresh_lin * dm) continue;                                                      /* :154 */
      vert_t v[4];
      const int at[4][2] = {{x, y + 1}, {x, y}, {x + 1, y + 1}, {x + 1, y}};
      for (int k = 0; k < 4; k++) {
        const float* q = vert + 4 * ((size_t)at[k][1] * w + at[k][0]);
        v[k].px = q[0]; v[k].py = q[1]; v[k].z = q[2]; v[k].ok = q[3] != 0.0f;
      }
      if (!(v[0].ok && v[1].ok && v[2].ok && v[3].ok)) continue;                                                     /* :162 */
      raster_tri(zbuf, w, h, &v[0], &v[1], &v[2]); /* triangle strip v0 v1 v2 v3 */
      raster_tri(zbuf, w, h, &v[1], &v[2], &v[3]);
    }
}

/* the mesh vertex of every pixel of a depth image in metres (aligner.hlsl:66-103), 4 floats per pixel */
static void mesh_vertices(const float* depth, float* vert, int w, int h, const or_calib* cb) {
  float Kinv[16];
  invert_intrinsic(cb->depth_intrinsic, Kinv);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const vert_t v = quad_vertex(depth[(size_t)y * w + x], w, h, Kinv, cb->depth_extrinsic, cb->color_intrinsic, cb->color_width, cb->color_height, x, y);
      float* q = vert + 4 * ((size_t)y * w + x);
      q[0] = v.px; q[1] = v.py; q[2] = v.z; q[3] = v.ok ? 1.0f : 0.0f;
    }
}

/* aligner.h:21-87: result in metres, `invalid` where nothing was drawn */
void or_calib_depth_to_color(const float* depth, float* out, int w, int h, const or_calib* cb, float invalid) {
  float* zbuf = (float*)malloc((size_t)w * h * sizeof(float));
  float* vert = (float*)malloc((size_t)w * h * 4 * sizeof(float));
  for (size_t i = 0; i < (size_t)w * h; i++) zbuf[i] = 1.0f;
  mesh_vertices(depth, vert, w, h, cb);
  or_calib_stage_raster(w, h, depth, vert, zbuf);
  for (size_t i = 0; i < (size_t)w * h; i++)  /* aligner.h:78-81 */
    out[i] = zbuf[i] == 1.0f ? invalid : DEPTH_WORLD_MIN + zbuf[i] * (DEPTH_WORLD_MAX - DEPTH_WORLD_MIN);
  free(zbuf); free(vert);
}

/* aligner.h:90-117 / calibration.h:153-183: the reference's CPU variant (forward point splat, last writer wins in scan order) */
void or_calib_depth_to_color_splat(const float* depth, float* out, int w, int h, const or_calib* cb, float invalid) {
  float Kinv[16];
  invert_intrinsic(cb->depth_intrinsic, Kinv);
  const float* E = cb->depth_extrinsic;
  const float* Kc = cb->color_intrinsic;
  const float sw = (float)(w - 1) / (float)(cb->color_width - 1), sh = (float)(h - 1) / (float)(cb->color_height - 1);
  for (size_t i = 0; i < (size_t)w * h; i++) out[i] = invalid;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const float d = depth[(size_t)y * w + x];
      if (d == invalid) continue;
      const float ax = (float)x * d, ay = (float)y * d;
      const float cx = Kinv[0] * ax + Kinv[1] * ay + Kinv[2] * d, cy = Kinv[4] * ax + Kinv[5] * ay + Kinv[6] * d, cz = Kinv[8] * ax + Kinv[9] * ay + Kinv[10] * d;
      const float wx = E[0] * cx + E[1] * cy + E[2] * cz + E[3], wy = E[4] * cx + E[5] * cy + E[6] * cz + E[7], wz = E[8] * cx + E[9] * cy + E[10] * cz + E[11];
      float qx = Kc[0] * wx + Kc[1] * wy + Kc[2] * wz, qy = Kc[4] * wx + Kc[5] * wy + Kc[6] * wz;
      const float qz = Kc[8] * wx + Kc[9] * wy + Kc[10] * wz;
      qx /= qz; qy /= qz;
      const int ix = round_i(qx * sw), iy = round_i(qy * sh);
      if (ix >= 0 && ix < w && iy >= 0 && iy < h) out[(size_t)iy * w + ix] = qz;
    }
}

/* calibration.h:272-281 + the vertices and the clear of the draw: raw u16 -> the table-corrected (on the source pixel), undistorted depth in metres,
 * the mesh vertex of every pixel and the cleared depth buffer.  lut may be NULL. */
void or_calib_stage_prepare(const or_calib* cb, const or_lut* lut, float shift, const uint16_t* depth_in, float* und, float* vert, float* zbuf) {
  const int w = (int)cb->depth_width, h = (int)cb->depth_height;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      int sx, sy;
      sample_loc(cb->depth_intrinsic, cb->depth_dist, (unsigned)x, (unsigned)y, &sx, &sy);
      float v = 0.0f; /* invalid value of the depth image, calibration.h:276 */
      if (sx >= 0 && sx < w && sy >= 0 && sy < h) {
        uint16_t u = depth_in[(size_t)sy * w + sx];
        if (lut) u = undistort_distance_px(u, sx, sy, w, h, lut, shift);                                              /* :272 */
        v = (float)u / shift;                                                                                          /* :275-278 */
      }
      und[(size_t)y * w + x] = v;
      zbuf[(size_t)y * w + x] = 1.0f;
    }
  mesh_vertices(und, vert, w, h, cb);
}

/* aligner.h:78-81 + calibration.h:286-301: depth buffer -> metres -> "invalidate depth where we have no color" -> u16.  rgb (undistorted) may be NULL. */
void or_calib_stage_finalize(const or_calib* cb, float shift, const float* zbuf, const uint8_t* rgb, uint16_t* depth_out) {
  const int w = (int)cb->depth_width, h = (int)cb->depth_height, cw = (int)cb->color_width, ch = (int)cb->color_height;
  const float sw = (float)(w - 1) / (float)(cw - 1), sh = (float)(h - 1) / (float)(ch - 1);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const float zb = zbuf[(size_t)y * w + x];
      float d = zb == 1.0f ? 0.0f : DEPTH_WORLD_MIN + zb * (DEPTH_WORLD_MAX - DEPTH_WORLD_MIN);
      if (rgb) {                                                                                                       /* :286-295 */
        int cx = round_i((float)x / sw), cy = round_i((float)y / sh);
        if (cx > cw - 1) cx = cw - 1;  /* c(x, y) of an out-of-range coordinate is undefined in the reference; clamped */
        if (cy > ch - 1) cy = ch - 1;
        const uint8_t* p = rgb + 3 * ((size_t)cy * cw + cx);
        if (p[0] == 0 && p[1] == 0 && p[2] == 0) d = 0.0f;
      }
      const int r = round_i(d * shift);                                                                                /* :298-301 */
      depth_out[(size_t)y * w + x] = (uint16_t)(r < 0 ? 0 : (r > 65535 ? 65535 : r));
    }
}

/* calibration.h:262-304: one frame, the composition of the stages.  rgb_in / rgb_out may be NULL (no colour: nothing is invalidated by black pixels). */
void or_calib_frame(const or_calib* cb, const or_lut* lut, float shift, const uint8_t* rgb_in, uint8_t* rgb_out, const uint16_t* depth_in, uint16_t* depth_out) {
  const int w = (int)cb->depth_width, h = (int)cb->depth_height, cw = (int)cb->color_width, ch = (int)cb->color_height;
  if (rgb_in && rgb_out) or_calib_undistort_rgb(rgb_in, rgb_out, cw, ch, cb->color_intrinsic, cb->color_dist);      /* :264-268 */
  float* und = (float*)malloc((size_t)w * h * 4);
  float* zbuf = (float*)malloc((size_t)w * h * 4);
  float* vert = (float*)malloc((size_t)w * h * 16);
  or_calib_stage_prepare(cb, lut, shift, depth_in, und, vert, zbuf);                                                   /* :272-281 */
  or_calib_stage_raster(w, h, und, vert, zbuf);                                                                        /* :283 */
  or_calib_stage_finalize(cb, shift, zbuf, rgb_out, depth_out);                                                        /* :286-301 */
  free(und); free(zbuf); free(vert);
}
