/* depth_lut_checker.c -- DESIGN.md section 4k, literally: the depth-distortion table of calibrate_depth's estimate mode and its apply mode, one
 * image at a time, one pixel at a time, in the reference's order (CameraParameterEstimation/apps/calibrate_depth/src/calibrate_depth.cpp:647-836,
 * :565-644; grid3d.h).  Plain C, binary32, built with -O2 -ffp-contract=off.  The reciprocal of the ray's length is the reference's
 * (float)(1.0 / (double)sqrtf(..)) (vector.h:1140-1157); the product's host path and kernels use 1.0f / s (dl_recip_* hold the two together). */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

#define UNKNOWN_GRID_VALUE (-321.0f)

/* 1: the image is used; 0: it is skipped (:691-697) */
int dl_filter(const float T[16]) {
  const float nx = T[2], ny = T[6], nz = T[10];
  const float q = nz / 1.0f * sqrtf(nx * nx + ny * ny + nz * nz);
  const float a = (float)(acosf(q) * 180.0 / M_PI);
  return a > 25.0f ? 0 : 1;
}

static uint16_t unshift(uint16_t d) { return (uint16_t)(((d >> 3) & 0x1FFF) | ((d & 7) << 13)); }

/* one image into the sums; K = {fx, fy, mx, my}; T row-major; acc / div: (W/2) x (H/2) x n_slices */
void dl_accumulate(const uint16_t* img, int W, int H, const float K[4], const float T[16], float n_slices, float max_depth, int bitshift, float* acc,
                   float* div) {
  const float fx = K[0], fy = K[1], mx = K[2], my = K[3];
  const float nx = T[2], ny = T[6], nz = T[10];
  const float px = T[3], py = T[7], pz = T[11];
  const float plane_d = -(nx * px + ny * py + nz * pz);
  const int xres = W / 2, yres = H / 2;
  const float z_bin = n_slices / max_depth;
  if (!dl_filter(T)) return;
  for (int j = 0; j < H; j++)
    for (int i = 0; i < W; i++) {
      uint16_t d = img[(size_t)j * W + i];
      if (bitshift) d = unshift(d);
      const float depth = (float)d * 0.001f;
      const float posx = ((float)i - mx) * depth / fx;
      const float posy = ((float)(H - j) - my) * depth / fy;
      const float posz = -depth;
      float real;
      if ((double)depth > 0.01) {
        const float s = sqrtf(posx * posx + posy * posy + posz * posz);
        const float r = (float)(1.0 / (double)s);
        const float vx = posx * r, vy = posy * r, vz = posz * r;
        const float t = -(0.0f + plane_d) / (vx * nx + vy * ny + vz * nz);
        real = -(0.0f + t * vz);
      } else {
        real = depth;
      }
      const int x = i / 2, y = j / 2, z = (int)floorf(depth * z_bin);
      if (z > (int)n_slices - 1 || z == 0) continue;
      const size_t c = ((size_t)z * yres + y) * xres + x;
      acc[c] += depth * real;
      div[c] += real * real;
    }
}

/* :809-833 */
void dl_finish(const float* acc, const float* div, int xres, int yres, int zres, float* m) {
  const size_t n = (size_t)xres * yres * zres;
  for (size_t i = 0; i < n; i++) m[i] = div[i] == 0.0f ? UNKNOWN_GRID_VALUE : acc[i] / div[i];
  const int stripe = 8 / 2;
  for (int z = 0; z < zres; z++)
    for (int y = 0; y < yres; y++) {
      const float val = m[((size_t)z * yres + y) * xres + (xres - stripe - 1)];
      for (int x = xres - stripe; x < xres; x++) m[((size_t)z * yres + y) * xres + x] = val;
    }
  for (size_t i = 0; i < n; i++)
    if (m[i] == UNKNOWN_GRID_VALUE) m[i] = 1.0f;
}

/* grid3d.h:177-209 */
static float get_value(const float* t, int xr, int yr, int zr, float x, float y, float z) {
  const int x1 = (int)x, y1 = (int)y, z1 = (int)z;
  int x2 = x1 + 1, y2 = y1 + 1, z2 = z1 + 1;
  if (x2 >= xr) x2 = x1;
  if (y2 >= yr) y2 = y1;
  if (z2 >= zr) z2 = z1;
  const float dx = x - (float)x1, dy = y - (float)y1, dz = z - (float)z1;
#define G(a, b, c) t[((size_t)(c) * yr + (b)) * xr + (a)]
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

/* :565-644 on one image */
void dl_apply(const float* t, int xr, int yr, int zr, float max_dist, const uint16_t* in, int W, int H, int bitshift, uint16_t* out) {
  const float x_bin = (float)(W / xr), y_bin = (float)(H / yr), z_bin = (float)zr / max_dist;
  for (int j = 0; j < H; j++)
    for (int i = 0; i < W; i++) {
      uint16_t d = in[(size_t)j * W + i];
      if (bitshift) d = unshift(d);
      const float depth = (float)d * 0.001f;
      const float zi = fminf(depth * z_bin, (float)zr - 1.0f);
      float x = (float)i / x_bin, y = (float)j / y_bin;
      if (x >= (float)xr) x = (float)xr - 1.0f;   /* the table does not divide the image: the last cell (section 4k) */
      if (y >= (float)yr) y = (float)yr - 1.0f;
      const float mult = 1.0f / get_value(t, xr, yr, zr, x, y, zi);
      const float v = 1000.0f * (depth * mult);
      uint16_t nd = !(v >= 0.0f) ? (uint16_t)0 : (v >= 65535.0f ? (uint16_t)65535 : (uint16_t)v);
      if (bitshift) nd = (uint16_t)(((nd & 0xE000) >> 13) | ((nd << 3) & 0xFFF8));
      out[(size_t)j * W + i] = nd;
    }
}

/* the two reciprocal forms on n values: how many differ */
long dl_recip_differ(const float* s, long n) {
  long bad = 0;
  for (long i = 0; i < n; i++) {
    const float a = 1.0f / s[i];
    const float b = (float)(1.0 / (double)s[i]);
    union { float f; uint32_t u; } ua, ub;
    ua.f = a; ub.f = b;
    if (ua.u != ub.u) bad++;
  }
  return bad;
}
