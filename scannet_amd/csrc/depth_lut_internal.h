// depth_lut_internal.h -- the per-pixel rule of calibrate_depth's two batch modes, stated once for the kernels
// (depth_lut.hip) and the host path (depth_lut.cpp), and the estimator both serve.  Binary32, no contraction (-ffp-contract=off), left to right.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"
#include "lut_value.h"

constexpr int LUT_MAX_BATCH = 64;                 // images per launch of k_lut_accumulate
constexpr size_t LUT_LDS_BUDGET = 64 * 1024;      // LDS one workgroup of k_lut_accumulate may take: at least two workgroups share a CU's 160 KiB
constexpr int LUT_MAX_SLICES = (int)(LUT_LDS_BUDGET / (64 * 2 * sizeof(float)));   // 128 with the smallest workgroup, one wave
constexpr float LUT_UNKNOWN = -321.0f;            // UNKNOWN_GRID_VALUE, grid3d.h
constexpr int LUT_STRIPE = 4;                     // stripe_width = 8 / x_bin, calibrate_depth.cpp:813

struct LutGeom {
  int w, h, xres, yres, ns;
  float fx, fy, mx, my;
  float zbin;       // n_slices / max_depth, both floats (:774)
  int bitshift;
};

struct LutImage {   // one image of a batch: where its pixels are and the plane it shows (:684-688)
  const uint16_t* px;
  float nx, ny, nz, d;
  int used;         // the angle filter (:691-697), decided on the host
  int pad;
};

// :623 / init_pointcloud: the sensor's 13.3 fixed point rotated back into millimetres
__host__ __device__ inline uint16_t lut_unshift(uint16_t d) { return (uint16_t)(((d >> 3) & 0x1FFF) | ((d & 7) << 13)); }
// :633
__host__ __device__ inline uint16_t lut_shift(uint16_t d) { return (uint16_t)(((d & 0xE000) >> 13) | ((d << 3) & 0xFFF8)); }

// Pixel (i, j) of an image: the slice it falls into, 1 .. ns - 1, or 0 when the sample is dropped (:793); ta = depth * real, td = real * real.
__host__ __device__ inline int lut_sample(const LutGeom& g, const LutImage& im, int i, int j, uint16_t raw, float& ta, float& td) {
  const uint16_t d = g.bitshift ? lut_unshift(raw) : raw;
  const float depth = (float)d * 0.001f;
  const int z = (int)floorf(depth * g.zbin);
  if (z > g.ns - 1 || z == 0) return 0;
  float real = depth;
  if ((double)depth > 0.01) {
    const float px = ((float)i - g.mx) * depth / g.fx;
    const float py = ((float)(g.h - j) - g.my) * depth / g.fy;
    const float pz = -depth;
    const float r = 1.0f / sqrtf(px * px + py * py + pz * pz);   // == (float)(1.0 / (double)s): 53 >= 2 * 24 + 2
    const float vx = px * r, vy = py * r, vz = pz * r;
    const float t = -(0.0f + im.d) / (vx * im.nx + vy * im.ny + vz * im.nz);
    real = -(0.0f + t * vz);
  }
  ta = depth * real;
  td = real * real;
  return z;
}

struct LutApplyK {
  int w, h, xr, yr, zr;
  float xbin, ybin, zbin;   // (float)(w / xr), (float)(h / yr), zr / max_dist (:584-586)
  int bitshift;
};

// :622-634.  Where the table's resolution does not divide the image, i / xbin can reach xres: the reference's GetValue asserts there; the
// coordinate is then the last cell's (lut_cell, lut_value.h).  A product of 65 536 or more (undefined in the reference) is 65 535; a negative or NaN one is 0.
__host__ __device__ inline uint16_t lut_apply_pixel(const LutApplyK& k, const float* __restrict__ t, int i, int j, uint16_t raw) {
  const uint16_t d = k.bitshift ? lut_unshift(raw) : raw;
  const float depth = (float)d * 0.001f;
  const float zi = fminf(depth * k.zbin, (float)k.zr - 1.0f);
  const float x = lut_cell(i, k.xbin, k.xr), y = lut_cell(j, k.ybin, k.yr);
  const float mult = 1.0f / lut_value(t, k.xr, k.yr, k.zr, x, y, zi);
  const float v = 1000.0f * (depth * mult);
  uint16_t nd = !(v >= 0.0f) ? (uint16_t)0 : (v >= 65535.0f ? (uint16_t)65535 : (uint16_t)v);
  if (k.bitshift) nd = lut_shift(nd);
  return nd;
}

// One cell of the finished table from the sums (:809-833): divide, stripe, unknowns, in that order.
__host__ __device__ inline float lut_finish_cell(const float* __restrict__ acc, const float* __restrict__ div, int xres, size_t row, int x) {
  const int xs = x >= xres - LUT_STRIPE ? xres - LUT_STRIPE - 1 : x;
  const float a = acc[row + xs], b = div[row + xs];
  const float m = b == 0.0f ? LUT_UNKNOWN : a / b;
  return m == LUT_UNKNOWN ? 1.0f : m;
}

struct sf_lut_estimator {
  LutGeom g;
  float max_depth = 0;
  int device = -1;      // -1: the host path
  uint64_t images = 0, used = 0;
  std::vector<float> acc, div;   // host path: the sums
  // device
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float *d_acc = nullptr, *d_div = nullptr, *d_out = nullptr;
  LutImage* d_tab = nullptr;
  uint16_t* d_stage = nullptr;   // LUT_MAX_BATCH images, for host images
  int block = 0;                 // workgroup size chosen from ns
};

// depth_lut.hip
int lut_dev_create(sf_lut_estimator* e);
void lut_dev_destroy(sf_lut_estimator* e);
int lut_dev_add(sf_lut_estimator* e, int n, const LutImage* tab, bool host_pixels, float* kernel_us);   // n <= LUT_MAX_BATCH
int lut_dev_sums(sf_lut_estimator* e, float* acc, float* div);
int lut_dev_finish(sf_lut_estimator* e, float* table);
int lut_dev_apply(int device, const LutApplyK& k, const float* table, int n, const void* const* in, void* const* out, bool host_pixels, float* kernel_us);
