// lut_value.h -- the trilinear read of the depth-distortion table, shared by the `calibrate` stage's k_depth_prepare (calibrate.hip) and by
// k_lut_apply / the host path of calibrate_depth's apply mode (depth_lut.hip, depth_lut.cpp).  Grid3D::GetValue(float, float, float):
// Calibrate/src/grid3d.cpp:119-151 and CameraParameterEstimation/apps/calibrate_depth/src/grid3d.h:177-209 are the same text.
#pragma once
#include <hip/hip_runtime.h>

// The table cell coordinate of pixel i along an axis of `res` cells, bin = (float)(size / res) pixels per cell (calibration.h:241, calibrate_depth.cpp:626).
// Where res does not divide the image size, i / bin reaches res (the reference's GetValue asserts there): the coordinate is then the last cell's.
__host__ __device__ inline float lut_cell(int i, float bin, int res) {
  const float x = (float)i / bin;
  return x >= (float)res ? (float)res - 1.0f : x;
}

// grid3d.cpp:119-151.  x in [0, xr), y in [0, yr), z in [0, zr): only the upper neighbour is clamped.
__host__ __device__ inline float lut_value(const float* __restrict__ t, int xr, int yr, int zr, float x, float y, float z) {
  const int x1 = (int)x, y1 = (int)y, z1 = (int)z;
  int x2 = x1 + 1, y2 = y1 + 1, z2 = z1 + 1;
  if (x2 >= xr) x2 = x1;
  if (y2 >= yr) y2 = y1;
  if (z2 >= zr) z2 = z1;
  const float dx = x - (float)x1, dy = y - (float)y1, dz = z - (float)z1;
  auto G = [&](int a, int b, int c) { return t[((size_t)c * yr + b) * xr + a]; };
  float v = 0.0f;
  v += G(x1, y1, z1) * (1.0f - dx) * (1.0f - dy) * (1.0f - dz);
  v += G(x1, y1, z2) * (1.0f - dx) * (1.0f - dy) * dz;
  v += G(x1, y2, z1) * (1.0f - dx) * dy * (1.0f - dz);
  v += G(x1, y2, z2) * (1.0f - dx) * dy * dz;
  v += G(x2, y1, z1) * dx * (1.0f - dy) * (1.0f - dz);
  v += G(x2, y1, z2) * dx * (1.0f - dy) * dz;
  v += G(x2, y2, z1) * dx * dy * (1.0f - dz);
  v += G(x2, y2, z2) * dx * dy * dz;
  return v;
}
