// axis_align_math.h -- the fp32 operations of the axis-alignment rule, written once for the host path (axis_align.cpp) and the
// kernels (axis_align.hip).  Every translation unit is built with -ffp-contract=off: each line below is the sequence of separately rounded IEEE
// operations the section lists, and HIP's division and square root are correctly rounded.  tests/axis_align_checker.c restates them independently.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AA_HD __host__ __device__ inline
#else
#define AA_HD inline   // a plain C++ compiler builds the host path alone
#endif

namespace sf {
namespace aa {

constexpr int kCovBlock = 256;   // vertices per block of the covariance sums
constexpr int kChunk = 1024;     // clusters per chunk of the match kernel
constexpr int kMaxBatch = 1024;  // vertices per speculation batch (and the capacity of the commit kernel's dirty list)

struct Cluster {   // one row of the cluster table
  float rep[4];    // representative plane: unit normal, d (n . x + d = 0)
  float sn[3];     // sumNormal
  float sp[3];     // sumPoint
  uint32_t count;
};

AA_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// v / |v|; the zero vector stays zero
AA_HD void normalize3(float& x, float& y, float& z) {
  const float l = sqrtf((x * x + y * y) + z * z);
  if (l == 0.0f) { x = 0.0f; y = 0.0f; z = 0.0f; return; }
  x = x / l; y = y / l; z = z / l;
}

AA_HD void cross3(float ax, float ay, float az, float bx, float by, float bz, float& cx, float& cy, float& cz) {
  cx = ay * bz - az * by;
  cy = az * bx - ax * bz;
  cz = ax * by - ay * bx;
}

// the affine part of a row-major 4x4 on a point (w = 1, no perspective division)
AA_HD void xform(const float* m, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
  oy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  oz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

// signed distance of p to a representative plane
AA_HD float plane_dist(float rx, float ry, float rz, float rd, float px, float py, float pz) { return dot3(rx, ry, rz, px, py, pz) + rd; }

// Cluster::check (planeExtract.h:31-36)
AA_HD bool check(float rx, float ry, float rz, float rd, float nx, float ny, float nz, float px, float py, float pz, float nthr, float dthr) {
  const float d_norm = dot3(nx, ny, nz, rx, ry, rz);
  const float d_dist = fabsf(plane_dist(rx, ry, rz, rd, px, py, pz));
  return d_norm > nthr && d_dist < dthr;
}

// Cluster::Cluster(init) (planeExtract.h:14-20)
AA_HD void found(Cluster& c, float nx, float ny, float nz, float px, float py, float pz) {
  c.rep[0] = nx; c.rep[1] = ny; c.rep[2] = nz; c.rep[3] = -dot3(nx, ny, nz, px, py, pz);
  c.sn[0] = nx; c.sn[1] = ny; c.sn[2] = nz;
  c.sp[0] = px; c.sp[1] = py; c.sp[2] = pz;
  c.count = 1;
}

// Cluster::addPoint (planeExtract.h:21-29)
AA_HD void join(Cluster& c, float nx, float ny, float nz, float px, float py, float pz) {
  c.sn[0] = c.sn[0] + nx; c.sn[1] = c.sn[1] + ny; c.sn[2] = c.sn[2] + nz;
  c.sp[0] = c.sp[0] + px; c.sp[1] = c.sp[1] + py; c.sp[2] = c.sp[2] + pz;
  c.count = c.count + 1;
  float rx = c.sn[0], ry = c.sn[1], rz = c.sn[2];
  normalize3(rx, ry, rz);
  const float k = (float)c.count;
  const float mx = c.sp[0] / k, my = c.sp[1] / k, mz = c.sp[2] / k;
  c.rep[0] = rx; c.rep[1] = ry; c.rep[2] = rz; c.rep[3] = -dot3(rx, ry, rz, mx, my, mz);
}

}  // namespace aa
}  // namespace sf
