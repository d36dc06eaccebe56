// voxel_labels_internal.h -- the rule of DESIGN.md section 4m as the host path (voxel_labels.cpp) and the kernels (voxel_labels.hip) share it: the record of a
// face (everything that depends on the face alone), the squared distance of a point to it, and the range of 8-node tiles a grown box touches.  Every
// operation is one binary32 operation, rounded by itself (-ffp-contract=off; no fmaf here); divisions are IEEE divisions on both sides.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/scanfuse.h"

#if defined(__HIPCC__)
#define VL_HD __host__ __device__ inline
#else
#define VL_HD inline
#endif

namespace sf {
namespace vl {

constexpr int TILE = 8;             // nodes per tile edge
constexpr int32_t MAX_COORD = 1 << 22;   // |lo_voxel| + n per axis: node coordinates stay exact in binary32 and a tile range is safe with one node of slack

struct FaceRec {   // 80 bytes: five 16-byte loads
  float ax, ay, az;      // vertex a
  float ux, uy, uz;      // ab = b - a
  float vx, vy, vz;      // ac = c - a
  float e00, e01, e11;   // ab.ab, ab.ac, ac.ac
  float lox, loy, loz;   // min(a, b, c) - t, t = band * voxel_size
  float hix, hiy, hiz;   // max(a, b, c) + t
  int32_t f;             // the face's index
  int32_t valid;         // 0: the face is skipped everywhere
};
static_assert(sizeof(FaceRec) == 80, "FaceRec is five float4");

VL_HD bool finite32(float v) { return fabsf(v) <= FLT_MAX; }   // false for NaN

VL_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// indices are below the vertex count (checked by the caller)
VL_HD FaceRec make_record(const float* xyz, const uint32_t* tris, uint64_t f, float t) {
  FaceRec r;
  const uint32_t i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
  const float ax = xyz[3 * (uint64_t)i0], ay = xyz[3 * (uint64_t)i0 + 1], az = xyz[3 * (uint64_t)i0 + 2];
  const float bx = xyz[3 * (uint64_t)i1], by = xyz[3 * (uint64_t)i1 + 1], bz = xyz[3 * (uint64_t)i1 + 2];
  const float cx = xyz[3 * (uint64_t)i2], cy = xyz[3 * (uint64_t)i2 + 1], cz = xyz[3 * (uint64_t)i2 + 2];
  bool ok = i0 != i1 && i0 != i2 && i1 != i2;
  ok = ok && finite32(ax) && finite32(ay) && finite32(az) && finite32(bx) && finite32(by) && finite32(bz) && finite32(cx) && finite32(cy) && finite32(cz);
  r.ax = ax; r.ay = ay; r.az = az;
  r.ux = bx - ax; r.uy = by - ay; r.uz = bz - az;
  r.vx = cx - ax; r.vy = cy - ay; r.vz = cz - az;
  r.e00 = dot3(r.ux, r.uy, r.uz, r.ux, r.uy, r.uz);
  r.e01 = dot3(r.ux, r.uy, r.uz, r.vx, r.vy, r.vz);
  r.e11 = dot3(r.vx, r.vy, r.vz, r.vx, r.vy, r.vz);
  const float det = r.e00 * r.e11 - r.e01 * r.e01;   // zero length, collinear (as binary32 sees it) or too large to square: no face
  ok = ok && det > 0.0f && det <= FLT_MAX;
  r.lox = fminf(fminf(ax, bx), cx) - t; r.loy = fminf(fminf(ay, by), cy) - t; r.loz = fminf(fminf(az, bz), cz) - t;
  r.hix = fmaxf(fmaxf(ax, bx), cx) + t; r.hiy = fmaxf(fmaxf(ay, by), cy) + t; r.hiz = fmaxf(fmaxf(az, bz), cz) + t;
  r.f = (int32_t)f;
  r.valid = ok ? 1 : 0;
  return r;
}

VL_HD bool in_box(const FaceRec& r, float px, float py, float pz) {
  return px >= r.lox && px <= r.hix && py >= r.loy && py <= r.hiy && pz >= r.loz && pz <= r.hiz;
}

// Ericson, Real-Time Collision Detection 5.1.5, the regions in the book's order; the closest point is a + s ab + t ac
VL_HD float dist2(const FaceRec& r, float px, float py, float pz) {
  const float wx = px - r.ax, wy = py - r.ay, wz = pz - r.az;
  const float d1 = dot3(r.ux, r.uy, r.uz, wx, wy, wz);
  const float d2 = dot3(r.vx, r.vy, r.vz, wx, wy, wz);
  const float d3 = d1 - r.e00, d4 = d2 - r.e01, d5 = d1 - r.e01, d6 = d2 - r.e11;
  float s, t;
  if (d1 <= 0.0f && d2 <= 0.0f) {                          // vertex a
    s = 0.0f; t = 0.0f;
  } else if (d3 >= 0.0f && d4 <= d3) {                     // vertex b
    s = 1.0f; t = 0.0f;
  } else {
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {          // edge ab
      const float inv = 1.0f / (d1 - d3);
      s = d1 * inv; t = 0.0f;
    } else if (d6 >= 0.0f && d5 <= d6) {                   // vertex c
      s = 0.0f; t = 1.0f;
    } else {
      const float vb = d5 * d2 - d1 * d6;
      if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {        // edge ac
        const float inv = 1.0f / (d2 - d6);
        s = 0.0f; t = d2 * inv;
      } else {
        const float va = d3 * d6 - d5 * d4;
        const float m = d4 - d3, n = d5 - d6;
        if (va <= 0.0f && m >= 0.0f && n >= 0.0f) {        // edge bc
          const float inv = 1.0f / (m + n);
          t = m * inv; s = 1.0f - t;
        } else {                                           // interior
          const float inv = 1.0f / ((va + vb) + vc);
          s = vb * inv; t = vc * inv;
        }
      }
    }
  }
  const float rx = wx - (s * r.ux + t * r.vx);
  const float ry = wy - (s * r.uy + t * r.vy);
  const float rz = wz - (s * r.uz + t * r.vz);
  return (rx * rx + ry * ry) + rz * rz;
}

// is (d, f) a new winner over (best, best_f)?  d <= r2 < inf, so the first candidate always is
VL_HD bool better(float d, int32_t f, float r2, float best, int32_t best_f) { return d <= r2 && (d < best || (d == best && f < best_f)); }

VL_HD float node_pos(int32_t lo, int32_t i, float voxel) { return (float)(lo + i) * voxel; }

// The tiles along one axis that can hold a node p with blo <= p <= bhi: one node of slack either side covers the roundings of the two divisions and of
// node_pos while |lo| + n <= MAX_COORD.  Clamped in float before any conversion to int.  false: no tile.
VL_HD bool tile_range(float blo, float bhi, float voxel, int32_t lo, int32_t n, int32_t* t0, int32_t* t1) {
  const float flo = (float)lo, fn = (float)n;
  float g0 = floorf(blo / voxel - flo) - 1.0f;
  float g1 = ceilf(bhi / voxel - flo) + 1.0f;
  g0 = fminf(fmaxf(g0, 0.0f), fn);
  g1 = fminf(fmaxf(g1, -1.0f), fn - 1.0f);
  const int32_t x0 = (int32_t)g0, x1 = (int32_t)g1;
  if (x1 < x0) return false;
  *t0 = x0 / TILE;
  *t1 = x1 / TILE;
  return true;
}

struct Geo {
  int32_t nx, ny, nz;
  int32_t lox, loy, loz;
  int32_t tx, ty, tz;   // tiles per axis
  float voxel;
};

inline Geo make_geo(const sf_grid_header& h) {
  Geo g;
  g.nx = h.nx; g.ny = h.ny; g.nz = h.nz;
  g.lox = h.lo_voxel[0]; g.loy = h.lo_voxel[1]; g.loz = h.lo_voxel[2];
  g.tx = (h.nx + TILE - 1) / TILE; g.ty = (h.ny + TILE - 1) / TILE; g.tz = (h.nz + TILE - 1) / TILE;
  g.voxel = h.voxel_size;
  return g;
}

// what the bin stage hook hands back (any pointer may be null)
struct BinsOut {
  uint32_t* counts;     // per tile
  uint32_t* offsets;    // per tile: exclusive scan of counts
  int32_t* list;        // face indices, tile after tile; order within a tile is free
  uint64_t capacity;    // entries of list
  uint64_t* total;      // entries in all
};

// voxel_labels.hip.  Arguments are checked by the callers in voxel_labels.cpp.  face / dist2 / data / label / xy may be host or device memory.
int nearest_device(const sf_grid_header& h, const float* xyz, uint64_t nv, const uint32_t* tris, uint64_t nf, float t, float r2, int device, int32_t* face,
                   float* dist2, const BinsOut* bins);
int sample_device(const sf_grid_header& h, const float* value, const uint8_t* byte_label, int32_t wx, int32_t wy, int32_t wz, int64_t z0, int32_t stride,
                  int device, uint64_t first, uint64_t max_samples, float* data, uint8_t* label, int32_t* xy, uint64_t* total);

}  // namespace vl
}  // namespace sf
