// object_voxels_internal.h -- the rule of DESIGN.md section 4n as the host path (object_voxels.cpp) and the kernels (object_voxels.hip) share it: the object
// of a face, the cube of an object, the quantisation of a vertex, the exact triangle / cell overlap test, and the grid index of a cell centre.  Every
// float operation is one binary32 operation, rounded by itself (-ffp-contract=off; no fmaf here); everything after the quantisation is integer arithmetic.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/scanfuse.h"

#if defined(__HIPCC__)
#define OV_HD __host__ __device__ inline
#else
#define OV_HD inline
#endif

namespace sf {
namespace ov {

constexpr int32_t MAX_DIM = 32;                    // quantised coordinates stay within 0 .. 2^13
constexpr uint32_t MAX_OBJECT = 65536;             // the largest vertex_object value: objectId 65 535
constexpr int32_t MASK_WORDS = MAX_DIM * MAX_DIM * MAX_DIM / 32;   // the bit mask of one object at the largest dim: 4 KiB
constexpr uint32_t CHUNK = 256;                    // faces per raster workgroup

OV_HD bool finite32(float v) { return fabsf(v) <= FLT_MAX; }   // false for NaN

// The object of face f: the value two of its vertices share, else its first vertex's.  *counts: no index is repeated and every coordinate is finite --
// such a face widens its object's box and is counted.  Indices are below the vertex count (checked by the caller).
OV_HD uint32_t face_object(const float* xyz, const uint32_t* tris, const uint32_t* vertex_object, uint64_t f, bool* counts) {
  const uint32_t i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
  const uint32_t oa = vertex_object[i0], ob = vertex_object[i1], oc = vertex_object[i2];
  bool ok = i0 != i1 && i0 != i2 && i1 != i2;
  const float* a = xyz + 3 * (uint64_t)i0;
  const float* b = xyz + 3 * (uint64_t)i1;
  const float* c = xyz + 3 * (uint64_t)i2;
  ok = ok && finite32(a[0]) && finite32(a[1]) && finite32(a[2]) && finite32(b[0]) && finite32(b[1]) && finite32(b[2]) && finite32(c[0]) && finite32(c[1]) &&
       finite32(c[2]);
  *counts = ok;
  return ob == oc ? ob : oa;
}

struct Cube {
  float ox, oy, oz;   // the corner of cell (0, 0, 0)
  float c;            // the cell's edge
  float scale;        // 256 / c
  int32_t valid;      // e, c and scale are finite and positive
};

// lo / hi: per-axis min / max over the vertices of the object's counted faces (+inf / -inf without one: not valid)
OV_HD Cube make_cube(float lox, float loy, float loz, float hix, float hiy, float hiz, int32_t dim, int32_t fit) {
  Cube q;
  const float e = fmaxf(fmaxf(hix - lox, hiy - loy), hiz - loz);
  const float c = e / (float)fit;
  const float half = (float)dim * 0.5f;
  q.ox = (lox + hix) * 0.5f - half * c;
  q.oy = (loy + hiy) * 0.5f - half * c;
  q.oz = (loz + hiz) * 0.5f - half * c;
  q.c = c;
  q.scale = 256.0f / c;
  q.valid = (e > 0.0f && finite32(e) && c > 0.0f && finite32(c) && q.scale > 0.0f && finite32(q.scale)) ? 1 : 0;
  return q;
}

// 1/256 cells from the cube's corner, to nearest (ties to even), clamped in float to 0 .. 256 dim; a NaN (an origin that overflowed) becomes 0
OV_HD int32_t quantise(float v, float o, float scale, int32_t dim) {
  const float r = rintf((v - o) * scale);
  return (int32_t)fminf(fmaxf(r, 0.0f), (float)(256 * dim));
}

struct QTri {   // a quantised triangle
  int32_t ax, ay, az, bx, by, bz, cx, cy, cz;
};

OV_HD QTri quantise_face(const float* xyz, const uint32_t* tris, uint64_t f, const Cube& q, int32_t dim) {
  const float* a = xyz + 3 * (uint64_t)tris[3 * f];
  const float* b = xyz + 3 * (uint64_t)tris[3 * f + 1];
  const float* c = xyz + 3 * (uint64_t)tris[3 * f + 2];
  QTri t;
  t.ax = quantise(a[0], q.ox, q.scale, dim); t.ay = quantise(a[1], q.oy, q.scale, dim); t.az = quantise(a[2], q.oz, q.scale, dim);
  t.bx = quantise(b[0], q.ox, q.scale, dim); t.by = quantise(b[1], q.oy, q.scale, dim); t.bz = quantise(b[2], q.oz, q.scale, dim);
  t.cx = quantise(c[0], q.ox, q.scale, dim); t.cy = quantise(c[1], q.oy, q.scale, dim); t.cz = quantise(c[2], q.oz, q.scale, dim);
  return t;
}

// no area after quantisation: the cross product of two edges is the zero vector (components below 2^27)
OV_HD bool no_area(const QTri& t) {
  const int32_t ux = t.bx - t.ax, uy = t.by - t.ay, uz = t.bz - t.az, vx = t.cx - t.ax, vy = t.cy - t.ay, vz = t.cz - t.az;
  return (uy * vz - uz * vy) == 0 && (uz * vx - ux * vz) == 0 && (ux * vy - uy * vx) == 0;
}

OV_HD int32_t min3(int32_t a, int32_t b, int32_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
OV_HD int32_t max3(int32_t a, int32_t b, int32_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
OV_HD int32_t iabs(int32_t a) { return a < 0 ? -a : a; }

// the closed cells [256 i, 256 i + 256] that the closed interval [qlo, qhi] meets, within 0 .. dim - 1 (never empty: 0 <= qlo <= qhi <= 256 dim)
OV_HD void cell_range(int32_t qlo, int32_t qhi, int32_t dim, int32_t* i0, int32_t* i1) {
  const int32_t a = (qlo - 1) >> 8, b = qhi >> 8;
  *i0 = a < 0 ? 0 : a;
  *i1 = b > dim - 1 ? dim - 1 : b;
}

// the projections p0, p1, p2 of the triangle on an axis against the cell's radius r on it: true when the axis separates them
OV_HD bool apart(int32_t p0, int32_t p1, int32_t p2, int32_t r) { return min3(p0, p1, p2) > r || max3(p0, p1, p2) < -r; }

// the three axes edge x (1,0,0), edge x (0,1,0), edge x (0,0,1) of one edge (ex, ey, ez); the vertices are relative to the cell's centre, the cell's half
// edge is 128.  Products stay below 2^27, sums below 2^28.
OV_HD bool edge_apart(int32_t ex, int32_t ey, int32_t ez, int32_t x0, int32_t y0, int32_t z0, int32_t x1, int32_t y1, int32_t z1, int32_t x2, int32_t y2, int32_t z2) {
  const int32_t fx = iabs(ex), fy = iabs(ey), fz = iabs(ez);
  if (apart(ez * y0 - ey * z0, ez * y1 - ey * z1, ez * y2 - ey * z2, 128 * (fz + fy))) return true;
  if (apart(ex * z0 - ez * x0, ex * z1 - ez * x1, ex * z2 - ez * x2, 128 * (fz + fx))) return true;
  return apart(ey * x0 - ex * y0, ey * x1 - ex * y1, ey * x2 - ex * y2, 128 * (fy + fx));
}

// Does the closed triangle meet the closed cell (i, j, k) as point sets?  The separating-axis test over the 3 cell axes, the face normal and the 9
// edge x axis products: exact in integers for a triangle with area (Akenine-Moller's test with closed comparisons).
OV_HD bool meets(const QTri& t, int32_t i, int32_t j, int32_t k) {
  const int32_t mx = 256 * i + 128, my = 256 * j + 128, mz = 256 * k + 128;
  const int32_t x0 = t.ax - mx, y0 = t.ay - my, z0 = t.az - mz;
  const int32_t x1 = t.bx - mx, y1 = t.by - my, z1 = t.bz - mz;
  const int32_t x2 = t.cx - mx, y2 = t.cy - my, z2 = t.cz - mz;
  if (apart(x0, x1, x2, 128) || apart(y0, y1, y2, 128) || apart(z0, z1, z2, 128)) return false;
  const int32_t e0x = x1 - x0, e0y = y1 - y0, e0z = z1 - z0;
  const int32_t e1x = x2 - x1, e1y = y2 - y1, e1z = z2 - z1;
  const int32_t e2x = x0 - x2, e2y = y0 - y2, e2z = z0 - z2;
  const int32_t nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;   // below 2^27 each
  const int64_t d = ((int64_t)nx * x0 + (int64_t)ny * y0) + (int64_t)nz * z0;                           // below 2^42
  const int64_t r = 128 * (((int64_t)iabs(nx) + (int64_t)iabs(ny)) + (int64_t)iabs(nz));
  if (d > r || d < -r) return false;
  if (edge_apart(e0x, e0y, e0z, x0, y0, z0, x1, y1, z1, x2, y2, z2)) return false;
  if (edge_apart(e1x, e1y, e1z, x0, y0, z0, x1, y1, z1, x2, y2, z2)) return false;
  return !edge_apart(e2x, e2y, e2z, x0, y0, z0, x1, y1, z1, x2, y2, z2);
}

// The grid node of a cell centre along one axis (include/scanfuse.h: g = w / voxel_size - lo_voxel + 0.5, floor): *in is decided in float, before any
// conversion (false for NaN); the index returned is clamped to the grid, so that a load with it is safe whenever n >= 1.
OV_HD int32_t grid_node(float o, float c, int32_t k, float voxel, int32_t lo, int32_t n, bool* in) {
  const float p = o + ((float)k + 0.5f) * c;
  const float g = floorf(p / voxel - (float)lo + 0.5f);
  *in = g >= 0.0f && g < (float)n;
  return (int32_t)fminf(fmaxf(g, 0.0f), (float)(n > 0 ? n - 1 : 0));
}

struct Kept {   // an object of the page being written
  uint32_t object;        // the vertex_object value: objectId + 1
  uint32_t label;
  uint32_t first, count;  // its faces in the list
  Cube cube;
};

struct GridRef {   // the known channel's source; mode 0: no grid (all ones), 1: weight[nz][ny][nx], 2: a grid without a node (nothing is inside)
  int32_t mode;
  int32_t nx, ny, nz;
  int32_t lox, loy, loz;
  float voxel;
  const uint8_t* weight;
};

// what the key / fill stage hands back (object_voxels.hip -> tests); any pointer may be null
struct StageOut {
  uint32_t* face_object;   // per face: its object, 0 where the face is not counted or has none
  uint32_t* counts;        // per vertex_object value 0 .. num_objects (entry 0 stays 0)
  uint32_t* offsets;       // exclusive scan of counts
  uint32_t* list;          // face indices, object after object; the order within an object is free
  uint64_t capacity;       // entries of list
  uint64_t* total;         // entries in all
};

// object_voxels.hip.  Arguments are checked by the callers in object_voxels.cpp.  The outputs may be host or device memory.
int voxelize_device(const float* xyz, uint64_t nv, const uint32_t* tris, uint64_t nf, const uint32_t* vertex_object, const int32_t* object_class,
                    uint32_t num_objects, const GridRef& grid, uint64_t grid_nodes, const sf_objvox_params& p, int device, uint64_t first, uint64_t max_objects,
                    uint8_t* data, uint8_t* label, int32_t* object_id, float* origin, float* cell, uint64_t* total, const StageOut* stage);

// is the object kept?  (shared by the plan, the host path and the device path's host side)
inline bool kept(const sf_objvox_params& p, int32_t cls, uint32_t faces, const Cube& q) {
  if (cls < 0 && !p.all_objects) return false;
  return q.valid && faces >= 1 && (int64_t)faces >= (int64_t)p.min_faces;
}
inline uint32_t label_of(int32_t cls) { return cls < 0 ? 255u : (uint32_t)cls; }

}  // namespace ov
}  // namespace sf
