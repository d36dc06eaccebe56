/* object_voxels_checker.c -- DESIGN.md section 4n by brute force, for tests/test_object_voxels.py and tests/test_object_voxels_gpu.py: every face of an
 * object against every cell of its cube, one object after the other, no lists and no bit masks.  Written from the design text, not from the
 * library's header.  Built with gcc -O2 -ffp-contract=off: every float operation below is one binary32 operation. */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef long long i64;

static int is_finite(float v) { return v == v && v != INFINITY && v != -INFINITY; }

/* the object of a face: the value two vertices share, else the first vertex's */
static uint32_t object_of(const uint32_t* tri, const uint32_t* vobj) {
  const uint32_t a = vobj[tri[0]], b = vobj[tri[1]], c = vobj[tri[2]];
  return b == c ? b : a;
}

/* is the face one that widens its object's box: no repeated index, nine finite coordinates */
static int counted(const uint32_t* tri, const float* xyz) {
  if (tri[0] == tri[1] || tri[0] == tri[2] || tri[1] == tri[2]) return 0;
  for (int v = 0; v < 3; v++)
    for (int a = 0; a < 3; a++)
      if (!is_finite(xyz[3 * (i64)tri[v] + a])) return 0;
  return 1;
}

static i64 quant(float v, float o, float scale, int dim) {
  float r = rintf((v - o) * scale);   /* the default rounding mode: to nearest, ties to even */
  const float top = (float)(256 * dim);
  if (!(r >= 0.0f)) r = 0.0f;         /* a NaN goes to 0 as well */
  if (r > top) r = top;
  return (i64)r;
}

/* does the axis L separate the triangle (vertices relative to the cell's centre) from the cell of half edge 128? */
static int separates(const i64 L[3], i64 v[3][3]) {
  i64 lo = 0, hi = 0;
  for (int i = 0; i < 3; i++) {
    const i64 p = L[0] * v[i][0] + L[1] * v[i][1] + L[2] * v[i][2];
    if (i == 0 || p < lo) lo = p;
    if (i == 0 || p > hi) hi = p;
  }
  const i64 r = 128 * (llabs(L[0]) + llabs(L[1]) + llabs(L[2]));
  return lo > r || hi < -r;
}

static void cross(const i64 a[3], const i64 b[3], i64 out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}

/* closed triangle against closed cell: 3 cell axes, the normal, 9 edge x axis products */
static int meets(i64 q[3][3], int i, int j, int k) {
  const i64 centre[3] = {256 * (i64)i + 128, 256 * (i64)j + 128, 256 * (i64)k + 128};
  i64 v[3][3], e[3][3], L[3];
  for (int n = 0; n < 3; n++)
    for (int a = 0; a < 3; a++) v[n][a] = q[n][a] - centre[a];
  for (int a = 0; a < 3; a++) {
    const i64 unit[3] = {a == 0, a == 1, a == 2};
    if (separates(unit, v)) return 0;
  }
  for (int a = 0; a < 3; a++) { e[0][a] = v[1][a] - v[0][a]; e[1][a] = v[2][a] - v[1][a]; e[2][a] = v[0][a] - v[2][a]; }
  cross(e[0], e[1], L);
  if (separates(L, v)) return 0;
  for (int n = 0; n < 3; n++)
    for (int a = 0; a < 3; a++) {
      const i64 unit[3] = {a == 0, a == 1, a == 2};
      cross(e[n], unit, L);
      if (separates(L, v)) return 0;
    }
  return 1;
}

/* -> how many objects are kept; the first `capacity` of them are written.  gdims == NULL: no grid. */
i64 ovc_voxelize(const float* xyz, const uint32_t* tris, i64 nf, const uint32_t* vobj, const int32_t* cls, int32_t nobj, int dim, int fit, int min_faces,
                 int all_objects, const int32_t* gdims, const int32_t* glo, float voxel, const uint8_t* weight, i64 capacity, uint8_t* data, uint8_t* label,
                 int32_t* object_id, float* origin, float* cell) {
  i64 kept = 0;
  const i64 cells = (i64)dim * dim * dim;
  for (int32_t id = 0; id < nobj; id++) {
    if (cls[id] < 0 && !all_objects) continue;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    i64 faces = 0;
    for (i64 f = 0; f < nf; f++) {
      const uint32_t* tri = tris + 3 * f;
      if (object_of(tri, vobj) != (uint32_t)id + 1 || !counted(tri, xyz)) continue;
      faces++;
      for (int v = 0; v < 3; v++)
        for (int a = 0; a < 3; a++) {
          const float x = xyz[3 * (i64)tri[v] + a];
          if (x < lo[a]) lo[a] = x;
          if (x > hi[a]) hi[a] = x;
        }
    }
    if (faces < 1 || faces < min_faces) continue;
    float e = hi[0] - lo[0];
    if (hi[1] - lo[1] > e) e = hi[1] - lo[1];
    if (hi[2] - lo[2] > e) e = hi[2] - lo[2];
    const float c = e / (float)fit;
    const float scale = 256.0f / c;
    if (!(is_finite(e) && e > 0.0f && is_finite(c) && c > 0.0f && is_finite(scale) && scale > 0.0f)) continue;
    float o[3];
    for (int a = 0; a < 3; a++) {
      const float m = (lo[a] + hi[a]) * 0.5f;
      o[a] = m - ((float)dim * 0.5f) * c;
    }
    if (kept < capacity) {
      uint8_t* occ = data + kept * 2 * cells;
      uint8_t* known = occ + cells;
      memset(occ, 0, (size_t)cells);
      for (i64 f = 0; f < nf; f++) {
        const uint32_t* tri = tris + 3 * f;
        if (object_of(tri, vobj) != (uint32_t)id + 1 || !counted(tri, xyz)) continue;
        i64 q[3][3], u[3], w[3], n[3];
        for (int v = 0; v < 3; v++)
          for (int a = 0; a < 3; a++) q[v][a] = quant(xyz[3 * (i64)tri[v] + a], o[a], scale, dim);
        for (int a = 0; a < 3; a++) { u[a] = q[1][a] - q[0][a]; w[a] = q[2][a] - q[0][a]; }
        cross(u, w, n);
        if (n[0] == 0 && n[1] == 0 && n[2] == 0) continue;   /* no area after quantisation */
        i64 qlo[3], qhi[3];
        for (int a = 0; a < 3; a++) {
          qlo[a] = qhi[a] = q[0][a];
          for (int v = 1; v < 3; v++) { if (q[v][a] < qlo[a]) qlo[a] = q[v][a]; if (q[v][a] > qhi[a]) qhi[a] = q[v][a]; }
        }
        /* every cell; a layer, a row or a cell whose closed interval the triangle's extent misses is apart along that cell axis already */
        for (int k = 0; k < dim; k++) {
          if (qhi[2] < 256 * k || qlo[2] > 256 * k + 256) continue;
          for (int j = 0; j < dim; j++) {
            if (qhi[1] < 256 * j || qlo[1] > 256 * j + 256) continue;
            for (int i = 0; i < dim; i++) {
              if (qhi[0] < 256 * i || qlo[0] > 256 * i + 256) continue;
              if (meets(q, i, j, k)) occ[((i64)k * dim + j) * dim + i] = 1;
            }
          }
        }
      }
      for (int k = 0; k < dim; k++)
        for (int j = 0; j < dim; j++)
          for (int i = 0; i < dim; i++) {
            const i64 at = ((i64)k * dim + j) * dim + i;
            uint8_t seen = 1;
            if (gdims) {
              const int idx[3] = {i, j, k};
              i64 node[3];
              int inside = 1;
              for (int a = 0; a < 3; a++) {
                const float p = o[a] + ((float)idx[a] + 0.5f) * c;
                const float g = floorf(p / voxel - (float)glo[a] + 0.5f);
                if (!(g >= 0.0f && g < (float)gdims[a])) inside = 0;   /* decided in float */
                else node[a] = (i64)g;
              }
              seen = inside && weight[(node[2] * gdims[1] + node[1]) * gdims[0] + node[0]] > 0;
            }
            known[at] = (seen || occ[at]) ? 1 : 0;
          }
      label[kept] = cls[id] < 0 ? 255 : (uint8_t)cls[id];
      object_id[kept] = id;
      for (int a = 0; a < 3; a++) origin[3 * kept + a] = o[a];
      cell[kept] = c;
    }
    kept++;
  }
  return kept;
}
