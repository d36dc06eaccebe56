/* voxel_labels_checker.c -- DESIGN.md section 4m restated by brute force: every node against every face, no tiles, no bins, no records kept.  Written
 * from the section's text, not from the library's sources; built by the tests themselves (gcc -O2 -ffp-contract=off: every operation below is one
 * binary32 operation).  Arrays are [z][y][x], x fastest. */
#include <math.h>
#include <stdint.h>

static int finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

static float dot(const float* a, const float* b) {
  float s = a[0] * b[0];
  float u = a[1] * b[1];
  s = s + u;
  u = a[2] * b[2];
  return s + u;
}

/* 4m "the face": 0 when the face is skipped; else ab, ac, the three products, the grown box */
static int face_of(const float* xyz, const uint32_t* tri, float t, float* a, float* ab, float* ac, float* e, float* lo, float* hi) {
  if (tri[0] == tri[1] || tri[0] == tri[2] || tri[1] == tri[2]) return 0;
  const float* A = xyz + 3 * (uint64_t)tri[0];
  const float* B = xyz + 3 * (uint64_t)tri[1];
  const float* Cc = xyz + 3 * (uint64_t)tri[2];
  if (!finite3(A) || !finite3(B) || !finite3(Cc)) return 0;
  for (int k = 0; k < 3; k++) {
    a[k] = A[k];
    ab[k] = B[k] - A[k];
    ac[k] = Cc[k] - A[k];
    float mn = A[k] < B[k] ? A[k] : B[k];
    mn = mn < Cc[k] ? mn : Cc[k];
    float mx = A[k] > B[k] ? A[k] : B[k];
    mx = mx > Cc[k] ? mx : Cc[k];
    lo[k] = mn - t;
    hi[k] = mx + t;
  }
  e[0] = dot(ab, ab);
  e[1] = dot(ab, ac);
  e[2] = dot(ac, ac);
  float p = e[0] * e[2];
  float q = e[1] * e[1];
  float det = p - q;
  if (!(det > 0.0f) || !isfinite(det)) return 0;
  return 1;
}

/* 4m "the distance": the regions in the order A, B, AB, C, AC, BC, inside */
static float dist2_of(const float* a, const float* ab, const float* ac, const float* e, const float* p) {
  float w[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  float d1 = dot(ab, w), d2 = dot(ac, w);
  float d3 = d1 - e[0], d4 = d2 - e[1], d5 = d1 - e[1], d6 = d2 - e[2];
  float s, t;
  float vc = d1 * d4 - d3 * d2;
  float vb = d5 * d2 - d1 * d6;
  float va = d3 * d6 - d5 * d4;
  float m = d4 - d3, n = d5 - d6;
  if (d1 <= 0.0f && d2 <= 0.0f) {
    s = 0.0f; t = 0.0f;
  } else if (d3 >= 0.0f && d4 <= d3) {
    s = 1.0f; t = 0.0f;
  } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    float inv = 1.0f / (d1 - d3);
    s = d1 * inv; t = 0.0f;
  } else if (d6 >= 0.0f && d5 <= d6) {
    s = 0.0f; t = 1.0f;
  } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    float inv = 1.0f / (d2 - d6);
    s = 0.0f; t = d2 * inv;
  } else if (va <= 0.0f && m >= 0.0f && n >= 0.0f) {
    float inv = 1.0f / (m + n);
    t = m * inv; s = 1.0f - t;
  } else {
    float inv = 1.0f / ((va + vb) + vc);
    s = vb * inv; t = vc * inv;
  }
  float r[3];
  for (int k = 0; k < 3; k++) {
    float q = s * ab[k];
    float u = t * ac[k];
    q = q + u;
    r[k] = w[k] - q;
  }
  return dot(r, r);
}

/* face / dist2 of every node; dims = {nx, ny, nz}, lo = lo_voxel */
void vc_nearest(const int32_t* dims, const int32_t* lo, float voxel, const float* xyz, const uint32_t* tris, int64_t nf, float band, int32_t* face,
                float* dist2) {
  const float t = band * voxel;
  const float r2 = t * t;
  const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
  for (int64_t i = 0; i < n; i++) {
    face[i] = -1;
    dist2[i] = INFINITY;
  }
  for (int64_t f = 0; f < nf; f++) {
    float a[3], ab[3], ac[3], e[3], blo[3], bhi[3];
    if (!face_of(xyz, tris + 3 * f, t, a, ab, ac, e, blo, bhi)) continue;
    for (int32_t z = 0; z < dims[2]; z++) {
      float p[3];
      p[2] = (float)(lo[2] + z) * voxel;
      if (!(p[2] >= blo[2] && p[2] <= bhi[2])) continue;
      for (int32_t y = 0; y < dims[1]; y++) {
        p[1] = (float)(lo[1] + y) * voxel;
        if (!(p[1] >= blo[1] && p[1] <= bhi[1])) continue;
        for (int32_t x = 0; x < dims[0]; x++) {
          p[0] = (float)(lo[0] + x) * voxel;
          if (!(p[0] >= blo[0] && p[0] <= bhi[0])) continue;
          const float d = dist2_of(a, ab, ac, e, p);
          if (!(d <= r2)) continue;                   /* NaN and inf stay out */
          const int64_t i = ((int64_t)z * dims[1] + y) * dims[0] + x;
          /* faces come in ascending order: an equal distance keeps the earlier one */
          if (d < dist2[i]) {
            face[i] = (int32_t)f;
            dist2[i] = d;
          }
        }
      }
    }
  }
}

/* 4m "labels" */
void vc_labels(const int32_t* face, int64_t n, const uint32_t* tris, const uint16_t* vlabel, const uint8_t* vinst, uint16_t* label, uint8_t* inst,
               uint8_t* byte_label) {
  for (int64_t i = 0; i < n; i++) {
    label[i] = 0; inst[i] = 0; byte_label[i] = 0;
    if (face[i] < 0) continue;
    const uint32_t* v = tris + 3 * (int64_t)face[i];
    uint16_t l0 = vlabel[v[0]], l1 = vlabel[v[1]], l2 = vlabel[v[2]];
    uint16_t l = (l0 == l1 || l0 == l2) ? l0 : (l1 == l2 ? l1 : l0);
    label[i] = l;
    if (vinst) {
      uint8_t i0 = vinst[v[0]], i1 = vinst[v[1]], i2 = vinst[v[2]];
      inst[i] = (i0 == i1 || i0 == i2) ? i0 : (i1 == i2 ? i1 : i0);
    }
    byte_label[i] = (l == 0 || l > 254) ? 255 : (uint8_t)l;
  }
}
