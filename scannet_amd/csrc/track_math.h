// track_math.h -- the per-pixel rules the camera tracker (track.hip) and the global alignment (align.hip) share: metres from a u16 frame, the 2x2
// reduction, camera-space vertices and normals, the correspondence rule, the point-to-plane row with its 29 values and their reduction over a 256-pixel
// workgroup; and the host's side of a Gauss-Newton step: the level camera, the Cholesky solve, the pose update and its acceptance
// (DESIGN.md "Camera tracking" and "Global alignment").  Every operation is written as the specification states it; nothing here contracts.
#ifndef SCANFUSE_TRACK_MATH_H
#define SCANFUSE_TRACK_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "fuser_internal.h"

namespace tk {

constexpr int TK_MAX_LEVELS = 4;
constexpr int TK_NSYS = 29;         // 21 of J^T J, 6 of J^T r, sum r^2, count
constexpr int TK_NSYS_RGBD = 31;    // the 29, then the colour term's sum r_c^2 and count (photo_math.h)
template <bool COLOUR>
constexpr int nsys_of = COLOUR ? TK_NSYS_RGBD : TK_NSYS;   // the values of a solver kernel's instantiation
constexpr int TK_PSTRIDE = 32;      // floats per workgroup partial
constexpr float TK_DOWN_THRES = 0.03f;   // 2x2 reduction: depths within this many metres of the reference pixel's are averaged
constexpr double TK_PIVOT_REL = 1e-5;     // a Cholesky pivot at or below this share of its diagonal entry counts as non-positive

struct Cam {
  int W, H;
  float fx, fy, mx, my;
};
struct Rows {
  float T[12];   // rows 0..2 of a rigid transform
};

__device__ inline float3 xf(const Rows& R, float3 v) {
  return make_float3(fmaf(R.T[2], v.z, fmaf(R.T[1], v.y, fmaf(R.T[0], v.x, R.T[3]))), fmaf(R.T[6], v.z, fmaf(R.T[5], v.y, fmaf(R.T[4], v.x, R.T[7]))),
                     fmaf(R.T[10], v.z, fmaf(R.T[9], v.y, fmaf(R.T[8], v.x, R.T[11]))));
}
__device__ inline float3 rot(const Rows& R, float3 n) {
  return make_float3(fmaf(R.T[2], n.z, fmaf(R.T[1], n.y, R.T[0] * n.x)), fmaf(R.T[6], n.z, fmaf(R.T[5], n.y, R.T[4] * n.x)),
                     fmaf(R.T[10], n.z, fmaf(R.T[9], n.y, R.T[8] * n.x)));
}
__device__ inline float dot3(float3 a, float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline float3 cross3(float3 a, float3 b) { return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ inline float3 unproject(const Cam& c, int x, int y, float d) {
  return make_float3(((float)x - c.mx) / c.fx * d, ((float)y - c.my) / c.fy * d, d);
}

// pixel i of the integration image in metres, from a u16 frame at the input size: k_prepass's rule (nearest resample, then the depth range)
__device__ inline float depth0_at(const uint16_t* __restrict__ in, const ParamsK& P, int i) {
  uint16_t u;
  if (P.inW > 0) {
    const unsigned xi = (unsigned)((float)(i % P.W) * P.rsx + 0.5f), yi = (unsigned)((float)(i / P.W) * P.rsy + 0.5f);
    u = (xi < (unsigned)P.inW && yi < (unsigned)P.inH) ? in[(size_t)yi * P.inW + xi] : (uint16_t)0;
  } else {
    u = in[i];
  }
  float v = (float)u / P.depth_shift;
  if (u == 0 || v < P.dmin || v > P.dmax) v = -INFINITY;
  return v;
}

// one 2x2 reduction: the mean of the valid depths of the block within TK_DOWN_THRES of its top-left (reference) pixel s00, in the order
// (0,0), (1,0), (0,1), (1,1); invalid where the reference pixel is
__device__ inline float down4(float s00, float s10, float s01, float s11) {
  float out = -INFINITY;
  if (s00 > 0.0f) {
    const float v[4] = {s00, s10, s01, s11};
    float sum = 0.0f, cnt = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (v[k] > 0.0f && fabsf(v[k] - s00) <= TK_DOWN_THRES) {
        sum = sum + v[k];
        cnt = cnt + 1.0f;
      }
    out = sum / cnt;
  }
  return out;
}

// camera-space vertex and normal of pixel (x, y) with depth dz; dr, dd: the depths of (x + 1, y) and (x, y + 1), read only when both pixels exist
// (has_nb).  x = -inf where invalid.  Normal: cross(v(x, y+1) - v, v(x+1, y) - v) normalised
__device__ inline void vertex_normal(const Cam& c, int x, int y, float dz, bool has_nb, float dr, float dd, float4* vo, float4* no) {
  *vo = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
  *no = *vo;
  if (dz > 0.0f) {
    const float3 v = unproject(c, x, y, dz);
    *vo = make_float4(v.x, v.y, v.z, 0.0f);
    if (has_nb && dr > 0.0f && dd > 0.0f) {
      const float3 vr = unproject(c, x + 1, y, dr), vd = unproject(c, x, y + 1, dd);
      const float3 n = cross3(make_float3(vd.x - v.x, vd.y - v.y, vd.z - v.z), make_float3(vr.x - v.x, vr.y - v.y, vr.z - v.z));
      const float len = sqrtf(dot3(n, n));
      if (len > 0.0f) *no = make_float4(n.x / len, n.y / len, n.z / len, 0.0f);
    }
  }
}

// the 29 values of one correspondence: world point p, model normal nm, d = p - q.  J = (p x nm, nm), r = nm . d.  (acc may be longer: the colour term's
// two sums follow the 29, align_colour.hip)
template <int N>
__device__ inline void row29(float3 p, float3 nm, float3 d, float (&acc)[N]) {
  static_assert(N >= TK_NSYS, "the row has TK_NSYS values");
  const float r = dot3(nm, d);
  const float3 c = cross3(p, nm);
  const float J[6] = {c.x, c.y, c.z, nm.x, nm.y, nm.z};
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = a; b < 6; b++) acc[k++] = J[a] * J[b];
#pragma unroll
  for (int a = 0; a < 6; a++) acc[21 + a] = J[a] * r;
  acc[27] = r * r;
  acc[28] = 1.0f;
}

// one source pixel (camera-space vertex v4, normal n4) against a target: T the source's pose, M the source in the target's camera, c that camera at the
// level.  target(ux, uy, &q, &nm) looks up the world point and normal of target pixel (ux, uy) and returns false where it has none.  Fills acc and
// returns true where the pixel is a correspondence
template <typename Target, int N>
__device__ inline bool correspond(const Cam& c, const Rows& T, const Rows& M, float4 v4, float4 n4, float dist_thres, float normal_thres, Target target,
                                  float (&acc)[N]) {
  if (v4.z > 0.0f && n4.x > -INFINITY) {
    const float3 v = make_float3(v4.x, v4.y, v4.z);
    const float3 p = xf(T, v), n = rot(T, make_float3(n4.x, n4.y, n4.z));
    const float3 pc = xf(M, v);
    if (pc.z > 0.0f) {
      const float ux = floorf(fmaf(pc.x / pc.z, c.fx, c.mx) + 0.5f), uy = floorf(fmaf(pc.y / pc.z, c.fy, c.my) + 0.5f);
      if (ux >= 0.0f && ux < (float)c.W && uy >= 0.0f && uy < (float)c.H) {
        float3 q, nm;
        if (target((int)ux, (int)uy, &q, &nm)) {
          const float3 d = make_float3(p.x - q.x, p.y - q.y, p.z - q.z);
          if (sqrtf(dot3(d, d)) <= dist_thres && dot3(nm, n) >= normal_thres) {
            row29(p, nm, d, acc);
            return true;
          }
        }
      }
    }
  }
  return false;
}

// the workgroup's 256 lanes reduced to one N-float partial (N = 29; 31 with the colour term's two sums, align_colour.hip): xor butterfly 32 .. 1 within
// the wave (every lane ends with the wave's sum: a + b and b + a are the same float), (w0 + w1) + (w2 + w3) across the four waves.  No atomics.
template <int N>
__device__ inline void reduce256(float (&acc)[N], float (&red)[4][N], float* __restrict__ partial) {
  static_assert(N <= TK_PSTRIDE, "a partial holds TK_PSTRIDE floats");
#pragma unroll
  for (int k = 0; k < N; k++)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc[k] = acc[k] + __shfl_xor(acc[k], off);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < N; k++) red[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    partial[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// value k of nb workgroup partials summed in index order, in double
__device__ inline double sum_partials(const float* __restrict__ partials, int nb, int k) {
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < nb; b++) s += (double)partials[(size_t)b * TK_PSTRIDE + k];
  return s;
}

// ---- host, double: shared by the two solvers ---------------------------------------------------------------------------------------------------

// the camera of level l: (W >> l) x (H >> l) with the ray caster's scaled intrinsics; false below 8 x 8
inline bool level_cam(const ParamsK& P, int l, Cam* c) {
  c->W = P.W >> l;
  c->H = P.H >> l;
  const float sx = (float)c->W / (float)P.W, sy = (float)c->H / (float)P.H;
  c->fx = P.fx * sx; c->mx = P.mx * sx;
  c->fy = P.fy * sy; c->my = P.my * sy;
  return c->W >= 8 && c->H >= 8;
}

// A x = -b for the symmetric N x N system A (row-major, full) by Cholesky in double, sums in index order; false at a pivot <= TK_PIVOT_REL x its diagonal entry
inline bool solve_spd(const double* A, const double* b, int N, double* x) {
  std::vector<double> L((size_t)N * N, 0.0), y(N);
  for (int j = 0; j < N; j++) {
    double s = A[(size_t)j * N + j];
    for (int m = 0; m < j; m++) s -= L[(size_t)j * N + m] * L[(size_t)j * N + m];
    if (!(s > TK_PIVOT_REL * A[(size_t)j * N + j])) return false;
    L[(size_t)j * N + j] = std::sqrt(s);
    for (int i = j + 1; i < N; i++) {
      double e = A[(size_t)i * N + j];
      for (int m = 0; m < j; m++) e -= L[(size_t)i * N + m] * L[(size_t)j * N + m];
      L[(size_t)i * N + j] = e / L[(size_t)j * N + j];
    }
  }
  for (int i = 0; i < N; i++) {
    double e = -b[i];
    for (int m = 0; m < i; m++) e -= L[(size_t)i * N + m] * y[m];
    y[i] = e / L[(size_t)i * N + i];
  }
  for (int i = N - 1; i >= 0; i--) {
    double e = y[i];
    for (int m = i + 1; m < N; m++) e -= L[(size_t)m * N + i] * x[m];
    x[i] = e / L[(size_t)i * N + i];
  }
  return true;
}

// the inverse of the 3x3 block of a pose's rows (doubles or floats, four to a row): cofactors over the determinant, as the oracle's frame set-up
template <typename F>
inline void inverse3(const F* A, double* inv) {
  const double a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[4], a11 = A[5], a12 = A[6], a20 = A[8], a21 = A[9], a22 = A[10];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  inv[0] = c00 / det; inv[1] = (a02 * a21 - a01 * a22) / det; inv[2] = (a01 * a12 - a02 * a11) / det;
  inv[3] = c01 / det; inv[4] = (a00 * a22 - a02 * a20) / det; inv[5] = (a02 * a10 - a00 * a12) / det;
  inv[6] = c02 / det; inv[7] = (a01 * a20 - a00 * a21) / det; inv[8] = (a00 * a11 - a01 * a10) / det;
}

// T_ref^-1 (inverse3) composed with T, in double: rounded to float once
inline void compose_ref(const double* Tref, const double* T, float* M) {
  double inv[9];
  inverse3(Tref, inv);
  const double dt[3] = {T[3] - Tref[3], T[7] - Tref[7], T[11] - Tref[11]};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[4 * r + c] = (float)((inv[3 * r] * T[c] + inv[3 * r + 1] * T[4 + c]) + inv[3 * r + 2] * T[8 + c]);
    M[4 * r + 3] = (float)((inv[3 * r] * dt[0] + inv[3 * r + 1] * dt[1]) + inv[3 * r + 2] * dt[2]);
  }
}

// T <- [Rodrigues(omega) | t] T, xi = (omega, t)
inline void apply_update(const double* xi, double* T) {
  const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
  const double th = std::sqrt((w0 * w0 + w1 * w1) + w2 * w2);
  double a = 1.0, b = 0.5;
  if (th >= 1e-8) {
    a = std::sin(th) / th;
    b = (1.0 - std::cos(th)) / (th * th);
  }
  const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  double R[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
      R[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + b * k2;
    }
  double out[12];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 4; j++) out[4 * i + j] = (R[i][0] * T[j] + R[i][1] * T[4 + j]) + R[i][2] * T[8 + j];
    out[4 * i + 3] += xi[3 + i];
  }
  for (int i = 0; i < 12; i++) T[i] = out[i];
}

// the distance of T from G as the motion bounds measure it: metres between the origins, the angle of R_G^T R_T from its trace
inline void motion(const double* G, const double* T, double* dist, double* ang) {
  const double dt[3] = {T[3] - G[3], T[7] - G[7], T[11] - G[11]};
  *dist = std::sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
  double tr = 0.0;   // trace(R_G^T R_T)
  for (int i = 0; i < 3; i++) tr += (G[i] * T[i] + G[4 + i] * T[4 + i]) + G[8 + i] * T[8 + i];
  *ang = std::acos(std::fmin(1.0, std::fmax(-1.0, (tr - 1.0) * 0.5)));
}

inline bool finite12(const float* T) {
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(T[i])) return false;
  return true;
}

// a solved pose T is taken when all of it is finite and it lies within both motion bounds of where it started, T0
inline bool accept_pose(const double* T0, const double* T, double max_t, double max_r) {
  double dist, ang;
  motion(T0, T, &dist, &ang);
  bool fin = true;
  for (int i = 0; i < 12; i++) fin = fin && std::isfinite(T[i]);
  return fin && dist <= max_t && ang <= max_r;
}

inline void write_pose16(const double* T, float* out) {
  for (int i = 0; i < 12; i++) out[i] = (float)T[i];
  out[12] = out[13] = out[14] = 0.0f;
  out[15] = 1.0f;
}

}  // namespace tk

#endif
