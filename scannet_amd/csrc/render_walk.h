// render_walk.h -- the ONE statement of the mesh render's walk: the counter hash, the camera ray, the threaded tree's
// traversal, the triangle test, the bounce sampler and the path.  Every function is __host__ __device__ inline: k_render / k_render_rays
// (render.hip) and the host path (render_host.cpp, device = -1) compile the same text, and tests/render_checker.c restates it without a tree.
// The build passes -ffp-contract=off: nothing fuses but the fmaf() written here; `/` and sqrtf are correctly rounded on both sides.  No libm
// transcendental, no fminf / fmaxf (their NaN rules differ between targets): minima and maxima are written as comparisons.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/scanfuse.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RW_HD __host__ __device__ inline
#else
#define RW_HD inline
#endif

namespace rw {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr float BIG = 3.402823466e38f;   // FLT_MAX
constexpr int LEAF_MAX = 15;             // a leaf's triangle count lives in 4 bits
constexpr uint64_t TRI_MAX = 1ull << 28; // ... and its first slot in 28
constexpr int TRIES = 8;

// The tree in depth-first pre-order.  An inner node's first child is the next node; `skip` is the first node behind the subtree (the node count
// for the last one), so skip > own index everywhere: the traversal's node index only grows.  info: count = info & 15 (0: inner node), first
// triangle slot = info >> 4.
struct alignas(16) Node { float lo[3]; uint32_t skip; float hi[3]; uint32_t info; };
// A triangle in leaf order: the three corners as given and their colours (r | g << 8 | b << 16).  Its index in the mesh is Scene::index[slot].
struct alignas(16) Tri { float v0[3]; uint32_t c0; float v1[3]; uint32_t c1; float v2[3]; uint32_t c2; };

struct Scene {
  const Node* nodes;
  const Tri* tris;
  const uint32_t* index;
  uint32_t n_nodes;
  float guard;   // the triangle test's guard band: 2^-14 x the largest |coordinate| of the mesh
};

struct V3 { float x, y, z; };
struct Hit { uint32_t slot, index; float t, u, v; };

RW_HD V3 v3(const float* p) { return V3{p[0], p[1], p[2]}; }
RW_HD V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RW_HD V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
RW_HD float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RW_HD float min3(float a, float b, float c) { const float m = a < b ? a : b; return m < c ? m : c; }
RW_HD float max3(float a, float b, float c) { const float m = a > b ? a : b; return m > c ? m : c; }
RW_HD float absf(float a) { return a < 0.f ? -a : a; }

// ---- samples: a counter-based hash of (pixel, sample, bounce, dimension, try) -> 24-bit uniforms in [0, 1)
RW_HD uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
RW_HD float uniform(uint32_t pixel, uint32_t sample, uint32_t bounce, uint32_t dim, uint32_t tr) {
  uint32_t h = mix(pixel + 0x9e3779b9u);
  h = mix(h + sample);
  h = mix(h + ((bounce << 8) | (dim << 4) | tr));
  return (float)(h >> 8) * 5.9604644775390625e-8f;   // 2^-24; both steps are exact
}

// ---- the triangle test: Moeller-Trumbore with the order written out, inclusive edges, det == 0 (and NaN) a miss, and the guard band
RW_HD bool tri_test(V3 o, V3 d, const Tri& T, float guard, float& t, float& u, float& v) {
  const V3 v0 = v3(T.v0), v1 = v3(T.v1), v2 = v3(T.v2);
  const V3 e1 = sub(v1, v0), e2 = sub(v2, v0);
  const V3 p = cross(d, e2);
  const float det = dot(e1, p);
  if (!(det > 0.f || det < 0.f)) return false;
  const float inv = 1.f / det;
  const V3 s = sub(o, v0);
  u = dot(s, p) * inv;
  if (!(u >= 0.f && u <= 1.f)) return false;
  const V3 q = cross(s, e1);
  v = dot(d, q) * inv;
  if (!(v >= 0.f && u + v <= 1.f)) return false;
  t = dot(e2, q) * inv;
  if (!(t > 0.f && t <= BIG)) return false;
  // the guard: the point the walk would continue from lies in the triangle's box widened by `guard`.  Every accepted hit therefore sits inside
  // every tree box above the triangle, whatever cancellation did to u, v and t of a sliver (DESIGN.md 4j "Why the tree cannot change the answer")
  const float px = fmaf(t, d.x, o.x), py = fmaf(t, d.y, o.y), pz = fmaf(t, d.z, o.z);
  if (!(px >= min3(v0.x, v1.x, v2.x) - guard && px <= max3(v0.x, v1.x, v2.x) + guard)) return false;
  if (!(py >= min3(v0.y, v1.y, v2.y) - guard && py <= max3(v0.y, v1.y, v2.y) + guard)) return false;
  if (!(pz >= min3(v0.z, v1.z, v2.z) - guard && pz <= max3(v0.z, v1.z, v2.z) + guard)) return false;
  return true;
}

// ---- a ray as the traversal wants it.  Per axis: mode 0 the slab's two planes give an interval of t; 1 (d == 0) the origin is between the planes
// or the box is missed; 2 (d != 0 but 1/d overflows) the axis says nothing.  No 0 x inf is ever formed.
struct Ray { V3 o, d, inv; int mx, my, mz; float slack; };
RW_HD int axis_mode(float d, float inv) { return d == 0.f ? 1 : ((inv > BIG || inv < -BIG) ? 2 : 0); }
RW_HD Ray make_ray(V3 o, V3 d) {
  Ray r;
  r.o = o; r.d = d;
  r.inv = V3{1.f / d.x, 1.f / d.y, 1.f / d.z};
  r.mx = axis_mode(d.x, r.inv.x); r.my = axis_mode(d.y, r.inv.y); r.mz = axis_mode(d.z, r.inv.z);
  r.slack = max3(absf(o.x), absf(o.y), absf(o.z)) * 1.9073486328125e-6f;   // 2^-19 x the origin's largest |coordinate|
  return r;
}
RW_HD void slab(float lo, float hi, float o, float inv, int mode, float slack, float& tn, float& tf) {
  const float l = lo - slack, h = hi + slack;
  const float inf = BIG + BIG;
  float a = -inf, b = inf;
  if (mode == 0) {
    const float t1 = (l - o) * inv, t2 = (h - o) * inv;
    a = t1 < t2 ? t1 : t2;
    b = t1 < t2 ? t2 : t1;
  } else if (mode == 1 && !(o >= l && o <= h)) {
    a = inf; b = -inf;
  }
  tn = a > tn ? a : tn;
  tf = b < tf ? b : tf;
}

// ---- closest hit: among ALL triangles the test accepts (but `exclude`, by mesh index) the smallest float t, the lowest mesh index on equal t.
// A node is skipped only when its interval [tn, tf] clipped to [0, t_best] is empty: "<=", because an equal t with a lower index still wins.
RW_HD void closest_hit(const Scene& S, const Ray& r, uint32_t exclude, Hit& best) {
  best.slot = NONE; best.index = NONE; best.t = BIG + BIG; best.u = 0.f; best.v = 0.f;
  uint32_t n = 0;
  while (n < S.n_nodes) {                       // n only grows: at most n_nodes turns
    const Node nd = S.nodes[n];
    float tn = 0.f, tf = best.t;
    slab(nd.lo[0], nd.hi[0], r.o.x, r.inv.x, r.mx, r.slack, tn, tf);
    slab(nd.lo[1], nd.hi[1], r.o.y, r.inv.y, r.my, r.slack, tn, tf);
    slab(nd.lo[2], nd.hi[2], r.o.z, r.inv.z, r.mz, r.slack, tn, tf);
    uint32_t next = nd.skip;
    if (tn <= tf) {
      next = n + 1;
      const uint32_t count = nd.info & 15u, first = nd.info >> 4;
      for (uint32_t k = 0; k < count; k++) {    // count <= LEAF_MAX
        float t, u, v;
        if (!tri_test(r.o, r.d, S.tris[first + k], S.guard, t, u, v)) continue;
        const uint32_t idx = S.index[first + k];
        if (idx == exclude) continue;
        if (t < best.t || (t == best.t && idx < best.index)) { best.slot = first + k; best.index = idx; best.t = t; best.u = u; best.v = v; }
      }
    }
    n = next > n ? next : n + 1;                // set_mesh checked skip > n; the loop would end without that check too
  }
}

// ---- the camera ray of pixel (x, y), sub-pixel position (jx, jy) in [0, 1)
RW_HD V3 camera_dir(const sf_camera& c, int W, int H, int x, int y, float jx, float jy) {
  const float px = (float)x + jx, py = (float)y + jy;
  const float a = (px + px) / (float)W - 1.f;
  const float b = 1.f - (py + py) / (float)H;
  const float sx = a * c.tan_half_fov;
  const float sy = b * (c.tan_half_fov / c.aspect);
  const V3 w = V3{fmaf(sy, c.up[0], fmaf(sx, c.right[0], c.forward[0])), fmaf(sy, c.up[1], fmaf(sx, c.right[1], c.forward[1])),
                  fmaf(sy, c.up[2], fmaf(sx, c.right[2], c.forward[2]))};
  const float len = sqrtf(dot(w, w));
  return V3{w.x / len, w.y / len, w.z / len};
}

// ---- the bounce: (n + s) / |n + s| with s uniform on the unit sphere (Marsaglia 1972: a point of the unit disk by rejection, lifted).  After TRIES
// rejected points s = n; if |n + s|^2 is not a positive finite number the direction is n.
RW_HD V3 bounce_dir(V3 n, uint32_t pixel, uint32_t sample, uint32_t bounce) {
  V3 s = n;
  for (uint32_t tr = 0; tr < (uint32_t)TRIES; tr++) {
    const float u1 = uniform(pixel, sample, bounce, 0, tr), u2 = uniform(pixel, sample, bounce, 1, tr);
    const float a = (u1 + u1) - 1.f, b = (u2 + u2) - 1.f;
    const float q = a * a + b * b;
    if (q < 1.f) {
      const float r = sqrtf(1.f - q);
      s = V3{(a + a) * r, (b + b) * r, 1.f - (q + q)};
      break;
    }
  }
  const V3 w = V3{n.x + s.x, n.y + s.y, n.z + s.z};
  const float len2 = dot(w, w);
  if (!(len2 > 0.f && len2 <= BIG)) return n;
  const float len = sqrtf(len2);
  return V3{w.x / len, w.y / len, w.z / len};
}

RW_HD float byte_unit(uint32_t packed, int shift) { return (float)((packed >> shift) & 255u) / 255.f; }

// ---- one sample's path: RGBA
RW_HD void sample_path(const Scene& S, const sf_camera& c, const sf_render_params& p, int x, int y, uint32_t sample, float out[4]) {
  const uint32_t pixel = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
  const bool ao = p.integrator == SF_RENDER_AO;
  const int bounces = ao ? 1 : p.max_depth;
  const float jx = p.pixel_centre ? 0.5f : uniform(pixel, sample, 0, 0, 0), jy = p.pixel_centre ? 0.5f : uniform(pixel, sample, 0, 1, 0);
  V3 o = v3(c.origin), d = camera_dir(c, p.width, p.height, x, y, jx, jy);
  float tr = 1.f, tg = 1.f, tb = 1.f;
  uint32_t exclude = NONE;
  out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; out[3] = 1.f;
  for (int k = 0; k <= bounces; k++) {           // bounces <= 16: at most 17 rays
    const Ray r = make_ray(o, d);
    Hit h;
    closest_hit(S, r, exclude, h);
    if (h.index == NONE) {                       // the sky: radiance 1
      out[0] = tr; out[1] = tg; out[2] = tb;
      if (k == 0) out[3] = 0.f;
      return;
    }
    if (k == bounces) return;                    // a hit behind the last bounce: radiance 0
    const Tri T = S.tris[h.slot];
    const V3 e1 = sub(v3(T.v1), v3(T.v0)), e2 = sub(v3(T.v2), v3(T.v0));
    const V3 g = cross(e1, e2);
    if (!(dot(d, g) < 0.f)) return;              // from behind (or edge on): radiance 0
    const float len2 = dot(g, g);
    if (!(len2 > 0.f && len2 <= BIG)) return;    // no normal to bounce about: radiance 0
    const float len = sqrtf(len2);
    const V3 n = V3{g.x / len, g.y / len, g.z / len};
    if (!ao) {
      const float w0 = (1.f - h.u) - h.v;
      tr = tr * ((w0 * byte_unit(T.c0, 0) + h.u * byte_unit(T.c1, 0)) + h.v * byte_unit(T.c2, 0));
      tg = tg * ((w0 * byte_unit(T.c0, 8) + h.u * byte_unit(T.c1, 8)) + h.v * byte_unit(T.c2, 8));
      tb = tb * ((w0 * byte_unit(T.c0, 16) + h.u * byte_unit(T.c1, 16)) + h.v * byte_unit(T.c2, 16));
    }
    o = V3{fmaf(h.t, d.x, o.x), fmaf(h.t, d.y, o.y), fmaf(h.t, d.z, o.z)};
    d = bounce_dir(n, pixel, sample, (uint32_t)k + 1u);
    exclude = h.index;
  }
}

// ---- a pixel: its samples summed in sample order, divided by their number
RW_HD void render_pixel(const Scene& S, const sf_camera& c, const sf_render_params& p, int x, int y, float out[4]) {
  float sr = 0.f, sg = 0.f, sb = 0.f, sa = 0.f;
  for (int s = 0; s < p.samples; s++) {          // samples <= SF_RENDER_MAX_SAMPLES
    float v[4];
    sample_path(S, c, p, x, y, (uint32_t)s, v);
    sr = sr + v[0]; sg = sg + v[1]; sb = sb + v[2]; sa = sa + v[3];
  }
  const float n = (float)p.samples;
  out[0] = sr / n; out[1] = sg / n; out[2] = sb / n; out[3] = sa / n;
}

}  // namespace rw
