// render_host.cpp -- the host side of the mesh render: the deterministic tree builder, the camera of mts_render.py:69-99
// in double, the film, the thumbnail's integer area average, and the HOST PATH of the walk (render_walk.h over threads of rows; device = -1 --
// explicit, never a fallback).  Plain C++ without HIP or the library's error state, so tests/render_host_main.cpp builds it with sanitizers.
#include "render_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>

namespace rh {

int check_params(const sf_render_params& p, std::string& err) {
  if (p.width < 1 || p.width > SF_RENDER_MAX_SIDE || p.height < 1 || p.height > SF_RENDER_MAX_SIDE) { err = "render: width and height are 1 .. 8192"; return SF_ERR_INVALID_ARG; }
  if (p.samples < 1 || p.samples > SF_RENDER_MAX_SAMPLES) { err = "render: samples are 1 .. 4096"; return SF_ERR_INVALID_ARG; }
  if (p.max_depth < 1 || p.max_depth > SF_RENDER_MAX_DEPTH) { err = "render: max_depth is 1 .. 16"; return SF_ERR_INVALID_ARG; }
  if (p.integrator != SF_RENDER_PATH && p.integrator != SF_RENDER_AO) { err = "render: the integrators are path (0) and ao (1)"; return SF_ERR_INVALID_ARG; }
  if (!(p.fov > 0.f && p.fov < 180.f)) { err = "render: fov is in (0, 180) degrees"; return SF_ERR_INVALID_ARG; }
  if (!std::isfinite(p.exposure)) { err = "render: exposure is not finite"; return SF_ERR_INVALID_ARG; }
  return SF_OK;
}

// ---------------------------------------------------------------- the tree
namespace {
struct Builder {
  const float* xyz;
  const uint8_t* rgba;
  const uint32_t* tris;
  int leaf;
  float pad;
  std::vector<float> lo, hi;        // 3 per triangle: its box
  std::vector<uint32_t> order;      // the triangles, permuted in place
  Tree* out;

  float key(uint32_t t, int a) const { return lo[3 * (size_t)t + a] + hi[3 * (size_t)t + a]; }

  void emit_leaf(size_t begin, size_t end) {
    for (size_t i = begin; i < end; i++) {
      const uint32_t t = order[i];
      rw::Tri T;
      uint32_t* cols[3] = {&T.c0, &T.c1, &T.c2};
      float* pos[3] = {T.v0, T.v1, T.v2};
      for (int k = 0; k < 3; k++) {
        const uint32_t v = tris[3 * (size_t)t + k];
        std::memcpy(pos[k], xyz + 3 * (size_t)v, 12);
        *cols[k] = rgba ? ((uint32_t)rgba[4 * (size_t)v] | ((uint32_t)rgba[4 * (size_t)v + 1] << 8) | ((uint32_t)rgba[4 * (size_t)v + 2] << 16)) : 0x808080u;
      }
      out->tris.push_back(T);
      out->index.push_back(t);
    }
  }

  // Nodes [begin, end) of `order`, at least one.  Split: the middle of the centroid bounds (keys lo + hi) along their longest axis, by a stable
  // partition; when that leaves a side empty, or below depth 48, the range is halved as it stands.  Stable everywhere: a leaf's triangles are in
  // ascending mesh order and the same mesh always gives the same tree.
  void build(size_t begin, size_t end, int depth) {
    const size_t me = out->nodes.size();
    out->nodes.push_back(rw::Node{});
    float blo[3], bhi[3], clo[3], chi[3];
    for (int a = 0; a < 3; a++) { blo[a] = clo[a] = INFINITY; bhi[a] = chi[a] = -INFINITY; }
    for (size_t i = begin; i < end; i++)
      for (int a = 0; a < 3; a++) {
        const uint32_t t = order[i];
        blo[a] = std::min(blo[a], lo[3 * (size_t)t + a]);
        bhi[a] = std::max(bhi[a], hi[3 * (size_t)t + a]);
        clo[a] = std::min(clo[a], key(t, a));
        chi[a] = std::max(chi[a], key(t, a));
      }
    uint32_t info = 0;
    if (end - begin <= (size_t)leaf) {
      info = ((uint32_t)out->tris.size() << 4) | (uint32_t)(end - begin);
      emit_leaf(begin, end);
    } else {
      int axis = 0;
      for (int a = 1; a < 3; a++)
        if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
      const float mid = clo[axis] * 0.5f + chi[axis] * 0.5f;
      size_t m = begin;
      if (depth < 48)
        m = (size_t)(std::stable_partition(order.begin() + begin, order.begin() + end, [&](uint32_t t) { return key(t, axis) < mid; }) - order.begin());
      if (m == begin || m == end) m = begin + (end - begin) / 2;
      build(begin, m, depth + 1);
      build(m, end, depth + 1);
    }
    rw::Node& nd = out->nodes[me];
    for (int a = 0; a < 3; a++) { nd.lo[a] = blo[a] - pad; nd.hi[a] = bhi[a] + pad; }
    nd.skip = (uint32_t)out->nodes.size();
    nd.info = info;
  }
};
}  // namespace

int build_tree(const float* xyz, const uint8_t* rgba, uint64_t nv, const uint32_t* tris, uint64_t nf, int leaf, Tree& out, std::string& err) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!xyz || !tris || nv == 0 || nf == 0) { err = "render: the mesh is empty"; return SF_ERR_INVALID_ARG; }
  if (nf >= rw::TRI_MAX) { err = "render: the tree's nodes index fewer than 2^28 triangles"; return SF_ERR_INVALID_ARG; }
  if (leaf < 1 || leaf > rw::LEAF_MAX) { err = "render: a leaf holds 1 .. 15 triangles"; return SF_ERR_INVALID_ARG; }
  float big = 0.f;
  for (uint64_t i = 0; i < 3 * nv; i++) {
    if (!std::isfinite(xyz[i])) { err = "render: vertex " + std::to_string(i / 3) + " is not finite"; return SF_ERR_INVALID_ARG; }
    big = std::max(big, std::fabs(xyz[i]));
  }
  for (uint64_t i = 0; i < 3 * nf; i++)
    if (tris[i] >= nv) { err = "render: triangle " + std::to_string(i / 3) + " names vertex " + std::to_string(tris[i]) + " of " + std::to_string(nv); return SF_ERR_INVALID_ARG; }
  out = Tree();
  out.guard = big * 6.103515625e-05f;       // 2^-14
  Builder b{xyz, rgba, tris, leaf, big * 1.220703125e-04f /* 2^-13 */, {}, {}, {}, &out};
  b.lo.resize(3 * nf);
  b.hi.resize(3 * nf);
  b.order.resize(nf);
  for (uint64_t t = 0; t < nf; t++) {
    b.order[t] = (uint32_t)t;
    const float *p0 = xyz + 3 * (size_t)tris[3 * t], *p1 = xyz + 3 * (size_t)tris[3 * t + 1], *p2 = xyz + 3 * (size_t)tris[3 * t + 2];
    for (int a = 0; a < 3; a++) {
      b.lo[3 * t + a] = std::min(p0[a], std::min(p1[a], p2[a]));
      b.hi[3 * t + a] = std::max(p0[a], std::max(p1[a], p2[a]));
    }
  }
  out.nodes.reserve(2 * nf);
  out.tris.reserve(nf);
  out.index.reserve(nf);
  b.build(0, nf, 0);
  // what the traversal's bound rests on, checked, not assumed: links only point forward, leaves stay inside the triangle array
  const uint64_t nn = out.nodes.size();
  for (uint64_t i = 0; i < nn; i++) {
    const rw::Node& nd = out.nodes[i];
    const uint64_t count = nd.info & 15u, first = nd.info >> 4;
    if (nd.skip <= i || nd.skip > nn || first + count > nf) { err = "render: the tree builder produced a bad link"; return SF_ERR_BOUNDS; }
  }
  out.build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return SF_OK;
}

// ---------------------------------------------------------------- the camera (double)
namespace {
struct D3 { double x, y, z; };
D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 dcross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dlen(D3 a) { return std::sqrt(ddot(a, a)); }
bool finite3(D3 a) { return std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z); }
D3 rotate(D3 v, D3 k, double c, double s) { return c * v + s * dcross(k, v) + (ddot(k, v) * (1.0 - c)) * k; }   // Rodrigues, k a unit vector
D3 from(const float* p, D3 dflt) { return p ? D3{p[0], p[1], p[2]} : dflt; }
void put(float* o, D3 a) { o[0] = (float)a.x; o[1] = (float)a.y; o[2] = (float)a.z; }
}  // namespace

int make_camera(const float aabb6[6], const sf_render_params& p, const float* world_up, const float* camera_up, const float* camera_offset,
                float bsphere_mult, float theta_deg, sf_camera* out, std::string& err) {
  const int rc = check_params(p, err);
  if (rc != SF_OK) return rc;
  const D3 lo{aabb6[0], aabb6[1], aabb6[2]}, hi{aabb6[3], aabb6[4], aabb6[5]};
  const D3 wu = from(world_up, {0, 0, 1}), cu = from(camera_up, {0, 1, 0}), off = from(camera_offset, {0, 0, 0});
  if (!finite3(lo) || !finite3(hi) || !finite3(wu) || !finite3(cu) || !finite3(off) || !std::isfinite(bsphere_mult) || !std::isfinite(theta_deg)) {
    err = "render camera: an input is not finite";
    return SF_ERR_INVALID_ARG;
  }
  if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) { err = "render camera: the box is empty"; return SF_ERR_INVALID_ARG; }
  if (!(dlen(wu) > 0)) { err = "render camera: world_up is zero"; return SF_ERR_INVALID_ARG; }
  const D3 along = off + wu;
  if (!(dlen(along) > 0)) { err = "render camera: camera_offset + world_up is zero"; return SF_ERR_INVALID_ARG; }
  const D3 centre = 0.5 * (lo + hi);
  const double radius = dlen(hi - centre);
  const D3 arm = ((double)bsphere_mult * radius / dlen(along)) * along;
  const D3 axis = (1.0 / dlen(wu)) * wu;
  const double th = (double)theta_deg * 3.14159265358979323846 / 180.0, c = std::cos(th), s = std::sin(th);
  const D3 arm_r = rotate(arm, axis, c, s), cu_r = rotate(cu, axis, c, s);
  if (!(dlen(arm_r) > 0)) { err = "render camera: the camera sits in the centre of the box (zero radius or bsphere_mult)"; return SF_ERR_INVALID_ARG; }
  const D3 fwd = (-1.0 / dlen(arm_r)) * arm_r;
  const D3 r0 = dcross(fwd, cu_r);
  if (!(dlen(r0) > 1e-9 * dlen(cu_r)) || !(dlen(cu_r) > 0)) { err = "render camera: camera_up is parallel to the view direction"; return SF_ERR_INVALID_ARG; }
  const D3 right = (1.0 / dlen(r0)) * r0, up = dcross(right, fwd);
  std::memset(out, 0, sizeof(*out));
  put(out->origin, centre + arm_r);
  put(out->right, right);
  put(out->up, up);
  put(out->forward, fwd);
  out->tan_half_fov = (float)std::tan((double)p.fov * 3.14159265358979323846 / 360.0);
  out->aspect = (float)((double)p.width / (double)p.height);
  return SF_OK;
}

// ---------------------------------------------------------------- the host path
namespace {
template <class F>
void parallel(uint64_t n_items, int threads, F f) {   // f(item) over a shared counter
  std::atomic<uint64_t> next{0};
  auto work = [&]() {
    for (;;) {
      const uint64_t i = next.fetch_add(1);
      if (i >= n_items) return;
      f(i);
    }
  };
  const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), n_items));
  std::vector<std::thread> pool;
  for (int i = 1; i < nt; i++) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
}
}  // namespace

void render_rows(const Tree& t, const sf_render_params& p, int n, const sf_camera* cams, float* rgba, int threads) {
  const rw::Scene S = t.scene();
  const uint64_t H = (uint64_t)p.height, W = (uint64_t)p.width;
  parallel((uint64_t)n * H, threads, [&](uint64_t row) {
    const uint64_t cam = row / H, y = row % H;
    float* o = rgba + (cam * H + y) * W * 4;
    for (uint64_t x = 0; x < W; x++) rw::render_pixel(S, cams[cam], p, (int)x, (int)y, o + 4 * x);
  });
}

void trace_rays(const Tree& t, uint64_t n, const float* rays6, uint32_t* tri_out, float* tuv_out, int threads) {
  const rw::Scene S = t.scene();
  const uint64_t chunk = 256;
  parallel((n + chunk - 1) / chunk, threads, [&](uint64_t c) {
    for (uint64_t i = c * chunk; i < std::min(n, (c + 1) * chunk); i++) {
      const rw::Ray r = rw::make_ray(rw::v3(rays6 + 6 * i), rw::v3(rays6 + 6 * i + 3));
      rw::Hit h;
      rw::closest_hit(S, r, rw::NONE, h);
      const bool hit = h.index != rw::NONE;
      tri_out[i] = h.index;
      tuv_out[3 * i] = hit ? h.t : 0.f; tuv_out[3 * i + 1] = hit ? h.u : 0.f; tuv_out[3 * i + 2] = hit ? h.v : 0.f;
    }
  });
}

// ---------------------------------------------------------------- film and thumbnail
void film(const float* rgba, uint64_t num_pixels, float exposure, uint8_t* rgba8) {
  const double gain = std::exp2((double)exposure);
  for (uint64_t i = 0; i < num_pixels; i++) {
    for (int c = 0; c < 3; c++) {
      double v = (double)rgba[4 * i + c] * gain;
      v = v <= 0.0031308 ? 12.92 * v : 1.055 * std::pow(v, 1.0 / 2.4) - 0.055;
      if (!(v > 0.0)) v = 0.0;
      if (v > 1.0) v = 1.0;
      rgba8[4 * i + c] = (uint8_t)(int)(255.0 * v + 0.5);
    }
    double a = (double)rgba[4 * i + 3];
    if (!(a > 0.0)) a = 0.0;
    if (a > 1.0) a = 1.0;
    rgba8[4 * i + 3] = (uint8_t)(int)(255.0 * a + 0.5);
  }
}

void thumbnail_size(uint32_t w, uint32_t h, uint32_t box_w, uint32_t box_h, uint32_t* ow, uint32_t* oh) {
  const uint64_t W = w, H = h, BW = box_w, BH = box_h;
  if (BW * H <= BH * W) {   // the width fills the box
    *ow = box_w;
    *oh = (uint32_t)std::max<uint64_t>(1, (2 * H * BW + W) / (2 * W));
  } else {
    *oh = box_h;
    *ow = (uint32_t)std::max<uint64_t>(1, (2 * W * BH + H) / (2 * H));
  }
}

// Output pixel X covers [X w, (X + 1) w) and source pixel x covers [x ow, (x + 1) ow) on a line of w * ow units (rows alike): the weight of a source
// pixel is its overlap in x times its overlap in y, the weights of one output pixel sum to w * h, and the value is (sum + w h / 2) / (w h) in
// integers, every channel alike (alpha is not premultiplied).
void thumbnail(const uint8_t* in, uint32_t w, uint32_t h, int channels, uint32_t ow, uint32_t oh, uint8_t* out) {
  const uint64_t W = w, H = h, OW = ow, OH = oh, total = W * H;
  for (uint64_t Y = 0; Y < OH; Y++)
    for (uint64_t X = 0; X < OW; X++) {
      uint64_t sum[4] = {0, 0, 0, 0};
      const uint64_t y0 = Y * H / OH, y1 = ((Y + 1) * H + OH - 1) / OH, x0 = X * W / OW, x1 = ((X + 1) * W + OW - 1) / OW;
      for (uint64_t y = y0; y < y1; y++) {
        const uint64_t wy = std::min((y + 1) * OH, (Y + 1) * H) - std::max(y * OH, Y * H);
        for (uint64_t x = x0; x < x1; x++) {
          const uint64_t wx = std::min((x + 1) * OW, (X + 1) * W) - std::max(x * OW, X * W);
          for (int c = 0; c < channels; c++) sum[c] += wy * wx * in[(y * W + x) * channels + c];
        }
      }
      for (int c = 0; c < channels; c++) out[(Y * OW + X) * channels + c] = (uint8_t)((sum[c] + total / 2) / total);
    }
}

}  // namespace rh
