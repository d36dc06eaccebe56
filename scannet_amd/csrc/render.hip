// render.hip -- the mesh render on gfx950 and its C ABI (include/scanfuse.h "Mesh render and thumbnail").
//   k_render       one lane per pixel, an 8x8 tile of pixels per wave (four tiles per workgroup), up to SF_RENDER_MAX_BATCH views along grid z: every
//                  lane walks its pixel's samples in order (render_walk.h), so the sample-order sum needs no second pass
//   k_render_rays  closest hit of a batch of rays, one lane per ray (the tests' stage hook)
// The tree is threaded with skip links: the traversal keeps one node index that only grows -- no stack, no private memory.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "common.h"
#include "hip_util.h"
#include "mesh.h"
#include "render_internal.h"

namespace {

__global__ __launch_bounds__(256) void k_render(rw::Scene S, sf_render_params p, const sf_camera* __restrict__ cams, float4* __restrict__ rgba) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = ((int)blockIdx.x * 2 + (wave & 1)) * 8 + (lane & 7);
  const int y = ((int)blockIdx.y * 2 + (wave >> 1)) * 8 + (lane >> 3);
  if (x >= p.width || y >= p.height) return;
  const sf_camera c = cams[blockIdx.z];
  float out[4];
  rw::render_pixel(S, c, p, x, y, out);
  rgba[((size_t)blockIdx.z * (size_t)p.height + (size_t)y) * (size_t)p.width + (size_t)x] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(256) void k_render_rays(rw::Scene S, uint64_t n, const float* __restrict__ rays6, uint32_t* __restrict__ tri_out,
                                                     float* __restrict__ tuv_out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const rw::Ray r = rw::make_ray(rw::v3(rays6 + 6 * i), rw::v3(rays6 + 6 * i + 3));
  rw::Hit h;
  rw::closest_hit(S, r, rw::NONE, h);
  const bool hit = h.index != rw::NONE;
  tri_out[i] = h.index;
  tuv_out[3 * i] = hit ? h.t : 0.f;
  tuv_out[3 * i + 1] = hit ? h.u : 0.f;
  tuv_out[3 * i + 2] = hit ? h.v : 0.f;
}

int g_leaf = 4;

}  // namespace

struct sf_renderer {
  sf_render_params params;
  int device = -1;
  bool has_mesh = false;
  rh::Tree tree;
  sf::DevBuf d_nodes, d_tris, d_index, d_cams, d_out, d_rays, d_hit_tri, d_hit_tuv;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  rw::Scene device_scene() const {
    return rw::Scene{d_nodes.as<rw::Node>(), d_tris.as<rw::Tri>(), d_index.as<uint32_t>(), (uint32_t)tree.nodes.size(), tree.guard};
  }
};

SF_API void sf_render_params_default(sf_render_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->width = 640; p->height = 480; p->samples = 16; p->max_depth = 8;
  p->integrator = SF_RENDER_PATH; p->fov = 45.f; p->exposure = 1.f; p->pixel_centre = 0;
}

SF_API int sf_render_camera(const sf_mesh* mesh, const float* aabb6, const sf_render_params* params, const float* world_up, const float* camera_up,
                            const float* camera_offset, float bsphere_mult, float theta_deg, sf_camera* out) {
  if (!out || (!mesh && !aabb6)) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_camera: NULL argument (a mesh or a box, and the output)");
  sf_render_params p;
  if (params) p = *params; else sf_render_params_default(&p);
  float box[6];
  if (mesh) {
    const size_t nv = mesh->pos.size() / 3;
    if (nv == 0) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_camera: the mesh is empty");
    for (int a = 0; a < 3; a++) box[a] = box[3 + a] = mesh->pos[a];
    for (size_t v = 0; v < nv; v++)
      for (int a = 0; a < 3; a++) {
        const float c = mesh->pos[3 * v + a];
        if (!std::isfinite(c)) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_camera: vertex %zu is not finite", v);
        box[a] = c < box[a] ? c : box[a];
        box[3 + a] = c > box[3 + a] ? c : box[3 + a];
      }
  } else {
    std::memcpy(box, aabb6, sizeof(box));
  }
  std::string err;
  const int rc = rh::make_camera(box, p, world_up, camera_up, camera_offset, bsphere_mult, theta_deg, out, err);
  return rc == SF_OK ? SF_OK : sf::fail(rc, "%s", err.c_str());
}

SF_API int sf_renderer_create(const sf_render_params* params, int device, sf_renderer** out) {
  if (!out) return sf::fail(SF_ERR_INVALID_ARG, "sf_renderer_create: NULL output");
  *out = nullptr;
  sf_render_params p;
  if (params) p = *params; else sf_render_params_default(&p);
  std::string err;
  const int rc = rh::check_params(p, err);
  if (rc != SF_OK) return sf::fail(rc, "%s", err.c_str());
  if (device < -1) return sf::fail(SF_ERR_INVALID_ARG, "sf_renderer_create: device is -1 (the host path) or a HIP device");
  if (device >= 0)   // before the renderer exists: a refused device leaves nothing to take down on it
    if (int rc = sf::open_device(device, SF_ERR_DEVICE, "the render on a device needs one (device = -1 is the host path, and it is never taken silently)")) return rc;
  sf_renderer* r = new sf_renderer();
  r->params = p;
  r->device = device;
  if (device >= 0) {
    hipError_t e = hipStreamCreate(&r->stream);
    if (e == hipSuccess) e = hipEventCreate(&r->ev0);
    if (e == hipSuccess) e = hipEventCreate(&r->ev1);
    if (e != hipSuccess) {
      sf_renderer_destroy(r);
      return sf::fail(SF_ERR_DEVICE, "sf_renderer_create on device %d: %s", device, hipGetErrorString(e));
    }
  }
  *out = r;
  return SF_OK;
}

SF_API void sf_renderer_destroy(sf_renderer* r) {
  if (!r) return;
  if (r->device >= 0) {
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    if (r->ev0) (void)hipEventDestroy(r->ev0);
    if (r->ev1) (void)hipEventDestroy(r->ev1);
    if (r->stream) (void)hipStreamDestroy(r->stream);
  }
  delete r;
}

SF_API int sf_renderer_set_mesh(sf_renderer* r, const sf_mesh* mesh) {
  if (!r || !mesh) return sf::fail(SF_ERR_INVALID_ARG, "sf_renderer_set_mesh: NULL argument");
  const uint64_t nv = mesh->pos.size() / 3, nf = mesh->tri.size() / 3;
  const bool coloured = mesh->col.size() == 4 * nv && nv > 0;
  rh::Tree t;
  std::string err;
  const int rc = rh::build_tree(mesh->pos.data(), coloured ? mesh->col.data() : nullptr, nv, mesh->tri.data(), nf, g_leaf, t, err);
  if (rc != SF_OK) return sf::fail(rc, "%s", err.c_str());   // the renderer keeps the mesh it had
  if (r->device >= 0) {
    SF_HIP_CHECK(hipSetDevice(r->device));
    SF_HIP_CHECK(hipStreamSynchronize(r->stream));
    r->has_mesh = false;
    const size_t bn = t.nodes.size() * sizeof(rw::Node), bt = t.tris.size() * sizeof(rw::Tri), bi = t.index.size() * sizeof(uint32_t);
    SF_HIP_CHECK(r->d_nodes.reserve(bn));
    SF_HIP_CHECK(r->d_tris.reserve(bt));
    SF_HIP_CHECK(r->d_index.reserve(bi));
    SF_HIP_CHECK(hipMemcpyAsync(r->d_nodes.p, t.nodes.data(), bn, hipMemcpyHostToDevice, r->stream));
    SF_HIP_CHECK(hipMemcpyAsync(r->d_tris.p, t.tris.data(), bt, hipMemcpyHostToDevice, r->stream));
    SF_HIP_CHECK(hipMemcpyAsync(r->d_index.p, t.index.data(), bi, hipMemcpyHostToDevice, r->stream));
    SF_HIP_CHECK(hipStreamSynchronize(r->stream));
  }
  r->tree = std::move(t);
  r->has_mesh = true;
  return SF_OK;
}

SF_API int sf_renderer_run(sf_renderer* r, int n, const sf_camera* cameras, float* rgba, float* kernel_us) {
  if (!r || !cameras || !rgba || n < 1) return sf::fail(SF_ERR_INVALID_ARG, "sf_renderer_run: NULL argument or no view");
  if (!r->has_mesh) return sf::fail(SF_ERR_INVALID_ARG, "sf_renderer_run: no mesh (sf_renderer_set_mesh first)");
  for (int i = 0; i < n; i++) {
    const sf_camera& c = cameras[i];
    bool finite = std::isfinite(c.tan_half_fov) && std::isfinite(c.aspect);
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(c.origin[k]) && std::isfinite(c.right[k]) && std::isfinite(c.up[k]) && std::isfinite(c.forward[k]);
    if (!finite) return sf::fail(SF_ERR_INVALID_ARG, "sf_renderer_run: camera %d is not finite", i);
    if (!(c.aspect > 0.f) || !(c.tan_half_fov > 0.f)) return sf::fail(SF_ERR_INVALID_ARG, "sf_renderer_run: camera %d has no field of view", i);
  }
  const sf_render_params& p = r->params;
  const size_t image = (size_t)p.width * p.height;
  if (kernel_us) *kernel_us = 0.f;
  if (r->device < 0) {
    const auto t0 = std::chrono::steady_clock::now();
    rh::render_rows(r->tree, p, n, cameras, rgba, sf::usable_cpus());
    if (kernel_us) *kernel_us = (float)(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e6);
    return SF_OK;
  }
  SF_HIP_CHECK(hipSetDevice(r->device));
  const int batch = n < SF_RENDER_MAX_BATCH ? n : SF_RENDER_MAX_BATCH;
  SF_HIP_CHECK(r->d_cams.reserve((size_t)batch * sizeof(sf_camera)));
  SF_HIP_CHECK(r->d_out.reserve((size_t)batch * image * sizeof(float4)));
  const rw::Scene S = r->device_scene();
  for (int first = 0; first < n; first += batch) {
    const int m = n - first < batch ? n - first : batch;
    SF_HIP_CHECK(hipMemcpyAsync(r->d_cams.p, cameras + first, (size_t)m * sizeof(sf_camera), hipMemcpyHostToDevice, r->stream));
    const dim3 grid((unsigned)((p.width + 15) / 16), (unsigned)((p.height + 15) / 16), (unsigned)m);
    SF_HIP_CHECK(hipEventRecord(r->ev0, r->stream));
    hipLaunchKernelGGL(k_render, grid, dim3(256), 0, r->stream, S, p, r->d_cams.as<sf_camera>(), r->d_out.as<float4>());
    SF_HIP_CHECK(hipGetLastError());
    SF_HIP_CHECK(hipEventRecord(r->ev1, r->stream));
    SF_HIP_CHECK(hipMemcpyAsync(rgba + (size_t)first * image * 4, r->d_out.p, (size_t)m * image * sizeof(float4), hipMemcpyDeviceToHost, r->stream));
    SF_HIP_CHECK(hipStreamSynchronize(r->stream));
    if (kernel_us) {
      float ms = 0.f;
      SF_HIP_CHECK(hipEventElapsedTime(&ms, r->ev0, r->ev1));
      *kernel_us += ms * 1000.f;
    }
  }
  return SF_OK;
}

SF_API int sf_render_film(const float* rgba, uint64_t num_pixels, float exposure, uint8_t* rgba8) {
  if (!rgba || !rgba8) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_film: NULL argument");
  if (!std::isfinite(exposure)) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_film: exposure is not finite");
  rh::film(rgba, num_pixels, exposure, rgba8);
  return SF_OK;
}

SF_API int sf_image_thumbnail(const uint8_t* in, uint32_t width, uint32_t height, int channels, uint32_t box_w, uint32_t box_h, uint8_t* out,
                              uint32_t* out_w, uint32_t* out_h) {
  if (!in || !out || !out_w || !out_h) return sf::fail(SF_ERR_INVALID_ARG, "sf_image_thumbnail: NULL argument");
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || box_w < 1 || box_h < 1 || box_w > 65535 || box_h > 65535 || channels < 1 || channels > 4)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_image_thumbnail: sides are 1 .. 65535, channels 1 .. 4");
  rh::thumbnail_size(width, height, box_w, box_h, out_w, out_h);
  rh::thumbnail(in, width, height, channels, *out_w, *out_h, out);
  return SF_OK;
}

// ---------------------------------------------------------------- stage hooks (include/scanfuse_internal.h)
SF_API int sf_render_stage_nodes(const sf_renderer* r, float* boxes6, uint32_t* links2, uint64_t capacity, uint64_t* n_nodes) {
  if (!r || !n_nodes) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_stage_nodes: NULL argument");
  if (!r->has_mesh) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_stage_nodes: no mesh");
  const uint64_t nn = r->tree.nodes.size();
  *n_nodes = nn;
  if (!boxes6 && !links2) return SF_OK;
  if (capacity < nn) return sf::fail(SF_ERR_BOUNDS, "sf_render_stage_nodes: %llu nodes, room for %llu", (unsigned long long)nn, (unsigned long long)capacity);
  for (uint64_t i = 0; i < nn; i++) {
    const rw::Node& nd = r->tree.nodes[i];
    if (boxes6)
      for (int a = 0; a < 3; a++) { boxes6[6 * i + a] = nd.lo[a]; boxes6[6 * i + 3 + a] = nd.hi[a]; }
    if (links2) { links2[2 * i] = nd.skip; links2[2 * i + 1] = nd.info; }
  }
  return SF_OK;
}

SF_API int sf_render_stage_rays(sf_renderer* r, uint64_t n, const float* rays6, uint32_t* tri_out, float* tuv_out) {
  if (!r || !rays6 || !tri_out || !tuv_out) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_stage_rays: NULL argument");
  if (!r->has_mesh) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_stage_rays: no mesh");
  if (n == 0) return SF_OK;
  if (n > (1ull << 31)) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_stage_rays: at most 2^31 rays per call");
  for (uint64_t i = 0; i < 6 * n; i++)
    if (!std::isfinite(rays6[i])) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_stage_rays: ray %llu is not finite", (unsigned long long)(i / 6));
  if (r->device < 0) {
    rh::trace_rays(r->tree, n, rays6, tri_out, tuv_out, sf::usable_cpus());
    return SF_OK;
  }
  SF_HIP_CHECK(hipSetDevice(r->device));
  SF_HIP_CHECK(r->d_rays.reserve(n * 24));
  SF_HIP_CHECK(r->d_hit_tri.reserve(n * 4));
  SF_HIP_CHECK(r->d_hit_tuv.reserve(n * 12));
  SF_HIP_CHECK(hipMemcpyAsync(r->d_rays.p, rays6, n * 24, hipMemcpyHostToDevice, r->stream));
  hipLaunchKernelGGL(k_render_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->stream, r->device_scene(), n, r->d_rays.as<float>(),
                     r->d_hit_tri.as<uint32_t>(), r->d_hit_tuv.as<float>());
  SF_HIP_CHECK(hipGetLastError());
  SF_HIP_CHECK(hipMemcpyAsync(tri_out, r->d_hit_tri.p, n * 4, hipMemcpyDeviceToHost, r->stream));
  SF_HIP_CHECK(hipMemcpyAsync(tuv_out, r->d_hit_tuv.p, n * 12, hipMemcpyDeviceToHost, r->stream));
  SF_HIP_CHECK(hipStreamSynchronize(r->stream));
  return SF_OK;
}

SF_API int sf_render_stage_sample(const float n3[3], uint32_t pixel, uint32_t sample, uint32_t bounce, float dir3[3]) {
  if (!n3 || !dir3) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_stage_sample: NULL argument");
  const rw::V3 d = rw::bounce_dir(rw::v3(n3), pixel, sample, bounce);
  dir3[0] = d.x; dir3[1] = d.y; dir3[2] = d.z;
  return SF_OK;
}

SF_API int sf_render_tune(const char* key, int value) {
  if (!key) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_tune: NULL key");
  if (std::strcmp(key, "leaf") == 0) {
    if (value < 1 || value > rw::LEAF_MAX) return sf::fail(SF_ERR_INVALID_ARG, "sf_render_tune: leaf is 1 .. 15");
    g_leaf = value;
    return SF_OK;
  }
  return sf::fail(SF_ERR_INVALID_ARG, "sf_render_tune: unknown key %s", key);
}
