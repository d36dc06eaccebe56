// render_internal.h -- the host side of the mesh render (render_host.cpp) as render.hip and tests/render_host_main.cpp see it.  Nothing here
// touches HIP or the library's error state: every function returns an sf_status and, on failure, a message in `err`.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "render_walk.h"

namespace rh {

struct Tree {
  std::vector<rw::Node> nodes;    // pre-order, skip links
  std::vector<rw::Tri> tris;      // leaf order
  std::vector<uint32_t> index;    // mesh index of each slot
  float guard = 0.f;
  double build_seconds = 0.0;
  rw::Scene scene() const { return rw::Scene{nodes.data(), tris.data(), index.data(), (uint32_t)nodes.size(), guard}; }
};

int check_params(const sf_render_params& p, std::string& err);
// rgba: 4 bytes per vertex or NULL (every byte 128).  leaf: 1 .. rw::LEAF_MAX triangles.
int build_tree(const float* xyz, const uint8_t* rgba, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, int leaf, Tree& out, std::string& err);
int make_camera(const float aabb6[6], const sf_render_params& p, const float* world_up, const float* camera_up, const float* camera_offset,
                float bsphere_mult, float theta_deg, sf_camera* out, std::string& err);
void render_rows(const Tree& t, const sf_render_params& p, int n, const sf_camera* cams, float* rgba, int threads);
void trace_rays(const Tree& t, uint64_t n, const float* rays6, uint32_t* tri_out, float* tuv_out, int threads);
void film(const float* rgba, uint64_t num_pixels, float exposure, uint8_t* rgba8);
void thumbnail_size(uint32_t w, uint32_t h, uint32_t box_w, uint32_t box_h, uint32_t* ow, uint32_t* oh);
void thumbnail(const uint8_t* in, uint32_t w, uint32_t h, int channels, uint32_t ow, uint32_t oh, uint8_t* out);

}  // namespace rh
