// render_host_main.cpp -- the host side of the mesh render (scannet_amd/csrc/render_host.cpp over render_walk.h) as a stand-alone program:
// tests/test_render.py builds it together with render_host.cpp using g++ -fsanitize=address,undefined and runs it once over the `room` case.
//
//   render_host_main <in> <out>
//   in : int64 nv, nf; int32 width, height, samples, max_depth, integrator, pixel_centre, views, leaf; float xyz[3 nv]; uint8 rgba[4 nv];
//        uint32 tris[3 nf]; float theta[views]
//   out: float rgba[views x height x width x 4] (the host path, 4 threads); uint8 film[height x width x 4] of view 0; uint8 thumb[fit of 64 x 64]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../scannet_amd/csrc/render_internal.h"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> counts;
  std::vector<int32_t> h;
  std::vector<float> xyz, theta;
  std::vector<uint8_t> rgba;
  std::vector<uint32_t> tris;
  if (!get(f, counts, 2) || !get(f, h, 8) || !get(f, xyz, 3 * (size_t)counts[0]) || !get(f, rgba, 4 * (size_t)counts[0]) || !get(f, tris, 3 * (size_t)counts[1]) ||
      !get(f, theta, (size_t)h[6])) {
    std::fprintf(stderr, "short input\n");
    return 2;
  }
  std::fclose(f);
  sf_render_params p = {};
  p.width = h[0]; p.height = h[1]; p.samples = h[2]; p.max_depth = h[3]; p.integrator = h[4]; p.pixel_centre = h[5];
  p.fov = 45.f; p.exposure = 1.f;
  std::string err;
  rh::Tree tree;
  // the two refusals that no sf_mesh can carry to sf_renderer_set_mesh: a triangle count the node format cannot index (refused before an array
  // is read) and an index past the vertices (sf_mesh_create refuses that one itself)
  const uint32_t past[3] = {0, 1, (uint32_t)counts[0]};
  if (rh::build_tree(xyz.data(), rgba.data(), (uint64_t)counts[0], tris.data(), rw::TRI_MAX, h[7], tree, err) != SF_ERR_INVALID_ARG ||
      rh::build_tree(xyz.data(), rgba.data(), (uint64_t)counts[0], past, 1, h[7], tree, err) != SF_ERR_INVALID_ARG) {
    std::fprintf(stderr, "build_tree took 2^28 triangles or an index past the vertices\n");
    return 1;
  }
  if (rh::build_tree(xyz.data(), rgba.data(), (uint64_t)counts[0], tris.data(), (uint64_t)counts[1], h[7], tree, err) != SF_OK) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return 1;
  }
  float box[6] = {xyz[0], xyz[1], xyz[2], xyz[0], xyz[1], xyz[2]};
  for (size_t v = 0; v < (size_t)counts[0]; v++)
    for (int a = 0; a < 3; a++) {
      box[a] = xyz[3 * v + a] < box[a] ? xyz[3 * v + a] : box[a];
      box[3 + a] = xyz[3 * v + a] > box[3 + a] ? xyz[3 * v + a] : box[3 + a];
    }
  std::vector<sf_camera> cams((size_t)h[6]);
  for (size_t i = 0; i < cams.size(); i++)
    if (rh::make_camera(box, p, nullptr, nullptr, nullptr, 2.5f, theta[i], &cams[i], err) != SF_OK) {
      std::fprintf(stderr, "%s\n", err.c_str());
      return 1;
    }
  const size_t image = (size_t)p.width * p.height;
  std::vector<float> out(cams.size() * image * 4);
  rh::render_rows(tree, p, (int)cams.size(), cams.data(), out.data(), 4);
  std::vector<uint8_t> px(image * 4);
  rh::film(out.data(), image, p.exposure, px.data());
  uint32_t tw = 0, th = 0;
  rh::thumbnail_size((uint32_t)p.width, (uint32_t)p.height, 64, 64, &tw, &th);
  std::vector<uint8_t> small((size_t)tw * th * 4);
  rh::thumbnail(px.data(), (uint32_t)p.width, (uint32_t)p.height, 4, tw, th, small.data());
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = std::fwrite(out.data(), 4, out.size(), o) == out.size() && std::fwrite(px.data(), 1, px.size(), o) == px.size() &&
                  std::fwrite(small.data(), 1, small.size(), o) == small.size();
  std::fclose(o);
  return ok ? 0 : 2;
}
