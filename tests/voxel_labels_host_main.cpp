// voxel_labels_host_main.cpp -- the host path of the voxel-task data (scannet_amd/csrc/voxel_labels.cpp) as a program of its own, for
// tests/test_voxel_labels.py::test_host_code_under_sanitizers: built with -fsanitize=address,undefined and run; nothing is preloaded.  It links
// voxel_labels.cpp alone, so the few things that file takes from the rest of the library are defined here: the error string, the CPU count, a grid
// that is two borrowed arrays, and the device entry points (which this program never reaches).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scanfuse.h"
#include "../scannet_amd/csrc/voxel_labels_internal.h"

namespace sf {
std::string& last_error_ref() {
  static std::string s;
  return s;
}
int usable_cpus() { return 4; }
namespace vl {
int nearest_device(const sf_grid_header&, const float*, uint64_t, const uint32_t*, uint64_t, float, float, int, int32_t*, float*, const BinsOut*) { return SF_ERR_DEVICE; }
int sample_device(const sf_grid_header&, const float*, const uint8_t*, int32_t, int32_t, int32_t, int64_t, int32_t, int, uint64_t, uint64_t, float*, uint8_t*,
                  int32_t*, uint64_t*) {
  return SF_ERR_DEVICE;
}
}  // namespace vl
}  // namespace sf

struct sf_grid {
  sf_grid_header h;
  const float* value;
  const uint8_t* weight;
};
extern "C" int sf_grid_info(const sf_grid* g, sf_grid_header* out) { *out = g->h; return SF_OK; }
extern "C" int sf_grid_data(const sf_grid* g, const float** value, const uint8_t** weight) {
  if (value) *value = g->value;
  if (weight) *weight = g->weight;
  return SF_OK;
}
extern "C" const char* sf_last_error(void) { return sf::last_error_ref().c_str(); }

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, sf_last_error()); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(uint32_t& s) { return (float)rnd(s) / 16777216.0f; }

int main() {
  sf_grid_header h;
  std::memset(&h, 0, sizeof(h));
  h.nx = 21; h.ny = 19; h.nz = 13;
  h.voxel_size = 0.05f;
  h.lo_voxel[0] = -4; h.lo_voxel[1] = -2; h.lo_voxel[2] = -3;
  const size_t n = (size_t)h.nx * h.ny * h.nz;
  // a soup of 600 triangles, some large, and the faces the rule skips
  uint32_t seed = 12345u;
  std::vector<float> xyz;
  std::vector<uint32_t> tris;
  for (int f = 0; f < 600; f++) {
    const float size = f % 10 == 0 ? 0.5f : 0.07f;
    const float c[3] = {-0.3f + 1.3f * unit(seed), -0.2f + 1.2f * unit(seed), -0.25f + 0.9f * unit(seed)};
    for (int v = 0; v < 3; v++) {
      for (int a = 0; a < 3; a++) xyz.push_back(c[a] + size * (unit(seed) - 0.5f));
      tris.push_back((uint32_t)(3 * f + v));
    }
  }
  const uint32_t nv0 = (uint32_t)(xyz.size() / 3);
  const float bad[9] = {NAN, 0.1f, 0.1f, 0.2f, INFINITY, 0.1f, 0.1f, 0.2f, 1e30f};
  xyz.insert(xyz.end(), bad, bad + 9);
  const uint32_t extra[12] = {0, 0, 1, nv0, 1, 2, 3, nv0 + 1, 5, 6, 7, nv0 + 2};
  tris.insert(tris.end(), extra, extra + 12);
  const uint64_t nv = xyz.size() / 3, nf = tris.size() / 3;
  std::vector<int32_t> face(n), face2(n);
  std::vector<float> d2(n);
  CHECK(sf_voxlabel_nearest_faces(&h, xyz.data(), nv, tris.data(), nf, 0.8660254f, -1, face.data(), d2.data()) == SF_OK);
  CHECK(sf_voxlabel_nearest_faces(&h, xyz.data(), nv, tris.data(), nf - 4, 0.8660254f, -1, face2.data(), nullptr) == SF_OK);
  CHECK(face == face2);                                            // the skipped faces change nothing
  size_t hit = 0;
  const float t = 0.8660254f * 0.05f, r2 = t * t;
  for (size_t i = 0; i < n; i++) {
    CHECK(face[i] >= -1 && face[i] < (int32_t)(nf - 4));
    CHECK(face[i] < 0 ? std::isinf(d2[i]) : d2[i] <= r2);
    hit += face[i] >= 0;
  }
  CHECK(hit > 100 && hit < n);
  // refusals leave the outputs alone
  const std::vector<int32_t> before = face;
  tris[5] = (uint32_t)nv;
  CHECK(sf_voxlabel_nearest_faces(&h, xyz.data(), nv, tris.data(), nf, 0.8660254f, -1, face.data(), nullptr) == SF_ERR_INVALID_ARG);
  tris[5] = 5;
  CHECK(sf_voxlabel_nearest_faces(&h, xyz.data(), nv, tris.data(), nf, NAN, -1, face.data(), nullptr) == SF_ERR_INVALID_ARG);
  CHECK(face == before);
  // empty inputs
  sf_grid_header e = h;
  e.nx = 0;
  CHECK(sf_voxlabel_nearest_faces(&e, xyz.data(), nv, tris.data(), nf, 1.0f, -1, nullptr, nullptr) == SF_OK);
  CHECK(sf_voxlabel_nearest_faces(&h, nullptr, 0, nullptr, 0, 1.0f, -1, face2.data(), nullptr) == SF_OK);
  for (size_t i = 0; i < n; i++) CHECK(face2[i] == -1);
  // labels
  std::vector<uint16_t> vlabel(nv), label(n);
  std::vector<uint8_t> vinst(nv), inst(n), bl(n);
  for (uint64_t v = 0; v < nv; v++) { vlabel[v] = (uint16_t)(rnd(seed) % 3 == 0 ? 300 : rnd(seed) % 40); vinst[v] = (uint8_t)(rnd(seed) % 7); }
  CHECK(sf_voxlabel_labels(face.data(), n, tris.data(), nf, nv, vlabel.data(), vinst.data(), label.data(), inst.data(), bl.data()) == SF_OK);
  for (size_t i = 0; i < n; i++) CHECK(face[i] < 0 ? (label[i] == 0 && bl[i] == 0) : (bl[i] == ((label[i] == 0 || label[i] > 254) ? 255 : label[i])));
  face2 = face;
  face2[7] = (int32_t)nf;
  CHECK(sf_voxlabel_labels(face2.data(), n, tris.data(), nf, nv, vlabel.data(), nullptr, label.data(), nullptr, bl.data()) == SF_ERR_INVALID_ARG);
  // samples: windows over every border, a page in the middle and one past the end
  std::vector<float> value(n);
  std::vector<uint8_t> weight(n, 1);
  for (size_t i = 0; i < n; i++) value[i] = (float)i;
  sf_grid g = {h, value.data(), weight.data()};
  sf_voxlabel_params p;
  sf_voxlabel_params_default(&p);
  uint64_t total = 0;
  CHECK(sf_voxlabel_sample_columns(&g, bl.data(), &p, -1, 0, 0, nullptr, nullptr, nullptr, &total) == SF_OK);
  CHECK(total > 4 && total <= (uint64_t)h.nx * h.ny);
  const size_t per = (size_t)p.wx * p.wy * p.wz;
  std::vector<float> data(3 * per);
  std::vector<uint8_t> slabel(3 * (size_t)p.wz);
  std::vector<int32_t> xy(6);
  CHECK(sf_voxlabel_sample_columns(&g, bl.data(), &p, -1, total - 2, 3, data.data(), slabel.data(), xy.data(), &total) == SF_OK);
  for (int s = 0; s < 2; s++) {
    const int x = xy[2 * s], y = xy[2 * s + 1];
    CHECK(x >= 0 && x < h.nx && y >= 0 && y < h.ny);
    for (int k = 0; k < p.wz; k++) {
      const int z = -h.lo_voxel[2] + k;
      const float centre = data[s * per + ((size_t)k * p.wy + p.wy / 2) * p.wx + p.wx / 2];
      CHECK(z < h.nz ? centre == value[((size_t)z * h.ny + y) * h.nx + x] : (std::isinf(centre) && centre < 0));
    }
  }
  CHECK(sf_voxlabel_sample_columns(&g, bl.data(), &p, -1, total + 5, 3, data.data(), slabel.data(), xy.data(), &total) == SF_OK);
  p.wx = 30;
  CHECK(sf_voxlabel_sample_columns(&g, bl.data(), &p, -1, 0, 0, nullptr, nullptr, nullptr, &total) == SF_ERR_INVALID_ARG);
  p.wx = 5; p.wy = 5; p.wz = 7; p.z0_default = 0; p.z0 = -3; p.stride = 2;
  CHECK(sf_voxlabel_sample_columns(&g, bl.data(), &p, -1, 0, 3, data.data(), slabel.data(), xy.data(), &total) == SF_OK);
  CHECK(sf_voxlabel_sample_columns(&g, bl.data(), &p, 0, 0, 3, data.data(), slabel.data(), xy.data(), &total) == SF_ERR_DEVICE);
  std::printf("voxel labels host: ok\n");
  return 0;
}
