// object_voxels_host_main.cpp -- the host path of the object-task data (scannet_amd/csrc/object_voxels.cpp) as a program of its own, for
// tests/test_object_voxels.py::test_host_code_under_sanitizers: built with -fsanitize=address,undefined and run; nothing is preloaded.  It links
// object_voxels.cpp alone, so the few things that file takes from the rest of the library are defined here: the error string, the CPU count, a grid
// that is a borrowed array, and the device entry point (which this program never reaches).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scanfuse.h"
#include "scanfuse_internal.h"
#include "../scannet_amd/csrc/object_voxels_internal.h"

namespace sf {
std::string& last_error_ref() {
  static std::string s;
  return s;
}
int usable_cpus() { return 4; }
namespace ov {
int voxelize_device(const float*, uint64_t, const uint32_t*, uint64_t, const uint32_t*, const int32_t*, uint32_t, const GridRef&, uint64_t, const sf_objvox_params&, int,
                    uint64_t, uint64_t, uint8_t*, uint8_t*, int32_t*, float*, float*, uint64_t*, const StageOut*) {
  return SF_ERR_DEVICE;
}
}  // namespace ov
}  // namespace sf

struct sf_grid {
  sf_grid_header h;
  const uint8_t* weight;
};
extern "C" int sf_grid_info(const sf_grid* g, sf_grid_header* out) { *out = g->h; return SF_OK; }
extern "C" int sf_grid_data(const sf_grid* g, const float** value, const uint8_t** weight) {
  if (value) *value = nullptr;
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
  // 40 objects of 3 .. 42 faces (some large, some far from the grid), and the faces the rule skips
  uint32_t seed = 4242u;
  std::vector<float> xyz;
  std::vector<uint32_t> tris, vobj;
  const uint32_t nobj = 42;
  for (uint32_t o = 0; o < 40; o++) {
    const float base[3] = {-1.0f + 4.0f * unit(seed), -1.0f + 4.0f * unit(seed), 2.0f * unit(seed)};
    for (uint32_t f = 0; f < 3 + o; f++) {
      const float size = f % 7 == 0 ? 0.8f : 0.1f;
      for (int v = 0; v < 3; v++) {
        for (int a = 0; a < 3; a++) xyz.push_back(base[a] + 0.5f * unit(seed) + size * (unit(seed) - 0.5f));
        tris.push_back((uint32_t)(xyz.size() / 3 - 1));
        vobj.push_back(o + 1);
      }
    }
  }
  const float bad[12] = {NAN, 0.1f, 0.1f, 0.2f, INFINITY, 0.1f, 0.1f, 0.2f, 1e30f, -3e38f, 3e38f, 0.0f};
  const uint32_t nv0 = (uint32_t)(xyz.size() / 3);
  xyz.insert(xyz.end(), bad, bad + 12);
  for (int i = 0; i < 4; i++) vobj.push_back(41);
  const uint32_t extra[] = {nv0, 0, 1, nv0 + 1, 2, 3, 5, 5, 6, nv0 + 2, nv0 + 3, 7, nv0 + 2, nv0 + 3, nv0 + 2};
  tris.insert(tris.end(), extra, extra + 15);
  const uint64_t nv = xyz.size() / 3, nf = tris.size() / 3;
  std::vector<int32_t> cls(nobj);
  for (uint32_t o = 0; o < nobj; o++) cls[o] = o % 5 == 2 ? -1 : (int32_t)(o % 50);

  sf_grid g;
  std::memset(&g, 0, sizeof(g));
  g.h.nx = 37; g.h.ny = 41; g.h.nz = 23;
  g.h.voxel_size = 0.05f;
  g.h.lo_voxel[0] = -10; g.h.lo_voxel[1] = -12; g.h.lo_voxel[2] = -3;
  std::vector<uint8_t> weight((size_t)g.h.nx * g.h.ny * g.h.nz);
  for (auto& w : weight) w = (uint8_t)(rnd(seed) % 3);
  g.weight = weight.data();

  sf_objvox_params p;
  sf_objvox_params_default(&p);
  uint64_t total = 0;
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, &g, &p, -1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &total) == SF_OK);
  CHECK(total == 33);   // 32 of the 40 have a class, and so has the object of the one face that spans 3e38
  const size_t per = 2 * 27000;
  std::vector<uint8_t> data(total * per), label(total);
  std::vector<int32_t> oid(total);
  std::vector<float> origin(3 * total), cell(total);
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, &g, &p, -1, 0, total, data.data(), label.data(), oid.data(), origin.data(),
                           cell.data(), &total) == SF_OK);
  uint64_t occ = 0, known = 0;
  for (uint64_t s = 0; s < total; s++)
    for (size_t i = 0; i < 27000; i++) { occ += data[s * per + i]; known += data[s * per + 27000 + i]; CHECK(data[s * per + i] <= data[s * per + 27000 + i]); }
  CHECK(occ > 1000 && known > occ && known < total * 27000);
  // a page in the middle and one past the end write the same bytes / nothing
  std::vector<uint8_t> page(3 * per, 9), plabel(3, 9);
  std::vector<int32_t> pid(3, -9);
  std::vector<float> porigin(9, -9.0f), pcell(3, -9.0f);
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, &g, &p, -1, total - 2, 3, page.data(), plabel.data(), pid.data(),
                           porigin.data(), pcell.data(), &total) == SF_OK);
  CHECK(std::memcmp(page.data(), data.data() + (total - 2) * per, 2 * per) == 0 && page[2 * per] == 9 && pid[1] == oid[total - 1] && pid[2] == -9);
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, &g, &p, -1, total + 3, 3, page.data(), plabel.data(), pid.data(),
                           porigin.data(), pcell.data(), &total) == SF_OK);
  CHECK(page[0] == data[(total - 2) * per]);
  // every object, a small cube, no grid, a grid without a node
  p.all_objects = 1; p.dim = 7; p.fit = 5; p.min_faces = 10;
  uint64_t total2 = 0;
  std::vector<uint8_t> small(nobj * 2 * 343), slabel(nobj);
  std::vector<int32_t> sid(nobj);
  std::vector<float> sorigin(3 * nobj), scell(nobj);
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, nullptr, &p, -1, 0, nobj, small.data(), slabel.data(), sid.data(),
                           sorigin.data(), scell.data(), &total2) == SF_OK);
  CHECK(total2 == 33 && sid[0] == 7);
  for (size_t i = 343; i < 686; i++) CHECK(small[i] == 1);
  sf_grid e = g;
  e.h.nx = 0;
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, &e, &p, -1, 0, nobj, small.data(), slabel.data(), sid.data(),
                           sorigin.data(), scell.data(), &total2) == SF_OK);
  for (size_t i = 0; i < 343; i++) CHECK(small[i] == small[343 + i]);
  uint64_t count = 0;
  CHECK(sf_objvox_plan(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, &p, sid.data(), sorigin.data(), scell.data(), 4, &count) == SF_OK && count == 33);
  std::vector<uint32_t> fobj(nf), counts(nobj + 1), offsets(nobj + 1), list(nf);
  CHECK(sf_objvox_stage_faces(xyz.data(), nv, tris.data(), nf, vobj.data(), nobj, -1, fobj.data(), counts.data(), offsets.data(), list.data(), nf, &count) == SF_OK);
  CHECK(count == nf - 4 && fobj[nf - 1] == 0 && fobj[nf - 2] == 41 && counts[41] == 1 && counts[42] == 0);
  // refusals, an empty mesh, the device
  tris[4] = (uint32_t)nv;
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, nullptr, &p, -1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &total2) ==
        SF_ERR_INVALID_ARG);
  tris[4] = 1;
  p.dim = 33;
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, nullptr, &p, -1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &total2) ==
        SF_ERR_INVALID_ARG);
  p.dim = 30; p.fit = 24;
  CHECK(sf_objvox_voxelize(nullptr, 0, nullptr, 0, nullptr, cls.data(), nobj, nullptr, &p, -1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &total2) == SF_OK);
  CHECK(total2 == 0);
  CHECK(sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, nullptr, &p, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &total2) ==
        SF_ERR_DEVICE);
  std::printf("object voxels host: ok\n");
  return 0;
}
