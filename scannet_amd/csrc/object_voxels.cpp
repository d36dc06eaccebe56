// object_voxels.cpp -- the object tasks' data from a scan (include/scanfuse.h "Object-task data"): the entry points, their checks,
// the class lookup, and the host path -- the rule of object_voxels_internal.h, object by object on at most 16 threads.  It writes the bytes the device
// writes: occupancy is an OR over faces, so neither the order of an object's list nor who walks it shows.  What reads the result is
// Tasks/ObjectClassification/torch/provider.lua:40-47 and Tasks/ObjectRetrieval/generate_feat.lua:74-81,101-109 (datasets `data` and `label`).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "object_voxels_internal.h"

namespace {

using sf::ov::Cube;
using sf::ov::GridRef;
using sf::ov::Kept;
using sf::ov::QTri;

constexpr int MAX_THREADS = 16;

template <typename F>
void parallel_for(uint64_t jobs, F&& body) {   // body(job): jobs are handed out one by one
  int n = sf::usable_cpus();
  if (n > MAX_THREADS) n = MAX_THREADS;
  if ((uint64_t)n > jobs) n = (int)jobs;
  if (n < 1) n = 1;
  std::atomic<uint64_t> next{0};
  auto run = [&]() {
    for (uint64_t j = next.fetch_add(1); j < jobs; j = next.fetch_add(1)) body(j);
  };
  if (n == 1) { run(); return; }
  std::vector<std::thread> pool;
  for (int i = 1; i < n; i++) pool.emplace_back(run);
  run();
  for (auto& t : pool) t.join();
}

int check_mesh(const float* xyz, uint64_t nv, const uint32_t* tris, uint64_t nf, const uint32_t* vertex_object, uint32_t num_objects, const char* who) {
  if ((nf && !tris) || (nv && (!xyz || !vertex_object))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (nv > (1ull << 32) || nf > (1ull << 31)) return sf::fail(SF_ERR_INVALID_ARG, "%s: %llu vertices, %llu faces", who, (unsigned long long)nv, (unsigned long long)nf);
  if (num_objects > sf::ov::MAX_OBJECT) return sf::fail(SF_ERR_INVALID_ARG, "%s: %u objects (object ids go up to 65535)", who, num_objects);
  for (uint64_t i = 0; i < 3 * nf; i++)
    if (tris[i] >= nv) return sf::fail(SF_ERR_INVALID_ARG, "%s: face %llu names vertex %u of %llu", who, (unsigned long long)(i / 3), tris[i], (unsigned long long)nv);
  for (uint64_t v = 0; v < nv; v++)
    if (vertex_object[v] > num_objects)
      return sf::fail(SF_ERR_INVALID_ARG, "%s: vertex %llu carries object %u of %u", who, (unsigned long long)v, vertex_object[v], num_objects);
  return SF_OK;
}

int check_params(const sf_objvox_params* p, const int32_t* object_class, uint32_t num_objects, const char* who) {
  if (!p || (num_objects && !object_class)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (p->dim < 1 || p->dim > sf::ov::MAX_DIM || p->fit < 1 || p->fit > p->dim)
    return sf::fail(SF_ERR_INVALID_ARG, "%s: dim %d (1 .. 32), fit %d (1 .. dim)", who, p->dim, p->fit);
  for (uint32_t i = 0; i < num_objects; i++)
    if (object_class[i] < -1 || object_class[i] > 254) return sf::fail(SF_ERR_INVALID_ARG, "%s: object %u has class %d (-1 .. 254)", who, i, object_class[i]);
  return SF_OK;
}

struct Groups {   // the faces of every object: indexed by the vertex_object value
  std::vector<uint32_t> face_object, counts, offsets, list;
};

void host_groups(const float* xyz, const uint32_t* tris, uint64_t nf, const uint32_t* vertex_object, uint32_t num_objects, Groups& g) {
  g.face_object.assign(nf, 0);
  g.counts.assign((size_t)num_objects + 1, 0);
  g.offsets.assign((size_t)num_objects + 1, 0);
  for (uint64_t f = 0; f < nf; f++) {
    bool counts = false;
    const uint32_t o = sf::ov::face_object(xyz, tris, vertex_object, f, &counts);
    if (!counts || o == 0) continue;
    g.face_object[f] = o;
    g.counts[o]++;
  }
  uint32_t run = 0;
  for (size_t i = 0; i < g.counts.size(); i++) { g.offsets[i] = run; run += g.counts[i]; }
  g.list.resize(run);
  std::vector<uint32_t> cursor(g.offsets);
  for (uint64_t f = 0; f < nf; f++)
    if (g.face_object[f]) g.list[cursor[g.face_object[f]]++] = (uint32_t)f;
}

Cube host_cube(const float* xyz, const uint32_t* tris, const Groups& g, uint32_t o, const sf_objvox_params& p) {
  const float inf = std::numeric_limits<float>::infinity();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t j = 0; j < g.counts[o]; j++) {
    const uint64_t f = g.list[g.offsets[o] + j];
    for (int v = 0; v < 3; v++)
      for (int a = 0; a < 3; a++) {
        const float x = xyz[3 * (uint64_t)tris[3 * f + v] + a];
        lo[a] = fminf(lo[a], x);
        hi[a] = fmaxf(hi[a], x);
      }
  }
  return sf::ov::make_cube(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], p.dim, p.fit);
}

// the kept objects in ascending objectId order
void host_kept(const float* xyz, const uint32_t* tris, const Groups& g, const int32_t* object_class, uint32_t num_objects, const sf_objvox_params& p,
               std::vector<Kept>& out) {
  for (uint32_t o = 1; o <= num_objects; o++) {
    const int32_t cls = object_class[o - 1];
    if (g.counts[o] == 0 || (cls < 0 && !p.all_objects)) continue;
    const Cube q = host_cube(xyz, tris, g, o, p);
    if (!sf::ov::kept(p, cls, g.counts[o], q)) continue;
    out.push_back(Kept{o, sf::ov::label_of(cls), g.offsets[o], g.counts[o], q});
  }
}

void host_object(const float* xyz, const uint32_t* tris, const Groups& g, const Kept& k, const GridRef& grid, int32_t dim, uint8_t* data) {
  const size_t cells = (size_t)dim * dim * dim;
  uint8_t* occ = data;
  uint8_t* known = data + cells;
  std::memset(occ, 0, cells);
  for (uint32_t j = 0; j < k.count; j++) {
    const QTri t = sf::ov::quantise_face(xyz, tris, g.list[k.first + j], k.cube, dim);
    if (sf::ov::no_area(t)) continue;
    int32_t x0, x1, y0, y1, z0, z1;
    sf::ov::cell_range(sf::ov::min3(t.ax, t.bx, t.cx), sf::ov::max3(t.ax, t.bx, t.cx), dim, &x0, &x1);
    sf::ov::cell_range(sf::ov::min3(t.ay, t.by, t.cy), sf::ov::max3(t.ay, t.by, t.cy), dim, &y0, &y1);
    sf::ov::cell_range(sf::ov::min3(t.az, t.bz, t.cz), sf::ov::max3(t.az, t.bz, t.cz), dim, &z0, &z1);
    for (int32_t z = z0; z <= z1; z++)
      for (int32_t y = y0; y <= y1; y++)
        for (int32_t x = x0; x <= x1; x++) {
          uint8_t& cell = occ[((size_t)z * dim + y) * dim + x];
          if (!cell && sf::ov::meets(t, x, y, z)) cell = 1;
        }
  }
  for (int32_t z = 0; z < dim; z++) {
    bool zin = false, yin = false, xin = false;
    const int32_t gz = grid.mode ? sf::ov::grid_node(k.cube.oz, k.cube.c, z, grid.voxel, grid.loz, grid.nz, &zin) : 0;
    for (int32_t y = 0; y < dim; y++) {
      const int32_t gy = grid.mode ? sf::ov::grid_node(k.cube.oy, k.cube.c, y, grid.voxel, grid.loy, grid.ny, &yin) : 0;
      for (int32_t x = 0; x < dim; x++) {
        const size_t i = ((size_t)z * dim + y) * dim + x;
        uint8_t v = 1;
        if (grid.mode) {
          const int32_t gx = sf::ov::grid_node(k.cube.ox, k.cube.c, x, grid.voxel, grid.lox, grid.nx, &xin);
          const uint8_t w = grid.mode == 1 ? grid.weight[((size_t)gz * grid.ny + gy) * grid.nx + gx] : (uint8_t)0;
          v = ((zin && yin && xin && w > 0) || occ[i]) ? 1 : 0;
        }
        known[i] = v;
      }
    }
  }
}

int grid_ref(const sf_grid* grid, GridRef& r, uint64_t* nodes) {
  std::memset(&r, 0, sizeof(r));
  *nodes = 0;
  if (!grid) return SF_OK;
  sf_grid_header h;
  int rc = sf_grid_info(grid, &h);
  if (rc != SF_OK) return rc;
  if (h.nx < 0 || h.ny < 0 || h.nz < 0 || !std::isfinite(h.voxel_size) || !(h.voxel_size > 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_objvox_voxelize: grid dims %d x %d x %d, voxel_size %g", h.nx, h.ny, h.nz, (double)h.voxel_size);
  const uint8_t* weight = nullptr;
  if ((rc = sf_grid_data(grid, nullptr, &weight)) != SF_OK) return rc;
  *nodes = (uint64_t)h.nx * (uint64_t)h.ny * (uint64_t)h.nz;
  r.mode = *nodes ? 1 : 2;
  r.nx = h.nx; r.ny = h.ny; r.nz = h.nz;
  r.lox = h.lo_voxel[0]; r.loy = h.lo_voxel[1]; r.loz = h.lo_voxel[2];
  r.voxel = h.voxel_size;
  r.weight = weight;
  return SF_OK;
}

bool slurp(const char* path, std::string& out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::stringstream ss;
  ss << f.rdbuf();
  out = ss.str();
  return true;
}

std::vector<std::string> split_tabs(const std::string& s) {
  std::vector<std::string> v;
  std::string cur;
  for (char c : s) { if (c == '\t') { v.push_back(cur); cur.clear(); } else if (c != '\r') cur.push_back(c); }
  v.push_back(cur);
  return v;
}

std::string trimmed(const std::string& s) {
  size_t b = 0, e = s.size();
  while (b < e && (s[b] == ' ' || s[b] == '\t' || s[b] == '\r')) b++;
  while (e > b && (s[e - 1] == ' ' || s[e - 1] == '\t' || s[e - 1] == '\r')) e--;
  return s.substr(b, e - b);
}

bool whole_int(const std::string& s, long long* v) {
  if (s.empty()) return false;
  char* end = nullptr;
  *v = std::strtoll(s.c_str(), &end, 10);
  return end && *end == '\0';
}

}  // namespace

SF_API void sf_objvox_params_default(sf_objvox_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->dim = 30;
  p->fit = 24;
  p->min_faces = 1;
  p->all_objects = 0;
}

SF_API int sf_objvox_classes(const char* object_labels, const char* label_map_tsv, const char* classes_txt, const char* label_from, const char* label_to,
                             uint32_t num_objects, int32_t* object_class) {
  if (!object_labels || !label_map_tsv || !classes_txt || (num_objects && !object_class)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  for (uint32_t i = 0; i < num_objects; i++) object_class[i] = -1;
  std::string text;
  if (!slurp(classes_txt, text)) return sf::fail(SF_ERR_IO, "failed to open file %s", classes_txt);
  std::unordered_map<std::string, int32_t> by_name;
  std::vector<long long> ids;
  {
    std::istringstream in(text);
    std::string line;
    while (std::getline(in, line)) {
      line = trimmed(line);
      if (line.empty()) continue;
      size_t e = 0;
      while (e < line.size() && line[e] != ' ' && line[e] != '\t') e++;
      long long id = 0;
      if (!whole_int(line.substr(0, e), &id) || id < 0 || id > 254) return sf::fail(SF_ERR_FORMAT, "%s: line \"%s\" (want <id> <name>, id 0 .. 254)", classes_txt, line.c_str());
      ids.push_back(id);
      by_name[trimmed(line.substr(e))] = (int32_t)id;
    }
  }
  if (!slurp(label_map_tsv, text)) return sf::fail(SF_ERR_IO, "error reading label mapping file %s", label_map_tsv);
  std::unordered_map<std::string, std::string> value_of;
  {
    std::istringstream in(text);
    std::string line;
    if (!std::getline(in, line)) return sf::fail(SF_ERR_FORMAT, "%s is empty", label_map_tsv);
    const std::vector<std::string> header = split_tabs(line);
    auto column = [&](const char* name) {
      for (size_t i = 0; i < header.size(); i++) if (header[i] == name) return (int)i;
      return -1;
    };
    int from = label_from ? column(label_from) : column("raw_category");
    if (from < 0 && !label_from) from = column("category");
    const int to = column(label_to ? label_to : "ShapeNetCore55");
    if (from < 0 || to < 0)
      return sf::fail(SF_ERR_FORMAT, "%s has no column %s", label_map_tsv, from < 0 ? (label_from ? label_from : "raw_category / category") : (label_to ? label_to : "ShapeNetCore55"));
    while (std::getline(in, line)) {
      const std::vector<std::string> parts = split_tabs(line);
      if ((int)parts.size() > from && (int)parts.size() > to && !parts[(size_t)from].empty())   // a key named twice: the last row, as a dictionary would
        value_of[parts[(size_t)from]] = trimmed(parts[(size_t)to]);
    }
  }
  std::istringstream in(object_labels);
  std::string line;
  while (std::getline(in, line)) {
    const size_t tab = line.find('\t');
    long long id = 0;
    if (tab == std::string::npos || !whole_int(line.substr(0, tab), &id)) return sf::fail(SF_ERR_FORMAT, "sf_objvox_classes: object line \"%s\" (want id<TAB>label)", line.c_str());
    if (id < 0 || id >= (long long)num_objects) continue;
    const auto it = value_of.find(line.substr(tab + 1));
    if (it == value_of.end() || it->second.empty()) continue;
    const auto bn = by_name.find(it->second);
    long long as_int = 0;
    if (bn != by_name.end()) object_class[id] = bn->second;
    else if (whole_int(it->second, &as_int) && std::find(ids.begin(), ids.end(), as_int) != ids.end()) object_class[id] = (int32_t)as_int;
  }
  return SF_OK;
}

SF_API int sf_objvox_stage_faces(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, const uint32_t* vertex_object, uint32_t num_objects,
                                 int device, uint32_t* face_object, uint32_t* counts, uint32_t* offsets, uint32_t* list, uint64_t capacity, uint64_t* total) {
  int rc = check_mesh(xyz, num_vertices, tris, num_faces, vertex_object, num_objects, "sf_objvox_stage_faces");
  if (rc != SF_OK) return rc;
  if (device >= 0) {
    const sf::ov::StageOut out = {face_object, counts, offsets, list, capacity, total};
    sf_objvox_params p;
    sf_objvox_params_default(&p);
    GridRef none;
    std::memset(&none, 0, sizeof(none));
    uint64_t unused = 0;
    return sf::ov::voxelize_device(xyz, num_vertices, tris, num_faces, vertex_object, nullptr, num_objects, none, 0, p, device, 0, 0, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, &unused, &out);
  }
  try {
    Groups g;
    host_groups(xyz, tris, num_faces, vertex_object, num_objects, g);
    if (total) *total = g.list.size();
    if (list && capacity < g.list.size()) return sf::fail(SF_ERR_BOUNDS, "the face stage: %zu entries, capacity %llu", g.list.size(), (unsigned long long)capacity);
    if (face_object && num_faces) std::memcpy(face_object, g.face_object.data(), num_faces * 4);
    if (counts) std::memcpy(counts, g.counts.data(), g.counts.size() * 4);
    if (offsets) std::memcpy(offsets, g.offsets.data(), g.offsets.size() * 4);
    if (list && !g.list.empty()) std::memcpy(list, g.list.data(), g.list.size() * 4);
  } catch (const std::bad_alloc&) {
    return sf::fail(SF_ERR_IO, "sf_objvox_stage_faces: out of memory");
  }
  return SF_OK;
}

SF_API int sf_objvox_plan(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, const uint32_t* vertex_object, const int32_t* object_class,
                          uint32_t num_objects, const sf_objvox_params* p, int32_t* object_id, float* origin, float* cell, uint64_t capacity, uint64_t* count) {
  if (!count) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  int rc = check_params(p, object_class, num_objects, "sf_objvox_plan");
  if (rc == SF_OK) rc = check_mesh(xyz, num_vertices, tris, num_faces, vertex_object, num_objects, "sf_objvox_plan");
  if (rc != SF_OK) return rc;
  try {
    Groups g;
    std::vector<Kept> kept;
    host_groups(xyz, tris, num_faces, vertex_object, num_objects, g);
    host_kept(xyz, tris, g, object_class, num_objects, *p, kept);
    *count = kept.size();
    for (uint64_t i = 0; i < kept.size() && i < capacity; i++) {
      if (object_id) object_id[i] = (int32_t)kept[i].object - 1;
      if (origin) { origin[3 * i] = kept[i].cube.ox; origin[3 * i + 1] = kept[i].cube.oy; origin[3 * i + 2] = kept[i].cube.oz; }
      if (cell) cell[i] = kept[i].cube.c;
    }
  } catch (const std::bad_alloc&) {
    return sf::fail(SF_ERR_IO, "sf_objvox_plan: out of memory");
  }
  return SF_OK;
}

SF_API int sf_objvox_voxelize(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, const uint32_t* vertex_object,
                              const int32_t* object_class, uint32_t num_objects, const sf_grid* grid, const sf_objvox_params* p, int device, uint64_t first,
                              uint64_t max_objects, uint8_t* data, uint8_t* label, int32_t* object_id, float* origin, float* cell, uint64_t* total) {
  if (!total) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  int rc = check_params(p, object_class, num_objects, "sf_objvox_voxelize");
  if (rc == SF_OK) rc = check_mesh(xyz, num_vertices, tris, num_faces, vertex_object, num_objects, "sf_objvox_voxelize");
  if (rc != SF_OK) return rc;
  if (max_objects && (!data || !label || !object_id || !origin || !cell))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_objvox_voxelize: max_objects %llu without outputs", (unsigned long long)max_objects);
  GridRef gr;
  uint64_t grid_nodes = 0;
  if ((rc = grid_ref(grid, gr, &grid_nodes)) != SF_OK) return rc;
  if (device >= 0)
    return sf::ov::voxelize_device(xyz, num_vertices, tris, num_faces, vertex_object, object_class, num_objects, gr, grid_nodes, *p, device, first, max_objects, data,
                                   label, object_id, origin, cell, total, nullptr);
  *total = 0;
  try {
    Groups g;
    std::vector<Kept> kept;
    host_groups(xyz, tris, num_faces, vertex_object, num_objects, g);
    host_kept(xyz, tris, g, object_class, num_objects, *p, kept);
    *total = kept.size();
    if (first >= kept.size() || max_objects == 0) return SF_OK;
    const uint64_t n = std::min<uint64_t>(max_objects, kept.size() - first);
    const size_t per = 2 * (size_t)p->dim * p->dim * p->dim;
    const int32_t dim = p->dim;
    parallel_for(n, [&](uint64_t s) {
      const Kept& k = kept[first + s];
      host_object(xyz, tris, g, k, gr, dim, data + s * per);
      label[s] = (uint8_t)k.label;
      object_id[s] = (int32_t)k.object - 1;
      origin[3 * s] = k.cube.ox; origin[3 * s + 1] = k.cube.oy; origin[3 * s + 2] = k.cube.oz;
      cell[s] = k.cube.c;
    });
  } catch (const std::bad_alloc&) {
    return sf::fail(SF_ERR_IO, "sf_objvox_voxelize: out of memory");
  }
  return SF_OK;
}
