// voxel_labels.cpp -- the voxel task's data from a scan (include/scanfuse.h "Voxel-task data"): the entry points, their checks,
// and the host path -- the rule of voxel_labels_internal.h over the same 8^3-node tiles as the kernels of voxel_labels.hip, on at most 16 threads.  It
// writes the bytes the device writes: the winner of a node is a minimum over a total order, so neither the order of a tile's list nor who walks it shows.
// What reads the result is Tasks/SemanticVoxelLabeling/torch/provider.lua:59-97 (datasets `data` and `label`; label 0 empty, 255 unannotated) and
// BenchmarkScripts/3d_helpers/export_semantic_label_grid_for_evaluation.py:35-47 (the per-vertex read of a [z][y][x] grid).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "common.h"
#include "voxel_labels_internal.h"

namespace {

using sf::vl::FaceRec;
using sf::vl::Geo;
using sf::vl::TILE;

constexpr int MAX_THREADS = 16;

int pool_size(uint64_t jobs) {
  int n = sf::usable_cpus();
  if (n > MAX_THREADS) n = MAX_THREADS;
  if ((uint64_t)n > jobs) n = (int)jobs;
  return n < 1 ? 1 : n;
}

template <typename F>
void parallel_for(uint64_t jobs, F&& body) {   // body(job): jobs are handed out one by one
  const int n = pool_size(jobs);
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

// the geometry of a grid the stage accepts: dims >= 0, a voxel size, node coordinates that binary32 holds exactly, at most 2^40 nodes
int check_geometry(const sf_grid_header* h, const char* who, uint64_t* n_nodes) {
  if (h->nx < 0 || h->ny < 0 || h->nz < 0 || !std::isfinite(h->voxel_size) || !(h->voxel_size > 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "%s: dims %d x %d x %d, voxel_size %g", who, h->nx, h->ny, h->nz, (double)h->voxel_size);
  const int32_t dims[3] = {h->nx, h->ny, h->nz};
  for (int a = 0; a < 3; a++) {
    const int64_t lo = h->lo_voxel[a], hi = lo + dims[a];
    if (lo < -(int64_t)sf::vl::MAX_COORD || hi > (int64_t)sf::vl::MAX_COORD)
      return sf::fail(SF_ERR_INVALID_ARG, "%s: nodes %lld .. %lld on axis %d leave +-2^22", who, (long long)lo, (long long)hi, a);
  }
  const uint64_t nxy = (uint64_t)h->nx * (uint64_t)h->ny;
  if (nxy > (1ull << 40) || (nxy != 0 && (uint64_t)h->nz > (1ull << 40) / nxy)) return sf::fail(SF_ERR_INVALID_ARG, "%s: more than 2^40 nodes", who);
  *n_nodes = nxy * (uint64_t)h->nz;
  return SF_OK;
}

int check_search(const sf_grid_header* h, const float* xyz, uint64_t nv, const uint32_t* tris, uint64_t nf, float band, const char* who, uint64_t* n_nodes,
                 float* t, float* r2) {
  if (!h) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  int rc = check_geometry(h, who, n_nodes);
  if (rc != SF_OK) return rc;
  if (!std::isfinite(band) || !(band > 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "%s: band %g", who, (double)band);
  *t = band * h->voxel_size;
  *r2 = *t * *t;
  if (!std::isfinite(*r2) || !(*r2 > 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "%s: (band * voxel_size)^2 = %g", who, (double)*r2);
  if ((nf && !tris) || (nv && !xyz)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (nv > (1ull << 32) || nf > (1ull << 31) - 1) return sf::fail(SF_ERR_INVALID_ARG, "%s: %llu vertices, %llu faces", who, (unsigned long long)nv, (unsigned long long)nf);
  for (uint64_t i = 0; i < 3 * nf; i++)
    if (tris[i] >= nv) return sf::fail(SF_ERR_INVALID_ARG, "%s: face %llu names vertex %u of %llu", who, (unsigned long long)(i / 3), tris[i], (unsigned long long)nv);
  return SF_OK;
}

struct Bins {
  std::vector<FaceRec> rec;
  std::vector<uint32_t> counts, offsets;
  std::vector<int32_t> list;
};

bool face_tiles(const FaceRec& r, const Geo& g, int32_t lo[3], int32_t hi[3]) {
  return r.valid && sf::vl::tile_range(r.lox, r.hix, g.voxel, g.lox, g.nx, &lo[0], &hi[0]) &&
         sf::vl::tile_range(r.loy, r.hiy, g.voxel, g.loy, g.ny, &lo[1], &hi[1]) && sf::vl::tile_range(r.loz, r.hiz, g.voxel, g.loz, g.nz, &lo[2], &hi[2]);
}

int host_bins(const Geo& g, const float* xyz, const uint32_t* tris, uint64_t nf, float t, Bins& b) {
  const uint64_t n_tiles = (uint64_t)g.tx * (uint64_t)g.ty * (uint64_t)g.tz;
  b.rec.resize(nf);
  const uint64_t chunk = 4096;
  parallel_for((nf + chunk - 1) / chunk, [&](uint64_t j) {
    const uint64_t e = std::min(nf, (j + 1) * chunk);
    for (uint64_t f = j * chunk; f < e; f++) b.rec[f] = sf::vl::make_record(xyz, tris, f, t);
  });
  b.counts.assign(n_tiles, 0);
  b.offsets.assign(n_tiles, 0);
  int32_t lo[3], hi[3];
  uint64_t total = 0;
  for (uint64_t f = 0; f < nf; f++) {
    if (!face_tiles(b.rec[f], g, lo, hi)) continue;
    for (int32_t z = lo[2]; z <= hi[2]; z++)
      for (int32_t y = lo[1]; y <= hi[1]; y++)
        for (int32_t x = lo[0]; x <= hi[0]; x++) b.counts[((size_t)z * g.ty + y) * g.tx + x]++;
    total += (uint64_t)(hi[0] - lo[0] + 1) * (uint64_t)(hi[1] - lo[1] + 1) * (uint64_t)(hi[2] - lo[2] + 1);
  }
  if (total >= (1ull << 32)) return sf::fail(SF_ERR_CAPACITY, "the nearest-face search: %llu (face, tile) pairs", (unsigned long long)total);
  uint32_t run = 0;
  for (uint64_t i = 0; i < n_tiles; i++) { b.offsets[i] = run; run += b.counts[i]; }
  b.list.resize(total);
  std::vector<uint32_t> cursor(b.offsets);
  for (uint64_t f = 0; f < nf; f++) {
    if (!face_tiles(b.rec[f], g, lo, hi)) continue;
    for (int32_t z = lo[2]; z <= hi[2]; z++)
      for (int32_t y = lo[1]; y <= hi[1]; y++)
        for (int32_t x = lo[0]; x <= hi[0]; x++) b.list[cursor[((size_t)z * g.ty + y) * g.tx + x]++] = (int32_t)f;
  }
  return SF_OK;
}

void host_tile(const Geo& g, const Bins& b, uint64_t tile, float r2, int32_t* face, float* dist2) {
  const int32_t tix = (int32_t)(tile % (uint64_t)g.tx), tiy = (int32_t)((tile / (uint64_t)g.tx) % (uint64_t)g.ty), tiz = (int32_t)(tile / ((uint64_t)g.tx * g.ty));
  const uint32_t n = b.counts[tile];
  const int32_t* list = b.list.data() + b.offsets[tile];
  const int32_t x1 = std::min(g.nx, (tix + 1) * TILE), y1 = std::min(g.ny, (tiy + 1) * TILE), z1 = std::min(g.nz, (tiz + 1) * TILE);
  for (int32_t z = tiz * TILE; z < z1; z++) {
    const float pz = sf::vl::node_pos(g.loz, z, g.voxel);
    for (int32_t y = tiy * TILE; y < y1; y++) {
      const float py = sf::vl::node_pos(g.loy, y, g.voxel);
      for (int32_t x = tix * TILE; x < x1; x++) {
        const float px = sf::vl::node_pos(g.lox, x, g.voxel);
        float best = std::numeric_limits<float>::infinity();
        int32_t bf = std::numeric_limits<int32_t>::max();
        for (uint32_t j = 0; j < n; j++) {
          const FaceRec& r = b.rec[list[j]];
          if (!sf::vl::in_box(r, px, py, pz)) continue;
          const float d = sf::vl::dist2(r, px, py, pz);
          if (sf::vl::better(d, r.f, r2, best, bf)) { best = d; bf = r.f; }
        }
        const size_t i = ((size_t)z * g.ny + y) * g.nx + x;
        face[i] = bf == std::numeric_limits<int32_t>::max() ? -1 : bf;
        if (dist2) dist2[i] = best;
      }
    }
  }
}

}  // namespace

SF_API void sf_voxlabel_params_default(sf_voxlabel_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->band = 0.8660254f;
  p->wx = 31; p->wy = 31; p->wz = 62;
  p->z0 = 0;
  p->z0_default = 1;
  p->stride = 1;
}

SF_API int sf_voxlabel_nearest_faces(const sf_grid_header* h, const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, float band,
                                     int device, int32_t* face, float* dist2) {
  uint64_t n_nodes = 0;
  float t = 0.0f, r2 = 0.0f;
  int rc = check_search(h, xyz, num_vertices, tris, num_faces, band, "sf_voxlabel_nearest_faces", &n_nodes, &t, &r2);
  if (rc != SF_OK) return rc;
  if (n_nodes && !face) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (device >= 0) return sf::vl::nearest_device(*h, xyz, num_vertices, tris, num_faces, t, r2, device, n_nodes ? face : nullptr, dist2, nullptr);
  if (n_nodes == 0) return SF_OK;
  const Geo g = sf::vl::make_geo(*h);
  try {
    Bins b;
    if ((rc = host_bins(g, xyz, tris, num_faces, t, b)) != SF_OK) return rc;
    parallel_for(b.counts.size(), [&](uint64_t tile) { host_tile(g, b, tile, r2, face, dist2); });
  } catch (const std::bad_alloc&) {
    return sf::fail(SF_ERR_IO, "sf_voxlabel_nearest_faces: out of memory");
  }
  return SF_OK;
}

SF_API int sf_voxlabel_stage_bins(const sf_grid_header* h, const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, float band,
                                  int device, uint32_t* counts, uint32_t* offsets, int32_t* list, uint64_t capacity, uint64_t* total) {
  uint64_t n_nodes = 0;
  float t = 0.0f, r2 = 0.0f;
  int rc = check_search(h, xyz, num_vertices, tris, num_faces, band, "sf_voxlabel_stage_bins", &n_nodes, &t, &r2);
  if (rc != SF_OK) return rc;
  if (device >= 0) {
    const sf::vl::BinsOut out = {counts, offsets, list, capacity, total};
    return sf::vl::nearest_device(*h, xyz, num_vertices, tris, num_faces, t, r2, device, nullptr, nullptr, &out);
  }
  if (total) *total = 0;
  if (n_nodes == 0) return SF_OK;
  try {
    Bins b;
    if ((rc = host_bins(sf::vl::make_geo(*h), xyz, tris, num_faces, t, b)) != SF_OK) return rc;
    if (total) *total = b.list.size();
    if (list && capacity < b.list.size()) return sf::fail(SF_ERR_BOUNDS, "the bin stage: %zu entries, capacity %llu", b.list.size(), (unsigned long long)capacity);
    if (counts) std::memcpy(counts, b.counts.data(), b.counts.size() * 4);
    if (offsets) std::memcpy(offsets, b.offsets.data(), b.offsets.size() * 4);
    if (list && !b.list.empty()) std::memcpy(list, b.list.data(), b.list.size() * 4);
  } catch (const std::bad_alloc&) {
    return sf::fail(SF_ERR_IO, "sf_voxlabel_stage_bins: out of memory");
  }
  return SF_OK;
}

SF_API int sf_voxlabel_labels(const int32_t* face, uint64_t num_nodes, const uint32_t* tris, uint64_t num_faces, uint64_t num_vertices,
                              const uint16_t* vertex_label, const uint8_t* vertex_instance, uint16_t* label, uint8_t* instance, uint8_t* byte_label) {
  if (num_nodes && !face) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (num_faces && (!tris || !vertex_label)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (instance && num_faces && !vertex_instance) return sf::fail(SF_ERR_INVALID_ARG, "sf_voxlabel_labels: an instance grid needs vertex instances");
  for (uint64_t i = 0; i < 3 * num_faces; i++)
    if (tris[i] >= num_vertices)
      return sf::fail(SF_ERR_INVALID_ARG, "sf_voxlabel_labels: face %llu names vertex %u of %llu", (unsigned long long)(i / 3), tris[i], (unsigned long long)num_vertices);
  for (uint64_t i = 0; i < num_nodes; i++)
    if (face[i] < -1 || (face[i] >= 0 && (uint64_t)face[i] >= num_faces))
      return sf::fail(SF_ERR_INVALID_ARG, "sf_voxlabel_labels: node %llu names face %d of %llu", (unsigned long long)i, face[i], (unsigned long long)num_faces);
  const uint64_t chunk = 1u << 16;
  parallel_for((num_nodes + chunk - 1) / chunk, [&](uint64_t j) {
    const uint64_t e = std::min(num_nodes, (j + 1) * chunk);
    for (uint64_t i = j * chunk; i < e; i++) {
      uint16_t l = 0;
      uint8_t in = 0, bl = 0;
      if (face[i] >= 0) {
        const uint32_t* v = tris + 3 * (uint64_t)face[i];
        // the value two vertices share, else the first vertex's
        l = vertex_label[v[1]] == vertex_label[v[2]] ? vertex_label[v[1]] : vertex_label[v[0]];
        if (vertex_instance) in = vertex_instance[v[1]] == vertex_instance[v[2]] ? vertex_instance[v[1]] : vertex_instance[v[0]];
        bl = (l == 0 || l > 254) ? (uint8_t)255 : (uint8_t)l;
      }
      if (label) label[i] = l;
      if (instance) instance[i] = in;
      if (byte_label) byte_label[i] = bl;
    }
  });
  return SF_OK;
}

SF_API int sf_voxlabel_sample_columns(const sf_grid* grid, const uint8_t* byte_label, const sf_voxlabel_params* p, int device, uint64_t first, uint64_t max_samples,
                                      float* data, uint8_t* label, int32_t* xy, uint64_t* total) {
  if (!grid || !p || !total) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  sf_grid_header h;
  int rc = sf_grid_info(grid, &h);
  if (rc != SF_OK) return rc;
  uint64_t n_nodes = 0;
  if ((rc = check_geometry(&h, "sf_voxlabel_sample_columns", &n_nodes)) != SF_OK) return rc;
  if (p->wx < 1 || p->wy < 1 || (p->wx & 1) == 0 || (p->wy & 1) == 0 || p->wz < 1 || p->stride < 1)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_voxlabel_sample_columns: window %d x %d x %d (x and y odd, all positive), stride %d", p->wx, p->wy, p->wz, p->stride);
  const uint64_t per = (uint64_t)p->wx * (uint64_t)p->wy;   // < 2^62
  if (per > (1ull << 40) || (uint64_t)p->wz > (1ull << 40) / per || (max_samples && per * (uint64_t)p->wz > (1ull << 60) / max_samples))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_voxlabel_sample_columns: %llu samples of %d x %d x %d do not fit", (unsigned long long)max_samples, p->wx, p->wy, p->wz);
  if (n_nodes && !byte_label) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (max_samples && (!data || !label || !xy)) return sf::fail(SF_ERR_INVALID_ARG, "sf_voxlabel_sample_columns: max_samples %llu without outputs", (unsigned long long)max_samples);
  const float* value = nullptr;
  if ((rc = sf_grid_data(grid, &value, nullptr)) != SF_OK) return rc;
  const int64_t z0 = p->z0_default ? -(int64_t)h.lo_voxel[2] : (int64_t)p->z0;
  const int32_t wx = p->wx, wy = p->wy, wz = p->wz;
  if (device >= 0) return sf::vl::sample_device(h, value, byte_label, wx, wy, wz, z0, p->stride, device, first, max_samples, data, label, xy, total);
  *total = 0;
  if (n_nodes == 0) return SF_OK;
  const int64_t zlo = std::max<int64_t>(z0, 0), zhi = std::min<int64_t>(z0 + wz, h.nz);
  std::vector<uint32_t> cols;
  try {
    for (int32_t y = 0; y < h.ny; y += p->stride)
      for (int32_t x = 0; x < h.nx; x += p->stride) {
        bool any = false;
        for (int64_t z = zlo; z < zhi && !any; z++) {
          const uint8_t v = byte_label[((size_t)z * h.ny + y) * h.nx + x];
          any = v != 0 && v != 255;
        }
        if (any) cols.push_back((uint32_t)((uint64_t)y * h.nx + x));
      }
  } catch (const std::bad_alloc&) {
    return sf::fail(SF_ERR_IO, "sf_voxlabel_sample_columns: out of memory");
  }
  *total = cols.size();
  if (first >= cols.size() || max_samples == 0) return SF_OK;
  const uint64_t n = std::min<uint64_t>(max_samples, cols.size() - first);
  const float ninf = -std::numeric_limits<float>::infinity();
  parallel_for(n * (uint64_t)wz, [&](uint64_t job) {
    const uint64_t s = job / (uint64_t)wz, k = job % (uint64_t)wz;
    const uint32_t col = cols[first + s];
    const int32_t x = (int32_t)(col % (uint32_t)h.nx), y = (int32_t)(col / (uint32_t)h.nx);
    const int64_t z = z0 + (int64_t)k;
    const bool zin = z >= 0 && z < h.nz;
    float* out = data + job * per;
    for (int32_t j = 0; j < wy; j++) {
      const int32_t yy = y + j - wy / 2;
      const bool rin = zin && yy >= 0 && yy < h.ny;
      const float* row = rin ? value + ((size_t)z * h.ny + yy) * h.nx : nullptr;
      for (int32_t i = 0; i < wx; i++) {
        const int32_t xx = x + i - wx / 2;
        out[(size_t)j * wx + i] = (rin && xx >= 0 && xx < h.nx) ? row[xx] : ninf;
      }
    }
    label[s * (uint64_t)wz + k] = zin ? byte_label[((size_t)z * h.ny + y) * h.nx + x] : (uint8_t)0;
    if (k == 0) { xy[2 * s] = x; xy[2 * s + 1] = y; }
  });
  return SF_OK;
}
