// freespace.cpp -- the pipeline's `freespace` stage (Server/scan_processor.py:15; "exe to call for computing occupancy grids", Server/config.py:20;
// product ${id}.grid, Server/config/scan_stages.json:43-47).  FreeSpace.exe and its file format are not in the reference tree: the rule and the
// format here are this library's statement, unpinned.  What the tree does say is what a consumer reads
// (Tasks/SemanticVoxelLabeling/torch/provider.lua:80-97: a float volume in voxel units, known = value >= -1;
// BenchmarkScripts/3d_helpers/export_semantic_label_grid_for_evaluation.py:35-47: [z][y][x] with a world2grid matrix).
//
// Host only, plain C++ over the library's own C interface: the plan (which box of blocks can a scan update at all), the stage (allocate the box,
// fuse the scan through sf_fuse_run, read the known box back) and the grid file.  The arithmetic of the rule is the fuser's: a voxel a frame sees in
// front of the surface by more than the truncation is integrated as sdf = +trunc with a weight, so known = weight > 0.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "common.h"

struct sf_grid {
  sf_grid_header h;
  std::vector<float> value;
  std::vector<uint8_t> weight;
};

namespace {

constexpr char GRID_MAGIC[8] = {'S', 'F', 'G', 'R', 'I', 'D', '1', '\0'};
constexpr size_t GRID_HEADER_BYTES = 8 + 12 + 4 + 12 + 64 + 8;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void fill_world2grid(sf_grid_header& h) {
  // g = w / voxel - lo + 0.5: floor(g) is the nearest lattice node (export_semantic_label_grid_for_evaluation.py:40-46 floors, then clamps)
  std::memset(h.world2grid, 0, sizeof(h.world2grid));
  for (int a = 0; a < 3; a++) {
    h.world2grid[5 * a] = 1.0f / h.voxel_size;
    h.world2grid[4 * a + 3] = 0.5f - (float)h.lo_voxel[a];
  }
  h.world2grid[15] = 1.0f;
}

// nx * ny * nz of non-negative dims without leaving 64 bits (every factor < 2^31); false beyond 2^40 voxels
bool voxel_count(const sf_grid_header& h, uint64_t* n) {
  const uint64_t nxy = (uint64_t)h.nx * (uint64_t)h.ny;
  if (nxy > (1ull << 40) || (nxy != 0 && (uint64_t)h.nz > (1ull << 40) / nxy)) return false;
  *n = nxy * (uint64_t)h.nz;
  return true;
}

// little-endian hosts only (as the .sens reader): the fields go out as they lie in memory
void put(std::vector<uint8_t>& b, const void* p, size_t n) { b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n); }

}  // namespace

SF_API void sf_freespace_params_default(sf_freespace_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->voxel_size = 0.05f;
  p->max_blocks = 1u << 21;
  p->every = 1;
}

SF_API int sf_freespace_plan(const sf_sens* s, const sf_freespace_params* fp, sf_params* fuser_params, int32_t lo_block[3], int32_t hi_block[3]) {
  if (!s || !fp || !fuser_params || !lo_block || !hi_block) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (!(fp->voxel_size > 0.0f) || !std::isfinite(fp->voxel_size) || fp->every < 1 || fp->max_blocks == 0)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_freespace_plan: voxel_size %g, every %d, max_blocks %u", (double)fp->voxel_size, fp->every, fp->max_blocks);
  if (std::memchr(fp->params_file, 0, sizeof(fp->params_file)) == nullptr) return sf::fail(SF_ERR_INVALID_ARG, "sf_freespace_plan: params_file is not terminated");
  sf_sens_info info;
  int rc = sf_sens_get_info(s, &info);
  if (rc != SF_OK) return rc;
  sf_params p;
  sf_params_default(&p);
  if (fp->params_file[0] && (rc = sf_params_load_file(fp->params_file, &p)) != SF_OK) return rc;
  p.voxel_size = fp->voxel_size;
  p.depth_width = (int32_t)info.depth_width; p.depth_height = (int32_t)info.depth_height;
  p.fx = info.depth_intrinsic[0]; p.fy = info.depth_intrinsic[5]; p.mx = info.depth_intrinsic[2]; p.my = info.depth_intrinsic[6];
  p.depth_shift = info.depth_shift;
  p.color_width = p.color_height = 0;   // geometry is all the stage reads back
  p.cfx = p.cfy = p.cmx = p.cmy = 0.0f;
  p.gc_enabled = 0;                     // garbage collection would free the free-space blocks, by its rule
  if (p.depth_width < 2 || p.depth_height < 2 || !(p.fx > 0.0f) || !(p.fy > 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_freespace_plan: depth frames %d x %d, focal lengths %g %g", p.depth_width, p.depth_height, (double)p.fx, (double)p.fy);
  // the effective integration camera, as sf_fuser_create derives it
  float W = (float)p.depth_width, H = (float)p.depth_height, fx = p.fx, fy = p.fy, mx = p.mx, my = p.my;
  if (p.integration_width > 1 && p.integration_height > 1 && (p.integration_width != p.depth_width || p.integration_height != p.depth_height)) {
    const float iw = (float)p.integration_width, ih = (float)p.integration_height;
    fx = p.fx * (iw / W); fy = p.fy * (ih / H);
    mx = p.mx * ((iw - 1.0f) / (W - 1.0f)); my = p.my * ((ih - 1.0f) / (H - 1.0f));
    W = iw; H = ih;
  }
  // every voxel the rule can update has 0 < z_cam < zfar and a pixel in (-1.5, W - 0.5) x (-1.5, H - 0.5) (oracle/tsdf_oracle.c:200-202): it lies within
  // R = zfar sqrt(1 + ax^2 + ay^2) of the camera centre
  const double maxd = p.max_integration_dist;
  const double zfar = maxd + (double)p.trunc_base + (double)p.trunc_scale * maxd;
  const double ax = std::fmax((double)mx + 1.5, (double)W - 0.5 - (double)mx) / (double)fx;
  const double ay = std::fmax((double)my + 1.5, (double)H - 0.5 - (double)my) / (double)fy;
  const double R = zfar * std::sqrt(1.0 + ax * ax + ay * ay);
  if (!(R > 0.0) || !std::isfinite(R)) return sf::fail(SF_ERR_INVALID_ARG, "sf_freespace_plan: the reach of a frame is %g m", R);
  double cmin[3] = {0, 0, 0}, cmax[3] = {0, 0, 0};
  uint64_t used = 0;
  for (uint64_t i = 0; i < info.num_frames; i += (uint64_t)fp->every) {
    float pose[16];
    int valid = 0;
    if ((rc = sf_sens_pose(s, i, pose, &valid)) != SF_OK) return rc;
    if (!valid) continue;
    const double c[3] = {pose[3], pose[7], pose[11]};
    if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2])) continue;
    for (int a = 0; a < 3; a++) {
      cmin[a] = used ? std::fmin(cmin[a], c[a]) : c[a];
      cmax[a] = used ? std::fmax(cmax[a], c[a]) : c[a];
    }
    used++;
  }
  if (!used) return sf::fail(SF_ERR_INVALID_ARG, "sf_freespace_plan: no frame of the scan has a valid pose");
  const double voxel = fp->voxel_size;
  double blocks = 1.0;
  for (int a = 0; a < 3; a++) {
    const double lo = std::floor((cmin[a] - R) / voxel) - 1.0, hi = std::ceil((cmax[a] + R) / voxel) + 1.0;
    const double lb = std::floor(lo / 8.0), hb = std::floor(hi / 8.0);
    if (!(lb >= -1048576.0) || !(hb <= 1048575.0))
      return sf::fail(SF_ERR_INVALID_ARG, "sf_freespace_plan: the box leaves the block range on axis %d (camera centres %g .. %g m at %g m voxels)", a, cmin[a], cmax[a], voxel);
    lo_block[a] = (int32_t)lb;
    hi_block[a] = (int32_t)hb;
    blocks *= hb - lb + 1.0;
  }
  if (blocks > (double)fp->max_blocks)
    return sf::fail(SF_ERR_CAPACITY, "sf_freespace_plan: the box holds %.0f blocks, max_blocks is %u (%.1f GiB of voxels; a larger voxel_size or max_blocks)", blocks,
                    fp->max_blocks, blocks * 4096.0 / 1073741824.0);
  // the heap: the box, and some room for blocks the allocation walk may name on its rim; the table: 2.5 slots per block
  const uint64_t nb = (uint64_t)blocks;
  p.num_sdf_blocks = (uint32_t)(nb + nb / 64 + 1024);
  p.hash_bucket_size = 10;
  p.hash_num_buckets = (uint32_t)(p.num_sdf_blocks / 4 + 1024);
  *fuser_params = p;
  return SF_OK;
}

SF_API int sf_grid_create(const sf_grid_header* h, const float* value, const uint8_t* weight, sf_grid** out) {
  if (!h || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *out = nullptr;
  if (h->nx < 0 || h->ny < 0 || h->nz < 0 || !std::isfinite(h->voxel_size) || !(h->voxel_size > 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_grid_create: dims %d x %d x %d, voxel_size %g", h->nx, h->ny, h->nz, (double)h->voxel_size);
  uint64_t n = 0;
  if (!voxel_count(*h, &n)) return sf::fail(SF_ERR_INVALID_ARG, "sf_grid_create: more than 2^40 voxels");
  if (n && (!value || !weight)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  sf_grid* g = new (std::nothrow) sf_grid();
  if (!g) return sf::fail(SF_ERR_IO, "out of memory");
  g->h = *h;
  try {
    g->value.assign(value, value + n);
    g->weight.assign(weight, weight + n);
  } catch (const std::bad_alloc&) {
    delete g;
    return sf::fail(SF_ERR_IO, "sf_grid_create: out of memory for %llu voxels", (unsigned long long)n);
  }
  *out = g;
  return SF_OK;
}

SF_API int sf_grid_info(const sf_grid* g, sf_grid_header* out) {
  if (!g || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *out = g->h;
  return SF_OK;
}

SF_API int sf_grid_data(const sf_grid* g, const float** value, const uint8_t** weight) {
  if (!g) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (value) *value = g->value.data();
  if (weight) *weight = g->weight.data();
  return SF_OK;
}

SF_API void sf_grid_free(sf_grid* g) { delete g; }

SF_API int sf_grid_save(const sf_grid* g, const char* path) {
  if (!g || !path) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  std::vector<uint8_t> head;
  put(head, GRID_MAGIC, 8);
  put(head, &g->h.nx, 4); put(head, &g->h.ny, 4); put(head, &g->h.nz, 4);
  put(head, &g->h.voxel_size, 4);
  put(head, g->h.lo_voxel, 12);
  put(head, g->h.world2grid, 64);
  put(head, &g->h.frames_used, 8);
  FILE* f = std::fopen(path, "wb");
  if (!f) return sf::fail(SF_ERR_IO, "cannot write %s", path);
  bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
  if (ok && !g->value.empty()) ok = std::fwrite(g->value.data(), 4, g->value.size(), f) == g->value.size();
  if (ok && !g->weight.empty()) ok = std::fwrite(g->weight.data(), 1, g->weight.size(), f) == g->weight.size();
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) { std::remove(path); return sf::fail(SF_ERR_IO, "short write to %s", path); }
  return SF_OK;
}

SF_API int sf_grid_load(const char* path, sf_grid** out) {
  if (!path || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *out = nullptr;
  FILE* f = std::fopen(path, "rb");
  if (!f) return sf::fail(SF_ERR_IO, "cannot open %s", path);
  uint8_t head[GRID_HEADER_BYTES];
  if (std::fread(head, 1, sizeof(head), f) != sizeof(head)) { std::fclose(f); return sf::fail(SF_ERR_FORMAT, "%s: shorter than a grid header", path); }
  if (std::memcmp(head, GRID_MAGIC, 8) != 0) { std::fclose(f); return sf::fail(SF_ERR_FORMAT, "%s: not a grid file (magic)", path); }
  sf_grid_header h;
  std::memset(&h, 0, sizeof(h));
  std::memcpy(&h.nx, head + 8, 4); std::memcpy(&h.ny, head + 12, 4); std::memcpy(&h.nz, head + 16, 4);
  std::memcpy(&h.voxel_size, head + 20, 4);
  std::memcpy(h.lo_voxel, head + 24, 12);
  std::memcpy(h.world2grid, head + 36, 64);
  std::memcpy(&h.frames_used, head + 100, 8);
  if (h.nx < 0 || h.ny < 0 || h.nz < 0) { std::fclose(f); return sf::fail(SF_ERR_FORMAT, "%s: dims %d x %d x %d", path, h.nx, h.ny, h.nz); }
  if (!std::isfinite(h.voxel_size)) { std::fclose(f); return sf::fail(SF_ERR_FORMAT, "%s: voxel_size is not finite", path); }
  bool sized = std::fseek(f, 0, SEEK_END) == 0;
  const long long end = sized ? (long long)std::ftell(f) : -1;
  sized = sized && end >= 0 && std::fseek(f, (long)GRID_HEADER_BYTES, SEEK_SET) == 0;
  uint64_t n = 0;
  const bool fits = voxel_count(h, &n);
  if (!sized || !fits || (uint64_t)end != GRID_HEADER_BYTES + 5ull * n) {
    std::fclose(f);
    return sf::fail(SF_ERR_FORMAT, "%s: %lld bytes do not hold a %d x %d x %d grid", path, end, h.nx, h.ny, h.nz);
  }
  sf_grid* g = new (std::nothrow) sf_grid();
  if (!g) { std::fclose(f); return sf::fail(SF_ERR_IO, "out of memory"); }
  g->h = h;
  bool ok = true;
  try {
    g->value.resize(n);
    g->weight.resize(n);
  } catch (const std::bad_alloc&) {
    ok = false;
  }
  if (ok && n) ok = std::fread(g->value.data(), 4, n, f) == n && std::fread(g->weight.data(), 1, n, f) == n;
  std::fclose(f);
  if (!ok) { delete g; return sf::fail(SF_ERR_IO, "%s: could not read %llu voxels", path, (unsigned long long)n); }
  *out = g;
  return SF_OK;
}

SF_API int sf_freespace_sens(const sf_sens* s, const sf_freespace_params* fp, int device, int decode_threads, sf_grid** out, sf_freespace_stats* stats) {
  if (!s || !fp || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *out = nullptr;
  sf_freespace_stats st;
  std::memset(&st, 0, sizeof(st));
  const double t0 = now_s();
  sf_params p;
  int32_t lo[3], hi[3];
  int rc = sf_freespace_plan(s, fp, &p, lo, hi);
  if (rc != SF_OK) return rc;
  st.box_blocks = (uint64_t)(hi[0] - lo[0] + 1) * (uint64_t)(hi[1] - lo[1] + 1) * (uint64_t)(hi[2] - lo[2] + 1);
  for (int a = 0; a < 3; a++) { st.lo_block[a] = lo[a]; st.hi_block[a] = hi[a]; }
  const double t1 = now_s();
  st.seconds_plan = t1 - t0;
  sf_fuser* f = nullptr;
  if ((rc = sf_fuser_create(&p, device, &f)) != SF_OK) return rc;   // SF_ERR_DEVICE without a GPU: the fuser has no host fall-back
  const double t2 = now_s();
  st.seconds_create = t2 - t1;
  sf_grid* g = nullptr;
  do {
    uint64_t made = 0;
    if ((rc = sf_fuser_allocate_box(f, lo, hi, &made)) != SF_OK) break;
    const double t3 = now_s();
    st.seconds_allocate = t3 - t2;
    sf_sens_info info;
    if ((rc = sf_sens_get_info(s, &info)) != SF_OK) break;
    if (fp->every == 1) {
      sf_run_stats rs;
      if ((rc = sf_fuse_run(f, s, 0, 0, decode_threads, &rs)) != SF_OK) break;
      st.frames_used = rs.frames_integrated;
    } else {
      // sf_fuse_run takes a range of frames: a stride is one call per frame (a pass per frame instead of one per 32)
      for (uint64_t i = 0; i < info.num_frames && rc == SF_OK; i += (uint64_t)fp->every) {
        sf_run_stats rs;
        rc = sf_fuse_run(f, s, i, i + 1, decode_threads, &rs);
        if (rc == SF_OK) st.frames_used += rs.frames_integrated;
      }
      if (rc != SF_OK) break;
    }
    sf_stats fs;
    if ((rc = sf_fuser_stats(f, &fs)) != SF_OK) break;
    if (fs.alloc_failures != 0) {
      rc = sf::fail(SF_ERR_CAPACITY, "sf_freespace_sens: %u blocks could not be allocated beside the box of %llu", fs.alloc_failures, (unsigned long long)st.box_blocks);
      break;
    }
    const double t4 = now_s();
    st.seconds_fuse = t4 - t3;
    int32_t klo[3] = {0, 0, 0}, khi[3] = {0, 0, 0};
    uint64_t known = 0;
    if ((rc = sf_fuser_known_bounds(f, klo, khi, &known)) != SF_OK) break;
    const double t5 = now_s();
    st.seconds_bounds = t5 - t4;
    st.known = known;
    sf_grid_header h;
    std::memset(&h, 0, sizeof(h));
    h.voxel_size = p.voxel_size;
    h.frames_used = st.frames_used;
    g = new (std::nothrow) sf_grid();
    if (!g) { rc = sf::fail(SF_ERR_IO, "out of memory"); break; }
    if (known) {
      const int32_t dims[3] = {khi[0] - klo[0] + 1, khi[1] - klo[1] + 1, khi[2] - klo[2] + 1};
      h.nx = dims[0]; h.ny = dims[1]; h.nz = dims[2];
      for (int a = 0; a < 3; a++) h.lo_voxel[a] = klo[a];
      const size_t n = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
      try {
        g->value.resize(n);
        g->weight.resize(n);
      } catch (const std::bad_alloc&) {
        rc = sf::fail(SF_ERR_IO, "sf_freespace_sens: out of memory for %zu voxels", n);
        break;
      }
      if ((rc = sf_fuser_export_dense(f, klo, dims, 1, g->value.data(), g->weight.data(), nullptr, 0)) != SF_OK) break;
      // free: known and at least the smallest truncation in front of what the frames saw; near: the other known voxels
      const float thr = p.trunc_base / p.voxel_size;
      uint64_t fr = 0;
      for (size_t i = 0; i < n; i++) fr += (g->weight[i] != 0 && g->value[i] >= thr) ? 1u : 0u;
      st.free_voxels = fr;
      st.near_voxels = known - fr;
    }
    fill_world2grid(h);
    g->h = h;
    st.seconds_export = now_s() - t5;
  } while (false);
  sf_fuser_destroy(f);
  if (rc != SF_OK) { delete g; return rc; }
  st.seconds_total = now_s() - t0;
  if (stats) *stats = st;
  *out = g;
  return SF_OK;
}
