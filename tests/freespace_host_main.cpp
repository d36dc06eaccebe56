// freespace_host_main.cpp -- the host side of the free-space stage (scannet_amd/csrc/freespace.cpp: the plan, the grid and its file) as a stand-alone
// program: tests/test_freespace.py builds it together with freespace.cpp using g++ -fsanitize=address,undefined and runs it once.
//
//   freespace_host_main <scratch directory>
//
// freespace.cpp speaks to the rest of the library through the C interface alone, so the few entry points it calls are stated here: a scan is a header
// and a list of poses, and there is no GPU (sf_fuser_create answers SF_ERR_DEVICE, as the library does on a machine without one).  The program runs the
// plan over scans with lost poses, with none that is valid and with a box beyond max_blocks, the stage (which must report SF_ERR_DEVICE and give no
// grid), and the grid reader over a written file, over every truncation of it, and over each malformed header sf_grid_load names.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../scannet_amd/csrc/common.h"

struct sf_sens {
  sf_sens_info info;
  std::vector<float> poses;   // 16 per frame
};

namespace sf {
std::string& last_error_ref() {
  static thread_local std::string err;
  return err;
}
}  // namespace sf

extern "C" {
const char* sf_last_error(void) { return sf::last_error_ref().c_str(); }
void sf_params_default(sf_params* p) {
  std::memset(p, 0, sizeof(*p));
  p->depth_width = 640; p->depth_height = 480;
  p->fx = p->fy = 577.87f; p->mx = 319.5f; p->my = 239.5f;
  p->depth_shift = 1000.0f; p->depth_min = 0.1f; p->depth_max = 6.0f;
  p->voxel_size = 0.004f; p->trunc_base = 0.06f; p->trunc_scale = 0.02f; p->max_integration_dist = 4.0f;
  p->weight_sample = 1; p->weight_max = 255; p->mc_thresh_factor = 10.0f;
  p->hash_num_buckets = 1u << 19; p->hash_bucket_size = 10; p->num_sdf_blocks = 1u << 20;
}
int sf_params_load_file(const char*, sf_params*) { return sf::fail(SF_ERR_IO, "no parameter files in this program"); }
int sf_sens_get_info(const sf_sens* s, sf_sens_info* out) { *out = s->info; return SF_OK; }
int sf_sens_pose(const sf_sens* s, uint64_t frame, float out16[16], int* valid) {
  if (frame >= s->info.num_frames) return sf::fail(SF_ERR_BOUNDS, "frame out of bounds");
  std::memcpy(out16, s->poses.data() + 16 * frame, 64);
  if (valid) *valid = out16[0] != -std::numeric_limits<float>::infinity();
  return SF_OK;
}
int sf_fuser_create(const sf_params*, int, sf_fuser** out) { *out = nullptr; return sf::fail(SF_ERR_DEVICE, "no HIP device: libscanfuse has no CPU fallback"); }
void sf_fuser_destroy(sf_fuser*) {}
int sf_fuser_allocate_box(sf_fuser*, const int32_t*, const int32_t*, uint64_t*) { return SF_ERR_DEVICE; }
int sf_fuser_known_bounds(sf_fuser*, int32_t*, int32_t*, uint64_t*) { return SF_ERR_DEVICE; }
int sf_fuser_export_dense(sf_fuser*, const int32_t*, const int32_t*, int, float*, uint8_t*, uint8_t*, int) { return SF_ERR_DEVICE; }
int sf_fuser_stats(sf_fuser*, sf_stats*) { return SF_ERR_DEVICE; }
int sf_fuse_run(sf_fuser*, const sf_sens*, uint64_t, uint64_t, int, sf_run_stats*) { return SF_ERR_DEVICE; }
}

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static sf_sens make_scan(int n, int lost_every) {
  sf_sens s;
  std::memset(&s.info, 0, sizeof(s.info));
  s.info.version = 4;
  s.info.depth_width = 160; s.info.depth_height = 120;
  s.info.depth_shift = 1000.0f;
  s.info.depth_intrinsic[0] = s.info.depth_intrinsic[5] = 144.4675f;
  s.info.depth_intrinsic[2] = 79.5f; s.info.depth_intrinsic[6] = 59.5f;
  s.info.depth_intrinsic[10] = s.info.depth_intrinsic[15] = 1.0f;
  s.info.num_frames = (uint64_t)n;
  const float ninf = -std::numeric_limits<float>::infinity();
  for (int i = 0; i < n; i++) {
    float T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    T[3] = 1.0f + 0.1f * (float)i; T[7] = -2.0f + 0.05f * (float)i; T[11] = 1.5f;
    if (lost_every && i % lost_every == 0) for (float& v : T) v = ninf;
    s.poses.insert(s.poses.end(), T, T + 16);
  }
  return s;
}

static bool write_file(const std::string& path, const std::vector<uint8_t>& b, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = n == 0 || std::fwrite(b.data(), 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];

  // ---- the plan
  sf_freespace_params fp;
  sf_freespace_params_default(&fp);
  EXPECT(fp.voxel_size == 0.05f && fp.max_blocks == (1u << 21) && fp.every == 1 && fp.params_file[0] == 0);
  sf_params p;
  int32_t lo[3], hi[3];
  {
    const sf_sens s = make_scan(40, 7);
    EXPECT(sf_freespace_plan(&s, &fp, &p, lo, hi) == SF_OK);
    // every camera centre used lies inside the box with the reach of a frame (> zfar = 4.14 m) to spare
    for (int i = 0; i < 40; i++) {
      if (i % 7 == 0) continue;
      const float c[3] = {s.poses[16 * i + 3], s.poses[16 * i + 7], s.poses[16 * i + 11]};
      for (int a = 0; a < 3; a++) EXPECT((double)lo[a] * 8 * 0.05 <= c[a] - 4.14 && (double)(hi[a] * 8 + 7) * 0.05 >= c[a] + 4.14);
    }
    const uint64_t blocks = (uint64_t)(hi[0] - lo[0] + 1) * (uint64_t)(hi[1] - lo[1] + 1) * (uint64_t)(hi[2] - lo[2] + 1);
    EXPECT(p.num_sdf_blocks >= blocks && p.voxel_size == 0.05f && p.depth_width == 160 && p.gc_enabled == 0 && p.color_width == 0);
    EXPECT((uint64_t)p.hash_num_buckets * p.hash_bucket_size >= 2 * blocks);
    int32_t lo3[3], hi3[3];
    fp.every = 3;
    EXPECT(sf_freespace_plan(&s, &fp, &p, lo3, hi3) == SF_OK);
    for (int a = 0; a < 3; a++) EXPECT(lo3[a] >= lo[a] && hi3[a] <= hi[a]);
    fp.every = 1;
    fp.max_blocks = 100;
    EXPECT(sf_freespace_plan(&s, &fp, &p, lo, hi) == SF_ERR_CAPACITY && std::strstr(sf_last_error(), "blocks") != nullptr);
    fp.max_blocks = 1u << 21;
    fp.voxel_size = std::numeric_limits<float>::quiet_NaN();
    EXPECT(sf_freespace_plan(&s, &fp, &p, lo, hi) == SF_ERR_INVALID_ARG);
    fp.voxel_size = 1e-9f;   // a box beyond the table's block range
    EXPECT(sf_freespace_plan(&s, &fp, &p, lo, hi) == SF_ERR_INVALID_ARG);
    fp.voxel_size = 0.05f;
    fp.every = 0;
    EXPECT(sf_freespace_plan(&s, &fp, &p, lo, hi) == SF_ERR_INVALID_ARG);
    fp.every = 1;
    std::memset(fp.params_file, 'x', sizeof(fp.params_file));   // not terminated
    EXPECT(sf_freespace_plan(&s, &fp, &p, lo, hi) == SF_ERR_INVALID_ARG);
    std::memset(fp.params_file, 0, sizeof(fp.params_file));
    EXPECT(sf_freespace_plan(nullptr, &fp, &p, lo, hi) == SF_ERR_INVALID_ARG);
  }
  {
    const sf_sens lost = make_scan(5, 1);   // every pose lost
    EXPECT(sf_freespace_plan(&lost, &fp, &p, lo, hi) == SF_ERR_INVALID_ARG);
    const sf_sens none = make_scan(0, 0);
    EXPECT(sf_freespace_plan(&none, &fp, &p, lo, hi) == SF_ERR_INVALID_ARG);
  }

  // ---- the stage without a GPU
  {
    const sf_sens s = make_scan(8, 0);
    sf_grid* g = reinterpret_cast<sf_grid*>(&failures);
    sf_freespace_stats st;
    EXPECT(sf_freespace_sens(&s, &fp, 0, 0, &g, &st) == SF_ERR_DEVICE && g == nullptr);
  }

  // ---- the grid and its file
  sf_grid_header h;
  std::memset(&h, 0, sizeof(h));
  h.nx = 5; h.ny = 4; h.nz = 3; h.voxel_size = 0.05f; h.lo_voxel[0] = -7; h.lo_voxel[1] = 2; h.lo_voxel[2] = -1; h.frames_used = 40;
  for (int a = 0; a < 3; a++) { h.world2grid[5 * a] = 1.0f / h.voxel_size; h.world2grid[4 * a + 3] = 0.5f - (float)h.lo_voxel[a]; }
  h.world2grid[15] = 1.0f;
  std::vector<float> value(60);
  std::vector<uint8_t> weight(60);
  for (int i = 0; i < 60; i++) { weight[i] = (uint8_t)(i % 3); value[i] = weight[i] ? 0.25f * (float)i - 3.0f : -std::numeric_limits<float>::infinity(); }
  sf_grid* g = nullptr;
  EXPECT(sf_grid_create(&h, value.data(), weight.data(), &g) == SF_OK && g != nullptr);
  const std::string good = dir + "/good.grid";
  EXPECT(sf_grid_save(g, good.c_str()) == SF_OK);
  sf_grid_free(g);
  sf_grid_free(nullptr);
  std::vector<uint8_t> bytes;
  {
    FILE* f = std::fopen(good.c_str(), "rb");
    EXPECT(f != nullptr);
    if (f) {
      uint8_t buf[4096];
      size_t n;
      while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
      std::fclose(f);
    }
  }
  const size_t HEAD = 108;
  EXPECT(bytes.size() == HEAD + 60 * 5);
  if (bytes.size() != HEAD + 60 * 5) { std::fprintf(stderr, "%d failures\n", failures); return 1; }
  g = nullptr;
  EXPECT(sf_grid_load(good.c_str(), &g) == SF_OK && g != nullptr);
  if (g) {
    sf_grid_header r;
    const float* rv = nullptr;
    const uint8_t* rw = nullptr;
    EXPECT(sf_grid_info(g, &r) == SF_OK && std::memcmp(&r, &h, sizeof(h)) == 0);
    EXPECT(sf_grid_data(g, &rv, &rw) == SF_OK && std::memcmp(rv, value.data(), 240) == 0 && std::memcmp(rw, weight.data(), 60) == 0);
    const std::string again = dir + "/again.grid";
    EXPECT(sf_grid_save(g, again.c_str()) == SF_OK);
    sf_grid_free(g);
  }
  const std::string bad = dir + "/bad.grid";
  auto refused = [&](const std::vector<uint8_t>& b, size_t n) {
    sf_grid* q = reinterpret_cast<sf_grid*>(&failures);
    return write_file(bad, b, n) && sf_grid_load(bad.c_str(), &q) == SF_ERR_FORMAT && q == nullptr;
  };
  for (size_t n = 0; n < bytes.size(); n++) EXPECT(refused(bytes, n));   // every truncation, the empty file among them
  {
    std::vector<uint8_t> b = bytes;
    b.push_back(0);
    EXPECT(refused(b, b.size()));   // a byte too many
    b = bytes; b[6] = '2';
    EXPECT(refused(b, b.size()));   // magic
    b = bytes; const int32_t neg = -5; std::memcpy(b.data() + 8, &neg, 4);
    EXPECT(refused(b, b.size()));   // a negative dimension
    b = bytes; const int32_t big = 0x7FFFFFFF; std::memcpy(b.data() + 8, &big, 4); std::memcpy(b.data() + 12, &big, 4); std::memcpy(b.data() + 16, &big, 4);
    EXPECT(refused(b, b.size()));   // dims whose product leaves 64 bits
    b = bytes; const int32_t two30 = 1 << 30; std::memcpy(b.data() + 8, &two30, 4); const int32_t one = 1; std::memcpy(b.data() + 12, &one, 4); std::memcpy(b.data() + 16, &one, 4);
    EXPECT(refused(b, b.size()));   // a size that does not match the file
    b = bytes; const float nan = std::numeric_limits<float>::quiet_NaN(); std::memcpy(b.data() + 20, &nan, 4);
    EXPECT(refused(b, b.size()));   // voxel_size not finite
    b = bytes; const float inf = std::numeric_limits<float>::infinity(); std::memcpy(b.data() + 20, &inf, 4);
    EXPECT(refused(b, b.size()));
  }
  {
    sf_grid* q = nullptr;
    EXPECT(sf_grid_load((dir + "/missing.grid").c_str(), &q) == SF_ERR_IO && q == nullptr);
    sf_grid_header z = h;
    z.nx = z.ny = z.nz = 0;   // the grid of a scan that observed nothing
    EXPECT(sf_grid_create(&z, nullptr, nullptr, &q) == SF_OK && q != nullptr);
    const std::string empty = dir + "/empty.grid";
    EXPECT(sf_grid_save(q, empty.c_str()) == SF_OK);
    sf_grid_free(q);
    q = nullptr;
    EXPECT(sf_grid_load(empty.c_str(), &q) == SF_OK && q != nullptr);
    sf_grid_free(q);
    z.nx = -1;
    EXPECT(sf_grid_create(&z, nullptr, nullptr, &q) == SF_ERR_INVALID_ARG);
  }
  if (failures) { std::fprintf(stderr, "%d failures\n", failures); return 1; }
  std::printf("freespace host: ok\n");
  return 0;
}
