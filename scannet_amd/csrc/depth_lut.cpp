// depth_lut.cpp -- calibrate_depth's batch modes (CameraParameterEstimation/apps/calibrate_depth/src/calibrate_depth.cpp): the C ABI of the
// table estimator and of the apply step, their host path (device -1: the rule of depth_lut_internal.h on host threads, the kernels' bits),
// the file readers (:112-362) and the tool's body (:647-894, :565-644).  DESIGN.md section 4k.
#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "depth_lut_internal.h"

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// fn(i) for i in [0, n) on up to `threads` host threads
template <class F>
void parallel_for(int n, int threads, F fn) {
  threads = std::max(1, std::min(threads, n));
  if (threads == 1) {
    for (int i = 0; i < n; i++) fn(i);
    return;
  }
  std::atomic<int> next(0);
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++)
    pool.emplace_back([&]() {
      for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
    });
  for (auto& th : pool) th.join();
}

// bsc::angle((0, 0, 1), n) in degrees (geometry.h:58-73): dot / len_1 * len_2 as written there, acosf (the overload is this library's reading)
float plane_angle(const float n[3]) {
  const float q = n[2] / 1.0f * sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  return (float)(acosf(q) * 180.0 / M_PI);
}

LutImage plane_of(const float T[16], const uint16_t* px) {   // :684-697
  LutImage im;
  std::memset(&im, 0, sizeof(im));
  im.px = px;
  const float n[3] = {T[2], T[6], T[10]}, p[3] = {T[3], T[7], T[11]};
  im.nx = n[0]; im.ny = n[1]; im.nz = n[2];
  im.d = -(n[0] * p[0] + n[1] * p[1] + n[2] * p[2]);
  im.used = plane_angle(n) > 25.0f ? 0 : 1;
  return im;
}

void host_add(sf_lut_estimator* e, int n, const LutImage* tab) {
  const LutGeom& g = e->g;
  const size_t ncell = (size_t)g.xres * g.yres;
  float* acc = e->acc.data();
  float* div = e->div.data();
  const long long work = (long long)n * g.w * g.h;
  parallel_for(g.yres, work < (1 << 18) ? 1 : sf::usable_cpus(), [&](int y) {   // table rows are independent
    for (int k = 0; k < n; k++) {
      if (!tab[k].used) continue;
      for (int dj = 0; dj < 2; dj++) {
        const int j = 2 * y + dj;
        const uint16_t* row = tab[k].px + (size_t)j * g.w;
        for (int i = 0; i < g.w; i++) {
          float ta, td;
          const int z = lut_sample(g, tab[k], i, j, row[i], ta, td);
          if (z == 0) continue;
          const size_t c = (size_t)z * ncell + (size_t)y * g.xres + (size_t)(i >> 1);
          acc[c] += ta;
          div[c] += td;
        }
      }
    }
  });
}

bool finite16(const float* m) {
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(m[i])) return false;
  return true;
}

int make_apply(const sf_lut* lut, int w, int h, int bitshift, LutApplyK& k) {
  if (!lut || !lut->data) return sf::fail(SF_ERR_INVALID_ARG, "NULL table");
  if (lut->xres < 1 || lut->yres < 1 || lut->zres < 1 || !(lut->max_dist > 0.0f) || !std::isfinite(lut->max_dist))
    return sf::fail(SF_ERR_INVALID_ARG, "implausible table %d x %d x %d, max distance %g", lut->xres, lut->yres, lut->zres, (double)lut->max_dist);
  if (w < 1 || h < 1 || (long long)w * h > (1ll << 28)) return sf::fail(SF_ERR_INVALID_ARG, "image size %d x %d", w, h);
  if (lut->xres > w || lut->yres > h) return sf::fail(SF_ERR_INVALID_ARG, "the table (%d x %d) is finer than the image (%d x %d)", lut->xres, lut->yres, w, h);
  k.w = w; k.h = h; k.xr = lut->xres; k.yr = lut->yres; k.zr = lut->zres;
  k.xbin = (float)(w / lut->xres);
  k.ybin = (float)(h / lut->yres);
  k.zbin = (float)lut->zres / lut->max_dist;
  k.bitshift = bitshift ? 1 : 0;
  return SF_OK;
}

std::string join(const std::string& root, const std::string& name) {
  if (root.empty() || (!name.empty() && name[0] == '/')) return name;
  return root + "/" + name;
}

int read_depth_png(const std::string& path, uint32_t& w, uint32_t& h, std::vector<uint16_t>& px) {
  int ch = 0, bits = 0;
  void* data = nullptr;
  const int rc = sf_png_read(path.c_str(), &w, &h, &ch, &bits, &data);
  if (rc != SF_OK) return rc;
  if (ch != 1 || bits != 16) {
    sf_free(data);
    return sf::fail(SF_ERR_FORMAT, "%s: %d channel(s) of %d bits, a depth image is 16-bit grey", path.c_str(), ch, bits);
  }
  px.assign((const uint16_t*)data, (const uint16_t*)data + (size_t)w * h);
  sf_free(data);
  return SF_OK;
}

// 4 x 4 inverse in double by Gauss-Jordan with partial pivoting; false when singular
bool invert4(const double a[16], double out[16]) {
  double m[4][8];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) { m[r][c] = a[4 * r + c]; m[r][4 + c] = r == c ? 1.0 : 0.0; }
  for (int c = 0; c < 4; c++) {
    int p = c;
    for (int r = c + 1; r < 4; r++)
      if (std::fabs(m[r][c]) > std::fabs(m[p][c])) p = r;
    if (!(std::fabs(m[p][c]) > 1e-300)) return false;
    if (p != c)
      for (int k = 0; k < 8; k++) std::swap(m[p][k], m[c][k]);
    const double s = 1.0 / m[c][c];
    for (int k = 0; k < 8; k++) m[c][k] *= s;
    for (int r = 0; r < 4; r++) {
      if (r == c) continue;
      const double f = m[r][c];
      if (f != 0.0)
        for (int k = 0; k < 8; k++) m[r][k] -= f * m[c][k];
    }
  }
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) out[4 * r + c] = m[r][4 + c];
  return true;
}

}  // namespace

// ---- the table file ----------------------------------------------------------------------------------------------------------------------
// Grid3D::WriteFile, grid3d.h:464-494: int xres, yres, zres; float maxDist; the floats
SF_API int sf_lut_save(const char* path, const sf_lut* t) {
  if (!path || !t || !t->data) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (t->xres <= 0 || t->yres <= 0 || t->zres <= 0 || (int64_t)t->xres * t->yres * t->zres > (1ll << 28))
    return sf::fail(SF_ERR_INVALID_ARG, "implausible table %d x %d x %d", t->xres, t->yres, t->zres);
  std::ofstream f(path, std::ios::binary);
  if (!f) return sf::fail(SF_ERR_IO, "Could not open file %s for writing!", path);
  const int32_t res[3] = {t->xres, t->yres, t->zres};
  f.write((const char*)res, 12);
  f.write((const char*)&t->max_dist, 4);
  f.write((const char*)t->data, (std::streamsize)((size_t)t->xres * t->yres * t->zres * 4));
  f.close();
  if (!f) return sf::fail(SF_ERR_IO, "Unable to write grid values to file %s", path);
  return SF_OK;
}

// ---- the estimator -----------------------------------------------------------------------------------------------------------------------
SF_API int sf_lut_estimator_max_batch(void) { return LUT_MAX_BATCH; }

SF_API void sf_lut_estimator_destroy(sf_lut_estimator* e) {
  if (!e) return;
  if (e->device >= 0) lut_dev_destroy(e);
  delete e;
}

SF_API int sf_lut_estimator_create(int width, int height, float fx, float fy, float mx, float my, int n_slices, float max_depth, int bitshift, int device,
                                   sf_lut_estimator** out) {
  if (!out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *out = nullptr;
  if (width < 2 * (LUT_STRIPE + 1) || height < 2 || (width & 1) || (height & 1) || (long long)width * height > (1ll << 28))
    return sf::fail(SF_ERR_INVALID_ARG, "image size %d x %d: both even, the width at least %d", width, height, 2 * (LUT_STRIPE + 1));
  if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(mx) || !std::isfinite(my) || fx == 0.0f || fy == 0.0f)
    return sf::fail(SF_ERR_INVALID_ARG, "invalid depth intrinsics");
  if (n_slices < 1 || !(max_depth > 0.0f) || !std::isfinite(max_depth) || !std::isfinite((float)n_slices / max_depth))
    return sf::fail(SF_ERR_INVALID_ARG, "n_slices %d, max_depth %g", n_slices, (double)max_depth);
  if (device < -1) return sf::fail(SF_ERR_INVALID_ARG, "device %d", device);
  if (n_slices > LUT_MAX_SLICES)   // the same bound on the host path: both paths serve the same tables
    return sf::fail(SF_ERR_PARAM, "n_slices %d: a lane's sums do not fit the LDS (limit %d)", n_slices, LUT_MAX_SLICES);
  sf_lut_estimator* e = new sf_lut_estimator();
  e->g = LutGeom{width, height, width / 2, height / 2, n_slices, fx, fy, mx, my, (float)n_slices / max_depth, bitshift ? 1 : 0};
  e->max_depth = max_depth;
  e->device = device;
  if (device >= 0) {
    const int rc = lut_dev_create(e);
    if (rc != SF_OK) { sf_lut_estimator_destroy(e); return rc; }
  } else {
    const size_t cells = (size_t)e->g.xres * e->g.yres * n_slices;
    e->acc.assign(cells, 0.0f);
    e->div.assign(cells, 0.0f);
  }
  *out = e;
  return SF_OK;
}

static int estimator_add(sf_lut_estimator* e, int n, const void* const* images, const float* plane_poses, bool host_pixels, float* kernel_us) {
  if (!e || !images || !plane_poses) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (n < 1) return sf::fail(SF_ERR_INVALID_ARG, "%d images", n);
  for (int k = 0; k < n; k++) {
    if (!images[k]) return sf::fail(SF_ERR_INVALID_ARG, "image %d is NULL", k);
    if (!host_pixels && ((uintptr_t)images[k] & 3)) return sf::fail(SF_ERR_INVALID_ARG, "device image %d is not 4-byte aligned", k);
    if (!finite16(plane_poses + 16 * (size_t)k)) return sf::fail(SF_ERR_INVALID_ARG, "plane pose %d is not finite", k);
  }
  if (kernel_us) *kernel_us = 0.0f;
  std::vector<LutImage> tab((size_t)std::min(n, LUT_MAX_BATCH));
  for (int b = 0; b < n; b += LUT_MAX_BATCH) {
    const int m = std::min(LUT_MAX_BATCH, n - b);
    for (int k = 0; k < m; k++) {
      tab[k] = plane_of(plane_poses + 16 * (size_t)(b + k), (const uint16_t*)images[b + k]);
      e->images++;
      e->used += (uint64_t)tab[k].used;
    }
    if (e->device < 0) {
      const double t0 = now_s();
      host_add(e, m, tab.data());
      if (kernel_us) *kernel_us += (float)((now_s() - t0) * 1e6);
    } else {
      float us = 0.0f;
      const int rc = lut_dev_add(e, m, tab.data(), host_pixels, kernel_us ? &us : nullptr);
      if (rc != SF_OK) return rc;
      if (kernel_us) *kernel_us += us;
    }
  }
  return SF_OK;
}

SF_API int sf_lut_estimator_add(sf_lut_estimator* e, int n, const uint16_t* const* images, const float* plane_poses) {
  return estimator_add(e, n, (const void* const*)images, plane_poses, true, nullptr);
}

SF_API int sf_lut_estimator_add_device(sf_lut_estimator* e, int n, const void* const* d_images, const float* plane_poses, float* kernel_us) {
  if (e && e->device < 0) return sf::fail(SF_ERR_INVALID_ARG, "the host path takes host images (sf_lut_estimator_add)");
  return estimator_add(e, n, d_images, plane_poses, false, kernel_us);
}

SF_API int sf_lut_estimator_sums(sf_lut_estimator* e, float* acc, float* div, uint64_t* images, uint64_t* used) {
  if (!e || !acc || !div) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (images) *images = e->images;
  if (used) *used = e->used;
  if (e->device >= 0) return lut_dev_sums(e, acc, div);
  std::memcpy(acc, e->acc.data(), e->acc.size() * 4);
  std::memcpy(div, e->div.data(), e->div.size() * 4);
  return SF_OK;
}

SF_API int sf_lut_estimator_finish(sf_lut_estimator* e, sf_lut* out) {
  if (!e || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const LutGeom& g = e->g;
  const size_t cells = (size_t)g.xres * g.yres * g.ns;
  float* data = (float*)std::malloc(cells * 4);
  if (!data) return sf::fail(SF_ERR_IO, "out of memory");
  if (e->device >= 0) {
    const int rc = lut_dev_finish(e, data);
    if (rc != SF_OK) { std::free(data); return rc; }
  } else {
    for (size_t row = 0; row < cells; row += (size_t)g.xres)
      for (int x = 0; x < g.xres; x++) data[row + x] = lut_finish_cell(e->acc.data(), e->div.data(), g.xres, row, x);
  }
  out->xres = g.xres; out->yres = g.yres; out->zres = g.ns;
  out->max_dist = e->max_depth;
  out->data = data;
  return SF_OK;
}

// ---- apply -------------------------------------------------------------------------------------------------------------------------------
SF_API int sf_lut_apply(const sf_lut* lut, int n, const uint16_t* const* in, uint16_t* const* out, int width, int height, int bitshift, int device) {
  LutApplyK k;
  const int rc = make_apply(lut, width, height, bitshift, k);
  if (rc != SF_OK) return rc;
  if (n < 1 || !in || !out) return sf::fail(SF_ERR_INVALID_ARG, "no images");
  for (int j = 0; j < n; j++)
    if (!in[j] || !out[j]) return sf::fail(SF_ERR_INVALID_ARG, "image %d is NULL", j);
  if (device >= 0) {
    for (int b = 0; b < n; b += LUT_MAX_BATCH) {
      const int rcd = lut_dev_apply(device, k, lut->data, std::min(LUT_MAX_BATCH, n - b), (const void* const*)(in + b), (void* const*)(out + b), true, nullptr);
      if (rcd != SF_OK) return rcd;
    }
    return SF_OK;
  }
  if (device != -1) return sf::fail(SF_ERR_INVALID_ARG, "device %d", device);
  const long long work = (long long)n * width * height;
  parallel_for(n * height, work < (1 << 18) ? 1 : sf::usable_cpus(), [&](int r) {
    const int img = r / height, j = r % height;
    const uint16_t* src = in[img] + (size_t)j * width;
    uint16_t* dst = out[img] + (size_t)j * width;
    for (int i = 0; i < width; i++) dst[i] = lut_apply_pixel(k, lut->data, i, j, src[i]);
  });
  return SF_OK;
}

SF_API int sf_lut_apply_device(const sf_lut* lut, int n, const void* const* d_in, void* const* d_out, int width, int height, int bitshift, int device,
                               float* kernel_us) {
  LutApplyK k;
  const int rc = make_apply(lut, width, height, bitshift, k);
  if (rc != SF_OK) return rc;
  if (n < 1 || !d_in || !d_out) return sf::fail(SF_ERR_INVALID_ARG, "no images");
  for (int j = 0; j < n; j++)
    if (!d_in[j] || !d_out[j]) return sf::fail(SF_ERR_INVALID_ARG, "image %d is NULL", j);
  if (device < 0) return sf::fail(SF_ERR_INVALID_ARG, "the host path takes host images (sf_lut_apply)");
  return lut_dev_apply(device, k, lut->data, n, d_in, d_out, false, kernel_us);
}

// ---- files (:112-362) --------------------------------------------------------------------------------------------------------------------
SF_API void sf_depth_calib_free(sf_depth_calib* c) {
  if (!c) return;
  std::free(c->plane_poses);
  if (c->image_names) {
    for (int i = 0; i < c->n_scans; i++) std::free(c->image_names[i]);
    std::free(c->image_names);
  }
  c->plane_poses = nullptr;
  c->image_names = nullptr;
  c->n_scans = 0;
}

// ReadPlanePoses, :184-223: N row-major matrices; each becomes inverse(F * D2C * F) * pose, F = diag(1, -1, -1, 1)
static int read_plane_poses(const std::string& path, const float d2c[16], int n, float* out) {
  double m[16], inv[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) m[4 * r + c] = (double)d2c[4 * r + c] * ((r == 1 || r == 2) ? -1.0 : 1.0) * ((c == 1 || c == 2) ? -1.0 : 1.0);
  if (!invert4(m, inv)) return sf::fail(SF_ERR_FORMAT, "depthToColorExtrinsics is singular");
  std::ifstream f(path);
  if (!f) return sf::fail(SF_ERR_IO, "Unable to read plane_poses file %s", path.c_str());
  for (int i = 0; i < n; i++) {
    float p[16];
    for (int k = 0; k < 16; k++)
      if (!(f >> p[k]) || !std::isfinite(p[k])) return sf::fail(SF_ERR_FORMAT, "%s: pose %d of %d is missing, truncated or not finite", path.c_str(), i, n);
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) {
        double s = 0.0;
        for (int k = 0; k < 4; k++) s += inv[4 * r + k] * (double)p[4 * k + c];
        out[16 * (size_t)i + 4 * r + c] = (float)s;
      }
  }
  return SF_OK;
}

SF_API int sf_depth_calib_load(const char* config_path, const char* root, sf_depth_calib* out) {
  if (!config_path || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  std::memset(out, 0, sizeof(*out));
  const std::string rootdir = root ? root : "";
  std::ifstream f(config_path);
  if (!f) return sf::fail(SF_ERR_IO, "Unable to open configuration file %s", config_path);
  bool have_params = false, have_n = false, have_poses = false;
  std::vector<std::string> names;
  std::string line;
  int line_no = 0;
  auto bad = [&](int code, const std::string& what) {
    sf_depth_calib_free(out);
    return sf::fail(code, "%s:%d: %s", config_path, line_no, what.c_str());
  };
  while (std::getline(f, line)) {
    line_no++;
    std::istringstream is(line);
    std::string cmd;
    if (!(is >> cmd) || cmd[0] == '#') continue;
    if (cmd == "parameters") {
      std::string name;
      if (!(is >> name)) return bad(SF_ERR_FORMAT, "parameters: no file name");
      sf_calib_params p;
      const int rc = sf_calib_params_load(join(rootdir, name).c_str(), &p);
      if (rc != SF_OK) { sf_depth_calib_free(out); return rc; }
      out->fx = p.depth_intrinsic[0]; out->fy = p.depth_intrinsic[5]; out->mx = p.depth_intrinsic[2]; out->my = p.depth_intrinsic[6];
      std::memcpy(out->depth_to_color, p.depth_extrinsic, 64);
      have_params = true;
    } else if (cmd == "n_images") {
      long long n = 0;
      if (!(is >> n) || n < 1 || n > (1 << 24)) return bad(SF_ERR_FORMAT, "n_images: a count of 1 or more is expected");
      if (have_poses) return bad(SF_ERR_FORMAT, "n_images after plane_poses");
      out->n_images = (int32_t)n;
      have_n = true;
    } else if (cmd == "plane_poses") {
      std::string name;
      if (!(is >> name)) return bad(SF_ERR_FORMAT, "plane_poses: no file name");
      if (!have_params || !have_n) return bad(SF_ERR_FORMAT, "plane_poses before parameters and n_images (the reference would silently use defaults)");
      if (have_poses) return bad(SF_ERR_FORMAT, "plane_poses given twice");
      out->plane_poses = (float*)std::malloc((size_t)out->n_images * 64);
      if (!out->plane_poses) return bad(SF_ERR_IO, "out of memory");
      const int rc = read_plane_poses(join(rootdir, name), out->depth_to_color, out->n_images, out->plane_poses);
      if (rc != SF_OK) { sf_depth_calib_free(out); return rc; }
      have_poses = true;
    } else if (cmd == "scan") {
      std::string depth_name, colour_name;
      if (!(is >> depth_name >> colour_name)) return bad(SF_ERR_FORMAT, "scan: two image names and 16 numbers are expected");
      for (int k = 0; k < 16; k++) {
        float v;
        if (!(is >> v)) return bad(SF_ERR_FORMAT, "scan: two image names and 16 numbers are expected");
      }
      names.push_back(depth_name);
    }
  }
  line_no = 0;
  if (!have_poses) return bad(SF_ERR_FORMAT, "no plane_poses line");
  if ((size_t)out->n_images > names.size()) return bad(SF_ERR_FORMAT, "n_images is larger than the number of scan lines");
  out->image_names = (char**)std::calloc(names.size(), sizeof(char*));
  if (!out->image_names) return bad(SF_ERR_IO, "out of memory");
  out->n_scans = (int32_t)names.size();
  for (size_t i = 0; i < names.size(); i++) {
    out->image_names[i] = (char*)std::malloc(names[i].size() + 1);
    if (!out->image_names[i]) return bad(SF_ERR_IO, "out of memory");
    std::memcpy(out->image_names[i], names[i].c_str(), names[i].size() + 1);
  }
  return SF_OK;
}

// ---- the tool's body -----------------------------------------------------------------------------------------------------------------------
SF_API void sf_calibrate_depth_options_default(sf_calibrate_depth_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_depth = 5.0f;   // :1153-1154
  o->n_slices = 15;
  o->bitshift = 1;
}

namespace {

// ReportBinCounts, :516-563
void report_bins(const sf_depth_calib& c, const sf_calibrate_depth_options& o) {
  const int z_bin = (int)((float)o.n_slices / o.max_depth);
  int counts[128] = {0};
  int total = 0;
  for (int i = 0; i < c.n_images; i++) {
    const float* T = c.plane_poses + 16 * (size_t)i;
    const float n[3] = {T[2], T[6], T[10]};
    if (plane_angle(n) < 25.0f) {
      const float distance = -T[11];
      const float fi = distance * (float)z_bin;
      if (fi > -1.0f && fi < 128.0f) counts[(int)fi] += 1;   // a bin outside the table is dropped, not written
      total++;
    }
  }
  std::printf("Depth Bins: \n");
  for (int i = 0; i < o.n_slices && i < 128; i++) {
    const float lo = (float)i * (1.0f / (float)z_bin), hi = (float)(i + 1) * (1.0f / (float)z_bin);
    std::printf("\tBin %3d (%5.3f - %5.3f) : %3d\n", i, (double)lo, (double)hi, counts[i]);
  }
  std::printf("Will use %d/%d images for calibration\n", total, c.n_images);
}

// :845-891
int write_slices(const sf_lut& t, const std::string& root, bool verbose) {
  const size_t per = (size_t)t.xres * t.yres, cells = per * t.zres;
  float mn = 1e9f, mx = -1e9f;   // Grid3D::Min / Max
  for (size_t i = 0; i < cells; i++) {
    if (t.data[i] == LUT_UNKNOWN) continue;
    if (t.data[i] < mn) mn = t.data[i];
    if (t.data[i] > mx) mx = t.data[i];
  }
  std::vector<uint8_t> img(per * 3);
  for (int z = 0; z < t.zres; z++) {
    float smin = INFINITY, smax = -INFINITY;
    for (size_t j = 0; j < per; j++) {
      float val = t.data[z * per + j];
      smin = std::min(smin, val); smax = std::max(smax, val);
      float col[3] = {1.0f, 0.5f, 0.0f};
      if (val != LUT_UNKNOWN) {
        val = (val - mn) / (mx - mn);
        col[0] = col[1] = col[2] = 0.0f;
        if (val < 0.5f) {
          col[0] = (float)(1.0 - 2.0 * val);
          col[1] = (float)(2.0 * val);
        } else {
          col[1] = (float)(1 - 2 * (val - 0.5));
          col[2] = (float)(2 * (val - 0.5));
        }
      }
      for (int k = 0; k < 3; k++) {
        const float v = col[k] * 255.0f;
        img[3 * j + k] = !(v >= 0.0f) ? (uint8_t)0 : (v >= 255.0f ? (uint8_t)255 : (uint8_t)v);   // a flat table divides 0 by 0: black
      }
    }
    if (verbose) std::printf("\tSlice %3d -> Min: %5.4f Max %5.4f\n", z, (double)smin, (double)smax);
    char name[64];
    std::snprintf(name, sizeof(name), "slice_%03d.png", z);
    const int rc = sf_png_write(join(root, name).c_str(), img.data(), (uint32_t)t.xres, (uint32_t)t.yres, 3, 8);
    if (rc != SF_OK) return rc;
  }
  return SF_OK;
}

// reads images [b, b + m) on the pool; all must be w x h (set from the first image ever read when w == 0)
int read_batch(const std::vector<std::string>& paths, int b, int m, int threads, uint32_t& w, uint32_t& h, std::vector<std::vector<uint16_t>>& px) {
  px.resize((size_t)m);
  std::vector<int> rcs((size_t)m, SF_OK);
  std::vector<std::string> errs((size_t)m);
  std::vector<uint32_t> ws((size_t)m), hs((size_t)m);
  parallel_for(m, threads, [&](int k) {
    rcs[k] = read_depth_png(paths[(size_t)(b + k)], ws[k], hs[k], px[k]);
    if (rcs[k] != SF_OK) errs[k] = sf_last_error();   // the message is per thread
  });
  for (int k = 0; k < m; k++) {
    if (rcs[k] != SF_OK) return sf::fail(rcs[k], "%s", errs[k].c_str());
    if (w == 0) { w = ws[k]; h = hs[k]; }
    if (ws[k] != w || hs[k] != h)
      return sf::fail(SF_ERR_FORMAT, "%s is %u x %u, the sequence is %u x %u: all images must be alike", paths[(size_t)(b + k)].c_str(), ws[k], hs[k], w, h);
  }
  return SF_OK;
}

}  // namespace

SF_API int sf_calibrate_depth(const char* config, const char* estimate_path, const char* apply_path, const sf_calibrate_depth_options* options, int device,
                              int threads, sf_calibrate_depth_stats* stats) {
  if (!config) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (!estimate_path && !apply_path) return sf::fail(SF_ERR_INVALID_ARG, "neither a table to estimate nor one to apply: the viewer is not provided");
  sf_calibrate_depth_options o;
  if (options) o = *options; else sf_calibrate_depth_options_default(&o);
  if (o.n_slices < 1 || !(o.max_depth > 0.0f) || !std::isfinite(o.max_depth)) return sf::fail(SF_ERR_INVALID_ARG, "n_slices %d, max_depth %g", o.n_slices, (double)o.max_depth);
  if (threads <= 0) threads = sf::usable_cpus();
  const std::string root = o.root ? o.root : "";
  const double t_start = now_s();
  sf_calibrate_depth_stats st;
  std::memset(&st, 0, sizeof(st));
  st.threads = (uint32_t)threads;
  sf_depth_calib c;
  int rc = sf_depth_calib_load(config, o.root, &c);
  if (rc != SF_OK) return rc;
  st.images = (uint64_t)c.n_images;
  const int chunk = LUT_MAX_BATCH;
  std::vector<std::vector<uint16_t>> px;

  if (estimate_path) {   // EstimateDistortion, :647-894
    if (o.verbose) report_bins(c, o);
    std::vector<std::string> paths;
    for (int i = 0; i < c.n_images; i++) paths.push_back(join(root, std::string("depth_raw/") + c.image_names[i]));
    sf_lut_estimator* e = nullptr;
    uint32_t w = 0, h = 0;
    for (int b = 0; b < c.n_images && rc == SF_OK; b += chunk) {
      const int m = std::min(chunk, c.n_images - b);
      double t0 = now_s();
      rc = read_batch(paths, b, m, threads, w, h, px);
      st.seconds_read += now_s() - t0;
      if (rc != SF_OK) break;
      if (!e) {
        rc = sf_lut_estimator_create((int)w, (int)h, c.fx, c.fy, c.mx, c.my, o.n_slices, o.max_depth, o.bitshift, device, &e);
        if (rc != SF_OK) break;
      }
      std::vector<const uint16_t*> ptr((size_t)m);
      for (int k = 0; k < m; k++) ptr[k] = px[k].data();
      t0 = now_s();
      rc = sf_lut_estimator_add(e, m, ptr.data(), c.plane_poses + 16 * (size_t)b);
      st.seconds_estimate += now_s() - t0;
    }
    sf_lut t = {0, 0, 0, 0.0f, nullptr};
    if (rc == SF_OK) {
      const double t0 = now_s();
      rc = sf_lut_estimator_finish(e, &t);
      st.seconds_estimate += now_s() - t0;
    }
    if (rc == SF_OK) {
      st.images_used = e->used;
      st.images_skipped = e->images - e->used;
      if (o.verbose && st.images_skipped) {
        std::printf("Skipped images: \n");
        for (int i = 0; i < c.n_images; i++) {
          const float* T = c.plane_poses + 16 * (size_t)i;
          const float n[3] = {T[2], T[6], T[10]};
          if (plane_angle(n) > 25.0f) std::printf("\t %s\n", c.image_names[i]);
        }
      }
      rc = sf_lut_save(estimate_path, &t);
    }
    if (rc == SF_OK && o.save_slices) rc = write_slices(t, root, o.verbose != 0);
    sf_lut_free(&t);
    sf_lut_estimator_destroy(e);
  }

  if (rc == SF_OK && apply_path) {   // ApplyUndistortion, :565-644
    sf_lut t = {0, 0, 0, 0.0f, nullptr};
    rc = sf_lut_load(apply_path, &t);
    if (rc == SF_OK) {
      std::vector<std::string> in_paths, out_paths;
      for (int i = 0; i < c.n_images; i++) {
        std::string name = c.image_names[i];
        name = name.size() > 4 ? name.substr(0, name.size() - 4) : std::string();
        in_paths.push_back(join(root, "depth_raw/" + name + ".png"));
        out_paths.push_back(join(root, "depth/" + name + ".png"));
      }
      ::mkdir(join(root, "depth").c_str(), 0775);
      uint32_t w = 0, h = 0;
      for (int b = 0; b < c.n_images && rc == SF_OK; b += chunk) {
        const int m = std::min(chunk, c.n_images - b);
        double t0 = now_s();
        rc = read_batch(in_paths, b, m, threads, w, h, px);
        st.seconds_read += now_s() - t0;
        if (rc != SF_OK) break;
        std::vector<std::vector<uint16_t>> res((size_t)m, std::vector<uint16_t>((size_t)w * h));
        std::vector<const uint16_t*> ip((size_t)m);
        std::vector<uint16_t*> op((size_t)m);
        for (int k = 0; k < m; k++) { ip[k] = px[k].data(); op[k] = res[k].data(); }
        t0 = now_s();
        rc = sf_lut_apply(&t, m, ip.data(), op.data(), (int)w, (int)h, o.bitshift, device);
        st.seconds_apply += now_s() - t0;
        if (rc != SF_OK) break;
        std::vector<int> rcs((size_t)m, SF_OK);
        std::vector<std::string> errs((size_t)m);
        t0 = now_s();
        parallel_for(m, threads, [&](int k) {
          rcs[k] = sf_png_write_gray(out_paths[(size_t)(b + k)].c_str(), res[k].data(), w, h, 16);
          if (rcs[k] != SF_OK) errs[k] = sf_last_error();
        });
        st.seconds_write += now_s() - t0;
        for (int k = 0; k < m && rc == SF_OK; k++)
          if (rcs[k] != SF_OK) rc = sf::fail(rcs[k], "%s", errs[k].c_str());
        st.images_applied += (uint64_t)m;
      }
    }
    sf_lut_free(&t);
  }
  sf_depth_calib_free(&c);
  st.seconds_total = now_s() - t_start;
  if (stats) *stats = st;
  return rc;
}
