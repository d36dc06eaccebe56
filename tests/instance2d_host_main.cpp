// instance2d_host_main.cpp -- the host path of the 2-D instance task (scannet_amd/csrc/instance2d.cpp, the AP accumulator of evaluation.cpp and the
// file mode of instance2d_files.cpp with png.cpp and zlib_codec.cpp) as a program of its own, for
// tests/test_instance2d.py::test_host_code_under_sanitizers: built with -fsanitize=address,undefined and run; nothing is preloaded.  The few things
// those files take from the rest of the library are defined here: the error string, the CPU count and the device paths (which this program never
// reaches).  Every array is allocated at its exact size, so a read or write past an end is caught.  With a directory as its argument it runs the file
// mode there on whole inputs, and on a prediction list and on PNG files cut at every length.
#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "scanfuse.h"
#include "scanfuse_internal.h"
#include "../scannet_amd/csrc/evaluation_internal.h"

namespace sf {
std::string& last_error_ref() {
  static std::string s;
  return s;
}
int usable_cpus() { return 4; }
namespace ev {
int confusion_on_device(const void*, const void*, int, uint64_t, uint64_t, uint32_t, int, int, uint64_t*, uint64_t*) { return SF_ERR_DEVICE; }
int confusion_images_on_device(const void*, const void*, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, int, uint64_t*,
                               uint64_t*) {
  return SF_ERR_DEVICE;
}
int overlaps_on_device(const uint32_t*, uint64_t, uint32_t, const uint8_t*, uint32_t, uint64_t, int, uint32_t*) { return SF_ERR_DEVICE; }
int image_plan_on_device(const void*, int, uint32_t, uint32_t, const ValidSet&, uint32_t, int, uint32_t*, int32_t*, uint32_t*) { return SF_ERR_DEVICE; }
int overlaps_images_on_device(const void*, int, uint32_t, uint32_t, const ValidSet&, uint32_t, const uint32_t*, const int32_t*, const uint8_t*, uint32_t, uint64_t,
                              const uint32_t*, int, uint32_t*) {
  return SF_ERR_DEVICE;
}
}  // namespace ev
}  // namespace sf

extern "C" const char* sf_last_error(void) { return sf::last_error_ref().c_str(); }

#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, sf_last_error()); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static const int32_t CLASSES[18] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};

// a batch of images of runs of ids, planned, overlapped and scored; the counts are checked against sums that need no second implementation
template <typename T>
static int arrays_of_width(uint32_t seed, uint32_t batch, uint32_t w, uint32_t h) {
  const size_t n = (size_t)w * h;
  std::vector<T> gt(batch * n);
  const uint32_t values[8] = {0, 5, 39, 1, 5001, 5002, 39001, 7003};
  for (size_t i = 0; i < gt.size();) {
    const T v = (T)values[rnd(seed) % 8];
    for (uint32_t run = 1 + rnd(seed) % 40; run && i < gt.size(); run--) gt[i++] = v;
  }
  std::vector<uint32_t> count(batch);
  CHECK(sf_eval_image_plan(gt.data(), (int)sizeof(T), batch, w, h, CLASSES, 18, 0, -1, count.data(), nullptr, nullptr) == SF_OK);
  uint32_t capacity = 0;
  for (uint32_t c : count) capacity = c > capacity ? c : capacity;
  std::vector<int32_t> ids((size_t)batch * capacity);
  std::vector<uint32_t> pixels((size_t)batch * capacity);
  CHECK(sf_eval_image_plan(gt.data(), (int)sizeof(T), batch, w, h, CLASSES, 18, capacity, -1, count.data(), ids.data(), pixels.data()) == SF_OK);
  if (capacity > 1) {   // one entry too few: refused, and nothing is written (with arrays of no entry the call would only count)
    std::vector<int32_t> few((size_t)batch * (capacity - 1), -7);
    std::vector<uint32_t> fewp((size_t)batch * (capacity - 1), 7u), fewc(batch, 77u);
    const int few_rc = sf_eval_image_plan(gt.data(), (int)sizeof(T), batch, w, h, CLASSES, 18, capacity - 1, -1, fewc.data(), few.data(), fewp.data());
    CHECK(few_rc == SF_ERR_BOUNDS);
    for (int32_t v : few) CHECK(v == -7);
    for (uint32_t v : fewc) CHECK(v == 77u);
  }
  const uint32_t P = 2 * batch + 1;
  const uint64_t stride = n + 3;   // rows further apart than an image
  std::vector<uint8_t> masks((size_t)(P - 1) * stride + n);
  std::vector<uint32_t> mask_image(P);
  for (uint32_t p = 0; p < P; p++) {
    mask_image[p] = p % batch;
    for (size_t i = 0; i < n; i++) masks[p * stride + i] = (rnd(seed) % 3) ? 0 : (uint8_t)(1 + rnd(seed) % 255);
  }
  std::vector<uint32_t> table((size_t)P * (capacity + 2));
  CHECK(sf_eval_overlaps_images(gt.data(), (int)sizeof(T), batch, w, h, CLASSES, 18, capacity, count.data(), ids.data(), masks.data(), P, stride, mask_image.data(), -1,
                                table.data()) == SF_OK);
  for (uint32_t p = 0; p < P; p++) {
    const uint32_t* row = table.data() + (size_t)p * (capacity + 2);
    uint64_t covered = 0, inside = row[capacity];
    for (size_t i = 0; i < n; i++) covered += masks[p * stride + i] != 0;
    for (uint32_t g = 0; g < count[mask_image[p]]; g++) inside += row[g];
    CHECK(covered == row[capacity + 1] && inside <= covered);
  }
  sf_eval_ap2d* acc = nullptr;
  CHECK(sf_eval_ap2d_create(CLASSES, 18, 100, &acc) == SF_OK);
  for (uint32_t b = 0; b < batch; b++) {
    std::vector<int32_t> label;
    std::vector<double> conf;
    std::vector<uint32_t> rows;
    for (uint32_t p = 0; p < P; p++)
      if (mask_image[p] == b) {
        label.push_back(p % 4 == 3 ? 13 : (p % 2 ? 5 : 39));
        conf.push_back((double)(rnd(seed) % 5) / 4.0);
        rows.insert(rows.end(), table.begin() + (size_t)p * (capacity + 2), table.begin() + (size_t)(p + 1) * (capacity + 2));
      }
    CHECK(sf_eval_ap2d_add_image(acc, count[b], ids.data() + (size_t)b * capacity, pixels.data() + (size_t)b * capacity, (uint32_t)label.size(), label.data(),
                                 conf.data(), rows.data(), capacity) == SF_OK);
  }
  std::vector<double> ap(18 * SF_EVAL_AP2D_OVERLAPS), cls(18 * 2);
  double avg[2];
  CHECK(sf_eval_ap2d_finish(acc, ap.data(), cls.data(), avg) == SF_OK);
  sf_eval_ap2d_destroy(acc);
  for (double v : ap) CHECK(std::isnan(v) || (v >= 0.0 && v <= 1.0));
  return 0;
}

static int write_file(const std::string& path, const std::string& bytes) {
  std::ofstream f(path, std::ios::binary);
  f << bytes;
  return f.good() ? 0 : 1;
}

static std::string read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// a directory of two images with their lists and masks; then the list and each kind of PNG cut at every length: every outcome but a crash is fine
static int files(const std::string& root) {
  const std::string pred = root + "/pred", gt = root + "/gt";
  mkdir(pred.c_str(), 0777);
  mkdir((pred + "/masks").c_str(), 0777);
  mkdir((pred + "/sub").c_str(), 0777);
  mkdir(gt.c_str(), 0777);
  const uint32_t w = 37, h = 23;
  std::vector<uint16_t> img((size_t)w * h, 0);
  for (uint32_t y = 2; y < 20; y++)
    for (uint32_t x = 3; x < 30; x++) img[(size_t)y * w + x] = 5001;
  for (uint32_t x = 0; x < w; x++) img[x] = 5;
  std::vector<uint8_t> img8((size_t)w * h, 39), mask((size_t)w * h, 0);
  for (uint32_t y = 2; y < 20; y++)
    for (uint32_t x = 3; x < 30; x++) mask[(size_t)y * w + x] = 255;
  CHECK(sf_png_write_gray((gt + "/a.png").c_str(), img.data(), w, h, 16) == SF_OK);
  CHECK(sf_png_write_gray((gt + "/b.png").c_str(), img8.data(), w, h, 8) == SF_OK);
  CHECK(sf_png_write_gray((pred + "/masks/m0.png").c_str(), mask.data(), w, h, 8) == SF_OK);
  const std::string list = "masks/m0.png 5 0.75\nmasks/m0.png 5 0.5\nmasks/none.png 13 1\n";
  CHECK(write_file(pred + "/a.txt", list) == 0);
  CHECK(write_file(pred + "/sub/b.txt", "../masks/m0.png 39 1e-3\n") == 0);
  char* report = nullptr;
  CHECK(sf_eval_instance2d_dir(pred.c_str(), gt.c_str(), nullptr, 100, -1, &report) == SF_OK);
  CHECK(report && std::strstr(report, "chair          :          1.000          1.000"));
  sf_free(report);
  CHECK(sf_eval_instance2d_dir(pred.c_str(), gt.c_str(), nullptr, 100, -1, &report) == SF_OK);   // the result file of the first run is left out
  sf_free(report);
  for (size_t cut = 0; cut < list.size(); cut++) {
    CHECK(write_file(pred + "/a.txt", list.substr(0, cut)) == 0);
    (void)sf_eval_instance2d_dir(pred.c_str(), gt.c_str(), nullptr, 100, -1, &report);
    sf_free(report);
  }
  CHECK(write_file(pred + "/a.txt", list) == 0);
  const char* cut_files[3] = {"/gt/a.png", "/gt/b.png", "/pred/masks/m0.png"};
  for (const char* rel : cut_files) {
    const std::string whole = read_file(root + rel);
    CHECK(whole.size() > 40);
    for (size_t cut = 0; cut < whole.size(); cut++) {
      CHECK(write_file(root + rel, whole.substr(0, cut)) == 0);
      const int rc = sf_eval_instance2d_dir(pred.c_str(), gt.c_str(), nullptr, 100, -1, &report);
      CHECK((rc == SF_OK) == (report != nullptr));
      if (cut < whole.size() / 2) CHECK(rc == SF_ERR_FORMAT || rc == SF_ERR_IO);   // half an image is none
      sf_free(report);
    }
    CHECK(write_file(root + rel, whole) == 0);
  }
  CHECK(sf_eval_instance2d_dir(pred.c_str(), gt.c_str(), nullptr, 100, -1, &report) == SF_OK);
  sf_free(report);
  return 0;
}

int main(int argc, char** argv) {
  if (arrays_of_width<uint8_t>(1, 3, 17, 3)) return 1;
  if (arrays_of_width<uint16_t>(2, 5, 67, 45)) return 1;
  if (arrays_of_width<uint32_t>(3, 1, 1, 1)) return 1;
  if (arrays_of_width<uint32_t>(4, 17, 15, 1)) return 1;
  if (arrays_of_width<uint16_t>(5, 2, 128, 96)) return 1;
  double th[SF_EVAL_AP2D_OVERLAPS];
  CHECK(sf_eval_ap2d_thresholds(th) == SF_OK && th[0] == 0.5 && th[9] > 0.95 && th[9] < 0.9500001);
  if (argc > 1 && files(argv[1])) return 1;
  std::printf("instance2d host: ok\n");
  return 0;
}
