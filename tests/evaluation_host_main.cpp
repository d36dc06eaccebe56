// evaluation_host_main.cpp -- the host path of the benchmark's scores (scannet_amd/csrc/evaluation.cpp) as a program of its own, for
// tests/test_evaluation.py::test_host_code_under_sanitizers: built with -fsanitize=address,undefined and run; nothing is preloaded.  It links
// evaluation.cpp alone, so the few things that file takes from the rest of the library are defined here: the error string, the CPU count and the
// device paths (which this program never reaches).  Every array is allocated at its exact size, so a read or write past an end is caught.  With a
// directory as its argument it also runs the file modes and the export (evaluation_files.cpp, with annotations.cpp, png.cpp and zlib_codec.cpp) on
// whole, truncated and malformed `.txt`, prediction-list, PNG, JSON and label-map inputs written there.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <sys/stat.h>

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

static const int32_t LABELS[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};

template <typename T>
static int confusion_of_width(uint32_t seed) {
  const uint64_t n = 200003;   // several jobs of the host path and a ragged last one
  std::vector<T> gt(n), pred(n);
  for (uint64_t i = 0; i < n; i++) {
    gt[i] = (T)(rnd(seed) % 45u);
    pred[i] = (rnd(seed) % 16u) ? gt[i] : (T)rnd(seed);   // any bit pattern of the type
  }
  std::vector<uint64_t> conf(41 * 41, 0);
  uint64_t oor = 0, sum = 0;
  CHECK(sf_eval_confusion(gt.data(), pred.data(), (int)sizeof(T), n, LABELS, 20, SF_EVAL_MODE_3D, -1, conf.data(), nullptr) == SF_OK);
  for (uint64_t v : conf) sum += v;
  CHECK(sum > n / 3 && sum < n);
  std::fill(conf.begin(), conf.end(), 0);
  CHECK(sf_eval_confusion(gt.data(), pred.data(), (int)sizeof(T), n, LABELS, 20, SF_EVAL_MODE_2D, -1, conf.data(), &oor) == SF_OK);
  sum = 0;
  for (uint64_t v : conf) sum += v;
  CHECK(sum + oor == n && oor > 0);
  CHECK(sf_eval_confusion(nullptr, nullptr, (int)sizeof(T), 0, LABELS, 20, SF_EVAL_MODE_3D, -1, conf.data(), nullptr) == SF_OK);
  return 0;
}

static void put(const std::string& path, const std::string& bytes) {
  std::ofstream f(path, std::ios::binary);
  f << bytes;
}

static std::string get(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// the file modes on inputs that are whole, cut short at every length, and wrong in each field
static int files(const std::string& root) {
  const std::string pred = root + "/pred", gt = root + "/gt", out = root + "/out.txt";
  mkdir(pred.c_str(), 0755);
  mkdir((pred + "/pred_mask").c_str(), 0755);
  mkdir(gt.c_str(), 0755);
  char* report = nullptr;
  std::string ids, labels, mask;
  for (int v = 0; v < 300; v++) {
    ids += std::to_string(v < 150 ? 3001 : (v < 250 ? 5002 : 0)) + "\n";
    labels += std::to_string(v < 150 ? 3 : (v < 250 ? 5 : 0)) + "\n";
    mask += v < 140 ? "1\n" : "0\n";
  }
  // label3d: the whole file, then cut at every length (a cut inside a number leaves a shorter number: fewer lines or another value, both handled)
  put(gt + "/a.txt", labels);
  put(pred + "/a.txt", labels);
  CHECK(sf_eval_label_dir(pred.c_str(), gt.c_str(), out.c_str(), -1, &report) == SF_OK && report && std::strstr(report, "cabinet       : 1.000"));
  sf_free(report);
  for (size_t cut = 0; cut < 40; cut++) {
    put(pred + "/a.txt", labels.substr(0, labels.size() - cut));
    const int rc = sf_eval_label_dir(pred.c_str(), gt.c_str(), out.c_str(), -1, &report);
    CHECK(rc == SF_OK || rc == SF_ERR_FORMAT);
    sf_free(report);
  }
  const char* broken[] = {"x\n", "1 2\n", "\n", "--1\n", "1.5\n", "99999999999999999999999\n", "\xff\xfe\n", "-\n", "+\n"};
  for (const char* b : broken) {
    put(pred + "/a.txt", std::string("3001\n") + b);
    CHECK(sf_eval_label_dir(pred.c_str(), gt.c_str(), out.c_str(), -1, &report) == SF_ERR_FORMAT && report == nullptr);
  }
  put(pred + "/a.txt", "");   // no line at all against 300
  CHECK(sf_eval_label_dir(pred.c_str(), gt.c_str(), out.c_str(), -1, nullptr) == SF_ERR_FORMAT);
  // instance3d: a good list, the list cut at every length, and lines wrong in each field
  put(gt + "/a.txt", ids);
  put(pred + "/pred_mask/m.txt", mask);
  const std::string list = "pred_mask/m.txt 3 0.9\npred_mask/m.txt 3 0.5\npred_mask/none.txt 1 0.5\n";
  put(pred + "/a.txt", list);
  CHECK(sf_eval_instance_dir(pred.c_str(), gt.c_str(), out.c_str(), 100, -1, &report) == SF_OK && std::strstr(report, "cabinet        :          1.000"));
  sf_free(report);
  for (size_t cut = 1; cut < list.size(); cut++) {
    put(pred + "/a.txt", list.substr(0, cut));
    const int rc = sf_eval_instance_dir(pred.c_str(), gt.c_str(), out.c_str(), 100, -1, &report);
    CHECK(rc == SF_OK || rc == SF_ERR_FORMAT || rc == SF_ERR_IO);
    sf_free(report);
  }
  const char* lines[] = {"/etc/passwd 3 0.5", "../gt/a.txt 3 0.5", "pred_mask/../../gt/a.txt 3 0.5", "pred_mask/m.txt 3", "pred_mask/m.txt 3 0.5 1", "pred_mask/m.txt  3 0.5",
                         "pred_mask/m.txt x 0.5", "pred_mask/m.txt 3 nan", "pred_mask/m.txt 1e300 0.5", " 3 0.5", "", "pred_mask 3 0.5"};
  for (const char* l : lines) {
    put(pred + "/a.txt", std::string(l) + "\n");
    const int rc = sf_eval_instance_dir(pred.c_str(), gt.c_str(), out.c_str(), 100, -1, &report);
    CHECK((rc == SF_ERR_FORMAT || rc == SF_ERR_IO) && report == nullptr);
  }
  put(pred + "/pred_mask/short.txt", mask.substr(0, 100));   // a mask of another length
  put(pred + "/a.txt", "pred_mask/short.txt 3 0.5\n");
  CHECK(sf_eval_instance_dir(pred.c_str(), gt.c_str(), out.c_str(), 100, -1, &report) == SF_ERR_FORMAT);
  // label2d: PNG pairs, then the prediction cut at every length and with each byte of its head changed
  const std::string pp = root + "/ppred", pg = root + "/pgt";
  mkdir(pp.c_str(), 0755);
  mkdir(pg.c_str(), 0755);
  std::vector<uint8_t> g8(64 * 48), p8(64 * 48);
  std::vector<uint16_t> g16(64 * 48);
  for (size_t i = 0; i < g8.size(); i++) { g8[i] = (uint8_t)((i / 7) % 41); p8[i] = (uint8_t)((i / 5) % 41); g16[i] = g8[i]; }
  CHECK(sf_png_write_gray((pg + "/0.png").c_str(), g16.data(), 64, 48, 16) == SF_OK && sf_png_write_gray((pp + "/0.png").c_str(), p8.data(), 64, 48, 8) == SF_OK);
  CHECK(sf_eval_pixel_dir(pp.c_str(), pg.c_str(), out.c_str(), -1, &report) == SF_OK && std::strstr(report, "Score Average"));
  sf_free(report);
  const std::string whole = get(pp + "/0.png");
  for (size_t cut = 0; cut < whole.size(); cut += (cut < 64 ? 1 : 7)) {
    put(pp + "/0.png", whole.substr(0, cut));
    const int rc = sf_eval_pixel_dir(pp.c_str(), pg.c_str(), out.c_str(), -1, &report);   // the reader accepts a file that lacks only its IEND chunk
    CHECK((rc != SF_OK && report == nullptr) || (rc == SF_OK && cut + 12 >= whole.size()));
    sf_free(report);
  }
  for (size_t at = 0; at < 64 && at < whole.size(); at++) {
    std::string bad = whole;
    bad[at] = (char)(bad[at] ^ 0x55);
    put(pp + "/0.png", bad);
    const int rc = sf_eval_pixel_dir(pp.c_str(), pg.c_str(), out.c_str(), -1, &report);
    CHECK(rc == SF_OK || report == nullptr);
    sf_free(report);
  }
  p8[5] = 41;   // an id the matrix has no row for
  CHECK(sf_png_write_gray((pp + "/0.png").c_str(), p8.data(), 64, 48, 8) == SF_OK);
  CHECK(sf_eval_pixel_dir(pp.c_str(), pg.c_str(), out.c_str(), -1, &report) == SF_ERR_FORMAT && std::strstr(sf_last_error(), "0.png"));
  CHECK(sf_png_write_gray((pp + "/0.png").c_str(), p8.data(), 32, 96, 8) == SF_OK);   // another size
  CHECK(sf_eval_pixel_dir(pp.c_str(), pg.c_str(), out.c_str(), -1, &report) == SF_ERR_FORMAT);
  CHECK(sf_eval_pixel_dir((root + "/nowhere").c_str(), pg.c_str(), nullptr, -1, &report) == SF_ERR_IO);
  // export: a scan folder of two groups; then its three files cut at every length
  const std::string scan = root + "/scene0001_00", sg = scan + "/scene0001_00_vh_clean_2.0.010000.segs.json", ag = scan + "/scene0001_00.aggregation.json";
  const std::string map = root + "/map.tsv", eo = root + "/export";
  mkdir(scan.c_str(), 0755);
  mkdir(eo.c_str(), 0755);
  const std::string segs_text = "{\"sceneId\": \"s\", \"segIndices\": [4, 4, 5, 5, 5, 9]}";
  const std::string agg_text = "{\"segGroups\": [{\"id\": 0, \"objectId\": 0, \"segments\": [4], \"label\": \"chair\"}, "
                               "{\"id\": 1, \"objectId\": 3, \"segments\": [5], \"label\": \"a \\\"table\\\"\"}]}";
  const std::string map_text = "raw_category\tnyu40id\nchair\t5\na \"table\"\t7\n";
  put(sg, segs_text);
  put(ag, agg_text);
  put(map, map_text);
  for (const char* type : {"label", "instance", "instance-gt"}) CHECK(sf_eval_export_scan(scan.c_str(), map.c_str(), type, (eo + "/" + type + ".txt").c_str()) == SF_OK);
  CHECK(get(eo + "/label.txt") == "5\n5\n7\n7\n7\n0\n" && get(eo + "/instance-gt.txt") == "5001\n5001\n7004\n7004\n7004\n0\n");
  CHECK(get(eo + "/instance.txt") == "pred_mask/instance_1.txt 5 1.000000\npred_mask/instance_2.txt 7 1.000000\n" && get(eo + "/pred_mask/instance_2.txt") == "0\n0\n1\n1\n1\n0\n");
  CHECK(sf_eval_export_scan(scan.c_str(), map.c_str(), "other", (eo + "/x.txt").c_str()) == SF_ERR_INVALID_ARG);
  uint64_t nv = 0;
  uint32_t five[5];
  CHECK(sf_eval_export_ids(sg.c_str(), ag.c_str(), map.c_str(), 5, five, nullptr, &nv) == SF_ERR_BOUNDS && nv == 6);
  const std::string* texts[3] = {&segs_text, &agg_text, &map_text};
  const std::string* paths[3] = {&sg, &ag, &map};
  for (int which = 0; which < 3; which++) {
    for (size_t cut = 0; cut < texts[which]->size(); cut++) {
      put(*paths[which], texts[which]->substr(0, cut));
      uint32_t l[6], in[6];
      const int rc = sf_eval_export_ids(sg.c_str(), ag.c_str(), map.c_str(), 6, l, in, &nv);
      CHECK(rc == SF_OK || rc == SF_ERR_FORMAT || rc == SF_ERR_IO);
      CHECK(rc != SF_OK || nv <= 6);
    }
    put(*paths[which], *texts[which]);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && files(argv[1])) return 1;
  uint32_t seed = 777u;
  if (confusion_of_width<uint8_t>(1) || confusion_of_width<uint16_t>(2) || confusion_of_width<uint32_t>(3)) return 1;
  {   // images: every size pair the check lets through reads inside its arrays
    const uint32_t sizes[5][4] = {{1296, 968, 640, 480}, {1296, 968, 1296, 968}, {641, 481, 641, 481}, {1, 1, 1, 1}, {7, 3, 7, 900}};
    for (const auto& s : sizes) {
      std::vector<uint16_t> gt((size_t)2 * s[0] * s[1]), pred((size_t)2 * s[2] * s[3]);
      for (auto& v : gt) v = (uint16_t)(rnd(seed) % 41u);
      for (auto& v : pred) v = (uint16_t)(rnd(seed) % 50u);
      std::vector<uint64_t> conf(41 * 41, 0);
      uint64_t oor = 0, sum = 0;
      CHECK(sf_eval_confusion_images(gt.data(), pred.data(), 2, 2, s[0], s[1], s[2], s[3], 41, -1, conf.data(), &oor) == SF_OK);
      for (uint64_t v : conf) sum += v;
      CHECK(sum + oor == 2ull * 640 * 480);
    }
    uint64_t c = 0, o = 0;
    uint8_t px = 0;
    CHECK(sf_eval_confusion_images(&px, &px, 1, 1, 1296, 968, 648, 484, 41, -1, &c, &o) == SF_ERR_INVALID_ARG);
    CHECK(sf_eval_confusion_images(&px, &px, 1, 1, 0, 968, 0, 484, 41, -1, &c, &o) == SF_ERR_INVALID_ARG);
    CHECK(sf_eval_confusion_images(&px, &px, 1, 1, 1, 1, 1, 1, 64, -1, &c, &o) == SF_ERR_INVALID_ARG);
    CHECK(sf_eval_confusion_images(&px, &px, 1, 1, 1, 1, 1, 1, 1, 0, &c, &o) == SF_ERR_DEVICE);
  }
  {   // iou on the smallest matrix a class list allows, and the refusals of the class list
    const int32_t one[1] = {0};
    const uint64_t m[4] = {3, 1, 0, 0};
    double iou = 0;
    uint64_t tp = 0, denom = 0;
    CHECK(sf_eval_iou(m, 2, one, 1, &iou, &tp, &denom) == SF_OK && tp == 3 && denom == 4 && iou == 0.75);
    CHECK(sf_eval_iou(m, 1, one, 1, &iou, nullptr, nullptr) == SF_OK);   // without the unknown column
    const int32_t bad[2] = {62, 3};
    CHECK(sf_eval_iou(m, 2, bad, 2, &iou, nullptr, nullptr) == SF_ERR_INVALID_ARG);
    CHECK(sf_eval_iou(m, 2, LABELS, 20, &iou, nullptr, nullptr) == SF_ERR_INVALID_ARG);   // the matrix is too small for class 39
  }
  // a scan: plan, overlaps, AP; then the same with nothing in it
  const int32_t inst_labels[18] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};
  sf_eval_ap* acc = nullptr;
  CHECK(sf_eval_ap_create(inst_labels, 18, 100, &acc) == SF_OK);
  for (int scan = 0; scan < 3; scan++) {
    const uint64_t n = 20011;
    std::vector<int32_t> gt(n);
    int32_t cur = 0;
    for (uint64_t v = 0; v < n; v++) {
      if (rnd(seed) % 300u == 0) {
        const uint32_t pick = rnd(seed) % 24u;
        cur = pick < 18 ? inst_labels[pick] * 1000 + (int32_t)(rnd(seed) % 3u) : (pick == 18 ? 0 : (pick == 19 ? -5 : (int32_t)(rnd(seed) % 3000u)));
      }
      gt[v] = cur;
    }
    uint32_t G = 0;
    std::vector<uint32_t> slot(n);
    CHECK(sf_eval_instance_plan(gt.data(), n, inst_labels, 18, nullptr, nullptr, 0, slot.data(), &G) == SF_OK && G > 0);
    std::vector<int32_t> iid(G);
    std::vector<uint32_t> verts(G);
    CHECK(sf_eval_instance_plan(gt.data(), n, inst_labels, 18, iid.data(), verts.data(), G, nullptr, &G) == SF_OK);
    CHECK(sf_eval_instance_plan(gt.data(), n, inst_labels, 18, iid.data(), verts.data(), G - 1, nullptr, &G) == SF_ERR_BOUNDS);
    const uint32_t P = 40;
    const uint64_t stride = n + 13;
    std::vector<uint8_t> masks((size_t)(P - 1) * stride + n, 0);   // the last row ends with the array
    std::vector<int32_t> label(P);
    std::vector<double> conf(P);
    for (uint32_t p = 0; p < P; p++) {
      const uint64_t a = rnd(seed) % n, len = 1 + rnd(seed) % 900u;
      for (uint64_t v = a; v < n && v < a + len; v++) masks[p * stride + v] = (uint8_t)(1 + rnd(seed) % 255u);
      label[p] = (p % 7 == 0) ? -1 : inst_labels[rnd(seed) % 18u];
      conf[p] = (double)(rnd(seed) % 8u) / 8.0;
    }
    std::vector<uint32_t> table((size_t)P * (G + 2), 0xDEADBEEFu);
    CHECK(sf_eval_instance_overlaps(slot.data(), n, G, masks.data(), P, stride, -1, table.data()) == SF_OK);
    for (uint32_t p = 0; p < P; p++) {
      uint64_t sum = 0;
      for (uint32_t g = 0; g <= G; g++) sum += table[(size_t)p * (G + 2) + g];
      CHECK(sum == table[(size_t)p * (G + 2) + G + 1] && sum >= 1);
    }
    CHECK(sf_eval_ap_add_scan(acc, G, iid.data(), verts.data(), P, label.data(), conf.data(), table.data()) == SF_OK);
    table[G + 1] += 1;   // a table that does not add up is refused and leaves the accumulator as it was
    CHECK(sf_eval_ap_add_scan(acc, G, iid.data(), verts.data(), P, label.data(), conf.data(), table.data()) == SF_ERR_INVALID_ARG);
    conf[0] = NAN;
    table[G + 1] -= 1;
    CHECK(sf_eval_ap_add_scan(acc, G, iid.data(), verts.data(), P, label.data(), conf.data(), table.data()) == SF_ERR_INVALID_ARG);
  }
  CHECK(sf_eval_ap_add_scan(acc, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == SF_OK);
  std::vector<double> ap(18 * SF_EVAL_AP_OVERLAPS), cls(18 * 3), avg(3);
  CHECK(sf_eval_ap_finish(acc, ap.data(), cls.data(), avg.data()) == SF_OK);
  int live = 0;
  for (double v : ap) {
    CHECK(std::isnan(v) || (v >= 0.0 && v <= 1.0));
    live += !std::isnan(v);
  }
  CHECK(live >= 100 && avg[0] >= 0.0 && avg[2] <= 1.0);
  CHECK(sf_eval_ap_finish(acc, ap.data(), nullptr, nullptr) == SF_OK);
  sf_eval_ap_destroy(acc);
  sf_eval_ap_destroy(nullptr);
  {   // nothing: n = 0, P = 0, G = 0
    uint32_t G = 99, t[2] = {7, 7};
    CHECK(sf_eval_instance_plan(nullptr, 0, inst_labels, 18, nullptr, nullptr, 0, nullptr, &G) == SF_OK && G == 0);
    CHECK(sf_eval_instance_overlaps(nullptr, 0, 0, nullptr, 1, 0, -1, t) == SF_OK && t[0] == 0 && t[1] == 0);
    CHECK(sf_eval_instance_overlaps(nullptr, 0, 0, nullptr, 0, 0, -1, t) == SF_OK);
    CHECK(sf_eval_instance_overlaps(nullptr, 5, 0, nullptr, 1, 5, -1, t) == SF_ERR_INVALID_ARG);
    CHECK(sf_eval_instance_overlaps(nullptr, 0, 0, nullptr, 1, 0, 0, t) == SF_ERR_DEVICE);
    double th[SF_EVAL_AP_OVERLAPS];
    CHECK(sf_eval_ap_thresholds(th) == SF_OK && th[0] == 0.5 && th[9] == 0.25 && th[8] > 0.9 && th[8] < 0.9000001);
  }
  std::printf("evaluation host: ok\n");
  return 0;
}
