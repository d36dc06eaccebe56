// evaluation.cpp -- the benchmark's scores (include/scanfuse.h "Benchmark scores"): the entry points and their checks, the host
// path of the two counting stages (the rules of evaluation_internal.h on at most 16 threads), the IoU, the instance plan and the AP accumulator.  The
// counts are integers, so the host path gives the bits the kernels of evaluation.hip give.  What it replaces:
// BenchmarkScripts/3d_evaluation/evaluate_semantic_label.py, evaluate_semantic_instance.py with util_3d.py, and
// 2d_evaluation/evalPixelLevelSemanticLabeling.py with addToConfusionMatrix_impl.c.  The AP over images of the 2-D instance task (section 4p,
// evalInstanceLevelSemanticLabeling.py:301-515) is here too, beside the AP over scans whose curve it shares; its counting stages are instance2d.cpp.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"
#include "evaluation_internal.h"

namespace {

using sf::ev::MODE_2D;
using sf::ev::MODE_3D;

constexpr uint64_t GRAIN = 1u << 16;   // elements of one job of the host path

using sf::ev::parallel_for;   // at most 16 threads

int check_width(int elem_bytes, const char* who) {
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return sf::fail(SF_ERR_INVALID_ARG, "%s: elements of %d bytes (1, 2 or 4)", who, elem_bytes);
  return SF_OK;
}

inline uint32_t load(const void* p, int elem_bytes, uint64_t i) {
  if (elem_bytes == 1) return ((const uint8_t*)p)[i];
  if (elem_bytes == 2) return ((const uint16_t*)p)[i];
  return ((const uint32_t*)p)[i];
}

// cells[dim * dim + 1]: the matrix and the out-of-range cell
template <typename T>
void count_span(const T* gt, const T* pred, uint64_t b, uint64_t e, uint64_t valid, uint32_t dim, int mode, uint64_t* cells) {
  for (uint64_t i = b; i < e; i++) {
    const uint32_t k = mode == (int)MODE_3D ? sf::ev::key_3d(gt[i], pred[i], valid, dim) : sf::ev::key_2d(gt[i], pred[i], dim);
    if (k != sf::ev::KEY_SKIP) cells[k]++;
  }
}

void host_confusion(const void* gt, const void* pred, int elem_bytes, uint64_t n, uint64_t valid, uint32_t dim, int mode, uint64_t* confusion, uint64_t* oor) {
  const size_t cells = (size_t)dim * dim + 1;
  const uint64_t jobs = (n + GRAIN - 1) / GRAIN;
  std::mutex m;
  std::vector<uint64_t> total(cells, 0);
  parallel_for(jobs, [&](uint64_t j) {
    std::vector<uint64_t> mine(cells, 0);
    const uint64_t b = j * GRAIN, e = std::min(n, b + GRAIN);
    if (elem_bytes == 1) count_span((const uint8_t*)gt, (const uint8_t*)pred, b, e, valid, dim, mode, mine.data());
    else if (elem_bytes == 2) count_span((const uint16_t*)gt, (const uint16_t*)pred, b, e, valid, dim, mode, mine.data());
    else count_span((const uint32_t*)gt, (const uint32_t*)pred, b, e, valid, dim, mode, mine.data());
    std::lock_guard<std::mutex> g(m);
    for (size_t i = 0; i < cells; i++) total[i] += mine[i];
  });
  for (size_t i = 0; i + 1 < cells; i++) confusion[i] += total[i];
  if (oor) *oor += total[cells - 1];
}

void host_confusion_images(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gw, uint32_t gh, uint32_t pw, uint32_t ph, uint32_t dw,
                           uint32_t dh, uint32_t dim, uint64_t* confusion, uint64_t* oor) {
  const size_t cells = (size_t)dim * dim + 1;
  std::mutex m;
  std::vector<uint64_t> total(cells, 0);
  std::vector<uint32_t> gx(dw), px(dw);   // the source column of every destination column
  for (uint32_t x = 0; x < dw; x++) { gx[x] = sf::ev::nn_source(x, gw, dw); px[x] = sf::ev::nn_source(x, pw, dw); }
  const uint64_t rows = (uint64_t)batch * dh, ROWS = 32;   // a job is 32 destination rows
  parallel_for((rows + ROWS - 1) / ROWS, [&](uint64_t j) {
    std::vector<uint64_t> mine(cells, 0);
    for (uint64_t r = j * ROWS; r < rows && r < (j + 1) * ROWS; r++) {
      const uint64_t b = r / dh;
      const uint32_t y = (uint32_t)(r - b * dh);
      const uint64_t grow = (b * gh + sf::ev::nn_source(y, gh, dh)) * gw, prow = (b * ph + sf::ev::nn_source(y, ph, dh)) * pw;
      for (uint32_t x = 0; x < dw; x++) mine[sf::ev::key_2d(load(gt, elem_bytes, grow + gx[x]), load(pred, elem_bytes, prow + px[x]), dim)]++;
    }
    std::lock_guard<std::mutex> g(m);
    for (size_t i = 0; i < cells; i++) total[i] += mine[i];
  });
  for (size_t i = 0; i + 1 < cells; i++) confusion[i] += total[i];
  *oor += total[cells - 1];
}

void host_overlaps(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, uint32_t* table) {
  const size_t bins = (size_t)G + 2;
  parallel_for(P, [&](uint64_t p) {
    uint32_t* row = table + p * bins;
    std::memset(row, 0, bins * 4);
    const uint8_t* mask = masks + p * stride;
    for (uint64_t v = 0; v < n; v++)
      if (mask[v]) {
        row[sf::ev::overlap_bin(slot[v], G)]++;
        row[G + 1]++;
      }
  });
}

}  // namespace

namespace sf {
namespace ev {

int check_images(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gw, uint32_t gh, uint32_t pw, uint32_t ph, uint32_t dim,
                 const uint64_t* confusion, const uint64_t* oor) {
  if (int rc = check_width(elem_bytes, "sf_eval_confusion_images")) return rc;
  if (!confusion || !oor || (batch && (!gt || !pred))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (dim < 1 || dim > sf::ev::MAX_DIM) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_images: dim %u (1 .. %u)", dim, sf::ev::MAX_DIM);
  const uint32_t lim = 1u << 15;
  if (batch && (gw < 1 || gh < 1 || pw < 1 || ph < 1 || gw > lim || gh > lim || pw > lim || ph > lim))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_images: images of %u x %u and %u x %u (1 .. 32768 per side)", gw, gh, pw, ph);
  if (batch > (1u << 20)) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_images: %u pairs in one call (up to 2^20)", batch);
  // evalPixelLevelSemanticLabeling.py:240
  if (batch && !(pw == gw || (pw == SF_EVAL_IMAGE_WIDTH && ph == SF_EVAL_IMAGE_HEIGHT)))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_images: a prediction of %u x %u against a ground truth of %u x %u (the same width, or 640 x 480)", pw, ph, gw,
                    gh);
  return SF_OK;
}

int check_valid(const int32_t* valid_ids, uint32_t n_valid, uint64_t* mask, uint32_t* dim, const char* who) {
  if (!valid_ids || n_valid == 0) return sf::fail(SF_ERR_INVALID_ARG, "%s: no valid class ids", who);
  uint64_t m = 0;
  int32_t top = 0;
  for (uint32_t i = 0; i < n_valid; i++) {
    const int32_t id = valid_ids[i];
    if (id < 0 || id > (int32_t)MAX_DIM - 2) return sf::fail(SF_ERR_INVALID_ARG, "%s: class id %d (0 .. %u)", who, id, MAX_DIM - 2);
    if ((m >> id) & 1ull) return sf::fail(SF_ERR_INVALID_ARG, "%s: class id %d twice", who, id);
    m |= 1ull << id;
    top = std::max(top, id);
  }
  *mask = m;
  *dim = (uint32_t)top + 2u;
  return SF_OK;
}

// the 2-D instance task (section 4p): ids 1 .. 999, so that a void value (a valid id) can never be an instance id (1000 and up)
int check_valid_2d(const int32_t* valid_ids, uint32_t n_valid, ValidSet* vs, const char* who) {
  if (!valid_ids || n_valid == 0) return sf::fail(SF_ERR_INVALID_ARG, "%s: no valid class ids", who);
  std::memset(vs, 0, sizeof(*vs));
  for (uint32_t i = 0; i < n_valid; i++) {
    const int32_t id = valid_ids[i];
    if (id < 1 || id > 999) return sf::fail(SF_ERR_INVALID_ARG, "%s: class id %d (1 .. 999)", who, id);
    if (in_set(vs->bits, (uint32_t)id)) return sf::fail(SF_ERR_INVALID_ARG, "%s: class id %d twice", who, id);
    vs->bits[id >> 5] |= 1u << (id & 31);
    vs->top = std::max(vs->top, (uint32_t)id);
  }
  return SF_OK;
}

}  // namespace ev
}  // namespace sf

SF_API int sf_eval_confusion(const void* gt, const void* pred, int elem_bytes, uint64_t n, const int32_t* valid_ids, uint32_t n_valid, int mode, int device,
                             uint64_t* confusion, uint64_t* out_of_range) {
  uint64_t valid = 0;
  uint32_t dim = 0;
  if (int rc = check_width(elem_bytes, "sf_eval_confusion")) return rc;
  if (int rc = sf::ev::check_valid(valid_ids, n_valid, &valid, &dim, "sf_eval_confusion")) return rc;
  if (mode != (int)MODE_3D && mode != (int)MODE_2D) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion: mode %d", mode);
  if (!confusion || (mode == (int)MODE_2D && !out_of_range) || (n && (!gt || !pred))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (n > sf::ev::MAX_ELEMENTS) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion: %llu elements in one call (up to 2^40)", (unsigned long long)n);
  if (device >= 0) return sf::ev::confusion_on_device(gt, pred, elem_bytes, n, valid, dim, mode, device, confusion, out_of_range);
  host_confusion(gt, pred, elem_bytes, n, valid, dim, mode, confusion, out_of_range);
  return SF_OK;
}

SF_API int sf_eval_confusion_images(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gt_width, uint32_t gt_height, uint32_t pred_width,
                                    uint32_t pred_height, uint32_t dim, int device, uint64_t* confusion, uint64_t* out_of_range) {
  if (int rc = sf::ev::check_images(gt, pred, elem_bytes, batch, gt_width, gt_height, pred_width, pred_height, dim, confusion, out_of_range)) return rc;
  if (device >= 0)
    return sf::ev::confusion_images_on_device(gt, pred, elem_bytes, batch, gt_width, gt_height, pred_width, pred_height, SF_EVAL_IMAGE_WIDTH, SF_EVAL_IMAGE_HEIGHT,
                                              dim, device, confusion, out_of_range);
  host_confusion_images(gt, pred, elem_bytes, batch, gt_width, gt_height, pred_width, pred_height, SF_EVAL_IMAGE_WIDTH, SF_EVAL_IMAGE_HEIGHT, dim, confusion,
                        out_of_range);
  return SF_OK;
}

// get_iou, evaluate_semantic_label.py:68-82
SF_API int sf_eval_iou(const uint64_t* confusion, uint32_t dim, const int32_t* valid_ids, uint32_t n_valid, double* iou, uint64_t* tp, uint64_t* denom) {
  uint64_t valid = 0;
  uint32_t need = 0;
  if (int rc = sf::ev::check_valid(valid_ids, n_valid, &valid, &need, "sf_eval_iou")) return rc;
  if (!confusion || !iou) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (dim < need - 1 || dim > sf::ev::MAX_DIM) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_iou: a matrix of %u rows for class ids up to %u", dim, need - 2);
  for (uint32_t i = 0; i < n_valid; i++) {
    const uint32_t id = (uint32_t)valid_ids[i];
    const uint64_t t = confusion[(size_t)id * dim + id];
    uint64_t row = 0, fp = 0;
    for (uint32_t c = 0; c < dim; c++) row += confusion[(size_t)id * dim + c];
    for (uint32_t j = 0; j < n_valid; j++)
      if (valid_ids[j] != (int32_t)id) fp += confusion[(size_t)valid_ids[j] * dim + id];
    const uint64_t d = t + fp + (row - t);
    iou[i] = d ? (double)t / (double)d : std::numeric_limits<double>::quiet_NaN();
    if (tp) tp[i] = t;
    if (denom) denom[i] = d;
  }
  return SF_OK;
}

// util_3d.get_instances and the void mask of assign_instances_for_scan (evaluate_semantic_instance.py:256,267)
SF_API int sf_eval_instance_plan(const int32_t* gt_ids, uint64_t n, const int32_t* valid_ids, uint32_t n_valid, int32_t* instance_id, uint32_t* instance_verts,
                                 uint32_t capacity, uint32_t* slot, uint32_t* count) {
  uint64_t valid = 0;
  uint32_t dim = 0;
  if (int rc = sf::ev::check_valid(valid_ids, n_valid, &valid, &dim, "sf_eval_instance_plan")) return rc;
  if (!count || (n && !gt_ids)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (n >= (1ull << 32)) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_instance_plan: %llu vertices (below 2^32)", (unsigned long long)n);
  auto is_instance = [&](int32_t id) {   // non-zero, and id // 1000 is a valid class: a negative id floors below zero
    if (id <= 0) return false;
    const uint32_t label = (uint32_t)id / 1000u;
    return label < dim && ((valid >> label) & 1ull) != 0;
  };
  std::vector<int32_t> ids;
  for (uint64_t v = 0; v < n; v++)
    if (is_instance(gt_ids[v])) ids.push_back(gt_ids[v]);
  std::sort(ids.begin(), ids.end());
  std::vector<int32_t> uniq;
  std::vector<uint32_t> verts;
  for (size_t i = 0; i < ids.size(); i++) {
    if (uniq.empty() || uniq.back() != ids[i]) { uniq.push_back(ids[i]); verts.push_back(0); }
    verts.back()++;
  }
  const uint32_t G = (uint32_t)uniq.size();
  *count = G;
  for (uint32_t g = 0; g < G && g < capacity; g++) {
    if (instance_id) instance_id[g] = uniq[g];
    if (instance_verts) instance_verts[g] = verts[g];
  }
  if (slot)
    for (uint64_t v = 0; v < n; v++)
      slot[v] = is_instance(gt_ids[v]) ? (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), gt_ids[v]) - uniq.begin()) : G;
  if ((instance_id || instance_verts) && capacity < G) return sf::fail(SF_ERR_BOUNDS, "sf_eval_instance_plan: %u instances, capacity %u", G, capacity);
  return SF_OK;
}

namespace sf {
namespace ev {
int check_overlaps(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* table) {
  if ((P && !table) || (P && n && (!slot || !masks))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (n >= (1ull << 32)) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_instance_overlaps: %llu vertices (below 2^32: the counters are 32-bit)", (unsigned long long)n);
  if (stride < n) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_instance_overlaps: a mask stride of %llu for %llu vertices", (unsigned long long)stride, (unsigned long long)n);
  if (P > 65535u || G > (1u << 24)) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_instance_overlaps: %u predictions (up to 65535), %u instances (up to 2^24)", P, G);
  return SF_OK;
}
}  // namespace ev
}  // namespace sf

SF_API int sf_eval_instance_overlaps(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, int device, uint32_t* table) {
  if (int rc = sf::ev::check_overlaps(slot, n, G, masks, P, stride, table)) return rc;
  if (device >= 0) return sf::ev::overlaps_on_device(slot, n, G, masks, P, stride, device, table);
  host_overlaps(slot, n, G, masks, P, stride, table);
  return SF_OK;
}

// ---- the AP over scans (evaluate_matches and compute_averages, evaluate_semantic_instance.py:75-242) ----

namespace {

struct Match {   // a ground-truth instance and a prediction of its class that share vertices
  uint32_t other;          // index of the prediction (in Gt::preds) or of the instance (in Pred::gts) within the scan's class
  uint32_t intersection;
};
struct Gt {
  int32_t id;
  uint32_t verts;
  std::vector<Match> preds;   // in prediction order
};
struct Pred {
  double conf;
  uint32_t verts, void_intersection;
  std::vector<Match> gts;     // in ascending instance id
};
struct ClassScan {
  std::vector<Gt> gts;        // every instance of the class, the small ones included
  std::vector<Pred> preds;    // the kept predictions of the class
};

}  // namespace

struct sf_eval_ap {
  std::vector<int32_t> valid_ids;
  uint64_t valid = 0;
  uint32_t dim = 0;
  uint32_t min_region = 100;
  std::vector<std::vector<ClassScan>> scans;   // [class][scan]
};

SF_API int sf_eval_ap_create(const int32_t* valid_ids, uint32_t n_valid, uint32_t min_region_size, sf_eval_ap** out) {
  if (!out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *out = nullptr;
  uint64_t valid = 0;
  uint32_t dim = 0;
  if (int rc = sf::ev::check_valid(valid_ids, n_valid, &valid, &dim, "sf_eval_ap_create")) return rc;
  sf_eval_ap* a = new sf_eval_ap;
  a->valid_ids.assign(valid_ids, valid_ids + n_valid);
  a->valid = valid;
  a->dim = dim;
  a->min_region = min_region_size;
  a->scans.resize(n_valid);
  *out = a;
  return SF_OK;
}

SF_API void sf_eval_ap_destroy(sf_eval_ap* acc) { delete acc; }

SF_API int sf_eval_ap_add_scan(sf_eval_ap* acc, uint32_t G, const int32_t* instance_id, const uint32_t* instance_verts, uint32_t P, const int32_t* pred_label,
                               const double* pred_conf, const uint32_t* table) {
  if (!acc || (G && (!instance_id || !instance_verts)) || (P && (!pred_label || !pred_conf || !table))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const size_t bins = (size_t)G + 2;
  auto class_of = [&](int64_t label) -> int {
    if (label < 0 || label >= (int64_t)acc->dim || !((acc->valid >> label) & 1ull)) return -1;
    for (size_t i = 0; i < acc->valid_ids.size(); i++)
      if (acc->valid_ids[i] == (int32_t)label) return (int)i;
    return -1;
  };
  for (uint32_t g = 0; g < G; g++) {
    if (instance_id[g] <= 0 || class_of(instance_id[g] / 1000) < 0)
      return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap_add_scan: instance %u has id %d, which names no valid class", g, instance_id[g]);
    if (g && instance_id[g] <= instance_id[g - 1]) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap_add_scan: the instance ids do not ascend at %u", g);
  }
  for (uint32_t p = 0; p < P; p++) {
    if (std::isnan(pred_conf[p])) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap_add_scan: prediction %u has no confidence (NaN)", p);
    const uint32_t* row = table + p * bins;
    uint64_t sum = 0;
    for (uint32_t g = 0; g <= G; g++) {
      sum += row[g];
      if (g < G && row[g] > instance_verts[g]) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap_add_scan: prediction %u shares %u vertices with an instance of %u", p, row[g], instance_verts[g]);
    }
    if (sum != row[G + 1]) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap_add_scan: the counts of prediction %u add up to %llu, not to its %u vertices", p, (unsigned long long)sum, row[G + 1]);
  }
  std::vector<ClassScan> add(acc->valid_ids.size());
  std::vector<uint32_t> index(G);   // of an instance within its class
  for (uint32_t g = 0; g < G; g++) {
    ClassScan& cs = add[class_of(instance_id[g] / 1000)];
    index[g] = (uint32_t)cs.gts.size();
    cs.gts.push_back(Gt{instance_id[g], instance_verts[g], {}});
  }
  for (uint32_t p = 0; p < P; p++) {
    const int c = class_of(pred_label[p]);
    const uint32_t* row = table + p * bins;
    if (c < 0 || row[G + 1] < acc->min_region) continue;   // dropped: no valid class, or too small
    ClassScan& cs = add[c];
    Pred pr{pred_conf[p], row[G + 1], row[G], {}};
    const uint32_t pi = (uint32_t)cs.preds.size();
    for (uint32_t g = 0; g < G; g++)
      if (row[g] > 0 && class_of(instance_id[g] / 1000) == c) {
        pr.gts.push_back(Match{index[g], row[g]});
        cs.gts[index[g]].preds.push_back(Match{pi, row[g]});
      }
    cs.preds.push_back(std::move(pr));
  }
  for (size_t c = 0; c < add.size(); c++) acc->scans[c].push_back(std::move(add[c]));
  return SF_OK;
}

namespace {

// the overlap thresholds as numpy makes them: np.append(np.arange(0.5, 0.95, 0.05), 0.25); arange fills start + i * ((start + step) - start)
void thresholds(double* th) {
  volatile double start = 0.5, step = 0.05;
  volatile double next = start + step;
  const double delta = next - start;
  for (int i = 0; i < 9; i++) th[i] = start + (double)i * delta;
  th[9] = 0.25;
}

double iou_of(uint32_t inter, uint32_t a, uint32_t b) { return (double)inter / (double)((uint64_t)a + b - inter); }

// the precision-recall curve and its step-wise integral (evaluate_semantic_instance.py:169-217; evalInstanceLevelSemanticLabeling.py:435-488, the same
// lines): y = (score, true) in any order, hard_fn = the ground truth no prediction matched.  Both accumulators end here.
double curve_ap(std::vector<std::pair<double, double>>& y, uint64_t hard_fn) {
  std::sort(y.begin(), y.end(), [](const std::pair<double, double>& a, const std::pair<double, double>& b) { return a.first < b.first; });
  const size_t n = y.size();
  std::vector<double> cum(n);
  double run = 0.0;
  for (size_t i = 0; i < n; i++) { run += y[i].second; cum[i] = run; }
  const double num_true = n ? cum[n - 1] : 0.0;   // the reference indexes an empty array here (IndexError); the curve is the artificial point alone: 0
  std::vector<double> precision, recall;
  for (size_t i = 0; i < n; i++) {
    if (i && y[i].first == y[i - 1].first) continue;   // the first index of each distinct score
    const double before = i ? cum[i - 1] : 0.0;
    const double tp = num_true - before, fp = (double)n - (double)i - tp, fn = before + (double)hard_fn;
    precision.push_back(tp / (tp + fp));
    recall.push_back(tp / (tp + fn));
  }
  precision.push_back(1.0);
  recall.push_back(0.0);
  // recall_for_conv = [r0, r0 .. r(K-1), 0, 0]; np.convolve(., [-0.5, 0, 0.5], 'valid')[j] = 0.5 a[j] - 0.5 a[j + 2]
  std::vector<double> a;
  a.push_back(recall[0]);
  a.insert(a.end(), recall.begin(), recall.end());
  a.push_back(0.0);
  double ap = 0.0;
  for (size_t j = 0; j < precision.size(); j++) ap += precision[j] * (0.5 * a[j] + -0.5 * a[j + 2]);
  return ap;
}

double class_ap(const std::vector<ClassScan>& scans, double th, uint32_t min_region) {
  std::vector<std::pair<double, double>> y;   // (score, true)
  uint64_t hard_fn = 0;
  bool has_gt = false, has_pred = false;
  const double ninf = -std::numeric_limits<double>::infinity();
  for (const ClassScan& cs : scans) {
    std::vector<char> visited(cs.preds.size(), 0);
    if (!cs.preds.empty()) has_pred = true;
    for (const Gt& gt : cs.gts) {
      if (gt.id < 1000 || gt.verts < min_region) continue;   // groups and small instances are no ground truth here
      has_gt = true;
      bool matched = false;
      double score = ninf;
      for (const Match& m : gt.preds) {
        if (visited[m.other]) continue;
        const Pred& pr = cs.preds[m.other];
        if (!(iou_of(m.intersection, gt.verts, pr.verts) > th)) continue;
        if (matched) {   // the lower score is a false positive; this prediction is not marked visited
          const double hi = std::max(score, pr.conf), lo = std::min(score, pr.conf);
          score = hi;
          y.emplace_back(lo, 0.0);
        } else {
          matched = true;
          score = pr.conf;
          visited[m.other] = 1;
        }
      }
      if (matched) y.emplace_back(score, 1.0);
      else hard_fn++;
    }
    for (const Pred& pr : cs.preds) {
      bool found = false;
      for (const Match& m : pr.gts)
        if (iou_of(m.intersection, cs.gts[m.other].verts, pr.verts) > th) { found = true; break; }
      if (found) continue;
      uint64_t ignore = pr.void_intersection;
      for (const Match& m : pr.gts) {
        const Gt& gt = cs.gts[m.other];
        if (gt.id < 1000) ignore += m.intersection;
        if (gt.verts < min_region) ignore += m.intersection;
      }
      if ((double)ignore / (double)pr.verts <= th) y.emplace_back(pr.conf, 0.0);
    }
  }
  if (!has_gt) return std::numeric_limits<double>::quiet_NaN();
  if (!has_pred) return 0.0;
  return curve_ap(y, hard_fn);
}

double nanmean(const std::vector<double>& v) {
  double s = 0.0;
  size_t n = 0;
  for (double x : v)
    if (!std::isnan(x)) { s += x; n++; }
  return n ? s / (double)n : std::numeric_limits<double>::quiet_NaN();
}

}  // namespace

SF_API int sf_eval_ap_thresholds(double* th) {
  if (!th) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  thresholds(th);
  return SF_OK;
}

SF_API int sf_eval_ap_finish(const sf_eval_ap* acc, double* ap, double* class_averages, double* averages) {
  if (!acc || !ap) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  double th[SF_EVAL_AP_OVERLAPS];
  thresholds(th);
  const size_t C = acc->valid_ids.size();
  parallel_for(C * SF_EVAL_AP_OVERLAPS, [&](uint64_t j) {
    const size_t c = j / SF_EVAL_AP_OVERLAPS, o = j % SF_EVAL_AP_OVERLAPS;
    ap[j] = class_ap(acc->scans[c], th[o], acc->min_region);
  });
  std::vector<double> all, all50, all25;
  for (size_t c = 0; c < C; c++) {
    const double* row = ap + c * SF_EVAL_AP_OVERLAPS;
    double s = 0.0;
    for (int o = 0; o < 9; o++) { s += row[o]; all.push_back(row[o]); }
    all50.push_back(row[0]);
    all25.push_back(row[9]);
    if (class_averages) {
      class_averages[3 * c] = s / 9.0;
      class_averages[3 * c + 1] = row[0];
      class_averages[3 * c + 2] = row[9];
    }
  }
  if (averages) {
    averages[0] = nanmean(all);
    averages[1] = nanmean(all50);
    averages[2] = nanmean(all25);
  }
  return SF_OK;
}

// ---- the AP over images (evaluateMatches and computeAverages, evalInstanceLevelSemanticLabeling.py:301-515) ----

struct sf_eval_ap2d {
  std::vector<int32_t> valid_ids;
  std::vector<int> class_of;   // [1000]: the position of a class id among valid_ids, or -1
  uint32_t min_region = 100;
  std::vector<std::vector<ClassScan>> images;   // [class][image]
};

SF_API int sf_eval_ap2d_create(const int32_t* valid_ids, uint32_t n_valid, uint32_t min_region_size, sf_eval_ap2d** out) {
  if (!out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *out = nullptr;
  sf::ev::ValidSet vs;
  if (int rc = sf::ev::check_valid_2d(valid_ids, n_valid, &vs, "sf_eval_ap2d_create")) return rc;
  sf_eval_ap2d* a = new sf_eval_ap2d;
  a->valid_ids.assign(valid_ids, valid_ids + n_valid);
  a->class_of.assign(1000, -1);
  for (uint32_t i = 0; i < n_valid; i++) a->class_of[valid_ids[i]] = (int)i;
  a->min_region = min_region_size;
  a->images.resize(n_valid);
  *out = a;
  return SF_OK;
}

SF_API void sf_eval_ap2d_destroy(sf_eval_ap2d* acc) { delete acc; }

SF_API int sf_eval_ap2d_add_image(sf_eval_ap2d* acc, uint32_t G, const int32_t* instance_id, const uint32_t* instance_pixels, uint32_t P,
                                  const int32_t* pred_label, const double* pred_conf, const uint32_t* table, uint32_t capacity) {
  if (!acc || (G && (!instance_id || !instance_pixels)) || (P && (!pred_label || !pred_conf || !table))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (G > capacity) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap2d_add_image: %u instances in rows of capacity %u", G, capacity);
  const size_t bins = (size_t)capacity + 2;
  auto class_of = [&](int64_t label) -> int { return label < 1 || label > 999 ? -1 : acc->class_of[(size_t)label]; };
  for (uint32_t g = 0; g < G; g++) {
    if (instance_id[g] <= 0 || class_of(instance_id[g] / 1000) < 0)
      return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap2d_add_image: instance %u has id %d, which names no valid class", g, instance_id[g]);
    if (g && instance_id[g] <= instance_id[g - 1]) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap2d_add_image: the instance ids do not ascend at %u", g);
  }
  for (uint32_t p = 0; p < P; p++) {
    if (std::isnan(pred_conf[p])) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap2d_add_image: prediction %u has no confidence (NaN)", p);
    const uint32_t* row = table + p * bins;
    uint64_t sum = row[capacity];
    for (uint32_t g = 0; g < G; g++) {
      sum += row[g];
      if (row[g] > instance_pixels[g]) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap2d_add_image: prediction %u shares %u pixels with an instance of %u", p, row[g], instance_pixels[g]);
    }
    // pixels that are neither of an instance nor void count in the total alone
    if (sum > row[capacity + 1]) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_ap2d_add_image: the counts of prediction %u add up to %llu, above its %u pixels", p, (unsigned long long)sum, row[capacity + 1]);
  }
  std::vector<ClassScan> add(acc->valid_ids.size());
  std::vector<uint32_t> index(G);   // of an instance within its class
  for (uint32_t g = 0; g < G; g++) {
    ClassScan& cs = add[class_of(instance_id[g] / 1000)];
    index[g] = (uint32_t)cs.gts.size();
    cs.gts.push_back(Gt{instance_id[g], instance_pixels[g], {}});
  }
  for (uint32_t p = 0; p < P; p++) {
    const int c = class_of(pred_label[p]);
    const uint32_t* row = table + p * bins;
    if (c < 0 || row[capacity + 1] == 0) continue;   // dropped: no valid class (:239), or empty (:255); no minimum size
    ClassScan& cs = add[c];
    Pred pr{pred_conf[p], row[capacity + 1], row[capacity], {}};
    const uint32_t pi = (uint32_t)cs.preds.size();
    for (uint32_t g = 0; g < G; g++)
      if (row[g] > 0 && class_of(instance_id[g] / 1000) == c) {
        pr.gts.push_back(Match{index[g], row[g]});
        cs.gts[index[g]].preds.push_back(Match{pi, row[g]});
      }
    cs.preds.push_back(std::move(pr));
  }
  for (size_t c = 0; c < add.size(); c++) acc->images[c].push_back(std::move(add[c]));
  return SF_OK;
}

namespace {

// numpy's arange(0.5, 1., 0.05): ten values start + i * ((start + step) - start)
void thresholds_2d(double* th) {
  volatile double start = 0.5, step = 0.05;
  volatile double next = start + step;
  const double delta = next - start;
  for (int i = 0; i < SF_EVAL_AP2D_OVERLAPS; i++) th[i] = start + (double)i * delta;
}

// evalInstanceLevelSemanticLabeling.py:349-432 for one class and threshold: no visited flag, no minimum prediction size; small ground truth is ignored
double class_ap_2d(const std::vector<ClassScan>& images, double th, uint32_t min_region) {
  std::vector<std::pair<double, double>> y;   // (score, true)
  uint64_t hard_fn = 0;
  bool has_gt = false, has_pred = false;
  for (const ClassScan& cs : images) {
    if (!cs.preds.empty()) has_pred = true;   // :365, the predictions that are ignored below included
    for (const Gt& gt : cs.gts) {
      if (gt.verts < min_region) continue;    // :361; instID >= 1000 always holds, the distance fields have no effect
      has_gt = true;
      bool matched = false;
      double score = 0.0;
      for (const Match& m : gt.preds) {
        const Pred& pr = cs.preds[m.other];
        if (!(iou_of(m.intersection, gt.verts, pr.verts) > th)) continue;
        if (matched) {   // :383-390: the lower of the two scores is a false positive, the instance keeps the higher
          const double hi = std::max(score, pr.conf), lo = std::min(score, pr.conf);
          score = hi;
          y.emplace_back(lo, 0.0);
        } else {
          matched = true;
          score = pr.conf;
        }
      }
      if (matched) y.emplace_back(score, 1.0);
      else hard_fn++;
    }
    for (const Pred& pr : cs.preds) {   // :405-428
      bool found = false;
      for (const Match& m : pr.gts)
        if (iou_of(m.intersection, cs.gts[m.other].verts, pr.verts) > th) { found = true; break; }
      if (found) continue;
      uint64_t ignore = pr.void_intersection;
      for (const Match& m : pr.gts)
        if (cs.gts[m.other].verts < min_region) ignore += m.intersection;
      if ((double)ignore / (double)pr.verts <= th) y.emplace_back(pr.conf, 0.0);
    }
  }
  if (!has_gt) return std::numeric_limits<double>::quiet_NaN();
  if (!has_pred) return 0.0;
  return curve_ap(y, hard_fn);
}

}  // namespace

SF_API int sf_eval_ap2d_thresholds(double* th) {
  if (!th) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  thresholds_2d(th);
  return SF_OK;
}

SF_API int sf_eval_ap2d_finish(const sf_eval_ap2d* acc, double* ap, double* class_averages, double* averages) {
  if (!acc || !ap) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  double th[SF_EVAL_AP2D_OVERLAPS];
  thresholds_2d(th);
  const size_t C = acc->valid_ids.size();
  parallel_for(C * SF_EVAL_AP2D_OVERLAPS, [&](uint64_t j) {
    const size_t c = j / SF_EVAL_AP2D_OVERLAPS, o = j % SF_EVAL_AP2D_OVERLAPS;
    ap[j] = class_ap_2d(acc->images[c], th[o], acc->min_region);
  });
  std::vector<double> all, all50;
  for (size_t c = 0; c < C; c++) {
    const double* row = ap + c * SF_EVAL_AP2D_OVERLAPS;
    double s = 0.0;
    for (int o = 0; o < SF_EVAL_AP2D_OVERLAPS; o++) { s += row[o]; all.push_back(row[o]); }
    all50.push_back(row[0]);
    if (class_averages) {
      class_averages[2 * c] = s / (double)SF_EVAL_AP2D_OVERLAPS;   // :512
      class_averages[2 * c + 1] = row[0];                          // :513
    }
  }
  if (averages) {
    averages[0] = nanmean(all);     // :506
    averages[1] = nanmean(all50);   // :507
  }
  return SF_OK;
}
