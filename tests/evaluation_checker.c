/* evaluation_checker.c -- the counting rules of the benchmark's scores by brute force, one plain loop per rule, written from
 * the section and not from the library's header: class membership is a search of the list, the resize is the floating-point formula, instances are
 * found by repeated minimum search.  Values arrive as int64 (what the element holds, read as an unsigned integer).  tests/evaluation_cases.py builds
 * it with gcc and holds the library's host and device paths against it, count for count. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static int is_valid(int64_t id, const int32_t* valid, int n_valid) {
  for (int i = 0; i < n_valid; i++)
    if (valid[i] == id) return 1;
  return 0;
}

static int64_t dim_of(const int32_t* valid, int n_valid) {
  int64_t top = 0;
  for (int i = 0; i < n_valid; i++)
    if (valid[i] > top) top = valid[i];
  return top + 2;
}

/* conf[dim][dim] is added to */
void evc_confusion_3d(const int64_t* gt, const int64_t* pred, int64_t n, const int32_t* valid, int n_valid, uint64_t* conf) {
  const int64_t dim = dim_of(valid, n_valid);
  for (int64_t i = 0; i < n; i++) {
    if (!is_valid(gt[i], valid, n_valid)) continue;
    const int64_t col = is_valid(pred[i], valid, n_valid) ? pred[i] : dim - 1;
    conf[gt[i] * dim + col] += 1;
  }
}

void evc_confusion_2d(const int64_t* gt, const int64_t* pred, int64_t n, int64_t dim, uint64_t* conf, uint64_t* out_of_range) {
  for (int64_t i = 0; i < n; i++) {
    if (gt[i] >= dim || pred[i] >= dim || gt[i] < 0 || pred[i] < 0) *out_of_range += 1;
    else conf[gt[i] * dim + pred[i]] += 1;
  }
}

/* nearest neighbour: source index = floor((dst + 0.5) * src / dst size) */
void evc_resize(const int64_t* src, int64_t sw, int64_t sh, int64_t* dst, int64_t dw, int64_t dh) {
  for (int64_t y = 0; y < dh; y++)
    for (int64_t x = 0; x < dw; x++) {
      const int64_t sy = (int64_t)floor(((double)y + 0.5) * (double)sh / (double)dh), sx = (int64_t)floor(((double)x + 0.5) * (double)sw / (double)dw);
      dst[y * dw + x] = src[sy * sw + sx];
    }
}

void evc_iou(const uint64_t* conf, int64_t dim, const int32_t* valid, int n_valid, double* iou, uint64_t* tp, uint64_t* denom) {
  for (int i = 0; i < n_valid; i++) {
    const int64_t id = valid[i];
    uint64_t t = conf[id * dim + id], fn = 0, fp = 0;
    for (int64_t c = 0; c < dim; c++)
      if (c != id) fn += conf[id * dim + c];
    for (int j = 0; j < n_valid; j++)
      if (valid[j] != id) fp += conf[(int64_t)valid[j] * dim + id];
    tp[i] = t;
    denom[i] = t + fp + fn;
    iou[i] = denom[i] ? (double)t / (double)denom[i] : NAN;
  }
}

static int64_t floor_div_1000(int64_t id) { return id >= 0 ? id / 1000 : -((-id + 999) / 1000); }

/* -> G; ids[], verts[] (room for n), slot[n] */
int64_t evc_plan(const int32_t* gt_ids, int64_t n, const int32_t* valid, int n_valid, int32_t* ids, uint32_t* verts, uint32_t* slot) {
  int64_t G = 0, last = 0;
  for (;;) {   /* the smallest instance id above the last one */
    int64_t next = -1;
    for (int64_t v = 0; v < n; v++) {
      const int64_t id = gt_ids[v];
      if (id != 0 && id > last && is_valid(floor_div_1000(id), valid, n_valid) && (next < 0 || id < next)) next = id;
    }
    if (next < 0) break;
    uint32_t count = 0;
    for (int64_t v = 0; v < n; v++)
      if (gt_ids[v] == next) count++;
    ids[G] = (int32_t)next;
    verts[G] = count;
    G++;
    last = next;
  }
  for (int64_t v = 0; v < n; v++) {
    slot[v] = (uint32_t)G;
    if (!is_valid(floor_div_1000(gt_ids[v]), valid, n_valid) || gt_ids[v] == 0) continue;
    for (int64_t g = 0; g < G; g++)
      if (ids[g] == gt_ids[v]) slot[v] = (uint32_t)g;
  }
  return G;
}

/* table[P][G + 2] is written */
void evc_overlaps(const uint32_t* slot, int64_t n, int64_t G, const uint8_t* masks, int64_t P, int64_t stride, uint32_t* table) {
  memset(table, 0, (size_t)(P * (G + 2)) * 4);
  for (int64_t p = 0; p < P; p++)
    for (int64_t v = 0; v < n; v++) {
      if (masks[p * stride + v] == 0) continue;
      table[p * (G + 2) + G + 1] += 1;
      if (slot[v] >= G) table[p * (G + 2) + G] += 1;
      else table[p * (G + 2) + slot[v]] += 1;
    }
}
