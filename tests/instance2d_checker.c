/* instance2d_checker.c -- the counts of the 2-D instance task by brute force, for tests/instance2d_cases.py: one pass over the
 * image per instance for its pixel count (instance.py:23-24), one per (prediction, instance) pair for their intersection
 * (evalInstanceLevelSemanticLabeling.py:278), one per prediction for void (:230, :266) and one for its pixel count (:251-252).  No table, no sort of
 * the pixels, no sharing with the library.  Pixels arrive as int64 values. */
#include <stdint.h>
#include <stdlib.h>

static int is_valid(int64_t v, const int32_t* valid, int n_valid) {
  for (int i = 0; i < n_valid; i++)
    if (valid[i] == v) return 1;
  return 0;
}

/* the distinct values whose value // 1000 is a valid class, ascending, with their pixel counts; ids and pixels hold n entries.  -> their number */
int64_t i2c_plan(const int64_t* img, int64_t n, const int32_t* valid, int n_valid, int64_t* ids, int64_t* pixels) {
  int64_t G = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t v = img[i];
    if (v < 0 || !is_valid(v / 1000, valid, n_valid)) continue;
    int seen = 0;
    for (int64_t g = 0; g < G && !seen; g++) seen = ids[g] == v;
    if (!seen) ids[G++] = v;
  }
  for (int64_t a = 1; a < G; a++) { /* insertion sort */
    const int64_t v = ids[a];
    int64_t b = a;
    for (; b > 0 && ids[b - 1] > v; b--) ids[b] = ids[b - 1];
    ids[b] = v;
  }
  for (int64_t g = 0; g < G; g++) {
    int64_t c = 0;
    for (int64_t i = 0; i < n; i++) c += img[i] == ids[g];
    pixels[g] = c;
  }
  return G;
}

/* row[G + 2] of one mask over one image: per instance, void, all */
void i2c_overlaps(const int64_t* img, int64_t n, const int32_t* valid, int n_valid, const int64_t* ids, int64_t G, const uint8_t* mask, int64_t* row) {
  for (int64_t g = 0; g < G; g++) {
    int64_t c = 0;
    for (int64_t i = 0; i < n; i++) c += (img[i] == ids[g]) && mask[i] != 0;
    row[g] = c;
  }
  int64_t v = 0, all = 0;
  for (int64_t i = 0; i < n; i++) v += is_valid(img[i], valid, n_valid) && mask[i] != 0;
  for (int64_t i = 0; i < n; i++) all += mask[i] != 0;
  row[G] = v;
  row[G + 1] = all;
}
