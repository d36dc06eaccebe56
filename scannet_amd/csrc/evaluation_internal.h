// evaluation_internal.h -- the rules of the benchmark scores (include/scanfuse.h "Benchmark scores"), written once for the host
// path (evaluation.cpp) and the kernels (evaluation.hip): which cell of the confusion matrix an element counts in, the source pixel of the nearest-neighbour
// resize, and the bin of a vertex in a prediction's overlap histogram.  Everything here is integer arithmetic, so every schedule gives the same counts.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SF_EV_HD __host__ __device__ inline
#else
#define SF_EV_HD inline
#endif

namespace sf {
namespace ev {

constexpr uint32_t MAX_DIM = 63;             // the valid-class set is one 64-bit mask: membership is a shift; four LDS copies of 63 x 63 + 1 counters stay under 64 KiB
constexpr uint32_t KEY_SKIP = 0xFFFFFFFFu;   // the element is not counted
constexpr uint64_t MAX_ELEMENTS = 1ull << 40;
constexpr uint32_t MODE_3D = 0, MODE_2D = 1;

// Elements are unsigned integers of 1, 2 or 4 bytes.  A negative value of a signed type is a value >= 2^(bits - 1) here: no valid class and above every
// dim, which is what the rules below ask of it.

// 3-D mode (evaluate_semantic_label.py:60-65): an element whose ground truth is no valid class is skipped; a prediction that is no valid class goes to
// column dim - 1.  -> gt * dim + pred, or KEY_SKIP
SF_EV_HD uint32_t key_3d(uint32_t gt, uint32_t pred, uint64_t valid, uint32_t dim) {
  if (gt >= dim || !((valid >> gt) & 1ull)) return KEY_SKIP;
  const uint32_t col = (pred < dim && ((valid >> pred) & 1ull)) ? pred : dim - 1u;
  return gt * dim + col;
}

// 2-D mode (addToConfusionMatrix_impl.c): every pixel counts at [gt][pred]; an id >= dim in either image is counted as out of range instead, in the
// extra cell dim * dim (the reference writes outside its matrix there).
SF_EV_HD uint32_t key_2d(uint32_t gt, uint32_t pred, uint32_t dim) {
  if (gt >= dim || pred >= dim) return dim * dim;
  return gt * dim + pred;
}

template <uint32_t MODE>
SF_EV_HD uint32_t key_of(uint32_t gt, uint32_t pred, uint64_t valid, uint32_t dim) {
  return MODE == MODE_3D ? key_3d(gt, pred, valid, dim) : key_2d(gt, pred, dim);
}

// nearest-neighbour resize: source index = floor((dst + 0.5) * src / size) = ((2 dst + 1) * src) / (2 size), exact in integers (sizes below 2^24)
SF_EV_HD uint32_t nn_source(uint32_t dst, uint32_t src, uint32_t size) {
  return (uint32_t)(((2ull * dst + 1ull) * src) / (2ull * size));
}

// overlap histogram of a prediction: bins 0 .. G - 1 the ground-truth instances, bin G void (a slot above G counts as void), bin G + 1 the vertex count
SF_EV_HD uint32_t overlap_bin(uint32_t slot, uint32_t G) { return slot < G ? slot : G; }

// ---- shared between evaluation.cpp and evaluation.hip ----
int check_valid(const int32_t* valid_ids, uint32_t n_valid, uint64_t* mask, uint32_t* dim, const char* who);
int check_images(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gw, uint32_t gh, uint32_t pw, uint32_t ph, uint32_t dim,
                 const uint64_t* confusion, const uint64_t* oor);
int check_overlaps(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* table);
int confusion_on_device(const void* gt, const void* pred, int elem_bytes, uint64_t n, uint64_t valid, uint32_t dim, int mode, int device, uint64_t* confusion,
                        uint64_t* out_of_range);
int confusion_images_on_device(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gw, uint32_t gh, uint32_t pw, uint32_t ph, uint32_t dw,
                               uint32_t dh, uint32_t dim, int device, uint64_t* confusion, uint64_t* out_of_range);
int overlaps_on_device(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, int device, uint32_t* table);

}  // namespace ev
}  // namespace sf
