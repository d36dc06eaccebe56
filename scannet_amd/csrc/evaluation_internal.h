// evaluation_internal.h -- the rules of the benchmark scores (include/scanfuse.h "Benchmark scores"), written once for the host
// path (evaluation.cpp) and the kernels (evaluation.hip): which cell of the confusion matrix an element counts in, the source pixel of the nearest-neighbour
// resize, and the bin of a vertex in a prediction's overlap histogram.  Everything here is integer arithmetic, so every schedule gives the same counts.
#pragma once
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#if defined(__HIPCC__)
#define SF_EV_HD __host__ __device__ inline
#else
#define SF_EV_HD inline
#endif

namespace sf {
int usable_cpus();   // common.h

namespace ev {

// the host paths' loop: body(job) on at most 16 threads, jobs handed out one by one
template <typename F>
void parallel_for(uint64_t jobs, F&& body) {
  int n = sf::usable_cpus();
  if (n > 16) n = 16;
  if ((uint64_t)n > jobs) n = (int)jobs;
  if (n < 1) n = 1;
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

// ---- 2-D instances (include/scanfuse.h "Benchmark scores, 2-D instances") ----

// The valid classes of the 2-D instance task, ids 1 .. 999, as a bitmap: a kernel takes it by value and copies it into LDS.
struct ValidSet {
  uint32_t bits[32];
  uint32_t top;   // the largest valid id: the per-image counters cover ids below (top + 1) * 1000
};

SF_EV_HD bool in_set(const uint32_t* bits, uint32_t v) { return v < 1024u && ((bits[v >> 5] >> (v & 31u)) & 1u) != 0u; }
// a pixel is void where its raw value is a valid class id (evalInstanceLevelSemanticLabeling.py:226-230), and of an instance where value / 1000 is
// one (instances2dict.py:40-43); valid ids are below 1000, so no value is both
SF_EV_HD bool is_void_2d(const uint32_t* bits, uint32_t v) { return in_set(bits, v); }
SF_EV_HD bool is_instance_2d(const uint32_t* bits, uint32_t v) { return in_set(bits, v / 1000u); }
inline uint32_t id_range(const ValidSet& vs) { return (vs.top + 1u) * 1000u; }

constexpr uint32_t MAX_BATCH_2D = 65535, MAX_CAPACITY_2D = 1u << 20;

int check_valid_2d(const int32_t* valid_ids, uint32_t n_valid, ValidSet* vs, const char* who);
int check_image_plan(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, uint32_t capacity, const uint32_t* count,
                     const int32_t* instance_id, const uint32_t* instance_pixels, const char* who);
int check_overlaps_images(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, uint32_t capacity, const uint32_t* count,
                          const int32_t* instance_id, const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* mask_image, const uint32_t* table,
                          const char* who);
int image_plan_on_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t n, const ValidSet& vs, uint32_t capacity, int device, uint32_t* count,
                         int32_t* instance_id, uint32_t* instance_pixels);
int overlaps_images_on_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t n, const ValidSet& vs, uint32_t capacity, const uint32_t* count,
                              const int32_t* instance_id, const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* mask_image, int device,
                              uint32_t* table);

}  // namespace ev
}  // namespace sf
