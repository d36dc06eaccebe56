// instance2d.cpp -- the 2-D instance task's counting stages on the host (include/scanfuse.h "Benchmark scores, 2-D instances"):
// the entry points and their checks, the per-image plan (instances2dict.py:40-43 with instance.py:13-24) and the batched overlaps
// (evalInstanceLevelSemanticLabeling.py:226-230, :251-252, :266, :278) on at most 16 threads.  The rules are evaluation_internal.h's, the kernels of
// the same counts are evaluation.hip's, the AP over the tables is evaluation.cpp's.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "evaluation_internal.h"

namespace {

using sf::ev::ValidSet;

inline uint32_t load(const void* p, int elem_bytes, uint64_t i) {
  if (elem_bytes == 1) return ((const uint8_t*)p)[i];
  if (elem_bytes == 2) return ((const uint16_t*)p)[i];
  return ((const uint32_t*)p)[i];
}

struct Plan {   // of one image
  std::vector<int32_t> id;
  std::vector<uint32_t> pixels;
};

void host_plan(const void* gt, int elem_bytes, uint32_t batch, uint64_t n, const ValidSet& vs, std::vector<Plan>& plans) {
  const uint32_t range = sf::ev::id_range(vs);
  plans.resize(batch);
  sf::ev::parallel_for(batch, [&](uint64_t b) {
    std::vector<uint32_t> counter(range, 0u);   // ids at or above the range have no valid class
    for (uint64_t i = b * n; i < (b + 1) * n; i++) {
      const uint32_t v = load(gt, elem_bytes, i);
      if (v < range) counter[v]++;
    }
    for (uint32_t v = 0; v < range; v++)
      if (counter[v] && sf::ev::is_instance_2d(vs.bits, v)) {
        plans[b].id.push_back((int32_t)v);
        plans[b].pixels.push_back(counter[v]);
      }
  });
}

void host_overlaps(const void* gt, int elem_bytes, uint64_t n, const ValidSet& vs, uint32_t capacity, const uint32_t* count, const int32_t* instance_id,
                   const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* mask_image, uint32_t* table) {
  const size_t bins = (size_t)capacity + 2;
  sf::ev::parallel_for(P, [&](uint64_t p) {
    uint32_t* row = table + p * bins;
    std::memset(row, 0, bins * 4);
    const uint8_t* mask = masks + p * stride;
    const uint32_t b = mask_image[p], G = count[b];
    const int32_t* ids = instance_id + (size_t)b * capacity;
    for (uint64_t i = 0; i < n; i++) {
      if (!mask[i]) continue;
      row[capacity + 1]++;
      const uint32_t v = load(gt, elem_bytes, (uint64_t)b * n + i);
      if (sf::ev::is_void_2d(vs.bits, v)) { row[capacity]++; continue; }
      if (v > 0x7FFFFFFFu) continue;
      const int32_t* at = std::lower_bound(ids, ids + G, (int32_t)v);
      if (at != ids + G && *at == (int32_t)v) row[at - ids]++;   // neither an instance nor void: the pixel count alone
    }
  });
}

}  // namespace

namespace sf {
namespace ev {

static int check_gt(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const char* who) {
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return sf::fail(SF_ERR_INVALID_ARG, "%s: pixels of %d bytes (1, 2 or 4)", who, elem_bytes);
  if (batch > MAX_BATCH_2D) return sf::fail(SF_ERR_INVALID_ARG, "%s: %u images in one call (up to %u)", who, batch, MAX_BATCH_2D);
  if (batch && !gt) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (batch && (width < 1 || height < 1)) return sf::fail(SF_ERR_INVALID_ARG, "%s: images of %u x %u", who, width, height);
  if ((uint64_t)width * height >= (1ull << 32)) return sf::fail(SF_ERR_INVALID_ARG, "%s: images of %u x %u (below 2^32 pixels: the counters are 32-bit)", who, width, height);
  if ((uintptr_t)gt & (uintptr_t)(elem_bytes - 1)) return sf::fail(SF_ERR_INVALID_ARG, "%s: images that are not aligned to their %d-byte pixels", who, elem_bytes);
  return SF_OK;
}

int check_image_plan(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, uint32_t capacity, const uint32_t* count,
                     const int32_t* instance_id, const uint32_t* instance_pixels, const char* who) {
  if (int rc = check_gt(gt, elem_bytes, batch, width, height, who)) return rc;
  if (batch && !count) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if ((instance_id == nullptr) != (instance_pixels == nullptr)) return sf::fail(SF_ERR_INVALID_ARG, "%s: the ids and the pixel counts are given together or not at all", who);
  if (capacity > MAX_CAPACITY_2D) return sf::fail(SF_ERR_INVALID_ARG, "%s: a capacity of %u (up to 2^20)", who, capacity);
  return SF_OK;
}

int check_overlaps_images(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, uint32_t capacity, const uint32_t* count,
                          const int32_t* instance_id, const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* mask_image, const uint32_t* table,
                          const char* who) {
  if (int rc = check_gt(gt, elem_bytes, batch, width, height, who)) return rc;
  if (P > 65535u) return sf::fail(SF_ERR_INVALID_ARG, "%s: %u masks in one call (up to 65535)", who, P);
  if (capacity > MAX_CAPACITY_2D) return sf::fail(SF_ERR_INVALID_ARG, "%s: a capacity of %u (up to 2^20)", who, capacity);
  if (P && (!masks || !mask_image || !table || !count || (capacity && !instance_id))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (P && batch == 0) return sf::fail(SF_ERR_INVALID_ARG, "%s: %u masks over no image", who, P);
  if (P && stride < (uint64_t)width * height) return sf::fail(SF_ERR_INVALID_ARG, "%s: a mask stride of %llu for images of %u x %u", who, (unsigned long long)stride, width, height);
  return SF_OK;
}

}  // namespace ev
}  // namespace sf

SF_API uint64_t sf_eval_image_plan_scratch(uint32_t batch, const int32_t* valid_ids, uint32_t n_valid) {
  ValidSet vs;
  if (batch > sf::ev::MAX_BATCH_2D || sf::ev::check_valid_2d(valid_ids, n_valid, &vs, "sf_eval_image_plan_scratch")) return 0;
  return (uint64_t)batch * sf::ev::id_range(vs) * 4u;
}

SF_API int sf_eval_image_plan(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids, uint32_t n_valid,
                              uint32_t capacity, int device, uint32_t* count, int32_t* instance_id, uint32_t* instance_pixels) {
  ValidSet vs;
  if (int rc = sf::ev::check_valid_2d(valid_ids, n_valid, &vs, "sf_eval_image_plan")) return rc;
  if (int rc = sf::ev::check_image_plan(gt, elem_bytes, batch, width, height, capacity, count, instance_id, instance_pixels, "sf_eval_image_plan")) return rc;
  if (batch == 0) return SF_OK;
  const uint64_t n = (uint64_t)width * height;
  if (device >= 0) return sf::ev::image_plan_on_device(gt, elem_bytes, batch, (uint32_t)n, vs, capacity, device, count, instance_id, instance_pixels);
  std::vector<Plan> plans;
  host_plan(gt, elem_bytes, batch, n, vs, plans);
  if (instance_id)
    for (uint32_t b = 0; b < batch; b++)
      if (plans[b].id.size() > capacity)   // before anything is written
        return sf::fail(SF_ERR_BOUNDS, "sf_eval_image_plan: image %u holds %zu instances, capacity %u", b, plans[b].id.size(), capacity);
  for (uint32_t b = 0; b < batch; b++) {
    const size_t G = plans[b].id.size();
    count[b] = (uint32_t)G;
    if (instance_id && G) {
      std::memcpy(instance_id + (size_t)b * capacity, plans[b].id.data(), G * 4);
      std::memcpy(instance_pixels + (size_t)b * capacity, plans[b].pixels.data(), G * 4);
    }
  }
  return SF_OK;
}

SF_API int sf_eval_overlaps_images(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids, uint32_t n_valid,
                                   uint32_t capacity, const uint32_t* count, const int32_t* instance_id, const uint8_t* masks, uint32_t P, uint64_t stride,
                                   const uint32_t* mask_image, int device, uint32_t* table) {
  ValidSet vs;
  const char* who = "sf_eval_overlaps_images";
  if (int rc = sf::ev::check_valid_2d(valid_ids, n_valid, &vs, who)) return rc;
  if (int rc = sf::ev::check_overlaps_images(gt, elem_bytes, batch, width, height, capacity, count, instance_id, masks, P, stride, mask_image, table, who)) return rc;
  if (P == 0) return SF_OK;
  for (uint32_t b = 0; b < batch; b++) {
    if (count[b] > capacity) return sf::fail(SF_ERR_INVALID_ARG, "%s: image %u has %u instances, capacity %u", who, b, count[b], capacity);
    const int32_t* ids = instance_id + (size_t)b * capacity;
    for (uint32_t g = 0; g < count[b]; g++)
      if (ids[g] < 0 || (g && ids[g] <= ids[g - 1])) return sf::fail(SF_ERR_INVALID_ARG, "%s: the instance ids of image %u do not ascend at %u", who, b, g);
  }
  for (uint32_t p = 0; p < P; p++)
    if (mask_image[p] >= batch) return sf::fail(SF_ERR_INVALID_ARG, "%s: mask %u lies over image %u of %u", who, p, mask_image[p], batch);
  const uint64_t n = (uint64_t)width * height;
  if (device >= 0)
    return sf::ev::overlaps_images_on_device(gt, elem_bytes, batch, (uint32_t)n, vs, capacity, count, instance_id, masks, P, stride, mask_image, device, table);
  host_overlaps(gt, elem_bytes, n, vs, capacity, count, instance_id, masks, P, stride, mask_image, table);
  return SF_OK;
}
