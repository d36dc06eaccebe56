// evaluation.hip -- the device path of the benchmark's scores (include/scanfuse.h "Benchmark scores").  The rules are
// evaluation_internal.h's, the host path of the same counts is evaluation.cpp.
//
//   k_eval_confusion<T, MODE>    a flat run of (gt, pred) elements of 1, 2 or 4 bytes -> the confusion matrix.  Neighbouring vertices and pixels carry the
//                                same pair, so one atomic per element would queue on one address: a lane reads 16 bytes of each array per step, merges runs
//                                of equal keys in registers, and adds a run to its wave's private 32-bit matrix in LDS; a workgroup ends with one 64-bit
//                                global add per non-zero cell.
//   k_eval_confusion_images<T>   the 2-D mode on a batch of image pairs, with the nearest-neighbour resize fused: a lane walks a span of one destination
//                                row and reads both sources at the computed indices; the same registers, LDS matrices and flush.
//   k_eval_overlaps              a workgroup takes one prediction's mask and a span of vertices: the LDS histogram over the ground-truth instances, void
//                                and the vertex count; slots are read only where 16 mask bytes are not all zero.  More bins than the LDS holds: passes
//                                over bin ranges.
//   k_eval_image_ids<T>          section 4p, the plan of a batch of id images: a workgroup takes a span of one image, merges runs of equal ids in
//                                registers and counts them in an LDS table of (id, count): one global add per distinct id it met.
//   k_eval_image_compact         a workgroup per image: the non-zero counters of valid classes as ascending ids and pixel counts (a prefix sum).
//   k_eval_overlaps_images<T>    a workgroup takes one mask and a span of its image: ids are read where the mask is set, a run is void or an
//                                instance found in the image's sorted id list in LDS; the LDS histogram ends in one global add per non-zero bin.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "common.h"
#include "evaluation_internal.h"
#include "hip_util.h"

namespace {

using sf::ev::KEY_SKIP;
using sf::ev::MODE_2D;
using sf::ev::MODE_3D;
using sf::DeviceScope;
using sf::same_device;

constexpr uint32_t THREADS = 256, WAVES = THREADS / 64;
constexpr uint32_t MAX_BLOCKS = 2048;
// A workgroup's LDS counters are 32-bit.  A call holds at most MAX_ELEMENTS elements and, from MAX_BLOCKS vectors on, is spread over MAX_BLOCKS workgroups
// to within one 16-byte vector each, so a workgroup counts fewer than 2^32 elements and no counter wraps.
static_assert(sf::ev::MAX_ELEMENTS / MAX_BLOCKS + 16u * THREADS < (1ull << 32), "a workgroup's 32-bit counters could wrap");

extern __shared__ __attribute__((aligned(16))) uint32_t s_cells[];   // WAVES private copies of dim * dim + 1 counters

struct Run {   // a lane's current run of equal keys
  uint32_t key = KEY_SKIP, count = 0;
};

__device__ inline void run_add(Run& r, uint32_t key, uint32_t* mine) {
  if (key == r.key) {
    r.count++;
    return;
  }
  if (r.key != KEY_SKIP) atomicAdd(&mine[r.key], r.count);
  r.key = key;
  r.count = 1;
}

__device__ inline void run_end(Run& r, uint32_t* mine) {
  if (r.key != KEY_SKIP && r.count) atomicAdd(&mine[r.key], r.count);
}

__device__ inline void cells_clear(uint32_t cells) {
  for (uint32_t i = threadIdx.x; i < WAVES * cells; i += THREADS) s_cells[i] = 0u;
  __syncthreads();
}

// one 64-bit global add per non-zero cell; the last cell is the out-of-range count
__device__ inline void cells_flush(uint32_t cells, unsigned long long* __restrict__ confusion, unsigned long long* __restrict__ out_of_range) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < cells; i += THREADS) {
    uint32_t sum = 0u;   // below 2^32: the static_assert above
    for (uint32_t w = 0; w < WAVES; w++) sum += s_cells[w * cells + i];
    if (!sum) continue;
    if (i + 1u < cells) atomicAdd(&confusion[i], (unsigned long long)sum);
    else if (out_of_range) atomicAdd(out_of_range, (unsigned long long)sum);
  }
}

template <typename T>
union Vec16 {
  uint4 v;
  T e[16 / sizeof(T)];
};

// gt + head is 16-byte aligned; vectors [0, nvec) start there.  pred_vec: pred + head is 16-byte aligned too.  Elements [0, head) and [head + nvec * E, n)
// are the first workgroup's, one element per lane.
template <typename T, uint32_t MODE>
__global__ __launch_bounds__(THREADS) void k_eval_confusion(const T* __restrict__ gt, const T* __restrict__ pred, uint64_t n, uint32_t head, uint64_t nvec,
                                                            int pred_vec, uint64_t valid, uint32_t dim, unsigned long long* __restrict__ confusion,
                                                            unsigned long long* __restrict__ out_of_range) {
  constexpr uint32_t E = 16 / sizeof(T);
  const uint32_t cells = dim * dim + 1u;
  uint32_t* mine = s_cells + (threadIdx.x >> 6) * cells;
  cells_clear(cells);
  Run run;
  // this workgroup's vectors: [first, last), an even split
  const uint64_t per = nvec / gridDim.x, extra = nvec % gridDim.x;
  const uint64_t first = blockIdx.x * per + (blockIdx.x < extra ? blockIdx.x : extra);
  const uint64_t last = first + per + (blockIdx.x < extra ? 1u : 0u);
  for (uint64_t v = first + threadIdx.x; v < last; v += THREADS) {
    const uint64_t at = head + v * E;   // at + E <= n
    Vec16<T> g, p;
    g.v = *reinterpret_cast<const uint4*>(gt + at);
    if (pred_vec) {
      p.v = *reinterpret_cast<const uint4*>(pred + at);
    } else {
#pragma unroll
      for (uint32_t j = 0; j < E; j++) p.e[j] = pred[at + j];
    }
#pragma unroll
    for (uint32_t j = 0; j < E; j++) run_add(run, sf::ev::key_of<MODE>((uint32_t)g.e[j], (uint32_t)p.e[j], valid, dim), mine);
  }
  run_end(run, mine);
  if (blockIdx.x == 0) {
    const uint64_t tail = head + nvec * E;   // <= n; n - tail < E
    for (uint64_t i = threadIdx.x; i < head; i += THREADS) {
      const uint32_t k = sf::ev::key_of<MODE>((uint32_t)gt[i], (uint32_t)pred[i], valid, dim);
      if (k != KEY_SKIP) atomicAdd(&mine[k], 1u);
    }
    for (uint64_t i = tail + threadIdx.x; i < n; i += THREADS) {
      const uint32_t k = sf::ev::key_of<MODE>((uint32_t)gt[i], (uint32_t)pred[i], valid, dim);
      if (k != KEY_SKIP) atomicAdd(&mine[k], 1u);
    }
  }
  cells_flush(cells, confusion, out_of_range);
}

// rows = batch * dh destination rows, grid-strided; a lane's span of a row is `span` pixels wide (span * THREADS >= dw)
template <typename T>
__global__ __launch_bounds__(THREADS) void k_eval_confusion_images(const T* __restrict__ gt, const T* __restrict__ pred, uint32_t rows, uint32_t gw, uint32_t gh,
                                                                   uint32_t pw, uint32_t ph, uint32_t dw, uint32_t dh, uint32_t span, uint32_t dim,
                                                                   unsigned long long* __restrict__ confusion,
                                                                   unsigned long long* __restrict__ out_of_range) {
  const uint32_t cells = dim * dim + 1u;
  uint32_t* mine = s_cells + (threadIdx.x >> 6) * cells;
  cells_clear(cells);
  Run run;
  const uint32_t x0 = threadIdx.x * span, x1 = min(x0 + span, dw);
  for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const uint32_t b = r / dh, y = r - b * dh;
    const T* grow = gt + ((uint64_t)b * gh + sf::ev::nn_source(y, gh, dh)) * gw;     // inside image b: nn_source(y, gh, dh) < gh
    const T* prow = pred + ((uint64_t)b * ph + sf::ev::nn_source(y, ph, dh)) * pw;
    for (uint32_t x = x0; x < x1; x++)
      run_add(run, sf::ev::key_2d((uint32_t)grow[sf::ev::nn_source(x, gw, dw)], (uint32_t)prow[sf::ev::nn_source(x, pw, dw)], dim), mine);
  }
  run_end(run, mine);
  cells_flush(cells, confusion, out_of_range);
}

constexpr uint32_t OV_BINS = 4096;    // 16 KiB of LDS
constexpr uint32_t OV_SPAN = 1u << 15;   // vertices of one workgroup: 8 steps of 256 lanes x 16

struct alignas(4) Slots4 {   // four slots at a 4-byte aligned address
  uint32_t s[4];
};

__device__ inline void bin_add(Run& r, uint32_t bin, uint32_t lo, uint32_t nb, uint32_t* hist) {
  const uint32_t b = bin - lo;   // wraps above nb below lo
  if (b < nb) run_add(r, b, hist);
}

// blockIdx.y: the prediction; blockIdx.x: the span of vertices.  table[P][G + 2] was zeroed.  Bins [lo, lo + nb) per pass; bin G + 1 is the vertex count.
__global__ __launch_bounds__(THREADS) void k_eval_overlaps(const uint32_t* __restrict__ slot, uint32_t n, uint32_t G, const uint8_t* __restrict__ masks,
                                                           uint64_t stride, uint32_t* __restrict__ table) {
  __shared__ uint32_t s_hist[OV_BINS];
  const uint32_t bins = G + 2u;
  const uint8_t* mask = masks + (uint64_t)blockIdx.y * stride;
  uint32_t* row = table + (uint64_t)blockIdx.y * bins;
  const uint32_t begin = blockIdx.x * OV_SPAN;   // below n: the grid has ceil(n / OV_SPAN) spans
  const uint32_t end = (uint32_t)min((uint64_t)n, (uint64_t)begin + OV_SPAN);
  // 16-byte steps start where the mask row is aligned
  const uint32_t mis = (uint32_t)((16u - ((uintptr_t)(mask + begin) & 15u)) & 15u);
  const uint32_t vbegin = (uint32_t)min((uint64_t)begin + mis, (uint64_t)end);
  const uint32_t nvec = (end - vbegin) / 16u;
  const uint32_t vend = vbegin + nvec * 16u;   // <= end; fewer than 16 elements on either side of the vector part
  for (uint32_t lo = 0; lo < bins; lo += OV_BINS) {
    const uint32_t nb = min(OV_BINS, bins - lo);
    for (uint32_t i = threadIdx.x; i < nb; i += THREADS) s_hist[i] = 0u;
    __syncthreads();
    Run run;
    uint32_t covered = 0u;
    for (uint32_t v = threadIdx.x; v < nvec; v += THREADS) {
      const uint32_t at = vbegin + v * 16u;
      Vec16<uint8_t> m;
      m.v = *reinterpret_cast<const uint4*>(mask + at);
      if (!(m.v.x | m.v.y | m.v.z | m.v.w)) continue;
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const Slots4 s = *reinterpret_cast<const Slots4*>(slot + at + 4u * q);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
          if (m.e[4u * q + j]) {
            covered++;
            bin_add(run, sf::ev::overlap_bin(s.s[j], G), lo, nb, s_hist);
          }
      }
    }
    // the unaligned head and the tail of the span, an element per lane
    const uint32_t side = threadIdx.x < 16u ? begin + threadIdx.x : vend + (threadIdx.x - 16u);
    const bool in_side = threadIdx.x < 16u ? side < vbegin : (threadIdx.x < 32u && side < end);
    if (in_side && mask[side]) {
      covered++;
      bin_add(run, sf::ev::overlap_bin(slot[side], G), lo, nb, s_hist);
    }
    run_end(run, s_hist);
    if (covered && G + 1u - lo < nb) atomicAdd(&s_hist[G + 1u - lo], covered);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += THREADS)
      if (s_hist[i]) atomicAdd(&row[lo + i], s_hist[i]);
    __syncthreads();
  }
}

// ---- 2-D instances ----

constexpr uint32_t ID_TABLE = 1024;           // entries of a workgroup's open-addressed (id, count) table: 8 KiB of LDS
constexpr uint32_t ID_PROBES = 32;            // an id that finds neither itself nor a free entry in so many steps is counted by the range passes
constexpr uint32_t ID_DIRECT = 2048;          // bins of a range pass: 8 KiB of LDS
constexpr uint32_t ID_EMPTY = 0xFFFFFFFFu;    // no id: the counters cover ids below 1 000 000
constexpr uint32_t OI_LIST = 2048;            // instance ids of one pass of k_eval_overlaps_images: 8 KiB of LDS, and as many bins + 2

using sf::ev::ValidSet;

// the valid-class bitmap arrives by value; constant indices only, so that it is read from the kernel's arguments and never spilled
__device__ inline void valid_to_lds(const ValidSet& vs, uint32_t* s_valid) {
#pragma unroll
  for (uint32_t i = 0; i < 32; i++)
    if (threadIdx.x == i) s_valid[i] = vs.bits[i];
}

template <typename F>
__device__ inline void run_step(Run& r, uint32_t key, F&& flush) {   // run_add with the flush left to the caller
  if (key == r.key) {
    r.count++;
    return;
  }
  if (r.key != KEY_SKIP) flush(r.key, r.count);
  r.key = key;
  r.count = 1;
}

// The elements [begin, end) of p, each handed to f once: 16 bytes per lane and step from where p is aligned, and the fewer than 16 / sizeof(T)
// elements on either side one per lane.
template <typename T, typename F>
__device__ inline void span_values(const T* __restrict__ p, uint32_t begin, uint32_t end, F&& f) {
  constexpr uint32_t E = 16 / sizeof(T);
  const uint32_t mis = (uint32_t)(((16u - ((uintptr_t)(p + begin) & 15u)) & 15u) / sizeof(T));   // p is aligned to T
  const uint32_t vbegin = (uint32_t)min((uint64_t)begin + mis, (uint64_t)end);
  const uint32_t nvec = (end - vbegin) / E;
  const uint32_t vend = vbegin + nvec * E;
  for (uint32_t v = threadIdx.x; v < nvec; v += THREADS) {
    Vec16<T> g;
    g.v = *reinterpret_cast<const uint4*>(p + vbegin + v * E);
#pragma unroll
    for (uint32_t j = 0; j < E; j++) f((uint32_t)g.e[j]);
  }
  const uint32_t side = threadIdx.x < 16u ? begin + threadIdx.x : vend + (threadIdx.x - 16u);
  const bool in_side = threadIdx.x < 16u ? side < vbegin : (threadIdx.x < 32u && side < end);
  if (in_side) f((uint32_t)p[side]);
}

// -> false: the id has no place in the table (and then never gets one: entries are not freed, so a later probe meets the same occupants)
__device__ inline bool table_add(uint32_t* keys, uint32_t* counts, uint32_t id, uint32_t n) {
  uint32_t h = (id * 2654435761u) >> 22;   // 10 bits
  for (uint32_t i = 0; i < ID_PROBES; i++) {
    uint32_t k = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
    if (k == ID_EMPTY) k = atomicCAS(&keys[h], ID_EMPTY, id);
    if (k == ID_EMPTY || k == id) {
      atomicAdd(&counts[h], n);
      return true;
    }
    h = (h + 1u) & (ID_TABLE - 1u);
  }
  return false;
}

__device__ inline bool table_has(const uint32_t* keys, uint32_t id) {
  uint32_t h = (id * 2654435761u) >> 22;
  for (uint32_t i = 0; i < ID_PROBES; i++) {
    const uint32_t k = keys[h];
    if (k == id) return true;
    if (k == ID_EMPTY) return false;
    h = (h + 1u) & (ID_TABLE - 1u);
  }
  return false;
}

// blockIdx.y: the image; blockIdx.x: its span of OV_SPAN pixels.  counters[batch][range] were zeroed.  A workgroup adds each distinct id it met to the
// image's counters once: runs of equal ids are merged in registers and go to the LDS table, which is flushed at the end; the ids the table could not
// hold are counted by passes over id ranges [lo, lo + ID_DIRECT) into direct bins, a pass per range between the smallest and the largest such id.
template <typename T>
__global__ __launch_bounds__(THREADS) void k_eval_image_ids(const T* __restrict__ gt, uint32_t n, uint32_t range, uint32_t* __restrict__ counters) {
  __shared__ uint32_t s_keys[ID_TABLE], s_counts[ID_TABLE], s_direct[ID_DIRECT];
  __shared__ uint32_t s_left[2];   // the smallest and the largest id without a place in the table
  const T* img = gt + (uint64_t)blockIdx.y * n;
  uint32_t* out = counters + (uint64_t)blockIdx.y * range;
  const uint32_t begin = blockIdx.x * OV_SPAN;   // below n: the grid has ceil(n / OV_SPAN) spans
  const uint32_t end = (uint32_t)min((uint64_t)n, (uint64_t)begin + OV_SPAN);
  for (uint32_t i = threadIdx.x; i < ID_TABLE; i += THREADS) {
    s_keys[i] = ID_EMPTY;
    s_counts[i] = 0u;
  }
  if (threadIdx.x == 0) {
    s_left[0] = ID_EMPTY;
    s_left[1] = 0u;
  }
  __syncthreads();
  {
    Run run;
    auto flush = [&](uint32_t id, uint32_t count) {
      if (table_add(s_keys, s_counts, id, count)) return;
      atomicMin(&s_left[0], id);
      atomicMax(&s_left[1], id);
    };
    span_values(img, begin, end, [&](uint32_t v) { run_step(run, v < range ? v : KEY_SKIP, flush); });   // ids at or above the range: no valid class
    if (run.key != KEY_SKIP) flush(run.key, run.count);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < ID_TABLE; i += THREADS)
    if (s_keys[i] != ID_EMPTY && s_counts[i]) atomicAdd(&out[s_keys[i]], s_counts[i]);
  const uint32_t left_lo = s_left[0], left_hi = s_left[1];
  if (left_lo == ID_EMPTY) return;   // the whole workgroup
  for (uint32_t lo = left_lo; lo <= left_hi; lo += ID_DIRECT) {   // left_hi < range <= 10^6: lo does not wrap
    for (uint32_t i = threadIdx.x; i < ID_DIRECT; i += THREADS) s_direct[i] = 0u;
    __syncthreads();
    Run run;
    auto flush = [&](uint32_t bin, uint32_t count) { atomicAdd(&s_direct[bin], count); };
    span_values(img, begin, end, [&](uint32_t v) {
      const uint32_t bin = v - lo;   // wraps above ID_DIRECT below lo
      run_step(run, (v < range && bin < ID_DIRECT && !table_has(s_keys, v)) ? bin : KEY_SKIP, flush);
    });
    if (run.key != KEY_SKIP) flush(run.key, run.count);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ID_DIRECT; i += THREADS)
      if (s_direct[i]) atomicAdd(&out[lo + i], s_direct[i]);   // lo + i < range: only ids below the range were counted
    __syncthreads();
  }
}

// blockIdx.x: the image.  Its non-zero counters whose class is valid, in ascending id: four counters per lane and step (they share a class: 1000 is a
// multiple of 4), an inclusive scan over the wave and the waves' totals through LDS.  count[b] is the number found; the first `capacity` are written.
__global__ __launch_bounds__(THREADS) void k_eval_image_compact(const uint32_t* __restrict__ counters, uint32_t range, const ValidSet vs, uint32_t capacity,
                                                                uint32_t* __restrict__ count, int32_t* __restrict__ ids, uint32_t* __restrict__ pixels) {
  __shared__ uint32_t s_valid[32], s_wave[WAVES];
  valid_to_lds(vs, s_valid);
  __syncthreads();
  const uint32_t* in = counters + (uint64_t)blockIdx.x * range;
  int32_t* out_id = ids + (uint64_t)blockIdx.x * capacity;
  uint32_t* out_px = pixels + (uint64_t)blockIdx.x * capacity;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t base = 0u;
  for (uint32_t chunk = 0; chunk < range; chunk += THREADS * 4u) {
    const uint32_t i0 = chunk + threadIdx.x * 4u;   // range is a multiple of 4: i0 < range means i0 + 3 < range
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (i0 < range && sf::ev::in_set(s_valid, i0 / 1000u)) c = *reinterpret_cast<const uint4*>(in + i0);
    const uint32_t mine = (c.x != 0u) + (c.y != 0u) + (c.z != 0u) + (c.w != 0u);
    uint32_t x = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63u) s_wave[wave] = x;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) {
      const uint32_t t = s_wave[w];
      if (w < wave) before += t;
      total += t;
    }
    uint32_t at = base + before + x - mine;
    if (c.x) { if (at < capacity) { out_id[at] = (int32_t)i0; out_px[at] = c.x; } at++; }
    if (c.y) { if (at < capacity) { out_id[at] = (int32_t)(i0 + 1u); out_px[at] = c.y; } at++; }
    if (c.z) { if (at < capacity) { out_id[at] = (int32_t)(i0 + 2u); out_px[at] = c.z; } at++; }
    if (c.w) { if (at < capacity) { out_id[at] = (int32_t)(i0 + 3u); out_px[at] = c.w; } at++; }
    base += total;
    __syncthreads();   // s_wave is written again
  }
  if (threadIdx.x == 0) count[blockIdx.x] = base;
}

// blockIdx.y: the mask; blockIdx.x: the span of pixels.  table[P][capacity + 2] was zeroed.  The image's ascending ids [lo, lo + nb) are in LDS per
// pass; a run of equal covered values is void (the raw value is a valid class id), or an instance found by binary search, or neither.  Void and the
// pixel count are the first pass's.
template <typename T>
__global__ __launch_bounds__(THREADS) void k_eval_overlaps_images(const T* __restrict__ gt, uint32_t n, const ValidSet vs, uint32_t capacity, uint32_t batch,
                                                                  const uint32_t* __restrict__ count, const int32_t* __restrict__ ids,
                                                                  const uint8_t* __restrict__ masks, uint64_t stride, const uint32_t* __restrict__ mask_image,
                                                                  uint32_t* __restrict__ table) {
  __shared__ uint32_t s_valid[32], s_ids[OI_LIST], s_hist[OI_LIST + 2];
  const uint32_t b = mask_image[blockIdx.y];
  if (b >= batch) return;   // the whole workgroup: a mask without an image keeps its zero row
  const uint32_t G = min(count[b], capacity);
  const T* img = gt + (uint64_t)b * n;
  const int32_t* list = ids + (uint64_t)b * capacity;
  const uint8_t* mask = masks + (uint64_t)blockIdx.y * stride;
  uint32_t* row = table + (uint64_t)blockIdx.y * ((uint64_t)capacity + 2u);
  const uint32_t begin = blockIdx.x * OV_SPAN;   // below n
  const uint32_t end = (uint32_t)min((uint64_t)n, (uint64_t)begin + OV_SPAN);
  // 16-byte steps start where the mask row is aligned
  const uint32_t mis = (uint32_t)((16u - ((uintptr_t)(mask + begin) & 15u)) & 15u);
  const uint32_t vbegin = (uint32_t)min((uint64_t)begin + mis, (uint64_t)end);
  const uint32_t nvec = (end - vbegin) / 16u;
  const uint32_t vend = vbegin + nvec * 16u;
  valid_to_lds(vs, s_valid);
  for (uint32_t lo = 0; lo == 0u || lo < G; lo += OI_LIST) {
    const uint32_t nb = min(OI_LIST, G - lo);   // 0 where the image has no instance
    for (uint32_t i = threadIdx.x; i < nb; i += THREADS) s_ids[i] = (uint32_t)list[lo + i];
    for (uint32_t i = threadIdx.x; i < nb + 2u; i += THREADS) s_hist[i] = 0u;
    __syncthreads();
    Run run;
    uint32_t covered = 0u;
    auto flush = [&](uint32_t v, uint32_t c) {
      if (sf::ev::is_void_2d(s_valid, v)) {
        if (lo == 0u) atomicAdd(&s_hist[nb], c);
        return;
      }
      uint32_t a = 0u, z = nb;   // the first id >= v
      while (a < z) {
        const uint32_t m = (a + z) >> 1;
        if (s_ids[m] < v) a = m + 1u;
        else z = m;
      }
      if (a < nb && s_ids[a] == v) atomicAdd(&s_hist[a], c);
    };
    for (uint32_t v = threadIdx.x; v < nvec; v += THREADS) {
      const uint32_t at = vbegin + v * 16u;
      Vec16<uint8_t> m;
      m.v = *reinterpret_cast<const uint4*>(mask + at);
      if (!(m.v.x | m.v.y | m.v.z | m.v.w)) continue;
#pragma unroll
      for (uint32_t j = 0; j < 16; j++)
        if (m.e[j]) {
          covered++;
          run_step(run, (uint32_t)img[at + j], flush);
        }
    }
    // the unaligned head and the tail of the span, a pixel per lane
    const uint32_t side = threadIdx.x < 16u ? begin + threadIdx.x : vend + (threadIdx.x - 16u);
    const bool in_side = threadIdx.x < 16u ? side < vbegin : (threadIdx.x < 32u && side < end);
    if (in_side && mask[side]) {
      covered++;
      run_step(run, (uint32_t)img[side], flush);
    }
    if (run.key != KEY_SKIP) flush(run.key, run.count);   // a value of 2^32 - 1 is neither an instance nor void
    if (lo == 0u && covered) atomicAdd(&s_hist[nb + 1u], covered);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += THREADS)
      if (s_hist[i]) atomicAdd(&row[lo + i], s_hist[i]);
    if (lo == 0u && threadIdx.x < 2u && s_hist[nb + threadIdx.x]) atomicAdd(&row[capacity + threadIdx.x], s_hist[nb + threadIdx.x]);
    __syncthreads();
  }
}

template <typename T>
int launch_confusion_t(const T* gt, const T* pred, uint64_t n, uint64_t valid, uint32_t dim, int mode, hipStream_t s, unsigned long long* confusion,
                       unsigned long long* oor) {
  constexpr uint32_t E = 16 / sizeof(T);
  uint64_t head = ((16u - ((uintptr_t)gt & 15u)) & 15u) / sizeof(T);   // gt is aligned to its element: checked by the caller
  if (head > n) head = n;
  const uint64_t nvec = (n - head) / E;
  const int pred_vec = (((uintptr_t)(pred + head)) & 15u) == 0;
  const uint64_t want = (nvec + THREADS - 1) / THREADS;
  const uint32_t blocks = (uint32_t)(want < 1 ? 1 : (want > MAX_BLOCKS ? MAX_BLOCKS : want));
  const size_t lds = (size_t)WAVES * ((size_t)dim * dim + 1) * 4;   // at most 4 x (63 x 63 + 1) x 4 = 63 520 bytes at MAX_DIM = 63, under the 64 KiB a launch may ask for; dim 64 would not fit
  if (mode == (int)MODE_3D)
    k_eval_confusion<T, MODE_3D><<<blocks, THREADS, lds, s>>>(gt, pred, n, (uint32_t)head, nvec, pred_vec, valid, dim, confusion, oor);
  else
    k_eval_confusion<T, MODE_2D><<<blocks, THREADS, lds, s>>>(gt, pred, n, (uint32_t)head, nvec, pred_vec, valid, dim, confusion, oor);
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}

int launch_confusion(const void* gt, const void* pred, int elem_bytes, uint64_t n, uint64_t valid, uint32_t dim, int mode, hipStream_t s,
                     unsigned long long* confusion, unsigned long long* oor) {
  if (n == 0) return SF_OK;
  if (((uintptr_t)gt | (uintptr_t)pred) & (uintptr_t)(elem_bytes - 1)) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion: an array that is not aligned to its %d-byte elements", elem_bytes);
  if (elem_bytes == 1) return launch_confusion_t((const uint8_t*)gt, (const uint8_t*)pred, n, valid, dim, mode, s, confusion, oor);
  if (elem_bytes == 2) return launch_confusion_t((const uint16_t*)gt, (const uint16_t*)pred, n, valid, dim, mode, s, confusion, oor);
  return launch_confusion_t((const uint32_t*)gt, (const uint32_t*)pred, n, valid, dim, mode, s, confusion, oor);
}

template <typename T>
int launch_images_t(const T* gt, const T* pred, uint32_t batch, uint32_t gw, uint32_t gh, uint32_t pw, uint32_t ph, uint32_t dw, uint32_t dh, uint32_t dim,
                    hipStream_t s, unsigned long long* confusion, unsigned long long* oor) {
  const uint32_t rows = batch * dh;   // batch <= 2^20, dh = 480
  const uint32_t span = (dw + THREADS - 1) / THREADS;
  const uint32_t blocks = rows < MAX_BLOCKS ? rows : MAX_BLOCKS;   // a workgroup counts at most (rows / blocks + 1) * dw < 2^32 pixels
  const size_t lds = (size_t)WAVES * ((size_t)dim * dim + 1) * 4;
  k_eval_confusion_images<T><<<blocks, THREADS, lds, s>>>(gt, pred, rows, gw, gh, pw, ph, dw, dh, span, dim, confusion, oor);
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}

int launch_images(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gw, uint32_t gh, uint32_t pw, uint32_t ph, uint32_t dw, uint32_t dh,
                  uint32_t dim, hipStream_t s, unsigned long long* confusion, unsigned long long* oor) {
  if (batch == 0) return SF_OK;
  if (((uintptr_t)gt | (uintptr_t)pred) & (uintptr_t)(elem_bytes - 1)) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_images: an array that is not aligned to its %d-byte elements", elem_bytes);
  if (elem_bytes == 1) return launch_images_t((const uint8_t*)gt, (const uint8_t*)pred, batch, gw, gh, pw, ph, dw, dh, dim, s, confusion, oor);
  if (elem_bytes == 2) return launch_images_t((const uint16_t*)gt, (const uint16_t*)pred, batch, gw, gh, pw, ph, dw, dh, dim, s, confusion, oor);
  return launch_images_t((const uint32_t*)gt, (const uint32_t*)pred, batch, gw, gh, pw, ph, dw, dh, dim, s, confusion, oor);
}

// table is zeroed, then counted into
int launch_overlaps(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, hipStream_t s, uint32_t* table) {
  if (P == 0) return SF_OK;
  if (n && ((uintptr_t)slot & 3u)) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_instance_overlaps: slots that are not aligned to 4 bytes");   // before anything is written
  SF_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)P * ((size_t)G + 2) * 4, s));
  if (n == 0) return SF_OK;   // the table of no vertices is all zero
  const uint32_t spans = (uint32_t)((n + OV_SPAN - 1) / OV_SPAN);   // n < 2^32: at most 2^17 spans
  k_eval_overlaps<<<dim3(spans, P), THREADS, 0, s>>>(slot, (uint32_t)n, G, masks, stride, table);
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}

// counters are zeroed, counted into and compacted: three steps on one stream
template <typename T>
void launch_image_ids_t(const T* gt, uint32_t batch, uint32_t n, uint32_t range, hipStream_t s, uint32_t* counters) {
  const uint32_t spans = (uint32_t)(((uint64_t)n + OV_SPAN - 1) / OV_SPAN);
  k_eval_image_ids<T><<<dim3(spans, batch), THREADS, 0, s>>>(gt, n, range, counters);
}

int launch_image_plan(const void* gt, int elem_bytes, uint32_t batch, uint32_t n, const ValidSet& vs, uint32_t capacity, hipStream_t s, uint32_t* counters,
                      uint32_t* count, int32_t* ids, uint32_t* pixels) {
  if (batch == 0) return SF_OK;
  const uint32_t range = sf::ev::id_range(vs);
  if ((uintptr_t)counters & 15u) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_image_plan: a counter array that is not aligned to 16 bytes");   // before anything is written
  if (((uintptr_t)count | (uintptr_t)ids | (uintptr_t)pixels) & 3u) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_image_plan: results that are not aligned to 4 bytes");
  SF_HIP_CHECK(hipMemsetAsync(counters, 0, (size_t)batch * range * 4, s));
  if (elem_bytes == 1) launch_image_ids_t((const uint8_t*)gt, batch, n, range, s, counters);
  else if (elem_bytes == 2) launch_image_ids_t((const uint16_t*)gt, batch, n, range, s, counters);
  else launch_image_ids_t((const uint32_t*)gt, batch, n, range, s, counters);
  SF_HIP_CHECK(hipGetLastError());
  k_eval_image_compact<<<batch, THREADS, 0, s>>>(counters, range, vs, ids ? capacity : 0u, count, ids, pixels);
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}

// table is zeroed, then counted into
int launch_overlaps_images(const void* gt, int elem_bytes, uint32_t batch, uint32_t n, const ValidSet& vs, uint32_t capacity, const uint32_t* count,
                           const int32_t* ids, const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* mask_image, hipStream_t s, uint32_t* table) {
  if (P == 0) return SF_OK;
  if (((uintptr_t)count | (uintptr_t)ids | (uintptr_t)mask_image | (uintptr_t)table) & 3u)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_overlaps_images: an array that is not aligned to 4 bytes");   // before anything is written
  SF_HIP_CHECK(hipMemsetAsync(table, 0, (size_t)P * ((size_t)capacity + 2) * 4, s));
  const dim3 grid((uint32_t)(((uint64_t)n + OV_SPAN - 1) / OV_SPAN), P);
  if (elem_bytes == 1) k_eval_overlaps_images<uint8_t><<<grid, THREADS, 0, s>>>((const uint8_t*)gt, n, vs, capacity, batch, count, ids, masks, stride, mask_image, table);
  else if (elem_bytes == 2) k_eval_overlaps_images<uint16_t><<<grid, THREADS, 0, s>>>((const uint16_t*)gt, n, vs, capacity, batch, count, ids, masks, stride, mask_image, table);
  else k_eval_overlaps_images<uint32_t><<<grid, THREADS, 0, s>>>((const uint32_t*)gt, n, vs, capacity, batch, count, ids, masks, stride, mask_image, table);
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}

}  // namespace

namespace sf {
namespace ev {

// host arrays in, host counters out (added to): copy up, count, read back
int confusion_on_device(const void* gt, const void* pred, int elem_bytes, uint64_t n, uint64_t valid, uint32_t dim, int mode, int device, uint64_t* confusion,
                        uint64_t* out_of_range) {
  if (int rc = open_device(device, SF_ERR_DEVICE, "%s on a device needs an MI355X (device = -1 is the host path)", "sf_eval_confusion")) return rc;
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  const size_t cells = (size_t)dim * dim + 1, bytes = (size_t)n * elem_bytes;
  DevBuf d_gt, d_pred, d_cells;
  SF_HIP_CHECK(d_gt.alloc(bytes));
  SF_HIP_CHECK(d_pred.alloc(bytes));
  SF_HIP_CHECK(d_cells.alloc(cells * 8));
  if (bytes) {
    SF_HIP_CHECK(hipMemcpyAsync(d_gt.p, gt, bytes, hipMemcpyHostToDevice, sg.s));
    SF_HIP_CHECK(hipMemcpyAsync(d_pred.p, pred, bytes, hipMemcpyHostToDevice, sg.s));
  }
  SF_HIP_CHECK(hipMemsetAsync(d_cells.p, 0, cells * 8, sg.s));
  unsigned long long* c = d_cells.as<unsigned long long>();
  if (int rc = launch_confusion(d_gt.p, d_pred.p, elem_bytes, n, valid, dim, mode, sg.s, c, c + cells - 1)) return rc;
  std::vector<uint64_t> got(cells);
  SF_HIP_CHECK(hipMemcpyAsync(got.data(), d_cells.p, cells * 8, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  for (size_t i = 0; i + 1 < cells; i++) confusion[i] += got[i];
  if (out_of_range) *out_of_range += got[cells - 1];
  return SF_OK;
}

int confusion_images_on_device(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gw, uint32_t gh, uint32_t pw, uint32_t ph, uint32_t dw,
                               uint32_t dh, uint32_t dim, int device, uint64_t* confusion, uint64_t* out_of_range) {
  if (int rc = open_device(device, SF_ERR_DEVICE, "%s on a device needs an MI355X (device = -1 is the host path)", "sf_eval_confusion_images")) return rc;
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  const size_t cells = (size_t)dim * dim + 1;
  const size_t gbytes = (size_t)batch * gw * gh * elem_bytes, pbytes = (size_t)batch * pw * ph * elem_bytes;
  DevBuf d_gt, d_pred, d_cells;
  SF_HIP_CHECK(d_gt.alloc(gbytes));
  SF_HIP_CHECK(d_pred.alloc(pbytes));
  SF_HIP_CHECK(d_cells.alloc(cells * 8));
  if (gbytes) SF_HIP_CHECK(hipMemcpyAsync(d_gt.p, gt, gbytes, hipMemcpyHostToDevice, sg.s));
  if (pbytes) SF_HIP_CHECK(hipMemcpyAsync(d_pred.p, pred, pbytes, hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemsetAsync(d_cells.p, 0, cells * 8, sg.s));
  unsigned long long* c = d_cells.as<unsigned long long>();
  if (int rc = launch_images(d_gt.p, d_pred.p, elem_bytes, batch, gw, gh, pw, ph, dw, dh, dim, sg.s, c, c + cells - 1)) return rc;
  std::vector<uint64_t> got(cells);
  SF_HIP_CHECK(hipMemcpyAsync(got.data(), d_cells.p, cells * 8, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  for (size_t i = 0; i + 1 < cells; i++) confusion[i] += got[i];
  *out_of_range += got[cells - 1];
  return SF_OK;
}

int overlaps_on_device(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, int device, uint32_t* table) {
  if (int rc = open_device(device, SF_ERR_DEVICE, "%s on a device needs an MI355X (device = -1 is the host path)", "sf_eval_instance_overlaps")) return rc;
  if (P == 0) return SF_OK;
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  const size_t tbytes = (size_t)P * ((size_t)G + 2) * 4, mbytes = (size_t)(P - 1) * stride + n;
  DevBuf d_slot, d_masks, d_table;
  SF_HIP_CHECK(d_slot.alloc(n * 4));
  SF_HIP_CHECK(d_masks.alloc(mbytes));
  SF_HIP_CHECK(d_table.alloc(tbytes));
  if (n) {
    SF_HIP_CHECK(hipMemcpyAsync(d_slot.p, slot, n * 4, hipMemcpyHostToDevice, sg.s));
    SF_HIP_CHECK(hipMemcpyAsync(d_masks.p, masks, mbytes, hipMemcpyHostToDevice, sg.s));
  }
  if (int rc = launch_overlaps(d_slot.as<uint32_t>(), n, G, d_masks.as<uint8_t>(), P, stride, sg.s, d_table.as<uint32_t>())) return rc;
  SF_HIP_CHECK(hipMemcpyAsync(table, d_table.p, tbytes, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  return SF_OK;
}

// host images in, the host plan out: copy up, count, compact, read back; nothing is written when an image holds more than `capacity` instances
int image_plan_on_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t n, const ValidSet& vs, uint32_t capacity, int device, uint32_t* count,
                         int32_t* instance_id, uint32_t* instance_pixels) {
  if (int rc = open_device(device, SF_ERR_DEVICE, "%s on a device needs an MI355X (device = -1 is the host path)", "sf_eval_image_plan")) return rc;
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  const size_t bytes = (size_t)batch * n * elem_bytes, cells = instance_id ? (size_t)batch * capacity : 0;
  DevBuf d_gt, d_counters, d_count, d_ids, d_pixels;
  SF_HIP_CHECK(d_gt.alloc(bytes));
  SF_HIP_CHECK(d_counters.alloc((size_t)batch * id_range(vs) * 4));
  SF_HIP_CHECK(d_count.alloc((size_t)batch * 4));
  SF_HIP_CHECK(d_ids.alloc(cells * 4));
  SF_HIP_CHECK(d_pixels.alloc(cells * 4));
  SF_HIP_CHECK(hipMemcpyAsync(d_gt.p, gt, bytes, hipMemcpyHostToDevice, sg.s));
  if (int rc = launch_image_plan(d_gt.p, elem_bytes, batch, n, vs, capacity, sg.s, d_counters.as<uint32_t>(), d_count.as<uint32_t>(),
                                 instance_id ? d_ids.as<int32_t>() : nullptr, instance_id ? d_pixels.as<uint32_t>() : nullptr))
    return rc;
  std::vector<uint32_t> got(batch);
  SF_HIP_CHECK(hipMemcpyAsync(got.data(), d_count.p, (size_t)batch * 4, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  if (instance_id)
    for (uint32_t b = 0; b < batch; b++)
      if (got[b] > capacity) return sf::fail(SF_ERR_BOUNDS, "sf_eval_image_plan: image %u holds %u instances, capacity %u", b, got[b], capacity);
  if (cells) {
    std::vector<int32_t> id(cells);
    std::vector<uint32_t> px(cells);
    SF_HIP_CHECK(hipMemcpyAsync(id.data(), d_ids.p, cells * 4, hipMemcpyDeviceToHost, sg.s));
    SF_HIP_CHECK(hipMemcpyAsync(px.data(), d_pixels.p, cells * 4, hipMemcpyDeviceToHost, sg.s));
    SF_HIP_CHECK(hipStreamSynchronize(sg.s));
    for (uint32_t b = 0; b < batch; b++) {   // entries from count[b] on are not written
      std::memcpy(instance_id + (size_t)b * capacity, id.data() + (size_t)b * capacity, (size_t)got[b] * 4);
      std::memcpy(instance_pixels + (size_t)b * capacity, px.data() + (size_t)b * capacity, (size_t)got[b] * 4);
    }
  }
  std::memcpy(count, got.data(), (size_t)batch * 4);
  return SF_OK;
}

int overlaps_images_on_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t n, const ValidSet& vs, uint32_t capacity, const uint32_t* count,
                              const int32_t* instance_id, const uint8_t* masks, uint32_t P, uint64_t stride, const uint32_t* mask_image, int device,
                              uint32_t* table) {
  if (int rc = open_device(device, SF_ERR_DEVICE, "%s on a device needs an MI355X (device = -1 is the host path)", "sf_eval_overlaps_images")) return rc;
  if (P == 0) return SF_OK;
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  const size_t gbytes = (size_t)batch * n * elem_bytes, mbytes = (size_t)(P - 1) * stride + n, tbytes = (size_t)P * ((size_t)capacity + 2) * 4;
  DevBuf d_gt, d_count, d_ids, d_masks, d_image, d_table;
  SF_HIP_CHECK(d_gt.alloc(gbytes));
  SF_HIP_CHECK(d_count.alloc((size_t)batch * 4));
  SF_HIP_CHECK(d_ids.alloc((size_t)batch * capacity * 4));
  SF_HIP_CHECK(d_masks.alloc(mbytes));
  SF_HIP_CHECK(d_image.alloc((size_t)P * 4));
  SF_HIP_CHECK(d_table.alloc(tbytes));
  SF_HIP_CHECK(hipMemcpyAsync(d_gt.p, gt, gbytes, hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemcpyAsync(d_count.p, count, (size_t)batch * 4, hipMemcpyHostToDevice, sg.s));
  if (capacity) SF_HIP_CHECK(hipMemcpyAsync(d_ids.p, instance_id, (size_t)batch * capacity * 4, hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemcpyAsync(d_masks.p, masks, mbytes, hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemcpyAsync(d_image.p, mask_image, (size_t)P * 4, hipMemcpyHostToDevice, sg.s));
  if (int rc = launch_overlaps_images(d_gt.p, elem_bytes, batch, n, vs, capacity, d_count.as<uint32_t>(), d_ids.as<int32_t>(), d_masks.as<uint8_t>(), P, stride,
                                      d_image.as<uint32_t>(), sg.s, d_table.as<uint32_t>()))
    return rc;
  SF_HIP_CHECK(hipMemcpyAsync(table, d_table.p, tbytes, hipMemcpyDeviceToHost, sg.s));   // one read-back per batch
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  return SF_OK;
}

}  // namespace ev
}  // namespace sf

// ---- device memory in, device memory out, on the caller's stream; nothing is copied and nothing waits ----

SF_API int sf_eval_confusion_device(const void* gt, const void* pred, int elem_bytes, uint64_t n, const int32_t* valid_ids, uint32_t n_valid, int mode, void* stream,
                                    uint64_t* confusion, uint64_t* out_of_range) {
  uint64_t valid = 0;
  uint32_t dim = 0;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_device: elements of %d bytes (1, 2 or 4)", elem_bytes);
  if (int rc = sf::ev::check_valid(valid_ids, n_valid, &valid, &dim, "sf_eval_confusion_device")) return rc;
  if (mode != (int)MODE_3D && mode != (int)MODE_2D) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_device: mode %d", mode);
  if (!confusion || (mode == (int)MODE_2D && !out_of_range) || (n && (!gt || !pred))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (n > sf::ev::MAX_ELEMENTS) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_device: %llu elements in one call (up to 2^40)", (unsigned long long)n);
  if (((uintptr_t)confusion | (uintptr_t)out_of_range) & 7u) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_device: counters that are not aligned to 8 bytes");
  const void* ptrs[4] = {n ? gt : nullptr, n ? pred : nullptr, confusion, out_of_range};
  DeviceScope scope;
  if (int rc = same_device(ptrs, 4, "sf_eval_confusion_device", scope)) return rc;
  return launch_confusion(gt, pred, elem_bytes, n, valid, dim, mode, (hipStream_t)stream, (unsigned long long*)confusion, (unsigned long long*)out_of_range);
}

SF_API int sf_eval_confusion_images_device(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gt_width, uint32_t gt_height,
                                           uint32_t pred_width, uint32_t pred_height, uint32_t dim, void* stream, uint64_t* confusion, uint64_t* out_of_range) {
  if (int rc = sf::ev::check_images(gt, pred, elem_bytes, batch, gt_width, gt_height, pred_width, pred_height, dim, confusion, out_of_range)) return rc;
  if (((uintptr_t)confusion | (uintptr_t)out_of_range) & 7u) return sf::fail(SF_ERR_INVALID_ARG, "sf_eval_confusion_images_device: counters that are not aligned to 8 bytes");
  const void* ptrs[4] = {batch ? gt : nullptr, batch ? pred : nullptr, confusion, out_of_range};
  DeviceScope scope;
  if (int rc = same_device(ptrs, 4, "sf_eval_confusion_images_device", scope)) return rc;
  return launch_images(gt, pred, elem_bytes, batch, gt_width, gt_height, pred_width, pred_height, SF_EVAL_IMAGE_WIDTH, SF_EVAL_IMAGE_HEIGHT, dim,
                       (hipStream_t)stream, (unsigned long long*)confusion, (unsigned long long*)out_of_range);
}

SF_API int sf_eval_instance_overlaps_device(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, void* stream,
                                            uint32_t* table) {
  if (int rc = sf::ev::check_overlaps(slot, n, G, masks, P, stride, table)) return rc;
  const void* ptrs[3] = {(P && n) ? slot : nullptr, (P && n) ? masks : nullptr, P ? table : nullptr};
  DeviceScope scope;
  if (int rc = same_device(ptrs, 3, "sf_eval_instance_overlaps_device", scope)) return rc;
  return launch_overlaps(slot, n, G, masks, P, stride, (hipStream_t)stream, table);
}

SF_API int sf_eval_image_plan_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids, uint32_t n_valid,
                                     uint32_t capacity, void* stream, void* scratch, uint32_t* count, int32_t* instance_id, uint32_t* instance_pixels) {
  ValidSet vs;
  const char* who = "sf_eval_image_plan_device";
  if (int rc = sf::ev::check_valid_2d(valid_ids, n_valid, &vs, who)) return rc;
  if (int rc = sf::ev::check_image_plan(gt, elem_bytes, batch, width, height, capacity, count, instance_id, instance_pixels, who)) return rc;
  if (batch == 0) return SF_OK;
  if (!scratch) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const void* ptrs[5] = {gt, scratch, count, instance_id, instance_pixels};
  DeviceScope scope;
  if (int rc = same_device(ptrs, 5, who, scope)) return rc;
  return launch_image_plan(gt, elem_bytes, batch, width * height, vs, capacity, (hipStream_t)stream, (uint32_t*)scratch, count, instance_id, instance_pixels);
}

SF_API int sf_eval_overlaps_images_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids,
                                          uint32_t n_valid, uint32_t capacity, const uint32_t* count, const int32_t* instance_id, const uint8_t* masks, uint32_t P,
                                          uint64_t stride, const uint32_t* mask_image, void* stream, uint32_t* table) {
  ValidSet vs;
  const char* who = "sf_eval_overlaps_images_device";
  if (int rc = sf::ev::check_valid_2d(valid_ids, n_valid, &vs, who)) return rc;
  if (int rc = sf::ev::check_overlaps_images(gt, elem_bytes, batch, width, height, capacity, count, instance_id, masks, P, stride, mask_image, table, who)) return rc;
  if (P == 0) return SF_OK;
  const void* ptrs[6] = {gt, count, capacity ? instance_id : nullptr, masks, mask_image, table};
  DeviceScope scope;
  if (int rc = same_device(ptrs, 6, who, scope)) return rc;
  return launch_overlaps_images(gt, elem_bytes, batch, width * height, vs, capacity, count, instance_id, masks, P, stride, mask_image, (hipStream_t)stream, table);
}
