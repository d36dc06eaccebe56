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
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.h"
#include "evaluation_internal.h"
#include "hip_util.h"

namespace {

using sf::ev::KEY_SKIP;
using sf::ev::MODE_2D;
using sf::ev::MODE_3D;

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

bool on_device(const void* p, int* device) {
  if (!p) return false;
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (device) *device = a.device;
  return a.type == hipMemoryTypeDevice;
}

int need_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return sf::fail(SF_ERR_DEVICE, "no HIP device: %s on a device needs an MI355X (device = -1 is the host path)", who);
  }
  if (device >= ndev) return sf::fail(SF_ERR_DEVICE, "%s: device %d of %d", who, device, ndev);
  SF_HIP_CHECK(hipSetDevice(device));
  return SF_OK;
}

// the device of a _device call is current for the launch only: the caller's current device is put back when the call returns
struct DeviceScope {
  int old = -1;
  bool changed = false;
  DeviceScope() = default;
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
  ~DeviceScope() { if (changed) (void)hipSetDevice(old); }
  hipError_t enter(int dev) {
    hipError_t e = hipGetDevice(&old);
    if (e != hipSuccess || old == dev) return e;
    e = hipSetDevice(dev);
    changed = e == hipSuccess;
    return e;
  }
};

// every pointer of a _device call must be device memory, all on one device: that device is made current for the life of `scope`.  The look-ups are
// hipPointerGetAttributes, a query on the host that waits for nothing on the device.
int same_device(const void* const* ptrs, int count, const char* who, DeviceScope& scope) {
  int dev = -1;
  for (int i = 0; i < count; i++) {
    if (!ptrs[i]) continue;
    int d = -1;
    if (!on_device(ptrs[i], &d)) return sf::fail(SF_ERR_INVALID_ARG, "%s: argument %d is not device memory", who, i);
    if (dev >= 0 && d != dev) return sf::fail(SF_ERR_INVALID_ARG, "%s: arguments on devices %d and %d", who, dev, d);
    dev = d;
  }
  if (dev >= 0) SF_HIP_CHECK(scope.enter(dev));
  return SF_OK;
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

}  // namespace

namespace sf {
namespace ev {

// host arrays in, host counters out (added to): copy up, count, read back
int confusion_on_device(const void* gt, const void* pred, int elem_bytes, uint64_t n, uint64_t valid, uint32_t dim, int mode, int device, uint64_t* confusion,
                        uint64_t* out_of_range) {
  if (int rc = need_device(device, "sf_eval_confusion")) return rc;
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
  if (int rc = need_device(device, "sf_eval_confusion_images")) return rc;
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
  if (int rc = need_device(device, "sf_eval_instance_overlaps")) return rc;
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
