// depth_lut.hip -- calibrate_depth's two batch modes on gfx950: estimating the depth-distortion table the `calibrate`
// stage reads (EstimateDistortion, CameraParameterEstimation/apps/calibrate_depth/src/calibrate_depth.cpp:647-836) and applying one to depth
// images (ApplyUndistortion, :565-644).
//   k_lut_accumulate   the two sums of every table cell over a batch of images (:716-750 + :778-806, fused: the training pairs are never stored)
//   k_lut_finish       divide, side stripe, unknowns (:809-833)
//   k_lut_apply        :618-636 for a batch of images, through the `calibrate` stage's lut_value
// The sums are sequential binary32 sums in the reference's order -- image, then row, then column.  A table column (x, y) takes samples from the
// 2 x 2 pixels under it only, so ONE LANE owns a column and walks the batch's images in order: no atomics, and the bits are the reference's.  The
// slice a sample falls into is data-dependent; a register array indexed by it would live in private memory, so the lane's 2 * n_slices running
// sums live in LDS, laid out [slice][lane]: whatever mix of slices a wave touches, its 64 lanes hit 64 different banks.  They are loaded from the
// estimator's sums at the start of a launch and stored at its end, so launches chain.  The table of a 640 x 480 sequence is 76 800 lanes, about a
// wave per SIMD: the loop would wait a full memory latency per image, so the two 4-byte loads of LUT_GROUP images are issued ahead of the arithmetic.
#include <hip/hip_runtime.h>

#include <cstring>

#include "depth_lut_internal.h"
#include "hip_util.h"

namespace {

constexpr const char* LUT_NEEDS_DEVICE = "pass device -1 for the host path, there is no silent fallback";
constexpr int LUT_GROUP = 8;   // images whose loads are in flight together

template <int T>
__global__ __launch_bounds__(T) void k_lut_accumulate(LutGeom g, const LutImage* __restrict__ tab, int n, float* __restrict__ acc, float* __restrict__ div) {
  extern __shared__ float sums[];   // [2 * ns][T]: row 2z the accumulation, row 2z + 1 the divisor of slice z
  const int ncell = g.xres * g.yres;
  const int c = (int)blockIdx.x * T + (int)threadIdx.x;
  if (c >= ncell) return;           // a lane touches its own LDS words only: no barrier anywhere
  const int x = c % g.xres, y = c / g.xres;
  float* mine = sums + threadIdx.x;
  for (int z = 0; z < g.ns; z++) {
    mine[(2 * z) * T] = acc[(size_t)z * ncell + c];
    mine[(2 * z + 1) * T] = div[(size_t)z * ncell + c];
  }
  const int half = g.w / 2;                 // 4-byte words per image row (w is even)
  const int w0 = 2 * y * half + x;          // pixels (2x, 2y), (2x + 1, 2y); the row below is `half` words on
  for (int b = 0; b < n; b += LUT_GROUP) {
    uint32_t r0[LUT_GROUP], r1[LUT_GROUP];
#pragma unroll
    for (int k = 0; k < LUT_GROUP; k++) {
      r0[k] = r1[k] = 0;
      if (b + k < n) {
        const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(tab[b + k].px);
        r0[k] = p[w0];
        r1[k] = p[w0 + half];
      }
    }
#pragma unroll
    for (int k = 0; k < LUT_GROUP; k++) {
      if (b + k >= n) break;
      const LutImage im = tab[b + k];
      if (!im.used) continue;
      const uint16_t px[4] = {(uint16_t)(r0[k] & 0xFFFF), (uint16_t)(r0[k] >> 16), (uint16_t)(r1[k] & 0xFFFF), (uint16_t)(r1[k] >> 16)};
#pragma unroll
      for (int q = 0; q < 4; q++) {   // j, then i
        float ta, td;
        const int z = lut_sample(g, im, 2 * x + (q & 1), 2 * y + (q >> 1), px[q], ta, td);
        if (z != 0) {                 // 1 <= z <= ns - 1
          mine[(2 * z) * T] += ta;
          mine[(2 * z + 1) * T] += td;
        }
      }
    }
  }
  for (int z = 0; z < g.ns; z++) {
    acc[(size_t)z * ncell + c] = mine[(2 * z) * T];
    div[(size_t)z * ncell + c] = mine[(2 * z + 1) * T];
  }
}

__global__ __launch_bounds__(256) void k_lut_finish(int xres, int yres, int ns, const float* __restrict__ acc, const float* __restrict__ div, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n = (size_t)xres * yres * ns;
  if (i >= n) return;
  const int x = (int)(i % (size_t)xres);
  out[i] = lut_finish_cell(acc, div, xres, i - (size_t)x, x);
}

struct LutApplyImage { const uint16_t* in; uint16_t* out; };

__global__ __launch_bounds__(256) void k_lut_apply(LutApplyK k, const float* __restrict__ table, const LutApplyImage* __restrict__ tab) {
  const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (p >= k.w * k.h) return;
  const LutApplyImage im = tab[blockIdx.y];
  im.out[p] = lut_apply_pixel(k, table, p % k.w, p / k.w, im.in[p]);
}

int pick_block(int ns) {   // the largest workgroup whose sums fit the LDS budget; 0: none does
  for (int t : {256, 128, 64})
    if ((size_t)t * 2 * sizeof(float) * (size_t)ns <= LUT_LDS_BUDGET) return t;
  return 0;
}

}  // namespace

int lut_dev_create(sf_lut_estimator* e) {
  e->block = pick_block(e->g.ns);
  if (!e->block) return sf::fail(SF_ERR_PARAM, "n_slices %d: a lane's sums do not fit the LDS (limit %d)", e->g.ns, LUT_MAX_SLICES);
  const int rc = sf::open_device(e->device, SF_ERR_INVALID_ARG, LUT_NEEDS_DEVICE);
  if (rc != SF_OK) return rc;
  const size_t cells = (size_t)e->g.xres * e->g.yres * e->g.ns, px = (size_t)e->g.w * e->g.h;
  SF_HIP_CHECK(hipMalloc((void**)&e->d_acc, cells * 4));
  SF_HIP_CHECK(hipMalloc((void**)&e->d_div, cells * 4));
  SF_HIP_CHECK(hipMalloc((void**)&e->d_out, cells * 4));
  SF_HIP_CHECK(hipMalloc((void**)&e->d_tab, sizeof(LutImage) * LUT_MAX_BATCH));
  SF_HIP_CHECK(hipMalloc((void**)&e->d_stage, px * 2 * LUT_MAX_BATCH));
  SF_HIP_CHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  SF_HIP_CHECK(hipEventCreate(&e->e0));
  SF_HIP_CHECK(hipEventCreate(&e->e1));
  SF_HIP_CHECK(hipMemsetAsync(e->d_acc, 0, cells * 4, e->stream));
  SF_HIP_CHECK(hipMemsetAsync(e->d_div, 0, cells * 4, e->stream));
  return SF_OK;
}

void lut_dev_destroy(sf_lut_estimator* e) {
  if (hipSetDevice(e->device) != hipSuccess) (void)hipGetLastError();   // an estimator whose device was refused at create: no error is left for the next launch check
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (void* p : {(void*)e->d_acc, (void*)e->d_div, (void*)e->d_out, (void*)e->d_tab, (void*)e->d_stage})
    if (p) (void)hipFree(p);
  if (e->e0) (void)hipEventDestroy(e->e0);
  if (e->e1) (void)hipEventDestroy(e->e1);
  if (e->stream) (void)hipStreamDestroy(e->stream);
}

// host_pixels: tab[].px are host images, staged here; else device images (4-byte aligned, checked by the caller)
int lut_dev_add(sf_lut_estimator* e, int n, const LutImage* tab, bool host_pixels, float* kernel_us) {
  if (n < 1 || n > LUT_MAX_BATCH) return sf::fail(SF_ERR_INVALID_ARG, "batch of %d images (limit %d)", n, LUT_MAX_BATCH);
  SF_HIP_CHECK(hipSetDevice(e->device));
  const size_t px = (size_t)e->g.w * e->g.h;
  LutImage t[LUT_MAX_BATCH];
  std::memcpy(t, tab, sizeof(LutImage) * n);
  if (host_pixels)
    for (int k = 0; k < n; k++) {
      SF_HIP_CHECK(hipMemcpyAsync(e->d_stage + px * k, tab[k].px, px * 2, hipMemcpyHostToDevice, e->stream));
      t[k].px = e->d_stage + px * k;
    }
  SF_HIP_CHECK(hipMemcpyAsync(e->d_tab, t, sizeof(LutImage) * n, hipMemcpyHostToDevice, e->stream));
  SF_HIP_CHECK(hipStreamSynchronize(e->stream));   // `t` is on this stack: the copy (and whatever was queued before it) is done before the launch goes out
  const int ncell = e->g.xres * e->g.yres, T = e->block;
  const dim3 grid((ncell + T - 1) / T);
  const size_t lds = (size_t)T * 2 * sizeof(float) * e->g.ns;
  if (kernel_us) SF_HIP_CHECK(hipEventRecord(e->e0, e->stream));
  if (T == 256) hipLaunchKernelGGL(k_lut_accumulate<256>, grid, dim3(256), lds, e->stream, e->g, e->d_tab, n, e->d_acc, e->d_div);
  else if (T == 128) hipLaunchKernelGGL(k_lut_accumulate<128>, grid, dim3(128), lds, e->stream, e->g, e->d_tab, n, e->d_acc, e->d_div);
  else hipLaunchKernelGGL(k_lut_accumulate<64>, grid, dim3(64), lds, e->stream, e->g, e->d_tab, n, e->d_acc, e->d_div);
  SF_HIP_CHECK(hipGetLastError());
  if (kernel_us) {
    SF_HIP_CHECK(hipEventRecord(e->e1, e->stream));
    SF_HIP_CHECK(hipEventSynchronize(e->e1));
    float ms = 0;
    SF_HIP_CHECK(hipEventElapsedTime(&ms, e->e0, e->e1));
    *kernel_us = ms * 1e3f;
  } else if (host_pixels) {
    SF_HIP_CHECK(hipStreamSynchronize(e->stream));   // the caller's images and the stage may be reused
  }
  return SF_OK;
}

int lut_dev_sums(sf_lut_estimator* e, float* acc, float* div) {
  SF_HIP_CHECK(hipSetDevice(e->device));
  const size_t cells = (size_t)e->g.xres * e->g.yres * e->g.ns;
  SF_HIP_CHECK(hipMemcpyAsync(acc, e->d_acc, cells * 4, hipMemcpyDeviceToHost, e->stream));
  SF_HIP_CHECK(hipMemcpyAsync(div, e->d_div, cells * 4, hipMemcpyDeviceToHost, e->stream));
  SF_HIP_CHECK(hipStreamSynchronize(e->stream));
  return SF_OK;
}

int lut_dev_finish(sf_lut_estimator* e, float* table) {
  SF_HIP_CHECK(hipSetDevice(e->device));
  const size_t cells = (size_t)e->g.xres * e->g.yres * e->g.ns;
  hipLaunchKernelGGL(k_lut_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, e->stream, e->g.xres, e->g.yres, e->g.ns, e->d_acc, e->d_div, e->d_out);
  SF_HIP_CHECK(hipGetLastError());
  SF_HIP_CHECK(hipMemcpyAsync(table, e->d_out, cells * 4, hipMemcpyDeviceToHost, e->stream));
  SF_HIP_CHECK(hipStreamSynchronize(e->stream));
  return SF_OK;
}

// n images of k.w x k.h through `table` (host memory).  Synchronous.
int lut_dev_apply(int device, const LutApplyK& k, const float* table, int n, const void* const* in, void* const* out, bool host_pixels, float* kernel_us) {
  if (n < 1 || n > 65535) return sf::fail(SF_ERR_INVALID_ARG, "batch of %d images (limit 65535)", n);
  const int rc = sf::open_device(device, SF_ERR_INVALID_ARG, LUT_NEEDS_DEVICE);
  if (rc != SF_OK) return rc;
  const size_t cells = (size_t)k.xr * k.yr * k.zr, px = (size_t)k.w * k.h;
  sf::DevBuf d_table, d_tab, d_px;
  sf::EventSpan span;
  std::vector<LutApplyImage> t(n);
  SF_HIP_CHECK(d_table.alloc(cells * 4));
  SF_HIP_CHECK(d_tab.alloc(sizeof(LutApplyImage) * n));
  SF_HIP_CHECK(hipMemcpy(d_table.p, table, cells * 4, hipMemcpyHostToDevice));
  if (host_pixels) {
    SF_HIP_CHECK(d_px.alloc(px * 2 * 2 * (size_t)n));
    for (int j = 0; j < n; j++) {
      t[j].in = d_px.as<uint16_t>() + px * (2 * (size_t)j);
      t[j].out = d_px.as<uint16_t>() + px * (2 * (size_t)j + 1);
      SF_HIP_CHECK(hipMemcpy((void*)t[j].in, in[j], px * 2, hipMemcpyHostToDevice));
    }
  } else {
    for (int j = 0; j < n; j++) t[j] = LutApplyImage{(const uint16_t*)in[j], (uint16_t*)out[j]};
  }
  SF_HIP_CHECK(hipMemcpy(d_tab.p, t.data(), sizeof(LutApplyImage) * n, hipMemcpyHostToDevice));
  if (kernel_us) span.begin(nullptr);
  hipLaunchKernelGGL(k_lut_apply, dim3((unsigned)((px + 255) / 256), (unsigned)n), dim3(256), 0, nullptr, k, d_table.as<float>(), d_tab.as<LutApplyImage>());
  SF_HIP_CHECK(hipGetLastError());
  if (kernel_us) span.end(nullptr);
  SF_HIP_CHECK(hipDeviceSynchronize());
  if (kernel_us) *kernel_us = span.us();
  if (host_pixels)
    for (int j = 0; j < n; j++) SF_HIP_CHECK(hipMemcpy(out[j], t[j].out, px * 2, hipMemcpyDeviceToHost));
  return SF_OK;
}
