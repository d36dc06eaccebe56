// fuser_prepass.hip -- stage 1 of a fusion pass: the depth pre-pass (u16 -> metres, range gate, colour look-up) of every frame of a batch, and the
// ray-slope tables its colour look-up reads (made once, by sf_fuser_create).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fuser_internal.h"
#include "jpeg_idct.h"

namespace {

// One pixel of a JPEG picture from its component planes (what k_jpeg_idct of jpeg_gpu.hip leaves): chroma upsampling and the fixed-point YCbCr -> RGB of
// jpeg_idct.h, the integer functions the host decoder and k_jpeg_rgb are built from -- the same bytes, for the pixels the pre-pass looks up only.
struct YccPicture {
  int ncomp, sx[3], sy[3], cw[3], ch[3], bw[3];
  const uint8_t* plane[3];
  __device__ YccPicture(const SfJpegLayout* __restrict__ L, const uint8_t* planes) {
    const int W = L->width, H = L->height;
    ncomp = L->ncomp;
    const uint8_t* q = planes;
    for (int c = 0; c < 3; c++) {
      const int cc = c < ncomp ? c : 0;
      sx[c] = L->hmax > L->h[cc] ? 2 : 1; sy[c] = L->vmax > L->v[cc] ? 2 : 1;
      cw[c] = (W + sx[c] - 1) >> (sx[c] - 1); ch[c] = (H * L->v[cc] + L->vmax - 1) >> (L->vmax - 1);
      bw[c] = L->bw[cc];
      plane[c] = q;
      if (c < ncomp) q += (size_t)L->bw[cc] * L->bh[cc];
    }
  }
  __device__ uint32_t pixel(int x, int y) const {   // r | g << 8 | b << 16
    uint8_t o[3];
    if (ncomp == 1) { o[0] = o[1] = o[2] = plane[0][(size_t)y * bw[0] + x]; }
    else {
      int v[3];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        __builtin_assume(sx[c] >= 1 && sx[c] <= 2 && sy[c] >= 1 && sy[c] <= 2);
        v[c] = sf_jpeg_upsample(plane[c], bw[c], cw[c], ch[c], sx[c], sy[c], x, y);
      }
      sf_jpeg_ycc_to_rgb(v[0], v[1], v[2], o);
    }
    return (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
  }
};

// ---------------------------------------------------------------------------------------------------
// K1: depth pre-pass.  u16 -> metres (sensorData.h:968-977: d = depth / depthShift, 0 invalid), range
// gate (zParametersScanNet.txt:34-35) -> -inf; optional rgb -> packed u32.  8 pixels per lane; blockIdx.y = frame
// of the batch (every frame of a batch is converted by ONE launch).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_prepass(BatchIn in, float* __restrict__ depthf_all, uint2* __restrict__ texel_all, int n,
                                                 float shift, float dmin, float dmax, int32_t* counters, int compact_counter, ParamsK P,
                                                 const float* __restrict__ ray_kx, const float* __restrict__ ray_ky) {
  const int j = blockIdx.y;  // frame of the batch
  const uint16_t* __restrict__ depth = in.depth[j];
  const uint8_t* __restrict__ rgb = in.rgb[j];
  float* __restrict__ depthf = depthf_all + (size_t)j * n;
  // RGB-D: the frame's pixels once more as 8-byte texels {depth as the float's bits, rgb in the low three bytes}: the integrate kernel gathers a
  // voxel's depth AND colour with one request (round 4: two 4-byte gathers per voxel and frame kept the CU's texture-address unit busy 82 % of a pass)
  uint2* __restrict__ texel = texel_all + (size_t)j * n;
  const int i0 = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (blockIdx.x == 0 && j == 0 && threadIdx.x == 0) {
    atomicExch(reinterpret_cast<unsigned long long*>(&counters[compact_counter]), 0ull);
  }
  const bool ycc = rgb != nullptr && in.lay[j] != nullptr;   // uniform
  if (i0 >= n && !ycc) return;   // (the planes' look-ups below are dealt out across the whole workgroup)
  uint16_t u[8];
  if (P.inW > 0) {
    // s_integrationWidth / Height: nearest resample of the inW x inH input (scanfuse.h sf_params::integration_width)
    for (int k = 0; k < 8; k++) {
      const int i = i0 + k;
      if (i >= n) { u[k] = 0; continue; }
      const unsigned xi = (unsigned)((float)(i % P.W) * P.rsx + 0.5f), yi = (unsigned)((float)(i / P.W) * P.rsy + 0.5f);
      u[k] = (xi < (unsigned)P.inW && yi < (unsigned)P.inH) ? depth[(size_t)yi * P.inW + xi] : (uint16_t)0;
    }
  } else if (i0 + 8 <= n) {
    const uint4 raw = *reinterpret_cast<const uint4*>(depth + i0);
    u[0] = raw.x & 0xFFFF; u[1] = raw.x >> 16; u[2] = raw.y & 0xFFFF; u[3] = raw.y >> 16;
    u[4] = raw.z & 0xFFFF; u[5] = raw.z >> 16; u[6] = raw.w & 0xFFFF; u[7] = raw.w >> 16;
  } else {
    for (int k = 0; k < 8; k++) u[k] = (i0 + k < n) ? depth[i0 + k] : (uint16_t)0;
  }
  float d[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    float v = (float)u[k] / shift;
    // ... and the integration distance (zParametersScanNet.txt:51), the oracle's "if (!(d < max_integration_dist)) continue": a property of the pixel,
    // gated here once instead of per voxel and frame in fuse_update.  The allocation kernels test d < maxd themselves: -inf changes nothing for them.
    if (u[k] == 0 || v < dmin || v > dmax || !(v < P.maxd)) v = -INFINITY;
    d[k] = v;
  }
  if (i0 + 8 <= n) {
    *reinterpret_cast<float4*>(depthf + i0) = make_float4(d[0], d[1], d[2], d[3]);
    *reinterpret_cast<float4*>(depthf + i0 + 4) = make_float4(d[4], d[5], d[6], d[7]);
  } else {
    for (int k = 0; k < 8 && i0 + k < n; k++) depthf[i0 + k] = d[k];
  }
  if (ycc) {
    // a JPEG picture as component planes: the pixel under each depth pixel (its own, or -- colour at its own resolution -- the one under the depth pixel's ray,
    // the look-up below) is upsampled and converted here.  Consecutive LANES take consecutive pixels for this part (the depths change hands through LDS): a
    // wave's look-ups then fall on one or two rows of each plane and its texel stores are whole 512-byte runs; with the lane's own eight consecutive pixels
    // every byte load of a wave touched 64 different cache lines (k_prepass 200 -> 440 us per 32-frame batch beside the fusion).
    __shared__ float s_d[2048];
#pragma unroll
    for (int k = 0; k < 8; k++) s_d[threadIdx.x * 8 + k] = d[k];
    __syncthreads();
    const YccPicture pic(reinterpret_cast<const SfJpegLayout*>(in.lay[j]), rgb);
    const int wg0 = blockIdx.x * 2048;
#pragma unroll 2
    for (int k = 0; k < 8; k++) {
      const int p = wg0 + k * 256 + (int)threadIdx.x;
      if (p >= n) break;
      const int y = p / P.W, x = p - y * P.W;
      uint32_t c = 0u;
      if (P.cW == 0) c = pic.pixel(x, y);
      else {
        const float u = fmaf(ray_kx[x], P.cfx, P.cmx) + 0.5f;
        const float v = fmaf(ray_ky[y], P.cfy, P.cmy) + 0.5f;
        if (u >= 0.0f && u < (float)P.cW && v >= 0.0f && v < (float)P.cH) c = pic.pixel((int)u, (int)v);
      }
      texel[p] = make_uint2(__float_as_uint(s_d[k * 256 + (int)threadIdx.x]), c);
    }
  } else if (rgb) {
    if (P.cW == 0) {
      // colour at depth resolution: the lane's 8 pixels are 24 contiguous bytes = three 8-byte loads (24 * lane is 8-byte aligned when the
      // image base is), repacked to one dword per pixel
      if (i0 + 8 <= n && ((uintptr_t)rgb & 7) == 0) {
        const uint2* q = reinterpret_cast<const uint2*>(rgb + 3 * (size_t)i0);
        const uint2 a = q[0], b = q[1], c = q[2];
        const uint32_t w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
        uint32_t px[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int bit = 24 * k, lo = bit >> 5, sh = bit & 31;   // three bytes starting at bit 24 k of the 192-bit run
          const uint64_t two = (uint64_t)w[lo] | ((uint64_t)(lo + 1 < 6 ? w[lo + 1] : 0u) << 32);
          px[k] = (uint32_t)(two >> sh) & 0xFFFFFFu;
        }
#pragma unroll
        for (int k = 0; k < 8; k += 2)
          *reinterpret_cast<uint4*>(texel + i0 + k) = make_uint4(__float_as_uint(d[k]), px[k], __float_as_uint(d[k + 1]), px[k + 1]);
      } else {
        for (int k = 0; k < 8 && i0 + k < n; k++) {
          const uint8_t* c = rgb + 3 * (size_t)(i0 + k);
          texel[i0 + k] = make_uint2(__float_as_uint(d[k]), (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16));
        }
      }
    } else {
      // colour image at its own resolution: the colour pixel under the depth pixel's ray (nearest), black outside.  The ray slopes
      // (x - mx) / fx and (y - my) / fy depend on the column / row only: they come from the tables k_ray_tables filled once with the
      // same IEEE divisions (round-1 code divided twice per pixel: 58 us per 16-frame batch against 8 us without colour).
      for (int k = 0; k < 8 && i0 + k < n; k++) {
        const int x = (i0 + k) % P.W, y = (i0 + k) / P.W;
        const float u = fmaf(ray_kx[x], P.cfx, P.cmx) + 0.5f;
        const float v = fmaf(ray_ky[y], P.cfy, P.cmy) + 0.5f;
        if (!(u >= 0.0f && u < (float)P.cW && v >= 0.0f && v < (float)P.cH)) { texel[i0 + k] = make_uint2(__float_as_uint(d[k]), 0u); continue; }
        const uint8_t* c = rgb + 3 * ((size_t)(int)v * (size_t)P.cW + (size_t)(int)u);
        texel[i0 + k] = make_uint2(__float_as_uint(d[k]), (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16));
      }
    }
  }
}

// (x - mx) / fx per column and (y - my) / fy per row of the integration image: the ray slopes the colour look-up of k_prepass multiplies
__global__ void k_ray_tables(float* kx, float* ky, ParamsK P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P.W) kx[i] = ((float)i - P.mx) / P.fx;
  if (i < P.H) ky[i] = ((float)i - P.my) / P.fy;
}

}  // namespace

void sf_launch_prepass(const sf_fuser* f, int sl, int n, const BatchIn& in, hipStream_t s) {
  const int npx = f->p.depth_width * f->p.depth_height;
  hipLaunchKernelGGL(k_prepass, dim3((npx / 8 + 255) / 256 + 1, n), dim3(256), 0, s, in, f->depthf2[sl], f->color2[sl], npx, f->p.depth_shift,
                     f->p.depth_min, f->p.depth_max, f->counters, sf_compact_counter(sl), f->pk, f->ray_kx, f->ray_ky);
}

void sf_launch_ray_tables(const sf_fuser* f) {
  const ParamsK& k = f->pk;
  hipLaunchKernelGGL(k_ray_tables, dim3((std::max(k.W, k.H) + 255) / 256), dim3(256), 0, f->stream, f->ray_kx, f->ray_ky, k);
}
