// track_colour.hip -- the dense colour term of the camera tracker (DESIGN.md "The colour term of the tracker", 4g): 4f's photometric row with the
// ray-cast model's colour as the target.
//
// Once per frame, level by level: the frame's RGB8 picture and the model's rendered colour become an intensity image (k_track_photo_in0,
// k_track_photo_model0: the model has no intensity where it has no depth or no normal), every coarser level is the 2x2 mean of the one below
// (k_track_photo_down), and each level gets one float4 {intensity, gx, gy, 0} per pixel (k_track_photo_grad), so that a bilinear tap is one 16-byte
// load.  Per iteration track.hip's k_track_assoc<true> is its depth kernel with a second row: every depth correspondence (tk::correspond, unchanged; its
// target stays the subsampled level-0 model) whose pixel has an intensity and whose four taps in the model's map of the level have an intensity and a
// gradient adds colour_weight x the row (p x a, a) to the 27 sums, and its r_c^2 and 1 behind the depth term's two; k_track_final<true> sums the 31
// values of the partials in index order in double.  The host loop is track.hip's.  tests/track_checker.c restates every operation bit for bit.
#include <hip/hip_runtime.h>

#include "common.h"
#include "photo_math.h"
#include "track_internal.h"

namespace {

using namespace tk;

// level 0 of the frame: the intensity of the colour pixel under every integration pixel's ray (photo_math.h intensity0_at)
__global__ void __launch_bounds__(256) k_track_photo_in0(const uint8_t* __restrict__ rgb, const ParamsK P, float* __restrict__ I0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P.W * P.H) return;
  I0[i] = intensity0_at(rgb, P, i % P.W, i / P.W);
}

// level 0 of the model: the intensity of the rendered colour where the model pixel is valid as k_track_model takes it (a miss renders 0, 0, 0, which
// is not black)
__global__ void __launch_bounds__(256) k_track_photo_model0(const uint8_t* __restrict__ mrgb, const float* __restrict__ md, const float* __restrict__ mn, int n,
                                                            float* __restrict__ I0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  I0[i] = (md[i] > 0.0f && mn[3 * (size_t)i] > -INFINITY) ? intensity_rgb8(mrgb + 3 * (size_t)i) : -INFINITY;
}

// one 2x2 mean (photo_math.h mean4) of the frame's (blockIdx.y = 0) and of the model's (1) intensity image
__global__ void __launch_bounds__(256) k_track_photo_down(const float* __restrict__ src0, const float* __restrict__ src1, int Ws, float* __restrict__ dst0,
                                                          float* __restrict__ dst1, int Wd, int Hd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Wd * Hd) return;
  const float* __restrict__ src = blockIdx.y ? src1 : src0;
  float* __restrict__ dst = blockIdx.y ? dst1 : dst0;
  const int x = i % Wd, y = i / Wd;
  const float* s = src + (size_t)(2 * y) * Ws + 2 * x;
  dst[i] = mean4(s[0], s[1], s[Ws], s[Ws + 1]);
}

// {I, gx, gy, 0} of every pixel of a level of the frame (blockIdx.y = 0) and of the model (1): central differences (photo_math.h photo_texel); the
// four neighbours are read only inside the image
__global__ void __launch_bounds__(256) k_track_photo_grad(const float* __restrict__ I0, const float* __restrict__ I1, int W, int H, float4* __restrict__ out0,
                                                          float4* __restrict__ out1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const float* __restrict__ I = blockIdx.y ? I1 : I0;
  float4* __restrict__ out = blockIdx.y ? out1 : out0;
  const int x = i % W, y = i / W;
  const bool inner = x >= 1 && x + 1 < W && y >= 1 && y + 1 < H;
  float xl = 0.0f, xr = 0.0f, yu = 0.0f, yd = 0.0f;
  if (inner) {
    xl = I[i - 1];
    xr = I[i + 1];
    yu = I[i - W];
    yd = I[i + W];
  }
  out[i] = photo_texel(I[i], inner, xl, xr, yu, yd);
}

}  // namespace

int sf_track_photo_reserve(sf_fuser* f, const Cam* cams, int levels) {
  TrackWork* w = f->track;
  if (w->photo_levels >= levels) return SF_OK;
  const size_t n0 = (size_t)cams[0].W * cams[0].H;
  hipError_t e = w->d_rgb.reserve(sf_track_picture_bytes(f));
  if (e == hipSuccess) e = w->model_rgb.reserve(n0 * 3);
  for (int s = 0; s < 2; s++)
    for (int l = 0; l < levels; l++) {
      const size_t n = (size_t)cams[l].W * cams[l].H;
      if (e == hipSuccess) e = w->inten[s][l].reserve(n * sizeof(float));
      if (e == hipSuccess) e = w->photo[s][l].reserve(n * sizeof(float4));
    }
  if (e != hipSuccess) { sf_track_release(f); return sf::fail(SF_ERR_DEVICE, "tracking colour buffers: %s", hipGetErrorString(e)); }
  w->photo_levels = levels;
  return SF_OK;
}

int sf_track_photo_prepare(sf_fuser* f, const void* d_rgb, const Cam* cams, int levels) {
  TrackWork* w = f->track;
  const int n0 = cams[0].W * cams[0].H;
  hipLaunchKernelGGL(k_track_photo_in0, dim3((n0 + 255) / 256), dim3(256), 0, f->stream, (const uint8_t*)d_rgb, f->pk, w->inten[0][0].as<float>());
  SF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_track_photo_model0, dim3((n0 + 255) / 256), dim3(256), 0, f->stream, w->model_rgb.as<const uint8_t>(), w->model_depth.as<const float>(),
                     w->model_normal.as<const float>(), n0, w->inten[1][0].as<float>());
  SF_HIP_CHECK(hipGetLastError());
  for (int l = 1; l < levels; l++) {
    const int n = cams[l].W * cams[l].H;
    hipLaunchKernelGGL(k_track_photo_down, dim3((n + 255) / 256, 2), dim3(256), 0, f->stream, w->inten[0][l - 1].as<const float>(),
                       w->inten[1][l - 1].as<const float>(), cams[l - 1].W, w->inten[0][l].as<float>(), w->inten[1][l].as<float>(), cams[l].W, cams[l].H);
    SF_HIP_CHECK(hipGetLastError());
  }
  for (int l = 0; l < levels; l++) {
    const int n = cams[l].W * cams[l].H;
    hipLaunchKernelGGL(k_track_photo_grad, dim3((n + 255) / 256, 2), dim3(256), 0, f->stream, w->inten[0][l].as<const float>(), w->inten[1][l].as<const float>(),
                       cams[l].W, cams[l].H, w->photo[0][l].as<float4>(), w->photo[1][l].as<float4>());
    SF_HIP_CHECK(hipGetLastError());
  }
  return SF_OK;
}
