// align_colour.hip -- the dense colour term of the global alignment (DESIGN.md "The colour term of the global alignment", 4f; BundleFusion's
// s_denseColorThresh / s_denseColorGradientMin, zParametersBundlingScanNet.txt:24-25).
//
// Once per call: k_photo_prep turns every keyframe's RGB8 picture into one float4 {intensity, gx, gy, 0} per pixel of the solver's level, so that a
// bilinear tap is one 16-byte load.  Per Gauss-Newton iteration align.hip's k_align_assoc<true> is its depth kernel with a second row: every depth
// correspondence (tk::correspond, unchanged) whose source has an intensity and whose four target taps have an intensity and a gradient adds
// colour_weight x the photometric row (p x a, a) to the pair's 27 sums, and its r_c^2 and 1 behind the depth term's two; k_align_final<true> sums the
// 31 values of a pair's partials in index order in double.  The host loop is align.hip's.  tests/align_checker.c restates every operation bit for bit.
#include <hip/hip_runtime.h>

#include "align_internal.h"
#include "common.h"
#include "photo_math.h"

namespace {

using namespace tk;   // photo_math.h: the intensity rule, the level means, the bilinear tap and the colour row, shared with track_colour.hip

// all K pictures at once (blockIdx.y = frame): RGB8 -> intensity -> L reductions -> {I, gx, gy, 0} of level L, the gradient by central differences
// (-inf on the border and where one of the four neighbours has no intensity)
template <int L>
__global__ void __launch_bounds__(256) k_photo_prep(const uint8_t* __restrict__ pictures, size_t picture_stride, const ParamsK P, const Cam c,
                                                    float4* __restrict__ photo) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int npx = c.W * c.H;
  if (i >= npx) return;
  const uint8_t* rgb = pictures + (size_t)blockIdx.y * picture_stride;
  const int x = i % c.W, y = i / c.W;
  // the pixel and its four neighbours one after the other in a rolled loop: at level 3 each is 64 colour pixels, and the five unrolled took 350
  // registers (one wave per SIMD) where the loop takes 103 (four); a border pixel reads itself five times and has no gradient
  const bool inner = x >= 1 && x + 1 < c.W && y >= 1 && y + 1 < c.H;
  float I = 0.0f, xl = 0.0f, xr = 0.0f, yu = 0.0f, yd = 0.0f;
#pragma nounroll
  for (int t = 0; t < 5; t++) {
    const int dx = !inner ? 0 : (t == 1 ? -1 : (t == 2 ? 1 : 0)), dy = !inner ? 0 : (t == 3 ? -1 : (t == 4 ? 1 : 0));
    const float s = level_intensity<L>(rgb, P, x + dx, y + dy);
    I = t == 0 ? s : I;
    xl = t == 1 ? s : xl;
    xr = t == 2 ? s : xr;
    yu = t == 3 ? s : yu;
    yd = t == 4 ? s : yd;
  }
  photo[(size_t)blockIdx.y * npx + i] = photo_texel(I, inner, xl, xr, yu, yd);
}

}  // namespace

int sf_photo_prepare(sf_fuser* f, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K, int level, const Cam& cam) {
  AlignWork* w = f->align;
  const int npx = cam.W * cam.H;
  const dim3 grid((npx + 255) / 256, (unsigned)K);
#define PH_PREP(L) \
  hipLaunchKernelGGL(k_photo_prep<L>, grid, dim3(256), 0, f->stream, (const uint8_t*)d_rgb, (size_t)rgb_stride_bytes, f->pk, cam, w->photo.as<float4>())
  switch (level) {
    case 0: PH_PREP(0); break;
    case 1: PH_PREP(1); break;
    case 2: PH_PREP(2); break;
    default: PH_PREP(3); break;
  }
#undef PH_PREP
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}
