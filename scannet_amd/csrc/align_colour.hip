// align_colour.hip -- the dense colour term of the global alignment (DESIGN.md "The colour term of the global alignment", 4f; BundleFusion's
// s_denseColorThresh / s_denseColorGradientMin, zParametersBundlingScanNet.txt:24-25).
//
// Once per call: k_photo_prep turns every keyframe's RGB8 picture into one float4 {intensity, gx, gy, 0} per pixel of the solver's level, so that a
// bilinear tap is one 16-byte load.  Per Gauss-Newton iteration k_photo_assoc is k_align_assoc with a second row: every depth correspondence
// (tk::correspond, unchanged) whose source has an intensity and whose four target taps have an intensity and a gradient adds colour_weight x the
// photometric row (p x a, a) to the pair's 27 sums, and its r_c^2 and 1 behind the depth term's two; k_photo_final sums the 31 values of a pair's
// partials in index order in double.  The host loop is align.hip's.  tests/align_colour_checker.c restates every operation bit for bit.
#include <hip/hip_runtime.h>

#include "align_internal.h"
#include "common.h"

namespace {

using namespace tk;

// intensity of pixel (x, y) of the integration image, in [0, 1]: the colour pixel under the same ray by the pre-pass's rule (nearest); -inf outside the picture
__device__ inline float intensity0_at(const uint8_t* __restrict__ rgb, const ParamsK& P, int x, int y) {
  int cx = x, cy = y, cw = P.W;
  if (P.cW > 0) {
    const float u = fmaf(((float)x - P.mx) / P.fx, P.cfx, P.cmx) + 0.5f;
    const float v = fmaf(((float)y - P.my) / P.fy, P.cfy, P.cmy) + 0.5f;
    if (!(u >= 0.0f && u < (float)P.cW && v >= 0.0f && v < (float)P.cH)) return -INFINITY;
    cx = (int)u;
    cy = (int)v;
    cw = P.cW;
  }
  const uint8_t* q = rgb + 3 * ((size_t)cy * (size_t)cw + (size_t)cx);
  return ((0.299f * (float)q[0] + 0.587f * (float)q[1]) + 0.114f * (float)q[2]) / 255.0f;
}

// level L: the mean of the 2x2 block of level L - 1 in the order (0,0), (1,0), (0,1), (1,1); invalid if one of the four is
template <int L>
__device__ inline float level_intensity(const uint8_t* __restrict__ rgb, const ParamsK& P, int x, int y) {
  if constexpr (L == 0) {
    return intensity0_at(rgb, P, x, y);
  } else {
    const float s00 = level_intensity<L - 1>(rgb, P, 2 * x, 2 * y), s10 = level_intensity<L - 1>(rgb, P, 2 * x + 1, 2 * y);
    const float s01 = level_intensity<L - 1>(rgb, P, 2 * x, 2 * y + 1), s11 = level_intensity<L - 1>(rgb, P, 2 * x + 1, 2 * y + 1);
    return (s00 >= 0.0f && s10 >= 0.0f && s01 >= 0.0f && s11 >= 0.0f) ? (((s00 + s10) + s01) + s11) * 0.25f : -INFINITY;
  }
}

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
  float4 o = make_float4(I, -INFINITY, -INFINITY, 0.0f);
  if (inner && xl >= 0.0f && xr >= 0.0f && yu >= 0.0f && yd >= 0.0f) {
    o.y = (xr - xl) * 0.5f;
    o.z = (yd - yu) * 0.5f;
  }
  photo[(size_t)blockIdx.y * npx + i] = o;
}

// bilinear sample of one component: the two rows along x, then along y
__device__ inline float bilin(float t00, float t10, float t01, float t11, float ax, float ay) {
  const float top = fmaf(ax, t10 - t00, t00), bot = fmaf(ax, t11 - t01, t01);
  return fmaf(ay, bot - top, top);
}

// one pair per blockIdx.y: k_align_assoc's association and depth row, and in the same lane the colour row of the correspondence; one 31-float partial
// per 256-pixel workgroup, partials[P][nb][32].  photo == nullptr: no colour rows
__global__ void __launch_bounds__(256) k_photo_assoc(const float4* __restrict__ vmap, const float4* __restrict__ nmap, const float4* __restrict__ photo,
                                                     const AlignPair* __restrict__ table, const Cam c, float dist_thres, float normal_thres, float weight,
                                                     float colour_thres, float gradient_min, float* __restrict__ partials) {
  __shared__ float red[4][AL_NSYS_RGBD];
  const AlignPair& e = table[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int npx = c.W * c.H;
  float acc[AL_NSYS_RGBD];
#pragma unroll
  for (int k = 0; k < AL_NSYS_RGBD; k++) acc[k] = 0.0f;
  if (e.active && i < npx) {
    const size_t so = (size_t)e.i * npx, to = (size_t)e.j * npx;
    const float4 v4 = vmap[so + i];
    const bool hit = correspond(c, e.Ti, e.M, v4, nmap[so + i], dist_thres, normal_thres, [&](int ux, int uy, float3* q, float3* nm) {
      const size_t t = to + (size_t)(uy * c.W + ux);
      const float4 w4 = vmap[t], m4 = nmap[t];
      if (!(w4.z > 0.0f && m4.x > -INFINITY)) return false;
      *q = xf(e.Tj, make_float3(w4.x, w4.y, w4.z));
      *nm = rot(e.Tj, make_float3(m4.x, m4.y, m4.z));
      return true;
    }, acc);
    if (hit && photo) {
      const float Is = photo[so + i].x;
      const float3 v = make_float3(v4.x, v4.y, v4.z);
      const float3 p = xf(e.Ti, v), pc = xf(e.M, v);   // a correspondence has pc.z > 0
      const float uf = fmaf(pc.x / pc.z, c.fx, c.mx), vf = fmaf(pc.y / pc.z, c.fy, c.my);
      // the four taps (x0, y0) .. (x0 + 1, y0 + 1) lie inside the image: compared in float before any conversion, so that a huge or non-finite
      // projection forms no address
      if (Is >= 0.0f && uf >= 0.0f && uf < (float)(c.W - 1) && vf >= 0.0f && vf < (float)(c.H - 1)) {
        const float xf0 = floorf(uf), yf0 = floorf(vf);
        const float4* t = photo + to + (size_t)((int)yf0 * c.W + (int)xf0);
        const float4 t00 = t[0], t10 = t[1], t01 = t[c.W], t11 = t[c.W + 1];
        if (t00.x >= 0.0f && t00.y > -INFINITY && t10.x >= 0.0f && t10.y > -INFINITY && t01.x >= 0.0f && t01.y > -INFINITY && t11.x >= 0.0f &&
            t11.y > -INFINITY) {
          const float ax = uf - xf0, ay = vf - yf0;
          const float It = bilin(t00.x, t10.x, t01.x, t11.x, ax, ay);
          const float gx = bilin(t00.y, t10.y, t01.y, t11.y, ax, ay), gy = bilin(t00.z, t10.z, t01.z, t11.z, ax, ay);
          const float r = It - Is;
          if (!(fabsf(r) > colour_thres || sqrtf(gx * gx + gy * gy) < gradient_min)) {
            const float gxf = gx * c.fx, gyf = gy * c.fy;
            const float3 g = make_float3(gxf / pc.z, gyf / pc.z, -((gxf * pc.x + gyf * pc.y) / (pc.z * pc.z)));
            const float3 a = rot(e.Tj, g);
            const float3 cr = cross3(p, a);
            const float J[6] = {cr.x, cr.y, cr.z, a.x, a.y, a.z};
            if (weight != 0.0f) {   // weight 0: the depth term's sums stay as they are, whatever the colour row holds
              int k = 0;
#pragma unroll
              for (int u = 0; u < 6; u++)
#pragma unroll
                for (int w = u; w < 6; w++, k++) acc[k] = acc[k] + weight * (J[u] * J[w]);
#pragma unroll
              for (int u = 0; u < 6; u++) acc[21 + u] = acc[21 + u] + weight * (J[u] * r);
            }
            acc[29] = r * r;
            acc[30] = 1.0f;
          }
        }
      }
    }
  }
  reduce256(acc, red, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * TK_PSTRIDE);
}

// one wave per pair: lane k sums value k of the pair's partials in index order, in double; out[P][31]
__global__ void __launch_bounds__(64) k_photo_final(const float* __restrict__ partials, int nb, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k < AL_NSYS_RGBD) out[(size_t)blockIdx.x * AL_NSYS_RGBD + k] = sum_partials(partials + (size_t)blockIdx.x * nb * TK_PSTRIDE, nb, k);
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

int sf_photo_systems(sf_fuser* f, uint64_t P, const Cam& cam, const sf_align_params* a, bool with_photo) {
  AlignWork* w = f->align;
  const int npx = cam.W * cam.H, nb = (npx + 255) / 256;
  hipLaunchKernelGGL(k_photo_assoc, dim3(nb, (unsigned)P), dim3(256), 0, f->stream, w->vmap.as<const float4>(), w->nmap.as<const float4>(),
                     with_photo ? w->photo.as<const float4>() : nullptr, w->d_table.as<const AlignPair>(), cam, a->dist_thres, a->normal_thres,
                     a->colour_weight, a->colour_thres, a->colour_gradient_min, w->partials.as<float>());
  SF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_photo_final, dim3((unsigned)P), dim3(64), 0, f->stream, w->partials.as<const float>(), nb, w->d_sys.as<double>());
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}
