// photo_math.h -- the per-pixel rules of the dense colour term that the global alignment (align_colour.hip) and the camera tracker
// (track_colour.hip) share: the intensity of an RGB8 pixel, the integration pixel's look-up in a colour picture, the 2x2 level mean, the
// central-difference gradient, the bilinear tap and the photometric row with its additions to the 31 values.  Every operation is written as the
// specification states it; nothing here contracts.
#ifndef SCANFUSE_PHOTO_MATH_H
#define SCANFUSE_PHOTO_MATH_H

#include <hip/hip_runtime.h>

#include "fuser_internal.h"
#include "track_math.h"

namespace tk {

// intensity in [0, 1] of an RGB8 pixel
__device__ inline float intensity_rgb8(const uint8_t* __restrict__ q) {
  return ((0.299f * (float)q[0] + 0.587f * (float)q[1]) + 0.114f * (float)q[2]) / 255.0f;
}

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
  return intensity_rgb8(rgb + 3 * ((size_t)cy * (size_t)cw + (size_t)cx));
}

// the mean of a 2x2 block in the order (0,0), (1,0), (0,1), (1,1); invalid if one of the four is
__device__ inline float mean4(float s00, float s10, float s01, float s11) {
  return (s00 >= 0.0f && s10 >= 0.0f && s01 >= 0.0f && s11 >= 0.0f) ? (((s00 + s10) + s01) + s11) * 0.25f : -INFINITY;
}

// level L of a picture, recomputed from its RGB8 pixels: L nested 2x2 means
template <int L>
__device__ inline float level_intensity(const uint8_t* __restrict__ rgb, const ParamsK& P, int x, int y) {
  if constexpr (L == 0) {
    return intensity0_at(rgb, P, x, y);
  } else {
    const float s00 = level_intensity<L - 1>(rgb, P, 2 * x, 2 * y), s10 = level_intensity<L - 1>(rgb, P, 2 * x + 1, 2 * y);
    const float s01 = level_intensity<L - 1>(rgb, P, 2 * x, 2 * y + 1), s11 = level_intensity<L - 1>(rgb, P, 2 * x + 1, 2 * y + 1);
    return mean4(s00, s10, s01, s11);
  }
}

// {I, gx, gy, 0} of a pixel from its own intensity and its four neighbours' (xl, xr, yu, yd): central differences, -inf on the border (inner false)
// and where one of the four has no intensity
__device__ inline float4 photo_texel(float I, bool inner, float xl, float xr, float yu, float yd) {
  float4 o = make_float4(I, -INFINITY, -INFINITY, 0.0f);
  if (inner && xl >= 0.0f && xr >= 0.0f && yu >= 0.0f && yd >= 0.0f) {
    o.y = (xr - xl) * 0.5f;
    o.z = (yd - yu) * 0.5f;
  }
  return o;
}

// bilinear sample of one component: the two rows along x, then along y
__device__ inline float bilin(float t00, float t10, float t01, float t11, float ax, float ay) {
  const float top = fmaf(ax, t10 - t00, t00), bot = fmaf(ax, t11 - t01, t01);
  return fmaf(ay, bot - top, top);
}

// The colour row of a depth correspondence.  tmap: the target's {I, gx, gy, 0} map of camera c; Rt: the target's pose (its rotation carries the
// gradient to the world); Is: the source pixel's own intensity; p = T v (world), pc = M v (the target's camera; a correspondence has pc.z > 0).
// Where the pixel has a row: weight x (J_c J_c^T, J_c r_c) is added to acc[0..26] (weight 0: nothing is added, so the depth term's sums keep their
// bits), acc[29] = r_c^2 and acc[30] = 1.
template <int N>
__device__ inline void colour_row(const float4* __restrict__ tmap, const Cam& c, const Rows& Rt, float Is, float3 p, float3 pc, float weight,
                                  float colour_thres, float gradient_min, float (&acc)[N]) {
  static_assert(N >= TK_NSYS_RGBD, "the colour row's two sums follow the 29");
  const float uf = fmaf(pc.x / pc.z, c.fx, c.mx), vf = fmaf(pc.y / pc.z, c.fy, c.my);
  // the four taps (x0, y0) .. (x0 + 1, y0 + 1) lie inside the image: compared in float before any conversion, so that a huge or non-finite
  // projection forms no address
  if (Is >= 0.0f && uf >= 0.0f && uf < (float)(c.W - 1) && vf >= 0.0f && vf < (float)(c.H - 1)) {
    const float xf0 = floorf(uf), yf0 = floorf(vf);
    const float4* t = tmap + (size_t)((int)yf0 * c.W + (int)xf0);
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
        const float3 a = rot(Rt, g);
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

}  // namespace tk

#endif
