// track.hip -- camera tracking against the fused volume: depth-only, frame-to-model, projective point-to-plane ICP over an image pyramid
// (DESIGN.md "Camera tracking").
//
// Per frame: the depth frame becomes metres at the integration size (the fuser's pre-pass rule), then a pyramid of 2x2 reductions with a vertex and
// a normal map per level; the volume is ray-cast once at the reference pose (raycast.hip, depth and normals) and turned into a world vertex map.
// Per iteration: k_track_assoc pairs every input pixel with the model pixel it projects to, builds its point-to-plane row and reduces the 29 values
// of the normal equations of its 256-pixel workgroup (xor butterfly in the wave, (w0 + w1) + (w2 + w3) across waves: no atomics); k_track_final
// sums the partials in index order in double.  The host solves the 6x6 system in double and updates the pose.  Every step is deterministic and
// tests/track_checker.c restates it bit for bit.  sf_fuser_track_rgbd* run the same host loop over the kernels' colour instantiation, which adds the
// dense colour term's row to every correspondence and two sums to the system's values (track_colour.hip makes the intensity maps).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "common.h"
#include "fuser_internal.h"
#include "hip_util.h"
#include "photo_math.h"
#include "scanfuse_internal.h"
#include "track_internal.h"
#include "track_math.h"

namespace {

using namespace tk;   // track_math.h: the rules shared with align.hip

struct AssocArgs {
  Cam c;
  int W0, shift;     // the model image (level 0) and the level's subsampling of it (the depth target)
  Rows T, M, Rref;   // the estimate (world), the estimate in the reference camera (T_ref^-1 T), the reference pose
  float dist_thres, normal_thres;
  float weight, colour_thres, gradient_min;   // the colour term's
};

// u16 frame at the input size -> metres at the integration size: k_prepass's rule (nearest resample, then the depth range)
__global__ void __launch_bounds__(256) k_track_depth0(const uint16_t* __restrict__ in, const ParamsK P, float* __restrict__ d0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P.W * P.H) return;
  d0[i] = depth0_at(in, P, i);
}

// one 2x2 reduction (track_math.h down4)
__global__ void __launch_bounds__(256) k_track_down(const float* __restrict__ src, int Ws, float* __restrict__ dst, int Wd, int Hd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Wd * Hd) return;
  const int x = i % Wd, y = i / Wd;
  const float* s = src + (size_t)(2 * y) * Ws + 2 * x;
  dst[i] = down4(s[0], s[1], s[Ws], s[Ws + 1]);
}

// camera-space vertex and normal of every pixel of a level; x = -inf where invalid (track_math.h vertex_normal)
__global__ void __launch_bounds__(256) k_track_vn(const float* __restrict__ d, const Cam c, float4* __restrict__ vmap, float4* __restrict__ nmap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.W * c.H) return;
  const int x = i % c.W, y = i / c.W;
  const float dz = d[i];
  const bool nb = dz > 0.0f && x + 1 < c.W && y + 1 < c.H;
  float4 vo, no;
  vertex_normal(c, x, y, dz, nb, nb ? d[i + 1] : 0.0f, nb ? d[i + c.W] : 0.0f, &vo, &no);
  vmap[i] = vo;
  nmap[i] = no;
}

// the ray-cast image (level 0) as world vertices T_ref * unproject(depth) and world normals; x = -inf where either is missing
__global__ void __launch_bounds__(256) k_track_model(const float* __restrict__ md, const float* __restrict__ mn, const Cam c, const Rows Tref,
                                                     float4* __restrict__ mq, float4* __restrict__ mnorm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.W * c.H) return;
  const float dz = md[i];
  const float nx = mn[3 * (size_t)i], ny = mn[3 * (size_t)i + 1], nz = mn[3 * (size_t)i + 2];
  float4 q = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f), n = q;
  if (dz > 0.0f && nx > -INFINITY) {
    const float3 p = xf(Tref, unproject(c, i % c.W, i / c.W, dz));
    q = make_float4(p.x, p.y, p.z, 0.0f);
    n = make_float4(nx, ny, nz, 0.0f);
  }
  mq[i] = q;
  mnorm[i] = n;
}

// one level's association and point-to-plane rows, reduced to one 29-float partial per 256-pixel workgroup.  COLOUR: 31 floats, with the colour row of
// the correspondence against the model's map of the level in the same lane; photo_in == nullptr: no colour rows
template <bool COLOUR>
__global__ void __launch_bounds__(256) k_track_assoc(const float4* __restrict__ vmap, const float4* __restrict__ nmap, const float4* __restrict__ mq,
                                                     const float4* __restrict__ mnorm, const float4* __restrict__ photo_in,
                                                     const float4* __restrict__ photo_model, const AssocArgs A, float* __restrict__ partials,
                                                     uint8_t* __restrict__ mask) {
  constexpr int N = nsys_of<COLOUR>;
  __shared__ float red[4][N];
  const int i = blockIdx.x * 256 + threadIdx.x;
  float acc[N];
#pragma unroll
  for (int k = 0; k < N; k++) acc[k] = 0.0f;
  if (i < A.c.W * A.c.H) {
    const float4 v4 = vmap[i];
    // the depth target is the model image (level 0) subsampled; its normal is read only where its vertex is valid
    const bool ok = correspond(A.c, A.T, A.M, v4, nmap[i], A.dist_thres, A.normal_thres, [&](int ux, int uy, float3* q, float3* nm) {
      const size_t j = (size_t)(uy << A.shift) * A.W0 + (ux << A.shift);
      const float4 q4 = mq[j];
      if (!(q4.x > -INFINITY)) return false;
      const float4 m4 = mnorm[j];
      *q = make_float3(q4.x, q4.y, q4.z);
      *nm = make_float3(m4.x, m4.y, m4.z);
      return true;
    }, acc);
    if constexpr (COLOUR) {
      if (ok && photo_in) {
        const float Is = photo_in[i].x;
        const float3 v = make_float3(v4.x, v4.y, v4.z);
        colour_row(photo_model, A.c, A.Rref, Is, xf(A.T, v), xf(A.M, v), A.weight, A.colour_thres, A.gradient_min, acc);
      }
    }
    if (mask) mask[i] = ok ? 1 : 0;
  }
  reduce256(acc, red, partials + (size_t)blockIdx.x * TK_PSTRIDE);
}

// the workgroups' partials summed in index order, in double: lane k sums value k
template <bool COLOUR>
__global__ void __launch_bounds__(64) k_track_final(const float* __restrict__ partials, int nb, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k < nsys_of<COLOUR>) out[k] = sum_partials(partials, nb, k);
}

}  // namespace

void sf_track_release(sf_fuser* f) {
  if (!f) return;
  delete f->track;
  f->track = nullptr;
}

namespace {

// what can be checked without a fuser
int check_track_params(const sf_track_params* t) {
  if (!t) return sf::fail(SF_ERR_INVALID_ARG, "NULL tracking parameters");
  if (t->levels < 1 || t->levels > TK_MAX_LEVELS) return sf::fail(SF_ERR_INVALID_ARG, "tracking levels %d (1..4)", t->levels);
  for (int l = 0; l < t->levels; l++) {
    if (t->max_iters[l] < 1 || t->max_iters[l] > 100) return sf::fail(SF_ERR_INVALID_ARG, "max_iters[%d] = %d (1..100)", l, t->max_iters[l]);
    if (!std::isfinite(t->dist_thres[l]) || !(t->dist_thres[l] > 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "dist_thres[%d] = %g: not a positive finite number", l, t->dist_thres[l]);
    if (!(t->normal_thres[l] >= -1.0f && t->normal_thres[l] <= 1.0f)) return sf::fail(SF_ERR_INVALID_ARG, "normal_thres[%d] = %g (-1..1)", l, t->normal_thres[l]);
  }
  if (!std::isfinite(t->early_out) || !(t->early_out >= 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "early_out %g: not a finite number >= 0", t->early_out);
  if (t->min_correspondences < 6) return sf::fail(SF_ERR_INVALID_ARG, "min_correspondences %d (>= 6)", t->min_correspondences);
  if (!std::isfinite(t->max_translation) || !(t->max_translation > 0.0f) || !std::isfinite(t->max_rotation) || !(t->max_rotation > 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "motion bound %g m, %g rad: not positive finite numbers", t->max_translation, t->max_rotation);
  const sf_raycast_params& r = t->raycast;
  if (r.width != 0 || r.height != 0 || r.fx != 0.0f || r.fy != 0.0f || r.mx != 0.0f || r.my != 0.0f)
    return sf::fail(SF_ERR_INVALID_ARG, "tracking ray cast: the image size and intrinsics must be 0 (the integration camera)");
  return SF_OK;
}

// the colour term's three parameters and its picture, which only the rgbd entry points read
int check_colour_args(const sf_track_params* t, const void* rgb) {
  if (!std::isfinite(t->colour_weight) || !(t->colour_weight >= 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "tracking colour_weight %g: not a finite number >= 0", t->colour_weight);
  if (!std::isfinite(t->colour_thres) || !(t->colour_thres >= 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "tracking colour_thres %g: not a finite number >= 0", t->colour_thres);
  if (!std::isfinite(t->colour_gradient_min) || !(t->colour_gradient_min >= 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "tracking colour_gradient_min %g: not a finite number >= 0", t->colour_gradient_min);
  if (!rgb && t->colour_weight > 0.0f) return sf::fail(SF_ERR_INVALID_ARG, "tracking colour_weight %g without a colour picture", t->colour_weight);
  return SF_OK;
}

// the buffers of `levels` levels, made on first use and again only when more levels are asked for than the set holds
int ensure_work(sf_fuser* f, const Cam* cams, int levels) {
  if (f->track && f->track->levels >= levels) return SF_OK;
  sf_track_release(f);
  TrackWork* w = f->track = new TrackWork();
  w->levels = levels;
  const size_t n0 = (size_t)cams[0].W * cams[0].H;
  hipError_t e = w->d_in.reserve(f->in_px * sizeof(uint16_t));
  const auto dev = [&e](sf::DevBuf& b, size_t bytes) { if (e == hipSuccess) e = b.reserve(bytes); };
  for (int l = 0; l < levels; l++) {
    const size_t n = (size_t)cams[l].W * cams[l].H;
    dev(w->depth[l], n * sizeof(float));
    dev(w->vmap[l], n * sizeof(float4));
    dev(w->nmap[l], n * sizeof(float4));
  }
  dev(w->model_depth, n0 * sizeof(float));
  dev(w->model_normal, n0 * 3 * sizeof(float));
  dev(w->mq, n0 * sizeof(float4));
  dev(w->mn, n0 * sizeof(float4));
  dev(w->partials, ((n0 + 255) / 256) * TK_PSTRIDE * sizeof(float));
  dev(w->d_sys, TK_PSTRIDE * sizeof(double));
  dev(w->d_mask, n0);
  if (e == hipSuccess) e = w->h_sys.reserve(TK_PSTRIDE * sizeof(double));
  if (e != hipSuccess) { sf_track_release(f); return sf::fail(SF_ERR_DEVICE, "tracking buffers: %s", hipGetErrorString(e)); }
  return SF_OK;
}

Rows rows_of(const float* T) {
  Rows r;
  std::memcpy(r.T, T, sizeof(r.T));
  return r;
}

// the input pyramid of a frame in HBM and the model of the volume at T_ref, queued on f->stream
// d_rgb: the frame's picture in HBM, and the model is cast with its colour; nullptr: depth only
int prepare(sf_fuser* f, const void* d_depth, const float* Tref, const sf_track_params* t, const Cam* cams, const void* d_rgb = nullptr) {
  TrackWork* w = f->track;
  const int n0 = cams[0].W * cams[0].H;
  hipLaunchKernelGGL(k_track_depth0, dim3((n0 + 255) / 256), dim3(256), 0, f->stream, (const uint16_t*)d_depth, f->pk, w->depth[0].as<float>());
  SF_HIP_CHECK(hipGetLastError());
  for (int l = 1; l < t->levels; l++) {
    const int n = cams[l].W * cams[l].H;
    hipLaunchKernelGGL(k_track_down, dim3((n + 255) / 256), dim3(256), 0, f->stream, w->depth[l - 1].as<const float>(), cams[l - 1].W, w->depth[l].as<float>(),
                       cams[l].W, cams[l].H);
    SF_HIP_CHECK(hipGetLastError());
  }
  for (int l = 0; l < t->levels; l++) {
    const int n = cams[l].W * cams[l].H;
    hipLaunchKernelGGL(k_track_vn, dim3((n + 255) / 256), dim3(256), 0, f->stream, w->depth[l].as<const float>(), cams[l], w->vmap[l].as<float4>(),
                       w->nmap[l].as<float4>());
    SF_HIP_CHECK(hipGetLastError());
  }
  // the ray cast orders itself behind both front streams and blocks later front-chain work (raycast.hip)
  const int rc = sf_fuser_raycast_device(f, Tref, 1, &t->raycast, w->model_depth.p, w->model_normal.p, d_rgb ? w->model_rgb.p : nullptr);
  if (rc != SF_OK) return rc;
  hipLaunchKernelGGL(k_track_model, dim3((n0 + 255) / 256), dim3(256), 0, f->stream, w->model_depth.as<const float>(), w->model_normal.as<const float>(), cams[0],
                     rows_of(Tref), w->mq.as<float4>(), w->mn.as<float4>());
  SF_HIP_CHECK(hipGetLastError());
  return d_rgb ? sf_track_photo_prepare(f, d_rgb, cams, t->levels) : SF_OK;
}

// one level's system at the estimate T (double, rows 0..2 used), summed into w->h_sys; the mask optionally into w->d_mask
// rgbd: the 31 values of the kernels' colour instantiation, with colour rows when photo
int system_at(sf_fuser* f, int l, const Cam* cams, const double* T, const double* Tref, const sf_track_params* t, bool want_mask, bool rgbd = false,
              bool photo = false) {
  TrackWork* w = f->track;
  AssocArgs A;
  A.c = cams[l];
  A.W0 = cams[0].W;
  A.shift = l;
  for (int i = 0; i < 12; i++) { A.T.T[i] = (float)T[i]; A.Rref.T[i] = (float)Tref[i]; }
  compose_ref(Tref, T, A.M.T);
  A.dist_thres = t->dist_thres[l];
  A.normal_thres = t->normal_thres[l];
  A.weight = t->colour_weight;
  A.colour_thres = t->colour_thres;
  A.gradient_min = t->colour_gradient_min;
  const int n = cams[l].W * cams[l].H, nb = (n + 255) / 256;
  hipLaunchKernelGGL(rgbd ? k_track_assoc<true> : k_track_assoc<false>, dim3(nb), dim3(256), 0, f->stream, w->vmap[l].as<const float4>(),
                     w->nmap[l].as<const float4>(), w->mq.as<const float4>(), w->mn.as<const float4>(), photo ? w->photo[0][l].as<const float4>() : nullptr,
                     photo ? w->photo[1][l].as<const float4>() : nullptr, A, w->partials.as<float>(), want_mask ? w->d_mask.as<uint8_t>() : nullptr);
  SF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rgbd ? k_track_final<true> : k_track_final<false>, dim3(1), dim3(64), 0, f->stream, w->partials.as<const float>(), nb, w->d_sys.as<double>());
  SF_HIP_CHECK(hipGetLastError());
  SF_HIP_CHECK(hipMemcpyAsync(w->h_sys.p, w->d_sys.p, (rgbd ? TK_NSYS_RGBD : TK_NSYS) * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(hipStreamSynchronize(f->stream));
  return SF_OK;
}

// the 6x6 system of the 29 values: A xi = -b
bool solve6(const double* sys, double* xi) {
  double A[6][6];
  int k = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) A[a][b] = A[b][a] = sys[k++];
  return solve_spd(&A[0][0], sys + 21, 6, xi);
}

// what the three entry points share: the checks in their order (own_checks: the caller's own, behind the NULL checks), the level cameras, the device, the
// buffers and, for a host frame, its copy into w->d_in
// rgbd: the call is one of sf_fuser_track_rgbd*; rgb (its picture, on the host when host_rgb) may still be NULL (colour_weight 0)
template <typename Checks>
int begin(sf_fuser* f, const sf_track_params* t, bool args_ok, Checks own_checks, Cam* cams, const uint16_t* host_depth, bool rgbd = false,
          const void* rgb = nullptr, bool host_rgb = false) {
  int rc = check_track_params(t);
  if (rc != SF_OK) return rc;
  if (rgbd && (rc = check_colour_args(t, rgb)) != SF_OK) return rc;
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  if (!args_ok) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if ((rc = own_checks()) != SF_OK) return rc;
  if (rgb && f->pk.cW > 0 && !(std::isfinite(f->pk.cfx) && f->pk.cfx > 0.0f && std::isfinite(f->pk.cfy) && f->pk.cfy > 0.0f && std::isfinite(f->pk.cmx) &&
                               std::isfinite(f->pk.cmy)))
    return sf::fail(SF_ERR_INVALID_ARG, "tracking with colour: the fuser's colour intrinsics (cfx %g, cfy %g, cmx %g, cmy %g) cannot map a %d x %d picture", f->pk.cfx,
                    f->pk.cfy, f->pk.cmx, f->pk.cmy, f->pk.cW, f->pk.cH);
  for (int l = 0; l < t->levels; l++)
    if (!level_cam(f->pk, l, &cams[l])) return sf::fail(SF_ERR_INVALID_ARG, "tracking level %d would be %d x %d (at least 8 x 8)", l, cams[l].W, cams[l].H);
  SF_HIP_CHECK(hipSetDevice(f->device));
  if ((rc = ensure_work(f, cams, t->levels)) != SF_OK) return rc;
  if (rgb && (rc = sf_track_photo_reserve(f, cams, t->levels)) != SF_OK) return rc;
  if (host_depth) SF_HIP_CHECK(hipMemcpyAsync(f->track->d_in.p, host_depth, f->in_px * sizeof(uint16_t), hipMemcpyHostToDevice, f->stream));
  if (rgb && host_rgb) SF_HIP_CHECK(hipMemcpyAsync(f->track->d_rgb.p, rgb, sf_track_picture_bytes(f), hipMemcpyHostToDevice, f->stream));
  return SF_OK;
}

// depth (and, for sf_fuser_track_rgbd*, the picture rgb or NULL): a frame in HBM (on_device) or on the host
int track(sf_fuser* f, const void* depth, bool on_device, const float* guess, const float* ref, const sf_track_params* t, float* pose_out, sf_track_result* res,
          bool rgbd = false, const void* rgb = nullptr) {
  Cam cams[TK_MAX_LEVELS];
  int rc = begin(f, t, depth && guess && pose_out, [] { return (int)SF_OK; }, cams, on_device ? nullptr : (const uint16_t*)depth, rgbd, rgb, !on_device);
  if (rc != SF_OK) return rc;
  const void* d_rgb = !rgb ? nullptr : (on_device ? rgb : f->track->d_rgb.p);
  sf_track_result r;
  std::memset(&r, 0, sizeof(r));
  for (int i = 0; i < 16; i++) pose_out[i] = -INFINITY;   // the "tracking lost" pose
  if (!ref) ref = guess;
  if (!finite12(guess) || !finite12(ref)) {
    r.lost_reason = 1;
    if (res) *res = r;
    return SF_OK;
  }
  if ((rc = prepare(f, on_device ? depth : f->track->d_in.p, ref, t, cams, d_rgb)) != SF_OK) return rc;
  double T[12], Tref[12], G[12];
  for (int i = 0; i < 12; i++) { T[i] = guess[i]; G[i] = guess[i]; Tref[i] = ref[i]; }
  const double* sys = f->track->h_sys.as<const double>();
  for (int l = t->levels - 1; l >= 0 && r.lost_reason == 0; l--) {
    for (int it = 0; it < t->max_iters[l]; it++) {
      if ((rc = system_at(f, l, cams, T, Tref, t, false, rgbd, d_rgb != nullptr)) != SF_OK) return rc;
      if (l == 0) {
        r.correspondences = (int32_t)sys[28];
        r.rms_residual = sys[28] > 0.0 ? (float)std::sqrt(sys[27] / sys[28]) : 0.0f;
        if (rgbd) {
          r.colour_correspondences = (int32_t)sys[30];
          r.colour_rms_residual = sys[30] > 0.0 ? (float)std::sqrt(sys[29] / sys[30]) : 0.0f;
        }
        if (sys[28] < (double)t->min_correspondences) { r.lost_reason = 2; break; }
      }
      double xi[6];
      if (!solve6(sys, xi)) { r.lost_reason = 3; break; }
      apply_update(xi, T);
      r.iterations[l]++;
      double mx = 0.0;
      for (int k = 0; k < 6; k++) mx = std::fmax(mx, std::fabs(xi[k]));
      if (mx < (double)t->early_out) break;
    }
  }
  if (r.lost_reason == 0 && !accept_pose(G, T, (double)t->max_translation, (double)t->max_rotation)) r.lost_reason = 4;
  if (r.lost_reason == 0) {
    r.tracked = 1;
    write_pose16(T, pose_out);
  }
  if (res) *res = r;
  return SF_OK;
}

}  // namespace

SF_API int sf_fuser_track_device(sf_fuser* f, const void* d_depth, const float guess[16], const float ref[16], const sf_track_params* t, float pose_out[16],
                                 sf_track_result* result) {
  return track(f, d_depth, true, guess, ref, t, pose_out, result);
}

SF_API int sf_fuser_track(sf_fuser* f, const uint16_t* depth, const float guess[16], const float ref[16], const sf_track_params* t, float pose_out[16],
                          sf_track_result* result) {
  return track(f, depth, false, guess, ref, t, pose_out, result);
}

namespace {

// sf_fuser_track_system and sf_fuser_track_rgbd_system (rgbd; its picture rgb may be NULL): one level's 29 or 31 values and optionally its mask
int system_export(sf_fuser* f, const uint16_t* depth, bool rgbd, const uint8_t* rgb, int level, const float* T, const float* T_ref, const sf_track_params* t,
                  double* sys, uint8_t* mask) {
  Cam cams[TK_MAX_LEVELS];
  int rc = begin(f, t, depth && T && T_ref && sys, [&] {
    if (level < 0 || level >= t->levels) return sf::fail(SF_ERR_INVALID_ARG, "level %d of %d", level, t->levels);
    if (!finite12(T) || !finite12(T_ref)) return sf::fail(SF_ERR_INVALID_ARG, "non-finite pose");
    return (int)SF_OK;
  }, cams, depth, rgbd, rgb, true);
  if (rc != SF_OK) return rc;
  TrackWork* w = f->track;
  if ((rc = prepare(f, w->d_in.p, T_ref, t, cams, rgb ? w->d_rgb.p : nullptr)) != SF_OK) return rc;
  double Td[12], Rd[12];
  for (int i = 0; i < 12; i++) { Td[i] = T[i]; Rd[i] = T_ref[i]; }
  if ((rc = system_at(f, level, cams, Td, Rd, t, mask != nullptr, rgbd, rgb != nullptr)) != SF_OK) return rc;
  for (int k = 0; k < (rgbd ? TK_NSYS_RGBD : TK_NSYS); k++) sys[k] = w->h_sys.as<const double>()[k];
  if (mask) SF_HIP_CHECK(hipMemcpy(mask, w->d_mask.p, (size_t)cams[level].W * cams[level].H, hipMemcpyDeviceToHost));
  return SF_OK;
}

}  // namespace

SF_API int sf_fuser_track_system(sf_fuser* f, const uint16_t* depth, int level, const float T[16], const float T_ref[16], const sf_track_params* t,
                                 double sys[29], uint8_t* mask) {
  return system_export(f, depth, false, nullptr, level, T, T_ref, t, sys, mask);
}

SF_API int sf_fuser_track_rgbd_device(sf_fuser* f, const void* d_depth, const void* d_rgb, const float guess[16], const float ref[16], const sf_track_params* t,
                                      float pose_out[16], sf_track_result* result) {
  return track(f, d_depth, true, guess, ref, t, pose_out, result, true, d_rgb);
}

SF_API int sf_fuser_track_rgbd(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float guess[16], const float ref[16], const sf_track_params* t,
                               float pose_out[16], sf_track_result* result) {
  return track(f, depth, false, guess, ref, t, pose_out, result, true, rgb);
}

SF_API int sf_fuser_track_rgbd_system(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, int level, const float T[16], const float T_ref[16],
                                      const sf_track_params* t, double sys[31], uint8_t* mask) {
  return system_export(f, depth, true, rgb, level, T, T_ref, t, sys, mask);
}
