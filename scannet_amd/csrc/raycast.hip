// raycast.hip -- depth, world-normal and colour images of the fused volume seen from a camera (DESIGN.md "Ray casting").
//
// One lane per pixel, one wave per 8x8 pixel tile, four waves per workgroup (16x16 pixels): the rays of a wave stay close, so they probe the same
// blocks and read the same cache lines.  Every sample is a trilinear read of 8 voxels found through the hash table; each lane keeps the last block it
// looked up ({key, ptr}, a miss included), which answers the base corner of nearly every sample of a ray.  The kernel reads the volume and writes the
// images, nothing else: no atomics, no counters, the same bits from the same volume, poses and parameters.  tests/raycast_checker.c is the same
// arithmetic on the CPU over the blocks sf_fuser_export_blocks writes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "common.h"
#include "fuser_internal.h"
#include "hip_util.h"

namespace {

constexpr int RC_MAX_POSES = 32;   // poses per launch: their rows travel in the kernel arguments
constexpr double RC_MAX_SAMPLES = 65536.0;   // most samples a ray may take: parameters that would march further are refused

struct RayArgs {
  int W, H;
  float fx, fy, mx, my;
  float dmin, dmax;
  float delta;   // sample spacing: ray_increment_factor x trunc_base
  float thr_sample, thr_dist;   // thres_sample_dist_factor x delta, thres_dist_factor x delta
  float voxel;
  int refine;
  int kmax;      // samples k < kmax (sample_bound)
};
struct RayPoses {
  float T[RC_MAX_POSES][12];   // rows 0..2 of camToWorld
  uint32_t valid;              // bit j: pose j is not the -inf "tracking lost" pose
};

struct BlockCache {
  uint64_t key;
  int ptr;
};

__device__ inline int cached_slot(const HashEntry* __restrict__ table, const ParamsK& P, BlockCache& c, int bx, int by, int bz) {
  const uint64_t key = pack_key(bx, by, bz);
  if (key != c.key) {
    c.key = key;
    c.ptr = hash_lookup(table, P, bx, by, bz);
  }
  return c.ptr;
}

__device__ inline float lerp(float a, float b, float t) { return fmaf(t, b - a, a); }
__device__ inline float vsdf(uint2 v) { return __uint_as_float(v.x); }
__device__ inline float vch(uint2 v, int s) { return (float)((v.y >> s) & 0xFFu); }

// Trilinear sample at voxel coordinates q: false unless all 8 corner blocks exist and all 8 corner weights are > 0.
template <bool COLOR>
__device__ inline bool sample_q(const HashEntry* __restrict__ table, const uint2* __restrict__ vox, const ParamsK& P, BlockCache& bc, float qx, float qy,
                                float qz, float& sdf, float& cr, float& cg, float& cb) {
  const float flx = floorf(qx), fly = floorf(qy), flz = floorf(qz);
  const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
  const float tx = qx - flx, ty = qy - fly, tz = qz - flz;
  const int bx0 = ix >> 3, by0 = iy >> 3, bz0 = iz >> 3;
  const int bx1 = (ix + 1) >> 3, by1 = (iy + 1) >> 3, bz1 = (iz + 1) >> 3;
  const int lx0 = ix & 7, ly0 = iy & 7, lz0 = iz & 7;
  const int lx1 = (ix + 1) & 7, ly1 = (iy + 1) & 7, lz1 = (iz + 1) & 7;
  // each distinct corner block is looked up once: the base block through the lane's cache, the others (a corner across a block face) directly
  const int s000 = cached_slot(table, P, bc, bx0, by0, bz0);
  if (s000 < 0) return false;
  const bool sx = bx1 != bx0, sy = by1 != by0, sz = bz1 != bz0;
  const int s100 = sx ? hash_lookup(table, P, bx1, by0, bz0) : s000;
  const int s010 = sy ? hash_lookup(table, P, bx0, by1, bz0) : s000;
  const int s110 = sx && sy ? hash_lookup(table, P, bx1, by1, bz0) : (sx ? s100 : s010);
  const int s001 = sz ? hash_lookup(table, P, bx0, by0, bz1) : s000;
  const int s101 = sz ? (sx ? hash_lookup(table, P, bx1, by0, bz1) : s001) : s100;
  const int s011 = sz ? (sy ? hash_lookup(table, P, bx0, by1, bz1) : s001) : s010;
  const int s111 = sz ? (sx && sy ? hash_lookup(table, P, bx1, by1, bz1) : (sx ? s101 : s011)) : s110;
  if ((s100 | s010 | s110 | s001 | s101 | s011 | s111) < 0) return false;
  // the 8 voxel loads, all issued before the first use
  const uint2 v000 = vox[(size_t)s000 * 512 + (lz0 * 64 + ly0 * 8 + lx0)];
  const uint2 v100 = vox[(size_t)s100 * 512 + (lz0 * 64 + ly0 * 8 + lx1)];
  const uint2 v010 = vox[(size_t)s010 * 512 + (lz0 * 64 + ly1 * 8 + lx0)];
  const uint2 v110 = vox[(size_t)s110 * 512 + (lz0 * 64 + ly1 * 8 + lx1)];
  const uint2 v001 = vox[(size_t)s001 * 512 + (lz1 * 64 + ly0 * 8 + lx0)];
  const uint2 v101 = vox[(size_t)s101 * 512 + (lz1 * 64 + ly0 * 8 + lx1)];
  const uint2 v011 = vox[(size_t)s011 * 512 + (lz1 * 64 + ly1 * 8 + lx0)];
  const uint2 v111 = vox[(size_t)s111 * 512 + (lz1 * 64 + ly1 * 8 + lx1)];
  const uint32_t wmin = min(min(min(v000.y >> 24, v100.y >> 24), min(v010.y >> 24, v110.y >> 24)),
                            min(min(v001.y >> 24, v101.y >> 24), min(v011.y >> 24, v111.y >> 24)));
  if (wmin == 0u) return false;
  // x first, then y, then z
  sdf = lerp(lerp(lerp(vsdf(v000), vsdf(v100), tx), lerp(vsdf(v010), vsdf(v110), tx), ty),
             lerp(lerp(vsdf(v001), vsdf(v101), tx), lerp(vsdf(v011), vsdf(v111), tx), ty), tz);
  if (COLOR) {
#define SF_RC_CH(out, s)                                                                                                  \
  out = lerp(lerp(lerp(vch(v000, s), vch(v100, s), tx), lerp(vch(v010, s), vch(v110, s), tx), ty),                        \
             lerp(lerp(vch(v001, s), vch(v101, s), tx), lerp(vch(v011, s), vch(v111, s), tx), ty), tz)
    SF_RC_CH(cr, 0);
    SF_RC_CH(cg, 8);
    SF_RC_CH(cb, 16);
#undef SF_RC_CH
  }
  return true;
}

__global__ void __launch_bounds__(256) k_raycast(const HashEntry* __restrict__ table, const uint2* __restrict__ vox, const ParamsK P, const RayArgs A,
                                                 const RayPoses poses, float* __restrict__ out_depth, float* __restrict__ out_normal,
                                                 uint8_t* __restrict__ out_rgb) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= A.W || y >= A.H) return;
  const int j = blockIdx.z;
  const size_t px = (size_t)j * A.W * A.H + (size_t)y * A.W + x;
  float depth = -INFINITY, nx = -INFINITY, ny = -INFINITY, nz = -INFINITY;
  uint32_t rgb = 0u;
  if ((poses.valid >> j) & 1u) {
    const float* T = poses.T[j];
    const float cx = ((float)x - A.mx) / A.fx, cy = ((float)y - A.my) / A.fy;
    const float rho = sqrtf(cx * cx + cy * cy + 1.0f);
    const float ux = cx / rho, uy = cy / rho, uz = 1.0f / rho;
    const float wx = T[0] * ux + T[1] * uy + T[2] * uz;
    const float wy = T[4] * ux + T[5] * uy + T[6] * uz;
    const float wz = T[8] * ux + T[9] * uy + T[10] * uz;
    const float ox = T[3], oy = T[7], oz = T[11];
    const float lam0 = A.dmin * rho, lam_end = A.dmax * rho;
    const float yv = recip_rn(A.voxel);
    BlockCache bc{KEY_EMPTY, -1};
    float dummy0, dummy1, dummy2;
    bool prev_ok = false;
    float prev_s = 0.0f, prev_lam = 0.0f;
    for (int k = 0; k < A.kmax; k++) {
      const float lam = fmaf((float)k, A.delta, lam0);
      if (!(lam <= lam_end)) break;
      float s;
      const bool ok = sample_q<false>(table, vox, P, bc, div_rn(fmaf(lam, wx, ox), A.voxel, yv), div_rn(fmaf(lam, wy, oy), A.voxel, yv),
                                      div_rn(fmaf(lam, wz, oz), A.voxel, yv), s, dummy0, dummy1, dummy2);
      if (ok && prev_ok && prev_s > 0.0f && s <= 0.0f && fabsf(prev_s - s) < A.thr_sample && fabsf(s) < A.thr_dist) {
        // regula falsi between the bracketing samples; an invalid sample on the way makes the pixel a miss
        float la = prev_lam, sa = prev_s, lb = lam, sb = s, c = lam;
        bool hit = true;
        for (int it = 0; it < A.refine; it++) {
          c = la + (sa / (sa - sb)) * (lb - la);
          float sc;
          if (!sample_q<false>(table, vox, P, bc, div_rn(fmaf(c, wx, ox), A.voxel, yv), div_rn(fmaf(c, wy, oy), A.voxel, yv),
                               div_rn(fmaf(c, wz, oz), A.voxel, yv), sc, dummy0, dummy1, dummy2)) {
            hit = false;
            break;
          }
          if (sa * sc > 0.0f) { la = c; sa = sc; }
          else { lb = c; sb = sc; }
        }
        if (hit) {
          const float qx = div_rn(fmaf(c, wx, ox), A.voxel, yv), qy = div_rn(fmaf(c, wy, oy), A.voxel, yv), qz = div_rn(fmaf(c, wz, oz), A.voxel, yv);
          float sc, cr = 0.0f, cg = 0.0f, cb = 0.0f;
          sample_q<true>(table, vox, P, bc, qx, qy, qz, sc, cr, cg, cb);   // the last refinement sample again: valid, same bits
          depth = c / rho;
          rgb = (uint32_t)(uint8_t)(cr + 0.5f) | ((uint32_t)(uint8_t)(cg + 0.5f) << 8) | ((uint32_t)(uint8_t)(cb + 0.5f) << 16);
          if (out_normal) {
            float sxp, sxm, syp, sym, szp, szm;
            bool nok = sample_q<false>(table, vox, P, bc, qx + 1.0f, qy, qz, sxp, dummy0, dummy1, dummy2);
            nok = nok && sample_q<false>(table, vox, P, bc, qx - 1.0f, qy, qz, sxm, dummy0, dummy1, dummy2);
            nok = nok && sample_q<false>(table, vox, P, bc, qx, qy + 1.0f, qz, syp, dummy0, dummy1, dummy2);
            nok = nok && sample_q<false>(table, vox, P, bc, qx, qy - 1.0f, qz, sym, dummy0, dummy1, dummy2);
            nok = nok && sample_q<false>(table, vox, P, bc, qx, qy, qz + 1.0f, szp, dummy0, dummy1, dummy2);
            nok = nok && sample_q<false>(table, vox, P, bc, qx, qy, qz - 1.0f, szm, dummy0, dummy1, dummy2);
            if (nok) {
              const float dx = sxp - sxm, dy = syp - sym, dz = szp - szm;
              const float len = sqrtf(dx * dx + dy * dy + dz * dz);
              if (len > 0.0f) { nx = dx / len; ny = dy / len; nz = dz / len; }
            }
          }
        }
        break;   // a refined crossing ends the march, hit or miss
      }
      prev_ok = ok;
      prev_s = s;
      prev_lam = lam;
    }
  }
  if (out_depth) out_depth[px] = depth;
  if (out_normal) {
    out_normal[3 * px] = nx;
    out_normal[3 * px + 1] = ny;
    out_normal[3 * px + 2] = nz;
  }
  if (out_rgb) {
    out_rgb[3 * px] = (uint8_t)rgb;
    out_rgb[3 * px + 1] = (uint8_t)(rgb >> 8);
    out_rgb[3 * px + 2] = (uint8_t)(rgb >> 16);
  }
}

// what can be checked without a fuser
int check_params(const sf_raycast_params* r) {
  if (!r) return sf::fail(SF_ERR_INVALID_ARG, "NULL ray-cast parameters");
  if (r->width < 0 || r->height < 0 || (r->width > 0) != (r->height > 0)) return sf::fail(SF_ERR_INVALID_ARG, "ray-cast image %d x %d", r->width, r->height);
  if (!std::isfinite(r->depth_min) || !std::isfinite(r->depth_max) || !(r->depth_min < r->depth_max))
    return sf::fail(SF_ERR_INVALID_ARG, "ray-cast depth range [%g, %g]", r->depth_min, r->depth_max);
  if (r->refine_iters < 1 || r->refine_iters > 8) return sf::fail(SF_ERR_INVALID_ARG, "refine_iters %d (1..8)", r->refine_iters);
  if (!std::isfinite(r->ray_increment_factor) || !(r->ray_increment_factor > 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "ray increment factor %g: not a positive finite number", r->ray_increment_factor);
  if (!std::isfinite(r->thres_sample_dist_factor) || !std::isfinite(r->thres_dist_factor))
    return sf::fail(SF_ERR_INVALID_ARG, "ray threshold factors %g, %g: not finite", r->thres_sample_dist_factor, r->thres_dist_factor);
  return SF_OK;
}

// K, the bound on the samples of every ray of the image: ceil((depth_max - depth_min) * rho_max / delta) + 2 in double, rho_max the ray
// length factor of the image's farthest corner.  Where the depth range ends first -- every sensible parameter set -- K never binds; it makes a march
// of any length impossible, and a K above RC_MAX_SAMPLES (a vanishing increment, a huge depth range) is refused.  tests/raycast_checker.c has the same.
int sample_bound(const RayArgs& a, int* kmax) {
  const double ax = std::fmax(std::fabs(0.0 - (double)a.mx), std::fabs((double)(a.W - 1) - (double)a.mx)) / std::fabs((double)a.fx);
  const double ay = std::fmax(std::fabs(0.0 - (double)a.my), std::fabs((double)(a.H - 1) - (double)a.my)) / std::fabs((double)a.fy);
  const double n = ((double)a.dmax - (double)a.dmin) * std::sqrt(ax * ax + ay * ay + 1.0) / (double)a.delta;
  if (!(n <= RC_MAX_SAMPLES))
    return sf::fail(SF_ERR_INVALID_ARG, "a ray would take %g samples (limit %g): depth range [%g, %g] at a spacing of %g m", n, RC_MAX_SAMPLES, a.dmin, a.dmax, a.delta);
  *kmax = (int)std::ceil(n) + 2;
  return SF_OK;
}

// defaults filled in and checked; the kernel's constants
int resolve(const sf_fuser* f, const sf_raycast_params* r, RayArgs* a) {
  int rc = check_params(r);
  if (rc != SF_OK) return rc;
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  a->W = r->width > 0 || r->height > 0 ? r->width : f->pk.W;
  a->H = r->width > 0 || r->height > 0 ? r->height : f->pk.H;
  if (a->W <= 0 || a->H <= 0) return sf::fail(SF_ERR_INVALID_ARG, "ray-cast image %d x %d", a->W, a->H);
  if (r->fx == 0.0f && r->fy == 0.0f && r->mx == 0.0f && r->my == 0.0f) {
    const float sx = (float)a->W / (float)f->pk.W, sy = (float)a->H / (float)f->pk.H;
    a->fx = f->pk.fx * sx; a->mx = f->pk.mx * sx;
    a->fy = f->pk.fy * sy; a->my = f->pk.my * sy;
  } else {
    a->fx = r->fx; a->fy = r->fy; a->mx = r->mx; a->my = r->my;
  }
  if (!(a->fx != 0.0f && a->fy != 0.0f) || !std::isfinite(a->fx) || !std::isfinite(a->fy) || !std::isfinite(a->mx) || !std::isfinite(a->my))
    return sf::fail(SF_ERR_INVALID_ARG, "ray-cast intrinsics %g, %g, %g, %g", a->fx, a->fy, a->mx, a->my);
  a->dmin = r->depth_min;
  a->dmax = r->depth_max;
  a->delta = r->ray_increment_factor * f->p.trunc_base;
  if (!(a->delta > 0.0f) || !std::isfinite(a->delta)) return sf::fail(SF_ERR_INVALID_ARG, "non-positive ray increment %g x %g", r->ray_increment_factor, f->p.trunc_base);
  a->thr_sample = r->thres_sample_dist_factor * a->delta;
  a->thr_dist = r->thres_dist_factor * a->delta;
  a->voxel = f->pk.voxel;
  a->refine = r->refine_iters;
  return sample_bound(*a, &a->kmax);
}

// a pose whose rows hold anything but finite numbers (the all -inf "tracking lost" pose among them) gives an all-miss image
bool pose_usable(const float* T) {
  for (int i = 0; i < 12; i++)
    if (!std::isfinite(T[i])) return false;
  return true;
}

}  // namespace

// f->stream waits for what both front streams hold so far: whatever reads the frames' effect on f->stream comes behind every frame queued on the handle
int sf_order_behind_fronts(sf_fuser* f) {
  for (hipEvent_t& e : f->ev_raycast)
    if (!e) SF_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const hipStream_t fronts[2] = {f->front, f->front_lo};
  for (int i = 0; i < 2; i++)
    if (fronts[i]) {
      SF_HIP_CHECK(hipEventRecord(f->ev_raycast[i], fronts[i]));
      SF_HIP_CHECK(hipStreamWaitEvent(f->stream, f->ev_raycast[i], 0));
    }
  return SF_OK;
}

// the counterpart, after sf_order_behind_fronts: both front streams wait for what f->stream holds so far
int sf_order_fronts_behind(sf_fuser* f) {
  SF_HIP_CHECK(hipEventRecord(f->ev_raycast[2], f->stream));
  for (hipStream_t s : {f->front, f->front_lo})
    if (s) SF_HIP_CHECK(hipStreamWaitEvent(s, f->ev_raycast[2], 0));
  return SF_OK;
}

SF_API int sf_fuser_raycast_size(sf_fuser* f, const sf_raycast_params* r, int32_t* width, int32_t* height) {
  RayArgs a;
  const int rc = resolve(f, r, &a);
  if (rc != SF_OK) return rc;
  if (width) *width = a.W;
  if (height) *height = a.H;
  return SF_OK;
}

SF_API int sf_fuser_raycast_device(sf_fuser* f, const float* poses, uint64_t n, const sf_raycast_params* r, void* d_depth, void* d_normals_xyz, void* d_rgb) {
  RayArgs a;
  const int rc = resolve(f, r, &a);
  if (rc != SF_OK) return rc;
  if (!poses && n) return sf::fail(SF_ERR_INVALID_ARG, "NULL poses");
  if (n == 0 || (!d_depth && !d_normals_xyz && !d_rgb)) return SF_OK;
  SF_HIP_CHECK(hipSetDevice(f->device));
  // behind every frame queued so far, on the main stream and on both front streams ...
  if (const int oc = sf_order_behind_fronts(f)) return oc;
  const size_t npx = (size_t)a.W * a.H;
  const dim3 grid((a.W + 15) / 16, (a.H + 15) / 16, 1);
  for (uint64_t j0 = 0; j0 < n; j0 += RC_MAX_POSES) {
    const int m = (int)(n - j0 < (uint64_t)RC_MAX_POSES ? n - j0 : RC_MAX_POSES);
    RayPoses rp;
    std::memset(&rp, 0, sizeof(rp));
    for (int j = 0; j < m; j++) {
      const float* T = poses + 16 * (j0 + j);
      if (!pose_usable(T)) continue;
      std::memcpy(rp.T[j], T, 12 * sizeof(float));
      rp.valid |= 1u << j;
    }
    hipLaunchKernelGGL(k_raycast, dim3(grid.x, grid.y, m), dim3(256), 0, f->stream, f->table, reinterpret_cast<const uint2*>(f->voxels), f->pk, a, rp,
                       d_depth ? (float*)d_depth + j0 * npx : nullptr, d_normals_xyz ? (float*)d_normals_xyz + 3 * j0 * npx : nullptr,
                       d_rgb ? (uint8_t*)d_rgb + 3 * j0 * npx : nullptr);
    SF_HIP_CHECK(hipGetLastError());
  }
  // ... and ahead of everything queued later: the next frame's allocation must not insert into the table while the kernel reads it
  return sf_order_fronts_behind(f);
}

SF_API int sf_fuser_raycast(sf_fuser* f, const float pose[16], const sf_raycast_params* r, float* depth, float* normals_xyz, uint8_t* rgb) {
  RayArgs a;
  const int rc = resolve(f, r, &a);
  if (rc != SF_OK) return rc;
  if (!pose) return sf::fail(SF_ERR_INVALID_ARG, "NULL pose");
  if (!depth && !normals_xyz && !rgb) return SF_OK;
  SF_HIP_CHECK(hipSetDevice(f->device));
  const size_t npx = (size_t)a.W * a.H;
  const size_t bytes = npx * 4 + (normals_xyz ? npx * 12 : 0) + (rgb ? npx * 3 : 0);
  sf::DevBuf own;
  SF_HIP_CHECK(own.alloc(bytes));
  uint8_t* buf = own.as<uint8_t>();
  float* d_depth = (float*)buf;   // always made: the other two follow it
  float* d_nrm = normals_xyz ? (float*)(buf + npx * 4) : nullptr;
  uint8_t* d_rgb = rgb ? buf + npx * 4 + (normals_xyz ? npx * 12 : 0) : nullptr;
  int out = sf_fuser_raycast_device(f, pose, 1, r, d_depth, d_nrm, d_rgb);
  hipError_t e = hipSuccess;
  if (out == SF_OK && depth) e = hipMemcpyAsync(depth, d_depth, npx * 4, hipMemcpyDeviceToHost, f->stream);
  if (out == SF_OK && e == hipSuccess && normals_xyz) e = hipMemcpyAsync(normals_xyz, d_nrm, npx * 12, hipMemcpyDeviceToHost, f->stream);
  if (out == SF_OK && e == hipSuccess && rgb) e = hipMemcpyAsync(rgb, d_rgb, npx * 3, hipMemcpyDeviceToHost, f->stream);
  const hipError_t e2 = hipStreamSynchronize(f->stream);
  if (out != SF_OK) return out;
  if (e != hipSuccess || e2 != hipSuccess) return sf::fail(SF_ERR_DEVICE, "ray-cast download failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  return SF_OK;
}
