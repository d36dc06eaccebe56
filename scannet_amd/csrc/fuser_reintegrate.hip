// fuser_reintegrate.hip -- re-integration of frames whose poses were revised (SURVEY App. C "deintegrate: used when a frame's pose is revised"; the
// trajectory-manager keys s_maxFrameFixes / s_topNActive / s_minPoseDistSqrt of Server/tools/recons/zParametersScanNet.txt:25-28).  k_reintegrate is
// stage 4 of a MIXED-SIGN pass: every slot of the pass either takes its image out of the tiles (the pose the volume holds) or puts it in (the revised
// pose), in slot order, with the tile in registers -- the tiles the old and the new view share are read and written once.  Around it: the planner of
// one trajectory-manager step (sf_reint_plan, host only) and the loop that decodes the planned frames of a .sens file and runs the passes
// (sf_fuse_update_trajectory).  The pass scheduler itself is run_batch (fuser.hip); DESIGN.md section 4d.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "fuser_device.h"
#include "fuser_fuse.h"
#include "fuser_internal.h"
#include "hip_util.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// K4r: the tile loop of k_integrate (fuser_integrate.hip) in which some slots subtract.  Slot q of the pass is "deintegrate image R.img[q] under
// pose B.Ti[q]" (bit q of R.neg set) or "integrate image R.img[q] under B.Ti[q]"; the two slots of a moved frame name ONE converted image.  The slot
// mask of a tile comes from the same compaction as a frame mask (every slot has a sequence number in slot order: a block born in a + slot is seen by
// the slots behind it, - slots included, and by none before it), the sign of a slot is a bit of a kernel argument: the choice between the two update
// bodies is a scalar branch around straight-line code, never a per-lane select.
//   + body: fuse_update<+1> exactly as the multi-frame pass of k_integrate runs it (WM 2 / XR: table reciprocal, v_lerp_u8 colour, x-row lanes) where the
//           parameters allow, the generic bodies (TAB / WM as sf_launch_integrate picks them) where not;
//   - body: fuse_update<-1>, the specification's plain update (two IEEE divisions per voxel pair, colour untouched, voxel zeroed at weight <= 0) on the
//           depth plane alone -- the pre-pass writes the metres of an RGB-D frame twice, beside the colour and on their own.
// Tiles go back whole when some slot changed them (ROWS false), as in the multi-frame pass.
// Registers: the two bodies are live one after the other, not together, so the budget is the larger body's -- see DESIGN.md 4d for the figures
// tests/test_reintegrate_plan.py holds the kernel to.  The + body keeps the select tail of fuse_update (PRED false): with the predicated write-back of
// k_integrate the colour x-row variant needs 96 registers and spills four.
// ---------------------------------------------------------------------------------------------------
constexpr int REINT_WAVES = 5;   // workgroups (of 4 waves) per CU = waves per SIMD the register budget is set for: k_integrate's

template <int COLOR, bool TAB, int WM, bool XR>
__global__ __launch_bounds__(256, REINT_WAVES) void k_reintegrate(uint4* __restrict__ voxels, const uint64_t* __restrict__ block_keys,
                                                                  const int32_t* __restrict__ compact, const uint32_t* __restrict__ cmask,
                                                                  const float* __restrict__ depthf_all, const uint2* __restrict__ texel_all,
                                                                  int32_t* counters, int32_t* host_mirror, int compact_counter, int xcd_walk, ParamsK P,
                                                                  BatchTi B, ReintSlots R) {
  __shared__ float s_rtab[RTAB];  // correctly rounded 1/m for the weighted-mean division of the + body
  if (TAB) {
    for (int i = threadIdx.x; i < RTAB; i += 256) s_rtab[i] = 1.0f / (float)(i > 0 ? i : 1);
    __syncthreads();
  }
  constexpr int WMN = WM == 3 ? 3 : 0;   // the - body: depth-dependent observation weight or the generic one (what deintegration runs)
  const int n = counters[compact_counter];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    atomicExch(&counters[C_LAST_BLOCKS], counters[compact_counter + 1]);
    if (host_mirror) *host_mirror = n;
  }
  const int lx = XR ? 0 : (2 * lane) & 7;
  const int ly = XR ? lane & 7 : (lane >> 2) & 7;
  const int lzb = XR ? lane >> 3 : lane >> 5;
  const size_t npx = (size_t)P.W * P.H;
  // the list walk of k_integrate: each XCD one contiguous eighth
  const int wg_total = (n + 3) >> 2;
  const int chunk = xcd_walk ? (wg_total + 7) >> 3 : wg_total;
  const int lanes = xcd_walk ? 8 : 1;
  const int sub = xcd_walk ? (int)(blockIdx.x & 7) : 0;
  const int per_sub = max(1, (int)gridDim.x / lanes);
  for (int loc = xcd_walk ? (int)(blockIdx.x >> 3) : (int)blockIdx.x; loc < chunk; loc += per_sub) {
    const int i = ((sub * chunk + loc) << 2) + wave;
    if (i >= n) continue;
    const int slot = compact[i];
    uint32_t slots = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmask[i]);  // wave-uniform: the slot loop runs on the scalar unit
    int bx, by, bz;
    unpack_key(block_keys[slot], bx, by, bz);
    uint4* vb = voxels + (size_t)slot * 256;
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = vb[XR ? lane * 4 + j : j * 64 + lane];
    const v2f wx = {(float)(8 * bx + lx) * P.voxel, (float)(8 * bx + lx + 1) * P.voxel};
    const float wy = (float)(8 * by + ly) * P.voxel;
    float wz[4];
    v2f wxp[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      wz[j] = (float)(8 * bz + (XR ? 0 : 2 * j) + lzb) * P.voxel;
      wxp[j] = v2f{(float)(8 * bx + 2 * j) * P.voxel, (float)(8 * bx + 2 * j + 1) * P.voxel};
    }
    uint64_t dirty[4] = {0ull, 0ull, 0ull, 0ull};
    while (slots != 0u) {
      const int q = __builtin_ctz(slots);
      slots &= slots - 1u;
      const float* Ti = B.Ti[q];
      const size_t im = (size_t)R.img[q];
      const float* __restrict__ depthf = depthf_all + im * npx;
      const uint2* __restrict__ texel = texel_all + im * npx;
      if ((R.neg >> q) & 1u) fuse_rows<-1, 0, false, WMN, 0, 4, false, XR>(P, Ti, depthf, texel, s_rtab, wx, wy, wz, wxp, v, dirty);
      else fuse_rows<1, COLOR, TAB, WM, 0, 4, false, XR, false>(P, Ti, depthf, texel, s_rtab, wx, wy, wz, wxp, v, dirty);   // PRED false: see above
    }
    if (dirty[0] != 0ull) {   // wave-uniform: some slot changed a voxel of this tile
#pragma unroll
      for (int j = 0; j < 4; j++) vb[XR ? lane * 4 + j : j * 64 + lane] = v[j];
    }
  }
}

struct ReintegrateLaunch {
  const sf_fuser* f;
  int sl;
  const BatchTi& bt;
  const ReintSlots& rs;
  hipStream_t s;

  template <int COLOR, bool TAB, int WM, bool XR>
  void run() const {
    const int grid = sf_list_grid(f, *f->host_mirror);
    hipLaunchKernelGGL((k_reintegrate<COLOR, TAB, WM, XR>), dim3(grid), dim3(256), 0, s, f->voxels, f->block_keys, f->compact2[sl], f->cmask2[sl],
                       f->depthf2[sl], f->color2[sl], f->counters, f->host_mirror, sf_compact_counter(sl), f->xcd_walk ? 1 : 0, f->pk, bt, rs);
  }
  template <bool TAB, int WM>
  void colour(bool col) const {
    if (col) run<1, TAB, WM, false>();
    else run<0, TAB, WM, false>();
  }
};

}  // namespace

// The variant of a mixed-sign pass, by the rules of sf_launch_integrate: the shipped parameters run the x-row layout with the table division and the
// saturating weight byte; colour_first 1, weight_sample != 1 and weight_mode 1 take the generic bodies of the same kernel.
void sf_launch_reintegrate(const sf_fuser* f, int sl, bool col, const BatchTi& bt, const ReintSlots& rs, hipStream_t s) {
  const ReintegrateLaunch L{f, sl, bt, rs, s};
  const bool ws1 = f->p.weight_sample == 1 && f->p.weight_mode == 0;
  const bool shipped = ws1 && f->pk.wmax == 255;
  const bool table = f->p.weight_sample >= 1 && f->p.weight_sample <= RTAB - 256 && f->p.weight_mode == 0;
  if (shipped) {
    if (!col) L.run<0, true, 2, true>();
    else if (f->p.colour_first) L.run<1, true, 2, false>();
    else L.run<2, true, 2, true>();
  }
  else if (ws1) L.colour<true, 1>(col);
  else if (table) L.colour<true, 0>(col);
  else if (f->p.weight_mode == 1) L.colour<false, 3>(col);
  else L.colour<false, 0>(col);
}

// ======================================================================================================
// One step of the trajectory manager (host only, double precision): which frames to re-integrate next.
// ======================================================================================================
namespace {

bool pose_lost(const float* p) {
  for (int i = 0; i < 16; i++)
    if (p[i] != -INFINITY) return false;
  return true;
}

// d^2 = |t_b - t_a|^2 + angle(R_a^T R_b)^2.  The angle as atan2(sin, cos) of M = R_a^T R_b -- sin from the antisymmetric part, cos from the trace --: exact 0 for
// identical poses (M is then symmetric bit for bit, whatever the float rotation's distance from orthonormal), and accurate for the small angles a drift consists of
double pose_dist2(const float* a, const float* b) {
  double d2 = 0.0, M[3][3];
  for (int r = 0; r < 3; r++) {
    const double dt = (double)b[4 * r + 3] - (double)a[4 * r + 3];
    d2 += dt * dt;
  }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0.0;
      for (int k = 0; k < 3; k++) s += (double)a[4 * k + i] * (double)b[4 * k + j];
      M[i][j] = s;
    }
  const double x = M[2][1] - M[1][2], y = M[0][2] - M[2][0], z = M[1][0] - M[0][1];
  const double sn = 0.5 * std::sqrt((x * x + y * y) + z * z);
  const double cs = 0.5 * (((M[0][0] + M[1][1]) + M[2][2]) - 1.0);
  const double th = std::atan2(sn, cs);
  return d2 + th * th;
}

}  // namespace

SF_API int sf_reint_plan(const float* integrated_poses, const float* target_poses, uint64_t n, const sf_reint_params* rp, uint64_t* frames_out,
                         uint64_t capacity, uint64_t* n_out) {
  if ((!integrated_poses || !target_poses) && n > 0) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (!rp || !n_out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (rp->max_frame_fixes < 0 || rp->top_n_active < 0 || !(rp->min_pose_dist_sqrt >= 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_reint_plan: max_frame_fixes %d, top_n_active %d, min_pose_dist_sqrt %g", rp->max_frame_fixes, rp->top_n_active,
                    (double)rp->min_pose_dist_sqrt);
  std::vector<std::pair<double, uint64_t>> cand;
  for (uint64_t i = 0; i < n; i++) {
    const float* a = integrated_poses + 16 * i;
    const float* b = target_poses + 16 * i;
    const bool la = pose_lost(a), lb = pose_lost(b);
    if (la && lb) continue;
    const double d2 = (la || lb) ? (double)INFINITY : pose_dist2(a, b);
    if (d2 > (double)rp->min_pose_dist_sqrt) cand.emplace_back(d2, i);   // (a NaN distance -- a pose that is no rigid motion -- is no candidate)
  }
  std::sort(cand.begin(), cand.end(), [](const std::pair<double, uint64_t>& x, const std::pair<double, uint64_t>& y) {
    return x.first > y.first || (x.first == y.first && x.second < y.second);
  });
  const uint64_t keep = std::min<uint64_t>(std::min<uint64_t>(cand.size(), (uint64_t)rp->top_n_active), (uint64_t)rp->max_frame_fixes);
  *n_out = keep;
  if (keep > capacity) return sf::fail(SF_ERR_BOUNDS, "sf_reint_plan: %llu frames planned, room for %llu", (unsigned long long)keep, (unsigned long long)capacity);
  if (keep > 0 && !frames_out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  for (uint64_t k = 0; k < keep; k++) frames_out[k] = cand[k].second;
  return SF_OK;
}

// ======================================================================================================
// The trajectory manager's loop over a .sens file: plan, decode the planned frames on a host pool, upload, re-integrate in plan order.
// ======================================================================================================
SF_API int sf_fuse_update_trajectory(sf_fuser* f, const struct sf_sens* s, float* integrated_poses, const float* target_poses, const sf_reint_params* rp,
                                     uint64_t max_steps, int with_colour, int decode_threads, sf_reint_stats* stats) {
  if (!f || !s || !integrated_poses || !target_poses || !rp) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const auto t0 = std::chrono::steady_clock::now();
  sf_reint_stats st;
  std::memset(&st, 0, sizeof(st));
  if (stats) *stats = st;
  sf_sens_info info;
  int rc = sf_sens_get_info(s, &info);
  if (rc != SF_OK) return rc;
  if ((int)info.depth_width != f->in_W || (int)info.depth_height != f->in_H)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_fuse_update_trajectory: the file's depth frames are %u x %u, the fuser was created for %d x %d", info.depth_width,
                    info.depth_height, f->in_W, f->in_H);
  const size_t npx = (size_t)f->pk.W * f->pk.H;
  const size_t cpx = f->pk.cW ? (size_t)f->pk.cW * f->pk.cH : npx;
  if (with_colour && (info.color_width == 0 || (size_t)info.color_width * info.color_height != cpx || (info.color_compression != 0 && info.color_compression != 2)))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_fuse_update_trajectory: the file's colour frames (%u x %u, compression %d) do not fit the fuser", info.color_width,
                    info.color_height, info.color_compression);
  const uint64_t n = info.num_frames;
  const size_t dbytes = f->in_px * 2, cbytes = cpx * 3;
  const uint64_t cap = (uint64_t)std::max(0, std::min(rp->max_frame_fixes, rp->top_n_active));
  std::vector<uint64_t> plan(cap ? cap : 1);
  std::vector<uint16_t> hd;
  std::vector<uint8_t> hc;
  std::vector<float> po, pn;
  sf::DevBuf d_depth, d_rgb;   // freed with the call, on every way out (hipFree waits for the passes that still read them)
  SF_HIP_CHECK(hipSetDevice(f->device));
  for (uint64_t step = 0; max_steps == 0 || step < max_steps; step++) {
    uint64_t m = 0;
    rc = sf_reint_plan(integrated_poses, target_poses, n, rp, plan.data(), cap, &m);
    if (rc != SF_OK) return rc;
    if (m == 0) break;
    if (!d_depth.p) {
      SF_HIP_CHECK(d_depth.alloc(dbytes * cap));
      if (with_colour) SF_HIP_CHECK(d_rgb.alloc(cbytes * cap));
      hd.resize(f->in_px * cap);
      if (with_colour) hc.resize(cbytes * cap);
      po.resize(16 * cap);
      pn.resize(16 * cap);
    }
    // decode: a pool takes the planned frames in turn
    int threads = decode_threads > 0 ? decode_threads : sf::usable_cpus();
    threads = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)threads, m, 32}));
    std::atomic<uint64_t> next{0};
    std::atomic<int> failed{SF_OK};
    auto work = [&]() {
      for (uint64_t k = next.fetch_add(1); k < m; k = next.fetch_add(1)) {
        int r = sf_sens_decode_depth(s, plan[k], hd.data() + f->in_px * k);
        if (r == SF_OK && with_colour) r = sf_sens_decode_color(s, plan[k], hc.data() + cbytes * k);
        if (r != SF_OK) failed.store(r);
      }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (failed.load() != SF_OK) return sf::fail(failed.load(), "sf_fuse_update_trajectory: a planned frame could not be decoded");
    for (uint64_t k = 0; k < m; k++) {
      std::memcpy(&po[16 * k], integrated_poses + 16 * plan[k], 64);
      std::memcpy(&pn[16 * k], target_poses + 16 * plan[k], 64);
    }
    // the buffers are reused by the next step: the passes of the step before have read them (the blocking copies below order behind nothing of the
    // fuser's own streams)
    if (step > 0) { rc = sf_fuser_sync(f); if (rc != SF_OK) return rc; }
    SF_HIP_CHECK(hipMemcpy(d_depth.p, hd.data(), dbytes * m, hipMemcpyHostToDevice));
    if (with_colour) SF_HIP_CHECK(hipMemcpy(d_rgb.p, hc.data(), cbytes * m, hipMemcpyHostToDevice));
    rc = sf_fuser_reintegrate_batch_device(f, d_depth.p, dbytes, with_colour ? d_rgb.p : nullptr, cbytes, po.data(), pn.data(), m);
    if (rc != SF_OK) { (void)sf_fuser_sync(f); return rc; }
    for (uint64_t k = 0; k < m; k++) {
      const bool lo = pose_lost(&po[16 * k]), ln = pose_lost(&pn[16 * k]);
      if (lo) st.frames_added++;
      else if (ln) st.frames_removed++;
      else st.frames_moved++;
      std::memcpy(integrated_poses + 16 * plan[k], &pn[16 * k], 64);
    }
    st.steps++;
    st.passes += (uint64_t)sf_fuser_reintegrate_passes(f);
  }
  rc = sf_fuser_sync(f);
  st.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (stats) *stats = st;
  return rc;
}
