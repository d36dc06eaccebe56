// fuser.hip -- voxel-hash TSDF fusion for gfx950 (MI355X), host side: create / destroy / reset, the batch scheduler (run_batch: slots, streams,
// events), the integrate entry points, tuning, statistics and profiling.  The kernels live with their launchers, one stage per file:
// fuser_prepass.hip (depth pre-pass), fuser_alloc.hip (sparse block allocation), fuser_compact.hip (frustum compaction), fuser_integrate.hip
// (integrate / deintegrate), fuser_blocks.hip (garbage collection, block export / import); fuser_device.h holds what several of them share.
// At the end of this file: the stage hooks of the front chain (sf_fuser_stage_*, scanfuse_internal.h), which run one stage of a pass for the tests.
//
// Replaces the scene-representation part of the external DepthSensing.exe / FriedLiver.exe that the
// reference pipeline shells out to (Server/scan_processor.py:126,138); the arithmetic is the specification
// in DESIGN.md section 3, reproduced operation for operation so that the voxels are
// bit-identical to the CPU checker's.  Built with -ffp-contract=off: every fmaf() of these files is a deliberate
// fused multiply-add of the spec, nothing else is contracted.
//
// Data layout in HBM:
//   table      HashEntry[num_buckets * bucket_size]   16 B: {u64 key (3 x 21-bit block coords), i32 heap block, u32 birth frame}
//   block_keys u64[num_sdf_blocks]                    directory: key of the block living in heap slot i, or EMPTY
//   heap       i32[num_sdf_blocks] + free counter     free list of heap slots (wave-aggregated pops)
//   voxels     8 B x 512 x num_sdf_blocks             {f32 sdf; u8 r,g,b,weight}, one 4 KiB tile per block, index z*64+y*8+x
//   depthf     f32[B][W*H], texel {f32 depth, rgb8} [B][W*H]   pre-pass outputs of the B <= 32 frames of a batch (L2 / Infinity-Cache resident); the
//                                                             texel plane only for RGB-D batches: ONE 8-byte gather per voxel and frame fetches both
//   compact    i32[num_sdf_blocks] + u32 mask         heap slots of the blocks some frame of the batch sees; bit j = frame j updates it
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "codecs_internal.h"
#include "fuser_internal.h"
#include "hip_util.h"
#include "jpeg_idct.h"

// ======================================================================================================
// host side
// ======================================================================================================
hipError_t sf_quiesce(sf_fuser* f) {
  hipError_t e = hipSuccess;
  if (f->front) e = hipStreamSynchronize(f->front);
  if (f->front_lo) { const hipError_t e1 = hipStreamSynchronize(f->front_lo); if (e == hipSuccess) e = e1; }
  const hipError_t e2 = hipStreamSynchronize(f->stream);
  return e != hipSuccess ? e : e2;
}

namespace {

// per-frame constants in double, rounded once to float.
bool frame_setup(const sf_params& p, const float* pose, FrameK& f) {
  if (pose[0] == -INFINITY) return false;
  for (int i = 0; i < 12; i++) f.T[i] = pose[i];
  const double a00 = pose[0], a01 = pose[1], a02 = pose[2], t0 = pose[3];
  const double a10 = pose[4], a11 = pose[5], a12 = pose[6], t1 = pose[7];
  const double a20 = pose[8], a21 = pose[9], a22 = pose[10], t2 = pose[11];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double inv[9] = {c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det,
                         c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det,
                         c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det};
  for (int r = 0; r < 3; r++) {
    const double ti = -(inv[3 * r] * t0 + inv[3 * r + 1] * t1 + inv[3 * r + 2] * t2);
    f.Ti[4 * r] = (float)inv[3 * r];
    f.Ti[4 * r + 1] = (float)inv[3 * r + 1];
    f.Ti[4 * r + 2] = (float)inv[3 * r + 2];
    f.Ti[4 * r + 3] = (float)ti;
  }
  const double rad = 4.0 * std::sqrt(3.0) * (double)p.voxel_size;
  f.radius = (float)rad;
  const double fx = p.fx, fy = p.fy, mx = p.mx, my = p.my;
  // lower planes at u = -1.5: the voxel rule casts (int)(u + 0.5f) before it tests the pixel, and the cast truncates (-1, 0) to pixel 0
  // (DESIGN.md 3.2 / 3.5); the block test must keep every block the voxel rule would touch
  const double xl = mx + 1.5, xh = ((double)p.depth_width - 0.5) - mx;
  const double yl = my + 1.5, yh = ((double)p.depth_height - 0.5) - my;
  f.xa[0] = (float)fx;  f.xc[0] = (float)xl; f.xr[0] = (float)(rad * std::sqrt(fx * fx + xl * xl));
  f.xa[1] = (float)-fx; f.xc[1] = (float)xh; f.xr[1] = (float)(rad * std::sqrt(fx * fx + xh * xh));
  f.ya[0] = (float)fy;  f.yc[0] = (float)yl; f.yr[0] = (float)(rad * std::sqrt(fy * fy + yl * yl));
  f.ya[1] = (float)-fy; f.yc[1] = (float)yh; f.yr[1] = (float)(rad * std::sqrt(fy * fy + yh * yh));
  f.zfar = p.max_integration_dist + std::fmaf(p.trunc_scale, p.max_integration_dist, p.trunc_base);
  return true;
}

}  // namespace

// Whether the next frame's pre-pass / allocation / compaction should run on the front stream beside the persistent kernel.  Measured on
// MI355X (profiles/r02): at 4 mm (48-67 k tiles per frame, front kernels 36 us) running them beside k_integrate_pipe stretches it by more
// than it hides (7.8 k frames/s serial, 7.5 k overlapped, also with the two streams on disjoint CU masks); at 1 mm (1.7 M tiles, front
// kernels 1 ms) it hides 0.5 ms per frame (310 vs 269 frames/s).  So: overlap once the previous pass's tile set is beyond 512 MiB.
// The same size also turns k_integrate_pipe's tile traffic non-temporal (twice the Infinity Cache: DESIGN.md 5.2).
bool sf_big_tile_set(uint32_t tiles) { return (uint64_t)tiles * 4096ull > (512ull << 20); }
bool sf_big_pass(const sf_fuser* f) { return sf_big_tile_set((uint32_t)*f->host_mirror); }
// One frame per launch without colour runs the persistent k_integrate_pipe (sf_pipe_batch), which fills every CU: kernels of the next frame
// on the front stream would only get CUs by starving some of its waves (measured: 113 us overlapped vs 90 us alone, and no
// more frames/s), so such a batch goes down ONE stream, pre-pass to integrate.
// The decision is latched at the end of every pass (run_batch) so that a caller's staging (sf_input_stream) and the pass that follows see the
// same answer: host_mirror is written by the device while they run.
bool sf_single_stream_batch(const sf_fuser* f, int n, bool color, int sign) { return sf_pipe_batch(f, n, color, sign) && !f->pipe_beside; }
// the stream the pre-pass of such a batch reads its frames on: where callers must have staged them
hipStream_t sf_input_stream(const sf_fuser* f, int n, bool color, int sign) {
  if (!f->overlap || sf_single_stream_batch(f, n, color, sign)) return f->stream;
  // The front stream has the device's highest priority: in a pass of several frames its short kernels must slip in between the workgroups of the integrate
  // kernel, or the next pass waits for them.  Beside the PERSISTENT kernel of one frame per launch (1 mm voxels: the tile set is far beyond the cache) that
  // priority is what the integrate kernel pays for: the allocation's 72 KiB workgroups, dispatched first, take the LDS its third workgroup per CU needs until
  // they are through -- 0.54 of peak HBM shipped and 322-335 frames/s, against 0.60-0.61 / 360 with the front chain at the MAIN stream's priority and 0.62 / 369
  // at the device's lowest (profiles/r06_alloc_1mm.txt: two or three runs each, nothing else changed).  So such a frame's front chain goes down a second
  // front stream, `front_lo` (front_prio -1, the default; 1 / 0: always the high-priority / always the second one), at the device's lowest priority.  One thing to
  // know about that: the first stream of a priority class makes the runtime open that class's hardware queues for the life of the PROCESS, and a later sf_fuse_run
  // in the same process -- seven to nine busy streams -- then runs 12 % slower (depth-only end to end 34.2 k -> 30.0 k frames/s; bench.py therefore runs its 1 mm
  // leg last).  A process that does both sets front_lo_lowest 0: the second stream at the main stream's priority, 0.60-0.61 here instead of 0.62.
  const bool lo = f->front_lo != nullptr && (f->front_prio == 0 || (f->front_prio < 0 && sf_pipe_batch(f, n, color, sign)));
  return lo ? f->front_lo : f->front;
}

namespace {

// One batch: n <= f->batch frames with valid poses, all with or all without colour.  The front stream prepares
// batch slot `sl` (pre-pass, allocation, compaction for all n frames, three launches) while the back stream is
// still fusing the previous batch out of the other slot.  Allocation only touches new hash entries / heap slots,
// integrate only the tiles of its own compact list, so the two never write the same data; slot reuse is ordered
// by ev_fused[sl].
// A MIXED-SIGN pass (rs != nullptr; sf_fuser_reintegrate_batch_device): the n poses are the pass's slots, slot q deintegrates (bit q of
// rs->neg) or integrates the pre-pass plane rs->img[q]; d_depth / d_rgb name the n_planes >= n frames the pre-pass converts, plane by plane -- a - slot's own
// plane is the fuser's frame of zeros, so that the allocation, which walks plane q for slot q, finds nothing to allocate there --, sign = +1 when some slot
// integrates (the allocation runs), -1 when none does, colour as rs_col says.  Everything else -- slots, streams, events, sequence numbers -- is the same pass.
int run_batch(sf_fuser* f, const void* const* d_depth, const void* const* d_rgb, const float* const* poses, int n, int sign, const void* const* d_lay = nullptr,
              const ReintSlots* rs = nullptr, int n_planes = 0, bool rs_col = false) {
  BatchIn in;
  BatchFrames bf;
  BatchTi bt;
  std::memset(&in, 0, sizeof(in));
  std::memset(&bf, 0, sizeof(bf));
  std::memset(&bt, 0, sizeof(bt));
  bf.n = n;
  bf.seq0 = f->frame_seq;
  const bool col = rs ? rs_col : (d_rgb != nullptr && d_rgb[0] != nullptr);
  for (int j = 0; j < n; j++) {
    if (!frame_setup(f->p, poses[j], bf.f[j])) return sf::fail(SF_ERR_INVALID_ARG, "run_batch: invalid pose in batch");
    std::memcpy(bt.Ti[j], bf.f[j].Ti, sizeof(bt.Ti[j]));
    in.depth[j] = (const uint16_t*)d_depth[j];
    in.rgb[j] = col ? (const uint8_t*)d_rgb[j] : nullptr;
    in.lay[j] = (col && d_lay) ? (const uint8_t*)d_lay[j] : nullptr;
  }
  for (int j = n; j < n_planes; j++) {   // images only - slots read
    in.depth[j] = (const uint16_t*)d_depth[j];
    in.rgb[j] = col ? (const uint8_t*)d_rgb[j] : nullptr;
  }
  f->frame_seq += (uint32_t)n;
  const int sl = f->slot;
  f->slot ^= 1;
  hipStream_t s = f->stream;
  hipStream_t sa = sf_input_stream(f, n, col, sign);  // callers stage the batch's frames on this stream too
  if (f->overlap && sa != s) {
    if (f->last_front != nullptr && f->last_front != sa) {   // the other front stream served the pass before: this pass's front chain starts behind that one's
      (void)hipEventRecord(f->ev_front_switch, f->last_front);
      (void)hipStreamWaitEvent(sa, f->ev_front_switch, 0);
    }
    f->last_front = sa;
    if (f->serial_tail) {  // single-stream batches came before: the front stream starts behind everything they queued
      (void)hipEventRecord(f->ev_input, s);
      (void)hipStreamWaitEvent(sa, f->ev_input, 0);
      f->serial_tail = false;
    }
    (void)hipStreamWaitEvent(sa, f->ev_fused[sl], 0);
  }
  // one colourless frame at the integration size through the ray-space allocation kernel: that kernel converts the depth itself
  const bool fuse_pre = f->alloc_ray && n == 1 && sign > 0 && !col && f->pk.inW == 0 && !rs;
  if (!fuse_pre) sf_launch_prepass(f, sl, rs ? n_planes : n, in, sa);
  if (sign > 0) sf_launch_alloc(f, sl, n, bf, in, sa, fuse_pre);
  sf_launch_compact(f, sl, bf, sa);
  if (f->overlap && sa != s) {
    (void)hipEventRecord(f->ev_compact[sl], sa);
    (void)hipStreamWaitEvent(s, f->ev_compact[sl], 0);
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (f->profile) {
    if (f->events_used == f->events.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return sf::fail(SF_ERR_DEVICE, "hipEventCreate failed");
      f->events.emplace_back(a, b);
    }
    e0 = f->events[f->events_used].first;
    e1 = f->events[f->events_used].second;
    f->events_used++;
    (void)hipEventRecord(e0, s);
  }
  if (rs) sf_launch_reintegrate(f, sl, col, bt, *rs, s);
  else sf_launch_integrate(f, sl, n, sign, col, bt, s);
  if (f->profile) (void)hipEventRecord(e1, s);
  if (f->overlap && sa != s) (void)hipEventRecord(f->ev_fused[sl], s);
  if (f->overlap && sa == s) f->serial_tail = true;  // no cross-stream traffic at all while single-stream batches follow each other
  f->pipe_beside = f->pipe_overlap == 1 || (f->pipe_overlap < 0 && sf_big_pass(f));
  if ((f->pipe_beside || f->front_prio == 0) && f->front_lo == nullptr && f->overlap) {   // the second front stream, on first need (sf_input_stream)
    int prio_lo = 0, prio_hi = 0;
    hipError_t e_ = hipSuccess;
    if (f->front_lo_lowest) {
      e_ = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
      if (e_ == hipSuccess) e_ = hipStreamCreateWithPriority(&f->front_lo, hipStreamNonBlocking, prio_lo);
    } else {
      e_ = hipStreamCreateWithFlags(&f->front_lo, hipStreamNonBlocking);   // the main stream's priority
    }
    if (e_ != hipSuccess) {
      f->front_lo = nullptr;   // (the high-priority one serves)
      (void)hipGetLastError();
    }
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return sf::fail(SF_ERR_DEVICE, "kernel launch failed: %s", hipGetErrorString(err));
  f->frames_integrated += (uint64_t)n;
  return SF_OK;
}

int run_frame(sf_fuser* f, const void* d_depth, const void* d_rgb, const float* pose, int sign) {
  if (pose[0] == -INFINITY) {
    f->frames_skipped++;
    return sf::fail(SF_ERR_SKIPPED, "frame skipped: camToWorld is -inf (tracking lost)");
  }
  const void* dd[1] = {d_depth};
  const void* dr[1] = {d_rgb};
  const float* pp[1] = {pose};
  return run_batch(f, dd, dr, pp, 1, sign);
}

}  // namespace

SF_API int sf_device_count(int* count) {
  if (!count) return sf::fail(SF_ERR_INVALID_ARG, "count is NULL");
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return sf::fail(SF_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *count = n;
  return SF_OK;
}

SF_API int sf_fuser_create(const sf_params* p, int device, sf_fuser** out) {
  if (!p || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (p->depth_width <= 0 || p->depth_height <= 0 || !(p->voxel_size > 0) || p->hash_num_buckets == 0 || p->hash_bucket_size == 0 ||
      p->num_sdf_blocks == 0 || !(p->fx > 0) || !(p->fy > 0) || !(p->depth_shift > 0))
    return sf::fail(SF_ERR_INVALID_ARG, "invalid reconstruction parameters");
  if (p->color_width > 0 && p->color_height > 0 && !(p->cfx > 0 && p->cfy > 0))
    return sf::fail(SF_ERR_INVALID_ARG, "colour resolution given without colour intrinsics");
  if ((p->integration_width > 0) != (p->integration_height > 0) || p->integration_width == 1 || p->integration_height == 1 ||
      (p->integration_width > 0 && (p->depth_width < 2 || p->depth_height < 2)))
    return sf::fail(SF_ERR_INVALID_ARG, "integration size %d x %d", p->integration_width, p->integration_height);
  if ((p->frustum_mode | p->colour_round | p->colour_first | p->weight_mode | p->weight_wrap) & ~1)
    return sf::fail(SF_ERR_INVALID_ARG, "frustum_mode / colour_round / colour_first / weight_mode / weight_wrap must be 0 or 1");
  if (p->frustum_mode == 1 && !(p->depth_max > p->depth_min))
    return sf::fail(SF_ERR_INVALID_ARG, "frustum_mode 1 normalises z by the sensor depth range: depth_max must exceed depth_min");
  if ((uint64_t)p->hash_num_buckets * p->hash_bucket_size > 0x7FFFFFFFull || p->num_sdf_blocks > 0x3FFFFFFFu)
    return sf::fail(SF_ERR_INVALID_ARG, "hash table / heap too large for 32-bit slot indices");
  if (int rc = sf::open_device(device, SF_ERR_INVALID_ARG, "libscanfuse has no CPU fallback, the fuser needs an MI355X")) return rc;
  // (until round 6 the first fuser of a process started sf_fuse_run's side streams and rings on a background thread here -- 90 MB pinned and
  // 330 MB of device memory also for callers that never run a file.  A caller that will -- bin/depthsensing, bench.py, tools/e2e_bench.py -- asks with
  // sf_fuse_run_prepare(file, params, device) before this call; without it the first sf_fuse_run makes its set itself.)
  sf_fuser* f = new sf_fuser();
  // every failure below leaves through sf_fuser_destroy (streams, events, device and pinned allocations made so far)
#define SF_CREATE_CHECK(call)                                                                               \
  do {                                                                                                      \
    hipError_t e_ = (call);                                                                                 \
    if (e_ != hipSuccess) {                                                                                 \
      sf_fuser_destroy(f);                                                                                  \
      return sf::fail(SF_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_));                        \
    }                                                                                                       \
  } while (0)
  f->p = *p;
  if (f->p.weight_max > 255 && !f->p.weight_wrap) f->p.weight_max = 255;  // uchar weight saturates (SURVEY App. C decision)
  if (f->p.weight_max > 0x00FFFFFF) f->p.weight_max = 0x00FFFFFF;   // weight_wrap: "no limit" for an 8-bit sum; the clamp compare stays exact in 32 bits
  if (f->p.weight_max < 1) f->p.weight_max = 1;
  f->device = device;
  sf_alloc_choose_window(f, p);
  ParamsK& k = f->pk;
  k.W = p->depth_width; k.H = p->depth_height; k.fx = p->fx; k.fy = p->fy; k.mx = p->mx; k.my = p->my;
  k.inW = k.inH = 0; k.rsx = k.rsy = 1.0f;
  const bool resample = p->integration_width > 0 && p->integration_height > 0 &&
                        (p->integration_width != p->depth_width || p->integration_height != p->depth_height);
  if (resample) {
    // everything behind the pre-pass works at the integration size with the intrinsics that follow the resample
    k.inW = p->depth_width; k.inH = p->depth_height;
    k.W = p->integration_width; k.H = p->integration_height;
    k.rsx = (float)(k.inW - 1) / (float)(k.W - 1);
    k.rsy = (float)(k.inH - 1) / (float)(k.H - 1);
    k.fx = p->fx * ((float)k.W / (float)k.inW); k.fy = p->fy * ((float)k.H / (float)k.inH);
    k.mx = p->mx * ((float)(k.W - 1) / (float)(k.inW - 1)); k.my = p->my * ((float)(k.H - 1) / (float)(k.inH - 1));
    f->p.depth_width = k.W; f->p.depth_height = k.H; f->p.fx = k.fx; f->p.fy = k.fy; f->p.mx = k.mx; f->p.my = k.my;   // frame_setup sees the integration camera
  }
  f->in_W = p->depth_width; f->in_H = p->depth_height;
  f->in_px = (size_t)p->depth_width * p->depth_height;
  k.depth_shift = p->depth_shift; k.dmin = p->depth_min; k.dmax = p->depth_max; k.voxel = p->voxel_size;
  k.tbase = p->trunc_base; k.tscale = p->trunc_scale; k.maxd = p->max_integration_dist;
  k.wsample = p->weight_sample; k.wmax = f->p.weight_max;
  k.num_buckets = p->hash_num_buckets; k.bucket_size = p->hash_bucket_size;
  k.total_slots = p->hash_num_buckets * p->hash_bucket_size; k.num_blocks = p->num_sdf_blocks;
  k.slab_axis = -1; k.slab_lo = 0; k.slab_hi = 0; k.slab_thick = 0; k.slab_world = 1; k.slab_rank = 0;
  k.cW = p->color_width > 0 && p->color_height > 0 ? p->color_width : 0;
  k.cH = k.cW ? p->color_height : 0;
  k.cfx = p->cfx; k.cfy = p->cfy; k.cmx = p->cmx; k.cmy = p->cmy;
  k.frustum_mode = p->frustum_mode; k.colour_round = p->colour_round; k.colour_first = p->colour_first; k.weight_mode = p->weight_mode;
  if (resample && k.cW == 0) {   // colour frames at the INPUT depth resolution: "their own resolution" as far as the integration camera is concerned
    k.cW = p->depth_width; k.cH = p->depth_height;
    k.cfx = p->fx; k.cfy = p->fy; k.cmx = p->mx; k.cmy = p->my;
  }
  hipDeviceProp_t prop;
  SF_CREATE_CHECK(hipGetDeviceProperties(&prop, device));
  f->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  f->compact_grid = (int)((k.num_blocks + 1023) / 1024);
  if (f->compact_grid > f->num_cus * 8) f->compact_grid = f->num_cus * 8;
  const size_t npx = (size_t)k.W * k.H;
#define SF_ALLOC(ptr, bytes)                                                                      \
  do {                                                                                            \
    hipError_t e_ = hipMalloc((void**)&(ptr), (bytes));                                           \
    if (e_ != hipSuccess) {                                                                       \
      sf_fuser_destroy(f);                                                                        \
      return sf::fail(SF_ERR_DEVICE, "hipMalloc(%zu bytes) failed: %s", (size_t)(bytes), hipGetErrorString(e_)); \
    }                                                                                             \
  } while (0)
  SF_CREATE_CHECK(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
  {
    // the front stream runs short latency-bound kernels that must slip in between the workgroups of the
    // bandwidth-bound integrate kernel: give it the highest priority the device offers
    int prio_lo = 0, prio_hi = 0;
    SF_CREATE_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    SF_CREATE_CHECK(hipStreamCreateWithPriority(&f->front, hipStreamNonBlocking, prio_hi));
    // (front_lo, the front chain's stream beside the persistent kernel, is made by the first pass that latches that schedule: a stream nobody uses still takes its turn
    // in the mapping of streams to hardware queues, and sf_fuse_run's seven to nine streams are short of those already)
    SF_CREATE_CHECK(hipEventCreateWithFlags(&f->ev_front_switch, hipEventDisableTiming));
  }
  for (int q = 0; q < 2; q++) {
    SF_CREATE_CHECK(hipEventCreateWithFlags(&f->ev_compact[q], hipEventDisableTiming));
    SF_CREATE_CHECK(hipEventCreateWithFlags(&f->ev_fused[q], hipEventDisableTiming));
  }
  SF_CREATE_CHECK(hipEventCreateWithFlags(&f->ev_input, hipEventDisableTiming));
  SF_ALLOC(f->table, (size_t)k.total_slots * sizeof(HashEntry));
  {
    // one entry per 8 heap blocks, 8 entries per line: 2 MB at 2^20 blocks (4 mm), 64 MB at 2^25 (1 mm) -- what a frame touches of it is ~100 x less than
    // the table entries it would probe
    uint32_t lines = 1024;
    while ((uint64_t)lines * 64ull < (uint64_t)k.num_blocks && lines < (1u << 24)) lines <<= 1;
    f->brick_lines = lines;
    SF_ALLOC(f->bricks, (size_t)lines * 8 * 16);
  }
  SF_ALLOC(f->heap, (size_t)k.num_blocks * 4);
  SF_ALLOC(f->block_keys, (size_t)k.num_blocks * 8);
  SF_ALLOC(f->block_entry, (size_t)k.num_blocks * 4);
  SF_ALLOC(f->block_flags, (size_t)k.num_blocks);
  SF_ALLOC(f->voxels, (size_t)k.num_blocks * 4096);
  for (int q = 0; q < 2; q++) {
    SF_ALLOC(f->depthf2[q], npx * 4 * MAX_BATCH);
    SF_ALLOC(f->color2[q], npx * 8 * MAX_BATCH);   // {depth, rgb} texels of an RGB-D batch
    SF_ALLOC(f->compact2[q], (size_t)k.num_blocks * 4);
    SF_ALLOC(f->cmask2[q], (size_t)k.num_blocks * 4);
  }
  f->compact = f->compact2[0];
  SF_ALLOC(f->counters, C_COUNT * 4);
  SF_ALLOC(f->ray_kx, (size_t)k.W * 4);
  SF_ALLOC(f->ray_ky, (size_t)k.H * 4);
  const size_t rgb_bytes = (k.cW ? (size_t)k.cW * k.cH : npx) * 3;
  for (int q = 0; q < sf_fuser::HOST_RING; q++) {
    SF_ALLOC(f->staging_depth[q], f->in_px * 2);
    SF_ALLOC(f->staging_rgb[q], rgb_bytes);
  }
#undef SF_ALLOC
  for (int q = 0; q < sf_fuser::HOST_RING; q++) {
    SF_CREATE_CHECK(hipHostMalloc(&f->pinned_depth[q], f->in_px * 2, hipHostMallocDefault));
    SF_CREATE_CHECK(hipHostMalloc(&f->pinned_rgb[q], rgb_bytes, hipHostMallocDefault));
    SF_CREATE_CHECK(hipEventCreateWithFlags(&f->ev_h2d[q], hipEventDisableTiming));
    SF_CREATE_CHECK(hipEventCreateWithFlags(&f->ev_consumed[q], hipEventDisableTiming));
  }
  SF_CREATE_CHECK(hipHostMalloc((void**)&f->host_mirror, 64, hipHostMallocMapped));
  *f->host_mirror = 0;
  SF_CREATE_CHECK(hipMemsetAsync(f->table, 0xFF, (size_t)k.total_slots * sizeof(HashEntry), f->stream));
  SF_CREATE_CHECK(hipMemsetAsync(f->bricks, 0, (size_t)f->brick_lines * 128, f->stream));
  SF_CREATE_CHECK(hipMemsetAsync(f->voxels, 0, (size_t)k.num_blocks * 4096, f->stream));
  SF_CREATE_CHECK(hipMemsetAsync(f->block_flags, 0, (size_t)k.num_blocks, f->stream));
  SF_CREATE_CHECK(hipMemsetAsync(f->counters, 0, C_COUNT * 4, f->stream));
  sf_launch_init_heap(f);
  sf_launch_ray_tables(f);
  const int32_t free0 = (int32_t)k.num_blocks;
  SF_CREATE_CHECK(hipMemcpyAsync(&f->counters[C_HEAP_FREE], &free0, 4, hipMemcpyHostToDevice, f->stream));
  SF_CREATE_CHECK(sf_quiesce(f));
#undef SF_CREATE_CHECK
  *out = f;
  return SF_OK;
}

SF_API void sf_fuser_destroy(sf_fuser* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->front) (void)hipStreamSynchronize(f->front);   // every stream drained before ANYTHING they read or write goes (the host-frame ring's
  if (f->front_lo) (void)hipStreamSynchronize(f->front_lo);
  if (f->stream) (void)hipStreamSynchronize(f->stream); // page-locked slots are read by copies queued on either of them)
  for (auto& e : f->events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  (void)hipFree(f->table); (void)hipFree(f->bricks); (void)hipFree(f->heap); (void)hipFree(f->block_keys); (void)hipFree(f->block_entry); (void)hipFree(f->block_flags); (void)hipFree(f->voxels);
  for (int q = 0; q < 2; q++) { (void)hipFree(f->depthf2[q]); (void)hipFree(f->color2[q]); (void)hipFree(f->compact2[q]); (void)hipFree(f->cmask2[q]); }
  (void)hipFree(f->counters); (void)hipFree(f->ray_kx); (void)hipFree(f->ray_ky); (void)hipFree(f->void_depth);
  for (int q = 0; q < 2; q++) { if (f->ev_compact[q]) (void)hipEventDestroy(f->ev_compact[q]); if (f->ev_fused[q]) (void)hipEventDestroy(f->ev_fused[q]); }
  if (f->ev_input) (void)hipEventDestroy(f->ev_input);
  if (f->front) { (void)hipStreamSynchronize(f->front); (void)hipStreamDestroy(f->front); }
  if (f->front_lo) { (void)hipStreamSynchronize(f->front_lo); (void)hipStreamDestroy(f->front_lo); }
  if (f->ev_front_switch) (void)hipEventDestroy(f->ev_front_switch);
  for (hipEvent_t e : f->ev_raycast) if (e) (void)hipEventDestroy(e);
  sf_track_release(f);
  sf_align_release(f);
  for (int q = 0; q < sf_fuser::HOST_RING; q++) {
    (void)hipFree(f->staging_depth[q]); (void)hipFree(f->staging_rgb[q]);
    if (f->pinned_depth[q]) (void)hipHostFree(f->pinned_depth[q]);
    if (f->pinned_rgb[q]) (void)hipHostFree(f->pinned_rgb[q]);
    if (f->ev_h2d[q]) (void)hipEventDestroy(f->ev_h2d[q]);
    if (f->ev_consumed[q]) (void)hipEventDestroy(f->ev_consumed[q]);
  }
  if (f->host_mirror) (void)hipHostFree(f->host_mirror);
  for (int q = 0; q < 2; q++) { if (f->mc_bounce[q]) (void)hipHostFree(f->mc_bounce[q]); if (f->mc_bounce_ev[q]) (void)hipEventDestroy(f->mc_bounce_ev[q]); }
  if (f->stream) (void)hipStreamDestroy(f->stream);
  delete f;
}

// Back to the state sf_fuser_create leaves: empty table, full heap, zeroed tiles (only the slots ever handed out are touched: a 4 mm room is
// ~0.5 GB of the 4.3 GB reserved), counters and frame numbering restarted; parameters, streams and tuning stay.  What the reference's tools do
// between two scans is to exit and start again (Server/scan_processor.py:137-141 runs one process per scan); a long-lived caller -- the scan
// queue of scannet_amd/shard.py, bench.py's repetitions -- keeps the 4+ GB allocation instead.
SF_API int sf_fuser_reset(sf_fuser* f) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  int32_t hw = 0;
  SF_HIP_CHECK(hipMemcpy(&hw, &f->counters[C_HIGH_WATER], 4, hipMemcpyDeviceToHost));
  const ParamsK& k = f->pk;
  if (hw < 0 || (uint32_t)hw > k.num_blocks) hw = (int32_t)k.num_blocks;
  SF_HIP_CHECK(hipMemsetAsync(f->table, 0xFF, (size_t)k.total_slots * sizeof(HashEntry), f->stream));
  SF_HIP_CHECK(hipMemsetAsync(f->bricks, 0, (size_t)f->brick_lines * 128, f->stream));
  if (hw > 0) {
    SF_HIP_CHECK(hipMemsetAsync(f->voxels, 0, (size_t)hw * 4096, f->stream));
    SF_HIP_CHECK(hipMemsetAsync(f->block_flags, 0, (size_t)hw, f->stream));
  }
  SF_HIP_CHECK(hipMemsetAsync(f->counters, 0, C_COUNT * 4, f->stream));
  sf_launch_init_heap(f);
  const int32_t free0 = (int32_t)k.num_blocks;
  SF_HIP_CHECK(hipMemcpyAsync(&f->counters[C_HEAP_FREE], &free0, 4, hipMemcpyHostToDevice, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  *f->host_mirror = 0;
  f->frame_seq = 1;
  f->slot = 0;
  f->serial_tail = false;
  f->pipe_beside = f->pipe_overlap == 1;
  f->frames_integrated = f->frames_skipped = 0;
  f->events_used = 0;
  return SF_OK;
}

// The caller's buffers are ordinary (pageable) memory and are its own again the moment the call returns -- a live stream decodes the next
// frame into the same buffer, a binding may free it.  So the frame is copied into a page-locked slot of the ring HERE, on the caller's
// thread (614 KB: ~50 us), and everything behind that -- H2D, pre-pass, allocation, compaction, integrate -- is queued and left running.
// Round 2 drained both streams and waited for the H2D in every call: the GPU idled while the host copied and the host idled while the GPU
// fused (one frame per launch: 7.8 k frames/s with resident frames, less through this entry point).
// in_stream: the stream the pre-pass will read the frame on.  *slot: f->staging_depth / f->staging_rgb [*slot] hold the frame in stream order.
static int stage_host_frame(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, hipStream_t in_stream, int* slot) {
  const size_t npx = (size_t)f->pk.W * f->pk.H;
  const size_t rgb_bytes = (f->pk.cW ? (size_t)f->pk.cW * f->pk.cH : npx) * 3;
  const int q = f->host_slot;
  f->host_slot = (q + 1) % sf_fuser::HOST_RING;
  const bool reused = f->host_frames >= (uint64_t)sf_fuser::HOST_RING;
  if (reused) SF_HIP_CHECK(hipEventSynchronize(f->ev_h2d[q]));   // the copy of HOST_RING frames ago has read the slot
  std::memcpy(f->pinned_depth[q], depth, f->in_px * 2);
  if (rgb) std::memcpy(f->pinned_rgb[q], rgb, rgb_bytes);
  if (reused) SF_HIP_CHECK(hipStreamWaitEvent(in_stream, f->ev_consumed[q], 0));   // the kernels that read the device copy
  SF_HIP_CHECK(hipMemcpyAsync(f->staging_depth[q], f->pinned_depth[q], f->in_px * 2, hipMemcpyHostToDevice, in_stream));
  if (rgb) SF_HIP_CHECK(hipMemcpyAsync(f->staging_rgb[q], f->pinned_rgb[q], rgb_bytes, hipMemcpyHostToDevice, in_stream));
  SF_HIP_CHECK(hipEventRecord(f->ev_h2d[q], in_stream));
  *slot = q;
  return SF_OK;
}

// ... and the slot handed back once its frame's launches are queued: the pre-pass (the only reader of the device copy) precedes the integrate launch in
// stream order, so an event behind that launch covers it
static int retire_host_frame(sf_fuser* f, int slot) {
  SF_HIP_CHECK(hipEventRecord(f->ev_consumed[slot], f->stream));
  f->host_frames++;
  return SF_OK;
}

static int fuse_host(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float* pose, int sign) {
  if (!f || !depth || !pose) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (pose[0] == -INFINITY) { f->frames_skipped++; return sf::fail(SF_ERR_SKIPPED, "frame skipped: camToWorld is -inf (tracking lost)"); }
  SF_HIP_CHECK(hipSetDevice(f->device));
  int q = 0;
  const int rs = stage_host_frame(f, depth, rgb, sf_input_stream(f, 1, rgb != nullptr, sign), &q);
  if (rs != SF_OK) return rs;
  const int rc = run_frame(f, f->staging_depth[q], rgb ? f->staging_rgb[q] : nullptr, pose, sign);
  const int rr = retire_host_frame(f, q);
  return rr != SF_OK ? rr : rc;
}

SF_API int sf_fuser_integrate(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float pose[16]) {
  return fuse_host(f, depth, rgb, pose, +1);
}
SF_API int sf_fuser_deintegrate(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float pose[16]) {
  return fuse_host(f, depth, rgb, pose, -1);
}
SF_API int sf_fuser_integrate_device(sf_fuser* f, const void* d_depth, const void* d_rgb, const float pose[16]) {
  if (!f || !d_depth || !pose) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  return run_frame(f, d_depth, d_rgb, pose, +1);
}
SF_API int sf_fuser_deintegrate_device(sf_fuser* f, const void* d_depth, const void* d_rgb, const float pose[16]) {
  if (!f || !d_depth || !pose) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  return run_frame(f, d_depth, d_rgb, pose, -1);
}
static int integrate_batch_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes, const float* poses,
                                  uint64_t n) {
  if (!f || !d_depth || !poses) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  const void* dd[MAX_BATCH];
  const void* dr[MAX_BATCH];
  const float* pp[MAX_BATCH];
  int m = 0;
  int pass = 0;
  for (uint64_t i = 0; i <= n; i++) {
    if (i < n) {
      if (poses[16 * i] == -INFINITY) { f->frames_skipped++; continue; }  // tracking lost: skip (sensorData.h:382)
      dd[m] = (const uint8_t*)d_depth + i * frame_stride_bytes;
      dr[m] = d_rgb ? (const uint8_t*)d_rgb + i * rgb_stride_bytes : nullptr;
      pp[m] = poses + 16 * i;
      m++;
    }
    // the first pass of a call has nothing to hide its pre-pass / allocation / compaction behind: a short one (`ramp` frames) gets the
    // integrate stream busy sooner, and the passes behind it double -- ramp, 2 ramp, 4 ramp ... up to the batch size -- so that the
    // front chain of pass k + 1 still fits under the integrate launch of pass k (same voxels under any batching; a 20-frame call: 29.3 k frames/s
    // with no ramp, 30.0 k with 4 frames, 30.7 k with 8).
    // A call that would fit ONE pass (ramp < n <= batch) is fused as two halves: the second half's front chain hides behind the first half's integrate launch
    // (20 frames: 8 + 12 gives 31.4 k frames/s, 10 + 10 32.5 k, 6 + 12 + 2 29.6 k, 12 + 8 31.2 k).
    constexpr int ramp = 8;
    int want = f->batch;
    if (ramp < f->batch && n > (uint64_t)ramp) {
      if (n <= (uint64_t)f->batch) want = (int)((n + 1) / 2);
      else if (pass == 0) want = ramp;
      else if (pass < 6) want = std::min(f->batch, ramp << pass);
    }
    if (m == want || (i == n && m > 0)) {
      f->tail_pass = i == n;   // nothing of this call follows: its integrate launch has the chip to itself
      f->head_pass = pass == 0 && n > (uint64_t)m;   // nothing of this call runs beside its front chain (a one-pass call: neither head nor hidden)
      const int rc = run_batch(f, dd, d_rgb ? dr : nullptr, pp, m, +1);
      f->tail_pass = false;
      f->head_pass = false;
      if (rc != SF_OK) return rc;
      m = 0;
      pass++;
    }
  }
  return SF_OK;
}
SF_API int sf_fuser_integrate_batch_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const float* poses, uint64_t n) {
  return integrate_batch_device(f, d_depth, frame_stride_bytes, nullptr, 0, poses, n);
}
SF_API int sf_fuser_integrate_batch_device_rgb(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes,
                                               const float* poses, uint64_t n) {
  if (!d_rgb) return sf::fail(SF_ERR_INVALID_ARG, "NULL colour frames (sf_fuser_integrate_batch_device is the geometry-only entry point)");
  return integrate_batch_device(f, d_depth, frame_stride_bytes, d_rgb, rgb_stride_bytes, poses, n);
}

SF_API int sf_fuser_batch_frames(const sf_fuser* f) { return f ? f->batch : 0; }

// ------------------------------------------------------------------------------------------------------
// Re-integration: for frame j = 0 .. n - 1 in order, deintegrate (depth_j, old_j), then integrate (depth_j, new_j) -- as mixed-sign passes.
// The operations of the call, in that order, are dealt into passes of up to f->batch slots; the two slots of a moved frame stay in one pass (they share the
// frame's converted image).  A pass of + slots only is an ordinary integrate pass, a single - slot an ordinary deintegrate launch; everything else runs
// k_reintegrate.  A frame that only leaves the volume (new pose lost) has no + slot whose plane could hold its image: the image goes to a plane behind the
// slots' (MAX_BATCH planes per batch slot in all).
// ------------------------------------------------------------------------------------------------------
namespace {

struct ReintPass {
  sf_fuser* f;
  bool col;
  int m = 0, x = 0;   // slots, images behind the slots' planes
  const void* dd[MAX_BATCH];
  const void* dr[MAX_BATCH];
  const void* xd[MAX_BATCH];   // the images of frames that only leave
  const float* pp[MAX_BATCH];
  int ximg[MAX_BATCH];         // slot -> index into xd, or -1
  ReintSlots rs;

  explicit ReintPass(sf_fuser* f_, bool col_) : f(f_), col(col_) { std::memset(&rs, 0, sizeof(rs)); }
  bool fits(int slots, int extra) const { return m + slots <= std::max(f->batch, 2) && m + slots + x + extra <= MAX_BATCH; }
  void add(const void* depth, const void* rgb, const float* pose_old, const float* pose_new) {
    if (pose_old) {
      rs.neg |= 1u << m;
      ximg[m] = -1;
      if (pose_new) rs.img[m] = (uint32_t)(m + 1);
      else { ximg[m] = x; xd[x++] = depth; }
      dd[m] = depth;   // (a single - slot runs the ordinary deintegrate launch on its own plane; a mixed pass puts the frame of zeros here)
      dr[m] = rgb;
      pp[m++] = pose_old;
    }
    if (pose_new) {
      rs.img[m] = (uint32_t)m;
      ximg[m] = -1;
      dd[m] = depth;
      dr[m] = rgb;
      pp[m++] = pose_new;
    }
  }
  int flush() {
    if (m == 0) return SF_OK;
    int rc;
    if (rs.neg == 0u) rc = run_batch(f, dd, col ? dr : nullptr, pp, m, +1);
    else if (m == 1) rc = run_batch(f, dd, col ? dr : nullptr, pp, 1, -1);
    else {
      if (!f->void_depth) {
        SF_HIP_CHECK(hipMalloc(&f->void_depth, f->in_px * 2));
        SF_HIP_CHECK(hipMemset(f->void_depth, 0, f->in_px * 2));
        SF_HIP_CHECK(hipDeviceSynchronize());
      }
      for (int q = 0; q < m; q++) {
        if (!((rs.neg >> q) & 1u)) continue;
        if (ximg[q] >= 0) rs.img[q] = (uint32_t)(m + ximg[q]);
        dd[q] = f->void_depth;
        dr[q] = nullptr;
      }
      for (int k = 0; k < x; k++) { dd[m + k] = xd[k]; dr[m + k] = nullptr; }
      const bool plus = rs.neg != (m == 32 ? 0xFFFFFFFFu : ((1u << m) - 1u));
      rc = run_batch(f, dd, dr, pp, m, plus ? +1 : -1, nullptr, &rs, m + x, col);
    }
    f->reint_passes++;
    m = x = 0;
    std::memset(&rs, 0, sizeof(rs));
    return rc;
  }
};

}  // namespace

SF_API int sf_fuser_reintegrate_batch_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes,
                                             const float* old_poses, const float* new_poses, uint64_t n) {
  if (!f || (n > 0 && (!d_depth || !old_poses || !new_poses))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  f->reint_passes = 0;
  ReintPass pass(f, d_rgb != nullptr);
  for (uint64_t i = 0; i < n; i++) {
    const float* po = old_poses + 16 * i;
    const float* pn = new_poses + 16 * i;
    const bool has_old = po[0] != -INFINITY, has_new = pn[0] != -INFINITY;
    f->frames_skipped += (uint64_t)(!has_old) + (uint64_t)(!has_new);   // what the two calls of the sequence would have counted
    if (!has_old && !has_new) continue;
    const void* depth = (const uint8_t*)d_depth + i * frame_stride_bytes;
    const void* rgb = d_rgb ? (const uint8_t*)d_rgb + i * rgb_stride_bytes : nullptr;
    if (f->batch < 2) {   // one slot per pass (tune "batch" 1): the sequence itself
      int rc = SF_OK;
      if (has_old) { rc = run_frame(f, depth, rgb, po, -1); f->reint_passes++; }
      if (rc == SF_OK && has_new) { rc = run_frame(f, depth, rgb, pn, +1); f->reint_passes++; }
      if (rc != SF_OK) return rc;
      continue;
    }
    const int slots = (int)has_old + (int)has_new, extra = has_old && !has_new ? 1 : 0;
    if (!pass.fits(slots, extra)) {
      const int rc = pass.flush();
      if (rc != SF_OK) return rc;
    }
    pass.add(depth, rgb, has_old ? po : nullptr, has_new ? pn : nullptr);
  }
  return pass.flush();
}

// One frame from host buffers: the frame goes through the page-locked ring of fuse_host once and serves both slots.
SF_API int sf_fuser_reintegrate(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float old_pose[16], const float new_pose[16]) {
  if (!f || !depth || !old_pose || !new_pose) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const bool has_old = old_pose[0] != -INFINITY, has_new = new_pose[0] != -INFINITY;
  if (!has_old || !has_new || f->batch < 2) {   // at most one operation per launch: the calls of the sequence themselves
    const int r0 = fuse_host(f, depth, rgb, old_pose, -1);
    if (r0 != SF_OK && r0 != SF_ERR_SKIPPED) return r0;
    const int r1 = fuse_host(f, depth, rgb, new_pose, +1);
    if (r1 != SF_OK && r1 != SF_ERR_SKIPPED) return r1;
    if (r0 == SF_ERR_SKIPPED && r1 == SF_ERR_SKIPPED) return SF_ERR_SKIPPED;
    sf::last_error_ref().clear();
    return SF_OK;
  }
  SF_HIP_CHECK(hipSetDevice(f->device));
  int q = 0;
  const int rs = stage_host_frame(f, depth, rgb, sf_input_stream(f, 2, rgb != nullptr, +1), &q);   // where the pass's pre-pass reads the frame
  if (rs != SF_OK) return rs;
  f->reint_passes = 0;
  ReintPass pass(f, rgb != nullptr);
  pass.add(f->staging_depth[q], rgb ? f->staging_rgb[q] : nullptr, old_pose, new_pose);
  const int rc = pass.flush();
  const int rr = retire_host_frame(f, q);
  return rr != SF_OK ? rr : rc;
}

// scanfuse_internal.h: scheduling switches (bench.py, tests); every setting leaves the voxels bit-identical
SF_API int sf_fuser_tune(sf_fuser* f, const char* key, int value) {
  if (!f || !key) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  const std::string k(key);
  auto in = [&](int lo, int hi) { return value >= lo && value <= hi; };
  if (k == "batch" && in(1, MAX_BATCH)) f->batch = value;
  else if (k == "overlap" && in(0, 1)) f->overlap = value != 0;
  else if (k == "xcd_walk" && in(0, 1)) f->xcd_walk = value != 0;
  else if (k == "pipe" && in(0, 1)) f->pipe_mode = value;
  else if (k == "pipe_overlap" && in(-1, 1)) { f->pipe_overlap = value; f->pipe_beside = value == 1; }
  else if (k == "alloc_group" && in(1, MAX_BATCH)) f->alloc_group = value;
  // which of the two front streams a pass's pre-pass / allocation / compaction goes down (sf_input_stream): -1 the second one (front_lo) beside the persistent kernel of
  // one frame per launch, the high-priority one otherwise (default); 1 always the high-priority one (rounds 2-5); 0 always the second one
  else if (k == "front_prio" && in(-1, 1)) f->front_prio = value;
  else if (k == "front_lo_lowest" && in(0, 1)) f->front_lo_lowest = value != 0;   // before the stream's first need: 1 = the device's lowest priority, 0 = the main stream's
  else if (k == "alloc_ray" && in(0, 1)) f->alloc_ray = value != 0;   // 1: the ray-space window whatever the geometry (rays outside it take the slow path), 0: the cube window
  else if (k == "tail_wide" && in(0, 1)) f->tail_wide = value;
  else if (k == "brick_cache" && in(0, 1)) {   // 0: every look-up of the allocation kernels probes the table
    f->brick_on = value != 0;
    SF_HIP_CHECK(hipMemsetAsync(f->bricks, 0, (size_t)f->brick_lines * 128, f->stream));
    SF_HIP_CHECK(sf_quiesce(f));
  }
  else return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_tune: unknown key or value out of range: %s = %d", key, value);
  return SF_OK;
}

// fuser_internal.h, for pipeline.hip
int sf_fuser_run_batch(sf_fuser* f, const void* const* d_depth, const void* const* d_rgb, const float* const* poses, int n) {
  if (n < 1 || n > f->batch) return sf::fail(SF_ERR_INVALID_ARG, "batch of %d frames (limit %d)", n, f->batch);
  return run_batch(f, d_depth, d_rgb, poses, n, +1);
}

int sf_fuser_run_batch_ycc(sf_fuser* f, const void* const* d_depth, const void* const* d_planes, const void* const* d_layout, const float* const* poses, int n) {
  if (n < 1 || n > f->batch) return sf::fail(SF_ERR_INVALID_ARG, "batch of %d frames (limit %d)", n, f->batch);
  return run_batch(f, d_depth, d_planes, poses, n, +1, d_layout);
}

SF_API int sf_fuser_sync(sf_fuser* f) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  return SF_OK;
}
SF_API void* sf_fuser_stream(sf_fuser* f) { return f ? (void*)f->stream : nullptr; }

SF_API int sf_fuser_stats(sf_fuser* f, sf_stats* out) {
  if (!f || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  int32_t c[C_COUNT];
  SF_HIP_CHECK(hipMemcpyAsync(c, f->counters, sizeof(c), hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  std::memset(out, 0, sizeof(*out));
  out->frames_integrated = f->frames_integrated;
  out->frames_skipped = f->frames_skipped;
  out->heap_free = (uint32_t)c[C_HEAP_FREE];
  out->blocks_allocated = f->pk.num_blocks - (uint32_t)c[C_HEAP_FREE];
  out->last_frame_blocks = (uint32_t)c[C_LAST_BLOCKS];
  out->alloc_failures = (uint32_t)c[C_ALLOC_FAIL];
  uint64_t tot;
  std::memcpy(&tot, &c[C_TOTAL_LO], 8);
  out->total_frame_blocks = tot;
  std::memcpy(&tot, &c[C_TILES_LO], 8);
  out->total_pass_tiles = tot;
  out->hash_slots_used = (uint32_t)c[C_SLOTS_USED];
  out->high_water = (uint32_t)c[C_HIGH_WATER];
  return SF_OK;
}

SF_API int sf_fuser_alloc_direct_count(sf_fuser* f, uint64_t* out) {
  if (!f || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  int32_t c = 0;
  SF_HIP_CHECK(hipMemcpy(&c, &f->counters[C_ALLOC_DIRECT], 4, hipMemcpyDeviceToHost));
  *out = (uint64_t)(uint32_t)c;
  return SF_OK;
}

SF_API int sf_fuser_alloc_probe_count(sf_fuser* f, uint64_t* out) {
  if (!f || !out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  int32_t c = 0;
  SF_HIP_CHECK(hipMemcpy(&c, &f->counters[C_ALLOC_PROBED], 4, hipMemcpyDeviceToHost));
  *out = (uint64_t)(uint32_t)c;
  return SF_OK;
}

SF_API int sf_fuser_profile_enable(sf_fuser* f, int on) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  f->profile = on != 0;
  return SF_OK;
}
SF_API int sf_fuser_profile_read(sf_fuser* f, double* integrate_ms, uint64_t* launches, uint64_t* blocks) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  double ms = 0;
  for (size_t i = 0; i < f->events_used; i++) {
    float t = 0;
    SF_HIP_CHECK(hipEventElapsedTime(&t, f->events[i].first, f->events[i].second));
    ms += t;
  }
  if (integrate_ms) *integrate_ms = ms;
  if (launches) *launches = f->events_used;
  if (blocks) {
    int32_t c[2];
    SF_HIP_CHECK(hipMemcpy(c, &f->counters[C_TOTAL_LO], 8, hipMemcpyDeviceToHost));
    std::memcpy(blocks, c, 8);
  }
  f->events_used = 0;
  return SF_OK;
}


SF_API int sf_device_malloc(int device, uint64_t bytes, void** out) {
  if (!out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(device));
  SF_HIP_CHECK(hipMalloc(out, bytes));
  return SF_OK;
}
SF_API int sf_device_free(void* p) { SF_HIP_CHECK(hipFree(p)); return SF_OK; }
SF_API int sf_device_upload(void* dst, const void* src, uint64_t bytes) { SF_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return SF_OK; }
SF_API int sf_device_download(void* dst, const void* src, uint64_t bytes) { SF_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return SF_OK; }

// ======================================================================================================
// Stage hooks of the front chain (scanfuse_internal.h; tests/test_front_stages.py): ONE stage of a pass on an existing fuser, through the launcher run_batch
// uses for it, on the main stream and the buffers of batch slot 0, between two sf_quiesce.  Every argument is checked before the first launch.
// ======================================================================================================
namespace {

int stage_enter(sf_fuser* f, int n, const char* who) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "%s: NULL fuser", who);
  if (n < 1 || n > MAX_BATCH) return sf::fail(SF_ERR_INVALID_ARG, "%s: %d frames (1..%d)", who, n, MAX_BATCH);
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  return SF_OK;
}

int stage_counters(sf_fuser* f, int32_t* c) {
  SF_HIP_CHECK(hipMemcpyAsync(c, f->counters, C_COUNT * 4, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  return SF_OK;
}

uint64_t counter64(const int32_t* c, int at) {
  uint64_t v;
  std::memcpy(&v, c + at, 8);
  return v;
}

bool stage_frames(const sf_fuser* f, int n, const float* poses, uint32_t seq0, BatchFrames& bf) {
  std::memset(&bf, 0, sizeof(bf));
  bf.n = n;
  bf.seq0 = seq0;
  for (int j = 0; j < n; j++)
    if (!frame_setup(f->p, poses + 16 * j, bf.f[j])) return false;
  return true;
}

}  // namespace

SF_API int sf_fuser_stage_prepass(sf_fuser* f, int n, const uint16_t* depth, const uint8_t* rgb, int misalign, const uint8_t* const* jpeg, const uint64_t* jpeg_bytes,
                                  float* depthf_out, uint64_t* texel_out) {
  const int rc0 = stage_enter(f, n, "sf_fuser_stage_prepass");
  if (rc0 != SF_OK) return rc0;
  const bool col = rgb != nullptr || jpeg != nullptr;
  if (!depth || !depthf_out || (rgb && jpeg) || (col && !texel_out) || (!col && texel_out) || (jpeg && !jpeg_bytes) || misalign < 0 || misalign > 7 || (!rgb && misalign != 0))
    return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_prepass: depth and depthf_out; colour as ONE of rgb (misalign 0..7) or jpeg + jpeg_bytes, with texel_out");
  const size_t npx = (size_t)f->pk.W * f->pk.H;
  const uint32_t cw = (uint32_t)(f->pk.cW ? f->pk.cW : f->pk.W), ch = (uint32_t)(f->pk.cW ? f->pk.cH : f->pk.H);
  const size_t rgb_bytes = (size_t)cw * ch * 3;
  // the entropy decoding of every picture comes first: a stream the device path does not take is an error before any launch
  std::vector<std::vector<uint32_t>> pay((size_t)(jpeg ? n : 0));
  uint32_t max_blocks = 0;
  for (int j = 0; jpeg && j < n; j++) {
    if (!jpeg[j] || jpeg_bytes[j] == 0) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_prepass: picture %d is empty", j);
    const uint64_t padded = (uint64_t)((cw + 15) & ~15u) * ((ch + 15) & ~15u);
    pay[j].resize((sizeof(SfJpegLayout) + padded * 3 / 64 * 4 + padded * 3 * 4) / 4 + 64);
    const int rc = jpeg_decode_coef(jpeg[j], jpeg_bytes[j], cw, ch, reinterpret_cast<uint8_t*>(pay[j].data()), pay[j].size() * 4);
    if (rc != SF_OK) return rc;
    max_blocks = std::max(max_blocks, reinterpret_cast<const SfJpegLayout*>(pay[j].data())->nblocks);
  }
  sf::DevBuf d_depth, d_rgb, d_pay[MAX_BATCH], d_planes[MAX_BATCH];
  SF_HIP_CHECK(d_depth.alloc((size_t)n * f->in_px * 2));
  SF_HIP_CHECK(hipMemcpyAsync(d_depth.p, depth, (size_t)n * f->in_px * 2, hipMemcpyHostToDevice, f->stream));
  BatchIn in;
  std::memset(&in, 0, sizeof(in));
  for (int j = 0; j < n; j++) in.depth[j] = d_depth.as<uint16_t>() + (size_t)j * f->in_px;
  if (rgb) {
    SF_HIP_CHECK(d_rgb.alloc((size_t)n * rgb_bytes + 8));
    SF_HIP_CHECK(hipMemcpyAsync(d_rgb.as<uint8_t>() + misalign, rgb, (size_t)n * rgb_bytes, hipMemcpyHostToDevice, f->stream));
    for (int j = 0; j < n; j++) in.rgb[j] = d_rgb.as<uint8_t>() + misalign + (size_t)j * rgb_bytes;
  }
  if (jpeg) {
    const uint8_t* pp[MAX_BATCH];
    uint8_t* pl[MAX_BATCH];
    for (int j = 0; j < n; j++) {
      const SfJpegLayout& L = *reinterpret_cast<const SfJpegLayout*>(pay[j].data());
      SF_HIP_CHECK(d_pay[j].alloc(sf_jpeg_payload_bytes(L)));
      SF_HIP_CHECK(d_planes[j].alloc(sf_jpeg_plane_bytes(L)));
      SF_HIP_CHECK(hipMemcpyAsync(d_pay[j].p, pay[j].data(), sf_jpeg_payload_bytes(L), hipMemcpyHostToDevice, f->stream));
      pp[j] = d_pay[j].as<uint8_t>();
      pl[j] = d_planes[j].as<uint8_t>();
      in.rgb[j] = pl[j];
      in.lay[j] = pp[j];   // the payload begins with the picture's SfJpegLayout
    }
    for (int q0 = 0; q0 < n; q0 += 16) {   // (a launch of jpeg_gpu_planes takes up to 16 pictures)
      const int rc = jpeg_gpu_planes(f->stream, std::min(16, n - q0), pp + q0, pl + q0, max_blocks);
      if (rc != SF_OK) { (void)sf_quiesce(f); return rc; }
    }
  }
  sf_launch_prepass(f, 0, n, in, f->stream);
  const hipError_t le = hipGetLastError();
  SF_HIP_CHECK(hipMemcpyAsync(depthf_out, f->depthf2[0], (size_t)n * npx * 4, hipMemcpyDeviceToHost, f->stream));
  if (col) SF_HIP_CHECK(hipMemcpyAsync(texel_out, f->color2[0], (size_t)n * npx * 8, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  if (le != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuser_stage_prepass: launch failed: %s", hipGetErrorString(le));
  return SF_OK;
}

SF_API int sf_fuser_stage_alloc(sf_fuser* f, int n, const uint16_t* depth, const float* poses, int head, int fuse_pre, float* depthf_out, uint64_t deltas[3]) {
  const int rc0 = stage_enter(f, n, "sf_fuser_stage_alloc");
  if (rc0 != SF_OK) return rc0;
  if (!depth || !poses || !deltas || (head & ~1) || (fuse_pre & ~1)) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_alloc: NULL argument, or head / fuse_pre not 0 or 1");
  // the fused variant exactly where run_batch picks it: one colourless frame at the integration size through the ray-space kernel
  if (fuse_pre && !(f->alloc_ray && n == 1 && f->pk.inW == 0)) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_alloc: a pass of this shape does not fuse the pre-pass");
  BatchFrames bf;
  if (!stage_frames(f, n, poses, f->frame_seq, bf)) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_alloc: invalid pose in batch");
  int32_t c0[C_COUNT], c1[C_COUNT];
  int rc = stage_counters(f, c0);
  if (rc != SF_OK) return rc;
  sf::DevBuf d_depth;
  SF_HIP_CHECK(d_depth.alloc((size_t)n * f->in_px * 2));
  SF_HIP_CHECK(hipMemcpyAsync(d_depth.p, depth, (size_t)n * f->in_px * 2, hipMemcpyHostToDevice, f->stream));
  BatchIn in;
  std::memset(&in, 0, sizeof(in));
  for (int j = 0; j < n; j++) in.depth[j] = d_depth.as<uint16_t>() + (size_t)j * f->in_px;
  f->frame_seq += (uint32_t)n;
  if (!fuse_pre) sf_launch_prepass(f, 0, n, in, f->stream);
  f->head_pass = head != 0;
  sf_launch_alloc(f, 0, n, bf, in, f->stream, fuse_pre != 0);
  f->head_pass = false;
  const hipError_t le = hipGetLastError();
  if (depthf_out) SF_HIP_CHECK(hipMemcpyAsync(depthf_out, f->depthf2[0], (size_t)n * f->pk.W * f->pk.H * 4, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  if (le != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuser_stage_alloc: launch failed: %s", hipGetErrorString(le));
  rc = stage_counters(f, c1);
  if (rc != SF_OK) return rc;
  deltas[0] = (uint32_t)(c1[C_ALLOC_DIRECT] - c0[C_ALLOC_DIRECT]);
  deltas[1] = (uint32_t)(c1[C_ALLOC_PROBED] - c0[C_ALLOC_PROBED]);
  deltas[2] = (uint32_t)(c1[C_ALLOC_FAIL] - c0[C_ALLOC_FAIL]);
  return SF_OK;
}

SF_API int sf_fuser_stage_compact(sf_fuser* f, int n, const float* poses, uint32_t seq0, int32_t* list_out, uint32_t* mask_out, uint64_t capacity, uint64_t* counter_word,
                                  uint64_t deltas[2]) {
  const int rc0 = stage_enter(f, n, "sf_fuser_stage_compact");
  if (rc0 != SF_OK) return rc0;
  if (!poses || !list_out || !mask_out || !counter_word || !deltas) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_compact: NULL argument");
  BatchFrames bf;
  if (!stage_frames(f, n, poses, seq0, bf)) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_compact: invalid pose in batch");
  int32_t c0[C_COUNT], c1[C_COUNT];
  int rc = stage_counters(f, c0);
  if (rc != SF_OK) return rc;
  if (c0[C_HIGH_WATER] < 0 || (uint64_t)c0[C_HIGH_WATER] > capacity)   // the list never holds more than the directory's used stretch
    return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_compact: capacity %llu below the directory's %d entries", (unsigned long long)capacity, c0[C_HIGH_WATER]);
  SF_HIP_CHECK(hipMemsetAsync(&f->counters[sf_compact_counter(0)], 0, 8, f->stream));   // what the pass's pre-pass does
  sf_launch_compact(f, 0, bf, f->stream);
  const hipError_t le = hipGetLastError();
  SF_HIP_CHECK(sf_quiesce(f));
  if (le != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuser_stage_compact: launch failed: %s", hipGetErrorString(le));
  rc = stage_counters(f, c1);
  if (rc != SF_OK) return rc;
  const uint64_t word = counter64(c1, sf_compact_counter(0));
  const uint64_t len = word & 0xFFFFFFFFull;
  if (len > capacity) return sf::fail(SF_ERR_BOUNDS, "sf_fuser_stage_compact: the list holds %llu entries, capacity %llu", (unsigned long long)len, (unsigned long long)capacity);
  if (len) {
    SF_HIP_CHECK(hipMemcpyAsync(list_out, f->compact2[0], len * 4, hipMemcpyDeviceToHost, f->stream));
    SF_HIP_CHECK(hipMemcpyAsync(mask_out, f->cmask2[0], len * 4, hipMemcpyDeviceToHost, f->stream));
    SF_HIP_CHECK(sf_quiesce(f));
  }
  *counter_word = word;
  deltas[0] = counter64(c1, C_TOTAL_LO) - counter64(c0, C_TOTAL_LO);
  deltas[1] = counter64(c1, C_TILES_LO) - counter64(c0, C_TILES_LO);
  return SF_OK;
}

SF_API int sf_fuser_stage_live(sf_fuser* f, int include_ghosts, int32_t* list_out, uint64_t capacity, uint64_t* n_out) {
  const int rc0 = stage_enter(f, 1, "sf_fuser_stage_live");
  if (rc0 != SF_OK) return rc0;
  if (!list_out || !n_out || (include_ghosts & ~1)) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_live: NULL argument, or include_ghosts not 0 or 1");
  int32_t c0[C_COUNT];
  int rc = stage_counters(f, c0);
  if (rc != SF_OK) return rc;
  if (c0[C_HIGH_WATER] < 0 || (uint64_t)c0[C_HIGH_WATER] > capacity)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_live: capacity %llu below the directory's %d entries", (unsigned long long)capacity, c0[C_HIGH_WATER]);
  int32_t n = 0;
  rc = sf_compact_live(f, &n, include_ghosts);
  if (rc != SF_OK) return rc;
  if (n > 0) {
    SF_HIP_CHECK(hipMemcpyAsync(list_out, f->compact, (size_t)n * 4, hipMemcpyDeviceToHost, f->stream));
    SF_HIP_CHECK(sf_quiesce(f));
  }
  *n_out = (uint64_t)n;
  return SF_OK;
}

SF_API int sf_fuser_stage_dump(sf_fuser* f, uint64_t* key_out, int32_t* ptr_out, uint32_t* birth_out, int32_t* heap_out, uint64_t* block_keys_out, int32_t* block_entry_out,
                               uint8_t* block_flags_out, int32_t* counters_out) {
  const int rc0 = stage_enter(f, 1, "sf_fuser_stage_dump");
  if (rc0 != SF_OK) return rc0;
  if (!key_out || !ptr_out || !birth_out || !heap_out || !block_keys_out || !block_entry_out || !block_flags_out || !counters_out)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_stage_dump: NULL argument");
  const size_t slots = f->pk.total_slots, nb = f->pk.num_blocks;
  std::vector<HashEntry> t(slots);
  SF_HIP_CHECK(hipMemcpyAsync(t.data(), f->table, slots * sizeof(HashEntry), hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(hipMemcpyAsync(heap_out, f->heap, nb * 4, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(hipMemcpyAsync(block_keys_out, f->block_keys, nb * 8, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(hipMemcpyAsync(block_entry_out, f->block_entry, nb * 4, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(hipMemcpyAsync(block_flags_out, f->block_flags, nb, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(hipMemcpyAsync(counters_out, f->counters, C_COUNT * 4, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  for (size_t i = 0; i < slots; i++) { key_out[i] = t[i].key; ptr_out[i] = t[i].ptr; birth_out[i] = t[i].birth; }
  return SF_OK;
}
