// pipeline.hip -- .sens stream -> fuser: multi-threaded depth decode overlapped with H2D copies and the
// fusion kernels.  Replaces the per-frame loop of the external DepthSensing.exe around the reference's
// RGBDFrameCacheRead (SensReader/c++/src/sensorData.h:1717-1831: ONE decode thread, spin-waiting consumer):
// here a pool of decode threads fills a ring of pinned host buffers in frame order, the caller's thread
// issues the asynchronous copy + kernels for each frame as soon as it is decoded, and nothing spins.
// Frames whose camToWorld is -inf (tracking lost, sensorData.h:382) are skipped, as every reference
// consumer does (Alignment/src/alignment.h:26,54; Filter2dAnnotations.cpp:317).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "codecs_internal.h"
#include "fuser_internal.h"
#include "hip_util.h"
#include "jpeg_huff.h"
#include "jpeg_idct.h"
#include "sens.h"

// The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and kernels of streams that share a queue
// run one after the other.  sf_fuse_run drives up to seven streams (the fuser's two, two for colour copies, three for the inflate kernels); on four
// queues every third batch's inflate sat in the integrate pass's queue (29 k -> 20 k frames/s in the loop).  The variable belongs to the PROCESS
// (it is read at its first HIP call): neither the library nor its tools touch the environment, and a run that finds
// fewer queues than it has streams says so through sf_fuse_run_note() while returning SF_OK.

// the default of the JPEG entropy decoding (see RunPlan::gpu_huffman), decided by measurement (profiles/r05_e2e_rgbd.json: 1296x968 pictures of ~200 KB,
// device + 4 host threads 12.3 k frames/s before the five side streams, host decoding on 16 threads 10.0 k, on 4 threads 3.2 k): on the device whenever the
// batch has a side stream to decode on
#define SF_JPEG_DEVICE_HUFFMAN_DEFAULT(has_side_stream) (has_side_stream)

namespace {

// The side streams (inflate and JPEG kernels, colour copies) run at the default priority.  Their kernels are small grids of LARGE workgroups (1024 lanes,
// 100+ registers per lane) that need a whole free CU; at the device's highest priority they ran no faster (profiles/r06_e2e_rgbd_ab.txt: 16 267 against
// 16 182 frames/s on a 2 048-frame RGB-D scan).
hipError_t create_side_stream(hipStream_t* out) { return hipStreamCreateWithFlags(out, hipStreamNonBlocking); }
thread_local uint64_t t_run_counts[4] = {0, 0, 0, 0};   // of this thread's last sf_fuse_run: depth frames inflated on the device / by the host threads, colour
                                                        // frames entropy-decoded on the device / by the host threads (sf_fuse_run_device_counts)
thread_local char t_run_note[320] = "";   // sf_fuse_run_note(): a hint about the calling thread's last run that is not an error

int hardware_queues_of_the_process() {   // what the runtime was (or will be) told; its default is 4
  const char* v = std::getenv("GPU_MAX_HW_QUEUES");
  const int n = v ? std::atoi(v) : 0;
  return n > 0 ? n : 4;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
size_t round_up(size_t n, size_t to) { return (n + to - 1) & ~(to - 1); }
constexpr int MAX_NZ = 6, MAX_COPY = 2;   // side streams / copy streams a run can want

// The plan of a run: its decisions, and the geometry of its ring.
struct RunSwitches {   // the environment, read once per run
  bool timing = false;              // SF_RUN_TIMING: where the run's time went, on stderr
  bool inflate_host = false;        // SF_INFLATE_HOST=1: always inflate depth on the host threads
  bool jpeg_host = false;           // SF_JPEG_HOST=1: always decode JPEG colour on the host threads
  bool jpeg_rgb_image = false;      // SF_JPEG_RGB_IMAGE=1: the device writes every picture out as RGB (k_jpeg_rgb) and the pre-pass picks its pixels from that (A/B measurements)
  bool jpeg_host_huffman = false, jpeg_gpu_huffman = false;   // SF_JPEG_HOST_HUFFMAN=1 / SF_JPEG_GPU_HUFFMAN=1: force where the JPEG entropy decoding runs (RunPlan::gpu_huffman)
  static bool on(const char* name) { return std::getenv(name) != nullptr; }
  static RunSwitches from_env() { return {on("SF_RUN_TIMING"), on("SF_INFLATE_HOST"), on("SF_JPEG_HOST"), on("SF_JPEG_RGB_IMAGE"), on("SF_JPEG_HOST_HUFFMAN"), on("SF_JPEG_GPU_HUFFMAN")}; }
};
struct ResourceNeed { int side_streams, copy_streams; size_t pinned_bytes, device_bytes, plan_bytes; };

struct RunPlan {
  RunSwitches sw;
  // What the geometry needs to know of the frames, set before lay_out(): sf_fuse_run measures it; sf_fuse_run_prepare, which runs before the fuser exists, bounds it.
  uint64_t nbatches = 0;        // of the run: a ring has no more slots than that
  size_t packed_depth = 0;      // GPU inflate: the largest batch's packed depth part (compressed frames: about half of the pixels)
  size_t max_color_bytes = 0;   // the largest colour blob
  uint32_t pay_blocks = 0;      // of a picture of the scan (its frames share the layout): 8x8 blocks of all components; 0 = no picture the device reconstructs
  size_t jpeg_plane_bytes = 0;  // ... and its component planes
  std::vector<uint8_t> zmode;     // GPU inflate, per frame of the run: 1 = travels compressed
  std::vector<uint32_t> zoff;     // ... its segment's offset in the slot's packed depth part
  std::vector<uint32_t> zbytes;   // ... per batch: bytes to copy
  // colour is fused when its frames match what the fuser was created for: depth resolution, or the colour resolution
  // given in sf_params (raw or JPEG); anything else: geometry only
  bool use_rgb = false, jpeg_colour = false;
  // zlib depth (the reference's writer: one final fixed-Huffman block per frame) is inflated on the GPU: a host thread only copies the compressed
  // frame into the pinned ring; streams the device does not take (dynamic / stored / several blocks, longer than the pixels) are inflated by
  // the host threads as before.
  bool gpu_inflate = false;
  // JPEG colour: the host threads only entropy-decode; the coefficients travel in place of the pixels and the GPU reconstructs
  // (jpeg_gpu.hip).  The payload is sized from the first colour frame's layout (a scan's frames share it); a frame that does not fit,
  // or has a layout the GPU path does not take, is decoded on the host as before.
  bool gpu_jpeg = false, ycc_ok = false;
  // where the entropy decoding runs: on the device when the batch has a side stream for it (the depth inflate's), else on the host threads.  On the device a
  // host thread only parses the headers and strips the byte stuffing (jpeg_prepare_huff), the entropy-coded segment travels and the GPU entropy-decodes too
  // (jpeg_huff_gpu.hip; frames with restart intervals stay with the host threads).  Same bytes; WITHOUT a side stream measured SLOWER with 16 host threads
  // (6.1 k against 7.5 k frames/s at 1296x968: 1.25 ms per 16 pictures on 16 CUs) -- there it is for hosts with few cores, and opt-in.
  bool gpu_huffman = false;
  int nthreads = 1, B = 0;   // decode pool; frames fused per pass over the voxel tiles = frames of a ring slot
  // side streams: batch g is inflated (and its JPEG pictures entropy-decoded and reconstructed) on stream g % NZ, beside the fusion of the batches before
  // it.  A batch takes ~1.8 ms to inflate and 0.8 ms to fuse: three in flight; with JPEG colour the side work is ~4.9 ms per batch (k_jpeg_huff 2.4 ms
  // per 32 pictures of 200 KB on 32 CUs): five (profiles/r05_timeline_e2e_rgbd.txt)
  int NZ = 3;
  // enough batch slots for every decode thread to be busy while two batches sit between copy and pre-pass
  // 3 slots (one decoding, one in flight, one being read by the pre-pass) are enough: 4, 6 and 10 measured no faster (tools/gpu/h2d_bw.hip:
  // the link moves 57 GB/s from pinned memory on two streams; a colour run is bound by the fusion kernels and ~15 ms of set-up)
  int NB = 1;
  uint32_t color_w = 0, color_h = 0, pay_entries = 0;
  size_t depth_b = 0, rgb_b = 0, pay_b = 0, planes_b = 0;   // per frame: depth pixels, colour pixels, coefficient payload, component planes
  // GPU inflate: the depth part of a pinned slot is PACKED -- per frame either the zlib stream from its third byte on (the device inflates it)
  // or, for a stream the device does not take, the pixels a host thread decoded; 64-byte aligned segments whose offsets are known before
  // anybody decodes (the sizes are in the file's frame table), so that the batch crosses PCIe in ONE copy (32 copies of ~330 KB cost the
  // enqueueing thread 0.6 ms per batch).  Otherwise: depth_b per frame.
  size_t slot_depth = 0, dslot_depth = 0;   // dslot_depth: on the device, the frames as pixels (where the inflate kernels write)
  // pinned slot: depth, then per frame ONE colour area that holds either pixels or coefficients (col_b = the larger of the two);
  // device slot: depth, pixels, coefficients, planes scratch, packed depth
  size_t col_b = 0, slot_col = 0, slot_planes = 0;
  // With the device's entropy decoder a picture travels as its prepared segment -- never more than its blob in the file plus the tables -- so the PINNED
  // slot holds that per frame instead of room for a decoded picture (1296x968: 0.26 MB instead of 3.8 MB per frame, 110 MB of page-locked memory for a run
  // instead of 833 MB: 45 ms of the first run of a process).  A picture the device does not take (restart intervals, ...) is decoded by its host thread
  // into a pageable buffer of its own and copied from there (coef_mode 3).
  size_t hcol_b = 0, hslot_col = 0, slot_b = 0, slot_comp = 0, dslot_b = 0;
  uint8_t *h_pool = nullptr, *d_pool = nullptr;   // ONE pinned host allocation and ONE device allocation for the whole ring (set once the run holds its resources)
  // the decisions: from the file's header, the colour size the fuser was made for (0: the depth size), the batch size and the switches
  RunPlan(const sf_sens_info& info, int cW, int cH, int batch, const RunSwitches& w, int decode_threads) : sw(w), B(batch) {
    const size_t npx = (size_t)info.depth_width * info.depth_height;   // of an input frame (the pre-pass resamples to the integration size when the two differ)
    const bool same_res = info.color_width == info.depth_width && info.color_height == info.depth_height;
    const bool own_res = cW > 0 && (int)info.color_width == cW && (int)info.color_height == cH;
    use_rgb = ((same_res && cW == 0) || own_res) && (info.color_compression >= 0 && info.color_compression <= 2);   // raw, PNG (host decode), JPEG
    jpeg_colour = use_rgb && info.color_compression == 2;
    gpu_inflate = info.depth_compression == 1 && (npx * 2) % 4 == 0 && !sw.inflate_host;
    color_w = info.color_width; color_h = info.color_height;
    depth_b = npx * 2;
    rgb_b = use_rgb ? (cW > 0 ? (size_t)cW * cH : npx) * 3 : 0;
    // default pool size: inflating a depth frame takes ~0.13 ms, so 32 threads outrun the GPU (measured: 16 threads 28 k frames/s,
    // 64 threads 26 k); baseline-JPEG colour costs milliseconds per frame and takes up to 64 (128 measured slower: 5.0 k vs 8.1 k frames/s)
    nthreads = decode_threads > 0 ? decode_threads : std::min(sf::usable_cpus(), jpeg_colour ? 64 : 32);
    nthreads = std::max(1, std::min(nthreads, 256));
    NZ = jpeg_colour ? 5 : 3;
  }
  bool wants_jpeg_probe() const { return jpeg_colour && !sw.jpeg_host; }
  void pack_depth(const sf_sens* s, uint64_t first, uint64_t total) {   // GPU inflate: where each frame sits in its slot's packed depth part
    zmode.assign(total, 0); zoff.assign(total, 0); zbytes.assign(nbatches, 0);
    for (uint64_t g = 0; g < nbatches; g++) {
      size_t at = 0;
      for (uint64_t k = g * (uint64_t)B; k < std::min<uint64_t>(total, (g + 1) * (uint64_t)B); k++) {
        const SensFrame& fd = s->frames[first + k];
        zoff[k] = (uint32_t)at;
        if (fd.pose[0] == -INFINITY) continue;
        zmode[k] = fd.depth && fd.depth_bytes - 2 <= depth_b && inflate_gpu_takes(fd.depth, fd.depth_bytes) ? 1 : 0;
        at += zmode[k] ? round_up((size_t)fd.depth_bytes - 2, 64) : round_up(depth_b, 64);
      }
      zbytes[g] = (uint32_t)at;
      packed_depth = std::max(packed_depth, at);
    }
  }
  // the geometry.  Every size grows with B and with each of the facts, which is what lets sf_fuse_run_prepare ask for enough with upper bounds of them.
  void lay_out() {
    gpu_jpeg = wants_jpeg_probe() && pay_blocks != 0;
    if (gpu_jpeg) {
      // room for the table and as many entries as the pixels have bytes: a frame with more non-zero coefficients than that (finer than
      // anything a camera compresses to) is decoded on the host
      pay_b = round_up(sizeof(SfJpegLayout) + 4 * (size_t)pay_blocks + rgb_b, 256);
      planes_b = round_up(jpeg_plane_bytes, 256);
      pay_entries = (uint32_t)((pay_b - sizeof(SfJpegLayout) - 4 * (size_t)pay_blocks) / 4);
    }
    ycc_ok = gpu_jpeg && !sw.jpeg_rgb_image;
    gpu_huffman = gpu_jpeg && !sw.jpeg_host_huffman && (sw.jpeg_gpu_huffman || SF_JPEG_DEVICE_HUFFMAN_DEFAULT(gpu_inflate));
    NB = (int)std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(gpu_inflate ? 3 + NZ : 3, ((uint64_t)nthreads + B - 1) / B + 2), std::max<uint64_t>(nbatches, 1)));
    slot_depth = round_up(gpu_inflate ? packed_depth : depth_b * B, 256);
    dslot_depth = gpu_inflate ? round_up(depth_b * B, 256) : slot_depth;
    col_b = std::max(rgb_b, pay_b);
    slot_col = round_up(col_b * B, 256);
    slot_planes = planes_b * B;
    hcol_b = gpu_huffman ? round_up(max_color_bytes + sizeof(SfJpegLayout) + sizeof(SfJpegHuffDesc) + 64, 256) : col_b;
    hslot_col = round_up(hcol_b * B, 256);
    slot_b = slot_depth + hslot_col;
    // the packed depth part on the device, with 256 readable bytes behind it (the lanes of k_inflate_tokens fetch 64 bytes at a time, two fetches ahead)
    slot_comp = gpu_inflate ? slot_depth + 256 : 0;
    dslot_b = dslot_depth + slot_col + (gpu_jpeg ? slot_col : 0) + slot_planes + slot_comp;   // every colour area strides by col_b: runs copy as one piece
  }
  // two copy streams = two SDMA engines: one alone moves ~20 GB/s.  With the GPU inflate the batch's depth rides on its inflate stream (copy, tokens,
  // copies-kernel of batch g, then the copy of batch g + NZ) and the copy streams carry the colour part only (behind the inflate kernels of an earlier
  // batch it arrived late).  Scratch of the inflate kernels: one u16 per output byte, one per stream.
  ResourceNeed need() const {   // (NZ <= MAX_NZ)
    return {gpu_inflate ? NZ : 0, (!gpu_inflate || use_rgb) ? MAX_COPY : 0, (size_t)NB * slot_b, (size_t)NB * dslot_b, gpu_inflate ? 2 * depth_b * (size_t)B : 0};
  }
  uint16_t* h_depth(int sl, int j) const { return (uint16_t*)(h_pool + (size_t)sl * slot_b + (size_t)j * depth_b); }
  uint8_t* d_depth(int sl, int j) const { return d_pool + (size_t)sl * dslot_b + (size_t)j * depth_b; }
  uint8_t* h_rgb(int sl, int j) const { return h_pool + (size_t)sl * slot_b + slot_depth + (size_t)j * hcol_b; }   // pixels, coefficients or a prepared segment
  uint8_t* d_rgb(int sl, int j) const { return d_pool + (size_t)sl * dslot_b + dslot_depth + (size_t)j * col_b; }
  uint8_t* d_pay(int sl, int j) const { return d_pool + (size_t)sl * dslot_b + dslot_depth + slot_col + (size_t)j * col_b; }
  uint8_t* d_planes(int sl, int j) const { return d_pool + (size_t)sl * dslot_b + dslot_depth + 2 * slot_col + (size_t)j * planes_b; }
  uint8_t* h_stage(int sl) const { return h_pool + (size_t)sl * slot_b; }                    // the packed depth part (GPU inflate)
  uint8_t* d_stage(int sl) const { return d_pool + (size_t)(sl + 1) * dslot_b - slot_comp; }   // ... on the device, behind everything else of the slot
};

// What sf_fuse_run sets up and does not need fresh: up to eight streams (a hardware queue each: ~5 ms to create, and the runtime creates them one
// after the other whatever the threads do), the pinned pool (~6 ms per 100 MB), the device pool and the inflate kernels' scratch.  Kept per device for the
// life of the process and handed to one run at a time -- a dataset rebuild fuses 1513 scans in a process; a run that finds the set taken makes its own.
struct RunResources {
  int device = -1;
  bool taken = false;
  hipStream_t copy[MAX_COPY] = {}, inflate[MAX_NZ] = {};
  uint8_t* h_pool = nullptr;
  size_t h_bytes = 0;
  uint8_t* d_pool = nullptr;   // the ring's device side: kept too -- the first DMA into freshly allocated device memory blocked
  size_t d_bytes = 0;          // the enqueueing thread 0.4 ms per call (36 ms of a first run's loop)
  uint8_t* d_plan[MAX_NZ] = {};
  size_t plan_bytes = 0;       // of EVERY entry of d_plan
  std::thread prep;   // sf_run_resources_prepare: grows the set in the background; joined by whoever takes the set first
};
// Brings the set up to what a run needs; what it has beyond that stays.  The one place where the set's streams and memory are made: called by the preparation
// thread (touch: it also pays what the first transfer out of / into fresh memory costs) and by a run that finds the set too small, or makes its own.
hipError_t grow_resources(RunResources* r, const ResourceNeed& w, bool touch) {
  hipError_t first = hipSuccess;   // a run stops at its first failure; the preparation thread makes what it can and leaves the rest, and the report, to the run
  auto failed = [&](hipError_t e) { if (e != hipSuccess && first == hipSuccess) first = e; return e != hipSuccess; };
  // either path creates its streams in the order it always did (the runtime deals hardware queues out as they come): a run makes its copy streams first
  for (int pass = 0; pass < 2; pass++) {
    const bool side = (pass == 0) == touch;
    hipStream_t* have = side ? r->inflate : r->copy;
    for (int q = 0; q < (side ? w.side_streams : w.copy_streams); q++)
      if (!have[q] && failed(create_side_stream(&have[q]))) { have[q] = nullptr; break; }
    if (first != hipSuccess && !touch) return first;
  }
  if (w.pinned_bytes > r->h_bytes) {
    if (r->h_pool) (void)hipHostFree(r->h_pool);
    r->h_pool = nullptr; r->h_bytes = 0;
    if (failed(hipHostMalloc((void**)&r->h_pool, w.pinned_bytes, hipHostMallocDefault))) r->h_pool = nullptr;
    else r->h_bytes = w.pinned_bytes;
  }
  bool fresh_device = false;
  if (w.device_bytes > r->d_bytes && (first == hipSuccess || touch)) {
    if (r->d_pool) (void)hipFree(r->d_pool);
    r->d_pool = nullptr; r->d_bytes = 0;
    if (failed(hipMalloc((void**)&r->d_pool, w.device_bytes))) r->d_pool = nullptr;
    else { r->d_bytes = w.device_bytes; fresh_device = true; }
  }
  if (first != hipSuccess && !touch) return first;
  // the first DMA out of freshly page-locked memory pays for mapping it (measured: the first run's hipMemcpyAsync calls blocked 0.4 ms each, 37-48 ms
  // of a run): one pass of copies over both pools here, on the preparation thread, pays it before the run
  if (touch && r->h_pool && r->d_pool)
    for (size_t at = 0; at < r->h_bytes; at += r->d_bytes)
      if (hipMemcpy(r->d_pool, r->h_pool + at, std::min(r->d_bytes, r->h_bytes - at), hipMemcpyHostToDevice) != hipSuccess) break;
  if (touch && fresh_device) (void)hipMemset(r->d_pool, 0, r->d_bytes);
  if (w.plan_bytes != 0) {
    if (r->plan_bytes < w.plan_bytes) {   // scratch of another frame size: start over
      for (uint8_t*& q : r->d_plan) { if (q) (void)hipFree(q); q = nullptr; }
      r->plan_bytes = w.plan_bytes;
    }
    // every entry holds r->plan_bytes (>= this need): an entry allocated NOW gets that size too, or a later run whose need lies between the two would
    // reuse it undersized (a device out-of-bounds write of k_inflate_*)
    for (int q = 0; q < w.side_streams; q++) {
      if (r->d_plan[q]) continue;
      if (failed(hipMalloc((void**)&r->d_plan[q], r->plan_bytes))) { r->d_plan[q] = nullptr; break; }
      if (touch) (void)hipMemset(r->d_plan[q], 0, r->plan_bytes);
    }
  }
  return first;
}
void free_resources(RunResources* r) {   // of a set that is not the process's
  for (hipStream_t q : r->inflate) if (q) (void)hipStreamDestroy(q);
  for (hipStream_t q : r->copy) if (q) (void)hipStreamDestroy(q);
  if (r->h_pool) (void)hipHostFree(r->h_pool);
  if (r->d_pool) (void)hipFree(r->d_pool);
  for (uint8_t* q : r->d_plan) if (q) (void)hipFree(q);
}
std::mutex g_res_mu;
std::vector<RunResources*> g_res;   // never freed: the streams and the pools die with the process
struct JoinAtExit {
  ~JoinAtExit() {
    std::lock_guard<std::mutex> lk(g_res_mu);
    for (RunResources* r : g_res)
      if (r->prep.joinable()) r->prep.join();
  }
} g_join_at_exit;
RunResources* acquire_resources(int device) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  for (RunResources* r : g_res)
    if (r->device == device && !r->taken) {
      if (r->prep.joinable()) r->prep.join();   // the preparation thread never takes g_res_mu
      r->taken = true;
      return r;
    }
  for (RunResources* r : g_res)
    if (r->device == device) return nullptr;   // taken: the caller works with resources of its own
  RunResources* r = new RunResources;
  r->device = device;
  r->taken = true;
  g_res.push_back(r);
  return r;
}
void release_resources(RunResources* r) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  r->taken = false;
}

// Grows the device's set on a thread of its own.  The first sf_fuse_run of a process used to pay for its set inside its timed loop -- a JPEG-colour scan wants
// 8 slots, five side streams, two copy streams, 170 MB pinned and 2.7 GB of device memory: 52 ms of set-up and ~110 ms of copy calls that blocked on fresh
// memory, of a scan that is fused in 0.3 s (profiles/r06_e2e_phase_clock.txt), and one process per scan is the pipeline's contract
// (Server/scan_processor.py:138).  sf_fuse_run_prepare sizes the set from the file before the fuser is created; the work runs beside sf_fuser_create.
void sf_run_resources_prepare(int device, const ResourceNeed& w) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  RunResources* r = nullptr;
  for (RunResources* q : g_res)
    if (q->device == device) {
      if (q->taken) return;   // a run is using the set
      r = q;
    }
  if (r) {
    if (r->prep.joinable()) r->prep.join();   // the preparation thread never takes g_res_mu
    int have_side = 0, have_copy = 0;
    for (hipStream_t x : r->inflate) have_side += x != nullptr;
    for (hipStream_t x : r->copy) have_copy += x != nullptr;
    if (r->h_bytes >= w.pinned_bytes && r->d_bytes >= w.device_bytes && (w.plan_bytes == 0 || r->plan_bytes >= w.plan_bytes) && have_side >= w.side_streams &&
        have_copy >= w.copy_streams)
      return;
  } else {
    r = new RunResources;
    r->device = device;
    g_res.push_back(r);
  }
  try {
    r->prep = std::thread([r, device, w]() {
      if (hipSetDevice(device) != hipSuccess) return;
      if (w.side_streams > 0) inflate_gpu_warm();                       // the code objects of the kernels the side streams run
      if (w.side_streams > 3) { jpeg_gpu_warm(); jpeg_huff_gpu_warm(); }   // (five side streams: a JPEG-colour scan)
      (void)grow_resources(r, w, true);
    });
  } catch (...) {
    // no thread: the first run sets everything up itself
  }
}

// The ring.  Frames are handled in batches of B = sf_fuser_batch_frames(): batch g lives in ring slot g % NB.
//   decode pool : frame k is decoded as soon as batch (k / B) - NB has left its pinned buffers (counter `landed`, advanced by ONE
//                 thread that follows the copy events); the workers never enter the HIP runtime and share no lock -- progress
//                 counters are atomics polled with a short sleep (a mutex + condition variable woke 64 threads per frame and
//                 cost more than the decoding)
//   the caller's thread : waits until a batch is fully decoded, queues ONE H2D copy per run of consecutive valid frames (up to
//                 B x 614 KB per call instead of B calls) on the copy stream, then the batch's kernels
// One ring slot = one batch of B frames: contiguous pinned host buffers, contiguous device buffers, its events.
struct BatchSlot {
  hipEvent_t copied = nullptr;    // H2D of this batch finished (its pinned buffers may be refilled)
  hipEvent_t copied_rgb = nullptr;  // the colour part of it, on the other copy stream
  hipEvent_t copied_rgb2 = nullptr; // ... its second half, when that has a stream of its own
  hipEvent_t inflated = nullptr;    // the frames that travelled compressed are pixels now (recorded on the inflate stream)
  // pre-pass of this batch finished (its device buffers may be overwritten): one event per input stream a sub-batch of the slot ran on --
  // the fuser orders its two streams among themselves, but the ring does not lean on that
  hipEvent_t consumed[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  std::atomic<int> decoded{0};    // frames of the current generation the pool has finished with
  std::atomic<int> failed{0};
  // per frame, what the pinned colour area holds: 0 = RGB; 1 = JPEG coefficients (the host entropy-decoded, the GPU reconstructs);
  // 2 = the entropy-coded segment, prepared (the GPU decodes AND reconstructs); 3 = nothing: the pixels are in the frame's pageable fall-back buffer
  uint8_t coef_mode[MAX_BATCH] = {0};
  uint32_t pay_used[MAX_BATCH] = {0};    // bytes of that payload
  bool packed_segs = false;   // every colour frame of the batch travelled as a prepared segment and the batch's segments went to the device as ONE piece (two halves):
                              // frame j's segment sits at d_rgb(slot, 0) + j * hcol_b -- the pinned stride -- instead of at the head of its own pixel area
  hipError_t create_events() {
    hipError_t e = hipSuccess;
    for (hipEvent_t* ev : {&copied, &copied_rgb, &copied_rgb2, &inflated, &consumed[0], &consumed[1]})
      if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    return e;
  }
  ~BatchSlot() {
    for (hipEvent_t ev : {copied, copied_rgb, copied_rgb2, inflated, consumed[0], consumed[1]}) if (ev) (void)hipEventDestroy(ev);
  }
};

void nap() { std::this_thread::sleep_for(std::chrono::microseconds(20)); }

struct DecodePool {   // the host threads of a run and what they share with the thread that queues the GPU work
  const sf_sens* s;
  const uint64_t first, total;
  const RunPlan& p;
  std::vector<BatchSlot>& ring;
  std::vector<std::vector<uint8_t>> fallback_rgb;   // coef_mode 3: pixels a host thread decoded, pageable, per slot and frame
  std::atomic<uint64_t> next{0}, landed{0}, issued{0};  // frame counter of the pool; batches whose copies completed / were queued
  std::atomic<bool> abort{false};
  std::atomic<uint64_t> decode_ns{0};
  std::mutex err_mu;
  std::string pool_err; int pool_rc = SF_OK;   // the first failure of a worker, under err_mu
  std::vector<std::thread> workers;
  std::thread reaper;
  DecodePool(const sf_sens* s_, uint64_t first_, uint64_t total_, const RunPlan& p_, std::vector<BatchSlot>& ring_)
      : s(s_), first(first_), total(total_), p(p_), ring(ring_), fallback_rgb(p_.gpu_huffman ? (size_t)p_.NB * p_.B : 0) {}
  void start(int device) {
    for (int t = 0; t < p.nthreads; t++) workers.emplace_back([this] { work(); });
    reaper = std::thread([this, device] { reap(device); });
  }
  void join(bool failed) {
    if (failed) abort.store(true);
    for (std::thread& t : workers) t.join();
    if (failed) issued.store(p.nbatches + 1);
    reaper.join();
  }
  int decode_colour(uint64_t frame, int sl, int j, int* mode) {
    const SensFrame& fr = s->frames[frame];
    BatchSlot& bs = ring[(size_t)sl];
    uint8_t* pay = p.h_rgb(sl, j);
    *mode = 0;
    if (p.gpu_jpeg) {
      // the DEVICE area strides by col_b: a longer entropy segment takes the host path
      if (p.gpu_huffman && jpeg_prepare_huff(fr.color, fr.color_bytes, p.color_w, p.color_h, pay, std::min(p.hcol_b, p.col_b)) == SF_OK &&
          reinterpret_cast<const SfJpegLayout*>(pay)->nblocks == p.pay_blocks) {
        *mode = 2;
        bs.pay_used[j] = (uint32_t)(sizeof(SfJpegLayout) + sizeof(SfJpegHuffDesc) + 4 * (size_t)reinterpret_cast<const SfJpegHuffDesc*>(pay + sizeof(SfJpegLayout))->ecs_words);
      } else if (p.gpu_huffman) {
        // not a picture for the device: the host decoder's pixels, in a buffer of this frame's own (the pinned slot has no room for them)
        *mode = 3;
        try {
          std::vector<uint8_t>& fb = fallback_rgb[(size_t)sl * p.B + (size_t)j];
          fb.resize(p.rgb_b);
          return sf_sens_decode_color(s, frame, fb.data());
        } catch (...) { return sf::fail(SF_ERR_IO, "out of memory decoding colour frame %llu", (unsigned long long)frame); }
      } else if (jpeg_decode_coef(fr.color, fr.color_bytes, p.color_w, p.color_h, pay, p.pay_b) == SF_OK && reinterpret_cast<const SfJpegLayout*>(pay)->nblocks == p.pay_blocks) {
        *mode = 1;
        bs.pay_used[j] = (uint32_t)sf_jpeg_payload_bytes(*reinterpret_cast<const SfJpegLayout*>(pay));
      }
    }
    return *mode ? SF_OK : sf_sens_decode_color(s, frame, pay);   // raw colour, or a JPEG the GPU path does not take (errors surface here)
  }
  void work() {
    for (;;) {
      const uint64_t k = next.fetch_add(1);
      if (k >= total || abort.load(std::memory_order_relaxed)) return;
      const uint64_t g = k / (uint64_t)p.B;
      const int j = (int)(k % (uint64_t)p.B), sl = (int)(g % (uint64_t)p.NB);
      while (g >= landed.load(std::memory_order_acquire) + (uint64_t)p.NB) {  // batch g - NB still owns the pinned buffers
        if (abort.load(std::memory_order_relaxed)) return;
        nap();
      }
      const uint64_t frame = first + k;
      const auto t0 = std::chrono::steady_clock::now();
      int rc = SF_OK;
      const SensFrame& fd = s->frames[frame];
      if (fd.pose[0] != -INFINITY) {
        if (p.gpu_inflate && p.zmode[k]) {
          uint8_t* dst = p.h_stage(sl) + p.zoff[k];
          const size_t nb = (size_t)fd.depth_bytes - 2;
          std::memcpy(dst, fd.depth + 2, nb);
          for (size_t q = nb; q & 63; q++) dst[q] = 0;   // the device reads whole words; the segment is whole 64 bytes
        } else {
          rc = sens_decode_depth(s, frame, p.gpu_inflate ? reinterpret_cast<uint16_t*>(p.h_stage(sl) + p.zoff[k]) : p.h_depth(sl, j));
        }
        if (rc == SF_OK && p.use_rgb && fd.color_bytes) {
          int mode = 0;
          rc = decode_colour(frame, sl, j, &mode);
          ring[(size_t)sl].coef_mode[j] = (uint8_t)mode;
        }
      }
      decode_ns.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
      if (rc != SF_OK) {
        std::lock_guard<std::mutex> lk(err_mu);
        if (pool_rc == SF_OK) { pool_rc = rc; pool_err = sf_last_error(); }
        ring[(size_t)sl].failed.fetch_add(1);
      }
      ring[(size_t)sl].decoded.fetch_add(1, std::memory_order_release);
    }
  }
  void reap(int device) {  // the only other thread inside the HIP runtime: copies complete in order on the copy stream
    (void)hipSetDevice(device);
    for (uint64_t g = 0; g < p.nbatches; g++) {
      while (issued.load(std::memory_order_acquire) <= g) {
        if (abort.load(std::memory_order_relaxed)) return;
        nap();
      }
      (void)hipEventSynchronize(ring[(size_t)(g % (uint64_t)p.NB)].copied);
      landed.store(g + 1, std::memory_order_release);
    }
  }
};
struct Batch {   // what the steps of a batch hand to each other
  uint64_t g = 0, k0 = 0;   // its number; the index of its first frame in the run
  int sl = 0, cnt = 0;      // its ring slot, its frames
  BatchSlot* bs = nullptr;
  bool valid[MAX_BATCH], rgbf[MAX_BATCH];   // per frame: has a pose; ... and colour to fuse
  hipStream_t cs_depth = nullptr, cs_rgb = nullptr, cs_rgb2 = nullptr, side = nullptr;
  bool any_comp = false, any_rgb = false;    // a frame travelled compressed; a colour frame travelled
  bool side_work = false, side_jpeg = false, ycc_batch = false;   // `inflated` was recorded; the side stream reconstructed the pictures; ... as planes only
};
// One sf_fuse_run: what its steps share, and the owner of what lives as long as the run -- the ring's events, the status buffers, the hold on the resource set.
struct Run {
  sf_fuser* f;
  const sf_sens* s;
  const uint64_t first, total;
  RunPlan p;
  std::vector<BatchSlot> ring;
  RunResources* res = nullptr;   // nullptr: another run of this process holds the device's set
  RunResources own;
  bool holding = false;
  RunResources* r = nullptr;     // the set the run works with: res, or own
  ResourceNeed w{};              // ... and what of it the run uses
  sf::DevBuf d_zstatus;   // 2 ints per ring slot and frame, written by the device's inflate only when a frame fails
  sf::DevBuf d_jstatus;   // ... by the device's entropy decoder only when a picture fails
  int result = SF_OK;
  std::string err;
  uint64_t n_int = 0, n_skip = 0, n_dev_z = 0, n_host_z = 0, n_dev_j = 0, n_host_j = 0;
  double t_wait_ready = 0, t_api = 0, t_flush = 0, t_launch_z = 0, t_memcpy = 0;   // SF_RUN_TIMING
  Run(sf_fuser* f_, const sf_sens* s_, uint64_t first_, uint64_t last_, int decode_threads)
      : f(f_), s(s_), first(first_), total(last_ - first_), p(s_->info, f_->pk.cW, f_->pk.cH, f_->batch, RunSwitches::from_env(), decode_threads) {}
  ~Run() { release(); }
  double tick() const { return p.sw.timing ? now_s() : 0; }
  bool fail_hip(const char* what, hipError_t e) { result = SF_ERR_DEVICE; err = std::string(what) + hipGetErrorString(e); return false; }
  bool fail_rc(int rc) { result = rc; err = sf_last_error(); return false; }
  void plan() {
    res = acquire_resources(f->device), holding = true;   // (joins the preparation thread)
    p.nbatches = (total + (uint64_t)p.B - 1) / (uint64_t)p.B;
    if (p.wants_jpeg_probe())
      for (uint64_t k = first; k < first + total; k++) {   // the first colour frame's layout
        const SensFrame& fr = s->frames[k];
        if (fr.pose[0] == -INFINITY || fr.color_bytes == 0) continue;
        const uint64_t padded = (uint64_t)((p.color_w + 15) & ~15u) * ((p.color_h + 15) & ~15u);
        std::vector<uint32_t> probe((sizeof(SfJpegLayout) + padded * 3 / 64 * 4 + padded * 3 * 4) / 4 + 64);
        if (jpeg_decode_coef(fr.color, fr.color_bytes, p.color_w, p.color_h, reinterpret_cast<uint8_t*>(probe.data()), probe.size() * 4) != SF_OK) break;
        const SfJpegLayout* L = reinterpret_cast<const SfJpegLayout*>(probe.data());
        p.pay_blocks = L->nblocks;
        p.jpeg_plane_bytes = sf_jpeg_plane_bytes(*L);
        break;
      }
    if (p.gpu_inflate) p.pack_depth(s, first, total);
    for (uint64_t k = first; k < first + total; k++) p.max_color_bytes = std::max<size_t>(p.max_color_bytes, (size_t)s->frames[k].color_bytes);
    p.lay_out();
  }
  // Streams and pools come from the process-wide set when it is free (the first run on a device that nobody prepared grows it: 23 ms for a depth-only run,
  // 55 ms with colour, of a scan that is fused in 0.25 s); the status buffers and the events are the run's own.
  hipError_t acquire() {
    r = res ? res : &own, w = p.need();
    hipError_t e = grow_resources(r, w, false);
    if (e != hipSuccess) return e;
    p.h_pool = r->h_pool;
    p.d_pool = r->d_pool;
    const size_t status_b = (size_t)p.NB * p.B * 8;
    for (sf::DevBuf* st : {p.gpu_inflate ? &d_zstatus : nullptr, p.gpu_huffman ? &d_jstatus : nullptr}) {
      if (st && (e = st->alloc(status_b)) != hipSuccess) return e;
      if (st && (e = hipMemset(st->p, 0, status_b)) != hipSuccess) return e;
    }
    ring = std::vector<BatchSlot>((size_t)p.NB);
    for (BatchSlot& sl : ring)
      if ((e = sl.create_events()) != hipSuccess) return e;
    return hipSuccess;
  }
  void release() {
    if (!holding) return;
    holding = false;
    ring.clear();
    d_jstatus.release();
    d_zstatus.release();
    if (res) release_resources(res);
    else free_resources(&own);
  }
  bool wait_decoded(DecodePool& pool, Batch& b) {
    const double t0 = tick();
    while (b.bs->decoded.load(std::memory_order_acquire) < b.cnt) nap();
    if (p.sw.timing) t_wait_ready += now_s() - t0;
    if (b.bs->failed.load() != 0) {
      std::lock_guard<std::mutex> lk(pool.err_mu);
      result = pool.pool_rc; err = pool.pool_err;
      return false;
    }
    b.bs->decoded.store(0, std::memory_order_relaxed);  // next generation of this slot starts only after `landed` passes g
    for (int j = 0; j < b.cnt; j++) {
      const SensFrame& fr = s->frames[first + b.k0 + (uint64_t)j];
      b.valid[j] = fr.pose[0] != -INFINITY;
      b.rgbf[j] = b.valid[j] && p.use_rgb && fr.color_bytes != 0;
      if (!b.valid[j]) { n_skip++; f->frames_skipped++; }
      else if (s->info.depth_compression == 1) { if (p.gpu_inflate && p.zmode[b.k0 + (uint64_t)j]) n_dev_z++; else n_host_z++; }
      if (b.rgbf[j] && p.jpeg_colour) { if (b.bs->coef_mode[j] == 2) n_dev_j++; else n_host_j++; }
    }
    return true;
  }
  // ---- copies: one per run of consecutive valid frames
  bool queue_copies(const DecodePool& pool, Batch& b) {
    BatchSlot& bs = *b.bs;
    const int sl = b.sl, cnt = b.cnt;
    hipError_t e = hipSuccess;
    // depth on one copy stream, colour on the other, batches alternating between them: two transfers are in flight at any time
    b.cs_depth = (b.g & 1) ? r->copy[1] : r->copy[0]; b.cs_rgb = (b.g & 1) ? r->copy[0] : r->copy[1];
    b.cs_rgb2 = b.cs_depth;   // the colour part is the larger one: its second half follows the depth on the other stream
    if (p.gpu_inflate) {      // ... or: depth in front of its stream's inflate kernels, the colour halves on the two copy streams
      b.cs_depth = b.side = r->inflate[b.g % p.NZ];
      b.cs_rgb = p.use_rgb ? r->copy[0] : b.cs_depth;
      b.cs_rgb2 = p.use_rgb ? r->copy[1] : b.cs_depth;
    }
    const hipStream_t cs_depth = b.cs_depth, cs_rgb = b.cs_rgb, cs_rgb2 = b.cs_rgb2;
    const bool own_rgb2 = cs_rgb2 != cs_depth && cs_rgb2 != cs_rgb;
    for (int q = 0; q < 2 && e == hipSuccess; q++)
      if (bs.used[q]) {  // device buffers still read by this slot's previous pre-pass?
        e = hipStreamWaitEvent(cs_depth, bs.consumed[q], 0);
        if (e == hipSuccess) e = hipStreamWaitEvent(cs_rgb, bs.consumed[q], 0);
        if (e == hipSuccess && own_rgb2) e = hipStreamWaitEvent(cs_rgb2, bs.consumed[q], 0);
      }
    if (p.gpu_inflate) {   // the packed depth part in one piece
      const double tm = tick();
      if (p.zbytes[b.g]) e = hipMemcpyAsync(p.d_stage(sl), p.h_stage(sl), p.zbytes[b.g], hipMemcpyHostToDevice, cs_depth);
      if (p.sw.timing) t_memcpy += now_s() - tm;
      for (int j = 0; j < cnt; j++) b.any_comp = b.any_comp || (b.valid[j] && p.zmode[b.k0 + (uint64_t)j]);
    } else {
      for (int j = 0; j < cnt && e == hipSuccess;) {   // one copy per run of consecutive valid frames
        if (!b.valid[j]) { j++; continue; }
        int j1 = j;
        while (j1 < cnt && b.valid[j1]) j1++;
        e = hipMemcpyAsync(p.d_depth(sl, j), p.h_depth(sl, j), (size_t)(j1 - j) * p.depth_b, hipMemcpyHostToDevice, cs_depth);
        j = j1;
      }
    }
    for (int j = 0; j < cnt && e == hipSuccess;) {   // pixels: runs of frames decoded on the host
      if (!b.rgbf[j] || bs.coef_mode[j]) { j++; continue; }
      int j1 = j;
      while (j1 < cnt && b.rgbf[j1] && !bs.coef_mode[j1]) j1++;
      const int jm = j + (j1 - j + 1) / 2;
      e = hipMemcpyAsync(p.d_rgb(sl, j), p.h_rgb(sl, j), (size_t)(jm - j) * p.col_b, hipMemcpyHostToDevice, cs_rgb);
      if (e == hipSuccess && j1 > jm) e = hipMemcpyAsync(p.d_rgb(sl, jm), p.h_rgb(sl, jm), (size_t)(j1 - jm) * p.col_b, hipMemcpyHostToDevice, cs_rgb2);
      b.any_rgb = true;
      j = j1;
    }
    for (int j = 0; j < cnt && e == hipSuccess; j++) {   // pictures the host decoded into pageable buffers (the call returns once the bytes are staged)
      if (!b.rgbf[j] || bs.coef_mode[j] != 3) continue;
      e = hipMemcpyAsync(p.d_rgb(sl, j), pool.fallback_rgb[(size_t)sl * p.B + (size_t)j].data(), p.rgb_b, hipMemcpyHostToDevice, cs_rgb);
      b.any_rgb = true;
    }
    // Every frame a prepared segment (the usual batch of a JPEG-colour scan): the pinned colour areas are one contiguous piece (stride hcol_b), and so they
    // travel -- two copies per batch, one per copy stream, instead of one ~200 KB copy per frame (32 calls of the runtime per batch: 0.4-0.5 ms of this
    // thread, the largest item of the loop).  They land packed at the head of the slot's pixel region; k_jpeg_huff of the WHOLE batch has read them before
    // the first k_jpeg_rgb writes a pixel there (same stream, in order).
    bs.packed_segs = false;
    if (p.gpu_huffman && cnt > 1 && (size_t)cnt * p.hcol_b <= p.slot_col) {
      bool all2 = true;
      for (int j = 0; j < cnt; j++) all2 = all2 && b.valid[j] && b.rgbf[j] && bs.coef_mode[j] == 2;
      if (all2 && e == hipSuccess) {
        const int jm = cnt / 2;
        const size_t tail = (size_t)(cnt - 1 - jm) * p.hcol_b + bs.pay_used[cnt - 1];   // the last frame's area only as far as it is used
        e = hipMemcpyAsync(p.d_rgb(sl, 0), p.h_rgb(sl, 0), (size_t)jm * p.hcol_b, hipMemcpyHostToDevice, cs_rgb);
        if (e == hipSuccess) e = hipMemcpyAsync(p.d_rgb(sl, 0) + (size_t)jm * p.hcol_b, p.h_rgb(sl, jm), tail, hipMemcpyHostToDevice, cs_rgb2);
        bs.packed_segs = true;
        b.any_rgb = true;
      }
    }
    for (int j = 0, k = 0; j < cnt && e == hipSuccess && !bs.packed_segs; j++) {   // coefficients / entropy-coded segments: what each frame really holds, alternating streams
      if (!b.rgbf[j] || !bs.coef_mode[j] || bs.coef_mode[j] == 3) continue;
      // a prepared segment lands where the pixels will be written: it is dead once k_jpeg_huff has turned it into the coefficient payload
      e = hipMemcpyAsync(bs.coef_mode[j] == 2 ? p.d_rgb(sl, j) : p.d_pay(sl, j), p.h_rgb(sl, j), bs.pay_used[j], hipMemcpyHostToDevice, (k++ & 1) ? cs_rgb2 : cs_rgb);
      b.any_rgb = true;
    }
    if (e == hipSuccess && b.any_rgb) {   // `copied` on the depth stream stands for both parts
      e = hipEventRecord(bs.copied_rgb, cs_rgb);
      if (e == hipSuccess) e = hipStreamWaitEvent(cs_depth, bs.copied_rgb, 0);
      if (e == hipSuccess && own_rgb2) {
        e = hipEventRecord(bs.copied_rgb2, cs_rgb2);
        if (e == hipSuccess) e = hipStreamWaitEvent(cs_depth, bs.copied_rgb2, 0);
      }
    }
    if (e == hipSuccess) e = hipEventRecord(bs.copied, cs_depth);
    return e == hipSuccess || fail_hip("copy pipeline: ", e);
  }
  // ---- inflate behind the batch's copy: 1024 lanes per frame tokenise, a 256-lane workgroup per frame makes the copies (inflate_gpu.hip)
  bool queue_inflate(Batch& b) {
    if (!b.any_comp) return true;
    uint8_t* zplan = r->d_plan[b.g % p.NZ];
    const hipError_t e = hipStreamWaitEvent(b.side, b.bs->copied, 0);
    if (e != hipSuccess) return fail_hip("inflate pipeline: ", e);
    const uint32_t* zw[32]; uint32_t zn[32]; uint8_t* zo[32]; uint16_t* zb[32]; int32_t zt[32];   // the arguments of a launch
    int nz = 0, slot0 = 0;
    for (int j = 0; j <= b.cnt; j++) {
      if (j < b.cnt && b.valid[j] && p.zmode[b.k0 + (uint64_t)j]) {
        const uint64_t k = b.k0 + (uint64_t)j;
        if (nz == 0) slot0 = j;
        zw[nz] = reinterpret_cast<const uint32_t*>(p.d_stage(b.sl) + p.zoff[k]);
        zn[nz] = (uint32_t)(s->frames[first + k].depth_bytes - 2); zo[nz] = p.d_depth(b.sl, j);
        zb[nz] = reinterpret_cast<uint16_t*>(zplan + 2 * p.depth_b * (size_t)j); zt[nz] = (int32_t)(first + k);
        nz++;
      }
      if (nz == 32 || (j == b.cnt && nz > 0)) {   // a launch takes up to 32 frames
        const double tz = tick();
        const int rcz = inflate_gpu_batch(b.side, nz, zw, zn, zo, zb, (uint32_t)p.depth_b, zt, d_zstatus.as<int32_t>() + 2 * ((size_t)b.sl * p.B + (size_t)slot0));
        if (p.sw.timing) t_launch_z += now_s() - tz;
        if (rcz != SF_OK) return fail_rc(rcz);
        nz = 0;
      }
    }
    return true;
  }
  // The JPEG work of the frames [j0, j1) of a batch on `stream`: entropy decoding of the pictures that travelled as prepared segments (k_jpeg_huff: one 1024-lane
  // workgroup per picture, huff_group pictures per launch), then the reconstruction of those and of the pictures that travelled as coefficients -- their
  // component planes only (planes_only: the pre-pass converts the one pixel per depth pixel it looks up, k_prepass, YccPicture -- no k_jpeg_rgb, no 3.8 MB RGB
  // image per picture written and read back), or IDCT + upsampling + colour conversion into the frame's pixel area.
  bool queue_jpeg(const Batch& b, int j0, int j1, hipStream_t stream, int huff_group, bool planes_only) {
    const BatchSlot& bs = *b.bs;
    const int sl = b.sl;
    const uint8_t* pay[MAX_BATCH]; uint8_t* rgb[MAX_BATCH]; uint8_t* planes[MAX_BATCH];   // the pictures to reconstruct
    int nj = 0;
    const uint8_t* seg[MAX_BATCH]; uint8_t* out[MAX_BATCH]; uint32_t cap[MAX_BATCH]; int32_t tag[MAX_BATCH];   // ... to entropy-decode
    int nh = 0, slot0 = 0;
    for (int q = j0; q <= j1; q++) {
      const bool picture = q < j1 && b.rgbf[q] && (bs.coef_mode[q] == 1 || bs.coef_mode[q] == 2);
      if (picture) { pay[nj] = p.d_pay(sl, q); rgb[nj] = p.d_rgb(sl, q); planes[nj] = p.d_planes(sl, q); nj++; }
      if (picture && bs.coef_mode[q] == 2) {
        if (nh == 0) slot0 = q;
        seg[nh] = bs.packed_segs ? p.d_rgb(sl, 0) + (size_t)q * p.hcol_b : p.d_rgb(sl, q);
        out[nh] = p.d_pay(sl, q); cap[nh] = p.pay_entries; tag[nh] = (int32_t)(first + b.k0 + (uint64_t)q);
        nh++;
      }
      if (nh == huff_group || (q == j1 && nh > 0)) {
        const int rch = jpeg_gpu_huffman(stream, nh, seg, out, cap, tag, d_jstatus.as<int32_t>() + 2 * ((size_t)sl * p.B + (size_t)slot0));
        if (rch != SF_OK) return fail_rc(rch);
        nh = 0;
      }
    }
    for (int q0 = 0; q0 < nj; q0 += 16) {   // jpeg_gpu.hip reconstructs at most 16 frames per launch
      const int n = std::min(16, nj - q0);
      const int rcj = planes_only ? jpeg_gpu_planes(stream, n, pay + q0, planes + q0, p.pay_blocks)
                                  : jpeg_gpu_reconstruct(stream, n, pay + q0, rgb + q0, planes + q0, p.pay_blocks, p.color_w, p.color_h);
      if (rcj != SF_OK) return fail_rc(rcj);
    }
    return true;
  }
  // JPEG colour on the batch's side stream too (when there is one): entropy decoding of the pictures that travelled as segments and the
  // reconstruction of every picture that travelled as coefficients or segments -- beside the fusion of the batches before, three batches in flight,
  // instead of in front of this batch's pre-pass on the fuser's input stream (where a 32-picture batch cost 2 x 1.25 ms of a stream that also
  // carries allocation and compaction).  Then `inflated`: the side stream is through with the batch.
  bool queue_side_jpeg(Batch& b) {
    if (p.gpu_jpeg && p.gpu_inflate && b.any_rgb) {
      if (!b.any_comp) {
        const hipError_t e = hipStreamWaitEvent(b.side, b.bs->copied, 0);
        if (e != hipSuccess) return fail_hip("inflate / jpeg pipeline: ", e);
      }
      int pictures = 0, n_rgbf = 0;
      for (int q = 0; q < b.cnt; q++) {
        n_rgbf += b.rgbf[q] ? 1 : 0;
        pictures += b.rgbf[q] && (b.bs->coef_mode[q] == 1 || b.bs->coef_mode[q] == 2) ? 1 : 0;
      }
      b.ycc_batch = p.ycc_ok && pictures > 0 && pictures == n_rgbf;   // every colour frame of the batch a picture the device reconstructs: the planes are all the pre-pass needs
      if (!queue_jpeg(b, 0, b.cnt, b.side, 32, b.ycc_batch)) return false;
      b.side_jpeg = pictures > 0;
    }
    b.side_work = b.any_comp || b.side_jpeg;
    if (b.side_work) {
      const hipError_t e = hipEventRecord(b.bs->inflated, b.side);
      if (e != hipSuccess) return fail_hip("inflate / jpeg pipeline: ", e);
    }
    return true;
  }
  // ---- kernels: the valid frames in order, a sub-batch is all-colour or all-geometry
  bool fuse_sub_batches(Batch& b) {
    BatchSlot& bs = *b.bs;
    const int sl = b.sl, cnt = b.cnt;
    hipStream_t used_streams[2] = {nullptr, nullptr};   // the input streams this slot's sub-batches ran on
    for (int j = 0; j < cnt;) {
      if (!b.valid[j]) { j++; continue; }
      const void *dd[MAX_BATCH], *dr[MAX_BATCH], *dl[MAX_BATCH];
      const float* pp[MAX_BATCH];
      int m = 0;
      const bool rgb = b.rgbf[j];
      const int jfirst = j;
      for (; j < cnt && m < p.B && (!b.valid[j] || b.rgbf[j] == rgb); j++) {
        if (!b.valid[j]) continue;
        const uint64_t k = b.k0 + (uint64_t)j;
        // pixels: inflated on the device into the slot's frame area, or (a stream the device does not take) as the host thread decoded them
        dd[m] = (p.gpu_inflate && !p.zmode[k]) ? p.d_stage(sl) + p.zoff[k] : p.d_depth(sl, j);
        dr[m] = rgb ? (b.ycc_batch ? p.d_planes(sl, j) : p.d_rgb(sl, j)) : nullptr;
        dl[m] = (rgb && b.ycc_batch) ? p.d_pay(sl, j) : nullptr;
        pp[m++] = s->frames[first + k].pose;
      }
      hipStream_t in_stream = sf_input_stream(f, m, rgb, +1);  // the stream this sub-batch's pre-pass runs on
      if (hipStreamWaitEvent(in_stream, bs.copied, 0) != hipSuccess || (b.side_work && hipStreamWaitEvent(in_stream, bs.inflated, 0) != hipSuccess)) {
        result = SF_ERR_DEVICE; err = "hipStreamWaitEvent failed";
        return false;
      }
      // no side stream (depth not inflated on the device): the JPEG work of this sub-batch's frames ahead of its pre-pass, 16 pictures per entropy-decoding launch
      if (rgb && p.gpu_jpeg && !b.side_jpeg && !queue_jpeg(b, jfirst, j, in_stream, 16, false)) return false;
      const int rc = (rgb && b.ycc_batch) ? sf_fuser_run_batch_ycc(f, dd, dr, dl, pp, m) : sf_fuser_run_batch(f, dd, rgb ? dr : nullptr, pp, m);
      if (rc != SF_OK) return fail_rc(rc);
      n_int += (uint64_t)m;
      if (used_streams[0] == nullptr || used_streams[0] == in_stream) used_streams[0] = in_stream;
      else used_streams[1] = in_stream;
    }
    for (int q = 0; q < 2; q++) {
      bs.used[q] = used_streams[q] != nullptr;   // false: nothing on that stream read the device buffers
      if (bs.used[q]) (void)hipEventRecord(bs.consumed[q], used_streams[q]);
    }
    return true;
  }
  // A frame the device gave up on fails the run, as it would on the host: its status (2 ints per ring slot and frame: code, frame number) is non-zero.
  void read_status(const int32_t* d_status, const char* status_of, const char* frame_of, const char* what) {
    if (result != SF_OK || !d_status) return;
    std::vector<int32_t> st((size_t)p.NB * p.B * 2);
    const hipError_t re = hipMemcpy(st.data(), d_status, st.size() * 4, hipMemcpyDeviceToHost);
    if (re != hipSuccess) { fail_hip((std::string(status_of) + " could not be read back: ").c_str(), re); return; }
    for (size_t i = 0; i < st.size() && result == SF_OK; i += 2)
      if (st[i] != 0) {   // the frame itself was fused as "no measurement" (k_inflate_copy zero-fills what it gives up on)
        result = SF_ERR_FORMAT;
        err = std::string(frame_of) + std::to_string(st[i + 1]) + what + " (device status " + std::to_string(st[i]) + ")";
      }
  }
};
}  // namespace

SF_API int sf_fuse_run(sf_fuser* f, const sf_sens* s, uint64_t first, uint64_t last, int decode_threads, sf_run_stats* stats) {
  if (!f || !s) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const uint64_t nframes = s->frames.size();
  if (last == 0 || last > nframes) last = nframes;
  if (first > last) return sf::fail(SF_ERR_BOUNDS, "first frame %llu beyond last %llu", (unsigned long long)first, (unsigned long long)last);
  if ((int)s->info.depth_width != f->in_W || (int)s->info.depth_height != f->in_H)
    return sf::fail(SF_ERR_INVALID_ARG, "fuser was created for %dx%d depth frames, the .sens file holds %ux%u", f->in_W, f->in_H,
                    s->info.depth_width, s->info.depth_height);
  SF_HIP_CHECK(hipSetDevice(f->device));
  const double t_start = now_s();
  Run run(f, s, first, last, decode_threads);
  const RunPlan& p = run.p;
  const bool timing = p.sw.timing;
  run.plan();
  const double ts0 = run.tick();
  const hipError_t se = run.acquire();
  if (se != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuse_run set-up (streams, pinned and device pools) failed: %s", hipGetErrorString(se));
  const double t_setup_end = run.tick();
  if (timing)
    std::fprintf(stderr, "sf_fuse_run set-up: frame table + layout %.1f ms; streams, pinned pool, device pool, events %.1f ms\n", (ts0 - t_start) * 1e3, (t_setup_end - ts0) * 1e3);
  DecodePool pool(s, first, run.total, p, run.ring);
  pool.start(f->device);
  for (uint64_t g = 0; g < p.nbatches && run.result == SF_OK; g++) {
    Batch b;
    b.g = g; b.k0 = g * (uint64_t)p.B;
    b.sl = (int)(g % (uint64_t)p.NB); b.bs = &run.ring[(size_t)b.sl];
    b.cnt = (int)std::min<uint64_t>((uint64_t)p.B, run.total - b.k0);
    if (!run.wait_decoded(pool, b)) break;
    const double t1 = run.tick();
    if (!run.queue_copies(pool, b)) break;
    pool.issued.store(g + 1, std::memory_order_release);
    if (!run.queue_inflate(b) || !run.queue_side_jpeg(b)) break;
    const double t2 = run.tick();
    run.t_api += t2 - t1;
    run.fuse_sub_batches(b);
    if (timing) run.t_flush += now_s() - t2;
  }
  const double t_loop_end = run.tick();
  pool.join(run.result != SF_OK);
  const hipError_t qe = sf_quiesce(f);
  if (timing)
    std::fprintf(stderr, "sf_fuse_run: setup %.3f s (streams, %.0f MB pinned, %.0f MB device), loop %.3f s (wait for decoded batches %.3f, copy enqueue %.3f, kernels enqueue %.3f), "
                         "join+drain %.3f s, %d batch slots x %d frames; inside copy enqueue: packed depth memcpy calls %.3f s, inflate launches %.3f s\n",
                 t_setup_end - t_start, (double)p.NB * p.slot_b / 1e6, (double)p.NB * p.dslot_b / 1e6, t_loop_end - t_setup_end,
                 run.t_wait_ready, run.t_api, run.t_flush, now_s() - t_loop_end, p.NB, p.B, run.t_memcpy, run.t_launch_z);
  for (int q = 0; q < run.w.copy_streams; q++) (void)hipStreamSynchronize(run.r->copy[q]);
  for (int q = 0; q < run.w.side_streams; q++) (void)hipStreamSynchronize(run.r->inflate[q]);
  if (qe == hipSuccess) {
    run.read_status(run.d_zstatus.as<int32_t>(), "inflate: the device's frame status", "inflate: depth frame ", ": corrupt stream, or it does not inflate to the frame's size");
    run.read_status(run.d_jstatus.as<int32_t>(), "jpeg: the device's picture status", "jpeg: colour frame ", ": corrupt or truncated entropy-coded segment");
  }
  run.release();
  t_run_counts[0] = run.n_dev_z; t_run_counts[1] = run.n_host_z; t_run_counts[2] = run.n_dev_j; t_run_counts[3] = run.n_host_j;
  if (run.result != SF_OK) return sf::fail(run.result, "%s", run.err.c_str());
  if (qe != hipSuccess) return sf::fail(SF_ERR_DEVICE, "device error while fusing: %s", hipGetErrorString(qe));
  {   // a note, not an error: the run used more streams than the process has hardware queues (see the top of this file)
    const int streams_used = 2 + run.w.copy_streams + (p.gpu_inflate ? p.NZ : 0), queues = hardware_queues_of_the_process();
    t_run_note[0] = 0;
    if (streams_used > queues)   // through sf_fuse_run_note(), not sf_last_error(): a caller that reads a non-empty last error as a failure must not
      std::snprintf(t_run_note, sizeof(t_run_note), "sf_fuse_run drove %d streams over %d hardware queues (kernels of streams that share a queue run one after the other; "
                    "GPU_MAX_HW_QUEUES, read at the process's first HIP call, sets the number)", streams_used, queues);
  }
  if (stats) {
    stats->frames_total = run.total;
    stats->frames_integrated = run.n_int;
    stats->frames_skipped = run.n_skip;
    stats->decode_threads = (uint32_t)p.nthreads;
    stats->color_fused = p.use_rgb ? 1u : 0u;
    stats->seconds_total = now_s() - t_start;
    stats->seconds_decode_cpu = (double)pool.decode_ns.load() * 1e-9;
  }
  return SF_OK;
}

// scanfuse.h: the streams, the page-locked ring and the device ring a later sf_fuse_run of THIS file will want, made on a thread of their own from now on -- call it
// with the file open and BEFORE sf_fuser_create, whose own allocations (the volume: gigabytes to reserve and clear) then run beside it.  Nothing here changes
// what a run does, only when the set-up is paid: a set that is large enough is taken as it is, one that is not is grown by the run.
// The sizes come from the run's own RunPlan, fed with upper bounds of what the run will measure (the fuser does not exist yet); every size of the plan grows
// with each of them: MAX_BATCH frames per slot; per frame of the packed depth part the largest depth blob (what pack_depth gives a frame the device inflates,
// as it does every frame of the reference's writer -- a stream the host must inflate packs as pixels and may make the run grow the set); a picture of
// 3 x padded / 64 blocks and 3 x padded bytes of planes (no layout has more); a ring not capped by the number of batches.  So a run of the same file with the
// default batch, switches and thread count finds a set at least as large as it needs.
SF_API int sf_fuse_run_prepare(const sf_sens* s, const sf_params* prm, int device) {
  if (!s || !prm) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return sf::fail(SF_ERR_DEVICE, "no HIP device %d", device);
  if ((size_t)s->info.depth_width * s->info.depth_height == 0 || s->frames.empty()) return SF_OK;
  RunPlan p(s->info, prm->color_width, prm->color_height, MAX_BATCH, RunSwitches(), 0);
  p.nbatches = UINT64_MAX;
  size_t max_depth = 0;
  for (const SensFrame& fr : s->frames) {
    max_depth = std::max<size_t>(max_depth, (size_t)fr.depth_bytes);
    p.max_color_bytes = std::max<size_t>(p.max_color_bytes, (size_t)fr.color_bytes);
  }
  p.packed_depth = round_up(std::min(max_depth, p.depth_b), 64) * MAX_BATCH;
  const size_t padded = (size_t)((p.color_w + 15) & ~15u) * ((p.color_h + 15) & ~15u);
  p.pay_blocks = (uint32_t)(padded * 3 / 64);
  p.jpeg_plane_bytes = padded * 3;
  p.lay_out();
  sf_run_resources_prepare(device, p.need());
  return SF_OK;
}

SF_API const char* sf_fuse_run_note(void) { return t_run_note; }
// scanfuse_internal.h: where the frames of this thread's last sf_fuse_run were decoded -- out[0] depth frames inflated on the device, out[1] zlib
// depth frames inflated by the host threads, out[2] JPEG colour frames entropy-decoded on the device, out[3] by the host threads.
SF_API int sf_fuse_run_device_counts(uint64_t out[4]) {
  if (!out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  for (int i = 0; i < 4; i++) out[i] = t_run_counts[i];
  return SF_OK;
}
