/*
 * scanfuse.h -- C ABI of the MI355X-native RGB-D integration hot path (libscanfuse.so).
 *
 * This is the drop-in boundary for the `improve` and `segment` stages of the reference pipeline
 * (Server/scan_processor.py:137-138,155-156).  Plain pointers and sizes only; no exception crosses the
 * ABI.  Every function returns SF_OK (0) or a negative sf_status; the message of the last failure on the
 * calling thread is available from sf_last_error().
 *
 * Each group below cites the reference interface it replaces (paths relative to the reference root).
 */
#ifndef SCANFUSE_H
#define SCANFUSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum sf_status {
  SF_OK = 0,
  SF_ERR_INVALID_ARG = -1,
  SF_ERR_IO = -2,
  SF_ERR_FORMAT = -3,      /* bad .sens / PLY / zlib / parameter file */
  SF_ERR_UNSUPPORTED = -4, /* e.g. arithmetic-coded JPEG colour, PreserveBoundary in simplify.mlx */
  SF_ERR_DEVICE = -5,      /* HIP error, no GPU */
  SF_ERR_CAPACITY = -6,    /* SDF block heap or hash table exhausted */
  SF_ERR_BOUNDS = -7,
  SF_ERR_SKIPPED = -8,     /* frame skipped: camToWorld is all -inf (tracking lost, sensorData.h:382) */
  SF_ERR_PARAM = -9        /* a parameter beyond what a kernel can serve (sf_lut_estimator_create: n_slices); nothing was launched */
} sf_status;

const char* sf_last_error(void);
const char* sf_version(void);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction parameters.  Field names follow Server/tools/recons/zParametersScanNet.txt (the
 * mLib ParameterFile the reference passes to FriedLiver.exe / DepthSensing.exe as argv[1]).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_params {
  int32_t depth_width, depth_height;   /* size of the depth frames handed to integrate()          */
  float fx, fy, mx, my;                /* depth intrinsics (sensorData.h:305-312 layout)          */
  float depth_shift;                   /* m_depthShift, sensorData.h:895 (1000)                   */
  float depth_min, depth_max;          /* s_sensorDepthMin / Max            (:34-35)              */
  float voxel_size;                    /* s_SDFVoxelSize                    (:47)                 */
  float trunc_base, trunc_scale;       /* s_SDFTruncation / Scale           (:49-50)              */
  float max_integration_dist;          /* s_SDFMaxIntegrationDistance       (:51)                 */
  int32_t weight_sample;               /* s_SDFIntegrationWeightSample      (:52)                 */
  int32_t weight_max;                  /* s_SDFIntegrationWeightMax (:53), saturated at 255       */
  float mc_thresh_factor;              /* s_SDFMarchingCubeThreshFactor     (:48)                 */
  uint32_t hash_num_buckets;           /* s_hashNumBuckets                  (:56)                 */
  uint32_t hash_bucket_size;           /* HASH_BUCKET_SIZE (pound-defined upstream, :55) = 10     */
  uint32_t num_sdf_blocks;             /* s_hashNumSDFBlocks                (:57)                 */
  uint32_t mc_max_triangles;           /* s_marchingCubesMaxNumTriangles (:106): parsed and kept, NOT applied -- upstream's 5 000 000 is a buffer size
                                          that real scans (7.85 M faces) exceed; sf_fuser_extract_mesh sizes its buffers from the count pass */
  int32_t gc_enabled;                  /* s_garbageCollectionEnabled        (:83)                 */
  /* Colour frames at their own resolution (real ScanNet scans: 1296x968 colour, 640x480 depth, sensorData.h:1269-1272).
   * color_width == 0: rgb buffers are depth_width x depth_height.  Otherwise rgb buffers are color_width x color_height
   * and every depth pixel (x, y) takes the colour pixel under the same ray: u = (x - mx) / fx * cfx + cmx (nearest),
   * black outside the colour image -- depth and colour share the extrinsics in ScanNet's .sens files. */
  int32_t color_width, color_height;
  float cfx, cfy, cmx, cmy;            /* colour intrinsics (m_calibrationColor, sensorData.h:1264) */
  /* s_integrationWidth / s_integrationHeight (zParametersScanNet.txt:20-21, shipped as 320 x 240: "input depth gets re-sampled to this
   * width").  0 x 0: integrate at depth_width x depth_height.  Otherwise every frame is resampled to this size before anything else:
   * integration pixel (x, y) takes input pixel ((uint)(x * (depth_width - 1) / (integration_width - 1) + 0.5f), same in y) -- nearest, the
   * sampling convention of the reference's own resample kernels (AnnotationTools/Filter2dAnnotations/filter.cu:647-665) --, the intrinsics
   * follow it (fx * iw / dw, mx * (iw - 1) / (dw - 1): Calibrate/src/calibration.h:125-128), colour is looked up under the same ray. */
  int32_t integration_width, integration_height;
  /* Upstream-conformance switches (DESIGN.md section 6b "upstream vs this specification").  The TSDF algorithm lives in external code
   * (VoxelHashing / BundleFusion) that is not in the reference tree; SURVEY.md App. C is the specification built here and 0 selects it
   * everywhere.  Where the public upstream sources are remembered to differ, the other value reproduces THAT behaviour -- in the kernels,
   * in the CPU checker (oracle/tsdf_oracle.c) and in the float64 literal evaluator (oracle/spec_literal.py) alike -- so that a maintainer
   * who holds the Windows binaries can pick the semantics that match them.
   *   frustum_mode  0: a block is allocated / fused in a frame when its bounding sphere touches the view frustum (conservative: every voxel
   *                    that projects into the image is visited).
   *                 1: VoxelHashing's isSDFBlockInCameraFrustumApprox: the block CENTRE is projected, its normalised device coordinates
   *                    are scaled by 0.95 and must lie in [-1, 1]^2 x [0, 1] (z against s_sensorDepthMin / Max) -- border blocks whose
   *                    centre falls outside are neither allocated nor fused although some of their voxels project into the image.
   *   colour_round  0: running colour average (old + new) / 2 in integer arithmetic (App. C as written: truncation).
   *                 1: (uchar)(0.5f * old + 0.5f * new + 0.5f) per channel (combineVoxel upstream: round half up).
   *   colour_first  0: a voxel with weight 0 takes the observed colour as it is.
   *                 1: a voxel whose accumulated colour is black (r + g + b == 0) does (combineVoxel upstream).
   *   weight_mode   0: every observation weighs s_SDFIntegrationWeightSample (BundleFusion forces this; App. C).
   *                 1: VoxelHashing: (uchar)max(weightSample * 1.5f * (1 - (d - depthMin) / (depthMax - depthMin)), 1.0f).  With the shipped
   *                    weightSample = 1 (zParametersScanNet.txt:52) both give 1 for every depth. */
  int32_t frustum_mode, colour_round, colour_first, weight_mode;
  /*   weight_wrap   0: the 8-bit weight saturates at min(s_SDFIntegrationWeightMax, 255) (SURVEY App. C decision).
   *                 1: upstream stores min(weightMax, w0 + w1) into its `uchar weight` -- with the shipped weightMax = 99999999
   *                    (zParametersScanNet.txt:53) the 256th observation of a voxel WRAPS its weight to 0 and the running mean starts again.
   *                    weight_max is then taken as given (not clamped to 255) and the stored weight is the sum modulo 256. */
  int32_t weight_wrap;
} sf_params;

/* SURVEY 8d camera + zParametersScanNet.txt values with BASELINE.json's 4 mm / 2^19-bucket overrides */
void sf_params_default(sf_params* p);
/* Parse an mLib ParameterFile ("name = v1 v2 ...; // comment").  Unknown keys are ignored; keys that are
 * present override *p (call sf_params_default first).  Replaces GlobalAppState::readMembers upstream;
 * in-tree format examples: Alignment/src/globalAppState.h:8-41. */
int sf_params_load_file(const char* path, sf_params* p);
/* The five upstream-conformance switches at once: which = 1 "VoxelHashing" (DepthSensing.exe, the binary the `improve` stage runs,
 * Server/scan_processor.py:34-35,138): frustum_mode = colour_round = colour_first = weight_mode = weight_wrap = 1; which = 2 "BundleFusion"
 * (FriedLiver.exe, the `recons` stage, :27-29,126): the same with weight_mode = 0 (that code base computes the depth-dependent weight and then
 * forces it to 1); which = 0: SURVEY App. C (all 0, the default).  The upstream behaviour is AS REMEMBERED -- neither code base is in the
 * reference tree -- which is why it is a preset a maintainer can confirm with one mesh (INTEGRATION.md "Conformance packet"),
 * not the default.  Also a parameter-file key: s_scanfuseUpstream = 0 | 1 | 2 (applied before the five individual keys, which override it). */
int sf_params_upstream_preset(sf_params* p, int which);

/* ------------------------------------------------------------------------------------------------
 * Voxel-hash TSDF fuser.  Replaces the scene-representation calls of the external DepthSensing.exe /
 * FriedLiver.exe (call sites Server/scan_processor.py:126,138).  One fuser per HIP
 * device + stream; a handle is not thread-safe, distinct handles are independent.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_fuser sf_fuser;

typedef struct sf_stats {
  uint64_t frames_integrated, frames_skipped;
  uint32_t blocks_allocated;     /* live SDF blocks                                              */
  uint32_t heap_free;            /* free SDF blocks ("heapFreeCount" of processed.txt)           */
  uint32_t last_frame_blocks;    /* N_blk of the last integrate: allocated AND in the frustum    */
  uint32_t alloc_failures;       /* blocks that could not be allocated (heap / table exhausted)  */
  uint64_t total_frame_blocks;   /* sum of N_blk over all frames since create / reset_counters   */
  uint32_t hash_slots_used;
  uint32_t high_water;           /* 1 + highest heap block index ever handed out                 */
  uint64_t total_pass_tiles;     /* sum over the passes (of up to sf_fuser_batch_frames() frames) of the tiles the pass read and wrote:
                                    what temporal blocking moves through HBM, against total_frame_blocks for frame-by-frame fusion */
} sf_stats;

int sf_device_count(int* count);
int sf_fuser_create(const sf_params* p, int device, sf_fuser** out);
void sf_fuser_destroy(sf_fuser* f);

/* Host-buffer entry points: depth = W*H u16 (row-major, as decompressDepthAlloc returns it,
 * sensorData.h:943-946), rgb = W*H*3 u8 at depth resolution or NULL, pose = row-major camToWorld
 * (RGBDFrame::getCameraToWorld, sensorData.h:432).  The buffers have been read when the call returns (they may be reused or freed at once);
 * the fusion itself runs asynchronously (sf_fuser_sync / any later call orders behind it).  SF_ERR_SKIPPED for -inf poses. */
int sf_fuser_integrate(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float pose[16]);
int sf_fuser_deintegrate(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float pose[16]);

/* Device-buffer entry points (inputs already resident in HBM; used by bench.py and by sf_fuse_run). */
int sf_fuser_integrate_device(sf_fuser* f, const void* d_depth, const void* d_rgb, const float pose[16]);
int sf_fuser_deintegrate_device(sf_fuser* f, const void* d_depth, const void* d_rgb, const float pose[16]);
/* n frames laid out `frame_stride_bytes` apart starting at d_depth; poses = n*16 floats on the host; -inf poses are
 * skipped.  Frames are fused sf_fuser_batch_frames() at a time: one pass over the voxel tiles applies every frame of
 * the batch in frame order (temporal blocking) -- the result is bit-identical to frame-by-frame integration. */
int sf_fuser_integrate_batch_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes,
                                    const float* poses, uint64_t n);
/* The same with a colour frame per depth frame (rgb: depth_width x depth_height x 3 bytes, or color_width x color_height x 3 when sf_params
 * gives a colour resolution), `rgb_stride_bytes` apart. */
int sf_fuser_integrate_batch_device_rgb(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes,
                                        const float* poses, uint64_t n);
int sf_fuser_batch_frames(const sf_fuser* f);   /* 32 */

/* Empty volume again (table, heap, tiles, counters, frame numbering); parameters, streams and tuning stay.  The reference's tools are
 * one process per scan (Server/scan_processor.py:137-141); a caller that fuses scan after scan keeps its allocation this way. */
int sf_fuser_reset(sf_fuser* f);
int sf_fuser_garbage_collect(sf_fuser* f, uint32_t* freed);
int sf_fuser_sync(sf_fuser* f);
int sf_fuser_stats(sf_fuser* f, sf_stats* out); /* synchronises */
void* sf_fuser_stream(sf_fuser* f);            /* the hipStream_t all work of this handle is queued on */


/* Copy out the live blocks (for parity checks): coords = n*3 int32 block coordinates, voxels = n*4096
 * bytes ({float sdf; uchar r,g,b,weight} x 512, index z*64+y*8+x).  Pass NULLs to query n only. */
int sf_fuser_export_blocks(sf_fuser* f, int32_t* coords, void* voxels, uint64_t capacity, uint64_t* n);

/* The sparse volume as a dense one (scannet_amd/csrc/fuser_dense.hip; what the `freespace` stage below is made of).
 *   sf_fuser_allocate_box   every block of [lo_block, hi_block] (inclusive) that is not in the table is inserted with zeroed voxels, on the device; blocks
 *                           that exist, ghosts among them, keep their bytes and their state; *allocated = how many were new (a second call on the same box: 0).
 *                           SF_ERR_CAPACITY, with nothing changed, when the free heap cannot hold the box's missing blocks; SF_ERR_CAPACITY when an insertion
 *                           found no hash slot (the caller may sf_fuser_reset); SF_ERR_INVALID_ARG for lo > hi, 2^31 or more blocks or a coordinate outside the
 *                           table's 21 bits; SF_ERR_UNSUPPORTED while a slab or stripe partition is set.
 *   sf_fuser_known_bounds   the inclusive box, in global voxel indices, of the owned voxels with weight > 0, and their count; known == 0 leaves the boxes as they are.
 *   sf_fuser_export_dense   region [lo_voxel, lo_voxel + dims) as [z][y][x] arrays, x fastest (rgb: 3 bytes per voxel); any output may be NULL.  A voxel of a
 *                           block that is not allocated reads as {0, 0, 0}.  mode 0: sdf as stored; mode 1: the task volume, -INFINITY where weight == 0, else
 *                           sdf / voxel_size.  The region may be unaligned, negative, partly or wholly outside the allocated space.  Ordered behind everything
 *                           queued on the handle; changes nothing in the volume.  SF_ERR_INVALID_ARG for a dimension <= 0 or 2^40 or more voxels. */
int sf_fuser_allocate_box(sf_fuser* f, const int32_t lo_block[3], const int32_t hi_block[3], uint64_t* allocated);
int sf_fuser_known_bounds(sf_fuser* f, int32_t lo_voxel[3], int32_t hi_voxel[3], uint64_t* known);
int sf_fuser_export_dense(sf_fuser* f, const int32_t lo_voxel[3], const int32_t dims[3], int mode, float* sdf, uint8_t* weight, uint8_t* rgb, int dst_on_device);

/* One large scan over several GPUs (BASELINE configs[4]): the block space is cut into slabs along `axis`; a fuser with a
 * slab set still sees every frame but only allocates (hence fuses) the blocks whose coordinate on `axis` lies in
 * [lo_block, hi_block).  axis < 0 removes the partition.  Before meshing, each fuser imports -- as GHOST blocks, which are
 * read as neighbours but never fused, meshed or garbage-collected -- the lowest block layer of the slab above it (marching
 * cubes needs the +1 voxel neighbours): sf_fuser_export_blocks_where(axis, lo, lo + 1) on the owner, an all-gather (RCCL
 * over xGMI when the buffers are device tensors: dst_on_device / src_on_device = 1), sf_fuser_import_blocks(ghost = 1) on
 * the neighbour.  Slabs along x concatenate into the canonical mesh (scannet_amd/partition.py). */
int sf_fuser_set_slab(sf_fuser* f, int axis, int32_t lo_block, int32_t hi_block);
int sf_fuser_export_blocks_where(sf_fuser* f, int axis, int32_t lo, int32_t hi, int include_ghosts, int32_t* coords, void* voxels,
                                 uint64_t capacity, uint64_t* n, int dst_on_device);   /* coords = voxels = NULL: count only */
int sf_fuser_import_blocks(sf_fuser* f, const int32_t* coords, const void* voxels, uint64_t n, int ghost, int src_on_device);
/* The same partition as STRIPES: layers of `thickness_blocks` blocks along `axis`, dealt round-robin to the `world` fusers starting at
 * `origin_block` (owner = floor((c - origin) / thickness) mod world).  A slab per GPU leaves all GPUs but one idle while the camera
 * is inside one slab; stripes a fraction of the view frustum thick spread every frame over all of them, at the price of one
 * boundary layer per stripe in the exchange (1 / thickness of the blocks).
 * The exchange without host staging: sf_fuser_export_boundary writes the lowest layer of each of this fuser's slabs / stripes
 * (coords n x 3 int32, voxels n x 4096 bytes; NULLs: count only) -- into device memory with dst_on_device = 1 --, the payloads are
 * all-gathered (RCCL), and sf_fuser_import_ghosts keeps, of a gathered payload, exactly the blocks this fuser needs as ghosts (the
 * ones directly above a layer it owns); *imported = how many. */
int sf_fuser_set_stripes(sf_fuser* f, int axis, int32_t origin_block, int32_t thickness_blocks, int world, int rank);
int sf_fuser_export_boundary(sf_fuser* f, int32_t* coords, void* voxels, uint64_t capacity, uint64_t* n, int dst_on_device);
int sf_fuser_import_ghosts(sf_fuser* f, const int32_t* coords, const void* voxels, uint64_t n, int src_on_device, uint64_t* imported);

/* The exchange step itself for host programs WITHOUT a process group (bin/depthsensing --ranks N: N copies of one executable, one per GPU; callers that
 * have torch.distributed use scannet_amd/partition.py): rank r's boundary layers go to rank r - 1, rank r + 1's come in and the wanted ones are kept
 * as ghosts -- from device memory to device memory, nothing staged on the host.  Transport: RCCL (ncclSend / ncclRecv over xGMI; librccl.so is loaded
 * with dlopen when the first exchange is created) for ranks on distinct GPUs, a hipIpc mapping of the owner's buffer for ranks that share a device
 * (RCCL refuses those) or where librccl is absent; SF_EXCHANGE_AUTO picks -- identically on every rank, from notes the ranks leave in
 * `rendezvous_dir` (a directory only this run's ranks see; a file named "abort" in it makes every wait give up).  The north star's all-gather of the
 * boundary blocks is this ring shift with the blocks nobody but one neighbour needs left out (SURVEY 8e "cheaper equivalent").
 * SF_ERR_UNSUPPORTED: no device-to-device transport on every rank -- the caller falls back to its own (files). */
typedef struct sf_exchange sf_exchange;
enum { SF_EXCHANGE_AUTO = 0, SF_EXCHANGE_RCCL = 1, SF_EXCHANGE_IPC = 2 };
int sf_exchange_create(const char* rendezvous_dir, int rank, int ranks, int device, int transport, sf_exchange** out);
int sf_exchange_boundary(sf_exchange* x, sf_fuser* f, uint64_t* sent, uint64_t* received, uint64_t* kept);
const char* sf_exchange_transport(const sf_exchange* x);   /* what sf_exchange_create chose, for the log */
void sf_exchange_destroy(sf_exchange* x);

/* Fuse frames [first, last) of an opened .sens file (last = 0: to the end): a pool of `decode_threads` (0 = one
 * per core, at most 32 / 64) fills pinned buffers in frame order -- zlib depth frames as the reference's writer
 * stores them (one fixed-Huffman block, stb_image_write.h:733-736) are copied COMPRESSED and inflated on the GPU
 * (4 threads keep up); any other depth stream and JPEG / PNG colour are decoded by the pool (JPEG: entropy decoding
 * only, the rest on the GPU) --, copies and kernels are queued as frames become ready.  Replaces the frame loop around
 * RGBDFrameCacheRead (sensorData.h:1717-1831) and, inside it, decompressDepthAlloc / decompressColorAlloc
 * (sensorData.h:600-616, 693-709).  The fuser must have been created for the file's depth resolution.  Colour is fused
 * when it is stored at depth resolution or at the colour resolution given in sf_params.  Streams and the page-locked
 * pool are kept for the next call of the process.  The library never touches the process
 * environment: the run wants a hardware queue per stream (HIP's GPU_MAX_HW_QUEUES, default 4, the application's to
 * export before its first HIP call); on fewer it still returns SF_OK and leaves a "note: ..." text in sf_last_error().
 * A depth frame whose stream is corrupt fails the run with SF_ERR_FORMAT; when the device inflated it, the frame was
 * fused as "no measurement" (zero depth) before the failure reached the host -- never with another frame's pixels. */
typedef struct sf_run_stats {
  uint64_t frames_total, frames_integrated, frames_skipped;
  uint32_t decode_threads, color_fused;
  double seconds_total;       /* wall time of the call: first byte decoded -> last kernel complete */
  double seconds_decode_cpu;  /* decode time summed over the pool */
} sf_run_stats;
struct sf_sens;
int sf_fuse_run(sf_fuser* f, const struct sf_sens* s, uint64_t first, uint64_t last, int decode_threads, sf_run_stats* stats);
/* A hint about the calling thread's most recent successful sf_fuse_run that is NOT an error ("" when there is none): today, that the run drove more streams than
 * the process has hardware queues (GPU_MAX_HW_QUEUES, read by the HIP runtime at its first call: INTEGRATION.md section 4).  sf_last_error() stays empty on success. */
const char* sf_fuse_run_note(void);
/* Optional, for a process that fuses ONE scan (the pipeline's contract: one `DepthSensing.exe` per scan, Server/scan_processor.py:138): with the file open
 * and BEFORE sf_fuser_create, start making what sf_fuse_run will want for THIS file -- its side streams (a hardware queue each: ~5 ms), the page-locked ring,
 * the device ring, one pass of copies over both -- on a thread of its own, beside sf_fuser_create's own gigabytes of allocation.  A JPEG-colour scan wants
 * several times what a depth-only one does; without this call the first sf_fuse_run pays the difference inside its loop (RGB-D: 9.8 k frames/s in the first
 * run of a process against 16 k in the second).  Changes nothing a run computes. */
int sf_fuse_run_prepare(const struct sf_sens* s, const sf_params* p, int device);

/* Iso-surface extraction (marching cubes over all live blocks, exact weld): the `<id>_vh.ply` product of the
 * improve stage (Server/scan_processor.py:141, scan_stages.json:33-42).  Vertices are ordered by grid-edge key,
 * triangles by cube; the result is deterministic.  Free with sf_mesh_free; write with sf_mesh_write_ply.
 * The number of triangles is bounded by the 32-bit indices alone (sf_params.mc_max_triangles is not applied).  SF_ERR_CAPACITY, with a message that names
 * the block, when a block that takes part lies outside block coordinates -65536 .. 65535 on an axis: the grid-edge key of a vertex holds 20 bits per
 * voxel coordinate. */
struct sf_mesh;
int sf_fuser_extract_mesh(sf_fuser* f, struct sf_mesh** out);

/* Ray casting: depth, world normal and colour images of the fused volume seen from a camera (the model view DepthSensing.exe renders every frame;
 * the ray-cast keys of Server/tools/recons/zParametersScanNet.txt:22-23,36-37,61-63).  The semantics, per pixel, are DESIGN.md section "Ray casting".
 * A miss gives depth -inf, normal (-inf, -inf, -inf), colour 0, 0, 0.  A ray cast changes nothing in the volume, its counters or frame numbering. */
typedef struct sf_raycast_params {
  int32_t width, height;            /* s_rayCastWidth / Height; 0: the fuser's integration size                                  */
  float fx, fy, mx, my;             /* all 0: the fuser's depth intrinsics scaled by width / W, height / H                       */
  float depth_min, depth_max;       /* s_renderDepthMin / Max: 0.1, 6.0                                                          */
  float ray_increment_factor;       /* s_SDFRayIncrementFactor: 0.8 (sample spacing = factor x s_SDFTruncation)                  */
  float thres_sample_dist_factor;   /* s_SDFRayThresSampleDistFactor: 50.5                                                       */
  float thres_dist_factor;          /* s_SDFRayThresDistFactor: 50.0                                                             */
  int32_t refine_iters;             /* regula-falsi steps, 1..8: 3                                                               */
  int32_t reserved[4];
} sf_raycast_params;
void sf_raycast_params_default(sf_raycast_params* r);
/* the seven keys above from an mLib ParameterFile (s_rayCastWidth / Height -> width / height); keys that are absent leave *r as it is */
int sf_raycast_params_load_file(const char* path, sf_raycast_params* r);
/* The image size W x H these parameters give on this fuser (what the buffers below must hold), or SF_ERR_INVALID_ARG as the calls below. */
int sf_fuser_raycast_size(sf_fuser* f, const sf_raycast_params* r, int32_t* width, int32_t* height);
/* One pose (row-major camToWorld), host buffers, synchronous: depth W*H f32 (metres along camera z), normals W*H*3 f32, rgb W*H*3 u8; any
 * output may be NULL.  SF_ERR_INVALID_ARG for a size <= 0 after defaults, a non-finite parameter, depth_min >= depth_max, refine_iters outside
 * 1..8, a non-positive sample spacing, or a ray that would take more than 65 536 samples (DESIGN.md section "Ray casting"). */
int sf_fuser_raycast(sf_fuser* f, const float pose[16], const sf_raycast_params* r, float* depth, float* normals_xyz, uint8_t* rgb);
/* n poses (host, 16 floats each; a pose with a non-finite element in its first three rows -- the all -inf "tracking lost" pose among them --
 * gives an all-miss image), outputs in HBM image after image; queued on sf_fuser_stream behind
 * every frame queued on the handle before it, and ahead of everything queued after it. */
int sf_fuser_raycast_device(sf_fuser* f, const float* poses, uint64_t n, const sf_raycast_params* r, void* d_depth, void* d_normals_xyz, void* d_rgb);

/* Camera tracking: frame-to-model projective point-to-plane ICP over an image pyramid (what DepthSensing.exe does with the keys of
 * zParametersTrackingDefault.txt, the second argument of scan_processor.py:126), depth only through sf_fuser_track*, with a dense colour row on every
 * depth correspondence through sf_fuser_track_rgbd* (it pins the motion inside a plane, which depth alone leaves free).  The semantics, per pixel and
 * per iteration, are DESIGN.md section "Camera tracking" (4c) and "The colour term of the tracker" (4g).  The key names below are VoxelHashing's as
 * remembered (the upstream tracker is not in the reference tree).  Lists are finest level first.  A track changes nothing in the volume, its counters
 * or frame numbering. */
typedef struct sf_track_params {
  int32_t levels;                   /* s_maxLevels: pyramid levels, 1..4: 3                                                      */
  int32_t max_iters[4];             /* s_maxOuterIter: iterations per level, 1..100: 10 5 4 4                                   */
  float dist_thres[4];              /* s_distThres: metres, > 0: 0.15 0.15 0.15 0.15                                            */
  float normal_thres[4];            /* s_normalThres: smallest cosine between the two normals, -1..1: 0.7 0.7 0.7 0.7            */
  float early_out;                  /* s_residualEarlyOut: a level ends when max |xi| of an update falls below this, >= 0: 1e-5  */
  int32_t min_correspondences;      /* s_minCorrespondences: fewest level-0 correspondences, >= 6: 1000                          */
  float max_translation;            /* s_maxTranslation: metres between the guess and the result, > 0: 0.3                       */
  float max_rotation;               /* s_maxRotation: radians between the guess and the result, > 0: 0.5                         */
  sf_raycast_params raycast;        /* the model render: width, height and intrinsics must be 0 (the fuser's integration camera)  */
  /* the colour term: read by sf_fuser_track_rgbd* only, sf_fuser_track* ignore the three; sf_track_params_load_file reads no key for them */
  float colour_weight;              /* weight of the squared intensity residual beside the squared metres, finite, >= 0: 0 (off)  */
  float colour_thres;               /* largest |intensity residual| (intensity in 0..1), finite, >= 0: 0.1                        */
  float colour_gradient_min;        /* smallest gradient length per level pixel, finite, >= 0: 0.005                              */
  int32_t reserved[5];
} sf_track_params;
void sf_track_params_default(sf_track_params* t);
/* the keys above from an mLib ParameterFile (zParametersTrackingDefault.txt); keys that are absent leave *t as it is; t->raycast is not touched */
int sf_track_params_load_file(const char* path, sf_track_params* t);
typedef struct sf_track_result {
  int32_t tracked;                  /* 1: pose_out is the result; 0: lost, pose_out is all -inf (the .sens "tracking lost" pose)   */
  int32_t iterations[4];            /* iterations run per level, finest first                                                    */
  int32_t correspondences;          /* of the last level-0 system                                                               */
  float rms_residual;               /* sqrt(sum r^2 / correspondences) of that system                                           */
  int32_t lost_reason;              /* 0 tracked, 1 no usable guess / reference pose, 2 too few correspondences, 3 singular system, 4 motion above the bound */
  int32_t colour_correspondences;   /* sf_fuser_track_rgbd*: correspondences of the last level-0 system that also gave a colour row (else 0) */
  float colour_rms_residual;        /* sqrt(sum r_c^2 / colour_correspondences) of that system, intensity in 0..1                 */
  int32_t reserved[4];
} sf_track_result;
/* One depth frame (host, u16, the fuser's input size; the fuser's pre-pass rule makes metres at the integration size) tracked against the volume:
 * the model is ray-cast once at ref (NULL: the guess), the estimate starts at guess; pose_out row-major camToWorld.  Synchronous.  Sees every frame
 * queued on the handle before it.  SF_ERR_INVALID_ARG for a parameter that is out of range or not finite; a guess or reference with a non-finite
 * element gives "lost", not an error. */
int sf_fuser_track(sf_fuser* f, const uint16_t* depth, const float guess[16], const float ref[16], const sf_track_params* t, float pose_out[16],
                   sf_track_result* result);
/* The same for a depth frame already in HBM (read on sf_fuser_stream(f)). */
int sf_fuser_track_device(sf_fuser* f, const void* d_depth, const float guess[16], const float ref[16], const sf_track_params* t, float pose_out[16],
                          sf_track_result* result);
/* The same with the frame's colour picture: RGB8 at the size the fuser fuses colour at (color_width x color_height, else the
 * depth frames' own size).  Every depth correspondence whose pixel has an intensity, and whose four taps in the model's rendered colour have an intensity
 * and a gradient, adds colour_weight x the photometric row to the 6x6 system.  With colour_weight == 0 the pose, the result's fields above and the
 * system are sf_fuser_track's bits.  rgb == NULL is allowed only then.  SF_ERR_INVALID_ARG also for one of the three colour parameters negative or not
 * finite, and for a positive colour_weight on a fuser whose colour intrinsics cannot map a picture (cfx or cfy not a positive finite number). */
int sf_fuser_track_rgbd(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float guess[16], const float ref[16], const sf_track_params* t,
                        float pose_out[16], sf_track_result* result);
/* The same for a depth frame and a picture already in HBM (read on sf_fuser_stream(f)). */
int sf_fuser_track_rgbd_device(sf_fuser* f, const void* d_depth, const void* d_rgb, const float guess[16], const float ref[16], const sf_track_params* t,
                               float pose_out[16], sf_track_result* result);

/* Re-integration: the volume-side half of a trajectory correction.  sf_fuser_deintegrate* exists "when a frame's pose is revised" (SURVEY App. C;
 * BundleFusion's main loop takes up to s_maxFrameFixes frames per step out at their old pose and puts them back at the new one); these calls
 * do that for many frames in ONE pass over the tiles they touch instead of two passes per frame.  The volume afterwards is bit for bit what this
 * sequence leaves, for j = 0 .. n - 1 in order: sf_fuser_deintegrate_device(depth_j, rgb_j, old_j), then sf_fuser_integrate_device(depth_j, rgb_j, new_j).
 * An all -inf old pose: the frame was never integrated, it is only put in; an all -inf new pose: tracking is lost now, it is only taken out; both: nothing
 * happens.  sf_stats moves as that sequence moves it -- every all -inf pose is one skipped call of it, hence one count in frames_skipped, every other
 * pose one in frames_integrated -- except total_pass_tiles, which counts what the passes really read.  d_rgb may be NULL (geometry only).  Up to
 * sf_fuser_batch_frames() operations share a pass, the two of a frame always do.  Revised poses come from sf_fuser_align below (a dense-depth solver
 * over keyframes, with BundleFusion's dense colour term through sf_fuser_align_rgbd) or from the caller (sf_sens_apply_transform on part of a scan, a
 * second tracking sweep, a solver of its own): BundleFusion's SIFT matching and loop detection are not in this library; of its local / global hierarchy
 * the dense part is (sf_fuser_align_scan below). */
int sf_fuser_reintegrate_batch_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes,
                                      const float* old_poses, const float* new_poses, uint64_t n);
/* one frame from host buffers (as sf_fuser_integrate takes them); SF_ERR_SKIPPED when both poses are all -inf */
int sf_fuser_reintegrate(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, const float old_pose[16], const float new_pose[16]);

/* The trajectory manager's three keys (Server/tools/recons/zParametersScanNet.txt:25-28).  The manager itself is BundleFusion's and is not in the
 * reference tree: what the keys mean below is this library's statement, built from the file's own comments. */
typedef struct sf_reint_params {
  int32_t max_frame_fixes;          /* s_maxFrameFixes: most frames re-integrated per step, >= 0: 30                              */
  int32_t top_n_active;             /* s_topNActive: the candidates kept (largest pose change first) before that limit, >= 0: 30 */
  float min_pose_dist_sqrt;         /* s_minPoseDistSqrt: a frame is a candidate when its squared pose distance exceeds this: 0  */
  int32_t reserved[5];
} sf_reint_params;
void sf_reint_params_default(sf_reint_params* r);
/* the three keys from an mLib ParameterFile; keys that are absent leave *r as it is */
int sf_reint_params_load_file(const char* path, sf_reint_params* r);
/* One step of the manager, on the host in double precision, no GPU: which frames to re-integrate now.  Poses are n x 16 floats, row-major camToWorld:
 * what the volume holds and what it should hold.  Distance of a frame: d2 = |t_target - t_integrated|^2 (m^2) + theta^2 (rad^2), theta the angle of
 * M = R_integrated^T R_target, atan2(|(M21 - M12, M02 - M20, M10 - M01)| / 2, (trace M - 1) / 2), exactly 0 for identical poses; +inf when exactly one of the two is all -inf (the frame must go in or out); a frame with both all -inf is no candidate.
 * Candidates: d2 > min_pose_dist_sqrt.  Order: d2 descending, ties by ascending frame index; the first top_n_active are kept and of those the first
 * max_frame_fixes returned.  *n_out = how many; SF_ERR_BOUNDS (with *n_out set) when capacity is smaller. */
int sf_reint_plan(const float* integrated_poses, const float* target_poses, uint64_t n, const sf_reint_params* r, uint64_t* frames_out, uint64_t capacity,
                  uint64_t* n_out);
typedef struct sf_reint_stats {
  uint64_t steps, frames_moved, frames_removed, frames_added, passes;
  double seconds_total;
} sf_reint_stats;
/* Steps of the manager over an opened .sens file until a plan is empty (max_steps = 0) or max_steps are done: plan, decode the planned frames on a pool
 * of decode_threads (0: one per usable core, at most 32; sf_sens_decode_depth / sf_sens_decode_color), upload, re-integrate in plan order, write the new
 * poses into integrated_poses (in: what the volume holds, out: what it holds now).  with_colour: the file's colour frames (RAW or JPEG, at the size the
 * fuser fuses colour at) go with the depth.  The volume is never reset.  Synchronous. */
int sf_fuse_update_trajectory(sf_fuser* f, const struct sf_sens* s, float* integrated_poses, const float* target_poses, const sf_reint_params* r,
                              uint64_t max_steps, int with_colour, int decode_threads, sf_reint_stats* stats);

/* Global alignment: the producer of the revised poses above.  K keyframes (u16 depth at the fuser's input size, camToWorld poses) are aligned jointly
 * over a list of directed frame pairs by a depth-only projective point-to-plane term, BundleFusion's dense depth term between keyframes (the keys of
 * Server/tools/recons/zParametersBundlingScanNet.txt:22-44; the code that reads them is not in the reference tree).  The semantics, per pixel, per pair
 * and per Gauss-Newton iteration, are DESIGN.md section 4e "Global alignment".  sf_fuser_align_rgbd* add BundleFusion's dense colour term to every
 * depth correspondence (s_denseColorThresh, s_denseColorGradientMin, :24-25): it pins the motion inside a plane, which depth
 * alone leaves free.  SIFT matching, loop detection, the bilateral depth filter and the Gaussian pre-filter of the colour frames (s_colorDownSigma)
 * are not built; scans of more than 256 keyframes go through sf_fuser_align_scan* below, the dense part of BundleFusion's local / global hierarchy.
 * An alignment changes nothing in the volume, its counters or frame numbering. */
typedef struct sf_align_params {
  int32_t level;                    /* the one image size the solver works at, (W >> level) x (H >> level), 0..3: 1                 */
  int32_t down_width, down_height;  /* s_downsampledWidth / Height (:44-45); both 0: `level` decides, else the level of that size   */
  int32_t max_iters;                /* s_numGlobalNonLinIterations (:41): Gauss-Newton iterations, 1..100: 8                        */
  float dist_thres;                 /* s_denseDistThresh (:22): metres, > 0: 0.15                                                   */
  float normal_thres;               /* s_denseNormalThresh (:23): smallest cosine between the two normals, -1..1: 0.7               */
  float depth_min, depth_max;       /* s_denseDepthMin / Max (:26-27): metres; both 0: the fuser's own depth range                  */
  float early_out;                  /* the loop ends after an update with max |xi| below this, >= 0: 1e-5                          */
  int32_t min_pair_correspondences; /* a pair with fewer correspondences is dropped for that iteration, >= 1: 500                   */
  int32_t fixed_frame;              /* the keyframe that keeps its pose (the gauge), 0..K-1: 0                                      */
  float pair_max_dist;              /* sf_align_pairs: metres between two camera centres, >= 0: 1.0                                 */
  float pair_max_angle;             /* sf_align_pairs: radians between two orientations, >= 0: 0.6                                  */
  float max_translation;            /* metres between a frame's input pose and its result, > 0: 0.5                                 */
  float max_rotation;               /* radians between them, > 0: 0.5                                                               */
  /* the colour term: read by sf_fuser_align_rgbd* only, sf_fuser_align* ignore the three */
  float colour_weight;              /* weight of the squared intensity residual beside the squared metres, finite, >= 0: 0 (off)    */
  float colour_thres;               /* s_denseColorThresh: largest |intensity residual| (intensity in 0..1), finite, >= 0: 0.1      */
  float colour_gradient_min;        /* s_denseColorGradientMin: smallest gradient length per level pixel, finite, >= 0: 0.005       */
  int32_t reserved[6];
} sf_align_params;
void sf_align_params_default(sf_align_params* a);
/* s_denseDistThresh, s_denseNormalThresh, s_denseColorThresh, s_denseColorGradientMin, s_denseDepthMin / Max, s_downsampledWidth / Height and s_numGlobalNonLinIterations of an mLib ParameterFile
 * (zParametersBundlingScanNet.txt:22-44); keys that are absent leave *a as it is.  s_submapSize (:31) is the tool's keyframe stride, not a field. */
int sf_align_params_load_file(const char* path, sf_align_params* a);
typedef struct sf_align_result {
  int32_t status;                   /* 0 solved, 1 singular system, 2 fewer than two frames connected to the fixed frame            */
  int32_t iterations;               /* updates applied                                                                              */
  int32_t pairs_used;               /* pairs in the last system                                                                     */
  int32_t frames_unconnected;       /* frames with a finite pose that no kept pair connects to the fixed frame: returned as given   */
  int32_t frames_rejected;          /* frames that moved further than the bounds: returned as given                                 */
  int32_t reserved0;
  int64_t correspondences;          /* of the last system                                                                           */
  float rms_first, rms_last;        /* sqrt(sum r^2 / correspondences) of the first and of the last system                          */
  int64_t colour_correspondences;   /* sf_fuser_align_rgbd*: correspondences of the last system that also gave a colour row (else 0) */
  float colour_rms_first, colour_rms_last;   /* sqrt(sum r_c^2 / colour_correspondences), intensity in 0..1, first and last system  */
  int32_t reserved[2];
} sf_align_result;
/* The default pair list (host only, double): for i < j both (i, j) and (j, i) when j = i + 1, or when the camera centres are within pair_max_dist and the
 * orientations within pair_max_angle (sf_reint_plan's angle); ascending i, then j, the forward pair first.  A frame whose pose has a non-finite element
 * in its first three rows is in no pair.  pairs_out: 2 x capacity int32 (source, target); writing stops at the capacity, *n_out is the full count. */
int sf_align_pairs(const float* poses, uint64_t K, const sf_align_params* a, int32_t* pairs_out, uint64_t capacity, uint64_t* n_out);
/* The correction of the keyframes carried to every frame (host only, double): frame f, whose nearest keyframe at or before it is k, gets
 * (T_k' T_k^-1) T_f; frames before the first keyframe use the first; a keyframe gets its new pose as it is; a keyframe whose old or new pose is not
 * finite passes its frames to the previous usable keyframe (the first usable one when there is none before); a lost frame stays lost.
 * keyframes: K ascending frame indices; new_key_poses: K x 16. */
int sf_align_spread(const float* poses, uint64_t n, const uint64_t* keyframes, uint64_t K, const float* new_key_poses, float* poses_out);
/* K keyframes in HBM, `frame_stride_bytes` apart (read on sf_fuser_stream(f)); poses_in / poses_out K x 16 floats on the host; pairs 2 x P int32.
 * 2 <= K <= 256, 1 <= P <= 4096, source != target.  Synchronous; ordered behind every frame queued on the handle before it.  SF_ERR_INVALID_ARG for a
 * parameter or an index out of range; a system that cannot be solved is a status of *result, with poses_out = poses_in. */
int sf_fuser_align_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, uint64_t K, const float* poses_in, const int32_t* pairs, uint64_t P,
                          const sf_align_params* a, float* poses_out, sf_align_result* result);
/* The same from host frames (K x input-size u16, one after the other). */
int sf_fuser_align(sf_fuser* f, const uint16_t* depth, uint64_t K, const float* poses_in, const int32_t* pairs, uint64_t P, const sf_align_params* a,
                   float* poses_out, sf_align_result* result);
/* The same with the keyframes' colour pictures: K RGB8 pictures `rgb_stride_bytes` apart, at the size the fuser fuses colour at
 * (color_width x color_height, or depth_width x depth_height -- the size of the depth frames themselves, also where s_integrationWidth / Height resample them -- when color_width is 0).  Every depth correspondence whose source and target have an intensity
 * (and the target a gradient) adds colour_weight x a photometric row to the pair's normal equations; the solve, the pair rule and every other field of
 * the result are sf_fuser_align_device's, and with colour_weight 0 so are all their bits.  d_rgb may be NULL when colour_weight is 0 (no colour rows
 * are counted then); NULL with colour_weight > 0, a negative or non-finite weight, threshold or gradient bound: SF_ERR_INVALID_ARG. */
int sf_fuser_align_rgbd_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K,
                               const float* poses_in, const int32_t* pairs, uint64_t P, const sf_align_params* a, float* poses_out, sf_align_result* result);
/* The same from host frames (K x input-size u16 and K x colour-size RGB8, one after the other). */
int sf_fuser_align_rgbd(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, uint64_t K, const float* poses_in, const int32_t* pairs, uint64_t P,
                        const sf_align_params* a, float* poses_out, sf_align_result* result);


/* Scans of any length: groups of consecutive keyframes under the global solve.  BundleFusion solves chunks of s_submapSize
 * consecutive frames locally, each with its own gauge, and the chunks' first frames globally (Server/tools/recons/zParametersBundlingScanNet.txt:31,
 * s_submapSize = 10; the code that reads the key is not in the reference tree).  What is built here is that hierarchy for the DENSE terms above: every
 * group is sf_fuser_align*'s own problem with its first member fixed, all groups of all levels are solved at once, their first frames one level up, and
 * the top by sf_fuser_align* itself.  What is not BundleFusion's: its local level matches SIFT features and its global level uses the chunks' merged
 * features; neither is built, so a loop closure between frames of different groups acts only at the level where both frames are represented. */
typedef struct sf_align_scan_params {
  int32_t group_size;               /* frames of a group (the last of a level may have fewer), 2..16: 16                            */
  int32_t top_frames;               /* most frames of the top level, which sf_fuser_align* solves, 2..256: 256                      */
  int32_t reserved[6];
} sf_align_scan_params;
void sf_align_scan_params_default(sf_align_scan_params* s);
typedef struct sf_align_scan_result {
  int32_t levels;                   /* grouping levels below the top; 0: the call was one sf_fuser_align*                           */
  int32_t groups;                   /* groups of all levels                                                                         */
  int32_t groups_status[3];         /* how many of them ended with status 0 / 1 / 2                                                 */
  int32_t max_iterations;           /* the largest iteration count of a group or of the top                                         */
  int32_t frames_unconnected;       /* summed over the groups and the top                                                           */
  int32_t frames_rejected;          /* summed over the groups and the top                                                           */
  int64_t correspondences;          /* of the last systems, summed over the groups and the top                                      */
  sf_align_result top;              /* the top level's own result                                                                   */
  int32_t reserved[4];
} sf_align_scan_result;
/* The plan (host only, double, no GPU).  L starts as the frames whose poses are finite in rows 0..2, ascending.  While L has more than top_frames
 * frames, or sf_align_pairs on the poses of L yields more than 4096 pairs: L is split into consecutive runs of group_size (the last may be shorter,
 * down to one frame), each run is a group of this level, and L becomes the first frame of every run.  What is left of L is the top.  Groups come in
 * level order and within a level in frame order: group g has the frames members[group_first[g] .. group_first[g + 1] - 1] and the level
 * group_level[g]; its fixed frame is its first member.  group_first has room for groups_capacity + 1 values.  Writing stops at each capacity, the
 * counts are the full ones (as sf_align_pairs).  Any output array may be NULL when its capacity is 0. */
int sf_align_scan_plan(const float* poses, uint64_t K, const sf_align_params* a, const sf_align_scan_params* s, int32_t* members, uint64_t members_capacity,
                       int32_t* group_first, int32_t* group_level, uint64_t groups_capacity, int32_t* top, uint64_t top_capacity, uint64_t* n_members,
                       uint64_t* n_groups, uint64_t* n_top, int32_t* levels);
/* G groups of the K keyframes in HBM solved at once: group g has the frames members[group_first[g] .. group_first[g + 1] - 1] (1..16 of them, indices
 * into the K frames; a frame may be a member of several groups), G <= 4096, M = group_first[G] <= 8192, 1 <= K <= 4096.  poses_in / poses_out: M x 16
 * floats, one pose per member SLOT; results: one per group.  d_rgb NULL: the depth term only.  a->fixed_frame must be 0.  For a group of n >= 2
 * members, poses_out and every field of its result are bit for bit what sf_fuser_align_device (with pictures: sf_fuser_align_rgbd_device) returns for
 * that group alone: frames 0 .. n - 1, fixed_frame 0, the sf_align_pairs list of the group's own poses_in, the same parameters.  A group of one
 * member, or whose pair list is empty, has status 2, every other field 0 and its poses as given.  Per Gauss-Newton iteration all groups still
 * running share one pair table, one run of sf_fuser_align*'s kernels (in launches of at most 4096 pairs), the group solve on the device (one
 * workgroup per group) and ONE read-back; the pose update stays on the host. */
int sf_fuser_align_groups_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K,
                                 const int32_t* members, const int32_t* group_first, uint64_t G, const float* poses_in, const sf_align_params* a,
                                 float* poses_out, sf_align_result* results);
/* 2 <= K <= 4096 keyframes in HBM: sf_align_scan_plan; ALL groups of ALL levels in one sf_fuser_align_groups_device call, every group from the input
 * poses (a first frame never moves in its own group, so the levels are independent); the top by sf_fuser_align_device (with pictures:
 * sf_fuser_align_rgbd_device) over the sf_align_pairs list of the top's poses; then the corrections carried down level by level: a group whose first
 * member now has the pose T' becomes sf_align_spread(the group's solved poses, keyframes {0}, {T'}).  A frame whose pose is not finite is returned
 * as it came.  With no grouping level, poses_out and result->top are sf_fuser_align[_rgbd]_device's bits for the frames with finite poses.
 * a->fixed_frame must be 0: the first frame with a finite pose keeps its pose. */
int sf_fuser_align_scan_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K,
                               const float* poses_in, const sf_align_params* a, const sf_align_scan_params* s, float* poses_out, sf_align_scan_result* result);
/* The same from host frames (K x input-size u16 and, unless rgb is NULL, K x colour-size RGB8, one after the other). */
int sf_fuser_align_scan(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, uint64_t K, const float* poses_in, const sf_align_params* a,
                        const sf_align_scan_params* s, float* poses_out, sf_align_scan_result* result);

/* Host <-> device helpers so that callers without a HIP binding can stage inputs in HBM. */
int sf_device_malloc(int device, uint64_t bytes, void** out);
int sf_device_free(void* p);
int sf_device_upload(void* dst, const void* src, uint64_t bytes);
int sf_device_download(void* dst, const void* src, uint64_t bytes);

/* ------------------------------------------------------------------------------------------------
 * zlib codec used for .sens depth blobs.  Replaces stb::stbi_zlib_decode_malloc / stbi_zlib_compress as
 * called from SensReader/c++/src/sensorData.h:703-709 and :659-670.  Like the reference reader the
 * decoder validates the 2-byte zlib header and does NOT verify the trailing Adler-32.
 * ---------------------------------------------------------------------------------------------- */
int sf_zlib_inflate(const void* src, uint64_t src_bytes, void* dst, uint64_t dst_capacity, uint64_t* out_bytes);
int sf_zlib_deflate(const void* src, uint64_t src_bytes, void* dst, uint64_t dst_capacity, uint64_t* out_bytes);
uint64_t sf_zlib_deflate_bound(uint64_t src_bytes);

/* ------------------------------------------------------------------------------------------------
 * .sens v4 container.  Replaces ml::SensorData (SensReader/c++/src/sensorData.h:285-1936):
 *   sf_sens_open          SensorData(filename) / loadFromFile          :855-859, :1250-1290
 *   sf_sens_get_info      header members                               :1257-1273
 *   sf_sens_decode_depth  decompressDepthAlloc(frameIdx)               :943-946 (strict bounds check; the
 *                         reference's `>` off-by-one at :944 is not reproduced); caller owns dst (W*H u16)
 *   sf_sens_decode_color  decompressColorAlloc(frameIdx)               :933-936 (RAW and baseline JPEG)
 *   sf_sens_pose          m_frames[i].getCameraToWorld()               :432; *valid = 0 for the all -inf
 *                         "tracking lost" pose (:382, SensReader/c++/README.txt:55-57)
 *   sf_sens_create/add_frame/save   initDefault / addFrame / saveToFile  :891-921, :1101-1109
 *   sf_sens_set_pose      RGBDFrame::setCameraToWorld                  :436 (trajectory rewrite by `recons`)
 * The reference throws MLibException on open / version errors (:883-886, :1253-1255); here every failure is
 * a negative sf_status.  The file is memory-mapped; compressed blobs are never copied.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_sens sf_sens;

typedef struct sf_sens_info {
  uint32_t version;                    /* 4 */
  uint32_t color_width, color_height, depth_width, depth_height;
  int32_t color_compression;           /* -1 unknown, 0 raw, 1 png, 2 jpeg   (sensorData.h:346-351) */
  int32_t depth_compression;           /* -1 unknown, 0 raw u16, 1 zlib u16, 2 occi u16 (:352-357)  */
  float depth_shift;
  uint64_t num_frames, num_imu;
  float color_intrinsic[16], color_extrinsic[16], depth_intrinsic[16], depth_extrinsic[16]; /* row-major */
  char sensor_name[256];
} sf_sens_info;

typedef struct sf_sens_frame_meta_t {
  uint64_t timestamp_color, timestamp_depth;  /* microseconds (sensorData.h:440-457) */
  uint64_t color_bytes, depth_bytes;          /* compressed sizes */
} sf_sens_frame_meta_t;

int sf_sens_open(const char* path, sf_sens** out);
void sf_sens_close(sf_sens* s);
int sf_sens_get_info(const sf_sens* s, sf_sens_info* out);
int sf_sens_decode_depth(const sf_sens* s, uint64_t frame, uint16_t* dst);
int sf_sens_decode_color(const sf_sens* s, uint64_t frame, uint8_t* dst_rgb);
int sf_sens_pose(const sf_sens* s, uint64_t frame, float out16[16], int* valid);
/* SensorData::computeDepthImage(frameIdx) (:968-982): W*H floats in metres, (float)depth / depthShift, 0 -> 0.0f (its invalid value) */
int sf_sens_depth_image(const sf_sens* s, uint64_t frame, float* dst_metres);
int sf_sens_frame_meta(const sf_sens* s, uint64_t frame, sf_sens_frame_meta_t* out);
/* RGBDFrame::getColorCompressed / getDepthCompressed (sensorData.h:418-429): the frame's compressed blobs where they lie (any out pointer may be
 * NULL); valid until sf_sens_close or, for a file under construction, until the next frame is added. */
int sf_sens_frame_blobs(const sf_sens* s, uint64_t frame, const uint8_t** color, uint64_t* color_bytes, const uint8_t** depth, uint64_t* depth_bytes);
/* Writer.  `header` supplies everything but num_frames / num_imu.  color = W*H*3 RGB bytes for TYPE_RAW, an
 * already encoded blob for TYPE_JPEG / TYPE_PNG, or NULL / 0 for no colour; depth = W*H u16, compressed as
 * header->depth_compression says (0 raw, 1 zlib). */
int sf_sens_create(const sf_sens_info* header, sf_sens** out);
int sf_sens_add_frame(sf_sens* s, const uint8_t* color, uint64_t color_bytes, const uint16_t* depth, const float pose[16],
                      uint64_t timestamp_color, uint64_t timestamp_depth);
/* n depth-only frames (`frame_stride_bytes` apart; poses = n x 16 floats; depth time stamps timestamp0 + i * step) compressed on `threads`
 * threads (0 = every CPU this process may use) and appended in order -- the result is the file n sf_sens_add_frame calls would write. */
int sf_sens_add_depth_frames(sf_sens* s, const uint16_t* depth, uint64_t frame_stride_bytes, uint64_t n, const float* poses,
                             uint64_t timestamp0_us, uint64_t timestamp_step_us, int threads);
/* A frame whose colour and depth blobs are already in the container's compression types -- stored as given (what RGBDFrame::loadFromFile
 * keeps per frame, sensorData.h:743-754): transcoding, merging files, depth streams another writer compressed. */
int sf_sens_add_frame_blobs(sf_sens* s, const uint8_t* color, uint64_t color_bytes, const uint8_t* depth, uint64_t depth_bytes,
                            const float pose[16], uint64_t timestamp_color, uint64_t timestamp_depth);
int sf_sens_set_pose(sf_sens* s, uint64_t frame, const float pose[16]);
int sf_sens_save(const sf_sens* s, const char* path);
/* SensorData::loadFromImages(sourceFolder, basename = "frame-", colorEnding = "png") (sensorData.h:1468-1559, FreeImage builds only): a folder as
 * saveToImages / bin/sens writes it -- info.txt (or _info.txt), <basename>%06d.color.jpg|png (kept as the colour blob), .depth.png (16-bit grey; or
 * the .depth.pgm saveToImages really writes), .pose.txt -- into a .sens in memory (zlib depth, time stamps 0), frames until one is incomplete.
 * basename NULL: "frame-"; color_ending NULL: what frame 0 has.  scannet_amd/csrc/sens_images.cpp. */
int sf_sens_load_from_images(const char* folder, const char* basename, const char* color_ending, sf_sens** out);
/* SensorData::saveToImages(outputFolder, basename = "frame-") (sensorData.h:1380-1466): _info.txt + per frame <basename>%06d.color.jpg|png (the stored
 * blob; a TYPE_RAW frame as a PNG), .depth.pgm (16-bit big-endian, depth shift in the comment), .pose.txt -- the folder the reference writes, byte for
 * byte.  Frames are written by a pool of threads; progress (nullable) is called on the caller's thread with (frame, num_frames, user) in frame order.
 * bin/sens is this call plus the reference tool's stdout. */
int sf_sens_save_to_images(const sf_sens* s, const char* folder, const char* basename, void (*progress)(uint64_t, uint64_t, void*), void* user);
/* SensorData::saveToPointCloud(filename, frameFrom, frameTo) (:1564-1602, compiled only with mLib; the reference's statement of the unprojection, SURVEY 8a row
 * a6): every valid depth pixel of frames [frame_from, frame_to) (frame_to = 0: one frame) unprojected with K_depth^-1, moved by the frame's camera-to-world
 * (identity for a lost pose) and coloured by the pixel the colour camera sees there (alpha 255; (0,0,0,0) outside the colour image) -> a binary PLY point cloud. */
int sf_sens_save_point_cloud(const sf_sens* s, const char* ply_path, uint64_t frame_from, uint64_t frame_to, uint64_t* n_points);
/* Editing a file in memory, opened or under construction (then sf_sens_save):
 *   sf_sens_replace_depth   SensorData::replaceDepth(frameIdx, depth)  :948-955,499-502 (W*H u16, compressed with the file's type; depth time stamp -> 0
 *                           as freeDepth leaves it, :516-521) -- what the Calibrate stage does to every frame (Calibrate/src/calibration.h:303)
 *   sf_sens_replace_color   SensorData::replaceColor(frameIdx, color)  :957-964,505-508 (`color` as sf_sens_add_frame takes it; colour time stamp -> 0)
 *   sf_sens_append          SensorData::append(second)                 :1605-1624 (frames only, no IMU; ANY difference in frame sizes or compression
 *                           types is refused -- the reference's test joins its six comparisons with && and so lets almost everything through)
 *   sf_sens_equal           SensorData::operator==                     :1626-1650 (floats and doubles compared as numbers: -inf equals -inf, NaN nothing) */
int sf_sens_replace_depth(sf_sens* s, uint64_t frame, const uint16_t* depth);
int sf_sens_replace_color(sf_sens* s, uint64_t frame, const uint8_t* color, uint64_t color_bytes);
int sf_sens_append(sf_sens* s, const sf_sens* other);
int sf_sens_equal(const sf_sens* a, const sf_sens* b, int* equal);
/* SensorData::applyTransform(t) (:1047-1054): camera-to-world of every tracked frame <- t * m (row-major); all -inf poses are left alone */
int sf_sens_apply_transform(sf_sens* s, const float t[16]);

/* Frames streamed into a file as they arrive: SensorData::LiveSensorDataWriter (sensorData.h:1112-1246, _HAS_MLIB builds only there).  The header goes
 * out at open (a path that exists: overwritten, or -- overwrite = 0 -- the name's numeric suffix is counted up until it is free, :1118-1131;
 * sf_sens_writer_path says which); add copies the caller's buffers into a queue of at most cache_frames (0: 500, the reference's default) and blocks
 * while it is full; one background thread compresses and writes in order; close drains, writes "0 IMU frames" and patches the frame count (:1146-1157).
 * The file is byte for byte what the in-memory writer saves.  An error of any frame is returned by the next add and by close.
 * scannet_amd/csrc/sens_writer.cpp. */
typedef struct sf_sens_writer sf_sens_writer;
int sf_sens_writer_open(const sf_sens_info* header, const char* path, int overwrite, uint32_t cache_frames, sf_sens_writer** out);
const char* sf_sens_writer_path(const sf_sens_writer* w);
int sf_sens_writer_add_frame(sf_sens_writer* w, const uint8_t* color, uint64_t color_bytes, const uint16_t* depth, const float pose[16],
                             uint64_t timestamp_color, uint64_t timestamp_depth);
int sf_sens_writer_add_frame_blobs(sf_sens_writer* w, const uint8_t* color, uint64_t color_bytes, const uint8_t* depth, uint64_t depth_bytes,
                                   const float pose[16], uint64_t timestamp_color, uint64_t timestamp_depth);
int sf_sens_writer_close(sf_sens_writer* w, uint64_t* frames_written /*nullable*/);

/* IMU frames of a .sens under construction: 128 bytes each = rotationRate, acceleration, magneticField, attitude, gravity
 * (5 x 3 doubles) + u64 time stamp in microseconds (sensorData.h:796-803); addIMUFrame :923-926. */
int sf_sens_add_imu(sf_sens* s, const void* frame128);
/* Reading them back: sf_sens_imu = m_IMUFrames[index] (:1691); sf_sens_find_closest_imu = findClosestIMUFrame(frameIdx, basedOnRGB) (:1000-1044,
 * README.txt:49): nearest in time to the frame's colour (based_on_rgb) or depth time stamp; frame128 / index may be NULL. */
int sf_sens_imu(const sf_sens* s, uint64_t index, void* frame128);
int sf_sens_find_closest_imu(const sf_sens* s, uint64_t frame, int based_on_rgb, void* frame128, uint64_t* index);

/* ------------------------------------------------------------------------------------------------
 * ScannerApp captures and the `convert` stage (scannet_amd/csrc/occipital.cpp).  Replaces
 *   uplinksimple::decode / encode    ScannerApp/depth2pgm/uplinksimple_image-codecs.h:180-249 / :253-396
 *   uplinksimple::shift2depth        ScannerApp/depth2pgm/uplinksimple_shift2depth.h:9-90
 *   Converter convertToSens          Converter/main.cpp:16-179, MetaData Converter/src/metaData.h:11-72
 * sf_occ_decode is bounds-checked (SF_ERR_FORMAT on a truncated stream; the reference only asserts).  sf_occ_encode rejects
 * values above 2047 (the code has 11 bits; the reference would corrupt its own stream).
 * ---------------------------------------------------------------------------------------------- */
int sf_occ_decode(const uint8_t* stream, uint64_t stream_bytes, uint64_t num_elements, uint16_t* out_shift);
uint64_t sf_occ_encode_bound(uint64_t num_elements);
int sf_occ_encode(const uint16_t* shift_in, uint64_t num_elements, uint8_t* out, uint64_t out_capacity, uint64_t* out_bytes);
uint16_t sf_occ_shift2depth(uint16_t shift);
int sf_occ_shift2depth_buffer(uint16_t* buf, uint64_t n, int zero_invalid /* values >= shift2depth(0xffff) -> 0, Converter/main.cpp:89-93 */);

typedef struct sf_capture_meta {     /* <base>.txt (Converter/src/metaData.h:17-60) */
  uint32_t num_color_frames, num_depth_frames, num_imu;
  uint32_t color_width, color_height, depth_width, depth_height;
  float fx_color, fy_color, mx_color, my_color, fx_depth, fy_depth, mx_depth, my_depth;
  float color_to_depth_extrinsics[16];   /* row-major; identity when absent */
  int32_t has_extrinsics;
} sf_capture_meta;
typedef struct sf_convert_stats {
  uint64_t frames, depth_frames_in_capture, imu_frames, imu_skipped, depth_stream_bytes;
  uint32_t threads;
} sf_convert_stats;
typedef struct sf_capture sf_capture;
/* colour source of sf_capture_convert: *blob / *bytes for frame `frame` (valid until the next call); SF_OK or an sf_status */
typedef int (*sf_capture_color_fn)(void* user, uint64_t frame, const uint8_t** blob, uint64_t* bytes);
int sf_capture_open(const char* any_capture_file /* <base>.txt|.depth|.imu|.h264 */, sf_capture** out);
void sf_capture_close(sf_capture* c);
int sf_capture_get_meta(const sf_capture* c, sf_capture_meta* out);
int sf_capture_decode_depth(const sf_capture* c, uint64_t frame, uint16_t* dst_mm, uint64_t* timestamp_us /*nullable*/);
/* capture -> .sens: zlib depth, depthShift 1000, "StructureSensor", identity poses, depth time stamp on both streams,
 * IMU records with a zero time stamp skipped.  color_fn NULL: frames without colour; else color_compression 0 (raw RGB) or
 * 2 (JPEG blobs passed through). */
int sf_capture_convert(const sf_capture* c, const char* out_sens, sf_capture_color_fn color_fn, void* color_user, int color_compression,
                       int threads, sf_convert_stats* stats /*nullable*/);

/* ------------------------------------------------------------------------------------------------
 * `calibrate` stage, per-frame image operations on the GPU (scannet_amd/csrc/calibrate.hip).  Replaces the frame body of
 * Calibration::calibrateScan, Calibrate/src/calibration.h:253-307: colour undistortion (:185-223), distance-dependent
 * depth correction through the 3-D look-up table (:226-250, Grid3D::GetValue src/grid3d.cpp:119-151), depth undistortion,
 * the depth-to-colour warp that the reference draws with Direct3D 11 (src/aligner.h:21-87, shaders/aligner.hlsl), "invalidate
 * depth where we have no color" and the conversion back to u16 (:286-301).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_calib_params {     /* class Calib, calibration.h:10-72; parameter-file keys :22-48 */
  uint32_t color_width, color_height, depth_width, depth_height;
  float color_intrinsic[16], depth_intrinsic[16];   /* row-major 4x4, fx [0], fy [5], mx [2], my [6] */
  float depth_extrinsic[16];                        /* depthToColorExtrinsics */
  float color_dist[5], depth_dist[5];               /* k1..k5: k1 k2 k5 radial, k3 k4 tangential (:204-209) */
} sf_calib_params;
typedef struct sf_lut {              /* Grid3D, src/grid3d.h: xres*yres*zres floats, index (z*yres + y)*xres + x */
  int32_t xres, yres, zres;
  float max_dist;
  float* data;                       /* owned: sf_lut_free */
} sf_lut;
int sf_calib_params_load(const char* path, sf_calib_params* out);   /* "name = value" parameter file */
int sf_lut_load(const char* path, sf_lut* out);                     /* Grid3D::ReadFile, grid3d.cpp:362-406 */
void sf_lut_free(sf_lut* t);
typedef struct sf_calibrator sf_calibrator;
/* lut may be NULL (no distance correction).  depth_shift = the .sens header's (1000).  No CPU fallback. */
int sf_calibrator_create(const sf_calib_params* p, const sf_lut* lut, float depth_shift, int device, sf_calibrator** out);
void sf_calibrator_destroy(sf_calibrator* c);
int sf_calibrator_max_batch(void);   /* frames per call: 16 */
/* n frames per call, host buffers: rgb = colour_width*colour_height*3 bytes (or rgb_in == NULL: depth only), depth = W*H u16.
 * rgb_out receives the undistorted colour image, depth_out the corrected, undistorted depth aligned to the colour camera. */
int sf_calibrator_run(sf_calibrator* c, int n, const uint8_t* const* rgb_in, uint8_t* const* rgb_out, const uint16_t* const* depth_in,
                      uint16_t* const* depth_out);
/* the same on device buffers; kernel_us != NULL: synchronous, returns the duration of the batch's kernels in microseconds */
int sf_calibrator_run_device(sf_calibrator* c, int n, const void* const* d_rgb_in, void* const* d_rgb_out, const void* const* d_depth_in,
                             void* const* d_depth_out, float* kernel_us);

/* The stage end to end: Calibration::calibrateScan(inSens, outSens, params, table), calibration.h:87-137 (scannet_amd/csrc/
 * calib_stage.cpp): decode -> GPU -> re-encode, header rewritten as :119-129 say, input deleted when the names differ. */
typedef struct sf_calibrate_stats {
  uint64_t frames, frames_with_colour;
  int32_t skipped_existing;   /* input missing, output present: nothing done (:89-93)              */
  int32_t already_aligned;    /* depth extrinsic was the identity: file moved, not rewritten (:112-116) */
  double seconds_total;
  uint32_t threads;
} sf_calibrate_stats;
int sf_calibrate_sens(const char* in_sens, const char* out_sens, const char* params_txt, const char* lut_path /*nullable*/, int device,
                      int threads, sf_calibrate_stats* stats /*nullable*/);
/* Baseline JPEG of an RGB image (T.81 Annex K tables, IJG quality scaling; subsample != 0: 4:2:0).  Replaces the uplink encoder
 * behind RGBDFrame::compressColor(TYPE_JPEG), sensorData.h:565-596.  *out_bytes is set even when dst is too small. */
int sf_jpeg_encode(const uint8_t* rgb, uint32_t width, uint32_t height, int quality, int subsample, uint8_t* dst, uint64_t dst_capacity,
                   uint64_t* out_bytes);
/* Baseline JPEG -> RGB as RGBDFrame::decompressColorAlloc_stb does it (sensorData.h:609-616): sf_jpeg_decode on the host (what
 * sf_sens_decode_color runs for a TYPE_JPEG frame); sf_jpeg_decode_gpu = entropy decoding on the host, IDCT + chroma upsampling +
 * YCbCr -> RGB on the GPU -- the split sf_fuse_run uses for colour frames -- returning the same bytes. */
int sf_jpeg_decode(const uint8_t* data, uint64_t bytes, uint32_t width, uint32_t height, uint8_t* dst_rgb);
int sf_jpeg_decode_gpu(const uint8_t* data, uint64_t bytes, uint32_t width, uint32_t height, int device, uint8_t* dst_rgb);

/* ------------------------------------------------------------------------------------------------
 * 2-D annotation filter (scannet_amd/csrc/filter2d.hip).  Replaces the CUDA kernels AnnotationTools/Filter2dAnnotations/filter.cu
 * calls from Filter2dAnnotations.cpp:326-397 -- bilateralFilterFloatMap (:210-259), resampleFloatMap (:514-573), resampleUCharMap
 * (:647-676), filterAnnotations (:1020-1078), convertInstanceToLabel (:1082-1103) -- and the per-frame sequence around them.
 * Tables: FilterData::init (Filter2dAnnotations.cpp:52-61) with 256 / 80 / 256 entries; bins >= 80 cast no vote.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_filter2d sf_filter2d;
int sf_filter2d_create(int depth_width, int depth_height, int color_width, int color_height, int device, sf_filter2d** out);
void sf_filter2d_destroy(sf_filter2d* f);
int sf_filter2d_set_tables(sf_filter2d* f, const uint8_t instance_to_idx[256], const uint8_t idx_to_instance[80], const uint16_t instance_to_label[256]);
/* one frame: depth W_d*H_d u16 (mm), rgb W_c*H_c*3, instance_in W_c*H_c u8 (rendered annotation) -> instance_out u8, label_out u16 */
int sf_filter2d_frame(sf_filter2d* f, const uint16_t* depth, const uint8_t* rgb, const uint8_t* instance_in, uint8_t* instance_out,
                      uint16_t* label_out, float* kernel_us /*nullable*/);

/* PNG images of the annotation tools (scannet_amd/csrc/png.cpp): replaces FreeImageWrapper::loadImage / saveImage as
 * Filter2dAnnotations.cpp:340-341,400-401 uses them.  Non-interlaced, bit depth 8 / 16, grey (+alpha) and RGB(A) on read; grey on
 * write.  *data is malloc'ed (sf_free); 16-bit samples are in host byte order. */
int sf_png_read(const char* path, uint32_t* width, uint32_t* height, int* channels, int* bits, void** data);
int sf_png_write_gray(const char* path, const void* data, uint32_t width, uint32_t height, int bits);
/* grey (channels = 1), RGB (channels = 3) or RGBA (channels = 4: the `render` stage's pictures, below), 8 or 16 bits: the 16-bit depth PNGs of
 * SensReader/python/SensorData.py:78-91 (pypng there) and the colour PNG that SensorData::saveToImages makes of a TYPE_RAW colour frame
 * (sensorData.h:1432-1440) */
int sf_png_write(const char* path, const void* data, uint32_t width, uint32_t height, int channels, int bits);
void sf_free(void* p);

/* ------------------------------------------------------------------------------------------------
 * Annotation projection (scannet_amd/csrc/project.hip, annotations.cpp).  Replaces the Direct3D 11 render + read-back + filters of
 * AnnotationTools/ProjectAnnotations/Visualizer.cpp:57-193 (render) with shaders/drawAnnotations.hlsl:9-33, and the vertex labelling
 * of Visualizer.cpp:259-377.  Parameters: ProjectAnnotations/zParametersScan.txt:6,12-15.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_project_params {
  uint32_t color_width, color_height;      /* render target = the .sens colour size (Visualizer.cpp:51)      */
  uint32_t depth_width, depth_height;
  float fx, fy;                            /* m_calibrationColor.m_intrinsic(0,0) / (1,1) (:91)              */
  float depth_min, depth_max;              /* s_depthMin 0.1, s_depthMax 15.0                                */
  float depth_dist_thresh;                 /* s_depthDistThresh 0.2                                          */
  int32_t filter_using_original_depth;     /* s_filterUsingOrigialDepthImage false                           */
} sf_project_params;
typedef struct sf_projector sf_projector;
int sf_projector_create(const sf_project_params* params, int device, sf_projector** out);
void sf_projector_destroy(sf_projector* p);
int sf_projector_max_batch(void);
/* the mesh to draw, with the (instance, label) pair its m_Colors .z / .w hold (Visualizer.cpp:275,289); host pointers, copied */
int sf_projector_set_mesh(sf_projector* p, const float* xyz, uint64_t num_vertices, const uint32_t* triangles, uint64_t num_triangles,
                          const uint8_t* vertex_instance, const uint16_t* vertex_label);
/* n <= sf_projector_max_batch() frames.  cam2world: n x 16 row-major, first element -inf = no valid transform -> empty images
 * (:63,187-192).  orig_depth: n x depth_w*depth_h u16 millimetres (NULL: no depth-consistency filter).  Outputs n x color_w*color_h.
 * zcam_out (nullable): rendered depth in metres at colour resolution (:123-141). */
int sf_projector_run(sf_projector* p, int n, const float* cam2world, const uint16_t* orig_depth, uint8_t* instance_out, uint16_t* label_out,
                     float* zcam_out /*nullable*/, float* kernel_us /*nullable*/);
/* page-locked host buffers: images passed to / from sf_projector_run in such memory are copied at PCIe speed (pageable works, slower) */
int sf_host_alloc(uint64_t bytes, void** out);
void sf_host_free(void* p);
/* computeObjectIdsAndColorsPerVertex (:259-295) for the mesh the segs.json indexes: vertex -> (instance, label), 0 = unannotated */
int sf_annotation_vertex_ids(const char* segs_json, const char* aggregation_json, const char* label_map_tsv, uint64_t num_vertices,
                             uint8_t* vertex_instance, uint16_t* vertex_label, uint32_t* num_labels /*nullable*/);
/* propagateAnnotations (:297-377): ids of the decimated mesh carried to the high-resolution one (exact 3-nearest-neighbour search) */
int sf_annotation_propagate(const float* src_xyz, uint64_t src_vertices, const uint32_t* src_tris, uint64_t src_triangles, const uint8_t* src_instance,
                            const uint16_t* src_label, const float* dst_xyz, uint64_t dst_vertices, const uint32_t* dst_tris, uint64_t dst_triangles,
                            float normal_thresh, uint8_t* dst_instance, uint16_t* dst_label);

/* ------------------------------------------------------------------------------------------------
 * Triangle meshes and the PLY surface (README.md:45-46: binary little-endian PLY, vertex float x,y,z +
 * uchar red,green,blue,alpha, face list uchar int vertex_indices).  sf_ply_read replaces tinyply as the
 * Segmentator uses it (Segmentator/segmentator.cpp:131-141, tinyply.cpp:54-108,306-360): ascii / binary
 * little / big endian, x y z as 4-byte floats, triangle lists named vertex_indices or vertex_index with a
 * 4-byte index type; anything else is SF_ERR_FORMAT (tinyply throws or misreads).  .obj files are read like
 * tiny_obj_loader's first shape (segmentator.cpp:142-174).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_mesh sf_mesh;
int sf_ply_read(const char* path, sf_mesh** out);                 /* .ply or .obj by extension */
int sf_mesh_create(const float* xyz, const uint8_t* rgba /*nullable*/, uint64_t num_vertices, const uint32_t* tris,
                   uint64_t num_faces, sf_mesh** out);
int sf_mesh_counts(const sf_mesh* m, uint64_t* num_vertices, uint64_t* num_faces);
/* any destination may be NULL: xyz 3 floats, rgba 4 bytes, tris 3 u32, keys 1 u64 (marching-cubes meshes only) */
int sf_mesh_copy(const sf_mesh* m, float* xyz, uint8_t* rgba, uint32_t* tris, uint64_t* keys);
/* marching-cubes meshes only: the key of the cube each face came from (faces are in ascending key order) -- the meshes of a
 * partitioned scan merge into the one-GPU face order by a stable sort on it (scannet_amd/partition.py) */
int sf_mesh_copy_face_keys(const sf_mesh* m, uint64_t* face_keys);
/* One scan over several GPUs (BASELINE configs[4]; no reference counterpart: DepthSensing fuses a scan on one GPU, Server/scan_processor.py:138):
 * sf_mesh_create_keyed rebuilds a marching-cubes mesh from the arrays sf_mesh_copy / sf_mesh_copy_face_keys gave (another process's part);
 * sf_mesh_merge_parts turns the parts of a partitioned scan (sf_fuser_set_stripes / sf_fuser_set_slab, ghosts exchanged before meshing) into the
 * mesh ONE fuser would have extracted, byte for byte: vertices unique by edge key in key order (of the copies of a shared edge the lowest part's),
 * faces re-indexed and -- when every part has face keys -- stably sorted by cube key; without face keys they stay part after part (slabs in
 * rank order).  The merged mesh carries its keys, so merges nest.  bin/depthsensing --ranks N is the caller. */
int sf_mesh_create_keyed(const float* xyz, const uint8_t* rgba /*nullable*/, const uint64_t* keys, uint64_t num_vertices, const uint32_t* tris,
                         const uint64_t* face_keys /*nullable*/, uint64_t num_faces, sf_mesh** out);
int sf_mesh_merge_parts(const sf_mesh* const* parts, int n_parts, sf_mesh** out);
int sf_mesh_write_ply(const sf_mesh* m, const char* path);        /* the PLY surface above */
void sf_mesh_free(sf_mesh* m);

/* ------------------------------------------------------------------------------------------------
 * Mesh cleaning: `<id>_vh.ply` -> `<id>_vh_clean.ply`.  Replaces `meshlabserver -i in.ply -o out.ply -m vc -s clean.mlx`
 * (Server/scan_processor.py:134,143) for the filter scripts the pipeline ships -- Server/tools/meshclean/clean.mlx:3-10
 * and cleanLoRes.mlx:3-10: "Merge Close Vertices" (absolute Threshold 0.0010689), "Remove Duplicate Faces", "Remove
 * Isolated pieces (wrt Face Num.)" (MinComponentSize 7500 / 1000), "Remove Unreferenced Vertex".  Semantics: the VCG
 * algorithms behind those filters, restated in scannet_amd/csrc/clean.cpp.  simplify.mlx (scan_processor.py:144-145) =
 * quadric edge collapse (below) followed by the same four filters with MinComponentSize 1000.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_clean_stats {
  uint64_t vertices_in, faces_in;
  uint64_t vertices_merged;        /* vertices collapsed into a lower-index vertex                  */
  uint64_t faces_degenerate;       /* faces with a repeated vertex after merging                    */
  uint64_t faces_duplicate;
  uint64_t components_in, components_removed, faces_small_component;
  uint64_t vertices_unreferenced;
  uint64_t vertices_out, faces_out;
} sf_clean_stats;

/* "Quadric Edge Collapse Decimation" (Server/tools/meshclean/simplify.mlx:3-16), the first filter of the two
 * `meshlabserver ... -s simplify.mlx` calls of the decimate stage (Server/scan_processor.py:144-145).  Semantics: VCG's
 * TriEdgeCollapseQuadric restated in scannet_amd/csrc/simplify.cpp (parity unpinned: MeshLab is not in the tree). */
typedef struct sf_simplify_params {
  uint64_t target_faces;           /* simplify.mlx:4  TargetFaceNum (used when target_perc == 0)            */
  float target_perc;               /* :5  TargetPerc 0.2: keep this fraction of the faces                     */
  float quality_thr;               /* :6  QualityThr 0.3                                                      */
  int32_t preserve_boundary;       /* :7  false (true: SF_ERR_UNSUPPORTED)                                    */
  float boundary_weight;           /* :8  BoundaryWeight 1                                                    */
  int32_t preserve_normal;         /* :9  false (true: unsupported)                                           */
  int32_t preserve_topology;       /* :10 false (true: unsupported)                                           */
  int32_t optimal_placement;       /* :11 true                                                                */
  int32_t planar_quadric;          /* :12 false                                                               */
  int32_t quality_weight;          /* :13 false (true: unsupported)                                           */
  int32_t auto_clean;              /* :14 true                                                                */
} sf_simplify_params;
typedef struct sf_simplify_stats {
  uint64_t vertices_in, faces_in, target_faces;
  uint64_t collapses, stale_popped;
  uint64_t faces_zero_area, vertices_duplicate;   /* AutoClean */
  uint64_t vertices_out, faces_out;
  float max_priority;              /* largest scaled quadric error / quality of an executed collapse */
  uint32_t rounds;                 /* sf_mesh_simplify_gpu: rounds of independent collapses (0 from the sequential filter) */
} sf_simplify_stats;
void sf_simplify_default_params(sf_simplify_params* p);   /* the values simplify.mlx ships */
int sf_mesh_simplify(const sf_mesh* in, const sf_simplify_params* p, sf_mesh** out, sf_simplify_stats* stats /*nullable*/);

/* The same filter on HIP device `device` as rounds of independent collapses (scannet_amd/csrc/simplify_gpu.hip): same quadrics, placement,
 * priority and stop rule, a different order -- different triangles with the same guarantees (face budget, flat stays flat, closed stays
 * closed, deterministic) in a fraction of the time: the sequential filter is 22 s of a scan's 24 s of host time.  Opt-in; SF_ERR_DEVICE
 * without a GPU. */
int sf_mesh_simplify_gpu(const sf_mesh* in, const sf_simplify_params* p, int device, sf_mesh** out, sf_simplify_stats* stats /*nullable*/);

typedef struct sf_clean_script {   /* what a .mlx FilterScript asks for */
  int32_t merge_close_vertices, remove_duplicate_faces, remove_small_components, remove_unreferenced;
  float merge_distance;            /* clean.mlx:4  Threshold value (absolute)   */
  uint32_t min_component_faces;    /* clean.mlx:8  MinComponentSize             */
  int32_t simplify;                /* simplify.mlx: "Quadric Edge Collapse Decimation" comes first */
  sf_simplify_params simplify_params;
  sf_simplify_stats simplify_stats;  /* filled by sf_mesh_clean_script when simplify != 0 */
  int32_t simplify_device;           /* -1 (what sf_mlx_load sets): the sequential host filter; >= 0: sf_mesh_simplify_gpu on that device */
  int32_t clean_device;              /* -1 (what sf_mlx_load sets): the host cleaning filters; >= 0: sf_mesh_clean_gpu on that device (same output) */
} sf_clean_script;

int sf_mesh_clean(const sf_mesh* in, float merge_distance, uint32_t min_component_faces, sf_mesh** out, sf_clean_stats* stats /*nullable*/);
/* The same four filters on HIP device `device` (scannet_amd/csrc/clean_gpu.hip): identical arrays and statistics -- the greedy clustering
 * resolved in rounds down the index order, duplicate faces and connected components by radix sorts and a lock-free union-find --, a
 * few tens of milliseconds for a scan-sized mesh instead of 1.7 s of one host thread.  Opt-in; SF_ERR_DEVICE without a GPU. */
int sf_mesh_clean_gpu(const sf_mesh* in, float merge_distance, uint32_t min_component_faces, int device, sf_mesh** out, sf_clean_stats* stats /*nullable*/);
int sf_mlx_load(const char* mlx_path, sf_clean_script* out);
int sf_mesh_clean_script(const sf_mesh* in, sf_clean_script* script, sf_mesh** out, sf_clean_stats* stats /*nullable*/);

/* ------------------------------------------------------------------------------------------------
 * Segmentator: Felzenszwalb-Huttenlocher graph segmentation on vertex normals.  Replaces
 * Segmentator/segmentator.cpp: segment() :123-251 (normals :185-208, edge weights :211-229,
 * segment_graph :71-92, small-segment merge :237-243), writeToJSON :253-266, main :268-289.
 * segIndices are bit-exact with the reference binary (same union-find roots): the edge sort is libstdc++
 * std::sort with the reference's weight-only comparator, all float arithmetic is un-contracted IEEE fp32.
 * ---------------------------------------------------------------------------------------------- */
int sf_segment_mesh(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, float kThresh,
                    int segMinVerts, int32_t* segIndices_out);
/* The same labels with the two data-parallel stages -- vertex normals (a lane per vertex walks its faces in face order: the running mean's order is the
 * reference's) and edge weights -- on GPU `device` (csrc/segment_gpu.hip); the sort and the sweeps stay on the host.  Fails without a device. */
int sf_segment_mesh_gpu(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, float kThresh,
                        int segMinVerts, int device, int32_t* segIndices_out);
/* Reads mesh_path (.ply/.obj), segments, writes the JSON.  out_json NULL => reference naming:
 * <mesh minus extension>.<std::to_string(kThresh)>.segs.json (segmentator.cpp:282-286).  Prints nothing. */
int sf_segment_file(const char* mesh_path, float kThresh, int segMinVerts, const char* out_json, uint64_t* num_segments);
/* The same with what the drop-in CLI prints (segmentator.cpp:176-180, :285): counts4 = {vertexCount, verts.size(), faceCount,
 * faces.size()}, the path written, and whether an .obj held more than one shape (only the first is used, :166-169). */
int sf_segment_file_ex(const char* mesh_path, float kThresh, int segMinVerts, const char* out_json, uint64_t* num_segments,
                       uint64_t* counts4, char* out_path, uint64_t out_path_cap, int* obj_multi);
/* sf_segment_file_ex with sf_segment_mesh_gpu inside (`bin/segmentator ... --gpu [device]`, not a flag of the reference's): the same JSON. */
int sf_segment_file_gpu(const char* mesh_path, float kThresh, int segMinVerts, const char* out_json, uint64_t* num_segments,
                        uint64_t* counts4, char* out_path, uint64_t out_path_cap, int* obj_multi, int device);

/* ------------------------------------------------------------------------------------------------
 * Axis alignment: the `alignment.exe <scan dir>` call of the `clean` stage (Server/scan_processor.py:132-135).  Replaces
 * Alignment::alignScan (Alignment/src/alignment.h:154-308) with upVectorFromViews :23-35, hasGravity :71-80, upVectorFromGravity :82-107,
 * removeInvalidIMUFrames :128-152, and PlaneExtract (Alignment/src/planeExtract.h:75-154) with Cluster :13-71: up vector, floor plane, walls onto
 * x and y, the scan into the positive octant with the floor at z = 0 -- one rigid transform applied to every .ply of the folder and to every pose
 * of the .sens.  mLib and CGAL are not in the reference tree, so the arithmetic is this library's statement: DESIGN.md section 4i, operation by
 * operation, with tests/axis_align_checker.c as its executable form.  alignScanFromAlnFile (:322-362) is unreachable from the reference's main and
 * is not built.  scannet_amd/csrc/axis_align.cpp (the rule on the host, device = -1) and axis_align.hip (the same bits on HIP device >= 0).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_axis_align_params {
  float merge_distance;             /* alignment.h:211 mergeCloseVertices: 0.0005                                           */
  uint32_t min_piece_faces;         /* :212 removeIsolatedPieces, counted in FACES as sf_mesh_clean counts a piece: 5000     */
  uint32_t gravity_min_records;     /* :71 hasGravity numThresh: gravity is used when MORE records than this carry it: 10   */
  float cluster_normal_thresh;      /* planeExtract.h:88 normalThresh: 0.90                                                 */
  float cluster_dist_thresh;        /* :88 distThresh: 0.05                                                                 */
  uint32_t min_cluster_points;      /* :122 removeSmallClusters minSize: 500                                                */
  float behind_dist;                /* alignment.h:238 removeNonBoundingClusters distThresh: 0.1                            */
  uint32_t behind_max;              /* :238 numthresh: a cluster with MORE vertices behind it than this goes: 100           */
  float floor_normal_z;             /* :245 a floor's representative normal has z above this: 0.8                           */
  float floor_inlier_dist;          /* planeExtract.h:41 reComputeNormalAlignment: 0.05                                     */
  int32_t reserved[6];
} sf_axis_align_params;
void sf_axis_align_params_default(sf_axis_align_params* p);
typedef struct sf_axis_align_stats {
  uint64_t vertices, faces;         /* the working mesh, after cleaning                                                     */
  uint64_t clusters_founded;        /* planeExtract.h:88-104                                                                */
  uint64_t clusters_after_small;    /* left by removeSmallClusters :122-131                                                 */
  uint64_t clusters_kept;           /* left by removeNonBoundingClusters :134-143                                           */
  uint64_t floor_points;            /* members of the floor cluster                                                         */
  uint64_t floor_inliers;           /* of them within floor_inlier_dist of its plane                                        */
  uint64_t frames_without_gravity;  /* frames whose closest IMU record carried no gravity (alignment.h:91-94)               */
  uint64_t imu_records_dropped;     /* records with time stamp 0 (:128-152)                                                 */
  int32_t up_source;                /* 0: the views, 1: gravity                                                             */
  int32_t floor_found;              /* 0: "could not find a horizontal plane" (:255), the floor rotation is the identity    */
  /* the device path's counters (0 on the host path): speculation batches, representatives of clusters changed earlier in a batch that were
   * evaluated again, vertices for which the commit scanned the whole table again */
  uint64_t gpu_batches, gpu_dirty_evaluations, gpu_fallback_rescans;
  /* sf_axis_align_scan: 0 aligned; skipped: 1 no processed.txt, 2 valid = false, 3 aligned already (no force), 4 frame 0's pose is -inf */
  int32_t outcome;
  int32_t reverted;                 /* 1: frame 0's pose was not the identity and the previous alignment was undone first (:189-208) */
  float transform[16];              /* the result, row-major                                                                 */
  double seconds[6];                /* wall time: cleaning, normals, clustering, behind counts, covariance, everything else  */
  double gpu_seconds_match, gpu_seconds_commit;   /* the clustering's two kernels summed over the batches (HIP events), only under sf_axis_align_tune("profile", 1) */
} sf_axis_align_stats;
/* The transform of a scan from its surface and its trajectory (neither is changed): `mesh` is the scan's `<base>.ply` as read; the working mesh
 * (sf_mesh_clean with merge_distance / min_piece_faces; sf_mesh_clean_gpu on the device path) serves the estimate only.  params NULL: the defaults.
 * device -1: the host path; >= 0: that HIP device (SF_ERR_DEVICE without one), the same 16 floats.  SF_ERR_INVALID_ARG for a .sens without
 * frames or a parameter that is negative or not finite. */
int sf_axis_align_estimate(const sf_mesh* mesh, const struct sf_sens* sens, const sf_axis_align_params* params, int device, float transform[16],
                           sf_axis_align_stats* stats /*nullable*/);
/* MeshDataf::applyTransform as alignment.h:205,298 uses it: every position <- the affine part of the row-major 4x4 (the
 * host loop: what the tool and sf_axis_align_scan use for the folder's files). */
int sf_mesh_apply_transform(sf_mesh* mesh, const float transform[16]);
/* Alignment::alignScan(path, forceRealign) (:154-308) on the folder <dir> with base = its last path component: the gates on processed.txt
 * (:156-170), the revert (:189-208), the estimate from <dir>/<base>.ply and <dir>/<base>.sens, then the transform applied to every *.ply of the
 * folder (names ascending) and to the .sens, which is rewritten in place without its IMU records of time stamp 0, and processed.txt saved in
 * ProcessedFile::saveToFile's five-line format (Alignment/src/processedFile.h:57-63) with aligned = true.  A skipped folder is SF_OK with
 * stats->outcome set and nothing written.  Prints nothing: bin/alignment prints the reference's messages from *stats. */
int sf_axis_align_scan(const char* dir, int force, const sf_axis_align_params* params /*nullable*/, int device, sf_axis_align_stats* stats /*nullable*/);


/* ------------------------------------------------------------------------------------------------
 * Mesh render and thumbnail: the `render` and `thumbnail` stages (Server/scan_processor.py:159-165 with :42-45; Server/mts_render.py,
 * Server/thumbnail.sh).  Replaces the Mitsuba preview of the vertex-coloured decimated mesh under a constant sky (mts_render.py:33-66: `diffuse`
 * with `vertexcolors`, a `constant` emitter, a 45-degree `perspective` sensor, `ldrfilm` RGBA) and its camera (:69-99: the bounding sphere of the
 * mesh's AABB, bsphere_mult radii out along camera_offset + world_up, turned by theta about world_up).  Mitsuba is not in the reference tree and
 * its sampler is not specified bit for bit, so the picture is this library's statement of that scene: DESIGN.md section 4j, operation by
 * operation, with tests/render_checker.c as its executable form (brute force, no tree).  scannet_amd/csrc/render_walk.h is the one statement
 * of the walk; render.hip runs it on HIP device >= 0, render_host.cpp on host threads (device = -1): the same float bits.
 * ---------------------------------------------------------------------------------------------- */
enum { SF_RENDER_PATH = 0, SF_RENDER_AO = 1 };   /* mts_render.py:134-135 --integrator; `mlt` and `vpl` are refused by bin/render */
#define SF_RENDER_MAX_SAMPLES 4096
#define SF_RENDER_MAX_DEPTH 16
#define SF_RENDER_MAX_SIDE 8192
#define SF_RENDER_MAX_BATCH 32
typedef struct sf_render_params {
  int32_t width, height;   /* mts_render.py:140-145: 640 x 480; 1 .. SF_RENDER_MAX_SIDE                                              */
  int32_t samples;         /* :137-139 samples per pixel: 16; 1 .. SF_RENDER_MAX_SAMPLES                                             */
  int32_t max_depth;       /* bounces a path may take before a further hit ends it with radiance 0: 8; 1 .. SF_RENDER_MAX_DEPTH      */
  int32_t integrator;      /* SF_RENDER_PATH, or SF_RENDER_AO: reflectance 1 and one bounce                                          */
  float fov;               /* :50 degrees across the image WIDTH (Mitsuba's default fovAxis): 45; in (0, 180)                        */
  float exposure;          /* :152-154 the film scales radiance by 2^exposure: 1.0 (sf_render_film takes it as an argument)          */
  int32_t pixel_centre;    /* 0: the sub-pixel position of a sample comes from the hash; 1: it is (0.5, 0.5)                         */
  int32_t reserved[8];
} sf_render_params;
void sf_render_params_default(sf_render_params* p);
typedef struct sf_camera {   /* a view as the walk takes it: right-handed, `forward` into the scene, pixel (0, 0) top left */
  float origin[3], right[3], up[3], forward[3];
  float tan_half_fov;      /* tan(fov / 2)                                                                                           */
  float aspect;            /* width / height                                                                                         */
  float reserved[2];
} sf_camera;
/* mts_render.py:69-99.  The box is the mesh's AABB, or aabb6 = {min x y z, max x y z} when mesh is NULL.  Centre (min + max) / 2, radius the
 * distance from it to max; origin = centre + bsphere_mult * radius * normalize(camera_offset + world_up), then the origin (about the centre) and
 * camera_up turned by theta_deg about world_up; forward = towards the centre, right = normalize(forward x camera_up), up = right x forward.
 * Computed in double, returned as floats.  world_up / camera_up / camera_offset NULL: (0,0,1) / (0,1,0) / (0,0,0).  SF_ERR_INVALID_ARG for a
 * non-finite input, a zero world_up or camera_offset + world_up, a camera_up parallel to the view direction, an empty box, bad params. */
int sf_render_camera(const sf_mesh* mesh, const float* aabb6, const sf_render_params* params, const float* world_up, const float* camera_up,
                     const float* camera_offset, float bsphere_mult, float theta_deg, sf_camera* out);
typedef struct sf_renderer sf_renderer;
/* device -1: the host path (threads over rows); >= 0: that HIP device, SF_ERR_DEVICE without one -- never a silent fallback.  params NULL: the defaults. */
int sf_renderer_create(const sf_render_params* params, int device, sf_renderer** out);
/* Builds the tree over the mesh (deterministic, on the host) and, on a device, uploads it; may be called again with another mesh.  A mesh without
 * colours renders with every byte 128.  SF_ERR_INVALID_ARG for an empty mesh, an index >= the vertex count, a non-finite vertex, 2^28 or more triangles. */
int sf_renderer_set_mesh(sf_renderer* r, const sf_mesh* mesh);
/* n >= 1 views -> rgba: n x height x width x 4 floats, the mean radiance and alpha of every pixel (before the film).  On a device the views go
 * SF_RENDER_MAX_BATCH per launch.  kernel_us (nullable): the launches' time by HIP events (device) or the wall time of the rows (host), microseconds. */
int sf_renderer_run(sf_renderer* r, int n, const sf_camera* cameras, float* rgba, float* kernel_us);
void sf_renderer_destroy(sf_renderer* r);
/* The film (Mitsuba's ldrfilm, gamma -1), in double, per pixel: rgb x 2^exposure, the sRGB curve (12.92 v up to 0.0031308, else
 * 1.055 v^(1/2.4) - 0.055), clamped to [0, 1], (int)(255 v + 0.5); alpha: clamped, (int)(255 a + 0.5).  NaN gives 0. */
int sf_render_film(const float* rgba, uint64_t num_pixels, float exposure, uint8_t* rgba8);
/* Server/thumbnail.sh's `convert -resize WxH` (128 x 128 there): the picture fitted into box_w x box_h keeping its aspect ratio -- the side that
 * fills the box takes the box's size, the other (int)(side * scale + 0.5), at least 1, so 640 x 480 gives 128 x 96 -- by an area average in integer
 * arithmetic on the 8-bit values of every channel; ImageMagick's filter, pngquant and optipng are not reproduced.  channels 1..4.
 * out holds box_w x box_h x channels bytes at most; the size comes back in out_w / out_h. */
int sf_image_thumbnail(const uint8_t* in, uint32_t width, uint32_t height, int channels, uint32_t box_w, uint32_t box_h, uint8_t* out,
                       uint32_t* out_w, uint32_t* out_h);

/* ------------------------------------------------------------------------------------------------
 * Depth-distortion table: estimate and apply (scannet_amd/csrc/depth_lut.hip, depth_lut.cpp).  Replaces the two batch modes
 * of CameraParameterEstimation/apps/calibrate_depth/src/calibrate_depth.cpp -- EstimateDistortion (:647-836, `-e`) and ApplyUndistortion
 * (:565-644, `-a`) -- with the table and its file of src/grid3d.h (GetValue :177-209, WriteFile :464-494) and the angle / intersect / normalize of
 * basics/linalg/geometry.h:58-73 and vector.h:1140-1157.  The OpenGL viewer, calibration_explorer and the Matlab scripts are not provided.
 * device -1: the host path (the same bits); >= 0: that HIP device, SF_ERR_DEVICE without one -- never a silent fallback.
 * ---------------------------------------------------------------------------------------------- */
int sf_lut_save(const char* path, const sf_lut* t);                  /* Grid3D::WriteFile, grid3d.h:464-494: what sf_lut_load reads */
typedef struct sf_lut_estimator sf_lut_estimator;
/* Images are width x height u16, both even, width >= 10; the table is (width / 2) x (height / 2) x n_slices (:771-776 hard-codes 640 x 480).
 * n_slices above what a workgroup's LDS holds (128): SF_ERR_PARAM on either path, nothing is launched.  bitshift: :623 (the default of the tool). */
int sf_lut_estimator_create(int width, int height, float fx, float fy, float mx, float my, int n_slices, float max_depth, int bitshift, int device,
                            sf_lut_estimator** out);
/* n >= 1 host images and their n plane poses (n x 16 floats, row-major, in the depth camera's frame: :680-688), in sequence order; calls chain.
 * An image whose plane is tilted more than 25 degrees contributes nothing (:691-697).  Synchronous. */
int sf_lut_estimator_add(sf_lut_estimator* e, int n, const uint16_t* const* images, const float* plane_poses);
/* the same on device images (4-byte aligned), sf_lut_estimator_max_batch() per launch; kernel_us != NULL: synchronous, the launches' duration in
 * microseconds; NULL: the last launch is left running on the estimator's stream (sums / finish / destroy order behind it) */
int sf_lut_estimator_add_device(sf_lut_estimator* e, int n, const void* const* d_images, const float* plane_poses, float* kernel_us);
int sf_lut_estimator_max_batch(void);   /* images per launch: 64 */
/* :809-833: divide, side stripe, unknowns -> 1.  out->data is owned by the caller (sf_lut_free); the estimator may go on taking images. */
int sf_lut_estimator_finish(sf_lut_estimator* e, sf_lut* out);
void sf_lut_estimator_destroy(sf_lut_estimator* e);
/* :618-636 on n images of width x height: out = in corrected through the table (which must not be finer than the image).  A result of 65 536 mm
 * or more, undefined in the reference, is 65 535; where the table's resolution does not divide the image, the last cell serves the remainder. */
int sf_lut_apply(const sf_lut* lut, int n, const uint16_t* const* in, uint16_t* const* out, int width, int height, int bitshift, int device);
int sf_lut_apply_device(const sf_lut* lut, int n, const void* const* d_in, void* const* d_out, int width, int height, int bitshift, int device,
                        float* kernel_us /*nullable*/);
/* The configuration file (:296-362: `parameters <file>`, `n_images <N>`, `plane_poses <file>`, `scan <depth> <colour> <16 numbers>`, # comments), the
 * parameter file behind it (sf_calib_params_load; :112-181 reads fx_depth fy_depth mx_depth my_depth depthToColorExtrinsics) and the plane poses
 * (:184-223): N row-major matrices, each returned as inverse(F D2C F) pose, F = diag(1, -1, -1, 1), the inverse in double.  File names are
 * relative to root (NULL: the current directory).  plane_poses before parameters and n_images, n_images above the scan lines, a truncated poses
 * file: SF_ERR_FORMAT (the reference goes on with defaults or uninitialised poses). */
typedef struct sf_depth_calib {
  float fx, fy, mx, my;
  float depth_to_color[16];
  int32_t n_images, n_scans;   /* the n_images line; the scan lines read (>= n_images) */
  float* plane_poses;          /* n_images x 16, row-major, converted                */
  char** image_names;          /* n_scans depth image names                          */
} sf_depth_calib;
int sf_depth_calib_load(const char* config_path, const char* root /*nullable*/, sf_depth_calib* out);
void sf_depth_calib_free(sf_depth_calib* c);
typedef struct sf_calibrate_depth_options {   /* struct Options, :96-107, defaults :1150-1156 */
  float max_depth;        /* -d: 5.0 */
  int32_t n_slices;       /* -s: 15  */
  int32_t bitshift;       /* -b: 1   */
  int32_t verbose;        /* -v: the bin table of ReportBinCounts (:516-563) and the skipped images, on stdout */
  int32_t save_slices;    /* -l: slice_%03d.png under root, the colour ramp of :845-891 */
  const char* root;       /* depth_raw/, depth/ and the files the configuration names live here; NULL: the current directory */
  int32_t reserved[8];
} sf_calibrate_depth_options;
void sf_calibrate_depth_options_default(sf_calibrate_depth_options* o);
typedef struct sf_calibrate_depth_stats {
  uint64_t images, images_used, images_skipped, images_applied;
  double seconds_read, seconds_estimate, seconds_apply, seconds_write, seconds_total;
  uint32_t threads;
} sf_calibrate_depth_stats;
/* The tool's body: estimate_path != NULL writes the table estimated from depth_raw/<name> (-e); apply_path != NULL then reads that table and
 * writes depth/<name minus 4 characters>.png from depth_raw/<the same>.png (-a).  Both NULL: SF_ERR_INVALID_ARG (the reference opens its viewer).
 * PNG decode and encode run on `threads` host threads (<= 0: the CPUs this process may use). */
int sf_calibrate_depth(const char* config, const char* estimate_path /*nullable*/, const char* apply_path /*nullable*/,
                       const sf_calibrate_depth_options* options /*nullable*/, int device, int threads, sf_calibrate_depth_stats* stats /*nullable*/);

/* ------------------------------------------------------------------------------------------------
 * Free-space grids: the `freespace` stage (Server/scan_processor.py:15; FreeSpace.exe, "exe to call for computing occupancy grids",
 * Server/config.py:20; product ${id}.grid, Server/config/scan_stages.json:43-47).  Neither the binary nor its file format is in the reference
 * tree: the rule and the format are this library's statement, unpinned.  What the tree says is what a consumer reads: a
 * float volume in voxel units whose "known/unknown" channel is value >= -1 (Tasks/SemanticVoxelLabeling/torch/provider.lua:80-97,
 * Tasks/README.md:20), laid out [z][y][x] beside a world2grid matrix (BenchmarkScripts/3d_helpers/export_semantic_label_grid_for_evaluation.py:35-47).
 * The rule is the fuser's own: a voxel a frame sees in front of the surface by more than the truncation is integrated as sdf = +trunc with a
 * weight, so known = weight > 0.  The stage allocates every block a frame can reach (sf_fuser_allocate_box), fuses the scan through sf_fuse_run and
 * reads the box of the known voxels back (sf_fuser_known_bounds, sf_fuser_export_dense mode 1).
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_freespace_params {
  float voxel_size;                 /* metres: 0.05 (this library's choice)                                                          */
  uint32_t max_blocks;              /* the largest box of 8^3-voxel blocks (4 KiB each) the stage will allocate: 1 << 21             */
  int32_t every;                    /* every N-th frame of the scan, >= 1: 1                                                        */
  int32_t reserved[5];
  char params_file[1024];           /* an mLib ParameterFile for the other TSDF constants; "": sf_params_default                     */
} sf_freespace_params;
void sf_freespace_params_default(sf_freespace_params* p);
/* Host only, double: the box of blocks (inclusive) that holds every voxel the frames used can update -- the box of the camera centres of the
 * frames with a valid pose, widened by R + one voxel, R = zfar sqrt(1 + ax^2 + ay^2), zfar = max_dist + trunc_base + trunc_scale max_dist,
 * ax = max(mx + 1.5, W - 0.5 - mx) / fx (ay likewise; the effective integration camera) -- and the fuser parameters for it (the file's camera,
 * the heap and the table sized from the box, colour and garbage collection off).  SF_ERR_CAPACITY: more than max_blocks blocks (the count is in
 * sf_last_error()); SF_ERR_INVALID_ARG: no frame with a valid pose. */
int sf_freespace_plan(const struct sf_sens* s, const sf_freespace_params* p, sf_params* fuser_params, int32_t lo_block[3], int32_t hi_block[3]);
typedef struct sf_freespace_stats {
  uint64_t box_blocks, frames_used;
  uint64_t known, free_voxels, near_voxels;   /* weight > 0; of those, sdf >= trunc_base; the others                                */
  int32_t lo_block[3], hi_block[3];
  double seconds_plan, seconds_create, seconds_allocate, seconds_fuse, seconds_bounds, seconds_export, seconds_total;
} sf_freespace_stats;
/* The grid: value[nz][ny][nx] (x fastest) = sdf / voxel_size, -inf where weight == 0; weight[nz][ny][nx]; lattice node (x, y, z) of the grid lies at
 * (lo_voxel + (x, y, z)) * voxel_size metres; world2grid (row-major) maps metres to g = w / voxel_size - lo_voxel + 0.5, so floor(g) is the nearest node. */
typedef struct sf_grid sf_grid;
typedef struct sf_grid_header {
  int32_t nx, ny, nz;
  float voxel_size;
  int32_t lo_voxel[3];
  float world2grid[16];
  uint64_t frames_used;
} sf_grid_header;
/* plan, fuser (on `device`), allocate_box, sf_fuse_run (decode_threads as there), known_bounds, export.  No known voxel: a grid of dims 0.
 * SF_ERR_DEVICE without a GPU (the fuser has no host fall-back); SF_ERR_CAPACITY when a block could not be allocated.  Free with sf_grid_free. */
int sf_freespace_sens(const struct sf_sens* s, const sf_freespace_params* p, int device, int decode_threads, sf_grid** out, sf_freespace_stats* stats /*nullable*/);
int sf_grid_create(const sf_grid_header* h, const float* value, const uint8_t* weight, sf_grid** out);   /* copies */
int sf_grid_info(const sf_grid* g, sf_grid_header* out);
int sf_grid_data(const sf_grid* g, const float** value, const uint8_t** weight);   /* owned by the grid */
/* The file, little-endian: char magic[8] = "SFGRID1\0"; int32 nx, ny, nz; float voxel_size; int32 lo_voxel[3]; float world2grid[16]; uint64
 * frames_used; float value[nz][ny][nx]; uint8 weight[nz][ny][nx].  sf_grid_load: SF_ERR_FORMAT for a bad magic, negative dims, a size that does not
 * match the file, a voxel_size that is not finite. */
int sf_grid_save(const sf_grid* g, const char* path);
int sf_grid_load(const char* path, sf_grid** out);
void sf_grid_free(sf_grid* g);

/* ------------------------------------------------------------------------------------------------
 * Voxel-task data: label grids and column samples.  The reference's generator for the data of
 * Tasks/SemanticVoxelLabeling is "to come soon" (Tasks/README.md:14); what the tree does say is what reads it: datasets `data` [n][1][62][31][31]
 * and `label` [n][62] (Tasks/SemanticVoxelLabeling/torch/provider.lua:59-60; the sizes in test_scenes.lua:44), label 0 = empty and 255 = unannotated
 * (provider.lua:63-75), channel data from the free-space volume above (provider.lua:80-97), and the per-vertex read of a [z][y][x] label grid
 * (BenchmarkScripts/3d_helpers/export_semantic_label_grid_for_evaluation.py:35-47).  The rule -- the nearest face of a lattice node, the label of a
 * face, which columns become samples -- is this library's statement, unpinned.  device = -1 is the host path (at most 16 threads), which writes the
 * bytes the device writes; device >= 0 without a GPU is SF_ERR_DEVICE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sf_voxlabel_params {
  float band;                       /* voxels: a node takes a face within band * voxel_size; 0.8660254f, the half diagonal of a cell  */
  int32_t wx, wy, wz;               /* the sample window, x and y odd: 31, 31, 62 (test_scenes.lua:44)                               */
  int32_t z0;                       /* the window's first grid layer when z0_default == 0; any value                                 */
  int32_t z0_default;               /* != 0: z0 = -lo_voxel[2], the layer of world z = 0: 1                                          */
  int32_t stride;                   /* every stride-th column in x and in y, >= 1: 1                                                 */
  int32_t reserved[9];
} sf_voxlabel_params;
void sf_voxlabel_params_default(sf_voxlabel_params* p);
/* face[nz][ny][nx] = the face with the smallest (squared distance, index) among the faces within band * voxel_size of the node, -1 where there is
 * none; dist2 (nullable) = that squared distance in metres^2, +inf at those nodes.  Of the header only nx, ny, nz, voxel_size and lo_voxel are read.
 * Faces with a repeated index, a non-finite coordinate or no area (as binary32 sees it) are skipped.  With device >= 0, face and dist2 may be device
 * memory.  SF_ERR_INVALID_ARG, before anything is launched or written: an index >= num_vertices, a band or voxel_size that is not finite and
 * positive, nodes beyond +-2^22 or more than 2^40 of them. */
int sf_voxlabel_nearest_faces(const sf_grid_header* h, const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, float band,
                              int device /* -1: host */, int32_t* face, float* dist2 /*nullable*/);
/* Host.  A face takes the value two of its vertices share, else its first vertex's; labels and instances apart.  label / instance: the winning
 * face's, 0 where face == -1; byte_label, the task's: 0 where face == -1, 255 where the face's label is 0 or above 254, else the label.  Any output
 * may be NULL; vertex_instance may be NULL when instance is. */
int sf_voxlabel_labels(const int32_t* face, uint64_t num_nodes, const uint32_t* tris, uint64_t num_faces, uint64_t num_vertices, const uint16_t* vertex_label,
                       const uint8_t* vertex_instance /*nullable*/, uint16_t* label, uint8_t* instance, uint8_t* byte_label);
/* Column (x, y) is a sample iff x and y are multiples of stride and its own column holds a byte label other than 0 and 255 in the layers
 * z0 .. z0 + wz - 1 that lie in the grid; samples are numbered y-major.  *total = how many there are; samples first .. first + n - 1,
 * n = min(max_samples, total - first), go to data[n][1][wz][wy][wx] (the grid's value, -inf outside it), label[n][wz] (the centre column's byte
 * label, 0 outside) and xy[n][2].  max_samples = 0 with NULL outputs counts only.  With device >= 0 the outputs may be device memory. */
int sf_voxlabel_sample_columns(const sf_grid* g, const uint8_t* byte_label, const sf_voxlabel_params* p, int device /* -1: host */, uint64_t first,
                               uint64_t max_samples, float* data, uint8_t* label, int32_t* xy, uint64_t* total);

/* ------------------------------------------------------------------------------------------------
 * Object-task data: an occupancy and a known grid per annotated object.  The generator of this data is "to come soon" as well
 * (Tasks/README.md:14); what reads it: Tasks/ObjectClassification/torch/provider.lua:40-47 and train_partial.lua, and
 * Tasks/ObjectRetrieval/generate_feat.lua:32,74-81,101-109 -- datasets `data` [n][2][30][30][30] (channel 0 the "partially-scanned objects, voxelized to
 * 30x30x30", channel 1 the "additional data channel encoding known/unknown voxels according to the camera scanning trajectory", Tasks/README.md:20)
 * and `label` [n], 0-based: the first column of Tasks/Benchmark/classes_ObjClassification-ShapeNetCore55.txt (generate_feat.lua:42 against :78 and
 * :109).  Objects are told apart as BenchmarkScripts/3d_helpers/export_train_mesh_for_evaluation.py:38-54,86-90 does: by the segGroup's objectId.  The
 * rule -- the cube of an object, the quantisation, which cells a face sets, which cells are known -- is this library's statement, unpinned.
 * device = -1 is the host path (at most 16 threads), which writes the bytes the device writes; device >= 0 without a GPU is SF_ERR_DEVICE.
 * ---------------------------------------------------------------------------------------------- */
/* vertex_object[v] = objectId + 1 of the segGroup whose `segments` hold the vertex's segment (a later group overwrites an earlier one), 0: no group.
 * *num_objects = the largest objectId + 1 (0 without a group).  *labels (nullable): one "objectId\tlabel\n" line per objectId that a group names, ascending,
 * the label of the last such group; malloc'ed (sf_free).  SF_ERR_FORMAT: a segs.json of another vertex count, no segGroups, an objectId above 65 535. */
int sf_annotation_vertex_objects(const char* segs_json, const char* aggregation_json, uint64_t num_vertices, uint32_t* vertex_object, uint32_t* num_objects,
                                 char** labels /*nullable*/);
/* Host.  object_class[i] for the lines of `object_labels` (the text above), -1 where the object has no class or no line: the label is looked up in the
 * label map (key column label_from; NULL: "raw_category", or "category" when the file has no such column; value column label_to, NULL:
 * "ShapeNetCore55"), the value is matched against the classes file (lines of `<id> <name>`): it equals a name, or parses as an integer equal to an
 * id.  SF_ERR_IO: a file that cannot be read; SF_ERR_FORMAT: a column that is not there, a classes file with an id outside 0 .. 254. */
int sf_objvox_classes(const char* object_labels, const char* label_map_tsv, const char* classes_txt, const char* label_from /*nullable*/,
                      const char* label_to /*nullable*/, uint32_t num_objects, int32_t* object_class);
typedef struct sf_objvox_params {
  int32_t dim;                      /* cells per axis, 1 .. 32: 30 (provider.lua:40-47)                                               */
  int32_t fit;                      /* the object's largest extent in cells, 1 .. dim: 24                                             */
  int32_t min_faces;                /* objects with fewer counted faces are left out: 1                                               */
  int32_t all_objects;              /* != 0: objects without a class are kept, with label 255: 0                                      */
  int32_t reserved[12];
} sf_objvox_params;
void sf_objvox_params_default(sf_objvox_params* p);
/* Host.  The objects sf_objvox_voxelize keeps, in ascending objectId order: *count of them; the first min(*count, capacity) go to object_id[],
 * origin[][3] (the corner of cell (0, 0, 0), metres) and cell[] (the cell's edge) -- each nullable.  vertex_object: num_vertices values 0 .. num_objects;
 * object_class: num_objects values -1 .. 254.  Refusals as in sf_objvox_voxelize. */
int sf_objvox_plan(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, const uint32_t* vertex_object, const int32_t* object_class,
                   uint32_t num_objects, const sf_objvox_params* p, int32_t* object_id, float* origin, float* cell, uint64_t capacity, uint64_t* count);
/* *total = how many objects are kept; objects first .. first + n - 1 of them, n = min(max_objects, total - first), go to data[n][2][dim][dim][dim]
 * ([c][z][y][x]; channel 0: 1 where a face of the object meets the closed cell, channel 1: 1 where the cell is occupied or the grid's node nearest to
 * its centre has weight > 0; all ones without a grid), label[n] (the class id; 255 without a class), object_id[n] (objectId, 0-based), origin[n][3] and
 * cell[n].  max_objects = 0 with NULL outputs counts only.  With device >= 0 the outputs may be device memory.  SF_ERR_INVALID_ARG, before anything
 * is launched or written: an index >= num_vertices, dim outside 1 .. 32, fit outside 1 .. dim, a vertex_object value above num_objects, num_objects
 * above 65 536, a class outside -1 .. 254, more than 2^31 faces. */
int sf_objvox_voxelize(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, const uint32_t* vertex_object, const int32_t* object_class,
                       uint32_t num_objects, const sf_grid* grid /*nullable*/, const sf_objvox_params* p, int device /* -1: host */, uint64_t first,
                       uint64_t max_objects, uint8_t* data, uint8_t* label, int32_t* object_id, float* origin, float* cell, uint64_t* total);

/* ------------------------------------------------------------------------------------------------
 * Benchmark scores: label IoU and instance AP from predictions.  What they replace:
 * BenchmarkScripts/3d_evaluation/evaluate_semantic_label.py:48-82 (confusion matrix and IoU), evaluate_semantic_instance.py:75-309 with
 * util_3d.py:148-159 (instances, overlaps, AP), 2d_evaluation/evalPixelLevelSemanticLabeling.py:226-264 with addToConfusionMatrix_impl.c (the 2-D
 * matrix after a nearest-neighbour resize to 640 x 480).  Every count is an integer: device = -1 is the host path (at most 16 threads), which gives
 * the counts the device gives; device >= 0 without a GPU is SF_ERR_DEVICE.  The _device twins take device memory and a HIP stream (hipStream_t as
 * void*, NULL: the default stream): they copy nothing, wait for nothing and add into counters that stay on the device.  Every pointer must be device
 * memory of one device (looked up with hipPointerGetAttributes, a host-side query); that device is current during the call and the caller's current
 * device is put back before it returns.  A refused call writes nothing.
 * Elements are unsigned integers of elem_bytes = 1, 2 or 4 bytes, both arrays alike; a negative value of a signed type reads as a large one, which is
 * no valid class.  valid_ids: n_valid distinct class ids 0 .. 61; dim = the largest + 2.
 * ---------------------------------------------------------------------------------------------- */
#define SF_EVAL_MODE_3D 0 /* gt not a valid class: skipped; pred not a valid class: column dim - 1 (evaluate_semantic_label.py:60-65) */
#define SF_EVAL_MODE_2D 1 /* every element counts at [gt][pred]; an id >= dim in either array: counted in *out_of_range instead      */
#define SF_EVAL_IMAGE_WIDTH 640
#define SF_EVAL_IMAGE_HEIGHT 480
#define SF_EVAL_AP_OVERLAPS 10 /* 0.5, 0.55 .. 0.9, then 0.25 (evaluate_semantic_instance.py:66) */
/* confusion[dim][dim] and *out_of_range (nullable in the 3-D mode) are ADDED to: zero them before the first call.  n up to 2^40. */
int sf_eval_confusion(const void* gt, const void* pred, int elem_bytes, uint64_t n, const int32_t* valid_ids, uint32_t n_valid, int mode,
                      int device /* -1: host */, uint64_t* confusion, uint64_t* out_of_range);
int sf_eval_confusion_device(const void* gt, const void* pred, int elem_bytes, uint64_t n, const int32_t* valid_ids /* host */, uint32_t n_valid, int mode,
                             void* stream, uint64_t* confusion, uint64_t* out_of_range);
/* The 2-D mode on `batch` pairs gt[batch][gt_height][gt_width], pred[batch][pred_height][pred_width]: both are resized to 640 x 480 by nearest
 * neighbour, source index = floor((dst + 0.5) * src / dst size) per axis, and counted as SF_EVAL_MODE_2D with the dim given (41 for NYU40).
 * SF_ERR_INVALID_ARG unless pred_width == gt_width or the prediction is 640 x 480 (evalPixelLevelSemanticLabeling.py:240); sides up to 32768. */
int sf_eval_confusion_images(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gt_width, uint32_t gt_height, uint32_t pred_width,
                             uint32_t pred_height, uint32_t dim, int device /* -1: host */, uint64_t* confusion, uint64_t* out_of_range);
int sf_eval_confusion_images_device(const void* gt, const void* pred, int elem_bytes, uint32_t batch, uint32_t gt_width, uint32_t gt_height,
                                    uint32_t pred_width, uint32_t pred_height, uint32_t dim, void* stream, uint64_t* confusion, uint64_t* out_of_range);
/* Host.  Per valid class i: tp = the diagonal, fn = the row sum - tp, fp = the column sum over the other valid rows, denom[i] = tp + fp + fn,
 * iou[i] = tp / denom in binary64, NaN when denom is 0 (get_iou, evaluate_semantic_label.py:68-82).  tp and denom nullable.  dim: the matrix's. */
int sf_eval_iou(const uint64_t* confusion, uint32_t dim, const int32_t* valid_ids, uint32_t n_valid, double* iou, uint64_t* tp, uint64_t* denom);
/* Host.  gt_ids[n] are label * 1000 + k.  The instances are the distinct ids > 0 whose id / 1000 is a valid class, ascending: *count of them (G); the
 * first min(G, capacity) go to instance_id[] and instance_verts[] (nullable; SF_ERR_BOUNDS when capacity < G).  slot[n] (nullable): the index of the
 * vertex's instance, G where the vertex is void (id / 1000 no valid class) -- by the G of this call. */
int sf_eval_instance_plan(const int32_t* gt_ids, uint64_t n, const int32_t* valid_ids, uint32_t n_valid, int32_t* instance_id, uint32_t* instance_verts,
                          uint32_t capacity, uint32_t* slot, uint32_t* count);
/* masks[P][stride] bytes, a vertex is covered where the byte is non-zero; stride >= n.  table[P][G + 2] is WRITTEN: [p][g] = covered vertices of
 * prediction p in instance g, [p][G] = in void (a slot >= G), [p][G + 1] = covered vertices in all.  n below 2^32, P up to 65535, G up to 2^24. */
int sf_eval_instance_overlaps(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, int device /* -1: host */,
                              uint32_t* table);
int sf_eval_instance_overlaps_device(const uint32_t* slot, uint64_t n, uint32_t G, const uint8_t* masks, uint32_t P, uint64_t stride, void* stream,
                                     uint32_t* table);
/* The AP over scans (evaluate_matches and compute_averages, evaluate_semantic_instance.py:75-242).  add_scan takes a scan's plan, its predictions in
 * the order of the prediction file (label, confidence) and their overlap table; a prediction whose label is no valid class or that covers fewer than
 * min_region_size vertices is dropped.  finish: ap[n_valid][SF_EVAL_AP_OVERLAPS] (NaN: the class has no ground truth), class_averages[n_valid][3]
 * (nullable) = {mean over the nine overlaps 0.5 .. 0.9, at 0.5, at 0.25}, averages[3] (nullable) = their means over the classes that are not NaN. */
typedef struct sf_eval_ap sf_eval_ap;
int sf_eval_ap_create(const int32_t* valid_ids, uint32_t n_valid, uint32_t min_region_size /* 100 */, sf_eval_ap** out);
int sf_eval_ap_add_scan(sf_eval_ap* acc, uint32_t G, const int32_t* instance_id, const uint32_t* instance_verts, uint32_t P, const int32_t* pred_label,
                        const double* pred_conf, const uint32_t* table);
int sf_eval_ap_finish(const sf_eval_ap* acc, double* ap, double* class_averages, double* averages);
void sf_eval_ap_destroy(sf_eval_ap* acc);
/* The three scores from the benchmark's files, as the scripts take them (NYU40: the 20 label classes, the 18 instance classes).  Every `.txt` file of
 * pred_path (label, instance) or every file (pixel: PNG images, 8 or 16 bits, one channel) needs a file of its name in gt_path; the result file itself
 * is left out.  output_file NULL or "": pred_path/semantic_label_evaluation.txt, semantic_instance_evaluation.txt, semantic_label.txt.  The result
 * file is written in the script's layout (evaluate_semantic_label.py:85-103, evaluate_semantic_instance.py:350-360 with each number printed so that
 * it parses back to the same binary64, evalPixelLevelSemanticLabeling.py:157-173); *report (nullable; malloc'ed, sf_free) is the text of the tables the
 * script prints.  A class whose denominator is 0 prints nan.  SF_ERR_IO: no result files, a file without ground truth, an unreadable file;
 * SF_ERR_FORMAT: a line that is no integer, arrays of different lengths, a mask path that is absolute or leaves pred_path
 * (util_3d.py:125-145), an image of the wrong size or with several channels, a pixel id of 41 or more (named with its file). */
int sf_eval_label_dir(const char* pred_path, const char* gt_path, const char* output_file /*nullable*/, int device /* -1: host */, char** report);
int sf_eval_instance_dir(const char* pred_path, const char* gt_path, const char* output_file /*nullable*/, uint32_t min_region_size /* 100 */,
                         int device /* -1: host */, char** report);
int sf_eval_pixel_dir(const char* pred_path, const char* gt_path, const char* output_file /*nullable*/, int device /* -1: host */, char** report);
/* Host.  The ground truth of a scan per vertex (3d_helpers/export_train_mesh_for_evaluation.py:38-90): the segGroups in file order, a later group
 * overwrites an earlier one; label_ids[v] = the nyu40id the label map gives the group's label (columns raw_category -> nyu40id, util.py:32-42),
 * instance_ids[v] = the group's objectId + 1; 0 where no group holds the vertex's segment.  *num_vertices = the length of segIndices; the arrays
 * (each nullable) hold `capacity` values: SF_ERR_BOUNDS when that is too few.  SF_ERR_FORMAT: a label that is no raw_category of the map, a map
 * without the two columns, an nyu40id cell that is no integer. */
int sf_eval_export_ids(const char* segs_json, const char* aggregation_json, const char* label_map_tsv, uint64_t capacity, uint32_t* label_ids,
                       uint32_t* instance_ids, uint64_t* num_vertices);
/* The same to files, for the scan folder scan_path = .../<id> with <id>.aggregation.json and <id>_vh_clean_2.0.010000.segs.json in it.  type "label":
 * one label id per line (the reference's bytes); "instance": the prediction format -- a line `pred_mask/<name>_<k>.txt <label id> 1.000000` per
 * object, <name> the output file's name without its extension, k the object's position among the sorted distinct instance ids (0 counts where a
 * vertex is unannotated), and the 0/1 masks under pred_mask/ beside the output file (util_3d.py:57-77); "instance-gt": label id * 1000 + objectId + 1
 * per line, 0 where unannotated: what sf_eval_instance_dir reads as ground truth. */
int sf_eval_export_scan(const char* scan_path, const char* label_map_file, const char* type, const char* output_file);

/* ------------------------------------------------------------------------------------------------
 * Benchmark scores, 2-D instances: the image-level instance AP.  What they replace:
 * BenchmarkScripts/2d_evaluation/evalInstanceLevelSemanticLabeling.py:204-298 (assignGt2Preds), :301-496 (evaluateMatches), :498-515
 * (computeAverages) with instances2dict.py:27-46 and instance.py:13-24.  Ground truth is a batch of id images gt[batch][height][width] of
 * elem_bytes = 1, 2 or 4 bytes per pixel, all of one size, with fewer than 2^32 pixels each; a pixel is value = label * 1000 + k.  valid_ids: n_valid
 * distinct class ids 1 .. 999 (anything else: SF_ERR_INVALID_ARG), so that a void value can never be an instance id:
 *   instance  value / 1000 is a valid class (instances2dict.py:40-43)
 *   void      the raw value is itself a valid class id (evalInstanceLevelSemanticLabeling.py:226-230) -- not the 3-D void
 * Every count is an integer: device = -1 is the host path (at most 16 threads) and gives the counts the kernels give.  The _device twins follow the
 * rules of the _device calls above: device memory of one device, a HIP stream, nothing copied, nothing waited for, results left on the device,
 * the caller's current device put back, and a refused call has written nothing.
 * ---------------------------------------------------------------------------------------------- */
#define SF_EVAL_AP2D_OVERLAPS 10 /* numpy's arange(0.5, 1., 0.05) (evalInstanceLevelSemanticLabeling.py:74) */
/* The plan of every image: count[b] = its number of instances, instance_id[b][capacity] = their ids ascending, instance_pixels[b][capacity] = their
 * pixel counts; entries from count[b] on are not written.  The two arrays may both be NULL: only count[] is written.  Otherwise SF_ERR_BOUNDS when
 * some image holds more than `capacity` instances, and nothing is written then.  batch up to 65535, capacity up to 2^20. */
int sf_eval_image_plan(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids, uint32_t n_valid,
                       uint32_t capacity, int device /* -1: host */, uint32_t* count, int32_t* instance_id, uint32_t* instance_pixels);
/* Bytes of the counter array the device plan needs: batch * (largest valid id + 1) * 1000 * 4; 0 for arguments sf_eval_image_plan refuses. */
uint64_t sf_eval_image_plan_scratch(uint32_t batch, const int32_t* valid_ids /* host */, uint32_t n_valid);
/* scratch: sf_eval_image_plan_scratch() bytes, aligned to 16.  count[b] is the image's true number of instances, of which the first
 * min(count[b], capacity) are written: the caller compares count[] with its capacity once it has read it. */
int sf_eval_image_plan_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids /* host */,
                              uint32_t n_valid, uint32_t capacity, void* stream, void* scratch, uint32_t* count, int32_t* instance_id,
                              uint32_t* instance_pixels);
/* masks[P][stride] bytes (stride >= width * height), a pixel is covered where the byte is non-zero; mask p lies over image mask_image[p].
 * table[P][capacity + 2] is WRITTEN: [p][g] = covered pixels of mask p in instance g of its image (0 from count[] on), [p][capacity] = covered void
 * pixels, [p][capacity + 1] = covered pixels in all.  count and instance_id are sf_eval_image_plan's.  P up to 65535.  The host call refuses
 * (SF_ERR_INVALID_ARG) a count above capacity, ids that do not ascend and a mask_image >= batch; the _device twin cannot read them: it counts a
 * count above capacity as capacity and leaves the row of a mask without an image zero. */
int sf_eval_overlaps_images(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids, uint32_t n_valid,
                            uint32_t capacity, const uint32_t* count, const int32_t* instance_id, const uint8_t* masks, uint32_t P, uint64_t stride,
                            const uint32_t* mask_image, int device /* -1: host */, uint32_t* table);
int sf_eval_overlaps_images_device(const void* gt, int elem_bytes, uint32_t batch, uint32_t width, uint32_t height, const int32_t* valid_ids /* host */,
                                   uint32_t n_valid, uint32_t capacity, const uint32_t* count, const int32_t* instance_id, const uint8_t* masks, uint32_t P,
                                   uint64_t stride, const uint32_t* mask_image, void* stream, uint32_t* table);
/* The AP over images (evaluateMatches and computeAverages).  add_image takes one image's plan (G instances), its P predictions (label,
 * confidence; a NaN confidence is refused) and their rows table[P][capacity + 2], G <= capacity.  A prediction whose label is no valid class or that
 * covers no pixel is dropped; there is no minimum size for predictions.  Ground truth below min_region_size pixels is ignored, not matched.
 * finish: ap[n_valid][SF_EVAL_AP2D_OVERLAPS] (NaN: the class has no ground truth), class_averages[n_valid][2] (nullable) = {mean over the ten
 * thresholds, at 0.5}, averages[2] (nullable) = the mean of the ap entries that are not NaN, and of those at 0.5.  The result depends on neither
 * the order of the images nor the order of an image's predictions.  thresholds[SF_EVAL_AP2D_OVERLAPS]: the ten values, bit for bit numpy's. */
typedef struct sf_eval_ap2d sf_eval_ap2d;
int sf_eval_ap2d_create(const int32_t* valid_ids, uint32_t n_valid, uint32_t min_region_size /* 100 */, sf_eval_ap2d** out);
int sf_eval_ap2d_add_image(sf_eval_ap2d* acc, uint32_t G, const int32_t* instance_id, const uint32_t* instance_pixels, uint32_t P, const int32_t* pred_label,
                           const double* pred_conf, const uint32_t* table, uint32_t capacity);
int sf_eval_ap2d_finish(const sf_eval_ap2d* acc, double* ap, double* class_averages, double* averages);
void sf_eval_ap2d_destroy(sf_eval_ap2d* acc);
int sf_eval_ap2d_thresholds(double* thresholds);
/* evalInstanceLevelSemanticLabeling.py on its files, for the 18 instance classes.  Every `.txt` under pred_path, sub-folders included (:609-612),
 * is the prediction list of one image: lines `<relative path of a mask> <label id> <confidence>` split at single blanks (:122-137); its ground
 * truth is gt_path/<base name>.png, one channel of 8 or 16 bits; a mask is a one-channel 8-bit PNG of the same size, relative to the list's folder.
 * The result file (default pred_path/semantic_instance.txt; left out of the walk) has the lines of :567-576 with 17 significant digits per number;
 * *report (nullable; malloc'ed, sf_free) is the table of printResults (:517-553).  SF_ERR_IO: no lists, a list without ground truth, an unreadable
 * file; SF_ERR_FORMAT: a line that is not three fields, a number that is none, a NaN confidence, a mask path that is absolute or leaves pred_path,
 * two lists of one base name, an image that is not one channel of the bits above, a mask of another size (each named with its file). */
int sf_eval_instance2d_dir(const char* pred_path, const char* gt_path, const char* output_file /*nullable*/, uint32_t min_region_size /* 100 */,
                           int device /* -1: host */, char** report);

#ifdef __cplusplus
}
#endif
#endif /* SCANFUSE_H */
