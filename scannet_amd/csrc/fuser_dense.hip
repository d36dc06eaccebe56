// fuser_dense.hip -- the sparse volume as a dense one: a whole box of blocks allocated on the device, the bounding box of the observed voxels, and any
// region of the volume copied out as a dense [z][y][x] array.  What the free-space stage (freespace.cpp) is made of; each call is
// useful alone.  None of them touches a fusion kernel: a fuser on which they are never called behaves as before.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "fuser_device.h"
#include "fuser_internal.h"
#include "hip_util.h"

namespace {

constexpr int KEY_COORD_MIN = -(1 << 20), KEY_COORD_MAX = (1 << 20) - 1;   // what pack_key's 21 bits per axis hold

// ---------------------------------------------------------------------------------------------------
// k_alloc_box: one lane per block of the box, coordinates from the lane's index (x fastest).  insert == 0 only counts the blocks that are not
// in the table (the host compares that with the free heap before anything is changed); insert == 1 claims them with the table's own protocol
// (hash_find_or_claim + give_block, as k_import): birth 0 -- the block exists for every frame --, voxels as the heap holds them: zero.  The
// claiming lanes of a wave take their heap positions with ONE atomic on the heap counter.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_alloc_box(int lox, int loy, int loz, int nx, int ny, uint32_t n, int insert, unsigned long long* result,
                                                  HashEntry* table, int32_t* heap, uint64_t* block_keys, int32_t* block_entry, uint8_t* block_flags,
                                                  int32_t* counters, ParamsK P) {
  const HashRefs h{table, heap, block_keys, block_entry, block_flags, counters};
  const int lane = threadIdx.x & 63;
  const uint32_t waves = (n + 63u) / 64u;
  for (uint32_t wv = blockIdx.x * 4u + (threadIdx.x >> 6); wv < waves; wv += gridDim.x * 4u) {   // wave-uniform trip count: the ballots below see whole waves
    const uint32_t i = wv * 64u + (uint32_t)lane;
    bool got = false;
    HashEntry* e = nullptr;
    uint64_t key = 0;
    if (i < n) {
      const uint32_t row = i / (uint32_t)nx;
      const int bx = lox + (int)(i - row * (uint32_t)nx);
      const int by = loy + (int)(row % (uint32_t)ny);
      const int bz = loz + (int)(row / (uint32_t)ny);
      key = pack_key(bx, by, bz);
      if (insert) {
        e = hash_find_or_claim(h, P, key, bx, by, bz, 0u);
        got = e != nullptr;
      } else {
        got = hash_lookup(table, P, bx, by, bz) < 0;
      }
    }
    const unsigned long long m = __ballot(got);
    if (m == 0ull) continue;
    const int cnt = __popcll(m), leader = __ffsll(m) - 1;
    int base = 0;
    if (insert) {
      if (lane == leader) {
        atomicAdd(&counters[C_SLOTS_USED], cnt);
        base = atomicSub(&counters[C_HEAP_FREE], cnt);
      }
      base = __shfl(base, leader);
      if (got) give_block(h, e, key, base - 1 - __popcll(m & ((1ull << lane) - 1ull)));   // (a position below 0: heap exhausted, counted as a failure)
    }
    if (lane == leader) atomicAdd(result, (unsigned long long)cnt);
  }
}

// ---------------------------------------------------------------------------------------------------
// k_known_bounds: the inclusive box, in global voxel indices, of the voxels with weight > 0 over the listed blocks, and how many there are.  A workgroup
// reads one 4 KiB tile per turn (a lane: one 16-byte load, two voxels) and keeps its running box in registers; at the end a wave reduction, the four
// waves through LDS, one integer min / max / add per workgroup.  Integers: the order does not matter, the result is exact.
//   out[0..2] = min, out[3..5] = max (int32), out[6..7] = count (64-bit)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_known_bounds(const uint4* __restrict__ voxels, const uint64_t* __restrict__ block_keys, const int32_t* __restrict__ live,
                                                     int n, int32_t* out) {
  __shared__ int s_box[4][6];
  __shared__ uint32_t s_cnt[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lx = (t & 3) * 2, ly = (t >> 2) & 7, lz = t >> 5;
  int x0 = INT_MAX, y0 = INT_MAX, z0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN, z1 = INT_MIN;
  uint32_t cnt = 0;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int slot = live[i];
    const uint4 v = voxels[(size_t)slot * 256 + t];
    const bool k0 = (v.y >> 24) != 0u, k1 = (v.w >> 24) != 0u;
    if (k0 || k1) {
      int bx, by, bz;
      unpack_key(block_keys[slot], bx, by, bz);
      const int gx = 8 * bx + lx, gy = 8 * by + ly, gz = 8 * bz + lz;
      x0 = min(x0, k0 ? gx : gx + 1);
      x1 = max(x1, k1 ? gx + 1 : gx);
      y0 = min(y0, gy); y1 = max(y1, gy);
      z0 = min(z0, gz); z1 = max(z1, gz);
      cnt += (k0 ? 1u : 0u) + (k1 ? 1u : 0u);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    x0 = min(x0, __shfl_xor(x0, o)); y0 = min(y0, __shfl_xor(y0, o)); z0 = min(z0, __shfl_xor(z0, o));
    x1 = max(x1, __shfl_xor(x1, o)); y1 = max(y1, __shfl_xor(y1, o)); z1 = max(z1, __shfl_xor(z1, o));
    cnt += (uint32_t)__shfl_xor((int)cnt, o);
  }
  if (lane == 0) {
    s_box[wave][0] = x0; s_box[wave][1] = y0; s_box[wave][2] = z0;
    s_box[wave][3] = x1; s_box[wave][4] = y1; s_box[wave][5] = z1;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (t < 6) {
    const int a = s_box[0][t], b = s_box[1][t], c = s_box[2][t], d = s_box[3][t];
    if (t < 3) atomicMin(&out[t], min(min(a, b), min(c, d)));
    else atomicMax(&out[t], max(max(a, b), max(c, d)));
  } else if (t == 6) {
    const unsigned long long total = (unsigned long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (total) atomicAdd(reinterpret_cast<unsigned long long*>(out + 6), total);
  }
}

// ---------------------------------------------------------------------------------------------------
// k_export_dense: region [lo, lo + dims) of the volume as dense arrays, x fastest.  A workgroup owns a RUN of up to 8 blocks along x (one block row
// (by, bz) of the region's block grid at a time, grid-stride over the runs):
//   1. lanes 0..7 look the run's blocks up in the table -- one look-up per block, not per voxel;
//   2. the tiles go to LDS with one 16-byte load per lane and block (a block that is not allocated is a tile of zeros);
//   3. the 64 voxel rows of the run are written from LDS, a wave per row, lane = x within the run: 256 contiguous bytes of sdf, 64 of weight,
//      192 of rgb per row, whatever the alignment of the region.
// In LDS a tile takes 520 voxels' worth (4 160 bytes) instead of 4 096: with the 64-byte pad the eight blocks a wave reads one row of fall on
// different banks.
// ---------------------------------------------------------------------------------------------------
constexpr int RUN = 8;
constexpr int TILE_PITCH = 520;   // uint2 (voxels) per tile in LDS

struct DenseArgs {
  int lox, loy, loz;        // region origin, voxels
  int nx, ny, nz;           // region size, voxels
  int bx0, by0, bz0;        // first block of the region on each axis
  int nbx, nby, nbz;        // blocks the region touches on each axis
  int mode;
  float voxel;
  float* sdf;
  uint8_t* weight;
  uint8_t* rgb;
};

__global__ __launch_bounds__(256) void k_export_dense(const uint4* __restrict__ voxels, const HashEntry* __restrict__ table, DenseArgs A, ParamsK P) {
  __shared__ uint2 s_tile[RUN * TILE_PITCH];
  __shared__ int s_slot[RUN];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int runs_x = (A.nbx + RUN - 1) / RUN;
  const unsigned long long items = (unsigned long long)runs_x * (unsigned long long)A.nby * (unsigned long long)A.nbz;
  for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
    const unsigned long long row = it / (unsigned long long)runs_x;
    const int rx = (int)(it - row * (unsigned long long)runs_x);
    const int by = A.by0 + (int)(row % (unsigned long long)A.nby);
    const int bz = A.bz0 + (int)(row / (unsigned long long)A.nby);
    const int bxr = A.bx0 + rx * RUN;
    const int cnt = min(RUN, A.nbx - rx * RUN);
    if (t < RUN) {
      const int bx = bxr + t;
      const bool keyed = bx >= KEY_COORD_MIN && bx <= KEY_COORD_MAX && by >= KEY_COORD_MIN && by <= KEY_COORD_MAX && bz >= KEY_COORD_MIN && bz <= KEY_COORD_MAX;
      s_slot[t] = t < cnt && keyed ? hash_lookup(table, P, bx, by, bz) : -1;
    }
    __syncthreads();
    for (int b = 0; b < cnt; b++) {
      const int slot = s_slot[b];
      const uint4 v = slot >= 0 ? voxels[(size_t)slot * 256 + t] : make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4*>(&s_tile[b * TILE_PITCH + 2 * t]) = v;
    }
    __syncthreads();
    // (64-bit: the last block of a region that ends at the top of the 32-bit voxel range reaches past it)
    const long long ox = ((long long)bxr * 8 + lane) - A.lox;   // this lane's x in the region
    const bool x_in = lane < cnt * 8 && ox >= 0 && ox < A.nx;
    for (int r = wave; r < 64; r += 4) {       // row r of the run: ly = r & 7, lz = r >> 3
      const long long oy = (long long)by * 8 + (r & 7) - A.loy, oz = (long long)bz * 8 + (r >> 3) - A.loz;
      if (!x_in || oy < 0 || oy >= A.ny || oz < 0 || oz >= A.nz) continue;
      const uint2 q = s_tile[(lane >> 3) * TILE_PITCH + r * 8 + (lane & 7)];
      const size_t at = ((size_t)oz * (size_t)A.ny + (size_t)oy) * (size_t)A.nx + (size_t)ox;
      const uint32_t w = q.y >> 24;
      if (A.sdf) {
        float s = __uint_as_float(q.x);
        if (A.mode == 1) s = w == 0u ? -INFINITY : s / A.voxel;   // the task volume: voxel units, one true division
        A.sdf[at] = s;
      }
      if (A.weight) A.weight[at] = (uint8_t)w;
      if (A.rgb) {
        A.rgb[3 * at] = (uint8_t)(q.y & 0xFFu);
        A.rgb[3 * at + 1] = (uint8_t)((q.y >> 8) & 0xFFu);
        A.rgb[3 * at + 2] = (uint8_t)((q.y >> 16) & 0xFFu);
      }
    }
    __syncthreads();
  }
}

inline int floor_div8(int v) { return v >> 3; }

thread_local float t_dense_us = -1.0f;   // k_export_dense of the calling thread's most recent export on a fuser with profiling enabled

}  // namespace

SF_API int sf_fuser_allocate_box(sf_fuser* f, const int32_t lo_block[3], const int32_t hi_block[3], uint64_t* allocated) {
  if (allocated) *allocated = 0;
  if (!f || !lo_block || !hi_block) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  uint64_t n = 1;
  for (int a = 0; a < 3; a++) {
    if (lo_block[a] > hi_block[a]) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_allocate_box: lo %d > hi %d on axis %d", lo_block[a], hi_block[a], a);
    if (lo_block[a] < KEY_COORD_MIN || hi_block[a] > KEY_COORD_MAX)
      return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_allocate_box: block coordinates [%d, %d] on axis %d leave the table's 21-bit range", lo_block[a], hi_block[a], a);
    n *= (uint64_t)((int64_t)hi_block[a] - lo_block[a] + 1);   // each factor <= 2^21: no overflow before the test below
    if (n >= (1ull << 31)) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_allocate_box: a box of 2^31 or more blocks");
  }
  if (f->pk.slab_axis >= 0) return sf::fail(SF_ERR_UNSUPPORTED, "sf_fuser_allocate_box: a slab / stripe partition is set on this fuser");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  sf::DevBuf res_buf;
  SF_HIP_CHECK(res_buf.alloc(16));
  unsigned long long* d_res = res_buf.as<unsigned long long>();
  const int nx = hi_block[0] - lo_block[0] + 1, ny = hi_block[1] - lo_block[1] + 1;
  const uint32_t wgs = (uint32_t)((n + 255) / 256);
  const dim3 grid(wgs < (uint32_t)f->num_cus * 16u ? wgs : (uint32_t)f->num_cus * 16u);
  unsigned long long res[2] = {0, 0};
  int32_t heap_free = 0, fail0 = 0, fail1 = 0;
  hipError_t e = hipMemsetAsync(d_res, 0, 16, f->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_alloc_box, grid, dim3(256), 0, f->stream, lo_block[0], lo_block[1], lo_block[2], nx, ny, (uint32_t)n, 0, d_res, f->table, f->heap,
                       f->block_keys, f->block_entry, f->block_flags, f->counters, f->pk);
    e = hipMemcpyAsync(&res[0], d_res, 8, hipMemcpyDeviceToHost, f->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&heap_free, &f->counters[C_HEAP_FREE], 4, hipMemcpyDeviceToHost, f->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&fail0, &f->counters[C_ALLOC_FAIL], 4, hipMemcpyDeviceToHost, f->stream);
  if (e == hipSuccess) e = sf_quiesce(f);
  if (e != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuser_allocate_box: %s", hipGetErrorString(e));
  if (res[0] > (unsigned long long)(heap_free > 0 ? heap_free : 0))
    return sf::fail(SF_ERR_CAPACITY, "sf_fuser_allocate_box: the box needs %llu new blocks, the heap has %d free (num_sdf_blocks %u); nothing was changed", res[0],
                    heap_free, f->pk.num_blocks);
  if (res[0] > 0) {
    hipLaunchKernelGGL(k_alloc_box, grid, dim3(256), 0, f->stream, lo_block[0], lo_block[1], lo_block[2], nx, ny, (uint32_t)n, 1, d_res + 1, f->table, f->heap,
                       f->block_keys, f->block_entry, f->block_flags, f->counters, f->pk);
    e = hipMemcpyAsync(&res[1], d_res + 1, 8, hipMemcpyDeviceToHost, f->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&fail1, &f->counters[C_ALLOC_FAIL], 4, hipMemcpyDeviceToHost, f->stream);
    if (e == hipSuccess) e = sf_quiesce(f);
  } else {
    fail1 = fail0;
  }
  if (e != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuser_allocate_box: %s", hipGetErrorString(e));
  if (fail1 != fail0)
    return sf::fail(SF_ERR_CAPACITY, "sf_fuser_allocate_box: %d blocks of the box found no hash slot within %d probes (hash_num_buckets %u); sf_fuser_reset empties the volume",
                    fail1 - fail0, MAX_PROBES, f->pk.num_buckets);
  if (allocated) *allocated = (uint64_t)res[1] - (uint64_t)(fail1 - fail0);
  return SF_OK;
}

SF_API int sf_fuser_known_bounds(sf_fuser* f, int32_t lo_voxel[3], int32_t hi_voxel[3], uint64_t* known) {
  if (!f || !known) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  *known = 0;
  SF_HIP_CHECK(hipSetDevice(f->device));
  int32_t n = 0;
  const int rc = sf_compact_live(f, &n, 0);   // owned blocks: a ghost is a copy of somebody else's
  if (rc != SF_OK) return rc;
  if (n == 0) return SF_OK;
  int32_t box[8] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN, 0, 0};
  sf::DevBuf box_buf;
  SF_HIP_CHECK(box_buf.alloc(sizeof(box)));
  int32_t* d_box = box_buf.as<int32_t>();
  hipError_t e = hipMemcpyAsync(d_box, box, sizeof(box), hipMemcpyHostToDevice, f->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_known_bounds, dim3(n < f->num_cus * 8 ? n : f->num_cus * 8), dim3(256), 0, f->stream, f->voxels, f->block_keys, f->compact, n, d_box);
    e = hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, f->stream);
  }
  if (e == hipSuccess) e = sf_quiesce(f);
  if (e != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuser_known_bounds: %s", hipGetErrorString(e));
  uint64_t cnt;
  std::memcpy(&cnt, &box[6], 8);
  *known = cnt;
  if (cnt == 0) return SF_OK;
  for (int a = 0; a < 3; a++) {
    if (lo_voxel) lo_voxel[a] = box[a];
    if (hi_voxel) hi_voxel[a] = box[3 + a];
  }
  return SF_OK;
}

SF_API int sf_fuser_export_dense(sf_fuser* f, const int32_t lo_voxel[3], const int32_t dims[3], int mode, float* sdf, uint8_t* weight, uint8_t* rgb,
                                 int dst_on_device) {
  if (!f || !lo_voxel || !dims) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (mode != 0 && mode != 1) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_export_dense: mode %d (0: sdf as stored, 1: the task volume)", mode);
  uint64_t total = 1;
  for (int a = 0; a < 3; a++) {
    if (dims[a] <= 0) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_export_dense: dimension %d on axis %d", dims[a], a);
    if ((int64_t)lo_voxel[a] + dims[a] - 1 > INT32_MAX) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_export_dense: the region leaves the 32-bit voxel range on axis %d", a);
    total *= (uint64_t)dims[a];
    if (total >= (1ull << 40)) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_export_dense: a region of 2^40 or more voxels");
  }
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));   // behind everything queued on the handle, on whichever of its streams
  if (!sdf && !weight && !rgb) return SF_OK;
  DenseArgs A;
  A.lox = lo_voxel[0]; A.loy = lo_voxel[1]; A.loz = lo_voxel[2];
  A.nx = dims[0]; A.ny = dims[1]; A.nz = dims[2];
  A.bx0 = floor_div8(A.lox); A.by0 = floor_div8(A.loy); A.bz0 = floor_div8(A.loz);
  A.nbx = floor_div8(A.lox + A.nx - 1) - A.bx0 + 1;
  A.nby = floor_div8(A.loy + A.ny - 1) - A.by0 + 1;
  A.nbz = floor_div8(A.loz + A.nz - 1) - A.bz0 + 1;
  A.mode = mode;
  A.voxel = f->pk.voxel;
  A.sdf = sdf; A.weight = weight; A.rgb = rgb;
  sf::DevBuf tmp[3];   // the staging arrays of a host destination
  hipError_t e = hipSuccess;
  if (!dst_on_device) {
    if (sdf) { e = tmp[0].alloc(total * 4); A.sdf = tmp[0].as<float>(); }
    if (e == hipSuccess && weight) { e = tmp[1].alloc(total); A.weight = tmp[1].as<uint8_t>(); }
    if (e == hipSuccess && rgb) { e = tmp[2].alloc(total * 3); A.rgb = tmp[2].as<uint8_t>(); }
    if (e != hipSuccess)
      return sf::fail(SF_ERR_DEVICE, "sf_fuser_export_dense: hipMalloc of the staging arrays (%llu voxels) failed: %s", (unsigned long long)total, hipGetErrorString(e));
  }
  const unsigned long long items = (unsigned long long)((A.nbx + RUN - 1) / RUN) * (unsigned long long)A.nby * (unsigned long long)A.nbz;
  const unsigned long long cap = (unsigned long long)f->num_cus * 16ull;
  // sf_fuser_profile_enable: the kernel between two events of its own (sf_fuser_export_dense_kernel_us, scanfuse_internal.h)
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool timed = f->profile && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
  t_dense_us = -1.0f;
  if (timed) (void)hipEventRecord(ev[0], f->stream);
  hipLaunchKernelGGL(k_export_dense, dim3((unsigned)(items < cap ? items : cap)), dim3(256), 0, f->stream, f->voxels, f->table, A, f->pk);
  e = hipGetLastError();
  if (timed) (void)hipEventRecord(ev[1], f->stream);
  if (e == hipSuccess && !dst_on_device) {
    if (sdf) e = hipMemcpyAsync(sdf, tmp[0].p, total * 4, hipMemcpyDeviceToHost, f->stream);
    if (e == hipSuccess && weight) e = hipMemcpyAsync(weight, tmp[1].p, total, hipMemcpyDeviceToHost, f->stream);
    if (e == hipSuccess && rgb) e = hipMemcpyAsync(rgb, tmp[2].p, total * 3, hipMemcpyDeviceToHost, f->stream);
  }
  const hipError_t e2 = sf_quiesce(f);
  if (timed && e == hipSuccess && e2 == hipSuccess) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) t_dense_us = ms * 1000.0f;
  }
  for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
  if (e != hipSuccess || e2 != hipSuccess) return sf::fail(SF_ERR_DEVICE, "sf_fuser_export_dense: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  return SF_OK;
}

SF_API int sf_fuser_export_dense_kernel_us(float* us) {
  if (!us) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (t_dense_us < 0.0f) return sf::fail(SF_ERR_INVALID_ARG, "no timed export on this thread (sf_fuser_profile_enable, then sf_fuser_export_dense)");
  *us = t_dense_us;
  return SF_OK;
}
