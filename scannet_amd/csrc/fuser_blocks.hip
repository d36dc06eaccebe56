// fuser_blocks.hip -- block maintenance outside the fusion passes: heap initialisation, garbage collection, export and import of blocks, and the
// slab / stripe partition of one scan over several GPUs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fuser_device.h"
#include "fuser_internal.h"
#include "hip_util.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// Garbage collection: one 256-thread workgroup per live block; min |sdf| over observed
// voxels and max weight reduced through wave shuffles + LDS; freed blocks are zeroed, unlinked
// (tombstone) and pushed back on the heap.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gc(uint4* voxels, uint64_t* block_keys, const int32_t* __restrict__ live,
                                            HashEntry* table, int32_t* heap, int32_t* counters, float thr, ParamsK P) {
  __shared__ float s_min[4];
  __shared__ uint32_t s_max[4];
  const int n = counters[C_EXPORT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int slot = live[i];
    uint4* vb = voxels + (size_t)slot * 256;
    const uint4 v = vb[threadIdx.x];
    float mn = INFINITY;
    uint32_t mw = 0;
    const uint32_t w0 = v.y >> 24, w1 = v.w >> 24;
    if (w0 > 0) mn = fminf(mn, fabsf(__uint_as_float(v.x)));
    if (w1 > 0) mn = fminf(mn, fabsf(__uint_as_float(v.z)));
    mw = max(w0, w1);
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o));
      mw = max(mw, (uint32_t)__shfl_xor((int)mw, o));
    }
    if (lane == 0) { s_min[wave] = mn; s_max[wave] = mw; }
    __syncthreads();
    mn = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
    mw = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    __syncthreads();
    if (mw == 0 || mn >= thr) {
      vb[threadIdx.x] = make_uint4(0, 0, 0, 0);
      if (threadIdx.x == 0) {
        const uint64_t key = block_keys[slot];
        int bx, by, bz;
        unpack_key(key, bx, by, bz);
        uint32_t s = hash_home(P, bx, by, bz);
        for (int probe = 0; probe < MAX_PROBES; ++probe) {
          if (table[s].key == key) { table[s].key = KEY_TOMB; table[s].ptr = -1; break; }
          if (table[s].key == KEY_EMPTY) break;
          s++;
          if (s == P.total_slots) s = 0;
        }
        block_keys[slot] = KEY_EMPTY;
        const int at = atomicAdd(&counters[C_HEAP_FREE], 1);
        heap[at] = slot;
        atomicAdd(&counters[C_GC_FREED], 1);
      }
    }
  }
}

// After a collection that freed blocks: the hash table rebuilt from the directory.  Lock-free open addressing cannot reuse a tombstone
// safely while other lanes insert the same key (one claims the tombstone, another has already walked past it and claims an empty slot
// further on), and tombstones that are never reused only lengthen every probe chain over a long scan (round-1 finding).  Collection is
// synchronous, so it simply leaves no tombstone behind: table cleared, every live block (ghosts included) re-inserted at its home
// position, block_entry re-pointed.  A surviving block existed before the next batch, so its birth stamp restarts at 0.
__global__ __launch_bounds__(256) void k_rehash(HashEntry* table, const uint64_t* __restrict__ block_keys, int32_t* block_entry, int32_t* counters, ParamsK P) {
  const int hw = counters[C_HIGH_WATER];
  for (int slot = blockIdx.x * 256 + threadIdx.x; slot < hw; slot += gridDim.x * 256) {
    const uint64_t key = block_keys[slot];
    if (key == KEY_EMPTY) continue;
    int bx, by, bz;
    unpack_key(key, bx, by, bz);
    uint32_t at = hash_home(P, bx, by, bz);
    for (int probe = 0; probe < MAX_PROBES; ++probe) {
      if (atomicCAS((unsigned long long*)&table[at].key, (unsigned long long)KEY_EMPTY, (unsigned long long)key) == KEY_EMPTY) {
        table[at].ptr = slot;
        table[at].birth = 0u;
        block_entry[slot] = (int32_t)at;
        atomicAdd(&counters[C_SLOTS_USED], 1);
        break;
      }
      at++;
      if (at == P.total_slots) at = 0;
      // no slot within MAX_PROBES (the rebuild inserts in directory order, a key can land further from home than it was): the block stays in
      // the directory but cannot be looked up -- counted, sf_fuser_garbage_collect reports SF_ERR_CAPACITY
      if (probe == MAX_PROBES - 1) atomicAdd(&counters[C_ALLOC_FAIL], 1);
    }
  }
}

__global__ void k_init_heap(int32_t* heap, uint64_t* block_keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { heap[i] = n - 1 - i; block_keys[i] = KEY_EMPTY; }
}

__global__ __launch_bounds__(256) void k_gather(const uint4* __restrict__ voxels, const uint64_t* __restrict__ block_keys,
                                                const int32_t* __restrict__ live, int n, int32_t* coords, uint4* out) {
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int slot = live[i];
    out[(size_t)i * 256 + threadIdx.x] = voxels[(size_t)slot * 256 + threadIdx.x];
    if (threadIdx.x == 0) {
      int bx, by, bz;
      unpack_key(block_keys[slot], bx, by, bz);
      coords[3 * i] = bx; coords[3 * i + 1] = by; coords[3 * i + 2] = bz;
    }
  }
}

// Filtered export: the live blocks whose coordinate on `axis` lies in [lo, hi) (axis == -1: all; axis == -2: the boundary layers
// of this fuser's slab / stripes), appended in no particular order.  One workgroup per candidate block.
__global__ __launch_bounds__(256) void k_gather_where(const uint4* __restrict__ voxels, const uint64_t* __restrict__ block_keys,
                                                      const int32_t* __restrict__ live, int n, int axis, int lo, int hi, int capacity,
                                                      int32_t* counter, int32_t* coords, uint4* out, ParamsK P) {
  __shared__ int s_pos;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int slot = live[i];
    int bx, by, bz;
    unpack_key(block_keys[slot], bx, by, bz);
    const int c = axis == 0 ? bx : (axis == 1 ? by : bz);
    if (axis >= 0 && (c < lo || c >= hi)) continue;  // uniform per workgroup
    if (axis == -2 && !slab_boundary(P, bx, by, bz)) continue;  // the boundary layers of this fuser's slab / stripes
    if (threadIdx.x == 0) s_pos = atomicAdd(counter, 1);
    __syncthreads();
    const int pos = s_pos;
    if (pos < capacity && out != nullptr) {
      out[(size_t)pos * 256 + threadIdx.x] = voxels[(size_t)slot * 256 + threadIdx.x];
      if (threadIdx.x == 0) { coords[3 * pos] = bx; coords[3 * pos + 1] = by; coords[3 * pos + 2] = bz; }
    }
    __syncthreads();
  }
}

// Import: one workgroup per block; lane 0 finds or creates the entry (+ heap pop), all lanes copy the 4 KiB tile.  only_wanted: of an
// all-gathered payload keep just the blocks this fuser needs as ghosts (slab_wants_ghost), counted in C_IMPORTED.
__global__ __launch_bounds__(256) void k_import(const int32_t* __restrict__ coords, const uint4* __restrict__ src, int n, int ghost, int only_wanted,
                                                uint4* voxels, HashEntry* table, int32_t* heap, uint64_t* block_keys, int32_t* block_entry,
                                                uint8_t* block_flags, int32_t* counters, ParamsK P) {
  __shared__ int s_slot;
  const HashRefs h{table, heap, block_keys, block_entry, block_flags, counters};
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    if (threadIdx.x == 0) {
      const int bx = coords[3 * i], by = coords[3 * i + 1], bz = coords[3 * i + 2];
      int slot = -1;
      if (!only_wanted || slab_wants_ghost(P, bx, by, bz)) {
        const uint64_t key = pack_key(bx, by, bz);
        HashEntry* e = hash_find_or_claim(h, P, key, bx, by, bz, 0u);
        if (e) {
          atomicAdd(&counters[C_SLOTS_USED], 1);
          give_block(h, e, key, atomicSub(&counters[C_HEAP_FREE], 1) - 1);
          slot = e->ptr >= 0 && block_keys[e->ptr] == key ? e->ptr : -1;  // -1: heap exhausted
        } else {
          slot = hash_lookup(table, P, bx, by, bz);  // already present (re-import): overwrite
        }
        if (slot >= 0) { block_flags[slot] = ghost ? 1 : 0; atomicAdd(&counters[C_IMPORTED], 1); }
      }
      s_slot = slot;
    }
    __syncthreads();
    const int slot = s_slot;
    if (slot >= 0) voxels[(size_t)slot * 256 + threadIdx.x] = src[(size_t)i * 256 + threadIdx.x];
    __syncthreads();
  }
}

}  // namespace

void sf_launch_init_heap(const sf_fuser* f) {
  hipLaunchKernelGGL(k_init_heap, dim3((f->pk.num_blocks + 255) / 256), dim3(256), 0, f->stream, f->heap, f->block_keys, (int)f->pk.num_blocks);
}

SF_API int sf_fuser_garbage_collect(sf_fuser* f, uint32_t* freed) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  SF_HIP_CHECK(hipSetDevice(f->device));
  int32_t n = 0;
  const int rc = sf_compact_live(f, &n, 0);
  if (rc != SF_OK) return rc;
  SF_HIP_CHECK(hipMemsetAsync(&f->counters[C_GC_FREED], 0, 4, f->stream));
  const float thr = std::fmaf(f->p.trunc_scale, f->p.depth_max, f->p.trunc_base);
  if (n > 0)
    hipLaunchKernelGGL(k_gc, dim3(n < f->num_cus * 8 ? n : f->num_cus * 8), dim3(256), 0, f->stream, f->voxels, f->block_keys, f->compact,
                       f->table, f->heap, f->counters, thr, f->pk);
  int32_t fr = 0;
  SF_HIP_CHECK(hipMemcpyAsync(&fr, &f->counters[C_GC_FREED], 4, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  int32_t fail0 = 0, fail1 = 0;
  if (fr > 0) {   // leave no tombstone behind: rebuild the table from the directory
    SF_HIP_CHECK(hipMemcpyAsync(&fail0, &f->counters[C_ALLOC_FAIL], 4, hipMemcpyDeviceToHost, f->stream));
    SF_HIP_CHECK(hipMemsetAsync(f->table, 0xFF, (size_t)f->pk.total_slots * sizeof(HashEntry), f->stream));
    SF_HIP_CHECK(hipMemsetAsync(f->bricks, 0, (size_t)f->brick_lines * 128, f->stream));   // blocks left the table: the presence cache starts again
    SF_HIP_CHECK(hipMemsetAsync(&f->counters[C_SLOTS_USED], 0, 4, f->stream));
    hipLaunchKernelGGL(k_rehash, dim3(f->compact_grid), dim3(256), 0, f->stream, f->table, f->block_keys, f->block_entry, f->counters, f->pk);
    SF_HIP_CHECK(hipMemcpyAsync(&fail1, &f->counters[C_ALLOC_FAIL], 4, hipMemcpyDeviceToHost, f->stream));
    SF_HIP_CHECK(sf_quiesce(f));
  }
  if (freed) *freed = (uint32_t)fr;
  if (fail1 != fail0) return sf::fail(SF_ERR_CAPACITY, "garbage collection: %d surviving blocks found no hash slot within %d probes when the table was rebuilt", fail1 - fail0, MAX_PROBES);
  return SF_OK;
}

SF_API int sf_fuser_export_blocks(sf_fuser* f, int32_t* coords, void* voxels, uint64_t capacity, uint64_t* n_out) {
  if (!f || !n_out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  int32_t n = 0;
  const int rc = sf_compact_live(f, &n);
  if (rc != SF_OK) return rc;
  *n_out = (uint64_t)n;
  if (!coords && !voxels) return SF_OK;
  if (!coords || !voxels) return sf::fail(SF_ERR_INVALID_ARG, "coords and voxels must both be given");
  if (capacity < (uint64_t)n) return sf::fail(SF_ERR_BOUNDS, "capacity %llu < %d live blocks", (unsigned long long)capacity, n);
  if (n == 0) return SF_OK;
  sf::DevBuf d_coords, d_vox;
  SF_HIP_CHECK(d_coords.alloc((size_t)n * 12));
  SF_HIP_CHECK(d_vox.alloc((size_t)n * 4096));
  hipLaunchKernelGGL(k_gather, dim3(n < 65535 ? n : 65535), dim3(256), 0, f->stream, f->voxels, f->block_keys, f->compact, n, d_coords.as<int32_t>(), d_vox.as<uint4>());
  hipError_t e1 = hipMemcpyAsync(coords, d_coords.p, (size_t)n * 12, hipMemcpyDeviceToHost, f->stream);
  hipError_t e2 = hipMemcpyAsync(voxels, d_vox.p, (size_t)n * 4096, hipMemcpyDeviceToHost, f->stream);
  hipError_t e3 = sf_quiesce(f);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return sf::fail(SF_ERR_DEVICE, "export copy failed");
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------------
// One large scan over several GPUs (BASELINE configs[4]): slab ownership, boundary layer export / import
// ------------------------------------------------------------------------------------------------------
SF_API int sf_fuser_set_slab(sf_fuser* f, int axis, int32_t lo_block, int32_t hi_block) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  if (axis > 2) return sf::fail(SF_ERR_INVALID_ARG, "axis must be 0, 1, 2 or negative (no partition)");
  if (axis >= 0 && !(lo_block < hi_block)) return sf::fail(SF_ERR_INVALID_ARG, "empty slab [%d, %d)", lo_block, hi_block);
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  f->pk.slab_axis = axis < 0 ? -1 : axis;
  f->pk.slab_lo = lo_block;
  f->pk.slab_hi = hi_block;
  f->pk.slab_thick = 0; f->pk.slab_world = 1; f->pk.slab_rank = 0;
  return SF_OK;
}

SF_API int sf_fuser_set_stripes(sf_fuser* f, int axis, int32_t origin_block, int32_t thickness_blocks, int world, int rank) {
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  if (axis < 0 || axis > 2 || thickness_blocks < 1 || world < 1 || rank < 0 || rank >= world)
    return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_set_stripes: axis %d, thickness %d, rank %d of %d", axis, thickness_blocks, rank, world);
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  f->pk.slab_axis = axis;
  f->pk.slab_lo = origin_block;
  f->pk.slab_hi = 0;
  f->pk.slab_thick = thickness_blocks; f->pk.slab_world = world; f->pk.slab_rank = rank;
  return SF_OK;
}

SF_API int sf_fuser_export_boundary(sf_fuser* f, int32_t* coords, void* voxels, uint64_t capacity, uint64_t* n_out, int dst_on_device) {
  return sf_fuser_export_blocks_where(f, -2, 0, 0, 0, coords, voxels, capacity, n_out, dst_on_device);
}

SF_API int sf_fuser_export_blocks_where(sf_fuser* f, int axis, int32_t lo, int32_t hi, int include_ghosts, int32_t* coords, void* voxels,
                                        uint64_t capacity, uint64_t* n_out, int dst_on_device) {
  if (!f || !n_out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if ((coords == nullptr) != (voxels == nullptr)) return sf::fail(SF_ERR_INVALID_ARG, "coords and voxels must both be given (or both NULL to count)");
  SF_HIP_CHECK(hipSetDevice(f->device));
  int32_t n_live = 0;
  const int rc = sf_compact_live(f, &n_live, include_ghosts);
  if (rc != SF_OK) return rc;
  *n_out = 0;
  if (n_live == 0) return SF_OK;
  SF_HIP_CHECK(hipMemsetAsync(&f->counters[C_GC_FREED], 0, 4, f->stream));  // scratch counter (GC is synchronous, never concurrent)
  const bool want = coords != nullptr;
  const int cap = (int)std::min<uint64_t>(capacity, 0x7FFFFFFFull);
  const bool staged = want && !dst_on_device && cap > 0;   // a host destination: gathered into buffers of the call's own, then copied out
  sf::DevBuf own_coords, own_vox;
  if (staged) {
    SF_HIP_CHECK(own_coords.alloc((size_t)cap * 12));
    SF_HIP_CHECK(own_vox.alloc((size_t)cap * 4096));
  }
  int32_t* d_coords = staged ? own_coords.as<int32_t>() : coords;   // null when the call only counts
  uint4* d_vox = staged ? own_vox.as<uint4>() : (uint4*)voxels;
  hipLaunchKernelGGL(k_gather_where, dim3(n_live < 65535 ? n_live : 65535), dim3(256), 0, f->stream, f->voxels, f->block_keys, f->compact, n_live, axis, lo, hi,
                     want ? cap : 0, &f->counters[C_GC_FREED], d_coords, want && cap > 0 ? d_vox : nullptr, f->pk);
  int32_t n = 0;
  hipError_t e = hipMemcpyAsync(&n, &f->counters[C_GC_FREED], 4, hipMemcpyDeviceToHost, f->stream);
  if (e == hipSuccess) e = sf_quiesce(f);
  if (e == hipSuccess && staged) {
    const size_t m = (size_t)std::min(n, cap);
    e = hipMemcpy(coords, d_coords, m * 12, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(voxels, d_vox, m * 4096, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return sf::fail(SF_ERR_DEVICE, "export failed: %s", hipGetErrorString(e));
  *n_out = (uint64_t)n;
  if (want && (uint64_t)n > capacity) return sf::fail(SF_ERR_BOUNDS, "capacity %llu < %d matching blocks", (unsigned long long)capacity, n);
  return SF_OK;
}

static int import_blocks(sf_fuser* f, const int32_t* coords, const void* voxels, uint64_t n, int ghost, int src_on_device, int only_wanted, uint64_t* imported);

SF_API int sf_fuser_import_blocks(sf_fuser* f, const int32_t* coords, const void* voxels, uint64_t n, int ghost, int src_on_device) {
  return import_blocks(f, coords, voxels, n, ghost, src_on_device, 0, nullptr);
}
SF_API int sf_fuser_import_ghosts(sf_fuser* f, const int32_t* coords, const void* voxels, uint64_t n, int src_on_device, uint64_t* imported) {
  return import_blocks(f, coords, voxels, n, 1, src_on_device, 1, imported);
}

static int import_blocks(sf_fuser* f, const int32_t* coords, const void* voxels, uint64_t n, int ghost, int src_on_device, int only_wanted, uint64_t* imported) {
  if (imported) *imported = 0;
  if (!f || (n && (!coords || !voxels))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (n == 0) return SF_OK;
  if (n > 0x7FFFFFFFull) return sf::fail(SF_ERR_INVALID_ARG, "too many blocks");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  const int32_t* d_coords = coords;
  const uint4* d_vox = (const uint4*)voxels;
  sf::DevBuf tmp_c, tmp_v;
  if (!src_on_device) {
    SF_HIP_CHECK(tmp_c.alloc(n * 12));
    SF_HIP_CHECK(tmp_v.alloc(n * 4096));
    SF_HIP_CHECK(hipMemcpy(tmp_c.p, coords, n * 12, hipMemcpyHostToDevice));
    SF_HIP_CHECK(hipMemcpy(tmp_v.p, voxels, n * 4096, hipMemcpyHostToDevice));
    d_coords = tmp_c.as<int32_t>();
    d_vox = tmp_v.as<uint4>();
  }
  int32_t fail0 = 0, fail1 = 0, took = 0;
  (void)hipMemcpy(&fail0, &f->counters[C_ALLOC_FAIL], 4, hipMemcpyDeviceToHost);
  (void)hipMemsetAsync(&f->counters[C_IMPORTED], 0, 4, f->stream);
  hipLaunchKernelGGL(k_import, dim3(n < 65535 ? (unsigned)n : 65535u), dim3(256), 0, f->stream, d_coords, d_vox, (int)n, ghost, only_wanted, f->voxels, f->table,
                     f->heap, f->block_keys, f->block_entry, f->block_flags, f->counters, f->pk);
  hipError_t e = hipMemcpyAsync(&fail1, &f->counters[C_ALLOC_FAIL], 4, hipMemcpyDeviceToHost, f->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&took, &f->counters[C_IMPORTED], 4, hipMemcpyDeviceToHost, f->stream);
  if (e == hipSuccess) e = sf_quiesce(f);
  if (imported) *imported = (uint64_t)took;
  if (e != hipSuccess) return sf::fail(SF_ERR_DEVICE, "import failed: %s", hipGetErrorString(e));
  if (fail1 != fail0) return sf::fail(SF_ERR_CAPACITY, "%d imported blocks did not fit (heap or hash table exhausted)", fail1 - fail0);
  return SF_OK;
}
