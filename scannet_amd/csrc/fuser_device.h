// fuser_device.h -- device helpers that more than one stage of the fusion core uses: the block frustum test (allocation, compaction), the single-instruction
// min (allocation, integrate) and the find-or-claim of a hash entry with its heap block (allocation, import).  Included by the fuser*.hip translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "fuser_internal.h"

// bounding sphere of the block against the four side planes and the z range of the frustum (frustum_mode 0), or -- frustum_mode 1,
// DESIGN 6b -- VoxelHashing's isSDFBlockInCameraFrustumApprox: the block centre projected, normalised device coordinates x 0.95 inside
// [-1, 1]^2 x [0, 1] with z normalised by the SENSOR depth range.  Every operation individually rounded, true divisions: oracle/tsdf_oracle.c
// block_in_frustum runs the same sequence.
__device__ inline bool block_in_frustum(const ParamsK& P, const FrameK& F, int bx, int by, int bz) {
  const float cx = ((float)(8 * bx) + 3.5f) * P.voxel;
  const float cy = ((float)(8 * by) + 3.5f) * P.voxel;
  const float cz = ((float)(8 * bz) + 3.5f) * P.voxel;
  const float px = fmaf(F.Ti[0], cx, fmaf(F.Ti[1], cy, fmaf(F.Ti[2], cz, F.Ti[3])));
  const float py = fmaf(F.Ti[4], cx, fmaf(F.Ti[5], cy, fmaf(F.Ti[6], cz, F.Ti[7])));
  const float pz = fmaf(F.Ti[8], cx, fmaf(F.Ti[9], cy, fmaf(F.Ti[10], cz, F.Ti[11])));
  if (P.frustum_mode == 1) {   // kernarg scalar: a uniform branch
    const float zn = ((pz - P.dmin) / (P.dmax - P.dmin)) * 0.95f;
    if (!(zn >= 0.0f && zn <= 1.0f) || !(pz > 0.0f)) return false;   // also every NaN
    const float u = (px * P.fx) / pz + P.mx;
    const float v = (py * P.fy) / pz + P.my;
    const float wm1 = (float)(P.W - 1), hm1 = (float)(P.H - 1);
    const float nx = ((2.0f * u - wm1) / wm1) * 0.95f;
    const float ny = ((hm1 - 2.0f * v) / hm1) * 0.95f;
    return nx >= -1.0f && nx <= 1.0f && ny >= -1.0f && ny <= 1.0f;
  }
  bool in = pz > -F.radius;
  in = in && (pz < F.zfar + F.radius);
  in = in && (fmaf(F.xa[0], px, F.xc[0] * pz) >= -F.xr[0]);
  in = in && (fmaf(F.xa[1], px, F.xc[1] * pz) >= -F.xr[1]);
  in = in && (fmaf(F.ya[0], py, F.yc[0] * pz) >= -F.yr[0]);
  in = in && (fmaf(F.ya[1], py, F.yc[1] * pz) >= -F.yr[1]);
  return in;
}

// min(a, b) as ONE v_min_f32: fminf() makes clang canonicalise both operands first (v_max_f32 x, x, x each -- three instructions per voxel
// where the spec's min needs one; 16 of the 267 VALU instructions of a lane's frame).  The operands here are never NaN (depths come from
// 16-bit integers), and on equal or infinite operands v_min_f32 and fminf agree.
__device__ inline float min_f32(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

struct HashRefs {
  HashEntry* table;
  int32_t* heap;
  uint64_t* block_keys;
  int32_t* block_entry;
  uint8_t* block_flags;
  int32_t* counters;
  BrickCache bricks;   // presence cache (fuser_internal.h); bricks.e == nullptr: none
  uint32_t seq0;       // sequence number of the batch's first frame: a block born before it is older than every frame that asks now
};

// A block is "born" in the first frame that asks for it: frames of one batch are allocated by ONE launch, so the
// entry keeps the minimum sequence number over everybody who found or claimed it (the frames before its birth
// must not update the block -- sequentially it did not exist yet).
__device__ inline uint32_t note_birth(HashEntry* e, uint32_t seq) {
  const uint32_t b = __hip_atomic_load(&e->birth, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (b > seq) atomicMin(&e->birth, seq);
  return b;
}

// find-or-claim `key`; returns the claimed entry (needs a heap block) or nullptr (already present / table full)
__device__ inline HashEntry* hash_find_or_claim(const HashRefs& h, const ParamsK& P, uint64_t key, int bx, int by, int bz, uint32_t seq, int probe0 = 0) {
  uint32_t slot = hash_home(P, bx, by, bz) + (uint32_t)probe0;   // (probe0 > 0: the caller has looked at the first probe0 slots itself)
  if (slot >= P.total_slots) slot -= P.total_slots;
  for (int probe = probe0; probe < MAX_PROBES; ++probe) {
    HashEntry* e = h.table + slot;
    const uint64_t k = __hip_atomic_load(&e->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) {
      // found, and born before this batch: no later frame has anything to do for this block -- the presence cache may say so from now on
      if (note_birth(e, seq) < h.seq0 && h.bricks.e != nullptr) brick_note(h.bricks, bx, by, bz);
      return nullptr;
    }
    if (k == KEY_EMPTY) {
      const uint64_t old = atomicCAS((unsigned long long*)&e->key, (unsigned long long)KEY_EMPTY, (unsigned long long)key);
      if (old == KEY_EMPTY) { atomicMin(&e->birth, seq); return e; }   // (ours: no need to look at the birth frame first -- one round trip less in a chain of four)
      if (old == key) { note_birth(e, seq); return nullptr; }
    }
    slot++;
    if (slot == P.total_slots) slot = 0;
  }
  atomicAdd(&h.counters[C_ALLOC_FAIL], 1);
  return nullptr;
}

// hands heap position `at` to the claimed entry; returns the block's index + 1 for the caller's high-water mark (0: heap exhausted)
__device__ inline int give_block_quiet(const HashRefs& h, HashEntry* e, uint64_t key, int at) {
  if (at >= 0) {
    const int idx = h.heap[at];
    e->ptr = idx;
    h.block_keys[idx] = key;
    h.block_entry[idx] = (int32_t)(e - h.table);
    h.block_flags[idx] = 0;
    return idx + 1;
  }
  // heap exhausted: the entry stays claimed without a block; undo the pop and the caller's count of it as a used slot (a block that does not exist is counted
  // as a failure and nowhere else: hash_slots_used stays blocks_allocated, tests/front_exact.py check_directory)
  atomicAdd(&h.counters[C_HEAP_FREE], 1);
  atomicSub(&h.counters[C_SLOTS_USED], 1);
  atomicAdd(&h.counters[C_ALLOC_FAIL], 1);
  return 0;
}
// (no look at the mark first: a load of the word every workgroup's atomics land on waits in their queue like one of them, and the wave waits for IT -- measured
// on a 20-frame call into an empty volume, where every block is new: k_alloc_ray 114 -> 151 us per launch; the atomic without a return value costs the wave nothing)
__device__ inline void raise_high_water(const HashRefs& h, int hw) {
  if (hw > 0) atomicMax(&h.counters[C_HIGH_WATER], hw);
}
__device__ inline void give_block(const HashRefs& h, HashEntry* e, uint64_t key, int at) { raise_high_water(h, give_block_quiet(h, e, key, at)); }
