// fuser_alloc.hip -- stage 2 of a fusion pass: sparse block allocation.  k_alloc walks each ray's blocks through a cube window, k_alloc_ray through a
// window that follows the pencil of rays of a pixel tile; sf_fuser_create picks the window from the geometry, sf_launch_alloc the variant per pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "fuser_device.h"
#include "fuser_internal.h"

namespace {

// rv = RN(1 / voxel): the division itself through div_rn (fuser_internal.h), bit for bit w / voxel
__device__ inline int world_to_block(float w, float voxel, float rv) {
  const float q = div_rn(w, voxel, rv);
  const int vi = (int)(q >= 0.0f ? q + 0.5f : q - 0.5f);
  return vi >> 3;
}

// ---------------------------------------------------------------------------------------------------
// K2: allocation.  One lane per depth pixel, one 256-thread workgroup per 16x16 pixel tile and per GROUP of
// consecutive frames of the batch (blockIdx.z): the same pixel tile of neighbouring frames looks at almost the
// same blocks, so the workgroup walks its frames in order and only the blocks a frame adds go any further.
//   phase 1, per frame (no global memory traffic except the 1 KiB of depth):
//            every lane walks its 3-D DDA over the blocks of [d - t, d + t] and sets ONE BIT per visited block in
//            an LDS occupancy bitmap of a WIN^3-block window anchored at the tile's first ray (non-returning
//            ds_or: no latency on the lane, duplicates across the 256 rays and across steps collapse for free);
//            then the bitmap words are scanned: bits not yet queued by an earlier frame of the group are
//            frustum-tested for THIS frame and queued as (key, frame).  Rays that leave the window (tiles
//            straddling a depth discontinuity) go through a small LDS hash set instead.
//   phase 2, once per workgroup: the queued keys are probed in the global hash table by all lanes in parallel
//            (one memory round trip instead of one per DDA step); an EMPTY slot is claimed with a lock-free
//            64-bit CAS, the entry's birth frame becomes the minimum over everybody who asked for the block, and
//            the freshly claimed slots of a wave receive their heap blocks through ONE wave-aggregated pop
//            (ballot + prefix popcount).
// The allocated SET and every block's birth frame are deterministic (no insertion ever gives up, so no fix-point
// iteration as upstream); which heap slot a block lands in is not (neither is it upstream).
// ---------------------------------------------------------------------------------------------------
constexpr int ALLOC_SET = 256;        // LDS hash-set slots per workgroup (2 KiB): blocks outside the window
constexpr int ALLOC_LIST = 512;       // queue of (key, frame) for phase 2 (4 KiB + 0.5 KiB); 14.5 KiB LDS per workgroup in all => 8 workgroups per CU
constexpr int ALLOC_SET_PROBES = 32;

template <int WIN_LOG2, bool MULTI>
__global__ __launch_bounds__(256) void k_alloc(const float* __restrict__ depthf_all, HashEntry* table, int32_t* heap,
                                               uint64_t* block_keys, int32_t* block_entry, uint8_t* block_flags, int32_t* counters, ParamsK P,
                                               BatchFrames B, int group_frames, BrickCache bricks) {
  constexpr int WIN = 1 << WIN_LOG2;                // window edge in blocks
  // the queue of a workgroup: at 1 mm voxels (WIN 64) a pixel tile's rays visit ~1 300 blocks per frame -- with the 512 entries that serve 4 mm ALL of them
  // overflowed into the one-by-one path (sf_fuser_alloc_direct_count: 1.3 M blocks per frame, k_alloc<6> 2.2 ms: tools/gpu/alloc_1mm_probe.py)
  constexpr int LIST = WIN_LOG2 >= 6 ? 4096 : ALLOC_LIST;
  // (8 192 entries and a 2 048-slot set take the direct path from 1.3 M to 8 k blocks per frame and the kernel nowhere: its time is the table probes themselves,
  // profiles/r06_alloc_1mm.txt; 4 096 entries keep two workgroups per CU)
  constexpr int SET_LOG2 = 8, SET = 1 << SET_LOG2;
  constexpr int WIN_WORDS = (WIN * WIN * WIN) / 32; // occupancy bitmap words: 4 KiB (WIN 32) / 32 KiB (WIN 64)
  __shared__ uint32_t s_frame[WIN_WORDS];           // blocks the current frame's rays visit
  __shared__ uint32_t s_done[MULTI ? WIN_WORDS : 1];// blocks an earlier frame of the group has already queued
  __shared__ unsigned long long s_keys[SET];  // the same for blocks outside the window
  __shared__ unsigned long long s_list[LIST]; // queue for phase 2
  __shared__ uint8_t s_birth[LIST];           // ... and the frame (index in the batch) that queued the key
  __shared__ int s_count;
  __shared__ int s_chooser;
  __shared__ int s_anchored;
  __shared__ int s_anchor[3];
  __shared__ int s_box[6];
  __shared__ int s_claimed, s_pop_base;   // drain(): entries claimed by the workgroup in this call, and where its blocks start in the heap
  // the current frame's constants for the frustum tests of the scan (and of rays outside the window), two frames' worth so that a frame's copy never lands
  // under the previous frame's readers.  Read as B.f[j] they come through the scalar unit from the kernarg segment, a few words per load, each load a round
  // trip the wave waits for: at 1 mm voxels a tile names ~1 300 blocks per frame and a wave of k_alloc<6> spent its life -- 610 scalar loads, three quarters
  // of its cycles waiting (profiles/r06_pmc_alloc_1mm.txt) -- in that chain
  __shared__ uint32_t s_fk[2][sizeof(FrameK) / 4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) { s_count = 0; s_chooser = 256; s_anchored = 0; }
  if (threadIdx.x < 6) s_box[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
  const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  const HashRefs h{table, heap, block_keys, block_entry, block_flags, counters, bricks, B.seq0};
  for (int i = threadIdx.x; i < SET; i += 256) s_keys[i] = KEY_EMPTY;
  if (MULTI)
    for (int i = threadIdx.x; i < WIN_WORDS; i += 256) s_done[i] = 0u;
  const size_t npx = (size_t)P.W * P.H;
  const int j_begin = blockIdx.z * group_frames;
  const int j_end = min(B.n, j_begin + group_frames);

  // a block the workgroup cannot queue (queue full: pathological tile) goes straight to the global table
  int n_direct = 0;   // sf_fuser_alloc_direct_count (added up once per wave at the end: one atomic per call on a single word halved the 1 mm front chain)
  int n_probed = 0;   // look-ups that went to the hash table (the presence cache did not answer): sf_fuser_alloc_probe_count
  auto direct = [&](uint64_t key, int bx, int by, int bz, uint32_t seq) {
    n_direct++;
    if (h.bricks.e != nullptr && brick_known(h.bricks, bx, by, bz)) return;
    n_probed++;
    HashEntry* e = hash_find_or_claim(h, P, key, bx, by, bz, seq);
    if (e) {
      atomicAdd(&counters[C_SLOTS_USED], 1);
      give_block(h, e, key, atomicSub(&counters[C_HEAP_FREE], 1) - 1);
    }
  };

  // ---- phase 2: queued keys -> global hash, all lanes in parallel (callers put a barrier between the last queue write and this; every thread calls it)
  // The heap is popped ONCE per workgroup and call: the entries the lanes claimed are first packed into LDS (their table slots, 4 bytes each, over the keys
  // already read), then one atomic on the heap's free count serves them all.  Popped per wave and iteration -- and the high-water mark raised per lane --
  // the three words every workgroup of the launch shares were what a tile of a newly seen surface waited for: at 1 mm voxels ~1 900 new blocks, 8 iterations,
  // 25 us each; such workgroups (3 % of them) took 200 - 800 us where the mean is 59, and the longest one IS the kernel (profiles/r06_alloc_1mm.txt).
  auto drain = [&]() {
    const int n_unique = min(s_count, LIST);
    uint32_t* const s_ent = reinterpret_cast<uint32_t*>(s_list);
    if (threadIdx.x == 0) s_claimed = 0;
    // DU keys per lane and iteration, their first probes side by side: the table is 16-byte entries scattered over hundreds of megabytes, a look-up is a chain
    // of round trips (the key, the compare-and-swap, the birth frame), and a chain at a time kept a tile of ~4 000 new blocks 13 us per 256 keys
    constexpr int DU = 4;
    for (int i0 = 0; i0 < n_unique; i0 += 256 * DU) {
      uint64_t key[DU], k0[DU];
      uint32_t seq[DU];
      HashEntry* e0[DU];
      HashEntry* claimed[DU];
      bool live[DU], won[DU];
#pragma unroll
      for (int u = 0; u < DU; u++) {
        const int i = i0 + u * 256 + (int)threadIdx.x;
        key[u] = i < n_unique ? s_list[i] : KEY_EMPTY;
        const uint32_t bi = i < n_unique ? s_birth[i] : 0u;   // bit 7: queued by a ray outside the window -- the presence cache has not been asked about this block yet
        seq[u] = B.seq0 + (bi & 0x7Fu);
        live[u] = key[u] != KEY_EMPTY;
        claimed[u] = nullptr;
        int bx, by, bz;
        unpack_key(key[u], bx, by, bz);
        if (live[u] && (bi & 0x80u) != 0u && h.bricks.e != nullptr && brick_known(h.bricks, bx, by, bz)) live[u] = false;   // (the scan queues only what the cache does not know)
        e0[u] = h.table + hash_home(P, bx, by, bz);
        k0[u] = live[u] ? __hip_atomic_load(&e0[u]->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        if (live[u]) n_probed++;
      }
      __syncthreads();   // the keys of this iteration are in registers: the packed entries (never more than the keys read so far, half their size) may grow over them
#pragma unroll
      for (int u = 0; u < DU; u++)   // an empty home slot: try to take it
        won[u] = live[u] && k0[u] == KEY_EMPTY && atomicCAS((unsigned long long*)&e0[u]->key, (unsigned long long)KEY_EMPTY, (unsigned long long)key[u]) == KEY_EMPTY;
#pragma unroll
      for (int u = 0; u < DU; u++) {
        if (!live[u]) continue;
        if (won[u]) { atomicMin(&e0[u]->birth, seq[u]); claimed[u] = e0[u]; }   // taken
        else {   // somebody else's, ours already, or lost the race for it: the general walk from the home slot (one entry it has seen before, rarely)
          int bx, by, bz;
          unpack_key(key[u], bx, by, bz);
          claimed[u] = hash_find_or_claim(h, P, key[u], bx, by, bz, seq[u]);
        }
      }
      uint64_t cm[DU];
      int n_wave = 0;
#pragma unroll
      for (int u = 0; u < DU; u++) { cm[u] = __ballot(claimed[u] != nullptr); n_wave += __popcll((unsigned long long)cm[u]); }
      if (n_wave != 0) {
        int wbase = 0;
        if (lane == 0) wbase = atomicAdd(&s_claimed, n_wave);
        wbase = __builtin_amdgcn_readfirstlane(wbase);
#pragma unroll
        for (int u = 0; u < DU; u++) {
          if (claimed[u] != nullptr) s_ent[wbase + __popcll((unsigned long long)(cm[u] & ((1ull << lane) - 1ull)))] = (uint32_t)(claimed[u] - h.table);
          wbase += __popcll((unsigned long long)cm[u]);
        }
      }
    }
    __syncthreads();
    const int n_claimed = s_claimed;
    if (n_claimed == 0) return;   // (uniform)
    if (threadIdx.x == 0) {
      s_pop_base = atomicSub(&counters[C_HEAP_FREE], n_claimed);
      atomicAdd(&counters[C_SLOTS_USED], n_claimed);
    }
    __syncthreads();
    const int base = s_pop_base;
    int hw = 0;
    for (int i0 = 0; i0 < n_claimed; i0 += 256 * DU) {
      HashEntry* e[DU];
      uint64_t key[DU];
#pragma unroll
      for (int u = 0; u < DU; u++) {
        const int i = i0 + u * 256 + (int)threadIdx.x;
        e[u] = i < n_claimed ? h.table + s_ent[i] : nullptr;
        key[u] = e[u] != nullptr ? __hip_atomic_load(&e[u]->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
      }
#pragma unroll
      for (int u = 0; u < DU; u++)
        if (e[u] != nullptr) hw = max(hw, give_block_quiet(h, e[u], key[u], base - 1 - (i0 + u * 256 + (int)threadIdx.x)));
    }
    for (int o = 32; o > 0; o >>= 1) hw = max(hw, __shfl_xor(hw, o));
    if (lane == 0) raise_high_water(h, hw);
  };

  constexpr int ROUNDS = (WIN_LOG2 >= 6 && !MULTI) ? 8 : 1;   // windows a frame's rays may be walked in before the slow path (below)
  const bool in_image = x < P.W && y < P.H;
  const float kx = ((float)x - P.mx) / P.fx, ky = ((float)y - P.my) / P.fy;  // the pixel's ray direction is the same for every frame
  const float rvoxel = 1.0f / P.voxel;                                        // RN(1 / voxel) for world_to_block
  float d_next = in_image && j_begin < j_end ? depthf_all[(size_t)j_begin * npx + (size_t)(y * P.W + x)] : -INFINITY;
  for (int j = j_begin; j < j_end; ++j) {
    const FrameK& F = B.f[j];  // uniform index: scalar loads from the kernarg segment
    const float d_cur = d_next;
    // the next frame's depth is requested now and lands while this frame's rays are walked
    d_next = in_image && j + 1 < j_end ? depthf_all[(size_t)(j + 1) * npx + (size_t)(y * P.W + x)] : -INFINITY;
    for (int i = threadIdx.x; i < WIN_WORDS; i += 256) s_frame[i] = 0u;
    if (threadIdx.x < sizeof(FrameK) / 4) s_fk[j & 1][threadIdx.x] = reinterpret_cast<const uint32_t*>(&B.f[j])[threadIdx.x];   // per-lane words: vector loads
    const FrameK& FL = *reinterpret_cast<const FrameK*>(s_fk[j & 1]);   // valid behind the barrier below

    // ---- ray set-up
    bool active = false;
    int a_cx = 0, a_cy = 0, a_cz = 0, a_sx = 0, a_sy = 0, a_sz = 0, a_ex = 0, a_ey = 0, a_ez = 0;
    float a_tmx = INFINITY, a_tmy = INFINITY, a_tmz = INFINITY, a_tdx = INFINITY, a_tdy = INFINITY, a_tdz = INFINITY;
    if (in_image) {
      const float d = d_cur;
      if (d != -INFINITY && d < P.maxd) {
        const float t = fmaf(P.tscale, d, P.tbase);
        const float lo = min_f32(P.maxd, d - t);
        const float hi = min_f32(P.maxd, d + t);
        if (lo < hi) {
          float p0[3], p1[3];
          {
            const float ax = kx * lo, ay = ky * lo, az = lo;
#pragma unroll
            for (int r = 0; r < 3; r++) p0[r] = fmaf(F.T[4 * r], ax, fmaf(F.T[4 * r + 1], ay, fmaf(F.T[4 * r + 2], az, F.T[4 * r + 3])));
          }
          {
            const float ax = kx * hi, ay = ky * hi, az = hi;
#pragma unroll
            for (int r = 0; r < 3; r++) p1[r] = fmaf(F.T[4 * r], ax, fmaf(F.T[4 * r + 1], ay, fmaf(F.T[4 * r + 2], az, F.T[4 * r + 3])));
          }
          const float bsize = 8.0f * P.voxel;
          int cur[3], stp[3], bnd[3];
          float tm[3], td[3];
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const float dir = p1[c] - p0[c];
            cur[c] = world_to_block(p0[c], P.voxel, rvoxel);
            const int e = world_to_block(p1[c], P.voxel, rvoxel);
            stp[c] = dir > 0.0f ? 1 : (dir < 0.0f ? -1 : 0);
            bnd[c] = e + stp[c];
            if (stp[c] == 0) { tm[c] = INFINITY; td[c] = INFINITY; }
            else {
              const int nb = cur[c] + (stp[c] > 0 ? 1 : 0);
              const float plane = ((float)(8 * nb) - 0.5f) * P.voxel;
              const float rdir = recip_rn(dir);   // one reciprocal for both quotients
              tm[c] = div_rn(plane - p0[c], dir, rdir);
              td[c] = div_rn((float)stp[c] * bsize, dir, rdir);
            }
          }
          a_cx = cur[0]; a_cy = cur[1]; a_cz = cur[2];
          a_sx = stp[0]; a_sy = stp[1]; a_sz = stp[2]; a_ex = bnd[0]; a_ey = bnd[1]; a_ez = bnd[2];
          a_tmx = tm[0]; a_tmy = tm[1]; a_tmz = tm[2]; a_tdx = td[0]; a_tdy = td[1]; a_tdz = td[2];
          active = true;
        }
      }
    }
    // ROUNDS > 1 (the 64^3 window, one frame per workgroup): rays that leave the window are not taken through the slow path at once -- the window is laid
    // out again around THEM and they walk again, up to ROUNDS times.  A pixel tile on a depth discontinuity has two clusters of rays metres apart; one window
    // holds one of them, and the other's ~5 000 block visits went one by one through a 256-slot LDS set and then the global table (profiles/r06_alloc_1mm.txt:
    // ~35 such tiles per frame set the kernel's duration).  A block two rounds name is queued twice and found the second time: the set is the same.
    bool pending = active;
#pragma unroll 1
    for (int round = 0; round < ROUNDS; ++round) {
      if (round > 0) {   // behind drain()'s barrier: nobody reads the previous round's window any more
        if (threadIdx.x == 0) { s_chooser = 256; s_anchored = 0; }
        if (threadIdx.x < 6) s_box[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
        for (int i = threadIdx.x; i < WIN_WORDS; i += 256) s_frame[i] = 0u;
      }
      __syncthreads();  // s_frame zeroed, previous frame's scan finished
      // The tile's rays stay inside a small region of block space: the first active lane of the first frame that has
      // one anchors the WIN^3 window there for the whole group.
      if (s_anchored == 0) {
        if (pending) atomicMin(&s_chooser, (int)threadIdx.x);
        if (WIN_LOG2 >= 6) {
          // the box around every ray segment of the tile (first and last block per axis): where it fits, the window is centred on it.  Anchored on the first
          // active ray alone (WIN / 4 blocks behind its start), a tile whose other rays start 16 blocks nearer -- 13 cm at 1 mm voxels -- loses those rays
          int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
          if (pending) {
            const int ex = a_ex - a_sx, ey = a_ey - a_sy, ez = a_ez - a_sz;   // the last block of the walk
            lo[0] = min(a_cx, ex); hi[0] = max(a_cx, ex);
            lo[1] = min(a_cy, ey); hi[1] = max(a_cy, ey);
            lo[2] = min(a_cz, ez); hi[2] = max(a_cz, ez);
          }
#pragma unroll
          for (int c = 0; c < 3; c++) {
            for (int o = 32; o > 0; o >>= 1) { lo[c] = min(lo[c], __shfl_xor(lo[c], o)); hi[c] = max(hi[c], __shfl_xor(hi[c], o)); }
            if (lane == 0 && lo[c] <= hi[c]) { atomicMin(&s_box[c], lo[c]); atomicMax(&s_box[3 + c], hi[c]); }
          }
        }
        __syncthreads();
        if ((int)threadIdx.x == s_chooser) {
          // (a multiple of 4 in x: a word of the bitmap is then 8 whole bricks of the presence cache; where the window lies never changes WHAT is allocated)
          int an[3] = {a_cx - (a_sx >= 0 ? WIN / 4 : 3 * WIN / 4), a_cy - (a_sy >= 0 ? WIN / 4 : 3 * WIN / 4), a_cz - (a_sz >= 0 ? WIN / 4 : 3 * WIN / 4)};
          if (WIN_LOG2 >= 6) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
              const int ext = s_box[3 + c] - s_box[c] + 1;
              if (ext <= WIN) an[c] = s_box[c] - (WIN - ext) / 2;   // else: clusters of rays more than a window apart -- the first ray's stays, the rest is the next round's
            }
          }
          s_anchor[0] = an[0] & ~3;
          s_anchor[1] = an[1];
          s_anchor[2] = an[2];
          s_anchored = 1;
        }
        __syncthreads();
      }
      if (ROUNDS > 1 && s_chooser == 256) break;   // uniform: no ray (left) to walk
      const int anx = s_anchor[0], any_ = s_anchor[1], anz = s_anchor[2];

      // ---- DDA: one LDS bit per visited block
      bool left_window = false;
      if (pending) {
        int c_x = a_cx, c_y = a_cy, c_z = a_cz;   // (the ray's start stays: it may walk again)
        float tmx = a_tmx, tmy = a_tmy, tmz = a_tmz;
        uint64_t last_key = KEY_EMPTY;
        for (int it = 0; it < MAX_DDA_ITERS; ++it) {
          const uint32_t ux = (uint32_t)(c_x - anx), uy = (uint32_t)(c_y - any_), uz = (uint32_t)(c_z - anz);
          const bool inwin = (ux | uy | uz) < (uint32_t)WIN;
          const uint32_t bit = inwin ? ((uz << (2 * WIN_LOG2)) | (uy << WIN_LOG2) | ux) : 0xFFFFFFFFu;
          // The 8x8 pixel patch of a wave mostly sits in ONE block: 64 ds_or to the same LDS word serialise.  Drop
          // the lane when its left neighbour (DPP row_shr:1, free) sets the same bit; a disabled or out-of-row
          // neighbour reads as "different" (old value, bound_ctrl off), so run heads always write.
          const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFEu, (int)bit, 0x111, 0xF, 0xF, false);
          if (inwin) {
            if (left != bit) atomicOr(&s_frame[bit >> 5], 1u << (bit & 31));
          } else if (round + 1 < ROUNDS) {
            left_window = true;   // walks again in the next round's window
          } else {
            const uint64_t key = pack_key(c_x, c_y, c_z);
            if (key != last_key) {
              last_key = key;
              if (slab_owns(P, c_x, c_y, c_z) && block_in_frustum(P, FL, c_x, c_y, c_z)) {
                uint32_t sl = ((uint32_t)(key ^ (key >> 21) ^ (key >> 42)) * 2654435761u) >> (32 - SET_LOG2);
                bool placed = false;
                for (int pr = 0; pr < ALLOC_SET_PROBES; ++pr) {
                  const unsigned long long old = atomicCAS(&s_keys[sl], (unsigned long long)KEY_EMPTY, (unsigned long long)key);
                  if (old == key) { placed = true; break; }  // queued by an earlier step / ray / frame
                  if (old == KEY_EMPTY) {
                    const int pos = atomicAdd(&s_count, 1);
                    if (pos < LIST) { s_list[pos] = key; s_birth[pos] = (uint8_t)(j | 0x80); placed = true; }
                    break;  // queue full: direct path below
                  }
                  sl = (sl + 1) & (SET - 1);
                }
                if (!placed) direct(key, c_x, c_y, c_z, B.seq0 + (uint32_t)j);
              }
            }
          }
          bool done;
          if (tmx < tmy && tmx < tmz) { c_x += a_sx; done = (c_x == a_ex); tmx += a_tdx; }
          else if (tmz < tmy) { c_z += a_sz; done = (c_z == a_ez); tmz += a_tdz; }
          else { c_y += a_sy; done = (c_y == a_ey); tmy += a_tdy; }
          if (done) break;
        }
      }
      pending = left_window;
      __syncthreads();
      // ---- scan: blocks this frame visits that no earlier frame of the group queued -> frustum test -> queue
      // A lane takes a WORD (32 x-consecutive blocks) as far as whole words go -- read it, take out what an earlier frame of the group queued and what the presence
      // cache knows -- and a BLOCK from there on: the wave then walks the words that have bits left two at a time, lane b of each half-wave testing block b.
      // (One thread per word all the way -- a loop over the word's bits around the frustum test -- kept a wave as long as the fullest of its 64 words: a tile that looks at
      // a surface for the first time has ~5 500 blocks in ~400 words, a sixth of the lanes busy, and took 200 us here where the mean is 17; the longest workgroup IS
      // the kernel at one frame per launch.  profiles/r06_alloc_1mm.txt)
      for (int base = wave * 64; base < WIN_WORDS; base += 256) {
        const int w = base + lane;
        const uint32_t seen = MULTI ? (s_frame[w] & ~s_done[w]) : s_frame[w];
        uint32_t bits = seen;
        if (bits != 0u && bricks.e != nullptr) {
          // the word's 32 blocks are 8 whole bricks: what the presence cache knows of them is in the table already and older than this batch -- nothing to test,
          // queue or probe for those (and nothing for a later frame of the group either)
          const uint32_t bit0 = (uint32_t)w << 5;
          bits &= ~brick_known_row(bricks, anx + (int)(bit0 & (WIN - 1)), any_ + (int)((bit0 >> WIN_LOG2) & (WIN - 1)), anz + (int)(bit0 >> (2 * WIN_LOG2)));
        }
        uint32_t queued = seen & ~bits;
        uint64_t todo = __ballot(bits != 0u);
        while (todo != 0ull) {   // (uniform)
          const int l0 = __ffsll((unsigned long long)todo) - 1;
          todo &= todo - 1ull;
          const int l1 = todo != 0ull ? __ffsll((unsigned long long)todo) - 1 : l0;
          const bool second = todo != 0ull;
          todo &= todo - 1ull;   // (0 stays 0)
          const int src = lane < 32 ? l0 : l1;
          const uint32_t wbits = (uint32_t)__shfl((int)bits, src);
          const int b = lane & 31;
          const uint32_t wbit0 = (uint32_t)(base + src) << 5;
          const int bx = anx + (int)(wbit0 & (WIN - 1)) + b, by = any_ + (int)((wbit0 >> WIN_LOG2) & (WIN - 1)), bz = anz + (int)(wbit0 >> (2 * WIN_LOG2));
          const bool mine = ((wbits >> b) & 1u) != 0u && (lane < 32 || second);
          const bool foreign = mine && !slab_owns(P, bx, by, bz);   // another GPU's block: never ours, stop looking at it
          const bool pass = mine && !foreign && block_in_frustum(P, FL, bx, by, bz);   // (outside this frame's frustum: a later frame may still want it)
          const uint64_t pm = __ballot(pass);
          if (pm != 0ull) {
            int pos = 0;
            if (lane == 0) pos = atomicAdd(&s_count, __popcll((unsigned long long)pm));
            pos = __builtin_amdgcn_readfirstlane(pos) + __popcll((unsigned long long)(pm & ((1ull << lane) - 1ull)));
            if (pass) {
              if (pos < LIST) { s_list[pos] = pack_key(bx, by, bz); s_birth[pos] = (uint8_t)j; }
              else direct(pack_key(bx, by, bz), bx, by, bz, B.seq0 + (uint32_t)j);
            }
          }
          if (MULTI) {
            const uint64_t qm = __ballot(pass || foreign);
            if (lane == l0) queued |= (uint32_t)qm;
            if (second && lane == l1) queued |= (uint32_t)(qm >> 32);
          }
        }
        if (MULTI && queued) s_done[w] |= queued;  // word w is only ever touched by this lane
      }
      if (ROUNDS > 1) {   // the queue is emptied between rounds
        __syncthreads();
        drain();
        __syncthreads();
        if (threadIdx.x == 0) s_count = 0;
      }
    }
  }
  __syncthreads();
  drain();
  for (int o = 32; o > 0; o >>= 1) { n_direct += __shfl_xor(n_direct, o); n_probed += __shfl_xor(n_probed, o); }
  if (lane == 0 && n_direct) atomicAdd(&counters[C_ALLOC_DIRECT], n_direct);
  if (lane == 0 && n_probed) atomicAdd(&counters[C_ALLOC_PROBED], n_probed);
}

// ---------------------------------------------------------------------------------------------------
// K2r: the same allocation with the occupancy bitmap laid out in RAY SPACE (the default whenever the geometry fits, see alloc_ray in
// sf_fuser_create).  A 16x16 pixel tile looks down a thin pencil of rays: a few blocks wide but as deep as the scene -- and where the tile
// straddles a depth discontinuity (every furniture edge of a real room) its rays sit in two clusters metres apart.  The cube window of
// k_alloc (32^3 blocks = 1 m at 4 mm voxels, anchored at the first ray) covers one cluster; the other fell through to an LDS hash set and,
// when that filled, to one global-table probe PER DDA STEP: measured on the furnished room, 115 us -> 450 us (up to 1.2 ms) per batch.
// Here the window follows the pencil: block (c_a, c_u, c_v) -- a = the axis the tile's centre ray mostly runs along, u, v the other two --
// maps to   k  = +-(c_a - k0)                        slab index along the ray, 0 at the camera, RW_DEPTH = 256 slabs (8 m at 4 mm)
//           du = c_u - (ou + ((su k + fu) >> 12))    lateral offset from the centre ray's block in slab k, RW_LAT = 16 wide
// (dv likewise), bit = k * 256 + dv * 16 + du.  The map is a bijection onto the window for any integers k0, su, ou, ... -- how well the
// centre line is placed only decides how many rays stay inside --, so it is fixed once per workgroup from the group's FIRST frame and the
// "already queued by an earlier frame" bitmap stays valid across the frames of the group.  One slab = 256 bits = 8 words = one thread of the
// workgroup: the scan is two 16-byte LDS reads per thread and frame, and only the ~10 threads whose slab is occupied do anything more.
// Everything else (ray set-up, DDA, frustum test, queue, table probe, heap pop) is k_alloc's, statement for statement: the allocated SET
// and every birth frame are the same (tests/test_gpu_tsdf.py runs both kernels against the oracle).
// ---------------------------------------------------------------------------------------------------
constexpr int RW_LAT_LOG2 = 4, RW_LAT = 1 << RW_LAT_LOG2, RW_DEPTH = 256;
constexpr int RW_WORDS = RW_DEPTH * RW_LAT * RW_LAT / 32;   // 2048 words = 8 KiB per bitmap

// One ray's walk over the blocks of [d - t, d + t] in WINDOW coordinates, for the window axis AXIS (compile time): slab k along the pencil and
// the lateral block coordinates relative to the window origin (ru, rv), so that a step costs an add on one of them instead of the whole map.
// The three-way branch of the reference walk is evaluated as lane masks -- the same comparisons in the same order: x if strictly smallest, else
// z if smaller than y, else y -- so no lane waits for the branches the others take.  This walk only sets bits; it returns true when the ray left
// the window (rare: the map follows the camera), and the caller walks such a ray AGAIN for the blocks outside.
struct RayWalk {
  int cx, cy, cz, sx, sy, sz, ex, ey, ez;      // first block, step and one-past-the-last block per axis
  float tmx, tmy, tmz, tdx, tdy, tdz;          // parameter of the next block face / per block, per axis
};
struct WindowMap {
  int k0, sgn, su, ou, fu, sv, ov, fv;
};
template <int AXIS>
__device__ inline bool ray_walk_bits(const RayWalk& r, const WindowMap& w, uint32_t* s_frame) {
  // (a, u, v) = (AXIS, AXIS + 1, AXIS + 2) mod 3
  const int c_a = AXIS == 0 ? r.cx : (AXIS == 1 ? r.cy : r.cz), c_u = AXIS == 0 ? r.cy : (AXIS == 1 ? r.cz : r.cx), c_v = AXIS == 0 ? r.cz : (AXIS == 1 ? r.cx : r.cy);
  const int s_a = AXIS == 0 ? r.sx : (AXIS == 1 ? r.sy : r.sz), s_u = AXIS == 0 ? r.sy : (AXIS == 1 ? r.sz : r.sx), s_v = AXIS == 0 ? r.sz : (AXIS == 1 ? r.sx : r.sy);
  const int e_a = AXIS == 0 ? r.ex : (AXIS == 1 ? r.ey : r.ez), e_u = AXIS == 0 ? r.ey : (AXIS == 1 ? r.ez : r.ex), e_v = AXIS == 0 ? r.ez : (AXIS == 1 ? r.ex : r.ey);
  int k = w.sgn > 0 ? c_a - w.k0 : w.k0 - c_a;
  const int k_end = w.sgn > 0 ? e_a - w.k0 : w.k0 - e_a;
  const int dk = w.sgn > 0 ? s_a : -s_a;
  int ru = c_u - w.ou, rv = c_v - w.ov;
  const int ru_end = e_u - w.ou, rv_end = e_v - w.ov;
  float tmx = r.tmx, tmy = r.tmy, tmz = r.tmz;
  bool left_window = false;
  for (int it = 0; it < MAX_DDA_ITERS; ++it) {
    // (a slab index far outside the window only has to fail the range test: the 24-bit product may be anything there)
    const uint32_t du = (uint32_t)(ru - ((__mul24(w.su, k) + w.fu) >> 12));
    const uint32_t dv = (uint32_t)(rv - ((__mul24(w.sv, k) + w.fv) >> 12));
    const bool inwin = (uint32_t)k < (uint32_t)RW_DEPTH && (du | dv) < (uint32_t)RW_LAT;
    const uint32_t bit = inwin ? (((uint32_t)k << (2 * RW_LAT_LOG2)) | (dv << RW_LAT_LOG2) | du) : 0xFFFFFFFFu;
    // lanes whose left neighbour (DPP row_shr:1) sets the same bit stay silent: 64 same-address ds_or serialise (see k_alloc)
    const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFEu, (int)bit, 0x111, 0xF, 0xF, false);
    if (inwin && left != bit) atomicOr(&s_frame[bit >> 5], 1u << (bit & 31));
    left_window = left_window || !inwin;
    const bool go_x = tmx < tmy && tmx < tmz;
    const bool go_z = !go_x && tmz < tmy;
    const bool go_y = !go_x && !go_z;
    tmx += go_x ? r.tdx : 0.0f;   // x + 0 = x: the axes not taken keep their value bit for bit
    tmy += go_y ? r.tdy : 0.0f;
    tmz += go_z ? r.tdz : 0.0f;
    const bool go_a = AXIS == 0 ? go_x : (AXIS == 1 ? go_y : go_z);
    const bool go_u = AXIS == 0 ? go_y : (AXIS == 1 ? go_z : go_x);
    k += go_a ? dk : 0;
    ru += go_u ? s_u : 0;
    rv += (!go_a && !go_u) ? s_v : 0;
    // "the coordinate that moved reached its end" as two selects and ONE compare: written as a nested conditional of three compares the compiler built it out of
    // nested exec-mask regions (three s_and_saveexec / s_cbranch_execz pairs per step of the hot walk)
    const int moved = go_a ? k : (go_u ? ru : rv);
    const int moved_end = go_a ? k_end : (go_u ? ru_end : rv_end);
    if (moved == moved_end) break;
  }
  return left_window;
}

template <bool MULTI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_alloc_ray(const float* __restrict__ depthf_all, HashEntry* table, int32_t* heap,
                                                   uint64_t* block_keys, int32_t* block_entry, uint8_t* block_flags, int32_t* counters, ParamsK P,
                                                   BatchFrames B, int group_frames, const uint16_t* __restrict__ fuse_depth16,
                                                   float* depthf_out, int compact_counter) {
  // fuse_depth16 != nullptr (one frame per pass, no colour, no resampling: a live stream): the kernel is ALSO the depth pre-pass -- every lane
  // converts its own pixel (k_prepass's arithmetic), stores it for the integrate kernel's gathers and walks it; one launch and one
  // dependency hop less in a chain of four that is the whole frame time
  __shared__ uint4 s_frame4[RW_WORDS / 4];              // blocks the current frame's rays visit (slab-major)
  __shared__ uint4 s_done4[MULTI ? RW_WORDS / 4 : 1];   // blocks an earlier frame of the group has already queued
  __shared__ unsigned long long s_keys[ALLOC_SET];      // the same for blocks outside the window
  __shared__ unsigned long long s_list[ALLOC_LIST];     // queue for phase 2
  __shared__ uint8_t s_birth[ALLOC_LIST];               // ... and the frame (index in the batch) that queued the key
  __shared__ int s_count;
  uint32_t* const s_frame = reinterpret_cast<uint32_t*>(s_frame4);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_count = 0;
  const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  // No presence cache here (fuser_internal.h BrickCache: the cube window's kernels use it): the "already queued" bitmap of the ray-space window leaves this kernel
  // few look-ups to save -- 34.7 k against 34.8 k frames/s on the long stream with the cache on / off -- and its code, even switched off at run time, cost a 20-frame
  // call into an empty volume 2 % (35.1 k -> 34.3 k, five libraries on one box: profiles/r06_alloc_1mm.txt).  The cache stays right: it only ever holds blocks the cube
  // kernels FOUND in the table, and whatever takes blocks out of the table clears it.
  const HashRefs h{table, heap, block_keys, block_entry, block_flags, counters, BrickCache{nullptr, 0u}, B.seq0};
  for (int i = threadIdx.x; i < ALLOC_SET; i += 256) s_keys[i] = KEY_EMPTY;
  for (int i = threadIdx.x; i < RW_WORDS / 4; i += 256) s_frame4[i] = make_uint4(0, 0, 0, 0);
  if (MULTI)
    for (int i = threadIdx.x; i < RW_WORDS / 4; i += 256) s_done4[i] = make_uint4(0, 0, 0, 0);
  const size_t npx = (size_t)P.W * P.H;
  const int j_begin = blockIdx.z * group_frames;
  const int j_end = min(B.n, j_begin + group_frames);

  int n_direct = 0;   // sf_fuser_alloc_direct_count (added up once per wave at the end: one atomic per call on a single word halved the 1 mm front chain)
  auto direct = [&](uint64_t key, int bx, int by, int bz, uint32_t seq) {
    n_direct++;
    HashEntry* e = hash_find_or_claim(h, P, key, bx, by, bz, seq);
    if (e) {
      atomicAdd(&counters[C_SLOTS_USED], 1);
      give_block(h, e, key, atomicSub(&counters[C_HEAP_FREE], 1) - 1);
    }
  };

  // ---- the window map (uniform: every thread computes the same numbers), laid along the MEAN of the tile's centre rays in frames ja and jb --
  // the first and the last frame it will serve: a camera that turns during the pass sweeps the pencil sideways (0.2 degrees per frame in the
  // bench walk's corners = 7 blocks at 4 m over 16 frames), and rays that leave the window take the slow path (an LDS hash set, then one
  // global-table probe per step: the workgroups of such tiles ran 3x longer than the rest and set the kernel's duration)
  int w_axis = 0, w_k0 = 0, w_sgn = 1, w_su = 0, w_ou = 0, w_fu = 0, w_sv = 0, w_ov = 0, w_fv = 0;
  const float bs = 8.0f * P.voxel;
  const float kxc = (((float)(blockIdx.x * 16) + 7.5f) - P.mx) / P.fx, kyc = (((float)(blockIdx.y * 16) + 7.5f) - P.my) / P.fy;
  auto centre_ray = [&](int j, float (&dir)[3], float (&org)[3]) {
    const FrameK& Fj = B.f[min(max(j, 0), MAX_BATCH - 1)];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      dir[r] = Fj.T[4 * r] * kxc + Fj.T[4 * r + 1] * kyc + Fj.T[4 * r + 2];   // camera-space z component 1: dir * z = the point at depth z
      org[r] = Fj.T[4 * r + 3] / bs;                                         // camera centre in block units
    }
  };
  auto anchor = [&](int ja, int jb) {
    float da_[3], oa_[3], db_[3], ob_[3], dir[3], org[3];
    centre_ray(ja, da_, oa_);
    centre_ray(jb, db_, ob_);
#pragma unroll
    for (int r = 0; r < 3; r++) { dir[r] = 0.5f * (da_[r] + db_[r]); org[r] = 0.5f * (oa_[r] + ob_[r]); }
    const float ax = fabsf(dir[0]), ay = fabsf(dir[1]), az = fabsf(dir[2]);
    int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const float da = axis == 0 ? dir[0] : (axis == 1 ? dir[1] : dir[2]);
    const float oa = axis == 0 ? org[0] : (axis == 1 ? org[1] : org[2]);
    const float du_ = axis == 0 ? dir[1] : (axis == 1 ? dir[2] : dir[0]);   // u = (a + 1) % 3, v = (a + 2) % 3
    const float dv_ = axis == 0 ? dir[2] : (axis == 1 ? dir[0] : dir[1]);
    const float ou_ = axis == 0 ? org[1] : (axis == 1 ? org[2] : org[0]);
    const float ov_ = axis == 0 ? org[2] : (axis == 1 ? org[0] : org[1]);
    int sgn = da < 0.0f ? -1 : 1;
    const int cb = (int)floorf(oa);
    int k0 = cb - sgn;                                 // slab 1 holds the camera, slab 0 is one block of margin behind it
    const float inv = da != 0.0f ? 1.0f / da : 0.0f;
    const float slu = du_ * inv * (float)sgn, slv = dv_ * inv * (float)sgn;   // lateral blocks per slab, |.| <= 1
    // lateral position of the centre line at the middle of slab 0 (block units), minus half the window
    const float a0 = ((float)k0 + 0.5f) - oa;
    const float iu = ou_ + du_ * inv * a0 - (float)(RW_LAT / 2), iv = ov_ + dv_ * inv * a0 - (float)(RW_LAT / 2);
    const float fiu = floorf(iu), fiv = floorf(iv);
    w_axis = __builtin_amdgcn_readfirstlane(axis); w_k0 = __builtin_amdgcn_readfirstlane(k0); w_sgn = __builtin_amdgcn_readfirstlane(sgn);
    w_su = __builtin_amdgcn_readfirstlane((int)rintf(slu * 4096.0f)); w_ou = __builtin_amdgcn_readfirstlane((int)fiu);
    w_fu = __builtin_amdgcn_readfirstlane((int)((iu - fiu) * 4096.0f));
    w_sv = __builtin_amdgcn_readfirstlane((int)rintf(slv * 4096.0f)); w_ov = __builtin_amdgcn_readfirstlane((int)fiv);
    w_fv = __builtin_amdgcn_readfirstlane((int)((iv - fiv) * 4096.0f));
  };
  // How many consecutive frames one map can serve: the tile's centre point at the integration distance moves D blocks between the group's
  // first and last frame; anchored on the mean, a map holds a sweep of ~9 blocks (window +-8, half a tile's width and the block rounding
  // off).  A faster camera gets a fresh map -- and a cleared "already queued" bitmap, which only costs repeated look-ups -- every n_map frames.
  int n_map = max(1, j_end - j_begin);
  if (MULTI && j_end - j_begin > 1) {
    float d0[3], o0[3], d1[3], o1[3];
    centre_ray(j_begin, d0, o0);
    centre_ray(j_end - 1, d1, o1);
    const float far = P.maxd / bs;
    float D = 0.0f;
#pragma unroll
    for (int r = 0; r < 3; r++) D = fmaxf(D, fabsf((o1[r] + d1[r] * far) - (o0[r] + d0[r] * far)));
    if (D > 9.0f) n_map = max(1, (int)((float)(j_end - j_begin) * 9.0f / D));
    n_map = __builtin_amdgcn_readfirstlane(n_map);
  }
  int next_map = j_begin;
  const bool in_image = x < P.W && y < P.H;
  const float kx = ((float)x - P.mx) / P.fx, ky = ((float)y - P.my) / P.fy;  // the pixel's ray direction is the same for every frame
  const float rvoxel = 1.0f / P.voxel;                                        // RN(1 / voxel) for world_to_block
  float d_next;
  if (fuse_depth16 != nullptr) {   // uniform
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicExch(reinterpret_cast<unsigned long long*>(&counters[compact_counter]), 0ull);
    d_next = -INFINITY;
    if (in_image) {
      const uint16_t u = fuse_depth16[(size_t)(y * P.W + x)];
      float v = (float)u / P.depth_shift;
      if (u == 0 || v < P.dmin || v > P.dmax || !(v < P.maxd)) v = -INFINITY;   // k_prepass's gates, the integration distance included
      depthf_out[(size_t)(y * P.W + x)] = v;
      d_next = v;
    }
  } else {
    d_next = in_image && j_begin < j_end ? depthf_all[(size_t)j_begin * npx + (size_t)(y * P.W + x)] : -INFINITY;
  }
  __syncthreads();   // bitmaps zeroed
  for (int j = j_begin; j < j_end; ++j) {
    const FrameK& F = B.f[j];  // uniform index: scalar loads from the kernarg segment
    const float d_cur = d_next;
    d_next = in_image && j + 1 < j_end ? depthf_all[(size_t)(j + 1) * npx + (size_t)(y * P.W + x)] : -INFINITY;
    if (j == next_map) {   // uniform
      anchor(j, min(j + n_map, j_end) - 1);
      next_map = j + n_map;
      if (MULTI && j != j_begin)   // the queued-blocks bitmap was laid out by the old map (read again only behind the next barrier)
        for (int i = threadIdx.x; i < RW_WORDS / 4; i += 256) s_done4[i] = make_uint4(0, 0, 0, 0);
    }

    // ---- ray set-up (k_alloc's, statement for statement)
    bool active = false;
    int a_cx = 0, a_cy = 0, a_cz = 0, a_sx = 0, a_sy = 0, a_sz = 0, a_ex = 0, a_ey = 0, a_ez = 0;
    float a_tmx = INFINITY, a_tmy = INFINITY, a_tmz = INFINITY, a_tdx = INFINITY, a_tdy = INFINITY, a_tdz = INFINITY;
    if (in_image) {
      const float d = d_cur;
      if (d != -INFINITY && d < P.maxd) {
        const float t = fmaf(P.tscale, d, P.tbase);
        const float lo = min_f32(P.maxd, d - t);
        const float hi = min_f32(P.maxd, d + t);
        if (lo < hi) {
          float p0[3], p1[3];
          {
            const float ax = kx * lo, ay = ky * lo, az = lo;
#pragma unroll
            for (int r = 0; r < 3; r++) p0[r] = fmaf(F.T[4 * r], ax, fmaf(F.T[4 * r + 1], ay, fmaf(F.T[4 * r + 2], az, F.T[4 * r + 3])));
          }
          {
            const float ax = kx * hi, ay = ky * hi, az = hi;
#pragma unroll
            for (int r = 0; r < 3; r++) p1[r] = fmaf(F.T[4 * r], ax, fmaf(F.T[4 * r + 1], ay, fmaf(F.T[4 * r + 2], az, F.T[4 * r + 3])));
          }
          const float bsize = 8.0f * P.voxel;
          int cur[3], stp[3], bnd[3];
          float tm[3], td[3];
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const float dir = p1[c] - p0[c];
            cur[c] = world_to_block(p0[c], P.voxel, rvoxel);
            const int e = world_to_block(p1[c], P.voxel, rvoxel);
            stp[c] = dir > 0.0f ? 1 : (dir < 0.0f ? -1 : 0);
            bnd[c] = e + stp[c];
            if (stp[c] == 0) { tm[c] = INFINITY; td[c] = INFINITY; }
            else {
              const int nb = cur[c] + (stp[c] > 0 ? 1 : 0);
              const float plane = ((float)(8 * nb) - 0.5f) * P.voxel;
              const float rdir = recip_rn(dir);   // one reciprocal for both quotients
              tm[c] = div_rn(plane - p0[c], dir, rdir);
              td[c] = div_rn((float)stp[c] * bsize, dir, rdir);
            }
          }
          a_cx = cur[0]; a_cy = cur[1]; a_cz = cur[2];
          a_sx = stp[0]; a_sy = stp[1]; a_sz = stp[2]; a_ex = bnd[0]; a_ey = bnd[1]; a_ez = bnd[2];
          a_tmx = tm[0]; a_tmy = tm[1]; a_tmz = tm[2]; a_tdx = td[0]; a_tdy = td[1]; a_tdz = td[2];
          active = true;
        }
      }
    }

    // ---- DDA: one LDS bit per visited block.  The walk runs in WINDOW coordinates: slab k along the pencil and the lateral block
    // coordinates relative to the window origin (ru, rv), so that a step costs an add on one of them instead of the whole map -- and the
    // three-way branch of the reference walk is evaluated as three lane masks (the same comparisons in the same order: x if strictly
    // smallest, else z if smaller than y, else y), so no lane waits for the branches the others take.
    if (active) {
      // The axis the window runs along is the same for every lane of the workgroup (a scalar): the hot walk is compiled THREE times, once per
      // axis, and chosen by a scalar branch -- inside each copy "the window axis" is a compile-time name for one of x / y / z, so a step's
      // "which coordinate moves" is the very lane mask its comparison produced.  (With w_axis as a run-time select on the three masks the
      // compiler materialised them into registers and picked among them with vector selects: 11 of the 48 vector instructions of a step.)
      const RayWalk rw{a_cx, a_cy, a_cz, a_sx, a_sy, a_sz, a_ex, a_ey, a_ez, a_tmx, a_tmy, a_tmz, a_tdx, a_tdy, a_tdz};
      const WindowMap wm{w_k0, w_sgn, w_su, w_ou, w_fu, w_sv, w_ov, w_fv};
      bool left_window;
      if (w_axis == 0) left_window = ray_walk_bits<0>(rw, wm, s_frame);
      else if (w_axis == 1) left_window = ray_walk_bits<1>(rw, wm, s_frame);
      else left_window = ray_walk_bits<2>(rw, wm, s_frame);
      if (left_window) {   // the same walk once more (one copy, the axis a run-time value), this time for the blocks OUTSIDE the window: LDS hash set, then the global table
        const int c_a = w_axis == 0 ? a_cx : (w_axis == 1 ? a_cy : a_cz), c_u = w_axis == 0 ? a_cy : (w_axis == 1 ? a_cz : a_cx), c_v = w_axis == 0 ? a_cz : (w_axis == 1 ? a_cx : a_cy);
        const int s_a = w_axis == 0 ? a_sx : (w_axis == 1 ? a_sy : a_sz), s_u = w_axis == 0 ? a_sy : (w_axis == 1 ? a_sz : a_sx), s_v = w_axis == 0 ? a_sz : (w_axis == 1 ? a_sx : a_sy);
        const int e_a = w_axis == 0 ? a_ex : (w_axis == 1 ? a_ey : a_ez), e_u = w_axis == 0 ? a_ey : (w_axis == 1 ? a_ez : a_ex), e_v = w_axis == 0 ? a_ez : (w_axis == 1 ? a_ex : a_ey);
        int k = w_sgn > 0 ? c_a - w_k0 : w_k0 - c_a;
        const int k_end = w_sgn > 0 ? e_a - w_k0 : w_k0 - e_a;
        const int dk = w_sgn > 0 ? s_a : -s_a;
        int ru = c_u - w_ou, rv = c_v - w_ov;
        const int ru_end = e_u - w_ou, rv_end = e_v - w_ov;
        uint64_t last_key = KEY_EMPTY;
#pragma unroll 1
        for (int it = 0; it < MAX_DDA_ITERS; ++it) {
          const uint32_t du = (uint32_t)(ru - ((__mul24(w_su, k) + w_fu) >> 12));
          const uint32_t dv = (uint32_t)(rv - ((__mul24(w_sv, k) + w_fv) >> 12));
          const bool inwin = (uint32_t)k < (uint32_t)RW_DEPTH && (du | dv) < (uint32_t)RW_LAT;
          if (!inwin) {
            const int ca = w_sgn > 0 ? w_k0 + k : w_k0 - k, cu = ru + w_ou, cv = rv + w_ov;
            const int cx = w_axis == 0 ? ca : (w_axis == 1 ? cv : cu), cy = w_axis == 0 ? cu : (w_axis == 1 ? ca : cv), cz = w_axis == 0 ? cv : (w_axis == 1 ? cu : ca);
            const uint64_t key = pack_key(cx, cy, cz);
            if (key != last_key) {
              last_key = key;
              if (slab_owns(P, cx, cy, cz) && block_in_frustum(P, F, cx, cy, cz)) {
                uint32_t sl = ((uint32_t)(key ^ (key >> 21) ^ (key >> 42)) * 2654435761u) >> 24;  // 8 bits
                bool placed = false;
#pragma unroll 1
                for (int pr = 0; pr < ALLOC_SET_PROBES; ++pr) {
                  const unsigned long long old = atomicCAS(&s_keys[sl], (unsigned long long)KEY_EMPTY, (unsigned long long)key);
                  if (old == key) { placed = true; break; }  // queued by an earlier step / ray / frame
                  if (old == KEY_EMPTY) {
                    const int pos = atomicAdd(&s_count, 1);
                    if (pos < ALLOC_LIST) { s_list[pos] = key; s_birth[pos] = (uint8_t)j; placed = true; }
                    break;  // queue full: direct path below
                  }
                  sl = (sl + 1) & (ALLOC_SET - 1);
                }
                if (!placed) direct(key, cx, cy, cz, B.seq0 + (uint32_t)j);
              }
            }
          }
          const bool go_x = a_tmx < a_tmy && a_tmx < a_tmz;
          const bool go_z = !go_x && a_tmz < a_tmy;
          const bool go_y = !go_x && !go_z;
          a_tmx += go_x ? a_tdx : 0.0f;
          a_tmy += go_y ? a_tdy : 0.0f;
          a_tmz += go_z ? a_tdz : 0.0f;
          const bool go_a = w_axis == 0 ? go_x : (w_axis == 1 ? go_y : go_z);
          const bool go_u = w_axis == 0 ? go_y : (w_axis == 1 ? go_z : go_x);
          k += go_a ? dk : 0;
          ru += go_u ? s_u : 0;
          rv += (!go_a && !go_u) ? s_v : 0;
          const bool done = go_a ? k == k_end : (go_u ? ru == ru_end : rv == rv_end);
          if (done) break;
        }
      }
    }
    __syncthreads();
    // ---- scan: thread t owns slab t (8 words): blocks this frame visits that no earlier frame of the group queued -> frustum test -> queue
    const int k = (int)threadIdx.x;
    const uint4 f0 = s_frame4[2 * k], f1 = s_frame4[2 * k + 1];
    bool occupied = (f0.x | f0.y | f0.z | f0.w | f1.x | f1.y | f1.z | f1.w) != 0u;   // ~10 threads of the workgroup
    if (MULTI && occupied) {
      // the usual case inside a pass: everything this frame visits in the slab was queued by an earlier frame -- two more reads say so, and
      // the slab is cleared for the next frame without walking its words
      const uint4 d0 = s_done4[2 * k], d1 = s_done4[2 * k + 1];
      if (((f0.x & ~d0.x) | (f0.y & ~d0.y) | (f0.z & ~d0.z) | (f0.w & ~d0.w) | (f1.x & ~d1.x) | (f1.y & ~d1.y) | (f1.z & ~d1.z) | (f1.w & ~d1.w)) == 0u) {
        s_frame4[2 * k] = make_uint4(0, 0, 0, 0);
        s_frame4[2 * k + 1] = make_uint4(0, 0, 0, 0);
        occupied = false;
      }
    }
    if (occupied) {
      uint32_t* const s_done = reinterpret_cast<uint32_t*>(s_done4);
      const int ca = w_sgn > 0 ? w_k0 + k : w_k0 - k;
      const int cu0 = w_ou + ((w_su * k + w_fu) >> 12), cv0 = w_ov + ((w_sv * k + w_fv) >> 12);
#pragma unroll 1
      for (int w = 0; w < 8; w++) {   // the words come from LDS again: a register array indexed by w would live in scratch
        const uint32_t fw = s_frame[8 * k + w];
        if (fw == 0u) continue;
        s_frame[8 * k + w] = 0u;      // ready for the next frame (nobody else touches this slab before the next barrier)
        const uint32_t dw = MULTI ? s_done[8 * k + w] : 0u;
        uint32_t bits = fw & ~dw, queued = 0u;
        while (bits) {
          const int b = __ffs((int)bits) - 1;
          bits &= bits - 1u;
          const int idx = w * 32 + b;
          const int cu = cu0 + (idx & (RW_LAT - 1)), cv = cv0 + (idx >> RW_LAT_LOG2);
          const int bx = w_axis == 0 ? ca : (w_axis == 1 ? cv : cu);
          const int by = w_axis == 0 ? cu : (w_axis == 1 ? ca : cv);
          const int bz = w_axis == 0 ? cv : (w_axis == 1 ? cu : ca);
          if (!slab_owns(P, bx, by, bz)) { queued |= 1u << b; continue; }  // another GPU's block: never ours, stop looking at it
          if (!block_in_frustum(P, F, bx, by, bz)) continue;  // a later frame may still want it
          queued |= 1u << b;
          const int pos = atomicAdd(&s_count, 1);
          if (pos < ALLOC_LIST) { s_list[pos] = pack_key(bx, by, bz); s_birth[pos] = (uint8_t)j; }
          else direct(pack_key(bx, by, bz), bx, by, bz, B.seq0 + (uint32_t)j);
        }
        if (MULTI && queued) s_done[8 * k + w] = dw | queued;
      }
    }
    __syncthreads();   // slabs re-zeroed before the next frame's rays set bits
  }

  // ---- phase 2: queued keys -> global hash, all lanes in parallel (k_alloc's)
  const int n_unique = min(s_count, ALLOC_LIST);
  for (int i0 = 0; i0 < n_unique; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const uint64_t key = i < n_unique ? s_list[i] : KEY_EMPTY;
    HashEntry* claimed = nullptr;
    if (key != KEY_EMPTY) {
      int bx, by, bz;
      unpack_key(key, bx, by, bz);
      claimed = hash_find_or_claim(h, P, key, bx, by, bz, B.seq0 + (uint32_t)s_birth[i]);
    }
    const uint64_t cm = __ballot(claimed != nullptr);
    if (cm != 0ull) {
      const int n = __popcll((unsigned long long)cm);
      const int first = __ffsll((unsigned long long)cm) - 1;
      int base = 0;
      if (lane == first) {
        base = atomicSub(&counters[C_HEAP_FREE], n);
        atomicAdd(&counters[C_SLOTS_USED], n);
      }
      base = __shfl(base, first);
      int hw = 0;
      if (claimed != nullptr) {
        const int rank = __popcll((unsigned long long)(cm & ((1ull << lane) - 1ull)));
        hw = give_block_quiet(h, claimed, key, base - 1 - rank);
      }
      for (int o = 32; o > 0; o >>= 1) hw = max(hw, __shfl_xor(hw, o));   // the high-water mark once per wave, not per lane
      if (lane == first) raise_high_water(h, hw);
    }
  }
  for (int o = 32; o > 0; o >>= 1) n_direct += __shfl_xor(n_direct, o);
  if (lane == 0 && n_direct) atomicAdd(&counters[C_ALLOC_DIRECT], n_direct);
}

template <int WIN_LOG2, bool MULTI>
void launch_alloc(const sf_fuser* f, int sl, dim3 grid, const BatchFrames& bf, int gf, hipStream_t s) {
  const BrickCache bc{f->brick_on ? f->bricks : nullptr, f->brick_lines - 1u};
  hipLaunchKernelGGL((k_alloc<WIN_LOG2, MULTI>), grid, dim3(256), 0, s, f->depthf2[sl], f->table, f->heap, f->block_keys, f->block_entry, f->block_flags,
                     f->counters, f->pk, bf, gf, bc);
}

template <bool MULTI>
void launch_alloc_ray(const sf_fuser* f, int sl, dim3 grid, const BatchFrames& bf, int gf, const uint16_t* raw_depth, hipStream_t s) {
  hipLaunchKernelGGL((k_alloc_ray<MULTI>), grid, dim3(256), 0, s, f->depthf2[sl], f->table, f->heap, f->block_keys, f->block_entry, f->block_flags,
                     f->counters, f->pk, bf, gf, raw_depth, f->depthf2[sl], sf_compact_counter(sl));
}

}  // namespace

void sf_alloc_choose_window(sf_fuser* f, const sf_params* p) {
  // longest ray segment 2 * trunc(max distance) in blocks decides the LDS window size of k_alloc
  const float seg = 2.0f * (p->trunc_base + p->trunc_scale * p->max_integration_dist) / (8.0f * p->voxel_size);
  f->alloc_win64 = seg > 20.0f;
  // the ray-space window (k_alloc_ray) holds the pencil of a 16x16 pixel tile when 16 blocks span its width plus a few blocks of camera
  // motion inside a batch, and 256 slabs its depth: half a tile at the integration distance within 4 blocks, the longest ray within 250
  const float bsz = 8.0f * p->voxel_size;
  const float half_tile = 8.0f * p->max_integration_dist / std::min(p->fx, p->fy);
  const float reach = (p->max_integration_dist + p->trunc_base + p->trunc_scale * p->max_integration_dist) * 1.25f;
  f->alloc_ray = half_tile / bsz <= 4.0f && reach / bsz <= (float)(RW_DEPTH - 6);
}

void sf_launch_alloc(const sf_fuser* f, int sl, int n, const BatchFrames& bf, const BatchIn& in, hipStream_t s, bool fuse_pre) {
  // frames one allocation workgroup walks.  The FIRST pass of a batch call has nothing to run beside: its front chain is pure latency in front of the first
  // integrate launch (a 20-frame call: k_alloc_ray 133 us of a 650 us region at 8 frames per workgroup), so it is cut into more, shorter workgroups of at most
  // 4 frames (a 20-frame call: 30.8 k -> 31.8 k frames/s); every other pass hides its allocation behind the previous integrate launch and takes the cheaper,
  // longer ones.  The cube window's WIN 64 (32 KiB bitmap) has no room for the second bitmap: one frame per workgroup there.
  const int group = f->head_pass ? std::min(f->alloc_group, 4) : f->alloc_group;
  const bool win64 = f->alloc_win64 && !f->alloc_ray;
  const int gf = win64 ? 1 : std::min(group, n);
  const dim3 ag((f->p.depth_width + 15) / 16, (f->p.depth_height + 15) / 16, (n + gf - 1) / gf);
  if (f->alloc_ray) {
    const uint16_t* raw_depth = fuse_pre ? in.depth[0] : nullptr;   // one colourless frame at the integration size: k_alloc_ray converts the depth itself
    if (gf == 1) launch_alloc_ray<false>(f, sl, ag, bf, gf, raw_depth, s);
    else launch_alloc_ray<true>(f, sl, ag, bf, gf, raw_depth, s);
  }
  else if (win64) launch_alloc<6, false>(f, sl, ag, bf, gf, s);
  else if (gf == 1) launch_alloc<5, false>(f, sl, ag, bf, gf, s);
  else launch_alloc<5, true>(f, sl, ag, bf, gf, s);
}
