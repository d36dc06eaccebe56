// fuser_compact.hip -- stage 3 of a fusion pass: compaction of the block directory into the pass's list of tiles and frame masks; the same kernel
// lists every live block for export, garbage collection and meshing (sf_compact_live).
#include <hip/hip_runtime.h>

#include <cstring>

#include "fuser_device.h"
#include "fuser_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// K3: compactify.  Scans the block directory (8 B per heap slot up to the high-water mark -- not the
// 16 B x buckets x 10 hash table upstream scans) and appends the slots of the blocks that at least one
// frame of the batch updates, together with the bit mask of those frames: bit j is set iff the block is in
// frame j's frustum AND was born no later than frame j.  1024 directory entries per workgroup, ballot
// prefix sums inside the waves, one LDS exchange and TWO global atomics per workgroup (list position +
// last-frame count in one 64-bit word, the N_blk total in another cache line; a single counter word
// saturates at ~88 atomics/us on this chip).  all_live = 1 lists every live block (export), 2 every live block this
// fuser owns (GC, meshing); ghost copies of a neighbour slab's blocks are never fused.
// ---------------------------------------------------------------------------------------------------
// The frustum tests of a batch are (directory entry) x (frame) independent tests of ~25 instructions.  Until round 5 every lane ran the B.n tests of its four
// entries one after the other with the frame's constants re-read from the kernarg segment per test: 62-105 us per pass at 2 % of the vector ALUs' issue rate
// (1 600 waves in flight, each a serial chain of 128 scalar-load round trips).  Now, for batches of more than FEW frames, a lane IS a (entry, frame) pair:
// lane = sub * FPL + q holds frame q's constants in registers for the life of the workgroup (FPL = 8 / 16 / 32 frames per lane group), the workgroup's 1024
// block coordinates wait in LDS, and one step tests 64 / FPL entries against all frames at once -- the ballot of the step IS the entries' frame masks.
// Same function (block_in_frustum), same operands: the masks are the ones the serial loop produced.
constexpr int COMPACT_FEW = 4;   // up to this many frames per pass the serial loop stays (a live stream's one frame per pass would leave 31 of 32 lanes idle)

// ONE by-value argument, so that the frames' constants sit at a known offset of the kernarg segment: the workgroup copies them into LDS with one round of
// vector loads (all in flight together).  Read as `B.f[q]` they arrive through the scalar unit, a few cache lines per frame, each a separate round trip
// the wave waits for: the chain of ~80 such loads per workgroup, not the tests, was what the kernel's 56-62 us consisted of (0.9 M wave instructions, 2 %
// of the issue rate; profiles/r06_compactify.txt).
struct CompactArgs {
  const uint64_t* block_keys;
  const int32_t* block_entry;
  const uint8_t* block_flags;
  const HashEntry* table;
  int32_t* compact;
  uint32_t* cmask;
  int32_t* counters;
  int counter_id, all_live;
  ParamsK P;
  BatchFrames B;
};
constexpr int FRAMEK_WORDS = (int)(sizeof(FrameK) / 4);

// One thread per directory entry, COMPACT_THREADS entries per workgroup: a wave tests its 64 entries against all frames in 32 steps of ~300 dependent cycles.
// (Four entries per thread -- 128 steps per wave -- left the kernel at the length of that one chain: 52-62 us for 1.4 M wave instructions.  1024 threads per
// workgroup took the chain to 20 us ALONE but 170 us beside the integrate pass: a workgroup of 16 waves of 90 registers needs a whole CU to itself, and the
// integrate kernel's waves hold 480 of a SIMD's 512 registers -- a workgroup of 4 waves finds a home as soon as one wave per SIMD retires:
// profiles/r06_compactify.txt.)
constexpr int COMPACT_THREADS = 256;
constexpr int COMPACT_WAVES = COMPACT_THREADS / 64;

__global__ __launch_bounds__(COMPACT_THREADS) void k_compactify(CompactArgs A) {
  const uint64_t* __restrict__ block_keys = A.block_keys;
  const int32_t* __restrict__ block_entry = A.block_entry;
  const uint8_t* __restrict__ block_flags = A.block_flags;
  const HashEntry* __restrict__ table = A.table;
  int32_t* __restrict__ compact = A.compact;
  uint32_t* __restrict__ cmask = A.cmask;
  int32_t* counters = A.counters;
  const int counter_id = A.counter_id, all_live = A.all_live;
  const ParamsK& P = A.P;
  const BatchFrames& B = A.B;
  __shared__ int s_wtot[COMPACT_WAVES], s_wlast[COMPACT_WAVES], s_wpop[COMPACT_WAVES];
  __shared__ int s_base;
  __shared__ int4 s_c[COMPACT_THREADS];        // (bx, by, bz, listed?) of the workgroup's directory entries
  __shared__ uint32_t s_m[COMPACT_THREADS];    // their frame masks
  __shared__ uint32_t s_fk[MAX_BATCH * FRAMEK_WORDS];   // the batch's FrameK array, copied from the kernarg segment
  const int hw = counters[C_HIGH_WATER];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t last_bit = 1u << (B.n - 1);
  const bool wide = !all_live && B.n > COMPACT_FEW;   // uniform
  // frames per lane group: the smallest of 8 / 16 / 32 that holds the batch
  const int fshift = B.n <= 8 ? 3 : (B.n <= 16 ? 4 : 5);
  const int q = lane & ((1 << fshift) - 1), sub = lane >> fshift, epi = 64 >> fshift;
  FrameK F;
  if (wide && (int)(blockIdx.x * COMPACT_THREADS) < hw) {
    // the frames' constants: kernarg segment -> LDS by vector loads (per-lane addresses: every load of the workgroup is in flight at once), then frame q's
    // into this lane's registers for the life of the workgroup
    typedef __attribute__((address_space(4))) const uint32_t* karg_t;
    typedef __attribute__((address_space(4))) const char* kbyte_t;
    const karg_t kp = (karg_t)((kbyte_t)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(CompactArgs, B) + offsetof(BatchFrames, f));
    for (int i = threadIdx.x; i < B.n * FRAMEK_WORDS; i += COMPACT_THREADS) s_fk[i] = kp[i];
    __syncthreads();
    uint32_t* fw = reinterpret_cast<uint32_t*>(&F);
    const uint32_t* mine = s_fk + (q < B.n ? q : 0) * FRAMEK_WORDS;
#pragma unroll
    for (int i = 0; i < FRAMEK_WORDS; i++) fw[i] = mine[i];
  }
  for (int base = blockIdx.x * COMPACT_THREADS; base < hw; base += gridDim.x * COMPACT_THREADS) {
    const int i = base + (int)threadIdx.x;   // this thread's directory entry
    uint32_t m = 0u;
    if (wide) {
      int4 c = make_int4(0, 0, 0, 0);
      if (i < hw) {
        const uint64_t k = block_keys[i];
        if (k != KEY_EMPTY && !(block_flags[i] & 1)) {   // ghosts are never fused
          unpack_key(k, c.x, c.y, c.z);
          c.w = 1;
        }
      }
      s_c[threadIdx.x] = c;
      __syncthreads();
      const uint64_t gmask = fshift == 5 ? 0xFFFFFFFFull : ((1ull << (1 << fshift)) - 1ull);
#pragma unroll 2
      for (int e0 = wave * 64; e0 < wave * 64 + 64; e0 += epi) {   // this wave's 64 entries, 64 / FPL of them per step, against all frames at once
        const int4 cc = s_c[e0 + sub];
        const bool in = cc.w != 0 && q < B.n && block_in_frustum(P, F, cc.x, cc.y, cc.z);
        const uint64_t bal = __ballot(in);
        if (q == 0) s_m[e0 + sub] = (uint32_t)((bal >> (sub << fshift)) & gmask);
      }
      __syncthreads();
      m = s_m[threadIdx.x];
      if (m != 0u) {
        const uint32_t birth = table[block_entry[i]].birth;
        if (birth > B.seq0) {
          const uint32_t d = birth - B.seq0;
          m = d >= 32u ? 0u : (m & ~((1u << d) - 1u));
        }
      }
    }   // (passes of up to COMPACT_FEW frames and the list of every live block: k_compactify_few)
    const uint64_t bal = __ballot(m != 0u);
    const int rank = __popcll((unsigned long long)(bal & ((1ull << lane) - 1ull)));
    const int wtotal = __popcll((unsigned long long)bal);
    const int wlast = __popcll((unsigned long long)__ballot((m & last_bit) != 0u));
    int pop = __popc(m);
    for (int o = 32; o > 0; o >>= 1) pop += __shfl_xor(pop, o);
    if (lane == 0) { s_wtot[wave] = wtotal; s_wlast[wave] = wlast; s_wpop[wave] = pop; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0, tlast = 0;
      for (int w = 0; w < COMPACT_WAVES; w++) { total += s_wtot[w]; tlast += s_wlast[w]; }
      s_base = 0;
      if (total) {
        const unsigned long long add = (unsigned long long)(uint32_t)total | ((unsigned long long)(uint32_t)tlast << 32);
        s_base = (int)(uint32_t)atomicAdd(reinterpret_cast<unsigned long long*>(&counters[counter_id]), add);
      }
    } else if (threadIdx.x == 64 && !all_live) {   // the two statistics: another wave's lane, so that nobody waits for them behind the returning atomic
      int total = 0, tpop = 0;
      for (int w = 0; w < COMPACT_WAVES; w++) { total += s_wtot[w]; tpop += s_wpop[w]; }
      if (total) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&counters[C_TOTAL_LO]), (unsigned long long)tpop);
        atomicAdd(reinterpret_cast<unsigned long long*>(&counters[C_TILES_LO]), (unsigned long long)total);
      }
    }
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; w++) off += s_wtot[w];
    if (m != 0u) {
      compact[off + rank] = i;
      cmask[off + rank] = m;
    }
    __syncthreads();
  }
}

// The same list for FEW frames per pass (up to COMPACT_FEW: a live stream's one frame per launch) or for every live block (all_live): one thread per entry and a
// loop over the frames -- no lane groups, no LDS staging of the frames' constants -- and a kernel of its own so that neither sets the other's register budget.
__global__ __launch_bounds__(COMPACT_THREADS) void k_compactify_few(CompactArgs A) {
  const uint64_t* __restrict__ block_keys = A.block_keys;
  const int32_t* __restrict__ block_entry = A.block_entry;
  const uint8_t* __restrict__ block_flags = A.block_flags;
  const HashEntry* __restrict__ table = A.table;
  int32_t* __restrict__ compact = A.compact;
  uint32_t* __restrict__ cmask = A.cmask;
  int32_t* counters = A.counters;
  const int counter_id = A.counter_id, all_live = A.all_live;
  const ParamsK& P = A.P;
  const BatchFrames& B = A.B;
  __shared__ int s_wlast[COMPACT_WAVES], s_wpop[COMPACT_WAVES];
  __shared__ int s_base;
  const int hw = counters[C_HIGH_WATER];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t last_bit = 1u << (B.n - 1);
  // Few frames per pass and a long directory (a live stream at small voxels: 1.6 M entries at 1 mm): EU entries per thread and ONE place in the list asked for
  // per workgroup and 2 048 entries.  Asked for per 256 entries, the 6 100 returning atomics on the one list counter (and twice as many on the two statistics
  // words) WERE the kernel: 150 us for a pass over 15 MB of keys, ~25 ns per atomic (tools/gpu/period_summary.py, profiles/r06_alloc_1mm.txt).  The list keeps
  // its order: ascending directory index within a workgroup's stretch.
  constexpr int EU = 8;
  __shared__ int s_ut[EU][COMPACT_WAVES];
  for (int base = blockIdx.x * COMPACT_THREADS * EU; base < hw; base += gridDim.x * COMPACT_THREADS * EU) {
    uint64_t k[EU];
    uint8_t fl[EU];
    uint32_t m[EU];
    int rank[EU];
#pragma unroll
    for (int u = 0; u < EU; u++) {   // every load of the stretch in flight together
      const int i = base + u * COMPACT_THREADS + (int)threadIdx.x;
      k[u] = i < hw ? block_keys[i] : KEY_EMPTY;
      fl[u] = i < hw ? block_flags[i] : (uint8_t)0;
    }
    int wlast = 0, pop = 0;
#pragma unroll
    for (int u = 0; u < EU; u++) {
      m[u] = 0u;
      if (k[u] != KEY_EMPTY && !(all_live != 1 && (fl[u] & 1))) {  // ghosts are listed by all_live == 1 only
        if (all_live) m[u] = 1u;
        else {
          int bx, by, bz;
          unpack_key(k[u], bx, by, bz);
          for (int qq = 0; qq < B.n; qq++)
            if (block_in_frustum(P, B.f[qq], bx, by, bz)) m[u] |= 1u << qq;
          if (m[u] != 0u && B.n > 1) {
            const uint32_t birth = table[block_entry[base + u * COMPACT_THREADS + (int)threadIdx.x]].birth;
            if (birth > B.seq0) {
              const uint32_t d = birth - B.seq0;
              m[u] = d >= 32u ? 0u : (m[u] & ~((1u << d) - 1u));
            }
          }
        }
      }
      const uint64_t bal = __ballot(m[u] != 0u);
      rank[u] = __popcll((unsigned long long)(bal & ((1ull << lane) - 1ull)));
      if (lane == 0) s_ut[u][wave] = __popcll((unsigned long long)bal);
      wlast += __popcll((unsigned long long)__ballot((m[u] & last_bit) != 0u));
      pop += __popc(m[u]);
    }
    for (int o = 32; o > 0; o >>= 1) pop += __shfl_xor(pop, o);
    if (lane == 0) { s_wlast[wave] = wlast; s_wpop[wave] = pop; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0, tlast = 0;
      for (int w = 0; w < COMPACT_WAVES; w++) {
        tlast += s_wlast[w];
        for (int u = 0; u < EU; u++) total += s_ut[u][w];
      }
      s_base = 0;
      if (total) {
        const unsigned long long add = (unsigned long long)(uint32_t)total | ((unsigned long long)(uint32_t)tlast << 32);
        s_base = (int)(uint32_t)atomicAdd(reinterpret_cast<unsigned long long*>(&counters[counter_id]), add);
      }
    } else if (threadIdx.x == 64 && !all_live) {   // the two statistics: another wave's lane, so that nobody waits for them behind the returning atomic
      int total = 0, tpop = 0;
      for (int w = 0; w < COMPACT_WAVES; w++) {
        tpop += s_wpop[w];
        for (int u = 0; u < EU; u++) total += s_ut[u][w];
      }
      if (total) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&counters[C_TOTAL_LO]), (unsigned long long)tpop);
        atomicAdd(reinterpret_cast<unsigned long long*>(&counters[C_TILES_LO]), (unsigned long long)total);
      }
    }
    __syncthreads();
    int off = s_base;
#pragma unroll
    for (int u = 0; u < EU; u++) {
      int mine = off;
      for (int w = 0; w < COMPACT_WAVES; w++) {
        const int t = s_ut[u][w];
        if (w < wave) mine += t;
        off += t;
      }
      if (m[u] != 0u) {
        compact[mine + rank[u]] = base + u * COMPACT_THREADS + (int)threadIdx.x;
        cmask[mine + rank[u]] = m[u];
      }
    }
    __syncthreads();
  }
}

}  // namespace

void sf_launch_compact(const sf_fuser* f, int sl, const BatchFrames& bf, hipStream_t s) {
  const CompactArgs a{f->block_keys, f->block_entry, f->block_flags, f->table, f->compact2[sl], f->cmask2[sl], f->counters, sf_compact_counter(sl), 0, f->pk, bf};
  if (bf.n > COMPACT_FEW) hipLaunchKernelGGL(k_compactify, dim3(f->compact_grid * (1024 / COMPACT_THREADS)), dim3(COMPACT_THREADS), 0, s, a);
  else hipLaunchKernelGGL(k_compactify_few, dim3(f->compact_grid * (1024 / COMPACT_THREADS)), dim3(COMPACT_THREADS), 0, s, a);
}

int sf_compact_live(sf_fuser* f, int32_t* n_out, int include_ghosts) {
  SF_HIP_CHECK(sf_quiesce(f));
  BatchFrames dummy;
  std::memset(&dummy, 0, sizeof(dummy));
  dummy.n = 1;
  SF_HIP_CHECK(hipMemsetAsync(&f->counters[C_EXPORT], 0, 8, f->stream));
  hipLaunchKernelGGL(k_compactify_few, dim3(f->compact_grid * (1024 / COMPACT_THREADS)), dim3(COMPACT_THREADS), 0, f->stream, (CompactArgs{f->block_keys, f->block_entry, f->block_flags, f->table, f->compact,
                     f->cmask2[0], f->counters, (int)C_EXPORT, include_ghosts ? 1 : 2, f->pk, dummy}));
  SF_HIP_CHECK(hipMemcpyAsync(n_out, &f->counters[C_EXPORT], 4, hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(sf_quiesce(f));
  return SF_OK;
}
