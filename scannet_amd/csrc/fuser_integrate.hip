// fuser_integrate.hip -- stage 4 of a fusion pass: integrate / deintegrate the pass's frames into the tiles of its list.  k_integrate (every case,
// 25 variants), the software-pipelined k_integrate_pipe (one colourless frame per launch) and the tile read-modify-write of the calibration;
// sf_launch_integrate picks the variant.
#include <hip/hip_runtime.h>

#include "fuser_device.h"
#include "fuser_fuse.h"
#include "fuser_internal.h"
#include "hip_util.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// K4: integrate / deintegrate.  One wave per 8^3 block: the 4 KiB tile is read with four 16 B-per-lane
// loads (two x-adjacent voxels per load; in the x-row layout of multi-frame passes the lane's own 64 contiguous bytes), updated in
// registers by EVERY frame of the batch that sees the block (temporal blocking: HBM traffic per frame
// falls by the batch size, the kernel turns from HBM-bound at B = 1 to VALU/L2-gather-bound) and written
// back with the same pattern.  There is no reuse inside a tile, so it is not
// staged through LDS; the depth image (1.2 MB f32) is gathered through L1/L2.
// pair layout: lane l, load j: uint4 q = 64 j + l -> voxels 2q, 2q+1 -> x = (2l)&7 (+1), y = (l>>2)&7, z = 2j + (l>>5);
// x-row layout (XR): lane l, load j: uint4 q = 4 l + j -> x = 2j (+1), y = l & 7, z = l >> 3.
// ---------------------------------------------------------------------------------------------------

// 4 waves per SIMD (<= 128 VGPRs).  Tried for the one-frame-per-launch case: 5 waves / 96 VGPRs with the tile in two
// half passes -- the spills cost more than the occupancy buys (183 us vs 112 us per launch).
constexpr int INT_WAVES = 5;   // workgroups (of 4 waves) per CU the register budget of k_integrate is set for (plain pairs: 91 registers)
constexpr int INT_NJ = 4;      // rows of the tile fused together per frame: 4 = the whole tile at once, 2 = in halves (fewer live registers)
// NJ = 2 (the tile in halves: 63 registers, 8 waves per SIMD) looks 15 % faster in the two-stream schedule (696 against 814 us per launch) only because its
// waves take every register of the SIMDs and the allocation kernel on the other stream starves (372 -> 818 us): the pass as a whole is slower
// (profiles/r05_integrate_ab.txt).  Alone the two variants are within a few per cent.  NJ = 2 runs the LAST pass of a sf_fuser_integrate_batch_device call
// -- nothing is queued behind that pass, no front chain runs beside it: +0.8 % on a 20-frame call, measured --, every other pass NJ = 4 at 5 waves.  Same
// voxels either way (tests/test_gpu_tsdf.py::test_batched_pass_equals_frame_by_frame runs both).
template <int SIGN, int COLOR, bool TAB, int WM, bool ROWS, int NJ = INT_NJ, bool XR = false>
__global__ __launch_bounds__(256, NJ == 2 ? (XR ? 7 : 8) : INT_WAVES) void k_integrate(uint4* __restrict__ voxels, const uint64_t* __restrict__ block_keys,
                                                   const int32_t* __restrict__ compact, const uint32_t* __restrict__ cmask,
                                                   const float* __restrict__ depthf_all, const uint2* __restrict__ texel_all,
                                                   int32_t* counters, int32_t* host_mirror, int compact_counter, int xcd_walk, ParamsK P,
                                                   BatchTi B) {
  // The passes of several frames with the shipped parameters (predicated write-back, x-row layout) keep one 16-byte record per weight in LDS: everything
  // the update derives from the voxel's weight alone, 1/m among it (fill_weight_records).  Every other variant: the float table of 1/m.
  constexpr bool REC = SIGN > 0 && TAB && WM == 2 && !ROWS && XR;
  __shared__ uint4 s_tab[REC ? WREC : RTAB / 4];
  float* const s_rtab = reinterpret_cast<float*>(s_tab);  // correctly rounded 1/m for the weighted-mean division (fuse_update)
  if (REC) {
    fill_weight_records(s_tab, (int)threadIdx.x, 256);
    __syncthreads();
  } else if (TAB) {
    for (int i = threadIdx.x; i < RTAB; i += 256) s_rtab[i] = 1.0f / (float)(i > 0 ? i : 1);
    __syncthreads();
  }
  const int n = counters[compact_counter];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    atomicExch(&counters[C_LAST_BLOCKS], counters[compact_counter + 1]);  // counters share cache lines with words the front stream updates atomically
    if (host_mirror) *host_mirror = n;
  }
  // pair layout: lane l, load j = uint4 64 j + l = voxels x = (2l) & 7 (+1), y = (l >> 2) & 7, z = 2j + (l >> 5);
  // x-row layout (XR): lane l, load j = uint4 4 l + j = voxels x = 2j (+1), y = l & 7, z = l >> 3 (the lane's 64 contiguous bytes of the tile)
  const int lx = XR ? 0 : (2 * lane) & 7;
  const int ly = XR ? lane & 7 : (lane >> 2) & 7;
  const int lzb = XR ? lane >> 3 : lane >> 5;
  const size_t npx = (size_t)P.W * P.H;
  // XCD-aware walk of the list: workgroup b runs on XCD b % 8 (observed placement; a speed hint only, any placement is
  // correct).  Each XCD takes ONE contiguous eighth of the list -- neighbouring list entries are neighbouring blocks
  // that gather neighbouring depth pixels, so an XCD's 4 MiB L2 holds its own part of the batch's depth images instead
  // of all eight L2s each cycling through all 16 x 1.2 MB.  xcd_walk == 0: plain grid-stride order.
  const int wg_total = (n + 3) >> 2;                         // workgroups' worth of list entries
  const int chunk = xcd_walk ? (wg_total + 7) >> 3 : wg_total;
  const int lanes = xcd_walk ? 8 : 1;                        // interleaved sub-grids
  const int sub = xcd_walk ? (int)(blockIdx.x & 7) : 0;
  const int per_sub = max(1, (int)gridDim.x / lanes);
  for (int loc = xcd_walk ? (int)(blockIdx.x >> 3) : (int)blockIdx.x; loc < chunk; loc += per_sub) {
    const int i = ((sub * chunk + loc) << 2) + wave;
    if (i >= n) continue;
    const int slot = compact[i];
    uint32_t frames = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmask[i]);  // wave-uniform: the frame loop runs on the scalar unit
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
    // temporal blocking: the tile stays in registers while every frame of the batch that sees the block is fused
    // into it, in frame order (the same sequence of updates per voxel as frame-by-frame integration)
    while (frames != 0u) {
      const int q = __builtin_ctz(frames);
      frames &= frames - 1u;
      const float* Ti = B.Ti[q];
      const float* __restrict__ depthf = depthf_all + (size_t)q * npx;
      const uint2* __restrict__ texel = texel_all + (size_t)q * npx;
#pragma unroll
      for (int j0 = 0; j0 < 4; j0 += NJ) {
        if (j0 == 0) fuse_rows<SIGN, COLOR, TAB, WM, 0, NJ, ROWS, XR, true, REC>(P, Ti, depthf, texel, s_rtab, wx, wy, wz, wxp, v, dirty);
        if (j0 == 1) fuse_rows<SIGN, COLOR, TAB, WM, 1 % (5 - NJ), NJ, ROWS, XR, true, REC>(P, Ti, depthf, texel, s_rtab, wx, wy, wz, wxp, v, dirty);
        if (j0 == 2) fuse_rows<SIGN, COLOR, TAB, WM, 2 % (5 - NJ), NJ, ROWS, XR, true, REC>(P, Ti, depthf, texel, s_rtab, wx, wy, wz, wxp, v, dirty);
        if (j0 == 3) fuse_rows<SIGN, COLOR, TAB, WM, 3 % (5 - NJ), NJ, ROWS, XR, true, REC>(P, Ti, depthf, texel, s_rtab, wx, wy, wz, wxp, v, dirty);
      }
    }
    if (ROWS) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if ((dirty[j] >> lane) & 1ull) vb[XR ? lane * 4 + j : j * 64 + lane] = v[j];
    } else if (dirty[0] != 0ull) {   // wave-uniform: some frame of the pass changed a voxel of this tile -- the whole tile goes back, four 1 KiB stores
#pragma unroll
      for (int j = 0; j < 4; j++) vb[XR ? lane * 4 + j : j * 64 + lane] = v[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// K4p: the same update for the HBM-bound regime (ONE frame per launch: a live stream, SF_BATCH=1), software-pipelined.
// In k_integrate every wave is a serial chain  tile load -> project -> 8 depth gathers -> update -> store  and a SIMD holds
// four chains; measured the chains, not HBM, bound it.  Here a persistent wave walks its share of the list
// and keeps three things in flight for LATER tiles while it updates tile k in registers:
//   * tile k+2 and k+3 travel HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, four 1 KiB requests per tile, no VGPRs) into
//     a two-slot ring per wave;
//   * the eight depth gathers of tile k+1 (projected one turn early) land in LDS as well (global_load_lds_dword: per-lane
//     source address, lane-linear destination), two 2 KiB slots per wave;
// so nothing asynchronous ever targets a VGPR and every wait is a hand-counted s_waitcnt vmcnt(N) (vector-memory operations
// return in order: "at most N outstanding" = everything but the N youngest has landed).  Per turn k the issue order is
//   [tile k+1's stores of the previous turn: S(k-1)]  G(k+1) x8  D(k+3) x4   and the two waits are
//   top : tile k+1 (requested two turns ago) has landed      -- younger: S(k-2)? G(k) 8, D(k+2) 4, S(k-1)  => vmcnt(12)
//   mid : the gathers of tile k (issued last turn) have landed -- younger: D(k+2) 4, S(k-1), G(k+1) 8, D(k+3) 4 => vmcnt(16)
// (stores only make the true count larger, i.e. the waits conservative).  hipcc never sees these loads (it would wait
// vmcnt(0) at every use while an LDS-DMA is in flight); it only sees ordinary ds_reads after the waits.
// LDS per wave: 2 x 4 KiB tiles + 2 x 2 KiB gathers = 12 KiB => 3 workgroups (12 waves, 144 KiB) per CU, and 16 KiB left for a workgroup of
// the next frame's allocation (10.6 KiB for one frame per launch) to run beside it.  Geometry only, no colour:
// the colour variant stays on k_integrate.  Arithmetic = fuse_project / fuse_update, bit-identical to k_integrate.
// ---------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int PIPE_WGS = 3;   // workgroups of k_integrate_pipe per CU (48 KiB of LDS each): its occupancy bound and its persistent grid, PIPE_WGS per CU

// NT: tile loads and stores carry the non-temporal hint -- for passes whose tile set is many times the 256 MiB Infinity Cache (1 mm voxels:
// 5-7 GB per frame), where keeping streamed tiles on-die only evicts the depth image and the list; below that size the cache hits of
// consecutive frames are worth more (measured), so run_batch picks the variant from the previous pass's list length.
template <bool TAB, int WM, bool NT>
__global__ __launch_bounds__(256, PIPE_WGS) void k_integrate_pipe(uint4* __restrict__ voxels, const uint64_t* __restrict__ block_keys,
                                                        const int32_t* __restrict__ compact, const float* __restrict__ depthf, int32_t* counters,
                                                        int32_t* host_mirror, int compact_counter, ParamsK P, BatchTi B) {
  __shared__ uint4 s_tile[4][2][256];   // per wave: two 4 KiB tile slots
  __shared__ float s_gath[4][2][512];   // per wave: two slots of 8 gathers x 64 lanes
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int stride = (int)gridDim.x * 4;
  const int i0 = (int)blockIdx.x * 4 + wave;
  const int n = counters[compact_counter];
  uint4* const ring = &s_tile[wave][0][0];
  float* const gath = &s_gath[wave][0][0];
  const uint32_t ring_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_ptr_t)ring);
  const uint32_t gath_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_ptr_t)gath);
  auto slot_of = [&](int i) { return i < n ? __builtin_amdgcn_readfirstlane(compact[i]) : 0; };
  // LDS-DMA of one tile (4 x 1 KiB) into ring slot `ts`; the immediate offset applies to the global AND the LDS address
  auto dma_tile = [&](int slot, int ts) {
    const uint4* src = voxels + (size_t)slot * 256 + lane;
    uint32_t keep;
    if (NT)
      asm volatile(
          "s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[lds]\n\ts_nop 0\n\t"
          "global_load_lds_dwordx4 %[src], off nt\n\tglobal_load_lds_dwordx4 %[src], off offset:1024 nt\n\t"
          "global_load_lds_dwordx4 %[src], off offset:2048 nt\n\tglobal_load_lds_dwordx4 %[src], off offset:3072 nt\n\t"
          "s_mov_b32 m0, %[keep]"
          : [keep] "=&s"(keep)
          : [src] "v"(src), [lds] "s"(ring_lds + (uint32_t)ts * 4096u)
          : "memory");
    else
      asm volatile(
          "s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[lds]\n\ts_nop 0\n\t"
          "global_load_lds_dwordx4 %[src], off\n\tglobal_load_lds_dwordx4 %[src], off offset:1024\n\t"
          "global_load_lds_dwordx4 %[src], off offset:2048\n\tglobal_load_lds_dwordx4 %[src], off offset:3072\n\t"
          "s_mov_b32 m0, %[keep]"
          : [keep] "=&s"(keep)
          : [src] "v"(src), [lds] "s"(ring_lds + (uint32_t)ts * 4096u)
          : "memory");
  };
  // the 8 gathers of one tile into gather slot `gs` (request j -> bytes [256 j, 256 j + 256) of the slot)
  auto gather8 = [&](const uint32_t (&pix)[8], int gs) {
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = pix[k] << 2;
    uint32_t keep;
    const uint32_t base = gath_lds + (uint32_t)gs * 2048u;
    asm volatile(
        "s_mov_b32 %[keep], m0\n\t"
        "s_mov_b32 m0, %[b]\n\ts_nop 0\n\tglobal_load_lds_dword %[o0], %[d]\n\t"
        "s_add_u32 m0, %[b], 0x100\n\ts_nop 0\n\tglobal_load_lds_dword %[o1], %[d]\n\t"
        "s_add_u32 m0, %[b], 0x200\n\ts_nop 0\n\tglobal_load_lds_dword %[o2], %[d]\n\t"
        "s_add_u32 m0, %[b], 0x300\n\ts_nop 0\n\tglobal_load_lds_dword %[o3], %[d]\n\t"
        "s_add_u32 m0, %[b], 0x400\n\ts_nop 0\n\tglobal_load_lds_dword %[o4], %[d]\n\t"
        "s_add_u32 m0, %[b], 0x500\n\ts_nop 0\n\tglobal_load_lds_dword %[o5], %[d]\n\t"
        "s_add_u32 m0, %[b], 0x600\n\ts_nop 0\n\tglobal_load_lds_dword %[o6], %[d]\n\t"
        "s_add_u32 m0, %[b], 0x700\n\ts_nop 0\n\tglobal_load_lds_dword %[o7], %[d]\n\t"
        "s_mov_b32 m0, %[keep]"
        : [keep] "=&s"(keep)
        : [o0] "v"(o[0]), [o1] "v"(o[1]), [o2] "v"(o[2]), [o3] "v"(o[3]), [o4] "v"(o[4]), [o5] "v"(o[5]), [o6] "v"(o[6]), [o7] "v"(o[7]),
          [d] "s"(depthf), [b] "s"(base)
        : "memory", "scc");
  };
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    atomicExch(&counters[C_LAST_BLOCKS], counters[compact_counter + 1]);
    if (host_mirror) *host_mirror = n;
  }
  if (i0 >= n) return;
  const int lx = (2 * lane) & 7;
  const int ly = (lane >> 2) & 7;
  const int lzb = lane >> 5;
  const float* Ti = B.Ti[0];
  const FrameV FV = frame_constants(P, Ti);   // one frame per launch: the constants are the kernel's
  auto project = [&](uint64_t key, v2f (&pz)[4], uint32_t (&pix)[8], uint32_t& okmask) {
    int bx, by, bz;
    unpack_key(key, bx, by, bz);
    const v2f wx = {(float)(8 * bx + lx) * P.voxel, (float)(8 * bx + lx + 1) * P.voxel};
    const float wy = (float)(8 * by + ly) * P.voxel;
    float wz[4];
#pragma unroll
    for (int j = 0; j < 4; j++) wz[j] = (float)(8 * bz + 2 * j + lzb) * P.voxel;
    bool ok[8];
    fuse_project<0, 4, true>(P, FV, wx, wy, wz, pz, pix, ok);
    okmask = 0u;
#pragma unroll
    for (int k = 0; k < 8; k++) okmask |= ok[k] ? (1u << k) : 0u;
  };
  // ---- prologue: tiles 0 and 1 requested, tile 0 read and projected, its gathers and tile 2 requested.
  // List entries and block keys are wave-uniform scalar loads fetched ahead of their use (slot of tile k+4 and key of tile
  // k+2 during turn k), so that no dependent scalar round trip ever opens a turn.
  int i = i0;
  int slot = slot_of(i), slot1 = slot_of(i + stride), slot2 = slot_of(i + 2 * stride), slot3 = slot_of(i + 3 * stride);
  dma_tile(slot, 0);
  if (i + stride < n) dma_tile(slot1, 1);
  const uint64_t key0 = block_keys[slot];
  uint64_t key1 = i + stride < n ? block_keys[slot1] : 0ull;
  if (i + stride < n) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint4 v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = ring[0 * 256 + j * 64 + lane];
  v2f pz[4];
  uint32_t okmask;
  {
    uint32_t pix[8];
    project(key0, pz, pix, okmask);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // tile 0 is in registers: its ring slot may be overwritten
    gather8(pix, 0);
    if (i + 2 * stride < n) dma_tile(slot2, 0);
  }
  int par = 0;  // parity of the current turn: tile k sits in gather slot par, tile k+1 in ring slot par ^ 1
  for (;;) {
    const int i1 = i + stride, i4 = i + 4 * stride;
    const bool has1 = i1 < n, has2 = i + 2 * stride < n, has3 = i + 3 * stride < n;  // wave-uniform
    uint4 vn[4];
    v2f pzn[4];
    uint32_t okn = 0u;
    int slot4 = 0;
    uint64_t key2 = 0ull;
    if (has1) {
      // top: tile k+1 has landed (younger than it: at least G(k) 8 + D(k+2) 4 when tile k+2 exists, else only G(k) 8)
      if (has2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
#pragma unroll
      for (int j = 0; j < 4; j++) vn[j] = ring[(par ^ 1) * 256 + j * 64 + lane];
      uint32_t pixn[8];
      project(key1, pzn, pixn, okn);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // tile k+1 is in registers before its slot is handed to tile k+3
      gather8(pixn, par ^ 1);
      if (has3) dma_tile(slot3, par ^ 1);
      // scalar prefetch for later turns (after the lgkmcnt wait above, so that it is not waited for here)
      if (i4 < n) slot4 = __builtin_amdgcn_readfirstlane(compact[i4]);
      if (has2) key2 = block_keys[slot2];
      // mid: the gathers of tile k have landed (younger: D(k+2) 4 if any, G(k+1) 8, D(k+3) 4 if any)
      if (has3) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else if (has2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    float d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = gath[par * 512 + k * 64 + lane];
    // RN(1 / (weight + sample)) by v_rcp_f32 + a Newton step (recip_rn: correctly rounded for every normal divisor, the same bits
    // as k_integrate's LDS table) -- this kernel has VALU slots to spare and its LDS decides who may run beside it: 48 KiB per
    // workgroup x 3 leaves 16 KiB per CU, room for one workgroup of the NEXT frame's allocation / compaction on the front stream
    v2f rcp_m[4];
    if (TAB) {
#pragma unroll
      for (int j = 0; j < 4; j++) rcp_m[j] = recip_rn((v2f){(float)((v[j].y >> 24) + (uint32_t)P.wsample), (float)((v[j].w >> 24) + (uint32_t)P.wsample)});
    }
    bool ok[8];
#pragma unroll
    for (int k = 0; k < 8; k++) ok[k] = (okmask >> k) & 1u;
    uint32_t cdummy[8];
    uint64_t dirty[4] = {0ull, 0ull, 0ull, 0ull};
    fuse_update<1, 0, TAB, WM, 0, 4>(P, FV, rcp_m, d, cdummy, pz, ok, v, dirty);  // consumes d: the gather slot is free again
    uint4* vb = voxels + (size_t)slot * 256;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((dirty[j] >> lane) & 1ull) {
        if (NT) __builtin_nontemporal_store((u32x4){v[j].x, v[j].y, v[j].z, v[j].w}, reinterpret_cast<u32x4*>(&vb[j * 64 + lane]));
        else vb[j * 64 + lane] = v[j];
      }
    if (!has1) break;
    i = i1;
    slot = slot1; slot1 = slot2; slot2 = slot3; slot3 = slot4;
    key1 = key2;
#pragma unroll
    for (int j = 0; j < 4; j++) { v[j] = vn[j]; pz[j] = pzn[j]; }
    okmask = okn;
    par ^= 1;
  }
}

// ---------------------------------------------------------------------------------------------------
// Measurement aid: the memory traffic of k_integrate WITHOUT its arithmetic -- every tile of the compact list is read
// with the same four 1 KiB loads per wave and (mode 0) written back unchanged, same grid, same list walk.  Its duration
// is the ceiling the access pattern itself (scattered 4 KiB read-modify-write) allows on this HBM; bench.py reports
// the one-frame-per-launch kernel against it (sf_fuser_calib_tile_rmw).  The volume is left bit-identical.
// The same traffic taken apart (sf_fuser_calib_tile_rmw_ex): WHICH tiles -- the pass's list (scattered over the pool) or tiles 0 .. n - 1 of the pool
// (one contiguous span of the same size) -- and HOW a wave turns from reading to writing -- tile by tile, or G tiles read and then G tiles written.
// If the contiguous copy runs no faster than the scattered one, the 4 KiB granularity is not what holds the pattern below the read-only rate; if the
// batched turnaround does not either, it is HBM's read / write mix itself.
// ---------------------------------------------------------------------------------------------------
template <bool NT, int G>
__global__ __launch_bounds__(256, 4) void k_tile_rmw_ex(uint4* __restrict__ voxels, const int32_t* __restrict__ compact, const int32_t* __restrict__ counters,
                                                     int compact_counter, int xcd_walk, int read_only, int contiguous, uint32_t* sink) {
  const int n = counters[compact_counter];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int groups = (n + G - 1) / G;                 // wave-sized units of work: G tiles each
  const int wg_total = (groups + 3) >> 2;
  const int chunk = xcd_walk ? (wg_total + 7) >> 3 : wg_total;
  const int lanes = xcd_walk ? 8 : 1;
  const int sub = xcd_walk ? (int)(blockIdx.x & 7) : 0;
  const int per_sub = max(1, (int)gridDim.x / lanes);
  uint32_t acc = 0;
  for (int loc = xcd_walk ? (int)(blockIdx.x >> 3) : (int)blockIdx.x; loc < chunk; loc += per_sub) {
    const int u = ((sub * chunk + loc) << 2) + wave;
    if (u >= groups) continue;
    uint4 v[G][4];
    uint4* vb[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int i = min(u * G + g, n - 1);            // the last group repeats its last tile: written back unchanged twice
      vb[g] = voxels + (size_t)(contiguous ? i : compact[i]) * 256;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (NT) { const u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(&vb[g][j * 64 + lane])); v[g][j] = make_uint4(t.x, t.y, t.z, t.w); }
        else v[g][j] = vb[g][j * 64 + lane];
      }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (read_only) { acc ^= v[g][j].x ^ v[g][j].y ^ v[g][j].z ^ v[g][j].w; continue; }
        asm volatile("" : "+v"(v[g][j].x));  // opaque to the optimiser: the store below stays
        if (NT) __builtin_nontemporal_store((u32x4){v[g][j].x, v[g][j].y, v[g][j].z, v[g][j].w}, reinterpret_cast<u32x4*>(&vb[g][j * 64 + lane]));
        else vb[g][j * 64 + lane] = v[g][j];
      }
    }
  }
  if (read_only && acc == 0x9E3779B9u) *sink = acc;
}

// the LDS reciprocal table of the integrate kernels is indexed by weight + sample: it covers weight_sample up to RTAB - 256
bool recip_table_ok(const sf_fuser* f) { return f->p.weight_sample >= 1 && f->p.weight_sample <= RTAB - 256 && f->p.weight_mode == 0; }

// Grid of the list-walking kernels (k_integrate, the tile read-modify-write): enough workgroups (4 list entries each) for `entries` +25 %; the kernels'
// grid-stride loop covers any excess, surplus workgroups exit at once.  Whole sub-grids of 8 for the XCD-aware walk.
int list_grid(const sf_fuser* f, int entries) {
  int grid = (entries + entries / 4 + 4096 + 3) / 4;
  if (grid > f->num_cus * 64) grid = f->num_cus * 64;
  return (grid + 7) & ~7;
}

// One integrate launch of a pass of n frames out of batch slot sl: a member per kernel family, the variant as template arguments.
struct IntegrateLaunch {
  const sf_fuser* f;
  int sl, n;
  const BatchTi& bt;
  hipStream_t s;

  template <int SIGN, int COLOR, bool TAB, int WM, bool ROWS, int NJ = INT_NJ, bool XR = false>
  void integrate() const {
    const int grid = list_grid(f, *f->host_mirror);   // sized for the last list length the device reported
    hipLaunchKernelGGL((k_integrate<SIGN, COLOR, TAB, WM, ROWS, NJ, XR>), dim3(grid), dim3(256), 0, s, f->voxels, f->block_keys, f->compact2[sl],
                       f->cmask2[sl], f->depthf2[sl], f->color2[sl], f->counters, f->host_mirror, sf_compact_counter(sl), f->xcd_walk ? 1 : 0, f->pk, bt);
  }
  // per-row write-back masks for one frame per launch (HBM-bound) and for deintegration; a pass of several frames (VALU-bound) writes touched tiles whole
  template <int SIGN, int COLOR, bool TAB, int WM>
  void rows() const {
    if (SIGN < 0 || n == 1) integrate<SIGN, COLOR, TAB, WM, true>();
    else integrate<1, COLOR, TAB, WM, false>();
  }
  template <int SIGN, bool TAB, int WM>
  void colour(bool col) const {
    if (col) rows<SIGN, 1, TAB, WM>();
    else rows<SIGN, 0, TAB, WM>();
  }
  // the x-row lane layout of a pass of several frames; `wide`: the 8-wave variant (NJ 2)
  template <int COLOR>
  void xrow(bool wide) const {
    if (wide) integrate<1, COLOR, true, 2, false, 2, true>();
    else integrate<1, COLOR, true, 2, false, INT_NJ, true>();
  }
  template <int WM>
  void pipe(bool nt) const {
    const dim3 pg((unsigned)(f->num_cus * PIPE_WGS));   // persistent: exactly what the CUs hold
    if (nt) hipLaunchKernelGGL((k_integrate_pipe<true, WM, true>), pg, dim3(256), 0, s, f->voxels, f->block_keys, f->compact2[sl], f->depthf2[sl],
                               f->counters, f->host_mirror, sf_compact_counter(sl), f->pk, bt);
    else hipLaunchKernelGGL((k_integrate_pipe<true, WM, false>), pg, dim3(256), 0, s, f->voxels, f->block_keys, f->compact2[sl], f->depthf2[sl],
                            f->counters, f->host_mirror, sf_compact_counter(sl), f->pk, bt);
  }
};

template <bool NT, int G>
void launch_tile_rmw(const sf_fuser* f, int sl, int grid, int read_only, int contiguous, uint32_t* sink) {
  hipLaunchKernelGGL((k_tile_rmw_ex<NT, G>), dim3(grid), dim3(256), 0, f->stream, f->voxels, f->compact2[sl], f->counters, sf_compact_counter(sl),
                     f->xcd_walk ? 1 : 0, read_only, contiguous, sink);
}
template <bool NT>
void launch_tile_rmw_g(const sf_fuser* f, int sl, int G, int grid, int read_only, int contiguous, uint32_t* sink) {
  if (G == 1) launch_tile_rmw<NT, 1>(f, sl, grid, read_only, contiguous, sink);
  else if (G == 2) launch_tile_rmw<NT, 2>(f, sl, grid, read_only, contiguous, sink);
  else launch_tile_rmw<NT, 4>(f, sl, grid, read_only, contiguous, sink);
}

}  // namespace

int sf_list_grid(const sf_fuser* f, int entries) { return list_grid(f, entries); }

// One frame per launch without colour runs the persistent k_integrate_pipe (tune "pipe" 0: always k_integrate)
bool sf_pipe_batch(const sf_fuser* f, int n, bool color, int sign) { return sign > 0 && n == 1 && !color && recip_table_ok(f) && f->pipe_mode != 0; }

void sf_launch_integrate(const sf_fuser* f, int sl, int n, int sign, bool col, const BatchTi& bt, hipStream_t s) {
  const IntegrateLaunch L{f, sl, n, bt, s};
  const bool ws1 = f->p.weight_sample == 1 && f->p.weight_mode == 0;   // every observation weighs exactly 1
  const bool shipped = ws1 && f->pk.wmax == 255;                        // the shipped setting
  if (sf_pipe_batch(f, n, col, sign)) {
    const bool nt = sf_big_pass(f);   // non-temporal tile traffic once the previous pass's tile set was beyond twice the Infinity Cache
    if (shipped) L.pipe<2>(nt);
    else if (ws1) L.pipe<1>(nt);
    else L.pipe<0>(nt);
  } else if (sign > 0) {
    if (shipped) {
      // a pass of several frames runs the x-row lane layout (fuse_project_xr): same voxels, the gathers of one instruction on two image rows instead of five.
      // The last pass of a batch call has no front chain beside it: the 8-wave variant (NJ 2)
      const int cl = col ? (f->p.colour_first ? 1 : 2) : 0;
      const bool wide = f->tail_pass && f->tail_wide;
      if (cl == 1) L.rows<1, 1, true, 2>();
      else if (n == 1) { if (cl == 2) L.integrate<1, 2, true, 2, true>(); else L.integrate<1, 0, true, 2, true>(); }
      else if (cl == 2) L.xrow<2>(wide);
      else L.xrow<0>(wide);
    }
    else if (ws1) L.colour<1, true, 1>(col);
    else if (recip_table_ok(f)) L.colour<1, true, 0>(col);
    else if (f->p.weight_mode == 1) L.colour<1, false, 3>(col);
    else L.colour<1, false, 0>(col);
  }
  // deintegration
  else if (f->p.weight_mode == 1) L.colour<-1, false, 3>(col);
  else L.colour<-1, false, 0>(col);
}

// scanfuse_internal.h: the pattern ceiling taken apart.  mode bit 0: read only; bit 1: contiguous tiles 0 .. n - 1 instead of the pass's list; bits 2-3:
// tiles per turnaround 1 / 2 / 4 (0, 1, 2).  Every tile is written back as it was read: the volume is unchanged whatever it holds.
SF_API int sf_fuser_calib_tile_rmw_ex(sf_fuser* f, int mode, int iters, double* avg_us, uint32_t* tiles) {
  if (!f || iters < 1 || mode < 0 || (mode >> 2) > 2) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_calib_tile_rmw_ex: bad argument");
  SF_HIP_CHECK(hipSetDevice(f->device));
  SF_HIP_CHECK(sf_quiesce(f));
  const int sl = f->slot ^ 1;  // the list of the most recent pass
  int32_t n = 0;
  SF_HIP_CHECK(hipMemcpy(&n, &f->counters[sf_compact_counter(sl)], 4, hipMemcpyDeviceToHost));
  if ((uint32_t)n > (uint32_t)f->p.num_sdf_blocks) return sf::fail(SF_ERR_INVALID_ARG, "sf_fuser_calib_tile_rmw_ex: list length %d out of range", n);
  const int read_only = mode & 1, contiguous = (mode >> 1) & 1, G = 1 << (mode >> 2);
  const int grid = list_grid(f, (n + G - 1) / G);
  sf::DevBuf sink;
  SF_HIP_CHECK(sink.alloc(4));
  sf::EventSpan span;
  const bool nt = sf_big_tile_set((uint32_t)n);   // the cache policy k_integrate_pipe would pick for this tile set
  double total_us = 0;
  for (int it = 0; it < iters + 1; it++) {  // first launch untimed
    span.begin(f->stream);
    if (nt) launch_tile_rmw_g<true>(f, sl, G, grid, read_only, contiguous, sink.as<uint32_t>());
    else launch_tile_rmw_g<false>(f, sl, G, grid, read_only, contiguous, sink.as<uint32_t>());
    span.end(f->stream);
    SF_HIP_CHECK(hipEventSynchronize(span.b));
    if (it > 0) total_us += span.us();
  }
  if (avg_us) *avg_us = total_us / iters;
  if (tiles) *tiles = (uint32_t)n;
  return SF_OK;
}
// the pattern itself: the pass's list, tile by tile
SF_API int sf_fuser_calib_tile_rmw(sf_fuser* f, int read_only, int iters, double* avg_us, uint32_t* tiles) {
  return sf_fuser_calib_tile_rmw_ex(f, read_only ? 1 : 0, iters, avg_us, tiles);
}
