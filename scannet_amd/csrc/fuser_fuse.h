// fuser_fuse.h -- the update of one frame into one tile held in registers: projection (fuse_project, fuse_project_xr), the weighted-mean / weight / colour
// update itself (fuse_update) and the two chained with the depth gathers (fuse_rows).  Shared by the kernels that keep a tile in registers across the frames
// of a pass: k_integrate / k_integrate_pipe (fuser_integrate.hip) and k_reintegrate (fuser_reintegrate.hip).  Included by those translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "fuser_device.h"
#include "fuser_internal.h"

namespace {

// One frame into one tile held in registers (8 voxels per lane).  Once a batch amortises the HBM traffic the kernel sits on its instruction mix
// (SQ_INSTS_VALU x 2 clk / SIMD clk = 0.57 of the guide's issue peak, the texture addresser busy 0.56 of the time, HBM at 9 %: bench.py `roofline`,
// profiles/r06_integrate_xrow_ab.txt), so the update is written for instruction count:
//   * two straight-line phases: phase A projects all eight voxels and issues the eight depth gathers together at
//     clamped addresses, phase B applies the update (a per-voxel early-out chain serialises eight
//     L2 round trips and costs a scalar branch pair per test) -- under a select, or, for the shipped parameters, with the
//     instruction that produces a new word writing the tile register under the voxel's update mask (fuse_update);
//   * what is a property of the pixel or of the lane is not tested per voxel: the integration distance is gated by the pre-pass (-inf fails the
//     band test by itself), "in front of the camera" is two compares and a vote per lane in the x-row layout (fuse_project_xr);
//   * the lane's voxel pairs are written as v2f pairs (fuser_internal.h) and compiled as two plain fp32 operations each: on gfx950 a v_pk_*_f32 holds the
//     SIMD as long as two plain ones and issues beside nothing (rounds 1-4 shipped the packed form);
//   * the two IEEE divisions of DESIGN.md 3.5 are expanded by hand.  1/pcz: v_rcp_f32 seed + ONE Newton step --
//     correctly rounded from a seed that is one of the two floats either side of 1/pcz (tools/check_division.c part 4), which
//     gfx950's v_rcp_f32 delivers for every normal argument (sf_selftest_recip_one_step: all 2^32 bit patterns on the device, 0
//     mismatches; recip_rn, fuser_internal.h); no div_scale / div_fixup range handling (pcz is a camera-space depth in
//     metres).  (old*w + sdf*wn) / (w + wn): the divisor is a small integer, its
//     correctly rounded reciprocal comes from an LDS table and ONE Markstein correction q1 = fma(fma(-m, q0, n), r, q0)
//     yields the correctly rounded quotient (same tool: 1.4e9 cases incl. near-halfway); numerators below 2^-100
//     take the plain division so that underflow cannot bite;
//   * what depends on the voxel's 8-bit weight alone is not computed per voxel and frame: the multi-frame passes of the shipped parameters read
//     (float)w, (float)(w + 1), 1/(w + 1) and T = {new weight byte, "first observation" mask} as ONE 16-byte LDS record per voxel
//     (fill_weight_records, fuser_internal.h; fuse_update REC) -- no conversion, add, compare, select or saturating add per voxel;
//     every other variant keeps the float table of 1/m (RTAB).
// Every value stored is bit-identical to oracle/tsdf_oracle.c fuse_block.
// (v2f, pk_fma, splat, recip_rn, quot_rn live in fuser_internal.h: the device self-test in calib.hip runs the same code)

constexpr int RTAB = 512;  // LDS table of correctly rounded 1/m, m = weight + weight_sample < 512

// the per-frame / per-kernel constants the projection and the update multiply with (fuse_project, fuse_update).  They stay in the scalar registers they are
// loaded into: copying them into vector registers once per frame made the pass slower (plain pairs 808 -> 837 us: profiles/r05_integrate_ab.txt)
struct FrameV {
  float ti[12];
  float fx, fy, mx, my, tscale, tbase;
};
__device__ inline FrameV frame_constants(const ParamsK& P, const float* __restrict__ Ti) {
  FrameV F;
#pragma unroll
  for (int k = 0; k < 12; k++) F.ti[k] = Ti[k];
  F.fx = P.fx; F.fy = P.fy; F.mx = P.mx; F.my = P.my;
  F.tscale = P.tscale; F.tbase = P.tbase;
  return F;
}

__device__ inline int cvt_i32(float x) {  // v_cvt_i32_f32: truncates, saturates, NaN -> 0 (a C cast of NaN / inf would be undefined)
  int r;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// a + b saturating at 2^32 - 1: v_add_u32 with the VOP3 clamp bit (b in a scalar register: VOP3 takes no literal on gfx9)
__device__ inline uint32_t add_sat_u32(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_add_u32_e64 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "s"(b));
  return r;
}

// The producing instruction of a new voxel word, writing the tile register in place: called under `if (mask)`, i.e. with EXEC = the voxel's update mask
// (fuse_update).  Volatile: an asm the compiler may speculate is computed for every lane and selected afterwards.
__device__ inline void write_fma(uint32_t& dst, float a, float b, float c) {   // dst = fma(a, b, c)
  asm volatile("v_fma_f32 %0, %1, %2, %3" : "+v"(dst) : "v"(a), "v"(b), "v"(c));
}
__device__ inline void write_bfi(uint32_t& dst, uint32_t mask, uint32_t a, uint32_t b) {   // dst = (a & mask) | (b & ~mask); the mask in a scalar register
  asm volatile("v_bfi_b32 %0, %1, %2, %3" : "+v"(dst) : "s"(mask), "v"(a), "v"(b));
}

// weight_mode 1 (VoxelHashing): the weight of an observation falls with its depth; (uchar) of the float, at most 255
__device__ inline int depth_weight(const ParamsK& P, float d) {
  const float z01 = (d - P.dmin) / (P.dmax - P.dmin);
  const float wf = fmaxf(((float)P.wsample * 1.5f) * (1.0f - z01), 1.0f);
  return min(cvt_i32(wf), 255);   // saturating conversion: a masked lane's garbage depth cannot trap
}

// TAB: the weighted-mean division goes through the LDS reciprocal table (integrate with 1 <= weight_sample <= 256).
// Rows [J0, J0 + NJ) of the tile (a row = the 64 x 2 voxels one 16 B load per lane covers).  NJ = 4 gives the most
// independent work per issue slot, NJ = 2 called twice halves the live registers (single-frame, occupancy-bound variant).
// Phase A of one frame on rows [J0, J0 + NJ): camera-space z of the lane's voxel pairs, the pixel each voxel projects to
// (0 when it projects outside) and whether it projects inside.
// CLAMP: pixels that project outside read pixel 0 (callers that gather with plain global loads); without it the index of an outside
// voxel is whatever the saturating conversion gave (callers that gather through a bounds-checked buffer resource and mask by `ok`).
template <int J0, int NJ, bool CLAMP>
__device__ inline void fuse_project(const ParamsK& P, const FrameV& FV, v2f wx, float wy, const float (&wz)[4], v2f (&pz)[NJ],
                                    uint32_t (&pix)[2 * NJ], bool (&ok)[2 * NJ]) {
  const float* Ti = FV.ti;
  const uint32_t uw = (uint32_t)P.W, uh = (uint32_t)P.H;
  // Row constants first, two rows or two components per packed instruction:
  //      a{x,y}_j = fma(Ti[1|5], wy, fma(Ti[2|6], wz_j, Ti[3|7])),  az_j = fma(Ti[9], wy, fma(Ti[10], wz_j, Ti[11]))
  v2f axy[NJ], azz[NJ / 2];
#pragma unroll
  for (int j = 0; j < NJ; j++)
    axy[j] = pk_fma((v2f){Ti[1], Ti[5]}, splat(wy), pk_fma((v2f){Ti[2], Ti[6]}, splat(wz[J0 + j]), (v2f){Ti[3], Ti[7]}));
#pragma unroll
  for (int jj = 0; jj < NJ / 2; jj++)
    azz[jj] = pk_fma(splat(Ti[9]), splat(wy), pk_fma(splat(Ti[10]), (v2f){wz[J0 + 2 * jj], wz[J0 + 2 * jj + 1]}, splat(Ti[11])));
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const v2f pcx = pk_fma(splat(Ti[0]), wx, splat(axy[j].x));
    const v2f pcy = pk_fma(splat(Ti[4]), wx, splat(axy[j].y));
    const v2f pcz = pk_fma(splat(Ti[8]), wx, splat(azz[j >> 1][j & 1]));
    const v2f rz = recip_rn(pcz);
    const v2f uf = pk_add(pk_fma(pcx * splat(FV.fx), rz, splat(FV.mx)), splat(0.5f));
    const v2f vf = pk_add(pk_fma(pcy * splat(FV.fy), rz, splat(FV.my)), splat(0.5f));
    pz[j] = pcz;
#pragma unroll
    for (int hx = 0; hx < 2; hx++) {
      // pixel = (int)(u + 0.5f), THEN "skip if outside the image".  v_cvt_i32_f32 truncates towards zero like the C cast
      // ((-1, 0) -> pixel 0) and saturates, so "0 <= pixel < W" is ONE unsigned compare of the converted value
      const uint32_t px = (uint32_t)cvt_i32(uf[hx]), py = (uint32_t)cvt_i32(vf[hx]);
      const bool in = (pcz[hx] > 0.0f) && (px < uw) && (py < uh);
      const uint32_t p = __umul24(py, uw) + px;   // v_mad_u32_u24: exact for every inside pixel (py < H, W < 2^24), garbage outside
      ok[2 * j + hx] = in;
      pix[2 * j + hx] = CLAMP ? (in ? p : 0u) : p;
    }
  }
}

// The same projection for the X-ROW layout (XR): a lane holds the eight voxels of ONE x-row of the block -- y = lane & 7, z = lane >> 3, register pair j =
// voxels x = 2j, 2j + 1 -- instead of two x-neighbours in each of four z-layers.  Two things follow:
//   * the inner two fma of every camera-space coordinate, fma(Ti[1], wy, fma(Ti[2], wz, Ti[3])), depend on (y, z) only: ONE set per lane and frame instead of one
//     per z-row (6 fma instead of 24; the nesting -- hence every bit -- is the specification's);
//   * one gather instruction now reads the voxels of one x-plane of the block, 8 y x 8 z: 16 consecutive lanes (the unit the L1 coalesces) are 8 y x 2 z at one
//     x -- two image rows' worth of pixels for a level camera -- where the pair layout spread 4 x by 4 y over four or five rows.  The L1 tag pipeline was the
//     busiest unit of the pass (0.79-0.86 look-ups per CU and clock, 33.6 per gather instruction: profiles/r06_*).
template <int J0, int NJ>
__device__ inline void fuse_project_xr(const ParamsK& P, const FrameV& FV, const v2f (&wxp)[4], float wy, float wz, v2f (&pz)[NJ],
                                       uint32_t (&pix)[2 * NJ], bool (&ok)[2 * NJ]) {
  const float* Ti = FV.ti;
  const uint32_t uw = (uint32_t)P.W, uh = (uint32_t)P.H;
  const float ax = fmaf(Ti[1], wy, fmaf(Ti[2], wz, Ti[3]));
  const float ay = fmaf(Ti[5], wy, fmaf(Ti[6], wz, Ti[7]));
  const float az = fmaf(Ti[9], wy, fmaf(Ti[10], wz, Ti[11]));
#pragma unroll
  for (int j = 0; j < NJ; j++) pz[j] = pk_fma(splat(Ti[8]), wxp[J0 + j], splat(az));
  // "in front of the camera" once per lane: the lane's voxels differ in x only, wx rises along the row and fma rounds monotonically, so every pcz of the
  // row lies between the two end voxels' -- all are positive exactly when both ends are (a NaN az makes both ends NaN: the vote fails).  Two compares
  // and a wave vote instead of eight compares; only a wave the camera plane cuts (rare, wave-uniform) tests voxel by voxel.
  // (a ballot per compare: the ballot of an i1 that is not itself a compare costs a v_cndmask and a v_cmp)
  const bool front = (__ballot(pz[0].x > 0.0f) & __ballot(pz[NJ - 1].y > 0.0f)) == __ballot(1);
  bool zpos[2 * NJ];
#pragma unroll
  for (int k = 0; k < 2 * NJ; k++) zpos[k] = true;
  if (__builtin_expect(!front, 0)) {
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) zpos[k] = pz[k >> 1][k & 1] > 0.0f;
  }
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const v2f pcx = pk_fma(splat(Ti[0]), wxp[J0 + j], splat(ax));
    const v2f pcy = pk_fma(splat(Ti[4]), wxp[J0 + j], splat(ay));
    const v2f rz = recip_rn(pz[j]);
    const v2f uf = pk_add(pk_fma(pcx * splat(FV.fx), rz, splat(FV.mx)), splat(0.5f));
    const v2f vf = pk_add(pk_fma(pcy * splat(FV.fy), rz, splat(FV.my)), splat(0.5f));
#pragma unroll
    for (int hx = 0; hx < 2; hx++) {
      const uint32_t px = (uint32_t)cvt_i32(uf[hx]), py = (uint32_t)cvt_i32(vf[hx]);
      ok[2 * j + hx] = zpos[2 * j + hx] && (px < uw) && (py < uh);
      pix[2 * j + hx] = __umul24(py, uw) + px;
    }
  }
}

// Phase B: the update of DESIGN.md 3.5 from the gathered depths (colours) into the tile registers.
// WM (weight mode): 0 = any weight_sample / weight_max, 1 = weight_sample == 1, 2 = weight_sample == 1 and weight_max == 255 (the shipped
// parameters after the uchar clamp): the weight byte then increments with saturation as ONE add-with-carry on the {rgb, weight} word;
// 3 = the observation's weight depends on its depth (sf_params::weight_mode 1), otherwise as 0.
// dirty[j]: lane mask (a scalar register pair) of the lanes whose row j changed -- kept on the scalar unit across the frames of a batch.
// COLOR: 0 = geometry only, 1 = colour (every switch a wave-uniform mask), 2 = colour with colour_first == 0 compiled in.
// ROWS: dirty[] holds one lane mask per row (one frame per launch: the HBM-bound schedule writes back only the rows some lane changed); without
// it dirty[0] is a wave-uniform "some frame touched this tile" flag and the caller writes the whole tile back -- a ballot of an i1 that is not
// itself a compare costs a v_cndmask + v_cmp per row (8 VALU instructions on top of the 291 of a lane's RGB-D frame), and a pass of 32 frames is VALU-bound
// with HBM at 8 % of its peak.
// PRED: the shipped parameters write the new voxel under its update mask (below); false keeps the select tail for them too (k_reintegrate, whose two
// bodies leave no registers for the regions).
// REC: the constants of the update that depend on the voxel's weight alone come from `rec`, the LDS table of per-weight records (fill_weight_records,
// fuser_internal.h), read behind the early-out; rcp_m is not used then.  Only with the predicated write-back of the shipped parameters.
template <int SIGN, int COLOR, bool TAB, int WM, int J0, int NJ, bool ROWS = true, bool PRED = true, bool REC = false>
__device__ inline void fuse_update(const ParamsK& P, const FrameV& FV, const v2f (&rcp_m)[NJ], const float (&d)[2 * NJ], const uint32_t (&c)[2 * NJ], const v2f (&pz)[NJ],
                                   const bool (&ok)[2 * NJ], uint4 (&v)[4], uint64_t (&dirty)[4], const uint4* rec = nullptr) {
  static_assert(!REC || (PRED && SIGN > 0 && TAB && WM == 2), "the weight records serve the predicated write-back of the shipped parameters");
  constexpr bool WS1 = WM == 1 || WM == 2;
  // ---- phase B1: which voxels does this frame update?  Then a wave-uniform early-out: 10-25 % of the (block, frame) pairs the frustum
  // test lets through update nothing (blocks behind the surface, beyond the integration distance, over invalid depth, in the sliver
  // between the image border and the conservative sphere test) -- everything below (weighted mean, weights, selects: ~40 % of the
  // instructions of a frame) is skipped for them.  Measured on the configs[1] stream with the CPU checker: tools/waste.py.
  const float wn = (float)P.wsample;
  const uint32_t round_mask = P.colour_round ? 0x010101u : 0u;             // scalar registers
  const uint32_t first_mask = P.colour_first ? 0x00FFFFFFu : 0xFF000000u;
  constexpr bool wdep = WM == 3;   // depth-dependent observation weight (sf_params::weight_mode 1): its own instantiation, the generic path pays nothing for it
  v2f q[NJ], sdfc[NJ];
  v2f wnv[NJ];          // weight of this observation per voxel (a splat unless wdep)
  int wni[2 * NJ];
  uint32_t ncw[2 * NJ];
  bool upd[2 * NJ];
  bool sat[2 * NJ];
  bool any_upd = false;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const v2f dk = {d[2 * j], d[2 * j + 1]};
    v2f sdf = dk - pz[j];
    const v2f t = pk_fma(splat(FV.tscale), dk, splat(FV.tbase));
#pragma unroll
    for (int hx = 0; hx < 2; hx++) {
      // not behind the band.  No test of the depth itself: the pre-pass writes -inf for a pixel without a measurement, out of the sensor's range or at /
      // beyond the integration distance (a property of the pixel, gated once per pixel), and -inf fails this compare by itself --
      // t = fma(tscale, -inf, tbase) is -inf (NaN for tscale 0), sdf = -inf - pcz is -inf (NaN for pcz = -inf), and neither is greater than anything
      upd[2 * j + hx] = ok[2 * j + hx] && (sdf[hx] > -t[hx]);
      sdf[hx] = min_f32(sdf[hx], t[hx]);
      sat[2 * j + hx] = false;
      any_upd = any_upd || upd[2 * j + hx];
      wni[2 * j + hx] = wdep ? depth_weight(P, dk[hx]) : P.wsample;
    }
    wnv[j] = wdep ? (v2f){(float)wni[2 * j], (float)wni[2 * j + 1]} : splat(wn);
    sdfc[j] = sdf;
  }
  if (!__any((int)any_upd)) return;
  // ---- phase B2 of the shipped parameters (integration, table division, weight byte + 1 saturating at 255): no select between the new and the old
  // voxel.  upd[k] is a lane mask in a scalar register pair; the instruction that PRODUCES a new word -- the last fma of the quotient, the merge of
  // {rgb, weight} -- writes the tile register itself with EXEC = upd[k], one exec region per voxel (write_fma / write_bfi: volatile, so that the
  // compiler cannot compute them for every lane and select afterwards).  16 v_cndmask fewer per lane and frame with colour, 8 without: geometry only
  // keeps the select on the {rgb, weight} word, whose "weight already 255" carry has to be produced by an instruction either way.
  if constexpr (PRED && SIGN > 0 && TAB && WM == 2) {
    v2f q0[NJ], e[NJ];   // q = fma(e, r, q0) (quot_rn); its last fma is left to the write below
    v2f r[NJ];           // RN(1 / m)
    uint32_t T[2 * NJ];  // REC with colour: word .w of the voxel's record
    bool tiny = false;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      v2f wo, m;
      if constexpr (REC) {
        // everything here that depends on the weight alone is one LDS read per voxel: no conversion, no add, and for colour no compare, select or
        // saturating add below (geometry only reads 12 bytes: its weight word keeps the carry logic)
        const uint4* ra = rec + (v[J0 + j].y >> 24);
        const uint4* rb = rec + (v[J0 + j].w >> 24);
        wo = (v2f){__uint_as_float(ra->x), __uint_as_float(rb->x)};
        m = (v2f){__uint_as_float(ra->y), __uint_as_float(rb->y)};
        r[j] = (v2f){__uint_as_float(ra->z), __uint_as_float(rb->z)};
        if (COLOR) { T[2 * j] = ra->w; T[2 * j + 1] = rb->w; }
      } else {
        wo = (v2f){(float)(v[J0 + j].y >> 24), (float)(v[J0 + j].w >> 24)};
        m = wo + splat(wn);             // wn == 1.0f, as a run-time value: one add, not a second conversion
        r[j] = rcp_m[j];
      }
      const v2f old = {__uint_as_float(v[J0 + j].x), __uint_as_float(v[J0 + j].z)};
      const v2f n = pk_fma(old, wo, sdfc[j]);   // weight_sample == 1: sdf * 1.0f == sdf bit for bit
      q0[j] = n * r[j];
      e[j] = pk_fma(-m, q0[j], n);
      tiny = tiny || (fabsf(n.x) < 0x1p-100f) || (fabsf(n.y) < 0x1p-100f);
    }
    if (__builtin_expect(__any((int)tiny) != 0, 0)) {
      // some numerator of the wave is in the underflow range (practically: never): the plain IEEE quotient q, handed to the same write as
      // fma(-0, r, q) = q + (-0) = q for every q, the zeros' signs included.  (ONE write-back body: a second one for this case met the first at the
      // loop's end with the tile in other registers, and the live path copied the tile aside and back -- 32 v_mov per frame.)
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const v2f wo = {(float)(v[J0 + j].y >> 24), (float)(v[J0 + j].w >> 24)};
        const v2f old = {__uint_as_float(v[J0 + j].x), __uint_as_float(v[J0 + j].z)};
        const v2f n = pk_fma(old, wo, sdfc[j]);
        const v2f m = wo + splat(wn);
        q0[j] = (v2f){n.x / m.x, n.y / m.y};
        e[j] = splat(-0.0f);
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) {
#pragma unroll
      for (int hx = 0; hx < 2; hx++) {
        const int k = 2 * j + hx;
        uint32_t& sdf_word = hx ? v[J0 + j].z : v[J0 + j].x;
        uint32_t& cw_word = hx ? v[J0 + j].w : v[J0 + j].y;
        const uint32_t cw = cw_word;
        uint32_t rgb = cw, wsum = 0u;
        bool keep = false;   // geometry only: the weight is 255 already, the word stays
        if (COLOR) {
          // the blend of the generic path below (v_lerp_u8; "first observation" by the weight byte or the colour_first mask)
          const uint32_t ck = c[k];
          const uint32_t avg = __builtin_amdgcn_lerp(cw, ck, round_mask);
          if (REC && COLOR == 2) {
            rgb = (ck & T[k]) | (avg & ~T[k]);   // one bit select: the low 24 bits of T are set exactly on a first observation
          } else {
            const bool first = COLOR == 2 ? cw < 0x01000000u : (cw & first_mask) == 0u;   // colour_first: by the colour bytes, not by the weight
            rgb = first ? ck : avg;
          }
          wsum = REC ? T[k] : add_sat_u32(cw, 0x01000000u);   // 0xFFFFFFFF exactly when the weight was 255; only byte 3 is kept (of T: the new weight)
        } else {
          keep = __builtin_add_overflow(cw, 0x01000000u, &wsum);
        }
        if (upd[k]) {
          write_fma(sdf_word, e[j][hx], r[j][hx], q0[j][hx]);
          if (COLOR) write_bfi(cw_word, 0x00FFFFFFu, rgb, wsum);
        }
        if (!COLOR) cw_word = (upd[k] && !keep) ? wsum : cw_word;
      }
      if (ROWS) dirty[J0 + j] |= __ballot(upd[2 * j] || upd[2 * j + 1]);
    }
    if (!ROWS) dirty[0] = ~0ull;
    return;
  }
  // ---- phase B2, every other variant: new values into temporaries (the tile itself stays untouched until the end)
  bool slow = false;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const v2f sdf = sdfc[j];
    const uint32_t cwj[2] = {v[J0 + j].y, v[J0 + j].w};
    const v2f wo = {(float)(cwj[0] >> 24), (float)(cwj[1] >> 24)};
    const v2f old = {__uint_as_float(v[J0 + j].x), __uint_as_float(v[J0 + j].z)};
    if (SIGN > 0) {
      const v2f n = pk_fma(old, wo, WS1 ? sdf : sdf * wnv[j]);  // x * 1.0f == x bit for bit
      const v2f m = wo + wnv[j];
      if (TAB) {
        q[j] = quot_rn(n, m, rcp_m[j]);
        slow = slow || (fabsf(n.x) < 0x1p-100f) || (fabsf(n.y) < 0x1p-100f);
      } else {
        q[j] = (v2f){n.x / m.x, n.y / m.y};
      }
#pragma unroll
      for (int hx = 0; hx < 2; hx++) {
        const uint32_t cw = cwj[hx];
        const uint32_t w = cw >> 24;
        uint32_t rgb = cw;   // bytes 0..2 = the accumulated colour (byte 3, the weight, is masked out where the word is assembled)
        if (COLOR) {
          // (a + b) / 2 per channel (integer division) is ONE instruction on this ISA: v_lerp_u8 D = per byte (S0 + S1 + S2[bit 0 of the
          // byte]) >> 1 -- the sum is formed in 9 bits, nothing crosses a byte.  colour_round 1 (combineVoxel upstream, DESIGN 6b:
          // (uchar)(0.5f a + 0.5f b + 0.5f) = (a + b + 1) >> 1) is the same instruction with bit 0 of every colour byte of S2 set.  The weight byte
          // of the result is garbage and never used.  colour_first 1: "first observation" is a black accumulated colour instead of a zero weight --
          // a wave-uniform mask on the word, not a branch.  (Round 3 spent 12 VALU instructions per voxel on this blend: xor / and / shift / add3.)
          const uint32_t ck = c[2 * j + hx];
          const uint32_t avg = __builtin_amdgcn_lerp(cw, ck, round_mask);
          // COLOR 2 (colour_first == 0, the shipped semantics): "no observation yet" = the weight byte is zero = the word is below 2^24 -- one compare
          // against a literal instead of a mask and a compare
          const bool first = COLOR == 2 ? cw < 0x01000000u : (cw & first_mask) == 0u;
          rgb = first ? ck : avg;
        }
        if (WM == 2) {
          if (COLOR) {
            // weight byte + 1 saturating at 255: an unsigned add with the clamp bit on the whole word saturates to 0xFFFFFFFF exactly when the
            // weight was 255; only byte 3 of the sum is kept
            ncw[2 * j + hx] = (rgb & 0x00FFFFFFu) | (add_sat_u32(cw, 0x01000000u) & 0xFF000000u);
          } else {
            // without colour "keep the word at 255" is "do not touch the word": the carry of the add folds into the final select
            uint32_t inc;
            const bool full = __builtin_add_overflow(cw, 0x01000000u, &inc);
            ncw[2 * j + hx] = inc;
            sat[2 * j + hx] = full;
          }
        } else {
          uint32_t nw = w + (uint32_t)wni[2 * j + hx];
          if (nw > (uint32_t)P.wmax) nw = (uint32_t)P.wmax;
          ncw[2 * j + hx] = (rgb & 0x00FFFFFFu) | (nw << 24);
        }
      }
    } else {
      const v2f n = pk_fma(old, wo, -(sdf * wnv[j]));
      const v2f m = wo - wnv[j];
      q[j] = (v2f){n.x / m.x, n.y / m.y};  // discarded when the weight drops to <= 0 (then m <= 0)
#pragma unroll
      for (int hx = 0; hx < 2; hx++) {
        const int nw = (int)(cwj[hx] >> 24) - wni[2 * j + hx];
        if (nw <= 0) { q[j][hx] = __uint_as_float(0u); ncw[2 * j + hx] = 0u; }
        else ncw[2 * j + hx] = (cwj[hx] & 0xFFFFFFu) | ((uint32_t)nw << 24);
      }
    }
  }
  if (SIGN > 0 && TAB && __builtin_expect(__any((int)slow), 0)) {
    // some numerator of the wave is in the underflow range (practically: never): plain IEEE division for this tile
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const v2f wo = {(float)(v[J0 + j].y >> 24), (float)(v[J0 + j].w >> 24)};
      const v2f old = {__uint_as_float(v[J0 + j].x), __uint_as_float(v[J0 + j].z)};
      const v2f n = pk_fma(old, wo, sdfc[j] * wnv[j]);
      const v2f m = wo + wnv[j];
      q[j] = (v2f){n.x / m.x, n.y / m.y};
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    v[J0 + j].x = upd[2 * j] ? __float_as_uint(q[j].x) : v[J0 + j].x;
    v[J0 + j].y = (upd[2 * j] && !sat[2 * j]) ? ncw[2 * j] : v[J0 + j].y;
    v[J0 + j].z = upd[2 * j + 1] ? __float_as_uint(q[j].y) : v[J0 + j].z;
    v[J0 + j].w = (upd[2 * j + 1] && !sat[2 * j + 1]) ? ncw[2 * j + 1] : v[J0 + j].w;
    if (ROWS) dirty[J0 + j] |= __ballot(upd[2 * j] || upd[2 * j + 1]);
  }
  if (!ROWS) dirty[0] = ~0ull;   // reached only when some lane of the wave updates a voxel (the early-out above)
}


// The depth (colour) image of one frame as a buffer resource: gathers address it as SGPR descriptor + 32-bit VGPR byte offset (one
// v_mul_u32_u24 + one v_lshl_add_u32 per voxel instead of a 64-bit multiply-add, a select and a 64-bit shift-add), and an offset past
// the image -- a voxel that projects outside, whose index is garbage -- reads 0 instead of faulting; such voxels are masked by `ok`.
__device__ inline __amdgpu_buffer_rsrc_t image_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);   // raw buffer, dword data format (gfx9)
}

// REC: rtab is the table of per-weight records (256 x uint4) instead of the float table, read by fuse_update
template <int SIGN, int COLOR, bool TAB, int WM, int J0, int NJ, bool ROWS, bool XR = false, bool PRED = true, bool REC = false>
__device__ inline void fuse_rows(const ParamsK& P, const float* __restrict__ Ti, const float* __restrict__ depthf,
                                 const uint2* __restrict__ texel, const float* rtab, v2f wx, float wy, const float (&wz)[4], const v2f (&wxp)[4],
                                 uint4 (&v)[4], uint64_t (&dirty)[4]) {
  v2f pz[NJ], rcp_m[NJ];
  float d[2 * NJ];
  uint32_t c[2 * NJ];
  bool ok[2 * NJ];
  uint32_t pix[2 * NJ];
  // the weights are known before anything else: start the eight table reads now, they are consumed in phase B
  if (TAB && !REC) {
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      // weight_sample == 1 in the shipped parameters (WM >= 1): a constant index offset folds into the LDS instruction's immediate
      const uint32_t ws = (WM == 1 || WM == 2) ? 1u : (uint32_t)P.wsample;
      rcp_m[j] = (v2f){rtab[(v[J0 + j].y >> 24) + ws], rtab[(v[J0 + j].w >> 24) + ws]};
    }
  }
  // ---- phase A: project; then the gathers, all issued together
  const FrameV FV = frame_constants(P, Ti);
  if (XR) fuse_project_xr<J0, NJ>(P, FV, wxp, wy, wz[0], pz, pix, ok);   // wz[0]: the lane's one z
  else fuse_project<J0, NJ, false>(P, FV, wx, wy, wz, pz, pix, ok);
  const uint32_t img_bytes = (uint32_t)(P.W * P.H) * 4u;
  if (COLOR) {
    // RGB-D: depth and colour of a pixel sit side by side in the pre-pass's texel plane -- one 8-byte gather per voxel (two 4-byte gathers into
    // two planes were 16 requests per lane and frame; the texture-address unit, not the vector ALU, was the busier one)
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const __amdgpu_buffer_rsrc_t rt = image_rsrc(texel, 2u * img_bytes);
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) {
      const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rt, pix[k] << 3, 0, 0);
      d[k] = __uint_as_float(t.x);
      c[k] = t.y;
    }
  } else {
    const __amdgpu_buffer_rsrc_t rd = image_rsrc(depthf, img_bytes);
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) d[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rd, pix[k] << 2, 0, 0));
  }
  fuse_update<SIGN, COLOR, TAB, WM, J0, NJ, ROWS, PRED, REC>(P, FV, rcp_m, d, c, pz, ok, v, dirty, reinterpret_cast<const uint4*>(rtab));
}

}  // namespace
