// align_internal.h -- what the two files of the global alignment share: align.hip (the depth term's kernels and the host's Gauss-Newton loop) and
// align_colour.hip (the colour term's kernels): the pair table's row, the fuser's alignment work set and the colour side's launcher
#pragma once
#include "fuser_internal.h"
#include "hip_util.h"
#include "scanfuse.h"
#include "align_solve.h"
#include "track_math.h"

struct AlignPair {   // one row of the device table; read through the scalar unit (the index is blockIdx.y)
  int32_t i, j, active, pad;
  tk::Rows Ti, Tj, M;    // source pose, target pose, T_j^-1 T_i
};

struct AlignWork {   // every buffer grows on demand and never shrinks
  sf::DevBuf d_in;             // u8: host frames' device copy
  sf::DevBuf d_rgb;            // u8: host colour pictures' device copy
  sf::DevBuf vmap, nmap;       // float4 [K][npx]
  sf::DevBuf photo;            // float4 [K][npx] {intensity, gx, gy, 0} (sf_fuser_align_rgbd*)
  sf::DevBuf partials;         // float [P][nb][32]
  sf::DevBuf d_table;          // AlignPair [P]
  sf::HostBuf h_table;         // page-locked
  sf::DevBuf d_sys;            // double [P][29 or 31]
  sf::HostBuf h_sys;           // page-locked read-back
  // sf_fuser_align_groups_device (align_scan.hip)
  sf::DevBuf d_group;          // the groups' descriptions, local pair lists and running list
  sf::HostBuf h_group;
  sf::DevBuf d_record;         // als::GroupOut per running group
  sf::HostBuf h_record;
};

struct AlignJob {   // one call's frames, level and pair list
  const void* d_depth;   // the K frames in HBM, stride bytes apart
  uint64_t stride;
  uint64_t K, P;
  const int32_t* pairs = nullptr;
  int level;
  tk::Cam cam;
  float dmin, dmax;
  int nsys = tk::TK_NSYS;        // values per pair: 29, or 31 through sf_fuser_align_rgbd* (align_colour.hip's kernels)
  const void* d_rgb = nullptr;   // the K colour pictures in HBM, rgb_stride bytes apart; nullptr: none
  uint64_t rgb_stride = 0;
  const int32_t* remap = nullptr;   // frame k of the call is frame remap[k] of the maps (align_scan.hip: the top of a scan); nullptr: k itself
  bool maps_ready = false;          // the maps are in w->vmap / nmap / photo already
};

// align.hip, for align_scan.hip: the parameter checks, the set-up behind them, the maps, one row of the pair table, the kernels over a range of its
// rows, and the whole solve of the job's pair list (sf_fuser_align*'s own loop)
int sf_align_check_params(const sf_align_params* a);
int sf_align_begin(sf_fuser* f, const void* depth, bool on_device, uint64_t stride, bool out_ok, uint64_t K, uint64_t P, uint64_t chunk, const sf_align_params* a,
                   AlignJob* j, bool rgbd, const void* rgb, uint64_t rgb_stride);
int sf_align_prepare(sf_fuser* f, const AlignJob& j);
void sf_align_pair_row(AlignPair* e, int32_t fi, int32_t fj, bool active, const double* Ti, const double* Tj);
int sf_align_systems(sf_fuser* f, const AlignJob& j, const sf_align_params* a, uint64_t first, uint64_t count);
int sf_align_solve(sf_fuser* f, const AlignJob& j, const float* poses_in, const sf_align_params* a, float* poses_out, sf_align_result* res);

// align_colour.hip, queued on f->stream: the intensity and gradient maps of K pictures at `level` into w->photo
int sf_photo_prepare(sf_fuser* f, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K, int level, const tk::Cam& cam);
