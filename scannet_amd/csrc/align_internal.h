// align_internal.h -- what the two files of the global alignment share: align.hip (the depth term's kernels and the host's Gauss-Newton loop) and
// align_colour.hip (the colour term's kernels): the pair table's row, the fuser's alignment work set and the colour side's two launchers
#pragma once
#include "fuser_internal.h"
#include "hip_util.h"
#include "scanfuse.h"
#include "track_math.h"

constexpr int AL_NSYS_RGBD = 31;   // the 29 values of track_math.h, then the colour term's sum r_c^2 and count

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
};

// align_colour.hip, both queued on f->stream.  The intensity and gradient maps of K pictures at `level` into w->photo:
int sf_photo_prepare(sf_fuser* f, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K, int level, const tk::Cam& cam);
// the P pairs' 31-value systems from the maps and w->d_table into w->d_sys; with_photo false: no colour rows (the depth term's bits, the colour sums 0)
int sf_photo_systems(sf_fuser* f, uint64_t P, const tk::Cam& cam, const sf_align_params* a, bool with_photo);
