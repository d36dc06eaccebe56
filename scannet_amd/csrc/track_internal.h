// track_internal.h -- what the two files of the camera tracker share: track.hip (the depth term's kernels and the host's Gauss-Newton loop) and
// track_colour.hip (the colour term's kernels): the fuser's tracking work set and the colour side's launchers
#pragma once
#include "fuser_internal.h"
#include "hip_util.h"
#include "scanfuse.h"
#include "track_math.h"

struct TrackWork {
  int levels = 0;
  sf::DevBuf d_in;                            // u16: a host frame's device copy
  sf::DevBuf depth[tk::TK_MAX_LEVELS];        // float: metres per level
  sf::DevBuf vmap[tk::TK_MAX_LEVELS], nmap[tk::TK_MAX_LEVELS];   // float4
  sf::DevBuf model_depth, model_normal;       // float, 3 floats: the ray cast at level-0 size
  sf::DevBuf mq, mn;                          // float4: world vertices and normals of the model
  sf::DevBuf partials;                        // float
  sf::DevBuf d_sys;                           // double
  sf::HostBuf h_sys;                          // double: page-locked read-back
  sf::DevBuf d_mask;                          // u8
  // the colour term (sf_fuser_track_rgbd*): made on first colour use for `photo_levels` levels, again when more are asked for
  int photo_levels = 0;
  sf::DevBuf d_rgb;                           // u8: a host picture's device copy
  sf::DevBuf model_rgb;                       // u8 x 3: the ray cast's colour image
  sf::DevBuf inten[2][tk::TK_MAX_LEVELS];     // float: intensity per level, [0] the frame's, [1] the model's
  sf::DevBuf photo[2][tk::TK_MAX_LEVELS];     // float4 {I, gx, gy, 0} per level
};

// the colour pictures the fuser fuses: color_width x color_height, or the integration size
inline size_t sf_track_picture_bytes(const sf_fuser* f) { return (f->pk.cW ? (size_t)f->pk.cW * f->pk.cH : (size_t)f->pk.W * f->pk.H) * 3; }

// track_colour.hip.  The colour buffers of `levels` levels in f->track (which exists):
int sf_track_photo_reserve(sf_fuser* f, const tk::Cam* cams, int levels);
// queued on f->stream behind the model's ray cast (depth, normals and colour in f->track): the {I, gx, gy, 0} maps of every level of the picture
// d_rgb and of the model
int sf_track_photo_prepare(sf_fuser* f, const void* d_rgb, const tk::Cam* cams, int levels);
