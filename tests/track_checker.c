/*
 * tests/track_checker.c -- CPU restatement of the camera tracker, with the dense colour term optional (DESIGN.md sections 4c "Camera tracking" and
 * 4g "The colour term of the tracker"; scannet_amd/csrc/track.hip and track_colour.hip are the GPU side).
 *
 * Takes the model as the ray caster makes it (depth, world normals and, for the colour term, RGB8 colour at the integration size, cast at T_ref:
 * tests/raycast_checker.c on the CPU) and the frame's depth and RGB8 picture, builds the input pyramid and the two intensity pyramids, associates,
 * reduces the 31 values in the kernel's order and solves on the host as the library does, on the first 29 of them.  The rules themselves are
 * tests/solver_rules.h's; what is here is the tracker's own: its model, its pyramids and its host loop.  The frame's picture and the model's colour
 * may be NULL: no colour rows are formed, values 29 and 30 are 0 and the first 29 are the depth term's, as they are at colour_weight 0.
 */
#include "solver_rules.h"

#define TK_MAX_LEVELS 4

/* sf_track_params through the colour term's three fields */
typedef struct tk_params {
  int32_t levels;
  int32_t max_iters[4];
  float dist_thres[4];
  float normal_thres[4];
  float early_out;
  int32_t min_correspondences;
  float max_translation, max_rotation;
  int32_t raycast[16];           /* sf_raycast_params: the caller casts the model      */
  float colour_weight, colour_thres, colour_gradient_min;
} tk_params;

/* the leading fields of sf_track_result */
typedef struct tk_result {
  int32_t tracked, iterations[4], correspondences;
  float rms_residual;
  int32_t lost_reason;
  int32_t colour_correspondences;
  float colour_rms_residual;
} tk_result;

typedef struct {
  int levels;
  cam_t cam[TK_MAX_LEVELS];
  f3 *v[TK_MAX_LEVELS], *n[TK_MAX_LEVELS];   /* x = -inf: invalid */
  f3 *mq, *mn;                                /* the model, level 0 */
  f3 *pin[TK_MAX_LEVELS], *pm[TK_MAX_LEVELS]; /* {I, gx, gy} of the frame and of the model per level (-inf: invalid); NULL: no picture */
} state_t;

static void state_free(state_t* s) {
  for (int l = 0; l < TK_MAX_LEVELS; l++) { free(s->v[l]); free(s->n[l]); free(s->pin[l]); free(s->pm[l]); }
  free(s->mq);
  free(s->mn);
}

/* the {I, gx, gy} maps of every level from a level-0 intensity image d (taken over and freed) */
static void photo_pyramid(const state_t* s, float* d, f3** out) {
  for (int l = 0; l < s->levels; l++) {
    const cam_t* c = &s->cam[l];
    if (l > 0) {
      float* e = photo_down(d, s->cam[l - 1].W, s->cam[l - 1].H);
      free(d);
      d = e;
    }
    out[l] = (f3*)malloc(sizeof(f3) * c->W * c->H);
    photo_map(c, d, out[l]);
  }
  free(d);
}

static int model_valid(const float* md, const float* mnrm, int i) { return md[i] > 0.0f && mnrm[3 * i] > -INFINITY; }

/* -1: a level smaller than 8 x 8.  rgb (with mrgb, the model's colour) may be NULL: no colour rows */
static int state_build(state_t* s, const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, const float* md, const float* mnrm, const uint8_t* mrgb,
                       const tk_params* t, const float* Tref) {
  memset(s, 0, sizeof(*s));
  s->levels = t->levels;
  for (int l = 0; l < t->levels; l++)
    if (!level_cam(fr, l, &s->cam[l])) return -1;
  float* d = prepass_depth(fr, depth);
  for (int l = 0; l < t->levels; l++) {
    const cam_t* c = &s->cam[l];
    if (l > 0) {
      float* e = down4(d, s->cam[l - 1].W, s->cam[l - 1].H);
      free(d);
      d = e;
    }
    s->v[l] = (f3*)malloc(sizeof(f3) * c->W * c->H);
    s->n[l] = (f3*)malloc(sizeof(f3) * c->W * c->H);
    vertex_normal_maps(c, d, s->v[l], s->n[l]);
  }
  free(d);
  const cam_t* c0 = &s->cam[0];
  const int npx = c0->W * c0->H;
  s->mq = (f3*)malloc(sizeof(f3) * npx);
  s->mn = (f3*)malloc(sizeof(f3) * npx);
  for (int i = 0; i < npx; i++) {
    const f3 inv = {-INFINITY, -INFINITY, -INFINITY};
    s->mq[i] = inv;
    s->mn[i] = inv;
    if (model_valid(md, mnrm, i)) {
      s->mq[i] = xf(Tref, unproject(c0, i % c0->W, i / c0->W, md[i]));
      s->mn[i].x = mnrm[3 * i]; s->mn[i].y = mnrm[3 * i + 1]; s->mn[i].z = mnrm[3 * i + 2];
    }
  }
  if (rgb) {   /* the frame's picture and the model's rendered colour (valid where the model pixel is: a miss is not black) as pyramids */
    photo_pyramid(s, prepass_intensity(fr, rgb), s->pin);
    float* m = (float*)malloc(sizeof(float) * npx);
    for (int i = 0; i < npx; i++) m[i] = model_valid(md, mnrm, i) ? intensity_rgb8(mrgb + 3 * (size_t)i) : -INFINITY;
    photo_pyramid(s, m, s->pm);
  }
  return 0;
}

/* one pixel's 31 values; 1 when it is a (depth) correspondence.  rc, Jc (may be NULL): the colour row, when acc[30] is 1 */
static int pixel_row(const state_t* s, int l, int i, const float* Tf, const float* M, const float* Rf, const tk_params* t, float* acc, float* rc_out,
                     float* Jc_out) {
  const cam_t* c = &s->cam[l];
  const f3 v = s->v[l][i], nc = s->n[l][i];
  if (!(v.z > 0.0f && nc.x > -INFINITY)) return 0;
  const f3 p = xf(Tf, v), n = rot(Tf, nc), pc = xf(M, v);
  int ux, uy;
  if (!project_nearest(c, pc, &ux, &uy)) return 0;
  const size_t j = (size_t)(uy << l) * s->cam[0].W + (ux << l);
  const f3 q = s->mq[j];
  if (!(q.x > -INFINITY)) return 0;
  if (!plane_row(p, n, q, s->mn[j], t->dist_thres[l], t->normal_thres[l], acc)) return 0;
  float rc, Jc[6];
  if (s->pin[l] && colour_row(s->pin[l][i].x, s->pm[l], c, pc, p, Rf, t->colour_thres, t->colour_gradient_min, &rc, Jc)) {
    add_colour_row(acc, t->colour_weight, rc, Jc);
    if (rc_out) { *rc_out = rc; memcpy(Jc_out, Jc, sizeof(Jc)); }
  }
  return 1;
}

static void system_at(const state_t* s, int l, const double* T, const double* Tref, const tk_params* t, double* sys, uint8_t* mask) {
  float Tf[12], M[12], Rf[12];
  for (int i = 0; i < 12; i++) { Tf[i] = (float)T[i]; Rf[i] = (float)Tref[i]; }
  compose_ref(Tref, T, M);
  const int npx = s->cam[l].W * s->cam[l].H, nb = (npx + 255) / 256;
  double tot[SR_NSYS] = {0};
  static float lane[256][SR_NSYS];
  for (int b = 0; b < nb; b++) {
    memset(lane, 0, sizeof(lane));
    for (int tid = 0; tid < 256; tid++) {
      const int i = b * 256 + tid;
      if (i >= npx) continue;
      const int ok = pixel_row(s, l, i, Tf, M, Rf, t, lane[tid], NULL, NULL);
      if (mask) mask[i] = (uint8_t)ok;
    }
    reduce_block(lane, tot);
  }
  memcpy(sys, tot, sizeof(tot));
}

static int solve6(const double* sys, double* xi) {
  double A[6][6];
  unpack_sym6(sys, A);
  return cholesky_solve(&A[0][0], sys + 21, 6, xi);
}

static int args_ok(const tk_params* t, const uint8_t* rgb) { return colour_args_ok(rgb != NULL, t->colour_weight, t->colour_thres, t->colour_gradient_min); }

/* One level's 31-value system at T (the library's sf_fuser_track_system and sf_fuser_track_rgbd_system).  rgb: the frame's picture, mrgb: the model's
 * rendered colour; both NULL: no colour rows.  -1: a level below 8 x 8 or a colour argument the library refuses. */
int tk_system(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, const float* md, const float* mnrm, const uint8_t* mrgb, const tk_params* t,
              int level, const float* T, const float* Tref, double* sys, uint8_t* mask) {
  state_t s;
  if (!args_ok(t, rgb)) return -1;
  if (state_build(&s, fr, depth, rgb, md, mnrm, mrgb, t, Tref) != 0) { state_free(&s); return -1; }
  double Td[12], Rd[12];
  for (int i = 0; i < 12; i++) { Td[i] = T[i]; Rd[i] = Tref[i]; }
  system_at(&s, level, Td, Rd, t, sys, mask);
  state_free(&s);
  return 0;
}

/* The maps of a level for the tests: vmap npx x 3 floats (the frame's camera-space vertices), pmap npx x 3 floats {I, gx, gy} of the model; cam_out: W, H
 * as floats, fx, fy, mx, my */
int tk_maps(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, const float* md, const float* mnrm, const uint8_t* mrgb, const tk_params* t, int level,
            const float* Tref, float* vmap, float* pmap, float* cam_out) {
  state_t s;
  if (!rgb) return -1;
  if (state_build(&s, fr, depth, rgb, md, mnrm, mrgb, t, Tref) != 0) { state_free(&s); return -1; }
  const cam_t* c = &s.cam[level];
  memcpy(vmap, s.v[level], sizeof(f3) * c->W * c->H);
  memcpy(pmap, s.pm[level], sizeof(f3) * c->W * c->H);
  cam_out[0] = (float)c->W; cam_out[1] = (float)c->H; cam_out[2] = c->fx; cam_out[3] = c->fy; cam_out[4] = c->mx; cam_out[5] = c->my;
  state_free(&s);
  return 0;
}

/* The colour rows of a level at T for the tests: rows npx x 8 floats {has a colour row, r_c, J_c[6]}, zeros elsewhere */
int tk_rows(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, const float* md, const float* mnrm, const uint8_t* mrgb, const tk_params* t, int level,
            const float* T, const float* Tref, float* rows) {
  state_t s;
  if (!rgb) return -1;
  if (state_build(&s, fr, depth, rgb, md, mnrm, mrgb, t, Tref) != 0) { state_free(&s); return -1; }
  double Td[12], Rd[12];
  float Tf[12], Rf[12], M[12];
  for (int k = 0; k < 12; k++) { Td[k] = Tf[k] = T[k]; Rd[k] = Rf[k] = Tref[k]; }
  compose_ref(Rd, Td, M);
  const int npx = s.cam[level].W * s.cam[level].H;
  memset(rows, 0, sizeof(float) * 8 * npx);
  for (int px = 0; px < npx; px++) {
    float acc[SR_NSYS] = {0};
    float* o = rows + 8 * (size_t)px;
    if (pixel_row(&s, level, px, Tf, M, Rf, t, acc, o + 1, o + 2)) o[0] = acc[30];
  }
  state_free(&s);
  return 0;
}

/* The whole track (sf_fuser_track and sf_fuser_track_rgbd) with the model ray-cast at ref (NULL: the guess).  -1: a level below 8 x 8 or a colour
 * argument the library refuses. */
int tk_track(const sr_frame* fr, const uint16_t* depth, const uint8_t* rgb, const float* md, const float* mnrm, const uint8_t* mrgb, const tk_params* t,
             const float* guess, const float* ref, float* pose_out, tk_result* res) {
  if (!args_ok(t, rgb)) return -1;
  tk_result r;
  memset(&r, 0, sizeof(r));
  for (int i = 0; i < 16; i++) pose_out[i] = -INFINITY;
  if (!ref) ref = guess;
  if (!finite12(guess) || !finite12(ref)) {
    r.lost_reason = 1;
    *res = r;
    return 0;
  }
  state_t s;
  if (state_build(&s, fr, depth, rgb, md, mnrm, mrgb, t, ref) != 0) { state_free(&s); return -1; }
  double T[12], Tref[12], G[12], sys[SR_NSYS];
  for (int i = 0; i < 12; i++) { T[i] = guess[i]; G[i] = guess[i]; Tref[i] = ref[i]; }
  for (int l = t->levels - 1; l >= 0 && r.lost_reason == 0; l--) {
    for (int it = 0; it < t->max_iters[l]; it++) {
      system_at(&s, l, T, Tref, t, sys, NULL);
      if (l == 0) {
        r.correspondences = (int32_t)sys[28];
        r.rms_residual = rms_of(sys[27], sys[28]);
        r.colour_correspondences = (int32_t)sys[30];
        r.colour_rms_residual = rms_of(sys[29], sys[30]);
        if (sys[28] < (double)t->min_correspondences) { r.lost_reason = 2; break; }
      }
      double xi[6];
      if (!solve6(sys, xi)) { r.lost_reason = 3; break; }
      apply_update(xi, T);
      r.iterations[l]++;
      if (max_abs(xi, 6) < (double)t->early_out) break;
    }
  }
  state_free(&s);
  if (r.lost_reason == 0 && !motion_ok(G, T, t->max_translation, t->max_rotation)) r.lost_reason = 4;
  if (r.lost_reason == 0) {
    r.tracked = 1;
    write_pose(T, pose_out);
  }
  *res = r;
  return 0;
}
