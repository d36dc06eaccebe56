/*
 * tests/freespace_checker.c -- CPU checker of the free-space stage.  TEST INFRASTRUCTURE ONLY.
 *
 * A dense restatement of the integrate rule (oracle/tsdf_oracle.c fuse_block states the same operations per allocated block): for
 * EVERY voxel of a given box and every frame in order, the frame's update, one individually rounded binary32 operation after the other.  Its own
 * arrays, no hash table, no block test: a voxel is "known" here exactly when some frame's rule updated it, whichever blocks a fuser allocates.
 * Beside it the two dense export modes and a restatement of the stage's plan (which box can a scan update at all), both in their own words.
 *
 * Compile with -ffp-contract=off and -mfma: fmaf() marks the places where the rule asks for a fused multiply-add (tests/test_freespace.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  int32_t width, height;          /* the INTEGRATION image (a test that resamples does so before it calls) */
  float fx, fy, mx, my;           /* ... and its intrinsics */
  float depth_shift, depth_min, depth_max;
  float voxel_size, trunc_base, trunc_scale, max_integration_dist;
  int32_t weight_sample, weight_max, weight_mode, weight_wrap;
} fc_params;

typedef struct {
  fc_params p;
  int32_t lo[3], dims[3];         /* the box, global voxel indices */
  float* sdf;                     /* [z][y][x] */
  uint8_t* w;
  float* depthf;
} fc_volume;

fc_volume* fc_create(const fc_params* p, const int32_t lo[3], const int32_t dims[3]) {
  if (!p || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || p->width <= 0 || p->height <= 0) return NULL;
  fc_volume* v = (fc_volume*)calloc(1, sizeof(fc_volume));
  if (!v) return NULL;
  v->p = *p;
  if (v->p.weight_max > 255 && !v->p.weight_wrap) v->p.weight_max = 255;   /* a uchar weight saturates */
  if (v->p.weight_max < 1) v->p.weight_max = 1;
  const size_t n = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
  for (int a = 0; a < 3; a++) { v->lo[a] = lo[a]; v->dims[a] = dims[a]; }
  v->sdf = (float*)calloc(n, sizeof(float));
  v->w = (uint8_t*)calloc(n, 1);
  v->depthf = (float*)malloc((size_t)p->width * (size_t)p->height * sizeof(float));
  if (!v->sdf || !v->w || !v->depthf) { free(v->sdf); free(v->w); free(v->depthf); free(v); return NULL; }
  return v;
}

void fc_destroy(fc_volume* v) {
  if (!v) return;
  free(v->sdf); free(v->w); free(v->depthf); free(v);
}

/* world -> camera, rows 0..2: the inverse in double, rounded once */
static void world_to_camera(const float* pose, float* M) {
  const double a00 = pose[0], a01 = pose[1], a02 = pose[2], t0 = pose[3];
  const double a10 = pose[4], a11 = pose[5], a12 = pose[6], t1 = pose[7];
  const double a20 = pose[8], a21 = pose[9], a22 = pose[10], t2 = pose[11];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  double inv[9];
  inv[0] = c00 / det; inv[1] = (a02 * a21 - a01 * a22) / det; inv[2] = (a01 * a12 - a02 * a11) / det;
  inv[3] = c01 / det; inv[4] = (a00 * a22 - a02 * a20) / det; inv[5] = (a02 * a10 - a00 * a12) / det;
  inv[6] = c02 / det; inv[7] = (a01 * a20 - a00 * a21) / det; inv[8] = (a00 * a11 - a01 * a10) / det;
  for (int r = 0; r < 3; r++) {
    const double ti = -(inv[3 * r] * t0 + inv[3 * r + 1] * t1 + inv[3 * r + 2] * t2);
    M[4 * r] = (float)inv[3 * r]; M[4 * r + 1] = (float)inv[3 * r + 1]; M[4 * r + 2] = (float)inv[3 * r + 2];
    M[4 * r + 3] = (float)ti;
  }
}

static int depth_weight(const fc_params* p, float d) {
  const float z01 = (d - p->depth_min) / (p->depth_max - p->depth_min);
  const float wf = fmaxf(((float)p->weight_sample * 1.5f) * (1.0f - z01), 1.0f);
  return wf >= 255.0f ? 255 : (int)wf;
}

/* one frame into every voxel of the box; 0: the pose is "tracking lost" (all -inf), nothing happens */
int fc_integrate(fc_volume* v, const uint16_t* depth, const float* pose) {
  const fc_params* p = &v->p;
  if (pose[0] == -INFINITY) return 0;
  float M[12];
  world_to_camera(pose, M);
  const int npx = p->width * p->height;
  for (int i = 0; i < npx; i++) {
    const uint16_t u = depth[i];
    float d = (float)u / p->depth_shift;
    if (u == 0 || d < p->depth_min || d > p->depth_max) d = -INFINITY;
    v->depthf[i] = d;
  }
  for (int32_t z = 0; z < v->dims[2]; z++) for (int32_t y = 0; y < v->dims[1]; y++) {
    const float wy = (float)(v->lo[1] + y) * p->voxel_size;
    const float wz = (float)(v->lo[2] + z) * p->voxel_size;
    const float ax = fmaf(M[1], wy, fmaf(M[2], wz, M[3]));
    const float ay = fmaf(M[5], wy, fmaf(M[6], wz, M[7]));
    const float az = fmaf(M[9], wy, fmaf(M[10], wz, M[11]));
    const size_t row = ((size_t)z * (size_t)v->dims[1] + (size_t)y) * (size_t)v->dims[0];
    for (int32_t x = 0; x < v->dims[0]; x++) {
      const float wx = (float)(v->lo[0] + x) * p->voxel_size;
      const float pcx = fmaf(M[0], wx, ax);
      const float pcy = fmaf(M[4], wx, ay);
      const float pcz = fmaf(M[8], wx, az);
      if (!(pcz > 0.0f)) continue;
      const float rz = 1.0f / pcz;
      const float uf = fmaf(pcx * p->fx, rz, p->mx) + 0.5f;
      const float vf = fmaf(pcy * p->fy, rz, p->my) + 0.5f;
      if (!(uf > -1.0f && uf < (float)p->width && vf > -1.0f && vf < (float)p->height)) continue;
      const int ix = (int)uf, iy = (int)vf;
      const float d = v->depthf[iy * p->width + ix];
      if (d == -INFINITY) continue;
      if (!(d < p->max_integration_dist)) continue;
      float sdf = d - pcz;
      const float t = fmaf(p->trunc_scale, d, p->trunc_base);
      if (sdf <= -t) continue;
      if (sdf > t) sdf = t;
      const size_t at = row + (size_t)x;
      const float wo = (float)v->w[at];
      const int wni = p->weight_mode == 1 ? depth_weight(p, d) : p->weight_sample;
      const float wn = (float)wni;
      v->sdf[at] = fmaf(v->sdf[at], wo, sdf * wn) / (wo + wn);
      int w = (int)v->w[at] + wni;
      if (w > p->weight_max) w = p->weight_max;
      v->w[at] = (uint8_t)w;   /* weight_wrap: the sum modulo 256 */
    }
  }
  return 1;
}

/* the box as the two dense export modes give it: 0 sdf as stored; 1 the task volume, -inf where nothing was observed, else sdf / voxel_size */
void fc_export(const fc_volume* v, int mode, float* sdf, uint8_t* weight) {
  const size_t n = (size_t)v->dims[0] * (size_t)v->dims[1] * (size_t)v->dims[2];
  for (size_t i = 0; i < n; i++) {
    if (sdf) sdf[i] = mode == 1 ? (v->w[i] == 0 ? -INFINITY : v->sdf[i] / v->p.voxel_size) : v->sdf[i];
    if (weight) weight[i] = v->w[i];
  }
}

/* The plan in its own words.  in_w x in_h: the frames as stored, with their intrinsics; int_w x int_h: the size they are integrated at (0: as stored).
 * A voxel a frame updates has 0 < z_cam < zfar and projects into (-1.5, W - 0.5) x (-1.5, H - 0.5), so it is no further than R from the camera
 * centre; the box of the centres of the frames used, grown by R and a voxel, in blocks of 8.  Returns the number of blocks, -1 without a valid pose. */
double fc_plan(int32_t in_w, int32_t in_h, float fx, float fy, float mx, float my, int32_t int_w, int32_t int_h, float voxel_size, float max_dist,
               float trunc_base, float trunc_scale, const float* poses, int64_t n, int32_t every, int32_t lo_block[3], int32_t hi_block[3], double* reach) {
  float W = (float)in_w, H = (float)in_h;
  if (int_w > 1 && int_h > 1 && (int_w != in_w || int_h != in_h)) {
    const float iw = (float)int_w, ih = (float)int_h;
    fx = fx * (iw / W); fy = fy * (ih / H);
    mx = mx * ((iw - 1.0f) / (W - 1.0f)); my = my * ((ih - 1.0f) / (H - 1.0f));
    W = iw; H = ih;
  }
  const double zfar = (double)max_dist + (double)trunc_base + (double)trunc_scale * (double)max_dist;
  const double left = (double)mx + 1.5, right = (double)W - 0.5 - (double)mx;
  const double up = (double)my + 1.5, down = (double)H - 0.5 - (double)my;
  const double ax = (left > right ? left : right) / (double)fx, ay = (up > down ? up : down) / (double)fy;
  const double R = zfar * sqrt(1.0 + ax * ax + ay * ay);
  if (reach) *reach = R;
  double cmin[3], cmax[3];
  int64_t used = 0;
  for (int64_t i = 0; i < n; i += every) {
    const float* T = poses + 16 * i;
    int lost = 1;
    for (int k = 0; k < 16; k++) if (T[k] != -INFINITY) lost = 0;
    if (lost) continue;
    const double c[3] = {T[3], T[7], T[11]};
    if (!isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2])) continue;
    for (int a = 0; a < 3; a++) {
      if (!used || c[a] < cmin[a]) cmin[a] = c[a];
      if (!used || c[a] > cmax[a]) cmax[a] = c[a];
    }
    used++;
  }
  if (!used) return -1.0;
  double blocks = 1.0;
  for (int a = 0; a < 3; a++) {
    const double lo = floor((cmin[a] - R) / (double)voxel_size) - 1.0, hi = ceil((cmax[a] + R) / (double)voxel_size) + 1.0;
    lo_block[a] = (int32_t)floor(lo / 8.0);
    hi_block[a] = (int32_t)floor(hi / 8.0);
    blocks *= (double)hi_block[a] - (double)lo_block[a] + 1.0;
  }
  return blocks;
}
