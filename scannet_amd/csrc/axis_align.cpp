// axis_align.cpp -- the pipeline's Alignment stage: Alignment::alignScan (Alignment/src/alignment.h:154-308) with PlaneExtract
// (Alignment/src/planeExtract.h:75-154).  The rule is DESIGN.md section 4i; this file holds it whole on the host (device = -1): the driver of its
// twelve steps, the host form of every stage, and what stays on the host on the device path too (up vector, list sort, Jacobi, hull, rectangle,
// files).  The stages that walk the vertices run through sf::aa::Ops, whose second implementation is axis_align.hip.
#include <dirent.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "axis_align_internal.h"
#include "mesh.h"
#include "sens.h"

namespace sf {
int param_file_read(const char* path, std::map<std::string, std::vector<std::string>>& kv);   // params.cpp
}

namespace sf {
namespace aa {

int& batch_size() {
  static int b = kMaxBatch;
  return b;
}

int& profile() {
  static int on = 0;
  return on;
}

namespace {

constexpr float kNegInf = -std::numeric_limits<float>::infinity();

// ---- the stages on the host ------------------------------------------------------------------------------------------------------------------
struct HostOps final : Ops {
  std::vector<float> pos, nrm;
  std::vector<uint32_t> tri, idx;
  size_t nv = 0, nf = 0;

  int set_positions(const float* xyz, size_t n) override { nv = n; pos.assign(xyz, xyz + 3 * n); return SF_OK; }
  int set_faces(const uint32_t* t, size_t n) override { nf = n; tri.assign(t, t + 3 * n); return SF_OK; }
  int set_normals(const float* n) override { nrm.assign(n, n + 3 * nv); return SF_OK; }
  int set_index(const uint32_t* i) override { idx.assign(i, i + nv); return SF_OK; }
  int get_positions(float* xyz) override { std::memcpy(xyz, pos.data(), pos.size() * 4); return SF_OK; }
  int get_normals(float* n) override { if (nrm.size() != 3 * nv) return fail(SF_ERR_INVALID_ARG, "no normals"); std::memcpy(n, nrm.data(), nrm.size() * 4); return SF_OK; }
  int get_index(uint32_t* i) override { if (idx.size() != nv) return fail(SF_ERR_INVALID_ARG, "no cluster index"); std::memcpy(i, idx.data(), nv * 4); return SF_OK; }

  int transform(const float m[16], float bbox[6]) override {
    const float inf = std::numeric_limits<float>::infinity();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (size_t v = 0; v < nv; v++) {
      float o[3];
      xform(m, pos[3 * v], pos[3 * v + 1], pos[3 * v + 2], o[0], o[1], o[2]);
      for (int k = 0; k < 3; k++) {
        pos[3 * v + k] = o[k];
        if (o[k] < lo[k]) lo[k] = o[k];
        if (o[k] > hi[k]) hi[k] = o[k];
      }
    }
    for (int k = 0; k < 3; k++) { bbox[k] = lo[k] + 0.0f; bbox[3 + k] = hi[k] + 0.0f; }   // a zero bound is +0 whichever zero came first
    return SF_OK;
  }

  int normals() override {
    nrm.assign(3 * nv, 0.0f);
    for (size_t f = 0; f < nf; f++) {
      const uint32_t* t = &tri[3 * f];
      const float *A = &pos[3 * (size_t)t[0]], *B = &pos[3 * (size_t)t[1]], *C = &pos[3 * (size_t)t[2]];
      float cx, cy, cz;
      cross3(B[0] - A[0], B[1] - A[1], B[2] - A[2], C[0] - A[0], C[1] - A[1], C[2] - A[2], cx, cy, cz);
      for (int k = 0; k < 3; k++) {
        float* n = &nrm[3 * (size_t)t[k]];
        n[0] = n[0] + cx; n[1] = n[1] + cy; n[2] = n[2] + cz;
      }
    }
    for (size_t v = 0; v < nv; v++) normalize3(nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]);
    return SF_OK;
  }

  int cluster(float nthr, float dthr, std::vector<Cluster>& table, uint64_t counters[3]) override {
    if (nrm.size() != 3 * nv) return fail(SF_ERR_INVALID_ARG, "no normals");
    table.clear();
    idx.assign(nv, 0);
    for (size_t v = 0; v < nv; v++) {
      const float *n = &nrm[3 * v], *p = &pos[3 * v];
      size_t c = 0;
      for (; c < table.size(); c++) {
        const float* r = table[c].rep;
        if (check(r[0], r[1], r[2], r[3], n[0], n[1], n[2], p[0], p[1], p[2], nthr, dthr)) { join(table[c], n[0], n[1], n[2], p[0], p[1], p[2]); break; }
      }
      if (c == table.size()) {
        Cluster k;
        found(k, n[0], n[1], n[2], p[0], p[1], p[2]);
        table.push_back(k);
      }
      idx[v] = (uint32_t)c;
    }
    counters[0] = counters[1] = counters[2] = 0;
    return SF_OK;
  }

  int behind(const float* reps4, size_t K, float dist, uint32_t* counts) override {
    for (size_t k = 0; k < K; k++) {
      const float* r = reps4 + 4 * k;
      uint32_t n = 0;
      for (size_t v = 0; v < nv; v++)
        if (plane_dist(r[0], r[1], r[2], r[3], pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]) < -dist) n++;
      counts[k] = n;
    }
    return SF_OK;
  }

  int cov(uint32_t cluster, const float rep[4], float inlier, double sums[10]) override {
    if (idx.size() != nv) return fail(SF_ERR_INVALID_ARG, "no cluster index");
    for (int k = 0; k < 10; k++) sums[k] = 0.0;
    std::vector<double> leaf((size_t)kCovBlock * 10);
    for (size_t b0 = 0; b0 < nv; b0 += kCovBlock) {
      for (int i = 0; i < kCovBlock; i++) {
        double* l = &leaf[(size_t)i * 10];
        const size_t v = b0 + i;
        bool in = false;
        if (v < nv && idx[v] == cluster) in = fabsf(plane_dist(rep[0], rep[1], rep[2], rep[3], pos[3 * v], pos[3 * v + 1], pos[3 * v + 2])) < inlier;
        if (in) {
          const double x = pos[3 * v], y = pos[3 * v + 1], z = pos[3 * v + 2];
          l[0] = 1.0; l[1] = x; l[2] = y; l[3] = z; l[4] = x * x; l[5] = x * y; l[6] = x * z; l[7] = y * y; l[8] = y * z; l[9] = z * z;
        } else {
          for (int k = 0; k < 10; k++) l[k] = 0.0;
        }
      }
      for (int s = 1; s < kCovBlock; s *= 2)
        for (int i = 0; i + s < kCovBlock; i += 2 * s)
          for (int k = 0; k < 10; k++) leaf[(size_t)i * 10 + k] = leaf[(size_t)i * 10 + k] + leaf[(size_t)(i + s) * 10 + k];
      for (int k = 0; k < 10; k++) sums[k] = sums[k] + leaf[k];
    }
    return SF_OK;
  }
};

// ---- small matrices ---------------------------------------------------------------------------------------------------------------------------
void identity(float m[16]) { for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
void translation(float m[16], float x, float y, float z) { identity(m); m[3] = x; m[7] = y; m[11] = z; }
void rows3(float m[16], const float x[3], const float y[3], const float z[3]) {
  identity(m);
  for (int k = 0; k < 3; k++) { m[k] = x[k]; m[4 + k] = y[k]; m[8 + k] = z[k]; }
}
// t <- a * t, the float product of sf_sens_apply_transform: sums in index order
void compose(const float a[16], float t[16]) {
  float r[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float acc = a[i * 4 + 0] * t[0 * 4 + j];
      for (int k = 1; k < 4; k++) acc = acc + a[i * 4 + k] * t[k * 4 + j];
      r[i * 4 + j] = acc;
    }
  std::memcpy(t, r, 64);
}
// the inverse of a pose: Gauss-Jordan with partial pivoting in double, rounded to float once
bool invert(const float m[16], float out[16]) {
  double a[4][8];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) { a[i][j] = m[i * 4 + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
  for (int c = 0; c < 4; c++) {
    int p = c;
    for (int r = c + 1; r < 4; r++) if (std::fabs(a[r][c]) > std::fabs(a[p][c])) p = r;
    if (!(std::fabs(a[p][c]) > 0.0) || !std::isfinite(a[p][c])) return false;
    if (p != c) for (int j = 0; j < 8; j++) std::swap(a[p][j], a[c][j]);
    const double d = a[c][c];
    for (int j = 0; j < 8; j++) a[c][j] = a[c][j] / d;
    for (int r = 0; r < 4; r++) {
      if (r == c) continue;
      const double f = a[r][c];
      if (f == 0.0) continue;
      for (int j = 0; j < 8; j++) a[r][j] = a[r][j] - f * a[c][j];
    }
  }
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) out[i * 4 + j] = (float)a[i][4 + j];
  return true;
}

// ---- step 2: the up vector (alignment.h:23-35, :71-107) ---------------------------------------------------------------------------------------
int up_vector(const sf_sens* s, uint32_t gravity_min, float up[3], int32_t* source, uint64_t* no_gravity, uint64_t* dropped) {
  const size_t n = s->frames.size();
  if (n == 0) return fail(SF_ERR_INVALID_ARG, "no frames found in the sensor file");
  // removeInvalidIMUFrames :128-152: a view of the file without its records of time stamp 0 (poses and time stamps only)
  sf_sens view;
  view.info = s->info;
  view.frames.resize(n);
  for (size_t i = 0; i < n; i++) {
    std::memcpy(view.frames[i].pose, s->frames[i].pose, 64);
    view.frames[i].ts_color = s->frames[i].ts_color;
    view.frames[i].ts_depth = s->frames[i].ts_depth;
  }
  size_t with_gravity = 0, drop = 0;
  for (size_t i = 0; i + 128 <= s->imu.size(); i += 128) {
    uint64_t ts;
    std::memcpy(&ts, &s->imu[i + 120], 8);
    if (ts == 0) { drop++; continue; }
    view.imu.insert(view.imu.end(), s->imu.begin() + i, s->imu.begin() + i + 128);
    double g[3];
    std::memcpy(g, &s->imu[i + 96], 24);
    if (!(g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0)) with_gravity++;
  }
  if (dropped) *dropped = drop;
  const bool gravity = with_gravity > gravity_min;
  float v[3] = {0.0f, 0.0f, 0.0f};
  uint64_t none = 0;
  for (size_t i = 0; i < n; i++) {
    const float* m = view.frames[i].pose;
    float c[3];
    if (gravity) {
      uint8_t rec[128];
      const int rc = sf_sens_find_closest_imu(&view, i, 1, rec, nullptr);   // findClosestIMUFrame(i): basedOnRGB = true
      if (rc != SF_OK) return rc;
      if (m[0] == kNegInf) continue;
      double g[3];
      std::memcpy(g, rec + 96, 24);
      if (g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0) { none++; continue; }
      float x = (float)g[0], y = (float)g[1], z = (float)g[2];
      normalize3(x, y, z);
      c[0] = y; c[1] = x; c[2] = z;   // :98, the x/y swap
    } else {
      if (m[0] == kNegInf) continue;
      c[0] = 0.0f; c[1] = -1.0f; c[2] = 0.0f;
    }
    float w[3];
    for (int r = 0; r < 3; r++) w[r] = dot3(m[4 * r], m[4 * r + 1], m[4 * r + 2], c[0], c[1], c[2]);
    normalize3(w[0], w[1], w[2]);
    for (int r = 0; r < 3; r++) v[r] = v[r] + w[r];
  }
  const float k = (float)n;   // the count of ALL frames (:33, :104)
  for (int r = 0; r < 3; r++) v[r] = v[r] / k;
  normalize3(v[0], v[1], v[2]);
  std::memcpy(up, v, 12);
  if (source) *source = gravity ? 1 : 0;
  if (no_gravity) *no_gravity = none;
  return SF_OK;
}

// ---- step 5: floor rotation from the ten sums (host, double) ------------------------------------------------------------------------------------
constexpr int kJacobiSweeps = 16;

void floor_rotation(const double s[10], float m[16]) {
  identity(m);
  const double n = s[0];
  if (!(n > 0.0)) return;
  const double mx = s[1] / n, my = s[2] / n, mz = s[3] / n;
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  A[0][0] = s[4] / n - mx * mx; A[0][1] = s[5] / n - mx * my; A[0][2] = s[6] / n - mx * mz;
  A[1][1] = s[7] / n - my * my; A[1][2] = s[8] / n - my * mz; A[2][2] = s[9] / n - mz * mz;
  A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
  static const int PQ[3][2] = {{0, 1}, {0, 2}, {1, 2}};
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++)
    for (int e = 0; e < 3; e++) {
      const int p = PQ[e][0], q = PQ[e][1];
      if (A[p][q] == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
      const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
      const double app = A[p][p], aqq = A[q][q], apq = A[p][q];
      A[p][p] = app - t * apq;
      A[q][q] = aqq + t * apq;
      A[p][q] = 0.0; A[q][p] = 0.0;
      const int r = 3 - p - q;
      const double arp = A[r][p], arq = A[r][q];
      A[r][p] = c * arp - sn * arq; A[p][r] = A[r][p];
      A[r][q] = sn * arp + c * arq; A[q][r] = A[r][q];
      for (int k = 0; k < 3; k++) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - sn * vkq;
        V[k][q] = sn * vkp + c * vkq;
      }
    }
  int imin = 0, imax = 0;
  for (int k = 1; k < 3; k++) {
    if (A[k][k] < A[imin][imin]) imin = k;
    if (A[k][k] > A[imax][imax]) imax = k;
  }
  if (imin == imax) return;
  double Z[3] = {V[0][imin], V[1][imin], V[2][imin]}, X[3] = {V[0][imax], V[1][imax], V[2][imax]};
  if (Z[2] < 0.0) { Z[0] = -Z[0]; Z[1] = -Z[1]; Z[2] = -Z[2]; }
  double Y[3] = {Z[1] * X[2] - Z[2] * X[1], Z[2] * X[0] - Z[0] * X[2], Z[0] * X[1] - Z[1] * X[0]};
  auto unit = [](double* a) {
    const double l = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    if (l == 0.0) return;
    a[0] = a[0] / l; a[1] = a[1] / l; a[2] = a[2] / l;
  };
  unit(X); unit(Y); unit(Z);
  for (int k = 0; k < 3; k++) { m[k] = (float)X[k]; m[4 + k] = (float)Y[k]; m[8 + k] = (float)Z[k]; }
}

// ---- step 7: wall rotation (host, double): convex hull by a monotone chain, then the smallest rectangle with a side along a hull edge -------------
struct P2 { double x, y; };
double turn(const P2& o, const P2& a, const P2& b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

void wall_rotation(const float* xyz, size_t nv, float m[16]) {
  identity(m);
  std::vector<P2> pts(nv);
  for (size_t v = 0; v < nv; v++) { pts[v].x = xyz[3 * v]; pts[v].y = xyz[3 * v + 1]; }
  std::sort(pts.begin(), pts.end(), [](const P2& a, const P2& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
  pts.erase(std::unique(pts.begin(), pts.end(), [](const P2& a, const P2& b) { return a.x == b.x && a.y == b.y; }), pts.end());
  const size_t n = pts.size();
  if (n < 3) return;
  std::vector<P2> h(2 * n);
  size_t k = 0;
  for (size_t i = 0; i < n; i++) {   // lower hull
    while (k >= 2 && turn(h[k - 2], h[k - 1], pts[i]) <= 0.0) k--;
    h[k++] = pts[i];
  }
  for (size_t i = n - 1, lo = k + 1; i-- > 0;) {   // upper hull
    while (k >= lo && turn(h[k - 2], h[k - 1], pts[i]) <= 0.0) k--;
    h[k++] = pts[i];
  }
  k--;   // the last point is the first again
  if (k < 3) return;
  double best = 0.0, bx = 0.0, by = 0.0;
  bool have = false;
  for (size_t i = 0; i < k; i++) {
    const P2 &a = h[i], &b = h[(i + 1) % k];
    const double ex = b.x - a.x, ey = b.y - a.y, l = std::sqrt(ex * ex + ey * ey);
    if (l == 0.0) continue;
    const double ux = ex / l, uy = ey / l;
    double lo_u = 0, hi_u = 0, lo_v = 0, hi_v = 0;
    for (size_t j = 0; j < k; j++) {
      const double pu = ux * h[j].x + uy * h[j].y, pv = ux * h[j].y - uy * h[j].x;
      if (j == 0) { lo_u = hi_u = pu; lo_v = hi_v = pv; continue; }
      if (pu < lo_u) lo_u = pu;
      if (pu > hi_u) hi_u = pu;
      if (pv < lo_v) lo_v = pv;
      if (pv > hi_v) hi_v = pv;
    }
    const double area = (hi_u - lo_u) * (hi_v - lo_v);
    if (!have || area < best) { have = true; best = area; bx = ux; by = uy; }
  }
  if (!have) return;
  const double cand[4][2] = {{bx, by}, {-by, bx}, {-bx, -by}, {by, -bx}};   // the edge direction turned by 0, 90, 180, 270 degrees
  for (int q = 0; q < 4; q++) {
    const double c = cand[q][0], s = cand[q][1];
    if (c > 0.0 && s >= -c && s < c) {   // direction in [-45, 45) degrees: the rotation that takes it onto +x is by an angle in (-45, 45]
      m[0] = (float)c; m[1] = (float)s; m[4] = -(float)s; m[5] = (float)c;
      return;
    }
  }
}

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int check_params(const sf_axis_align_params& p) {
  const float f[6] = {p.merge_distance, p.cluster_normal_thresh, p.cluster_dist_thresh, p.behind_dist, p.floor_normal_z, p.floor_inlier_dist};
  for (float x : f)
    if (!std::isfinite(x) || x < 0.0f) return fail(SF_ERR_INVALID_ARG, "sf_axis_align_params: a threshold is negative or not finite");
  return SF_OK;
}

struct Planes {   // steps 4 and the first half of 5: what survives the sort and the two filters
  std::vector<Cluster> table;       // creation order
  std::vector<uint32_t> sorted;     // ids after the stable sort and removeSmallClusters
  std::vector<uint32_t> behind;     // per entry of sorted
  uint64_t counters[3] = {0, 0, 0};
};

int find_planes(Ops& ops, const sf_axis_align_params& P, Planes& out, double* t_cluster, double* t_behind) {
  double t0 = now();
  int rc = ops.cluster(P.cluster_normal_thresh, P.cluster_dist_thresh, out.table, out.counters);
  if (rc != SF_OK) return rc;
  std::vector<uint32_t> order(out.table.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return out.table[a].count > out.table[b].count; });   // planeExtract.h:62-64,103
  out.sorted.clear();
  for (uint32_t id : order)
    if (out.table[id].count >= P.min_cluster_points) out.sorted.push_back(id);   // :122-131
  double t1 = now();
  std::vector<float> reps(4 * out.sorted.size());
  for (size_t i = 0; i < out.sorted.size(); i++) std::memcpy(&reps[4 * i], out.table[out.sorted[i]].rep, 16);
  out.behind.assign(out.sorted.size(), 0);
  rc = ops.behind(reps.data(), out.sorted.size(), P.behind_dist, out.behind.data());   // :146-154
  if (t_cluster) *t_cluster = t1 - t0;
  if (t_behind) *t_behind = now() - t1;
  return rc;
}

// steps 2 (rotation) to 9 on a working set that holds the cleaned mesh
int run_rule(Ops& ops, size_t nv, const sf_axis_align_params& P, const float up[3], float T[16], sf_axis_align_stats& st) {
  float bbox[6], M[16];
  identity(T);
  double t0 = now();
  {   // alignment.h:223-228
    float x[3], y[3];
    cross3(up[0], up[1], up[2], up[1], -up[2], up[0], x[0], x[1], x[2]);
    normalize3(x[0], x[1], x[2]);
    cross3(up[0], up[1], up[2], x[0], x[1], x[2], y[0], y[1], y[2]);
    normalize3(y[0], y[1], y[2]);
    rows3(M, x, y, up);
  }
  int rc = ops.transform(M, bbox);
  if (rc != SF_OK) return rc;
  compose(M, T);
  double t1 = now();
  st.seconds[5] += t1 - t0;
  rc = ops.normals();   // :231
  if (rc != SF_OK) return rc;
  t0 = now();
  st.seconds[1] = t0 - t1;
  Planes pl;
  rc = find_planes(ops, P, pl, &st.seconds[2], &st.seconds[3]);
  if (rc != SF_OK) return rc;
  st.clusters_founded = pl.table.size();
  st.clusters_after_small = pl.sorted.size();
  st.gpu_seconds_match = ops.split[0]; st.gpu_seconds_commit = ops.split[1];
  st.gpu_batches = pl.counters[0]; st.gpu_dirty_evaluations = pl.counters[1]; st.gpu_fallback_rescans = pl.counters[2];
  int64_t floor = -1;
  for (size_t i = 0; i < pl.sorted.size(); i++) {
    if (pl.behind[i] > P.behind_max) continue;   // planeExtract.h:152
    st.clusters_kept++;
    if (floor < 0 && pl.table[pl.sorted[i]].rep[2] > P.floor_normal_z) floor = pl.sorted[i];   // alignment.h:245
  }
  t0 = now();
  if (floor >= 0) {
    double sums[10];
    rc = ops.cov((uint32_t)floor, pl.table[floor].rep, P.floor_inlier_dist, sums);
    if (rc != SF_OK) return rc;
    st.floor_found = 1;
    st.floor_points = pl.table[floor].count;
    st.floor_inliers = (uint64_t)sums[0];
    floor_rotation(sums, M);
    t1 = now();
    st.seconds[4] = t1 - t0;
    rc = ops.transform(M, bbox);
    if (rc != SF_OK) return rc;
    compose(M, T);
  }
  t1 = now();
  translation(M, 0.0f, 0.0f, -bbox[2]);   // :259-262
  if ((rc = ops.transform(M, bbox)) != SF_OK) return rc;
  compose(M, T);
  translation(M, -((bbox[0] + bbox[3]) * 0.5f), -((bbox[1] + bbox[4]) * 0.5f), 0.0f);   // :264-267
  if ((rc = ops.transform(M, bbox)) != SF_OK) return rc;
  compose(M, T);
  {   // :274-277
    std::vector<float> xyz(3 * nv);
    if ((rc = ops.get_positions(xyz.data())) != SF_OK) return rc;
    wall_rotation(xyz.data(), nv, M);
  }
  if ((rc = ops.transform(M, bbox)) != SF_OK) return rc;
  compose(M, T);
  translation(M, -bbox[0], -bbox[1], 0.0f);   // :282-285
  compose(M, T);
  st.seconds[5] += now() - t1;
  return SF_OK;
}

int make_ops(int device, std::unique_ptr<Ops>& ops) {
  if (device < 0) { ops.reset(make_host_ops()); return SF_OK; }
  Ops* g = nullptr;
  const int rc = make_gpu_ops(device, &g);
  if (rc != SF_OK) return rc;
  ops.reset(g);
  return SF_OK;
}

int estimate(const sf_mesh* mesh, const sf_sens* sens, const sf_axis_align_params* params, int device, float T[16], sf_axis_align_stats* stats) {
  if (!mesh || !sens || !T) return fail(SF_ERR_INVALID_ARG, "NULL argument");
  sf_axis_align_params P;
  if (params) P = *params; else sf_axis_align_params_default(&P);
  int rc = check_params(P);
  if (rc != SF_OK) return rc;
  sf_axis_align_stats st;
  std::memset(&st, 0, sizeof st);
  float up[3];
  if ((rc = up_vector(sens, P.gravity_min_records, up, &st.up_source, &st.frames_without_gravity, &st.imu_records_dropped)) != SF_OK) return rc;
  std::unique_ptr<Ops> ops;
  if ((rc = make_ops(device, ops)) != SF_OK) return rc;
  const double t0 = now();
  sf_mesh* work = nullptr;   // alignment.h:211-212
  rc = device < 0 ? sf_mesh_clean(mesh, P.merge_distance, P.min_piece_faces, &work, nullptr) : sf_mesh_clean_gpu(mesh, P.merge_distance, P.min_piece_faces, device, &work, nullptr);
  if (rc != SF_OK) return rc;
  st.seconds[0] = now() - t0;
  const size_t nv = work->pos.size() / 3, nf = work->tri.size() / 3;
  st.vertices = nv; st.faces = nf;
  if (nv == 0) { sf_mesh_free(work); return fail(SF_ERR_INVALID_ARG, "no vertex is left of the mesh after cleaning"); }
  rc = ops->set_positions(work->pos.data(), nv);
  if (rc == SF_OK) rc = ops->set_faces(work->tri.data(), nf);
  sf_mesh_free(work);
  if (rc == SF_OK) rc = run_rule(*ops, nv, P, up, T, st);
  if (rc != SF_OK) return rc;
  std::memcpy(st.transform, T, 64);
  if (stats) *stats = st;
  return SF_OK;
}

// the folder's meshes go through the same operations on either path
int apply_to_mesh(sf_mesh* m, const float t[16], Ops* gpu) {
  const size_t nv = m->pos.size() / 3;
  if (!gpu) {
    for (size_t v = 0; v < nv; v++) xform(t, m->pos[3 * v], m->pos[3 * v + 1], m->pos[3 * v + 2], m->pos[3 * v], m->pos[3 * v + 1], m->pos[3 * v + 2]);
    return SF_OK;
  }
  float bbox[6];
  int rc = gpu->set_positions(m->pos.data(), nv);
  if (rc == SF_OK) rc = gpu->transform(t, bbox);
  if (rc == SF_OK) rc = gpu->get_positions(m->pos.data());
  return rc;
}

bool read_bool(const std::map<std::string, std::vector<std::string>>& kv, const char* k) {
  auto it = kv.find(k);
  return it != kv.end() && !it->second.empty() && (it->second[0] == "true" || it->second[0] == "1");
}
unsigned read_uint(const std::map<std::string, std::vector<std::string>>& kv, const char* k) {
  auto it = kv.find(k);
  return it != kv.end() && !it->second.empty() ? (unsigned)std::strtoul(it->second[0].c_str(), nullptr, 10) : 0u;
}

int scan(const char* dir_in, int force, const sf_axis_align_params* params, int device, sf_axis_align_stats* stats) {
  if (!dir_in) return fail(SF_ERR_INVALID_ARG, "NULL argument");
  sf_axis_align_stats st;
  std::memset(&st, 0, sizeof st);
  auto done = [&](int outcome) { st.outcome = outcome; if (stats) *stats = st; return (int)SF_OK; };
  std::string dir = dir_in;
  std::replace(dir.begin(), dir.end(), '\\', '/');   // alignment.h:173
  std::string trimmed = dir;
  while (trimmed.size() > 1 && trimmed.back() == '/') trimmed.pop_back();
  const std::string base = trimmed.substr(trimmed.find_last_of('/') == std::string::npos ? 0 : trimmed.find_last_of('/') + 1);
  const std::string processed = dir + "/processed.txt";
  { std::ifstream probe(processed); if (!probe) return done(1); }   // :157-160
  std::map<std::string, std::vector<std::string>> kv;
  int rc = sf::param_file_read(processed.c_str(), kv);
  if (rc != SF_OK) return rc;
  if (!read_bool(kv, "valid")) return done(2);               // :163-166
  if (read_bool(kv, "aligned") && !force) return done(3);    // :167-170
  const std::string sens_path = dir + "/" + base + ".sens", ply_path = dir + "/" + base + ".ply";
  sf_sens* sens = nullptr;
  if ((rc = sf_sens_open(sens_path.c_str(), &sens)) != SF_OK) return rc;
  struct SensGuard { sf_sens* s; ~SensGuard() { sf_sens_close(s); } } sens_guard{sens};
  if (sens->frames.empty()) return fail(SF_ERR_INVALID_ARG, "no frames found in the sensor file");   // :187
  std::vector<std::string> plys;   // :202, :295
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.compare(n.size() - 4, 4, ".ply") == 0) plys.push_back(n);
    }
    closedir(d);
  } else {
    return fail(SF_ERR_IO, "could not list %s", dir.c_str());
  }
  std::sort(plys.begin(), plys.end());
  std::unique_ptr<Ops> gpu;
  if (device >= 0 && (rc = make_ops(device, gpu)) != SF_OK) return rc;
  struct MeshGuard { std::vector<sf_mesh*> m; ~MeshGuard() { for (sf_mesh* x : m) sf_mesh_free(x); } } meshes;
  sf_mesh* scan_mesh = nullptr;
  for (const std::string& n : plys) {
    sf_mesh* m = nullptr;
    if ((rc = sf_ply_read((dir + "/" + n).c_str(), &m)) != SF_OK) return rc;
    meshes.m.push_back(m);
    if (n == base + ".ply") scan_mesh = m;
  }
  if (!scan_mesh) return fail(SF_ERR_IO, "could not open %s", ply_path.c_str());
  float id[16];
  identity(id);
  {   // :189-208 (compared as floats: -0 equals 0)
    bool same = true;
    for (int i = 0; i < 16; i++) same = same && sens->frames[0].pose[i] == id[i];
    if (!same) {
      if (sens->frames[0].pose[0] == kNegInf) return done(4);   // :192-196
      float inv[16];
      if (!invert(sens->frames[0].pose, inv)) return fail(SF_ERR_FORMAT, "frame 0's pose cannot be inverted");
      st.reverted = 1;
      sf_sens_apply_transform(sens, inv);
      for (sf_mesh* m : meshes.m)
        if ((rc = apply_to_mesh(m, inv, gpu.get())) != SF_OK) return rc;
    }
  }
  float T[16];
  const int reverted = st.reverted;
  if ((rc = estimate(scan_mesh, sens, params, device, T, &st)) != SF_OK) return rc;
  st.reverted = reverted;
  // :292-307.  Everything is written beside its target first and renamed over it: the .sens is memory-mapped while it is rewritten.
  for (sf_mesh* m : meshes.m)
    if ((rc = apply_to_mesh(m, T, gpu.get())) != SF_OK) return rc;
  sf_sens_apply_transform(sens, T);
  {   // removeInvalidIMUFrames :128-152: the saved file is without them
    std::vector<uint8_t> kept;
    for (size_t i = 0; i + 128 <= sens->imu.size(); i += 128) {
      uint64_t ts;
      std::memcpy(&ts, &sens->imu[i + 120], 8);
      if (ts != 0) kept.insert(kept.end(), sens->imu.begin() + i, sens->imu.begin() + i + 128);
    }
    sens->imu.swap(kept);
  }
  std::vector<std::pair<std::string, std::string>> moves;
  auto cleanup = [&]() { for (auto& mv : moves) std::remove(mv.first.c_str()); };
  for (size_t i = 0; i < plys.size(); i++) {
    const std::string dst = dir + "/" + plys[i], tmp = dst + ".aligning";
    moves.emplace_back(tmp, dst);
    if ((rc = sf_mesh_write_ply(meshes.m[i], tmp.c_str())) != SF_OK) { cleanup(); return rc; }
  }
  moves.emplace_back(sens_path + ".aligning", sens_path);
  if ((rc = sf_sens_save(sens, moves.back().first.c_str())) != SF_OK) { cleanup(); return rc; }
  {
    const std::string tmp = processed + ".aligning";
    moves.emplace_back(tmp, processed);
    std::ofstream out(tmp);   // processedFile.h:57-63
    out << "valid = true\n"
        << "heapFreeCount = " << std::to_string(read_uint(kv, "heapFreeCount")) << "\n"
        << "numValidOptTransforms = " << std::to_string(read_uint(kv, "numValidOptTransforms")) << "\n"
        << "numTransforms = " << std::to_string(read_uint(kv, "numTransforms")) << "\n"
        << "aligned = true\n";
    out.close();
    if (!out) { cleanup(); return fail(SF_ERR_IO, "write to %s failed", tmp.c_str()); }
  }
  for (auto& mv : moves)
    if (std::rename(mv.first.c_str(), mv.second.c_str()) != 0) { cleanup(); return fail(SF_ERR_IO, "could not replace %s", mv.second.c_str()); }
  return done(0);
}

}  // namespace

Ops* make_host_ops() { return new HostOps; }

}  // namespace aa
}  // namespace sf

using namespace sf::aa;

#define AA_GUARD(expr)                                                                    \
  try { return (expr); }                                                                  \
  catch (const std::bad_alloc&) { return sf::fail(SF_ERR_CAPACITY, "out of host memory"); } \
  catch (const std::exception& e) { return sf::fail(SF_ERR_INVALID_ARG, "%s", e.what()); }

SF_API void sf_axis_align_params_default(sf_axis_align_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->merge_distance = 0.0005f;
  p->min_piece_faces = 5000;
  p->gravity_min_records = 10;
  p->cluster_normal_thresh = 0.90f;
  p->cluster_dist_thresh = 0.05f;
  p->min_cluster_points = 500;
  p->behind_dist = 0.1f;
  p->behind_max = 100;
  p->floor_normal_z = 0.8f;
  p->floor_inlier_dist = 0.05f;
}

SF_API int sf_axis_align_estimate(const sf_mesh* mesh, const sf_sens* sens, const sf_axis_align_params* params, int device, float transform[16],
                                  sf_axis_align_stats* stats) {
  AA_GUARD(estimate(mesh, sens, params, device, transform, stats));
}

SF_API int sf_mesh_apply_transform(sf_mesh* mesh, const float transform[16]) {
  if (!mesh || !transform) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  return apply_to_mesh(mesh, transform, nullptr);
}

SF_API int sf_axis_align_scan(const char* dir, int force, const sf_axis_align_params* params, int device, sf_axis_align_stats* stats) {
  AA_GUARD(scan(dir, force, params, device, stats));
}

// ---- stage hooks (scanfuse_internal.h) -------------------------------------------------------------------------------------------------------------
SF_API int sf_axis_align_tune(const char* key, int value) {
  if (key && std::strcmp(key, "profile") == 0 && (value == 0 || value == 1)) { profile() = value; return SF_OK; }
  if (!key || std::strcmp(key, "batch") != 0) return sf::fail(SF_ERR_INVALID_ARG, "sf_axis_align_tune: unknown key or value");
  if (value < 64 || value > kMaxBatch || value % 64 != 0) return sf::fail(SF_ERR_INVALID_ARG, "sf_axis_align_tune: batch is 64..%d in steps of 64", kMaxBatch);
  batch_size() = value;
  return SF_OK;
}

SF_API int sf_axis_align_stage_up(const sf_sens* sens, uint32_t gravity_min_records, float up3[3], int32_t* source, uint64_t* no_gravity) {
  if (!sens || !up3) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  AA_GUARD(up_vector(sens, gravity_min_records, up3, source, no_gravity, nullptr));
}

namespace {
int check_faces(const uint32_t* tris, uint64_t nf, uint64_t nv) {
  for (uint64_t i = 0; i < 3 * nf; i++)
    if (tris[i] >= nv) return sf::fail(SF_ERR_BOUNDS, "face %llu names vertex %u of %llu", (unsigned long long)(i / 3), tris[i], (unsigned long long)nv);
  return SF_OK;
}

int stage_normals(const float* xyz, uint64_t nv, const uint32_t* tris, uint64_t nf, int device, float* out) {
  int rc = check_faces(tris, nf, nv);
  if (rc != SF_OK) return rc;
  std::unique_ptr<Ops> ops;
  if ((rc = make_ops(device, ops)) != SF_OK) return rc;
  if ((rc = ops->set_positions(xyz, nv)) != SF_OK || (rc = ops->set_faces(tris, nf)) != SF_OK || (rc = ops->normals()) != SF_OK) return rc;
  return ops->get_normals(out);
}

int stage_planes(const float* xyz, const float* normals, uint64_t nv, const sf_axis_align_params* p, int device, uint32_t* index_out, uint64_t* n_founded,
                 uint32_t* ids, float* table10, uint32_t* counts, uint32_t* behind, uint64_t capacity, uint64_t* n_sorted, uint64_t counters[3]) {
  int rc = check_params(*p);
  if (rc != SF_OK) return rc;
  std::unique_ptr<Ops> ops;
  if ((rc = make_ops(device, ops)) != SF_OK) return rc;
  if ((rc = ops->set_positions(xyz, nv)) != SF_OK || (rc = ops->set_normals(normals)) != SF_OK) return rc;
  Planes pl;
  if ((rc = find_planes(*ops, *p, pl, nullptr, nullptr)) != SF_OK) return rc;
  if (index_out && (rc = ops->get_index(index_out)) != SF_OK) return rc;
  if (n_founded) *n_founded = pl.table.size();
  if (n_sorted) *n_sorted = pl.sorted.size();
  if (counters) std::memcpy(counters, pl.counters, sizeof pl.counters);
  for (size_t i = 0; i < pl.sorted.size() && i < capacity; i++) {
    const Cluster& c = pl.table[pl.sorted[i]];
    if (ids) ids[i] = pl.sorted[i];
    if (table10) { std::memcpy(table10 + 10 * i, c.rep, 16); std::memcpy(table10 + 10 * i + 4, c.sn, 12); std::memcpy(table10 + 10 * i + 7, c.sp, 12); }
    if (counts) counts[i] = c.count;
    if (behind) behind[i] = pl.behind[i];
  }
  return SF_OK;
}

int stage_behind(const float* xyz, uint64_t nv, const float* reps4, uint64_t K, float dist, int device, uint32_t* out) {
  std::unique_ptr<Ops> ops;
  int rc = make_ops(device, ops);
  if (rc != SF_OK || (rc = ops->set_positions(xyz, nv)) != SF_OK) return rc;
  return ops->behind(reps4, K, dist, out);
}

int stage_cov(const float* xyz, const uint32_t* index, uint64_t nv, uint32_t cluster, const float rep4[4], float inlier, int device, double sums[10]) {
  std::unique_ptr<Ops> ops;
  int rc = make_ops(device, ops);
  if (rc != SF_OK || (rc = ops->set_positions(xyz, nv)) != SF_OK || (rc = ops->set_index(index)) != SF_OK) return rc;
  return ops->cov(cluster, rep4, inlier, sums);
}

int stage_transform(const float* xyz, uint64_t nv, const float m[16], int device, float* out, float bbox[6]) {
  std::unique_ptr<Ops> ops;
  int rc = make_ops(device, ops);
  if (rc != SF_OK || (rc = ops->set_positions(xyz, nv)) != SF_OK || (rc = ops->transform(m, bbox)) != SF_OK) return rc;
  return out ? ops->get_positions(out) : (int)SF_OK;
}
}  // namespace

SF_API int sf_axis_align_stage_normals(const float* xyz, uint64_t num_vertices, const uint32_t* tris, uint64_t num_faces, int device, float* normals_out) {
  if ((!xyz && num_vertices) || (!tris && num_faces) || !normals_out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  AA_GUARD(stage_normals(xyz, num_vertices, tris, num_faces, device, normals_out));
}

SF_API int sf_axis_align_stage_planes(const float* xyz, const float* normals, uint64_t num_vertices, const sf_axis_align_params* p, int device, uint32_t* index_out,
                                      uint64_t* n_founded, uint32_t* ids, float* table10, uint32_t* counts, uint32_t* behind, uint64_t capacity, uint64_t* n_sorted,
                                      uint64_t counters[3]) {
  if (((!xyz || !normals) && num_vertices) || !p) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  AA_GUARD(stage_planes(xyz, normals, num_vertices, p, device, index_out, n_founded, ids, table10, counts, behind, capacity, n_sorted, counters));
}

SF_API int sf_axis_align_stage_behind(const float* xyz, uint64_t num_vertices, const float* reps4, uint64_t K, float behind_dist, int device, uint32_t* counts_out) {
  if ((!xyz && num_vertices) || ((!reps4 || !counts_out) && K)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  AA_GUARD(stage_behind(xyz, num_vertices, reps4, K, behind_dist, device, counts_out));
}

SF_API int sf_axis_align_stage_cov(const float* xyz, const uint32_t* index, uint64_t num_vertices, uint32_t cluster, const float rep4[4], float inlier_dist, int device,
                                   double sums10[10]) {
  if (((!xyz || !index) && num_vertices) || !rep4 || !sums10) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  AA_GUARD(stage_cov(xyz, index, num_vertices, cluster, rep4, inlier_dist, device, sums10));
}

SF_API int sf_axis_align_stage_transform(const float* xyz, uint64_t num_vertices, const float m[16], int device, float* xyz_out, float bbox6[6]) {
  if ((!xyz && num_vertices) || !m || !bbox6) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  AA_GUARD(stage_transform(xyz, num_vertices, m, device, xyz_out, bbox6));
}
