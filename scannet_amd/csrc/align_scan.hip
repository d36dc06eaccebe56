// align_scan.hip -- the global alignment for scans of any length: the plan that splits the keyframes into groups of consecutive frames
// under a top level, the batched solve of all groups at once, and the scan call that solves the top with align.hip's own loop and carries the
// corrections down.
//
// Every group is sf_fuser_align*'s problem, bit for bit.  Per Gauss-Newton iteration the host writes ONE pair table for all groups, align.hip's (or
// align_colour.hip's) kernels turn it into per-pair systems in launches of at most 4096 pairs, and k_group_solve -- one workgroup per running
// group -- drops thin pairs, finds the frames connected to the group's first, assembles the normal equations in LDS and solves them by Cholesky in
// double, in the order of align_solve.h, which the host's loop uses too.  One read-back of the groups' records; the pose update (sin, cos) stays on
// the host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "align_internal.h"
#include "common.h"
#include "scanfuse_internal.h"

namespace {

using namespace tk;

constexpr uint64_t AS_MAX_FRAMES = 4096;
constexpr uint64_t AS_MAX_GROUPS = 4096;
constexpr uint64_t AS_MAX_MEMBERS = 8192;
constexpr uint64_t AS_CHUNK = 4096;    // pairs per launch of the association kernels: sf_fuser_align*'s own bound
constexpr uint64_t AS_TOP_PAIRS = 4096;

struct GroupDesc {   // read through the scalar unit (the index is uniform)
  int32_t pair_first, npairs, member_first, n;
  uint32_t valid;
  int32_t pad[3];
};

// one workgroup per running group: the phases of align_solve.h with a barrier between them.  LDS and registers only
__global__ void __launch_bounds__(als::GROUP_THREADS) k_group_solve(const GroupDesc* __restrict__ groups, const uint16_t* __restrict__ lpairs,
                                                                          const int32_t* __restrict__ run, const double* __restrict__ sys, int nsys,
                                                                          double min_corr, als::GroupOut* __restrict__ records) {
  __shared__ als::GroupMem m;
  const int t = threadIdx.x;
  const GroupDesc d = groups[run[blockIdx.x]];
  const als::GroupIn g = {d.n, d.npairs, d.valid, lpairs + d.pair_first, sys + (size_t)d.pair_first * nsys, nsys, min_corr};
  als::GroupOut& o = records[blockIdx.x];
  als::phase_kept(g, m, t);
  __syncthreads();
  als::phase_adjacency(g, m, t);
  __syncthreads();
  als::phase_connect(g, m, t);
  __syncthreads();
  if (m.status == 0) {
    als::phase_clear(m, t);
    __syncthreads();
    als::phase_assemble(g, m, o, t);
    __syncthreads();
    const int N = m.N;
    for (int j = 0; j < N; j++) {
      const double numerator = als::phase_column_a(m, j, t);
      __syncthreads();
      if (m.bad) break;
      als::phase_column_b(m, j, t, numerator);
      __syncthreads();
    }
    if (!m.bad) als::phase_substitute(m, t);
  }
  __syncthreads();
  als::phase_record(g, m, o, t);
}

struct Group {   // the host's side of one group
  int n = 0, first = 0;          // members, first member slot
  int pair_first = 0, npairs = 0;
  uint32_t valid = 0, conn = 0;
  bool running = false, rows_off = false;
  sf_align_result r;
};

struct Layout {   // d_group / h_group: descriptions, local pairs, running list
  size_t pairs_at, run_at, bytes;
};
Layout layout(uint64_t G, uint64_t P) {
  Layout l;
  l.pairs_at = G * sizeof(GroupDesc);
  l.run_at = (l.pairs_at + P * sizeof(uint16_t) + 15) & ~(size_t)15;
  l.bytes = l.run_at + G * sizeof(int32_t);
  return l;
}

int check_groups(uint64_t K, const int32_t* members, const int32_t* group_first, uint64_t G, const sf_align_params* a) {
  if (a->fixed_frame != 0) return sf::fail(SF_ERR_INVALID_ARG, "fixed_frame %d: a group's fixed frame is its first member (0)", a->fixed_frame);
  if (K < 1 || K > AS_MAX_FRAMES) return sf::fail(SF_ERR_INVALID_ARG, "groups over %llu frames (1..%llu)", (unsigned long long)K, (unsigned long long)AS_MAX_FRAMES);
  if (G < 1 || G > AS_MAX_GROUPS) return sf::fail(SF_ERR_INVALID_ARG, "%llu groups (1..%llu)", (unsigned long long)G, (unsigned long long)AS_MAX_GROUPS);
  if (!members || !group_first) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (group_first[0] != 0) return sf::fail(SF_ERR_INVALID_ARG, "group_first[0] = %d (0)", group_first[0]);
  for (uint64_t g = 0; g < G; g++) {
    const int64_t n = (int64_t)group_first[g + 1] - group_first[g];
    if (n < 1 || n > als::GROUP_MAX) return sf::fail(SF_ERR_INVALID_ARG, "group %llu has %lld members (1..%d)", (unsigned long long)g, (long long)n, als::GROUP_MAX);
  }
  const uint64_t M = (uint64_t)group_first[G];
  if (M > AS_MAX_MEMBERS) return sf::fail(SF_ERR_INVALID_ARG, "%llu member slots (at most %llu)", (unsigned long long)M, (unsigned long long)AS_MAX_MEMBERS);
  for (uint64_t k = 0; k < M; k++)
    if (members[k] < 0 || (uint64_t)members[k] >= K) return sf::fail(SF_ERR_INVALID_ARG, "member slot %llu = frame %d of %llu", (unsigned long long)k, members[k], (unsigned long long)K);
  return SF_OK;
}

// every group's pair list by sf_align_pairs' rule over its own poses: local (source, target) per pair, and the groups' ranges
int group_pairs(const int32_t* group_first, uint64_t G, const float* poses_in, const sf_align_params* a, std::vector<Group>& gs, std::vector<int32_t>& local) {
  gs.assign(G, Group());
  local.clear();
  int32_t buf[2 * als::GROUP_MAX_PAIRS];
  for (uint64_t g = 0; g < G; g++) {
    Group& q = gs[g];
    std::memset(&q.r, 0, sizeof(q.r));
    q.first = group_first[g];
    q.n = group_first[g + 1] - group_first[g];
    for (int k = 0; k < q.n; k++)
      if (finite12(poses_in + 16 * (size_t)(q.first + k))) q.valid |= 1u << k;
    uint64_t P = 0;
    if (const int rc = sf_align_pairs(poses_in + 16 * (size_t)q.first, (uint64_t)q.n, a, buf, als::GROUP_MAX_PAIRS, &P)) return rc;
    q.pair_first = (int)(local.size() / 2);
    q.npairs = (int)P;   // at most n (n - 1)
    local.insert(local.end(), buf, buf + 2 * P);
    q.running = q.n >= 2 && P >= 1;
    if (!q.running) q.r.status = 2;
  }
  return SF_OK;
}

// the loop of align.hip's sf_align_solve for all groups at once.  j: the job of the K frames (buffers for P table rows reserved, maps not made yet)
int solve_groups(sf_fuser* f, AlignJob& j, const int32_t* members, uint64_t G, const float* poses_in, const sf_align_params* a, std::vector<Group>& gs,
                 const std::vector<int32_t>& local, float* poses_out) {
  AlignWork* w = f->align;
  const uint64_t M = (uint64_t)(gs[G - 1].first + gs[G - 1].n), P = local.size() / 2;
  std::memcpy(poses_out, poses_in, M * 16 * sizeof(float));
  std::vector<double> T0(M * 12, 0.0);
  for (uint64_t g = 0; g < G; g++)
    for (int k = 0; k < gs[g].n; k++)
      if ((gs[g].valid >> k) & 1u)
        for (int i = 0; i < 12; i++) T0[12 * (size_t)(gs[g].first + k) + i] = (double)poses_in[16 * (size_t)(gs[g].first + k) + i];
  std::vector<double> T = T0;
  int rc;
  if ((rc = sf_align_prepare(f, j)) != SF_OK) return rc;
  j.maps_ready = true;
  if (P == 0) return SF_OK;
  // the groups' descriptions and local pair lists, once
  const Layout l = layout(G, P);
  hipError_t e = w->d_group.reserve(l.bytes);
  if (e == hipSuccess) e = w->h_group.reserve(l.bytes);
  if (e == hipSuccess) e = w->d_record.reserve(G * sizeof(als::GroupOut));
  if (e == hipSuccess) e = w->h_record.reserve(G * sizeof(als::GroupOut));
  if (e != hipSuccess) return sf::fail(SF_ERR_DEVICE, "group solve buffers: %s", hipGetErrorString(e));
  uint8_t* hg = w->h_group.as<uint8_t>();
  GroupDesc* desc = reinterpret_cast<GroupDesc*>(hg);
  uint16_t* lp = reinterpret_cast<uint16_t*>(hg + l.pairs_at);
  int32_t* run = reinterpret_cast<int32_t*>(hg + l.run_at);
  for (uint64_t g = 0; g < G; g++) {
    desc[g] = GroupDesc{gs[g].pair_first, gs[g].npairs, gs[g].first, gs[g].n, gs[g].valid, {0, 0, 0}};
  }
  for (uint64_t p = 0; p < P; p++) lp[p] = (uint16_t)(local[2 * p] | (local[2 * p + 1] << 8));
  SF_HIP_CHECK(hipMemcpyAsync(w->d_group.p, hg, l.run_at, hipMemcpyHostToDevice, f->stream));
  const uint8_t* dg = w->d_group.as<const uint8_t>();
  AlignPair* table = w->h_table.as<AlignPair>();
  const als::GroupOut* rec = w->h_record.as<const als::GroupOut>();
  for (int it = 0; it < a->max_iters; it++) {
    // ONE pair table: a finished group's pairs go in inactive
    uint32_t R = 0;
    for (uint64_t g = 0; g < G; g++) {
      Group& q = gs[g];
      if (!q.running && q.rows_off) continue;
      for (int p = 0; p < q.npairs; p++) {
        const int li = local[2 * (size_t)(q.pair_first + p)], lj = local[2 * (size_t)(q.pair_first + p) + 1];
        const bool active = q.running && ((q.valid >> li) & 1u) && ((q.valid >> lj) & 1u);
        sf_align_pair_row(&table[q.pair_first + p], members[q.first + li], members[q.first + lj], active, &T[12 * (size_t)(q.first + li)], &T[12 * (size_t)(q.first + lj)]);
      }
      q.rows_off = !q.running;
      if (q.running) run[R++] = (int32_t)g;
    }
    if (R == 0) break;
    SF_HIP_CHECK(hipMemcpyAsync(w->d_table.p, table, P * sizeof(AlignPair), hipMemcpyHostToDevice, f->stream));
    SF_HIP_CHECK(hipMemcpyAsync(w->d_group.as<uint8_t>() + l.run_at, run, R * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    for (uint64_t first = 0; first < P; first += AS_CHUNK)
      if ((rc = sf_align_systems(f, j, a, first, P - first < AS_CHUNK ? P - first : AS_CHUNK)) != SF_OK) return rc;
    hipLaunchKernelGGL(k_group_solve, dim3(R), dim3(als::GROUP_THREADS), 0, f->stream, reinterpret_cast<const GroupDesc*>(dg),
                       reinterpret_cast<const uint16_t*>(dg + l.pairs_at), reinterpret_cast<const int32_t*>(dg + l.run_at), w->d_sys.as<const double>(), j.nsys,
                       (double)a->min_pair_correspondences, w->d_record.as<als::GroupOut>());
    SF_HIP_CHECK(hipGetLastError());
    SF_HIP_CHECK(hipMemcpyAsync(w->h_record.p, w->d_record.p, R * sizeof(als::GroupOut), hipMemcpyDeviceToHost, f->stream));
    SF_HIP_CHECK(hipStreamSynchronize(f->stream));
    for (uint32_t s = 0; s < R; s++) {
      Group& q = gs[run[s]];
      const als::GroupOut& o = rec[s];
      sf_align_result& r = q.r;
      q.conn = o.conn;
      if (o.status == 2) { r.status = 2; q.running = false; continue; }
      r.pairs_used = o.used;
      r.correspondences = (int64_t)o.corr;
      r.rms_last = o.corr > 0.0 ? (float)std::sqrt(o.r2 / o.corr) : 0.0f;
      if (it == 0) r.rms_first = r.rms_last;
      r.colour_correspondences = (int64_t)o.ccorr;
      r.colour_rms_last = o.ccorr > 0.0 ? (float)std::sqrt(o.cr2 / o.ccorr) : 0.0f;
      if (it == 0) r.colour_rms_first = r.colour_rms_last;
      if (o.status == 1) { r.status = 1; q.running = false; continue; }
      double mx = 0.0;
      for (int k = 1; k < q.n; k++) {
        if (!((o.conn >> k) & 1u)) continue;
        apply_update(&o.xi[6 * k], &T[12 * (size_t)(q.first + k)]);
        for (int i = 0; i < 6; i++) mx = std::fmax(mx, std::fabs(o.xi[6 * k + i]));
      }
      r.iterations++;
      if (mx < (double)a->early_out || it + 1 == a->max_iters) q.running = false;
    }
  }
  for (uint64_t g = 0; g < G; g++) {
    Group& q = gs[g];
    if (q.n < 2 || q.npairs < 1) continue;   // status 2, every other field 0
    for (int k = 1; k < q.n; k++) {
      const size_t s = (size_t)(q.first + k);
      if (!((q.valid >> k) & 1u)) continue;
      if (!((q.conn >> k) & 1u)) { q.r.frames_unconnected++; continue; }
      if (q.r.status != 0) continue;
      if (!accept_pose(&T0[12 * s], &T[12 * s], (double)a->max_translation, (double)a->max_rotation)) { q.r.frames_rejected++; continue; }
      write_pose16(&T[12 * s], poses_out + 16 * s);
    }
  }
  return SF_OK;
}

// frames: on the device (stride bytes apart) or on the host; the job of the K frames with room for P table rows
int begin_frames(sf_fuser* f, const void* depth, const void* rgb, bool on_device, uint64_t stride, uint64_t rgb_stride, uint64_t K, uint64_t P, const sf_align_params* a,
                 AlignJob* j) {
  const uint64_t rows = P < 1 ? 1 : P;
  return sf_align_begin(f, depth, on_device, stride, true, K, rows, rows < AS_CHUNK ? rows : AS_CHUNK, a, j, rgb != nullptr, rgb, rgb_stride);
}

}  // namespace

SF_API void sf_align_scan_params_default(sf_align_scan_params* s) {
  if (!s) return;
  std::memset(s, 0, sizeof(*s));
  s->group_size = 16;
  s->top_frames = 256;
}

SF_API int sf_align_scan_plan(const float* poses, uint64_t K, const sf_align_params* a, const sf_align_scan_params* s, int32_t* members, uint64_t members_capacity,
                              int32_t* group_first, int32_t* group_level, uint64_t groups_capacity, int32_t* top, uint64_t top_capacity, uint64_t* n_members,
                              uint64_t* n_groups, uint64_t* n_top, int32_t* levels) {
  if (!a || !s || !n_members || !n_groups || !n_top || !levels || (!poses && K > 0)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if ((!members && members_capacity > 0) || ((!group_first || !group_level) && groups_capacity > 0) || (!top && top_capacity > 0))
    return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (s->group_size < 2 || s->group_size > als::GROUP_MAX) return sf::fail(SF_ERR_INVALID_ARG, "group_size %d (2..%d)", s->group_size, als::GROUP_MAX);
  if (s->top_frames < 2 || s->top_frames > 256) return sf::fail(SF_ERR_INVALID_ARG, "top_frames %d (2..256)", s->top_frames);
  if (K > 0x7FFFFFFFull) return sf::fail(SF_ERR_INVALID_ARG, "sf_align_scan_plan: %llu frames", (unsigned long long)K);
  std::vector<int32_t> L;
  for (uint64_t k = 0; k < K; k++)
    if (finite12(poses + 16 * k)) L.push_back((int32_t)k);
  uint64_t M = 0, G = 0;
  int32_t level = 0;
  std::vector<float> lp;
  if (group_first && groups_capacity + 1 > 0) group_first[0] = 0;
  for (;;) {
    bool split = L.size() > (size_t)s->top_frames;
    if (!split) {
      lp.resize(L.size() * 16);
      for (size_t k = 0; k < L.size(); k++) std::memcpy(&lp[16 * k], poses + 16 * (size_t)L[k], 16 * sizeof(float));
      uint64_t P = 0;
      if (const int rc = sf_align_pairs(lp.data(), L.size(), a, nullptr, 0, &P)) return rc;
      split = P > AS_TOP_PAIRS;
    }
    if (!split) break;
    std::vector<int32_t> next;
    for (size_t at = 0; at < L.size(); at += (size_t)s->group_size) {
      const size_t n = L.size() - at < (size_t)s->group_size ? L.size() - at : (size_t)s->group_size;
      for (size_t k = 0; k < n; k++, M++)
        if (M < members_capacity) members[M] = L[at + k];
      if (G < groups_capacity) { group_level[G] = level; group_first[G + 1] = (int32_t)M; }
      G++;
      next.push_back(L[at]);
    }
    L.swap(next);
    level++;
  }
  for (size_t k = 0; k < L.size() && k < top_capacity; k++) top[k] = L[k];
  *n_members = M;
  *n_groups = G;
  *n_top = L.size();
  *levels = level;
  return SF_OK;
}

SF_API int sf_fuser_align_groups_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K,
                                        const int32_t* members, const int32_t* group_first, uint64_t G, const float* poses_in, const sf_align_params* a,
                                        float* poses_out, sf_align_result* results) {
  int rc = sf_align_check_params(a);
  if (rc != SF_OK) return rc;
  if ((rc = check_groups(K, members, group_first, G, a)) != SF_OK) return rc;
  if (!poses_in || !poses_out || !results) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  std::vector<Group> gs;
  std::vector<int32_t> local;
  if ((rc = group_pairs(group_first, G, poses_in, a, gs, local)) != SF_OK) return rc;
  AlignJob j;
  if ((rc = begin_frames(f, d_depth, d_rgb, true, frame_stride_bytes, rgb_stride_bytes, K, local.size() / 2, a, &j)) != SF_OK) return rc;
  if ((rc = solve_groups(f, j, members, G, poses_in, a, gs, local, poses_out)) != SF_OK) return rc;
  for (uint64_t g = 0; g < G; g++) results[g] = gs[g].r;
  return SF_OK;
}

namespace {

int scan(sf_fuser* f, const void* depth, const void* rgb, bool on_device, uint64_t stride, uint64_t rgb_stride, uint64_t K, const float* poses_in,
         const sf_align_params* a, const sf_align_scan_params* s, float* poses_out, sf_align_scan_result* result) {
  int rc = sf_align_check_params(a);
  if (rc != SF_OK) return rc;
  if (!s || !poses_in || !poses_out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (a->fixed_frame != 0) return sf::fail(SF_ERR_INVALID_ARG, "fixed_frame %d: the scan's fixed frame is its first frame with a finite pose (0)", a->fixed_frame);
  if (K < 2 || K > AS_MAX_FRAMES) return sf::fail(SF_ERR_INVALID_ARG, "alignment of a scan of %llu keyframes (2..%llu)", (unsigned long long)K, (unsigned long long)AS_MAX_FRAMES);
  // the plan
  std::vector<int32_t> members(2 * K + 16), group_first(K + 2), group_level(K + 1), top(K);
  uint64_t M = 0, G = 0, nt = 0;
  int32_t levels = 0;
  if ((rc = sf_align_scan_plan(poses_in, K, a, s, members.data(), members.size(), group_first.data(), group_level.data(), K + 1, top.data(), top.size(), &M, &G, &nt,
                               &levels)) != SF_OK)
    return rc;
  if (G > AS_MAX_GROUPS || M > AS_MAX_MEMBERS)
    return sf::fail(SF_ERR_INVALID_ARG, "the plan has %llu groups with %llu members (at most %llu, %llu): choose a larger group_size", (unsigned long long)G, (unsigned long long)M,
                    (unsigned long long)AS_MAX_GROUPS, (unsigned long long)AS_MAX_MEMBERS);
  sf_align_scan_result res;
  std::memset(&res, 0, sizeof(res));
  res.levels = levels;
  res.groups = (int32_t)G;
  // the top's poses and pairs; the groups' slot poses and pairs
  std::vector<float> top_in(nt * 16), top_out(nt * 16), slot_in(M * 16), slot_out(M * 16);
  for (uint64_t k = 0; k < nt; k++) std::memcpy(&top_in[16 * k], poses_in + 16 * (size_t)top[k], 16 * sizeof(float));
  for (uint64_t k = 0; k < M; k++) std::memcpy(&slot_in[16 * k], poses_in + 16 * (size_t)members[k], 16 * sizeof(float));
  std::vector<int32_t> top_pairs(2 * AS_TOP_PAIRS);
  uint64_t Pt = 0;
  if (nt >= 2 && (rc = sf_align_pairs(top_in.data(), nt, a, top_pairs.data(), AS_TOP_PAIRS, &Pt)) != SF_OK) return rc;
  std::vector<Group> gs;
  std::vector<int32_t> local;
  if (G > 0 && (rc = group_pairs(group_first.data(), G, slot_in.data(), a, gs, local)) != SF_OK) return rc;
  const uint64_t Pg = local.size() / 2;
  AlignJob j;
  if ((rc = begin_frames(f, depth, rgb, on_device, stride, rgb_stride, K, Pg > Pt ? Pg : Pt, a, &j)) != SF_OK) return rc;
  std::memcpy(poses_out, poses_in, K * 16 * sizeof(float));
  if (G > 0) {
    if ((rc = solve_groups(f, j, members.data(), G, slot_in.data(), a, gs, local, slot_out.data())) != SF_OK) return rc;
    for (uint64_t g = 0; g < G; g++) {
      const sf_align_result& r = gs[g].r;
      res.groups_status[r.status]++;
      if (r.iterations > res.max_iterations) res.max_iterations = r.iterations;
      res.frames_unconnected += r.frames_unconnected;
      res.frames_rejected += r.frames_rejected;
      res.correspondences += r.correspondences;
    }
  }
  // the top by sf_fuser_align*'s own loop, on the maps that are there already
  res.top.status = 2;
  if (nt >= 2) {
    // the top's index list reaches every one of the K frames: without a grouping level their maps are made here, all K of them
    if (!j.maps_ready && (rc = sf_align_prepare(f, j)) != SF_OK) return rc;
    j.maps_ready = true;
    AlignJob jt = j;
    jt.K = nt;
    jt.P = Pt;
    jt.pairs = top_pairs.data();
    jt.remap = top.data();
    if ((rc = sf_align_solve(f, jt, top_in.data(), a, top_out.data(), &res.top)) != SF_OK) return rc;
    if (res.top.iterations > res.max_iterations) res.max_iterations = res.top.iterations;
    res.frames_unconnected += res.top.frames_unconnected;
    res.frames_rejected += res.top.frames_rejected;
    res.correspondences += res.top.correspondences;
    for (uint64_t k = 0; k < nt; k++) std::memcpy(poses_out + 16 * (size_t)top[k], &top_out[16 * k], 16 * sizeof(float));
  }
  // the corrections carried down: the highest level first; a group's first member has its new pose by then
  const uint64_t key0 = 0;
  float spread[16 * als::GROUP_MAX];
  for (int32_t lv = levels - 1; lv >= 0; lv--)
    for (uint64_t g = 0; g < G; g++) {
      if (group_level[g] != lv) continue;
      const int n = gs[g].n, at = gs[g].first;
      if ((rc = sf_align_spread(&slot_out[16 * (size_t)at], (uint64_t)n, &key0, 1, poses_out + 16 * (size_t)members[at], spread)) != SF_OK) return rc;
      for (int k = 1; k < n; k++) std::memcpy(poses_out + 16 * (size_t)members[at + k], spread + 16 * k, 16 * sizeof(float));
    }
  if (result) *result = res;
  return SF_OK;
}

}  // namespace

SF_API int sf_fuser_align_scan_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K,
                                      const float* poses_in, const sf_align_params* a, const sf_align_scan_params* s, float* poses_out, sf_align_scan_result* result) {
  return scan(f, d_depth, d_rgb, true, frame_stride_bytes, rgb_stride_bytes, K, poses_in, a, s, poses_out, result);
}

SF_API int sf_fuser_align_scan(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, uint64_t K, const float* poses_in, const sf_align_params* a,
                               const sf_align_scan_params* s, float* poses_out, sf_align_scan_result* result) {
  return scan(f, depth, rgb, false, 0, 0, K, poses_in, a, s, poses_out, result);
}

// ---- the stage hook: k_group_solve alone --------------------------------------------------------------------------------------------------
SF_API int sf_align_group_solve_stage(int device, uint64_t G, const int32_t* group_first, const int32_t* pair_first, const int32_t* local_pairs,
                                      const uint32_t* valid_masks, const double* sys, int nsys, int min_pair_correspondences, double* xi_out, int32_t* status_out,
                                      int32_t* used_out, uint32_t* conn_out, double* sums_out) {
  if (!group_first || !pair_first || !valid_masks || !xi_out || !status_out || !used_out || !conn_out || !sums_out) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (G < 1 || G > AS_MAX_GROUPS) return sf::fail(SF_ERR_INVALID_ARG, "%llu groups (1..%llu)", (unsigned long long)G, (unsigned long long)AS_MAX_GROUPS);
  if (nsys != TK_NSYS && nsys != TK_NSYS_RGBD) return sf::fail(SF_ERR_INVALID_ARG, "%d values per pair (29 or 31)", nsys);
  if (group_first[0] != 0 || pair_first[0] != 0) return sf::fail(SF_ERR_INVALID_ARG, "group_first[0] and pair_first[0] must be 0");
  for (uint64_t g = 0; g < G; g++) {
    const int64_t n = (int64_t)group_first[g + 1] - group_first[g], np = (int64_t)pair_first[g + 1] - pair_first[g];
    if (n < 1 || n > als::GROUP_MAX || np < 0 || np > als::GROUP_MAX_PAIRS)
      return sf::fail(SF_ERR_INVALID_ARG, "group %llu: %lld members (1..%d), %lld pairs (0..%d)", (unsigned long long)g, (long long)n, als::GROUP_MAX, (long long)np, als::GROUP_MAX_PAIRS);
    for (int64_t p = pair_first[g]; p < pair_first[g + 1]; p++) {
      if (!local_pairs) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
      const int32_t i = local_pairs[2 * p], k = local_pairs[2 * p + 1];
      if (i < 0 || k < 0 || i >= n || k >= n || i == k) return sf::fail(SF_ERR_INVALID_ARG, "pair %lld = (%d, %d) of a group of %lld", (long long)p, i, k, (long long)n);
    }
  }
  const uint64_t P = (uint64_t)pair_first[G];
  if (P > 0 && !sys) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  SF_HIP_CHECK(hipSetDevice(device));
  const Layout l = layout(G, P);
  std::vector<uint8_t> hg(l.bytes, 0);
  GroupDesc* desc = reinterpret_cast<GroupDesc*>(hg.data());
  uint16_t* lp = reinterpret_cast<uint16_t*>(hg.data() + l.pairs_at);
  int32_t* run = reinterpret_cast<int32_t*>(hg.data() + l.run_at);
  for (uint64_t g = 0; g < G; g++) {
    desc[g] = GroupDesc{pair_first[g], pair_first[g + 1] - pair_first[g], group_first[g], group_first[g + 1] - group_first[g], valid_masks[g], {0, 0, 0}};
    run[g] = (int32_t)g;
  }
  for (uint64_t p = 0; p < P; p++) lp[p] = (uint16_t)(local_pairs[2 * p] | (local_pairs[2 * p + 1] << 8));
  sf::DevBuf dg, ds, dr;
  hipError_t e = dg.reserve(l.bytes);
  if (e == hipSuccess) e = ds.reserve((P ? P : 1) * nsys * sizeof(double));
  if (e == hipSuccess) e = dr.reserve(G * sizeof(als::GroupOut));
  if (e != hipSuccess) return sf::fail(SF_ERR_DEVICE, "stage buffers: %s", hipGetErrorString(e));
  SF_HIP_CHECK(hipMemcpy(dg.p, hg.data(), l.bytes, hipMemcpyHostToDevice));
  if (P) SF_HIP_CHECK(hipMemcpy(ds.p, sys, P * nsys * sizeof(double), hipMemcpyHostToDevice));
  const uint8_t* d = dg.as<const uint8_t>();
  hipLaunchKernelGGL(k_group_solve, dim3((unsigned)G), dim3(als::GROUP_THREADS), 0, 0, reinterpret_cast<const GroupDesc*>(d),
                     reinterpret_cast<const uint16_t*>(d + l.pairs_at), reinterpret_cast<const int32_t*>(d + l.run_at), ds.as<const double>(), nsys,
                     (double)min_pair_correspondences, dr.as<als::GroupOut>());
  SF_HIP_CHECK(hipGetLastError());
  std::vector<als::GroupOut> rec(G);
  SF_HIP_CHECK(hipMemcpy(rec.data(), dr.p, G * sizeof(als::GroupOut), hipMemcpyDeviceToHost));
  for (uint64_t g = 0; g < G; g++) {
    const int n = group_first[g + 1] - group_first[g];
    std::memcpy(xi_out + 6 * (size_t)group_first[g], rec[g].xi, 6 * (size_t)n * sizeof(double));
    status_out[g] = rec[g].status;
    used_out[g] = rec[g].used;
    conn_out[g] = rec[g].conn;
    sums_out[4 * g] = rec[g].corr; sums_out[4 * g + 1] = rec[g].r2; sums_out[4 * g + 2] = rec[g].ccorr; sums_out[4 * g + 3] = rec[g].cr2;
  }
  return SF_OK;
}
