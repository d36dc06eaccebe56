// align.hip -- global alignment: K keyframes aligned jointly over a list of directed frame pairs by a depth-only projective point-to-plane term
// (DESIGN.md "Global alignment"; BundleFusion's dense depth term between keyframes, zParametersBundlingScanNet.txt:22-44).
//
// Once per call: k_align_prep turns every keyframe into a camera-space vertex and a normal map at the one level the solver works at (the tracker's
// rules, track_math.h).  Per Gauss-Newton iteration: the host writes the pair table (indices, T_i, T_j, T_j^-1 T_i) and copies it over; k_align_assoc
// pairs every source pixel of every pair with the target pixel it projects to and reduces the pair's 29 values per 256-pixel workgroup (no atomics);
// k_align_final sums a pair's partials in index order in double; one read-back.  The host drops thin pairs, finds the frames connected to the fixed
// frame, assembles the sparse-by-blocks normal equations densely and solves them by Cholesky in double (align_solve.h states each entry's arithmetic
// once, for this loop and for align_scan.hip's group solve on the device).  Every step is deterministic and
// tests/align_checker.c restates it bit for bit.  sf_fuser_align_rgbd* run the same host loop over the kernels' colour instantiation, which adds the
// dense colour term's row to every correspondence and two sums to the pair's values (align_colour.hip makes the intensity maps).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "align_internal.h"
#include "common.h"
#include "photo_math.h"
#include "scanfuse_internal.h"

namespace {

using namespace tk;

constexpr int AL_MAX_FRAMES = 256;
constexpr int AL_MAX_PAIRS = 4096;

using PairEntry = AlignPair;   // one row of the device table; read through the scalar unit (the index is blockIdx.y)

// depth of pixel (x, y) of level L of a frame in metres: level 0 from the u16 frame, level L the 2x2 reduction of level L - 1
template <int L>
__device__ inline float level_depth(const uint16_t* __restrict__ in, const ParamsK& P, int x, int y) {
  if constexpr (L == 0) {
    return depth0_at(in, P, y * P.W + x);
  } else {
    const float s00 = level_depth<L - 1>(in, P, 2 * x, 2 * y);
    if (!(s00 > 0.0f)) return -INFINITY;   // down4 reads nothing else of an invalid reference pixel
    return down4(s00, level_depth<L - 1>(in, P, 2 * x + 1, 2 * y), level_depth<L - 1>(in, P, 2 * x, 2 * y + 1), level_depth<L - 1>(in, P, 2 * x + 1, 2 * y + 1));
  }
}

// the level's depth behind the solver's own gate
template <int L>
__device__ inline float gated_depth(const uint16_t* __restrict__ in, const ParamsK& P, int x, int y, float dmin, float dmax) {
  const float d = level_depth<L>(in, P, x, y);
  return (d >= dmin && d <= dmax) ? d : -INFINITY;
}

// all K frames at once (blockIdx.y = frame): u16 -> metres -> L reductions -> vertex and normal map of level L
template <int L>
__global__ void __launch_bounds__(256) k_align_prep(const uint8_t* __restrict__ frames, size_t frame_stride, const ParamsK P, const Cam c, float dmin, float dmax,
                                                    float4* __restrict__ vmap, float4* __restrict__ nmap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int npx = c.W * c.H;
  if (i >= npx) return;
  const uint16_t* in = reinterpret_cast<const uint16_t*>(frames + (size_t)blockIdx.y * frame_stride);
  const int x = i % c.W, y = i / c.W;
  const float dz = gated_depth<L>(in, P, x, y, dmin, dmax);
  const bool nb = dz > 0.0f && x + 1 < c.W && y + 1 < c.H;
  const float dr = nb ? gated_depth<L>(in, P, x + 1, y, dmin, dmax) : 0.0f;
  const float dd = nb ? gated_depth<L>(in, P, x, y + 1, dmin, dmax) : 0.0f;
  float4 vo, no;
  vertex_normal(c, x, y, dz, nb, dr, dd, &vo, &no);
  const size_t o = (size_t)blockIdx.y * npx + i;
  vmap[o] = vo;
  nmap[o] = no;
}

// one pair per blockIdx.y: association of the source frame's pixels with the target frame's maps and the pair's point-to-plane rows, reduced to one
// 29-float partial per 256-pixel workgroup; partials[P][nb][32].  COLOUR: 31 floats, with the colour row of the correspondence in the same lane;
// photo == nullptr: no colour rows
template <bool COLOUR>
__global__ void __launch_bounds__(256) k_align_assoc(const float4* __restrict__ vmap, const float4* __restrict__ nmap, const float4* __restrict__ photo,
                                                     const PairEntry* __restrict__ table, const Cam c, float dist_thres, float normal_thres, float weight,
                                                     float colour_thres, float gradient_min, float* __restrict__ partials) {
  constexpr int N = nsys_of<COLOUR>;
  __shared__ float red[4][N];
  const PairEntry& e = table[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int npx = c.W * c.H;
  float acc[N];
#pragma unroll
  for (int k = 0; k < N; k++) acc[k] = 0.0f;
  if (e.active && i < npx) {
    const size_t so = (size_t)e.i * npx, to = (size_t)e.j * npx;
    const float4 v4 = vmap[so + i];
    // the target is frame j's maps at the same level, moved to the world by T_j
    const bool hit = correspond(c, e.Ti, e.M, v4, nmap[so + i], dist_thres, normal_thres, [&](int ux, int uy, float3* q, float3* nm) {
      const size_t t = to + (size_t)(uy * c.W + ux);
      const float4 w4 = vmap[t], m4 = nmap[t];
      if (!(w4.z > 0.0f && m4.x > -INFINITY)) return false;
      *q = xf(e.Tj, make_float3(w4.x, w4.y, w4.z));
      *nm = rot(e.Tj, make_float3(m4.x, m4.y, m4.z));
      return true;
    }, acc);
    if constexpr (COLOUR) {
      if (hit && photo) {
        const float Is = photo[so + i].x;
        const float3 v = make_float3(v4.x, v4.y, v4.z);
        colour_row(photo + to, c, e.Tj, Is, xf(e.Ti, v), xf(e.M, v), weight, colour_thres, gradient_min, acc);
      }
    }
  }
  reduce256(acc, red, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * TK_PSTRIDE);
}

// one wave per pair: lane k sums value k of the pair's partials in index order, in double; out[P][29 or 31]
template <bool COLOUR>
__global__ void __launch_bounds__(64) k_align_final(const float* __restrict__ partials, int nb, double* __restrict__ out) {
  constexpr int N = nsys_of<COLOUR>;
  const int k = threadIdx.x;
  if (k < N) out[(size_t)blockIdx.x * N + k] = sum_partials(partials + (size_t)blockIdx.x * nb * TK_PSTRIDE, nb, k);
}

}  // namespace

void sf_align_release(sf_fuser* f) {
  if (!f) return;
  delete f->align;
  f->align = nullptr;
}

namespace {

// what can be checked without a fuser
int check_params(const sf_align_params* a) {
  if (!a) return sf::fail(SF_ERR_INVALID_ARG, "NULL alignment parameters");
  if (a->level < 0 || a->level >= TK_MAX_LEVELS) return sf::fail(SF_ERR_INVALID_ARG, "alignment level %d (0..3)", a->level);
  if (a->down_width < 0 || a->down_height < 0 || (a->down_width == 0) != (a->down_height == 0))
    return sf::fail(SF_ERR_INVALID_ARG, "alignment down_width x down_height %d x %d: both 0 or both positive", a->down_width, a->down_height);
  if (a->max_iters < 1 || a->max_iters > 100) return sf::fail(SF_ERR_INVALID_ARG, "alignment max_iters %d (1..100)", a->max_iters);
  if (!std::isfinite(a->dist_thres) || !(a->dist_thres > 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "alignment dist_thres %g: not a positive finite number", a->dist_thres);
  if (!(a->normal_thres >= -1.0f && a->normal_thres <= 1.0f)) return sf::fail(SF_ERR_INVALID_ARG, "alignment normal_thres %g (-1..1)", a->normal_thres);
  if (!std::isfinite(a->depth_min) || !std::isfinite(a->depth_max) || a->depth_min < 0.0f || a->depth_max < a->depth_min)
    return sf::fail(SF_ERR_INVALID_ARG, "alignment depth range %g .. %g", a->depth_min, a->depth_max);
  if (!std::isfinite(a->early_out) || !(a->early_out >= 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "alignment early_out %g: not a finite number >= 0", a->early_out);
  if (a->min_pair_correspondences < 1) return sf::fail(SF_ERR_INVALID_ARG, "min_pair_correspondences %d (>= 1)", a->min_pair_correspondences);
  if (!std::isfinite(a->max_translation) || !(a->max_translation > 0.0f) || !std::isfinite(a->max_rotation) || !(a->max_rotation > 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "alignment motion bound %g m, %g rad: not positive finite numbers", a->max_translation, a->max_rotation);
  return SF_OK;
}

int check_align_args(uint64_t K, const float* poses, const int32_t* pairs, uint64_t P, const sf_align_params* a) {
  if (const int rc = check_params(a)) return rc;
  if (K < 2 || K > (uint64_t)AL_MAX_FRAMES) return sf::fail(SF_ERR_INVALID_ARG, "alignment of %llu frames (2..%d)", (unsigned long long)K, AL_MAX_FRAMES);
  if (a->fixed_frame < 0 || (uint64_t)a->fixed_frame >= K) return sf::fail(SF_ERR_INVALID_ARG, "fixed_frame %d of %llu frames", a->fixed_frame, (unsigned long long)K);
  if (P < 1 || P > (uint64_t)AL_MAX_PAIRS) return sf::fail(SF_ERR_INVALID_ARG, "alignment over %llu pairs (1..%d)", (unsigned long long)P, AL_MAX_PAIRS);
  if (!poses || !pairs) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  for (uint64_t p = 0; p < P; p++) {
    const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
    if (i < 0 || j < 0 || (uint64_t)i >= K || (uint64_t)j >= K || i == j)
      return sf::fail(SF_ERR_INVALID_ARG, "pair %llu = (%d, %d): two different frames of 0..%llu", (unsigned long long)p, i, j, (unsigned long long)(K - 1));
  }
  return SF_OK;
}

// the level on this fuser and its camera (the tracker's level intrinsics)
int resolve_level(const sf_fuser* f, const sf_align_params* a, int* level, Cam* cam) {
  const int W = f->pk.W, H = f->pk.H;
  int l = a->level;
  if (a->down_width > 0) {
    l = -1;
    for (int k = 0; k < TK_MAX_LEVELS; k++)
      if ((W >> k) == a->down_width && (H >> k) == a->down_height) { l = k; break; }
    if (l < 0) return sf::fail(SF_ERR_INVALID_ARG, "alignment down_width x down_height %d x %d is no level 0..3 of %d x %d", a->down_width, a->down_height, W, H);
  }
  if (!level_cam(f->pk, l, cam)) return sf::fail(SF_ERR_INVALID_ARG, "alignment level %d would be %d x %d (at least 8 x 8)", l, cam->W, cam->H);
  *level = l;
  return SF_OK;
}

// the colour pictures the fuser fuses: color_width x color_height, or the integration size
uint64_t picture_bytes(const sf_fuser* f) { return (f->pk.cW ? (uint64_t)f->pk.cW * f->pk.cH : (uint64_t)f->pk.W * f->pk.H) * 3; }

// nsys: 29, or 31 with the colour term's sums; host_rgb / photo: the pictures come from the host / there are pictures at all
// P: rows of the pair table and of the systems; chunk: the most pairs one launch takes (0: P)
int ensure_work(sf_fuser* f, uint64_t K, uint64_t P, int npx, bool host_frames, int nsys = TK_NSYS, bool host_rgb = false, bool photo = false, uint64_t chunk = 0) {
  if (!f->align) f->align = new AlignWork();
  AlignWork* w = f->align;
  const size_t map_bytes = (size_t)K * npx * sizeof(float4);
  hipError_t e = w->d_in.reserve(host_frames ? (size_t)K * f->in_px * sizeof(uint16_t) : 0);
  if (e == hipSuccess) e = w->d_rgb.reserve(host_rgb ? (size_t)K * picture_bytes(f) : 0);
  if (e == hipSuccess) e = w->photo.reserve(photo ? map_bytes : 0);
  if (e == hipSuccess) e = w->vmap.reserve(map_bytes);
  if (e == hipSuccess) e = w->nmap.reserve(map_bytes);
  if (e == hipSuccess) e = w->partials.reserve((size_t)(chunk ? chunk : P) * ((npx + 255) / 256) * TK_PSTRIDE * sizeof(float));
  if (e == hipSuccess) e = w->d_table.reserve(P * sizeof(PairEntry));
  if (e == hipSuccess) e = w->h_table.reserve(P * sizeof(PairEntry));
  if (e == hipSuccess) e = w->d_sys.reserve(P * nsys * sizeof(double));
  if (e == hipSuccess) e = w->h_sys.reserve(P * nsys * sizeof(double));
  if (e != hipSuccess) { sf_align_release(f); return sf::fail(SF_ERR_DEVICE, "alignment buffers: %s", hipGetErrorString(e)); }
  return SF_OK;
}

using Job = AlignJob;

}  // namespace

// the maps of all K frames, queued on f->stream behind everything queued on the handle so far
int sf_align_prepare(sf_fuser* f, const AlignJob& j) {
  AlignWork* w = f->align;
  // the maps read no volume, so nothing queued later on the front streams has to wait for them
  if (const int oc = sf_order_behind_fronts(f)) return oc;
  const int npx = j.cam.W * j.cam.H;
  const dim3 grid((npx + 255) / 256, (unsigned)j.K);
#define AL_PREP(L)                                                                                                                           \
  hipLaunchKernelGGL(k_align_prep<L>, grid, dim3(256), 0, f->stream, (const uint8_t*)j.d_depth, (size_t)j.stride, f->pk, j.cam, j.dmin, j.dmax, \
                     w->vmap.as<float4>(), w->nmap.as<float4>())
  switch (j.level) {
    case 0: AL_PREP(0); break;
    case 1: AL_PREP(1); break;
    case 2: AL_PREP(2); break;
    default: AL_PREP(3); break;
  }
#undef AL_PREP
  SF_HIP_CHECK(hipGetLastError());
  return j.d_rgb ? sf_photo_prepare(f, j.d_rgb, j.rgb_stride, j.K, j.level, j.cam) : SF_OK;
}

// rows first .. first + count - 1 of w->d_table into the same rows of w->d_sys, queued on f->stream; count <= AL_MAX_PAIRS
// j.nsys 31: the kernels' colour instantiation, with colour rows when the job has pictures (without: the depth term's bits, the colour sums 0)
int sf_align_systems(sf_fuser* f, const AlignJob& j, const sf_align_params* a, uint64_t first, uint64_t count) {
  AlignWork* w = f->align;
  const bool rgbd = j.nsys == TK_NSYS_RGBD;
  const int npx = j.cam.W * j.cam.H, nb = (npx + 255) / 256;
  hipLaunchKernelGGL(rgbd ? k_align_assoc<true> : k_align_assoc<false>, dim3(nb, (unsigned)count), dim3(256), 0, f->stream, w->vmap.as<const float4>(),
                     w->nmap.as<const float4>(), j.d_rgb ? w->photo.as<const float4>() : nullptr, w->d_table.as<const PairEntry>() + first, j.cam, a->dist_thres,
                     a->normal_thres, a->colour_weight, a->colour_thres, a->colour_gradient_min, w->partials.as<float>());
  SF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rgbd ? k_align_final<true> : k_align_final<false>, dim3((unsigned)count), dim3(64), 0, f->stream, w->partials.as<const float>(), nb,
                     w->d_sys.as<double>() + first * j.nsys);
  SF_HIP_CHECK(hipGetLastError());
  return SF_OK;
}

// one row of the pair table: frames fi -> fj of the maps at the poses Ti, Tj (12 doubles each); active: both frames take part
void sf_align_pair_row(AlignPair* e, int32_t fi, int32_t fj, bool active, const double* Ti, const double* Tj) {
  std::memset(e, 0, sizeof(*e));
  e->i = fi;
  e->j = fj;
  e->active = active;
  if (!active) return;
  for (int k = 0; k < 12; k++) { e->Ti.T[k] = (float)Ti[k]; e->Tj.T[k] = (float)Tj[k]; }
  compose_ref(Tj, Ti, e->M.T);
}

namespace {

int prepare(sf_fuser* f, const Job& j) { return j.maps_ready ? SF_OK : sf_align_prepare(f, j); }

// the P systems at the poses T (K x 12 doubles; valid[k]: the frame takes part) into w->h_sys
int systems_at(sf_fuser* f, const Job& j, const double* T, const uint8_t* valid, const sf_align_params* a) {
  AlignWork* w = f->align;
  for (uint64_t p = 0; p < j.P; p++) {
    const int32_t pi = j.pairs[2 * p], pj = j.pairs[2 * p + 1];
    sf_align_pair_row(&w->h_table.as<PairEntry>()[p], j.remap ? j.remap[pi] : pi, j.remap ? j.remap[pj] : pj, valid[pi] && valid[pj], T + 12 * pi, T + 12 * pj);
  }
  SF_HIP_CHECK(hipMemcpyAsync(w->d_table.p, w->h_table.p, j.P * sizeof(PairEntry), hipMemcpyHostToDevice, f->stream));
  if (const int rc = sf_align_systems(f, j, a, 0, j.P)) return rc;
  SF_HIP_CHECK(hipMemcpyAsync(w->h_sys.p, w->d_sys.p, j.P * j.nsys * sizeof(double), hipMemcpyDeviceToHost, f->stream));
  SF_HIP_CHECK(hipStreamSynchronize(f->stream));
  return SF_OK;
}

int find_root(std::vector<int>& parent, int k) {
  while (parent[k] != k) k = parent[k] = parent[parent[k]];
  return k;
}

}  // namespace

// sf_fuser_align*'s Gauss-Newton loop over the job's pair list (align_scan.hip runs it for the top of a scan)
int sf_align_solve(sf_fuser* f, const AlignJob& j, const float* poses_in, const sf_align_params* a, float* poses_out, sf_align_result* res) {
  int rc;
  const uint64_t K = j.K;
  sf_align_result r;
  std::memset(&r, 0, sizeof(r));
  std::memcpy(poses_out, poses_in, K * 16 * sizeof(float));
  std::vector<double> T0(K * 12), T(K * 12);
  std::vector<uint8_t> valid(K);
  for (uint64_t k = 0; k < K; k++) {
    valid[k] = finite12(poses_in + 16 * k);
    for (int i = 0; i < 12; i++) T0[12 * k + i] = valid[k] ? (double)poses_in[16 * k + i] : 0.0;
  }
  T = T0;
  if ((rc = prepare(f, j)) != SF_OK) return rc;
  const double* sys = f->align->h_sys.as<const double>();
  const int fixed = a->fixed_frame;
  const size_t ns = (size_t)j.nsys;   // the loop reads a pair's first 29 values; the colour term's two only for the result
  std::vector<uint8_t> kept(j.P), conn(K, 0);
  std::vector<int> parent(K), slot(K);
  std::vector<double> A, b, y, xi;
  for (int it = 0; it < a->max_iters; it++) {
    if ((rc = systems_at(f, j, T.data(), valid.data(), a)) != SF_OK) return rc;
    for (uint64_t k = 0; k < K; k++) parent[k] = (int)k;
    for (uint64_t p = 0; p < j.P; p++) {
      const int pi = j.pairs[2 * p], pj = j.pairs[2 * p + 1];
      kept[p] = valid[pi] && valid[pj] && sys[p * ns + 28] >= (double)a->min_pair_correspondences;
      if (!kept[p]) continue;
      const int ra = find_root(parent, pi), rb = find_root(parent, pj);
      if (ra != rb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;   // the smaller index is the root
    }
    const int rf = find_root(parent, fixed);
    int n = 0, nconn = 0;
    for (uint64_t k = 0; k < K; k++) {
      conn[k] = valid[k] && find_root(parent, (int)k) == rf;
      slot[k] = -1;
      if (conn[k]) { nconn++; if ((int)k != fixed) slot[k] = n++; }
    }
    if (!valid[fixed] || nconn < 2) { r.status = 2; break; }
    const int N = 6 * n;
    A.assign(als::tri(N, 0), 0.0);   // the lower triangle, packed (align_solve.h)
    b.assign(N, 0.0);
    int used = 0;
    double corr = 0.0, r2 = 0.0, ccorr = 0.0, cr2 = 0.0;
    for (uint64_t p = 0; p < j.P; p++) {
      const int pi = j.pairs[2 * p], pj = j.pairs[2 * p + 1];
      if (!kept[p] || !conn[pi]) continue;
      const double* s = sys + p * ns;
      const int si = slot[pi], sj = slot[pj];
      for (int u = 0; u < 6; u++) {
        for (int v = 0; v < 6; v++) {
          als::assemble_diag(A.data(), si, sj, u, v, s[als::sym21(u, v)]);
          als::assemble_off(A.data(), si, sj, u, v, s[als::sym21(u, v)]);
        }
        als::assemble_rhs(b.data(), si, sj, u, s[21 + u]);
      }
      used++;
      r2 += s[27];
      corr += s[28];
      if (j.nsys == TK_NSYS_RGBD) { cr2 += s[29]; ccorr += s[30]; }
    }
    r.pairs_used = used;
    r.correspondences = (int64_t)corr;
    r.rms_last = corr > 0.0 ? (float)std::sqrt(r2 / corr) : 0.0f;
    if (it == 0) r.rms_first = r.rms_last;
    r.colour_correspondences = (int64_t)ccorr;
    r.colour_rms_last = ccorr > 0.0 ? (float)std::sqrt(cr2 / ccorr) : 0.0f;
    if (it == 0) r.colour_rms_first = r.colour_rms_last;
    xi.resize(N);
    y.resize(N);
    if (!als::solve_packed(A.data(), b.data(), N, y.data(), xi.data())) { r.status = 1; break; }
    double mx = 0.0;
    for (uint64_t k = 0; k < K; k++)
      if (slot[k] >= 0) apply_update(&xi[6 * slot[k]], &T[12 * k]);
    for (int k = 0; k < N; k++) mx = std::fmax(mx, std::fabs(xi[k]));
    r.iterations++;
    if (mx < (double)a->early_out) break;
  }
  // a frame with a finite pose that the last system did not reach, or that moved beyond the bounds, keeps its input pose
  for (uint64_t k = 0; k < K; k++) {
    if (!valid[k] || (int)k == fixed) continue;
    if (!conn[k]) { r.frames_unconnected++; continue; }
    if (r.status != 0) continue;
    if (!accept_pose(&T0[12 * k], &T[12 * k], (double)a->max_translation, (double)a->max_rotation)) { r.frames_rejected++; continue; }
    write_pose16(&T[12 * k], poses_out + 16 * k);
  }
  if (res) *res = r;
  return SF_OK;
}

namespace {

// the colour term's three parameters, which only the rgbd entry points read
int check_colour_args(const sf_align_params* a, const void* rgb) {
  if (!std::isfinite(a->colour_weight) || !(a->colour_weight >= 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "alignment colour_weight %g: not a finite number >= 0", a->colour_weight);
  if (!std::isfinite(a->colour_thres) || !(a->colour_thres >= 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "alignment colour_thres %g: not a finite number >= 0", a->colour_thres);
  if (!std::isfinite(a->colour_gradient_min) || !(a->colour_gradient_min >= 0.0f))
    return sf::fail(SF_ERR_INVALID_ARG, "alignment colour_gradient_min %g: not a finite number >= 0", a->colour_gradient_min);
  if (!rgb && a->colour_weight > 0.0f) return sf::fail(SF_ERR_INVALID_ARG, "alignment colour_weight %g without colour pictures", a->colour_weight);
  return SF_OK;
}

// what the entry points share: the checks in their order, the job, the device, the buffers and, for frames on the host, their copy into w->d_in (and
// w->d_rgb).  rgbd: the call is one of sf_fuser_align_rgbd*; rgb may still be NULL (colour_weight 0)
int begin(sf_fuser* f, const void* depth, bool on_device, uint64_t stride, bool out_ok, uint64_t K, const float* poses, const int32_t* pairs, uint64_t P,
          const sf_align_params* a, Job* j, bool rgbd = false, const void* rgb = nullptr, uint64_t rgb_stride = 0) {
  int rc = check_align_args(K, poses, pairs, P, a);
  if (rc != SF_OK) return rc;
  j->pairs = pairs;
  return sf_align_begin(f, depth, on_device, stride, out_ok, K, P, 0, a, j, rgbd, rgb, rgb_stride);
}

}  // namespace

int sf_align_check_params(const sf_align_params* a) { return check_params(a); }

// what follows the checks of the pair list: the colour arguments, the handle, the strides, the level, the device, the buffers (P table rows, `chunk`
// pairs per launch, 0: P) and, for frames on the host, their copy into w->d_in (and w->d_rgb)
int sf_align_begin(sf_fuser* f, const void* depth, bool on_device, uint64_t stride, bool out_ok, uint64_t K, uint64_t P, uint64_t chunk, const sf_align_params* a,
                   AlignJob* j, bool rgbd, const void* rgb, uint64_t rgb_stride) {
  int rc;
  if (rgbd && (rc = check_colour_args(a, rgb)) != SF_OK) return rc;
  if (!f) return sf::fail(SF_ERR_INVALID_ARG, "NULL fuser");
  if (!depth || !out_ok) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (rgb && on_device && rgb_stride < picture_bytes(f))
    return sf::fail(SF_ERR_INVALID_ARG, "picture stride %llu bytes for pictures of %llu", (unsigned long long)rgb_stride, (unsigned long long)picture_bytes(f));
  const uint64_t frame_bytes = f->in_px * sizeof(uint16_t);
  if (on_device && (stride < frame_bytes || stride % sizeof(uint16_t)))
    return sf::fail(SF_ERR_INVALID_ARG, "frame stride %llu bytes for frames of %llu", (unsigned long long)stride, (unsigned long long)frame_bytes);
  j->K = K; j->P = P;
  if ((rc = resolve_level(f, a, &j->level, &j->cam)) != SF_OK) return rc;
  const bool own = a->depth_min == 0.0f && a->depth_max == 0.0f;
  j->dmin = own ? f->pk.dmin : a->depth_min;
  j->dmax = own ? f->pk.dmax : a->depth_max;
  SF_HIP_CHECK(hipSetDevice(f->device));
  j->nsys = rgbd ? TK_NSYS_RGBD : TK_NSYS;
  if ((rc = ensure_work(f, K, P, j->cam.W * j->cam.H, !on_device, j->nsys, rgb && !on_device, rgb != nullptr, chunk)) != SF_OK) return rc;
  j->d_depth = depth;
  j->stride = stride;
  j->d_rgb = rgb;
  j->rgb_stride = rgb_stride;
  if (!on_device) {
    j->d_depth = f->align->d_in.p;
    j->stride = frame_bytes;
    SF_HIP_CHECK(hipMemcpyAsync(f->align->d_in.p, depth, K * frame_bytes, hipMemcpyHostToDevice, f->stream));
    if (rgb) {
      j->d_rgb = f->align->d_rgb.p;
      j->rgb_stride = picture_bytes(f);
      SF_HIP_CHECK(hipMemcpyAsync(f->align->d_rgb.p, rgb, K * picture_bytes(f), hipMemcpyHostToDevice, f->stream));
    }
  }
  return SF_OK;
}

SF_API int sf_fuser_align_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, uint64_t K, const float* poses_in, const int32_t* pairs, uint64_t P,
                                 const sf_align_params* a, float* poses_out, sf_align_result* result) {
  Job j;
  const int rc = begin(f, d_depth, true, frame_stride_bytes, poses_out != nullptr, K, poses_in, pairs, P, a, &j);
  return rc != SF_OK ? rc : sf_align_solve(f, j, poses_in, a, poses_out, result);
}

SF_API int sf_fuser_align(sf_fuser* f, const uint16_t* depth, uint64_t K, const float* poses_in, const int32_t* pairs, uint64_t P, const sf_align_params* a,
                          float* poses_out, sf_align_result* result) {
  Job j;
  const int rc = begin(f, depth, false, 0, poses_out != nullptr, K, poses_in, pairs, P, a, &j);
  return rc != SF_OK ? rc : sf_align_solve(f, j, poses_in, a, poses_out, result);
}

SF_API int sf_fuser_align_rgbd_device(sf_fuser* f, const void* d_depth, uint64_t frame_stride_bytes, const void* d_rgb, uint64_t rgb_stride_bytes, uint64_t K,
                                      const float* poses_in, const int32_t* pairs, uint64_t P, const sf_align_params* a, float* poses_out, sf_align_result* result) {
  Job j;
  const int rc = begin(f, d_depth, true, frame_stride_bytes, poses_out != nullptr, K, poses_in, pairs, P, a, &j, true, d_rgb, rgb_stride_bytes);
  return rc != SF_OK ? rc : sf_align_solve(f, j, poses_in, a, poses_out, result);
}

SF_API int sf_fuser_align_rgbd(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, uint64_t K, const float* poses_in, const int32_t* pairs, uint64_t P,
                               const sf_align_params* a, float* poses_out, sf_align_result* result) {
  Job j;
  const int rc = begin(f, depth, false, 0, poses_out != nullptr, K, poses_in, pairs, P, a, &j, true, rgb, 0);
  return rc != SF_OK ? rc : sf_align_solve(f, j, poses_in, a, poses_out, result);
}

namespace {

// the test exports: the P systems at the given poses, j.nsys doubles each
int systems_only(sf_fuser* f, const Job& j, const float* poses, const sf_align_params* a, double* sys) {
  int rc = prepare(f, j);
  if (rc != SF_OK) return rc;
  const uint64_t K = j.K;
  std::vector<double> T(K * 12, 0.0);
  std::vector<uint8_t> valid(K);
  for (uint64_t k = 0; k < K; k++) {
    valid[k] = finite12(poses + 16 * k);
    for (int i = 0; i < 12 && valid[k]; i++) T[12 * k + i] = (double)poses[16 * k + i];
  }
  if ((rc = systems_at(f, j, T.data(), valid.data(), a)) != SF_OK) return rc;
  std::memcpy(sys, f->align->h_sys.p, j.P * j.nsys * sizeof(double));
  return SF_OK;
}

}  // namespace

SF_API int sf_fuser_align_rgbd_system(sf_fuser* f, const uint16_t* depth, const uint8_t* rgb, uint64_t K, const float* poses, const int32_t* pairs, uint64_t P,
                                      const sf_align_params* a, double* sys) {
  Job j;
  const int rc = begin(f, depth, false, 0, sys != nullptr, K, poses, pairs, P, a, &j, true, rgb, 0);
  return rc != SF_OK ? rc : systems_only(f, j, poses, a, sys);
}

SF_API int sf_fuser_align_system(sf_fuser* f, const uint16_t* depth, uint64_t K, const float* poses, const int32_t* pairs, uint64_t P, const sf_align_params* a,
                                 double* sys) {
  Job j;
  const int rc = begin(f, depth, false, 0, sys != nullptr, K, poses, pairs, P, a, &j);
  return rc != SF_OK ? rc : systems_only(f, j, poses, a, sys);
}

// ======================================================================================================
// Host only, double precision: the default pair list and the spreading of the keyframes' correction.
// ======================================================================================================
SF_API int sf_align_pairs(const float* poses, uint64_t K, const sf_align_params* a, int32_t* pairs_out, uint64_t capacity, uint64_t* n_out) {
  if (!a || !n_out || (!poses && K > 0) || (!pairs_out && capacity > 0)) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  if (!(a->pair_max_dist >= 0.0f) || !(a->pair_max_angle >= 0.0f)) return sf::fail(SF_ERR_INVALID_ARG, "sf_align_pairs: pair_max_dist %g, pair_max_angle %g", a->pair_max_dist, a->pair_max_angle);
  if (K > 0x7FFFFFFFull) return sf::fail(SF_ERR_INVALID_ARG, "sf_align_pairs: %llu frames", (unsigned long long)K);
  uint64_t n = 0;
  for (uint64_t i = 0; i < K; i++) {
    const float* pa = poses + 16 * i;
    if (!finite12(pa)) continue;
    for (uint64_t jx = i + 1; jx < K; jx++) {
      const float* pb = poses + 16 * jx;
      if (!finite12(pb)) continue;
      bool take = jx == i + 1;
      if (!take) {
        double d2 = 0.0, M[3][3];
        for (int r = 0; r < 3; r++) {
          const double dt = (double)pb[4 * r + 3] - (double)pa[4 * r + 3];
          d2 += dt * dt;
        }
        for (int u = 0; u < 3; u++)
          for (int v = 0; v < 3; v++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)pa[4 * k + u] * (double)pb[4 * k + v];
            M[u][v] = s;
          }
        const double x = M[2][1] - M[1][2], y = M[0][2] - M[2][0], z = M[1][0] - M[0][1];
        const double sn = 0.5 * std::sqrt((x * x + y * y) + z * z);
        const double cs = 0.5 * (((M[0][0] + M[1][1]) + M[2][2]) - 1.0);
        take = std::sqrt(d2) <= (double)a->pair_max_dist && std::atan2(sn, cs) <= (double)a->pair_max_angle;
      }
      if (!take) continue;
      if (n < capacity) { pairs_out[2 * n] = (int32_t)i; pairs_out[2 * n + 1] = (int32_t)jx; }
      n++;
      if (n < capacity) { pairs_out[2 * n] = (int32_t)jx; pairs_out[2 * n + 1] = (int32_t)i; }
      n++;
    }
  }
  *n_out = n;
  return SF_OK;
}

SF_API int sf_align_spread(const float* poses, uint64_t n, const uint64_t* keyframes, uint64_t K, const float* new_key_poses, float* poses_out) {
  if ((n > 0 && (!poses || !poses_out)) || (K > 0 && (!keyframes || !new_key_poses))) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  for (uint64_t k = 0; k < K; k++)
    if (keyframes[k] >= n || (k > 0 && keyframes[k] <= keyframes[k - 1]))
      return sf::fail(SF_ERR_INVALID_ARG, "sf_align_spread: keyframes must be ascending frame indices below %llu", (unsigned long long)n);
  // the correction D_k = T_k' T_k^-1 of every usable keyframe, in double
  std::vector<double> D(K * 12, 0.0);
  std::vector<uint8_t> usable(K, 0);
  int64_t first = -1;
  for (uint64_t k = 0; k < K; k++) {
    const float* To = poses + 16 * keyframes[k];
    const float* Tn = new_key_poses + 16 * k;
    if (!finite12(To) || !finite12(Tn)) continue;
    usable[k] = 1;
    if (first < 0) first = (int64_t)k;
    double inv[9];
    inverse3(To, inv);
    double* d = &D[12 * k];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) d[4 * r + c] = ((double)Tn[4 * r] * inv[c] + (double)Tn[4 * r + 1] * inv[3 + c]) + (double)Tn[4 * r + 2] * inv[6 + c];
      d[4 * r + 3] = (double)Tn[4 * r + 3] - ((d[4 * r] * (double)To[3] + d[4 * r + 1] * (double)To[7]) + d[4 * r + 2] * (double)To[11]);
    }
  }
  uint64_t next = 0;        // the first keyframe after frame fi
  int64_t cur = first;      // the usable keyframe whose correction frame fi takes
  for (uint64_t fi = 0; fi < n; fi++) {
    bool is_key = false;
    while (next < K && keyframes[next] <= fi) {
      if (usable[next]) cur = (int64_t)next;
      is_key = keyframes[next] == fi && usable[next];
      next++;
    }
    const float* Tf = poses + 16 * fi;
    float* o = poses_out + 16 * fi;
    if (is_key) { std::memcpy(o, new_key_poses + 16 * cur, 16 * sizeof(float)); continue; }
    if (cur < 0 || !finite12(Tf)) { if (o != Tf) std::memcpy(o, Tf, 16 * sizeof(float)); continue; }
    const double* d = &D[12 * cur];
    float out[16];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) {
        double s = (d[4 * r] * (double)Tf[c] + d[4 * r + 1] * (double)Tf[4 + c]) + d[4 * r + 2] * (double)Tf[8 + c];
        if (c == 3) s += d[4 * r + 3];
        out[4 * r + c] = (float)s;
      }
    out[12] = out[13] = out[14] = 0.0f;
    out[15] = 1.0f;
    std::memcpy(o, out, sizeof(out));
  }
  return SF_OK;
}
