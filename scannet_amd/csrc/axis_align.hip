// axis_align.hip -- the vertex-walking stages of the axis alignment on gfx950, bit for bit the host path's (axis_align.cpp):
//   k_aa_normals    a lane per vertex walks its corners in face order (the corner sort of segment_gpu.hip) and adds the faces' cross products
//   k_aa_match      vertices of a batch x chunks of the cluster table: each vertex's first matching cluster in the table as it stood when the batch began
//   k_aa_commit     ONE workgroup (one wave) walks the batch in vertex order and settles every vertex against the clusters changed or founded earlier in
//                   the batch (the dirty list, kept in LDS with their current representatives and sums); the cluster updates run in vertex order, so the
//                   fp32 sums are the host's.  A launch pair per batch; no workgroup ever waits for another
//   k_aa_behind     the behind counts of all kept clusters in one pass over the vertices (integer counts: exact in any order)
//   k_aa_cov        the per-block double sums of the floor's inliers (a fixed tree inside a block of 256 consecutive vertices; the host adds the blocks in order)
//   k_aa_transform  positions through a float[16] in place, with the bounding box of the result
// The arithmetic is axis_align_math.h's, un-contracted.  tests/test_alignment_gpu.py holds each kernel against tests/axis_align_checker.c.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>   // rocprim's texture iterator calls memset without including it

#include <rocprim/rocprim.hpp>

#include <vector>

#include "axis_align_internal.h"
#include "hip_util.h"

namespace {

using namespace sf::aa;

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct Mat { float m[16]; };

__global__ __launch_bounds__(256) void k_aa_corner_keys(const uint32_t* __restrict__ tri, uint32_t n, uint32_t* __restrict__ key, uint32_t* __restrict__ corner) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) { key[i] = tri[i]; corner[i] = i; }
}

// skey / scorner: the 3F corners sorted by vertex, in corner (= face) order inside a vertex
__global__ __launch_bounds__(256) void k_aa_normals(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ scorner, uint32_t nc, const float* __restrict__ pos,
                                                    const uint32_t* __restrict__ tri, uint32_t nv, float* __restrict__ nrm) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= nv) return;
  uint32_t lo = 0, hi = nc;   // first corner whose vertex is >= v
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (skey[mid] < v) lo = mid + 1; else hi = mid;
  }
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  for (uint32_t i = lo; i < nc && skey[i] == v; i++) {
    const uint32_t* t = tri + 3 * (size_t)(scorner[i] / 3u);
    const float* A = pos + 3 * (size_t)t[0];
    const float* B = pos + 3 * (size_t)t[1];
    const float* C = pos + 3 * (size_t)t[2];
    float cx, cy, cz;
    cross3(B[0] - A[0], B[1] - A[1], B[2] - A[2], C[0] - A[0], C[1] - A[1], C[2] - A[2], cx, cy, cz);
    nx = nx + cx; ny = ny + cy; nz = nz + cz;
  }
  normalize3(nx, ny, nz);
  nrm[3 * (size_t)v] = nx; nrm[3 * (size_t)v + 1] = ny; nrm[3 * (size_t)v + 2] = nz;
}

// match[i], i < nb: the lowest cluster of the table at the start of the batch that vertex base + i passes (kNone: none).  Must hold kNone on entry.
__global__ __launch_bounds__(256) void k_aa_match(const float* __restrict__ pos, const float* __restrict__ nrm, uint32_t base, uint32_t nb, const float4* __restrict__ rep,
                                                  const uint32_t* __restrict__ ncl_ptr, uint32_t* __restrict__ match, float nthr, float dthr) {
  __shared__ float4 srep[kChunk];
  const uint32_t ncl = *ncl_ptr;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool valid = i < nb;
  float nx = 0, ny = 0, nz = 0, px = 0, py = 0, pz = 0;
  if (valid) {
    const size_t v = (size_t)base + i;
    nx = nrm[3 * v]; ny = nrm[3 * v + 1]; nz = nrm[3 * v + 2];
    px = pos[3 * v]; py = pos[3 * v + 1]; pz = pos[3 * v + 2];
  }
  for (uint32_t c0 = blockIdx.y * (uint32_t)kChunk; c0 < ncl; c0 += gridDim.y * (uint32_t)kChunk) {   // ncl is the same for every lane: the barriers are uniform
    const uint32_t cn = ncl - c0 < (uint32_t)kChunk ? ncl - c0 : (uint32_t)kChunk;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < cn; j += 256u) srep[j] = rep[c0 + j];
    __syncthreads();
    if (valid && __hip_atomic_load(&match[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > c0) {   // a lower match of another chunk makes this one moot
      for (uint32_t j = 0; j < cn; j++) {
        const float4 r = srep[j];
        if (check(r.x, r.y, r.z, r.w, nx, ny, nz, px, py, pz, nthr, dthr)) { atomicMin(&match[i], c0 + j); break; }
      }
    }
  }
}

__device__ inline uint64_t wave_min_u64(uint64_t x) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off, 64);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    x = o < x ? o : x;
  }
  return x;
}

// One wave settles the nb <= kMaxBatch vertices base .. base + nb - 1 in order.  Table: rep / sums (6 floats) / counts per cluster, *ncl_ptr clusters, capacity
// >= the vertices of the mesh (a vertex founds at most one cluster).  counters: {dirty re-evaluations, fallback rescans}.
__global__ __launch_bounds__(64) void k_aa_commit(const float* __restrict__ pos, const float* __restrict__ nrm, uint32_t base, uint32_t nb, float4* __restrict__ rep,
                                                  float* __restrict__ sums, uint32_t* __restrict__ counts, uint32_t* __restrict__ ncl_ptr, uint32_t* __restrict__ match,
                                                  uint32_t* __restrict__ index, unsigned long long* __restrict__ counters, float nthr, float dthr) {
  __shared__ uint32_t d_idx[kMaxBatch];
  __shared__ float4 d_rep[kMaxBatch];
  __shared__ float d_sum[kMaxBatch * 6];
  __shared__ uint32_t d_cnt[kMaxBatch];
  if (nb > (uint32_t)kMaxBatch) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t ncl0 = *ncl_ptr;   // the table the match kernel saw
  uint32_t ncl = ncl0, nd = 0;
  unsigned long long evals = 0, fallbacks = 0;
  for (uint32_t t0 = 0; t0 < nb; t0 += 64u) {
    const uint32_t cnt = nb - t0 < 64u ? nb - t0 : 64u;
    float lnx = 0, lny = 0, lnz = 0, lpx = 0, lpy = 0, lpz = 0;
    uint32_t lm = kNone;
    if (lane < cnt) {
      const size_t v = (size_t)base + t0 + lane;
      lnx = nrm[3 * v]; lny = nrm[3 * v + 1]; lnz = nrm[3 * v + 2];
      lpx = pos[3 * v]; lpy = pos[3 * v + 1]; lpz = pos[3 * v + 2];
      lm = match[t0 + lane];
      match[t0 + lane] = kNone;   // as the next batch's match kernel wants it
    }
    for (uint32_t j = 0; j < cnt; j++) {
      const float nx = __shfl(lnx, (int)j, 64), ny = __shfl(lny, (int)j, 64), nz = __shfl(lnz, (int)j, 64);
      const float px = __shfl(lpx, (int)j, 64), py = __shfl(lpy, (int)j, 64), pz = __shfl(lpz, (int)j, 64);
      const uint32_t m = (uint32_t)__shfl((int)lm, (int)j, 64);
      // the clusters changed or founded earlier in this batch, against their current representatives
      uint64_t best = ~0ull;
      bool m_in_d = false;
      for (uint32_t k = lane; k < nd; k += 64u) {
        const uint32_t c = d_idx[k];
        const float4 r = d_rep[k];
        if (c == m) m_in_d = true;
        if (check(r.x, r.y, r.z, r.w, nx, ny, nz, px, py, pz, nthr, dthr)) {
          const uint64_t key = ((uint64_t)c << 32) | k;
          best = key < best ? key : best;
        }
      }
      evals += nd;
      best = wave_min_u64(best);
      const bool m_dirty = __ballot(m_in_d) != 0ull;
      const uint32_t dbest = (uint32_t)(best >> 32);   // kNone: no dirty cluster passes
      const uint32_t dslot = (uint32_t)best;
      uint32_t target = kNone, slot = kNone;
      if (m != kNone && !m_dirty) {
        if (dbest < m) { target = dbest; slot = dslot; } else { target = m; }
      } else if (m != kNone && dbest <= m) {   // the snapshot match still passes, or a dirty cluster before it does
        target = dbest; slot = dslot;
      } else if (m != kNone) {
        // The snapshot match moved away and nothing dirty before it passes: the clean clusters behind it were never looked at.  Scan the table again, from
        // the cluster after m up to the lowest passing dirty one.  A clean cluster's row in global memory is current; a dirty one's is stale, and its current
        // representative was evaluated above, so dirty rows are passed over.
        fallbacks++;
        const uint32_t limit = dbest < ncl0 ? dbest : ncl0;
        uint32_t hit = kNone;
        for (uint32_t c0 = m + 1u; c0 < limit && hit == kNone; c0 += 64u) {
          const uint32_t c = c0 + lane;
          bool pass = false;
          if (c < limit) {
            const float4 r = rep[c];
            pass = check(r.x, r.y, r.z, r.w, nx, ny, nz, px, py, pz, nthr, dthr);
          }
          unsigned long long mask = __ballot(pass);
          while (mask != 0ull && hit == kNone) {
            const uint32_t cand = c0 + (uint32_t)__ffsll((long long)mask) - 1u;
            mask &= mask - 1ull;
            bool in_d = false;
            for (uint32_t k = lane; k < nd; k += 64u) in_d = in_d || d_idx[k] == cand;
            if (__ballot(in_d) == 0ull) hit = cand;
          }
        }
        if (hit != kNone) { target = hit; } else if (dbest != kNone) { target = dbest; slot = dslot; }
      } else if (dbest != kNone) {
        target = dbest; slot = dslot;
      }
      Cluster cl;
      if (target == kNone) {   // founds a cluster
        target = ncl++;
        found(cl, nx, ny, nz, px, py, pz);
        slot = nd++;
      } else {
        if (slot != kNone) {
          const float4 r = d_rep[slot];
          cl.rep[0] = r.x; cl.rep[1] = r.y; cl.rep[2] = r.z; cl.rep[3] = r.w;
          for (int q = 0; q < 3; q++) { cl.sn[q] = d_sum[slot * 6u + q]; cl.sp[q] = d_sum[slot * 6u + 3 + q]; }
          cl.count = d_cnt[slot];
        } else {   // a clean cluster's first change in this batch
          const float4 r = rep[target];
          cl.rep[0] = r.x; cl.rep[1] = r.y; cl.rep[2] = r.z; cl.rep[3] = r.w;
          for (int q = 0; q < 3; q++) { cl.sn[q] = sums[(size_t)target * 6 + q]; cl.sp[q] = sums[(size_t)target * 6 + 3 + q]; }
          cl.count = counts[target];
          slot = nd++;
        }
        join(cl, nx, ny, nz, px, py, pz);
      }
      if (lane == 0) {   // slot < kMaxBatch: a vertex adds at most one entry and nb <= kMaxBatch
        d_idx[slot] = target;
        d_rep[slot] = make_float4(cl.rep[0], cl.rep[1], cl.rep[2], cl.rep[3]);
        for (int q = 0; q < 3; q++) { d_sum[slot * 6u + q] = cl.sn[q]; d_sum[slot * 6u + 3 + q] = cl.sp[q]; }
        d_cnt[slot] = cl.count;
        index[(size_t)base + t0 + j] = target;
      }
      __syncthreads();
    }
  }
  for (uint32_t k = lane; k < nd; k += 64u) {
    const uint32_t c = d_idx[k];
    rep[c] = d_rep[k];
    for (int q = 0; q < 6; q++) sums[(size_t)c * 6 + q] = d_sum[k * 6u + q];
    counts[c] = d_cnt[k];
  }
  if (lane == 0) {
    *ncl_ptr = ncl;
    counters[0] += evals;
    counters[1] += fallbacks;
  }
}

constexpr int kBehindPerLane = 8;   // vertices a lane keeps in registers

// grid (vertex tiles of 256 * kBehindPerLane, chunks of kChunk planes): counts[k] += the tile's vertices further than dist behind plane k
__global__ __launch_bounds__(256) void k_aa_behind(const float* __restrict__ pos, uint32_t nv, const float4* __restrict__ reps, uint32_t K, float dist,
                                                   uint32_t* __restrict__ counts) {
  __shared__ float4 srep[kChunk];
  __shared__ uint32_t scnt[kChunk];
  const uint32_t c0 = blockIdx.y * (uint32_t)kChunk;
  const uint32_t cn = K - c0 < (uint32_t)kChunk ? K - c0 : (uint32_t)kChunk;   // the grid has no chunk at or past K
  for (uint32_t j = threadIdx.x; j < cn; j += 256u) { srep[j] = reps[c0 + j]; scnt[j] = 0; }
  float px[kBehindPerLane], py[kBehindPerLane], pz[kBehindPerLane];
  bool ok[kBehindPerLane];
#pragma unroll
  for (int q = 0; q < kBehindPerLane; q++) {
    const size_t v = ((size_t)blockIdx.x * kBehindPerLane + q) * 256u + threadIdx.x;
    ok[q] = v < nv;
    px[q] = ok[q] ? pos[3 * v] : 0.0f; py[q] = ok[q] ? pos[3 * v + 1] : 0.0f; pz[q] = ok[q] ? pos[3 * v + 2] : 0.0f;
  }
  __syncthreads();
  const float neg = -dist;
  for (uint32_t j = 0; j < cn; j++) {
    const float4 r = srep[j];
    uint32_t n = 0;
#pragma unroll
    for (int q = 0; q < kBehindPerLane; q++) n += (uint32_t)__popcll(__ballot(ok[q] && plane_dist(r.x, r.y, r.z, r.w, px[q], py[q], pz[q]) < neg));
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&scnt[j], n);
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < cn; j += 256u)
    if (scnt[j]) atomicAdd(&counts[c0 + j], scnt[j]);
}

// partial[b * 10 + k]: sum k of block b (vertices 256 b .. 256 b + 255), added in the fixed tree a[i] += a[i + s], s = 1, 2, .., 128
__global__ __launch_bounds__(256) void k_aa_cov(const float* __restrict__ pos, const uint32_t* __restrict__ index, uint32_t nv, uint32_t cluster, float rx, float ry, float rz,
                                                float rd, float inlier, double* __restrict__ partial) {
  __shared__ double a[10][kCovBlock];
  const uint32_t tid = threadIdx.x;
  const size_t v = (size_t)blockIdx.x * kCovBlock + tid;
  bool in = false;
  float fx = 0, fy = 0, fz = 0;
  if (v < nv && index[v] == cluster) {
    fx = pos[3 * v]; fy = pos[3 * v + 1]; fz = pos[3 * v + 2];
    in = fabsf(plane_dist(rx, ry, rz, rd, fx, fy, fz)) < inlier;
  }
  const double x = fx, y = fy, z = fz;
  a[0][tid] = in ? 1.0 : 0.0;
  a[1][tid] = in ? x : 0.0; a[2][tid] = in ? y : 0.0; a[3][tid] = in ? z : 0.0;
  a[4][tid] = in ? x * x : 0.0; a[5][tid] = in ? x * y : 0.0; a[6][tid] = in ? x * z : 0.0;
  a[7][tid] = in ? y * y : 0.0; a[8][tid] = in ? y * z : 0.0; a[9][tid] = in ? z * z : 0.0;
  __syncthreads();
  for (uint32_t s = 1; s < (uint32_t)kCovBlock; s *= 2u) {
    if ((tid & (2u * s - 1u)) == 0) {
#pragma unroll
      for (int k = 0; k < 10; k++) a[k][tid] = a[k][tid] + a[k][tid + s];
    }
    __syncthreads();
  }
  if (tid < 10) partial[(size_t)blockIdx.x * 10 + tid] = a[tid][0];
}

__device__ inline uint32_t order_key(float f) {   // unsigned order = float order
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// box[0..2]: keys of the minima (start 0xFFFFFFFF), box[3..5]: of the maxima (start 0)
__global__ __launch_bounds__(256) void k_aa_transform(float* __restrict__ pos, uint32_t nv, Mat M, uint32_t* __restrict__ box) {
  __shared__ uint32_t sbox[6];
  if (threadIdx.x < 3) sbox[threadIdx.x] = 0xFFFFFFFFu;
  else if (threadIdx.x < 6) sbox[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  for (size_t v = (size_t)blockIdx.x * 256u + threadIdx.x; v < nv; v += (size_t)gridDim.x * 256u) {
    float o[3];
    xform(M.m, pos[3 * v], pos[3 * v + 1], pos[3 * v + 2], o[0], o[1], o[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      pos[3 * v + k] = o[k];
      const uint32_t key = order_key(o[k]);
      lo[k] = key < lo[k] ? key : lo[k];
      hi[k] = key > hi[k] ? key : hi[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t a = (uint32_t)__shfl_xor((int)lo[k], off, 64), b = (uint32_t)__shfl_xor((int)hi[k], off, 64);
      lo[k] = a < lo[k] ? a : lo[k];
      hi[k] = b > hi[k] ? b : hi[k];
    }
    if ((threadIdx.x & 63u) == 0) { atomicMin(&sbox[k], lo[k]); atomicMax(&sbox[3 + k], hi[k]); }
  }
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(&box[threadIdx.x], sbox[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(&box[threadIdx.x], sbox[threadIdx.x]);
}

float key_to_float(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

struct GpuOps final : Ops {
  int device = 0;
  size_t nv = 0, nf = 0;
  bool have_nrm = false, have_idx = false;
  sf::DevBuf d_pos, d_tri, d_nrm, d_idx;
  hipStream_t s = nullptr;   // the null stream: every call ends with a synchronisation

  int use() { SF_HIP_CHECK(hipSetDevice(device)); return SF_OK; }
  int up(sf::DevBuf& b, const void* src, size_t bytes) {
    SF_HIP_CHECK(b.alloc(bytes));
    if (bytes) SF_HIP_CHECK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return SF_OK;
  }
  int down(void* dst, const sf::DevBuf& b, size_t bytes) {
    if (bytes) SF_HIP_CHECK(hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost));
    return SF_OK;
  }

  int set_positions(const float* xyz, size_t n) override {
    if (n >= 0x7FFFFFFFu / 3u) return sf::fail(SF_ERR_INVALID_ARG, "too many vertices for the device path");
    int rc = use();
    if (rc != SF_OK) return rc;
    nv = n; have_nrm = have_idx = false;
    return up(d_pos, xyz, n * 12);
  }
  int set_faces(const uint32_t* t, size_t n) override {
    if (n >= 0x7FFFFFFFu / 3u) return sf::fail(SF_ERR_INVALID_ARG, "too many faces for the device path");
    int rc = use();
    if (rc != SF_OK) return rc;
    nf = n;
    return up(d_tri, t, n * 12);
  }
  int set_normals(const float* n) override { int rc = use(); if (rc != SF_OK) return rc; have_nrm = true; return up(d_nrm, n, nv * 12); }
  int set_index(const uint32_t* i) override { int rc = use(); if (rc != SF_OK) return rc; have_idx = true; return up(d_idx, i, nv * 4); }
  int get_positions(float* xyz) override { int rc = use(); return rc != SF_OK ? rc : down(xyz, d_pos, nv * 12); }
  int get_normals(float* n) override {
    if (!have_nrm) return sf::fail(SF_ERR_INVALID_ARG, "no normals");
    int rc = use();
    return rc != SF_OK ? rc : down(n, d_nrm, nv * 12);
  }
  int get_index(uint32_t* i) override {
    if (!have_idx) return sf::fail(SF_ERR_INVALID_ARG, "no cluster index");
    int rc = use();
    return rc != SF_OK ? rc : down(i, d_idx, nv * 4);
  }

  int transform(const float m[16], float bbox[6]) override {
    int rc = use();
    if (rc != SF_OK) return rc;
    sf::DevBuf d_box;
    const uint32_t init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    if ((rc = up(d_box, init, sizeof init)) != SF_OK) return rc;
    Mat M;
    std::memcpy(M.m, m, 64);
    if (nv) {
      const size_t blocks = (nv + 255) / 256;
      hipLaunchKernelGGL(k_aa_transform, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, d_pos.as<float>(), (uint32_t)nv, M, d_box.as<uint32_t>());
      SF_HIP_CHECK(hipGetLastError());
    }
    uint32_t keys[6];
    if ((rc = down(keys, d_box, sizeof keys)) != SF_OK) return rc;
    for (int k = 0; k < 6; k++) bbox[k] = key_to_float(keys[k]) + 0.0f;   // a zero bound is +0 on either path
    if (nv == 0) for (int k = 0; k < 3; k++) { bbox[k] = INFINITY; bbox[3 + k] = -INFINITY; }
    return SF_OK;
  }

  int normals() override {
    int rc = use();
    if (rc != SF_OK) return rc;
    SF_HIP_CHECK(d_nrm.alloc(nv * 12));
    have_nrm = true;
    if (nv == 0) return SF_OK;
    const size_t nc = nf * 3;
    sf::DevBuf k0, k1, c0, c1, tmp;
    SF_HIP_CHECK(k0.alloc(nc * 4)); SF_HIP_CHECK(k1.alloc(nc * 4)); SF_HIP_CHECK(c0.alloc(nc * 4)); SF_HIP_CHECK(c1.alloc(nc * 4));
    if (nc) {
      hipLaunchKernelGGL(k_aa_corner_keys, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, d_tri.as<uint32_t>(), (uint32_t)nc, k0.as<uint32_t>(), c0.as<uint32_t>());
      size_t need = 0;
      int bits = 1;
      while (bits < 32 && (nv >> bits) != 0) bits++;   // the keys are vertex numbers below nv
      SF_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, need, k0.as<uint32_t>(), k1.as<uint32_t>(), c0.as<uint32_t>(), c1.as<uint32_t>(), nc, 0, (unsigned)bits, s));
      SF_HIP_CHECK(tmp.alloc(need));
      SF_HIP_CHECK(rocprim::radix_sort_pairs(tmp.p, need, k0.as<uint32_t>(), k1.as<uint32_t>(), c0.as<uint32_t>(), c1.as<uint32_t>(), nc, 0, (unsigned)bits, s));
    }
    hipLaunchKernelGGL(k_aa_normals, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, k1.as<uint32_t>(), c1.as<uint32_t>(), (uint32_t)nc, d_pos.as<float>(), d_tri.as<uint32_t>(),
                       (uint32_t)nv, d_nrm.as<float>());
    SF_HIP_CHECK(hipGetLastError());
    SF_HIP_CHECK(hipStreamSynchronize(s));
    return SF_OK;
  }

  int cluster(float nthr, float dthr, std::vector<Cluster>& table, uint64_t counters[3]) override {
    if (!have_nrm) return sf::fail(SF_ERR_INVALID_ARG, "no normals");
    int rc = use();
    if (rc != SF_OK) return rc;
    table.clear();
    counters[0] = counters[1] = counters[2] = 0;
    SF_HIP_CHECK(d_idx.alloc(nv * 4));
    have_idx = true;
    if (nv == 0) return SF_OK;
    const uint32_t B = (uint32_t)batch_size();   // 64..kMaxBatch (sf_axis_align_tune)
    sf::DevBuf d_rep, d_sums, d_counts, d_match, d_ncl, d_ctr;
    SF_HIP_CHECK(d_rep.alloc(nv * 16)); SF_HIP_CHECK(d_sums.alloc(nv * 24)); SF_HIP_CHECK(d_counts.alloc(nv * 4));   // a vertex founds at most one cluster
    SF_HIP_CHECK(d_match.alloc((size_t)kMaxBatch * 4)); SF_HIP_CHECK(d_ncl.alloc(4)); SF_HIP_CHECK(d_ctr.alloc(16));
    SF_HIP_CHECK(hipMemsetAsync(d_match.p, 0xFF, (size_t)kMaxBatch * 4, s));
    SF_HIP_CHECK(hipMemsetAsync(d_ncl.p, 0, 4, s));
    SF_HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, 16, s));
    struct Events {   // profile(): three events per batch
      std::vector<hipEvent_t> e;
      ~Events() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
      int mark(hipStream_t st) {
        hipEvent_t x;
        SF_HIP_CHECK(hipEventCreate(&x));
        e.push_back(x);
        SF_HIP_CHECK(hipEventRecord(x, st));
        return SF_OK;
      }
    } ev;
    const bool prof = profile() != 0;
    split[0] = split[1] = 0.0;
    for (size_t base = 0; base < nv; base += B) {
      const uint32_t nb = (uint32_t)(nv - base < B ? nv - base : B);
      if (prof && (rc = ev.mark(s)) != SF_OK) return rc;
      if (base)   // the first batch meets an empty table
        hipLaunchKernelGGL(k_aa_match, dim3((nb + 255u) / 256u, 8), dim3(256), 0, s, d_pos.as<float>(), d_nrm.as<float>(), (uint32_t)base, nb, d_rep.as<float4>(),
                           d_ncl.as<uint32_t>(), d_match.as<uint32_t>(), nthr, dthr);
      if (prof && (rc = ev.mark(s)) != SF_OK) return rc;
      hipLaunchKernelGGL(k_aa_commit, dim3(1), dim3(64), 0, s, d_pos.as<float>(), d_nrm.as<float>(), (uint32_t)base, nb, d_rep.as<float4>(), d_sums.as<float>(),
                         d_counts.as<uint32_t>(), d_ncl.as<uint32_t>(), d_match.as<uint32_t>(), d_idx.as<uint32_t>(), d_ctr.as<unsigned long long>(), nthr, dthr);
      if (prof && (rc = ev.mark(s)) != SF_OK) return rc;
      counters[0]++;
    }
    SF_HIP_CHECK(hipGetLastError());
    if (prof) {
      SF_HIP_CHECK(hipStreamSynchronize(s));
      for (size_t b = 0; b + 2 < ev.e.size(); b += 3) {
        float ms0 = 0, ms1 = 0;
        SF_HIP_CHECK(hipEventElapsedTime(&ms0, ev.e[b], ev.e[b + 1]));
        SF_HIP_CHECK(hipEventElapsedTime(&ms1, ev.e[b + 1], ev.e[b + 2]));
        split[0] += ms0 * 1e-3; split[1] += ms1 * 1e-3;
      }
    }
    uint32_t ncl = 0;
    unsigned long long ctr[2];
    if ((rc = down(&ncl, d_ncl, 4)) != SF_OK || (rc = down(ctr, d_ctr, 16)) != SF_OK) return rc;
    if (ncl > nv) return sf::fail(SF_ERR_DEVICE, "the cluster table came back with %u clusters for %zu vertices", ncl, nv);
    counters[1] = ctr[0]; counters[2] = ctr[1];
    std::vector<float> rep((size_t)ncl * 4), sums((size_t)ncl * 6);
    std::vector<uint32_t> cnt(ncl);
    if ((rc = down(rep.data(), d_rep, (size_t)ncl * 16)) != SF_OK || (rc = down(sums.data(), d_sums, (size_t)ncl * 24)) != SF_OK || (rc = down(cnt.data(), d_counts, (size_t)ncl * 4)) != SF_OK)
      return rc;
    table.resize(ncl);
    for (uint32_t c = 0; c < ncl; c++) {
      std::memcpy(table[c].rep, &rep[(size_t)c * 4], 16);
      std::memcpy(table[c].sn, &sums[(size_t)c * 6], 12);
      std::memcpy(table[c].sp, &sums[(size_t)c * 6 + 3], 12);
      table[c].count = cnt[c];
    }
    return SF_OK;
  }

  int behind(const float* reps4, size_t K, float dist, uint32_t* counts) override {
    if (K == 0) return SF_OK;
    if (K > 0x7FFFFFFFu) return sf::fail(SF_ERR_INVALID_ARG, "too many planes");
    int rc = use();
    if (rc != SF_OK) return rc;
    sf::DevBuf d_reps, d_cnt;
    if ((rc = up(d_reps, reps4, K * 16)) != SF_OK) return rc;
    SF_HIP_CHECK(d_cnt.alloc(K * 4));
    SF_HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, K * 4, s));
    const size_t per = (size_t)256 * kBehindPerLane, tiles = (nv + per - 1) / per, chunks = (K + kChunk - 1) / kChunk;
    if (chunks > 65535) return sf::fail(SF_ERR_INVALID_ARG, "too many planes");
    if (tiles) {
      hipLaunchKernelGGL(k_aa_behind, dim3((unsigned)tiles, (unsigned)chunks), dim3(256), 0, s, d_pos.as<float>(), (uint32_t)nv, d_reps.as<float4>(), (uint32_t)K, dist, d_cnt.as<uint32_t>());
      SF_HIP_CHECK(hipGetLastError());
    }
    return down(counts, d_cnt, K * 4);
  }

  int cov(uint32_t cluster, const float rep[4], float inlier, double sums[10]) override {
    for (int k = 0; k < 10; k++) sums[k] = 0.0;
    if (!have_idx) return sf::fail(SF_ERR_INVALID_ARG, "no cluster index");
    if (nv == 0) return SF_OK;
    int rc = use();
    if (rc != SF_OK) return rc;
    const size_t blocks = (nv + kCovBlock - 1) / kCovBlock;
    sf::DevBuf d_part;
    SF_HIP_CHECK(d_part.alloc(blocks * 80));
    hipLaunchKernelGGL(k_aa_cov, dim3((unsigned)blocks), dim3(kCovBlock), 0, s, d_pos.as<float>(), d_idx.as<uint32_t>(), (uint32_t)nv, cluster, rep[0], rep[1], rep[2], rep[3], inlier,
                       d_part.as<double>());
    SF_HIP_CHECK(hipGetLastError());
    std::vector<double> part(blocks * 10);
    if ((rc = down(part.data(), d_part, blocks * 80)) != SF_OK) return rc;
    for (size_t b = 0; b < blocks; b++)
      for (int k = 0; k < 10; k++) sums[k] = sums[k] + part[b * 10 + k];
    return SF_OK;
  }
};

}  // namespace

namespace sf {
namespace aa {

int make_gpu_ops(int device, Ops** out) {
  if (int rc = sf::open_device(device, SF_ERR_INVALID_ARG, "the axis alignment on a device needs one (device = -1 is the host path)")) return rc;
  GpuOps* g = new GpuOps;
  g->device = device;
  *out = g;
  return SF_OK;
}

}  // namespace aa
}  // namespace sf
