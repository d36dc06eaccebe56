// voxel_labels.hip -- the device path of the voxel task's data (include/scanfuse.h "Voxel-task data"): the nearest face of every
// grid node near a mesh, and the windowed gather of column samples.  The rule is voxel_labels_internal.h's, the host path of the same bytes is
// voxel_labels.cpp.
//
//   k_vl_count    a thread per face: its record (everything that depends on the face alone), and +1 on every 8^3-node tile its grown box touches
//   k_vl_scan     one workgroup: exclusive scan of the counts, and the non-empty entries in ascending order (tiles here, selected columns below)
//   k_vl_fill     a thread per face: its index into the list of every tile it touches (integer atomics: the winner is a minimum over a total order)
//   k_vl_clear    nodes of tiles without a face: -1 / +inf by a plain store
//   k_vl_nearest  a workgroup per non-empty tile, two nodes per lane; the tile's records come through LDS in chunks, every lane keeps its (d2, f) minimum
//   k_vl_select   a thread per column: does it hold a task label inside the window's layers
//   k_vl_sample   a workgroup per (sample, layer): lanes along x, clamped loads and a select for the -inf outside the grid
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>
#include <cstring>

#include "common.h"
#include "hip_util.h"
#include "voxel_labels_internal.h"

namespace {

using sf::vl::FaceRec;
using sf::vl::Geo;
using sf::vl::TILE;

constexpr int VL_CHUNK = 128;   // records per LDS chunk: 10 KiB

__global__ __launch_bounds__(256) void k_vl_count(const float* __restrict__ xyz, const uint32_t* __restrict__ tris, uint32_t nf, float t, Geo g,
                                                  FaceRec* __restrict__ rec, uint32_t* __restrict__ counts) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= nf) return;
  const FaceRec r = sf::vl::make_record(xyz, tris, f, t);
  rec[f] = r;
  if (!r.valid) return;
  int32_t x0, x1, y0, y1, z0, z1;
  if (!sf::vl::tile_range(r.lox, r.hix, g.voxel, g.lox, g.nx, &x0, &x1) || !sf::vl::tile_range(r.loy, r.hiy, g.voxel, g.loy, g.ny, &y0, &y1) ||
      !sf::vl::tile_range(r.loz, r.hiz, g.voxel, g.loz, g.nz, &z0, &z1))
    return;
  for (int32_t z = z0; z <= z1; z++)
    for (int32_t y = y0; y <= y1; y++)
      for (int32_t x = x0; x <= x1; x++) atomicAdd(&counts[((size_t)z * g.ty + y) * g.tx + x], 1u);
}

__global__ __launch_bounds__(256) void k_vl_fill(const FaceRec* __restrict__ rec, uint32_t nf, Geo g, const uint32_t* __restrict__ offsets,
                                                 uint32_t* __restrict__ cursor, int32_t* __restrict__ list, unsigned long long total) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= nf) return;
  const FaceRec r = rec[f];
  if (!r.valid) return;
  int32_t x0, x1, y0, y1, z0, z1;
  if (!sf::vl::tile_range(r.lox, r.hix, g.voxel, g.lox, g.nx, &x0, &x1) || !sf::vl::tile_range(r.loy, r.hiy, g.voxel, g.loy, g.ny, &y0, &y1) ||
      !sf::vl::tile_range(r.loz, r.hiz, g.voxel, g.loz, g.nz, &z0, &z1))
    return;
  for (int32_t z = z0; z <= z1; z++)
    for (int32_t y = y0; y <= y1; y++)
      for (int32_t x = x0; x <= x1; x++) {
        const size_t tile = ((size_t)z * g.ty + y) * g.tx + x;
        const unsigned long long at = (unsigned long long)offsets[tile] + atomicAdd(&cursor[tile], 1u);
        if (at < total) list[at] = (int32_t)f;
      }
}

// offsets[i] = sum of counts[0 .. i); work = the i with counts[i] != 0, ascending; totals = {sum, how many}
__global__ __launch_bounds__(1024) void k_vl_scan(const uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ offsets, uint32_t* __restrict__ work,
                                                  unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long s_sum[1024];
  __shared__ uint32_t s_cnt[1024];
  const uint32_t t = threadIdx.x;
  const unsigned long long per = ((unsigned long long)n + 1023ull) / 1024ull;
  const unsigned long long b64 = (unsigned long long)t * per, e64 = b64 + per;
  const uint32_t b = b64 < n ? (uint32_t)b64 : n, e = e64 < n ? (uint32_t)e64 : n;
  unsigned long long sum = 0;
  uint32_t cnt = 0;
  for (uint32_t i = b; i < e; i++) {
    const uint32_t c = counts[i];
    sum += c;
    cnt += c ? 1u : 0u;
  }
  s_sum[t] = sum;
  s_cnt[t] = cnt;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const unsigned long long v = t >= d ? s_sum[t - d] : 0ull;
    const uint32_t c = t >= d ? s_cnt[t - d] : 0u;
    __syncthreads();
    s_sum[t] += v;
    s_cnt[t] += c;
    __syncthreads();
  }
  unsigned long long run = s_sum[t] - sum;
  uint32_t w = s_cnt[t] - cnt;
  for (uint32_t i = b; i < e; i++) {
    const uint32_t c = counts[i];
    offsets[i] = (uint32_t)run;
    if (c) work[w++] = i;
    run += c;
  }
  if (t == 1023) {
    totals[0] = s_sum[1023];
    totals[1] = s_cnt[1023];
  }
}

__global__ __launch_bounds__(256) void k_vl_clear(Geo g, const uint32_t* __restrict__ counts, int32_t* __restrict__ face, float* __restrict__ dist2) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  const size_t n = (size_t)g.nx * g.ny * g.nz;
  if (i >= n) return;
  const int32_t x = (int32_t)(i % (size_t)g.nx), y = (int32_t)((i / (size_t)g.nx) % (size_t)g.ny), z = (int32_t)(i / ((size_t)g.nx * g.ny));
  if (counts[((size_t)(z / TILE) * g.ty + y / TILE) * g.tx + x / TILE] != 0) return;
  face[i] = -1;
  if (dist2) dist2[i] = INFINITY;
}

__global__ __launch_bounds__(256) void k_vl_nearest(Geo g, const FaceRec* __restrict__ rec, const uint32_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ counts, const int32_t* __restrict__ list,
                                                    const uint32_t* __restrict__ work, float r2, int32_t* __restrict__ face, float* __restrict__ dist2) {
  __shared__ __attribute__((aligned(16))) FaceRec s_rec[VL_CHUNK];
  const uint32_t tile = work[blockIdx.x];
  const int32_t tix = (int32_t)(tile % (uint32_t)g.tx), tiy = (int32_t)((tile / (uint32_t)g.tx) % (uint32_t)g.ty), tiz = (int32_t)(tile / ((uint32_t)g.tx * g.ty));
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t x = tix * TILE + (lane & 7), y = tiy * TILE + (lane >> 3), za = tiz * TILE + 2 * wave, zb = za + 1;
  const float px = sf::vl::node_pos(g.lox, x, g.voxel), py = sf::vl::node_pos(g.loy, y, g.voxel);
  const float pza = sf::vl::node_pos(g.loz, za, g.voxel), pzb = sf::vl::node_pos(g.loz, zb, g.voxel);
  // the wave's slab of nodes, 8 x 8 x 2 (node positions grow with the index: one product of a positive constant)
  const float sx0 = sf::vl::node_pos(g.lox, tix * TILE, g.voxel), sx1 = sf::vl::node_pos(g.lox, tix * TILE + 7, g.voxel);
  const float sy0 = sf::vl::node_pos(g.loy, tiy * TILE, g.voxel), sy1 = sf::vl::node_pos(g.loy, tiy * TILE + 7, g.voxel);
  float best_a = INFINITY, best_b = INFINITY;
  int32_t fa = INT_MAX, fb = INT_MAX;
  const uint32_t n = counts[tile], off = offsets[tile];
  for (uint32_t base = 0; base < n; base += VL_CHUNK) {
    const uint32_t m = n - base < (uint32_t)VL_CHUNK ? n - base : (uint32_t)VL_CHUNK;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m * 5u; i += 256u) {
      const uint32_t r = i / 5u, q = i - r * 5u;
      ((float4*)s_rec)[i] = ((const float4*)(rec + list[off + base + r]))[q];
    }
    __syncthreads();
    for (uint32_t j = 0; j < m; j++) {
      const FaceRec& R = s_rec[j];
      const int miss = (R.hix < sx0 || R.lox > sx1 || R.hiy < sy0 || R.loy > sy1 || R.hiz < pza || R.loz > pzb) ? 1 : 0;
      if (__builtin_amdgcn_readfirstlane(miss)) continue;   // the same for the whole wave
      if (sf::vl::in_box(R, px, py, pza)) {
        const float d = sf::vl::dist2(R, px, py, pza);
        if (sf::vl::better(d, R.f, r2, best_a, fa)) { best_a = d; fa = R.f; }
      }
      if (sf::vl::in_box(R, px, py, pzb)) {
        const float d = sf::vl::dist2(R, px, py, pzb);
        if (sf::vl::better(d, R.f, r2, best_b, fb)) { best_b = d; fb = R.f; }
      }
    }
  }
  if (x < g.nx && y < g.ny) {
    if (za < g.nz) {
      const size_t i = ((size_t)za * g.ny + y) * g.nx + x;
      face[i] = fa == INT_MAX ? -1 : fa;
      if (dist2) dist2[i] = best_a;
    }
    if (zb < g.nz) {
      const size_t i = ((size_t)zb * g.ny + y) * g.nx + x;
      face[i] = fb == INT_MAX ? -1 : fb;
      if (dist2) dist2[i] = best_b;
    }
  }
}

__global__ __launch_bounds__(256) void k_vl_select(const uint8_t* __restrict__ bl, int32_t nx, int32_t ny, int32_t zlo, int32_t zhi, int32_t stride,
                                                   uint32_t* __restrict__ flags) {
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= (size_t)nx * ny) return;
  const int32_t x = (int32_t)(c % (size_t)nx), y = (int32_t)(c / (size_t)nx);
  uint32_t any = 0;
  if (x % stride == 0 && y % stride == 0)
    for (int32_t z = zlo; z < zhi; z++) {
      const uint8_t v = bl[((size_t)z * ny + y) * nx + x];
      any |= (v != 0 && v != 255) ? 1u : 0u;
    }
  flags[c] = any;
}

__global__ __launch_bounds__(256) void k_vl_sample(const float* __restrict__ value, const uint8_t* __restrict__ bl, int32_t nx, int32_t ny, int32_t nz,
                                                   const uint32_t* __restrict__ cols, unsigned long long first, int32_t wx, int32_t wy, int32_t wz, long long z0,
                                                   float* __restrict__ data, uint8_t* __restrict__ label, int32_t* __restrict__ xy) {
  const uint32_t s = blockIdx.x / (uint32_t)wz, k = blockIdx.x - s * (uint32_t)wz;
  const uint32_t col = cols[first + s];
  const int32_t x = (int32_t)(col % (uint32_t)nx), y = (int32_t)(col / (uint32_t)nx);
  const long long z = z0 + (long long)k;
  const bool zin = z >= 0 && z < (long long)nz;
  const int32_t zc = z < 0 ? 0 : (z >= (long long)nz ? nz - 1 : (int32_t)z);
  float* out = data + (size_t)blockIdx.x * ((size_t)wy * wx);
  const float* layer = value + (size_t)zc * ny * nx;
  const uint32_t per = (uint32_t)wy * (uint32_t)wx;
  for (uint32_t e = threadIdx.x; e < per; e += 256u) {
    const uint32_t j = e / (uint32_t)wx, i = e - j * (uint32_t)wx;
    const int32_t yy = y + (int32_t)j - wy / 2, xx = x + (int32_t)i - wx / 2;
    const bool in = zin && yy >= 0 && yy < ny && xx >= 0 && xx < nx;
    const int32_t yc = min(max(yy, 0), ny - 1), xc = min(max(xx, 0), nx - 1);
    const float v = layer[(size_t)yc * nx + xc];
    out[e] = in ? v : -INFINITY;
  }
  if (threadIdx.x == 0) {
    label[(size_t)s * wz + k] = zin ? bl[((size_t)zc * ny + y) * nx + x] : (uint8_t)0;
    if (k == 0) { xy[2 * (size_t)s] = x; xy[2 * (size_t)s + 1] = y; }
  }
}

// device microseconds of the most recent call's launches: k_vl_count .. k_vl_fill, k_vl_clear + k_vl_nearest, k_vl_sample (sf_voxlabel_kernel_us)
std::atomic<float> g_bins_us{0.0f}, g_nearest_us{0.0f}, g_sample_us{0.0f};

}  // namespace

namespace sf {
namespace vl {

int nearest_device(const sf_grid_header& h, const float* xyz, uint64_t nv, const uint32_t* tris, uint64_t nf, float t, float r2, int device, int32_t* face,
                   float* dist2, const BinsOut* bins) {
  int rc = open_device(device, SF_ERR_DEVICE, "%s on a device needs an MI355X (device = -1 is the host path)", "the nearest-face search");
  if (rc != SF_OK) return rc;
  const Geo g = make_geo(h);
  const uint64_t n_nodes = (uint64_t)h.nx * (uint64_t)h.ny * (uint64_t)h.nz;
  const uint64_t n_tiles = (uint64_t)g.tx * (uint64_t)g.ty * (uint64_t)g.tz;
  if (bins && bins->total) *bins->total = 0;
  if (n_nodes == 0) return SF_OK;
  if (n_tiles > (1ull << 31) || nf > (1ull << 31) - 1 || n_nodes > (1ull << 31) * 256ull)
    return sf::fail(SF_ERR_INVALID_ARG, "the nearest-face search on a device: %llu tiles, %llu faces", (unsigned long long)n_tiles, (unsigned long long)nf);
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  DevBuf d_xyz, d_tris, d_rec, d_counts, d_offsets, d_work, d_cursor, d_totals, d_list, d_face, d_dist;
  SF_HIP_CHECK(d_xyz.alloc(nv * 12));
  SF_HIP_CHECK(d_tris.alloc(nf * 12));
  SF_HIP_CHECK(d_rec.alloc(nf * sizeof(FaceRec)));
  SF_HIP_CHECK(d_counts.alloc(n_tiles * 4));
  SF_HIP_CHECK(d_offsets.alloc(n_tiles * 4));
  SF_HIP_CHECK(d_work.alloc(n_tiles * 4));
  SF_HIP_CHECK(d_cursor.alloc(n_tiles * 4));
  SF_HIP_CHECK(d_totals.alloc(16));
  if (nv) SF_HIP_CHECK(hipMemcpyAsync(d_xyz.p, xyz, nv * 12, hipMemcpyHostToDevice, sg.s));
  if (nf) SF_HIP_CHECK(hipMemcpyAsync(d_tris.p, tris, nf * 12, hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, n_tiles * 4, sg.s));
  SF_HIP_CHECK(hipMemsetAsync(d_cursor.p, 0, n_tiles * 4, sg.s));
  const uint32_t face_blocks = (uint32_t)((nf + 255) / 256);
  EventSpan t_count, t_fill, t_near;
  t_count.begin(sg.s);
  if (nf) {
    k_vl_count<<<face_blocks, 256, 0, sg.s>>>(d_xyz.as<float>(), d_tris.as<uint32_t>(), (uint32_t)nf, t, g, d_rec.as<FaceRec>(), d_counts.as<uint32_t>());
    SF_HIP_CHECK(hipGetLastError());
  }
  k_vl_scan<<<1, 1024, 0, sg.s>>>(d_counts.as<uint32_t>(), (uint32_t)n_tiles, d_offsets.as<uint32_t>(), d_work.as<uint32_t>(), d_totals.as<unsigned long long>());
  SF_HIP_CHECK(hipGetLastError());
  t_count.end(sg.s);
  unsigned long long totals[2] = {0, 0};
  SF_HIP_CHECK(hipMemcpyAsync(totals, d_totals.p, 16, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  if (totals[0] >= (1ull << 32)) return sf::fail(SF_ERR_CAPACITY, "the nearest-face search: %llu (face, tile) pairs", totals[0]);
  SF_HIP_CHECK(d_list.alloc((size_t)totals[0] * 4));
  t_fill.begin(sg.s);
  if (totals[0]) {
    SF_HIP_CHECK(hipMemsetAsync(d_list.p, 0, (size_t)totals[0] * 4, sg.s));   // k_vl_nearest indexes the records with what it reads here
    k_vl_fill<<<face_blocks, 256, 0, sg.s>>>(d_rec.as<FaceRec>(), (uint32_t)nf, g, d_offsets.as<uint32_t>(), d_cursor.as<uint32_t>(), d_list.as<int32_t>(), totals[0]);
    SF_HIP_CHECK(hipGetLastError());
  }
  t_fill.end(sg.s);
  if (bins) {
    if (bins->total) *bins->total = totals[0];
    if (bins->counts) SF_HIP_CHECK(hipMemcpyAsync(bins->counts, d_counts.p, n_tiles * 4, hipMemcpyDeviceToHost, sg.s));
    if (bins->offsets) SF_HIP_CHECK(hipMemcpyAsync(bins->offsets, d_offsets.p, n_tiles * 4, hipMemcpyDeviceToHost, sg.s));
    if (bins->list) {
      if (bins->capacity < totals[0]) return sf::fail(SF_ERR_BOUNDS, "the bin stage: %llu entries, capacity %llu", totals[0], (unsigned long long)bins->capacity);
      if (totals[0]) SF_HIP_CHECK(hipMemcpyAsync(bins->list, d_list.p, (size_t)totals[0] * 4, hipMemcpyDeviceToHost, sg.s));
    }
    SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  }
  if (!face) {
    SF_HIP_CHECK(hipStreamSynchronize(sg.s));
    g_bins_us = t_count.us() + t_fill.us();
    return SF_OK;
  }
  const bool face_dev = on_device(face), dist_dev = on_device(dist2);
  int32_t* o_face = face;
  float* o_dist = dist2;
  if (!face_dev) { SF_HIP_CHECK(d_face.alloc(n_nodes * 4)); o_face = d_face.as<int32_t>(); }
  if (dist2 && !dist_dev) { SF_HIP_CHECK(d_dist.alloc(n_nodes * 4)); o_dist = d_dist.as<float>(); }
  t_near.begin(sg.s);
  k_vl_clear<<<(uint32_t)((n_nodes + 255) / 256), 256, 0, sg.s>>>(g, d_counts.as<uint32_t>(), o_face, o_dist);
  SF_HIP_CHECK(hipGetLastError());
  if (totals[1]) {
    k_vl_nearest<<<(uint32_t)totals[1], 256, 0, sg.s>>>(g, d_rec.as<FaceRec>(), d_offsets.as<uint32_t>(), d_counts.as<uint32_t>(), d_list.as<int32_t>(),
                                                       d_work.as<uint32_t>(), r2, o_face, o_dist);
    SF_HIP_CHECK(hipGetLastError());
  }
  t_near.end(sg.s);
  if (!face_dev) SF_HIP_CHECK(hipMemcpyAsync(face, o_face, n_nodes * 4, hipMemcpyDeviceToHost, sg.s));
  if (dist2 && !dist_dev) SF_HIP_CHECK(hipMemcpyAsync(dist2, o_dist, n_nodes * 4, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  g_bins_us = t_count.us() + t_fill.us();
  g_nearest_us = t_near.us();
  return SF_OK;
}

int sample_device(const sf_grid_header& h, const float* value, const uint8_t* byte_label, int32_t wx, int32_t wy, int32_t wz, int64_t z0, int32_t stride,
                  int device, uint64_t first, uint64_t max_samples, float* data, uint8_t* label, int32_t* xy, uint64_t* total) {
  int rc = open_device(device, SF_ERR_DEVICE, "%s on a device needs an MI355X (device = -1 is the host path)", "the column sampler");
  if (rc != SF_OK) return rc;
  *total = 0;
  const uint64_t n_nodes = (uint64_t)h.nx * (uint64_t)h.ny * (uint64_t)h.nz, n_cols = (uint64_t)h.nx * (uint64_t)h.ny;
  if (n_nodes == 0) return SF_OK;
  if (n_cols > (1ull << 31)) return sf::fail(SF_ERR_INVALID_ARG, "the column sampler on a device: %llu columns", (unsigned long long)n_cols);
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  DevBuf d_value, d_bl, d_flags, d_offsets, d_cols, d_totals, d_data, d_label, d_xy;
  SF_HIP_CHECK(d_bl.alloc(n_nodes));
  SF_HIP_CHECK(d_flags.alloc(n_cols * 4));
  SF_HIP_CHECK(d_offsets.alloc(n_cols * 4));
  SF_HIP_CHECK(d_cols.alloc(n_cols * 4));
  SF_HIP_CHECK(d_totals.alloc(16));
  SF_HIP_CHECK(hipMemcpyAsync(d_bl.p, byte_label, n_nodes, hipMemcpyHostToDevice, sg.s));
  const int64_t zlo = z0 < 0 ? 0 : (z0 > h.nz ? h.nz : z0), zend = z0 + wz;
  const int64_t zhi = zend < zlo ? zlo : (zend > h.nz ? h.nz : zend);
  k_vl_select<<<(uint32_t)((n_cols + 255) / 256), 256, 0, sg.s>>>(d_bl.as<uint8_t>(), h.nx, h.ny, (int32_t)zlo, (int32_t)zhi, stride, d_flags.as<uint32_t>());
  SF_HIP_CHECK(hipGetLastError());
  k_vl_scan<<<1, 1024, 0, sg.s>>>(d_flags.as<uint32_t>(), (uint32_t)n_cols, d_offsets.as<uint32_t>(), d_cols.as<uint32_t>(), d_totals.as<unsigned long long>());
  SF_HIP_CHECK(hipGetLastError());
  unsigned long long totals[2] = {0, 0};
  SF_HIP_CHECK(hipMemcpyAsync(totals, d_totals.p, 16, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  *total = totals[1];
  if (first >= totals[1] || max_samples == 0) return SF_OK;
  const uint64_t n = max_samples < totals[1] - first ? max_samples : totals[1] - first;
  if (n * (uint64_t)wz > (1ull << 31) - 1) return sf::fail(SF_ERR_INVALID_ARG, "the column sampler on a device: %llu samples of %d layers in one call", (unsigned long long)n, wz);
  const size_t per = (size_t)wz * wy * wx;
  const bool data_dev = on_device(data), label_dev = on_device(label), xy_dev = on_device(xy);
  float* o_data = data;
  uint8_t* o_label = label;
  int32_t* o_xy = xy;
  SF_HIP_CHECK(d_value.alloc(n_nodes * 4));
  SF_HIP_CHECK(hipMemcpyAsync(d_value.p, value, n_nodes * 4, hipMemcpyHostToDevice, sg.s));
  if (!data_dev) { SF_HIP_CHECK(d_data.alloc(n * per * 4)); o_data = d_data.as<float>(); }
  if (!label_dev) { SF_HIP_CHECK(d_label.alloc(n * wz)); o_label = d_label.as<uint8_t>(); }
  if (!xy_dev) { SF_HIP_CHECK(d_xy.alloc(n * 8)); o_xy = d_xy.as<int32_t>(); }
  EventSpan t_sample;
  t_sample.begin(sg.s);
  k_vl_sample<<<(uint32_t)(n * (uint64_t)wz), 256, 0, sg.s>>>(d_value.as<float>(), d_bl.as<uint8_t>(), h.nx, h.ny, h.nz, d_cols.as<uint32_t>(), first, wx, wy, wz,
                                                             (long long)z0, o_data, o_label, o_xy);
  SF_HIP_CHECK(hipGetLastError());
  t_sample.end(sg.s);
  if (!data_dev) SF_HIP_CHECK(deliver(data, o_data, n * per * 4, sg.s));
  if (!label_dev) SF_HIP_CHECK(deliver(label, o_label, n * wz, sg.s));
  if (!xy_dev) SF_HIP_CHECK(deliver(xy, o_xy, n * 8, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  g_sample_us = t_sample.us();
  return SF_OK;
}

}  // namespace vl
}  // namespace sf

SF_API int sf_voxlabel_kernel_us(float* bins_us, float* nearest_us, float* sample_us) {
  if (bins_us) *bins_us = g_bins_us;
  if (nearest_us) *nearest_us = g_nearest_us;
  if (sample_us) *sample_us = g_sample_us;
  return SF_OK;
}
