// object_voxels.hip -- the device path of the object tasks' data (include/scanfuse.h "Object-task data"): an occupancy and a
// known grid per annotated object.  The rule is object_voxels_internal.h's, the host path of the same bytes is object_voxels.cpp.
//
//   k_ov_key     a thread per face: its object and whether it is counted; a wave adds each run of equal objects to the object's count once
//   k_ov_scan    one workgroup: exclusive scan of the counts
//   k_ov_fill    a thread per face: its index into its object's list, a slot range per run (integer atomics: occupancy is an OR, the order of a list
//                does not show)
//   k_ov_box     a workgroup per object: min / max over the vertices of its faces, then the cube by one lane in the rule's operation order
//   k_ov_raster  a workgroup per (object, chunk of 256 faces): the object's bit mask in LDS, a face per lane, the exact overlap test over the cells of the
//                face's range; merged into the object's mask in memory by a plain store (one chunk) or by vector atomics (several)
//   k_ov_emit    a workgroup per (object, z layer): bits to bytes, the known lookup by a clamped load and a select, lanes along x and on through the rows
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <vector>

#include "common.h"
#include "hip_util.h"
#include "object_voxels_internal.h"

namespace {

using sf::ov::CHUNK;
using sf::ov::Cube;
using sf::ov::GridRef;
using sf::ov::Kept;
using sf::ov::MASK_WORDS;
using sf::ov::QTri;

struct WorkItem {
  uint32_t s;       // index into the page's kept objects
  uint32_t chunk;   // which 256 faces of it
};

// Neighbouring faces of a mesh mostly belong to one object, so a wave adds once per run of equal keys, not once per lane.  Every lane of the wave
// calls this (key 0 for a lane without a face).  -> is this lane the first of its run; *first: the run's first lane; *len: the run's length
__device__ inline bool key_run(uint32_t key, uint32_t* first, uint32_t* len) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t before = __shfl_up(key, 1);
  const bool head = lane == 0u || before != key;
  const unsigned long long heads = __ballot(head);                       // bit 0 is always set
  const unsigned long long upto = heads & (~0ull >> (63u - lane));      // the heads at or below this lane
  const unsigned long long above = lane == 63u ? 0ull : heads & (~0ull << (lane + 1u));
  *first = 63u - (uint32_t)__clzll((long long)upto);
  *len = (above ? (uint32_t)__ffsll((long long)above) - 1u : 64u) - *first;
  return head;
}

__global__ __launch_bounds__(256) void k_ov_key(const float* __restrict__ xyz, const uint32_t* __restrict__ tris, const uint32_t* __restrict__ vertex_object,
                                                uint32_t nf, uint32_t* __restrict__ face_object, uint32_t* __restrict__ counts) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  uint32_t key = 0u;
  if (f < nf) {
    bool counted = false;
    const uint32_t o = sf::ov::face_object(xyz, tris, vertex_object, f, &counted);
    key = counted ? o : 0u;
    face_object[f] = key;
  }
  uint32_t first, len;
  if (key_run(key, &first, &len) && key) atomicAdd(&counts[key], len);
}

// offsets[i] = sum of counts[0 .. i); *total = the sum
__global__ __launch_bounds__(1024) void k_ov_scan(const uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ offsets, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_sum[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t b = min(t * per, n), e = min(b + per, n);
  unsigned long long sum = 0;
  for (uint32_t i = b; i < e; i++) sum += counts[i];
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const unsigned long long v = t >= d ? s_sum[t - d] : 0ull;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  unsigned long long run = s_sum[t] - sum;
  for (uint32_t i = b; i < e; i++) {
    offsets[i] = (uint32_t)run;
    run += counts[i];
  }
  if (t == 1023) *total = s_sum[1023];
}

__global__ __launch_bounds__(256) void k_ov_fill(const uint32_t* __restrict__ face_object, uint32_t nf, const uint32_t* __restrict__ offsets,
                                                 uint32_t* __restrict__ cursor, uint32_t* __restrict__ list, unsigned long long total) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  const uint32_t key = f < nf ? face_object[f] : 0u;
  uint32_t first, len, base = 0u;
  if (key_run(key, &first, &len) && key) base = offsets[key] + atomicAdd(&cursor[key], len);   // below the list's length, which is at most 2^31
  base = __shfl(base, (int)first);
  const unsigned long long at = (unsigned long long)base + ((threadIdx.x & 63u) - first);
  if (key && at < total) list[at] = f;
}

__device__ inline float wave_min(float v) {
  for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
  return v;
}
__device__ inline float wave_max(float v) {
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}

// object blockIdx.x + 1.  min and max are exact and order-free; the cube is computed once, by one lane.
__global__ __launch_bounds__(256) void k_ov_box(const float* __restrict__ xyz, const uint32_t* __restrict__ tris, const uint32_t* __restrict__ counts,
                                                const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ list, int32_t dim, int32_t fit,
                                                Cube* __restrict__ cubes) {
  __shared__ float s_lo[4][3], s_hi[4][3];
  const uint32_t o = blockIdx.x + 1u;
  const uint32_t n = counts[o], off = offsets[o];
  float lox = INFINITY, loy = INFINITY, loz = INFINITY, hix = -INFINITY, hiy = -INFINITY, hiz = -INFINITY;
  for (uint32_t j = threadIdx.x; j < n; j += 256u) {
    const uint32_t f = list[off + j];
    for (int v = 0; v < 3; v++) {
      const float* p = xyz + 3 * (size_t)tris[3 * (size_t)f + v];
      lox = fminf(lox, p[0]); loy = fminf(loy, p[1]); loz = fminf(loz, p[2]);
      hix = fmaxf(hix, p[0]); hiy = fmaxf(hiy, p[1]); hiz = fmaxf(hiz, p[2]);
    }
  }
  lox = wave_min(lox); loy = wave_min(loy); loz = wave_min(loz);
  hix = wave_max(hix); hiy = wave_max(hiy); hiz = wave_max(hiz);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    s_lo[wave][0] = lox; s_lo[wave][1] = loy; s_lo[wave][2] = loz;
    s_hi[wave][0] = hix; s_hi[wave][1] = hiy; s_hi[wave][2] = hiz;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    lox = fminf(fminf(s_lo[0][0], s_lo[1][0]), fminf(s_lo[2][0], s_lo[3][0]));
    loy = fminf(fminf(s_lo[0][1], s_lo[1][1]), fminf(s_lo[2][1], s_lo[3][1]));
    loz = fminf(fminf(s_lo[0][2], s_lo[1][2]), fminf(s_lo[2][2], s_lo[3][2]));
    hix = fmaxf(fmaxf(s_hi[0][0], s_hi[1][0]), fmaxf(s_hi[2][0], s_hi[3][0]));
    hiy = fmaxf(fmaxf(s_hi[0][1], s_hi[1][1]), fmaxf(s_hi[2][1], s_hi[3][1]));
    hiz = fmaxf(fmaxf(s_hi[0][2], s_hi[1][2]), fmaxf(s_hi[2][2], s_hi[3][2]));
    cubes[o] = sf::ov::make_cube(lox, loy, loz, hix, hiy, hiz, dim, fit);
  }
}

__global__ __launch_bounds__(256) void k_ov_raster(const float* __restrict__ xyz, const uint32_t* __restrict__ tris, const uint32_t* __restrict__ list,
                                                   const Kept* __restrict__ kept, const WorkItem* __restrict__ work, int32_t dim, uint32_t words,
                                                   uint32_t* __restrict__ mask) {
  __shared__ uint32_t s_mask[MASK_WORDS];
  const WorkItem item = work[blockIdx.x];
  const Kept k = kept[item.s];
  for (uint32_t i = threadIdx.x; i < words; i += 256u) s_mask[i] = 0u;
  __syncthreads();
  const uint32_t j = item.chunk * CHUNK + threadIdx.x;
  if (j < k.count) {
    const QTri t = sf::ov::quantise_face(xyz, tris, list[k.first + j], k.cube, dim);
    if (!sf::ov::no_area(t)) {
      int32_t x0, x1, y0, y1, z0, z1;
      sf::ov::cell_range(sf::ov::min3(t.ax, t.bx, t.cx), sf::ov::max3(t.ax, t.bx, t.cx), dim, &x0, &x1);
      sf::ov::cell_range(sf::ov::min3(t.ay, t.by, t.cy), sf::ov::max3(t.ay, t.by, t.cy), dim, &y0, &y1);
      sf::ov::cell_range(sf::ov::min3(t.az, t.bz, t.cz), sf::ov::max3(t.az, t.bz, t.cz), dim, &z0, &z1);
      for (int32_t z = z0; z <= z1; z++)
        for (int32_t y = y0; y <= y1; y++)
          for (int32_t x = x0; x <= x1; x++)
            if (sf::ov::meets(t, x, y, z)) {
              const uint32_t bit = (uint32_t)((z * dim + y) * dim + x);   // below dim^3 <= 32 words x 1024
              atomicOr(&s_mask[bit >> 5], 1u << (bit & 31u));
            }
    }
  }
  __syncthreads();
  uint32_t* out = mask + (size_t)item.s * words;
  if (k.count <= CHUNK) {
    for (uint32_t i = threadIdx.x; i < words; i += 256u) out[i] = s_mask[i];
  } else {
    for (uint32_t i = threadIdx.x; i < words; i += 256u)
      if (s_mask[i]) atomicOr(&out[i], s_mask[i]);
  }
}

__global__ __launch_bounds__(256) void k_ov_emit(const Kept* __restrict__ kept, const uint32_t* __restrict__ mask, GridRef grid, int32_t dim, uint32_t words,
                                                 uint8_t* __restrict__ data, uint8_t* __restrict__ label, int32_t* __restrict__ object_id,
                                                 float* __restrict__ origin, float* __restrict__ cell) {
  const uint32_t s = blockIdx.x / (uint32_t)dim;
  const int32_t z = (int32_t)(blockIdx.x - s * (uint32_t)dim);
  const Kept k = kept[s];
  const uint32_t* bits = mask + (size_t)s * words;
  const uint32_t layer = (uint32_t)(dim * dim), cells = layer * (uint32_t)dim;
  uint8_t* occ = data + (size_t)s * 2u * cells + (size_t)z * layer;
  uint8_t* known = occ + cells;
  bool zin = false;
  const int32_t gz = grid.mode ? sf::ov::grid_node(k.cube.oz, k.cube.c, z, grid.voxel, grid.loz, grid.nz, &zin) : 0;
  for (uint32_t e = threadIdx.x; e < layer; e += 256u) {
    const int32_t y = (int32_t)(e / (uint32_t)dim), x = (int32_t)(e - (uint32_t)y * (uint32_t)dim);
    const uint32_t bit = (uint32_t)z * layer + e;
    const uint32_t o = (bits[bit >> 5] >> (bit & 31u)) & 1u;
    uint32_t kn = 1u;
    if (grid.mode) {
      bool yin = false, xin = false;
      const int32_t gy = sf::ov::grid_node(k.cube.oy, k.cube.c, y, grid.voxel, grid.loy, grid.ny, &yin);
      const int32_t gx = sf::ov::grid_node(k.cube.ox, k.cube.c, x, grid.voxel, grid.lox, grid.nx, &xin);
      uint32_t w = 0u;
      if (grid.mode == 1) w = grid.weight[((size_t)gz * grid.ny + gy) * grid.nx + gx];   // clamped: inside the grid whatever the centre is
      kn = ((zin && yin && xin && w > 0u) || o) ? 1u : 0u;
    }
    occ[e] = (uint8_t)o;
    known[e] = (uint8_t)kn;
  }
  if (z == 0 && threadIdx.x == 0) {
    label[s] = (uint8_t)k.label;
    object_id[s] = (int32_t)k.object - 1;
    origin[3 * (size_t)s] = k.cube.ox; origin[3 * (size_t)s + 1] = k.cube.oy; origin[3 * (size_t)s + 2] = k.cube.oz;
    cell[s] = k.cube.c;
  }
}

// device microseconds of the most recent call's launches: k_ov_key .. k_ov_box, k_ov_raster, k_ov_emit (sf_objvox_kernel_us)
std::atomic<float> g_group_us{0.0f}, g_raster_us{0.0f}, g_emit_us{0.0f};

}  // namespace

namespace sf {
namespace ov {

int voxelize_device(const float* xyz, uint64_t nv, const uint32_t* tris, uint64_t nf, const uint32_t* vertex_object, const int32_t* object_class,
                    uint32_t num_objects, const GridRef& grid, uint64_t grid_nodes, const sf_objvox_params& p, int device, uint64_t first, uint64_t max_objects,
                    uint8_t* data, uint8_t* label, int32_t* object_id, float* origin, float* cell, uint64_t* total, const StageOut* stage) {
  if (int rc = open_device(device, SF_ERR_DEVICE, "the object voxeliser on a device needs an MI355X (device = -1 is the host path)")) return rc;
  *total = 0;
  if (stage && stage->total) *stage->total = 0;
  const uint32_t n_keys = num_objects + 1u;   // indexed by the vertex_object value
  StreamGuard sg;
  SF_HIP_CHECK(hipStreamCreate(&sg.s));
  DevBuf d_xyz, d_tris, d_vo, d_fobj, d_counts, d_offsets, d_cursor, d_total, d_list, d_cubes, d_kept, d_work, d_mask, d_weight, d_data, d_label, d_id, d_origin, d_cell;
  SF_HIP_CHECK(d_xyz.alloc(nv * 12));
  SF_HIP_CHECK(d_tris.alloc(nf * 12));
  SF_HIP_CHECK(d_vo.alloc(nv * 4));
  SF_HIP_CHECK(d_fobj.alloc(nf * 4));
  SF_HIP_CHECK(d_counts.alloc((size_t)n_keys * 4));
  SF_HIP_CHECK(d_offsets.alloc((size_t)n_keys * 4));
  SF_HIP_CHECK(d_cursor.alloc((size_t)n_keys * 4));
  SF_HIP_CHECK(d_total.alloc(8));
  if (nv) SF_HIP_CHECK(hipMemcpyAsync(d_xyz.p, xyz, nv * 12, hipMemcpyHostToDevice, sg.s));
  if (nv) SF_HIP_CHECK(hipMemcpyAsync(d_vo.p, vertex_object, nv * 4, hipMemcpyHostToDevice, sg.s));
  if (nf) SF_HIP_CHECK(hipMemcpyAsync(d_tris.p, tris, nf * 12, hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemsetAsync(d_counts.p, 0, (size_t)n_keys * 4, sg.s));
  SF_HIP_CHECK(hipMemsetAsync(d_cursor.p, 0, (size_t)n_keys * 4, sg.s));
  const uint32_t face_blocks = (uint32_t)((nf + 255) / 256);
  EventSpan t_group, t_fill, t_raster, t_emit;
  t_group.begin(sg.s);
  if (nf) {
    k_ov_key<<<face_blocks, 256, 0, sg.s>>>(d_xyz.as<float>(), d_tris.as<uint32_t>(), d_vo.as<uint32_t>(), (uint32_t)nf, d_fobj.as<uint32_t>(), d_counts.as<uint32_t>());
    SF_HIP_CHECK(hipGetLastError());
  }
  k_ov_scan<<<1, 1024, 0, sg.s>>>(d_counts.as<uint32_t>(), n_keys, d_offsets.as<uint32_t>(), d_total.as<unsigned long long>());
  SF_HIP_CHECK(hipGetLastError());
  t_group.end(sg.s);
  unsigned long long listed = 0;
  SF_HIP_CHECK(hipMemcpyAsync(&listed, d_total.p, 8, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  if (listed > nf) return sf::fail(SF_ERR_DEVICE, "the object voxeliser: %llu listed faces of %llu", listed, (unsigned long long)nf);
  SF_HIP_CHECK(d_list.alloc((size_t)listed * 4));
  SF_HIP_CHECK(d_cubes.alloc((size_t)n_keys * sizeof(Cube)));
  t_fill.begin(sg.s);
  if (listed) {
    SF_HIP_CHECK(hipMemsetAsync(d_list.p, 0, (size_t)listed * 4, sg.s));   // the later kernels index the faces with what they read here
    k_ov_fill<<<face_blocks, 256, 0, sg.s>>>(d_fobj.as<uint32_t>(), (uint32_t)nf, d_offsets.as<uint32_t>(), d_cursor.as<uint32_t>(), d_list.as<uint32_t>(), listed);
    SF_HIP_CHECK(hipGetLastError());
  }
  if (stage) {
    t_fill.end(sg.s);
    if (stage->total) *stage->total = listed;
    if (stage->list && stage->capacity < listed)
      return sf::fail(SF_ERR_BOUNDS, "the face stage: %llu entries, capacity %llu", listed, (unsigned long long)stage->capacity);
    if (stage->face_object && nf) SF_HIP_CHECK(hipMemcpyAsync(stage->face_object, d_fobj.p, nf * 4, hipMemcpyDeviceToHost, sg.s));
    if (stage->counts) SF_HIP_CHECK(hipMemcpyAsync(stage->counts, d_counts.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, sg.s));
    if (stage->offsets) SF_HIP_CHECK(hipMemcpyAsync(stage->offsets, d_offsets.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, sg.s));
    if (stage->list && listed) SF_HIP_CHECK(hipMemcpyAsync(stage->list, d_list.p, (size_t)listed * 4, hipMemcpyDeviceToHost, sg.s));
    SF_HIP_CHECK(hipStreamSynchronize(sg.s));
    g_group_us = t_group.us() + t_fill.us();
    return SF_OK;
  }
  if (num_objects) {
    k_ov_box<<<num_objects, 256, 0, sg.s>>>(d_xyz.as<float>(), d_tris.as<uint32_t>(), d_counts.as<uint32_t>(), d_offsets.as<uint32_t>(), d_list.as<uint32_t>(), p.dim,
                                           p.fit, d_cubes.as<Cube>());
    SF_HIP_CHECK(hipGetLastError());
  }
  t_fill.end(sg.s);
  // which objects are kept, and the page's work list, on the host: a few bytes per object
  std::vector<uint32_t> counts(n_keys), offsets(n_keys);
  std::vector<Cube> cubes(n_keys);
  SF_HIP_CHECK(hipMemcpyAsync(counts.data(), d_counts.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipMemcpyAsync(offsets.data(), d_offsets.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, sg.s));
  if (num_objects) SF_HIP_CHECK(hipMemcpyAsync(cubes.data() + 1, d_cubes.as<Cube>() + 1, (size_t)num_objects * sizeof(Cube), hipMemcpyDeviceToHost, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  g_group_us = t_group.us() + t_fill.us();
  std::vector<Kept> all;
  for (uint32_t o = 1; o <= num_objects; o++) {
    if (counts[o] == 0 || !kept(p, object_class[o - 1], counts[o], cubes[o])) continue;
    if ((uint64_t)offsets[o] + counts[o] > listed) return sf::fail(SF_ERR_DEVICE, "the object voxeliser: object %u's faces leave the list", o - 1);
    all.push_back(Kept{o, label_of(object_class[o - 1]), offsets[o], counts[o], cubes[o]});
  }
  *total = all.size();
  if (first >= all.size() || max_objects == 0) return SF_OK;
  const uint64_t n = max_objects < all.size() - first ? max_objects : all.size() - first;
  std::vector<WorkItem> work;
  for (uint64_t s = 0; s < n; s++)
    for (uint32_t c = 0; c * CHUNK < all[first + s].count; c++) work.push_back(WorkItem{(uint32_t)s, c});
  const int32_t dim = p.dim;
  const size_t cells = (size_t)dim * dim * dim;
  const uint32_t words = (uint32_t)((cells + 31) / 32);   // at most MASK_WORDS: dim <= 32
  if (n * (uint64_t)dim > (1ull << 31) - 1 || work.size() > (1ull << 31) - 1)
    return sf::fail(SF_ERR_INVALID_ARG, "the object voxeliser on a device: %llu objects in one call", (unsigned long long)n);
  GridRef g = grid;
  if (g.mode == 1) {
    SF_HIP_CHECK(d_weight.alloc(grid_nodes));
    SF_HIP_CHECK(hipMemcpyAsync(d_weight.p, grid.weight, grid_nodes, hipMemcpyHostToDevice, sg.s));
    g.weight = d_weight.as<uint8_t>();
  } else {
    g.weight = nullptr;
  }
  SF_HIP_CHECK(d_kept.alloc(n * sizeof(Kept)));
  SF_HIP_CHECK(d_work.alloc(work.size() * sizeof(WorkItem)));
  SF_HIP_CHECK(d_mask.alloc(n * words * 4));
  SF_HIP_CHECK(hipMemcpyAsync(d_kept.p, all.data() + first, n * sizeof(Kept), hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemcpyAsync(d_work.p, work.data(), work.size() * sizeof(WorkItem), hipMemcpyHostToDevice, sg.s));
  SF_HIP_CHECK(hipMemsetAsync(d_mask.p, 0, n * words * 4, sg.s));
  const bool data_dev = on_device(data), label_dev = on_device(label), id_dev = on_device(object_id), origin_dev = on_device(origin), cell_dev = on_device(cell);
  uint8_t* o_data = data;
  uint8_t* o_label = label;
  int32_t* o_id = object_id;
  float* o_origin = origin;
  float* o_cell = cell;
  if (!data_dev) { SF_HIP_CHECK(d_data.alloc(n * 2 * cells)); o_data = d_data.as<uint8_t>(); }
  if (!label_dev) { SF_HIP_CHECK(d_label.alloc(n)); o_label = d_label.as<uint8_t>(); }
  if (!id_dev) { SF_HIP_CHECK(d_id.alloc(n * 4)); o_id = d_id.as<int32_t>(); }
  if (!origin_dev) { SF_HIP_CHECK(d_origin.alloc(n * 12)); o_origin = d_origin.as<float>(); }
  if (!cell_dev) { SF_HIP_CHECK(d_cell.alloc(n * 4)); o_cell = d_cell.as<float>(); }
  t_raster.begin(sg.s);
  k_ov_raster<<<(uint32_t)work.size(), 256, 0, sg.s>>>(d_xyz.as<float>(), d_tris.as<uint32_t>(), d_list.as<uint32_t>(), d_kept.as<Kept>(), d_work.as<WorkItem>(), dim,
                                                      words, d_mask.as<uint32_t>());
  SF_HIP_CHECK(hipGetLastError());
  t_raster.end(sg.s);
  t_emit.begin(sg.s);
  k_ov_emit<<<(uint32_t)(n * (uint64_t)dim), 256, 0, sg.s>>>(d_kept.as<Kept>(), d_mask.as<uint32_t>(), g, dim, words, o_data, o_label, o_id, o_origin, o_cell);
  SF_HIP_CHECK(hipGetLastError());
  t_emit.end(sg.s);
  if (!data_dev) SF_HIP_CHECK(deliver(data, o_data, n * 2 * cells, sg.s));
  if (!label_dev) SF_HIP_CHECK(deliver(label, o_label, n, sg.s));
  if (!id_dev) SF_HIP_CHECK(deliver(object_id, o_id, n * 4, sg.s));
  if (!origin_dev) SF_HIP_CHECK(deliver(origin, o_origin, n * 12, sg.s));
  if (!cell_dev) SF_HIP_CHECK(deliver(cell, o_cell, n * 4, sg.s));
  SF_HIP_CHECK(hipStreamSynchronize(sg.s));
  g_raster_us = t_raster.us();
  g_emit_us = t_emit.us();
  return SF_OK;
}

}  // namespace ov
}  // namespace sf

SF_API int sf_objvox_kernel_us(float* group_us, float* raster_us, float* emit_us) {
  if (group_us) *group_us = g_group_us;
  if (raster_us) *raster_us = g_raster_us;
  if (emit_us) *emit_us = g_emit_us;
  return SF_OK;
}
