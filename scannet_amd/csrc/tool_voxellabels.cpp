// tool_voxellabels.cpp -- bin/voxellabels: the voxel task's data from a scan's products (include/scanfuse.h "Voxel-task data").
// The reference's generator for Tasks/SemanticVoxelLabeling is "to come soon" (Tasks/README.md:14); what is written here is what its reader takes
// (Tasks/SemanticVoxelLabeling/torch/provider.lua:59-97: datasets `data` and `label`), as .npy files -- no HDF5 is written.
//
//   voxellabels <scan>.grid <mesh.ply> --segs=F --aggregation=F --label-map=F [-o prefix] [--band=voxels] [--window=WxHxD] [--z0=layer] [--stride=N]
//               [--max-samples=N] [--host | --device=N] [--ids-out=F] [--print-stats]
//
// <prefix>.label.npy (uint16) and <prefix>.instance.npy (uint8), [z][y][x] over the grid; <prefix>.samples.data.npy (float32 [n][1][D][H][W]) and
// <prefix>.samples.label.npy (uint8 [n][D]).  Without -o the prefix is the grid's path without ".grid".  --ids-out: the label grid read back at the
// mesh's vertices, one id per line (BenchmarkScripts/util_3d.py export_ids).  The host path is the default (DESIGN.md section 4m has the measurement);
// --device=N runs the kernels and writes the same bytes.  stderr stays empty on success.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scanfuse.h"

static int usage() {
  std::fprintf(stderr,
               "usage: voxellabels <scan>.grid <mesh.ply> --segs=F --aggregation=F --label-map=F [-o prefix] [--band=voxels] [--window=WxHxD] [--z0=layer]\n"
               "                   [--stride=N] [--max-samples=N] [--host | --device=N] [--ids-out=F] [--print-stats]\n");
  return 2;
}

static int die(const char* what, int rc) {
  std::fprintf(stderr, "voxellabels: %s: %s (%d)\n", what, sf_last_error(), rc);
  return 1;
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the header of a version 1.0 .npy file as numpy.save writes it: the dictionary padded with spaces so that the data start on a multiple of 64 bytes
static std::string npy_header(const char* descr, const std::vector<uint64_t>& shape) {
  std::string d = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (";
  for (size_t i = 0; i < shape.size(); i++) d += std::to_string(shape[i]) + (shape.size() == 1 ? "," : (i + 1 < shape.size() ? ", " : ""));
  d += "), }";
  const size_t pad = 64 - (10 + d.size() + 1) % 64;
  d.append(pad == 64 ? 0 : pad, ' ');
  d += '\n';
  std::string h("\x93NUMPY\x01\x00", 8);
  h += (char)(d.size() & 0xff);
  h += (char)(d.size() >> 8);
  return h + d;
}

static bool write_npy(const std::string& path, const char* descr, const std::vector<uint64_t>& shape, const void* data, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const std::string h = npy_header(descr, shape);
  bool ok = std::fwrite(h.data(), 1, h.size(), f) == h.size();
  if (ok && bytes) ok = std::fwrite(data, 1, bytes, f) == bytes;
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) std::remove(path.c_str());
  return ok;
}

int main(int argc, char** argv) {
  sf_voxlabel_params vp;
  sf_voxlabel_params_default(&vp);
  std::string grid_path, mesh_path, segs, agg, label_map, prefix, ids_out;
  int device = -1;
  bool print_stats = false;
  uint64_t max_samples = ~0ull;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "-o") {
      if (++i >= argc) return usage();
      prefix = argv[i];
    } else if (a.rfind("--segs=", 0) == 0) {
      segs = a.substr(7);
    } else if (a.rfind("--aggregation=", 0) == 0) {
      agg = a.substr(14);
    } else if (a.rfind("--label-map=", 0) == 0) {
      label_map = a.substr(12);
    } else if (a.rfind("--band=", 0) == 0) {
      vp.band = (float)std::atof(a.c_str() + 7);
    } else if (a.rfind("--window=", 0) == 0) {
      int w = 0, h = 0, d = 0;
      if (std::sscanf(a.c_str() + 9, "%dx%dx%d", &w, &h, &d) != 3) return usage();
      vp.wx = w; vp.wy = h; vp.wz = d;
    } else if (a.rfind("--z0=", 0) == 0) {
      vp.z0 = std::atoi(a.c_str() + 5);
      vp.z0_default = 0;
    } else if (a.rfind("--stride=", 0) == 0) {
      vp.stride = std::atoi(a.c_str() + 9);
    } else if (a.rfind("--max-samples=", 0) == 0) {
      max_samples = std::strtoull(a.c_str() + 14, nullptr, 10);
    } else if (a == "--host") {
      device = -1;
    } else if (a.rfind("--device=", 0) == 0) {
      device = std::atoi(a.c_str() + 9);
    } else if (a.rfind("--ids-out=", 0) == 0) {
      ids_out = a.substr(10);
    } else if (a == "--print-stats") {
      print_stats = true;
    } else if (!a.empty() && a[0] == '-') {
      return usage();
    } else if (grid_path.empty()) {
      grid_path = a;
    } else if (mesh_path.empty()) {
      mesh_path = a;
    } else {
      return usage();
    }
  }
  if (grid_path.empty() || mesh_path.empty() || segs.empty() || agg.empty() || label_map.empty()) return usage();
  if (prefix.empty()) {
    const size_t n = grid_path.size();
    prefix = n >= 5 && grid_path.compare(n - 5, 5, ".grid") == 0 ? grid_path.substr(0, n - 5) : grid_path;
  }
  const double t0 = now_s();
  sf_grid* grid = nullptr;
  int rc = sf_grid_load(grid_path.c_str(), &grid);
  if (rc != SF_OK) return die(grid_path.c_str(), rc);
  sf_grid_header h;
  sf_grid_info(grid, &h);
  sf_mesh* mesh = nullptr;
  if ((rc = sf_ply_read(mesh_path.c_str(), &mesh)) != SF_OK) { sf_grid_free(grid); return die(mesh_path.c_str(), rc); }
  uint64_t nv = 0, nf = 0;
  sf_mesh_counts(mesh, &nv, &nf);
  std::vector<float> xyz(3 * nv);
  std::vector<uint32_t> tris(3 * nf);
  rc = sf_mesh_copy(mesh, xyz.data(), nullptr, tris.data(), nullptr);
  sf_mesh_free(mesh);
  if (rc != SF_OK) { sf_grid_free(grid); return die(mesh_path.c_str(), rc); }
  std::vector<uint8_t> vinst(nv);
  std::vector<uint16_t> vlabel(nv);
  if ((rc = sf_annotation_vertex_ids(segs.c_str(), agg.c_str(), label_map.c_str(), nv, vinst.data(), vlabel.data(), nullptr)) != SF_OK) {
    sf_grid_free(grid);
    return die("annotations", rc);
  }
  const double t1 = now_s();
  const size_t n_nodes = (size_t)h.nx * (size_t)h.ny * (size_t)h.nz;
  std::vector<int32_t> face(n_nodes);
  std::vector<uint16_t> label(n_nodes);
  std::vector<uint8_t> inst(n_nodes), bl(n_nodes);
  if ((rc = sf_voxlabel_nearest_faces(&h, xyz.data(), nv, tris.data(), nf, vp.band, device, face.data(), nullptr)) != SF_OK) { sf_grid_free(grid); return die("nearest faces", rc); }
  const double t2 = now_s();
  if ((rc = sf_voxlabel_labels(face.data(), n_nodes, tris.data(), nf, nv, vlabel.data(), vinst.data(), label.data(), inst.data(), bl.data())) != SF_OK) {
    sf_grid_free(grid);
    return die("labels", rc);
  }
  const double t3 = now_s();
  // the samples, counted first (this is also where a bad window is refused: before any file is written), then page by page behind the .npy headers
  uint64_t total = 0;
  if ((rc = sf_voxlabel_sample_columns(grid, bl.data(), &vp, device, 0, 0, nullptr, nullptr, nullptr, &total)) != SF_OK) { sf_grid_free(grid); return die("samples", rc); }
  const uint64_t n_samples = total < max_samples ? total : max_samples;
  const std::vector<uint64_t> dims = {(uint64_t)h.nz, (uint64_t)h.ny, (uint64_t)h.nx};
  bool ok = write_npy(prefix + ".label.npy", "<u2", dims, label.data(), n_nodes * 2) && write_npy(prefix + ".instance.npy", "|u1", dims, inst.data(), n_nodes);
  const std::string data_path = prefix + ".samples.data.npy", slabel_path = prefix + ".samples.label.npy";
  FILE* fd = ok ? std::fopen(data_path.c_str(), "wb") : nullptr;
  FILE* fl = fd ? std::fopen(slabel_path.c_str(), "wb") : nullptr;
  ok = ok && fd && fl;
  if (ok) {
    const std::string hd = npy_header("<f4", {n_samples, 1, (uint64_t)vp.wz, (uint64_t)vp.wy, (uint64_t)vp.wx}), hl = npy_header("|u1", {n_samples, (uint64_t)vp.wz});
    ok = std::fwrite(hd.data(), 1, hd.size(), fd) == hd.size() && std::fwrite(hl.data(), 1, hl.size(), fl) == hl.size();
  }
  const size_t per = (size_t)vp.wx * (size_t)vp.wy * (size_t)vp.wz;
  const uint64_t page = per ? (((64ull << 20) / (per * 4)) ? (64ull << 20) / (per * 4) : 1) : 1;   // 64 MiB of samples at a time
  std::vector<float> data;
  std::vector<uint8_t> slabel;
  std::vector<int32_t> xy;
  for (uint64_t first = 0; ok && rc == SF_OK && first < n_samples; first += page) {
    const uint64_t n = n_samples - first < page ? n_samples - first : page;
    data.resize(n * per); slabel.resize(n * (size_t)vp.wz); xy.resize(2 * n);
    rc = sf_voxlabel_sample_columns(grid, bl.data(), &vp, device, first, n, data.data(), slabel.data(), xy.data(), &total);
    if (rc == SF_OK) ok = std::fwrite(data.data(), 4, data.size(), fd) == data.size() && std::fwrite(slabel.data(), 1, slabel.size(), fl) == slabel.size();
  }
  if (fd) ok = (std::fclose(fd) == 0) && ok;
  if (fl) ok = (std::fclose(fl) == 0) && ok;
  sf_grid_free(grid);
  if (rc != SF_OK) return die("samples", rc);
  if (!ok) { std::fprintf(stderr, "voxellabels: cannot write %s.*.npy\n", prefix.c_str()); return 1; }
  const double t4 = now_s();
  if (!ids_out.empty()) {
    // export_semantic_label_grid_for_evaluation.py:40-47: world2grid, floor, clamp, grid[z][y][x]
    FILE* f = n_nodes ? std::fopen(ids_out.c_str(), "w") : nullptr;
    if (!f) { std::fprintf(stderr, "voxellabels: cannot write %s%s\n", ids_out.c_str(), n_nodes ? "" : " (the grid is empty)"); return 1; }
    const float* m = h.world2grid;
    const int32_t dim[3] = {h.nx, h.ny, h.nz};
    for (uint64_t v = 0; v < nv; v++) {
      int64_t idx[3];
      for (int a = 0; a < 3; a++) {
        const float g = ((m[4 * a] * xyz[3 * v] + m[4 * a + 1] * xyz[3 * v + 1]) + m[4 * a + 2] * xyz[3 * v + 2]) + m[4 * a + 3];
        const float fl32 = std::floor(g);
        idx[a] = !(fl32 >= 0.0f) ? 0 : (fl32 >= (float)dim[a] ? dim[a] - 1 : (int64_t)fl32);
      }
      std::fprintf(f, "%u\n", (unsigned)label[((size_t)idx[2] * h.ny + idx[1]) * h.nx + idx[0]]);
    }
    if (std::fclose(f) != 0) { std::fprintf(stderr, "voxellabels: short write to %s\n", ids_out.c_str()); return 1; }
  }
  uint64_t hit = 0, task = 0;
  for (size_t i = 0; i < n_nodes; i++) { hit += face[i] >= 0; task += bl[i] != 0 && bl[i] != 255; }
  std::printf("Wrote %s.{label,instance,samples.data,samples.label}.npy: %d x %d x %d nodes, %llu of %llu samples of %d x %d x %d\n", prefix.c_str(), h.nx, h.ny, h.nz,
              (unsigned long long)n_samples, (unsigned long long)total, vp.wx, vp.wy, vp.wz);
  if (print_stats) {
    std::printf("mesh: %llu vertices, %llu faces; nodes: %llu with a face, %llu with a task label; path: %s\n", (unsigned long long)nv, (unsigned long long)nf,
                (unsigned long long)hit, (unsigned long long)task, device < 0 ? "host" : "device");
    std::printf("seconds: read %.4f, nearest %.4f, labels %.4f, samples %.4f, total %.4f\n", t1 - t0, t2 - t1, t3 - t2, t4 - t3, now_s() - t0);
  }
  return 0;
}
