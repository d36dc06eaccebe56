// tool_objectvoxels.cpp -- bin/objectvoxels: the object tasks' data from a scan's products (include/scanfuse.h "Object-task data").
// The reference's generator for Tasks/ObjectClassification and Tasks/ObjectRetrieval is "to come soon" (Tasks/README.md:14); what is written here is what
// their readers take (Tasks/ObjectClassification/torch/provider.lua:40-47, Tasks/ObjectRetrieval/generate_feat.lua:74-81,87,101-109: datasets `data` and
// `label`, and the file of sample names), as .npy files -- no HDF5 is written.
//
//   objectvoxels <mesh.ply> [<scan>.grid] --segs=F --aggregation=F --label-map=F --classes=F [-o prefix] [--dim=N] [--fit=N] [--min-faces=N]
//                [--label-from=col] [--label-to=col] [--all-objects] [--host | --device=N] [--print-stats]
//
// <prefix>.objects.data.npy (uint8 [n][2][dim][dim][dim]), <prefix>.objects.label.npy (uint8 [n]), <prefix>.objects.id.npy (int32 [n]) and
// <prefix>.objects.names.txt (one `<prefix basename>_<objectId> <label>` line per sample).  Without -o the prefix is the mesh's path without ".ply".
// Without a grid the known channel is all ones.  The host path is the default; --device=N runs the kernels and writes the same
// bytes.  stderr stays empty on success.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "scanfuse.h"

static int usage() {
  std::fprintf(stderr,
               "usage: objectvoxels <mesh.ply> [<scan>.grid] --segs=F --aggregation=F --label-map=F --classes=F [-o prefix] [--dim=N] [--fit=N] [--min-faces=N]\n"
               "                    [--label-from=col] [--label-to=col] [--all-objects] [--host | --device=N] [--print-stats]\n");
  return 2;
}

static int die(const char* what, int rc) {
  std::fprintf(stderr, "objectvoxels: %s: %s (%d)\n", what, sf_last_error(), rc);
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
  sf_objvox_params vp;
  sf_objvox_params_default(&vp);
  std::string grid_path, mesh_path, segs, agg, label_map, classes, prefix, label_from, label_to;
  int device = -1;
  bool print_stats = false;
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
    } else if (a.rfind("--classes=", 0) == 0) {
      classes = a.substr(10);
    } else if (a.rfind("--dim=", 0) == 0) {
      vp.dim = std::atoi(a.c_str() + 6);
    } else if (a.rfind("--fit=", 0) == 0) {
      vp.fit = std::atoi(a.c_str() + 6);
    } else if (a.rfind("--min-faces=", 0) == 0) {
      vp.min_faces = std::atoi(a.c_str() + 12);
    } else if (a.rfind("--label-from=", 0) == 0) {
      label_from = a.substr(13);
    } else if (a.rfind("--label-to=", 0) == 0) {
      label_to = a.substr(11);
    } else if (a == "--all-objects") {
      vp.all_objects = 1;
    } else if (a == "--host") {
      device = -1;
    } else if (a.rfind("--device=", 0) == 0) {
      device = std::atoi(a.c_str() + 9);
    } else if (a == "--print-stats") {
      print_stats = true;
    } else if (!a.empty() && a[0] == '-') {
      return usage();
    } else if (mesh_path.empty()) {
      mesh_path = a;
    } else if (grid_path.empty()) {
      grid_path = a;
    } else {
      return usage();
    }
  }
  if (mesh_path.empty() || segs.empty() || agg.empty() || label_map.empty() || classes.empty()) return usage();
  if (prefix.empty()) {
    const size_t n = mesh_path.size();
    prefix = n >= 4 && mesh_path.compare(n - 4, 4, ".ply") == 0 ? mesh_path.substr(0, n - 4) : mesh_path;
  }
  const double t0 = now_s();
  sf_grid* grid = nullptr;
  int rc = SF_OK;
  if (!grid_path.empty() && (rc = sf_grid_load(grid_path.c_str(), &grid)) != SF_OK) return die(grid_path.c_str(), rc);
  sf_mesh* mesh = nullptr;
  if ((rc = sf_ply_read(mesh_path.c_str(), &mesh)) != SF_OK) { sf_grid_free(grid); return die(mesh_path.c_str(), rc); }
  uint64_t nv = 0, nf = 0;
  sf_mesh_counts(mesh, &nv, &nf);
  std::vector<float> xyz(3 * nv);
  std::vector<uint32_t> tris(3 * nf);
  rc = sf_mesh_copy(mesh, xyz.data(), nullptr, tris.data(), nullptr);
  sf_mesh_free(mesh);
  if (rc != SF_OK) { sf_grid_free(grid); return die(mesh_path.c_str(), rc); }
  std::vector<uint32_t> vobj(nv);
  uint32_t nobj = 0;
  char* names = nullptr;
  if ((rc = sf_annotation_vertex_objects(segs.c_str(), agg.c_str(), nv, vobj.data(), &nobj, &names)) != SF_OK) { sf_grid_free(grid); return die("annotations", rc); }
  std::vector<int32_t> cls(nobj, -1);
  rc = sf_objvox_classes(names, label_map.c_str(), classes.c_str(), label_from.empty() ? nullptr : label_from.c_str(), label_to.empty() ? nullptr : label_to.c_str(), nobj,
                         cls.data());
  std::map<long, std::string> name_of;
  for (const char* p = names; p && *p;) {
    const char* e = std::strchr(p, '\n');
    const std::string line = e ? std::string(p, e) : std::string(p);
    const size_t tab = line.find('\t');
    if (tab != std::string::npos) name_of[std::atol(line.c_str())] = line.substr(tab + 1);
    p = e ? e + 1 : p + line.size();
  }
  sf_free(names);
  if (rc != SF_OK) { sf_grid_free(grid); return die("classes", rc); }
  const double t1 = now_s();
  // counted first (this is also where bad parameters are refused: before any file is written)
  uint64_t total = 0;
  if ((rc = sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, grid, &vp, device, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                               &total)) != SF_OK) {
    sf_grid_free(grid);
    return die("objects", rc);
  }
  const size_t per = 2 * (size_t)vp.dim * vp.dim * vp.dim;
  std::vector<uint8_t> data(total * per), label(total);
  std::vector<int32_t> oid(total);
  std::vector<float> origin(3 * total), cell(total);
  if (total) rc = sf_objvox_voxelize(xyz.data(), nv, tris.data(), nf, vobj.data(), cls.data(), nobj, grid, &vp, device, 0, total, data.data(), label.data(), oid.data(),
                                     origin.data(), cell.data(), &total);
  sf_grid_free(grid);
  if (rc != SF_OK) return die("objects", rc);
  const double t2 = now_s();
  const uint64_t d = (uint64_t)vp.dim;
  bool ok = write_npy(prefix + ".objects.data.npy", "|u1", {total, 2, d, d, d}, data.data(), data.size()) &&
            write_npy(prefix + ".objects.label.npy", "|u1", {total}, label.data(), label.size()) &&
            write_npy(prefix + ".objects.id.npy", "<i4", {total}, oid.data(), oid.size() * 4);
  if (ok) {
    const size_t slash = prefix.find_last_of('/');
    const std::string base = slash == std::string::npos ? prefix : prefix.substr(slash + 1);
    FILE* f = std::fopen((prefix + ".objects.names.txt").c_str(), "w");
    ok = f != nullptr;
    for (uint64_t i = 0; ok && i < total; i++) ok = std::fprintf(f, "%s_%d %s\n", base.c_str(), oid[i], name_of[oid[i]].c_str()) > 0;
    if (f) ok = (std::fclose(f) == 0) && ok;
  }
  if (!ok) { std::fprintf(stderr, "objectvoxels: cannot write %s.objects.*\n", prefix.c_str()); return 1; }
  uint64_t occ = 0, known = 0;
  const size_t cells = per / 2;
  for (uint64_t s = 0; s < total; s++)
    for (size_t i = 0; i < cells; i++) { occ += data[s * per + i]; known += data[s * per + cells + i]; }
  std::printf("Wrote %s.objects.{data,label,id}.npy and .names.txt: %llu objects of %d x %d x %d cells\n", prefix.c_str(), (unsigned long long)total, vp.dim, vp.dim, vp.dim);
  if (print_stats) {
    std::printf("mesh: %llu vertices, %llu faces, %u object ids; cells: %llu occupied, %llu known; grid: %s; path: %s\n", (unsigned long long)nv, (unsigned long long)nf, nobj,
                (unsigned long long)occ, (unsigned long long)known, grid_path.empty() ? "none" : "yes", device < 0 ? "host" : "device");
    std::printf("seconds: read %.4f, objects %.4f, write %.4f, total %.4f\n", t1 - t0, t2 - t1, now_s() - t2, now_s() - t0);
  }
  return 0;
}
