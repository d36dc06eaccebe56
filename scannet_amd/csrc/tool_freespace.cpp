// tool_freespace.cpp -- bin/freespace: the `freespace` stage's executable (Server/scan_processor.py:15; FreeSpace.exe <scan>.sens, Server/config.py:20;
// product ${id}.grid, Server/config/scan_stages.json:43-47).  The binary this replaces is not in the reference tree; the grid and its file are this
// library's statement (include/scanfuse.h "Free-space grids").
//
//   freespace <scan>.sens [-o out.grid] [--voxel=m] [--params=file] [--every=N] [--max-blocks=N] [--device=N] [--print-stats]
//
// Without -o the grid goes beside the scan, ".grid" in place of ".sens": the stage table's output check holds with the reference's one-argument call.
// stderr stays empty on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "scanfuse.h"

static int usage() {
  std::fprintf(stderr, "usage: freespace <scan>.sens [-o out.grid] [--voxel=m] [--params=file] [--every=N] [--max-blocks=N] [--device=N] [--print-stats]\n");
  return 2;
}

static int die(const char* what, int rc) {
  std::fprintf(stderr, "freespace: %s: %s (%d)\n", what, sf_last_error(), rc);
  return 1;
}

int main(int argc, char** argv) {
  sf_freespace_params fp;
  sf_freespace_params_default(&fp);
  std::string in, out;
  int device = std::getenv("SF_DEVICE") ? std::atoi(std::getenv("SF_DEVICE")) : 0;
  bool print_stats = false;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "-o") {
      if (++i >= argc) return usage();
      out = argv[i];
    } else if (a.rfind("--voxel=", 0) == 0) {
      fp.voxel_size = (float)std::atof(a.c_str() + 8);
    } else if (a.rfind("--params=", 0) == 0) {
      if (a.size() - 9 >= sizeof(fp.params_file)) return usage();
      std::strcpy(fp.params_file, a.c_str() + 9);
    } else if (a.rfind("--every=", 0) == 0) {
      fp.every = std::atoi(a.c_str() + 8);
    } else if (a.rfind("--max-blocks=", 0) == 0) {
      fp.max_blocks = (uint32_t)std::strtoul(a.c_str() + 13, nullptr, 10);
    } else if (a.rfind("--device=", 0) == 0) {
      device = std::atoi(a.c_str() + 9);
    } else if (a == "--print-stats") {
      print_stats = true;
    } else if (!a.empty() && a[0] == '-') {
      return usage();
    } else if (in.empty()) {
      in = a;
    } else {
      return usage();
    }
  }
  if (in.empty()) return usage();
  if (out.empty()) {
    const size_t n = in.size();
    out = (n >= 5 && in.compare(n - 5, 5, ".sens") == 0 ? in.substr(0, n - 5) : in) + ".grid";
  }
  sf_sens* sens = nullptr;
  int rc = sf_sens_open(in.c_str(), &sens);
  if (rc != SF_OK) return die(in.c_str(), rc);
  sf_grid* grid = nullptr;
  sf_freespace_stats st;
  rc = sf_freespace_sens(sens, &fp, device, 0, &grid, &st);
  sf_sens_close(sens);
  if (rc != SF_OK) return die("freespace", rc);
  rc = sf_grid_save(grid, out.c_str());
  sf_grid_header h;
  sf_grid_info(grid, &h);
  sf_grid_free(grid);
  if (rc != SF_OK) return die(out.c_str(), rc);
  std::printf("Wrote %s: %d x %d x %d voxels of %g m from %llu frames\n", out.c_str(), h.nx, h.ny, h.nz, (double)h.voxel_size, (unsigned long long)h.frames_used);
  if (print_stats) {
    std::printf("box: blocks [%d %d %d] .. [%d %d %d] = %llu blocks\n", st.lo_block[0], st.lo_block[1], st.lo_block[2], st.hi_block[0], st.hi_block[1], st.hi_block[2],
                (unsigned long long)st.box_blocks);
    std::printf("voxels: %llu known, %llu free, %llu near\n", (unsigned long long)st.known, (unsigned long long)st.free_voxels, (unsigned long long)st.near_voxels);
    std::printf("seconds: plan %.4f, create %.4f, allocate %.4f, fuse %.4f, bounds %.4f, export %.4f, total %.4f\n", st.seconds_plan, st.seconds_create,
                st.seconds_allocate, st.seconds_fuse, st.seconds_bounds, st.seconds_export, st.seconds_total);
  }
  return 0;
}
