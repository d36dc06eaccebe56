// tool_calibrate_depth.cpp -- drop-in for the two batch modes of CameraParameterEstimation/apps/calibrate_depth (calibrate_depth.cpp:1149-1200):
//   calibrate_depth <configuration> [-e out.lut] [-a in.lut] [-d max_depth] [-s n_slices] [-b 0|1] [-v] [-l] [--root=dir] [--host] [--device=N]
// -e estimates the depth-distortion table from the configuration's plane sequence (depth_raw/<name>), -a applies a table to
// depth_raw/<name minus 4 characters>.png and writes depth/<the same>.png; with both, the estimate runs first, as in the reference's main.
// The long options of the reference (--estimate_undistortion, --apply_undistortion, --max_depth, --n_slices, --bitshift, --verbose,
// --slice_visualization) are accepted too.  Not the reference's: --root=dir (the directory that holds depth_raw/, depth/ and the files the
// configuration names; default: the current directory, as there), --host (the host path, the default), --device=N (HIP device N: the same bytes).
// Without -e or -a the reference opens its OpenGL viewer, which is not provided: the usage is printed and the exit status is 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "scanfuse.h"

static int usage() {
  std::fprintf(stderr, "usage: calibrate_depth <configuration> [-e out.lut] [-a in.lut] [-d max_depth] [-s n_slices] [-b 0|1] [-v] [-l] [--root=dir] [--host] [--device=N]\n"
                       "  -e / -a: at least one is needed (the viewer of the original program is not provided)\n");
  return 2;
}

int main(int argc, char** argv) {
  sf_calibrate_depth_options o;
  sf_calibrate_depth_options_default(&o);
  std::string config, estimate, apply, root;
  int device = -1;   // README.md: PNG decoding dominates the tool's time, the device does not beat the host path end to end
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto value = [&](std::string& v) {
      if (i + 1 >= argc) return false;
      v = argv[++i];
      return true;
    };
    std::string v;
    char* end = nullptr;
    if (a == "-e" || a == "--estimate_undistortion") { if (!value(estimate)) return usage(); }
    else if (a == "-a" || a == "--apply_undistortion") { if (!value(apply)) return usage(); }
    else if (a == "-d" || a == "--max_depth") { if (!value(v)) return usage(); o.max_depth = std::strtof(v.c_str(), &end); if (*end) return usage(); }
    else if (a == "-s" || a == "--n_slices") { if (!value(v)) return usage(); o.n_slices = (int)std::strtof(v.c_str(), &end); if (*end) return usage(); }
    else if (a == "-b" || a == "--bitshift") { if (!value(v)) return usage(); o.bitshift = (v == "1" || v == "true") ? 1 : 0; if (v != "0" && v != "1" && v != "true" && v != "false") return usage(); }
    else if (a == "-v" || a == "--verbose") o.verbose = 1;
    else if (a == "-l" || a == "--slice_visualization") o.save_slices = 1;
    else if (a.rfind("--root=", 0) == 0) root = a.substr(7);
    else if (a == "--host") device = -1;
    else if (a.rfind("--device=", 0) == 0) { device = (int)std::strtol(a.c_str() + 9, &end, 10); if (*end || device < 0) return usage(); }
    else if (!a.empty() && a[0] == '-') return usage();
    else if (config.empty()) config = a;
    else return usage();
  }
  if (config.empty() || (estimate.empty() && apply.empty())) return usage();
  if (!root.empty()) o.root = root.c_str();
  sf_calibrate_depth_stats st;
  const int rc = sf_calibrate_depth(config.c_str(), estimate.empty() ? nullptr : estimate.c_str(), apply.empty() ? nullptr : apply.c_str(), &o, device, 0, &st);
  if (rc != SF_OK) {
    std::fprintf(stderr, "calibrate_depth: %s\n", sf_last_error());
    return 1;
  }
  if (o.verbose)
    std::printf("%llu images: %llu used, %llu skipped, %llu corrected; read %.3f s, estimate %.3f s, apply %.3f s, write %.3f s, total %.3f s on %s\n",
                (unsigned long long)st.images, (unsigned long long)st.images_used, (unsigned long long)st.images_skipped, (unsigned long long)st.images_applied,
                st.seconds_read, st.seconds_estimate, st.seconds_apply, st.seconds_write, st.seconds_total, device < 0 ? "the host path" : "the device");
  return 0;
}
