// tool_alignment.cpp -- drop-in for the `clean` stage's `alignment.exe <scan dir>` (Server/scan_processor.py:132-135; Alignment/main.cpp).
// Same argv: the scan folder, whose last path component names <base>.sens and <base>.ply.  Stdout: "aligning: <dir>" and the reference's
// messages (Alignment/src/alignment.h:158,164,168,190,193-194,255); nothing on stderr on success, a message and a non-zero exit on failure.
// Not the reference's: --force (its forceRealign), --gpu[=device] (the vertex stages on that HIP device, the same bytes), --print-transform.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "scanfuse.h"

int main(int argc, const char** argv) {
  const char* dir = nullptr;
  int force = 0, device = -1, print = 0;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--force") force = 1;
    else if (a == "--print-transform") print = 1;
    else if (a == "--gpu") device = 0;
    else if (a.rfind("--gpu=", 0) == 0) device = std::atoi(a.c_str() + 6);
    else if (a.rfind("--", 0) == 0) { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 255; }
    else if (!dir) dir = argv[i];
    else { std::fprintf(stderr, "one scan folder, please\n"); return 255; }
  }
  if (!dir || device < -1) {
    std::printf("Usage: alignment <scan dir> [--force] [--gpu[=device]] [--print-transform]\n");
    return 255;
  }
  std::printf("aligning: %s\n", dir);
  sf_axis_align_stats st;
  if (sf_axis_align_scan(dir, force, nullptr, device, &st) != SF_OK) {
    std::fprintf(stderr, "alignment: %s\n", sf_last_error());
    return 1;
  }
  switch (st.outcome) {
    case 1: std::printf("no reconstruction available for %s\n\t -> skipping folder\n", dir); return 0;
    case 2: std::printf("reconstruction was invalid for %s\n\t -> skipping folder\n", dir); return 0;
    case 3: std::printf("reconstruction is already aligned %s\n\t -> skipping folder\n", dir); return 0;
    case 4:
      std::printf("already found a previous alignment -> reverting to original\n");
      std::printf("error can't revert due to an invalid transform in the first frame\n\tskipping folder \n");
      return 0;
    default: break;
  }
  if (st.reverted) std::printf("already found a previous alignment -> reverting to original\n");
  if (!st.floor_found) std::printf("could not find a horizontal plane\n");
  if (print)
    for (int r = 0; r < 4; r++) std::printf("%.9g %.9g %.9g %.9g\n", st.transform[4 * r], st.transform[4 * r + 1], st.transform[4 * r + 2], st.transform[4 * r + 3]);
  return 0;
}
