// tool_evaluate.cpp -> bin/evaluate: the benchmark's scores from the benchmark's files, a drop-in for
// BenchmarkScripts/3d_evaluation/evaluate_semantic_label.py, evaluate_semantic_instance.py, 2d_evaluation/evalPixelLevelSemanticLabeling.py
//  and 2d_evaluation/evalInstanceLevelSemanticLabeling.py (section 4p).
//
//   bin/evaluate label3d    --pred_path D --gt_path D [--output_file F] [--host | --device=N]
//   bin/evaluate instance3d --pred_path D --gt_path D [--output_file F] [--min-region=N] [--host | --device=N]
//   bin/evaluate label2d    --pred_path D --gt_path D [--output_file F] [--host | --device=N]
//   bin/evaluate instance2d --pred_path D --gt_path D [--output_file F] [--min-region=N] [--host | --device=N]
//   bin/evaluate export     --scan_path D --label_map_file F --type label|instance|instance-gt --output_file F
//
// The tables go to stdout in the scripts' layout, the result file to --output_file (default: the script's name inside pred_path).  The host path is the
// default (DESIGN.md sections 4o and 4p say why); --device=N runs the counting kernels on that GPU and writes the same bytes.
// Exit status 0, or 2 with one line on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "scanfuse.h"

static int usage() {
  std::fprintf(stderr, "usage: evaluate label3d|instance3d|label2d|instance2d --pred_path D --gt_path D [--output_file F] [--min-region=N] [--host | --device=N]\n"
                       "       evaluate export --scan_path D --label_map_file F --type label|instance|instance-gt --output_file F\n");
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  const std::string mode = argv[1];
  std::string pred, gt, out, scan, label_map, type;
  int device = -1;
  unsigned long min_region = 100;
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    auto value = [&](const char* key, std::string& dst) {   // --key V or --key=V
      const std::string k = key;
      if (a == k && i + 1 < argc) { dst = argv[++i]; return true; }
      if (a.compare(0, k.size() + 1, k + "=") == 0) { dst = a.substr(k.size() + 1); return true; }
      return false;
    };
    std::string v;
    if (value("--pred_path", pred) || value("--gt_path", gt) || value("--output_file", out)) continue;
    if (value("--scan_path", scan) || value("--label_map_file", label_map) || value("--type", type)) continue;
    if (a == "--host") { device = -1; continue; }
    if (value("--device", v)) { device = std::atoi(v.c_str()); continue; }
    if (value("--min-region", v)) { min_region = std::strtoul(v.c_str(), nullptr, 10); continue; }
    return usage();
  }
  if (mode == "export") {
    if (scan.empty() || label_map.empty() || type.empty() || out.empty()) return usage();
    if (sf_eval_export_scan(scan.c_str(), label_map.c_str(), type.c_str(), out.c_str()) != SF_OK) {
      std::fprintf(stderr, "ERROR: %s\n", sf_last_error());
      return 2;
    }
    return 0;
  }
  if (pred.empty() || gt.empty()) return usage();
  char* report = nullptr;
  int rc;
  if (mode == "label3d") rc = sf_eval_label_dir(pred.c_str(), gt.c_str(), out.c_str(), device, &report);
  else if (mode == "instance3d") rc = sf_eval_instance_dir(pred.c_str(), gt.c_str(), out.c_str(), (uint32_t)min_region, device, &report);
  else if (mode == "label2d") rc = sf_eval_pixel_dir(pred.c_str(), gt.c_str(), out.c_str(), device, &report);
  else if (mode == "instance2d") rc = sf_eval_instance2d_dir(pred.c_str(), gt.c_str(), out.c_str(), (uint32_t)min_region, device, &report);
  else return usage();
  if (rc != SF_OK) {
    std::fprintf(stderr, "ERROR: %s\n", sf_last_error());
    return 2;
  }
  std::fputs(report, stdout);
  sf_free(report);
  return 0;
}
