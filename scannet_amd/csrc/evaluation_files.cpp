// evaluation_files.cpp -- the benchmark's scores from the benchmark's files (include/scanfuse.h "Benchmark scores"): what
// bin/evaluate and scannet_amd.evaluation.evaluate_*_dir run.  The files are paired, read and checked here, the counting is sf_eval_confusion,
// sf_eval_confusion_images, sf_eval_instance_overlaps and the AP accumulator (host or device, the same counts), and the tables and result files are
// written in the layout of BenchmarkScripts/3d_evaluation/evaluate_semantic_label.py:85-130, evaluate_semantic_instance.py:312-360 and
// 2d_evaluation/evalPixelLevelSemanticLabeling.py:147-222.
#include <dirent.h>
#include <sys/stat.h>

#include <cerrno>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "common.h"
#include "evaluation_files_internal.h"
#include "evaluation_internal.h"

namespace {

using namespace sf::evf;

struct Prediction {
  std::string mask_file;
  int64_t label;
  double conf;
};

// util_3d.read_instance_prediction_file: lines of `<relative mask path> <label id> <confidence>`; a path listed twice keeps its first place and takes
// the later label and confidence (a dict keyed by the path)
int read_prediction_file(const std::string& file, const std::string& pred_path, std::vector<Prediction>& out) {
  std::ifstream f(file, std::ios::binary);
  if (!f) return sf::fail(SF_ERR_IO, "unable to load %s", file.c_str());
  std::vector<std::string> root;
  normalise(pred_path, root);
  std::string line;
  while (std::getline(f, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::vector<std::string> parts;
    size_t pos = 0;
    while (pos <= line.size()) {
      size_t end = line.find(' ', pos);
      if (end == std::string::npos) end = line.size();
      parts.push_back(line.substr(pos, end - pos));
      pos = end + 1;
    }
    if (parts.size() != 3)
      return sf::fail(SF_ERR_FORMAT, "invalid instance prediction file %s. Expected (per line): [rel path prediction] [label id prediction] [confidence prediction]",
                      file.c_str());
    if (!parts[0].empty() && parts[0][0] == '/')
      return sf::fail(SF_ERR_FORMAT, "invalid instance prediction file %s. First entry in line must be a relative path", file.c_str());
    std::vector<std::string> at;
    normalise(pred_path + "/" + parts[0], at);
    const bool inside = at.size() > root.size() && std::equal(root.begin(), root.end(), at.begin());
    if (!inside)
      return sf::fail(SF_ERR_FORMAT, "predicted mask %s in prediction text file %s points outside of prediction path.", parts[0].c_str(), file.c_str());
    double label = 0.0, conf = 0.0;
    if (!python_float(parts[1], &label) || !python_float(parts[2], &conf) || !std::isfinite(label) || std::isnan(conf) || std::fabs(label) > 9e15)
      return sf::fail(SF_ERR_FORMAT, "invalid instance prediction file %s: label id and confidence must be numbers", file.c_str());
    const std::string mask = join(pred_path, parts[0]);
    Prediction p{mask, (int64_t)label, conf};   // int(float(.)): towards zero
    auto same = std::find_if(out.begin(), out.end(), [&](const Prediction& q) { return q.mask_file == mask; });
    if (same != out.end()) { same->label = p.label; same->conf = p.conf; }
    else out.push_back(p);
  }
  return SF_OK;
}

std::string label_result_file(const uint64_t* conf, const double* iou) {
  std::string s = "iou scores\n";
  for (uint32_t i = 0; i < N_LABEL; i++) s += fmt("%-14s(%-2d): ", LABEL_NAMES[i], LABEL_IDS[i]) + f3(iou[i], 5) + "\n";
  s += "\nconfusion matrix\n\t\t\t";
  for (uint32_t i = 0; i < N_LABEL; i++) s += fmt("%-8d", LABEL_IDS[i]);
  s += "\n";
  for (uint32_t r = 0; r < N_LABEL; r++) {
    s += fmt("%-14s(%-2d)", LABEL_NAMES[r], LABEL_IDS[r]);
    for (uint32_t c = 0; c < N_LABEL; c++) s += "\t" + f3((double)conf[(size_t)LABEL_IDS[r] * DIM + LABEL_IDS[c]], 5);
    s += "\n";
  }
  return s;
}

// evalPixelLevelSemanticLabeling.py:157-173 as it stands: the header row has no line end, and the matrix is indexed by the classes' positions 0 .. 19,
// not by their ids
std::string pixel_result_file(const uint64_t* conf, const double* iou) {
  std::string s = "iou scores\n";
  for (uint32_t i = 0; i < N_LABEL; i++) s += fmt("%-14s(%-2d): ", LABEL_NAMES[i], LABEL_IDS[i]) + f3(iou[i], 5) + "\n";
  s += "\nconfusion matrix\n";
  for (uint32_t i = 0; i < N_LABEL; i++) s += fmt("\t%-14s(%-2d)", LABEL_NAMES[i], LABEL_IDS[i]);
  for (uint32_t r = 0; r < N_LABEL; r++) {
    s += fmt("%-14s(%-2d)", LABEL_NAMES[r], LABEL_IDS[r]);
    for (uint32_t c = 0; c < N_LABEL; c++) s += "\t" + f3((double)conf[(size_t)r * DIM + c], 5);
    s += "\n";
  }
  return s;
}

}  // namespace

SF_API int sf_eval_label_dir(const char* pred_path, const char* gt_path, const char* output_file, int device, char** report) {
  if (report) *report = nullptr;
  if (!pred_path || !gt_path) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const std::string out = output_file && *output_file ? output_file : join(pred_path, "semantic_label_evaluation.txt");
  std::vector<std::string> names;
  if (int rc = pair_files(pred_path, gt_path, ".txt", "semantic_label_evaluation.txt", names)) return rc;
  std::vector<uint64_t> conf((size_t)DIM * DIM, 0);
  std::vector<int64_t> pred, gt;
  std::vector<uint32_t> p32, g32;
  for (const std::string& n : names) {
    if (int rc = load_ids(join(pred_path, n), pred)) return rc;
    if (int rc = load_ids(join(gt_path, n), gt)) return rc;
    if (pred.size() != gt.size()) return sf::fail(SF_ERR_FORMAT, "%s: number of predicted values does not match number of vertices", join(pred_path, n).c_str());
    p32.resize(pred.size());
    g32.resize(gt.size());
    for (size_t i = 0; i < pred.size(); i++) { p32[i] = as_element(pred[i]); g32[i] = as_element(gt[i]); }
    if (int rc = sf_eval_confusion(g32.data(), p32.data(), 4, g32.size(), LABEL_IDS, N_LABEL, SF_EVAL_MODE_3D, device, conf.data(), nullptr)) return rc;
  }
  double iou[N_LABEL];
  uint64_t tp[N_LABEL], denom[N_LABEL];
  if (int rc = sf_eval_iou(conf.data(), DIM, LABEL_IDS, N_LABEL, iou, tp, denom)) return rc;
  std::string text = fmt("evaluating %zu scans...\n", names.size()) + "classes          IoU\n----------------------------\n";
  for (uint32_t i = 0; i < N_LABEL; i++)
    text += fmt("%-14s: ", LABEL_NAMES[i]) + f3(iou[i], 5) + fmt("   (%6llu/%-6llu)\n", (unsigned long long)tp[i], (unsigned long long)denom[i]);
  if (int rc = write_text(out, label_result_file(conf.data(), iou))) return rc;
  text += "wrote results to " + out + "\n";
  return give(report, text);
}

SF_API int sf_eval_instance_dir(const char* pred_path, const char* gt_path, const char* output_file, uint32_t min_region_size, int device, char** report) {
  if (report) *report = nullptr;
  if (!pred_path || !gt_path) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const std::string out = output_file && *output_file ? output_file : join(pred_path, "semantic_instance_evaluation.txt");
  std::vector<std::string> names;
  if (int rc = pair_files(pred_path, gt_path, ".txt", "semantic_instance_evaluation.txt", names)) return rc;
  const int32_t* ids = LABEL_IDS + 2;
  sf_eval_ap* acc = nullptr;
  if (int rc = sf_eval_ap_create(ids, N_INST, min_region_size, &acc)) return rc;
  struct Guard {
    sf_eval_ap* a;
    ~Guard() { sf_eval_ap_destroy(a); }
  } guard{acc};
  std::vector<int64_t> gt, mask;
  for (const std::string& n : names) {
    std::vector<Prediction> preds;
    if (int rc = read_prediction_file(join(pred_path, n), pred_path, preds)) return rc;
    if (int rc = load_ids(join(gt_path, n), gt)) return rc;
    const size_t nv = gt.size(), P = preds.size();
    std::vector<int32_t> gt32(nv), label(P);
    for (size_t v = 0; v < nv; v++) gt32[v] = gt[v] < 0 || gt[v] > 0x7FFFFFFFll ? 0 : (int32_t)gt[v];   // neither an instance nor a valid class: void
    std::vector<double> conf(P);
    std::vector<uint8_t> masks(P * nv, 0);
    for (size_t p = 0; p < P; p++) {
      const int64_t l = preds[p].label;
      label[p] = l < -1 || l > 0x7FFFFFFFll ? -1 : (int32_t)l;
      conf[p] = preds[p].conf;
      if (!std::binary_search(ids, ids + N_INST, label[p])) continue;   // dropped for its label before its mask is read, as the reference does
      if (int rc = load_ids(preds[p].mask_file, mask)) return rc;
      if (mask.size() != nv)
        return sf::fail(SF_ERR_FORMAT, "wrong number of lines in %s(%zu) vs #mesh vertices (%zu), please double check and/or re-download the mesh",
                        preds[p].mask_file.c_str(), mask.size(), nv);
      for (size_t v = 0; v < nv; v++) masks[p * nv + v] = mask[v] != 0;
    }
    uint32_t G = 0;
    std::vector<uint32_t> slot(nv), verts(nv);   // at most one instance per vertex
    std::vector<int32_t> iid(nv);
    if (int rc = sf_eval_instance_plan(gt32.data(), nv, ids, N_INST, iid.data(), verts.data(), (uint32_t)nv, slot.data(), &G)) return rc;
    std::vector<uint32_t> table(P * ((size_t)G + 2));
    if (int rc = sf_eval_instance_overlaps(slot.data(), nv, G, masks.data(), (uint32_t)P, nv, device, table.data())) return rc;
    if (int rc = sf_eval_ap_add_scan(acc, G, iid.data(), verts.data(), (uint32_t)P, label.data(), conf.data(), table.data())) return rc;
  }
  std::vector<double> ap((size_t)N_INST * SF_EVAL_AP_OVERLAPS), cls((size_t)N_INST * 3);
  double avg[3];
  if (int rc = sf_eval_ap_finish(acc, ap.data(), cls.data(), avg)) return rc;
  const std::string bar(64, '#'), dash(64, '-');
  std::string text = fmt("evaluating %zu scans...\n", names.size()) + "\n" + bar + "\n" + fmt("%-15s:%15s%15s%15s\n", "what", "AP", "AP_50%", "AP_25%") + bar + "\n";
  std::string file = "class,class id,ap,ap50,ap25\n";
  for (uint32_t i = 0; i < N_INST; i++) {
    const char* name = LABEL_NAMES[i + 2];
    text += fmt("%-15s:", name) + f3(cls[3 * i], 15) + f3(cls[3 * i + 1], 15) + f3(cls[3 * i + 2], 15) + "\n";
    file += std::string(name) + "," + fmt("%d", ids[i]) + "," + g17(cls[3 * i]) + "," + g17(cls[3 * i + 1]) + "," + g17(cls[3 * i + 2]) + "\n";
  }
  text += dash + "\n" + fmt("%-15s:", "average") + f3(avg[0], 15) + f3(avg[1], 15) + f3(avg[2], 15) + "\n\n";
  if (int rc = write_text(out, file)) return rc;
  return give(report, text);
}

SF_API int sf_eval_pixel_dir(const char* pred_path, const char* gt_path, const char* output_file, int device, char** report) {
  if (report) *report = nullptr;
  if (!pred_path || !gt_path) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const std::string out = output_file && *output_file ? output_file : join(pred_path, "semantic_label.txt");
  std::vector<std::string> names;
  if (int rc = pair_files(pred_path, gt_path, nullptr, base_name(out), names)) return rc;
  std::vector<uint64_t> conf((size_t)DIM * DIM, 0);
  struct Image {
    uint32_t w = 0, h = 0;
    std::vector<uint16_t> px;
  };
  auto read = [](const std::string& path, Image& im, bool prediction) -> int {
    int channels = 0, bits = 0;
    void* data = nullptr;
    if (int rc = sf_png_read(path.c_str(), &im.w, &im.h, &channels, &bits, &data)) return sf::fail(rc, "Unable to load %s: %s", path.c_str(), sf::last_error_ref().c_str());
    int rc = SF_OK;
    if (channels != 1) rc = sf::fail(SF_ERR_FORMAT, prediction ? "Predicted image has multiple channels. (%s)" : "%s has multiple channels", path.c_str());
    else if (bits != 8 && bits != 16) rc = sf::fail(SF_ERR_FORMAT, "%s: %d bits per sample", path.c_str(), bits);
    else {
      im.px.resize((size_t)im.w * im.h);
      for (size_t i = 0; i < im.px.size(); i++) im.px[i] = bits == 8 ? ((const uint8_t*)data)[i] : ((const uint16_t*)data)[i];
    }
    sf_free(data);
    return rc;
  };
  for (const std::string& n : names) {
    Image p, g;
    if (int rc = read(join(pred_path, n), p, true)) return rc;
    if (int rc = read(join(gt_path, n), g, false)) return rc;
    if (!(p.w == g.w || (p.w == SF_EVAL_IMAGE_WIDTH && p.h == SF_EVAL_IMAGE_HEIGHT))) return sf::fail(SF_ERR_FORMAT, "Invalid image size for %s", join(pred_path, n).c_str());
    uint64_t oor = 0;
    std::vector<uint64_t> one((size_t)DIM * DIM, 0);
    if (int rc = sf_eval_confusion_images(g.px.data(), p.px.data(), 2, 1, g.w, g.h, p.w, p.h, DIM, device, one.data(), &oor)) return rc;
    if (oor) return sf::fail(SF_ERR_FORMAT, "%s: %llu pixels carry an id of %u or more in the prediction or the ground truth", join(pred_path, n).c_str(), (unsigned long long)oor, DIM);
    for (size_t i = 0; i < one.size(); i++) conf[i] += one[i];
  }
  double iou[N_LABEL];
  if (int rc = sf_eval_iou(conf.data(), DIM, LABEL_IDS, N_LABEL, iou, nullptr, nullptr)) return rc;
  std::string text = fmt("Evaluating %zu pairs of images...\n", names.size()) + "classes          IoU\n----------------------------\n";
  double sum = 0.0;
  uint32_t live = 0;
  for (uint32_t i = 0; i < N_LABEL; i++) {
    text += fmt("%-14s: ", LABEL_NAMES[i]) + f3(iou[i], 5) + "\n";
    if (!std::isnan(iou[i])) { sum += iou[i]; live++; }
  }
  const std::string dash(32, '-');
  text += dash + "\nScore Average : " + f3(live ? sum / live : NAN, 5) + "\n" + dash + "\n\n";
  if (int rc = write_text(out, pixel_result_file(conf.data(), iou))) return rc;
  text += "wrote results to " + out + "\n";
  return give(report, text);
}

// export_train_mesh_for_evaluation.py: the ground truth of a scan in the evaluation format.  type "label": one nyu40id per vertex; "instance": a
// prediction file beside its masks, as util_3d.export_instance_ids_for_eval names and writes them; "instance-gt": label * 1000 + objectId + 1 per vertex.
SF_API int sf_eval_export_scan(const char* scan_path, const char* label_map_file, const char* type, const char* output_file) {
  if (!scan_path || !label_map_file || !type || !output_file) return sf::fail(SF_ERR_INVALID_ARG, "NULL argument");
  const std::string kind = type, out = output_file;
  if (kind != "label" && kind != "instance" && kind != "instance-gt") return sf::fail(SF_ERR_INVALID_ARG, "export: type %s (label, instance or instance-gt)", type);
  std::string dir = scan_path;
  while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
  const std::string scan = base_name(dir);
  const std::string agg = join(dir, scan + ".aggregation.json"), segs = join(dir, scan + "_vh_clean_2.0.010000.segs.json");
  uint64_t nv = 0;
  if (int rc = sf_eval_export_ids(segs.c_str(), agg.c_str(), label_map_file, 0, nullptr, nullptr, &nv)) return rc;
  std::vector<uint32_t> label(nv), inst(nv);
  if (int rc = sf_eval_export_ids(segs.c_str(), agg.c_str(), label_map_file, nv, label.data(), inst.data(), &nv)) return rc;
  std::string text;
  if (kind == "label" || kind == "instance-gt") {
    for (uint64_t v = 0; v < nv; v++) text += fmt("%llu\n", (unsigned long long)(kind == "label" ? label[v] : (inst[v] ? (uint64_t)label[v] * 1000u + inst[v] : 0u)));
    return write_text(out, text);
  }
  // util_3d.py:57-77: the masks are numbered by the position of the instance among the sorted distinct ids, the id 0 included where it occurs
  const size_t slash = out.find_last_of('/');
  const std::string out_dir = slash == std::string::npos ? "" : out.substr(0, slash);
  std::string name = base_name(out);
  const size_t dot = name.find_last_of('.');
  if (dot != std::string::npos && dot > 0) name = name.substr(0, dot);
  const std::string mask_dir = join(out_dir, "pred_mask");
  if (mkdir(mask_dir.c_str(), 0777) != 0 && !(errno == EEXIST)) return sf::fail(SF_ERR_IO, "cannot create %s", mask_dir.c_str());
  std::vector<uint32_t> uniq(inst);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  for (size_t idx = 0; idx < uniq.size(); idx++) {
    if (uniq[idx] == 0) continue;
    const std::string rel = "pred_mask/" + name + "_" + std::to_string(idx) + ".txt";
    std::string mask;
    uint32_t first_label = 0;
    bool seen = false;
    for (uint64_t v = 0; v < nv; v++) {
      const bool in = inst[v] == uniq[idx];
      if (in && !seen) { first_label = label[v]; seen = true; }
      mask += in ? "1\n" : "0\n";
    }
    text += rel + fmt(" %u %f\n", first_label, 1.0);
    if (int rc = write_text(join(out_dir, rel), mask)) return rc;
  }
  return write_text(out, text);
}
