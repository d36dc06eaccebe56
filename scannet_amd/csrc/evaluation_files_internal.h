// evaluation_files_internal.h -- what the file modes of the benchmark's scores share (evaluation_files.cpp: DESIGN.md section 4o; instance2d_files.cpp:
// section 4p): the class names and ids, the formats of the tables, directory listing, the one-integer-per-line reader, os.path.normpath by components
// and Python's float().
#pragma once
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "common.h"

namespace sf {
namespace evf {

const char* const LABEL_NAMES[20] = {"wall",   "floor",    "cabinet", "bed",  "chair",   "sofa",         "table",          "door",   "window", "bookshelf",
                                     "picture", "counter", "desk",    "curtain", "refrigerator", "shower curtain", "toilet", "sink",   "bathtub", "otherfurniture"};
const int32_t LABEL_IDS[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39};
constexpr uint32_t DIM = 41, N_LABEL = 20, N_INST = 18;   // the instance classes are the label classes without wall and floor

inline std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

// "%w.3f" as Python prints it: nan without a sign
inline std::string f3(double v, int width) { return std::isnan(v) ? fmt("%*s", width, "nan") : fmt("%*.3f", width, v); }

inline std::string join(const std::string& dir, const std::string& name) { return dir.empty() || dir.back() == '/' ? dir + name : dir + "/" + name; }

inline bool is_file(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

inline int list_dir(const std::string& dir, std::vector<std::string>& names) {
  DIR* d = opendir(dir.c_str());
  if (!d) return sf::fail(SF_ERR_IO, "cannot list %s", dir.c_str());
  while (struct dirent* e = readdir(d)) {
    const std::string n = e->d_name;
    if (n != "." && n != "..") names.push_back(n);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  return SF_OK;
}

inline bool ends_with(const std::string& s, const char* tail) {
  const size_t n = std::strlen(tail);
  return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

// one integer per line (util_3d.load_ids: splitlines, then int64); spaces around the number are allowed, anything else is SF_ERR_FORMAT
inline int load_ids(const std::string& path, std::vector<int64_t>& out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return sf::fail(SF_ERR_IO, "unable to load %s", path.c_str());
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string text = ss.str();
  out.clear();
  size_t pos = 0, line = 0;
  while (pos < text.size()) {
    size_t end = text.find('\n', pos);
    if (end == std::string::npos) end = text.size();
    size_t a = pos, b = end;
    line++;
    while (a < b && (text[a] == ' ' || text[a] == '\t')) a++;
    while (b > a && (text[b - 1] == ' ' || text[b - 1] == '\t' || text[b - 1] == '\r')) b--;
    size_t d = a;
    if (d < b && (text[d] == '-' || text[d] == '+')) d++;
    if (d == b || b - d > 18) return sf::fail(SF_ERR_FORMAT, "unable to load %s: line %zu is no integer", path.c_str(), line);
    int64_t v = 0;
    for (size_t i = d; i < b; i++) {
      if (text[i] < '0' || text[i] > '9') return sf::fail(SF_ERR_FORMAT, "unable to load %s: line %zu is no integer", path.c_str(), line);
      v = v * 10 + (text[i] - '0');
    }
    out.push_back(text[a] == '-' ? -v : v);
    pos = end + 1;
  }
  return SF_OK;
}

// the files of pred_path that take part (`suffix` NULL: all regular files), without the result file; each needs a file of its name in gt_path
inline int pair_files(const std::string& pred_path, const std::string& gt_path, const char* suffix, const std::string& result_name, std::vector<std::string>& names) {
  std::vector<std::string> all;
  if (int rc = list_dir(pred_path, all)) return rc;
  for (const std::string& n : all)
    if (n != result_name && (suffix ? ends_with(n, suffix) : is_file(join(pred_path, n)))) names.push_back(n);
  if (names.empty()) return sf::fail(SF_ERR_IO, "No result files found.");
  for (const std::string& n : names)
    if (!is_file(join(gt_path, n))) return sf::fail(SF_ERR_IO, "Result file %s does not match any gt file", n.c_str());
  return SF_OK;
}

inline std::string base_name(const std::string& p) {
  const size_t s = p.find_last_of('/');
  return s == std::string::npos ? p : p.substr(s + 1);
}

inline int write_text(const std::string& path, const std::string& text) {
  std::ofstream f(path, std::ios::binary);
  if (!f || !(f << text) || !f.flush()) return sf::fail(SF_ERR_IO, "cannot write %s", path.c_str());
  return SF_OK;
}

inline int give(char** report, const std::string& text) {
  if (!report) return SF_OK;
  *report = (char*)std::malloc(text.size() + 1);
  if (!*report) return sf::fail(SF_ERR_IO, "out of memory");
  std::memcpy(*report, text.c_str(), text.size() + 1);
  return SF_OK;
}

// what a text id becomes as a 4-byte element: a value that does not fit is no class
inline uint32_t as_element(int64_t v) { return v < 0 || v > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v; }

// os.path.normpath, component by component: "." and empty components go, ".." takes back the component before it (or stays, at the front)
inline void normalise(const std::string& path, std::vector<std::string>& parts) {
  size_t pos = 0;
  while (pos <= path.size()) {
    size_t end = path.find('/', pos);
    if (end == std::string::npos) end = path.size();
    const std::string c = path.substr(pos, end - pos);
    if (c == "..") {
      if (!parts.empty() && parts.back() != "..") parts.pop_back();
      else parts.push_back(c);
    } else if (!c.empty() && c != ".") {
      parts.push_back(c);
    }
    pos = end + 1;
  }
}

// A number as Python's float() reads it: decimal digits with an optional point and exponent, or inf / infinity / nan, a sign, blanks around it.
// strtod alone would also take hexadecimal floats and nan(...), which float() refuses; digit-group underscores, which float() takes, are refused here.
inline bool python_float(const std::string& text, double* out) {
  size_t a = 0, b = text.size();
  while (a < b && std::strchr(" \t\r\n\f\v", text[a])) a++;
  while (b > a && std::strchr(" \t\r\n\f\v", text[b - 1])) b--;
  const std::string t = text.substr(a, b - a);
  if (t.empty() || t.find_first_of("xXpP(_") != std::string::npos) return false;
  char* end = nullptr;
  *out = std::strtod(t.c_str(), &end);
  return *end == 0;
}

inline std::string g17(double v) { return std::isnan(v) ? "nan" : fmt("%.17g", v); }

}  // namespace evf
}  // namespace sf
