// tool_render.cpp -- drop-in for the `render` stage's `python mts_render.py <mesh.ply>` (Server/scan_processor.py:42-43,159-160; Server/mts_render.py)
// and, with --thumb, the `thumbnail` stage's picture (scan_processor.py:45,163-165; Server/thumbnail.sh).  mts_render.py's command line (:127-171):
//   render <mesh.ply> [-o out.png] [--integrator path|ao] [--samples N] [--width W] [--height H] [--theta deg] [--exposure e] [--world_up v]
//          [--camera_up v] [--camera_offset v] [--bsphere_mult m] [--render_turntable] [--frames_per_degree d] [--cameras file (ignored, as there)]
// v is x | y | z | a,b,c and is normalised (:111-124).  Default output: <mesh without extension>.png (:100-101); turntable frames:
// <mesh file name>_%03d.png for 360 / d views d degrees apart (:84-90; the ffmpeg step :95 is out).  --integrator mlt | vpl are refused.
// Not the reference's: --max-depth N, --host (the host path), --device=N (default 0), --thumb[=WxH] (<out without .png>_thumb.png, 128x128; refused with --render_turntable).
// Nothing on stdout or stderr on success; a message and a non-zero exit on failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scanfuse.h"

static bool vec3(const std::string& s, float v[3]) {
  if (s == "x" || s == "y" || s == "z") { v[0] = s == "x"; v[1] = s == "y"; v[2] = s == "z"; return true; }
  double a, b, c;
  char tail;
  if (std::sscanf(s.c_str(), "%lf,%lf,%lf%c", &a, &b, &c, &tail) != 3) return false;
  const double n = std::sqrt(a * a + b * b + c * c);
  if (!(n > 0) || !std::isfinite(n)) return false;
  v[0] = (float)(a / n); v[1] = (float)(b / n); v[2] = (float)(c / n);
  return true;
}

static int fail(const char* what) {
  std::fprintf(stderr, "render: %s: %s\n", what, sf_last_error());
  return 1;
}

int main(int argc, char** argv) {
  sf_render_params p;
  sf_render_params_default(&p);
  std::string mesh_path, out_path;
  float world_up[3] = {0, 0, 1}, camera_up[3] = {0, 1, 0}, camera_offset[3] = {0, 0, 0}, bsphere_mult = 2.5f, theta = 0.f;
  int turntable = 0, step = 5, device = 0, thumb = 0;
  unsigned thumb_w = 128, thumb_h = 128;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto value = [&](std::string& v) {   // --key value or --key=value
      if (i + 1 >= argc) return false;
      v = argv[++i];
      return true;
    };
    std::string key = a, v;
    bool has = false;
    const size_t eq = a.find('=');
    if (a.rfind("--", 0) == 0 && eq != std::string::npos) { key = a.substr(0, eq); v = a.substr(eq + 1); has = true; }
    auto need = [&]() { return has || value(v); };
    bool ok = true;
    if (key == "-o") ok = need(), out_path = v;
    else if (key == "--cameras") ok = need();
    else if (key == "--integrator") {
      ok = need();
      if (v == "path") p.integrator = SF_RENDER_PATH;
      else if (v == "ao") p.integrator = SF_RENDER_AO;
      else if (v == "mlt" || v == "vpl") { std::fprintf(stderr, "render: the integrator %s is not provided (path and ao are)\n", v.c_str()); return 2; }
      else ok = false;
    }
    else if (key == "--samples") ok = need(), p.samples = std::atoi(v.c_str());
    else if (key == "--width") ok = need(), p.width = std::atoi(v.c_str());
    else if (key == "--height") ok = need(), p.height = std::atoi(v.c_str());
    else if (key == "--max-depth") ok = need(), p.max_depth = std::atoi(v.c_str());
    else if (key == "--frames_per_degree") ok = need(), step = std::atoi(v.c_str());
    else if (key == "--theta") ok = need(), theta = (float)std::atof(v.c_str());
    else if (key == "--exposure") ok = need(), p.exposure = (float)std::atof(v.c_str());
    else if (key == "--bsphere_mult") ok = need(), bsphere_mult = (float)std::atof(v.c_str());
    else if (key == "--world_up") ok = need() && vec3(v, world_up);
    else if (key == "--camera_up") ok = need() && vec3(v, camera_up);
    else if (key == "--camera_offset") ok = need() && vec3(v, camera_offset);
    else if (key == "--render_turntable") turntable = 1;
    else if (key == "--host") device = -1;
    else if (key == "--device") ok = has, device = std::atoi(v.c_str());
    else if (key == "--thumb") { thumb = 1; if (has) ok = std::sscanf(v.c_str(), "%ux%u", &thumb_w, &thumb_h) == 2; }
    else if (a.rfind("-", 0) == 0) { std::fprintf(stderr, "render: unknown option %s\n", argv[i]); return 2; }
    else if (mesh_path.empty()) mesh_path = a;
    else { std::fprintf(stderr, "render: one mesh, please\n"); return 2; }
    if (!ok) { std::fprintf(stderr, "render: bad or missing value for %s\n", key.c_str()); return 2; }
  }
  if (thumb && turntable) { std::fprintf(stderr, "render: --thumb goes with a single view, not with --render_turntable\n"); return 2; }
  if (mesh_path.empty() || (turntable && (step < 1 || step > 360))) {
    std::fprintf(stderr, "usage: render <mesh.ply> [-o out.png] [--integrator path|ao] [--samples N] [--width W] [--height H] [--theta deg] [--exposure e]\n"
                         "       [--world_up v] [--camera_up v] [--camera_offset v] [--bsphere_mult m] [--render_turntable] [--frames_per_degree d]\n"
                         "       [--max-depth N] [--host | --device=N] [--thumb[=WxH]]\n");
    return 2;
  }
  sf_mesh* mesh = nullptr;
  if (sf_ply_read(mesh_path.c_str(), &mesh) != SF_OK) return fail(mesh_path.c_str());
  const int n = turntable ? 360 / step : 1;
  std::vector<sf_camera> cams(n);
  for (int i = 0; i < n; i++)
    if (sf_render_camera(mesh, nullptr, &p, world_up, camera_up, camera_offset, bsphere_mult, turntable ? (float)(i * step) : theta, &cams[i]) != SF_OK) return fail("camera");
  sf_renderer* r = nullptr;
  if (sf_renderer_create(&p, device, &r) != SF_OK) return fail("renderer");
  if (sf_renderer_set_mesh(r, mesh) != SF_OK) return fail("mesh");
  const size_t image = (size_t)p.width * p.height;
  std::vector<float> rgba((size_t)n * image * 4);
  if (sf_renderer_run(r, n, cams.data(), rgba.data(), nullptr) != SF_OK) return fail("run");
  sf_renderer_destroy(r);
  sf_mesh_free(mesh);
  std::vector<uint8_t> px(image * 4);
  if (out_path.empty()) {
    const size_t slash = mesh_path.find_last_of('/'), dot = mesh_path.find_last_of('.');
    out_path = (dot != std::string::npos && (slash == std::string::npos || dot > slash) ? mesh_path.substr(0, dot) : mesh_path) + ".png";
  }
  for (int i = 0; i < n; i++) {
    if (sf_render_film(rgba.data() + (size_t)i * image * 4, image, p.exposure, px.data()) != SF_OK) return fail("film");
    char name[32];
    std::snprintf(name, sizeof(name), "_%03d.png", i);
    const std::string path = turntable ? mesh_path + name : out_path;
    if (sf_png_write(path.c_str(), px.data(), (uint32_t)p.width, (uint32_t)p.height, 4, 8) != SF_OK) return fail(path.c_str());
  }
  if (thumb) {
    std::vector<uint8_t> small((size_t)thumb_w * thumb_h * 4);
    uint32_t w = 0, h = 0;
    if (sf_image_thumbnail(px.data(), (uint32_t)p.width, (uint32_t)p.height, 4, thumb_w, thumb_h, small.data(), &w, &h) != SF_OK) return fail("thumbnail");
    std::string base = out_path;
    if (base.size() >= 4 && base.compare(base.size() - 4, 4, ".png") == 0) base.resize(base.size() - 4);
    const std::string path = base + "_thumb.png";
    if (sf_png_write(path.c_str(), small.data(), w, h, 4, 8) != SF_OK) return fail(path.c_str());
  }
  return 0;
}
