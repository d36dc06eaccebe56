"""The mesh render without a GPU: the host path (device = -1) against the brute-force checker tests/render_checker.c on the float bits
of every pixel; the tree against the checker's closest hit on rays built from its own boxes; known answers of the floor, the sampler, the camera,
the film and the thumbnail; refusals, struct layouts, bin/render --host, and the host sources once under sanitizers as a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, render
from scannet_amd.segmentator import Mesh
from tests import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "render")
needs_checker = pytest.mark.skipif(not rc.have_checker(), reason="needs gcc and a CPU with fused multiply-add")


# ---- host path == checker ---------------------------------------------------------------------------------------------------------------------------
@needs_checker
@pytest.mark.parametrize("name", ["floor", "lattice", "room", "ao", "inside"])
def test_host_path_matches_the_checker_bit_for_bit(name):
    ref, got = rc.checker_images(name), rc.product_images(name, -1)
    assert got.shape == ref.shape
    assert np.array_equal(rc.bits(got), rc.bits(ref)), "%d of %d floats differ" % ((rc.bits(got) != rc.bits(ref)).sum(), ref.size)
    if name == "inside":
        assert np.all(ref[..., :3] == 0) and np.all(ref[..., 3] == 1)
    else:
        assert 0 < ref[..., 3].mean() < 1 and ref[..., :3].std() > 0.01      # the mesh and the sky are both in the picture


@needs_checker
def test_lattice_centre_ray_is_axis_parallel_and_ties_go_to_the_lowest_index():
    c = rc.case("lattice")
    cam = c["cameras"][0]
    assert list(cam.forward) == [0.0, 0.0, -1.0] and cam.origin[0] == 3.0 and cam.origin[1] == 3.0
    rays = np.array([[3, 3, cam.origin[2], 0, 0, -1], [2.5, 3, 5, 0, 0, -1], [3, 1.25, 5, 0, 0, -1]], np.float32)   # a vertex, and two shared edges
    ref = rc.checker_rays(c, rays)
    with render.Renderer(c["p"], -1) as r:
        r.set_mesh(c["mesh"])
        got = r.rays(rays)
    assert rc.same_hits(got, ref)
    t = c["tris"]
    for k in range(3):   # the winner is the FIRST triangle of the list that holds the point
        holders = [i for i in range(len(t)) if rc.checker_rays(dict(c, tris=np.ascontiguousarray(t[i:i + 1])), rays[k:k + 1])[0][0] == 0]
        assert len(holders) >= 2 and got[0][k] == holders[0], (k, holders, got[0][k])


@needs_checker
def test_the_tree_never_changes_the_answer():
    c = rc.case("room")
    with render.Renderer(c["p"], -1) as r:
        r.set_mesh(c["mesh"])
        boxes, links = r.nodes()
        assert len(boxes) > 1000 and np.all(links[:, 0] > np.arange(len(links))) and links[-1, 0] == len(links)
        rays = np.concatenate([rc.box_rays(boxes), rc.hashed_rays(c)])
        got = r.rays(rays)
    ref = rc.checker_rays(c, rays)
    assert (ref[0] != rc.NONE).sum() > len(rays) // 4 and (ref[0] == rc.NONE).sum() > 100
    bad = np.flatnonzero((got[0] != ref[0]) | (rc.bits(got[1]) != rc.bits(ref[1])).any(1))
    assert len(bad) == 0, (len(bad), rays[bad[:3]], got[0][bad[:3]], ref[0][bad[:3]])


@needs_checker
def test_two_leaf_sizes_give_the_same_image_bits():
    ref = rc.checker_images("room")
    try:
        sizes = []
        for leaf in (1, 15):
            render.tune("leaf", leaf)
            c = rc.case("room")
            with render.Renderer(c["p"], -1) as r:
                r.set_mesh(c["mesh"])
                sizes.append(len(r.nodes()[0]))
                assert np.array_equal(rc.bits(r.run(c["cameras"])), rc.bits(ref)), leaf
        assert sizes[0] > 4 * sizes[1]
    finally:
        render.tune("leaf", 4)


# ---- known answers ----------------------------------------------------------------------------------------------------------------------------------
def _uniform(pixel, sample, dim):
    with np.errstate(over="ignore"):
        h = rc._mix(pixel.astype(np.uint32) + np.uint32(0x9e3779b9))
        h = rc._mix(h + np.uint32(sample))
        h = rc._mix(h + np.uint32(dim << 4))
    return (h >> np.uint32(8)).astype(np.float64) / 2.0 ** 24


def test_floor_pixels_are_the_interpolated_reflectance():
    """Every bounce off the floor leaves the scene, so a sample's radiance is the reflectance under it.  The reference is float64 geometry on the
    camera's floats and the hash's sub-pixel positions; the bound (S + 4) 2^-24 relative is what the rule's roundings allow."""
    c = rc.case("floor")
    p, cam = c["p"], c["cameras"][0]
    W, H, S = p.width, p.height, p.samples
    got = rc.product_images("floor", -1)[0].astype(np.float64)
    y, x = np.mgrid[0:H, 0:W]
    pixel = (y * W + x).astype(np.uint32)
    o, right, up, fwd = (np.array(list(v), np.float64) for v in (cam.origin, cam.right, cam.up, cam.forward))
    col = c["rgba"][:, :3].astype(np.float64) / 255
    total = np.zeros((H, W, 4))
    for s in range(S):
        px, py = x + _uniform(pixel, s, 0), y + _uniform(pixel, s, 1)
        sx = (2 * px / W - 1) * float(cam.tan_half_fov)
        sy = (1 - 2 * py / H) * float(cam.tan_half_fov) / float(cam.aspect)
        w = fwd + sx[..., None] * right + sy[..., None] * up
        P = o + (-o[2] / w[..., 2])[..., None] * w
        fx, fy = P[..., 0] / 2.0, P[..., 1] / 1.5
        hit = (fx >= 0) & (fx <= 1) & (fy >= 0) & (fy <= 1)
        lower = fy <= fx                                        # triangle (0, 1, 2), else (0, 2, 3)
        u, v = np.where(lower, fx - fy, fx), np.where(lower, fy, fy - fx)
        c1, c2 = np.where(lower[..., None], col[1], col[2]), np.where(lower[..., None], col[2], col[3])
        refl = (1 - u - v)[..., None] * col[0] + u[..., None] * c1 + v[..., None] * c2
        total[..., :3] += np.where(hit[..., None], refl, 1.0)
        total[..., 3] += hit
    ref = total / S
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)
    print("floor: worst relative error %.3g, bound %.3g" % (err.max(), (S + 4) * 2.0 ** -24))
    assert 0.2 < ref[..., 3].mean() < 0.9
    assert err.max() <= (S + 4) * 2.0 ** -24


def test_sampler_is_cosine_weighted():
    n = np.array([0.36, -0.48, 0.8], np.float32)
    d = np.array([render.sample_direction(n, pix, 0, 1) for pix in range(65536)], np.float64)
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-6)
    cos = d @ n.astype(np.float64)
    assert cos.min() >= -1e-6
    assert abs(cos.mean() - 2 / 3) < 0.005, cos.mean()          # the standard error is 0.0009; a uniform hemisphere gives 1/2
    assert np.abs(d.mean(0) - n.astype(np.float64) * 2 / 3).max() < 0.01


@needs_checker
def test_sampler_matches_the_checker():
    L = rc.checker()
    n = np.array([0.0, 0.6, 0.8], np.float32)
    for pix, s, b in [(0, 0, 1), (5, 3, 2), (123456, 15, 16), (2 ** 26 - 1, 4095, 7)]:
        ref = np.zeros(3, np.float32)
        L.rk_sample(rc._p(n), pix, s, b, rc._p(ref))
        assert np.array_equal(rc.bits(render.sample_direction(n, pix, s, b)), rc.bits(ref))


def _camera64(lo, hi, W, H, fov, world_up, camera_up, offset, mult, theta):
    lo, hi, wu, cu, off = (np.asarray(v, np.float64) for v in (lo, hi, world_up, camera_up, offset))
    centre = (lo + hi) / 2
    radius = np.linalg.norm(hi - centre)
    along = off + wu
    arm = mult * radius * along / np.linalg.norm(along)
    R = rc.ac.rotation(wu, np.deg2rad(theta))
    arm, cu = R @ arm, R @ cu
    fwd = -arm / np.linalg.norm(arm)
    right = np.cross(fwd, cu)
    right /= np.linalg.norm(right)
    return np.concatenate([centre + arm, right, np.cross(right, fwd), fwd, [np.tan(np.deg2rad(fov) / 2), W / H]])


@pytest.mark.parametrize("theta,world_up,offset", [(0.0, (0, 0, 1), (0, 0, 0)), (90.0, (0, 0, 1), (0, 0, 0)), (40.0, (0.3, -0.2, 0.9), (1, 0, 0))])
def test_camera_agrees_with_a_float64_statement(theta, world_up, offset):
    box = np.array([-1.5, 0.25, 0.0, 4.5, 3.75, 2.5], np.float32)
    p = render.default_params()
    cam = render.camera(box, p, world_up=world_up, camera_up=(0, 1, 0), camera_offset=offset, bsphere_mult=2.5, theta=theta)
    ref = _camera64(box[:3], box[3:], 640, 480, 45.0, world_up, (0, 1, 0), offset, 2.5, theta)
    assert np.abs(rc.camera_floats(cam).astype(np.float64) - ref).max() < 1e-6
    if theta == 0.0 and world_up == (0, 0, 1):   # the default view looks straight down with +x to the right and +y up in the picture
        assert list(cam.forward) == [0, 0, -1] and list(cam.right) == [1, 0, 0] and list(cam.up) == [0, 1, 0]


def test_film_known_values():
    knee = 0.0031308
    rgba = np.array([[0, 0.5, 1, 0], [knee / 2, knee, 0.25, 1], [0.1, 2.0, -1.0, 0.5], [np.nan, 0.5, 0.5, 2.0]], np.float32)
    out = render.film(rgba, exposure=0.0)
    srgb = lambda v: int(255 * min(max(12.92 * v if v <= knee else 1.055 * v ** (1 / 2.4) - 0.055, 0), 1) + 0.5)
    assert out[0].tolist() == [0, 188, 255, 0] and srgb(0.5) == 188
    assert out[1].tolist() == [srgb(float(np.float32(knee / 2))), srgb(float(np.float32(knee))), 137, 255] and out[1][0] == 5 and out[1][1] == 10
    assert out[2].tolist() == [srgb(float(np.float32(0.1))), 255, 0, 128]
    assert out[3].tolist() == [0, 188, 188, 255]
    assert render.film(np.array([[0.25, 0.5, 1.0, 1.0]], np.float32), exposure=1.0)[0].tolist() == [188, 255, 255, 255]   # the default exposure doubles


def test_thumbnail_of_a_ramp():
    x = np.arange(640, dtype=np.uint32)
    img = np.zeros((480, 640, 4), np.uint8)
    img[..., 0] = (x * 255 // 639)[None, :]
    img[..., 1] = (np.arange(480) * 255 // 479)[:, None]
    img[..., 2] = 77
    img[..., 3] = 255
    t = render.thumbnail(img)
    assert t.shape == (96, 128, 4)
    assert np.all(t[..., 2] == 77) and np.all(t[..., 3] == 255)
    ref_r = (img[0, :, 0].astype(np.uint64).reshape(128, 5).sum(1) * 5 * 640 * 480 // 25 + 640 * 480 // 2) // (640 * 480)   # five columns, equal weights
    assert np.array_equal(t[17, :, 0], ref_r.astype(np.uint8)) and t[0, 0, 0] == 0 and t[0, 127, 0] == 254 and t[0, 64, 0] == 128
    ref_g = (img[:, 0, 1].astype(np.uint64).reshape(96, 5).sum(1) * 2 + 5) // 10                # five rows, equal weights, rounded half up
    assert np.array_equal(t[:, 5, 1], ref_g.astype(np.uint8)) and t[0, 5, 1] == 1 and t[95, 5, 1] == 253   # rows 475 .. 479 hold 252 253 253 254 255
    assert render.thumbnail(np.full((100, 50), 9, np.uint8)).shape == (128, 64)          # smaller pictures are enlarged, as -resize does
    assert render.thumbnail(np.zeros((3, 1000, 3), np.uint8)).shape == (1, 128, 3)       # at least one row
    q = render.thumbnail(np.array([[0, 255], [255, 255]], np.uint8), box=(1, 1))
    assert q.tolist() == [[191]]                                                          # (765 + 2) // 4


def test_rgba_png_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (13, 21, 4), dtype=np.uint8)
    path = str(tmp_path / "rgba.png")
    render.write_png(path, img)
    L = _abi.lib()
    w, h, ch, bits, data = C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_void_p()
    L.sf_png_read.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    assert L.sf_png_read(path.encode(), C.byref(w), C.byref(h), C.byref(ch), C.byref(bits), C.byref(data)) == 0
    assert (w.value, h.value, ch.value, bits.value) == (21, 13, 4, 8)
    got = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), (13, 21, 4)).copy()
    L.sf_free.argtypes = [C.c_void_p]
    L.sf_free(data)
    assert np.array_equal(got, img)
    assert L.sf_png_write(path.encode(), rc._p(img), 21, 13, 2, 8) == -1   # grey + alpha stays refused


# ---- refusals and the ABI ---------------------------------------------------------------------------------------------------------------------------
def _refused(f, code=-1):
    with pytest.raises(Exception) as e:
        f()
    assert "(%d)" % code in str(e.value) or str(code) in str(e.value), str(e.value)


def test_refusals():
    box = np.array([0, 0, 0, 1, 1, 1], np.float32)
    _refused(lambda: render.camera(box, camera_up=(0, 0, 1)))                      # parallel to the view straight down
    _refused(lambda: render.camera(box, world_up=(0, 0, 0)))
    _refused(lambda: render.camera(box, world_up=(0, np.nan, 1)))
    _refused(lambda: render.camera(np.array([0, 0, 0, np.inf, 1, 1], np.float32)))
    _refused(lambda: render.camera(box, theta=np.inf))
    for bad in (dict(width=0), dict(samples=0), dict(samples=4097), dict(max_depth=0), dict(max_depth=17), dict(integrator=2), dict(fov=180.0), dict(height=8193)):
        _refused(lambda: render.Renderer(render.default_params(**bad), -1))
    tri = np.array([[0, 1, 2]], np.uint32)
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    with render.Renderer(render.default_params(width=8, height=8, samples=1), -1) as r:
        _refused(lambda: r.run(render.camera(box)))                               # no mesh yet
        _refused(lambda: r.set_mesh(Mesh.from_arrays(xyz, np.zeros((0, 3), np.uint32))))
        _refused(lambda: r.set_mesh(Mesh.from_arrays(xyz, np.array([[0, 1, 3]], np.uint32))), code=-7)   # no sf_mesh holds such an index: sf_mesh_create refuses it
        bad = xyz.copy()
        bad[1, 2] = np.nan
        _refused(lambda: r.set_mesh(Mesh.from_arrays(bad, tri)))
        r.set_mesh(Mesh.from_arrays(xyz, tri))                                    # a mesh without colours renders grey
        cam = render.camera(box)
        img = r.run(cam)
        assert img[0, 2, 2].tolist() == [np.float32(128) / np.float32(255)] * 3 + [1.0]
        cam.origin[0] = np.nan
        _refused(lambda: r.run(cam))
        _refused(lambda: r.rays(np.array([[0, 0, 1, 0, np.inf, -1]], np.float32)))
    _refused(lambda: render.tune("leaf", 16))
    _refused(lambda: render.tune("stack", 1))
    assert _abi.lib().sf_render_stage_sample(None, 0, 0, 0, None) == -1


def test_no_silent_fallback_to_the_host_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(Exception) as e:
        render.Renderer(render.default_params(), 0)
    assert "-5" in str(e.value) or "no HIP device" in str(e.value)
    assert b"never taken silently" in _abi.lib().sf_last_error()


def test_struct_layouts_match_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(sf_render_params), offsetof(sf_render_params, fov), offsetof(sf_render_params, pixel_centre), sizeof(sf_camera),
         offsetof(sf_camera, tan_half_fov));
  return 0;
}'''
    exe = str(tmp_path / "render_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(render.SfRenderParams), render.SfRenderParams.fov.offset, render.SfRenderParams.pixel_centre.offset, C.sizeof(render.SfCamera),
                   render.SfCamera.tan_half_fov.offset]


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ply(tmp_path_factory):
    c = rc.case("lattice")
    path = str(tmp_path_factory.mktemp("render_tool") / "scene0000_00_vh_clean_2.ply")
    c["mesh"].write_ply(path)
    return path


ARGS = ["--width", "40", "--height", "30", "--samples", "2", "--max-depth", "2"]


def _read_png(path):
    L = _abi.lib()
    w, h, ch, bits, data = C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_void_p()
    L.sf_png_read.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    assert L.sf_png_read(path.encode(), C.byref(w), C.byref(h), C.byref(ch), C.byref(bits), C.byref(data)) == 0
    out = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), (h.value, w.value, ch.value)).copy()
    L.sf_free.argtypes = [C.c_void_p]
    L.sf_free(data)
    return out


def test_tool_host_writes_render_mesh_bytes_and_the_thumbnail(small_ply):
    r = subprocess.run([TOOL, small_ply, "--host", "--thumb", "--theta", "30"] + ARGS, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == ""
    out, thumb = small_ply[:-4] + ".png", small_ply[:-4] + "_thumb.png"
    img = _read_png(out)
    ref = render.render_mesh(small_ply, device=-1, theta=30.0, width=40, height=30, samples=2, max_depth=2)
    assert img.shape == (30, 40, 4) and np.array_equal(img, ref)
    assert 0 < (img[..., 3] == 255).mean() < 1
    assert np.array_equal(_read_png(thumb), render.thumbnail(ref)) and _read_png(thumb).shape == (96, 128, 4)
    ao = small_ply[:-4] + "_ao.png"
    r = subprocess.run([TOOL, small_ply, "--host", "-o", ao, "--integrator", "ao", "--world_up", "z", "--camera_up", "0,2,0", "--cameras", "ignored.txt"] + ARGS,
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == ""
    assert np.array_equal(_read_png(ao), render.render_mesh(small_ply, device=-1, integrator="ao", width=40, height=30, samples=2, max_depth=2))


def test_tool_turntable_names(small_ply):
    r = subprocess.run([TOOL, small_ply, "--host", "--render_turntable", "--frames_per_degree", "120"] + ARGS, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == ""
    frames = [small_ply + "_%03d.png" % i for i in range(3)]
    assert all(os.path.exists(f) for f in frames) and not os.path.exists(small_ply + "_003.png")
    for i, f in enumerate(frames):
        assert np.array_equal(_read_png(f), render.render_mesh(small_ply, device=-1, theta=120.0 * i, width=40, height=30, samples=2, max_depth=2)), i


def test_tool_refuses_what_it_does_not_provide(small_ply):
    for integ in ("mlt", "vpl"):
        r = subprocess.run([TOOL, small_ply, "--host", "--integrator", integ], capture_output=True, text=True)
        assert r.returncode != 0 and integ in r.stderr
    assert subprocess.run([TOOL, small_ply, "--host", "--camera_up", "z"] + ARGS, capture_output=True, text=True).returncode != 0   # parallel to the view
    r = subprocess.run([TOOL, small_ply, "--host", "--render_turntable", "--thumb"] + ARGS, capture_output=True, text=True)
    assert r.returncode != 0 and "--thumb" in r.stderr
    with pytest.raises(TypeError):
        render.render_mesh(small_ply, device=-1, params=render.default_params(), samples=2)


# ---- the host sources once under sanitizers, as a stand-alone program ------------------------------------------------------------------------------------
@needs_checker
def test_host_sources_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "render_host_san")
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-mfma", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "render_host_main.cpp"),
           os.path.join(ROOT, "scannet_amd", "csrc", "render_host.cpp"), "-lpthread"]
    subprocess.run(cmd, check=True)
    c = rc.case("room")
    p = c["p"]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    thetas = np.array([th for th, _ in c["views"]], np.float32)
    with open(fin, "wb") as f:
        f.write(np.array([len(c["xyz"]), len(c["tris"])], np.int64).tobytes())
        f.write(np.array([p.width, p.height, p.samples, p.max_depth, p.integrator, p.pixel_centre, len(thetas), 4], np.int32).tobytes())
        f.write(c["xyz"].tobytes() + c["rgba"].tobytes() + c["tris"].tobytes() + thetas.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]      # the program also asks build_tree for the two refusals no sf_mesh can carry
    ref = rc.checker_images("room")
    raw = np.fromfile(fout, np.uint8)
    got = raw[:ref.size * 4].view(np.float32).reshape(ref.shape)
    assert np.array_equal(rc.bits(got), rc.bits(ref))
    px = raw[ref.size * 4:ref.size * 4 + p.width * p.height * 4].reshape(p.height, p.width, 4)
    assert np.array_equal(px, render.film(ref[0], 1.0))
    assert np.array_equal(raw[ref.size * 4 + px.size:].reshape(48, 64, 4), render.thumbnail(px, box=(64, 64)))
