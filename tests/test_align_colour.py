"""The dense colour term of the global alignment (DESIGN.md "The colour term of the global alignment", 4f; scannet_amd/csrc/align_colour.hip).

The rule is pinned as section 4e's is: tests/align_checker.c restates it in C (one checker for the depth term and the colour term, over
tests/solver_rules.h); the scenes are rendered in numpy by tests/solver_scenes.py.
  * without a GPU: a wall that depth alone cannot align (status 1) is aligned to sub-pixel accuracy with colour; the analytic row against a float64
    finite difference; the furnished room with a painted texture stays within 4e's bound; the checker against its recorded digests
    (tests/golden/solver_checker.json), colour_weight 0 giving the depth term's bits; parameters, struct layouts, the tool's refusals, the kernels'
    resources;
  * -m gpu: sf_fuser_align_rgbd_system and sf_fuser_align_rgbd against the checker bit for bit, the buffers' three states, the correction loop
    align_and_reintegrate(with_colour=True).
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, synth
from tests import solver_scenes as ss
from tests.solver_scenes import CFX, CFY, CH, CMX, CMY, CW, FOOT, FX, FY, H, MX, MY, SH, SW, W, WALL_Z, align_arrays as _arrays, texture, wall_scene
from tests.solver_scenes import align_res_tuple as res_tuple, resampled_scene, small_scene, worst_in_plane_error as in_plane_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "depthsensing")
FIXTURE = os.path.join(ROOT, "tests", "golden", "zParametersBundlingScanNet.txt")
SF_ERR_INVALID_ARG = -1
ROOM_T_BOUND, ROOM_R_BOUND = 0.015, 0.005   # DESIGN.md 4e's bound on the furnished room
LEVEL = ss.ALIGN_LEVEL
BOUND = 0.5 * FOOT                           # test 1's bound: half a level pixel's footprint (27.7 mm)


def frame_of(w=W, h=H, intr=None, colour=ss.WALL_CAMERA):
    return ss.align_frame(w, h, intr, colour)


def fuser_params(w=W, h=H, colour=ss.WALL_CAMERA, voxel=0.008):
    return ss.fuser_params(w, h, colour, voxel)


@pytest.fixture(scope="module")
def chk():
    """tests/align_checker.c is there to be compiled; the tests reach it through tests/solver_scenes.py."""
    if not ss.checkers_available():
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    return ss.align_lib()


def cpu_align(depth, rgb, poses, pairs, a, fr=None):
    return ss.cpu_align(depth, poses, pairs, a, fr or frame_of(), rgb)


def cpu_system(depth, rgb, poses, pairs, a, fr=None):
    return ss.cpu_align_system(depth, poses, pairs, a, fr or frame_of(), rgb)


def working_params(**over):
    """The defaults with the working weight of `--align-colour`."""
    from scannet_amd import fusion
    return fusion.default_align_params(**dict(dict(colour_weight=fusion.ALIGN_COLOUR_WEIGHT, level=LEVEL), **over))


@pytest.fixture(scope="module")
def wall():
    """Test 1's input: 4 keyframes."""
    return wall_scene(4)


@pytest.fixture(scope="module")
def wall_cpu(chk, wall):
    """The checker's answers on the wall, without and with colour (shared with the GPU tests)."""
    from scannet_amd import fusion
    depth, rgb, truth, start = wall
    pairs, count = fusion.align_pairs(start, fusion.default_align_params())
    assert count == len(pairs) == 12
    rc0, out0, res0 = cpu_align(depth, rgb, start, pairs, working_params(colour_weight=0.0))
    rc1, out1, res1 = cpu_align(depth, rgb, start, pairs, working_params())
    assert rc0 == 0 and rc1 == 0
    return pairs, (out0, res0), (out1, res1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 1: depth alone is singular on the wall; with colour every keyframe ends within half a level pixel's footprint
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_checker_wall_is_singular_without_colour_and_aligned_with_it(wall, wall_cpu):
    depth, rgb, truth, start = wall
    pairs, (out0, res0), (out1, res1) = wall_cpu
    e_start = in_plane_error(start, truth)
    assert e_start > 2.0 * FOOT   # the start is more than four times the bound off
    assert res0.status == 1 and out0.tobytes() == start.reshape(-1, 16).tobytes(), res0.as_dict()
    e = in_plane_error(out1, truth)
    print("wall: in-plane error %.2f mm -> %.2f mm (bound %.2f mm), %s" % (e_start * 1e3, e * 1e3, BOUND * 1e3, res1.as_dict()))
    assert res1.status == 0 and res1.frames_unconnected == 0 and res1.frames_rejected == 0, res1.as_dict()
    assert res1.colour_correspondences > 0 and res1.colour_rms_last < res1.colour_rms_first, res1.as_dict()
    assert e < BOUND, (e, BOUND, res1.as_dict())
    assert out1[0].tobytes() == start[0].reshape(16).tobytes()   # the fixed frame


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 2: the analytic row (p x a, a), +J for xi_i and -J for xi_j, against a float64 finite difference
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_colour_row_equals_a_finite_difference(chk, wall):
    """The bilinear interpolant's own derivative is a one-sided difference and is not what the term uses (it samples central differences), so the
    float64 residual here is the term's own linear intensity model about the sampled point, I_t + (gx, gy) . (u - u0, v - v0) - I_s with I_t, gx, gy
    as the checker sampled them: the finite difference then tests what the row states, the projection, the two rigid motions and their signs.
    Tolerance: central differences at steps h = 1e-4 and h / 2 differ by their own O(h^2) truncation error (measured below: 4e-9 relative to the
    row's largest entry); the bound is 10 x the larger of that and of float32's 6e-7 relative error of an entry of the analytic row (a handful of
    rounded operations), relative to the row's largest entry."""
    depth, rgb, truth, start = wall
    a = working_params()
    fr = frame_of()
    depth_, rgb_, poses, _ = _arrays(depth, rgb, start, [[1, 0]])
    i, j = 1, 0
    npx = (W >> LEVEL) * (H >> LEVEL)
    rows = np.zeros((npx, 8), np.float32)
    assert chk.al_rows(C.byref(fr), depth_.ctypes.data, rgb_.ctypes.data, len(poses), poses.ctypes.data, i, j, C.byref(a), rows.ctypes.data) == 0
    vmap, pmap, cam = np.zeros((npx, 3), np.float32), np.zeros((npx, 3), np.float32), np.zeros(6, np.float32)
    assert chk.al_maps(C.byref(fr), depth_.ctypes.data, rgb_.ctypes.data, len(poses), i, C.byref(a), vmap.ctypes.data, pmap.ctypes.data, cam.ctypes.data) == 0
    pj = np.zeros((npx, 3), np.float32)
    assert chk.al_maps(C.byref(fr), depth_.ctypes.data, rgb_.ctypes.data, len(poses), j, C.byref(a), vmap.copy().ctypes.data, pj.ctypes.data, cam.copy().ctypes.data) == 0
    wl, fx, fy, mx, my = int(cam[0]), float(cam[2]), float(cam[3]), float(cam[4]), float(cam[5])
    Ti, Tj = poses[i].reshape(4, 4).astype(np.float64), poses[j].reshape(4, 4).astype(np.float64)
    picked = np.flatnonzero(rows[:, 0] > 0)
    assert len(picked) > 500
    picked = picked[:: len(picked) // 48][:48]   # a few dozen pixels across the image

    def project(Ta, Tb, v):
        c = np.linalg.inv(Tb) @ Ta @ np.append(v, 1.0)
        return np.array([c[0] / c[2] * fx + mx, c[1] / c[2] * fy + my])

    def bil(comp, u):
        x0, y0 = int(np.floor(u[0])), int(np.floor(u[1]))
        ax, ay = u[0] - x0, u[1] - y0
        t = pj[:, comp].astype(np.float64)
        top = t[y0 * wl + x0] + ax * (t[y0 * wl + x0 + 1] - t[y0 * wl + x0])
        bot = t[(y0 + 1) * wl + x0] + ax * (t[(y0 + 1) * wl + x0 + 1] - t[(y0 + 1) * wl + x0])
        return top + ay * (bot - top)

    worst_fd, worst = 0.0, 0.0
    for px in picked:
        v = vmap[px].astype(np.float64)
        u0 = project(Ti, Tj, v)
        g = np.array([bil(1, u0), bil(2, u0)])

        def residual(xi_i, xi_j):
            return float(g @ (project(ss.increment(xi_i, Ti), ss.increment(xi_j, Tj), v) - u0))   # the constant I_t - I_s drops out of every difference

        J = rows[px, 2:8].astype(np.float64)
        scale = np.abs(J).max()
        for sign, which in ((1.0, 0), (-1.0, 1)):
            fd = {}
            for h in (1e-4, 5e-5):
                d = np.zeros(6)
                for k in range(6):
                    e = np.zeros(6)
                    e[k] = h
                    z = np.zeros(6)
                    hi = residual(e, z) if which == 0 else residual(z, e)
                    lo = residual(-e, z) if which == 0 else residual(z, -e)
                    d[k] = (hi - lo) / (2 * h)
                fd[h] = d
            worst_fd = max(worst_fd, np.abs(fd[1e-4] - fd[5e-5]).max() / scale)
            worst = max(worst, np.abs(fd[5e-5] - sign * J).max() / scale)
    tol = 10.0 * max(worst_fd, 6e-7)
    print("colour row: finite-difference error %.2e, analytic row against it %.2e, tolerance %.2e (relative to the row's largest entry)" % (worst_fd, worst, tol))
    assert worst < tol, (worst, tol)


def test_sampled_gradient_is_the_derivative_of_the_intensity(chk, wall):
    """What the finite difference above takes as given: that (gx, gy) of the map is the derivative of the map's intensity, with its sign and scale.
    (a) Against a float64 central difference of the map's own intensities: the float32 subtraction of two values in [0, 1] is exact to half an ulp of
    a value below 1, 3e-8, and the halving is exact: bound 1e-7.  (b) Against the analytic derivative of the texture at the pixel's centre on the wall,
    per level pixel (dX/dx = FOOT): the central difference of a sinusoid of wavelength L pixels is short by 1 - sinc(2 pi / L) <= 2.6 % at L = 16; a
    level pixel is the mean of four nearest colour pixels, each up to half a colour pixel (0.18 level pixels) from its ray, which over the
    difference's two-pixel baseline is at most 18 % of the gradient; an 8-bit sample is off by at most 0.5 / 255, twice that over the difference,
    halved: 0.002.  Bound: 0.21 x the largest gradient in the map + 0.002.  A flipped sign or a factor of two is far outside both."""
    depth, rgb, truth, start = wall
    a = working_params()
    fr = frame_of()
    depth_, rgb_, poses, _ = _arrays(depth, rgb, truth, [[1, 0]])
    wl, hl = W >> LEVEL, H >> LEVEL
    vmap, pmap, cam = np.zeros((wl * hl, 3), np.float32), np.zeros((wl * hl, 3), np.float32), np.zeros(6, np.float32)
    assert chk.al_maps(C.byref(fr), depth_.ctypes.data, rgb_.ctypes.data, len(poses), 0, C.byref(a), vmap.ctypes.data, pmap.ctypes.data, cam.ctypes.data) == 0
    I, gx, gy = (pmap[:, k].reshape(hl, wl).astype(np.float64) for k in range(3))
    ok = np.isfinite(gx)
    assert ok.sum() > 0.5 * wl * hl and not ok[0].any() and not ok[:, 0].any() and not ok[-1].any() and not ok[:, -1].any()
    assert (np.isfinite(I).sum() < wl * hl) and (np.isfinite(gy) == ok).all()   # the narrower colour field leaves pixels without intensity
    cx = np.full_like(I, np.nan)
    cy = np.full_like(I, np.nan)
    with np.errstate(invalid="ignore"):
        cx[:, 1:-1] = (I[:, 2:] - I[:, :-2]) * 0.5
        cy[1:-1, :] = (I[2:, :] - I[:-2, :]) * 0.5
    ea = max(np.abs(gx[ok] - cx[ok]).max(), np.abs(gy[ok] - cy[ok]).max())
    # (b) the analytic derivative: frame 0 is at the origin, so the pixel centre (2x + 0.5, 2y + 0.5) of level 0 meets the wall at ((. - mx) / fx) z
    yy, xx = np.mgrid[0:hl, 0:wl]
    X, Y = (2 * xx + 0.5 - MX) / FX * WALL_Z, (2 * yy + 0.5 - MY) / FY * WALL_Z
    h = 1e-6
    lum = np.array([0.299, 0.587, 0.114])
    ax_ = (texture(X + h, Y) - texture(X - h, Y)) @ lum / (2 * h) * FOOT
    ay_ = (texture(X, Y + h) - texture(X, Y - h)) @ lum / (2 * h) * FOOT
    big = max(np.abs(ax_).max(), np.abs(ay_).max())
    eb = max(np.abs(gx[ok] - ax_[ok]).max(), np.abs(gy[ok] - ay_[ok]).max())
    print("gradient: %.2e from the map's own central difference (bound 1e-7); %.4f from the texture's derivative (largest %.4f, bound %.4f)" % (
        ea, eb, big, 0.21 * big + 0.002))
    assert ea <= 1e-7, ea
    assert eb <= 0.21 * big + 0.002, (eb, big)


def test_picture_size_follows_the_fuser(wall):
    """The pictures are color_width x color_height, else the depth frames' own size -- also where the fuser resamples depth to another integration
    size: the library copies K x that many bytes (fuser.hip sets the colour camera to the depth frames' in that case)."""
    from scannet_amd import fusion
    f = fusion.Fuser.__new__(fusion.Fuser)   # the check reads the parameters alone: no device
    f.params = fusion.default_params(depth_width=144, depth_height=112, integration_width=72, integration_height=56)
    assert f._align_rgb(np.zeros(3 * 144 * 112 * 3, np.uint8), 3).size == 3 * 144 * 112 * 3
    with pytest.raises(ValueError):
        f._align_rgb(np.zeros(3 * 72 * 56 * 3, np.uint8), 3)   # the integration size is not it
    f.params = fusion.default_params(depth_width=144, depth_height=112, integration_width=72, integration_height=56, color_width=90, color_height=70)
    assert f._align_rgb(np.zeros(2 * 90 * 70 * 3, np.uint8), 2).size == 2 * 90 * 70 * 3
    with pytest.raises(ValueError):
        f._align_rgb(np.zeros(2 * 144 * 112 * 3, np.uint8), 2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 3: the furnished room of 4e's test with the texture painted on by world position does not get worse
# ---------------------------------------------------------------------------------------------------------------------------------------------
RW, RH = ss.RW, ss.RH


def test_checker_furnished_room_with_texture_stays_within_4e_bound(chk):
    from scannet_amd import fusion
    boxes = synth.clutter_boxes()
    truth = [synth.trajectory_pose(10 * k, ss.WALK_TOTAL) for k in range(8)]
    depth = np.stack([synth.render_room_depth(p, RW, RH, noise_frame=10 * k, noise=2, boxes=boxes).reshape(-1) for k, p in enumerate(truth)])
    start = ss.drifted(truth)
    rgb = np.stack([ss.paint_room(d, t) for d, t in zip(depth, truth)])
    fr = frame_of(RW, RH, colour=(0, 0, 0.0, 0.0, 0.0, 0.0))
    a = working_params()
    pairs, count = fusion.align_pairs(start, a)
    rc, out, res = cpu_align(depth, rgb, start, pairs, a, fr)
    assert rc == 0
    et, er = ss.worst_pose_error(out, truth)
    print("room with colour: worst %.3f mm / %.3f mrad, %s" % (et * 1e3, er * 1e3, res.as_dict()))
    assert res.status == 0 and res.frames_unconnected == 0 and res.frames_rejected == 0 and res.colour_correspondences > 0, res.as_dict()
    assert et < ROOM_T_BOUND and er < ROOM_R_BOUND, (et, er, res.as_dict())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 4: the checker says what it was recorded to say, and pictures at colour_weight 0 leave the depth term's bits alone
# ---------------------------------------------------------------------------------------------------------------------------------------------
ALIGN_CASES = [n for n in ss.CASE_NAMES if n.startswith("align-")]


@pytest.mark.parametrize("name", ALIGN_CASES)
def test_checker_reproduces_the_recorded_digests(chk, oracle, name):
    """tests/golden/solver_checker.json holds what the checker said on each case when it was recorded (first by the separate depth-only and colour
    checkers that tests/align_checker.c replaced).  A depth-only case is run without pictures and with random pictures at weight 0: both must give
    the recorded first 29 sums, poses and depth fields of the result."""
    want = json.load(open(ss.GOLDEN))["cases"][name]
    got = ss.run_case(name, oracle)
    assert got["inputs"] == want["inputs"], "%s: the case's INPUTS differ from the recorded ones (the scene, not the checker, changed)" % name
    assert got["outputs"] == want["outputs"], name
    if "-depth-" in name:
        idle = ss.run_case(name, oracle, idle_picture=True)
        assert idle["inputs"] == want["inputs"] and idle["outputs"] == want["outputs"], name


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 5: parameters, layouts, refusals, resources
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_colour_params_default_and_file(tmp_path):
    from scannet_amd import fusion
    a = fusion.default_align_params()
    assert (a.colour_weight, a.colour_thres, a.colour_gradient_min) == (0.0, np.float32(0.1), np.float32(0.005))
    assert fusion.ALIGN_COLOUR_WEIGHT > 0
    text = open(FIXTURE).read()
    assert "s_denseColorThresh = 0.1f" in text and "s_denseColorGradientMin = 0.005f" in text
    b = fusion.load_align_params(FIXTURE, fusion.default_align_params(colour_thres=0.5, colour_gradient_min=0.5, colour_weight=3.0))
    assert (b.colour_weight, b.colour_thres, b.colour_gradient_min) == (3.0, np.float32(0.1), np.float32(0.005))
    own = tmp_path / "own.txt"
    own.write_text("s_denseColorThresh = 0.25f;\ns_denseColorGradientMin = 0.02f;\n")
    c = fusion.load_align_params(own)
    assert (c.colour_thres, c.colour_gradient_min) == (np.float32(0.25), np.float32(0.02))
    own.write_text("s_denseColorThresh = grey;\n")
    with pytest.raises(_abi.ScanfuseError):
        fusion.load_align_params(own)


REFUSED = [("negative_weight", dict(colour_weight=-1.0), True), ("nan_weight", dict(colour_weight=float("nan")), True),
           ("inf_weight", dict(colour_weight=float("inf")), True), ("negative_threshold", dict(colour_weight=1.0, colour_thres=-0.1), True),
           ("negative_gradient", dict(colour_weight=1.0, colour_gradient_min=-0.1), True), ("no_pictures", dict(colour_weight=1.0), False)]


@pytest.mark.parametrize("name,over,with_rgb", REFUSED)
def test_refused_colour_arguments(chk, wall, name, over, with_rgb):
    """Arguments are checked before the fuser is looked at, so a NULL fuser tells a refused argument (-1 with its own message) from a passed one."""
    from scannet_amd import fusion
    depth, rgb, truth, start = wall
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    a = working_params(**over)
    rc, _, _ = cpu_align(depth[:2], rgb[:2] if with_rgb else None, start[:2], pairs, a)
    assert rc == -1
    L = _abi.lib()
    d_, r_, p_, q_ = _arrays(depth[:2], rgb[:2] if with_rgb else None, start[:2], pairs)
    out, res = np.empty_like(p_), fusion.SfAlignResult()
    L.sf_fuser_align_rgbd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(fusion.SfAlignParams), C.c_void_p,
                                      C.POINTER(fusion.SfAlignResult)]
    L.sf_last_error.restype = C.c_char_p
    assert L.sf_fuser_align_rgbd(None, d_.ctypes.data, None if r_ is None else r_.ctypes.data, 2, p_.ctypes.data, q_.ctypes.data, 2, C.byref(a), out.ctypes.data,
                                 C.byref(res)) == SF_ERR_INVALID_ARG
    assert b"colour" in L.sf_last_error(), L.sf_last_error()
    # the same parameters pass the argument checks once they are good: the refusal that is left is the NULL fuser's
    good = working_params()
    assert L.sf_fuser_align_rgbd(None, d_.ctypes.data, rgb[:2].ctypes.data, 2, p_.ctypes.data, q_.ctypes.data, 2, C.byref(good), out.ctypes.data,
                                 C.byref(res)) == SF_ERR_INVALID_ARG
    assert b"fuser" in L.sf_last_error(), L.sf_last_error()
    # the depth-only call ignores the three fields
    L.sf_fuser_align.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(fusion.SfAlignParams), C.c_void_p,
                                 C.POINTER(fusion.SfAlignResult)]
    assert L.sf_fuser_align(None, d_.ctypes.data, 2, p_.ctypes.data, q_.ctypes.data, 2, C.byref(a), out.ctypes.data, C.byref(res)) == SF_ERR_INVALID_ARG
    assert b"fuser" in L.sf_last_error(), L.sf_last_error()


def test_colour_structs_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sf_align_params), offsetof(sf_align_params, colour_weight), offsetof(sf_align_params, colour_thres),
         offsetof(sf_align_params, colour_gradient_min), offsetof(sf_align_params, reserved), sizeof(sf_align_result),
         offsetof(sf_align_result, colour_correspondences), offsetof(sf_align_result, colour_rms_first), offsetof(sf_align_result, colour_rms_last),
         offsetof(sf_align_result, reserved));
  return 0;
}'''
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = str(tmp_path / "alc_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    from scannet_amd import fusion
    P, R = fusion.SfAlignParams, fusion.SfAlignResult
    assert got == [C.sizeof(P), P.colour_weight.offset, P.colour_thres.offset, P.colour_gradient_min.offset, P.reserved.offset, C.sizeof(R),
                   R.colour_correspondences.offset, R.colour_rms_first.offset, R.colour_rms_last.offset, R.reserved.offset]
    assert got[0] == 96 and got[5] == 64   # the sizes before the colour term took its fields from `reserved`


def test_depthsensing_refuses_align_colour_without_align_and_without_colour_frames(tmp_path):
    if not os.path.exists(TOOL):
        pytest.skip("bin/depthsensing is built by build()")
    (tmp_path / "p.txt").write_text("s_SDFVoxelSize = 0.010f;\n")
    (tmp_path / "t.txt").write_text("s_maxLevels = 3;\n")
    base = [str(tmp_path / "p.txt"), str(tmp_path / "t.txt")]
    for flags in (["--align-colour"], ["--align-colour=0.5"], ["--track", "--align-colour"]):
        r = subprocess.run([TOOL] + base + [str(tmp_path / "none.sens")] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--align-colour" in r.stderr and "--align" in r.stderr.replace("--align-colour", ""), r.stderr
    for bad in ("--align-colour=-1", "--align-colour=x", "--align-colour=nan"):
        r = subprocess.run([TOOL] + base + [str(tmp_path / "none.sens"), "--track", "--align", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0
    # a file without colour frames is refused before the GPU is touched; the text names both flags
    r = subprocess.run([TOOL] + base + [ss.plain_sens(tmp_path, False), "--track", "--align", "--align-colour"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--align-colour" in r.stderr and "--align" in r.stderr.replace("--align-colour", "") and "colour frames" in r.stderr, r.stderr


def test_photo_kernels_live_in_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kr = ss.kernel_resources()
    rows = kr.kernels(os.path.join(ROOT, "scannet_amd", "libscanfuse.so"))
    every = [(kr.short(n), r) for r, n in zip(rows, kr.demangle([r["name"] for r in rows]))]
    # the colour term's own kernel, and the colour instantiation of the aligner's two (align.hip)
    mine = [(s, r) for s, r in every if s.startswith("k_photo_") or s in ("k_align_assoc<true>", "k_align_final<true>")]
    assert {s.split("<")[0] for s, _ in mine} == {"k_photo_prep", "k_align_assoc", "k_align_final"}
    assert len(mine) == 6 and len([s for s, _ in mine if s.startswith("k_photo_prep<")]) == 4   # one per level
    assert [s for s, _ in every if "assoc" in s and "align" in s and s != "k_align_assoc<true>"] == ["k_align_assoc<false>"]
    for s, r in mine:
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (s, r)
        assert r["lds"] <= 160 * 1024, (s, r["lds"])
    assoc = [r for s, r in mine if s == "k_align_assoc<true>"][0]
    assert assoc["lds"] == 4 * 31 * 4   # the cross-wave step of 31 sums


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return small_scene()


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2])
def test_gpu_rgbd_systems_bit_exact(chk, small, level):
    from scannet_amd import fusion
    depth, rgb, poses, pairs, colour = small
    a = working_params(level=level, min_pair_correspondences=1)
    rc, want = cpu_system(depth, rgb, poses, pairs, a, frame_of(SW, SH, colour=colour))
    assert rc == 0
    with fusion.Fuser(fuser_params(SW, SH, colour), device=0) as f:
        got = f.align_rgbd_system(depth, rgb, poses, pairs, a)
        none = f.align_rgbd_system(depth, None, poses, pairs, working_params(level=level, colour_weight=0.0))
        plain = f.align_system(depth, poses, pairs, a)
    print("level %d: depth counts %s, colour counts %s" % (level, want[:, 28].astype(int).tolist(), want[:, 30].astype(int).tolist()))
    assert got.shape == (12, 31) and got.tobytes() == want.tobytes(), (level, np.abs(got - want).max())
    assert (want[:9, 30] > 0).all() and (want[:9, 30] < want[:9, 28]).all()   # colour rows exist and the narrower colour field drops some
    assert not want[9:].any()                                                  # the lost frame's pairs and the pair without overlap
    assert none[:, :29].tobytes() == plain.tobytes() and not none[:, 29:].any()   # without pictures: the depth term's bits


def test_checker_resampled_depth_reads_pictures_at_the_depth_size(chk):
    depth, rgb, poses, pairs, p, fr = resampled_scene()
    rc, want = cpu_system(depth, rgb, poses, pairs, working_params(level=0, min_pair_correspondences=1), fr)
    assert rc == 0 and (want[:, 30] > 1000).all() and (want[:, 30] <= want[:, 28]).all(), want[:, 28:]
    assert np.sqrt(want[:, 29] / want[:, 30]).max() < 0.02   # at the true poses the pictures agree: the look-up hits the right pixels


@pytest.mark.gpu
def test_gpu_rgbd_systems_bit_exact_with_resampled_depth(chk):
    from scannet_amd import fusion
    depth, rgb, poses, pairs, p, fr = resampled_scene()
    with fusion.Fuser(p, device=0) as f:
        for level in (0, 1):
            a = working_params(level=level, min_pair_correspondences=1)
            rc, want = cpu_system(depth, rgb, poses, pairs, a, fr)
            got = f.align_rgbd_system(depth, rgb, poses, pairs, a)
            assert rc == 0 and (want[:, 30] > 0).all() and got.tobytes() == want.tobytes(), (level, np.abs(got - want).max())


@pytest.mark.gpu
def test_gpu_rgbd_solve_bit_exact_and_leaves_the_volume_alone(wall, wall_cpu):
    import torch
    from scannet_amd import fusion
    depth, rgb, truth, start = wall
    pairs, (out0, res0), (out1, res1) = wall_cpu
    with fusion.Fuser(fuser_params(), device=0) as f:
        for k in range(2):
            assert f.integrate(depth[k], truth[k], rgb=rgb[k])
        f.sync()
        before, st0 = ss.volume_digest(f), f.stats()
        out, res = f.align(depth, start, pairs, working_params(), rgb=rgb)
        assert res_tuple(res) == res_tuple(res1), (res.as_dict(), res1.as_dict())
        assert out.tobytes() == out1.tobytes()
        assert in_plane_error(out, truth) < BOUND
        # colour_weight 0: the depth-only call's bytes (singular on the wall), from host and from device frames
        a0 = working_params(colour_weight=0.0)
        o_d, r_d = f.align(depth, start, pairs, a0)
        o_c, r_c = f.align(depth, start, pairs, a0, rgb=rgb)
        assert r_d.status == 1 and o_c.tobytes() == o_d.tobytes() and res_tuple(r_c)[:8] == res_tuple(r_d)[:8] == res_tuple(res0)[:8]
        assert res_tuple(r_c) == res_tuple(res0)
        d = torch.from_numpy(depth.astype(np.int16)).to("cuda:0")
        c = torch.from_numpy(rgb).to("cuda:0")
        torch.cuda.synchronize()
        o_dev, r_dev = f.align_device(d, W * H * 2, start, pairs, working_params(), d_rgb=c, rgb_stride_bytes=CW * CH * 3)
        assert o_dev.tobytes() == out1.tobytes() and res_tuple(r_dev) == res_tuple(res1)
        o_dd, r_dd = f.align_device(d, W * H * 2, start, pairs, a0)   # sf_fuser_align_device
        o_d0, r_d0 = f.align_device(d, W * H * 2, start, pairs, a0, d_rgb=c, rgb_stride_bytes=CW * CH * 3)
        assert o_d0.tobytes() == o_dd.tobytes() and res_tuple(r_d0)[:8] == res_tuple(r_dd)[:8] and r_d0.colour_correspondences > 0
        assert ss.volume_digest(f) == before and f.stats() == st0


@pytest.mark.gpu
def test_gpu_rgbd_solvable_scene_with_weight_zero_equals_the_depth_only_call(chk):
    """On a scene depth can solve, the colour path at weight 0 returns sf_fuser_align_device's poses and every old field of its result."""
    from scannet_amd import fusion
    depth, rgb, start, pairs = ss.coloured_arc()   # three keyframes of the room's corner, random pictures at the colour camera's own size
    a = fusion.default_align_params()
    with fusion.Fuser(fuser_params(), device=0) as f:
        o_d, r_d = f.align(depth, start, pairs, a)
        o_c, r_c = f.align(depth, start, pairs, a, rgb=rgb)
    assert r_d.status == 0 and r_d.iterations > 1
    assert o_c.tobytes() == o_d.tobytes() and res_tuple(r_c)[:8] == res_tuple(r_d)[:8] and r_c.colour_correspondences > 0


@pytest.mark.gpu
def test_gpu_rgbd_buffers_grow_and_never_go_stale(chk, small):
    """One fuser's buffers through their three states: made for K = 2, P = 2 at level 2, every one of them grown for K = 6, P = 12 at level 0, and the
    small problem again in the larger buffers."""
    from scannet_amd import fusion
    depth, rgb, poses, pairs, colour = small
    fr = frame_of(SW, SH, colour=colour)
    little = (depth[:2], rgb[:2], poses[:2], pairs[:2], working_params(level=2, min_pair_correspondences=1))
    big = (depth, rgb, poses, pairs, working_params(level=0, min_pair_correspondences=1))
    want = {}
    for name, (d, c, p, q, a) in (("little", little), ("big", big)):
        rc, want[name] = cpu_system(d, c, p, q, a, fr)
        assert rc == 0 and (want[name][:2, 30] > 0).all()
    with fusion.Fuser(fuser_params(SW, SH, colour), device=0) as f:
        for step, name in enumerate(("little", "big", "little")):
            d, c, p, q, a = little if name == "little" else big
            got = f.align_rgbd_system(d, c, p, q, a)
            assert got.shape == want[name].shape and got.tobytes() == want[name].tobytes(), (step, name)


@pytest.mark.gpu
def test_gpu_align_and_reintegrate_with_colour(tmp_path):
    """8 keyframes of the wall in a .sens with its pictures: the depth-only loop changes nothing, the colour loop brings every keyframe under test 1's
    bound and moves the volume there."""
    from scannet_amd import fusion, sens
    depth, rgb, truth, start = wall_scene(8)
    Kd = synth.intrinsic_matrix(W, H)
    Kc = np.eye(4, dtype=np.float32)
    Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2] = CFX, CFY, CMX, CMY
    sd = sens.SensorData.create(CW, CH, W, H, Kc, Kd, sensor_name="StructureSensor")
    for k in range(8):
        sd.add_frame(depth[k], start[k], color=rgb[k], timestamp_depth=k)
    path = str(tmp_path / "wall.sens")
    sd.save(path)
    sd.close()
    sd = sens.SensorData(path)
    with fusion.Fuser(fuser_params(), device=0) as f:
        for k in range(8):
            assert f.integrate(depth[k], start[k], rgb=rgb[k])
        integrated = np.ascontiguousarray(start.reshape(8, 16))
        held = integrated.copy()
        before = ss.volume_digest(f)
        target, res, stats = fusion.align_and_reintegrate(f, sd, integrated, every=1, params=fusion.default_align_params(level=LEVEL), colour=True)
        assert res.status == 1 and target.tobytes() == held.tobytes() and stats["frames_moved"] == 0 and ss.volume_digest(f) == before, (res.as_dict(), stats)
        target, res, stats = fusion.align_and_reintegrate(f, sd, integrated, every=1, params=fusion.default_align_params(level=LEVEL), colour=True,
                                                          with_colour=True)
        e = in_plane_error(target, truth)
        print("loop: in-plane error %.2f mm -> %.2f mm, %s, %s" % (in_plane_error(start, truth) * 1e3, e * 1e3, res.as_dict(), stats))
        assert res.status == 0 and res.frames_rejected == 0 and res.frames_unconnected == 0, res.as_dict()
        assert e < BOUND, (e, BOUND)
        assert integrated.tobytes() == target.tobytes() and stats["frames_moved"] == 7 and ss.volume_digest(f) != before
    sd.close()
