"""The dense colour term of the camera tracker (DESIGN.md "The colour term of the tracker", 4g; scannet_amd/csrc/track_colour.hip).

The rule is pinned as section 4c's is: tests/track_checker.c restates it in C (one checker for the depth term and the colour term, over
tests/solver_rules.h), the oracle fuses, tests/raycast_checker.c renders the model's depth, normals and colour.
  * without a GPU: a frame sliding along one textured wall, which depth alone loses (lost_reason 3), is tracked to sub-pixel accuracy with colour; the
    analytic row against a float64 finite difference; the furnished room's loop with a painted texture stays within 4c's bound and is no worse than
    its depth-only run; the checker against its recorded digests (tests/golden/solver_checker.json), colour_weight 0 giving the depth term's bits; a
    model miss gives no colour row; parameters, struct layouts, the tool's refusals, the kernels' resources;
  * -m gpu: sf_fuser_track_rgbd_system and sf_fuser_track_rgbd against the checker bit for bit, the device entry point, the work set's states,
    track_and_fuse(with_colour=True), bin/depthsensing --track --track-colour.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, synth
from tests import solver_scenes as ss
from tests.solver_scenes import CAMERAS, FOOT0, H, W, cpu_model, cpu_system, cpu_track, in_plane_error, ptr as _p, walk_pose
from tests.solver_scenes import TrackWall as Wall, render_walk as render, track_res_tuple as res_tuple, under_the_depth_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "depthsensing")
SF_ERR_INVALID_ARG = -1
VOXEL = ss.TRACK_VOXEL
BOUND = 0.5 * FOOT0               # test 1's bound: half a level-0 pixel's footprint (13.8 mm), the sampling limit
# 4c's furnished room: its size, its loop and its bounds (tests/test_track.py)
ROOM_W, ROOM_H = 320, 240
LOOP_T_BOUND, LOOP_R_BOUND = 0.015, 0.005


def oracle_params(oracle, w=W, h=H, voxel=VOXEL):
    return ss.oracle_params(oracle, w, h, voxel)


def working_params(**over):
    """The defaults with the working weight of `--track-colour`."""
    from scannet_amd import fusion
    return fusion.default_track_params(**dict(dict(colour_weight=fusion.TRACK_COLOUR_WEIGHT), **over))


@pytest.fixture(scope="module")
def chk():
    """tests/raycast_checker.c and tests/track_checker.c are there to be compiled."""
    if not ss.checkers_available():
        pytest.skip("needs gcc and a CPU with fused multiply-add")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The wall (tests/solver_scenes.py TrackWall): FUSED frames sliding along it are fused with colour; the next frame lies one step (3 cm) further and is
# turned TURN about the normal
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(CAMERAS))
def wall(request, oracle):
    return Wall(oracle, request.param)


@pytest.fixture(scope="module")
def wall_cpu(chk, wall):
    """The checker's answers on the wall, without and with colour (shared with the GPU tests)."""
    a0 = cpu_track(wall.blocks, wall.op, wall.depth, wall.guess, working_params(colour_weight=0.0), colour=wall.colour, rgb=wall.rgb)
    a1 = cpu_track(wall.blocks, wall.op, wall.depth, wall.guess, working_params(), colour=wall.colour, rgb=wall.rgb)
    assert a0[0] == 0 and a1[0] == 0
    return a0[1:], a1[1:]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 1: depth alone loses the frame on the wall; with colour it is tracked within half a level-0 pixel's footprint
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_checker_wall_is_lost_without_colour_and_tracked_with_it(wall, wall_cpu):
    (pose0, res0), (pose1, res1) = wall_cpu
    e_start = in_plane_error(wall.guess, wall.truth)
    assert e_start > 2.0 * FOOT0   # the guess is more than four times the bound off
    assert res0.tracked == 0 and res0.lost_reason == 3 and np.isneginf(pose0).all(), res0.as_dict()
    assert res1.tracked == 1 and res1.lost_reason == 0, res1.as_dict()
    e = in_plane_error(pose1, wall.truth)
    et, er = ss.pose_error(pose1, wall.truth)
    print("wall: in-plane error %.2f mm -> %.2f mm (bound %.2f mm), whole pose %.2f mm / %.2f mrad, %s" % (e_start * 1e3, e * 1e3, BOUND * 1e3, et * 1e3, er * 1e3,
                                                                                                       res1.as_dict()))
    assert res1.colour_correspondences > 0.3 * res1.correspondences and res1.correspondences > 0.8 * W * H, res1.as_dict()
    assert e <= BOUND, (e, BOUND, res1.as_dict())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 2: the analytic row (p x a, a) for a left increment on T alone against a float64 finite difference
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_colour_row_equals_a_finite_difference(chk, wall):
    """As tests/test_align_colour.py's: the float64 residual is the term's own linear intensity model about the sampled point,
    I_t + (gx, gy) . (u - u0, v - v0) - I_s with gx, gy as the checker sampled them, so the difference tests what the row states: the projection, the
    rigid motion of T and its sign (the model does not move).  Bound: 10 x the larger of the difference quotient's own error (steps h and h / 2) and
    float32's 6e-7 relative error of an entry, relative to the row's largest entry."""
    t = working_params()
    level = 1
    model = cpu_model(wall.blocks, wall.op, wall.guess, t)
    T = ss.left_increment(wall.guess, 0.7 * FOOT0, -0.4 * FOOT0, 0.002)
    T32, R32 = np.ascontiguousarray(T, np.float32).reshape(16), np.ascontiguousarray(wall.guess, np.float32).reshape(16)
    wl = W >> level
    code, rows = ss.cpu_track_rows(wall.op, wall.depth, wall.rgb, model, level, T32, R32, t, wall.colour)
    assert code == 0
    code, vmap, pm, cam = ss.cpu_track_maps(wall.op, wall.depth, wall.rgb, model, level, R32, t, wall.colour)
    assert code == 0
    fx, fy, mx, my = (float(x) for x in cam[2:])
    Td, Rd = T32.reshape(4, 4).astype(np.float64), R32.reshape(4, 4).astype(np.float64)
    picked = np.flatnonzero(rows[:, 0] > 0)
    assert len(picked) > 500
    picked = picked[:: len(picked) // 48][:48]

    def project(Ta, v):
        q = np.linalg.inv(Rd) @ Ta @ np.append(v, 1.0)
        return np.array([q[0] / q[2] * fx + mx, q[1] / q[2] * fy + my])

    def bil(comp, u):
        x0, y0 = int(np.floor(u[0])), int(np.floor(u[1]))
        ax, ay = u[0] - x0, u[1] - y0
        m = pm[:, comp].astype(np.float64)
        top = m[y0 * wl + x0] + ax * (m[y0 * wl + x0 + 1] - m[y0 * wl + x0])
        bot = m[(y0 + 1) * wl + x0] + ax * (m[(y0 + 1) * wl + x0 + 1] - m[(y0 + 1) * wl + x0])
        return top + ay * (bot - top)

    worst_fd, worst = 0.0, 0.0
    for px in picked:
        v = vmap[px].astype(np.float64)
        u0 = project(Td, v)
        g = np.array([bil(1, u0), bil(2, u0)])
        J = rows[px, 2:8].astype(np.float64)
        scale = np.abs(J).max()
        fd = {}
        for h in (1e-4, 5e-5):
            dd = np.zeros(6)
            for k in range(6):
                e = np.zeros(6)
                e[k] = h
                dd[k] = (float(g @ (project(ss.increment(e, Td), v) - u0)) - float(g @ (project(ss.increment(-e, Td), v) - u0))) / (2 * h)
            fd[h] = dd
        worst_fd = max(worst_fd, np.abs(fd[1e-4] - fd[5e-5]).max() / scale)
        worst = max(worst, np.abs(fd[5e-5] - J).max() / scale)
    tol = 10.0 * max(worst_fd, 6e-7)
    print("colour row: finite-difference error %.2e, analytic row against it %.2e, tolerance %.2e (relative to the row's largest entry)" % (worst_fd, worst, tol))
    assert worst < tol, (worst, tol)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 3: the furnished room's loop of 4c with the texture painted on by world position: within 4c's bound, and no worse than depth alone
# ---------------------------------------------------------------------------------------------------------------------------------------------
def room_loop(oracle, t, n=ss.LOOP_FRAMES):
    """4c's track-and-fuse loop (tests/test_track.py cpu_loop) with every frame's painted picture fused and handed to the tracker."""
    op = oracle_params(oracle, ROOM_W, ROOM_H, 0.004)
    none = CAMERAS["same"]
    vol = oracle.Volume(op, threads=8)
    frames = ss.loop_frames(ROOM_W, ROOM_H)[:n]
    poses, results = [], []
    last = frames[0][1]
    for k, (d, truth) in enumerate(frames):
        rgb = ss.paint_room(d.reshape(-1), truth)
        if k == 0:
            pose, res = truth, None
        else:
            code, pose, res = cpu_track(vol.export(), op, d, last, t, colour=none, rgb=rgb)
            assert code == 0
        poses.append(pose)
        results.append(res)
        if res is None or res.tracked:
            vol.integrate(d, pose, rgb=rgb)
            last = pose
    blocks = vol.export()
    vol.close()
    return frames, poses, results, blocks


def _worst(frames, poses):
    errs = [ss.pose_error(p, truth) for p, (_, truth) in zip(poses[1:], frames[1:])]
    return max(e[0] for e in errs), max(e[1] for e in errs)


def test_checker_furnished_room_loop_with_colour(chk, oracle):
    frames, p0, r0, _ = room_loop(oracle, working_params(colour_weight=0.0))
    frames, p1, r1, _ = room_loop(oracle, working_params())
    assert all(r.tracked for r in r0[1:]) and all(r.tracked for r in r1[1:]), [res_tuple(r) for r in r1[1:] if not r.tracked]
    (t0, a0), (t1, a1) = _worst(frames, p0), _worst(frames, p1)
    print("room loop: depth only worst %.2f mm / %.2f mrad, with colour %.2f mm / %.2f mrad (bound %.0f mm / %.0f mrad)" % (
        t0 * 1e3, a0 * 1e3, t1 * 1e3, a1 * 1e3, LOOP_T_BOUND * 1e3, LOOP_R_BOUND * 1e3))
    assert min(r.colour_correspondences for r in r1[1:]) > 1000
    assert t1 < LOOP_T_BOUND and a1 < LOOP_R_BOUND, (t1, a1)
    assert t1 <= t0 and a1 <= a0, ((t0, a0), (t1, a1))   # colour does not make the loop worse than depth alone


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 4: the checker says what it was recorded to say, a picture at colour_weight 0 leaves the depth term's bits alone; a model miss gives no colour row
# ---------------------------------------------------------------------------------------------------------------------------------------------
TRACK_CASES = [n for n in ss.CASE_NAMES if n.startswith("track-")]


@pytest.mark.parametrize("name", TRACK_CASES)
def test_checker_reproduces_the_recorded_digests(chk, oracle, name):
    """tests/golden/solver_checker.json holds what the checker said on each case when it was recorded (first by the separate depth-only and colour
    checkers that tests/track_checker.c replaced).  A depth-only case is run without a picture and with a random picture at weight 0: both must give
    the recorded first 29 sums, masks, poses and depth fields of the result."""
    want = json.load(open(ss.GOLDEN))["cases"][name]
    got = ss.run_case(name, oracle)
    assert got["inputs"] == want["inputs"], "%s: the case's INPUTS differ from the recorded ones (the scene, not the checker, changed)" % name
    assert got["outputs"] == want["outputs"], name
    if "-depth-" in name:
        idle = ss.run_case(name, oracle, idle_picture=True)
        assert idle["inputs"] == want["inputs"] and idle["outputs"] == want["outputs"], name


def test_a_model_miss_gives_no_colour_row(chk, oracle):
    """A patch of the wall that no fused frame saw renders as a miss (colour 0, 0, 0): depth correspondences whose taps touch it get no colour row, so
    the black of a miss never enters a residual."""
    w = Wall(oracle, "same", hole=True)
    t = working_params()
    md, mn, mrgb = cpu_model(w.blocks, w.op, w.guess, t)
    miss = ~((md > 0) & (mn[..., 0] > -np.inf))   # k_track_model's validity
    assert miss[45:65, 70:90].all() and (mrgb[~(md > 0)] == 0).all() and not miss[5:30, 5:150].any()
    code, rows = ss.cpu_track_rows(w.op, w.depth, w.rgb, (md, mn, mrgb), 0, w.guess, w.guess, t, w.colour)
    assert code == 0
    code, sys, mask = cpu_system(w.blocks, w.op, w.depth, 0, w.guess, w.guess, t, colour=w.colour, rgb=w.rgb, model=(md, mn, mrgb))
    assert code == 0 and sys[30] == (rows[:, 0] > 0).sum() > 1000
    has = (rows[:, 0] > 0).reshape(H, W)
    # the estimate is the reference pose, so every pixel projects onto itself and its taps are itself and its right, lower and lower-right neighbours
    # (or the pixel before, where the projection rounds down): a pixel with a valid model pixel right beside the hole is a depth correspondence whose
    # taps need the intensity or the gradient of a missing pixel
    ring = miss_ring(miss)
    print("hole: %d model pixels miss, %d depth correspondences beside them, %d of those with a colour row; %d colour rows elsewhere" % (
        miss.sum(), (mask > 0)[ring].sum(), has[ring].sum(), has[~ring].sum()))
    assert (mask > 0)[ring].sum() > 50 and not has[ring].any()
    far = ~miss & ~miss_ring(miss | ring) & ~ring
    assert has[far & (mask > 0)].mean() > 0.5   # away from the hole most correspondences keep their row (the image's border and the two gates take the rest)


def miss_ring(miss):
    """Pixels one step outside the miss region whose own model pixel is valid: one of their taps' gradients needs a missing neighbour."""
    grown = miss.copy()
    grown[1:, :] |= miss[:-1, :]
    grown[:-1, :] |= miss[1:, :]
    grown[:, 1:] |= miss[:, :-1]
    grown[:, :-1] |= miss[:, 1:]
    return grown & ~miss


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 5: parameters, layouts, refusals, resources
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_colour_params_default():
    from scannet_amd import fusion
    t = fusion.default_track_params()
    assert (t.colour_weight, t.colour_thres, t.colour_gradient_min) == (0.0, np.float32(0.1), np.float32(0.005))
    assert list(t.reserved) == [0] * 5
    assert fusion.TRACK_COLOUR_WEIGHT > 0
    r = fusion.SfTrackResult()
    assert r.as_dict()["colour_correspondences"] == 0 and r.as_dict()["colour_rms_residual"] == 0.0


REFUSED = [("negative_weight", dict(colour_weight=-1.0), True), ("nan_weight", dict(colour_weight=float("nan")), True),
           ("inf_weight", dict(colour_weight=float("inf")), True), ("negative_threshold", dict(colour_weight=1.0, colour_thres=-0.1), True),
           ("nan_threshold", dict(colour_weight=1.0, colour_thres=float("nan")), True), ("inf_gradient", dict(colour_weight=1.0, colour_gradient_min=float("inf")), True),
           ("negative_gradient", dict(colour_weight=1.0, colour_gradient_min=-0.1), True), ("no_picture", dict(colour_weight=1.0), False)]


@pytest.mark.parametrize("name,over,with_rgb", REFUSED)
def test_refused_colour_arguments(name, over, with_rgb):
    """Arguments are checked before the fuser is looked at, so a NULL fuser tells a refused argument (-1 with its own message) from a passed one."""
    from scannet_amd import fusion
    L = _abi.lib()
    L.sf_last_error.restype = C.c_char_p
    vp = C.c_void_p
    args = [vp, vp, vp, vp, vp, C.POINTER(fusion.SfTrackParams), vp, C.POINTER(fusion.SfTrackResult)]
    L.sf_fuser_track_rgbd.argtypes = args
    L.sf_fuser_track_rgbd_device.argtypes = args
    t = working_params(**over)
    depth, rgb = np.zeros(16, np.uint16), np.zeros(48, np.uint8)
    pose, out, res = np.eye(4, dtype=np.float32).reshape(16), np.zeros(16, np.float32), fusion.SfTrackResult()
    for fn in (L.sf_fuser_track_rgbd, L.sf_fuser_track_rgbd_device):
        assert fn(None, _p(depth), _p(rgb) if with_rgb else None, _p(pose), None, C.byref(t), _p(out), C.byref(res)) == SF_ERR_INVALID_ARG
        assert b"colour" in L.sf_last_error(), L.sf_last_error()
    # the same call passes the argument checks once the parameters are good: the refusal that is left is the NULL fuser's
    good = working_params()
    assert L.sf_fuser_track_rgbd(None, _p(depth), _p(rgb), _p(pose), None, C.byref(good), _p(out), C.byref(res)) == SF_ERR_INVALID_ARG
    assert b"NULL fuser" in L.sf_last_error(), L.sf_last_error()
    # a NULL picture is allowed with weight 0
    off = working_params(colour_weight=0.0)
    assert L.sf_fuser_track_rgbd(None, _p(depth), None, _p(pose), None, C.byref(off), _p(out), C.byref(res)) == SF_ERR_INVALID_ARG
    assert b"NULL fuser" in L.sf_last_error(), L.sf_last_error()
    # the depth-only calls ignore the three fields
    L.sf_fuser_track.argtypes = [vp, vp, vp, vp, C.POINTER(fusion.SfTrackParams), vp, C.POINTER(fusion.SfTrackResult)]
    assert L.sf_fuser_track(None, _p(depth), _p(pose), None, C.byref(t), _p(out), C.byref(res)) == SF_ERR_INVALID_ARG
    assert b"NULL fuser" in L.sf_last_error(), L.sf_last_error()
    # the test hook checks in the same order
    L.sf_fuser_track_rgbd_system.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.POINTER(fusion.SfTrackParams), vp, vp]
    sys = np.zeros(31, np.float64)
    assert L.sf_fuser_track_rgbd_system(None, _p(depth), _p(rgb) if with_rgb else None, 0, _p(pose), _p(pose), C.byref(t), _p(sys), None) == SF_ERR_INVALID_ARG
    assert b"colour" in L.sf_last_error(), L.sf_last_error()


def test_colour_structs_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sf_track_params), offsetof(sf_track_params, raycast), offsetof(sf_track_params, colour_weight),
         offsetof(sf_track_params, colour_thres), offsetof(sf_track_params, colour_gradient_min), offsetof(sf_track_params, reserved), sizeof(sf_track_result),
         offsetof(sf_track_result, lost_reason), offsetof(sf_track_result, colour_correspondences), offsetof(sf_track_result, colour_rms_residual),
         offsetof(sf_track_result, reserved));
  return 0;
}'''
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = str(tmp_path / "tkc_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    from scannet_amd import fusion
    P, R = fusion.SfTrackParams, fusion.SfTrackResult
    assert got == [C.sizeof(P), P.raycast.offset, P.colour_weight.offset, P.colour_thres.offset, P.colour_gradient_min.offset, P.reserved.offset, C.sizeof(R),
                   R.lost_reason.offset, R.colour_correspondences.offset, R.colour_rms_residual.offset, R.reserved.offset]
    # the sizes and the offsets of what was there before the colour term took its fields from `reserved`
    assert got[0] == 164 and got[1] == 68 and got[2] == 132 and got[6] == 56 and got[7] == 28 and got[8] == 32
    # the checker's tk_params: the leading fields, sf_raycast_params as 16 words, the three floats
    assert C.sizeof(fusion.SfRaycastParams) == 64


def test_depthsensing_refuses_track_colour_without_track_and_without_colour_frames(tmp_path):
    if not os.path.exists(TOOL):
        pytest.skip("bin/depthsensing is built by build()")
    (tmp_path / "p.txt").write_text("s_SDFVoxelSize = 0.010f;\n")
    (tmp_path / "t.txt").write_text("s_maxLevels = 3;\n")
    base = [str(tmp_path / "p.txt"), str(tmp_path / "t.txt")]
    for flags in (["--track-colour"], ["--track-colour=0.5"]):
        r = subprocess.run([TOOL] + base + [str(tmp_path / "none.sens")] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--track-colour" in r.stderr and "--track" in r.stderr.replace("--track-colour", ""), r.stderr
    for bad in ("--track-colour=-1", "--track-colour=x", "--track-colour=nan", "--track-colour="):
        r = subprocess.run([TOOL] + base + [str(tmp_path / "none.sens"), "--track", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--track-colour" in r.stdout, (bad, r.stdout)   # the usage line names the flag
    # a file without colour frames is refused before the GPU is touched; the text names both flags
    r = subprocess.run([TOOL] + base + [ss.plain_sens(tmp_path, False), "--track", "--track-colour"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--track-colour" in r.stderr and "--track" in r.stderr.replace("--track-colour", "") and "colour frames" in r.stderr, r.stderr


def test_track_photo_kernels_live_in_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kr = ss.kernel_resources()
    rows = kr.kernels(os.path.join(ROOT, "scannet_amd", "libscanfuse.so"))
    every = {kr.short(n): r for r, n in zip(rows, kr.demangle([r["name"] for r in rows]))}
    # the colour term's own kernels, and both instantiations of the tracker's two (track.hip: <false> the depth term alone, <true> with the colour row)
    mine = {s: r for s, r in every.items() if s.startswith("k_track_photo_") or s.split("<")[0] in ("k_track_assoc", "k_track_final")}
    assert set(mine) == {"k_track_photo_in0", "k_track_photo_model0", "k_track_photo_down", "k_track_photo_grad", "k_track_assoc<false>", "k_track_assoc<true>",
                         "k_track_final<false>", "k_track_final<true>"}
    assert sorted(s for s in every if "assoc" in s and "track" in s) == ["k_track_assoc<false>", "k_track_assoc<true>"]
    for s, r in mine.items():
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (s, r)
        assert r["lds"] <= 160 * 1024, (s, r["lds"])
    assert mine["k_track_assoc<false>"]["lds"] == 464           # the cross-wave step of 29 sums
    assert mine["k_track_assoc<true>"]["lds"] == 4 * 31 * 4     # and of 31


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fused_wall(wall):
    """A fuser holding the wall's fused frames; the checker reads its exported blocks."""
    from scannet_amd import fusion
    f = fusion.Fuser(ss.fuser_params(W, H, wall.colour, VOXEL), device=0)
    for d, c, p in wall.fused:
        assert f.integrate(d, p, rgb=c)
    f.sync()
    return f


@pytest.fixture(scope="module")
def gpu_wall(wall):
    f = fused_wall(wall)
    yield f, f.export_blocks()
    f.close()


@pytest.mark.gpu
def test_gpu_volume_is_the_oracles(wall, gpu_wall):
    f, blocks = gpu_wall
    assert np.array_equal(blocks[0], wall.blocks[0]) and blocks[1].tobytes() == wall.blocks[1].tobytes()


@pytest.mark.gpu
def test_gpu_rgbd_system_bit_exact_every_level(chk, wall, gpu_wall):
    """All 31 sums and the mask at every level of 160 x 120 with four levels (19 200, 4 800 -- 18.75 workgroups, the last one partial --, 1 200 and 300
    pixels).  The second estimate is 9 level-0 pixels and 30 mrad off the reference, so a band of pixels projects outside the model image and another
    onto its last row and column: the float range test of the taps."""
    f, blocks = gpu_wall
    t = working_params(levels=4)
    estimates = [("near", ss.left_increment(wall.guess, 0.6 * FOOT0, -0.3 * FOOT0, 0.001)), ("outside", ss.left_increment(wall.guess, 9.0 * FOOT0, -7.5 * FOOT0, 0.03))]
    model = cpu_model(blocks, wall.op, wall.guess, t)
    for name, T in estimates:
        for level in range(t.levels):
            code, want, wmask = cpu_system(blocks, wall.op, wall.depth, level, T, wall.guess, t, colour=wall.colour, rgb=wall.rgb, model=model)
            got, gmask = f.track_system(wall.depth, level, T, wall.guess, t, mask=True, rgb=wall.rgb)
            assert code == 0 and np.array_equal(gmask, wmask), (name, level, int((gmask != wmask).sum()))
            assert got.tobytes() == want.tobytes(), (name, level, got, want)
            assert want[28] > 100 and want[30] > 50, (name, level, want[28], want[30])
            if name == "outside":
                assert want[28] < 0.97 * wmask.size, (level, want[28])


@pytest.mark.gpu
def test_gpu_rgbd_track_bit_exact_and_leaves_the_volume_alone(wall, wall_cpu, gpu_wall):
    f, blocks = gpu_wall
    (pose0, res0), (pose1, res1) = wall_cpu
    before, st0 = ss.volume_digest(f), f.stats()
    pose, res = f.track(wall.depth, wall.guess, params=working_params(), rgb=wall.rgb)
    assert res_tuple(res) == res_tuple(res1), (res_tuple(res), res_tuple(res1))
    assert res.tracked == 1 and pose.tobytes() == pose1.tobytes()
    assert in_plane_error(pose, wall.truth) <= BOUND
    lost, res = f.track(wall.depth, wall.guess, params=working_params(colour_weight=0.0), rgb=wall.rgb)
    assert lost is None and res_tuple(res) == res_tuple(res0) and res.lost_reason == 3
    assert ss.volume_digest(f) == before and f.stats() == st0


@pytest.mark.gpu
def test_gpu_rgbd_device_equals_host_and_weight_zero_equals_the_depth_only_call(wall, gpu_wall, oracle):
    import torch
    from scannet_amd import fusion
    f, _ = gpu_wall
    d = torch.from_numpy(wall.depth.astype(np.int16)).to("cuda:0")
    c = torch.from_numpy(wall.rgb).to("cuda:0")
    torch.cuda.synchronize()
    t = working_params()
    p1, r1 = f.track_device(d, wall.guess, params=t, d_rgb=c)
    p0, r0 = f.track(wall.depth, wall.guess, params=t, rgb=wall.rgb)
    assert r0.tracked == 1 and p1.tobytes() == p0.tobytes() and res_tuple(r1) == res_tuple(r0)
    # weight 0 on a scene depth can solve: the room's corner, with and without a picture, against sf_fuser_track
    gp = ss.fuser_params(ROOM_W, ROOM_H, ss.NO_COLOUR, 0.004, num_sdf_blocks=1 << 18)   # 4c's fuser (tests/test_track.py params_pair)
    with fusion.Fuser(gp, device=0) as g:
        frames = ss.corner_frames(ROOM_W, ROOM_H)
        rng = np.random.default_rng(3)
        for dd, p in frames:   # fused with colour: a model without colour renders black, which has no gradient and so no colour row
            assert g.integrate(dd, p, rgb=rng.integers(0, 256, ROOM_W * ROOM_H * 3, dtype=np.uint8))
        depth, truth = frames[0]
        guess = ss.perturb(truth, 0.02, deg=2.0)
        off = fusion.default_track_params()
        want, wres = g.track(depth, guess, ref=truth, params=off)
        rgb = rng.integers(0, 256, ROOM_W * ROOM_H * 3, dtype=np.uint8)
        for picture in (rgb, None):
            if picture is None:
                L = _abi.lib()
                vp = C.c_void_p
                L.sf_fuser_track_rgbd.argtypes = [vp, vp, vp, vp, vp, C.POINTER(fusion.SfTrackParams), vp, C.POINTER(fusion.SfTrackResult)]
                out, res = np.empty(16, np.float32), fusion.SfTrackResult()
                dd, gg, rr = np.ascontiguousarray(depth, np.uint16), guess.reshape(16).copy(), truth.reshape(16).copy()
                assert L.sf_fuser_track_rgbd(g._h, _p(dd), None, _p(gg), _p(rr), C.byref(off), _p(out), C.byref(res)) == 0
                got = out.reshape(4, 4)
                assert res.colour_correspondences == 0
            else:
                got, res = g.track(depth, guess, ref=truth, params=off, rgb=picture)
                assert res.colour_correspondences > 0
            assert wres.tracked == 1 and got.tobytes() == want.tobytes() and res_tuple(res)[:5] == res_tuple(wres)[:5]
        for level in range(off.levels):
            s29 = g.track_system(depth, level, guess, truth, off)
            s31 = g.track_system(depth, level, guess, truth, off, rgb=rgb)
            assert s31[:29].tobytes() == s29.tobytes() and s31[30] > 0


@pytest.mark.gpu
def test_gpu_work_set_states(chk, wall):
    """One fuser's tracking buffers through their states, each answer equal to a fresh fuser's: a colour call after a depth-only call, then a colour
    call with more levels (the set is made again), then a depth-only call."""
    T = ss.left_increment(wall.guess, 0.6 * FOOT0, -0.3 * FOOT0, 0.001)
    steps = [(2, 1, False), (2, 1, True), (4, 3, True), (2, 0, False), (3, 2, True)]
    f = fused_wall(wall)
    try:
        for step, (levels, level, colour) in enumerate(steps):
            t = working_params(levels=levels)
            got = f.track_system(wall.depth, level, T, wall.guess, t, mask=True, rgb=wall.rgb if colour else None)
            g = fused_wall(wall)
            try:
                want = g.track_system(wall.depth, level, T, wall.guess, t, mask=True, rgb=wall.rgb if colour else None)
            finally:
                g.close()
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), (step, got[0], want[0])
            assert want[0][28] > 100 and (not colour or want[0][30] > 50), (step, want[0])
    finally:
        f.close()


WALK = 6


@pytest.mark.gpu
def test_gpu_track_and_fuse_with_colour_reproduces_the_cpu_chain(chk, oracle):
    from scannet_amd import fusion
    colour = CAMERAS["narrow"]
    op = oracle_params(oracle)
    t = working_params()
    truth = [walk_pose(k, 0.002 * k) for k in range(WALK)]
    frames = [render(p, colour) for p in truth]
    vol = oracle.Volume(op, threads=8)
    cpu, last = [], truth[0]
    for k, (d, c) in enumerate(frames):
        if k == 0:
            pose = truth[0]
        else:
            code, pose, res = cpu_track(vol.export(), op, d, last, t, colour=colour, rgb=c)
            assert code == 0 and res.tracked == 1, (k, res.as_dict())
        vol.integrate(d, pose, rgb=under_the_depth_rays(c, colour))
        cpu.append(pose)
        last = pose
    coords, vox = vol.export()
    vol.close()
    with fusion.Fuser(ss.fuser_params(W, H, colour, VOXEL), device=0) as f:
        poses, results = fusion.track_and_fuse(f, frames, truth[0], with_colour=True)
        f.sync()
        for k in range(1, WALK):
            assert results[k]["tracked"] and results[k]["colour_correspondences"] > 0, (k, results[k])
            assert poses[k].tobytes() == np.asarray(cpu[k], np.float32).tobytes(), k
        gc, gv = f.export_blocks()
        assert np.array_equal(gc, coords) and gv.tobytes() == vox.tobytes()
    with fusion.Fuser(ss.fuser_params(W, H, colour, VOXEL), device=0) as f:   # the same walk without colour loses every frame after the first
        poses, results = fusion.track_and_fuse(f, frames, truth[0])
        assert [r["lost_reason"] for r in results[1:]] == [3] * (WALK - 1)


@pytest.mark.gpu
def test_gpu_depthsensing_track_colour(tmp_path):
    from scannet_amd import sens
    K = synth.intrinsic_matrix(W, H)
    sd = sens.SensorData.create(W, H, W, H, K, K, sensor_name="StructureSensor")
    truth = [walk_pose(k, 0.002 * k) for k in range(WALK)]
    for i, p in enumerate(truth):
        d, c = render(p, CAMERAS["same"])
        sd.add_frame(d, p if i == 0 else np.eye(4, dtype=np.float32), color=c, timestamp_depth=i)   # the converter's identity poses after frame 0
    path = str(tmp_path / "wall.sens")
    sd.save(path)
    sd.close()
    params = tmp_path / "zParametersScanNet.txt"
    params.write_text("s_SDFVoxelSize = 0.008f;\ns_hashNumSDFBlocks = 65536;\ns_hashNumBuckets = 100000;\n")
    tracking = tmp_path / "zParametersTrackingDefault.txt"
    tracking.write_text("s_maxLevels = 3;\n")
    out_sens = tmp_path / "tracked.sens"
    r = subprocess.run([TOOL, str(params), str(tracking), path, "--track", "--track-colour", "--write-sens=%s" % out_sens], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = re.search(r"Tracked (\d+) frames, lost (\d+)", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (WALK - 1, 0), r.stdout
    got = sens.SensorData(str(out_sens))
    assert len(got.frames) == WALK and all(np.isfinite(fr.camera_to_world).all() for fr in got.frames)
    got.close()
    r = subprocess.run([TOOL, str(params), str(tracking), path, "--track"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = re.search(r"Tracked (\d+) frames, lost (\d+)", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (0, WALK - 1), r.stdout
