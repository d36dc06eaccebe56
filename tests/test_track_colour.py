"""The dense colour term of the camera tracker (DESIGN.md "The colour term of the tracker", 4g; scannet_amd/csrc/track_colour.hip).

The rule is pinned as section 4c's is: tests/track_colour_checker.c restates it in C (the depth term with it), the oracle fuses, tests/raycast_checker.c
renders the model's depth, normals and colour.
  * without a GPU: a frame sliding along one textured wall, which depth alone loses (lost_reason 3), is tracked to sub-pixel accuracy with colour; the
    analytic row against a float64 finite difference; the furnished room's loop with a painted texture stays within 4c's bound and is no worse than
    its depth-only run; colour_weight 0 equals tests/track_checker.c byte for byte; a model miss gives no colour row; parameters, struct layouts, the
    tool's refusals, the kernels' resources;
  * -m gpu: sf_fuser_track_rgbd_system and sf_fuser_track_rgbd against the checker bit for bit, the device entry point, the work set's states,
    track_and_fuse(with_colour=True), bin/depthsensing --track --track-colour.
"""
import ctypes as C
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "depthsensing")
SF_ERR_INVALID_ARG = -1


def _load(name):
    spec = importlib.util.spec_from_file_location(name + "_scene", os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tt = _load("test_track")          # the CPU chain's helpers, the furnished room's loop, 4c's bounds
ac = _load("test_align_colour")   # the textured wall, its colour camera, the room's paint

W, H = ac.W, ac.H                 # 160 x 120
VOXEL = 0.008
FOOT0 = ac.WALL_Z / ac.FX         # metres of wall under one level-0 pixel: 13.8 mm
BOUND = 0.5 * FOOT0               # test 1's bound: half a level-0 pixel's footprint, the sampling limit
STEP = (0.03, 0.008)              # the walk along the wall, metres per frame
FUSED = 4                         # frames fused before the tracked one
TURN = 0.004                      # the tracked frame's turn about the wall's normal, radians
CAMERAS = {"narrow": (ac.CW, ac.CH, ac.CFX, ac.CFY, ac.CMX, ac.CMY), "same": (0, 0, 0.0, 0.0, 0.0, 0.0)}


def walk_pose(k, rz=0.0):
    return ac.wall_pose(STEP[0] * k, STEP[1] * k, rz)


def render(pose, colour):
    """(u16 depth [H*W], RGB8 picture at the colour camera's size, or at the depth camera's own when the fuser has no colour camera)."""
    if colour[0]:
        return ac.render_wall(pose, W, H, None, colour[0], colour[1], colour[2:])
    return ac.render_wall(pose, W, H, None, W, H, (ac.FX, ac.FY, ac.MX, ac.MY))


def under_the_depth_rays(rgb, colour):
    """What the fuser's pre-pass looks up for a picture of a colour camera (nearest pixel under the depth pixel's ray, black outside), for the oracle,
    which takes colour at the depth size: tests/test_gpu_tsdf.py::test_colour_at_its_own_resolution."""
    if not colour[0]:
        return rgb
    cw, ch, cfx, cfy, cmx, cmy = colour
    f32 = np.float32
    xs, ys = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    u = (((xs - f32(ac.MX)) / f32(ac.FX)).astype(np.float64) * np.float64(f32(cfx)) + np.float64(f32(cmx))).astype(f32) + f32(0.5)
    v = (((ys - f32(ac.MY)) / f32(ac.FY)).astype(np.float64) * np.float64(f32(cfy)) + np.float64(f32(cmy))).astype(f32) + f32(0.5)
    ok = (u >= 0) & (u < cw) & (v >= 0) & (v < ch)
    iu, iv = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
    return np.where(ok[..., None], rgb.reshape(ch, cw, 3)[iv, iu], 0).astype(np.uint8).reshape(-1)


def oracle_params(oracle, w=W, h=H, voxel=VOXEL):
    op = oracle.default_params(w, h, voxel)
    op.fx, op.fy, op.mx, op.my = synth.intrinsics(w, h)
    return op


def working_params(**over):
    """The defaults with the working weight of `--track-colour`."""
    from scannet_amd import fusion
    return fusion.default_track_params(**dict(dict(colour_weight=fusion.TRACK_COLOUR_WEIGHT), **over))


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    """(ray-cast checker, colour track checker)."""
    if shutil.which("gcc") is None or not tt._has_fma():
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    from scannet_amd import fusion
    rc = tt._compile(tmp_path_factory, "raycast_checker")
    rc.rc_raycast.restype = C.c_int64
    rc.rc_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(tt.RcArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    tk = tt._compile(tmp_path_factory, "track_colour_checker")
    FP, PP, RP, vp = C.POINTER(ac.AlcFrame), C.POINTER(fusion.SfTrackParams), C.POINTER(fusion.SfTrackResult), C.c_void_p
    tk.tkc_system.argtypes = [FP, vp, vp, vp, vp, vp, PP, C.c_int, vp, vp, vp, vp]
    tk.tkc_track.argtypes = [FP, vp, vp, vp, vp, vp, PP, vp, vp, vp, RP]
    tk.tkc_maps.argtypes = [FP, vp, vp, vp, vp, vp, PP, C.c_int, vp, vp, vp, vp]
    tk.tkc_rows.argtypes = [FP, vp, vp, vp, vp, vp, PP, C.c_int, vp, vp, vp]
    return rc, tk


def frame_of(op, colour):
    return ac.AlcFrame(op.width, op.height, op.width, op.height, op.fx, op.fy, op.mx, op.my, op.depth_shift, op.depth_min, op.depth_max, *colour)


def cpu_model(rc, blocks, op, pose, t):
    """The model the tracker casts at `pose`: raycast_checker.c at the integration size, depth, normals and colour."""
    r = t.raycast
    a = tt.RcArgs(op.width, op.height, op.fx, op.fy, op.mx, op.my, r.depth_min, r.depth_max, r.ray_increment_factor, r.thres_sample_dist_factor,
                  r.thres_dist_factor, r.refine_iters, op.voxel_size, op.trunc_base)
    depth = np.empty((op.height, op.width), np.float32)
    nrm = np.empty((op.height, op.width, 3), np.float32)
    rgb = np.empty((op.height, op.width, 3), np.uint8)
    coords, vox = np.ascontiguousarray(blocks[0], np.int32), np.ascontiguousarray(blocks[1])
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    rc.rc_raycast(coords.ctypes.data, vox.ctypes.data, len(coords), C.byref(a), p.ctypes.data, depth.ctypes.data, nrm.ctypes.data, rgb.ctypes.data)
    return depth, nrm, rgb


def _p(a):
    return None if a is None else a.ctypes.data


def cpu_track(chk, blocks, op, colour, depth, rgb, guess, t, ref=None):
    """The whole tracker with the colour term on the CPU over exported blocks -> (rc, pose [4,4] f32, SfTrackResult)."""
    from scannet_amd import fusion
    rc, tk = chk
    md, mn, mrgb = cpu_model(rc, blocks, op, guess if ref is None else ref, t)
    d = np.ascontiguousarray(depth, np.uint16)
    c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
    g = np.ascontiguousarray(guess, np.float32).reshape(16)
    rf = None if ref is None else np.ascontiguousarray(ref, np.float32).reshape(16)
    out = np.empty(16, np.float32)
    res = fusion.SfTrackResult()
    code = tk.tkc_track(C.byref(frame_of(op, colour)), _p(d), _p(c), _p(md), _p(mn), None if c is None else _p(mrgb), C.byref(t), _p(g), _p(rf), _p(out),
                        C.byref(res))
    return code, out.reshape(4, 4), res


def cpu_system(chk, blocks, op, colour, depth, rgb, level, T, Tref, t, model=None):
    rc, tk = chk
    md, mn, mrgb = model or cpu_model(rc, blocks, op, Tref, t)
    d = np.ascontiguousarray(depth, np.uint16)
    c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
    sys = np.zeros(31, np.float64)
    mask = np.zeros((op.height >> level, op.width >> level), np.uint8)
    T = np.ascontiguousarray(T, np.float32).reshape(16)
    Tref = np.ascontiguousarray(Tref, np.float32).reshape(16)
    code = tk.tkc_system(C.byref(frame_of(op, colour)), _p(d), _p(c), _p(md), _p(mn), None if c is None else _p(mrgb), C.byref(t), level, _p(T), _p(Tref),
                         _p(sys), _p(mask))
    return code, sys, mask


def res_tuple(r):
    """Every field of sf_track_result."""
    return (int(r.tracked), tuple(r.iterations), int(r.correspondences), np.float32(r.rms_residual).tobytes(), int(r.lost_reason),
            int(r.colour_correspondences), np.float32(r.colour_rms_residual).tobytes())


def in_plane_error(pose, truth):
    return float(np.hypot(*(np.asarray(pose, np.float64)[:2, 3] - np.asarray(truth, np.float64)[:2, 3])))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The wall: FUSED frames sliding along it are fused with colour; the next frame lies one step (3 cm) further and is turned TURN about the normal
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Wall:
    def __init__(self, oracle, camera, hole=False):
        self.colour = CAMERAS[camera]
        self.op = oracle_params(oracle)
        self.fused = []
        vol = oracle.Volume(self.op, threads=8)
        for k in range(FUSED):
            d, c = render(walk_pose(k), self.colour)
            if hole:   # a patch the sensor did not see: the model misses there
                d = d.reshape(H, W).copy()
                d[40:70, 60:100] = 0
                d = d.reshape(-1)
            self.fused.append((d, c, walk_pose(k)))
            vol.integrate(d, walk_pose(k), rgb=under_the_depth_rays(c, self.colour))
        self.blocks = vol.export()
        vol.close()
        self.truth = walk_pose(FUSED, TURN)
        self.guess = walk_pose(FUSED - 1)
        self.depth, self.rgb = render(self.truth, self.colour)


@pytest.fixture(scope="module", params=sorted(CAMERAS))
def wall(request, oracle):
    return Wall(oracle, request.param)


@pytest.fixture(scope="module")
def wall_cpu(chk, wall):
    """The checker's answers on the wall, without and with colour (shared with the GPU tests)."""
    a0 = cpu_track(chk, wall.blocks, wall.op, wall.colour, wall.depth, wall.rgb, wall.guess, working_params(colour_weight=0.0))
    a1 = cpu_track(chk, wall.blocks, wall.op, wall.colour, wall.depth, wall.rgb, wall.guess, working_params())
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
    et, er = tt.pose_error(pose1, wall.truth)
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
    rc, tk = chk
    t = working_params()
    level = 1
    fr = frame_of(wall.op, wall.colour)
    md, mn, mrgb = cpu_model(rc, wall.blocks, wall.op, wall.guess, t)
    T = ac.left_increment(wall.guess, 0.7 * FOOT0, -0.4 * FOOT0, 0.002)
    T32, R32 = np.ascontiguousarray(T, np.float32).reshape(16), np.ascontiguousarray(wall.guess, np.float32).reshape(16)
    wl, hl = W >> level, H >> level
    npx = wl * hl
    rows = np.zeros((npx, 8), np.float32)
    d, c = np.ascontiguousarray(wall.depth, np.uint16), np.ascontiguousarray(wall.rgb, np.uint8)
    assert tk.tkc_rows(C.byref(fr), _p(d), _p(c), _p(md), _p(mn), _p(mrgb), C.byref(t), level, _p(T32), _p(R32), _p(rows)) == 0
    vmap, pm, cam = np.zeros((npx, 3), np.float32), np.zeros((npx, 3), np.float32), np.zeros(6, np.float32)
    assert tk.tkc_maps(C.byref(fr), _p(d), _p(c), _p(md), _p(mn), _p(mrgb), C.byref(t), level, _p(R32), _p(vmap), _p(pm), _p(cam)) == 0
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
                dd[k] = (float(g @ (project(ac._inc(e, Td), v) - u0)) - float(g @ (project(ac._inc(-e, Td), v) - u0))) / (2 * h)
            fd[h] = dd
        worst_fd = max(worst_fd, np.abs(fd[1e-4] - fd[5e-5]).max() / scale)
        worst = max(worst, np.abs(fd[5e-5] - J).max() / scale)
    tol = 10.0 * max(worst_fd, 6e-7)
    print("colour row: finite-difference error %.2e, analytic row against it %.2e, tolerance %.2e (relative to the row's largest entry)" % (worst_fd, worst, tol))
    assert worst < tol, (worst, tol)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 3: the furnished room's loop of 4c with the texture painted on by world position: within 4c's bound, and no worse than depth alone
# ---------------------------------------------------------------------------------------------------------------------------------------------
def room_loop(chk, oracle, t, n=tt.LOOP_FRAMES):
    """4c's track-and-fuse loop (tests/test_track.py cpu_loop) with every frame's painted picture fused and handed to the tracker."""
    op = oracle_params(oracle, tt.W, tt.H, 0.004)
    none = CAMERAS["same"]
    vol = oracle.Volume(op, threads=8)
    frames = tt.loop_frames()[:n]
    poses, results = [], []
    last = frames[0][1]
    for k, (d, truth) in enumerate(frames):
        rgb = ac.paint_room(d.reshape(-1), truth)
        if k == 0:
            pose, res = truth, None
        else:
            code, pose, res = cpu_track(chk, vol.export(), op, none, d, rgb, last, t)
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
    errs = [tt.pose_error(p, truth) for p, (_, truth) in zip(poses[1:], frames[1:])]
    return max(e[0] for e in errs), max(e[1] for e in errs)


def test_checker_furnished_room_loop_with_colour(chk, oracle):
    frames, p0, r0, _ = room_loop(chk, oracle, working_params(colour_weight=0.0))
    frames, p1, r1, _ = room_loop(chk, oracle, working_params())
    assert all(r.tracked for r in r0[1:]) and all(r.tracked for r in r1[1:]), [res_tuple(r) for r in r1[1:] if not r.tracked]
    (t0, a0), (t1, a1) = _worst(frames, p0), _worst(frames, p1)
    print("room loop: depth only worst %.2f mm / %.2f mrad, with colour %.2f mm / %.2f mrad (bound %.0f mm / %.0f mrad)" % (
        t0 * 1e3, a0 * 1e3, t1 * 1e3, a1 * 1e3, tt.LOOP_T_BOUND * 1e3, tt.LOOP_R_BOUND * 1e3))
    assert min(r.colour_correspondences for r in r1[1:]) > 1000
    assert t1 < tt.LOOP_T_BOUND and a1 < tt.LOOP_R_BOUND, (t1, a1)
    assert t1 <= t0 and a1 <= a0, ((t0, a0), (t1, a1))   # colour does not make the loop worse than depth alone


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU 4: colour_weight 0 through the colour path is tests/track_checker.c byte for byte; a model miss gives no colour row
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_weight_zero_equals_the_depth_only_checker(chk, oracle, tmp_path_factory):
    from scannet_amd import fusion
    old = tt._compile(tmp_path_factory, "track_checker")
    old.tk_system.argtypes = [C.POINTER(tt.TkFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fusion.SfTrackParams), C.c_int, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]
    old.tk_track.argtypes = [C.POINTER(tt.TkFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fusion.SfTrackParams), C.c_void_p, C.c_void_p, C.c_void_p,
                             C.POINTER(tt.TkResult)]
    # the room's corner (three planes: solvable by depth) at 160 x 120 with a random picture at the colour camera's own size
    op = oracle_params(oracle, W, H, VOXEL)
    vol = oracle.Volume(op, threads=8)
    poses = [tt.corner_truth(), tt.look_at((1.7, 1.2, 1.45), (0.05, 0.0, 0.0)), tt.look_at((1.5, 1.4, 1.35), (0.0, 0.05, 0.05))]
    rng = np.random.default_rng(5)
    for p in poses:
        vol.integrate(synth.render_room_depth(p, W, H), p, rgb=rng.integers(0, 256, W * H * 3, dtype=np.uint8))
    blocks = vol.export()
    vol.close()
    depth = synth.render_room_depth(poses[0], W, H)
    rgb = rng.integers(0, 256, ac.CH * ac.CW * 3, dtype=np.uint8)
    colour = CAMERAS["narrow"]
    t = fusion.default_track_params()
    assert t.colour_weight == 0.0
    guess = tt.perturb(poses[0], 0.02, 2.0)
    code, pose, res = cpu_track(chk, blocks, op, colour, depth, rgb, guess, t, ref=poses[0])
    md, mn, _ = cpu_model(chk[0], blocks, op, poses[0], t)
    fr_old = tt.TkFrame(W, H, W, H, op.fx, op.fy, op.mx, op.my, op.depth_shift, op.depth_min, op.depth_max)
    d, g, rf = np.ascontiguousarray(depth, np.uint16), guess.reshape(16).copy(), poses[0].reshape(16).copy()
    want, want_res = np.empty(16, np.float32), tt.TkResult()
    assert old.tk_track(C.byref(fr_old), _p(d), _p(md), _p(mn), C.byref(t), _p(g), _p(rf), _p(want), C.byref(want_res)) == 0
    assert code == 0 and res.tracked == 1 and sum(res.iterations) > 3
    assert pose.tobytes() == want.tobytes()
    assert res_tuple(res)[:5] == tt.res_tuple(want_res)
    assert res.colour_correspondences > 0   # the rows were formed and weighed 0
    for level in range(t.levels):
        code, sys31, mask31 = cpu_system(chk, blocks, op, colour, depth, rgb, level, guess, poses[0], t)
        sys29, mask29 = np.zeros(29, np.float64), np.zeros_like(mask31)
        assert old.tk_system(C.byref(fr_old), _p(d), _p(md), _p(mn), C.byref(t), level, _p(g), _p(rf), _p(sys29), _p(mask29)) == 0
        assert code == 0 and sys31[:29].tobytes() == sys29.tobytes() and np.array_equal(mask31, mask29) and sys31[30] > 0, level
        # without a picture no colour row is formed
        code, sysn, _ = cpu_system(chk, blocks, op, colour, depth, None, level, guess, poses[0], t)
        assert code == 0 and sysn[:29].tobytes() == sys29.tobytes() and sysn[29] == 0.0 and sysn[30] == 0.0


def test_a_model_miss_gives_no_colour_row(chk, oracle):
    """A patch of the wall that no fused frame saw renders as a miss (colour 0, 0, 0): depth correspondences whose taps touch it get no colour row, so
    the black of a miss never enters a residual."""
    rc, tk = chk
    w = Wall(oracle, "same", hole=True)
    t = working_params()
    md, mn, mrgb = cpu_model(rc, w.blocks, w.op, w.guess, t)
    miss = ~((md > 0) & (mn[..., 0] > -np.inf))   # k_track_model's validity
    assert miss[45:65, 70:90].all() and (mrgb[~(md > 0)] == 0).all() and not miss[5:30, 5:150].any()
    fr = frame_of(w.op, w.colour)
    rows = np.zeros((W * H, 8), np.float32)
    d, c = np.ascontiguousarray(w.depth, np.uint16), np.ascontiguousarray(w.rgb, np.uint8)
    g = np.ascontiguousarray(w.guess, np.float32).reshape(16)
    assert tk.tkc_rows(C.byref(fr), _p(d), _p(c), _p(md), _p(mn), _p(mrgb), C.byref(t), 0, _p(g), _p(g), _p(rows)) == 0
    code, sys, mask = cpu_system(chk, w.blocks, w.op, w.colour, w.depth, w.rgb, 0, w.guess, w.guess, t, model=(md, mn, mrgb))
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
    r = subprocess.run([TOOL] + base + [ac._plain_sens(tmp_path, False), "--track", "--track-colour"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--track-colour" in r.stderr and "--track" in r.stderr.replace("--track-colour", "") and "colour frames" in r.stderr, r.stderr


def test_track_photo_kernels_live_in_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernels(os.path.join(ROOT, "scannet_amd", "libscanfuse.so"))
    mine = {kr.short(n): r for r, n in zip(rows, kr.demangle([r["name"] for r in rows])) if kr.short(n).startswith("k_track_photo_")}
    assert set(mine) == {"k_track_photo_in0", "k_track_photo_model0", "k_track_photo_down", "k_track_photo_grad", "k_track_photo_assoc", "k_track_photo_final"}
    for s, r in mine.items():
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (s, r)
        assert r["lds"] <= 160 * 1024, (s, r["lds"])
    assert mine["k_track_photo_assoc"]["lds"] == 4 * 31 * 4   # the cross-wave step of 31 sums


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _volume_digest(f):
    c, v = f.export_blocks()
    return hashlib.sha256(c.tobytes() + v.tobytes()).hexdigest()


def fused_wall(wall):
    """A fuser holding the wall's fused frames; the checker reads its exported blocks."""
    from scannet_amd import fusion
    f = fusion.Fuser(ac.fuser_params(W, H, wall.colour, VOXEL), device=0)
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
    estimates = [("near", ac.left_increment(wall.guess, 0.6 * FOOT0, -0.3 * FOOT0, 0.001)), ("outside", ac.left_increment(wall.guess, 9.0 * FOOT0, -7.5 * FOOT0, 0.03))]
    model = cpu_model(chk[0], blocks, wall.op, wall.guess, t)
    for name, T in estimates:
        for level in range(t.levels):
            code, want, wmask = cpu_system(chk, blocks, wall.op, wall.colour, wall.depth, wall.rgb, level, T, wall.guess, t, model=model)
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
    before, st0 = _volume_digest(f), f.stats()
    pose, res = f.track(wall.depth, wall.guess, params=working_params(), rgb=wall.rgb)
    assert res_tuple(res) == res_tuple(res1), (res_tuple(res), res_tuple(res1))
    assert res.tracked == 1 and pose.tobytes() == pose1.tobytes()
    assert in_plane_error(pose, wall.truth) <= BOUND
    lost, res = f.track(wall.depth, wall.guess, params=working_params(colour_weight=0.0), rgb=wall.rgb)
    assert lost is None and res_tuple(res) == res_tuple(res0) and res.lost_reason == 3
    assert _volume_digest(f) == before and f.stats() == st0


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
    op, gp = tt.params_pair(oracle)
    with fusion.Fuser(gp, device=0) as g:
        frames = tt.corner_frames()
        rng = np.random.default_rng(3)
        for dd, p in frames:   # fused with colour: a model without colour renders black, which has no gradient and so no colour row
            assert g.integrate(dd, p, rgb=rng.integers(0, 256, tt.W * tt.H * 3, dtype=np.uint8))
        depth, truth = frames[0]
        guess = tt.perturb(truth, 0.02, 2.0)
        off = fusion.default_track_params()
        want, wres = g.track(depth, guess, ref=truth, params=off)
        rgb = rng.integers(0, 256, tt.W * tt.H * 3, dtype=np.uint8)
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
    T = ac.left_increment(wall.guess, 0.6 * FOOT0, -0.3 * FOOT0, 0.001)
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
            code, pose, res = cpu_track(chk, vol.export(), op, colour, d, c, last, t)
            assert code == 0 and res.tracked == 1, (k, res.as_dict())
        vol.integrate(d, pose, rgb=under_the_depth_rays(c, colour))
        cpu.append(pose)
        last = pose
    coords, vox = vol.export()
    vol.close()
    with fusion.Fuser(ac.fuser_params(W, H, colour, VOXEL), device=0) as f:
        poses, results = fusion.track_and_fuse(f, frames, truth[0], with_colour=True)
        f.sync()
        for k in range(1, WALK):
            assert results[k]["tracked"] and results[k]["colour_correspondences"] > 0, (k, results[k])
            assert poses[k].tobytes() == np.asarray(cpu[k], np.float32).tobytes(), k
        gc, gv = f.export_blocks()
        assert np.array_equal(gc, coords) and gv.tobytes() == vox.tobytes()
    with fusion.Fuser(ac.fuser_params(W, H, colour, VOXEL), device=0) as f:   # the same walk without colour loses every frame after the first
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
