"""What the tests of the tracker and of the global alignment share (tests/test_track.py, test_track_colour.py, test_align.py, test_align_colour.py):
pose helpers, the two CPU checkers (tests/track_checker.c and tests/align_checker.c over tests/solver_rules.h, with tests/raycast_checker.c casting
the tracker's model) compiled once per session, the CPU chains built on them, and the scenes.  tests/golden/make_solver_checker_golden.py records
what the checkers say on the cases at the end of this file; the two colour modules hold the checkers to the record.
"""
import atexit
import ctypes as C
import functools
import hashlib
import importlib.util
import os
import shutil
import subprocess
import tempfile

import numpy as np

from scannet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_COLOUR = (0, 0, 0.0, 0.0, 0.0, 0.0)   # no colour camera: pictures are at the integration camera's own size


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Poses
# ---------------------------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target):
    """camToWorld of a camera at eye looking at target, world z up, image y down."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m.astype(np.float32)


def perturb(pose, dt, *, deg=None, rad=None, axis=(0.3, -0.5, 0.8), tdir=(0.6, 0.64, -0.48)):
    """pose moved dt metres along tdir and turned about axis (world frame, left increment); the angle is named: deg= degrees or rad= radians."""
    assert (deg is None) != (rad is None), "one of deg=, rad="
    th = np.radians(deg) if rad is None else rad
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    out = np.eye(4)
    out[:3, :3] = R @ pose[:3, :3].astype(np.float64)
    out[:3, 3] = R @ pose[:3, 3].astype(np.float64) + dt * np.asarray(tdir, np.float64) / np.linalg.norm(tdir)
    return out.astype(np.float32)


def pose_error(a, b):
    """(translation metres, rotation radians) between two camToWorld poses ([4,4] or [16])."""
    a, b = np.asarray(a, np.float64).reshape(4, 4), np.asarray(b, np.float64).reshape(4, 4)
    dt = float(np.linalg.norm(a[:3, 3] - b[:3, 3]))
    c = (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0) / 2.0
    return dt, float(np.arccos(np.clip(c, -1.0, 1.0)))


def worst_pose_error(out, truth):
    e = [pose_error(o, t) for o, t in zip(out, truth)]
    return max(x[0] for x in e), max(x[1] for x in e)


def in_plane_error(pose, truth):
    """The distance in the wall's plane (world x, y) between a pose and its truth, metres."""
    return float(np.hypot(*(np.asarray(pose, np.float64).reshape(4, 4)[:2, 3] - np.asarray(truth, np.float64).reshape(4, 4)[:2, 3])))


def worst_in_plane_error(out, truth):
    return max(in_plane_error(o, t) for o, t in zip(out, truth))


def rodrigues(w):
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx


def increment(xi, T):
    """exp(xi) T in float64: the solvers' left increment."""
    out = np.eye(4)
    R = rodrigues(xi[:3])
    out[:3, :3] = R @ T[:3, :3]
    out[:3, 3] = R @ T[:3, 3] + xi[3:]
    return out


def random_poses(n, seed, spread=1.5, turn=0.7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        w = rng.normal(size=3)
        w *= rng.uniform(0, turn) / np.linalg.norm(w)
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
        m = np.eye(4)
        m[:3, :3] = R
        m[:3, 3] = rng.uniform(-spread, spread, 3)
        out.append(m)
    return np.stack(out).astype(np.float32)


f32 = np.float32


def volume_digest(f):
    c, v = f.export_blocks()
    return hashlib.sha256(c.tobytes() + v.tobytes()).hexdigest()


def kernel_resources():
    """tools/kernel_resources.py as a module."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr


def plain_sens(tmp_path, colour):
    """A two-frame 16 x 12 .sens with or without colour frames, for the tool's refusals."""
    from scannet_amd import sens
    w, h = 16, 12
    K = synth.intrinsic_matrix(w, h)
    sd = sens.SensorData.create(w if colour else 0, h if colour else 0, w, h, K, K, sensor_name="StructureSensor")
    for i in range(2):
        sd.add_frame(np.full(w * h, 1500, np.uint16), np.eye(4, dtype=np.float32), color=np.zeros(w * h * 3, np.uint8) if colour else None, timestamp_depth=i)
    path = str(tmp_path / ("colour.sens" if colour else "grey.sens"))
    sd.save(path)
    sd.close()
    return path


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The checkers: compiled once per session
# ---------------------------------------------------------------------------------------------------------------------------------------------
def has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def checkers_available():
    """The checkers need gcc and a CPU with fused multiply-add (fmaf must be one instruction)."""
    return shutil.which("gcc") is not None and has_fma()


class RcArgs(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
                ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("ray_increment_factor", C.c_float), ("thres_sample_dist_factor", C.c_float), ("thres_dist_factor", C.c_float),
                ("refine_iters", C.c_int32), ("voxel_size", C.c_float), ("trunc_base", C.c_float)]


class Frame(C.Structure):
    """sr_frame of tests/solver_rules.h."""
    _fields_ = [("in_w", C.c_int32), ("in_h", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
                ("depth_shift", C.c_float), ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("color_w", C.c_int32), ("color_h", C.c_int32), ("cfx", C.c_float), ("cfy", C.c_float), ("cmx", C.c_float), ("cmy", C.c_float)]


@functools.lru_cache(maxsize=None)
def _build_dir():
    d = tempfile.mkdtemp(prefix="solver_checkers_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def compile_checker(name):
    """tests/<name>.c as a shared library."""
    so = os.path.join(_build_dir(), "lib%s.so" % name)
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", name + ".c"), "-lm"], check=True)
    return C.CDLL(so)


@functools.lru_cache(maxsize=None)
def raycast_lib():
    rc = compile_checker("raycast_checker")
    rc.rc_raycast.restype = C.c_int64
    rc.rc_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(RcArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return rc


@functools.lru_cache(maxsize=None)
def track_lib():
    from scannet_amd import fusion
    tk = compile_checker("track_checker")
    FP, PP, RP, vp = C.POINTER(Frame), C.POINTER(fusion.SfTrackParams), C.POINTER(fusion.SfTrackResult), C.c_void_p
    tk.tk_system.argtypes = [FP, vp, vp, vp, vp, vp, PP, C.c_int, vp, vp, vp, vp]
    tk.tk_track.argtypes = [FP, vp, vp, vp, vp, vp, PP, vp, vp, vp, RP]
    tk.tk_maps.argtypes = [FP, vp, vp, vp, vp, vp, PP, C.c_int, vp, vp, vp, vp]
    tk.tk_rows.argtypes = [FP, vp, vp, vp, vp, vp, PP, C.c_int, vp, vp, vp]
    return tk


@functools.lru_cache(maxsize=None)
def align_lib():
    from scannet_amd import fusion
    al = compile_checker("align_checker")
    FP, PP, RP, vp = C.POINTER(Frame), C.POINTER(fusion.SfAlignParams), C.POINTER(fusion.SfAlignResult), C.c_void_p
    al.al_system.argtypes = [FP, vp, vp, C.c_int64, vp, vp, C.c_int64, PP, vp]
    al.al_align.argtypes = [FP, vp, vp, C.c_int64, vp, vp, C.c_int64, PP, vp, RP]
    al.al_maps.argtypes = [FP, vp, vp, C.c_int64, C.c_int64, PP, vp, vp, vp]
    al.al_rows.argtypes = [FP, vp, vp, C.c_int64, vp, C.c_int32, C.c_int32, PP, vp]
    al.al_pairs.argtypes = [vp, C.c_int64, PP, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    al.al_spread.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, vp]
    return al


def ptr(a):
    return None if a is None else a.ctypes.data


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The tracker's CPU chain: the oracle fuses, raycast_checker.c casts the model, track_checker.c tracks
# ---------------------------------------------------------------------------------------------------------------------------------------------
def oracle_params(oracle, w, h, voxel):
    op = oracle.default_params(w, h, voxel)
    op.fx, op.fy, op.mx, op.my = synth.intrinsics(w, h)
    return op


def track_frame(op, colour=NO_COLOUR):
    return Frame(op.width, op.height, op.width, op.height, op.fx, op.fy, op.mx, op.my, op.depth_shift, op.depth_min, op.depth_max, *colour)


def blocks_of(vol):
    """An oracle volume's blocks, or (coords, voxels) as given (a fuser's export_blocks())."""
    return vol.export() if hasattr(vol, "export") else vol


def cpu_model(vol, op, pose, t):
    """The model the tracker casts at `pose`: raycast_checker.c at the integration size -> (depth, world normals, RGB8 colour)."""
    r = t.raycast
    a = RcArgs(op.width, op.height, op.fx, op.fy, op.mx, op.my, r.depth_min, r.depth_max, r.ray_increment_factor, r.thres_sample_dist_factor,
               r.thres_dist_factor, r.refine_iters, op.voxel_size, op.trunc_base)
    depth = np.empty((op.height, op.width), np.float32)
    nrm = np.empty((op.height, op.width, 3), np.float32)
    rgb = np.empty((op.height, op.width, 3), np.uint8)
    coords, vox = blocks_of(vol)
    coords, vox = np.ascontiguousarray(coords, np.int32), np.ascontiguousarray(vox)
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    raycast_lib().rc_raycast(coords.ctypes.data, vox.ctypes.data, len(coords), C.byref(a), p.ctypes.data, depth.ctypes.data, nrm.ctypes.data, rgb.ctypes.data)
    return depth, nrm, rgb


def missed_model(op):
    """The model of a reference pose that is not finite: nothing to cast, every pixel a miss."""
    return (np.full((op.height, op.width), -np.inf, np.float32), np.full((op.height, op.width, 3), -np.inf, np.float32),
            np.zeros((op.height, op.width, 3), np.uint8))


def cpu_track(vol, op, depth, guess, t, ref=None, colour=NO_COLOUR, rgb=None, model=None):
    """The whole tracker on the CPU over an oracle volume or exported blocks; rgb: the frame's picture or None (no colour rows).
    -> (code, pose [4,4] f32, SfTrackResult)."""
    from scannet_amd import fusion
    md, mn, mrgb = model or cpu_model(vol, op, guess if ref is None else ref, t)
    d = np.ascontiguousarray(depth, np.uint16)
    c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
    g = np.ascontiguousarray(guess, np.float32).reshape(16)
    rf = None if ref is None else np.ascontiguousarray(ref, np.float32).reshape(16)
    out = np.empty(16, np.float32)
    res = fusion.SfTrackResult()
    code = track_lib().tk_track(C.byref(track_frame(op, colour)), ptr(d), ptr(c), ptr(md), ptr(mn), None if c is None else ptr(mrgb), C.byref(t), ptr(g), ptr(rf),
                                ptr(out), C.byref(res))
    return code, out.reshape(4, 4), res


def cpu_system(vol, op, depth, level, T, Tref, t, colour=NO_COLOUR, rgb=None, model=None):
    """One level's 31 sums and its correspondence mask -> (code, sys [31] f64, mask)."""
    md, mn, mrgb = model or cpu_model(vol, op, Tref, t)
    d = np.ascontiguousarray(depth, np.uint16)
    c = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
    sys = np.zeros(31, np.float64)
    mask = np.zeros((op.height >> level, op.width >> level), np.uint8)
    T = np.ascontiguousarray(T, np.float32).reshape(16)
    Tref = np.ascontiguousarray(Tref, np.float32).reshape(16)
    code = track_lib().tk_system(C.byref(track_frame(op, colour)), ptr(d), ptr(c), ptr(md), ptr(mn), None if c is None else ptr(mrgb), C.byref(t), level, ptr(T),
                                 ptr(Tref), ptr(sys), ptr(mask))
    return code, sys, mask


def cpu_track_maps(op, depth, rgb, model, level, Tref, t, colour=NO_COLOUR):
    """tk_maps -> (code, vmap [npx,3], the model's {I, gx, gy} [npx,3], cam [6])."""
    md, mn, mrgb = model
    npx = (op.width >> level) * (op.height >> level)
    vmap, pm, cam = np.zeros((npx, 3), np.float32), np.zeros((npx, 3), np.float32), np.zeros(6, np.float32)
    d, c = np.ascontiguousarray(depth, np.uint16), None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
    R = np.ascontiguousarray(Tref, np.float32).reshape(16)
    code = track_lib().tk_maps(C.byref(track_frame(op, colour)), ptr(d), ptr(c), ptr(md), ptr(mn), ptr(mrgb), C.byref(t), level, ptr(R), ptr(vmap), ptr(pm), ptr(cam))
    return code, vmap, pm, cam


def cpu_track_rows(op, depth, rgb, model, level, T, Tref, t, colour=NO_COLOUR):
    """tk_rows -> (code, rows [npx,8]: {has a colour row, r_c, J_c[6]})."""
    md, mn, mrgb = model
    rows = np.zeros(((op.width >> level) * (op.height >> level), 8), np.float32)
    d, c = np.ascontiguousarray(depth, np.uint16), None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
    T, R = np.ascontiguousarray(T, np.float32).reshape(16), np.ascontiguousarray(Tref, np.float32).reshape(16)
    code = track_lib().tk_rows(C.byref(track_frame(op, colour)), ptr(d), ptr(c), ptr(md), ptr(mn), ptr(mrgb), C.byref(t), level, ptr(T), ptr(R), ptr(rows))
    return code, rows


def track_res_tuple(r):
    """Every field of sf_track_result; the first five are the depth term's."""
    return (int(r.tracked), tuple(r.iterations), int(r.correspondences), np.float32(r.rms_residual).tobytes(), int(r.lost_reason),
            int(r.colour_correspondences), np.float32(r.colour_rms_residual).tobytes())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The aligner on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------
def align_frame(w, h, intr=None, colour=NO_COLOUR):
    from scannet_amd import fusion
    p = fusion.default_params(depth_width=w, depth_height=h)
    fx, fy, mx, my = intr or synth.intrinsics(w, h)
    return Frame(w, h, w, h, fx, fy, mx, my, p.depth_shift, p.depth_min, p.depth_max, *colour)


def fuser_params(w, h, colour=NO_COLOUR, voxel=0.008, num_sdf_blocks=1 << 16):
    from scannet_amd import fusion
    fx, fy, mx, my = synth.intrinsics(w, h)
    extra = dict(color_width=colour[0], color_height=colour[1], cfx=colour[2], cfy=colour[3], cmx=colour[4], cmy=colour[5]) if colour[0] else {}
    return fusion.default_params(depth_width=w, depth_height=h, voxel_size=voxel, fx=fx, fy=fy, mx=mx, my=my, num_sdf_blocks=num_sdf_blocks, **extra)


def align_arrays(depth, rgb, poses, pairs):
    depth = np.ascontiguousarray(depth, np.uint16)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return depth, rgb, poses, pairs


def cpu_align(depth, poses, pairs, a, fr, rgb=None):
    """The whole alignment on the CPU; rgb: K pictures or None (no colour rows) -> (code, poses [K,16], SfAlignResult)."""
    from scannet_amd import fusion
    depth, rgb, poses, pairs = align_arrays(depth, rgb, poses, pairs)
    out = np.empty_like(poses)
    res = fusion.SfAlignResult()
    rc = align_lib().al_align(C.byref(fr), ptr(depth), ptr(rgb), len(poses), ptr(poses), ptr(pairs), len(pairs), C.byref(a), ptr(out), C.byref(res))
    return rc, out, res


def cpu_align_system(depth, poses, pairs, a, fr, rgb=None):
    """The per-pair systems -> (code, sys [P,31] f64)."""
    depth, rgb, poses, pairs = align_arrays(depth, rgb, poses, pairs)
    sys = np.zeros((len(pairs), 31), np.float64)
    rc = align_lib().al_system(C.byref(fr), ptr(depth), ptr(rgb), len(poses), ptr(poses), ptr(pairs), len(pairs), C.byref(a), ptr(sys))
    return rc, sys


def cpu_align_maps(depth, rgb, poses, k, a, fr):
    """al_maps of frame k -> (code, vmap [npx,3], {I, gx, gy} [npx,3], cam [6]); npx is the level's that `a` chooses."""
    depth, rgb, poses, _ = align_arrays(depth, rgb, poses, [[0, 1]])
    npx = fr.W * fr.H   # room for level 0
    vmap, pmap, cam = np.zeros((npx, 3), np.float32), np.zeros((npx, 3), np.float32), np.zeros(6, np.float32)
    rc = align_lib().al_maps(C.byref(fr), ptr(depth), ptr(rgb), len(poses), k, C.byref(a), ptr(vmap), ptr(pmap), ptr(cam))
    n = int(cam[0]) * int(cam[1])
    return rc, vmap[:n], pmap[:n], cam


def cpu_align_rows(depth, rgb, poses, i, j, a, fr):
    """al_rows of the pair (i, j) -> (code, rows [W*H of level 0, 8]; the level's npx rows come first)."""
    depth, rgb, poses, _ = align_arrays(depth, rgb, poses, [[0, 1]])
    rows = np.zeros((fr.W * fr.H, 8), np.float32)
    rc = align_lib().al_rows(C.byref(fr), ptr(depth), ptr(rgb), len(poses), ptr(poses), i, j, C.byref(a), ptr(rows))
    return rc, rows


def align_res_tuple(r):
    """Every field of sf_align_result; the first eight are the depth term's."""
    return (int(r.status), int(r.iterations), int(r.pairs_used), int(r.frames_unconnected), int(r.frames_rejected), int(r.correspondences),
            np.float32(r.rms_first).tobytes(), np.float32(r.rms_last).tobytes(), int(r.colour_correspondences),
            np.float32(r.colour_rms_first).tobytes(), np.float32(r.colour_rms_last).tobytes())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The room: its corner at the origin (two walls and the floor, about 2.5 m away), the furnished walk
# ---------------------------------------------------------------------------------------------------------------------------------------------
CORNER_EYE, CORNER_TARGET = (1.6, 1.3, 1.4), (0.0, 0.0, 0.0)
WALK_TOTAL = 1200                  # the walk's 12 m perimeter in 1200 frames: 1 cm per frame
LOOP_FRAMES = 30
DRIFT_T, DRIFT_R = 0.008, 0.004    # injected per keyframe: metres, radians


def corner_truth():
    return look_at(CORNER_EYE, CORNER_TARGET)


def corner_poses():
    """The truth and two nearby views."""
    return [corner_truth(), look_at((1.7, 1.2, 1.45), (0.05, 0.0, 0.0)), look_at((1.5, 1.4, 1.35), (0.0, 0.05, 0.05))]


def corner_frames(w, h):
    """The three views of the corner, noise free: [(depth, pose)]."""
    return [(synth.render_room_depth(p, w, h), p) for p in corner_poses()]


def loop_frames(w, h):
    """The first LOOP_FRAMES frames of the furnished room's walk, sensor noise 2: [(depth, true pose)]."""
    boxes = synth.clutter_boxes()
    out = []
    for i in range(LOOP_FRAMES):
        pose = synth.trajectory_pose(i, WALK_TOTAL)
        out.append((synth.render_room_depth(pose, w, h, noise_frame=i, noise=2, boxes=boxes), pose))
    return out


def drifted(truth):
    """Keyframe k starts k x (8 mm, 4 mrad) off the truth; keyframe 0 is true."""
    return np.stack([perturb(t, DRIFT_T * k, rad=DRIFT_R * k) if k else t for k, t in enumerate(truth)]).astype(np.float32)


def corner_arc(n, w, h, *, metres=None, radians=None):
    """n noise-free views of the corner on an arc about the vertical through it, centred on CORNER_EYE's azimuth and `metres` of arc or `radians` apart,
    all looking at the corner: (depth [n, h*w], truth [n,4,4], drifted start [n,4,4])."""
    assert (metres is None) != (radians is None), "one of metres=, radians="
    r, az0 = float(np.hypot(CORNER_EYE[0], CORNER_EYE[1])), float(np.arctan2(CORNER_EYE[1], CORNER_EYE[0]))
    az = [az0 + ((k - (n - 1) / 2) * metres / r if radians is None else (k - (n - 1) / 2) * radians) for k in range(n)]
    truth = [look_at((r * np.cos(a), r * np.sin(a), CORNER_EYE[2]), (0.0, 0.0, 0.0)) for a in az]
    depth = np.stack([synth.render_room_depth(p, w, h).reshape(-1) for p in truth])
    return depth, np.stack(truth), drifted(truth)


def structure_cases(corner, w, h):
    """name -> (depth [K, h*w], poses [K,16], pairs) from the 320 x 240 arc `corner`.  thin: frame 2 keeps a 20 x 20 patch of its depth, 100 pixels at
    level 1, so both its pairs fall below min_pair_correspondences = 500 and nothing connects it.  lost: frame 1 has the all -inf pose.  planes: two
    frames that each see one single plane."""
    depth, truth, start = corner
    thin = depth[:3].copy().reshape(3, h, w)
    keep = thin[2, 100:120, 150:170].copy()
    thin[2] = 0
    thin[2, 100:120, 150:170] = keep
    lost = start[:3].copy().reshape(3, 16)
    lost[1] = -np.inf
    star = np.array([[0, 1], [1, 0], [0, 2], [2, 0]], np.int32)
    plane = np.stack([synth.plane_frame(w, h).reshape(-1)] * 2)
    pp = np.stack([np.eye(4, dtype=np.float32), perturb(np.eye(4, dtype=np.float32), 0.01, rad=0.01)]).reshape(2, 16)
    return {"thin": (thin.reshape(3, -1), start[:3].reshape(3, 16), star),
            "lost": (depth[:3], lost, star),
            "planes": (plane, pp, np.array([[0, 1], [1, 0]], np.int32))}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The wall: a textured plane z = WALL_Z in the world, cameras at z = 0 looking along +z.  Depth and colour come per pixel from the ray-plane
# intersection; the colour camera has its own size and a narrower field, so the outer integration pixels have no colour.
# ---------------------------------------------------------------------------------------------------------------------------------------------
W, H = 160, 120
ALIGN_LEVEL = 1
WALL_Z = 2.0
FX, FY, MX, MY = synth.intrinsics(W, H)
FOOT = WALL_Z / (FX / (1 << ALIGN_LEVEL))    # metres of wall under one pixel of the aligner's level: 27.7 mm
FOOT0 = WALL_Z / FX                          # metres of wall under one level-0 pixel: 13.8 mm
CW, CH = 200, 150
NARROW = 1.12
CFX, CFY, CMX, CMY = FX * CW / W * NARROW, FY * CH / H * NARROW, (CW - 1) / 2.0, (CH - 1) / 2.0
WALL_CAMERA = (CW, CH, CFX, CFY, CMX, CMY)
CAMERAS = {"narrow": WALL_CAMERA, "same": NO_COLOUR}
# sinusoids in plane coordinates: wavelength in level pixels (16 .. 64), direction (radians), phase; one amplitude row per channel
WAVES = [(16.0, 0.3, 0.0), (24.0, 1.9, 1.0), (40.0, 2.6, 2.0), (64.0, 1.1, 4.0)]
AMPS = {"r": (0.06, 0.10, 0.12, 0.12), "g": (0.05, 0.12, 0.10, 0.14), "b": (0.10, 0.06, 0.14, 0.08)}
# in-plane start offsets in level pixels (at most 2) and turns about the wall's normal in radians, keyframes 1..; keyframe 0 is fixed at the truth
OFFSETS = [(2.0, -1.5, 0.004), (-1.7, 2.0, -0.006), (1.2, 1.8, 0.005), (-2.0, -0.8, 0.003), (0.9, -2.0, -0.004), (1.6, 1.1, 0.006), (-1.1, 1.7, -0.003)]


def texture(X, Y, scale=FOOT):
    """RGB in [0, 1] at plane coordinates (metres): [..., 3]."""
    out = []
    for ch in "rgb":
        v = np.full(np.shape(X), 0.5)
        for (lam, th, ph), a in zip(WAVES, AMPS[ch]):
            v = v + a * np.sin(2 * np.pi * (X * np.cos(th) + Y * np.sin(th)) / (lam * scale) + ph)
        out.append(v)
    return np.stack(out, -1)


def wall_pose(x, y, rz=0.0):
    """camToWorld of a camera at (x, y, 0) looking along +z, turned rz about z."""
    m = np.eye(4)
    m[:2, :2] = [[np.cos(rz), -np.sin(rz)], [np.sin(rz), np.cos(rz)]]
    m[:3, 3] = (x, y, 0.0)
    return m.astype(np.float32)


def _hits(pose, w, h, fx, fy, mx, my):
    """Ray-plane intersections of every pixel's ray with the wall: (range along the camera's z, world points)."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.stack([(xx - mx) / fx, (yy - my) / fy, np.ones((h, w))], -1)
    p = np.asarray(pose, np.float64)
    dw = d @ p[:3, :3].T
    s = (WALL_Z - p[2, 3]) / dw[..., 2]
    return s, p[:3, 3] + s[..., None] * dw


def render_wall(pose, w=W, h=H, intr=None, cw=CW, ch=CH, cintr=None):
    """(u16 depth in mm [h*w], RGB8 [ch*cw*3]) of the wall from `pose`."""
    fx, fy, mx, my = intr or (FX, FY, MX, MY)
    cfx, cfy, cmx, cmy = cintr or (CFX, CFY, CMX, CMY)
    s, _ = _hits(pose, w, h, fx, fy, mx, my)
    _, pts = _hits(pose, cw, ch, cfx, cfy, cmx, cmy)
    rgb = np.clip(np.rint(texture(pts[..., 0], pts[..., 1]) * 255.0), 0, 255).astype(np.uint8)
    return np.rint(s * 1000.0).astype(np.uint16).reshape(-1), rgb.reshape(-1)


def left_increment(pose, dx, dy, rz):
    """[Rz(rz) | (dx, dy, 0)] pose."""
    inc = wall_pose(dx, dy, rz).astype(np.float64)
    return (inc @ np.asarray(pose, np.float64)).astype(np.float32)


def wall_scene(K):
    """K keyframes sliding along the wall 5 cm apart: (depth [K, H*W], rgb [K, CH*CW*3], truth [K,4,4], start [K,4,4])."""
    truth = [wall_pose(0.05 * k, 0.012 * k) for k in range(K)]
    start = [truth[0]] + [left_increment(t, o[0] * FOOT, o[1] * FOOT, o[2]) for t, o in zip(truth[1:], OFFSETS)]
    frames = [render_wall(t) for t in truth]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack(truth), np.stack(start).astype(np.float32)


RW, RH = 320, 240


def paint_room(depth, pose):
    """RGB8 [RH*RW*3] at the depth camera's own pixels: the texture at each pixel's world position (two of its coordinates mixed, so that walls and
    floor all carry it)."""
    fx, fy, mx, my = synth.intrinsics(RW, RH)
    yy, xx = np.mgrid[0:RH, 0:RW]
    d = depth.reshape(RH, RW).astype(np.float64) / 1000.0
    cam = np.stack([(xx - mx) / fx * d, (yy - my) / fy * d, d], -1)
    p = np.asarray(pose, np.float64)
    wp = cam @ p[:3, :3].T + p[:3, 3]
    rgb = texture(wp[..., 0] + 0.7 * wp[..., 2], wp[..., 1] - 0.7 * wp[..., 2], scale=2.5 / (synth.intrinsics(RW, RH)[0] / 2))
    return np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8).reshape(-1)


SW, SH, SCW, SCH = 72, 56, 90, 70   # the small scene: level 0 is 4 032 pixels (a full last workgroup), level 1 36 x 28 = 1 008 (a partial one), level 2 18 x 14


def small_scene():
    """5 frames of the wall at 72 x 56 with 90 x 70 pictures and 12 pairs: both directions of neighbours; a pair whose projections reach the last row and
    column (frame 3 is up and left of frame 0, so frame 0's lower right pixels project onto frame 3's border taps); frame 4 has an all -inf pose;
    frames 0 and 2b (frame 2 turned to look away) share nothing."""
    intr = synth.intrinsics(SW, SH)
    cintr = (intr[0] * SCW / SW * NARROW * 0.93, intr[1] * SCH / SH * NARROW * 0.93, (SCW - 1) / 2.0, (SCH - 1) / 2.0)
    foot = WALL_Z / intr[0]
    truth = [wall_pose(0.0, 0.0), wall_pose(3.3 * foot, -1.2 * foot, 0.01), wall_pose(-2.4 * foot, 2.1 * foot, -0.02), wall_pose(-6.5 * foot, -5.5 * foot, 0.0),
             wall_pose(1.0 * foot, 1.0 * foot)]
    frames = [render_wall(t, SW, SH, intr, SCW, SCH, cintr) for t in truth]
    poses = np.stack(truth).astype(np.float32)
    poses[4] = -np.inf
    away = poses[2].copy()
    away[:3, 0] *= -1.0
    away[:3, 2] *= -1.0
    poses = np.concatenate([poses, away[None]])
    depth = np.stack([f[0] for f in frames] + [frames[2][0]])
    rgb = np.stack([f[1] for f in frames] + [frames[2][1]])
    pairs = np.array([[0, 1], [1, 0], [1, 2], [2, 1], [0, 2], [2, 0], [0, 3], [3, 0], [1, 3], [0, 4], [4, 1], [0, 5]], np.int32)
    return depth, rgb, poses, pairs, (SCW, SCH) + cintr


def resampled_scene():
    """Depth frames of 144 x 112 resampled by the fuser to 72 x 56, color_width 0: the pictures are 144 x 112, seen through the depth frames' camera.
    -> (depth, rgb, poses, pairs, fuser parameters, checker frame)."""
    from scannet_amd import fusion
    iw, ih, w, h = 144, 112, 72, 56
    intr = synth.intrinsics(iw, ih)
    foot = WALL_Z / intr[0]
    truth = [wall_pose(0.0, 0.0), wall_pose(4.2 * foot, -2.6 * foot, 0.01), wall_pose(-3.4 * foot, 3.1 * foot, -0.015)]
    frames = [render_wall(t, iw, ih, intr, iw, ih, intr) for t in truth]
    fx, fy = f32(intr[0]) * (f32(w) / f32(iw)), f32(intr[1]) * (f32(h) / f32(ih))          # fuser.hip's integration camera, in float
    mx, my = f32(intr[2]) * (f32(w - 1) / f32(iw - 1)), f32(intr[3]) * (f32(h - 1) / f32(ih - 1))
    p = fusion.default_params(depth_width=iw, depth_height=ih, voxel_size=0.008, fx=intr[0], fy=intr[1], mx=intr[2], my=intr[3], num_sdf_blocks=1 << 16,
                              integration_width=w, integration_height=h)
    fr = Frame(iw, ih, w, h, fx, fy, mx, my, p.depth_shift, p.depth_min, p.depth_max, iw, ih, intr[0], intr[1], intr[2], intr[3])
    pairs = np.array([[0, 1], [1, 0], [0, 2], [2, 1]], np.int32)
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack(truth).astype(np.float32), pairs, p, fr


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The tracker's wall: FUSED frames sliding along it are fused with colour; the next frame lies one step (3 cm) further and is turned TURN about the
# normal
# ---------------------------------------------------------------------------------------------------------------------------------------------
TRACK_VOXEL = 0.008
STEP = (0.03, 0.008)              # the walk along the wall, metres per frame
FUSED = 4                         # frames fused before the tracked one
TURN = 0.004                      # the tracked frame's turn about the wall's normal, radians


def walk_pose(k, rz=0.0):
    return wall_pose(STEP[0] * k, STEP[1] * k, rz)


def render_walk(pose, colour):
    """(u16 depth [H*W], RGB8 picture at the colour camera's size, or at the depth camera's own when the fuser has no colour camera)."""
    if colour[0]:
        return render_wall(pose, W, H, None, colour[0], colour[1], colour[2:])
    return render_wall(pose, W, H, None, W, H, (FX, FY, MX, MY))


def under_the_depth_rays(rgb, colour):
    """What the fuser's pre-pass looks up for a picture of a colour camera (nearest pixel under the depth pixel's ray, black outside), for the oracle,
    which takes colour at the depth size: tests/test_gpu_tsdf.py::test_colour_at_its_own_resolution."""
    if not colour[0]:
        return rgb
    cw, ch, cfx, cfy, cmx, cmy = colour
    xs, ys = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    u = (((xs - f32(MX)) / f32(FX)).astype(np.float64) * np.float64(f32(cfx)) + np.float64(f32(cmx))).astype(f32) + f32(0.5)
    v = (((ys - f32(MY)) / f32(FY)).astype(np.float64) * np.float64(f32(cfy)) + np.float64(f32(cmy))).astype(f32) + f32(0.5)
    ok = (u >= 0) & (u < cw) & (v >= 0) & (v < ch)
    iu, iv = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
    return np.where(ok[..., None], rgb.reshape(ch, cw, 3)[iv, iu], 0).astype(np.uint8).reshape(-1)


class TrackWall:
    def __init__(self, oracle, camera, hole=False):
        self.colour = CAMERAS[camera]
        self.op = oracle_params(oracle, W, H, TRACK_VOXEL)
        self.fused = []
        vol = oracle.Volume(self.op, threads=8)
        for k in range(FUSED):
            d, c = render_walk(walk_pose(k), self.colour)
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
        self.depth, self.rgb = render_walk(self.truth, self.colour)


def coloured_corner(oracle):
    """The room's corner (three planes: solvable by depth) at 160 x 120, fused with random colour, and a random picture at the colour camera's own size:
    (oracle parameters, blocks, the three poses, frame 0's depth, the picture, a guess 2 cm / 2 degrees off pose 0)."""
    op = oracle_params(oracle, W, H, TRACK_VOXEL)
    vol = oracle.Volume(op, threads=8)
    poses = corner_poses()
    rng = np.random.default_rng(5)
    for p in poses:
        vol.integrate(synth.render_room_depth(p, W, H), p, rgb=rng.integers(0, 256, W * H * 3, dtype=np.uint8))
    blocks = vol.export()
    vol.close()
    depth = synth.render_room_depth(poses[0], W, H)
    rgb = rng.integers(0, 256, CH * CW * 3, dtype=np.uint8)
    return op, blocks, poses, depth, rgb, perturb(poses[0], 0.02, deg=2.0)


def coloured_arc():
    """Three keyframes of the corner at 160 x 120 (solvable by depth) with random pictures at the colour camera's own size:
    (depth, rgb, drifted start, the default pairs)."""
    from scannet_amd import fusion
    depth, _, start = corner_arc(3, W, H, radians=0.06)
    rgb = np.random.default_rng(5).integers(0, 256, (3, CH * CW * 3), dtype=np.uint8)
    pairs, _ = fusion.align_pairs(start, fusion.default_align_params())
    return depth, rgb, start, pairs


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The recorded cases: what the two checkers say on small scenes, as digests (tests/golden/solver_checker.json, written by
# tests/golden/make_solver_checker_golden.py).  A "-depth-" case has no colour term: its outputs are the first 29 sums and the depth term's result
# fields, and they must not change when a picture is handed in at weight 0 (`idle_picture`).
# ---------------------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "solver_checker.json")


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, np.ndarray):
            h.update(np.ascontiguousarray(p).tobytes())
        elif isinstance(p, C.Structure):
            h.update(bytes(p))
        else:
            h.update(repr(p).encode())
    return h.hexdigest()


def _idle(shape):
    return np.random.default_rng(17).integers(0, 256, shape, dtype=np.uint8)


def _track_case(vol, op, depth, guess, t, ref=None, T=None, colour=NO_COLOUR, rgb=None, depth_only=False, model=None, systems=True, idle_picture=False):
    """Every level's system at T about the reference (for a colour case its maps and rows too) and the whole track from `guess`."""
    Tref = guess if ref is None else ref
    T = guess if T is None else T
    model = model or cpu_model(vol, op, Tref, t)
    fr = track_frame(op, colour)
    inputs = [np.asarray(depth), model[0], model[1], np.asarray(guess), np.asarray(Tref), np.asarray(T), t, fr]
    if not depth_only and rgb is not None:
        inputs += [np.asarray(rgb), model[2]]
    if depth_only and idle_picture:
        rgb = _idle(op.width * op.height * 3)
    out = {}
    for level in range(t.levels if systems else 0):
        code, sys, mask = cpu_system(vol, op, depth, level, T, Tref, t, colour, rgb, model)
        out["system_L%d" % level] = [code, sys[:29] if depth_only else sys, mask]
        if not depth_only:
            out["maps_L%d" % level] = list(cpu_track_maps(op, depth, rgb, model, level, Tref, t, colour))
            out["rows_L%d" % level] = list(cpu_track_rows(op, depth, rgb, model, level, T, Tref, t, colour))
    code, pose, res = cpu_track(vol, op, depth, guess, t, ref, colour, rgb, model)
    out["track"] = [code, pose, track_res_tuple(res)[:5] if depth_only else track_res_tuple(res)]
    return inputs, out


def _align_case(depth, poses, pairs, a, fr, rgb=None, depth_only=False, maps=(), rows=(), idle_picture=False):
    """The pairs' systems (for a colour case maps and rows too) and the whole alignment."""
    inputs = [np.asarray(depth), np.asarray(poses), np.asarray(pairs), a, fr] + ([] if depth_only or rgb is None else [np.asarray(rgb)])
    if depth_only and idle_picture:
        rgb = _idle((len(depth), fr.W * fr.H * 3))
    out = {}
    code, sys = cpu_align_system(depth, poses, pairs, a, fr, rgb)
    out["system"] = [code, sys[:, :29] if depth_only else sys]
    for k in maps:
        out["maps_%d" % k] = list(cpu_align_maps(depth, rgb, poses, k, a, fr))
    for i, j in rows:
        out["rows_%d_%d" % (i, j)] = list(cpu_align_rows(depth, rgb, poses, i, j, a, fr))
    code, new, res = cpu_align(depth, poses, pairs, a, fr, rgb)
    out["align"] = [code, new, align_res_tuple(res)[:8] if depth_only else align_res_tuple(res)]
    return inputs, out


@functools.lru_cache(maxsize=None)
def _corner_320(oracle):
    """tests/test_track.py's corner: three 320 x 240 views fused at 4 mm -> (oracle parameters, blocks, frame 0's depth)."""
    op = oracle_params(oracle, 320, 240, 0.004)
    vol = oracle.Volume(op, threads=8)
    frames = corner_frames(320, 240)
    for d, p in frames:
        vol.integrate(d, p)
    blocks = vol.export()
    vol.close()
    return op, blocks, frames[0][0]


@functools.lru_cache(maxsize=None)
def _track_wall(oracle, camera, hole):
    return TrackWall(oracle, camera, hole)


@functools.lru_cache(maxsize=None)
def _arc_320():
    return corner_arc(6, 320, 240, metres=0.1)


def _case_track_depth(which, oracle, idle_picture):
    from scannet_amd import fusion
    t = fusion.default_track_params()
    kw = dict(depth_only=True, idle_picture=idle_picture)
    if which == "corner160":
        op, blocks, poses, depth, _, guess = coloured_corner(oracle)
        return _track_case(blocks, op, depth, guess, t, ref=poses[0], **kw)
    if which == "single_plane":
        op = oracle_params(oracle, 320, 240, 0.004)
        vol = oracle.Volume(op, threads=8)
        plane, pose = synth.plane_frame(320, 240), np.eye(4, dtype=np.float32)
        vol.integrate(plane, pose)
        blocks = vol.export()
        vol.close()
        return _track_case(blocks, op, plane, perturb(pose, 0.01, deg=1.0), t, ref=pose, **kw)
    op, blocks, depth = _corner_320(oracle)
    truth = corner_truth()
    if which == "zero_depth":
        return _track_case(blocks, op, np.zeros_like(depth), truth, t, **kw)
    if which == "empty_volume":
        empty = oracle.Volume(op, threads=8)
        none = empty.export()
        empty.close()
        return _track_case(none, op, depth, truth, t, **kw)
    inputs, out = [], {}   # nonfinite: a guess, then a reference, with one entry NaN, inf, -inf; nothing is cast at such a reference
    model = cpu_model(blocks, op, truth, t)
    for bad in (np.nan, np.inf, -np.inf):
        g = truth.copy()
        g[1, 3] = bad
        for name, (guess, ref, m) in (("guess", (g, truth, model)), ("ref", (truth, g, missed_model(op)))):
            i, o = _track_case(blocks, op, depth, guess, t, ref=ref, model=m, systems=False, **kw)
            inputs += i
            out["%s_%r" % (name, float(bad))] = o["track"]
    return inputs, out


def _case_track_colour(wall, variant, oracle, idle_picture=False):
    from scannet_amd import fusion
    w = _track_wall(oracle, "same" if wall == "hole" else wall, wall == "hole")
    t = fusion.default_track_params(colour_weight=fusion.TRACK_COLOUR_WEIGHT if variant == "working" else 0.0)
    T = left_increment(w.guess, 0.6 * FOOT0, -0.3 * FOOT0, 0.001)
    return _track_case(w.blocks, w.op, w.depth, w.guess, t, T=T, colour=w.colour, rgb=None if variant == "no_picture" else w.rgb)


def _case_align_depth(which, oracle=None, idle_picture=False):
    from scannet_amd import fusion
    kw = dict(depth_only=True, idle_picture=idle_picture)
    if which.startswith("arc3_level"):
        depth, _, start, pairs = coloured_arc()
        return _align_case(depth, start, pairs, fusion.default_align_params(level=int(which[-1])), align_frame(W, H), **kw)
    fr = align_frame(320, 240)
    if which == "nothing_connected":
        depth, _, start = _arc_320()
        a = fusion.default_align_params(min_pair_correspondences=320 * 240)
        return _align_case(depth[:3], start[:3], np.array([[0, 1], [1, 2]], np.int32), a, fr, **kw)
    depth, poses, pairs = structure_cases(_arc_320(), 320, 240)[which]
    return _align_case(depth, poses, pairs, fusion.default_align_params(), fr, **kw)


def _case_pairs_spread(oracle=None, idle_picture=False):
    from scannet_amd import fusion
    a = fusion.default_align_params()
    poses = random_poses(40, 7).reshape(-1, 16)
    pairs = np.zeros((4096, 2), np.int32)
    n = C.c_uint64(0)
    rc = align_lib().al_pairs(ptr(poses), len(poses), C.byref(a), ptr(pairs), len(pairs), C.byref(n))
    old = random_poses(50, 11).reshape(-1, 16)
    keys = np.arange(2, 50, 7, dtype=np.uint64)
    new = random_poses(len(keys), 12).reshape(-1, 16)
    old[[0, 12, 23]] = -np.inf    # lost frames: before the first keyframe, between keyframes, a keyframe
    new[5] = np.nan                # a keyframe that came back without a pose
    spread = np.empty_like(old)
    rc2 = align_lib().al_spread(ptr(old), len(old), ptr(keys), len(keys), ptr(new), ptr(spread))
    return [poses, a, old, keys, new], {"pairs": [rc, int(n.value), pairs[:n.value]], "spread": [rc2, spread]}


def _case_align_colour(scene, variant, oracle=None, idle_picture=False):
    from scannet_amd import fusion
    over = {} if variant == "working" else dict(colour_weight=0.0)
    if scene == "wall4":
        depth, rgb, _, start = wall_scene(4)
        pairs, _ = fusion.align_pairs(start, fusion.default_align_params())
        a = fusion.default_align_params(**dict(dict(colour_weight=fusion.ALIGN_COLOUR_WEIGHT, level=ALIGN_LEVEL), **over))
        return _align_case(depth, start, pairs, a, align_frame(W, H, colour=WALL_CAMERA), rgb, maps=(0, 1), rows=((1, 0),))
    if scene.startswith("small_level"):
        depth, rgb, poses, pairs, colour = small_scene()
        a = fusion.default_align_params(**dict(dict(colour_weight=fusion.ALIGN_COLOUR_WEIGHT, level=int(scene[-1]), min_pair_correspondences=1), **over))
        return _align_case(depth, poses, pairs, a, align_frame(SW, SH, colour=colour), rgb, maps=(0, 3), rows=((0, 1), (0, 3)))
    depth, rgb, poses, pairs, _, fr = resampled_scene()
    a = fusion.default_align_params(**dict(dict(colour_weight=fusion.ALIGN_COLOUR_WEIGHT, level=0, min_pair_correspondences=1), **over))
    return _align_case(depth, poses, pairs, a, fr, rgb, maps=(0,), rows=((0, 1),))


def checker_cases():
    """name -> (case function, its arguments); every case function also takes oracle= and idle_picture= ("-depth-" cases alone look at the latter) and
    returns (input parts, {output name: parts})."""
    cases = {"align-depth-pairs_spread": (_case_pairs_spread,)}
    for which in ("corner160", "single_plane", "empty_volume", "zero_depth", "nonfinite"):
        cases["track-depth-" + which] = (_case_track_depth, which)
    for wall in ("narrow", "same", "hole"):
        for variant in ("working", "weight0", "no_picture"):
            cases["track-colour-%s-%s" % (wall, variant)] = (_case_track_colour, wall, variant)
    for which in ("arc3_level0", "arc3_level1", "arc3_level2", "thin", "lost", "planes", "nothing_connected"):
        cases["align-depth-" + which] = (_case_align_depth, which)
    for scene in ("wall4", "small_level0", "small_level1", "small_level2", "resampled"):
        for variant in ("working", "weight0"):
            cases["align-colour-%s-%s" % (scene, variant)] = (_case_align_colour, scene, variant)
    return cases


CASE_NAMES = sorted(checker_cases())


def run_case(name, oracle, idle_picture=False):
    """-> {"inputs": digest, "outputs": {name: digest}} of one case."""
    fn, *args = checker_cases()[name]
    inputs, outputs = fn(*args, oracle=oracle, idle_picture=idle_picture)
    return {"inputs": digest(inputs), "outputs": {k: digest(v) for k, v in sorted(outputs.items())}}
