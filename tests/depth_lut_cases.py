"""Shared by tests/test_depth_lut.py and tests/test_depth_lut_gpu.py: the CPU checker of the depth-distortion table (tests/depth_lut_checker.c,
DESIGN.md section 4k literally), synthetic plane sequences seen through the rule's pinhole, an independent float64 evaluation of the rule, and
the files the tool reads.  A case and its checker result are computed once per process and must not be modified by a test."""
import ctypes as C
import functools
import hashlib
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "depth_lut_checker.c")
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_lut_golden.json")


def have_checker():
    return shutil.which("gcc") is not None


@functools.lru_cache(maxsize=None)
def checker():
    d = tempfile.mkdtemp(prefix="depth_lut_checker_")
    so = os.path.join(d, "libdepth_lut_checker.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, CHECKER, "-lm"], check=True)
    L = C.CDLL(so)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.dl_filter.argtypes = [vp]
    L.dl_accumulate.argtypes = [vp, i, i, vp, vp, f, f, i, vp, vp]
    L.dl_accumulate.restype = None
    L.dl_finish.argtypes = [vp, vp, i, i, i, vp]
    L.dl_finish.restype = None
    L.dl_apply.argtypes = [vp, i, i, i, f, vp, i, i, i, vp]
    L.dl_apply.restype = None
    L.dl_recip_differ.argtypes = [vp, C.c_long]
    L.dl_recip_differ.restype = C.c_long
    return L


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- synthetic sequences -------------------------------------------------------------------------------------------------------------------
def intrinsics(W, H):
    return (np.float32(0.9 * W), np.float32(0.9 * W), np.float32(W / 2 - 0.5), np.float32(H / 2 + 0.5))


def plane_pose(distance, tilt_deg=0.0, about="y"):
    """4 x 4 pose of a plane `distance` metres down the optical axis (-z), turned tilt_deg about the x or y axis: normal = third column, point = fourth."""
    a = np.deg2rad(tilt_deg)
    c, s = np.cos(a), np.sin(a)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) if about == "y" else np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (0, 0, -distance)
    return T.astype(np.float32)


def true_depth(T, W, H, K):
    """Metres along -z at which the ray of every pixel (the rule's pinhole: x right, y up from row H - j) meets the plane of pose T, float64."""
    fx, fy, mx, my = [float(v) for v in K]
    T = np.asarray(T, np.float64)
    n, p = T[:3, 2], T[:3, 3]
    j, i = np.mgrid[0:H, 0:W]
    a, b = (i - mx) / fx, ((H - j) - my) / fy
    return np.dot(n, p) / (n[0] * a + n[1] * b - n[2])


def shift_in(mm):
    """millimetres -> the sensor's rotated u16 (what lut_unshift undoes)."""
    mm = np.asarray(mm, np.uint16)
    return (((mm & 0x1FFF) << 3) | (mm >> 13)).astype(np.uint16)


def shift_out(raw):
    raw = np.asarray(raw, np.uint16)
    return (((raw >> 3) & 0x1FFF) | ((raw & 7) << 13)).astype(np.uint16)


def observe(T, W, H, K, scale=1.0, bitshift=True):
    mm = np.rint(scale * 1000.0 * true_depth(T, W, H, K))
    mm = np.where((mm > 0) & (mm < 8192 if bitshift else mm < 65536), mm, 0).astype(np.uint16)   # 13 bits survive the rotation
    return shift_in(mm) if bitshift else mm


@functools.lru_cache(maxsize=None)
def sequence(name, bitshift=True):
    """name -> dict(W, H, K, n_slices, max_depth, bitshift, depths [N, H, W] uint16, poses [N, 4, 4] float32); read-only arrays."""
    if name.startswith("small"):          # the issue's small case; "small_WxH" for another size, "small_sN" for another n_slices
        W, H, ns, md = 48, 36, 5, 5.0
        for tok in name.split("_")[1:]:
            if tok[0] == "s":
                ns = int(tok[1:])
            else:
                W, H = [int(v) for v in tok.split("x")]
        K = intrinsics(W, H)
        poses = [plane_pose(d) for d in (0.6, 1.1, 1.7, 3.2, 4.6)]
        poses[2] = plane_pose(1.7, 8.0, "x")
        poses[3] = plane_pose(3.2, -11.0, "y")
        depths = [observe(T, W, H, K, 1.02, bitshift) for T in poses]
        poses.append(plane_pose(2.0, 30.0, "y"))                        # tilted beyond the filter: contributes nothing
        depths.append(observe(poses[-1], W, H, K, 1.02, bitshift))
        holes = observe(plane_pose(2.8, 5.0, "x"), W, H, K, 0.98, bitshift).copy()   # holes
        yy, xx = np.mgrid[0:H, 0:W]
        holes[(xx * 7 + yy * 13) % 5 == 0] = 0
        poses.append(plane_pose(2.8, 5.0, "x")); depths.append(holes)
        poses.append(plane_pose(1.5)); depths.append(np.zeros((H, W), np.uint16))     # all zeros
        poses.append(plane_pose(4.9, 20.0, "y")); depths.append(observe(poses[-1], W, H, K, 1.02, bitshift))   # reaches beyond max_depth
    elif name == "real":                  # the sensor's size once
        W, H, ns, md = 640, 480, 15, 5.0
        K = intrinsics(W, H)
        poses = [plane_pose(0.8, 6.0, "x"), plane_pose(2.2, -9.0, "y"), plane_pose(3.9, 3.0, "x")]
        depths = [observe(T, W, H, K, 0.97, bitshift) for T in poses]
    elif name == "roundtrip":             # 120 planes 0.45 .. 4.3 m, tilted up to 12 degrees, every depth observed as round(1.03 true) mm
        W, H, ns, md = 64, 48, 15, 5.0
        K = intrinsics(W, H)
        poses = [plane_pose(0.45 + (4.3 - 0.45) * k / 119.0, 12.0 * np.sin(1.7 * k), "xy"[k % 2]) for k in range(120)]
        depths = [observe(T, W, H, K, 1.03, bitshift) for T in poses]
    else:
        raise KeyError(name)
    d = np.ascontiguousarray(np.stack(depths), np.uint16)
    p = np.ascontiguousarray(np.stack(poses), np.float32)
    d.setflags(write=False)
    p.setflags(write=False)
    return dict(W=W, H=H, K=K, n_slices=ns, max_depth=md, bitshift=bitshift, depths=d, poses=p)


def repeat(seq, n):
    """The sequence's images cycled to n images (read-only views are copied)."""
    idx = np.arange(n) % len(seq["depths"])
    out = dict(seq)
    out["depths"] = np.ascontiguousarray(seq["depths"][idx])
    out["poses"] = np.ascontiguousarray(seq["poses"][idx])
    return out


# ---- the checker on a sequence ---------------------------------------------------------------------------------------------------------------
def checker_run(seq):
    """(acc, div, table) of the checker: [n_slices, H / 2, W / 2] float32 each."""
    L = checker()
    W, H, ns = seq["W"], seq["H"], seq["n_slices"]
    acc = np.zeros((ns, H // 2, W // 2), np.float32)
    div = np.zeros_like(acc)
    K = np.array(seq["K"], np.float32)
    for img, T in zip(seq["depths"], seq["poses"]):
        img = np.ascontiguousarray(img)
        T = np.ascontiguousarray(T, np.float32)
        L.dl_accumulate(img.ctypes.data, W, H, K.ctypes.data, T.ctypes.data, float(ns), float(seq["max_depth"]), int(seq["bitshift"]), acc.ctypes.data, div.ctypes.data)
    table = np.empty_like(acc)
    L.dl_finish(acc.ctypes.data, div.ctypes.data, W // 2, H // 2, ns, table.ctypes.data)
    return acc, div, table


@functools.lru_cache(maxsize=None)
def checker_case(name, bitshift=True):
    out = checker_run(sequence(name, bitshift))
    for a in out:
        a.setflags(write=False)
    return out


def checker_apply(lut, depths, bitshift=True):
    table, max_dist = lut
    t = np.ascontiguousarray(table, np.float32)
    d = np.ascontiguousarray(depths, np.uint16)
    out = np.empty_like(d)
    L = checker()
    for k in range(len(d)):
        L.dl_apply(t.ctypes.data, t.shape[2], t.shape[1], t.shape[0], float(max_dist), d[k].ctypes.data, d.shape[2], d.shape[1], int(bitshift), out[k].ctypes.data)
    return out


def checker_filter(T):
    T = np.ascontiguousarray(T, np.float32)
    return bool(checker().dl_filter(T.ctypes.data))


# ---- the rule in float64 numpy (independent of the C text) ---------------------------------------------------------------------------------------
def rule_float64(seq):
    """(m [ns, yres, xres] float64 with NaN where unknown, counts) BEFORE the stripe and the unknowns.  The input quantities -- the u16 turned into a
    binary32 depth, and the slice it selects -- are the rule's; every operation after them is float64."""
    W, H, ns = seq["W"], seq["H"], seq["n_slices"]
    fx, fy, mx, my = [float(v) for v in seq["K"]]
    zbin = np.float32(ns) / np.float32(seq["max_depth"])
    acc = np.zeros((ns, H // 2, W // 2))
    div = np.zeros_like(acc)
    cnt = np.zeros(acc.shape, np.int64)
    j, i = np.mgrid[0:H, 0:W]
    for raw, T in zip(seq["depths"], seq["poses"]):
        T = np.asarray(T, np.float64)
        n, p = T[:3, 2], T[:3, 3]
        q = n[2] * np.sqrt(n @ n)
        ang = np.degrees(np.arccos(q)) if abs(q) <= 1 else np.nan
        if ang > 25.0:
            continue
        d = shift_out(raw) if seq["bitshift"] else raw
        depth32 = d.astype(np.float32) * np.float32(0.001)
        z = np.floor(depth32 * zbin).astype(np.int64)
        depth = depth32.astype(np.float64)
        pos = np.stack([(i - mx) * depth / fx, ((H - j) - my) * depth / fy, -depth], -1)
        with np.errstate(all="ignore"):
            v = pos / np.linalg.norm(pos, axis=-1, keepdims=True)
            t = np.dot(n, p) / (v @ n)
            real = np.where(depth > 0.01, -t * v[..., 2], depth)
        ok = (z >= 1) & (z <= ns - 1)
        np.add.at(acc, (z[ok], (j // 2)[ok], (i // 2)[ok]), (depth * real)[ok])
        np.add.at(div, (z[ok], (j // 2)[ok], (i // 2)[ok]), (real * real)[ok])
        np.add.at(cnt, (z[ok], (j // 2)[ok], (i // 2)[ok]), 1)
    with np.errstate(all="ignore"):
        m = np.where(div != 0, acc / div, np.nan)
    return m, cnt


# ---- files ----------------------------------------------------------------------------------------------------------------------------------
PARAMS_TXT = """colorWidth = 1296
colorHeight = 968
depthWidth = %d
depthHeight = %d
fx_color = 1170.1
fy_color = 1170.2
mx_color = 647.7
my_color = 483.8
fx_depth = %r
fy_depth = %r
mx_depth = %r
my_depth = %r
depthToColorExtrinsics = %s
"""

D2C = np.array([[0.9998, -0.0113, 0.0157, 0.031], [0.0111, 0.9999, 0.0103, -0.004], [-0.0158, -0.0101, 0.9998, 0.002], [0, 0, 0, 1]], np.float64)


def write_sequence(root, seq, write_png, n_images=None, d2c=None, names=None):
    """Lays a sequence out as the tool reads it under `root`: calib.conf, parameters.txt, plane_poses.txt, depth_raw/*.png.  The poses file holds what
    the Matlab script would: pose_file = (F D2C F) pose, so that the loader's inverse gives the sequence's poses back.  Returns the configuration's path."""
    os.makedirs(os.path.join(root, "depth_raw"), exist_ok=True)
    d2c = D2C if d2c is None else d2c
    F = np.diag([1.0, -1.0, -1.0, 1.0])
    M = F @ d2c @ F
    N = len(seq["depths"])
    names = names or ["frame-%04d.png" % k for k in range(N)]
    K = seq["K"]
    with open(os.path.join(root, "parameters.txt"), "w") as f:
        f.write(PARAMS_TXT % (seq["W"], seq["H"], float(K[0]), float(K[1]), float(K[2]), float(K[3]), " ".join("%r" % float(v) for v in d2c.ravel())))
    with open(os.path.join(root, "plane_poses.txt"), "w") as f:
        for T in seq["poses"]:
            for row in (M @ np.asarray(T, np.float64)):
                f.write(" ".join("%.9g" % v for v in row) + "\n")
    with open(os.path.join(root, "calib.conf"), "w") as f:
        f.write("# synthetic calibration sequence\nparameters parameters.txt\nn_images %d\nplane_poses plane_poses.txt\n" % (N if n_images is None else n_images))
        for k in range(N):
            f.write("scan %s %s %s\n" % (names[k], names[k].replace("frame", "color").replace(".png", ".jpg"), " ".join(["1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"])))
    for k in range(N):
        write_png(os.path.join(root, "depth_raw", names[k]), seq["depths"][k])
    return os.path.join(root, "calib.conf")
