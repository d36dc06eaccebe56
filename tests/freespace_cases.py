"""What tests/test_freespace.py (no GPU) and tests/test_freespace_gpu.py share: the checker tests/freespace_checker.c built and bound, its parameters
made from the fuser's, and the synthetic inputs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from scannet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "freespace_checker.c")
NEG_INF_POSE = np.full((4, 4), -np.inf, np.float32)


class FcParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
                ("depth_shift", C.c_float), ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("voxel_size", C.c_float), ("trunc_base", C.c_float), ("trunc_scale", C.c_float), ("max_integration_dist", C.c_float),
                ("weight_sample", C.c_int32), ("weight_max", C.c_int32), ("weight_mode", C.c_int32), ("weight_wrap", C.c_int32)]


def has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


def build_checker(directory):
    """gcc -O2 -mfma -ffp-contract=off, as tests/test_raycast.py builds its checker; None when that cannot be done here."""
    if shutil.which("gcc") is None or not has_fma():
        return None
    so = os.path.join(str(directory), "libfreespace_checker.so")
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, CHECKER, "-lm"], check=True)
    L = C.CDLL(so)
    vp = C.c_void_p
    L.fc_create.restype = vp
    L.fc_create.argtypes = [C.POINTER(FcParams), vp, vp]
    L.fc_destroy.argtypes = [vp]
    L.fc_destroy.restype = None
    L.fc_integrate.argtypes = [vp, vp, vp]
    L.fc_export.argtypes = [vp, C.c_int, vp, vp]
    L.fc_export.restype = None
    L.fc_plan.restype = C.c_double
    L.fc_plan.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                          vp, C.c_int64, C.c_int32, vp, vp, C.POINTER(C.c_double)]
    return L


def resample(depth, W, H):
    """The pre-pass's nearest resample to the integration size: x_in = (uint)(x * (W_in - 1) / (W - 1) + 0.5f) (include/scanfuse.h integration_width)."""
    Hi, Wi = depth.shape
    sx = np.float32(Wi - 1) / np.float32(W - 1)
    sy = np.float32(Hi - 1) / np.float32(H - 1)
    xi = (np.arange(W, dtype=np.float32) * sx + np.float32(0.5)).astype(np.uint32)
    yi = (np.arange(H, dtype=np.float32) * sy + np.float32(0.5)).astype(np.uint32)
    return np.ascontiguousarray(depth[yi][:, xi])


def checker_params(sp):
    """FcParams from the fuser's parameters (an _abi.SfParams): the integration camera as sf_fuser_create derives it."""
    p = FcParams()
    W, H = sp.depth_width, sp.depth_height
    fx, fy, mx, my = (np.float32(v) for v in (sp.fx, sp.fy, sp.mx, sp.my))
    if sp.integration_width > 0 and (sp.integration_width != W or sp.integration_height != H):
        iw, ih = sp.integration_width, sp.integration_height
        fx, fy = fx * (np.float32(iw) / np.float32(W)), fy * (np.float32(ih) / np.float32(H))
        mx, my = mx * (np.float32(iw - 1) / np.float32(W - 1)), my * (np.float32(ih - 1) / np.float32(H - 1))
        W, H = iw, ih
    p.width, p.height, p.fx, p.fy, p.mx, p.my = W, H, fx, fy, mx, my
    for k in ("depth_shift", "depth_min", "depth_max", "voxel_size", "trunc_base", "trunc_scale", "max_integration_dist", "weight_sample", "weight_max",
              "weight_mode", "weight_wrap"):
        setattr(p, k, getattr(sp, k))
    return p


class Volume:
    """The checker's dense volume over the box [lo, lo + dims) of global voxel indices."""

    def __init__(self, L, params, lo, dims):
        self.L, self.p = L, params
        self.lo = np.ascontiguousarray(lo, np.int32).reshape(3)
        self.dims = np.ascontiguousarray(dims, np.int32).reshape(3)
        self.h = L.fc_create(C.byref(params), self.lo.ctypes.data_as(C.c_void_p), self.dims.ctypes.data_as(C.c_void_p))
        assert self.h, "fc_create failed"

    def integrate(self, depth, pose):
        d = np.ascontiguousarray(depth, np.uint16)
        assert d.shape == (self.p.height, self.p.width), (d.shape, self.p.height, self.p.width)
        T = np.ascontiguousarray(pose, np.float32).reshape(16)
        return bool(self.L.fc_integrate(self.h, d.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)))

    def export(self, task=False):
        shape = (int(self.dims[2]), int(self.dims[1]), int(self.dims[0]))
        sdf, w = np.empty(shape, np.float32), np.empty(shape, np.uint8)
        self.L.fc_export(self.h, 1 if task else 0, sdf.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
        return sdf, w

    def close(self):
        if self.h:
            self.L.fc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def plan(L, W, H, fx, fy, mx, my, poses, voxel, every=1, int_w=0, int_h=0, max_dist=4.0, trunc_base=0.06, trunc_scale=0.02):
    """fc_plan -> (lo_block, hi_block, blocks, R)"""
    T = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    R = C.c_double(0)
    n = L.fc_plan(W, H, fx, fy, mx, my, int_w, int_h, voxel, max_dist, trunc_base, trunc_scale, T.ctypes.data_as(C.c_void_p), len(T), every,
                  lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), C.byref(R))
    return lo, hi, n, R.value


def room_frames(n, W, H, total=400):
    """The noise-free empty room seen from n poses spread over the walk: [(depth u16 [H, W], pose f32 [4, 4])]."""
    out = []
    for i in range(n):
        pose = synth.trajectory_pose(i * total // n, total)
        out.append((synth.render_room_depth(pose, W, H), np.asarray(pose, np.float32)))
    return out


def noise_depth(W, H, seed):
    """A hashed-noise depth image: 0.3 .. 4.6 m with every eighth pixel zero and every eleventh beyond the sensor's range (65 000 mm)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 4600, (H, W)).astype(np.uint16)
    flat = d.reshape(-1)
    flat[::8] = 0
    flat[3::11] = 65000
    return d


def make_sens(frames, W, H, intr=None):
    """A depth-only .sens in memory from [(depth, pose)] (scannet_amd.sens writer)."""
    from scannet_amd import sens
    K = np.eye(4, dtype=np.float32)
    fx, fy, mx, my = intr if intr is not None else synth.intrinsics(W, H)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, mx, my
    sd = sens.SensorData.create(0, 0, W, H, K, K, color_compression=0, depth_compression=1)
    for d, pose in frames:
        sd.add_frame(d, pose)
    return sd
