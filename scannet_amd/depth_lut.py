"""The depth-distortion table the `calibrate` stage reads: estimate it from a calibration sequence of planes and apply it to depth images --
the two batch modes of CameraParameterEstimation/apps/calibrate_depth over the C ABI (scannet_amd/csrc/depth_lut.hip, depth_lut.cpp;
DESIGN.md section 4k).  device >= 0: HIP kernels; device -1: the host path, the same bits.  The default of estimate() / apply() /
calibrate_depth() is the host path: README.md has the measurement behind that."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import check
from .calibrate import SfLut

DEFAULT_DEVICE = -1


class SfDepthCalib(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float), ("depth_to_color", C.c_float * 16),
                ("n_images", C.c_int32), ("n_scans", C.c_int32), ("plane_poses", C.POINTER(C.c_float)), ("image_names", C.POINTER(C.c_char_p))]


class SfCalibrateDepthOptions(C.Structure):
    _fields_ = [("max_depth", C.c_float), ("n_slices", C.c_int32), ("bitshift", C.c_int32), ("verbose", C.c_int32), ("save_slices", C.c_int32),
                ("root", C.c_char_p), ("reserved", C.c_int32 * 8)]


class SfCalibrateDepthStats(C.Structure):
    _fields_ = [("images", C.c_uint64), ("images_used", C.c_uint64), ("images_skipped", C.c_uint64), ("images_applied", C.c_uint64),
                ("seconds_read", C.c_double), ("seconds_estimate", C.c_double), ("seconds_apply", C.c_double), ("seconds_write", C.c_double),
                ("seconds_total", C.c_double), ("threads", C.c_uint32)]


def _lib():
    L = _abi.lib()
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.sf_lut_save.argtypes = [C.c_char_p, C.POINTER(SfLut)]
    L.sf_lut_load.argtypes = [C.c_char_p, C.POINTER(SfLut)]
    L.sf_lut_free.argtypes = [C.POINTER(SfLut)]
    L.sf_lut_free.restype = None
    L.sf_lut_estimator_create.argtypes = [i, i, f, f, f, f, i, f, i, i, C.POINTER(vp)]
    L.sf_lut_estimator_add.argtypes = [vp, i, vp, vp]
    L.sf_lut_estimator_add_device.argtypes = [vp, i, vp, vp, C.POINTER(f)]
    L.sf_lut_estimator_max_batch.argtypes = []
    L.sf_lut_estimator_finish.argtypes = [vp, C.POINTER(SfLut)]
    L.sf_lut_estimator_destroy.argtypes = [vp]
    L.sf_lut_estimator_destroy.restype = None
    L.sf_lut_estimator_sums.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sf_lut_apply.argtypes = [C.POINTER(SfLut), i, vp, vp, i, i, i, i]
    L.sf_lut_apply_device.argtypes = [C.POINTER(SfLut), i, vp, vp, i, i, i, i, C.POINTER(f)]
    L.sf_depth_calib_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(SfDepthCalib)]
    L.sf_depth_calib_free.argtypes = [C.POINTER(SfDepthCalib)]
    L.sf_depth_calib_free.restype = None
    L.sf_calibrate_depth_options_default.argtypes = [C.POINTER(SfCalibrateDepthOptions)]
    L.sf_calibrate_depth_options_default.restype = None
    L.sf_calibrate_depth.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(SfCalibrateDepthOptions), i, i, C.POINTER(SfCalibrateDepthStats)]
    return L


def max_batch():
    return _lib().sf_lut_estimator_max_batch()


def _images(depths):
    """[N, H, W] (or a sequence of [H, W]) uint16 -> a contiguous array and the table of its N row pointers."""
    a = np.ascontiguousarray(depths, np.uint16)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("depth images: [N, H, W] uint16")
    ptr = (C.c_void_p * a.shape[0])(*[a.ctypes.data + k * a.strides[0] for k in range(a.shape[0])])
    return a, ptr


def _lut_struct(lut):
    """(table [zres, yres, xres] float32, max_dist) -> SfLut that borrows the array."""
    table, max_dist = lut
    t = np.ascontiguousarray(table, np.float32)
    if t.ndim != 3:
        raise ValueError("table: [zres, yres, xres] float32")
    s = SfLut(t.shape[2], t.shape[1], t.shape[0], float(max_dist), t.ctypes.data_as(C.POINTER(C.c_float)))
    return s, t


class Estimator:
    """Running sums of a table over a sequence: add() images with their plane poses in order, finish() gives (table, max_depth).
    K = (fx, fy, mx, my) of the depth camera."""

    def __init__(self, width, height, K, n_slices=15, max_depth=5.0, bitshift=True, device=DEFAULT_DEVICE):
        self._L = _lib()
        self._h = C.c_void_p()
        self.shape = (int(n_slices), int(height) // 2, int(width) // 2)
        self.size = (int(width), int(height))
        self.max_depth = float(max_depth)
        fx, fy, mx, my = [float(v) for v in K]
        check(self._L.sf_lut_estimator_create(int(width), int(height), fx, fy, mx, my, int(n_slices), float(max_depth), 1 if bitshift else 0, int(device),
                                              C.byref(self._h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._h:
            self._L.sf_lut_estimator_destroy(self._h)
            self._h = C.c_void_p()

    def add(self, depths, plane_poses):
        a, ptr = _images(depths)
        if (a.shape[2], a.shape[1]) != self.size:
            raise ValueError("images are %d x %d, the estimator takes %d x %d" % (a.shape[2], a.shape[1], self.size[0], self.size[1]))
        p = np.ascontiguousarray(plane_poses, np.float32).reshape(-1, 16)
        if len(p) != len(a):
            raise ValueError("%d images, %d plane poses" % (len(a), len(p)))
        check(self._L.sf_lut_estimator_add(self._h, len(a), ptr, p.ctypes.data))

    def sums(self):
        """(acc, div, images added, images used): the raw sums, [n_slices, H / 2, W / 2] float32 each."""
        acc, div = np.empty(self.shape, np.float32), np.empty(self.shape, np.float32)
        n, used = C.c_uint64(0), C.c_uint64(0)
        check(self._L.sf_lut_estimator_sums(self._h, acc.ctypes.data, div.ctypes.data, C.byref(n), C.byref(used)))
        return acc, div, n.value, used.value

    def finish(self):
        t = SfLut()
        check(self._L.sf_lut_estimator_finish(self._h, C.byref(t)))
        try:
            table = np.ctypeslib.as_array(t.data, shape=(t.zres, t.yres, t.xres)).copy()
            return table, float(t.max_dist)
        finally:
            self._L.sf_lut_free(C.byref(t))


def estimate(depths, plane_poses, K, n_slices=15, max_depth=5.0, bitshift=True, device=DEFAULT_DEVICE):
    """EstimateDistortion on [N, H, W] uint16 images and [N, 4, 4] plane poses (in the depth camera's frame) -> (table, max_depth)."""
    a = np.ascontiguousarray(depths, np.uint16)
    with Estimator(a.shape[2], a.shape[1], K, n_slices, max_depth, bitshift, device) as e:
        e.add(a, plane_poses)
        return e.finish()


def apply(lut, depths, bitshift=True, device=DEFAULT_DEVICE):
    """ApplyUndistortion: lut = (table [zres, yres, xres], max_dist); depths [N, H, W] uint16 -> the corrected images."""
    s, keep = _lut_struct(lut)
    a, ip = _images(depths)
    out = np.empty_like(a)
    op = (C.c_void_p * a.shape[0])(*[out.ctypes.data + k * out.strides[0] for k in range(a.shape[0])])
    check(_lib().sf_lut_apply(C.byref(s), a.shape[0], ip, op, a.shape[2], a.shape[1], 1 if bitshift else 0, int(device)))
    del keep
    return out


def save_lut(path, lut):
    s, keep = _lut_struct(lut)
    check(_lib().sf_lut_save(os.fsencode(path), C.byref(s)))
    del keep


def load_lut(path):
    t = SfLut()
    L = _lib()
    check(L.sf_lut_load(os.fsencode(path), C.byref(t)))
    try:
        return np.ctypeslib.as_array(t.data, shape=(t.zres, t.yres, t.xres)).copy(), float(t.max_dist)
    finally:
        L.sf_lut_free(C.byref(t))


def load_config(path, root=None):
    """The configuration file with what it names: dict(K, depth_to_color [4, 4], n_images, plane_poses [n_images, 4, 4] converted, image_names)."""
    c = SfDepthCalib()
    L = _lib()
    check(L.sf_depth_calib_load(os.fsencode(path), os.fsencode(root) if root else None, C.byref(c)))
    try:
        poses = np.ctypeslib.as_array(c.plane_poses, shape=(c.n_images, 4, 4)).copy()
        return dict(K=(c.fx, c.fy, c.mx, c.my), depth_to_color=np.array(c.depth_to_color, np.float32).reshape(4, 4), n_images=c.n_images, plane_poses=poses,
                    image_names=[os.fsdecode(c.image_names[k]) for k in range(c.n_scans)])
    finally:
        L.sf_depth_calib_free(C.byref(c))


def calibrate_depth(config, estimate_path=None, apply_path=None, max_depth=5.0, n_slices=15, bitshift=True, verbose=False, save_slices=False, root=None,
                    device=DEFAULT_DEVICE, threads=0):
    """The tool's body (bin/calibrate_depth): -e estimate_path, -a apply_path."""
    L = _lib()
    o = SfCalibrateDepthOptions()
    L.sf_calibrate_depth_options_default(C.byref(o))
    o.max_depth, o.n_slices, o.bitshift, o.verbose, o.save_slices = float(max_depth), int(n_slices), int(bool(bitshift)), int(bool(verbose)), int(bool(save_slices))
    o.root = os.fsencode(root) if root else None
    st = SfCalibrateDepthStats()
    check(L.sf_calibrate_depth(os.fsencode(config), os.fsencode(estimate_path) if estimate_path else None, os.fsencode(apply_path) if apply_path else None,
                               C.byref(o), int(device), int(threads), C.byref(st)))
    return {n: getattr(st, n) for n, _ in SfCalibrateDepthStats._fields_}
