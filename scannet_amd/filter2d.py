"""2-D annotation filter -- host-side mirror of AnnotationTools/Filter2dAnnotations (FilterData + the frame body of process())
over the C ABI; the kernels run on the GPU (scannet_amd/csrc/filter2d.hip)."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import check

MAX_NUM_LABELS_PER_SCENE = 80  # GlobalDefines.h:12


def _lib():
    L = _abi.lib()
    vp = C.c_void_p
    L.sf_filter2d_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.sf_filter2d_destroy.argtypes = [vp]
    L.sf_filter2d_destroy.restype = None
    L.sf_filter2d_set_tables.argtypes = [vp, vp, vp, vp]
    L.sf_filter2d_frame.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
    return L


def make_tables(object_ids_to_label):
    """Filter2dAnnotations.cpp:293-309: {object id (0-based): label id} -> (instance_to_idx[256], idx_to_instance[80], instance_to_label[256])."""
    to_idx = np.full(256, 255, np.uint8)
    to_inst = np.full(MAX_NUM_LABELS_PER_SCENE, 255, np.uint8)
    to_label = np.full(256, 65535, np.uint16)
    to_idx[0] = 0
    to_inst[0] = 0
    to_label[0] = 0
    idx = 1
    for obj, label in sorted(object_ids_to_label.items()):
        to_label[obj + 1] = label
        to_idx[obj + 1] = idx
        to_inst[idx] = obj + 1
        idx += 1
    return to_idx, to_inst, to_label


class Filter2d:
    def __init__(self, depth_wh, color_wh, device=0):
        self._h = C.c_void_p()
        self.depth_wh, self.color_wh = depth_wh, color_wh
        check(_lib().sf_filter2d_create(depth_wh[0], depth_wh[1], color_wh[0], color_wh[1], int(device), C.byref(self._h)))

    def close(self):
        if self._h:
            _lib().sf_filter2d_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_tables(self, to_idx, to_inst, to_label):
        a, b, c = (np.ascontiguousarray(to_idx, np.uint8), np.ascontiguousarray(to_inst, np.uint8), np.ascontiguousarray(to_label, np.uint16))
        assert a.size == 256 and b.size == 80 and c.size == 256
        self._keep = (a, b, c)
        check(_lib().sf_filter2d_set_tables(self._h, a.ctypes.data, b.ctypes.data, c.ctypes.data))

    def frame(self, depth, rgb, instance):
        """-> (instance_out uint8 [Hc, Wc], label_out uint16 [Hc, Wc], kernel microseconds)"""
        d = np.ascontiguousarray(depth, np.uint16)
        c = np.ascontiguousarray(rgb, np.uint8)
        i = np.ascontiguousarray(instance, np.uint8)
        cw, ch = self.color_wh
        io = np.empty((ch, cw), np.uint8)
        lo = np.empty((ch, cw), np.uint16)
        us = C.c_float(0)
        check(_lib().sf_filter2d_frame(self._h, d.ctypes.data, c.ctypes.data, i.ctypes.data, io.ctypes.data, lo.ctypes.data, C.byref(us)))
        return io, lo, us.value


# ---- stage hooks (include/scanfuse_internal.h): one kernel of filter2d.hip per call, host arrays in and out -- for tests/test_filter2d_stages.py ----
MAX_RADIUS = 35   # what the vote kernel's dynamic-LDS budget holds (scanfuse_internal.h)


def _stage_lib():
    L = _abi.lib()
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.sf_filter2d_stage_prepare.argtypes = [ci, vp, ci, vp, ci, vp, vp]
    L.sf_filter2d_stage_bilateral.argtypes = [ci, vp, cf, cf, ci, ci, vp]
    L.sf_filter2d_stage_resample_float.argtypes = [ci, vp, ci, ci, vp, ci, ci]
    L.sf_filter2d_stage_resample_uchar.argtypes = [ci, vp, ci, ci, vp, ci, ci]
    L.sf_filter2d_stage_vote.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, cf, cf, cf, vp]
    L.sf_filter2d_stage_to_label.argtypes = [ci, vp, vp, ci, vp]
    L.sf_filter2d_selftest_gauss.argtypes = [ci, cf, vp, vp, vp, C.c_uint64, vp, vp]
    return L


def _img(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    assert a.ndim == 2, "an image is [H, W]"
    return a


def stage_prepare(depth16, rgb, device=0):
    """k_f2d_prepare: (uint16 millimetres [any shape], uint8 [..., 3]) -> (depth float32, flat; intensity float32, flat)."""
    d = np.ascontiguousarray(depth16, np.uint16).ravel()
    c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    do, io = np.empty(d.size, np.float32), np.empty(len(c), np.float32)
    check(_stage_lib().sf_filter2d_stage_prepare(int(device), d.ctypes.data, d.size, c.ctypes.data, len(c), do.ctypes.data, io.ctypes.data))
    return do, io


def stage_bilateral(image, sigma_d, sigma_r, device=0):
    a = _img(image, np.float32)
    out = np.empty_like(a)
    check(_stage_lib().sf_filter2d_stage_bilateral(int(device), a.ctypes.data, float(sigma_d), float(sigma_r), a.shape[1], a.shape[0], out.ctypes.data))
    return out


def _stage_resample(fn, dtype, image, initial):
    a, out = _img(image, dtype), _img(initial, dtype).copy()
    check(fn(0, a.ctypes.data, a.shape[1], a.shape[0], out.ctypes.data, out.shape[1], out.shape[0]))
    return out


def stage_resample_float(image, initial):
    """k_f2d_resample_float of `image` into a copy of `initial` (its shape is the output size; pixels the kernel does not write keep its values)."""
    return _stage_resample(_stage_lib().sf_filter2d_stage_resample_float, np.float32, image, initial)


def stage_resample_uchar(image, initial):
    return _stage_resample(_stage_lib().sf_filter2d_stage_resample_uchar, np.uint8, image, initial)


def stage_vote(instance, depth, intensity, to_idx, to_inst, radius, sigma_d, sigma_r, intensity_scale, device=0):
    i, d, n = _img(instance, np.uint8), _img(depth, np.float32), _img(intensity, np.float32)
    a, b = np.ascontiguousarray(to_idx, np.uint8), np.ascontiguousarray(to_inst, np.uint8)
    assert i.shape == d.shape == n.shape and a.size == 256 and b.size == MAX_NUM_LABELS_PER_SCENE
    out = np.empty_like(i)
    check(_stage_lib().sf_filter2d_stage_vote(int(device), i.ctypes.data, d.ctypes.data, n.ctypes.data, a.ctypes.data, b.ctypes.data, int(radius), i.shape[1], i.shape[0],
                                              float(sigma_d), float(sigma_r), float(intensity_scale), out.ctypes.data))
    return out


def stage_to_label(instance, to_label, device=0):
    i, t = np.ascontiguousarray(instance, np.uint8), np.ascontiguousarray(to_label, np.uint16)
    assert t.size == 256
    out = np.empty(i.shape, np.uint16)
    check(_stage_lib().sf_filter2d_stage_to_label(int(device), i.ctypes.data, t.ctypes.data, i.size, out.ctypes.data))
    return out


def selftest_gauss(sigma, dist=None, dx=None, dy=None, device=0):
    """The kernels' gauss_r(sigma, dist) and / or gauss_d2(sigma, dx, dy), element-wise on the device -> (out_r or None, out_d or None)."""
    dist = None if dist is None else np.ascontiguousarray(dist, np.float32).ravel()
    dx = None if dx is None else np.ascontiguousarray(dx, np.int32).ravel()
    dy = None if dy is None else np.ascontiguousarray(dy, np.int32).ravel()
    n = dist.size if dist is not None else dx.size
    assert (dx is None) == (dy is None) and all(a is None or a.size == n for a in (dist, dx, dy))
    out_r = None if dist is None else np.empty(n, np.float32)
    out_d = None if dx is None else np.empty(n, np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data
    check(_stage_lib().sf_filter2d_selftest_gauss(int(device), float(sigma), ptr(dist), ptr(dx), ptr(dy), n, ptr(out_r), ptr(out_d)))
    return out_r, out_d


# ---- PNG images of the annotation tools (scannet_amd/csrc/png.cpp) -------------------------------------------------------
def png_read(path):
    """-> uint8 / uint16 array [H, W] (grey) or [H, W, C]."""
    import os
    L = _abi.lib()
    L.sf_png_read.argtypes = [C.c_char_p] + [C.POINTER(C.c_uint32)] * 2 + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_void_p)]
    L.sf_free.argtypes = [C.c_void_p]
    L.sf_free.restype = None
    w, h, c, b, d = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int(), C.c_void_p()
    check(L.sf_png_read(os.fsencode(path), C.byref(w), C.byref(h), C.byref(c), C.byref(b), C.byref(d)))
    ct = C.c_uint16 if b.value == 16 else C.c_uint8
    a = np.ctypeslib.as_array(C.cast(d, C.POINTER(ct)), (h.value, w.value, c.value)).copy()
    L.sf_free(d)
    return a[..., 0] if c.value == 1 else a


def png_write_gray(path, image):
    import os
    a = np.ascontiguousarray(image)
    assert a.ndim == 2 and a.dtype in (np.uint8, np.uint16)
    L = _abi.lib()
    L.sf_png_write_gray.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    check(L.sf_png_write_gray(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0], 8 * a.dtype.itemsize))
