"""Mesh render and thumbnail -- host-side mirror of the `render` and `thumbnail` stages (Server/mts_render.py, Server/thumbnail.sh; the calls of
Server/scan_processor.py:159-165) over the C ABI: `render_mesh(path_or_mesh)` gives the RGBA8 preview of a vertex-coloured mesh under a constant
sky, `thumbnail(image)` its 128 x 128 fit.  The rule is DESIGN.md section 4j."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import check
from .segmentator import Mesh

PATH, AO = 0, 1
INTEGRATORS = {"path": PATH, "ao": AO}
MAX_BATCH = 32


class SfRenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("samples", C.c_int32), ("max_depth", C.c_int32), ("integrator", C.c_int32),
                ("fov", C.c_float), ("exposure", C.c_float), ("pixel_centre", C.c_int32), ("reserved", C.c_int32 * 8)]


class SfCamera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("forward", C.c_float * 3),
                ("tan_half_fov", C.c_float), ("aspect", C.c_float), ("reserved", C.c_float * 2)]


def _lib():
    L = _abi.lib()
    vp = C.c_void_p
    L.sf_render_params_default.argtypes = [C.POINTER(SfRenderParams)]
    L.sf_render_params_default.restype = None
    L.sf_render_camera.argtypes = [vp, vp, C.POINTER(SfRenderParams), vp, vp, vp, C.c_float, C.c_float, C.POINTER(SfCamera)]
    L.sf_renderer_create.argtypes = [C.POINTER(SfRenderParams), C.c_int, C.POINTER(vp)]
    L.sf_renderer_set_mesh.argtypes = [vp, vp]
    L.sf_renderer_run.argtypes = [vp, C.c_int, vp, vp, C.POINTER(C.c_float)]
    L.sf_renderer_destroy.argtypes = [vp]
    L.sf_renderer_destroy.restype = None
    L.sf_render_film.argtypes = [vp, C.c_uint64, C.c_float, vp]
    L.sf_image_thumbnail.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.sf_render_stage_nodes.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sf_render_stage_rays.argtypes = [vp, C.c_uint64, vp, vp, vp]
    L.sf_render_stage_sample.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.sf_render_tune.argtypes = [C.c_char_p, C.c_int]
    L.sf_png_write.argtypes = [C.c_char_p, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    return L


def default_params(**overrides):
    """mts_render.py's defaults (sf_render_params_default) with the given fields replaced; integrator may be "path" / "ao"."""
    p = SfRenderParams()
    _lib().sf_render_params_default(C.byref(p))
    for k, v in overrides.items():
        if k == "reserved" or not hasattr(p, k):
            raise TypeError("unknown render parameter %r" % k)
        setattr(p, k, INTEGRATORS[v] if k == "integrator" and isinstance(v, str) else v)
    return p


def _vec(v):
    return None if v is None else np.ascontiguousarray(v, np.float32).reshape(3)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def camera(mesh_or_aabb, params=None, world_up=None, camera_up=None, camera_offset=None, bsphere_mult=2.5, theta=0.0):
    """The view of mts_render.py:69-99 on a Mesh or on a box {min x y z, max x y z}: an SfCamera."""
    cam = SfCamera()
    wu, cu, off = _vec(world_up), _vec(camera_up), _vec(camera_offset)
    mesh, box = (mesh_or_aabb._h, None) if isinstance(mesh_or_aabb, Mesh) else (None, np.ascontiguousarray(mesh_or_aabb, np.float32).reshape(6))
    check(_lib().sf_render_camera(mesh, _p(box), None if params is None else C.byref(params), _p(wu), _p(cu), _p(off), float(bsphere_mult), float(theta),
                                  C.byref(cam)))
    return cam


class Renderer:
    """sf_renderer: device -1 is the host path, >= 0 that GPU (an error without one)."""

    def __init__(self, params=None, device=0):
        self.params = params if params is not None else default_params()
        self.device = device
        self._h = C.c_void_p()
        check(_lib().sf_renderer_create(C.byref(self.params), int(device), C.byref(self._h)))
        self.kernel_us = 0.0

    def set_mesh(self, mesh):
        check(_lib().sf_renderer_set_mesh(self._h, mesh._h))

    def run(self, cameras):
        """cameras: an SfCamera or a sequence of them -> float32 [n, height, width, 4], the mean radiance and alpha before the film."""
        cams = [cameras] if isinstance(cameras, SfCamera) else list(cameras)
        arr = (SfCamera * len(cams))(*cams)
        out = np.zeros((len(cams), self.params.height, self.params.width, 4), np.float32)
        us = C.c_float(0)
        check(_lib().sf_renderer_run(self._h, len(cams), C.cast(arr, C.c_void_p), _p(out), C.byref(us)))
        self.kernel_us = us.value
        return out

    def nodes(self):
        """The tree (stage hook): boxes [N, 6], links [N, 2] = {skip, info}."""
        n = C.c_uint64(0)
        check(_lib().sf_render_stage_nodes(self._h, None, None, 0, C.byref(n)))
        boxes, links = np.zeros((n.value, 6), np.float32), np.zeros((n.value, 2), np.uint32)
        check(_lib().sf_render_stage_nodes(self._h, _p(boxes), _p(links), n.value, C.byref(n)))
        return boxes, links

    def rays(self, rays6):
        """Closest hits of rays [n, 6] (stage hook): triangle [n] (0xFFFFFFFF: none), tuv [n, 3]."""
        rays6 = np.ascontiguousarray(rays6, np.float32).reshape(-1, 6)
        tri, tuv = np.zeros(len(rays6), np.uint32), np.zeros((len(rays6), 3), np.float32)
        check(_lib().sf_render_stage_rays(self._h, len(rays6), _p(rays6), _p(tri), _p(tuv)))
        return tri, tuv

    def close(self):
        if getattr(self, "_h", None):
            _lib().sf_renderer_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_direction(n, pixel, sample, bounce):
    """The bounce direction about unit normal n (stage hook)."""
    n, d = _vec(n), np.zeros(3, np.float32)
    check(_lib().sf_render_stage_sample(_p(n), int(pixel), int(sample), int(bounce), _p(d)))
    return d


def tune(key, value):
    check(_lib().sf_render_tune(key.encode(), int(value)))


def film(rgba, exposure=1.0):
    """float RGBA [..., 4] -> uint8 RGBA: x 2^exposure, the sRGB curve, clamp, (int)(255 v + 0.5)."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    out = np.zeros(rgba.shape, np.uint8)
    check(_lib().sf_render_film(_p(rgba), rgba.size // 4, float(exposure), _p(out)))
    return out


def thumbnail(image, box=(128, 128)):
    """uint8 [H, W] or [H, W, C] fitted into box = (width, height) keeping its aspect ratio, by an integer area average."""
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape[:2]
    ch = 1 if image.ndim == 2 else image.shape[2]
    out = np.zeros(box[0] * box[1] * ch, np.uint8)
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    check(_lib().sf_image_thumbnail(_p(image), w, h, ch, int(box[0]), int(box[1]), _p(out), C.byref(ow), C.byref(oh)))
    out = out[:ow.value * oh.value * ch]
    return out.reshape(oh.value, ow.value) if image.ndim == 2 else out.reshape(oh.value, ow.value, ch)


def write_png(path, image):
    """uint8 [H, W, C], C = 1, 3 or 4."""
    image = np.ascontiguousarray(image, np.uint8)
    check(_lib().sf_png_write(os.fsencode(path), _p(image), image.shape[1], image.shape[0], 1 if image.ndim == 2 else image.shape[2], 8))


def render_mesh(path_or_mesh, device=0, params=None, theta=0.0, world_up=None, camera_up=None, camera_offset=None, bsphere_mult=2.5, **overrides):
    """mts_render.py's single view of a mesh file or Mesh -> uint8 [height, width, 4].  overrides: fields of the parameters (samples=..., integrator="ao")."""
    if params is not None and overrides:
        raise TypeError("render_mesh takes params or parameter overrides, not both")
    p = params if params is not None else default_params(**overrides)
    mesh = path_or_mesh if isinstance(path_or_mesh, Mesh) else Mesh.read(path_or_mesh)
    cam = camera(mesh, p, world_up, camera_up, camera_offset, bsphere_mult, theta)
    with Renderer(p, device) as r:
        r.set_mesh(mesh)
        return film(r.run(cam)[0], p.exposure)
