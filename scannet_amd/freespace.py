"""Free-space grids: the pipeline's `freespace` stage (Server/scan_processor.py:15; product ${id}.grid, Server/config/scan_stages.json:43-47) over
the C ABI (include/scanfuse.h "Free-space grids"; scannet_amd/csrc/freespace.cpp, fuser_dense.hip).  The rule and the file are this library's
statement; what the reference tree reads from such a grid is mirrored here: `save_npy` writes the `grid` / `world2grid` pair
BenchmarkScripts/3d_helpers/export_semantic_label_grid_for_evaluation.py:35-37 loads, `lookup` is its per-vertex read (:40-47)."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import SfParams, check


class SfFreespaceParams(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("max_blocks", C.c_uint32), ("every", C.c_int32), ("reserved", C.c_int32 * 5), ("params_file", C.c_char * 1024)]


class SfFreespaceStats(C.Structure):
    _fields_ = [("box_blocks", C.c_uint64), ("frames_used", C.c_uint64), ("known", C.c_uint64), ("free_voxels", C.c_uint64), ("near_voxels", C.c_uint64),
                ("lo_block", C.c_int32 * 3), ("hi_block", C.c_int32 * 3),
                ("seconds_plan", C.c_double), ("seconds_create", C.c_double), ("seconds_allocate", C.c_double), ("seconds_fuse", C.c_double),
                ("seconds_bounds", C.c_double), ("seconds_export", C.c_double), ("seconds_total", C.c_double)]

    def as_dict(self):
        out = {k: getattr(self, k) for k, _ in self._fields_ if not k.endswith("_block")}
        out.update(lo_block=list(self.lo_block), hi_block=list(self.hi_block))
        return out


class SfGridHeader(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("voxel_size", C.c_float), ("lo_voxel", C.c_int32 * 3),
                ("world2grid", C.c_float * 16), ("frames_used", C.c_uint64)]


def _lib():
    L = _abi.lib()
    vp = C.c_void_p
    L.sf_freespace_params_default.argtypes = [C.POINTER(SfFreespaceParams)]
    L.sf_freespace_params_default.restype = None
    L.sf_freespace_plan.argtypes = [vp, C.POINTER(SfFreespaceParams), C.POINTER(SfParams), vp, vp]
    L.sf_freespace_sens.argtypes = [vp, C.POINTER(SfFreespaceParams), C.c_int, C.c_int, C.POINTER(vp), C.POINTER(SfFreespaceStats)]
    L.sf_grid_create.argtypes = [C.POINTER(SfGridHeader), vp, vp, C.POINTER(vp)]
    L.sf_grid_info.argtypes = [vp, C.POINTER(SfGridHeader)]
    L.sf_grid_data.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sf_grid_save.argtypes = [vp, C.c_char_p]
    L.sf_grid_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.sf_grid_free.argtypes = [vp]
    L.sf_grid_free.restype = None
    return L


def default_params(**over):
    """sf_freespace_params_default, then the keyword overrides (voxel_size, max_blocks, every, params_file)."""
    p = SfFreespaceParams()
    _lib().sf_freespace_params_default(C.byref(p))
    for k, v in over.items():
        if k == "params_file":
            v = os.fsencode(v) if v else b""
            if len(v) >= 1024:
                raise ValueError("params_file is too long")
        elif not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def world2grid(voxel_size, lo_voxel):
    """g = w / voxel_size - lo_voxel + 0.5 as a 4 x 4 float32 matrix: floor(g) is the nearest lattice node."""
    m = np.zeros((4, 4), np.float32)
    for a in range(3):
        m[a, a] = np.float32(1.0) / np.float32(voxel_size)
        m[a, 3] = np.float32(0.5) - np.float32(lo_voxel[a])
    m[3, 3] = 1.0
    return m


class Grid:
    """value float32 [nz, ny, nx] (sdf / voxel_size, -inf where nothing was observed), weight uint8 [nz, ny, nx], world2grid float32 [4, 4]."""

    def __init__(self, value, weight, voxel_size, lo_voxel, frames_used=0, world2grid_matrix=None):
        self.value = np.ascontiguousarray(value, np.float32)
        self.weight = np.ascontiguousarray(weight, np.uint8)
        if self.value.ndim != 3 or self.value.shape != self.weight.shape:
            raise ValueError("value and weight must be [nz, ny, nx] arrays of one shape")
        self.voxel_size = float(np.float32(voxel_size))
        self.lo_voxel = np.asarray(lo_voxel, np.int32).reshape(3).copy()
        self.frames_used = int(frames_used)
        self.world2grid = world2grid(voxel_size, self.lo_voxel) if world2grid_matrix is None else np.asarray(world2grid_matrix, np.float32).reshape(4, 4).copy()

    @property
    def known(self):
        """bool [nz, ny, nx]: some frame observed the voxel (weight > 0; the same set as value >= -1's finite values, provider.lua:80-97)."""
        return self.weight > 0

    def _header(self):
        h = SfGridHeader()
        h.nz, h.ny, h.nx = self.value.shape
        h.voxel_size = self.voxel_size
        h.lo_voxel[:] = [int(v) for v in self.lo_voxel]
        h.world2grid[:] = [float(v) for v in self.world2grid.reshape(16)]
        h.frames_used = self.frames_used
        return h

    def save(self, path):
        save_grid(self, path)

    def save_npy(self, prefix):
        """<prefix>.grid.npy ([z][y][x] float32) and <prefix>.world2grid.npy (4 x 4): the pair export_semantic_label_grid_for_evaluation.py loads."""
        np.save(prefix + ".grid.npy", self.value)
        np.save(prefix + ".world2grid.npy", self.world2grid)
        return prefix + ".grid.npy", prefix + ".world2grid.npy"


def _from_handle(h):
    L = _lib()
    try:
        hd = SfGridHeader()
        check(L.sf_grid_info(h, C.byref(hd)))
        pv, pw = C.c_void_p(), C.c_void_p()
        check(L.sf_grid_data(h, C.byref(pv), C.byref(pw)))
        n = hd.nx * hd.ny * hd.nz
        shape = (hd.nz, hd.ny, hd.nx)
        if n:
            value = np.frombuffer(C.string_at(pv, n * 4), np.float32).reshape(shape).copy()
            weight = np.frombuffer(C.string_at(pw, n), np.uint8).reshape(shape).copy()
        else:
            value, weight = np.zeros(shape, np.float32), np.zeros(shape, np.uint8)
        return Grid(value, weight, hd.voxel_size, list(hd.lo_voxel), hd.frames_used, np.array(hd.world2grid, np.float32))
    finally:
        L.sf_grid_free(h)


def load_grid(path):
    h = C.c_void_p()
    check(_lib().sf_grid_load(os.fsencode(path), C.byref(h)))
    return _from_handle(h)


def save_grid(grid, path):
    L = _lib()
    hd = grid._header()
    h = C.c_void_p()
    check(L.sf_grid_create(C.byref(hd), grid.value.ctypes.data_as(C.c_void_p), grid.weight.ctypes.data_as(C.c_void_p), C.byref(h)))
    try:
        check(L.sf_grid_save(h, os.fsencode(path)))
    finally:
        L.sf_grid_free(h)


def plan(sensor_data, params=None):
    """sf_freespace_plan -> (fuser parameters, lo_block int32 [3], hi_block int32 [3]): the inclusive box of blocks the scan's frames can update."""
    p = params if params is not None else default_params()
    fp = SfParams()
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    check(_lib().sf_freespace_plan(sensor_data._h, C.byref(p), C.byref(fp), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    return fp, lo, hi


def carve_sens(sensor_data, params=None, device=0, decode_threads=0, stats=False):
    """sf_freespace_sens -> Grid (with stats: (Grid, dict)).  Raises ScanfuseError (SF_ERR_DEVICE) without a GPU: there is no host fall-back."""
    p = params if params is not None else default_params()
    st = SfFreespaceStats()
    h = C.c_void_p()
    check(_lib().sf_freespace_sens(sensor_data._h, C.byref(p), int(device), int(decode_threads), C.byref(h), C.byref(st)))
    g = _from_handle(h)
    return (g, st.as_dict()) if stats else g


def lookup(grid, vertices):
    """The per-vertex read of export_semantic_label_grid_for_evaluation.py:40-47: world2grid applied to [n, 3] world positions, floor, clamp into
    the grid, value[z, y, x] -> float32 [n]."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    value = grid.value if isinstance(grid, Grid) else np.asarray(grid[0])
    m = grid.world2grid if isinstance(grid, Grid) else np.asarray(grid[1], np.float32)
    if value.size == 0:
        raise ValueError("the grid is empty")
    g = np.concatenate([v, np.ones((len(v), 1), np.float32)], 1) @ m.T
    idx = np.floor(g[:, :3]).astype(np.int64)
    nz, ny, nx = value.shape
    x = np.clip(idx[:, 0], 0, nx - 1)
    y = np.clip(idx[:, 1], 0, ny - 1)
    z = np.clip(idx[:, 2], 0, nz - 1)
    return value[z, y, x]
