"""Voxel-task data from a scan: label grids and column samples over the C ABI (include/scanfuse.h "Voxel-task data"; scannet_amd/csrc/voxel_labels.cpp,
voxel_labels.hip; the rule is DESIGN.md section 4m).  The grid and its world2grid are the freespace stage's (`freespace.Grid`), the per-vertex ids are
`project.vertex_ids`, the read back out of a label grid is `freespace.lookup`.  What reads the result in the reference tree:
Tasks/SemanticVoxelLabeling/torch/provider.lua:59-97 (datasets `data` [n, 1, 62, 31, 31] and `label` [n, 62]; label 0 empty, 255 unannotated).

`device=None` is the host path (at most 16 threads), an int runs the kernels on that GPU: the bytes are the same."""
import ctypes as C

import numpy as np

from . import _abi, freespace
from ._abi import check

DEFAULT_BAND = float(np.float32(0.8660254))


class SfVoxlabelParams(C.Structure):
    _fields_ = [("band", C.c_float), ("wx", C.c_int32), ("wy", C.c_int32), ("wz", C.c_int32), ("z0", C.c_int32), ("z0_default", C.c_int32),
                ("stride", C.c_int32), ("reserved", C.c_int32 * 9)]


def _lib():
    L = _abi.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    H = C.POINTER(freespace.SfGridHeader)
    L.sf_voxlabel_params_default.argtypes = [C.POINTER(SfVoxlabelParams)]
    L.sf_voxlabel_params_default.restype = None
    L.sf_voxlabel_nearest_faces.argtypes = [H, vp, u64, vp, u64, C.c_float, C.c_int, vp, vp]
    L.sf_voxlabel_labels.argtypes = [vp, u64, vp, u64, u64, vp, vp, vp, vp, vp]
    L.sf_voxlabel_sample_columns.argtypes = [vp, vp, C.POINTER(SfVoxlabelParams), C.c_int, u64, u64, vp, vp, vp, C.POINTER(u64)]
    L.sf_voxlabel_stage_bins.argtypes = [H, vp, u64, vp, u64, C.c_float, C.c_int, vp, vp, vp, u64, C.POINTER(u64)]   # include/scanfuse_internal.h
    L.sf_voxlabel_kernel_us.argtypes = [C.POINTER(C.c_float)] * 3                                                      # include/scanfuse_internal.h
    freespace._lib()
    return L


def default_params(**over):
    """sf_voxlabel_params_default, then the keyword overrides (band, wx, wy, wz, z0, stride).  Setting z0 clears z0_default; z0=None sets it."""
    p = SfVoxlabelParams()
    _lib().sf_voxlabel_params_default(C.byref(p))
    for k, v in over.items():
        if k == "z0":
            p.z0_default = 1 if v is None else 0
            p.z0 = 0 if v is None else int(v)
        elif k in ("band", "wx", "wy", "wz", "stride", "z0_default"):
            setattr(p, k, v)
        else:
            raise AttributeError(k)
    return p


def _dev(device):
    return -1 if device is None else int(device)


def _ptr(a):
    """numpy array or an object with data_ptr() (a torch tensor on the device of the call) -> address"""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def header(dims, voxel_size, lo_voxel):
    """The geometry of a grid as the search reads it: dims = (nx, ny, nz)."""
    h = freespace.SfGridHeader()
    h.nx, h.ny, h.nz = (int(v) for v in dims)
    h.voxel_size = float(voxel_size)
    h.lo_voxel[:] = [int(v) for v in lo_voxel]
    h.world2grid[:] = [float(v) for v in freespace.world2grid(voxel_size, lo_voxel).reshape(16)] if voxel_size else [0.0] * 16
    return h


def _header_of(grid):
    return grid._header() if isinstance(grid, freespace.Grid) else grid


def _mesh(xyz, tris):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    return xyz, tris


def nearest_faces(grid, xyz, tris, band=DEFAULT_BAND, device=None, dist2=True, face_out=None, dist2_out=None):
    """sf_voxlabel_nearest_faces -> (face int32 [nz, ny, nx], dist2 float32 [nz, ny, nx] or None).  grid: a freespace.Grid or a header().  With a
    device, face_out / dist2_out may be torch tensors on it (int32 / float32, contiguous, one element per node): they are written and returned."""
    h = _header_of(grid)
    xyz, tris = _mesh(xyz, tris)
    shape = (h.nz, h.ny, h.nx)
    face = np.empty(shape, np.int32) if face_out is None else face_out
    d2 = dist2_out if dist2_out is not None else (np.empty(shape, np.float32) if dist2 else None)
    check(_lib().sf_voxlabel_nearest_faces(C.byref(h), _ptr(xyz), len(xyz), _ptr(tris), len(tris), float(band), _dev(device), _ptr(face), _ptr(d2)))
    return face, d2


def bins(grid, xyz, tris, band=DEFAULT_BAND, device=None):
    """The bin stage alone (sf_voxlabel_stage_bins) -> (counts uint32 [tz, ty, tx], offsets uint32 [tz, ty, tx], list int32 [total])."""
    h = _header_of(grid)
    xyz, tris = _mesh(xyz, tris)
    L = _lib()
    t = tuple((n + 7) // 8 for n in (h.nz, h.ny, h.nx))
    counts, offsets = np.zeros(t, np.uint32), np.zeros(t, np.uint32)
    total = C.c_uint64(0)
    args = (C.byref(h), _ptr(xyz), len(xyz), _ptr(tris), len(tris), float(band), _dev(device))
    check(L.sf_voxlabel_stage_bins(*args, _ptr(counts), _ptr(offsets), None, 0, C.byref(total)))
    lst = np.zeros(total.value, np.int32)
    check(L.sf_voxlabel_stage_bins(*args, _ptr(counts), _ptr(offsets), _ptr(lst), len(lst), C.byref(total)))
    return counts, offsets, lst


def kernel_us():
    """Device microseconds of this process's most recent device call: {bins, nearest, sample} (sf_voxlabel_kernel_us)."""
    b, n, s = C.c_float(0), C.c_float(0), C.c_float(0)
    check(_lib().sf_voxlabel_kernel_us(C.byref(b), C.byref(n), C.byref(s)))
    return dict(bins=b.value, nearest=n.value, sample=s.value)


def labels(face, tris, vertex_label, vertex_instance=None):
    """sf_voxlabel_labels -> (label uint16, instance uint8, byte_label uint8), each of face's shape.  A face takes the value two of its vertices share,
    else its first vertex's; byte_label is the task's: 0 empty, 255 unannotated (label 0 or above 254)."""
    face = np.ascontiguousarray(face, np.int32)
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    vl = np.ascontiguousarray(vertex_label, np.uint16).reshape(-1)
    vi = None if vertex_instance is None else np.ascontiguousarray(vertex_instance, np.uint8).reshape(-1)
    if vi is not None and len(vi) != len(vl):
        raise ValueError("one instance per vertex label")
    label, inst, bl = np.empty(face.shape, np.uint16), np.zeros(face.shape, np.uint8), np.empty(face.shape, np.uint8)
    check(_lib().sf_voxlabel_labels(_ptr(face), face.size, _ptr(tris), len(tris), len(vl), _ptr(vl), _ptr(vi), _ptr(label), _ptr(inst) if vi is not None else None,
                                    _ptr(bl)))
    return label, inst, bl


def count_columns(grid, byte_label, params=None, device=None):
    """How many columns sample_columns would return in all."""
    return sample_columns(grid, byte_label, params, device, 0, 0)[3]


def sample_columns(grid, byte_label, params=None, device=None, first=0, max_samples=None, out=None):
    """sf_voxlabel_sample_columns -> (data float32 [n, 1, wz, wy, wx], label uint8 [n, wz], xy int32 [n, 2], total).  max_samples=None: all from
    `first` on.  out = (data, label, xy): torch tensors on the device of the call, large enough for max_samples; they are written and returned whole."""
    L = _lib()
    p = params if params is not None else default_params()
    bl = np.ascontiguousarray(byte_label, np.uint8)
    if bl.shape != grid.value.shape:
        raise ValueError("byte_label must have the grid's shape")
    hd = grid._header()
    g = C.c_void_p()
    check(L.sf_grid_create(C.byref(hd), grid.value.ctypes.data_as(C.c_void_p), grid.weight.ctypes.data_as(C.c_void_p), C.byref(g)))
    try:
        total = C.c_uint64(0)
        if max_samples is None:
            check(L.sf_voxlabel_sample_columns(g, _ptr(bl), C.byref(p), _dev(device), 0, 0, None, None, None, C.byref(total)))
            max_samples = max(total.value - int(first), 0)
        n_cap = int(max_samples)
        if out is not None:
            data, label, xy = out
        else:
            data = np.empty((n_cap, 1, p.wz, p.wy, p.wx), np.float32) if n_cap else None
            label = np.empty((n_cap, p.wz), np.uint8) if n_cap else None
            xy = np.empty((n_cap, 2), np.int32) if n_cap else None
        check(L.sf_voxlabel_sample_columns(g, _ptr(bl), C.byref(p), _dev(device), int(first), n_cap, _ptr(data), _ptr(label), _ptr(xy), C.byref(total)))
    finally:
        L.sf_grid_free(g)
    if out is not None:
        return data, label, xy, total.value
    n = min(n_cap, max(total.value - int(first), 0))
    if n_cap == 0:
        data, label, xy = np.empty((0, 1, p.wz, p.wy, p.wx), np.float32), np.empty((0, p.wz), np.uint8), np.empty((0, 2), np.int32)
    return data[:n], label[:n], xy[:n], total.value


class LabelledScan:
    """What label_scan makes: face int32, label uint16, instance uint8, byte_label uint8, each [nz, ny, nx] over `grid`."""

    def __init__(self, grid, face, label, instance, byte_label, params, device):
        self.grid, self.face, self.label, self.instance, self.byte_label = grid, face, label, instance, byte_label
        self.params, self.device = params, device

    def samples(self, first=0, max_samples=None):
        return sample_columns(self.grid, self.byte_label, self.params, self.device, first, max_samples)

    def lookup(self, vertices, what="label"):
        """The per-vertex read of export_semantic_label_grid_for_evaluation.py:40-47 over one of the grids (freespace.lookup)."""
        return freespace.lookup((getattr(self, what), self.grid.world2grid), vertices)

    def save_npy(self, prefix, max_samples=None):
        """<prefix>.label.npy and <prefix>.instance.npy ([z][y][x]); <prefix>.samples.data.npy and <prefix>.samples.label.npy, the arrays under the
        dataset names `data` / `label` that provider.lua:59-60 reads (the .npy pair is the hand-over: no HDF5 is written here)."""
        data, label, _, _ = self.samples(0, max_samples)
        paths = [prefix + s for s in (".label.npy", ".instance.npy", ".samples.data.npy", ".samples.label.npy")]
        for path, a in zip(paths, (self.label, self.instance, data, label)):
            np.save(path, a)
        return paths


def label_scan(grid, xyz, tris, vertex_label, vertex_instance=None, params=None, device=None):
    """Mesh -> grid: the nearest face of every node within the band, then its labels.  device=None (the default) is the host path: the measured
    decision is in DESIGN.md section 4m."""
    p = params if params is not None else default_params()
    face, _ = nearest_faces(grid, xyz, tris, p.band, device, dist2=False)
    label, inst, bl = labels(face, tris, vertex_label, vertex_instance)
    return LabelledScan(grid, face, label, inst, bl, p, device)
