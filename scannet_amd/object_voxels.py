"""Object-task data from a scan: an occupancy and a known grid per annotated object over the C ABI (include/scanfuse.h "Object-task data";
scannet_amd/csrc/object_voxels.cpp, object_voxels.hip; the rule is DESIGN.md section 4n).  The known channel reads the freespace stage's grid
(`freespace.Grid`).  What reads the result in the reference tree: Tasks/ObjectClassification/torch/provider.lua:40-47 and
Tasks/ObjectRetrieval/generate_feat.lua:74-81,101-109 (datasets `data` [n, 2, 30, 30, 30] and `label` [n]).

`device=None` is the host path (at most 16 threads), an int runs the kernels on that GPU: the bytes are the same."""
import ctypes as C
import os

import numpy as np

from . import _abi, freespace
from ._abi import check


class SfObjvoxParams(C.Structure):
    _fields_ = [("dim", C.c_int32), ("fit", C.c_int32), ("min_faces", C.c_int32), ("all_objects", C.c_int32), ("reserved", C.c_int32 * 12)]


def _lib():
    L = _abi.lib()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    P = C.POINTER(SfObjvoxParams)
    L.sf_annotation_vertex_objects.argtypes = [C.c_char_p, C.c_char_p, u64, vp, C.POINTER(u32), C.POINTER(vp)]
    L.sf_objvox_classes.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, u32, vp]
    L.sf_objvox_params_default.argtypes = [P]
    L.sf_objvox_params_default.restype = None
    L.sf_objvox_plan.argtypes = [vp, u64, vp, u64, vp, vp, u32, P, vp, vp, vp, u64, C.POINTER(u64)]
    L.sf_objvox_voxelize.argtypes = [vp, u64, vp, u64, vp, vp, u32, vp, P, C.c_int, u64, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]
    L.sf_objvox_stage_faces.argtypes = [vp, u64, vp, u64, vp, u32, C.c_int, vp, vp, vp, vp, u64, C.POINTER(u64)]   # include/scanfuse_internal.h
    L.sf_objvox_kernel_us.argtypes = [C.POINTER(C.c_float)] * 3                                                     # include/scanfuse_internal.h
    L.sf_free.argtypes = [vp]
    L.sf_free.restype = None
    freespace._lib()
    return L


def default_params(**over):
    """sf_objvox_params_default, then the keyword overrides (dim, fit, min_faces, all_objects)."""
    p = SfObjvoxParams()
    _lib().sf_objvox_params_default(C.byref(p))
    for k, v in over.items():
        if k not in ("dim", "fit", "min_faces", "all_objects"):
            raise AttributeError(k)
        setattr(p, k, int(v))
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


def _mesh(xyz, tris, vertex_object):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    vo = np.ascontiguousarray(vertex_object, np.uint32).reshape(-1)
    if len(vo) != len(xyz):
        raise ValueError("one object value per vertex")
    return xyz, tris, vo


def vertex_objects(segs_json, aggregation_json, num_vertices):
    """sf_annotation_vertex_objects -> (vertex_object uint32 [V]: objectId + 1, 0 without a group; num_objects; {objectId: label string})."""
    L = _lib()
    vo = np.zeros(int(num_vertices), np.uint32)
    n, text = C.c_uint32(0), C.c_void_p()
    check(L.sf_annotation_vertex_objects(os.fsencode(str(segs_json)), os.fsencode(str(aggregation_json)), int(num_vertices), _ptr(vo), C.byref(n), C.byref(text)))
    try:
        raw = C.string_at(text).decode("utf-8", "replace") if text.value else ""
    finally:
        L.sf_free(text)
    names = {}
    for line in raw.split("\n"):
        if line:
            i, _, name = line.partition("\t")
            names[int(i)] = name
    return vo, n.value, names


def labels_text(names):
    """{objectId: label} -> the "objectId<TAB>label" lines sf_objvox_classes reads"""
    return "".join("%d\t%s\n" % (i, names[i]) for i in sorted(names))


def classes(names, label_map_tsv, classes_txt, num_objects, label_from=None, label_to=None):
    """sf_objvox_classes -> object_class int32 [num_objects], -1 where the object has no class.  names: {objectId: label} or the text itself."""
    text = names if isinstance(names, str) else labels_text(names)
    out = np.full(int(num_objects), -1, np.int32)
    enc = lambda s: None if s is None else str(s).encode()
    check(_lib().sf_objvox_classes(text.encode(), os.fsencode(str(label_map_tsv)), os.fsencode(str(classes_txt)), enc(label_from), enc(label_to), int(num_objects),
                                   _ptr(out)))
    return out


def _classes_arg(object_class):
    oc = np.ascontiguousarray(object_class, np.int32).reshape(-1)
    return oc, len(oc)


def plan(xyz, tris, vertex_object, object_class, params=None):
    """sf_objvox_plan -> (object_id int32 [n], origin float32 [n, 3], cell float32 [n]): the objects voxelize keeps, ascending."""
    L = _lib()
    p = params if params is not None else default_params()
    xyz, tris, vo = _mesh(xyz, tris, vertex_object)
    oc, nobj = _classes_arg(object_class)
    count = C.c_uint64(0)
    args = (_ptr(xyz), len(xyz), _ptr(tris), len(tris), _ptr(vo), _ptr(oc), nobj, C.byref(p))
    check(L.sf_objvox_plan(*args, None, None, None, 0, C.byref(count)))
    n = count.value
    oid, origin, cell = np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    check(L.sf_objvox_plan(*args, _ptr(oid), _ptr(origin), _ptr(cell), n, C.byref(count)))
    return oid, origin, cell


class ObjectSet:
    """What voxelize makes: data uint8 [n, 2, dim, dim, dim] ([c][z][y][x]; channel 0 occupancy, 1 known), label uint8 [n], object_id int32 [n]
    (objectId, ascending), origin float32 [n, 3], cell float32 [n]; total = the kept objects in all; names: {objectId: label} when known."""

    def __init__(self, data, label, object_id, origin, cell, total, names=None):
        self.data, self.label, self.object_id, self.origin, self.cell, self.total, self.names = data, label, object_id, origin, cell, total, names

    def __len__(self):
        return len(self.label)

    def save_npy(self, prefix):
        """<prefix>.objects.data.npy, .label.npy, .id.npy: the arrays under the dataset names `data` / `label` that provider.lua:40-47 reads (the .npy
        files are the hand-over: no HDF5 is written here); <prefix>.objects.names.txt: one `<prefix basename>_<objectId> <label>` line per sample, the
        --file_label_file of generate_feat.lua:87."""
        paths = [prefix + s for s in (".objects.data.npy", ".objects.label.npy", ".objects.id.npy", ".objects.names.txt")]
        for path, a in zip(paths, (self.data, self.label, self.object_id)):
            np.save(path, np.asarray(a))
        base = os.path.basename(prefix)
        with open(paths[3], "w") as f:
            for i in np.asarray(self.object_id):
                f.write("%s_%d %s\n" % (base, int(i), (self.names or {}).get(int(i), "")))
        return paths


def voxelize(xyz, tris, vertex_object, object_class, grid=None, params=None, device=None, first=0, max_objects=None, out=None, names=None):
    """sf_objvox_voxelize -> ObjectSet.  grid: a freespace.Grid or None (channel 1 all ones).  max_objects=None: all from `first` on.  out = (data,
    label, object_id, origin, cell): torch tensors on the device of the call, large enough for max_objects; they are written and returned whole."""
    L = _lib()
    p = params if params is not None else default_params()
    xyz, tris, vo = _mesh(xyz, tris, vertex_object)
    oc, nobj = _classes_arg(object_class)
    g = C.c_void_p()
    if grid is not None:
        hd = grid._header()
        check(L.sf_grid_create(C.byref(hd), grid.value.ctypes.data_as(C.c_void_p), grid.weight.ctypes.data_as(C.c_void_p), C.byref(g)))
    try:
        total = C.c_uint64(0)
        args = (_ptr(xyz), len(xyz), _ptr(tris), len(tris), _ptr(vo), _ptr(oc), nobj, g, C.byref(p), _dev(device))
        if max_objects is None:
            check(L.sf_objvox_voxelize(*args, 0, 0, None, None, None, None, None, C.byref(total)))
            max_objects = max(total.value - int(first), 0)
        cap = int(max_objects)
        d = max(int(p.dim), 0)
        if out is not None:
            data, label, oid, origin, cell = out
        elif cap:
            data, label, oid = np.empty((cap, 2, d, d, d), np.uint8), np.empty(cap, np.uint8), np.empty(cap, np.int32)
            origin, cell = np.empty((cap, 3), np.float32), np.empty(cap, np.float32)
        else:
            data = label = oid = origin = cell = None
        check(L.sf_objvox_voxelize(*args, int(first), cap, _ptr(data), _ptr(label), _ptr(oid), _ptr(origin), _ptr(cell), C.byref(total)))
    finally:
        if g.value:
            L.sf_grid_free(g)
    if out is not None:
        return ObjectSet(data, label, oid, origin, cell, total.value, names)
    if cap == 0:
        data, label, oid = np.empty((0, 2, d, d, d), np.uint8), np.empty(0, np.uint8), np.empty(0, np.int32)
        origin, cell = np.empty((0, 3), np.float32), np.empty(0, np.float32)
    n = min(cap, max(total.value - int(first), 0))
    return ObjectSet(data[:n], label[:n], oid[:n], origin[:n], cell[:n], total.value, names)


def stage_faces(xyz, tris, vertex_object, num_objects, device=None):
    """The key / scan / fill stage alone (sf_objvox_stage_faces) -> (face_object uint32 [F], counts uint32 [num_objects + 1], offsets, list uint32)."""
    L = _lib()
    xyz, tris, vo = _mesh(xyz, tris, vertex_object)
    n = int(num_objects) + 1
    fobj, counts, offsets = np.zeros(len(tris), np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    total = C.c_uint64(0)
    args = (_ptr(xyz), len(xyz), _ptr(tris), len(tris), _ptr(vo), int(num_objects), _dev(device))
    check(L.sf_objvox_stage_faces(*args, _ptr(fobj), _ptr(counts), _ptr(offsets), None, 0, C.byref(total)))
    lst = np.zeros(total.value, np.uint32)
    check(L.sf_objvox_stage_faces(*args, _ptr(fobj), _ptr(counts), _ptr(offsets), _ptr(lst), len(lst), C.byref(total)))
    return fobj, counts, offsets, lst


def kernel_us():
    """Device microseconds of this process's most recent device call: {group, raster, emit} (sf_objvox_kernel_us)."""
    a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
    check(_lib().sf_objvox_kernel_us(C.byref(a), C.byref(b), C.byref(c)))
    return dict(group=a.value, raster=b.value, emit=c.value)


def object_scan(xyz, tris, segs_json, aggregation_json, label_map_tsv, classes_txt, grid=None, params=None, device=None, label_from=None, label_to=None):
    """A scan's annotation files -> ObjectSet: vertex_objects, classes, voxelize.  device=None (the default) is the host path: the measured decision
    is in DESIGN.md section 4n."""
    vo, nobj, names = vertex_objects(segs_json, aggregation_json, len(np.asarray(xyz).reshape(-1, 3)))
    oc = classes(names, label_map_tsv, classes_txt, nobj, label_from, label_to)
    return voxelize(xyz, tris, vo, oc, grid, params, device, names=names)
