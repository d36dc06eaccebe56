"""Mesh cleaning -- host-side mirror of the meshlabserver clean step (Server/scan_processor.py:134,143 with
Server/tools/meshclean/clean.mlx / cleanLoRes.mlx) over the C ABI."""
import ctypes as C
import os

from . import _abi
from ._abi import check
from .segmentator import Mesh

CLEAN_MLX_MERGE_DISTANCE = 0.0010689   # clean.mlx:4 (absolute)
CLEAN_MLX_MIN_COMPONENT = 7500         # clean.mlx:8
CLEAN_LORES_MIN_COMPONENT = 1000       # cleanLoRes.mlx:8


class SfCleanStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("vertices_in", "faces_in", "vertices_merged", "faces_degenerate", "faces_duplicate",
                                          "components_in", "components_removed", "faces_small_component", "vertices_unreferenced",
                                          "vertices_out", "faces_out")]


class SfSimplifyParams(C.Structure):
    """simplify.mlx:3-16 ("Quadric Edge Collapse Decimation")."""
    _fields_ = [("target_faces", C.c_uint64), ("target_perc", C.c_float), ("quality_thr", C.c_float), ("preserve_boundary", C.c_int32),
                ("boundary_weight", C.c_float), ("preserve_normal", C.c_int32), ("preserve_topology", C.c_int32),
                ("optimal_placement", C.c_int32), ("planar_quadric", C.c_int32), ("quality_weight", C.c_int32), ("auto_clean", C.c_int32)]


class SfSimplifyStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("vertices_in", "faces_in", "target_faces", "collapses", "stale_popped", "faces_zero_area",
                                          "vertices_duplicate", "vertices_out", "faces_out")] + [("max_priority", C.c_float), ("rounds", C.c_uint32)]


class SfCleanScript(C.Structure):
    _fields_ = [("merge_close_vertices", C.c_int32), ("remove_duplicate_faces", C.c_int32), ("remove_small_components", C.c_int32),
                ("remove_unreferenced", C.c_int32), ("merge_distance", C.c_float), ("min_component_faces", C.c_uint32),
                ("simplify", C.c_int32), ("simplify_params", SfSimplifyParams), ("simplify_stats", SfSimplifyStats), ("simplify_device", C.c_int32), ("clean_device", C.c_int32)]


def _lib():
    L = _abi.lib()
    vp = C.c_void_p
    L.sf_mesh_clean.argtypes = [vp, C.c_float, C.c_uint32, C.POINTER(vp), C.POINTER(SfCleanStats)]
    L.sf_mlx_load.argtypes = [C.c_char_p, C.POINTER(SfCleanScript)]
    L.sf_mesh_clean_script.argtypes = [vp, C.POINTER(SfCleanScript), C.POINTER(vp), C.POINTER(SfCleanStats)]
    L.sf_simplify_default_params.argtypes = [C.POINTER(SfSimplifyParams)]
    L.sf_simplify_default_params.restype = None
    L.sf_mesh_simplify.argtypes = [vp, C.POINTER(SfSimplifyParams), C.POINTER(vp), C.POINTER(SfSimplifyStats)]
    return L


def simplify(mesh, gpu=None, **overrides):
    """"Quadric Edge Collapse Decimation" with simplify.mlx's parameters (keep 20 % of the faces) unless overridden;
    returns (Mesh, stats dict).  gpu=<device>: rounds of independent collapses on that GPU (sf_mesh_simplify_gpu) instead of the
    sequential host filter -- different triangles, same guarantees, a fraction of the time."""
    p = SfSimplifyParams()
    _lib().sf_simplify_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError("unknown simplify parameter %r" % k)
        setattr(p, k, v)
    h, st = C.c_void_p(), SfSimplifyStats()
    if gpu is None:
        check(_lib().sf_mesh_simplify(mesh._h, C.byref(p), C.byref(h), C.byref(st)))
    else:
        L = _lib()
        L.sf_mesh_simplify_gpu.argtypes = [C.c_void_p, C.POINTER(SfSimplifyParams), C.c_int, C.POINTER(C.c_void_p), C.POINTER(SfSimplifyStats)]
        check(L.sf_mesh_simplify_gpu(mesh._h, C.byref(p), int(gpu), C.byref(h), C.byref(st)))
    return Mesh(h), {n: getattr(st, n) for n, _ in SfSimplifyStats._fields_}


def clean(mesh, merge_distance=CLEAN_MLX_MERGE_DISTANCE, min_component_faces=CLEAN_MLX_MIN_COMPONENT, gpu=None):
    """The four clean.mlx filters on a Mesh; returns (Mesh, stats dict).  gpu=<device>: the same filters on that GPU (sf_mesh_clean_gpu),
    identical arrays and statistics."""
    h, st = C.c_void_p(), SfCleanStats()
    if gpu is None:
        check(_lib().sf_mesh_clean(mesh._h, float(merge_distance), int(min_component_faces), C.byref(h), C.byref(st)))
    else:
        L = _lib()
        L.sf_mesh_clean_gpu.argtypes = [C.c_void_p, C.c_float, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.POINTER(SfCleanStats)]
        check(L.sf_mesh_clean_gpu(mesh._h, float(merge_distance), int(min_component_faces), int(gpu), C.byref(h), C.byref(st)))
    return Mesh(h), {n: getattr(st, n) for n, _ in SfCleanStats._fields_}


def load_script(path):
    s = SfCleanScript()
    check(_lib().sf_mlx_load(os.fsencode(path), C.byref(s)))
    return s


def clean_file(in_ply, out_ply, script_mlx):
    """meshlabserver -i in_ply -o out_ply -m vc -s script_mlx"""
    s = load_script(script_mlx)
    m = Mesh.read(in_ply)
    h, st = C.c_void_p(), SfCleanStats()
    check(_lib().sf_mesh_clean_script(m._h, C.byref(s), C.byref(h), C.byref(st)))
    out = Mesh(h)
    out.write_ply(out_ply)
    out.close()
    m.close()
    res = {n: getattr(st, n) for n, _ in SfCleanStats._fields_}
    if s.simplify:
        res["simplify"] = {n: getattr(s.simplify_stats, n) for n, _ in SfSimplifyStats._fields_}
    return res


# ---- stage hooks of the GPU decimation (include/scanfuse_internal.h; tests/test_simplify_stages.py): one part of a round of sf_mesh_simplify_gpu on
# host arrays, launched through the helpers its round loop calls.  Same argument and result layout as oracle.simplify_stage_*.
def _stage_params(overrides):
    p = SfSimplifyParams()
    _lib().sf_simplify_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError("unknown simplify parameter %r" % k)
        setattr(p, k, v)
    return p


def _stage_mesh(xyz, tris, alive):
    import numpy as np
    t = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    v = None if xyz is None else np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    a = np.ones(len(t), np.uint8) if alive is None else np.ascontiguousarray(alive, np.uint8).reshape(-1)
    if len(a) != len(t):
        raise ValueError("one alive byte per face")
    return v, t, a


def stage_edges(xyz, tris, alive=None, Q=None, scale=0.0, needed=0, stalled=0, device=0, **overrides):
    """Adjacency, initial quadrics (Q is None), priorities and the threshold of one round -> {"E", "ukey", "ucnt", "Q", "pri", "x", "tau", "scale"}."""
    import numpy as np
    L = _lib()
    vp = C.c_void_p
    L.sf_simplify_stage_edges.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(SfSimplifyParams), C.c_double, C.c_uint64, C.c_int,
                                          C.POINTER(C.c_uint32), vp, vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    p = _stage_params(overrides)
    v, t, a = _stage_mesh(xyz, tris, alive)
    q = None if Q is None else np.ascontiguousarray(Q, np.float64).reshape(len(v), 10)
    n = 3 * len(t)
    ukey, ucnt, pri, x, Qo = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((len(v), 10), np.float64)
    E, tau, sc = C.c_uint32(0), C.c_float(0), C.c_double(0)
    check(L.sf_simplify_stage_edges(int(device), len(v), len(t), v.ctypes.data, t.ctypes.data, a.ctypes.data, None if q is None else q.ctypes.data, C.byref(p),
                                    float(scale), int(needed), int(stalled), C.byref(E), ukey.ctypes.data, ucnt.ctypes.data, Qo.ctypes.data, pri.ctypes.data,
                                    x.ctypes.data, C.byref(tau), C.byref(sc)))
    e = E.value
    return {"E": e, "ukey": ukey[:e], "ucnt": ucnt[:e], "Q": Qo, "pri": pri[:e], "x": x[:e], "tau": np.float32(tau.value), "scale": sc.value}


def stage_winners(nv, tris, alive, pri, tau, round_no, device=0):
    """The three winner passes of round `round_no` on the caller's priorities -> {"passes" (0 = no win, 1..3), "taken", "counters"}."""
    import numpy as np
    L = _lib()
    vp = C.c_void_p
    L.sf_simplify_stage_winners.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, C.c_float, C.c_uint32, vp, vp, vp]
    _, t, a = _stage_mesh(None, tris, alive)
    p = np.ascontiguousarray(pri, np.float32).reshape(-1)
    passes, taken, cnt = np.zeros(len(p), np.uint8), np.zeros(nv, np.uint8), np.zeros(3, np.uint32)
    check(L.sf_simplify_stage_winners(int(device), int(nv), len(t), t.ctypes.data, a.ctypes.data, len(p), p.ctypes.data, float(tau), int(round_no),
                                      passes.ctypes.data, taken.ctypes.data, cnt.ctypes.data))
    return {"passes": passes, "taken": taken, "counters": cnt}


def stage_collapse(xyz, tris, alive, Q, edges, x, device=0):
    """Collapse the (independent) edges named -> {"pos", "tri", "alive", "Q", "vdel"}: copies, the arguments are left alone."""
    import numpy as np
    L = _lib()
    vp = C.c_void_p
    L.sf_simplify_stage_collapse.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp]
    v, t, a = _stage_mesh(xyz, tris, alive)
    v, t, a = v.copy(), t.copy(), a.copy()
    q = np.array(Q, np.float64).reshape(len(v), 10)
    ed = np.ascontiguousarray(edges, np.uint32).reshape(-1)
    xs = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    vdel = np.zeros(len(v), np.uint8)
    check(L.sf_simplify_stage_collapse(int(device), len(v), len(t), v.ctypes.data, t.ctypes.data, a.ctypes.data, q.ctypes.data, len(ed), ed.ctypes.data, len(xs),
                                       xs.ctypes.data, vdel.ctypes.data))
    return {"pos": v, "tri": t, "alive": a, "Q": q, "vdel": vdel}


# ---- stage hooks of the GPU mesh clean (include/scanfuse_internal.h; tests/test_clean_stages.py): one of the four helpers sf_mesh_clean_gpu is the
# composition of, on host arrays.  Same result layout as tests/clean_exact.py.  An error code of the library comes back as ScanfuseError(.code).
def clean_stage_merge(xyz, radius, device=0):
    """Filter 1 -> {"target", "launches" (k_settle), "cells" (occupied), "merged" (k_count_merged)}."""
    import numpy as np
    L = _lib()
    vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)
    L.sf_clean_stage_merge.argtypes = [C.c_int, C.c_uint32, vp, C.c_float, vp, u32p, u32p, u32p]
    v = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    target = np.zeros(len(v), np.uint32)
    launches, cells, merged = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(L.sf_clean_stage_merge(int(device), len(v), v.ctypes.data, float(radius), target.ctypes.data, C.byref(launches), C.byref(cells), C.byref(merged)))
    return {"target": target, "launches": launches.value, "cells": cells.value, "merged": merged.value}


def clean_probe_merge(xyz, radius):
    """The host filter's clustering alone (clean.cpp's merge_close) -> target[V]."""
    import numpy as np
    L = _lib()
    L.sf_clean_probe_merge.argtypes = [C.c_uint32, C.c_void_p, C.c_float, C.c_void_p]
    v = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    target = np.zeros(len(v), np.uint32)
    check(L.sf_clean_probe_merge(len(v), v.ctypes.data, float(radius), target.ctypes.data))
    return target


def clean_stage_faces(nv, tris, target=None, device=0):
    """Degenerate and duplicate faces through the caller's target (None: nobody merged; nv may then be anything below 0xFFFFFFF0)
    -> {"verdict" (0 kept, 1 degenerate, 2 duplicate), "tri", "degenerate", "duplicate"}."""
    import numpy as np
    L = _lib()
    vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)
    L.sf_clean_stage_faces.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, u32p, u32p]
    t = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    tg = None if target is None else np.ascontiguousarray(target, np.uint32).reshape(-1)
    if tg is not None and len(tg) != nv:
        raise ValueError("one target per vertex")
    verdict, out = np.zeros(len(t), np.uint8), np.zeros((len(t), 3), np.uint32)
    deg, dup = C.c_uint32(0), C.c_uint32(0)
    check(L.sf_clean_stage_faces(int(device), int(nv), len(t), t.ctypes.data, None if tg is None else tg.ctypes.data, verdict.ctypes.data, out.ctypes.data,
                                 C.byref(deg), C.byref(dup)))
    return {"verdict": verdict, "tri": out[:len(t) - deg.value - dup.value].copy(), "degenerate": deg.value, "duplicate": dup.value}


def clean_stage_components(tris, min_faces, device=0):
    """-> {"root", "size" (of each face's component), "keep", "counters" {components, components below min_faces, faces in them}}."""
    import numpy as np
    L = _lib()
    vp = C.c_void_p
    L.sf_clean_stage_components.argtypes = [C.c_int, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp]
    t = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    root, size, keep, cnt = np.zeros(len(t), np.uint32), np.zeros(len(t), np.uint32), np.zeros(len(t), np.uint8), np.zeros(3, np.uint32)
    check(L.sf_clean_stage_components(int(device), len(t), t.ctypes.data, int(min_faces), root.ctypes.data, size.ctypes.data, keep.ctypes.data, cnt.ctypes.data))
    return {"root": root, "size": size[root], "keep": keep, "counters": cnt}


def clean_stage_compact(xyz, rgba, tris, device=0):
    """-> {"used", "remap", "pos", "col" (None without colour), "tri", "vertices_out"}."""
    import numpy as np
    L = _lib()
    vp = C.c_void_p
    L.sf_clean_stage_compact.argtypes = [C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint32)]
    v = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    c = None if rgba is None else np.ascontiguousarray(rgba, np.uint8).reshape(len(v), 4)
    t = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    used, remap = np.zeros(len(v), np.uint32), np.zeros(len(v), np.uint32)
    pos, col, tri = np.zeros((len(v), 3), np.float32), np.zeros((len(v), 4), np.uint8), np.zeros((len(t), 3), np.uint32)
    n = C.c_uint32(0)
    check(L.sf_clean_stage_compact(int(device), len(v), len(t), v.ctypes.data, None if c is None else c.ctypes.data, t.ctypes.data if len(t) else None,
                                   used.ctypes.data, remap.ctypes.data, pos.ctypes.data, col.ctypes.data, tri.ctypes.data if len(t) else None, C.byref(n)))
    return {"used": used, "remap": remap, "pos": pos[:n.value].copy(), "col": None if c is None else col[:n.value].copy(), "tri": tri, "vertices_out": n.value}
