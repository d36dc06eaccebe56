"""Axis alignment -- host-side mirror of Alignment::alignScan (Alignment/src/alignment.h:154-308; the `alignment.exe <scan dir>` call of
Server/scan_processor.py:132-135) over the C ABI: `estimate(mesh, sens)` returns the transform of a scan from its surface and trajectory,
`align_scan(dir)` does the reference's whole stage on a scan folder.  The rule is DESIGN.md section 4i."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import check


class SfAxisAlignParams(C.Structure):
    _fields_ = [("merge_distance", C.c_float), ("min_piece_faces", C.c_uint32), ("gravity_min_records", C.c_uint32),
                ("cluster_normal_thresh", C.c_float), ("cluster_dist_thresh", C.c_float), ("min_cluster_points", C.c_uint32),
                ("behind_dist", C.c_float), ("behind_max", C.c_uint32), ("floor_normal_z", C.c_float), ("floor_inlier_dist", C.c_float),
                ("reserved", C.c_int32 * 6)]


class SfAxisAlignStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("vertices", "faces", "clusters_founded", "clusters_after_small", "clusters_kept", "floor_points",
                                          "floor_inliers", "frames_without_gravity", "imu_records_dropped")] + [
        ("up_source", C.c_int32), ("floor_found", C.c_int32),
        ("gpu_batches", C.c_uint64), ("gpu_dirty_evaluations", C.c_uint64), ("gpu_fallback_rescans", C.c_uint64),
        ("outcome", C.c_int32), ("reverted", C.c_int32), ("transform", C.c_float * 16), ("seconds", C.c_double * 6),
        ("gpu_seconds_match", C.c_double), ("gpu_seconds_commit", C.c_double)]


OUTCOMES = ("aligned", "no processed.txt", "valid = false", "aligned already", "frame 0's pose is -inf")
SECONDS = ("cleaning", "normals", "clustering", "behind counts", "covariance", "rest")


def _lib():
    L = _abi.lib()
    vp = C.c_void_p
    L.sf_axis_align_params_default.argtypes = [C.POINTER(SfAxisAlignParams)]
    L.sf_axis_align_params_default.restype = None
    L.sf_axis_align_estimate.argtypes = [vp, vp, C.POINTER(SfAxisAlignParams), C.c_int, vp, C.POINTER(SfAxisAlignStats)]
    L.sf_mesh_apply_transform.argtypes = [vp, vp]
    L.sf_axis_align_scan.argtypes = [C.c_char_p, C.c_int, C.POINTER(SfAxisAlignParams), C.c_int, C.POINTER(SfAxisAlignStats)]
    return L


def default_params(**overrides):
    """The reference's constants (sf_axis_align_params_default) with the given fields replaced."""
    p = SfAxisAlignParams()
    _lib().sf_axis_align_params_default(C.byref(p))
    for k, v in overrides.items():
        if k == "reserved" or not hasattr(p, k):
            raise TypeError("unknown alignment parameter %r" % k)
        setattr(p, k, v)
    return p


def _stats(st):
    d = {n: getattr(st, n) for n, _ in SfAxisAlignStats._fields_ if n not in ("transform", "seconds")}
    d["transform"] = np.array(st.transform, np.float32).reshape(4, 4)
    d["seconds"] = dict(zip(SECONDS, st.seconds))
    d["outcome"] = OUTCOMES[st.outcome]
    return d


def estimate(mesh, sens, device=-1, params=None):
    """mesh: a segmentator.Mesh (the scan's <base>.ply), sens: a sens.SensorData; neither is changed.  Returns (4x4 float32 transform, stats
    dict).  device -1: the host path; >= 0: the vertex stages on that GPU, the same 16 floats."""
    t = np.zeros(16, np.float32)
    st = SfAxisAlignStats()
    check(_lib().sf_axis_align_estimate(mesh._h, sens._h, None if params is None else C.byref(params), int(device), t.ctypes.data_as(C.c_void_p), C.byref(st)))
    return t.reshape(4, 4), _stats(st)


def apply_transform(mesh, transform):
    """MeshDataf::applyTransform: every position of the Mesh through the affine part of the 4x4, in place."""
    t = np.ascontiguousarray(transform, np.float32).reshape(16)
    check(_lib().sf_mesh_apply_transform(mesh._h, t.ctypes.data_as(C.c_void_p)))


def align_scan(dir, force=False, device=-1, params=None):
    """Alignment::alignScan(dir, forceRealign) on a scan folder; returns the stats dict (its "outcome" says whether the folder was skipped)."""
    st = SfAxisAlignStats()
    check(_lib().sf_axis_align_scan(os.fsencode(dir), 1 if force else 0, None if params is None else C.byref(params), int(device), C.byref(st)))
    return _stats(st)
