"""Meshes, trajectories and call wrappers shared by tests/test_alignment.py (host path) and tests/test_alignment_gpu.py (kernels): the cases of
DESIGN.md section 4i, the checker tests/axis_align_checker.c compiled at test time, and thin ctypes wrappers of the stage hooks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from scannet_amd import _abi, alignment, sens
from scannet_amd.segmentator import Mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER_SRC = os.path.join(ROOT, "tests", "axis_align_checker.c")
TOOL = os.path.join(ROOT, "bin", "alignment")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the checker --------------------------------------------------------------------------------------------------------------------------------
class AacParams(C.Structure):
    _fields_ = [("nthr", C.c_float), ("dthr", C.c_float), ("min_points", C.c_uint32), ("behind_dist", C.c_float), ("behind_max", C.c_uint32),
                ("floor_z", C.c_float), ("floor_inlier", C.c_float)]


class AacResult(C.Structure):
    _fields_ = [("founded", C.c_uint64), ("after_small", C.c_uint64), ("kept", C.c_uint64), ("floor_inliers", C.c_uint64), ("floor", C.c_int64)]


class Checker:
    def __init__(self, directory):
        so = os.path.join(str(directory), "libaxis_align_checker.so")
        subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, CHECKER_SRC, "-lm"], check=True)
        self.L = C.CDLL(so)
        self.L.aac_cluster.restype = C.c_uint64
        self.L.aac_select.restype = C.c_uint64

    def up(self, poses, gravity=None):
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        g = None if gravity is None else np.ascontiguousarray(gravity, np.float64).reshape(-1, 3)
        out = np.zeros(3, np.float32)
        self.L.aac_up(_p(poses), C.c_uint64(len(poses)), _p(g), _p(out))
        return out

    def transform(self, xyz, m):
        out = np.array(xyz, np.float32, order="C", copy=True).reshape(-1, 3)
        m = np.ascontiguousarray(m, np.float32).reshape(16)
        bbox = np.zeros(6, np.float32)
        self.L.aac_transform(_p(out), C.c_uint64(len(out)), _p(m), _p(bbox))
        return out, bbox

    def normals(self, xyz, tris):
        out = np.zeros((len(xyz), 3), np.float32)
        self.L.aac_normals(_p(xyz), C.c_uint64(len(xyz)), _p(tris), C.c_uint64(len(tris)), _p(out))
        return out

    def planes(self, xyz, normals, p):
        """-> dict like stage_planes(): index, founded, ids, table, counts, behind of the clusters left by the sort and removeSmallClusters"""
        nv = len(xyz)
        index = np.zeros(nv, np.uint32)
        table = np.zeros((max(nv, 1), 10), np.float32)
        counts = np.zeros(max(nv, 1), np.uint32)
        ncl = self.L.aac_cluster(_p(xyz), _p(normals), C.c_uint64(nv), C.c_float(p.cluster_normal_thresh), C.c_float(p.cluster_dist_thresh), _p(index), _p(table), _p(counts))
        ids = np.zeros(max(ncl, 1), np.uint32)
        ns = self.L.aac_select(_p(counts), C.c_uint64(ncl), C.c_uint32(p.min_cluster_points), _p(ids))
        ids = ids[:ns].copy()
        reps = np.ascontiguousarray(table[ids, :4])
        return {"index": index, "founded": ncl, "ids": ids, "table": table[ids].copy(), "counts": counts[ids].copy(), "behind": self.behind(xyz, reps, p.behind_dist)}

    def behind(self, xyz, reps4, dist):
        reps4 = np.ascontiguousarray(reps4, np.float32).reshape(-1, 4)
        out = np.zeros(max(len(reps4), 1), np.uint32)
        self.L.aac_behind(_p(xyz), C.c_uint64(len(xyz)), _p(reps4), C.c_uint64(len(reps4)), C.c_float(dist), _p(out))
        return out[:len(reps4)]

    def cov(self, xyz, index, cluster, rep4, inlier):
        rep4 = np.ascontiguousarray(rep4, np.float32)
        out = np.zeros(10, np.float64)
        self.L.aac_cov(_p(xyz), _p(index), C.c_uint64(len(xyz)), C.c_uint32(cluster), _p(rep4), C.c_float(inlier), _p(out))
        return out

    def estimate(self, xyz, tris, up, p):
        """the cleaned mesh -> (4x4 transform, AacResult)"""
        work = np.array(xyz, np.float32, order="C", copy=True)
        up = np.ascontiguousarray(up, np.float32)
        ap = AacParams(p.cluster_normal_thresh, p.cluster_dist_thresh, p.min_cluster_points, p.behind_dist, p.behind_max, p.floor_normal_z, p.floor_inlier_dist)
        T, res = np.zeros(16, np.float32), AacResult()
        assert self.L.aac_estimate(_p(work), C.c_uint64(len(work)), _p(tris), C.c_uint64(len(tris)), _p(up), C.byref(ap), _p(T), C.byref(res)) == 0
        return T.reshape(4, 4), res


def have_gcc():
    return shutil.which("gcc") is not None


# ---- the stage hooks of include/scanfuse_internal.h -----------------------------------------------------------------------------------------------
def _L():
    L = _abi.lib()
    vp, u64 = C.c_void_p, C.c_uint64
    L.sf_axis_align_stage_up.argtypes = [vp, C.c_uint32, vp, C.POINTER(C.c_int32), C.POINTER(u64)]
    L.sf_axis_align_stage_normals.argtypes = [vp, u64, vp, u64, C.c_int, vp]
    L.sf_axis_align_stage_planes.argtypes = [vp, vp, u64, C.POINTER(alignment.SfAxisAlignParams), C.c_int, vp, C.POINTER(u64), vp, vp, vp, vp, u64, C.POINTER(u64), vp]
    L.sf_axis_align_stage_behind.argtypes = [vp, u64, vp, u64, C.c_float, C.c_int, vp]
    L.sf_axis_align_stage_cov.argtypes = [vp, vp, u64, C.c_uint32, vp, C.c_float, C.c_int, vp]
    L.sf_axis_align_stage_transform.argtypes = [vp, u64, vp, C.c_int, vp, vp]
    L.sf_axis_align_tune.argtypes = [C.c_char_p, C.c_int]
    return L


def stage_up(sd, gravity_min_records=10):
    up, src, none = np.zeros(3, np.float32), C.c_int32(-1), C.c_uint64(0)
    _abi.check(_L().sf_axis_align_stage_up(sd._h, gravity_min_records, _p(up), C.byref(src), C.byref(none)))
    return up, src.value, none.value


def stage_normals(xyz, tris, device=-1):
    out = np.zeros((len(xyz), 3), np.float32)
    _abi.check(_L().sf_axis_align_stage_normals(_p(xyz), len(xyz), _p(tris), len(tris), device, _p(out)))
    return out


def stage_planes(xyz, normals, p, device=-1):
    nv = len(xyz)
    index = np.zeros(nv, np.uint32)
    cap = max(nv, 1)
    ids, table, counts, behind = np.zeros(cap, np.uint32), np.zeros((cap, 10), np.float32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    founded, ns, ctr = C.c_uint64(0), C.c_uint64(0), np.zeros(3, np.uint64)
    _abi.check(_L().sf_axis_align_stage_planes(_p(xyz), _p(normals), nv, C.byref(p), device, _p(index), C.byref(founded), _p(ids), _p(table), _p(counts), _p(behind), cap,
                                               C.byref(ns), _p(ctr)))
    n = ns.value
    return {"index": index, "founded": founded.value, "ids": ids[:n], "table": table[:n], "counts": counts[:n], "behind": behind[:n],
            "batches": int(ctr[0]), "dirty": int(ctr[1]), "fallbacks": int(ctr[2])}


def same_planes(a, b):
    """bitwise: floats are compared as their 32-bit patterns"""
    return (a["founded"] == b["founded"] and np.array_equal(a["index"], b["index"]) and np.array_equal(a["ids"], b["ids"]) and
            np.array_equal(a["table"].view(np.uint32), b["table"].view(np.uint32)) and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["behind"], b["behind"]))


def stage_behind(xyz, reps4, dist, device=-1):
    reps4 = np.ascontiguousarray(reps4, np.float32).reshape(-1, 4)
    out = np.zeros(max(len(reps4), 1), np.uint32)
    _abi.check(_L().sf_axis_align_stage_behind(_p(xyz), len(xyz), _p(reps4), len(reps4), dist, device, _p(out)))
    return out[:len(reps4)]


def stage_cov(xyz, index, cluster, rep4, inlier, device=-1):
    rep4 = np.ascontiguousarray(rep4, np.float32)
    out = np.zeros(10, np.float64)
    _abi.check(_L().sf_axis_align_stage_cov(_p(xyz), _p(index), len(xyz), cluster, _p(rep4), inlier, device, _p(out)))
    return out


def stage_transform(xyz, m, device=-1):
    m = np.ascontiguousarray(m, np.float32).reshape(16)
    out, bbox = np.zeros((len(xyz), 3), np.float32), np.zeros(6, np.float32)
    _abi.check(_L().sf_axis_align_stage_transform(_p(xyz), len(xyz), _p(m), device, _p(out), _p(bbox)))
    return out, bbox


def tune_batch(value):
    _abi.check(_L().sf_axis_align_tune(b"batch", value))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------------------
def grid(origin, du, dv, nu, nv):
    """(nu + 1) x (nv + 1) vertices origin + i du + j dv; two triangles per cell, wound so that the normal is du x dv"""
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
    xyz = np.asarray(origin, np.float64) + i[..., None] * np.asarray(du, np.float64) + j[..., None] * np.asarray(dv, np.float64)
    idx = (i * (nv + 1) + j)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    tris = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return xyz.reshape(-1, 3), tris


def join(parts):
    xyz, tris, off = [], [], 0
    for x, t in parts:
        xyz.append(x)
        tris.append(t + off)
        off += len(x)
    return np.concatenate(xyz), np.concatenate(tris).astype(np.uint32)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


ROOM_R = rotation((0.3, 1.0, 0.2), 0.7)      # the known rotation about a tilted axis ...
ROOM_T = np.array([1.5, -2.0, 0.7])          # ... and shift that take the canonical room (z up, floor at z = 0) to where the "scan" lies
ROOM_SIZE = (6.0, 4.0, 3.0)
S = 0.125


def _walls():
    X, Y, Z = (int(round(v / S)) for v in ROOM_SIZE)
    sx, sy, sz = (S, 0, 0), (0, S, 0), (0, 0, S)
    return [grid((0, 0, 0), sz, sx, Z, X),                 # y = 0, normal +y: every face looks into the room, as a scanner sees it
            grid((0, ROOM_SIZE[1], 0), sx, sz, X, Z),      # y = 4, normal -y
            grid((0, 0, 0), sy, sz, Y, Z),                 # x = 0, normal +x
            grid((ROOM_SIZE[0], 0, 0), sz, sy, Z, Y)]      # x = 6, normal -x


def _place(xyz):
    return np.ascontiguousarray((xyz @ ROOM_R.T + ROOM_T).astype(np.float32))


def room():
    """A box room -- floor, four walls, a table -- of about 6 k vertices on a 12.5 cm grid, rotated and shifted.  Returns (xyz, tris, floor mask,
    wall masks [(mask, canonical normal)]): the masks select the INTERIOR vertices of each face of the box (border vertices are merged with the
    neighbouring face's by the cleaning, and the table leaves with the pieces below min_piece_faces)."""
    X, Y, Z = (int(round(v / S)) for v in ROOM_SIZE)
    parts = [grid((0, 0, 0), (S, 0, 0), (0, S, 0), X, Y)] + _walls() + [grid((2.0, 1.5, 0.75), (S, 0, 0), (0, S, 0), 8, 8)]
    xyz, tris = join(parts)
    eps = 1e-9
    inside = [(xyz[:, k] > eps) & (xyz[:, k] < ROOM_SIZE[k] - eps) for k in range(3)]
    floor = (np.abs(xyz[:, 2]) < eps) & inside[0] & inside[1]
    walls = [((np.abs(xyz[:, 1]) < eps) & inside[0] & inside[2], (0, 1, 0)), ((np.abs(xyz[:, 1] - ROOM_SIZE[1]) < eps) & inside[0] & inside[2], (0, -1, 0)),
             ((np.abs(xyz[:, 0]) < eps) & inside[1] & inside[2], (1, 0, 0)), ((np.abs(xyz[:, 0] - ROOM_SIZE[0]) < eps) & inside[1] & inside[2], (-1, 0, 0))]
    return _place(xyz), tris, floor, walls


def ceiling_room():
    """Four walls under a ceiling that looks down, and no floor: no cluster's normal has z > 0.8 after the up rotation."""
    X, Y, _ = (int(round(v / S)) for v in ROOM_SIZE)
    xyz, tris = join(_walls() + [grid((0, 0, ROOM_SIZE[2]), (0, S, 0), (S, 0, 0), Y, X)])   # y x x = -z
    return _place(xyz), tris


ROOM_PARAMS = dict(min_piece_faces=1000, min_cluster_points=300)   # thresholds scaled to the room: its faces have 825 to 1617 vertices


def room_trajectory(n=12):
    """Camera-to-world poses of a camera that walks the room looking around, its up (camera -y) the room's up apart from a wobble of a few degrees --
    so that the up vector of step 2 is close to the floor normal and step 5 has something left to do."""
    poses = []
    for i in range(n):
        yaw, pitch = 2 * np.pi * i / n, 0.05 * np.sin(1.3 * i) + 0.03
        base = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, -1.0, 0]])   # columns: camera x -> world x, camera y -> world -z (down), camera z -> world y
        Rc = rotation((0, 0, 1), yaw) @ rotation((1, 0, 0), pitch) @ base
        m = np.eye(4)
        m[:3, :3] = ROOM_R @ Rc
        m[:3, 3] = ROOM_R @ np.array([3 + np.cos(yaw), 2 + np.sin(yaw), 1.5]) + ROOM_T
        poses.append(m.astype(np.float32))
    return poses


def clutter(n_tri=3000, seed=5):
    """9 k vertices spread over 3 m with random normals (5 k of them found fewer than 1100 clusters): n_tri little triangles (2 cm), each a piece of its own -- every vertex normal is its
    triangle's, so almost every triangle founds a cluster and the table spans more than one chunk of the match kernel."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 3, (n_tri, 1, 3))
    xyz = (c + rng.uniform(-0.01, 0.01, (n_tri, 3, 3))).reshape(-1, 3)
    tris = np.arange(3 * n_tri, dtype=np.uint32).reshape(-1, 3)
    return np.ascontiguousarray(xyz.astype(np.float32)), tris


CLUTTER_PARAMS = dict(merge_distance=1e-6, min_piece_faces=0, min_cluster_points=3, behind_max=700, floor_normal_z=0.8)


def make_sens(poses, timestamps=None, imu=()):
    """A tiny .sens in memory: 4 x 4 depth frames with the given camera-to-world poses; imu: IMU_DTYPE records"""
    k = np.eye(4, dtype=np.float32)
    sd = sens.SensorData.create(4, 4, 4, 4, k, k)
    for i, m in enumerate(poses):
        t = 1000 * (i + 1) if timestamps is None else timestamps[i]
        sd.add_frame(np.full((4, 4), 1000, np.uint16), camera_to_world=m, timestamp_color=t, timestamp_depth=t)
    for r in imu:
        sd.add_imu_frame(r)
    return sd


def imu_record(gravity, timestamp):
    r = np.zeros((), sens.SensorData.IMU_DTYPE)
    r["gravity"] = gravity
    r["timeStamp"] = timestamp
    return r


def write_scan_folder(path, base, xyz, tris, poses, aligned=None, valid=True, processed=True):
    """<path>/<base>/: <base>.sens, <base>.ply, a second .ply (the same surface lifted by 1 cm), processed.txt"""
    d = os.path.join(str(path), base)
    os.makedirs(d)
    sd = make_sens(poses)
    sd.save(os.path.join(d, base + ".sens"))
    sd.close()
    rgba = np.full((len(xyz), 4), 200, np.uint8)
    for name, x in ((base + ".ply", xyz), (base + "_vh_clean.ply", xyz + np.float32(0.01))):
        m = Mesh.from_arrays(x, tris, rgba)
        m.write_ply(os.path.join(d, name))
        m.close()
    if processed:
        with open(os.path.join(d, "processed.txt"), "w") as f:
            f.write("valid = %s\nheapFreeCount = 12345\nnumValidOptTransforms = 7\nnumTransforms = 9\n" % ("true" if valid else "false"))
            if aligned is not None:
                f.write("aligned = %s\n" % ("true" if aligned else "false"))
    return d


def folder_bytes(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}
