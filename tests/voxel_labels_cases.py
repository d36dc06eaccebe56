"""What tests/test_voxel_labels.py (no GPU) and tests/test_voxel_labels_gpu.py share: the brute-force checker tests/voxel_labels_checker.c built and
bound, the case list of DESIGN.md section 4m, and the sampler restated as plain numpy indexing.  The checker's answer to a case is computed once."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "voxel_labels_checker.c")
BAND = float(np.float32(0.8660254))

_checker = []
_answers = {}


def build_checker():
    """gcc -O2 -ffp-contract=off (the rule has no fused operation); None when there is no gcc."""
    if _checker:
        return _checker[0]
    if shutil.which("gcc") is None:
        _checker.append(None)
        return None
    d = tempfile.mkdtemp(prefix="vl_checker_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libvoxel_labels_checker.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, CHECKER, "-lm"], check=True)
    L = C.CDLL(so)
    vp = C.c_void_p
    L.vc_nearest.argtypes = [vp, vp, C.c_float, vp, vp, C.c_int64, C.c_float, vp, vp]
    L.vc_nearest.restype = None
    L.vc_labels.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.vc_labels.restype = None
    _checker.append(L)
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def checker_nearest(L, dims, lo, voxel, xyz, tris, band):
    """-> face int32 [nz, ny, nx], dist2 float32 [nz, ny, nx]"""
    d, l = np.asarray(dims, np.int32), np.asarray(lo, np.int32)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    shape = (int(d[2]), int(d[1]), int(d[0]))
    face, dist2 = np.empty(shape, np.int32), np.empty(shape, np.float32)
    L.vc_nearest(_p(d), _p(l), float(voxel), _p(xyz), _p(tris), len(tris), float(band), _p(face), _p(dist2))
    return face, dist2


def checker_labels(L, face, tris, vlabel, vinst):
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    vlabel, vinst = np.ascontiguousarray(vlabel, np.uint16), np.ascontiguousarray(vinst, np.uint8)
    face = np.ascontiguousarray(face, np.int32)
    label, inst, bl = np.empty(face.shape, np.uint16), np.empty(face.shape, np.uint8), np.empty(face.shape, np.uint8)
    L.vc_labels(_p(face), face.size, _p(tris), _p(vlabel), _p(vinst), _p(label), _p(inst), _p(bl))
    return label, inst, bl


class Case:
    def __init__(self, name, dims, lo, voxel, xyz, tris, band=BAND, seed=0):
        self.name, self.dims, self.lo, self.voxel, self.band = name, tuple(dims), tuple(lo), float(np.float32(voxel)), float(np.float32(band))
        self.xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
        rng = np.random.default_rng(1000 + seed)
        self.vlabel = rng.choice(np.array([0, 3, 40, 254, 255, 300], np.uint16), len(self.xyz))
        self.vinst = rng.integers(0, 5, len(self.xyz)).astype(np.uint8)

    def header(self):
        from scannet_amd import voxel_labels
        return voxel_labels.header(self.dims, self.voxel, self.lo)

    def answer(self, L):
        """The checker's (face, dist2, label, instance, byte_label), computed once per case."""
        if self.name not in _answers:
            face, d2 = checker_nearest(L, self.dims, self.lo, self.voxel, self.xyz, self.tris, self.band)
            _answers[self.name] = (face, d2) + checker_labels(L, face, self.tris, self.vlabel, self.vinst)
        return _answers[self.name]


# the analytic plane: 1/16 m voxels, a 2 m square at the dyadic height 2.5 voxels cut along x + y = 1, both right angles at the first vertex
PLANE_H = 2.5 / 16.0


def plane_case():
    h = PLANE_H
    xyz = [(-0.5, -0.5, h), (1.5, -0.5, h), (-0.5, 1.5, h), (1.5, 1.5, h)]
    tris = [(0, 1, 2), (3, 2, 1)]
    return Case("plane", (20, 18, 12), (-2, -3, -4), 1.0 / 16.0, xyz, tris, band=2.0)


def coincident_case(order):
    """Two triangles on the same three points (six vertices), labels 5 and 9; order 1 swaps them."""
    tri = [(0.11, 0.07, 0.12), (0.43, 0.09, 0.2), (0.2, 0.38, 0.16)]
    c = Case("coincident%d" % order, (12, 11, 9), (0, 0, 0), 0.05, tri + tri, [(0, 1, 2), (3, 4, 5)])
    c.vlabel = np.array(([5] * 3 + [9] * 3) if order == 0 else ([9] * 3 + [5] * 3), np.uint16)
    c.vinst = np.array(([1] * 3 + [2] * 3) if order == 0 else ([2] * 3 + [1] * 3), np.uint8)
    return c


def unaligned_case():
    """19 x 13 x 10 nodes from (-7, -3, -2): partial tiles, negative indices; one triangle inside the tile of the nodes 0..7, one across several tiles and
    out of the grid on three sides."""
    xyz = [(-0.31, -0.12, -0.07), (-0.22, -0.1, -0.04), (-0.27, -0.03, 0.02),
           (-0.9, -0.4, -0.3), (0.95, 0.1, 0.2), (0.1, 0.9, 0.45)]
    return Case("unaligned", (19, 13, 10), (-7, -3, -2), 0.05, xyz, [(0, 1, 2), (3, 4, 5)])


def many_case():
    """1 000 small faces through the tile (1, 0, 0) of a 48 x 16 x 8 grid -- eight LDS chunks -- and a few through the tiles (4, 1, 0) and (5, 1, 0): the
    tiles between them hold nothing."""
    rng = np.random.default_rng(7)
    v = 0.05
    c = rng.uniform([10.5 * v, 2.5 * v, 2.5 * v], [12.5 * v, 4.5 * v, 4.5 * v], (1000, 1, 3))
    a = c + rng.uniform(-0.6 * v, 0.6 * v, (1000, 3, 3))
    c2 = rng.uniform([35.5 * v, 10 * v, 2 * v], [44 * v, 13 * v, 5 * v], (12, 1, 3))
    b = c2 + rng.uniform(-0.5 * v, 0.5 * v, (12, 3, 3))
    xyz = np.concatenate([a.reshape(-1, 3), b.reshape(-1, 3)])
    return Case("many", (48, 16, 8), (0, 0, 0), v, xyz, np.arange(len(xyz)).reshape(-1, 3))


def soup(n, dims, lo, voxel, seed):
    rng = np.random.default_rng(seed)
    lo_m = (np.array(lo) - 2) * voxel
    hi_m = (np.array(lo) + np.array(dims) + 2) * voxel
    centre = rng.uniform(lo_m, hi_m, (n, 1, 3))
    size = np.where(rng.random((n, 1, 1)) < 0.1, 12 * voxel, 1.5 * voxel)
    return (centre + rng.uniform(-1, 1, (n, 3, 3)) * size).reshape(-1, 3)


def soup_case():
    """2 000 random triangles, nine in ten small and one large, over 40 x 33 x 21 nodes."""
    xyz = soup(2000, (40, 33, 21), (-11, 4, -6), 0.05, 3)
    return Case("soup", (40, 33, 21), (-11, 4, -6), 0.05, xyz, np.arange(len(xyz)).reshape(-1, 3))


SKIPPED = ("repeated", "collinear", "zero_length", "nan", "inf", "huge")


def skipped_cases():
    """(the base mesh, the base mesh with six faces appended that the rule skips): the indices of the base faces are the same in both."""
    dims, lo, voxel = (21, 18, 12), (-3, -2, -1), 0.0625
    xyz = soup(150, dims, lo, voxel, 11)
    tris = np.arange(len(xyz)).reshape(-1, 3)
    base = Case("skipped_base", dims, lo, voxel, xyz, tris, band=1.5)
    n = len(xyz)
    extra = np.array([
        (0.25, 0.25, 0.25), (0.5, 0.25, 0.25), (0.25, 0.5, 0.25),            # n .. n+2: a good triangle, named with a repeated index
        (0.125, 0.125, 0.125), (0.25, 0.25, 0.25), (0.5, 0.5, 0.5),          # n+3 .. n+5: collinear (dyadic: the products are exact)
        (0.375, 0.25, 0.125), (0.375, 0.25, 0.125), (0.5, 0.375, 0.25),      # n+6 .. n+8: two vertices on one point
        (np.nan, 0.25, 0.25), (0.5, 0.25, 0.25), (0.25, 0.5, 0.25),          # n+9 ..
        (0.25, 0.25, 0.25), (0.5, np.inf, 0.25), (0.25, 0.5, 0.25),          # n+12 ..
        (0.25, 0.25, 0.25), (0.5, 0.25, 0.25), (0.25, 0.5, 1e30)], np.float32)  # n+15 ..
    bad = [(n, n + 1, n), (n + 3, n + 4, n + 5), (n + 6, n + 7, n + 8), (n + 9, n + 10, n + 11), (n + 12, n + 13, n + 14), (n + 15, n + 16, n + 17)]
    both = Case("skipped_all", dims, lo, voxel, np.concatenate([xyz, extra]), np.concatenate([tris, np.array(bad)]), band=1.5)
    both.vlabel[:n], both.vinst[:n] = base.vlabel, base.vinst
    return base, both


def empty_mesh_case():
    return Case("empty_mesh", (9, 8, 7), (0, 0, 0), 0.05, np.zeros((0, 3)), np.zeros((0, 3)))


def empty_grid_case():
    return Case("empty_grid", (0, 0, 0), (0, 0, 0), 0.05, soup(10, (8, 8, 8), (0, 0, 0), 0.05, 2), np.arange(30).reshape(-1, 3))


def all_cases():
    base, both = skipped_cases()
    return [plane_case(), coincident_case(0), coincident_case(1), unaligned_case(), many_case(), base, both, soup_case(), empty_mesh_case(), empty_grid_case()]


CASE_NAMES = ["plane", "coincident0", "coincident1", "unaligned", "many", "skipped_base", "skipped_all", "soup", "empty_mesh", "empty_grid"]


def case(name):
    return next(c for c in all_cases() if c.name == name)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the sampler as plain numpy indexing
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sampler_grid(nz, seed, ny=23, nx=37, lo=(-5, 2, -3)):
    """A freespace.Grid of noise with -inf holes and a byte-label grid with a sparse band of task labels, some columns holding only 0 / 255."""
    from scannet_amd import freespace
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 3, (nz, ny, nx)).astype(np.uint8)
    value = np.where(w > 0, rng.normal(0, 2, w.shape), -np.inf).astype(np.float32)
    bl = np.zeros((nz, ny, nx), np.uint8)
    pick = rng.random((nz, ny, nx))
    bl[pick < 0.01] = rng.integers(1, 255, int((pick < 0.01).sum()))
    bl[(pick > 0.01) & (pick < 0.03)] = 255
    return freespace.Grid(value, w, 0.05, lo), bl


def numpy_samples(grid, bl, wx, wy, wz, z0, stride):
    """-> (data [n, 1, wz, wy, wx], label [n, wz], xy [n, 2]) of every selected column, by indexing a padded copy."""
    nz, ny, nx = grid.value.shape
    if z0 is None:
        z0 = -int(grid.lo_voxel[2])
    zs = [z for z in range(z0, z0 + wz) if 0 <= z < nz]
    data, label, xy = [], [], []
    for y in range(0, ny, stride):
        for x in range(0, nx, stride):
            col = bl[zs, y, x] if zs else np.zeros(0, np.uint8)
            if not ((col != 0) & (col != 255)).any():
                continue
            d = np.full((wz, wy, wx), -np.inf, np.float32)
            lab = np.zeros(wz, np.uint8)
            for k in range(wz):
                z = z0 + k
                if not 0 <= z < nz:
                    continue
                lab[k] = bl[z, y, x]
                y0, y1 = max(y - wy // 2, 0), min(y + wy // 2 + 1, ny)
                x0, x1 = max(x - wx // 2, 0), min(x + wx // 2 + 1, nx)
                d[k, y0 - (y - wy // 2):y1 - (y - wy // 2), x0 - (x - wx // 2):x1 - (x - wx // 2)] = grid.value[z, y0:y1, x0:x1]
            data.append(d[None])
            label.append(lab)
            xy.append((x, y))
    n = len(xy)
    return (np.array(data, np.float32).reshape(n, 1, wz, wy, wx), np.array(label, np.uint8).reshape(n, wz), np.array(xy, np.int32).reshape(n, 2))


SAMPLER_CONFIGS = [
    # (nz, wx, wy, wz, z0, stride)
    (70, 31, 31, 62, None, 1),
    (20, 31, 31, 62, None, 1),
    (70, 31, 31, 62, -9, 3),
    (20, 31, 31, 62, 25, 1),      # beyond the grid: nothing is selected
    (70, 5, 5, 7, 40, 1),
    (20, 5, 5, 7, 16, 1),         # the window's last layers hang over the top
]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the two-box scene of the read-back test
# ---------------------------------------------------------------------------------------------------------------------------------------------
def box_mesh(lo, hi, n=4):
    """The six faces of a box, each an n x n lattice of vertices cut into triangles; vertices are not shared between faces."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    xyz, tris = [], []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (lo[axis], hi[axis]):
            base = len(xyz)
            for j in range(n):
                for i in range(n):
                    p = np.zeros(3)
                    p[axis] = side
                    p[u] = lo[u] + (hi[u] - lo[u]) * i / (n - 1)
                    p[v] = lo[v] + (hi[v] - lo[v]) * j / (n - 1)
                    xyz.append(p)
            for j in range(n - 1):
                for i in range(n - 1):
                    a = base + j * n + i
                    tris += [(a, a + 1, a + n), (a + n + 1, a + n, a + 1)]
    return np.array(xyz, np.float32), np.array(tris, np.uint32)


def two_box_scene():
    """Two boxes 0.3 m apart on lattice positions of a 5 cm grid, labels 7 and 21 (instances 1 and 2) -> (Case, grid)."""
    from scannet_amd import freespace
    a_xyz, a_tris = box_mesh((0.1, 0.1, 0.05), (0.5, 0.4, 0.35))
    b_xyz, b_tris = box_mesh((0.8, 0.2, 0.05), (1.1, 0.6, 0.5))
    xyz = np.concatenate([a_xyz, b_xyz])
    tris = np.concatenate([a_tris, b_tris + len(a_xyz)])
    c = Case("two_box", (28, 16, 14), (-1, -1, -1), 0.05, xyz, tris)
    c.vlabel = np.concatenate([np.full(len(a_xyz), 7), np.full(len(b_xyz), 21)]).astype(np.uint16)
    c.vinst = np.concatenate([np.full(len(a_xyz), 1), np.full(len(b_xyz), 2)]).astype(np.uint8)
    nz, ny, nx = c.dims[2], c.dims[1], c.dims[0]
    rng = np.random.default_rng(4)
    w = np.ones((nz, ny, nx), np.uint8)
    grid = freespace.Grid(rng.normal(0, 1, (nz, ny, nx)).astype(np.float32), w, c.voxel, c.lo)
    return c, grid


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the tool's files
# ---------------------------------------------------------------------------------------------------------------------------------------------
TOOL = os.path.join(ROOT, "bin", "voxellabels")


def write_scene_files(directory):
    """The two-box scene as the files bin/voxellabels reads: scan.grid, mesh.ply, segs.json, aggregation.json, labels.tsv -> (paths, case, grid)."""
    import json
    from scannet_amd import segmentator
    case, grid = two_box_scene()
    d = str(directory)
    paths = {k: os.path.join(d, v) for k, v in dict(grid="scan.grid", ply="mesh.ply", segs="mesh.segs.json", agg="mesh.aggregation.json",
                                                   tsv="labels.tsv").items()}
    grid.save(paths["grid"])
    m = segmentator.Mesh.from_arrays(case.xyz, case.tris)
    m.write_ply(paths["ply"])
    m.close()
    half = len(case.xyz) // 2
    seg = [10 if i < half else 20 for i in range(len(case.xyz))]
    json.dump({"params": {}, "sceneId": "two_box", "segIndices": seg}, open(paths["segs"], "w"))
    json.dump({"sceneId": "two_box", "appId": "test", "segGroups": [
        {"id": 0, "objectId": 0, "segments": [10], "label": "chair"}, {"id": 1, "objectId": 1, "segments": [20], "label": "table"}]}, open(paths["agg"], "w"))
    open(paths["tsv"], "w").write("id\tcategory\tcount\n0\twall\t1\n1\tchair\t1\n2\ttable\t1\n")
    return paths, case, grid


def tool_args(paths, prefix, *more):
    return [TOOL, paths["grid"], paths["ply"], "--segs=" + paths["segs"], "--aggregation=" + paths["agg"], "--label-map=" + paths["tsv"], "-o", prefix] + list(more)
