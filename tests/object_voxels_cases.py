"""What tests/test_object_voxels.py (no GPU) and tests/test_object_voxels_gpu.py share: the brute-force checker tests/object_voxels_checker.c built and
bound, and the case list of DESIGN.md section 4n.  The checker's and the exact statement's answers to a case are computed once.

Every object is scaled so that its largest extent covers `fit` cells in the middle of `dim`: with dim 30 and fit 24 an object whose box is
[0, 24]^3 has cells of edge 1 and its origin at -3, so a coordinate v lies at 256 (v + 3) exactly and integer coordinates are cell boundaries."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import object_voxels_exact as exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "object_voxels_checker.c")
CLASSES = os.path.join(ROOT, "tests", "golden", "classes_ObjClassification-ShapeNetCore55.txt")
TOOL = os.path.join(ROOT, "bin", "objectvoxels")
NAMES = ("data", "label", "object_id", "origin", "cell")

_checker = []
_answers = {}
_exact = {}


def build_checker():
    """gcc -O2 -ffp-contract=off (the rule has no fused operation); None when there is no gcc."""
    if _checker:
        return _checker[0]
    if shutil.which("gcc") is None:
        _checker.append(None)
        return None
    d = tempfile.mkdtemp(prefix="ov_checker_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libobject_voxels_checker.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, CHECKER, "-lm"], check=True)
    L = C.CDLL(so)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    L.ovc_voxelize.argtypes = [vp, vp, i64, vp, vp, i32, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_float, vp, i64, vp, vp, vp, vp, vp]
    L.ovc_voxelize.restype = i64
    _checker.append(L)
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same(got, want):
    """-> the names of the arrays that differ (data, label, object_id, and the bits of origin and cell)"""
    return [n for g, w, n in zip(got, want, NAMES) if not same_bits(g, w)]


class Case:
    def __init__(self, name, xyz, tris, vobj, cls, grid=None, **params):
        self.name = name
        self.xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
        self.vobj = np.ascontiguousarray(vobj, np.uint32).reshape(-1)
        self.cls = np.ascontiguousarray(cls, np.int32).reshape(-1)
        self.grid = grid
        self.params = dict(dim=30, fit=24, min_faces=1, all_objects=0)
        self.params.update(params)
        assert len(self.vobj) == len(self.xyz)

    def answer(self, L):
        """The checker's (data, label, object_id, origin, cell), computed once per case."""
        if self.name not in _answers:
            p, cap = self.params, len(self.cls)
            d = p["dim"]
            data, label, oid = np.zeros((cap, 2, d, d, d), np.uint8), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
            origin, cell = np.zeros((cap, 3), np.float32), np.zeros(cap, np.float32)
            gd = gl = w = None
            voxel = 0.0
            if self.grid is not None:
                w = np.ascontiguousarray(self.grid.weight, np.uint8)
                gd, gl = np.array(w.shape[::-1], np.int32), np.array(self.grid.lo_voxel, np.int32)
                voxel = float(self.grid.voxel_size)
            n = L.ovc_voxelize(_p(self.xyz), _p(self.tris), len(self.tris), _p(self.vobj), _p(self.cls), len(self.cls), d, p["fit"], p["min_faces"],
                               p["all_objects"], _p(gd), _p(gl), voxel, _p(w), cap, _p(data), _p(label), _p(oid), _p(origin), _p(cell))
            _answers[self.name] = (data[:n], label[:n], oid[:n], origin[:n], cell[:n])
        return _answers[self.name]

    def exact(self):
        """The exact statement's answer (tests/object_voxels_exact.py), computed once per case."""
        if self.name not in _exact:
            p = self.params
            g = None if self.grid is None else (np.asarray(self.grid.weight), float(self.grid.voxel_size), tuple(self.grid.lo_voxel))
            _exact[self.name] = exact.voxelize(self.xyz, self.tris, self.vobj, self.cls, p["dim"], p["fit"], p["min_faces"], bool(p["all_objects"]), g)
        return _exact[self.name]

    def library(self, device=None, **kw):
        from scannet_amd import object_voxels as ov
        s = ov.voxelize(self.xyz, self.tris, self.vobj, self.cls, self.grid, ov.default_params(**self.params), device, **kw)
        return (s.data, s.label, s.object_id, s.origin, s.cell), s.total


# ---------------------------------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def faces(points):
    """points [n, 3, 3]: triangles that share no vertex -> (xyz, tris)"""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    return pts.astype(np.float32), np.arange(len(pts), dtype=np.uint32).reshape(-1, 3)


# two small faces that pin an object's box to [0, 24]^3: cells of edge 1, origin -3
ANCHORS = [[(0, 0, 0), (1, 0, 0), (0, 1, 0.5)], [(24, 24, 24), (23, 24, 24), (24, 23, 23.5)]]


def box12(lo, hi):
    """The 12 faces of a box over its 8 corners."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    xyz = np.array([[(lo, hi)[(n >> a) & 1][a] for a in range(3)] for n in range(8)], np.float32)
    tris = []
    for a in range(3):
        u, v = [1 << b for b in range(3) if b != a]
        for side in (0, 1 << a):
            tris += [(side, side + u, side + v), (side + u + v, side + v, side + u)]
    return xyz, np.array(tris, np.uint32)


def soup(seed, n, size, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(lo + size, hi - size, (n, 1, 3))
    return faces(centre + rng.uniform(-size, size, (n, 3, 3)))


def one_object(name, points, **kw):
    xyz, tris = faces(points)
    return Case(name, xyz, tris, np.ones(len(xyz)), [18], **kw)


def boundary_case():
    """An axis-aligned triangle in the plane z = 5, a cell boundary: it meets the layers on both sides."""
    return one_object("boundary", ANCHORS + [[(2, 2, 5), (9, 2, 5), (2, 9, 5)]])


def corner_case():
    """A triangle with a vertex on the lattice point (10, 10, 10) that leads away into x, y, z > 10: it meets the eight cells around the point, seven of
    them at that one corner only."""
    return one_object("corner", ANCHORS + [[(10, 10, 10), (14, 11, 12), (11, 14, 12.5)]])


def oblique_case():
    """One large oblique face, an object of its own: its box covers the whole 24^3 cells, it meets few of them."""
    return one_object("oblique", [[(0, 0, 0), (24, 24, 12), (0, 24, 24)]])


def cube_case():
    """A cube [0, 3]^3 of 12 faces: its sides lie on the cell boundaries 3 and 27, so the cells 2, 3 and 26, 27 along an axis are met."""
    xyz, tris = box12((0, 0, 0), (3, 3, 3))
    return Case("cube", xyz, tris, np.ones(8), [4])


def cube_answer():
    occ = np.zeros((30, 30, 30), np.uint8)
    occ[2:28, 2:28, 2:28] = 1
    occ[4:26, 4:26, 4:26] = 0
    return occ


def big_case():
    """600 small faces in one object (three chunks on the device) beside a second object of 300 (two chunks, the second one short)."""
    a, ta = soup(11, 600, 0.04)
    b, tb = soup(12, 300, 0.1, 2.0, 4.0)
    return Case("big", np.concatenate([a, b]), np.concatenate([ta, tb + len(a)]), np.concatenate([np.ones(len(a)), np.full(len(b), 2)]), [18, 49])


def many_case():
    """70 objects of two thin faces each, ids 0 .. 69 with 7 of them without a class; one object id in between has no face at all."""
    rng = np.random.default_rng(5)
    pts, vobj, cls = [], [], []
    for i in range(71):
        cls.append(-1 if i % 10 == 3 else 1 + i % 50)
        if i == 40:
            continue
        base = rng.uniform(-5, 5, 3)
        length, w = rng.uniform(0.5, 2.0), rng.uniform(0.005, 0.03, 4)
        axis = i % 3
        d = np.zeros(3)
        d[axis] = length
        s, t = np.zeros(3), np.zeros(3)
        s[(axis + 1) % 3], t[(axis + 2) % 3] = w[0], w[1]
        pts += [[base, base + d + s, base + t], [base + d, base + s + t, base + d * 0.5 + t]]
        vobj += [i + 1] * 6
    xyz, tris = faces(pts)
    return Case("many", xyz, tris, vobj, cls)


def shared_case():
    """Two objects over shared vertices: the faces (1, 2, 2) and (2, 1, 2) belong to object 2, (1, 1, 2) and (1, 2, 3) to object 1 (vertex values)."""
    xyz = np.array([(0, 0, 0), (1, 0, 0.2), (0, 1, 0.4), (1, 1, 1), (2, 0.5, 1.5), (0.5, 2, 0.7), (2, 2, 2), (1.5, 0.2, 0.1)], np.float32)
    vobj = np.array([1, 1, 2, 2, 2, 1, 3, 1], np.uint32)
    tris = np.array([(0, 2, 3), (2, 1, 4), (0, 1, 2), (5, 3, 6), (7, 1, 0)], np.uint32)
    return Case("shared", xyz, tris, vobj, [18, 49, 5])


SKIPPED = ("repeated index", "NaN coordinate", "infinite coordinate", "collinear after quantisation", "two vertices in one quantum")


def skipped_cases():
    """-> (base, both): an object, and the same with one face of every skipped kind added to it (inside its box)."""
    xyz, tris = soup(21, 40, 0.15)
    extra = np.array([(0.5, 0.5, 0.5), (0.6, 0.5, 0.5), (0.5, 0.6, 0.5),            # repeated index: (n, n, n + 1)
                      (np.nan, 0.5, 0.5), (0.5, np.inf, 0.5),                       # with n + 1, n + 2
                      (0.25, 0.5, 0.5), (0.5, 0.5, 0.5), (0.75, 0.5, 0.5),          # collinear along x: y and z quantise alike
                      (0.4, 0.4, 0.4), (0.4 + 1e-7, 0.4, 0.4), (0.7, 0.3, 0.6)], np.float32)
    n = len(xyz)
    bad = np.array([(n, n, n + 1), (n + 3, n + 1, n + 2), (n + 1, n + 4, n + 2), (n + 5, n + 6, n + 7), (n + 8, n + 9, n + 10)], np.uint32)
    base = Case("skipped_base", xyz, tris, np.ones(n), [18])
    both = Case("skipped_all", np.concatenate([xyz, extra]), np.concatenate([tris, bad]), np.ones(n + len(extra)), [18])
    return base, both


def degenerate_objects_case(min_faces=1, name="degenerate"):
    """Object 0: one face whose three vertices coincide (zero extent); object 1: one face; object 2: two; object 3: five; object 4: only skipped faces."""
    pts = [[(1, 1, 1)] * 3, [(0, 0, 0), (1, 0.03, 0), (0, 0.06, 0.04)]]
    vobj = [1] * 3 + [2] * 3
    rng = np.random.default_rng(9)
    for o, n in ((3, 2), (4, 5)):
        pts += list(rng.uniform(o, o + 1, (n, 1, 3)) + rng.uniform(-0.08, 0.08, (n, 3, 3)))
        vobj += [o] * (3 * n)
    pts += [[(np.nan, 0, 0), (1, 2, 3), (3, 2, 1)]]
    vobj += [5] * 3
    xyz, tris = faces(pts)
    return Case(name, xyz, tris, vobj, [1, 3, 4, 5, 9], min_faces=min_faces)


def classless_case(all_objects):
    xyz, tris = soup(31, 30, 0.1)
    vobj = np.repeat(np.arange(1, 4), 30)
    return Case("classless_%d" % all_objects, xyz, tris, vobj, [18, -1, 49], all_objects=all_objects)


def dim8_case():
    xyz, tris = soup(41, 50, 0.08)
    return Case("dim8", xyz, tris, np.ones(len(xyz)), [30], dim=8, fit=8)


def empty_case():
    return Case("empty", np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), [18, 49])


def known_case(mode):
    """An object over [0, 2.4]^3 m (cells of 0.1 m from -0.3) and a 5 cm grid.  half: the grid covers x < 1.2 of the cube, a third of its weights are 0;
    the object has faces on both sides.  zero: the grid covers everything and every weight is 0.  none: a grid without a node."""
    from scannet_amd import freespace
    a, ta = soup(51, 60, 0.2, 0.0, 2.4)
    xyz = np.concatenate([a, np.array([(0, 0, 0), (0.1, 0, 0), (0, 0.1, 0.1), (2.4, 2.4, 2.4), (2.3, 2.4, 2.4), (2.4, 2.3, 2.3)], np.float32)])
    tris = np.concatenate([ta, np.array([(len(a), len(a) + 1, len(a) + 2), (len(a) + 3, len(a) + 4, len(a) + 5)], np.uint32)])
    rng = np.random.default_rng(6)
    if mode == "half":
        shape, lo = (70, 70, 34), (-10, -10, -10)                                     # x from -0.5 m to 1.2 m
        w = (rng.integers(0, 3, shape) > 0).astype(np.uint8) * 7
    elif mode == "zero":
        shape, lo = (70, 70, 70), (-10, -10, -10)
        w = np.zeros(shape, np.uint8)
    else:
        shape, lo = (0, 0, 0), (0, 0, 0)
        w = np.zeros(shape, np.uint8)
    grid = freespace.Grid(np.zeros(shape, np.float32), w, 0.05, lo)
    return Case("known_" + mode, xyz, tris, np.ones(len(xyz)), [47], grid=grid)


CASES = dict(boundary=boundary_case, corner=corner_case, oblique=oblique_case, cube=cube_case, big=big_case, many=many_case, shared=shared_case,
             skipped_all=lambda: skipped_cases()[1], degenerate=degenerate_objects_case, min_faces=lambda: degenerate_objects_case(3, "min_faces"),
             classless_0=lambda: classless_case(0), classless_1=lambda: classless_case(1), dim8=dim8_case, empty=empty_case,
             known_half=lambda: known_case("half"), known_zero=lambda: known_case("zero"), known_none=lambda: known_case("none"))
CASE_NAMES = list(CASES)
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the tool's files
# ---------------------------------------------------------------------------------------------------------------------------------------------
def write_scene_files(directory):
    """Three boxes and a free-space grid as the files bin/objectvoxels reads -> (paths, xyz, tris, grid).  Two chairs (objectIds 0 and 2, told apart),
    a table (objectId 1, ShapeNetCore55 value given as a number) and a "thing" without a class (objectId 5)."""
    import json
    from scannet_amd import freespace, segmentator
    boxes = [((0.1, 0.1, 0.0), (0.5, 0.6, 0.9)), ((1.0, 0.2, 0.0), (2.2, 1.0, 0.7)), ((0.2, 1.5, 0.0), (0.7, 1.9, 1.0)), ((1.5, 1.5, 0.3), (1.8, 1.9, 0.5))]
    xyz, tris, seg = [], [], []
    for n, (lo, hi) in enumerate(boxes):
        x, t = box12(lo, hi)
        tris.append(t + 8 * n)
        xyz.append(x)
        seg += [10 * (n + 1)] * 4 + [10 * (n + 1) + 1] * 4
    xyz, tris = np.concatenate(xyz), np.concatenate(tris)
    d = str(directory)
    paths = {k: os.path.join(d, v) for k, v in dict(grid="scan.grid", ply="mesh.ply", segs="mesh.segs.json", agg="mesh.aggregation.json", tsv="labels.tsv").items()}
    paths["classes"] = CLASSES
    rng = np.random.default_rng(3)
    grid = freespace.Grid(np.zeros((20, 44, 30), np.float32), (rng.integers(0, 4, (20, 44, 30)) > 0).astype(np.uint8), 0.05, (-2, -2, -2))
    grid.save(paths["grid"])
    m = segmentator.Mesh.from_arrays(xyz, tris)
    m.write_ply(paths["ply"])
    m.close()
    json.dump({"params": {}, "sceneId": "boxes", "segIndices": seg}, open(paths["segs"], "w"))
    json.dump({"sceneId": "boxes", "appId": "test", "segGroups": [
        {"id": 0, "objectId": 0, "segments": [10, 11], "label": "office chair"}, {"id": 1, "objectId": 1, "segments": [20, 21], "label": "table"},
        {"id": 2, "objectId": 2, "segments": [30, 31], "label": "chair"}, {"id": 3, "objectId": 5, "segments": [40, 41], "label": "thing"}]}, open(paths["agg"], "w"))
    open(paths["tsv"], "w").write("id\traw_category\tcategory\tShapeNetCore55\tother\n1\toffice chair\tchair\tchair\t18\n2\ttable\ttable\t49\ttable\n"
                                  "3\tchair\tchair\tchair\t18\n4\tthing\tobject\t\tthing\n")
    return paths, xyz, tris, grid


def tool_args(paths, prefix, *more, grid=True):
    return [TOOL, paths["ply"]] + ([paths["grid"]] if grid else []) + ["--segs=" + paths["segs"], "--aggregation=" + paths["agg"], "--label-map=" + paths["tsv"],
                                                                         "--classes=" + paths["classes"], "-o", prefix] + list(more)
