"""Shared by tests/test_render.py and tests/test_render_gpu.py: the CPU checker of the mesh render (tests/render_checker.c, brute force over every
triangle), the cases both suites render, the adversarial rays built from the tree's own boxes, and the product calls.  A case's checker image is
computed once per process and shared."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from scannet_amd import render
from scannet_amd.segmentator import Mesh
from tests import alignment_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "render_checker.c")
NONE = 0xFFFFFFFF


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def have_checker():
    return shutil.which("gcc") is not None and _has_fma()


@functools.lru_cache(maxsize=None)
def checker():
    d = tempfile.mkdtemp(prefix="render_checker_")
    so = os.path.join(d, "librender_checker.so")
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, CHECKER, "-lm", "-lpthread"], check=True)
    L = C.CDLL(so)
    vp, i64, u32 = C.c_void_p, C.c_int64, C.c_uint32
    L.rk_render.argtypes = [vp, vp, i64, vp, i64, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.rk_render.restype = None
    L.rk_rays.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp]
    L.rk_rays.restype = None
    L.rk_sample.argtypes = [vp, u32, u32, u32, vp]
    L.rk_sample.restype = None
    return L


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hashed_colours(n, seed=1):
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed * 7919)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(24)
    rgba = np.stack([(h >> np.uint64(8 * k)) & np.uint64(255) for k in range(3)] + [np.full(n, 255, np.uint64)], -1).astype(np.uint8)
    rgba[:, :3] = 40 + (rgba[:, :3].astype(np.int32) * 200 // 255)   # reflectances of 0.16 .. 0.94: bounces keep some light
    return np.ascontiguousarray(rgba)


# ---- the cases: name -> dict(xyz, rgba, tris, params (keyword overrides), views = [(theta, world_up)], box = the camera's box or None (the mesh's)) ----
def _floor():
    xyz = np.array([[0, 0, 0], [2, 0, 0], [2, 1.5, 0], [0, 1.5, 0]], np.float32)
    rgba = np.array([[250, 40, 30, 255], [60, 220, 50, 255], [40, 70, 240, 255], [230, 210, 90, 255]], np.uint8)
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return dict(xyz=xyz, rgba=rgba, tris=tris, params=dict(width=33, height=25, samples=3), views=[(0.0, None)], box=None)


def _lattice():
    n = 6   # even: the AABB's centre (3, 3, 0) is a lattice vertex, and the camera sits exactly above it
    xyz, tris = ac.grid((0, 0, 0), (1, 0, 0), (0, 1, 0), n, n)
    xyz, tris = xyz.astype(np.float32), tris.astype(np.uint32)
    around = [i for i, t in enumerate(tris) if any(np.array_equal(xyz[v], [3, 3, 0]) for v in t)]
    extra = np.concatenate([tris[around[::-1]], tris[[5, 17, 40]], np.array([[0, 0, 1], [0, 1, 2]], np.uint32)])   # given twice; and two of zero area
    tris = np.ascontiguousarray(np.concatenate([tris[:30], extra[:4], tris[30:], extra[4:]]))
    assert np.array_equal(xyz[[0, 1, 2], 0], [0, 0, 0])   # vertices 0, 1, 2 are collinear
    return dict(xyz=xyz, rgba=hashed_colours(len(xyz), 3), tris=tris, params=dict(width=33, height=25, samples=2, max_depth=2, pixel_centre=1),
                views=[(0.0, None)], box=None)


@functools.lru_cache(maxsize=None)
def _room_mesh():
    xyz, tris, _, _ = ac.room()
    cx, ct = ac.clutter(n_tri=300, seed=5)
    cx = (cx.astype(np.float64) @ ac.ROOM_R.T + ac.ROOM_T).astype(np.float32)   # the clutter into the room's corner
    xyz, tris = ac.join([(xyz, tris), (cx, ct)])
    return np.ascontiguousarray(xyz, np.float32), hashed_colours(len(xyz)), np.ascontiguousarray(tris, np.uint32)


def _room(integrator="path"):
    # alignment_cases.room() has 10.9 k triangles of its own, so pixels x samples x rays x triangles is nominally 3e8 here; most paths leave after a
    # bounce or two and the checker deals its rows to threads: it takes about 0.6 s per integrator
    xyz, rgba, tris = _room_mesh()
    return dict(xyz=xyz, rgba=rgba, tris=tris, params=dict(width=48, height=36, samples=4, max_depth=4, integrator=integrator),
                views=[(0.0, None), (120.0, None)], box=None)


def _inside():
    lo, hi = np.array([-1.0, -2.0, -0.5]), np.array([3.0, 1.0, 2.5])
    c = np.array([[lo[0] if not (i & 1) else hi[0], lo[1] if not (i & 2) else hi[1], lo[2] if not (i & 4) else hi[2]] for i in range(8)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # wound to look INTO the box
    tris = np.array([t for a, b, cc, d in quads for t in ((a, cc, b), (a, d, cc))], np.uint32)
    # a box a quarter of the size around the same centre puts the camera (2.5 radii of THAT box out) inside the closed one
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.1
    return dict(xyz=c, rgba=hashed_colours(8, 2), tris=tris, params=dict(width=17, height=13, samples=2, max_depth=3), views=[(0.0, None), (75.0, (0.2, 0.1, 1.0))],
                box=np.concatenate([mid - half, mid + half]).astype(np.float32))


CASES = {"floor": _floor, "lattice": _lattice, "room": _room, "ao": lambda: _room("ao"), "inside": _inside}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["name"] = name
    c["p"] = render.default_params(**c["params"])
    c["mesh"] = Mesh.from_arrays(c["xyz"], c["tris"], c["rgba"])
    c["cameras"] = [render.camera(c["mesh"] if c["box"] is None else c["box"], c["p"], world_up=up, theta=th) for th, up in c["views"]]
    return c


def camera_floats(cam):
    return np.array(list(cam.origin) + list(cam.right) + list(cam.up) + list(cam.forward) + [cam.tan_half_fov, cam.aspect], np.float32)


@functools.lru_cache(maxsize=None)
def checker_images(name):
    """[views, H, W, 4] float32 by the brute-force checker; read-only."""
    c, L = case(name), checker()
    p = c["p"]
    out = np.zeros((len(c["cameras"]), p.height, p.width, 4), np.float32)
    for i, cam in enumerate(c["cameras"]):
        cf = camera_floats(cam)
        L.rk_render(_p(c["xyz"]), _p(c["rgba"]), len(c["xyz"]), _p(c["tris"]), len(c["tris"]), _p(cf), p.width, p.height, p.samples, p.max_depth,
                    int(p.integrator == render.AO), p.pixel_centre, _p(out[i]))
    out.setflags(write=False)
    return out


def checker_rays(c, rays):
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    tri, tuv = np.zeros(len(rays), np.uint32), np.zeros((len(rays), 3), np.float32)
    checker().rk_rays(_p(c["xyz"]), len(c["xyz"]), _p(c["tris"]), len(c["tris"]), len(rays), _p(rays), _p(tri), _p(tuv))
    return tri, tuv


def product_images(name, device, batch=True):
    c = case(name)
    with render.Renderer(c["p"], device) as r:
        r.set_mesh(c["mesh"])
        return r.run(c["cameras"]) if batch else np.concatenate([r.run(cam) for cam in c["cameras"]])


# ---- rays that try to slip between the tree's boxes --------------------------------------------------------------------------------------------------
def _mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def hashed_unit(n, salt):
    with np.errstate(over="ignore"):
        return (_mix(np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(salt)) >> np.uint32(8)).astype(np.float64) / 2.0 ** 24


def box_rays(boxes, max_boxes=40):
    """From the node boxes: rays through corners (from outside along the diagonal and along each axis), along edges, in faces, from inside and from ON
    the boxes, with every combination of zero direction components."""
    pick = np.unique(np.linspace(0, len(boxes) - 1, min(max_boxes, len(boxes))).astype(int))
    rays = []
    dirs = [np.array(d, np.float64) for d in np.ndindex(3, 3, 3) if d != (1, 1, 1)]
    dirs = [d - 1 for d in dirs]   # every direction of {-1, 0, 1}^3 but zero: all combinations of zero components and signs
    for b in boxes[pick].astype(np.float64):
        lo, hi = b[:3], b[3:]
        mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 1e-3)
        corners = [np.where([(i >> k) & 1 for k in range(3)], hi, lo) for i in range(8)]
        for d in dirs:
            rays.append(np.concatenate([mid, d]))                    # from inside
            rays.append(np.concatenate([lo, d]))                     # from a corner, ON the box
            rays.append(np.concatenate([mid - 3 * ext * d, d]))      # from outside through the middle; axis-parallel ones run in nothing special ...
            rays.append(np.concatenate([lo - 2 * ext * d, d]))       # ... these run through a corner, along an edge (one non-zero) or in a face (two)
            rays.append(np.concatenate([hi - 2 * ext * d, d * ext])) # through the other corner, unnormalised and anisotropic
        for cnr in corners:
            rays.append(np.concatenate([mid + 4 * (cnr - mid), mid - cnr]))   # through the corner along the diagonal
    return np.ascontiguousarray(np.array(rays, np.float32))


def hashed_rays(c, n=100000):
    lo, hi = c["xyz"].min(0).astype(np.float64), c["xyz"].max(0).astype(np.float64)
    ext = hi - lo
    o = lo - 0.3 * ext + 1.6 * ext * np.stack([hashed_unit(n, 11 + k) for k in range(3)], -1)
    to = lo + ext * np.stack([hashed_unit(n, 31 + k) for k in range(3)], -1)
    return np.ascontiguousarray(np.concatenate([o, to - o], 1).astype(np.float32))


def same_hits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
