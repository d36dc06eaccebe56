"""Named, deterministic cases of the mesh clean's four filters (tests/test_clean_stages_cpu.py, tests/test_clean_stages.py).  Every one is the smallest
shape that still reaches its branch; V <= 4096 wherever tests/clean_exact.py is quadratic.  The builders may use the filter's grid formula (cells of
2 r (1 + 1e-5), eight cells on the point's side, 21 bits per axis) to AIM points at cell boundaries and key bits; the statement never does."""
import collections
import itertools
import math

import numpy as np

from tests import clean_exact as cx

F32 = np.float32
R = F32(0.0010689)                                   # clean.mlx:4
INV = 0.5 / (float(R) * (1.0 + 1e-5))                # cells per metre
SF_ERR_FORMAT, SF_ERR_UNSUPPORTED = -3, -4               # include/scanfuse.h

MergeCase = collections.namedtuple("MergeCase", "name pos r error")
FaceCase = collections.namedtuple("FaceCase", "name nv tri target")
CompCase = collections.namedtuple("CompCase", "name tri min_faces")
CompactCase = collections.namedtuple("CompactCase", "name pos col tri")
for _c in (MergeCase, FaceCase, CompCase, CompactCase):
    _c.__repr__ = lambda self: self.name


def _m(name, pos, r=R, error=None):
    return MergeCase(name, np.ascontiguousarray(pos, F32).reshape(-1, 3), F32(r), error)


def _ulp(x):
    x = F32(abs(x))
    return float(np.nextafter(x, F32(np.inf)) - x)


# ---- cell geometry ---------------------------------------------------------------------------------------------------------------------------------------
def _anchor_coord(k, variant):
    """the float whose scaled coordinate sits at k / k + 0.5 (variant 0 / 3), one ulp below (1 / 4) or above (2 / 5)"""
    x = F32((k + (0.5 if variant >= 3 else 0.0)) / INV)
    step = variant % 3
    return x if step == 0 else np.nextafter(x, F32(-np.inf) if step == 1 else F32(np.inf))


def _neighbours(anchor, d):
    """two points in direction d from the anchor: the float distance just under r, and at or just over it"""
    d = np.asarray(d, np.float64) / math.sqrt(sum(q * q for q in d))
    span = max(2e-5, 6 * _ulp(np.abs(anchor).max()) / float(R))
    ts = float(R) * (1.0 + np.linspace(-span, span, 1201))
    cand = (anchor.astype(np.float64)[None, :] + ts[:, None] * d[None, :]).astype(F32)
    dist = cx.dist_rows(anchor, cand)
    under, over = np.nonzero(dist < R)[0], np.nonzero(dist >= R)[0]
    return cand[under[np.argmax(dist[under])]], cand[over[np.argmin(dist[over])]]


def cell_geometry(origin_cells=(8, 8, 8), sign=1):
    """Per anchor variant x axis choice x 26 directions x {under, over}: a mesh of two, the lower-index neighbour first; the meshes sit four cells apart."""
    pos, g = [], 0
    for variant, axes in itertools.product(range(6), ((0,), (1,), (2,), (0, 1, 2))):
        for d in itertools.product((-1, 0, 1), repeat=3):
            if d == (0, 0, 0):
                continue
            for which in (0, 1):
                cell = [origin_cells[0] + 4 * (g % 11), origin_cells[1] + 4 * ((g // 11) % 11), origin_cells[2] + 4 * (g // 121)]
                anchor = np.array([_anchor_coord(cell[a], variant) if a in axes else F32((cell[a] + 0.3) / INV) for a in range(3)], F32)
                pos += [_neighbours(anchor, d)[which], anchor]
                g += 1
    return np.array(pos, F32) * F32(sign)


# ---- key width ---------------------------------------------------------------------------------------------------------------------------------------------
def _lattice_cluster(at, axis):
    """five points on the float lattice along `axis` from `at`, steps alternating between the largest below r and the next one"""
    p0 = np.array(at, F32)
    u = _ulp(p0[axis]) if p0[axis] != 0 else 2.0 ** -12
    n = int(float(R) / u)
    while True:                                        # the largest step whose float distance is still < r
        q = p0.copy()
        q[axis] = F32(float(p0[axis]) + (n + 1) * u)
        if not cx.dist_rows(p0, q[None])[0] < R:
            break
        n += 1
    out, x = [p0], float(p0[axis])
    for step in (n, n + 1, n, n + 1):
        x += step * u
        q = p0.copy()
        q[axis] = F32(x)
        out.append(q)
    return out


def key_width(axes, far):
    """two clusters `far` metres apart on every axis named: near the origin and at `far`"""
    pos = []
    for where in (0.0, far):
        at = [where if a in axes else 0.25 for a in range(3)]
        for a in axes:
            start = list(at)
            start[(a + 1) % 3] += 0.25 * a                 # the clusters of one place stand apart
            pos += _lattice_cluster(start, a)
    return np.array(pos, F32)


def key_alias():
    """Vertices whose cells agree in x and y and lie exactly 2^18, 2^19 and 2^20 cells apart in z -- cell keys equal in their low 60, 61 and 62 bits --
    with the groups interleaved in the index order, and in each group a second vertex half a radius beside the first."""
    z0, groups = 3, []
    for dz in (0, 1 << 18, 1 << 19, 1 << 20):
        z = F32((z0 + dz + 0.5) / INV)
        assert math.floor(float(z) * INV) == z0 + dz
        a = np.array([F32(5.25 / INV), F32(5.25 / INV), z], F32)
        groups.append((a, a + np.array([0.5 * float(R), 0, 0], F32)))
    return np.array([g[k] for k in (0, 1) for g in groups], F32)


# ---- rounding ----------------------------------------------------------------------------------------------------------------------------------------------
def _verdicts64(p0, p1):
    """vectorised guess of dist < r under the three roundings (binary64 holds every square exactly); each pair used is confirmed by clean_exact.dist_as"""
    e = (p0 - p1).astype(F32).astype(np.float64)
    x2, y2, z2 = e[:, 0] ** 2, e[:, 1] ** 2, e[:, 2] ** 2
    f = lambda a: a.astype(F32).astype(np.float64)
    sums = {cx.KERNEL: f(f(f(x2) + f(y2)) + f(z2)), cx.FUSED: f(z2 + f(y2 + f(x2))), cx.ASSOC: f(f(x2) + f(f(y2) + f(z2)))}
    return {k: np.sqrt(v.astype(F32)) < R for k, v in sums.items()}


def _rounding_search(seed=20261, want=40):
    rng = np.random.default_rng(seed)
    found = {(alt, ky): [] for alt in (cx.FUSED, cx.ASSOC) for ky in (True, False)}
    taken = np.zeros((0, 3), F32)
    tried = 0
    for _ in range(40):
        n = 400000
        p0 = rng.uniform(0.02, 0.2, (n, 3)).astype(F32)
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        p1 = (p0.astype(np.float64) + d * float(R)).astype(F32)
        close = np.abs(np.linalg.norm(p0.astype(np.float64) - p1.astype(np.float64), axis=1) - float(R)) < 3e-10
        p0, p1 = p0[close], p1[close]
        tried += len(p0)
        v = _verdicts64(p0, p1)
        for alt in (cx.FUSED, cx.ASSOC):
            for i in np.nonzero(v[cx.KERNEL] != v[alt])[0]:
                ky = bool(v[cx.KERNEL][i])
                if len(found[(alt, ky)]) >= want:
                    continue
                if len(taken) and (np.linalg.norm(taken.astype(np.float64) - p0[i].astype(np.float64), axis=1) < 5 * float(R)).any():
                    continue                           # every pair is a mesh of its own
                if bool(cx.dist_as(p0[i], p1[i], cx.KERNEL) < R) != ky or bool(cx.dist_as(p0[i], p1[i], alt) < R) == ky:
                    continue
                found[(alt, ky)].append((p0[i], p1[i]))
                taken = np.concatenate([taken, p0[i][None]])
        if all(len(x) >= want for x in found.values()):
            break
    return found, tried


ROUNDING_PAIRS, ROUNDING_TRIED = _rounding_search()


def rounding_batch():
    return np.array([p for key in sorted(ROUNDING_PAIRS, key=str) for pair in ROUNDING_PAIRS[key] for p in pair], F32)


# ---- greedy, tails, r == 0 -----------------------------------------------------------------------------------------------------------------------------------
def _chain(n, spacing=0.0008):
    return np.array([[spacing * i, 0, 0] for i in range(n)], F32)


def _cloud(n, seed, box=0.01):
    return np.random.default_rng(seed).uniform(0, box, (n, 3)).astype(F32)


def _spaced_with_merges(n, merged):
    pos = np.array([[0.01 * i, 0, 0] for i in range(n)], F32)
    for m in merged:
        pos[m] = pos[m - 1] + np.array([0.0005, 0, 0], F32)
    return pos


def _runs_r0():
    rng = np.random.default_rng(7)
    rows = [[0.5, 0.25, 0.125]] * 70 + [[0.5, 0.25, 0.75]] * 2 + [[i + 1.0, 0, 0] for i in range(30)]
    return np.array(rows, F32)[rng.permutation(len(rows))]


TAILS = (1, 63, 64, 65, 255, 256, 257)


def _merge_cases():
    out = [_m("cells", cell_geometry()), _m("cells-mirrored", cell_geometry(sign=-1)),
           _m("cells-at-8m", cell_geometry(origin_cells=(3742, 8, 8))), _m("cells-at-minus-8m", cell_geometry(origin_cells=(3742, 8, 8), sign=-1))]
    for name, axes in (("x", (0,)), ("y", (1,)), ("z", (2,)), ("xyz", (0, 1, 2))):
        out.append(_m("keys-2300m-" + name, key_width(axes, 2300.0)))
        out.append(_m("keys-minus-2300m-" + name, key_width(axes, -2300.0)))
    out.append(_m("keys-alias-bits-60-62", key_alias()))
    out.append(_m("wide-4600m", [[-2300, 0, 0], [2300, 0, 0], [2300.0005, 0, 0]], error=SF_ERR_UNSUPPORTED))
    box = lambda side: np.array([[0, 0, 0], [side, side, side], [side, side, side - 5e-7], [0.5 * side, 0, 0]], F32)
    # 2^21 cells of 2e-6 m are 4.19 m: a 1 m and a 3 m box are inside the limit (the issue that asked for these cases had the 3 m box beyond it), a 5 m box is not
    out += [_m("r1e-6-box-1m", box(1.0), r=1e-6), _m("r1e-6-box-3m", box(3.0), r=1e-6), _m("r1e-6-box-5m", box(5.0), r=1e-6, error=SF_ERR_UNSUPPORTED)]
    out += [_m("nan-coordinate", [[0, 0, 0], [0, np.nan, 0]], error=SF_ERR_FORMAT), _m("1e31-coordinate", [[0, 0, 0], [0, 0, 1e31]], error=SF_ERR_FORMAT)]
    out.append(_m("rounding", rounding_batch()))
    out += [_m("chain7", _chain(7)), _m("chain130", _chain(130)), _m("chain130-reversed", _chain(130)[::-1]),
            _m("apart130", _chain(130, spacing=0.0011)),                                                      # nobody has a lower neighbour: depth 0 everywhere
            _m("chain130-evens-first", np.concatenate([_chain(130)[0::2], _chain(130)[1::2]])),                   # depth 1 at most
            _m("two-centres", [[0, 0, 0], [0.0015, 0, 0], [0.00075, 0, 0], [1.0015, 0, 0], [1, 0, 0], [1.00075, 0, 0]]),
            _m("absorbed-neighbour-only", [[0, 0, 0], [0.0008, 0, 0], [0.0016, 0, 0]]),
            _m("one-cell-300", (np.array([20.05, 20.05, 20.05]) / INV + np.random.default_rng(3).uniform(0, 0.9 / INV, (300, 3))).astype(F32)),
            _m("coincident", [[0, 0, 0], [-0.0, 0, 0], [0, -0.0, -0.0], [1, 1, 1], [1, 1, 1], [0.5, 0, 0], [1, 1, 1]])]
    out += [_m("cloud-V%d" % v, _cloud(v, v)) for v in TAILS]
    out += [_m("count-lanes-from-64", _spaced_with_merges(256, (64, 127, 128, 255))), _m("count-last-partial-wave", _spaced_with_merges(330, (321, 329)))]
    # r == 0
    out += [_m("r0-runs-1-2-70", _runs_r0(), r=0),
            _m("r0-xy-equal-z-differs", [[1, 2, 3], [1, 2, 4], [1, 2, 3], [1, 2, 5], [1, 2, 4], [0, 2, 3]], r=0),
            _m("r0-z-equal-xy-differs", [[1, 2, 3], [1, 3, 3], [2, 2, 3], [1, 2, 3], [2, 2, 3], [1, 3, 3], [3, 1, 3]], r=0),
            _m("r0-signed-zeros", [[0, 1, 1], [-0.0, 1, 1], [1, 0, 1], [1, -0.0, 1], [1, 1, 0], [1, 1, -0.0], [-0.0, -0.0, -0.0], [0, 0, 0]], r=0),
            _m("r0-subnormals", [[0, 0, 0], [1e-40, 0, 0], [-1e-40, 0, 0], [1.4e-45, 0, 0], [0, 0, 1e-40], [0, 0, -1e-40], [0, 0, 1.4e-45], [0, 1e-40, 0],
                                 [1e-40, 0, 0], [0, 0, 1.4e-45], [-0.0, 0, 0]], r=0)]
    out += [_m("r0-lattice-V%d" % v, np.random.default_rng(100 + v).integers(0, 4, (v, 3)).astype(F32), r=0) for v in TAILS]
    return out


MERGE_CASES = _merge_cases()


# ---- faces ---------------------------------------------------------------------------------------------------------------------------------------------------
def _face_cases():
    u = lambda rows: np.array(rows, np.uint32).reshape(-1, 3)
    six = list(itertools.permutations((3, 7, 5)))
    big = 0xFFFFFFEF                                   # the largest vertex count sf_mesh_clean_gpu takes
    out = [FaceCase("degenerate-ab", 6, u([(0, 1, 2), (3, 3, 4), (2, 3, 4)]), None), FaceCase("degenerate-bc", 6, u([(0, 1, 2), (3, 4, 4), (2, 3, 4)]), None),
           FaceCase("degenerate-ac", 6, u([(0, 1, 2), (4, 3, 4), (2, 3, 4)]), None),
           FaceCase("six-corner-orders", 9, u([(0, 1, 2)] + six + [(8, 7, 6)]), None),
           FaceCase("three-and-four-copies", 9, u([(0, 1, 2), (5, 4, 3), (1, 2, 0), (3, 4, 5), (2, 1, 0), (4, 5, 3), (6, 7, 8), (5, 3, 4)]), None),
           FaceCase("lower-two-agree", 12, u([(1, 2, 3), (1, 2, 4), (2, 1, 5), (4, 2, 1), (9, 2, 1)]), None),
           FaceCase("highest-agrees", 12, u([(1, 2, 9), (1, 3, 9), (0, 2, 9), (9, 3, 1), (2, 9, 0), (9, 8, 7)]), None),
           FaceCase("ids-from-65536", 70000, u([(65536, 65537, 69999), (1, 65537, 69999), (65536, 65537, 4463), (69999, 65536, 65537), (65536 + 1, 1, 69999), (0, 65536, 0)]),
                    np.arange(70000, dtype=np.uint32)),
           FaceCase("ids-near-the-limit", big, u([(big - 1, big - 2, big - 3), (big - 1, big - 2, big - 65539), (big - 3, big - 1, big - 2), (65535, big - 2, big - 3),
                                                  (big - 65537, big - 2, big - 3), (big - 2, big - 3, 65535), (big - 1, 0, big - 1), (0, 1, 2)]), None),
           FaceCase("through-target", 8, u([(0, 1, 2), (0, 3, 2), (4, 5, 6), (4, 1, 7), (7, 5, 6), (2, 1, 4)]), np.array([0, 1, 2, 1, 0, 5, 6, 6], np.uint32)),
           FaceCase("all-degenerate", 4, u([(0, 0, 1), (1, 2, 2), (3, 1, 3), (2, 2, 2)]), None),
           FaceCase("all-but-one-duplicate", 4, u([(1, 2, 3)] + list(itertools.permutations((1, 2, 3))) * 3), None),
           FaceCase("F1", 3, u([(2, 0, 1)]), None), FaceCase("F1-degenerate", 3, u([(2, 0, 2)]), None)]
    for f in (255, 256, 257):
        out.append(FaceCase("random-F%d" % f, 12, np.random.default_rng(f).integers(0, 12, (f, 3)).astype(np.uint32), None))
    out.append(FaceCase("random-F257-through-target", 40, np.random.default_rng(9).integers(0, 40, (257, 3)).astype(np.uint32),
                        (np.arange(40) // 3 * 3).astype(np.uint32)))
    return out


FACE_CASES = _face_cases()


# ---- components ------------------------------------------------------------------------------------------------------------------------------------------------
def _strip(n):
    return np.array([(i, i + 1, i + 2) for i in range(n)], np.uint32)


def _grid_tris(nx, ny, first=0):
    t = []
    for y in range(ny - 1):
        for x in range(nx - 1):
            i = first + y * nx + x
            t += [(i, i + 1, i + nx), (i + 1, i + nx + 1, i + nx)]
    return np.array(t, np.uint32)


def _comp_cases():
    rng = np.random.default_rng(11)
    fan = np.array([(0, 1, 2 + i) for i in range(300)], np.uint32)
    strip = _strip(2000)
    touching = np.concatenate([_grid_tris(4, 4), np.where(_grid_tris(4, 4, first=16) == 16, 15, _grid_tris(4, 4, first=16))]).astype(np.uint32)
    sizes = np.concatenate([_strip(7), _strip(6) + 100, _strip(8) + 200, _strip(1) + 300])
    islands = np.arange(3 * 257, dtype=np.uint32).reshape(-1, 3)
    out = [CompCase("fan300", fan, 7), CompCase("fan300-and-a-strip", np.concatenate([_strip(40) + 1000, fan, _strip(5) + 2000])[rng.permutation(345)], 41),
           CompCase("strip2000-shuffled", strip[rng.permutation(2000)], 2000), CompCase("strip2000-reversed", strip[::-1], 2001), CompCase("strip2000", strip, 100),
           CompCase("grids-touching-in-a-vertex", touching, 19), CompCase("grids-touching-in-a-vertex-shuffled", touching[rng.permutation(len(touching))], 18)]
    out += [CompCase("sizes-6-7-8-1-min%d" % m, sizes, m) for m in (0, 1, 2, 6, 7, 8, 9)]
    out += [CompCase("islands257", islands, 1), CompCase("islands257-min2", islands, 2), CompCase("F1", _strip(1), 1),
            CompCase("third-edge-of-one", np.array([(0, 1, 2), (2, 0, 3)], np.uint32), 2), CompCase("third-edge-of-both", np.array([(0, 1, 2), (2, 5, 0)], np.uint32), 2),
            CompCase("third-edge-chain", np.array([(0, 1, 2), (2, 5, 0), (9, 8, 7), (5, 6, 2), (7, 4, 9)], np.uint32)[::-1], 3)]
    for f in (255, 256, 257):
        out.append(CompCase("random-F%d" % f, np.random.default_rng(f).integers(0, 300, (f, 3)).astype(np.uint32), 4))
    return out


COMP_CASES = _comp_cases()


# ---- compact -----------------------------------------------------------------------------------------------------------------------------------------------------
def _compact_cases():
    out = []
    for v in TAILS + (300,):
        rng = np.random.default_rng(500 + v)
        pos, col = rng.normal(size=(v, 3)).astype(F32), rng.integers(0, 256, (v, 4), dtype=np.uint8)
        lim = max(1, v - 1)                                                             # the last vertex stays unused ...
        tri = rng.choice(lim, (max(1, v // 6), 3)).astype(np.uint32) if v > 1 else np.zeros((1, 3), np.uint32)
        out.append(CompactCase("V%d-last-unused-colour" % v, pos, col, tri))
        out.append(CompactCase("V%d-last-used" % v, pos, None, np.concatenate([tri, np.array([(v - 1, 0, v // 2)], np.uint32)])))   # ... or is used
        out.append(CompactCase("V%d-no-faces" % v, pos, col if v % 2 else None, np.zeros((0, 3), np.uint32)))
    return out


COMPACT_CASES = _compact_cases()


# ---- whole ---------------------------------------------------------------------------------------------------------------------------------------------------------
def whole_cases():
    """every merge case that names no error, given faces (random triples, a strip, duplicates of both) and colours: (name, pos, col, tri, r, min_faces)"""
    out = []
    for k, c in enumerate(MERGE_CASES):
        if c.error is not None:
            continue
        v = len(c.pos)
        rng = np.random.default_rng(900 + k)
        tri = rng.integers(0, v, (2 * v, 3)).astype(np.uint32)
        if v >= 3:
            strip = np.array([(i, i + 1, i + 2) for i in range(0, v - 2)], np.uint32)
            tri = np.concatenate([tri, strip, strip[::3][:, ::-1], tri[::5]])
        out.append((c.name, c.pos, rng.integers(0, 256, (v, 4), dtype=np.uint8) if k % 2 else None, tri, c.r, (0, 1, 2, 5)[k % 4]))
    return out


def by_name(name):
    return next(c for c in MERGE_CASES + FACE_CASES + COMP_CASES + COMPACT_CASES if c.name == name)


def occupied_cells(pos, r):
    """how many cells of the filter's grid hold a vertex (the grid formula: a builder's aid, not part of the statement)"""
    inv = 0.5 / (float(F32(r)) * (1.0 + 1e-5))
    return len({tuple(math.floor(float(q) * inv) for q in p) for p in np.asarray(pos, F32).reshape(-1, 3)})


def run_stages(stages, pos, col, tri, r, min_faces):
    """The whole filter chain as the composition of (merge, faces, components, compact) -- the statement's, or the device's stage hooks -- with the
    statistics taken from the stage results alone: (pos, col, tri, stats)."""
    merge, faces, components, compact = stages
    pos, tri = np.asarray(pos, F32).reshape(-1, 3), np.asarray(tri, np.uint32).reshape(-1, 3)
    target = merge(pos, r)
    fa = faces(len(pos), tri, target)
    st = {"vertices_in": len(pos), "faces_in": len(tri), "vertices_merged": int((target != np.arange(len(pos))).sum()), "faces_degenerate": fa["degenerate"],
          "faces_duplicate": fa["duplicate"], "components_in": 0, "components_removed": 0, "faces_small_component": 0}
    left = fa["tri"]
    if len(left):
        co = components(left, min_faces)
        st["components_in"], st["components_removed"], st["faces_small_component"] = (int(x) for x in co["counters"])
        left = left[co["keep"] == 1]
    cm = compact(pos, col, left)
    st["vertices_out"], st["faces_out"] = cm["vertices_out"], len(left)
    st["vertices_unreferenced"] = st["vertices_in"] - st["vertices_merged"] - st["vertices_out"]
    return cm["pos"], cm["col"], cm["tri"], st
