"""The meshes and parameter sets of tests/test_simplify_stages_cpu.py and tests/test_simplify_stages.py: the smallest shapes at which each kernel of
scannet_amd/csrc/simplify_gpu.hip can go wrong, and the round loop of the decimation driven through stage calls (run_rounds)."""
import functools
import itertools

import numpy as np

from tests import meshes


def grid(nx, ny, z=None, flat_border=False):
    """integer lattice nx x ny with heights z(x, y), two triangles per cell; flat_border: height 0 along the border, whose edges are then unit axis steps"""
    def h(x, y):
        return 0 if z is None or (flat_border and (x in (0, nx - 1) or y in (0, ny - 1))) else z(x, y)
    v = np.array([(x, y, h(x, y)) for y in range(ny) for x in range(nx)], np.float32)
    f = []
    for y in range(ny - 1):
        for x in range(nx - 1):
            i = y * nx + x
            f += [(i, i + 1, i + nx), (i + 1, i + nx + 1, i + nx)]
    return v, np.array(f, np.uint32)


def rough(n, seed=3):
    """a heightfield rough enough that every summed quadric is full rank by a wide margin (meshes.bumpy(12) is too gentle for that: a third of its edges
    sit within a factor 2 of the det > 1e-6 trace^3 rule, where the statement cannot tell the two branches of the minimiser apart)"""
    rng = np.random.default_rng(seed)
    v, f = grid(n, n)
    v = v * np.float32(0.02)
    v[:, 2] = (0.02 * np.sin(v[:, 0] * 90) * np.cos(v[:, 1] * 70) + rng.normal(0, 0.004, len(v))).astype(np.float32)
    return v, f


def strip(n):
    """n quads in a row, one quad wide: 2n + 2 vertices, 3n + 1 edges; every interior edge joins two border vertices"""
    return grid(n + 1, 2)


def fan(n, hub_first):
    """a closed fan of n faces around a hub at the apex of a flat cone: n + 1 vertices, 2n edges.  hub_first: the hub is vertex 0, v0 of every spoke,
    and its ring (two entries per face) is the one the link test holds; otherwise the hub is vertex n, v1 of every spoke."""
    a = np.arange(n) * (2 * np.pi / n)
    rim = np.stack([np.cos(a), np.sin(a), np.zeros(n)], -1)
    hub = np.array([[0.0, 0.0, 0.25]])
    if hub_first:
        v = np.concatenate([hub, rim])
        f = [(0, 1 + i, 1 + (i + 1) % n) for i in range(n)]
    else:
        v = np.concatenate([rim, hub])
        f = [(n, i, (i + 1) % n) for i in range(n)]
    return v.astype(np.float32), np.array(f, np.uint32)


def islands(n):
    """n separate triangles (i, n + i, 2n + i): edges 2i and 2i + 1 are the two at vertex i, edge 2n + i the third; 3n vertices and edges"""
    v = np.array([(3 * i + dx, dy, 0) for dx, dy in ((0, 0), (1, 0), (0, 1)) for i in range(n)], np.float32)
    return v, np.array([(i, n + i, 2 * n + i) for i in range(n)], np.uint32)


TETRA = (np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]], np.float32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.uint32))
OCTA = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32),
        np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32))
CUBE = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float32) + np.float32([1, 2, 3]),
        np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]], np.uint32))

# coordinates of 1e25: the adjugate solve of the placement overflows (products of 1e200 and 1e125) to inf - inf on the edges at vertex 0, which take the
# NaN guard, and to plain inf elsewhere
HUGE = (np.array([[1.8125751127161427e+25, 3.328467551146e+25, -3.1436825958265357e+25], [-2.2197762659732882e+25, 2.2946393792005265e+25, 3.0431596004241657e+25],
                  [-2.141361693343259e+25, -1.2878098618813343e+25, 3.1064646755677202e+25], [-1.2438315557959556e+25, -2.2624906242131664e+25, 2.2705227977514614e+25],
                  [-2.251025742187055e+25, -1.0653322132274574e+25, 1.3605303857844111e+25]], np.float32),
        np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 4], [1, 4, 3], [2, 3, 4]], np.uint32))

DEFAULTS = {"quality_thr": 0.3, "boundary_weight": 1.0, "optimal_placement": 1, "planar_quadric": 0}


class Case:
    """One mesh with one parameter set.  exact_q: every binary64 operation of the initial quadrics is exact (integer coordinates, unit axis-aligned
    border edges, no planar_quadric).  closed_or_lattice: no edge may be unsure.  soup: held against the checker alone."""

    def __init__(self, name, mesh, exact_q=False, closed_or_lattice=False, soup=False, alive=None, **params):
        self.name, self.exact_q, self.closed_or_lattice, self.soup = name, exact_q, closed_or_lattice, soup
        self.pos, self.tri = np.ascontiguousarray(mesh[0], np.float32), np.ascontiguousarray(mesh[1], np.uint32)
        self.alive = np.ones(len(self.tri), np.uint8) if alive is None else np.asarray(alive, np.uint8)
        self.params = dict(DEFAULTS, **params)

    def __repr__(self):
        return self.name

    @property
    def oracle_kw(self):
        return dict(self.params)


def _lattice_cases():
    out = []
    # (grid3x3 left flat puts a quarter of its edges, under planar_quadric, within a factor 2 of the det > 1e-6 trace^3 rule: its centre is raised)
    shapes = (("grid3x3", grid(3, 3, z=lambda x, y: 1, flat_border=True)), ("grid5x4", grid(5, 4, z=lambda x, y: (x * y) % 3, flat_border=True)), ("tetra", TETRA), ("octa", OCTA), ("cube", CUBE))
    for (name, mesh), planar, bw, opt, thr in itertools.product(shapes, (0, 1), (1.0, 2.0), (0, 1), (0.0, 0.3)):
        out.append(Case("%s-planar%d-bw%g-opt%d-thr%g" % (name, planar, bw, opt, thr), mesh, exact_q=not planar, closed_or_lattice=True, planar_quadric=planar,
                        boundary_weight=bw, optimal_placement=opt, quality_thr=thr))
    return out


def _crease(x, y):
    return max(x - 2, 0)


def _with_ear(mesh):
    """one more vertex, joined by one face to the border edge (0, 1)"""
    v, f = mesh
    return np.concatenate([v, np.float32([[0.5, -1.0, 0.5]])]), np.concatenate([f, np.uint32([[1, 0, len(v)]])])


def _edge_cases():
    out = [
        # rank: flat (rank 1, every priority at the floor), two planes (rank 2 off the border), a noisy heightfield (full rank)
        Case("flat4x4", grid(4, 4), exact_q=True, closed_or_lattice=True),
        Case("crease5x5", grid(5, 5, z=_crease), closed_or_lattice=True),      # its border climbs the crease: not unit steps
        Case("rough12", rough(12)),
        # k_priority's 128-lane workgroup, k_winners' waves, the 256-wide grids over V
        Case("fan64-E128-V65", fan(64, False)),
        Case("strip32-E129-V66", strip(32), exact_q=True, closed_or_lattice=True),
        Case("grid17x15-V255", grid(17, 15, z=lambda x, y: (x * x + y) % 4, flat_border=True), exact_q=True, closed_or_lattice=True),
        Case("grid16x16-V256", grid(16, 16, z=lambda x, y: (x + y * y) % 4, flat_border=True), exact_q=True, closed_or_lattice=True),
        Case("grid16x16-ear-V257", _with_ear(grid(16, 16, z=lambda x, y: (x + y * y) % 4, flat_border=True))),
        # the ring limit: 96 entries pass, 98 reject; no limit on v1's valence
        Case("fan48-hub-v0", fan(48, True)),
        Case("fan49-hub-v0", fan(49, True)),
        Case("fan48-hub-v1", fan(48, False)),
        Case("fan49-hub-v1", fan(49, False)),
        Case("fan200-hub-v1", fan(200, False)),
        # border fans: grid3x3 above has the interior edge that ends on the border and the edges along it; here every interior edge joins two border
        # vertices, and the neighbour at the open end of v1's fan is found only as the vertex BEFORE v1 in a face
        Case("strip3", strip(3), exact_q=True, closed_or_lattice=True),
        # guards: without optimal placement edge (0, 3) moves vertex 0 to (6, 0), onto the line of its face (0, 1, 2): worst quality 0, priority 3e38
        Case("collinear-opt0", (np.array([[0, 4, 0], [0, 0, 0], [2, 0, 0], [6, 0, 0], [4, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 4], [0, 4, 3]], np.uint32)),
             closed_or_lattice=True, optimal_placement=0),
    ]
    return out


def _soup_cases():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [-1, 0, 1]], np.float32)
    return [
        Case("soup-three-faces-on-an-edge", (p, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 4]], np.uint32)), soup=True),
        Case("soup-face-twice", (p, np.array([[0, 1, 2], [0, 1, 2], [1, 0, 3]], np.uint32)), soup=True),
        Case("soup-flipped-pair", (p[:3], np.array([[0, 1, 2], [2, 1, 0]], np.uint32)), soup=True),
        Case("bumpy12-checker-only", meshes.bumpy(12), soup=True),      # see rough(): edges at the branch point of the minimiser
        Case("soup-dead-faces", grid(4, 4, z=lambda x, y: x % 2), soup=True, alive=[1, 0, 1, 1, 0, 1] * 3),
    ]


LATTICE_CASES = _lattice_cases()
EDGE_CASES = _edge_cases()
SOUP_CASES = _soup_cases()
ALL_CASES = LATTICE_CASES + EDGE_CASES + SOUP_CASES
# the lattice sweep is 80 parameter sets of five tiny meshes: the later stages take every mesh once per placement mode
STAGE_CASES = [c for c in LATTICE_CASES if "-planar0-bw1-" in c.name and c.name.endswith("thr0.3")] + EDGE_CASES + SOUP_CASES


def by_name(name):
    return next(c for c in ALL_CASES if c.name == name)


# ---- winners on hand-made priorities: (name, mesh, priorities of the edges in key order, tau, round) -------------------------------------------------
def winner_cases():
    out = []
    isl = islands(70)      # 210 edges: waves of 64 at edges 0, 64, 128; the last one holds 18
    n = 210

    def pri(ids, lo=1.0):
        p = np.full(n, 5.0, np.float32)
        p[list(ids)] = lo
        return p
    out.append(("islands-no-candidate", isl, pri(()), 2.0, 0))
    out.append(("islands-one-winner-in-wave-0", isl, pri((5,)), 2.0, 0))
    # the two edges at a face's lowest vertex are neighbours in key order and conflict: every other lane of wave 0
    out.append(("islands-32-winners-in-wave-0", isl, pri(range(0, 64, 2)), 2.0, 0))
    # islands(96): the third edges (96 + i, 192 + i) are edges 192 .. 287, one per triangle; 192 .. 255 fill the fourth wave of 64 lanes, and all win
    p96 = np.full(288, 5.0, np.float32)
    p96[192:256] = 1.0
    out.append(("islands96-64-winners-in-one-wave", islands(96), p96, 2.0, 0))
    out.append(("islands-winners-only-in-the-last-partial-wave", isl, pri(range(200, 210)), 2.0, 1))
    out.append(("islands-every-edge-tied", isl, np.full(n, 1.0, np.float32), 2.0, 2))
    g = grid(9, 8)
    ne = 8 * 8 + 9 * 7 + 8 * 7
    for rnd in (0, 5):
        out.append(("grid9x8-every-edge-tied-round%d" % rnd, g, np.full(ne, 1e-15, np.float32), 1e-15, rnd))
    rng = np.random.default_rng(11)
    p = rng.choice(np.float32([1e-15, 2e-15, 1.0, 3.0e38, np.inf]), ne).astype(np.float32)
    out.append(("grid9x8-mixed-priorities-tau-at-the-clamp", g, p, 3.0e38, 3))
    out.append(("grid9x8-mixed-priorities", g, p, 1.0, 1))
    f = fan(64, False)
    out.append(("fan64-every-edge-tied", f, np.full(128, 1.0, np.float32), 1.0, 0))
    return out


# ---- the round loop, through stage calls ------------------------------------------------------------------------------------------------------------
def run_rounds(stages, pos, tri, target_faces, **params):
    """The round loop of the decimation driven through the three stage calls of `stages` (edges, winners, collapse: oracle.simplify_stage_* or
    meshclean.stage_*), dead faces squeezed out as the product does -> (pos, tri, alive, vdel, log); log has one entry per round:
    {"faces" (in the arrays), "alive", "E", "tau", "winners", "take", "squeezed"}.  Degenerate faces are dropped up front."""
    edges, winners, collapse = stages
    params = dict(DEFAULTS, **params)
    pos, tri = np.array(pos, np.float32), np.array(tri, np.uint32)
    alive = ((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])).astype(np.uint8)
    vdel = np.zeros(len(pos), np.uint8)
    nalive, Q, scale, stalled, rnd, log = int(alive.sum()), None, 0.0, 0, 0, []
    while nalive > target_faces:
        squeezed = nalive * 4 < len(tri) * 3
        if squeezed:
            tri, alive = tri[alive != 0], np.ones(nalive, np.uint8)
        needed = (nalive - target_faces + 1) // 2
        ed = edges(pos, tri, alive, Q, scale=scale, needed=needed, stalled=stalled, **params)
        if ed["E"] == 0:
            break
        Q, scale = ed["Q"], ed["scale"]
        w = winners(len(pos), tri, alive, ed["pri"], ed["tau"], rnd)
        rnd += 1
        nwin, removed = int(w["counters"][0]), int(w["counters"][1])
        entry = {"faces": len(tri), "alive": nalive, "E": ed["E"], "tau": float(ed["tau"]), "winners": nwin, "take": nwin, "squeezed": squeezed}
        log.append(entry)
        if nwin == 0:
            stalled += 1
            if stalled >= 2:
                break
            continue
        stalled = 0
        ids = np.nonzero(w["passes"])[0]
        if nalive - removed >= target_faces:
            nalive -= removed
        else:      # the last round: winners in (priority bits, edge) order up to the budget
            order = sorted(ids, key=lambda e: (int(ed["pri"][e:e + 1].view(np.uint32)[0]), int(e)))
            take, gone = 0, 0
            while take < len(order) and nalive - gone > target_faces:
                gone += int(ed["ucnt"][order[take]])
                take += 1
            ids, entry["take"] = np.array(order[:take]), take
            nalive -= gone
        c = collapse(pos, tri, alive, Q, ids, ed["x"])
        pos, tri, alive, Q = c["pos"], c["tri"], c["alive"], c["Q"]
        vdel |= c["vdel"]
    return pos, tri, alive, vdel, log


@functools.lru_cache(None)
def whole_run_cases():
    """(name, mesh, target_faces): grid5x5's budget cuts inside the last round's winners; grid12x12 to 20 % squeezes its dead faces before the last round"""
    return (("grid5x5-cut", grid(5, 5, z=lambda x, y: (x * y) % 2), 21), ("grid12x12-squeeze", grid(12, 12, z=lambda x, y: (x * x + 2 * y) % 3), int(242 * 0.2)))
