"""The annotation projector, stage by stage (scannet_amd/csrc/project.hip; AnnotationTools/ProjectAnnotations/Visualizer.cpp:57-186).

Three parties:
  * the HIP kernels through the stage hooks of include/scanfuse_internal.h (Projector.stage_raster / stage_resolve / stage_vote), which launch them
    through the helpers sf_projector_run itself uses;
  * the checker oracle/project_oracle.c, split the same way (or_project_raster / _resolve / _vote), which the kernels are held to bit for bit;
  * tests/project_exact.py, an independent statement of the Direct3D 11 rules the checker's header lists: exact (integers and fractions) on a
    lattice of fronto-parallel triangles where every float32 operation of the transform is exact, float64 with "sure" pixels for general poses and
    sloped triangles, exact for the vote and (off exact equality) for the depth-consistency filter.

CPU part: the checker against the statements on every case the GPU part uses.  GPU part (-m gpu): every case against the checker's matching stage bit
for bit, lattice cases against the exact statement too, and wherever a case exists to reach a branch (the queue of k_pa_raster_big, its second grid
stride) the count the raster stage returns says that it was reached.

On the CPU the checker equals the exact statements on every lattice, vote and resolve case, and meets the float64 statement on sure pixels with at most
1.1 % of the covered pixels of a case left out as unsure (room pose 2; the cap is 3 %).

One-line mutations of project.hip tried on a scratch copy, each with the GPU tests here that failed under it:
  * the `e0 == 0 && !(TL & 1)` exclusion dropped from the 32-bit path only: test_gpu_raster_on_the_lattice[fill_rule], [diagonal_a], [diagonal_b],
    [clusters_*], [on_the_near_plane], [ties_far_apart], [ties_small_first];
  * `2 * t + sub` as the id in the big path: test_gpu_raster_on_the_lattice[wide_600], [viewport], [degenerate], [ties_small_first],
    [on_the_near_plane], test_gpu_raster_general_poses[room], [floor], [near_plane], [near_split], test_gpu_raster_batch_with_invalid_frames;
  * k_pa_raster_big without its grid stride: test_gpu_raster_on_the_lattice[wide_600];
  * 25 as `total` everywhere in the vote: test_gpu_vote at all seven sizes;
  * `sx` truncated instead of rounded in k_pa_resolve: test_gpu_resolve[162x121_80x60], [80x60_162x121], [1296x968_640x480]."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc
from scannet_amd import project
from tests import project_exact as px
from tests import test_project as tp

ALL1 = np.uint64(2 ** 64 - 1)
EYE = np.eye(4, dtype=np.float32)

# The float64 statement against the checker, measured on the CPU one triangle at a time over every triangle and pose of the float cases below
# (python -m tests.test_project_stages prints the figures); not derived from any device output.
#   EDGE_MEASURED         the largest distance (pixels) from a pixel centre to the triangle's projected boundary among the centres the two disagree
#                         on: the 1/256 snap moves an edge by up to sqrt(2) / 512 = 0.0028 pixel
#   DEPTH_FLAT_MEASURED   the largest |z_ndc| difference on centres both cover, on surfaces flatter than FLAT_SLOPE z_ndc per pixel: rounding
#   DEPTH_SHIFT_MEASURED  on steeper surfaces, the largest |z_ndc| difference divided by the surface's slope |grad z_ndc|: how many pixels the
#                         surface is displaced across the screen, again the snap (the checker's depth plane passes through the SNAPPED vertices)
# The margin of 4 covers the freedom of the fp32 transform and of the snap at other positions than the ones measured.
EDGE_MEASURED = 0.001744            # room
DEPTH_FLAT_MEASURED = 3.973e-07     # room (huge 1.1e-07; the other cases have no flat surface)
DEPTH_SHIFT_MEASURED = 0.003833    # room (near_plane and near_split 0.0025, huge 0.0018, floor 0.0007)
EDGE_MARGIN = 4 * EDGE_MEASURED
DEPTH_FLAT = 4 * DEPTH_FLAT_MEASURED
DEPTH_SHIFT = 4 * DEPTH_SHIFT_MEASURED
UNSURE_CAP = 0.03


# ================================================================================================================ lattice cases
class Lattice:
    """A mesh of fronto-parallel triangles given by their screen positions in 1/1024 pixel, for the lattice camera of tests/project_exact.py; plus
    triangles the rules never draw (None in `spec`)."""

    def __init__(self, w=128, h=64, near=0.1, far=15.0):
        self.w, self.h, self.near, self.far = w, h, near, far
        self.xyz, self.tris, self.spec = [], [], []
        self.late = None          # what the raster stage must report as queued, where the case is about that

    def params(self):
        return project.default_params((self.w, self.h), (self.w, self.h), 64.0, 64.0, depth_min=self.near, depth_max=self.far)

    def _vertex(self, kx, ky, z):
        # the preconditions of exactness: screen coordinates x 1024 are integers below 2^24, and the camera-space position is a binary32 number
        assert isinstance(kx, int) and isinstance(ky, int) and abs(kx) < 2 ** 24 and abs(ky) < 2 ** 24
        pos = px.lattice_vertex(kx, ky, z, self.w, self.h)
        for c in pos:
            assert Fraction(float(np.float32(c.numerator / c.denominator))) == c, (kx, ky, z)
        self.xyz.append([float(c) for c in pos])
        return len(self.xyz) - 1

    def tri(self, a, b, c, z):
        """a, b, c: (x, y) in pixels, multiples of 1/1024"""
        k = []
        for p in (a, b, c):
            q = (Fraction(p[0]) * 1024, Fraction(p[1]) * 1024)
            assert q[0].denominator == 1 and q[1].denominator == 1, p
            k.append((int(q[0]), int(q[1])))
        self.tris.append([self._vertex(kx, ky, z) for kx, ky in k])
        self.spec.append((k[0], k[1], k[2], Fraction(z)))
        return len(self.tris) - 1

    def rect(self, x0, y0, x1, y1, z):
        self.tri((x0, y0), (x1, y0), (x1, y1), z)
        self.tri((x0, y0), (x1, y1), (x0, y1), z)

    def raw(self, verts):
        """three camera-space positions the rules never draw (non-finite)"""
        base = len(self.xyz)
        self.xyz += [list(v) for v in verts]
        self.tris.append([base, base + 1, base + 2])
        self.spec.append(None)

    def bad_index(self, which):
        t = [0, 1, 2]
        t[which] = -1          # patched to V (the first index out of range) by arrays()
        self.tris.append(t)
        self.spec.append(None)

    def scatter(self, rng, n, size=12.0, zs=(0.5, 1, 2, 4), half=0.5):
        """n random small triangles; `half` of the coordinates sit exactly half-way between two 1/256 positions"""
        for _ in range(n):
            cx, cy = rng.uniform(-4, self.w + 4), rng.uniform(-4, self.h + 4)
            p = []
            for _ in range(3):
                k = [int(round((c + rng.uniform(-size, size)) * 1024)) for c in (cx, cy)]
                k = [(v // 4) * 4 + 2 if rng.random() < half else v for v in k]
                p.append((Fraction(k[0], 1024), Fraction(k[1], 1024)))
            self.tri(p[0], p[1], p[2], zs[rng.integers(len(zs))])

    def arrays(self):
        xyz = np.array(self.xyz, np.float32)
        tris = np.array(self.tris, np.int64)
        tris[tris < 0] = len(xyz)
        return xyz, tris.astype(np.uint32)


def _case_fill_rule():
    """rectangles and right triangles whose edges lie exactly on pixel centres -- left, top, right, bottom in turn"""
    m = Lattice()
    m.rect(10.5, 5.5, 20.5, 9.5, 2)                     # all four edges on centres: left and top in, right and bottom out
    m.rect(30.5, 5.25, 40.25, 9.75, 1)                  # left only
    m.rect(50.25, 5.5, 60.75, 9.25, 4)                  # top only
    m.rect(70.25, 5.25, 80.5, 9.75, 0.5)                # right only
    m.rect(90.25, 5.25, 100.75, 9.5, 2)                 # bottom only
    for k, (cx, cy) in enumerate([(10.5, 30.5), (40.5, 30.5), (70.5, 30.5), (100.5, 30.5)]):      # the right angle at each corner in turn
        sx, sy = (1, -1)[k & 1], (1, -1)[k >> 1]
        m.tri((cx, cy), (cx + 12 * sx, cy), (cx, cy + 12 * sy), 1)               # both legs through centres, the hypotenuse through centres too
        m.tri((cx, cy + 22), (cx, cy + 22 + 9 * sy), (cx + 14 * sx, cy + 22), 2)   # the other winding
    return m


def _case_shared_diagonal(order):
    """two triangles sharing a diagonal through pixel centres: the statement gives each centre to one of them, whichever is stored first"""
    m = Lattice()
    quads = [((10.5, 10.5), (26.5, 10.5), (26.5, 26.5), (10.5, 26.5)), ((60.5, 10.5), (76.5, 10.5), (76.5, 26.5), (60.5, 26.5))]
    for q, (a, b, c, d) in enumerate(quads):
        pair = [(a, b, c), (a, c, d)] if q == 0 else [(b, c, d), (d, a, b)]       # the diagonal a-c, then b-d
        for t in (pair if order == 0 else pair[::-1]):
            m.tri(*t, 2)
    m.tri((100.5, 40.5), (116.5, 40.5), (108.5, 56.5), 1)
    m.tri((116.5, 40.5), (100.5, 40.5), (108.5, 24.5), 1)                         # sharing a horizontal edge through centres
    return m


def _case_subpixel(seed):
    m = Lattice()
    m.scatter(np.random.default_rng(seed), 150)
    return m


def _case_degenerate():
    """zero-area triangles, slivers that cover no centre, a one-pixel triangle -- among drawable neighbours"""
    m = Lattice()
    m.rect(2.25, 2.25, 120.75, 60.75, 4)                                          # a backdrop
    m.tri((10.5, 10.5), (20.5, 20.5), (30.5, 30.5), 1)                            # collinear
    m.tri((40.5, 10.5), (40.5, 10.5), (50.5, 20.5), 1)                            # a repeated vertex
    m.tri((60.5, 10.5), (60.5, 10.5), (60.5, 10.5), 1)                            # a point
    m.tri((70, 10), (70 + Fraction(1, 1024), 10), (80, 20), 1)                    # zero area only after the snap
    sliver = [m.tri((5.25, 20.25), (110.75, 50.25), (110.75, 50.25 + Fraction(1, 256)), 1), m.tri((90.25, 3.25), (93.75, 58.75), (93.75 + Fraction(1, 128), 58.75), 1)]
    one = m.tri((50.25, 40.25), (51, 40.25), (50.25, 41), 1)                      # holds the centre (50.5, 40.5) only
    m.expect_cover = {sliver[0]: 0, sliver[1]: 0, one: 1}
    return m


BLOCK_WIDTHS, BLOCK_HEIGHTS = (1, 8, 9, 16, 17, 32, 33, 64, 65), (1, 2, 8, 9, 64, 65)


def _case_block_shapes(bh):
    """bounding boxes of bw x bh centres at the thresholds of the 32-bit path's block shape (sh = 3 / 4 / 5 / 6 for bw <= 8 / 16 / 32 / more) and
    at the largest box a span of 64 pixels has: a rectangle (both halves share the box) and one more triangle in a box of the same size"""
    m = Lattice(512, 128)
    x = 3
    for k, bw in enumerate(BLOCK_WIDTHS):
        ext = lambda a, n: (a + 0.25, a + 0.75) if n == 1 else (a + 0.5, a + n - 0.5)
        (x0, x1), (y0, y1) = ext(x, bw), ext(5 + 3 * k, bh)
        m.rect(x0, y0, x1, y1, 2)
        m.tri((x0, y1), (x1, y0), (x1, y1), 1)                                    # in front of the lower right half
        x += bw + 2
    m.late = 0
    return m


def _case_path_boundary(axis, extra):
    """one triangle whose longest edge component is 16384 (extra = 0) or 16385 (extra = 1) subpixels"""
    m = Lattice(128, 128)
    e = 64 + Fraction(extra, 256)
    # quarter-pixel positions: no centre comes within 1/256 pixel of an edge, so moving a vertex by 1/256 can change the last column / row only
    m.tri((10.25, 10.25), (10.25 + e, 30.25), (20.25, 50.25), 2) if axis == "x" else m.tri((10.25, 10.25), (30.25, 10.25 + e), (50.25, 20.25), 2)
    m.late = extra
    return m


def _case_whole_image():
    m = Lattice()
    m.tri((-100, -100), (400, -100), (-100, 300), 2)
    m.scatter(np.random.default_rng(5), 20)
    m.late = 1
    return m


def _case_600_wide():
    """600 thin triangles each 70 pixels wide, none hidden: the 512 workgroups of k_pa_raster_big take a second stride"""
    m = Lattice(512, 128)
    for t in range(600):
        x0, y0 = 4 + 100 * (t // 120) + Fraction(t % 7, 8), 3 + (t % 120) + Fraction(t % 5, 16)
        m.tri((x0, y0), (x0 + 70, y0 + Fraction(1, 4)), (x0, y0 + 1 + Fraction(3, 8)), (0.5, 1, 2, 4)[t % 4])
    m.late = 600
    return m


def _case_on_the_near_plane():
    """all three vertices exactly on the near plane: z_clip = A z - B is exactly 0 for z = depth_min = 0.5 (A / 2 and B are the same binary32 number),
    and 0 counts as inside"""
    m = Lattice(near=0.5, far=4.0)
    m.rect(2.25, 2.25, 120.75, 60.75, 1)
    m.tri((20.5, 10.5), (60.25, 12.75), (30.75, 50.5), 0.5)
    m.scatter(np.random.default_rng(6), 20, zs=(0.5, 1, 2, 4))
    return m


def _case_viewport():
    """triangles crossing each border and each corner, and wholly outside each side"""
    m = Lattice()
    W, H = m.w, m.h
    for cx, cy in [(0, 30), (W, 30), (60, 0), (60, H), (0, 0), (W, 0), (0, H), (W, H)]:
        m.tri((cx - 9.25, cy - 7.5), (cx + 10.5, cy - 3.25), (cx - 2.75, cy + 8.5), 2)
    for cx, cy in [(-20, 30), (W + 20, 30), (60, -20), (60, H + 20)]:            # wholly outside each side
        m.tri((cx - 9.25, cy - 7.5), (cx + 10.5, cy - 3.25), (cx - 2.75, cy + 8.5), 2)
    m.tri((-9, 20), (0.25, 25), (-3, 40), 2)                                       # outside by less than half a pixel: inside the view volume,
    m.tri((W - 0.25, 20), (W + 9, 25), (W + 3, 40), 2)                             # yet no centre in the box
    m.tri((-3000, 10.5), (3000, 10.5), (0, 14000), 4)                              # far larger than the image, queued
    m.tri((-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5), 1)                               # touches the corner pixel's centre: not covered (right / bottom)
    m.tri((0.5, 0.5), (1.5, 0.5), (0.5, 1.5), 1)                                   # covers exactly the corner pixel
    m.late = 1
    return m


def _case_clusters(F):
    m = Lattice()
    m.tri((10.5, 10.5), (40.25, 12.75), (12.75, 40.5), 2)
    m.scatter(np.random.default_rng(100 + F), F - 1, size=8.0)
    return m


def _case_culled_clusters():
    """one workgroup = four clusters of 64 triangles: visible, wholly behind the camera, wholly off-screen, and one whose box straddles the camera
    plane while all but one of its triangles are visible (it must be drawn)"""
    m = Lattice()
    rng = np.random.default_rng(7)
    m.scatter(rng, 64, size=8.0)
    for k in range(64):
        m.tri((10.5 + k, 10.5), (30.5 + k, 12.5), (12.5 + k, 40.5), -2)            # behind
    for k in range(64):
        m.tri((300.5 + k, 10.5), (330.5 + k, 12.5), (312.5 + k, 40.5), 2)          # to the right of the image
    m.tri((40.5, 20.5), (80.5, 22.5), (42.5, 50.5), -1)                            # behind, in the last cluster ...
    m.scatter(rng, 63, size=8.0)                                                   # ... whose other triangles are in view
    m.late = 0
    return m


def _case_ties(which):
    m = Lattice()
    rng = np.random.default_rng(8)
    if which == "far_apart":          # the same triangle at indices 3 and 200, in different clusters
        for t in range(260):
            m.tri((30.5, 10.5), (90.25, 20.75), (40.75, 55.5), 2) if t in (3, 200) else m.scatter(rng, 1, size=6.0, zs=(4,))
        m.expect_winner = (40, 30, 3)
    else:                             # a small triangle and a queued large one on one plane, in both index orders
        big, small = ((2.5, 2.5), (125.5, 4.5), (4.5, 61.5)), ((20.5, 10.5), (40.5, 12.5), (22.5, 30.5))
        for t in (big, small) if which == "big_first" else (small, big):
            m.tri(*t, 2)
        m.late = 1
        m.expect_winner = (25, 15, 0)
    return m


def _case_never_drawn():
    """NaN and +-inf in x, in z and in all coordinates of a vertex, and an index >= V: each in a cluster with drawable neighbours"""
    m = Lattice()
    rng = np.random.default_rng(9)
    good = [[-0.2, -0.1, 1.0], [0.3, -0.2, 1.0], [0.1, 0.3, 1.0]]
    for bad in (np.nan, np.inf, -np.inf):
        for coords in ((0,), (2,), (0, 1, 2)):
            for vertex in (0, 1, 2):
                m.scatter(rng, 3, size=10.0)
                v = [list(g) for g in good]
                for c in coords:
                    v[vertex][c] = bad
                m.raw(v)
    for which in range(3):
        m.scatter(rng, 3, size=10.0)
        m.bad_index(which)
    return m


LATTICE_CASES = {"fill_rule": _case_fill_rule, "diagonal_a": lambda: _case_shared_diagonal(0), "diagonal_b": lambda: _case_shared_diagonal(1),
                 "subpixel_0": lambda: _case_subpixel(0), "subpixel_1": lambda: _case_subpixel(1), "degenerate": _case_degenerate,
                 "whole_image": _case_whole_image, "wide_600": _case_600_wide, "on_the_near_plane": _case_on_the_near_plane, "viewport": _case_viewport,
                 "culled_clusters": _case_culled_clusters, "ties_far_apart": lambda: _case_ties("far_apart"), "ties_big_first": lambda: _case_ties("big_first"),
                 "ties_small_first": lambda: _case_ties("small_first"), "never_drawn": _case_never_drawn}
LATTICE_CASES.update({"blocks_h%d" % bh: functools.partial(_case_block_shapes, bh) for bh in BLOCK_HEIGHTS})
LATTICE_CASES.update({"boundary_%s%d" % (a, e): functools.partial(_case_path_boundary, a, e) for a in "xy" for e in (0, 1)})
LATTICE_CASES.update({"clusters_%d" % F: functools.partial(_case_clusters, F) for F in (1, 63, 64, 65, 257)})


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    """-> (the case, its arrays, the exact statement's index image and per-triangle info, the checker's keys), computed once"""
    m = LATTICE_CASES[name]()
    xyz, tris = m.arrays()
    index, info = px.lattice_raster(m.spec, m.w, m.h, Fraction(m.near).limit_denominator(1000), Fraction(m.far))
    keys = orc.project_raster(m.params(), xyz, tris, EYE)
    for a in (xyz, tris, keys):
        a.setflags(write=False)
    return m, xyz, tris, np.array(index, np.int64), info, keys


def key_index(keys):
    return np.where(keys == ALL1, px.NONE, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64))


def key_z(keys):
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


def expected_late(info):
    """what k_pa_raster must queue: the drawn triangles whose longest edge component exceeds 64 pixels and whose box holds a pixel centre"""
    return sum(1 for i in info if i is not None and i[0] > 16384 and i[1] > 0)


@pytest.mark.parametrize("name", sorted(LATTICE_CASES))
def test_checker_equals_the_exact_statement_on_the_lattice(name):
    m, xyz, tris, index, info, keys = lattice_case(name)
    assert np.array_equal(key_index(keys), index)
    assert (index != px.NONE).any()
    if m.late is not None:
        assert expected_late(info) == m.late


def test_lattice_cases_hold_what_they_are_for():
    """properties of the exact statement's own result that the cases were built to show"""
    m, _, _, index, info, _ = lattice_case("degenerate")
    for t, n in m.expect_cover.items():
        assert info[t][2] == n and info[t][1] > 0, t                     # a box with centres in it, of which the sliver covers none
    assert index[40, 50] == max(m.expect_cover)
    assert [info[t] for t in (2, 3, 4, 5)] == [None] * 4                 # zero area
    for name in ("diagonal_a", "diagonal_b"):                            # every centre of the two squares is owned once
        _, _, _, index, info, _ = lattice_case(name)
        assert sum(i[2] for i in info[:2]) == 256 == (index[10:26, 10:26] != px.NONE).sum() and sum(i[2] for i in info[2:4]) == 256
    a, b = lattice_case("diagonal_a")[3], lattice_case("diagonal_b")[3]
    assert np.array_equal(np.where(a[:, :90] >= 0, a[:, :90] ^ 1, a[:, :90]), b[:, :90])      # the owner does not depend on the storage order
    for name in ("ties_far_apart", "ties_big_first", "ties_small_first"):
        m, _, _, index, _, _ = lattice_case(name)
        x, y, t = m.expect_winner
        assert index[y, x] == t
    for bh in BLOCK_HEIGHTS:
        _, _, _, _, info, _ = lattice_case("blocks_h%d" % bh)
        assert [i[1] for i in info[::3]] == [bw * bh for bw in BLOCK_WIDTHS]
    for a in "xy":                                                       # the two sides of the path boundary: spans 16384 and 16385
        assert [lattice_case("boundary_%s%d" % (a, e))[4][0][0] for e in (0, 1)] == [16384, 16385]
        differ = np.argwhere(lattice_case("boundary_%s0" % a)[3] != lattice_case("boundary_%s1" % a)[3])
        assert len(np.unique(differ[:, 1 if a == "x" else 0])) <= 1
    _, _, _, index, info, _ = lattice_case("wide_600")
    assert len(np.unique(index[index >= 0])) == 600 and all(i[0] > 16384 for i in info)
    m, _, _, index, _, _ = lattice_case("on_the_near_plane")
    assert index[20, 30] == 2
    _, _, _, index, info, _ = lattice_case("viewport")
    assert index[0, 0] == len(info) - 1 and info[-2][2] == 0 and all(i[1] == 0 for i in info[8:14]) and all(i[2] > 0 for i in info[:8])


# ================================================================================================================ float cases
def _quad_mesh(quads):
    v, t = [], []
    for q in quads:
        t += [[len(v), len(v) + 1, len(v) + 2], [len(v), len(v) + 2, len(v) + 3]]
        v += list(q)
    return np.array(v, np.float32), np.array(t, np.uint32)


def _near_split_scene():
    """the last triangle of _near_plane_scene among neighbours of its own: exactly one queue entry"""
    v, t = _near_plane_scene()
    keep = np.r_[0:5, 6:11, 12:17, 29]
    return v[t[keep]].reshape(-1, 3), np.arange(3 * len(keep), dtype=np.uint32).reshape(-1, 3)


def _near_plane_scene():
    """identity pose, near plane at 0.1: among drawable neighbours, a triangle with one vertex behind (a quad: two halves), with two behind, with
    all three behind, with a vertex exactly on the plane, and one whose clipped quad has a half of at most 64 pixels and a half that is queued"""
    rng = np.random.default_rng(11)
    v, t = [], []

    def add(a, b, c):
        t.append([len(v), len(v) + 1, len(v) + 2])
        v.extend([a, b, c])

    def neighbours(n):
        for _ in range(n):
            c = np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.4, 0.4), rng.uniform(1.0, 3.0)])
            add(*(c + rng.normal(0, 0.08, (3, 3))))
    neighbours(5)
    add([-0.5, -0.2, 0.8], [-0.2, -0.25, 0.7], [-0.4, 0.1, -0.3])                  # one behind
    neighbours(5)
    add([0.3, -0.2, 0.9], [0.5, 0.1, -0.2], [0.1, 0.2, -0.4])                      # two behind
    neighbours(5)
    add([0.0, -0.1, -0.3], [0.2, 0.1, -0.2], [-0.2, 0.1, -0.05])                   # all behind
    neighbours(5)
    add([0.05, 0.02, np.float32(0.1)], [0.4, 0.3, 1.5], [-0.3, 0.35, 1.2])         # a vertex at z = depth_min: z_clip is within rounding of 0
    neighbours(5)
    add([0.15, 0.1, -0.1], [0.0, 0.0, 0.2], [0.3, 0.0, 4.0])                       # clipped: the half (P01, c1, c2) spans 32 pixels, (P01, c2, P20) 100
    neighbours(5)
    return np.array(v, np.float32), np.array(t, np.uint32)


def _huge_triangle_scene():
    """a triangle with vertices about 10^6 pixels away, around small ones"""
    rng = np.random.default_rng(12)
    v = [[-16000.0, -9000.0, 1.0], [17000.0, -8000.0, 1.1], [300.0, 15000.0, 0.9]]
    t = [[0, 1, 2]]
    for _ in range(20):
        c = np.array([rng.uniform(-0.9, 0.9), rng.uniform(-0.4, 0.4), rng.uniform(0.5, 0.8)])
        t.append([len(v), len(v) + 1, len(v) + 2])
        v.extend(c + rng.normal(0, 0.05, (3, 3)))
    return np.array(v, np.float32), np.array(t, np.uint32)


def _float_cases():
    room = tp.room_scene()
    floor = _quad_mesh([[[-60, -60, 0], [60, -60, 0], [60, 60, 0], [-60, 60, 0]]])
    small = project.default_params((128, 64), (128, 64), 64.0, 64.0)
    return {"room": (tp._params(), room[0], room[1], tp.room_poses()),
            "floor": (tp._params(), floor[0], floor[1], np.stack([tp._pose([0.0, 0.0, 0.12], 0.4, -0.05)])),
            "near_plane": (small, *_near_plane_scene(), EYE[None]),
            "near_split": (small, *_near_split_scene(), EYE[None]),
            "huge": (small, *_huge_triangle_scene(), EYE[None])}


# near_plane: both halves of the quad, the two-behind triangle and the larger half of the last one (spans of 186, 239, 264 and 96 pixels in float64
# against the threshold of 64; the halves that stay span 32 and 48)
FLOAT_LATE = {"near_plane": 4, "near_split": 1, "huge": 1}          # what the raster stage must report as queued, where the case is about that


@functools.lru_cache(maxsize=None)
def float_case(name):
    """-> (params, xyz, tris, poses, the checker's keys per pose, the float64 statement per pose), computed once"""
    P, xyz, tris, poses = _float_cases()[name]
    keys = np.stack([orc.project_raster(P, xyz, tris, T) for T in poses])
    st = [px.float_raster(xyz, tris, T, P.color_width, P.color_height, P.fx, P.fy, float(np.float32(P.depth_min)), float(np.float32(P.depth_max)),
                          EDGE_MARGIN, DEPTH_FLAT, DEPTH_SHIFT) for T in poses]
    keys.setflags(write=False)
    return P, xyz, tris, poses, keys, st


def check_against_float_statement(keys, st, P, who):
    """on sure pixels: the same coverage, the same triangle, z_ndc and camera z within the measured bound; at most UNSURE_CAP of the covered pixels
    unsure.  Returns the unsure fraction."""
    near, far = float(np.float32(P.depth_min)), float(np.float32(P.depth_max))
    A, B = far / (far - near), near * far / (far - near)
    drawn, sure = keys != ALL1, st["sure"]
    assert np.array_equal(drawn[sure], st["covered"][sure]), "%s: coverage on sure pixels" % who
    both = sure & drawn & st["covered"]
    assert np.array_equal(key_index(keys)[both], st["index"][both]), "%s: triangle on sure pixels" % who
    d = key_z(keys).astype(np.float64)
    err = np.abs(d[both] - st["z_ndc"][both])
    assert np.all(err <= st["bound"][both]), "%s: z_ndc off by %g times the bound" % (who, (err / st["bound"][both]).max())
    zc, lo, hi = B / (A - d[both]), st["z_ndc"][both] - st["bound"][both], st["z_ndc"][both] + st["bound"][both]
    assert np.all((zc >= B / (A - lo) * (1 - 1e-12)) & (zc <= B / (A - np.minimum(hi, 1.0)) * (1 + 1e-12))), "%s: camera z" % who   # z = B / (A - z_ndc), monotone
    covered = drawn | st["covered"]
    unsure = (covered & ~sure).sum() / max(1, covered.sum())
    assert covered.sum() > 100 and unsure <= UNSURE_CAP, "%s: %.4f of the covered pixels unsure" % (who, unsure)
    return unsure


@pytest.mark.parametrize("name", ["room", "floor", "near_plane", "near_split", "huge"])
def test_checker_agrees_with_the_float64_statement_on_sure_pixels(name):
    P, xyz, tris, poses, keys, st = float_case(name)
    for k in range(len(poses)):
        check_against_float_statement(keys[k], st[k], P, "checker, %s pose %d" % (name, k))


FLAT_SLOPE = 1e-4          # z_ndc per pixel: below it a surface counts as flat and its depth error as rounding


def measure_margins():
    """EDGE_MEASURED, DEPTH_FLAT_MEASURED and DEPTH_SHIFT_MEASURED: the checker against the float64 statement, one triangle at a time (no depth test
    between triangles is involved, so a disagreement about coverage is about an edge or about the far plane)"""
    worst = np.zeros(3)
    for name, (P, xyz, tris, poses) in _float_cases().items():
        case = np.zeros(3)
        near, far = float(np.float32(P.depth_min)), float(np.float32(P.depth_max))
        for T in poses:
            for t in tris:
                one = xyz[t]
                keys = orc.project_raster(P, one, [[0, 1, 2]], T)
                st = px.float_raster(one, [[0, 1, 2]], T, P.color_width, P.color_height, P.fx, P.fy, near, far, 0.0, 0.0, 0.0)
                drawn = keys != ALL1
                differ = drawn != st["covered"]
                at_far = differ & (st["far_gap"] < 1e-4)
                if at_far.any():
                    case[1] = max(case[1], st["far_gap"][at_far].max())
                if (differ & ~at_far).any():
                    case[0] = max(case[0], st["edge"][differ & ~at_far].max())
                both = drawn & st["covered"]
                err = np.abs(key_z(keys).astype(np.float64) - st["z_ndc"])
                flat = both & (st["slope"] < FLAT_SLOPE)
                if flat.any():
                    case[1] = max(case[1], err[flat].max())
                if (both & ~flat).any():
                    case[2] = max(case[2], (err / np.where(st["slope"] > 0, st["slope"], 1.0))[both & ~flat].max())
        print("%-12s edge %.6f pixel   depth: flat %.3e z_ndc, sloped %.6f pixel of shift" % (name, *case))
        worst = np.maximum(worst, case)
    print("EDGE_MEASURED = %.6f   DEPTH_FLAT_MEASURED = %.3e   DEPTH_SHIFT_MEASURED = %.6f" % tuple(worst))
    for name in _float_cases():
        P, xyz, tris, poses, keys, st = float_case(name)
        print(name, "unsure:", ["%.4f" % check_against_float_statement(keys[k], st[k], P, name) for k in range(len(poses))])


# ================================================================================================================ resolve cases
RESOLVE_SIZES = [(2, 2, 2, 2), (162, 121, 80, 60), (80, 60, 162, 121), (1296, 968, 640, 480)]
R_TRIS = np.arange(21, dtype=np.uint32).reshape(7, 3)[:, ::-1].copy()              # first vertices 2, 5, 8, ...
R_INST = (np.arange(21) * 7 % 250 + 1).astype(np.uint8)
R_LABEL = (np.arange(21) * 131 % 3000 + 1).astype(np.uint16)
R_LABEL[R_TRIS[5, 0]] = 0                                                          # a first vertex with label 0 (and an instance)
R_XYZ = np.random.default_rng(3).normal(0, 1, (21, 3)).astype(np.float32)


def _rha(v32):
    return np.floor(np.asarray(v32, np.float64) + 0.5).astype(np.int64)


@functools.lru_cache(maxsize=None)
def resolve_case(size):
    """Keys built by hand and a sensor depth image such that, per pixel, |drndr - dorig| sits at the bound - 1, at the bound, at the bound + 1 or far
    from it; with holes in the sensor depth, undrawn pixels, z_ndc bits of 0.0 and of 1.0, and a triangle whose first vertex has label 0."""
    w, h, dw, dh = size
    rng = np.random.default_rng(w + dw)
    near, far = float(np.float32(0.1)), 15.0
    A, B = far / (far - near), near * far / (far - near)
    dorig = rng.integers(1, 700, (dh, dw))
    delta = rng.choice([-1, 0, 1, 400, -150], (dh, dw))
    # the colour pixel a depth pixel's rendered depth is read at, and the millimetres it has to hold: 11 dorig + 200 + delta
    dx, sx = px.nearest_indices(w, dw)
    dy, sy = px.nearest_indices(h, dh)
    mm = rng.integers(300, 8000, (h, w))
    mm[np.ix_(sy, sx)] = (11 * dorig + 200 + delta)[np.ix_(dy, dx)]
    zc = (mm + 0.5) / 1000.0                                                       # half a millimetre clear of the truncation
    zbits = np.float32(A - B / zc).view(np.uint32).astype(np.uint64)
    special = rng.random((h, w))
    zbits[special < 0.02] = np.float32(0.0).view(np.uint32)                        # camera z 0, drndr 0
    zbits[(special >= 0.02) & (special < 0.04)] = np.float32(1.0).view(np.uint32)
    keys = (zbits << np.uint64(32)) | rng.integers(0, len(R_TRIS), (h, w)).astype(np.uint64)
    keys[(special >= 0.04) & (special < 0.08)] = ALL1
    depth = dorig.astype(np.uint16)
    depth[rng.random((dh, dw)) < 0.05] = 0
    if size == (2, 2, 2, 2):
        keys[0, 0], depth[0, 1] = ALL1, 0
    out = {}
    for flt in (0, 1):
        P = project.default_params((w, h), (dw, dh), 500.0, 500.0, filter_using_original_depth=flt)
        out[flt] = (P, orc.project_resolve(P, R_TRIS, R_INST, R_LABEL, keys, depth),
                    px.consistency(keys, R_TRIS[:, 0], R_INST, R_LABEL, depth, w, h, dw, dh, near, far, flt))
    P = project.default_params((w, h), (dw, dh), 500.0, 500.0)
    out[None] = (P, orc.project_resolve(P, R_TRIS, R_INST, R_LABEL, keys, None), px.consistency(keys, R_TRIS[:, 0], R_INST, R_LABEL, None, w, h, dw, dh, near, far, 0))
    keys.setflags(write=False)
    depth.setflags(write=False)
    return keys, depth, out


@pytest.mark.parametrize("size", RESOLVE_SIZES, ids=lambda s: "%dx%d_%dx%d" % s)
def test_checker_equals_the_exact_consistency_filter(size):
    keys, depth, out = resolve_case(size)
    w, h, dw, dh = size
    for flt in (0, 1, None):
        P, (ci, cl, cz), (si, sl, undecided, sz) = out[flt]
        ok = ~undecided
        assert np.array_equal(ci[ok], si[ok]) and np.array_equal(cl[ok], sl[ok]), flt
        assert np.array_equal(cz == 0, sz == 0) and np.allclose(cz, sz, rtol=1e-4, atol=0)
    if w > 2:
        # the case holds what it is for: pixels one millimetre either side of the bound and at it, holes, both outcomes
        _, sy = px.nearest_indices(h, dh)
        _, sx = px.nearest_indices(w, dw)
        dyi, dxi = px.nearest_indices(h, dh)[0], px.nearest_indices(w, dw)[0]
        drndr = np.floor(out[0][2][3] * 1000.0).astype(np.int64)[np.ix_(sy, sx)]
        dor = depth.astype(np.int64)[np.ix_(dyi, dxi)]
        live = (out[None][1][1] != 0) & (drndr != 0) & (dor != 0)
        off = np.abs(drndr - dor) - (200 + 10 * dor)
        for k in (-1, 0, 1):
            assert (live & (off == k)).sum() > 0.05 * live.sum(), k
        assert out[0][2][2].sum() > 0.05 * live.sum() and not (out[0][2][2] & (off != 0)).any()       # undecided = exact equality only
        removed0, removed1 = (out[None][1][1] != 0) & (out[0][1][1] == 0), (out[None][1][1] != 0) & (out[1][1][1] == 0)
        assert removed0.any() and (removed1 & ~removed0).any() and (out[0][1][1] != 0).any()
        assert ((out[None][1][1] == 0) & (out[None][1][0] != 0)).any()                                # label 0 with an instance passes through


# ================================================================================================================ vote cases
VOTE_SIZES = [(2, 2), (5, 5), (63, 7), (64, 8), (65, 9), (129, 17), (161, 121)]
PLANT = 9000


@functools.lru_cache(maxsize=None)
def vote_case(size):
    """-> list of (instance, label, checker's result, statement's result): random labels from four values plus 0 at two densities; for the wider
    sizes a third image with counts planted by hand along the top border"""
    w, h = size
    rng = np.random.default_rng(1000 * w + h)
    images = []
    for probs in ([0.2] * 5, [0.4, 0.3, 0.15, 0.1, 0.05]):
        label = rng.choice(np.array([0, 17, 300, 4000, 65535], np.uint16), (h, w), p=probs)
        images.append(label)
    if w >= 63:
        label = images[0].copy()
        label[:5] = 0
        for x, y in [(0, 0),                                     # 1 in 9: goes
                     (w - 1, 0), (w - 2, 1),                     # 2 in 9 at the corner: stays
                     (10, 0), (9, 1), (11, 2),                   # 3 in 15
                     (20, 1), (18, 0), (22, 0), (19, 3),         # 4 in 20
                     (30, 2), (28, 0), (32, 1), (29, 3), (31, 4),   # 5 in 25
                     (40, 0), (41, 2),                           # 2 in 15: goes
                     (50, 2), (48, 0), (52, 1), (49, 4)]:        # 4 in 25: goes
            label[y, x] = PLANT
        images.append(label)
    out = []
    for label in images:
        inst = rng.integers(1, 256, (h, w)).astype(np.uint8)     # instances differ between pixels that share a label
        inst.setflags(write=False)
        label.setflags(write=False)
        out.append((inst, label, orc.project_vote(inst, label), px.vote(inst, label)))
    return out


def _check_plants(label_out, w):
    assert label_out[0, 0] == 0 and label_out[0, w - 1] == PLANT and label_out[0, 10] == PLANT and label_out[1, 20] == PLANT and label_out[2, 30] == PLANT
    assert label_out[0, 40] == 0 and label_out[2, 50] == 0


def _vote_checker_against_statement(size):
    """-> the (window total, kept) pairs seen among the labelled pixels of the size's images"""
    w, h = size
    seen = set()
    for inst, label, (ci, cl), (si, sl, count, total) in vote_case(size):
        assert np.array_equal(ci, si) and np.array_equal(cl, sl)
        assert np.array_equal(si[sl != 0], inst[sl != 0])
        voted = label != 0
        seen |= {(int(t), bool(k)) for t, k in zip(total[voted], (sl != 0)[voted])}
    if w >= 63:
        _check_plants(vote_case(size)[2][3][1], w)
    assert {t for t, _ in seen} == set(np.unique(total).tolist())                 # a labelled pixel in every window class the size has
    if w >= 63:
        assert {t for t, _ in seen} == {9, 12, 15, 16, 20, 25}
    return seen


@pytest.mark.parametrize("size", VOTE_SIZES, ids=lambda s: "%dx%d" % s)
def test_checker_equals_the_exact_vote(size):
    _vote_checker_against_statement(size)


def test_vote_cases_put_every_window_class_on_both_sides_of_the_bound():
    seen = set()
    for size in VOTE_SIZES:
        seen |= _vote_checker_against_statement(size)
    assert seen >= {(t, k) for t in (9, 12, 15, 16, 20, 25) for k in (False, True)}


# ================================================================================================================ the device
def _projector(P, xyz, tris, inst=None, label=None):
    pr = project.Projector(P)
    pr.set_mesh(xyz, tris, np.ones(len(xyz), np.uint8) if inst is None else inst, np.ones(len(xyz), np.uint16) if label is None else label)
    return pr


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LATTICE_CASES))
def test_gpu_raster_on_the_lattice(name):
    m, xyz, tris, index, info, want = lattice_case(name)
    with _projector(m.params(), xyz, tris) as pr:
        keys, late = pr.stage_raster(EYE[None])
    print(name, "late_counts", late, "covered", (keys != ALL1).sum())
    assert np.array_equal(key_index(keys[0]), index), "against the exact statement"
    assert np.array_equal(keys[0], want), "against the checker, bit for bit"
    assert late[0] == expected_late(info)
    if m.late is not None:
        assert late[0] == m.late


@pytest.mark.gpu
@pytest.mark.parametrize("axis", ["x", "y"])
def test_gpu_raster_path_boundary_changes_one_line_at_most(axis):
    """the same triangle through the 32-bit path (span 16384) and through the queue (16385): the keys differ in the last column / row only"""
    got = []
    for e in (0, 1):
        m, xyz, tris, index, info, want = lattice_case("boundary_%s%d" % (axis, e))
        with _projector(m.params(), xyz, tris) as pr:
            keys, late = pr.stage_raster(EYE[None])
        assert late[0] == e and np.array_equal(keys[0], want)
        got.append(keys[0])
    differ = np.argwhere(got[0] != got[1])
    assert len(np.unique(differ[:, 1 if axis == "x" else 0])) <= 1
    assert (got[0] != ALL1).sum() > 500


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["room", "floor", "near_plane", "near_split", "huge"])
def test_gpu_raster_general_poses(name):
    P, xyz, tris, poses, want, st = float_case(name)
    with _projector(P, xyz, tris) as pr:
        keys, late = pr.stage_raster(poses)
    print(name, "late_counts", late)
    for k in range(len(poses)):
        assert np.array_equal(keys[k], want[k]), "against the checker, pose %d" % k
        check_against_float_statement(keys[k], st[k], P, "device, %s pose %d" % (name, k))
    if name in FLOAT_LATE:
        assert late[0] == FLOAT_LATE[name]
    if name == "floor":
        assert late[0] >= 1


@pytest.mark.gpu
def test_gpu_raster_batch_with_invalid_frames():
    P = project.default_params((128, 64), (128, 64), 64.0, 64.0)
    xyz, tris, _, _ = tp.room_scene(4)
    base = tp.room_poses()
    poses = np.stack([base[0], base[1], base[2], base[3], base[4], base[5], tp._pose([2.0, 2.0, 1.0], 2.5), tp._pose([4.0, 1.0, 2.0], 1.9, -0.5)])
    valid = [1, 0, 1, 1, 0, 1, 1, 1]
    batch = np.where(np.array(valid, bool)[:, None, None], poses, np.float32(-np.inf)).astype(np.float32)
    with _projector(P, xyz, tris) as pr:
        keys, late = pr.stage_raster(batch)
        for k in range(8):
            if not valid[k]:
                assert np.all(keys[k] == ALL1) and late[k] == 0
                continue
            one, late1 = pr.stage_raster(poses[k:k + 1])
            assert np.array_equal(one[0], keys[k]) and late1[0] == late[k]
            assert np.array_equal(keys[k], orc.project_raster(P, xyz, tris, poses[k])) and (keys[k] != ALL1).mean() > 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("size", RESOLVE_SIZES, ids=lambda s: "%dx%d_%dx%d" % s)
def test_gpu_resolve(size):
    keys, depth, out = resolve_case(size)
    for flt in (0, 1, None):
        P, (ci, cl, cz), (si, sl, undecided, _) = out[flt]
        with _projector(P, R_XYZ, R_TRIS, R_INST, R_LABEL) as pr:
            d = None if flt is None else depth[None]
            gi, gl, gz = pr.stage_resolve(keys[None], d)
            assert np.array_equal(gi[0], ci) and np.array_equal(gl[0], cl) and np.array_equal(gz[0].view(np.uint32), cz.view(np.uint32)), flt
            assert np.array_equal(gi[0][~undecided], si[~undecided]) and np.array_equal(gl[0][~undecided], sl[~undecided])
            ni, nl, nz = pr.stage_resolve(keys[None], d, want_depth=False)           # zcam_out NULL
            assert nz is None and np.array_equal(ni, gi) and np.array_equal(nl, gl)
            if flt == 0 and size[0] <= 162:                                          # two frames: the second with every pixel undrawn
                k2, d2 = np.stack([keys, np.full_like(keys, ALL1)]), np.stack([depth, depth])
                bi, bl, bz = pr.stage_resolve(k2, d2)
                assert np.array_equal(bi[0], ci) and np.array_equal(bl[0], cl) and not bi[1].any() and not bl[1].any() and not bz[1].any()
                bad = keys.copy()
                bad[-1, -1] = np.uint64(len(R_TRIS))                                 # a triangle the mesh does not have: refused, not launched
                with pytest.raises(Exception):
                    pr.stage_resolve(bad[None], d)


@pytest.mark.gpu
@pytest.mark.parametrize("size", VOTE_SIZES, ids=lambda s: "%dx%d" % s)
def test_gpu_vote(size):
    w, h = size
    cases = vote_case(size)
    with project.Projector(project.default_params((w, h), (w, h), 64.0, 64.0)) as pr:
        for inst, label, (ci, cl), (si, sl, _, _) in cases:
            gi, gl = pr.stage_vote(inst[None], label[None])
            assert np.array_equal(gi[0], ci) and np.array_equal(gl[0], cl), "against the checker"
            assert np.array_equal(gi[0], si) and np.array_equal(gl[0], sl), "against the exact statement"
        if w >= 63:
            _check_plants(gl[0], w)
        # a batch: each frame voted on its own
        n = len(cases)
        bi, bl = pr.stage_vote(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
        for k in range(n):
            assert np.array_equal(bi[k], cases[k][2][0]) and np.array_equal(bl[k], cases[k][2][1])


@pytest.mark.gpu
def test_gpu_stages_compose_to_the_product_path():
    """run() = raster, resolve, vote: the hooks launch the product path's own helpers"""
    P = tp._params()
    xyz, tris, inst, label = tp.room_scene()
    poses = tp.room_poses()[:3]
    depth = tp.sensor_depth(P, xyz, tris, inst, label, poses)
    with _projector(P, xyz, tris, inst, label) as pr:
        ri, rl, rz, _ = pr.run(poses, depth, want_depth=True)
        keys, _ = pr.stage_raster(poses)
        i1, l1, z1 = pr.stage_resolve(keys, depth)
        i2, l2 = pr.stage_vote(i1, l1)
    assert np.array_equal(ri, i2) and np.array_equal(rl, l2) and np.array_equal(rz, z1)
    for k in range(3):
        ci, cl, cz = orc.project_resolve(P, tris, inst, label, keys[k], depth[k])
        assert np.array_equal(i1[k], ci) and np.array_equal(l1[k], cl) and np.array_equal(z1[k], cz)


if __name__ == "__main__":
    measure_margins()
