"""The calibrate stage, kernel by kernel (scannet_amd/csrc/calibrate.hip; Calibrate/src/calibration.h:253-307, shaders/aligner.hlsl).

Three parties:
  * the HIP kernels through the stage hooks of include/scanfuse_internal.h (Calibrator.stage_undistort_rgb / stage_prepare / stage_raster /
    stage_finalize), which launch them through the helpers sf_calibrator_run_device itself uses;
  * the checker oracle/calib_oracle.c, split the same way (or_calib_undistort_rgb, or_calib_stage_prepare / _raster / _finalize), which the kernels
    are held to bit for bit;
  * tests/calibrate_exact.py, an independent statement in real arithmetic: exact where binary32 is exact (dyadic calibrations, vertex positions in
    1/512 pixel with one dyadic z per quad, constant power-of-two tables at dyadic cell coordinates), and elsewhere exact up to pixels it calls
    unsure: closer to a rounding tie than binary32 evaluation can move them.

CPU part: the checker against the statement on every case the GPU part uses.  GPU part (-m gpu): every case through the hooks against the checker's
stage bit for bit, the exact cases against the statement too.

Found while writing this: a table whose resolution does not divide the image (5 x 4 x 3 on 37 x 29; the (width / 2)-wide table calibrate_depth
writes for an odd width) gave a cell coordinate equal to the resolution, and the trilinear read, which clamps only the upper neighbour, read one cell
past the row -- past the table on its last row.  Kernel and checker shared it.  Both now take the rule calibrate_depth's apply mode states (lut_cell,
lut_value.h), and sf_calibrator_create refuses an in-memory table whose max_dist is not a positive finite number.  The non-dividing cases of
test_prepare / test_gpu_prepare hold only with that rule: the parent's coordinate, 36 / 7 = 5.14 of 5 columns, is outside what the statement's table
read defines.

One-line mutations of calibrate.hip (values and predicates only, never an address or a bound) tried on a scratch copy, each with the GPU tests here
that failed under it:
  * the `e0 == 0 && !tl0` exclusion dropped in raster_tri: test_gpu_raster[40x30];
  * `(int)(d * P.shift)` instead of round_i in k_finalize: test_gpu_finalize, all nine cases;
  * `d0 < DEPTH_WORLD_MIN` for `<=` in k_raster_quads: test_gpu_raster[40x30];
  * the winding swap of z1 / z2 omitted: test_gpu_raster[40x30], [17x16], [9x2];
  * `p[0] == 0` alone as the black test: test_gpu_finalize[larger_53x41], [equal_37x29], [smaller_20x15], [tiny_2x2], [large_shift], [shift_1024];
  * `px[10]` for `px[11]` in the packed store of k_undistort_rgb: test_gpu_undistort_rgb, every case;
  * `px[k % 9]` in its byte store: test_gpu_undistort_rgb[general-53x41-n4], [general-54x41-n4], [general-51x41-n4], [general-53x41-n16] -- the frames
    of a batch that start off a 4-byte boundary;
  * `px[k % 3]` in its byte store: the same four and [identity-54x41-n1], [identity-51x41-n1], the tail lane of an aligned frame.  The identity cases
    were added for this one: under the pincushion cases the last pixels of a frame sample outside and are black, and no test saw it.
  * `i0 + 4 < n` for `<=` in the packed store's condition changes no byte (the byte store writes the same values), so nothing can catch it."""
import ctypes as C
import functools
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import oracle as orc
from scannet_amd import calibrate
from tests import calibrate_exact as cx

ONE = np.float32(1.0).view(np.uint32)
f32 = np.float32

# The statement against the checker, measured on the CPU over every case below (python -m tests.test_calibrate_stages prints the figures); nothing here
# comes from device output.  A margin is the larger of 4 x what was measured and what the number format allows (*_ROUNDING: a bound, not an estimate):
#   SAMPLE_*   the distance (pixels) of a sample location from a half-integer.  MEASURED: the largest such distance among the pixels where checker and
#              statement round differently.  ROUNDING: the location is a chain of about twelve binary32 operations on magnitudes up to the image width
#              (64) amplified by the radial factor (< 2): 12 x 128 x 2^-24
#   LOOKUP_*   the same for the colour look-up position of k_finalize: two operations on magnitudes up to 52
#   RESULT_*   the distance (counts) of depth x shift from a rounding tie in finalize, relative to the value: three operations
#   NDC_*      the distance of fx, fy, fz from the bound of the validity test: about twenty operations on magnitudes up to 4
#   POS_*      the mesh vertex's target position and z against the exact ones, relative to max(1, |value|)
#   QUOTIENT   corrected depth: the exact quotient's distance (counts) from a whole number below which the truncating conversion may give either
#              neighbour: eight operations on magnitudes up to 65 536; not measured, the conversion itself is held to +-1 count there
SAMPLE_MEASURED = 0.0               # no pixel of any case rounds differently
SAMPLE_ROUNDING = 12 * 128 * 2.0 ** -24
LOOKUP_MEASURED = 0.0               # none differs outside the one tie column
LOOKUP_ROUNDING = 2 * 52 * 2.0 ** -24
RESULT_MEASURED = 6.3e-08           # equal_37x29; of the value
RESULT_ROUNDING = 3 * 2.0 ** -24
NDC_ROUNDING = 20 * 4 * 2.0 ** -24
POS_MEASURED = 8.41e-06             # random-40x30-t8x6x4
SAMPLE_MARGIN = max(4 * SAMPLE_MEASURED, SAMPLE_ROUNDING)
LOOKUP_MARGIN = max(4 * LOOKUP_MEASURED, LOOKUP_ROUNDING)
RESULT_MARGIN = max(4 * RESULT_MEASURED, RESULT_ROUNDING)
NDC_MARGIN = NDC_ROUNDING
POS_TOL = 4 * POS_MEASURED
QUOTIENT = 8 * 65536 * 2.0 ** -24
# the draw's z where binary32 interpolation is not exact: three conversions, three products, two sums of non-negative terms, the area's conversion and
# one division, each within 2^-24 relative
Z_REL = 10 * 2.0 ** -24
UNSURE_CAP = 0.03


def _params(cwh, dwh, Kc, Kd, E=None, cdist=(0,) * 5, ddist=(0,) * 5):
    return calibrate.make_params(cwh, dwh, Kc, Kd, E, color_dist=cdist, depth_dist=ddist)


def _translation(tx=0.0, ty=0.0, tz=0.0):
    e = np.eye(4, dtype=np.float32)
    e[0, 3], e[1, 3], e[2, 3] = tx, ty, tz
    return e


# ================================================================================================================ undistort_rgb
class UndCase:
    def __init__(self, name, cw, ch, K, c, n, named=()):
        self.name, self.cw, self.ch, self.K, self.c, self.n, self.named = name, cw, ch, K, c, n, named
        self.params = _params((cw, ch), (8, 8), K, (8.0, 8.0, 4.0, 4.0), cdist=c)

    @functools.cached_property
    def frames(self):
        rng = np.random.default_rng(self.cw * 1000 + self.ch + self.n)
        return rng.integers(1, 256, (self.n, self.ch, self.cw, 3), dtype=np.uint8)      # never black: a black output pixel sampled outside

    @functools.cached_property
    def checker(self):
        cb = orc.calib_from(self.params)
        return np.stack([orc.calib_undistort_rgb(cb, f) for f in self.frames])


@functools.lru_cache(None)
def _locations(K, c, w, h):
    return cx.sample_locations(K, c, w, h)


def _und_cases():
    out = []
    for cw, ch in ((52, 41), (53, 41), (54, 41), (51, 41), (64, 16), (64, 48)):      # pixel counts mod 4 = 0, 1, 2, 3; 1024 and 3072 pixels
        K = (60.0, 61.0, (cw - 1) / 2 + 0.3, (ch - 1) / 2 - 0.2)
        c = (0.42, -0.08, 0.004, -0.003, 0.02)      # pincushion: the border samples outside on every side
        for n in (1, 4):
            out.append(UndCase("general-%dx%d-n%d" % (cw, ch, n), cw, ch, K, c, n))
    for cw, ch in ((52, 41), (53, 41), (54, 41), (51, 41)):      # no distortion: the LAST pixels of the frame, the tail lane's, are not black
        out.append(UndCase("identity-%dx%d-n1" % (cw, ch), cw, ch, (60.0, 61.0, (cw - 1) / 2 + 0.3, (ch - 1) / 2 - 0.2), (0.0,) * 5, 1))
    out.append(UndCase("general-53x41-n16", 53, 41, (60.0, 61.0, 26.3, 19.8), (0.42, -0.08, 0.004, -0.003, 0.02), 16))
    # binary32 is exact here: fx = fy = 64, k1 = 1/16, a pixel 32 columns (rows) from the principal point on its row (column): n = 1/2, r^2 = 1/4,
    # radial = 1 + 1/64, location = principal point +- 32.5.  named = (x, y, sx, sy)
    k = (0.0625, 0.0, 0.0, 0.0, 0.0)
    out.append(UndCase("exact-plus_half", 64, 48, (64.0, 64.0, 16.0, 8.0), k, 4, ((48, 8, 49, 8), (16, 40, 16, 41))))
    out.append(UndCase("exact-minus_half", 64, 48, (64.0, 64.0, 32.0, 32.0), k, 4, ((0, 32, 0, 32), (32, 0, 32, 0))))
    out.append(UndCase("exact-below_minus_half", 64, 48, (64.0, 64.0, 32.0, 32.0), (0.0625 + 2.0 ** -10, 0.0, 0.0, 0.0, 0.0), 1, ((0, 32, -1, 32), (32, 0, 32, -1))))
    out.append(UndCase("exact-at_the_size", 64, 48, (64.0, 64.0, 31.0, 15.0), k, 1, ((63, 15, 64, 15), (31, 47, 31, 48))))
    out.append(UndCase("exact-64x16", 64, 16, (64.0, 64.0, 31.0, 8.0), k, 4, ((63, 8, 64, 8),)))
    return out


UND_CASES = _und_cases()


def _check_undistort(case, got, against_statement):
    assert got.shape == case.frames.shape
    if not against_statement:
        for j in range(case.n):              # every frame whole: a store that reaches into its neighbour shows in the neighbour
            assert np.array_equal(got[j], case.checker[j]), "%s frame %d: %d bytes differ" % (case.name, j, (got[j] != case.checker[j]).sum())
        return None
    sx, sy, dist = _locations(case.K, case.c, case.cw, case.ch)
    sure = dist > SAMPLE_MARGIN
    for x, y, nx, ny in case.named:          # decided by the statement's exact arithmetic, ties included
        assert (sx[y, x], sy[y, x]) == (nx, ny), (case.name, x, y, sx[y, x], sy[y, x])
        sure[y, x] = True
    unsure = 1.0 - sure.mean()
    assert unsure <= UNSURE_CAP, (case.name, unsure)
    for j in range(case.n):
        want = cx.gather(case.frames[j], sx, sy, 0)
        assert np.array_equal(got[j][sure], want[sure]), "%s frame %d" % (case.name, j)
    return unsure, sx, sy, dist


@pytest.mark.parametrize("case", UND_CASES, ids=lambda c: c.name)
def test_undistort_rgb(case):
    unsure, sx, sy, dist = _check_undistort(case, case.checker, True)
    if case.name.startswith("general"):      # the distortion reaches one pixel outside on every side
        assert (sx == -1).any() and (sx == case.cw).any() and (sy == -1).any() and (sy == case.ch).any()
    for x, y, nx, ny in case.named:
        if "below" not in case.name:
            assert dist[y, x] == 0.0           # an exact tie


# ================================================================================================================ prepare
class PrepCase:
    def __init__(self, name, dwh, cwh=(53, 41), Kd=(40.0, 41.0, 18.0, 14.0), Kc=(60.0, 61.0, 26.0, 20.0), E=None, ddist=(0,) * 5, grid=None, maxd=0.0,
                 shift=1000.0, frames=None, table_exact=False, named_ok=()):
        self.name, self.w, self.h, self.cw, self.ch = name, dwh[0], dwh[1], cwh[0], cwh[1]
        self.Kd, self.Kc, self.ddist, self.grid, self.maxd, self.shift = Kd, Kc, ddist, grid, maxd, shift
        self.E = np.eye(4, dtype=np.float32) if E is None else np.asarray(E, np.float32)
        self.table_exact, self.named_ok = table_exact, named_ok      # named_ok = (x, y, valid): vertices sitting ON a bound of the validity test
        self.ndc_exact = name in ("ndc-on_the_bounds", "ndc-just_above", "ndc-just_below")      # every operation up to the bound is exact in binary32 wherever a vertex comes near one: no vertex is unsure
        self.params = _params(cwh, dwh, Kc, Kd, self.E, ddist=ddist)
        self.frames = np.ascontiguousarray(frames, np.uint16)

    @functools.cached_property
    def checker(self):
        cb = orc.calib_from(self.params)
        r = [orc.calib_stage_prepare(cb, f, self.grid, self.maxd, self.shift) for f in self.frames]
        return tuple(np.stack([q[k] for q in r]) for k in range(3))


def _depth_frame(w, h, seed, maxd, shift):
    """0, 1, at and beyond the table's range, 65535, and everything between"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    d[::3] = rng.integers(300, 9000, d[::3].shape)
    at = int(round(maxd * shift)) if maxd else 4000
    special = [0, 1, 2, min(at, 65535), min(at + 1, 65535), max(at - 1, 0), 65535, 65534, 32768, 32767]
    d.ravel()[rng.choice(w * h, 5 * len(special), replace=False)] = np.repeat(special, 5)
    d[0, 0], d[-1, -1], d[0, -1], d[-1, 0] = 65535, 2000, 0, 1
    return d


def _prep_cases():
    rng = np.random.default_rng(77)
    out = []
    mild = (-0.05, 0.01, 0.001, -0.0007, 0.0)
    rot = [[0.99998, 0.006, -0.002, -0.037], [-0.006, 0.99997, 0.004, 0.003], [0.002, -0.004, 0.99999, -0.021], [0, 0, 0, 1]]
    tables = {(37, 29): [(5, 4, 3), (18, 14, 2), (1, 1, 1)], (40, 30): [(5, 4, 3), (8, 6, 4), (1, 1, 1), (40, 30, 2), (18, 14, 2)]}
    for (w, h), shapes in tables.items():
        for k, (lx, ly, lz) in enumerate(shapes):
            grid = (1.0 + 0.15 * rng.standard_normal((lz, ly, lx))).clip(0.6, 1.5).astype(np.float32)
            out.append(PrepCase("random-%dx%d-t%dx%dx%d" % (w, h, lx, ly, lz), (w, h), ddist=mild, E=rot if k % 2 else _translation(-0.037, 0.003, -0.021),
                                grid=grid, maxd=4.5, frames=[_depth_frame(w, h, 10 * k + s, 4.5, 1000.0) for s in range(2)]))
    # binary32 is exact: bins of 1 or 2 pixels (cell coordinates are multiples of 1/2), depth = raw / 1024, slice coordinate = raw / 2048 capped,
    # a table of one power of two: the eight products and their sum are exact, the value is the constant, the result is trunc(raw / constant)
    for (w, h), (lx, ly, lz) in (((37, 29), (18, 14, 2)), ((40, 30), (40, 30, 2))):
        for value in (1.0, 0.5, 2.0, 0.0, -1.0):
            out.append(PrepCase("constant_%g-%dx%d-t%dx%dx%d" % (value, w, h, lx, ly, lz), (w, h), grid=np.full((lz, ly, lx), value, np.float32), maxd=4.0,
                                shift=1024.0, frames=[_depth_frame(w, h, 5, 4.0, 1024.0)], table_exact=True))
    # linear in the x index, read at multiples of 1/2: the value 1 + x / 16 is exact, the quotient is not
    lin = np.broadcast_to(1.0 + np.arange(18, dtype=np.float32) / 8.0, (2, 14, 18))
    out.append(PrepCase("linear-37x29-t18x14x2", (37, 29), grid=np.ascontiguousarray(lin), maxd=4.0, shift=1024.0, frames=[_depth_frame(37, 29, 6, 4.0, 1024.0)]))
    out.append(PrepCase("no_table-37x29", (37, 29), ddist=mild, E=rot, frames=[_depth_frame(37, 29, 7, 0, 1000.0)]))
    out.append(PrepCase("no_table-40x30-shift5000", (40, 30), ddist=mild, shift=5000.0, frames=[_depth_frame(40, 30, 8, 0, 5000.0)]))
    # the validity test AT its bounds, where binary32 is exact: depth 2 (raw 2048 / 1024), depth camera f = 64 at (18, 14), colour camera f = 128 at
    # (36, 28): ux = 2 (x - 18) + 36, uy = 2 (y - 14) + 28, so fx = -1 at x = 0, +1 at x = 26 (ux = 52 = cw - 1), fy = +1 at y = 0, -1 at y = 20.
    # A translation of +-2^-24 moves ux, uy by 2^-18: one unit in the last place of 52 or 40, and off the bound on one side.
    flat = np.full((1, 29, 37), 2048, np.uint16)
    on = dict(dwh=(37, 29), Kd=(64.0, 64.0, 18.0, 14.0), Kc=(128.0, 128.0, 36.0, 28.0), shift=1024.0, frames=flat)
    t = 2.0 ** -24
    out.append(PrepCase("ndc-on_the_bounds", named_ok=((0, 5, True), (26, 5, True), (5, 0, True), (5, 20, True), (0, 0, True), (26, 20, True), (27, 5, False), (5, 21, False)), **on))
    out.append(PrepCase("ndc-just_above", E=_translation(t, t), named_ok=((0, 5, True), (26, 5, False), (5, 0, True), (5, 20, False)), **on))
    out.append(PrepCase("ndc-just_below", E=_translation(-t, -t), named_ok=((0, 5, False), (26, 5, True), (5, 0, False), (5, 20, True)), **on))
    # fz: raw 100 / 1000 is 0.1f and raw 10000 / 1000 is 10, so fz is exactly 0 and 1; a translation of one unit in the last place puts it outside
    fr = np.full((1, 29, 37), 2000, np.uint16)
    fr[0, 10, 12], fr[0, 12, 20], fr[0, 3, 3] = 100, 10000, 0
    z = dict(dwh=(37, 29), frames=fr)         # the projected z is the depth plus the translation whatever the intrinsics are
    out.append(PrepCase("ndc-depth_range", named_ok=((12, 10, True), (20, 12, True), (3, 3, False)), **z))
    out.append(PrepCase("ndc-depth_range_above", E=_translation(tz=2.0 ** -20), named_ok=((12, 10, True), (20, 12, False)), **z))
    out.append(PrepCase("ndc-depth_range_below", E=_translation(tz=-2.0 ** -27), named_ok=((12, 10, False), (20, 12, True)), **z))
    out.append(PrepCase("ndc-qz_zero", E=_translation(tz=-2.0), named_ok=(), **z))       # raw 2000: wz = 2 - 2
    return out


PREP_CASES = _prep_cases()


def _check_prepare(case, got, against_statement, stats=None):
    und, vert, zbuf = got
    n, h, w = case.frames.shape
    assert und.shape == (n, h, w) and vert.shape == (n, h, w, 4) and zbuf.shape == (n, h, w)
    if not against_statement:
        for k, name in enumerate(("depth", "vertices", "depth buffer")):
            a, b = got[k], case.checker[k]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s %s: %d words differ" % (case.name, name, (a.view(np.uint32) != b.view(np.uint32)).sum())
        return
    assert (zbuf == ONE).all()
    sx, sy, dist = _locations(case.Kd, tuple(case.ddist), w, h)
    sure = dist > SAMPLE_MARGIN
    assert 1.0 - sure.mean() <= UNSURE_CAP, case.name
    shift = f32(case.shift)
    unsure_vertices = 0
    for j in range(n):
        raw = case.frames[j]
        for y in range(h):
            for x in range(w):
                d = und[j, y, x]
                if sure[y, x]:
                    i, k = int(sx[y, x]), int(sy[y, x])
                    if not (0 <= i < w and 0 <= k < h):
                        assert d == 0.0
                    elif case.grid is None:
                        assert d == f32(raw[k, i]) / shift
                    else:
                        u, off = cx.corrected_depth(case.grid, case.maxd, case.shift, w, h, i, k, int(raw[k, i]))
                        if case.table_exact or off > QUOTIENT:
                            assert d == f32(u) / shift, (case.name, x, y, int(raw[k, i]), u, float(d) * case.shift)
                        else:           # the truncating conversion: either neighbour
                            assert d in (f32(max(u - 1, 0)) / shift, f32(u) / shift, f32(min(u + 1, 65535)) / shift), (case.name, x, y)
                # the vertex of the depth the checker holds here
                v = cx.vertex(d, x, y, w, h, case.cw, case.ch, case.Kd, case.Kc, case.E.ravel())
                g = vert[j, y, x]
                if v is None:
                    assert g[3] == 0.0, (case.name, x, y)      # qz = 0 is below the near bound whatever the position comes to
                    continue
                px_, py_, z_, ok, slack = v
                if slack > NDC_MARGIN or case.ndc_exact:
                    assert (g[3] != 0.0) == ok, (case.name, x, y, float(slack))
                else:
                    unsure_vertices += 1
                for a, b in ((g[0], px_), (g[1], py_), (g[2], z_)):
                    err = abs(F(float(a)) - b) / max(1, abs(b))
                    if stats is not None:
                        stats["pos"] = max(stats.get("pos", (0.0, "")), (float(err), case.name))
                    assert err <= POS_TOL, (case.name, x, y, float(a), float(b))
        for x, y, ok in case.named_ok:
            assert (vert[j, y, x, 3] != 0.0) == ok, (case.name, x, y)
            v = cx.vertex(und[j, y, x], x, y, w, h, case.cw, case.ch, case.Kd, case.Kc, case.E.ravel())
            assert v is None or v[3] == ok, (case.name, x, y)
    if stats is not None:
        stats["vert_unsure"] = max(stats.get("vert_unsure", (0.0, "")), (unsure_vertices / (n * w * h), case.name))
    assert unsure_vertices <= UNSURE_CAP * n * w * h, (case.name, unsure_vertices)


@pytest.mark.parametrize("case", PREP_CASES, ids=lambda c: c.name)
def test_prepare(case):
    _check_prepare(case, case.checker, True)


# ================================================================================================================ the draw
class Grid:
    """One frame of the raster stage built by hand: quads live in 2 x 2 vertex groups -- group (a, b) holds vertices (2a .. 2a + 1, 2b .. 2b + 1) --
    and the quads BETWEEN groups are switched off by the depth image: a group's four depths are 1 or 2 by the parity of a + b (a spread the
    discontinuity test rejects), an unused vertex has depth 0."""

    def __init__(self, w, h, name=""):
        self.w, self.h, self.name = w, h, name
        self.und = np.zeros((h, w), np.float32)
        self.pos = [[(512 * x, 512 * y) for x in range(w)] for y in range(h)]
        self.z = np.full((h, w), 0.5, np.float32)
        self.ok = np.ones((h, w), bool)
        self.init = np.ones((h, w), np.float32)
        self.used = set()

    def quad(self, tl, bl, tr, br, z, depth=None, group=None):
        """corner positions in pixels (multiples of 1/512, or None: not a number) of the vertex records at (x, y), (x, y + 1), (x + 1, y), (x + 1, y + 1);
        z: one number or four (same order)"""
        if group is None:
            group = next((a, b) for b in range((self.h) // 2) for a in range(self.w // 2) if (a, b) not in self.used)
        a, b = group
        assert group not in self.used and 2 * a + 1 < self.w and 2 * b + 1 < self.h, (self.name, group)
        self.used.add(group)
        zs = list(z) if isinstance(z, (list, tuple)) else [z] * 4
        base = f32(1.0 + ((a + b) & 1))
        ds = [base] * 4 if depth is None else list(depth)
        for (dx, dy), p, zz, dd in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (tl, bl, tr, br), zs, ds):
            x, y = 2 * a + dx, 2 * b + dy
            if p is None:
                self.pos[y][x] = None
            else:
                k = (F(p[0]) * 512, F(p[1]) * 512)
                assert k[0].denominator == 1 and k[1].denominator == 1, p
                k = (int(k[0]), int(k[1]))
                assert all(float(f32(v / 512.0)) * 512 == v for v in k), p      # the position is a binary32 number
                self.pos[y][x] = k
            assert float(f32(zz)) == zz and 0 <= zz <= 1
            self.z[y, x], self.und[y, x] = zz, dd
        return group

    def rect(self, x0, y0, x1, y1, z, **kw):
        return self.quad((x0, y0), (x0, y1), (x1, y0), (x1, y1), z, **kw)

    def vert(self):
        v = np.empty((self.h, self.w, 4), np.float32)
        for y in range(self.h):
            for x in range(self.w):
                p = self.pos[y][x]
                v[y, x, 0], v[y, x, 1] = (np.nan, np.nan) if p is None else (p[0] / 512.0, p[1] / 512.0)
        v[..., 2], v[..., 3] = self.z, self.ok
        return v

    @functools.cached_property
    def checker(self):
        return orc.calib_stage_raster(self.und, self.vert(), self.init.view(np.uint32))

    @functools.cached_property
    def statement(self):
        return cx.raster(self.w, self.h, self.und, self.pos, self.z, self.ok, self.init)


def _g_fill_rule():
    g = Grid(40, 30, "fill_rule")
    g.rect(2.5, 2.5, 8.5, 6.5, 0.5)                       # all four edges through centres: left and top in, right and bottom out
    g.rect(10.5, 2.25, 14.25, 6.75, 0.25)                 # left only
    g.rect(16.25, 2.5, 20.75, 6.25, 0.5)                  # top only
    g.rect(22.25, 2.25, 26.5, 6.75, 0.125)                # right only
    g.rect(28.25, 2.25, 33.75, 6.5, 0.5)                  # bottom only
    for k, (x, y) in enumerate([(4.5, 12.5), (14.5, 12.5), (24.5, 12.5), (34.5, 12.5)]):      # right triangles, the right angle at each corner in turn
        sx, sy = (1, -1)[k & 1], (1, -1)[k >> 1]
        a, b, c = (x, y), (x + 4 * sx, y), (x, y + 4 * sy)
        g.quad(a, b, c, c, 0.5)                           # the strip's second triangle has no area
        g.quad((x, y + 10), (x, y + 10 + 3 * sy), (x + 5 * sx, y + 10), (x, y + 10 + 3 * sy), 0.25)     # the other winding; the FIRST triangle has no area
    return g


def _g_windings():
    g = Grid(40, 30, "windings")
    g.rect(2.5, 2.5, 8.5, 8.5, 0.5)                                            # the strip's shared diagonal (tl - br) through centres
    g.quad((18.5, 2.5), (12.5, 2.5), (18.5, 8.5), (12.5, 8.5), 0.5)            # mirrored and turned: the other winding, the other diagonal
    g.quad((22.5, 8.5), (22.5, 2.5), (28.5, 8.5), (28.5, 2.5), 0.25)           # flipped top to bottom
    g.quad((32.5, 2.5), (38.5, 2.5), (32.5, 8.5), (38.5, 8.5), 0.25)           # transposed
    g.quad((2.5, 12.5), (2.5, 18.5), (8.5, 12.5), (8.5, 18.5), (0.125, 0.25, 0.5, 0.75))       # a z per vertex, both windings: the swap moves z too
    g.quad((18.5, 12.5), (12.5, 12.5), (18.5, 18.5), (12.5, 18.5), (0.125, 0.25, 0.5, 0.75))
    g.quad((22.25, 18.75), (22.75, 12.25), (28.5, 18.5), (29.0, 12.0), (0.75, 0.5, 0.25, 0.125))
    g.quad((2.0, 22.0), (6.0, 27.0), (6.0, 22.0), (2.0, 27.0), 0.5)            # a bow tie: the two triangles wind differently
    return g


def _g_halfway():
    g = Grid(40, 30, "halfway_snaps")
    h = F(1, 512)
    g.rect(2.5 - h, 2.5 - h, 8.5 - h, 6.5 - h, 0.5)              # half a 1/256 step short of the centres: snaps UP onto them
    g.rect(10.5 - 3 * h, 2.5 - 3 * h, 14.5 - 3 * h, 6.5 - 3 * h, 0.5)     # three halves short: snaps to one step short
    g.rect(16.5 + h, 2.5 + h, 20.5 + h, 6.5 + h, 0.25)
    g.rect(-1.5 - h, -1.5 - h, 1.5 - h, 1.5 - h, 0.25)           # negative odd multiples: -769/512 snaps to -384/256
    g.rect(-F(3, 512), 10, F(257, 512), 14, 0.5)                 # -3/512 -> -1/256; 257/512 -> 129/256: just past the first centre
    g.rect(-F(1, 512), 16, F(255, 512), 20, 0.5)                 # -1/512 -> 0; 255/512 -> 128/256: on the centre, a right edge: out
    rng = np.random.default_rng(3)
    for _ in range(40):
        c = rng.uniform(-3, [43, 33])
        p = [((2 * int(round(256 * (c[0] + rng.uniform(-3, 3)))) + 1) * h, (2 * int(round(256 * (c[1] + rng.uniform(-3, 3)))) + 1) * h) for _ in range(4)]
        g.quad(*p, float(rng.choice([0.125, 0.25, 0.5, 0.75])))
    return g


def _g_outside():
    g = Grid(40, 30, "outside_and_rejected")
    g.rect(-5, 4, 3.5, 9, 0.5)
    g.rect(36.25, 4, 47, 9, 0.5)
    g.rect(10, -6, 15, 2.75, 0.25)
    g.rect(10, 27.5, 15, 36, 0.25)
    g.rect(-9, -9, -1, -1, 0.5)                                   # wholly outside: nothing
    g.rect(41, 31, 50, 40, 0.5)
    g.quad(None, (20, 20), (25, 15), (25, 20), 0.5)               # the strip is (bl, tl, br), (tl, br, tr): tl is in both -> nothing drawn
    g.quad((20, 4), None, (25, 4), (25, 9), 0.5)                  # bl is in the first only: the second triangle is drawn
    g.quad((28, 12), (28, 17), None, (33, 17), 0.25)              # tr is in the second only: the first triangle is drawn
    big = 3906250                                                 # 1e9 / 256: the snapped value is not inside +-1e9, the triangles are dropped
    g.quad((2, 12), (2, 17), (big, 12), (7, 17), 0.5)             # tr: the first triangle (bl, tl, br) stays
    g.quad((-big, 20), (2, 25), (7, 20), (7, 25), 0.5)            # tl: both go
    g.quad((10, 12), (10, big), (15, 12), (15, 17), 0.25)         # bl
    g.quad((18, 22), (18, 27), (23, 22), (23, -big), 0.25)        # br
    return g


def _g_large():
    g = Grid(40, 30, "large_spans")
    near = 3906249.75                                             # the next float inside +-1e9 / 256
    g.quad((-near, -near), (-near, near), (near, -near), (near, near), 0.5)      # 64-bit products; covers the whole target
    g.quad((-near, 12.5), (-near, near), (near, 17.25), (near, near), 0.25)      # everything below a line through the target: rows 15 and up
    g.rect(-1, -1, 41, 31, 0.75)                                  # one quad over the whole target
    return g


def _threshold_pair():
    """(dmin, dmax) binary32 with dmax - dmin == 0.01f + 0.05f * (0.5f * (dmax + dmin)) exactly, all in binary32"""
    lo = f32(1.0) + np.arange(4096, dtype=np.float32) * f32(2.0 ** -12)
    approx = (lo + f32(0.01) + f32(0.025) * lo) / f32(0.975)
    for k in range(-8, 9):
        hi = approx
        for _ in range(abs(k)):
            hi = np.nextafter(hi, f32(np.inf if k > 0 else -np.inf))
        hit = (hi - lo) == f32(0.01) + f32(0.05) * (f32(0.5) * (hi + lo))
        if hit.any():
            i = int(np.argmax(hit))
            return lo[i], hi[i]
    raise AssertionError("no binary32 pair sits on the discontinuity threshold")


def _g_quad_tests():
    g = Grid(40, 30, "quad_tests")
    lo, hi = _threshold_pair()
    up = np.nextafter(hi, f32(np.inf))
    g.rect(2, 2, 6, 6, 0.5, depth=(lo, hi, lo, hi))               # the spread EQUALS the threshold: drawn
    g.rect(8, 2, 12, 6, 0.5, depth=(lo, up, lo, lo))              # one unit in the last place above: not drawn
    g.rect(14, 2, 18, 6, 0.5, depth=(up, lo, lo, lo))
    g.rect(20, 2, 24, 6, 0.5, depth=(lo, lo, lo, up))
    tenth, above = f32(0.1), np.nextafter(f32(0.1), f32(1))
    g.rect(26, 2, 30, 6, 0.25, depth=(above,) * 4)                # drawn
    for k in range(4):                                            # a corner AT 0.1f: not drawn
        g.rect(2 + 6 * k, 8, 6 + 6 * k, 12, 0.25, depth=[tenth if q == k else above for q in range(4)])
    for k in range(4):
        g.rect(2 + 6 * k, 14, 6 + 6 * k, 18, 0.25, depth=[f32(-np.inf) if q == k else f32(1.5) for q in range(4)])      # not drawn
    g.rect(26, 8, 30, 12, 0.25, depth=(f32(1.5), f32(np.nan), f32(1.5), f32(1.5)))      # not a number fails no comparison: drawn
    g.rect(32, 8, 36, 12, 0.25, depth=(f32(1.5), f32(1.5), f32(np.nan), f32(2.5)))      # ... and the spread of the rest still counts: not drawn
    for k in range(4):                                            # one invalid corner: not drawn
        a, b = g.rect(2 + 6 * k, 20, 6 + 6 * k, 24, 0.5)
        g.ok[2 * b + (k & 1), 2 * a + (k >> 1)] = False
    g.rect(32, 20, 36, 24, 0.5)
    return g


def _g_depth_test(flip):
    g = Grid(40, 30, "depth_test_%s" % ("reversed" if flip else "forward"))
    quads = [((2, 2, 12, 10), 0.5), ((6, 5, 16, 14), 0.25),                        # two, different z
             ((20, 2, 30, 10), 0.5), ((24, 5, 34, 14), 0.5),                       # two, equal z
             ((2, 16, 12, 24), 0.75), ((6, 18, 16, 27), 0.25), ((9, 15, 14, 29), 0.5),      # three
             ((20, 16, 36, 28), 0.5)]                                              # over an initial buffer below, equal and above
    for r, z in (quads[::-1] if flip else quads):
        g.rect(*r, z)
    g.init[16:28, 20:25], g.init[16:28, 25:30], g.init[16:28, 30:36] = 0.25, 0.5, 0.75
    g.init[0, :] = 0.0
    return g


def _g_scatter(w, h, seed, name):
    g = Grid(w, h, name)
    rng = np.random.default_rng(seed)
    for _ in range((w // 2) * (h // 2)):
        c = rng.uniform(-1, [w + 1, h + 1])
        p = []
        for _ in range(4):
            k = [int(round(512 * (v + rng.uniform(-2.5, 2.5)))) for v in c]
            p.append(tuple(F((q // 2) * 2 + 1 if rng.random() < 0.5 else q, 512) for q in k))
        g.quad(*p, float(rng.choice([0.125, 0.25, 0.5, 0.75])))
    return g


def _g_last_row_and_column(w, h):
    """every vertex used: the records of the last row and column are read, the lanes there draw nothing"""
    g = Grid(w, h, "dense_%dx%d" % (w, h))
    g.und[:] = 1.5
    for y in range(h):
        for x in range(w):
            g.pos[y][x] = (512 * x + 128, 512 * y + 256)
    g.z[:] = 0.25
    g.z[-1, :], g.z[:, -1] = 0.5, 0.5
    return g


@functools.lru_cache(None)
def _raster_cases():
    grids = [_g_fill_rule(), _g_windings(), _g_halfway(), _g_outside(), _g_large(), _g_quad_tests(), _g_depth_test(False), _g_depth_test(True),
             _g_last_row_and_column(40, 30)]
    for (w, h), seed in (((17, 16), 1), ((2, 2), 2), ((2, 9), 3), ((9, 2), 4)):
        grids += [_g_scatter(w, h, seed, "scatter_%dx%d" % (w, h)), _g_last_row_and_column(w, h)]
    grids.append(_g_last_row_and_column(1, 5))                    # no quad at all
    return {g.name: g for g in grids}


RASTER_NAMES = ["fill_rule", "windings", "halfway_snaps", "outside_and_rejected", "large_spans", "quad_tests", "depth_test_forward", "depth_test_reversed",
                "dense_40x30", "scatter_17x16", "dense_17x16", "scatter_2x2", "dense_2x2", "scatter_2x9", "dense_2x9", "scatter_9x2", "dense_9x2", "dense_1x5"]


def _check_raster(g, got_bits, against_statement):
    assert got_bits.shape == (g.h, g.w) and got_bits.dtype == np.uint32
    if not against_statement:
        assert np.array_equal(got_bits, g.checker), "%s: %d words differ" % (g.name, (got_bits != g.checker).sum())
        return
    got = got_bits.view(np.float32).astype(np.float64)
    zmin, exact, covered = g.statement
    assert np.array_equal(got[exact], zmin[exact]), (g.name, np.argwhere(exact & (got != zmin))[:5])
    assert (np.abs(got - zmin)[~exact] <= Z_REL * zmin[~exact]).all(), g.name


@pytest.mark.parametrize("name", RASTER_NAMES)
def test_raster(name):
    g = _raster_cases()[name]
    _check_raster(g, g.checker, True)
    zmin, exact, covered = g.statement
    drawn = g.checker != g.init.view(np.uint32)
    if name == "fill_rule":      # the first rectangle: left and top edge in, right and bottom edge out
        assert drawn[2:6, 2:8].all() and not drawn[6, 2:9].any() and not drawn[2:7, 8].any() and (covered[2:6, 2:8] == 1).all()
    if name == "windings":       # every centre of a quad, those on the shared diagonal included, belongs to exactly one of its two triangles
        for x0, y0 in ((2, 2), (12, 2), (22, 2), (32, 2), (2, 12), (12, 12)):
            assert (covered[y0:y0 + 6, x0:x0 + 6] == 1).all() and drawn[y0:y0 + 6, x0:x0 + 6].all(), (x0, y0)
    if name == "large_spans":
        assert drawn.all() and (zmin[15:] == 0.25).all() and (zmin[:15] == 0.5).all()
    if name == "quad_tests":
        on = [(2, 2), (26, 2), (26, 8), (32, 20)]
        off = [(8, 2), (14, 2), (20, 2), (32, 8)] + [(2 + 6 * k, y) for k in range(4) for y in (8, 14, 20)]
        assert all(drawn[y:y + 4, x:x + 4].all() for x, y in on) and not any(drawn[y:y + 4, x:x + 4].any() for x, y in off)
    if name == "outside_and_rejected":
        assert not drawn[15:20, 20:25].any() and drawn[4:9, 20:25].sum() in range(8, 16) and drawn[12:17, 28:33].sum() in range(8, 16)
        assert drawn[12:17, 2:7].sum() in range(8, 16) and not drawn[20:25, 2:7].any() and drawn[12:17, 10:15].sum() in range(8, 16) and not drawn[22:27, 18:23].any()
    if name == "dense_1x5":
        assert not drawn.any()


# ================================================================================================================ finalize
class FinCase:
    def __init__(self, name, cwh, shift=1000.0, colour=True, n=2, named=()):
        self.name, self.w, self.h, self.cw, self.ch, self.shift, self.n, self.named = name, 37, 29, cwh[0], cwh[1], shift, n, named
        self.params = _params(cwh, (37, 29), (60.0, 61.0, 26.0, 20.0), (40.0, 41.0, 18.0, 14.0))
        rng = np.random.default_rng(len(name) + cwh[0])
        z = rng.random((n, 29, 37), dtype=np.float32)
        z[rng.random(z.shape) < 0.1] = 1.0                                         # nothing drawn
        z[:, 0, :6] = [1.0, np.nextafter(f32(1), f32(0)), 0.0, 0.5, 2.0 ** -20, 0.25]
        self.zbuf = z.view(np.uint32)
        self.rgb = None
        if colour:
            kinds = np.array([(0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (255, 255, 255), (0, 7, 0)], np.uint8)
            pick = rng.integers(0, 8, (n, self.ch, self.cw))
            self.rgb = np.where((pick < 6)[..., None], kinds[np.minimum(pick, 5)], rng.integers(0, 256, (n, self.ch, self.cw, 3))).astype(np.uint8)
            if cwh == (2, 2):
                self.rgb[0] = kinds[:4].reshape(2, 2, 3)

    @functools.cached_property
    def checker(self):
        cb = orc.calib_from(self.params)
        return np.stack([orc.calib_stage_finalize(cb, self.zbuf[j], None if self.rgb is None else self.rgb[j], self.shift) for j in range(self.n)])


# the column x = 18 of 20x15 / 37x29 is an exact tie of a look-up whose binary32 scale is rounded: 2.7 % of the pixels are unsure by that alone, so
# that case takes a small shift, where next to no result is unsure.  named = (x, y, value): zb = 0 gives 0.1f; 0.1f x 5 is 0.5 + 3.7e-9, a binary32 tie that rounds up, 0.1f x 15 likewise 1.5 -> 2
FIN_CASES = [FinCase("larger_53x41", (53, 41)), FinCase("equal_37x29", (37, 29)), FinCase("smaller_20x15", (20, 15), shift=100.0), FinCase("tiny_2x2", (2, 2)),
             FinCase("no_colour", (53, 41), colour=False), FinCase("large_shift", (53, 41), shift=10000.0), FinCase("shift_1024", (37, 29), shift=1024.0),
             FinCase("tie_5", (53, 41), shift=5.0, colour=False, n=1, named=((2, 0, 1),)), FinCase("tie_15", (53, 41), shift=15.0, colour=False, n=1, named=((2, 0, 2),))]


def _check_finalize(case, got, against_statement, stats=None):
    assert got.shape == (case.n, case.h, case.w) and got.dtype == np.uint16
    if not against_statement:
        for j in range(case.n):
            assert np.array_equal(got[j], case.checker[j]), "%s frame %d: %d pixels differ" % (case.name, j, (got[j] != case.checker[j]).sum())
        return
    for j in range(case.n):
        want, dist, look = cx.finalize(case.zbuf[j], None if case.rgb is None else case.rgb[j], case.shift)
        sure = (dist > RESULT_MARGIN * np.maximum(want, 1)) & (look > LOOKUP_MARGIN)
        for x, y, v in case.named:
            assert want[y, x] == v
            sure[y, x] = True
        assert 1.0 - sure.mean() <= UNSURE_CAP, (case.name, 1.0 - sure.mean())
        if stats is not None:
            stats["fin_unsure"] = max(stats.get("fin_unsure", (0.0, "")), (1.0 - sure.mean(), case.name))
            bad = got[j] != want
            stats["result"] = max(stats.get("result", (0.0, "")), (float((dist / np.maximum(want, 1))[bad & (look > LOOKUP_MARGIN)].max(initial=0.0)), case.name))
            stats["lookup"] = max(stats.get("lookup", 0.0), float(look[bad & (dist > RESULT_MARGIN * np.maximum(want, 1))].max(initial=0.0)))
        assert np.array_equal(got[j][sure], want[sure]), (case.name, j, np.argwhere(sure & (got[j] != want))[:5])


@pytest.mark.parametrize("case", FIN_CASES, ids=lambda c: c.name)
def test_finalize(case):
    _check_finalize(case, case.checker, True)
    out = case.checker
    assert out[0, 0, 0] == 0                                                       # 1.0f: nothing drawn
    if case.rgb is None and case.shift == 1000.0:
        assert tuple(out[0, 0, 1:4]) == (10000, 100, 5050)                         # the predecessor of 1 is not the sentinel
    if case.shift == 10000.0:
        assert (out == 65535).any()
    if case.rgb is not None:                                                       # only a pixel with all three channels zero removes the depth
        lx, _ = cx.lookup_positions(37, case.cw)
        ly, _ = cx.lookup_positions(29, case.ch)
        seen = case.rgb[0][np.ix_(ly, lx)]
        for kind in ((0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, 0)):
            assert (seen == kind).all(-1).any(), kind
        assert lx.max() == case.cw - 1 and ly.max() == case.ch - 1


# ================================================================================================================ create
@pytest.mark.parametrize("res,maxd", [((5, 4, 3), 0.0), ((5, 4, 3), -1.0), ((5, 4, 3), float("nan")), ((5, 4, 3), float("inf")), ((0, 4, 3), 4.0),
                                      ((5, -1, 3), 4.0), ((5, 4, 0), 4.0)])
def test_create_rejects_an_implausible_table(res, maxd):
    """before any device is looked for: SF_ERR_INVALID_ARG (-1), never SF_ERR_DEVICE, and no calibrator"""
    L = calibrate._lib()
    g = np.ones(60, np.float32)
    lut = calibrate.SfLut(res[0], res[1], res[2], maxd, g.ctypes.data_as(C.POINTER(C.c_float)))
    p = _params((53, 41), (37, 29), (60.0, 61.0, 26.0, 20.0), (40.0, 41.0, 18.0, 14.0))
    h = C.c_void_p()
    assert L.sf_calibrator_create(C.byref(p), C.byref(lut), 1000.0, 0, C.byref(h)) == -1
    assert not h.value


# ================================================================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", UND_CASES, ids=lambda c: c.name)
def test_gpu_undistort_rgb(case):
    with calibrate.Calibrator(case.params) as cal:
        got = cal.stage_undistort_rgb(case.frames)
    _check_undistort(case, got, False)
    if case.named:
        _check_undistort(case, got, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PREP_CASES, ids=lambda c: c.name)
def test_gpu_prepare(case):
    with calibrate.Calibrator(case.params, case.grid, case.maxd, depth_shift=case.shift) as cal:
        got = cal.stage_prepare(case.frames)
    _check_prepare(case, got, False)
    if case.table_exact or case.named_ok:
        _check_prepare(case, got, True)


def _raster_batches():
    by_size = {}
    for name in RASTER_NAMES:
        g = _raster_cases()[name]
        by_size.setdefault((g.w, g.h), []).append(g)
    return by_size


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(40, 30), (17, 16), (2, 2), (2, 9), (9, 2), (1, 5)], ids=lambda s: "%dx%d" % s)
def test_gpu_raster(size):
    """every grid of a size alone, then all of them as one batch of 16 with an empty frame among them: each frame compared alone"""
    grids = _raster_batches()[size]
    empty = Grid(size[0], size[1], "empty")
    p = _params((53, 41), size, (60.0, 61.0, 26.0, 20.0), (40.0, 41.0, 18.0, 14.0))
    with calibrate.Calibrator(p) as cal:
        for g in grids:
            got = cal.stage_raster(g.und[None], g.vert()[None], g.init.view(np.uint32)[None])
            _check_raster(g, got[0], False)
            _check_raster(g, got[0], True)
        batch = ([empty] + grids * 16)[:16]
        batch[5], batch[0] = batch[0], batch[5]
        got = cal.stage_raster(np.stack([g.und for g in batch]), np.stack([g.vert() for g in batch]), np.stack([g.init.view(np.uint32) for g in batch]))
        for j, g in enumerate(batch):
            _check_raster(g, got[j], False)
        # what the hook refuses: a buffer outside [0, 1], a valid vertex with a negative z, another size, too many frames
        g = grids[0]
        bad = g.vert()[None].copy()
        bad[0, 0, 0, 2] = -0.5
        for args in ((g.und[None], g.vert()[None], np.full((1, size[1], size[0]), 0x3f800001, np.uint32)), (g.und[None], bad, g.init.view(np.uint32)[None]),
                     (np.zeros((1, 7, 5), np.float32), np.zeros((1, 7, 5, 4), np.float32), np.zeros((1, 7, 5), np.uint32)),
                     (np.zeros((17, size[1], size[0]), np.float32), np.zeros((17, size[1], size[0], 4), np.float32), np.zeros((17, size[1], size[0]), np.uint32))):
            with pytest.raises(Exception, match="scanfuse error -1"):
                cal.stage_raster(*args)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIN_CASES, ids=lambda c: c.name)
def test_gpu_finalize(case):
    with calibrate.Calibrator(case.params, depth_shift=case.shift) as cal:
        got = cal.stage_finalize(case.zbuf, case.rgb)
        _check_finalize(case, got, False)
        _check_finalize(case, got, True)
        with pytest.raises(Exception, match="scanfuse error -1"):
            cal.stage_finalize(np.zeros((1, 5, 7), np.uint32))
        with pytest.raises(Exception, match="scanfuse error -1"):
            cal.stage_undistort_rgb(np.zeros((1, 5, 7, 3), np.uint8))
        with pytest.raises(Exception, match="scanfuse error -1"):
            cal.stage_prepare(np.zeros((17, 29, 37), np.uint16))


# ================================================================================================================ measurement
def _measure():
    s = {}
    worst = (0.0, "")
    for case in UND_CASES:
        sx, sy, dist = _locations(case.K, case.c, case.cw, case.ch)
        want = cx.gather(case.frames[0], sx, sy, 0)
        bad = (case.checker[0] != want).any(-1)
        for x, y, _, _ in case.named:
            bad[y, x] = False
        s["sample"] = max(s.get("sample", 0.0), float(dist[bad].max(initial=0.0)))
        worst = max(worst, (float((dist <= SAMPLE_MARGIN).mean()), case.name))
    print("sample: largest distance from a half-integer among differing pixels %.3g; largest unsure share %.4f (%s)" % (s["sample"], worst[0], worst[1]))
    global POS_TOL
    POS_TOL = 1.0
    for case in PREP_CASES:
        _check_prepare(case, case.checker, True, s)
    print("vertex position / z, relative: %.3g (%s)" % s["pos"])
    for case in FIN_CASES:
        _check_finalize(case, case.checker, True, s)
    print("finalize: result %.3g (%s), look-up %.3g, unsure share %.4f (%s)" % (s["result"] + (s["lookup"],) + s["fin_unsure"]))
    print("vertices: largest unsure share %.4f (%s)" % s["vert_unsure"])


if __name__ == "__main__":
    _measure()
