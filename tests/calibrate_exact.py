"""An independent statement of the calibrate stage's rules (scannet_amd/csrc/calibrate.hip, oracle/calib_oracle.c), for
tests/test_calibrate_stages.py.  It shares no code with the kernels or the checker and is written from the rules the checker's header lists and the
formulas of Calibrate/src/calibration.h it cites, in REAL arithmetic (Python integers and fractions) on the binary32 parameters:

  sample_locations  where output pixel (x, y) samples the distorted image (Brown's model, round half up): the exact rational location, so a pixel whose
                    location is exactly k + 1/2 is decided here, and every other pixel is sure once it lies further from a half-integer than the
                    binary32 evaluation can move it
  table_value       the cell-coordinate rule (i / bin, the last cell where it reaches the resolution), the slice coordinate and the trilinear read with
                    only the upper neighbour clamped, exact; corrected_depth turns it into the u16 the conversion truncates to
  vertices          the mesh vertex of a pixel, exact: target position, projected z, and the NDC validity test with its bounds included
  raster            the draw: positions in 1/512 pixel snapped to 1/256 (half-way up), top-left rule (the helpers of tests/project_exact.py), no
                    culling, the exact affine z of each covering triangle, the smallest one against the initial buffer
  finalize          depth buffer -> metres -> u16 (round half up, saturating), the colour look-up position, the black test

Largest share of a case's pixels left out as unsure, over every case of tests/test_calibrate_stages.py (the cap is 3 %): sample locations 0.20 %
(undistort [exact-minus_half]); vertices 0.19 % (prepare [ndc-depth_range_below]); finalize 2.89 % ([smaller_20x15]: 2.70 % are the column x = 18, an
exact tie of the colour look-up whose binary32 scale 36 / 19 is rounded)."""
from fractions import Fraction

import numpy as np

from tests import project_exact as px

F = Fraction
HALF = F(1, 2)


def fr(v):
    """the exact value of a binary32 number"""
    return F(float(np.float32(v)))


def half_distance(v):
    """how far v lies from the nearest k + 1/2"""
    f = v - (v.numerator // v.denominator)
    return abs(f - HALF)


def round_half_up(v):
    return (v + HALF).numerator // (v + HALF).denominator


# ---------------------------------------------------------------------------------------------------------------- sample location
def sample_location(K, c, x, y):
    """calibration.h:192-212 in real arithmetic: K = (fx, fy, mx, my), c = (k1, k2, p1, p2, k3), all binary32 -> the exact (lx, ly)"""
    fx, fy, mx, my = (fr(v) for v in K)
    k1, k2, p1, p2, k3 = (fr(v) for v in c)
    nx, ny = (x - mx) / fx, (y - my) / fy
    r2 = nx * nx + ny * ny
    radial = 1 + r2 * k1 + r2 * r2 * k2 + r2 * r2 * r2 * k3
    lx = nx * radial + 2 * p1 * nx * ny + p2 * (r2 + 2 * nx * nx)
    ly = ny * radial + p1 * (r2 + 2 * ny * ny) + 2 * p2 * nx * ny
    return lx * fx + mx, ly * fy + my


def sample_locations(K, c, w, h):
    """-> sx, sy [h, w] int64 (round half up of the exact location) and dist [h, w] float64: the smaller distance of the two coordinates from a
    half-integer (0 = an exact tie, which the integers above decide: up)"""
    sx, sy, dist = np.empty((h, w), np.int64), np.empty((h, w), np.int64), np.empty((h, w))
    for y in range(h):
        for x in range(w):
            lx, ly = sample_location(K, c, x, y)
            sx[y, x], sy[y, x] = round_half_up(lx), round_half_up(ly)
            dist[y, x] = float(min(half_distance(lx), half_distance(ly)))
    return sx, sy, dist


def gather(img, sx, sy, invalid):
    """the undistorted image: the source pixel where it exists, `invalid` elsewhere"""
    h, w = img.shape[:2]
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.empty_like(img)
    out[...] = invalid
    out[inside] = img[sy[inside], sx[inside]]
    return out


# ---------------------------------------------------------------------------------------------------------------- table read
def cell_coordinate(i, size, res):
    """pixel i of `size` along an axis of `res` cells: i / (size // res), the last cell's where that reaches res"""
    x = F(i, size // res)
    return F(res - 1) if x >= res else x


def table_value(grid, w, h, i, j, depth):
    """grid [zres, yres, xres] binary32, max distance folded into `depth` = the slice coordinate before its cap (a Fraction) -> the exact trilinear
    value at source pixel (i, j).  grid3d.cpp:119-151: the lower neighbour is floor, the upper one is clamped to the last cell."""
    zres, yres, xres = grid.shape
    pos = (min(depth, F(zres - 1)), cell_coordinate(j, h, yres), cell_coordinate(i, w, xres))
    lo = [p.numerator // p.denominator for p in pos]
    hi = [min(a + 1, n - 1) for a, n in zip(lo, grid.shape)]
    t = [p - a for p, a in zip(pos, lo)]
    v = F(0)
    for cz, wz in ((lo[0], 1 - t[0]), (hi[0], t[0])):
        for cy, wy in ((lo[1], 1 - t[1]), (hi[1], t[1])):
            for cx, wx in ((lo[2], 1 - t[2]), (hi[2], t[2])):
                v += fr(grid[cz, cy, cx]) * wz * wy * wx
    return v


def corrected_depth(grid, max_dist, shift, w, h, i, j, raw):
    """calibration.h:226-250 on source pixel (i, j): -> (the u16 result of the truncating, saturating conversion, how far the exact quotient lies from
    the nearest whole number: 0.5 where saturation or a zero / negative table value decides).  depth = raw / shift is a binary32 quotient by
    definition; everything after it is real arithmetic."""
    depth = F(float(np.float32(raw) / np.float32(shift)))
    v = table_value(grid, w, h, i, j, depth * fr(grid.shape[0]) / fr(max_dist))
    if v == 0:
        return (0 if raw == 0 else 65535), 0.5          # 0 * inf is not a number: 0; anything else is +inf: saturates
    q = depth / v * fr(shift)
    if q < 0:
        return 0, 0.5
    if q >= 65536:
        return 65535, 0.5
    n = q.numerator // q.denominator
    return min(n, 65535), float(min(q - n, n + 1 - q))


# ---------------------------------------------------------------------------------------------------------------- mesh vertex
D_MIN, D_MAX = fr(0.1), fr(10.0)
D_RANGE = F(float(np.float32(10.0) - np.float32(0.1)))       # the binary32 difference the sources form


def vertex(d, x, y, w, h, cw, ch, Kd, Kc, E):
    """aligner.hlsl:52-103 + the viewport, in real arithmetic.  d: the pixel's depth in metres (binary32); Kd, Kc = (fx, fy, mx, my); E: 16 binary32
    numbers, row-major depth-to-colour.  -> None where the projection divides by zero, else (px, py, z, ok, slack): the target position, the projected
    z, the validity test (bounds included) and how far the closest of fx, fy, fz lies from the bound it is tested against."""
    d = fr(d)
    dfx, dfy, dmx, dmy = (fr(v) for v in Kd)
    cfx, cfy, cmx, cmy = (fr(v) for v in Kc)
    e = [fr(v) for v in E]
    cx, cy, cz = (x - dmx) * d / dfx, (y - dmy) * d / dfy, d              # the inverse intrinsic applied to (x d, y d, d)
    ww = e[12] * cx + e[13] * cy + e[14] * cz + e[15]
    if ww == 0:
        return None
    wx, wy, wz = ((e[4 * r] * cx + e[4 * r + 1] * cy + e[4 * r + 2] * cz + e[4 * r + 3]) / ww for r in range(3))
    qx, qy, qz = cfx * wx + cmx * wz, cfy * wy + cmy * wz, wz
    if qz == 0:
        return None
    fx = qx / qz / (cw - 1) * 2 - 1
    fy = 1 - qy / qz / (ch - 1) * 2
    fz = (qz - D_MIN) / D_RANGE
    # 0 <= fz <= 1 is near <= qz <= far: stated on qz, because the binary32 quotient is exactly 1 at qz = far while this real one, whose divisor is
    # the ROUNDED far - near, is not
    ok = -1 <= fx <= 1 and -1 <= fy <= 1 and D_MIN <= qz <= D_MAX
    slack = min(abs(fx - 1), abs(fx + 1), abs(fy - 1), abs(fy + 1), abs(qz - D_MIN) / D_RANGE, abs(qz - D_MAX) / D_RANGE)
    return (fx + 1) / 2 * w, (1 - fy) / 2 * h, fz, ok, slack


# ---------------------------------------------------------------------------------------------------------------- the draw
LIMIT = 10 ** 9          # a position whose 1/256-pixel value is not strictly inside +-1e9 drops its triangles


def snap512(k):
    """1/512 pixel -> 1/256 pixel, nearest, half-way cases up"""
    return (k + 1) // 2


def quad_is_drawn(d4, ok4):
    """aligner.hlsl:147-162 on the four corner depths (binary32): every corner above 0.1f (a NaN fails no comparison and takes no part), none -inf, the
    spread not above 0.01f + 0.05f * mean of the extremes -- that bound is a binary32 expression by definition -- and four valid vertices"""
    d = np.asarray(d4, np.float32)
    if np.any(d <= np.float32(0.1)) or np.any(np.isneginf(d)):
        return False
    dmax, dmin = np.float32(np.nanmax(d)), np.float32(np.nanmin(d))
    dm = np.float32(0.5) * (dmax + dmin)
    if dmax - dmin > np.float32(0.01) + np.float32(0.05) * dm:
        return False
    return all(ok4)


def triangle_fragments(p, z, w, h):
    """p: three (x, y) in 1/256 pixel, z: three Fractions -> [(i, j, exact z at the centre)], top-left rule, either winding; and the doubled area"""
    area = px._cross(*p[0], *p[1], *p[2])
    if area == 0:
        return [], 0
    sign = 1 if area > 0 else -1
    xs, ys = [q[0] for q in p], [q[1] for q in p]
    i_lo, i_hi = max(0, -((128 - min(xs)) // 256)), min(w - 1, (max(xs) - 128) // 256)
    j_lo, j_hi = max(0, -((128 - min(ys)) // 256)), min(h - 1, (max(ys) - 128) // 256)
    out = []
    for j in range(j_lo, j_hi + 1):
        cy = 256 * j + 128
        for i in range(i_lo, i_hi + 1):
            cx = 256 * i + 128
            e = []
            for k in range(3):
                a, b, v = p[k], p[(k + 1) % 3], p[(k + 2) % 3]
                ek = sign * px._cross(*a, *b, cx, cy)
                if ek < 0 or (ek == 0 and not px._owns_edge_point(a, b, v)):
                    break
                e.append(ek)
            else:
                # the weight of a vertex is the edge function of the opposite edge: e[0] (edge 0-1) belongs to vertex 2, e[1] to 0, e[2] to 1
                out.append((i, j, (e[1] * z[0] + e[2] * z[1] + e[0] * z[2]) / abs(area)))
    return out, abs(area)


def raster(w, h, und, pos512, z, ok, init):
    """One frame.  und [h, w] binary32 depth (the quad tests), pos512 [h][w] = (kx, ky) integers in 1/512 pixel or None (not a number), z [h, w]
    binary32, ok [h, w] bool, init [h, w] binary32 -> (zmin [h, w] float64: the smallest exact z over init and every covering triangle; exact [h, w]
    bool: binary32 interpolation is exact there -- every covering triangle has one z at its three vertices and a doubled area below 2^24, so the
    weights, their products with a dyadic z and their sums are whole numbers of a common unit below 2^24; covered [h, w] int: how many triangles
    cover the centre)."""
    best = [[fr(init[j, i]) for i in range(w)] for j in range(h)]
    exact = np.ones((h, w), bool)
    covered = np.zeros((h, w), np.int64)
    for y in range(h - 1):
        for x in range(w - 1):
            at = [(x, y + 1), (x, y), (x + 1, y + 1), (x + 1, y)]         # the strip v0 v1 v2 v3: triangles (v0 v1 v2) and (v1 v2 v3)
            if not quad_is_drawn([und[b, a] for a, b in at], [ok[b, a] for a, b in at]):
                continue
            for tri in (at[:3], at[1:]):
                p = [pos512[b][a] for a, b in tri]
                if any(q is None or abs(snap512(q[0])) >= LIMIT or abs(snap512(q[1])) >= LIMIT for q in p):
                    continue
                zs = [fr(z[b, a]) for a, b in tri]
                frags, area = triangle_fragments([(snap512(q[0]), snap512(q[1])) for q in p], zs, w, h)
                flat = zs[0] == zs[1] == zs[2] and area < 2 ** 24
                for i, j, zf in frags:
                    covered[j, i] += 1
                    exact[j, i] &= flat
                    if zf < best[j][i]:
                        best[j][i] = zf
    return np.array([[float(v) for v in row] for row in best]), exact, covered


# ---------------------------------------------------------------------------------------------------------------- finalize
def lookup_positions(n_out, n_in):
    """depth index -> (colour index, distance of the exact position from a half-integer): x / ((n_out - 1) / (n_in - 1)), round half up, clamped"""
    pos = [F(x * (n_in - 1), n_out - 1) if n_out > 1 else F(0) for x in range(n_out)]
    scale = F(n_out - 1, n_in - 1)
    if fr(float(scale)) == scale:
        # the scale is a binary32 number and the position is ONE correctly rounded quotient: half-integers are binary32 numbers, so the quotient
        # neither crosses nor misses one, and a tie is met exactly
        return np.array([min(round_half_up(p), n_in - 1) for p in pos]), np.full(n_out, 0.5)
    return np.array([min(round_half_up(p), n_in - 1) for p in pos]), np.array([float(half_distance(p)) for p in pos])


def finalize(zbuf_bits, rgb, shift):
    """zbuf_bits [h, w] uint32, rgb [ch, cw, 3] or None -> (u16 result, distance of the exact value x shift from a rounding tie (0.5 where the sentinel,
    a black pixel or the saturation decides), distance of the colour look-up position from a tie)"""
    zb = np.asarray(zbuf_bits, np.uint32).view(np.float32)
    h, w = zb.shape
    out, dist = np.zeros((h, w), np.int64), np.full((h, w), 0.5)
    look = np.full((h, w), 0.5)
    black = np.zeros((h, w), bool)
    if rgb is not None:
        cx, dx = lookup_positions(w, rgb.shape[1])
        cy, dy = lookup_positions(h, rgb.shape[0])
        black = (rgb[np.ix_(cy, cx)] == 0).all(-1)
        look = np.minimum.outer(dy, dx)
    s = fr(shift)
    for j in range(h):
        for i in range(w):
            if zb[j, i] == np.float32(1.0) or black[j, i]:
                continue
            v = (D_MIN + fr(zb[j, i]) * D_RANGE) * s
            if v >= 65536:
                out[j, i] = 65535
            else:
                out[j, i], dist[j, i] = min(max(round_half_up(v), 0), 65535), float(half_distance(v))
    return out.astype(np.uint16), dist, look
