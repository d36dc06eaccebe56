"""An independent statement of the annotation projector's rules (scannet_amd/csrc/project.hip, oracle/project_oracle.c), for
tests/test_project_stages.py.  It shares no code with the kernels or the checker and is written from the Direct3D 11 rules the checker's header
lists: pixel centres at +0.5, vertices snapped to 1/256 pixel (half-way cases up), top-left fill rule, depth test LESS with the earlier triangle
winning a tie, near-plane clipping, fragments beyond the far plane discarded; then the depth-consistency filter and the 5x5 vote of
AnnotationTools/ProjectAnnotations/Visualizer.cpp:144-186.

  lattice_raster   exact, in Python integers and fractions: fronto-parallel triangles whose screen positions are multiples of 1/1024 pixel, seen by
                   the lattice camera (identity pose, 128 x 64, fx = fy = 64), where every float32 operation of the transform is exact
  float_raster     float64: any pose, sloped triangles, the near clip; says which pixels it is sure about
  vote             exact, in integers
  consistency      exact in millimetres; says which pixels sit at exact equality, where it does not decide"""
from fractions import Fraction

import numpy as np

LATTICE_W, LATTICE_H, LATTICE_F = 128, 64, 64      # any power-of-two size keeps p00 = 2 fx / W and p11 = -2 fy / H powers of two (1 and -2 here)
NONE = -1


# ---------------------------------------------------------------------------------------------------------------- exact raster on the lattice
def lattice_vertex(kx, ky, z, w=LATTICE_W, h=LATTICE_H):
    """camera-space position (Fractions) of the point that the lattice camera projects to (kx / 1024, ky / 1024) pixels at camera depth z"""
    z = Fraction(z)
    return (Fraction(kx, 1024) - w // 2) * z / LATTICE_F, (Fraction(ky, 1024) - h // 2) * z / LATTICE_F, z


def _snap(k):
    """1/1024 pixel -> 1/256 pixel, nearest, half-way cases up: floor(k / 4 + 1 / 2)"""
    return (k + 2) // 4


def _cross(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _owns_edge_point(a, b, v):
    """A pixel centre lies exactly on edge a-b of a triangle whose third vertex is v.  Direct3D's top-left rule: the centre belongs to the triangle
    iff the edge is a top edge (horizontal, the interior below it: y grows downwards) or a left edge (not horizontal, the interior to its right)."""
    if a[1] == b[1]:
        return v[1] > a[1]
    x_on_line = a[0] + Fraction((b[0] - a[0]) * (v[1] - a[1]), b[1] - a[1])   # where the edge's line passes at the height of v
    return v[0] > x_on_line


def lattice_raster(triangles, w=LATTICE_W, h=LATTICE_H, near=Fraction(1, 10), far=Fraction(15)):
    """triangles: a list of ((kx0, ky0), (kx1, ky1), (kx2, ky2), z) in 1/1024 pixel and camera depth, or None for a triangle the rules never draw
    (a bad index, a non-finite vertex).  Returns the winning triangle index per pixel as a list of h lists (NONE where nothing covers the centre), and
    per triangle None (never drawn: out of the depth range, zero area) or (longest edge component in 1/256 pixel, pixel centres in its clamped bounding
    box, pixel centres it covers)."""
    best = [[None] * w for _ in range(h)]
    info = [None] * len(triangles)
    for index, tri in enumerate(triangles):
        if tri is None:
            continue
        z = Fraction(tri[3])
        if z < near or z > far:          # behind the near plane as a whole / z_ndc > 1
            continue
        p = [(_snap(kx), _snap(ky)) for kx, ky in tri[:3]]
        area = _cross(*p[0], *p[1], *p[2])
        if area == 0:
            continue
        sign = 1 if area > 0 else -1
        xs, ys = [q[0] for q in p], [q[1] for q in p]
        # centres (256 i + 128, 256 j + 128) inside the bounding box and the image
        i_lo, i_hi = max(0, -((128 - min(xs)) // 256)), min(w - 1, (max(xs) - 128) // 256)
        j_lo, j_hi = max(0, -((128 - min(ys)) // 256)), min(h - 1, (max(ys) - 128) // 256)
        span = max(max(abs(p[k][0] - p[(k + 1) % 3][0]), abs(p[k][1] - p[(k + 1) % 3][1])) for k in range(3))
        covered = 0
        for j in range(j_lo, j_hi + 1):
            cy = 256 * j + 128
            for i in range(i_lo, i_hi + 1):
                cx = 256 * i + 128
                inside = True
                for k in range(3):
                    a, b, v = p[k], p[(k + 1) % 3], p[(k + 2) % 3]
                    e = sign * _cross(*a, *b, cx, cy)
                    if e < 0 or (e == 0 and not _owns_edge_point(a, b, v)):
                        inside = False
                        break
                covered += inside
                if inside and (best[j][i] is None or (z, index) < best[j][i]):
                    best[j][i] = (z, index)
        info[index] = (span, max(0, i_hi - i_lo + 1) * max(0, j_hi - j_lo + 1), covered)
    return [[NONE if c is None else c[1] for c in row] for row in best], info


# ---------------------------------------------------------------------------------------------------------------- float64 raster
def _view(cam2world):
    c = np.asarray(cam2world, np.float64).reshape(4, 4)
    R = c[:3, :3] / np.linalg.norm(c[:3, :3], axis=0)      # normalised columns
    return R.T, -R.T @ c[:3, 3]


def _clip_near(poly, near):
    """Sutherland-Hodgman against z >= near, camera space"""
    out = []
    for k in range(len(poly)):
        a, b = poly[k], poly[(k + 1) % len(poly)]
        if a[2] >= near:
            out.append(a)
        if (a[2] >= near) != (b[2] >= near):
            t = (near - a[2]) / (b[2] - a[2])
            out.append(a + t * (b - a))
    return out


def float_raster(xyz, tris, cam2world, w, h, fx, fy, near, far, edge_margin, depth_flat, depth_shift):
    """-> dict of [h, w] arrays: `index` (NONE where nothing is drawn), `z_ndc` and `zcam` of the front-most surface, `covered`, and `sure`: the
    centre is further than edge_margin pixels from every edge of every drawn polygon, and neither the second surface nor the far plane is within
    the depth margins of the front-most surface.  A surface's depth margin at a pixel is depth_flat + depth_shift * |grad z_ndc|: a rounding term
    plus what moving the surface by depth_shift pixels across the screen does to its depth there (z_ndc is affine in screen space on a plane).
    `bound` = that margin for the front-most surface, `slope` = its |grad z_ndc| per pixel, `edge` = the distance in pixels to the nearest polygon
    edge, `far_gap` = how close (z_ndc) any surface under the centre comes to the far plane."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    R, t = _view(cam2world)
    cam = xyz @ R.T + t
    A, B = far / (far - near), near * far / (far - near)
    z1 = np.full((h, w), np.inf)
    z2 = np.full((h, w), np.inf)
    index = np.full((h, w), NONE, np.int64)
    edge = np.full((h, w), np.inf)
    far_gap = np.full((h, w), np.inf)
    far_clear = np.full((h, w), np.inf)
    g1 = np.zeros((h, w))
    g2 = np.zeros((h, w))
    for ti, tri in enumerate(np.asarray(tris).reshape(-1, 3)):
        if np.any(tri >= len(xyz)):
            continue
        P = cam[tri]
        if not np.all(np.isfinite(P)):
            continue
        poly = _clip_near([P[0], P[1], P[2]], near)
        if len(poly) < 3:
            continue
        poly = np.array(poly)
        sx, sy = w / 2.0 + fx * poly[:, 0] / poly[:, 2], h / 2.0 + fy * poly[:, 1] / poly[:, 2]
        i0, i1 = int(max(0, np.floor(sx.min() - 1.5))), int(min(w - 1, np.ceil(sx.max() + 0.5)))
        j0, j1 = int(max(0, np.floor(sy.min() - 1.5))), int(min(h - 1, np.ceil(sy.max() + 0.5)))
        if i1 < i0 or j1 < j0:
            continue
        cx, cy = np.meshgrid(np.arange(i0, i1 + 1) + 0.5, np.arange(j0, j1 + 1) + 0.5)
        area2 = sum(sx[k] * sy[(k + 1) % len(sx)] - sx[(k + 1) % len(sx)] * sy[k] for k in range(len(sx)))
        inside = np.ones(cx.shape, bool)
        dist = np.full(cx.shape, np.inf)
        for k in range(len(sx)):
            ax, ay, bx, by = sx[k], sy[k], sx[(k + 1) % len(sx)], sy[(k + 1) % len(sx)]
            ex, ey = bx - ax, by - ay
            L2 = ex * ex + ey * ey
            if L2 == 0.0:
                d = np.hypot(cx - ax, cy - ay)
            else:
                side = (ex * (cy - ay) - ey * (cx - ax)) * np.sign(area2)
                inside &= side > 0
                u = np.clip(((cx - ax) * ex + (cy - ay) * ey) / L2, 0.0, 1.0)
                d = np.hypot(cx - (ax + u * ex), cy - (ay + u * ey))
            dist = np.minimum(dist, d)
        blk = (slice(j0, j1 + 1), slice(i0, i1 + 1))
        edge[blk] = np.minimum(edge[blk], dist)
        if area2 == 0.0:
            continue
        # camera depth where the ray through the centre meets the triangle's plane
        n = np.cross(P[1] - P[0], P[2] - P[0])
        den = n[0] * (cx - w / 2.0) / fx + n[1] * (cy - h / 2.0) / fy + n[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            zc = np.where(den != 0.0, (n @ P[0]) / den, np.inf)
        on_plane = inside & np.isfinite(zc) & (zc > 0.0)
        slope = B * np.hypot(n[0] / fx, n[1] / fy) / abs(n @ P[0]) if (n @ P[0]) != 0.0 else np.inf      # 1 / z is affine in the pixel position
        gap = np.where(on_plane, np.abs(A - B / np.where(on_plane, zc, 1.0) - 1.0), np.inf)
        far_gap[blk] = np.minimum(far_gap[blk], gap)
        far_clear[blk] = np.minimum(far_clear[blk], gap - (depth_flat + depth_shift * slope))
        hit = on_plane & (zc <= far)
        zc = np.where(hit, zc, np.inf)
        a1, a2, ai = z1[blk], z2[blk], index[blk]
        first = zc < a1
        second = ~first & (zc < a2)
        g2[blk] = np.where(first, g1[blk], np.where(second, slope, g2[blk]))
        g1[blk] = np.where(first, slope, g1[blk])
        z2[blk] = np.where(first, a1, np.minimum(a2, zc))
        z1[blk] = np.where(first, zc, a1)
        index[blk] = np.where(first, ti, ai)
    covered = index != NONE
    with np.errstate(divide="ignore", invalid="ignore"):
        ndc1, ndc2 = A - B / z1, A - B / z2          # z = inf (nothing there) -> A > 1
    ndc2 = np.where(np.isfinite(z2), ndc2, np.inf)
    bound = depth_flat + depth_shift * g1
    sure = (edge > edge_margin) & (far_clear > 0.0) & (~covered | (ndc2 - ndc1 > bound + depth_flat + depth_shift * g2))
    return {"index": index, "z_ndc": np.where(covered, ndc1, np.nan), "zcam": np.where(covered, z1, 0.0), "covered": covered, "sure": sure, "edge": edge,
            "far_gap": far_gap, "bound": bound, "slope": g1}


# ---------------------------------------------------------------------------------------------------------------- exact vote
def vote(inst, label):
    """A labelled pixel keeps its label (and its instance) iff 5 * count >= total: count = the pixels of its 5 x 5 window, as they were before the
    vote, that carry its label; total = the pixels of the window inside the image."""
    inst, label = np.asarray(inst), np.asarray(label)
    h, w = label.shape
    count = np.zeros((h, w), np.int64)
    total = np.zeros((h, w), np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))       # centres whose neighbour (y + dy, x + dx) exists
            yn, xn = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
            total[ys, xs] += 1
            count[ys, xs] += label[yn, xn] == label[ys, xs]
    keep = (label != 0) & (5 * count >= total)
    return np.where(keep, inst, 0).astype(np.uint8), np.where(keep, label, 0).astype(np.uint16), count, total


# ---------------------------------------------------------------------------------------------------------------- exact consistency filter
def _round_half_away(v32):
    return np.floor(v32.astype(np.float64) + 0.5).astype(np.int64)      # non-negative arguments only


def nearest_indices(n_out, n_in):
    """colour index -> (depth index, colour index the rendered depth is read at): the nearest-neighbour resample of the rendered depth to the depth
    resolution.  The POSITIONS are binary32 products by definition (index times a binary32 scale), rounded to the nearest integer."""
    to_depth = _round_half_away(np.float32(n_in - 1) / np.float32(n_out - 1) * np.arange(n_out, dtype=np.float32))
    back = _round_half_away(to_depth.astype(np.float32) * (np.float32(n_out - 1) / np.float32(n_in - 1)))
    return to_depth, np.minimum(back, n_out - 1)


def consistency(keys, first_vertex, vinst, vlabel, orig_depth, w, h, dw, dh, near, far, filter_using_original_depth, thresh_mm=200):
    """keys [h, w] u64 -> (instance, label, undecided) before the vote.  A label goes iff filter_using_original_depth and dorig == 0, or
    drndr != 0 and dorig != 0 and |drndr - dorig| > thresh_mm + 10 dorig, all in whole millimetres; drndr = the rendered camera depth at the resampled
    position, truncated to millimetres.  `undecided`: pixels at exact equality, and pixels whose rendered depth is within 0.05 mm of a whole
    millimetre (where truncation depends on the last bit of the camera depth)."""
    keys = np.asarray(keys, np.uint64).reshape(h, w)
    drawn = keys != np.uint64(2 ** 64 - 1)
    tri = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    v0 = np.asarray(first_vertex, np.int64)[np.where(drawn, tri, 0)]
    inst = np.where(drawn, np.asarray(vinst)[v0], 0).astype(np.uint8)
    label = np.where(drawn, np.asarray(vlabel)[v0], 0).astype(np.uint16)
    d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    A, B = far / (far - near), near * far / (far - near)
    with np.errstate(divide="ignore", invalid="ignore"):
        zc = B / (A - d)
    zc = np.where(drawn & (d != 0.0) & (d != 1.0) & (zc >= near) & (zc <= far), zc, 0.0)
    if orig_depth is None:
        return inst, label, np.zeros((h, w), bool), zc
    mm = zc * 1000.0
    shaky = np.abs(mm - np.round(mm)) < 0.05
    dx, sx = nearest_indices(w, dw)
    dy, sy = nearest_indices(h, dh)
    drndr = np.floor(mm).astype(np.int64)[np.ix_(sy, sx)]
    dorig = np.asarray(orig_depth, np.int64).reshape(dh, dw)[np.ix_(dy, dx)]
    gap, bound = np.abs(drndr - dorig), thresh_mm + 10 * dorig
    gone = ((dorig == 0) if filter_using_original_depth else np.zeros((h, w), bool)) | ((drndr != 0) & (dorig != 0) & (gap > bound))
    undecided = (label != 0) & ((shaky & (zc != 0.0))[np.ix_(sy, sx)] | ((drndr != 0) & (dorig != 0) & (gap == bound)))
    gone &= label != 0
    return np.where(gone, 0, inst).astype(np.uint8), np.where(gone, 0, label).astype(np.uint16), undecided, zc
