"""DESIGN.md section 4n stated a second time, independently of the library and of tests/object_voxels_checker.c: the float part in numpy float32, one
operation at a time; the overlap of a quantised triangle and a cell by clipping the triangle against the cell's six half-spaces in rational
arithmetic (fractions.Fraction) -- the cell is set iff something is left.  Only the cells of the face's box plus one are tested: a cell beyond lies
outside one of the half-spaces with all three vertices.  The rule is exact after the quantisation, so there is no tolerance anywhere."""
from fractions import Fraction

import numpy as np

f32 = np.float32


def face_objects(tris, vobj):
    """-> (object per face, counted-so-far mask without the coordinate test)"""
    a, b, c = (vobj[tris[:, k].astype(np.int64)] for k in range(3))
    obj = np.where(b == c, b, a)
    distinct = (tris[:, 0] != tris[:, 1]) & (tris[:, 0] != tris[:, 2]) & (tris[:, 1] != tris[:, 2])
    return obj, distinct


def cube(v, dim, fit):
    """v: float32 [faces, 3, 3] -> (origin float32 [3], cell, scale) or None when the object is left out"""
    with np.errstate(all="ignore"):
        lo, hi = v.min((0, 1)), v.max((0, 1))
        e = (hi - lo).max()
        c = e / f32(fit)
        scale = f32(256.0) / c
        if not (np.isfinite(e) and e > 0 and np.isfinite(c) and c > 0 and np.isfinite(scale) and scale > 0):
            return None
        m = (lo + hi) * f32(0.5)
        o = m - (f32(dim) * f32(0.5)) * c
    return o.astype(f32), f32(c), f32(scale)


def quantise(v, o, scale, dim):
    with np.errstate(all="ignore"):
        r = np.rint((v - o) * scale)                                   # float32 throughout; rint rounds ties to even
        r = np.fmin(np.fmax(r, f32(0)), f32(256 * dim))                # fmax / fmin: a NaN goes to 0
    return r.astype(np.int64)


def clip_leaves_something(tri, cell):
    """Sutherland-Hodgman against the closed half-spaces of cell (i, j, k) = [256 i, 256 i + 256] x ...; tri: three integer points."""
    poly = [tuple(int(x) for x in p) for p in tri]
    for a in range(3):
        for sign, bound in ((1, 256 * cell[a] + 256), (-1, -256 * cell[a])):
            d = [sign * p[a] - bound for p in poly]                    # <= 0: inside (closed)
            if all(x > 0 for x in d):
                return False
            if all(x <= 0 for x in d):
                continue
            out = []
            for i in range(len(poly)):
                p, q, dp, dq = poly[i], poly[(i + 1) % len(poly)], d[i], d[(i + 1) % len(poly)]
                if dp <= 0:
                    out.append(p)
                if (dp < 0 and dq > 0) or (dp > 0 and dq < 0):
                    t = Fraction(dp) / Fraction(dp - dq)
                    out.append(tuple(Fraction(p[j]) + t * (Fraction(q[j]) - Fraction(p[j])) for j in range(3)))
            poly = out
            if not poly:
                return False
    return True


def occupancy(q, dim):
    """q: int64 [faces, 3, 3] -> uint8 [dim, dim, dim] ([z][y][x])"""
    occ = np.zeros((dim, dim, dim), np.uint8)
    for tri in q:
        u, w = tri[1] - tri[0], tri[2] - tri[0]
        if not np.cross(u, w).any():                                   # no area after quantisation
            continue
        lo, hi = tri.min(0) // 256 - 1, tri.max(0) // 256 + 1
        for k in range(max(lo[2], 0), min(hi[2], dim - 1) + 1):
            for j in range(max(lo[1], 0), min(hi[1], dim - 1) + 1):
                for i in range(max(lo[0], 0), min(hi[0], dim - 1) + 1):
                    if not occ[k, j, i] and clip_leaves_something(tri, (i, j, k)):
                        occ[k, j, i] = 1
    return occ


def known(occ, o, c, dim, grid):
    """grid: None or (weight uint8 [nz, ny, nx], voxel_size, lo_voxel)"""
    if grid is None:
        return np.ones_like(occ)
    weight, voxel, lo_voxel = grid
    idx, inside = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            n = weight.shape[2 - a]
            p = o[a] + (np.arange(dim, dtype=f32) + f32(0.5)) * c
            g = np.floor(p / f32(voxel) - f32(lo_voxel[a]) + f32(0.5))
            ok = (g >= 0) & (g < f32(n))                               # in float, before any conversion
            idx.append(np.where(ok, g, 0).astype(np.int64))
            inside.append(ok)
    seen = np.zeros_like(occ)
    if weight.size:
        w = weight[np.ix_(idx[2], idx[1], idx[0])] > 0
        seen = (w & inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :]).astype(np.uint8)
    return ((seen != 0) | (occ != 0)).astype(np.uint8)


def voxelize(xyz, tris, vobj, cls, dim=30, fit=24, min_faces=1, all_objects=False, grid=None):
    """-> (data uint8 [n, 2, dim, dim, dim], label uint8 [n], object_id int32 [n], origin float32 [n, 3], cell float32 [n])"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    vobj = np.asarray(vobj, np.uint32)
    data, label, oid, origin, cell = [], [], [], [], []
    if len(tris):
        obj, distinct = face_objects(tris, vobj)
        v = xyz[tris.astype(np.int64)]
        counted = distinct & np.isfinite(v).all((1, 2))
    for i, k in enumerate(cls):
        if not len(tris) or (k < 0 and not all_objects):
            continue
        mine = v[counted & (obj == i + 1)]
        if len(mine) < max(1, min_faces):
            continue
        cu = cube(mine, dim, fit)
        if cu is None:
            continue
        o, c, scale = cu
        occ = occupancy(quantise(mine, o, scale, dim), dim)
        data.append(np.stack([occ, known(occ, o, c, dim, grid)]))
        label.append(255 if k < 0 else k)
        oid.append(i)
        origin.append(o)
        cell.append(c)
    n = len(label)
    return (np.array(data, np.uint8).reshape(n, 2, dim, dim, dim), np.array(label, np.uint8), np.array(oid, np.int32),
            np.array(origin, f32).reshape(n, 3), np.array(cell, f32))
