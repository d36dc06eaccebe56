"""The four clean.mlx filters stated directly (tests/test_clean_stages_cpu.py, tests/test_clean_stages.py), independent of scannet_amd/csrc/clean.cpp,
scannet_amd/csrc/clean_gpu.hip and oracle/clean_oracle.py: no grid, no kd-tree, no sort keys, no union-find.

  clustering   VCG's ClusterVertex as published: vertices visited in index order; an unvisited vertex becomes a centre and takes every unvisited vertex at
               dist < r, by brute force over all pairs.  dist in numpy.float32, one rounding per operation: e = centre - p, sqrt((ex*ex + ey*ey) + ez*ez).
               r == 0: vertices whose three values compare equal as floats (-0.0 == +0.0) go to the lowest index.  Inputs are finite.
  lower_sets   L(j) = {i < j : dist(i, j) < r} and depth(j) = 0 where L(j) is empty, else 1 + max depth over L(j): a vertex is decided once all of L(j) is,
               so a resolution in rounds takes at most max depth + 1 of them.
  other roundings of the distance (fused multiply-adds; the other association of the sum), each step rounded once through rational arithmetic.
  faces        degenerate by the three comparisons; duplicates as frozensets, the first occurrence wins.
  components   breadth-first search over a dict from unordered vertex pair to faces (all faces of a pair are connected); the root is the lowest face.
  compact      used, remap (how many used vertices lie below), the gathered arrays.
  clean        the composition, with every field of sf_clean_stats.
Result layouts are those of scannet_amd.meshclean.clean_stage_*."""
from collections import deque
from fractions import Fraction

import numpy as np

F32 = np.float32
KERNEL, FUSED, ASSOC = "(ex2 + ey2) + ez2", "fma(ez, ez, fma(ey, ey, ex * ex))", "ex2 + (ey2 + ez2)"


# ---- the distance ---------------------------------------------------------------------------------------------------------------------------------------
def dist_rows(c, p):
    """float32 distance of centre c[3] to every row of p[n, 3], one rounding per operation."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = (np.asarray(c, F32)[None, :] - np.asarray(p, F32)).astype(F32)
        ex2, ey2, ez2 = e[:, 0] * e[:, 0], e[:, 1] * e[:, 1], e[:, 2] * e[:, 2]
        return np.sqrt((ex2 + ey2) + ez2)


def round32(q):
    """a non-negative rational to the nearest binary32, ties to even (finite results only)"""
    q = Fraction(q)
    if q == 0:
        return F32(0)
    assert q > 0
    e = (q.numerator.bit_length() - q.denominator.bit_length()) - 24
    while q >= Fraction(2) ** (e + 24):
        e += 1
    while q < Fraction(2) ** (e + 23):
        e -= 1
    e = max(e, -149)                                   # subnormals keep the spacing 2^-149
    scaled = q / Fraction(2) ** e
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and (m & 1)):
        m += 1
    v = Fraction(m) * Fraction(2) ** e
    out = F32(float(v))                                # m has at most 25 bits: exact in a double, exact or 2^k in binary32
    assert Fraction(float(out)) == v
    return out


def dist_as(c, p, how):
    """The distance of two points under one of the three roundings, every step rounded once from the exact value."""
    e = [Fraction(float(F32(F32(a) - F32(b)))) for a, b in zip(c, p)]           # the subtraction is common to all three
    x2, y2, z2 = e[0] * e[0], e[1] * e[1], e[2] * e[2]
    r = lambda q: Fraction(float(round32(q)))
    if how == KERNEL:
        s = r(r(r(x2) + r(y2)) + r(z2))
    elif how == FUSED:
        s = r(z2 + r(y2 + r(x2)))
    elif how == ASSOC:
        s = r(r(x2) + r(r(y2) + r(z2)))
    else:
        raise ValueError(how)
    return np.sqrt(F32(float(s)))                                              # IEEE: correctly rounded


# ---- filter 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def cluster(pos, r, how=KERNEL):
    """target[V] (uint32): the centre each vertex goes to, itself for a centre."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    n, r = len(pos), F32(r)
    target, visited = np.arange(n, dtype=np.uint32), np.zeros(n, bool)
    for i in range(n):
        if visited[i]:
            continue
        visited[i] = True
        if r > 0:
            if how == KERNEL:
                near = dist_rows(pos[i], pos) < r
            else:
                near = np.array([dist_as(pos[i], pos[j], how) < r for j in range(n)], bool)
        else:
            near = (pos == pos[i][None, :]).all(axis=1)
        take = near & ~visited
        target[take] = i
        visited |= take
    return target


def lower_sets(pos, r):
    """(L, depth): L[j] = the lower-index neighbours of j, depth[j] as in the module docstring."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    L, depth = [], np.zeros(len(pos), np.int64)
    for j in range(len(pos)):
        lj = np.nonzero(dist_rows(pos[j], pos[:j]) < F32(r))[0] if j else np.zeros(0, np.int64)
        L.append(lj)
        depth[j] = 1 + depth[lj].max() if len(lj) else 0
    return L, depth


# ---- faces -------------------------------------------------------------------------------------------------------------------------------------------------
def faces(tri, target=None):
    tri = np.asarray(tri, np.uint32).reshape(-1, 3)
    verdict, seen, out = np.zeros(len(tri), np.uint8), set(), []
    for f, (a, b, c) in enumerate(tri.tolist()):
        if target is not None:
            a, b, c = int(target[a]), int(target[b]), int(target[c])
        if a == b or b == c or a == c:
            verdict[f] = 1
            continue
        key = frozenset((a, b, c))
        if key in seen:
            verdict[f] = 2
            continue
        seen.add(key)
        out.append((a, b, c))
    return {"verdict": verdict, "tri": np.array(out, np.uint32).reshape(-1, 3), "degenerate": int((verdict == 1).sum()), "duplicate": int((verdict == 2).sum())}


def components(tri, min_faces):
    tri = np.asarray(tri, np.uint32).reshape(-1, 3)
    n = len(tri)
    by_pair = {}
    for f, (a, b, c) in enumerate(tri.tolist()):
        for u, v in ((a, b), (b, c), (c, a)):
            by_pair.setdefault(frozenset((u, v)), []).append(f)
    root, size = np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint32)
    for f0 in range(n):                                            # ascending: the first face to reach a component is its lowest
        if root[f0] != 0xFFFFFFFF:
            continue
        root[f0] = f0
        members, queue = [f0], deque([f0])
        while queue:
            a, b, c = tri[queue.popleft()].tolist()
            for u, v in ((a, b), (b, c), (c, a)):
                for g in by_pair[frozenset((u, v))]:
                    if root[g] == 0xFFFFFFFF:
                        root[g] = f0
                        members.append(g)
                        queue.append(g)
        size[members] = len(members)
    keep = (size >= min_faces).astype(np.uint8)
    is_root = root == np.arange(n, dtype=np.uint32)
    counters = np.array([is_root.sum(), (is_root & (keep == 0)).sum(), (keep == 0).sum()], np.uint32)
    return {"root": root, "size": size, "keep": keep, "counters": counters}


def compact(pos, col, tri):
    pos = np.asarray(pos, F32).reshape(-1, 3)
    tri = np.asarray(tri, np.uint32).reshape(-1, 3)
    used = np.zeros(len(pos), np.uint32)
    for f in tri.tolist():
        for v in f:
            used[v] = 1
    remap, w = np.zeros(len(pos), np.uint32), 0
    for v in range(len(pos)):
        remap[v] = w
        w += int(used[v])
    sel = used == 1
    return {"used": used, "remap": remap, "pos": pos[sel].copy(), "col": None if col is None else np.asarray(col, np.uint8).reshape(-1, 4)[sel].copy(),
            "tri": remap[tri.astype(np.int64)].reshape(-1, 3), "vertices_out": w}


STATS = ("vertices_in", "faces_in", "vertices_merged", "faces_degenerate", "faces_duplicate", "components_in", "components_removed", "faces_small_component",
         "vertices_unreferenced", "vertices_out", "faces_out")


def clean(pos, col, tri, r, min_faces):
    """(pos, col, tri, stats) of the whole filter chain, with the stage results for the composition test."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    tri = np.asarray(tri, np.uint32).reshape(-1, 3)
    target = cluster(pos, r)
    fa = faces(tri, target)
    co = components(fa["tri"], min_faces)
    left = fa["tri"][co["keep"] == 1]
    cm = compact(pos, col, left)
    merged = int((target != np.arange(len(pos))).sum())
    st = {"vertices_in": len(pos), "faces_in": len(tri), "vertices_merged": merged, "faces_degenerate": fa["degenerate"], "faces_duplicate": fa["duplicate"],
          "components_in": int(co["counters"][0]), "components_removed": int(co["counters"][1]), "faces_small_component": int(co["counters"][2]),
          "vertices_out": cm["vertices_out"], "faces_out": len(left)}
    # an unreferenced vertex is a centre no surviving face names
    st["vertices_unreferenced"] = int(((target == np.arange(len(pos))) & (cm["used"] == 0)).sum())
    assert st["vertices_in"] == st["vertices_merged"] + st["vertices_unreferenced"] + st["vertices_out"]
    assert st["faces_in"] == st["faces_degenerate"] + st["faces_duplicate"] + st["faces_small_component"] + st["faces_out"]
    return cm["pos"], cm["col"], cm["tri"], st, {"target": target, "faces": fa, "components": co, "compact": cm}
