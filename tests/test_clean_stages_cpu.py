"""The mesh clean's four filters, stage by stage, CPU half (default suite; the device half and the mutation table are tests/test_clean_stages.py).

Three parties: the statement tests/clean_exact.py (brute force over all pairs, frozensets, breadth-first search; no grid, no kd-tree, no sort keys, no
union-find), the cases tests/clean_cases.py, and what is held to the statement here on every case: the host filter's clustering alone
(sf_clean_probe_merge: clean.cpp's merge_close), oracle/clean_oracle.py's merge_close_vertices, sf_mesh_clean's arrays and every statistic, and
clean_oracle.clean's arrays.  Every comparison is exact, on integers and bit patterns.

The seeded search of tests/clean_cases.py kept 40 pairs of each of the four kinds (33 508 pairs within 3e-10 of r = 0.0010689 were looked at): the kernel's
order (ex2 + ey2) + ez2 says dist < r and the fused form says not, the other way round, and the same two against ex2 + (ey2 + ez2).  Each verdict is
checked below against rational arithmetic rounded once per step.

Outcome: the statement, the host probe, oracle/clean_oracle.py and sf_mesh_clean agree on every case; nothing had to be fixed in clean.cpp,
clean_gpu.hip or the oracle.

Two expectations of the issue that asked for these tests do not follow from its own definitions and are stated here as they are:
  * r = 1e-6 on a 3 m box is SUPPORTED: 2^21 cells of 2e-6 m reach 4.19 m.  The case is kept with that answer and a 5 m box (not supported) stands beside it.
  * a 130-chain in reverse index order is the same problem as the chain (vertex j still has j - 1 within r: depth(j) = j), so "depth 0 everywhere, one launch"
    cannot hold for it; it is kept and held to the bound 1 <= launches <= max depth + 1.  The cases with depth 0 everywhere ("apart130", the islands of the
    cell and rounding cases that do not merge, ...) are the ones that must take exactly one launch, and every case with max depth 0 is held to that."""
import functools

import numpy as np
import pytest

from oracle import clean_oracle
from scannet_amd import meshclean
from scannet_amd._abi import ScanfuseError
from scannet_amd.segmentator import Mesh
from tests import clean_cases as cc
from tests import clean_exact as cx

OK_MERGE = [c for c in cc.MERGE_CASES if c.error is None]
WHOLE = cc.whole_cases()
STATEMENT_STAGES = (cx.cluster, lambda nv, tri, target: cx.faces(tri, target), cx.components, cx.compact)


def _same(got, want, what):
    """two stage results agree in every field, to the bit"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        if want[k] is None or got[k] is None:
            assert got[k] is None and want[k] is None, (what, k)
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.ndim == 0 and w.ndim == 0:
            assert int(g) == int(w), (what, k, int(g), int(w))
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        same = np.array_equal(np.ascontiguousarray(g).reshape(-1).view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8))
        assert same, "%s: %s differs at %s" % (what, k, np.argwhere(np.atleast_1d(g != w))[:5].tolist())


@functools.lru_cache(maxsize=None)
def stated_target(name):
    c = cc.by_name(name)
    t = cx.cluster(c.pos, c.r)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def stated_depth(name):
    c = cc.by_name(name)
    return int(cx.lower_sets(c.pos, c.r)[1].max()) if c.r > 0 and len(c.pos) else 0


@functools.lru_cache(maxsize=None)
def stated_whole(name):
    _, pos, col, tri, r, mf = next(w for w in WHOLE if w[0] == name)
    return cx.clean(pos, col, tri, r, mf)


def _arrays_same(got, want, what):
    (gx, gc, gt), (wx, wc, wt) = got, want
    assert gx.shape == wx.shape and np.array_equal(gx.view(np.uint32), wx.view(np.uint32)), what
    assert np.array_equal(np.asarray(gt, np.uint32).reshape(-1, 3), np.asarray(wt, np.uint32).reshape(-1, 3)), what
    assert (gc is None and wc is None) or np.array_equal(gc, wc), what


def host_clean(pos, col, tri, r, mf, gpu=None):
    out, st = meshclean.clean(Mesh.from_arrays(pos, tri, col), float(r), int(mf), gpu=gpu)
    x, c, t = out.arrays()
    return (x.reshape(-1, 3), None if col is None else c, t), st


@pytest.mark.parametrize("case", cc.MERGE_CASES, ids=repr)
def test_host_clustering_is_the_statement(case):
    """clean.cpp's merge_close alone: the targets, or the error the case names."""
    if case.error is not None:
        with pytest.raises(ScanfuseError) as e:
            meshclean.clean_probe_merge(case.pos, case.r)
        assert e.value.code == case.error
        with pytest.raises(ScanfuseError) as e:
            meshclean.clean(Mesh.from_arrays(case.pos, np.zeros((0, 3), np.uint32)), float(case.r), 0)
        assert e.value.code == case.error
        return
    got = meshclean.clean_probe_merge(case.pos, case.r)
    want = stated_target(case.name)
    assert got.dtype == want.dtype and np.array_equal(got, want), np.nonzero(got != want)[0][:8]


@pytest.mark.parametrize("case", OK_MERGE, ids=repr)
def test_restatement_clustering_is_the_statement(case):
    got = clean_oracle.merge_close_vertices(case.pos, float(case.r))
    assert np.array_equal(got, stated_target(case.name)), np.nonzero(got != stated_target(case.name))[0][:8]


def test_cases_reach_what_they_are_named_for():
    """The statement's own figures on the cases: chain depths, who wins, both verdicts of every neighbour pair, runs of equal positions."""
    assert stated_target("chain7").tolist() == [0, 0, 2, 2, 4, 4, 6]
    for name, depth in (("chain130", 129), ("chain130-reversed", 129), ("apart130", 0), ("chain130-evens-first", 1)):
        assert stated_depth(name) == depth
        assert (cx.lower_sets(cc.by_name(name).pos, cc.R)[1] == np.arange(130)).all() == (depth == 129)
    assert stated_target("two-centres").tolist() == [0, 1, 0, 3, 4, 3]
    assert stated_target("absorbed-neighbour-only").tolist() == [0, 0, 2]
    assert stated_target("coincident").tolist() == [0, 0, 0, 3, 3, 5, 3]
    for name in ("cells", "cells-mirrored", "cells-at-8m", "cells-at-minus-8m"):
        t = stated_target(name).reshape(-1, 2, 2)                  # (pair of meshes, under / over, neighbour / anchor)
        assert (t[:, 0, 1] == t[:, 0, 0]).all() and (t[:, 1, 1] != t[:, 1, 0]).all() and len(t) == 6 * 4 * 26
    for name in ("keys-2300m-x", "keys-minus-2300m-y", "keys-2300m-xyz"):
        merged = stated_target(name) != np.arange(len(cc.by_name(name).pos))
        assert merged.reshape(-1, 5).tolist() == [[False, True, False, True, False]] * (len(merged) // 5)
    assert stated_target("keys-alias-bits-60-62").tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert np.bincount(np.bincount(stated_target("r0-runs-1-2-70"), minlength=102))[[1, 2, 70]].tolist() == [30, 1, 1]
    assert stated_target("r0-subnormals").tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 1, 6, 0]
    assert stated_target("r0-signed-zeros").tolist() == [0, 0, 2, 2, 4, 4, 6, 6]
    for name, where in (("count-lanes-from-64", [64, 127, 128, 255]), ("count-last-partial-wave", [321, 329])):
        assert np.nonzero(stated_target(name) != np.arange(len(stated_target(name))))[0].tolist() == where


def test_disagreement_pairs_against_exact_arithmetic():
    """At least 32 pairs each way and against each alternative; numpy's float32 arithmetic is the kernel's order, step by step."""
    batch, k = stated_target("rounding"), 0
    pos = cc.by_name("rounding").pos
    for key in sorted(cc.ROUNDING_PAIRS, key=str):
        alt, kernel_says = key
        pairs = cc.ROUNDING_PAIRS[key]
        assert len(pairs) >= 32, (key, len(pairs))
        for p0, p1 in pairs:
            assert np.array_equal(pos[k], p0) and np.array_equal(pos[k + 1], p1)
            dk, da = cx.dist_as(p0, p1, cx.KERNEL), cx.dist_as(p0, p1, alt)
            assert dk.tobytes() == cx.dist_rows(p0, p1[None])[0].tobytes()
            assert bool(dk < cc.R) == kernel_says and bool(da < cc.R) != kernel_says
            assert batch[k] == k and batch[k + 1] == (k if kernel_says else k + 1)
            mesh = np.array([p0, p1], np.float32)
            assert cx.cluster(mesh, cc.R, alt).tolist() == ([0, 1] if kernel_says else [0, 0])
            k += 2
    assert k == len(pos)


def test_round32_rounds_once_to_nearest_even():
    from fractions import Fraction as Fr
    one, eps = Fr(1), Fr(1, 2 ** 23)
    for q, want in ((one + eps / 2, 1.0), (one + 3 * eps / 2, 1.0 + 2 * 2.0 ** -23), (one + eps / 2 + Fr(1, 2 ** 80), 1.0 + 2.0 ** -23),
                    (Fr(1, 2 ** 150), 0.0), (Fr(3, 2 ** 150), 2.0 ** -148), (Fr(1, 3), float(np.float32(1) / np.float32(3)))):
        assert float(cx.round32(q)) == want


@pytest.mark.parametrize("w", WHOLE, ids=lambda w: w[0])
def test_host_filter_and_restatement_on_whole_cases(w):
    """sf_mesh_clean's arrays and every statistic, clean_oracle.clean's arrays, and the statement's stages composed: all the statement's whole."""
    name, pos, col, tri, r, mf = w
    sx, sc, stri, sst, _ = stated_whole(name)
    got, st = host_clean(pos, col, tri, r, mf)
    _arrays_same(got, (sx, sc, stri), name)
    assert st == sst and tuple(st) == cx.STATS, (st, sst)
    ox, oc, ot = clean_oracle.clean(pos, col, tri, float(r), mf)
    _arrays_same((ox, oc, ot), (sx, sc, stri), name + " restated")
    cpos, ccol, ctri, cst = cc.run_stages(STATEMENT_STAGES, pos, col, tri, r, mf)
    _arrays_same((cpos, ccol, ctri), (sx, sc, stri), name + " composed")
    assert cst == sst


def _on_distinct_vertices(tri):
    nv = int(np.asarray(tri).max()) + 1
    return np.stack([np.arange(nv), np.zeros(nv), np.zeros(nv)], 1).astype(np.float32)


@pytest.mark.parametrize("case", [c for c in cc.FACE_CASES if c.target is None and c.nv < 10 ** 6], ids=repr)
def test_host_filter_on_the_face_cases(case):
    pos = _on_distinct_vertices(case.tri)
    want = cx.clean(pos, None, case.tri, 0, 0)
    got, st = host_clean(pos, None, case.tri, 0, 0)
    _arrays_same(got, want[:3], case.name)
    assert st == want[3] and (st["faces_degenerate"], st["faces_duplicate"]) == tuple(cx.faces(case.tri)[k] for k in ("degenerate", "duplicate"))


@pytest.mark.parametrize("case", cc.COMP_CASES, ids=repr)
def test_host_filter_on_the_component_cases(case):
    pos = _on_distinct_vertices(case.tri)
    want = cx.clean(pos, None, case.tri, 0, case.min_faces)
    got, st = host_clean(pos, None, case.tri, 0, case.min_faces)
    _arrays_same(got, want[:3], case.name)
    assert st == want[3]


def test_component_cases_reach_what_they_are_named_for():
    c = cx.components(cc.by_name("fan300").tri, 7)
    assert c["counters"].tolist() == [1, 0, 0] and (c["root"] == 0).all() and (c["size"] == 300).all()
    for name in ("strip2000-shuffled", "strip2000-reversed", "strip2000"):
        c = cx.components(cc.by_name(name).tri, cc.by_name(name).min_faces)
        assert (c["root"] == 0).all() and c["keep"].all() == (name != "strip2000-reversed")
    c = cx.components(cc.by_name("grids-touching-in-a-vertex").tri, 19)
    assert sorted(set(c["root"].tolist())) == [0, 18] and not c["keep"].any()
    for m, removed in ((0, 0), (1, 0), (2, 1), (6, 1), (7, 2), (8, 3), (9, 4)):
        assert cx.components(cc.by_name("sizes-6-7-8-1-min%d" % m).tri, m)["counters"].tolist()[:2] == [4, removed]
    assert cx.components(cc.by_name("islands257").tri, 1)["counters"].tolist() == [257, 0, 0]
    assert cx.components(cc.by_name("islands257-min2").tri, 2)["counters"].tolist() == [257, 257, 257]
    for name in ("third-edge-of-one", "third-edge-of-both"):
        assert cx.components(cc.by_name(name).tri, 2)["root"].tolist() == [0, 0]
