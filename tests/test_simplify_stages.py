"""The GPU decimation, kernel by kernel (scannet_amd/csrc/simplify_gpu.hip: the quadric edge collapse as rounds of independent collapses).

Three parties:
  * the HIP kernels through the stage hooks of include/scanfuse_internal.h (meshclean.stage_edges / stage_winners / stage_collapse), which launch them
    through the helpers the round loop of sf_mesh_simplify_gpu itself calls;
  * the checker oracle/simplify_rounds_oracle.c, split the same way (or_simplify_stage_edges / _winners / _collapse; or_simplify_rounds is their
    composition), which the kernels are held to bit for bit on every case;
  * tests/simplify_exact.py, an independent statement: rational arithmetic for the quadrics, the full-rank and the rank-1 / rank-2 minimisers, mpmath
    where a root or an eigen-decomposition enters, the link rule as sets, the winner rule by brute force over all pairs, the collapse stated directly.

CPU half (tests/test_simplify_stages_cpu.py, default suite): the checker's stages against the statement on every case, the independence of one round's
winners (collapsed one at a time in two orders, the remaining winners' priority, position and link verdict unchanged to the bit), the whole run as the
composition of the stages, the host filter's numbers for the first round.  This module (-m gpu): every case through the hooks against the checker's
stage bit for bit; the exact cases against the statement too; the first round against the host filter (sf_simplify_probe_edge); whole runs through
the product against the checker, with the round log taken through the stage calls.

Margins, measured on the CPU between checker and statement over all cases (never against device output); every bound is 4 x the figure:
  quadric entries (cases that are not exact: diagonal or non-unit border edges, planar_quadric's weight / 100)   5.44e-16 -> 2.2e-15 of the largest entry
  position (a coordinate against the exact minimiser rounded to binary32, of the bounding-box diagonal)        7.51e-15 -> 3.0e-14
  priority where Q(x) does not cancel (relative, at the kernel's own binary32 position)                        1.00e-06 -> 4.0e-06
  priority where Q(x) cancels (flat parts; in units of one binary64 rounding of the terms of Q(x) plus one binary32 rounding of the result)  0.143 -> 0.57
  unsure edges (det / trace^3 within a factor 2 of 1e-6, an eigenvalue ratio within a factor 10 of 1e-9)       none in any case; cap 3 %, 0 on lattices
Exact cases (integer coordinates, unit axis-aligned border edges, no planar_quadric): the kernels' binary64 quadrics equal the rational ones to the bit.

What the statement says differently from the text of the issue that asked for it: the floor 1e-15 applies to scale * Q(x), not to Q(x) -- VCG's
QuadricEpsilon, what the host filter, the kernel and the checker all do, and what "every priority of a flat grid sits at the floor" requires.
meshes.bumpy(12) is held to the checker alone: a third of its edges sit within a factor 2 of the det rule (unsure); tests/simplify_cases.rough(12) is the
full-rank case.  64 winners in one wave: the third edges of 96 separate triangles are neighbours in key order and do not conflict; edges 192 .. 255
fill one wave of k_winners and all win.  The NaN guard of optimal_position IS reachable from finite input (coordinates of 1e25: the adjugate products
overflow); the case is kept.

Soups (three faces on an edge, a face twice, a flipped pair) and dead faces are held to the checker alone: the link test counts per corner, which is
the count of distinct common neighbours only where every edge has at most two consistently oriented faces.

One-line mutations of simplify_gpu.hip (values and predicates only, never an address, a bound or a loop), each built into a scratch copy of the
library and run under this module on the device; the tests that failed under it (counts are test ids of this module, 246 in all):
   1. border weight without its 0.5                 103: test_gpu_edges_stage on every open mesh (grids, strips, fans, soups), test_gpu_first_round_equals_the_host_filter
   2. off-border weight without / 100               80: test_gpu_edges_stage[*-planar1-*] and test_gpu_first_round_equals_the_host_filter[*-planar1-*], all forty each
   3. border test == 1 turned into >= 1             201: test_gpu_edges_stage on every case but the planar_quadric ones of open meshes, the host cross-check,
                                                    test_gpu_nan_guard_of_the_placement
   4. MAX_RING 96 turned into 94                    1: test_gpu_edges_stage[fan48-hub-v0] -- 96 entries, the only case at the limit
   5. the prv candidate dropped                     54: test_gpu_edges_stage[strip3], [strip32-E129-V66], [grid3x3-*], [grid5x4-*], every mesh with a border vertex
   6. the cand == v0 skip dropped                   none, and none can: the ring of v0 is gathered from v0's faces without v0 itself (`t[k] != a`), and a face
                                                    that names a vertex twice is never live, so v0 is never found in its own ring and the skipped candidate would
                                                    add 0 to `common`.  The skip saves the search, it changes no value.
   7. the clamp of min_qual to quality_thr dropped  111: test_gpu_edges_stage[*-thr0.3] and every default case, the host cross-check
   8. the floor 1e-15 turned into 1e-16             34: test_gpu_edges_stage[flat4x4], [crease5x5], [strip3], [strip32-E129-V66], the flat-bordered grids, the host cross-check
   9. mid taken as p0                               26: test_gpu_edges_stage[flat4x4], [crease5x5], [strip*], [soup-flipped-pair], the host cross-check, the NaN guard
  10. the lock key without its salt                 24: test_gpu_winners_stage[*-every-edge-tied*], [grid9x8-mixed-*], test_gpu_winners_and_collapse (round 1, and
                                                    passes 2 and 3 of round 0; pass 1 of round 0 has salt 0 and cannot show it)
  11. k_lock without the taken test                 40: test_gpu_winners_stage, all but [islands-no-candidate] (a winner wins again in the next pass)
  12. && turned into || in k_winners                26: test_gpu_winners_stage[grid9x8-*], [fan64-every-edge-tied], test_gpu_winners_and_collapse
  13. the face counter adding 2 instead of ucnt[e]  31: test_gpu_winners_stage[islands*] (one face per edge; the full wave of islands96 among them), [grid9x8-*], [fan64-*], test_gpu_winners_and_collapse
  14. k_collapse leaving Q[v1] unsummed             30: test_gpu_winners_and_collapse, every case with a winner; test_gpu_whole_runs_through_the_product
  15. k_collapse leaving alive of a shared face set 30: the same"""
import numpy as np
import pytest

from oracle import oracle as orc
from scannet_amd import meshclean
from scannet_amd.segmentator import Mesh
from tests import simplify_cases as sc
from tests import simplify_exact as sx
from tests import test_simplify_stages_cpu as cpu

pytestmark = pytest.mark.gpu

GPU_STAGES = (meshclean.stage_edges, meshclean.stage_winners, meshclean.stage_collapse)


def _same(got, want, what):
    """two stage results agree in every field, to the bit"""
    assert set(got) == set(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        same = np.array_equal(np.atleast_1d(g).view(np.uint8), np.atleast_1d(w).view(np.uint8))
        assert same, "%s: %s differs at %s" % (what, k, np.argwhere(np.atleast_1d(g != w))[:5].tolist())


def _gpu_edges(case, **kw):
    return meshclean.stage_edges(case.pos, case.tri, case.alive, **dict(case.params, **kw))


@pytest.mark.parametrize("case", sc.ALL_CASES, ids=repr)
def test_gpu_edges_stage(case):
    """k_emit, the sorts, k_vertex_ranges, k_fix_counts, the run-length encode, k_init_quadrics, k_priority and the quantile: the checker's stage to the
    bit; an exact case also the statement."""
    got = _gpu_edges(case)
    _same(got, cpu.checker_edges(case.name), case.name)
    if case.exact_q:
        cpu.check_figures(case, cpu.against_statement(case, got))


@pytest.mark.parametrize("name", ["grid5x4-planar0-bw1-opt1-thr0.3", "rough12", "strip32-E129-V66", "soup-dead-faces"])
def test_gpu_threshold_of_the_edges_stage(name):
    """The quantile: ranks below, at and beyond E - 1, and no threshold after a stalled round; always clamped to 3e38."""
    c = sc.by_name(name)
    E = cpu.checker_edges(name)["E"]
    for needed, stalled in ((0, 0), (1, 0), (2 * (E - 66) // 3, 0), (E, 0), (10 ** 9, 0), (3, 1)):
        needed = max(0, needed)
        got = _gpu_edges(c, needed=needed, stalled=stalled)
        want = orc.simplify_stage_edges(c.pos, c.tri, c.alive, needed=needed, stalled=stalled, **c.oracle_kw)
        _same(got, want, "%s needed %d stalled %d" % (name, needed, stalled))
        assert got["tau"] <= np.float32(3.0e38)
        if stalled:
            assert got["tau"] == np.float32(3.0e38)


@pytest.mark.parametrize("wc", sc.winner_cases(), ids=lambda w: w[0])
def test_gpu_winners_stage(wc):
    """k_lock and k_winners, three passes, on hand-made priorities: the pass each edge won in, the marks and the three counters."""
    name, (pos, tri), pri, tau, rnd = wc
    alive = np.ones(len(tri), np.uint8)
    got = meshclean.stage_winners(len(pos), tri, alive, pri, tau, rnd)
    _same(got, orc.simplify_stage_winners(len(pos), tri, alive, pri, tau, rnd), name)


@pytest.mark.parametrize("case", sc.STAGE_CASES, ids=repr)
def test_gpu_winners_and_collapse(case):
    """On the priorities of the case's own first round, as rounds 0 and 1: the winners, and k_collapse on them -- the checker's stage to the bit and the
    collapse as simplify_exact states it."""
    ed = cpu.checker_edges(case.name)
    for rnd in (0, 1):
        want = orc.simplify_stage_winners(len(case.pos), case.tri, case.alive, ed["pri"], ed["tau"], rnd)
        got = meshclean.stage_winners(len(case.pos), case.tri, case.alive, ed["pri"], ed["tau"], rnd)
        _same(got, want, "%s winners of round %d" % (case.name, rnd))
        ids = np.nonzero(want["passes"])[0]
        got = meshclean.stage_collapse(case.pos, case.tri, case.alive, ed["Q"], ids, ed["x"])
        _same(got, orc.simplify_stage_collapse(case.pos, case.tri, case.alive, ed["Q"], ids, ed["x"]), "%s collapse of round %d" % (case.name, rnd))
        _same(got, sx.collapse(case.pos, case.tri, case.alive, ed["Q"], ed["ukey"], ids, ed["x"]), "%s collapse of round %d, stated" % (case.name, rnd))


@pytest.mark.parametrize("name", ["grid5x4-planar0-bw1-opt1-thr0.3", "rough12", "fan48-hub-v1", "soup-three-faces-on-an-edge"])
def test_gpu_second_round_takes_the_summed_quadrics(name):
    """The edges stage on the mesh one round of collapses leaves, with the quadrics handed in (k_init_quadrics does not run again) and dead faces in place."""
    c, ed = sc.by_name(name), cpu.checker_edges(name)
    w = orc.simplify_stage_winners(len(c.pos), c.tri, c.alive, ed["pri"], ed["tau"], 0)
    m = orc.simplify_stage_collapse(c.pos, c.tri, c.alive, ed["Q"], np.nonzero(w["passes"])[0], ed["x"])
    assert (m["alive"] == 0).any()
    got = meshclean.stage_edges(m["pos"], m["tri"], m["alive"], m["Q"], scale=ed["scale"], needed=2, **c.params)
    _same(got, orc.simplify_stage_edges(m["pos"], m["tri"], m["alive"], m["Q"], scale=ed["scale"], needed=2, **c.oracle_kw), name)


def test_gpu_nan_guard_of_the_placement():
    """Coordinates of 1e25 (tests/test_simplify_stages_cpu.py::test_nan_guard_of_the_placement says what the guard must give, and holds the checker to it)."""
    _same(meshclean.stage_edges(*sc.HUGE), orc.simplify_stage_edges(*sc.HUGE), "1e25")


@pytest.mark.parametrize("case", cpu.HOST_CASES, ids=repr)
def test_gpu_first_round_equals_the_host_filter(case):
    """Every edge the link test accepts: k_init_quadrics' gather and k_priority against the host filter's scatter and its own priority
    (sf_simplify_probe_edge), bit for bit."""
    cpu.against_host(case, _gpu_edges(case))


def _product(pos, tri, **kw):
    out, st = meshclean.simplify(Mesh.from_arrays(pos, tri), gpu=0, **kw)
    x, _, t = out.arrays()
    return x, t, st


def test_gpu_whole_runs_through_the_product():
    """sf_mesh_simplify_gpu against or_simplify_rounds where the round loop takes its named paths, which the round log -- taken through the stage hooks,
    and equal to the one through the checker's stages -- shows it does: a budget that cuts inside the last round's winners (key order), dead faces
    squeezed out before the last round, two rounds without winners (stalled), three rounds for one collapse."""
    for name, (pos, tri), target in sc.whole_run_cases():
        p, t, alive, vdel, log = sc.run_rounds(GPU_STAGES, pos, tri, target)
        cp, ct, calive, cvdel, clog = sc.run_rounds(cpu.STAGES, pos, tri, target)
        assert log == clog, name
        for a, b in ((p, cp), (t, ct), (alive, calive), (vdel, cvdel)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
        if name.endswith("cut"):
            assert 0 < log[-1]["take"] < log[-1]["winners"], log
        else:
            assert any(r["squeezed"] for r in log[:-1]), log
        for clean in (0, 1):
            x, tt, st = _product(pos, tri, target_perc=0.0, target_faces=target, auto_clean=clean)
            ox, _, ot, ost = orc.simplify_rounds(pos, tri, target_perc=0.0, target_faces=target, auto_clean=clean)
            assert (st["rounds"], st["collapses"]) == (ost["rounds"], ost["collapses"]) == (len(log), sum(r["take"] for r in log)), name
            assert np.array_equal(x.view(np.uint32), ox.view(np.uint32)) and np.array_equal(tt, ot), name
            if not clean:
                assert np.array_equal(x.view(np.uint32), p[vdel == 0].view(np.uint32)), name
    for mesh, rounds, collapses in (((sc.by_name("soup-flipped-pair").pos, sc.by_name("soup-flipped-pair").tri), 2, 0), (sc.TETRA, 3, 1)):
        x, tt, st = _product(*mesh, target_perc=0.0, target_faces=1)
        ox, _, ot, ost = orc.simplify_rounds(*mesh, target_perc=0.0, target_faces=1)
        assert (st["rounds"], st["collapses"]) == (ost["rounds"], ost["collapses"]) == (rounds, collapses)
        assert np.array_equal(x.view(np.uint32), ox.view(np.uint32)) and np.array_equal(tt, ot)
        log = sc.run_rounds(GPU_STAGES, *mesh, 1)[4]
        assert len(log) == rounds and sum(r["take"] for r in log if r["winners"]) == collapses
