"""The checker of the GPU decimation, stage by stage (oracle/simplify_rounds_oracle.c: or_simplify_stage_edges / _winners / _collapse), against the
independent statement tests/simplify_exact.py on every case of tests/simplify_cases.py -- the CPU half of tests/test_simplify_stages.py, whose
docstring carries the figures measured here (python -m tests.test_simplify_stages_cpu prints them).  Nothing in this module touches the device."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import simplify_cases as sc
from tests import simplify_exact as sx

# Measured on the CPU, checker against statement, over ALL_CASES (the largest deviation and the case it came from); the bounds are 4 x these.
#   Q     an entry of a vertex quadric against the rational one, relative to the largest entry of its group (A, b or c) at that vertex; exact
#         cases must agree to the bit, the others differ by the rounding of d / |d| on edges that are not unit axis steps and of weight / 100
#   X     a coordinate of the position against the exact minimiser rounded to binary32, relative to the bounding-box diagonal
#   PRI   the binary32 priority against the statement's, evaluated at the SAME binary32 position, relative -- on the edges where Q(x) does not cancel
#   EVAL  the same on the edges where it does (simplify_exact.priority says which: the exact Q(x) is below 2^-29 of the sum of its terms' magnitudes,
#         as on every flat part, so the binary64 evaluation errs by more than binary32 resolves): the deviation in units of one binary64 rounding of
#         that sum (carried through the scale and the quality divisor) plus one binary32 rounding of the priority
Q_MEASURED = 5.44e-16        # cube-planar1-bw2-opt0-thr0
X_MEASURED = 7.51e-15        # fan200-hub-v1: a coordinate of 1e-14 against 0; every other position is the same binary32 number
PRI_MEASURED = 1.00e-06      # fan200-hub-v1: the face quality is binary32 arithmetic
EVAL_MEASURED = 0.143        # crease5x5
Q_TOL, X_TOL, PRI_TOL, EVAL_TOL = 4 * Q_MEASURED, 4 * X_MEASURED, 4 * PRI_MEASURED, 4 * EVAL_MEASURED
UNSURE_CAP = 0.03            # of a case's edges; 0 on the lattice and closed cases
UNSURE_MEASURED = 0.0        # no case has an unsure edge

STAGES = (orc.simplify_stage_edges, orc.simplify_stage_winners, orc.simplify_stage_collapse)


@functools.lru_cache(None)
def checker_edges(name):
    c = sc.by_name(name)
    return orc.simplify_stage_edges(c.pos, c.tri, c.alive, **c.oracle_kw)


@functools.lru_cache(None)
def statement(name):
    """What the statement says of a case's first round: quadrics, and per edge (v0, v1) -> placement, link verdict.  Shared by the CPU and GPU tests."""
    c = sc.by_name(name)
    faces = sx.live_faces(c.tri, c.alive)
    Q = sx.quadrics(c.pos, c.tri, c.alive, c.params["boundary_weight"], c.params["planar_quadric"])
    nb = sx.neighbours(faces)
    edges = sorted({(min(t[j], t[(j + 1) % 3]), max(t[j], t[(j + 1) % 3])) for t in faces for j in range(3)})
    wf = sx.well_formed(faces)
    place, link = {}, {}
    for v0, v1 in edges:
        if c.params["optimal_placement"]:
            place[(v0, v1)] = sx.placement(sx.q_sum(Q, v0, v1), c.pos[v0], c.pos[v1])
        if wf:
            link[(v0, v1)] = sx.link_accepts(faces, nb, v0, v1)
    at = {}
    for t in faces:
        for v in t:
            at.setdefault(v, []).append(t)
    return {"faces": faces, "at": at, "Q": Q, "edges": edges, "place": place, "link": link, "well_formed": wf, "scale": sx.scale_factor(c.pos)}


def against_statement(c, ed):
    """Hold one edges-stage result (the checker's or the kernels') to the statement -> the figures {"q", "x", "pri", "eval", "unsure"}; raises on what must be exact."""
    st = statement(c.name)
    diag = float(np.linalg.norm(c.pos.max(0) - c.pos.min(0)))
    ends = [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in ed["ukey"]]
    assert ends == st["edges"], "the edges are not the unique edges of the live faces in key order"
    cnt = sx.edge_face_counts(st["faces"])
    assert [int(n) for n in ed["ucnt"]] == [cnt[frozenset(e)] for e in ends]
    fig = {"q": 0.0, "x": 0.0, "pri": 0.0, "eval": 0.0, "unsure": 0.0}
    for v in range(len(c.pos)):
        want = st["Q"].get(v, [0] * 10)
        got = ed["Q"][v]
        if c.exact_q:
            assert np.array_equal(np.array([float(w) for w in want]).view(np.uint64), got.view(np.uint64)), "quadric of vertex %d is not the exact one" % v
            continue
        for lo, hi in ((0, 6), (6, 9), (9, 10)):
            ref = max(abs(float(w)) for w in want[lo:hi])
            for i in range(lo, hi):
                dev = abs(sx.Fr(float(got[i])) - want[i])
                if dev:
                    fig["q"] = max(fig["q"], float(dev / sx.Fr(ref)) if ref else float("inf"))
    unsure = 0
    for e, (v0, v1) in enumerate(ends):
        x = ed["x"][e]
        if c.params["optimal_placement"]:
            want, how, uns = st["place"][(v0, v1)]
            if uns:
                unsure += 1
                continue
            wf32 = np.array([float(w) for w in want], np.float64).astype(np.float32)
            fig["x"] = max(fig["x"], float(np.abs(x.astype(np.float64) - wf32.astype(np.float64)).max()) / diag)
        else:
            assert np.array_equal(x.view(np.uint32), c.pos[v1].view(np.uint32)), "without optimal placement the vertex goes to v1"
        if st["well_formed"]:
            assert bool(np.isinf(ed["pri"][e])) == (not st["link"][(v0, v1)]), "link rule: edge (%d, %d) %s" % (v0, v1, "accepted" if st["link"][(v0, v1)] else "rejected")
        if np.isinf(ed["pri"][e]):
            continue
        # the quadric the stage itself summed, so that what is measured is the priority arithmetic alone
        q = [sx.Fr(float(a)) + sx.Fr(float(b)) for a, b in zip(ed["Q"][v0], ed["Q"][v1])] if not c.exact_q else sx.q_sum(st["Q"], v0, v1)
        want, worst, slack, cancels = sx.priority(q, x, c.pos, st["at"][v0] + st["at"][v1], v0, v1, c.params["quality_thr"], st["scale"])
        got = sx.mpmath.mpf(float(ed["pri"][e]))
        if cancels:
            fig["eval"] = max(fig["eval"], float(abs(got - want) / (slack * 2.0 ** -53 + want * 2.0 ** -24)))
        else:
            fig["pri"] = max(fig["pri"], float(abs(got - want) / want))
    fig["unsure"] = unsure / max(1, len(ends))
    return fig


def check_figures(c, fig):
    assert fig["unsure"] <= (0.0 if c.closed_or_lattice else UNSURE_CAP), fig
    assert fig["q"] <= Q_TOL and fig["x"] <= X_TOL and fig["pri"] <= PRI_TOL and fig["eval"] <= EVAL_TOL, fig


NOT_SOUP = [c for c in sc.ALL_CASES if not c.soup]


@pytest.mark.parametrize("case", NOT_SOUP, ids=repr)
def test_checker_edges_stage_meets_the_statement(case):
    check_figures(case, against_statement(case, checker_edges(case.name)))


def test_named_branches_of_the_edges_stage():
    """The branches the cases are there for are really taken, on the checker (the kernels are then held to it bit for bit)."""
    ed = checker_edges("flat4x4")
    assert (ed["x"][:, 2] == 0.0).all(), "a flat grid's positions lie on the plane to the last bit"
    st = statement("flat4x4")
    for e in np.nonzero(np.isfinite(ed["pri"]))[0]:      # every priority at the floor: the error at the kernel's own position is exactly 0
        v0, v1 = st["edges"][e]
        assert sx.q_value(sx.q_sum(st["Q"], v0, v1), [sx.Fr(float(t)) for t in ed["x"][e]]) == 0 and 0 < ed["pri"][e] <= np.float32(1e-14)
    interior = (5, 6, 9, 10)      # away from the border quadrics the summed quadric is the plane's alone
    assert {st["place"][e][1] for e in st["edges"] if e[0] in interior and e[1] in interior} == {"rank1"}
    st = statement("crease5x5")
    assert {"rank1", "rank2"} <= {how for _, how, _ in st["place"].values()}
    assert "full" in {how for _, how, _ in statement("rough12")["place"].values()}
    for name, spokes_rejected in (("fan48-hub-v0", False), ("fan49-hub-v0", True), ("fan48-hub-v1", False), ("fan49-hub-v1", False), ("fan200-hub-v1", False)):
        c, ed = sc.by_name(name), checker_edges(name)
        n = len(c.tri)
        hub = 0 if name.endswith("v0") else n
        spoke = np.array([hub in ((int(k) >> 32), int(k) & 0xFFFFFFFF) for k in ed["ukey"]])
        assert spoke.sum() == n and np.isinf(ed["pri"][spoke]).all() == spokes_rejected and np.isinf(ed["pri"][spoke]).any() == spokes_rejected, name
        assert np.isfinite(ed["pri"][~spoke]).all(), "rim edges are unaffected"
    ed = checker_edges("strip3")      # interior edges of a strip one quad wide: accepted only through the neighbour found as `prv`
    assert np.isfinite(ed["pri"][ed["ucnt"] == 2]).all() and (ed["ucnt"] == 2).sum() == 5
    ed = checker_edges("collinear-opt0")
    e = [int(k) for k in ed["ukey"]].index((0 << 32) | 3)
    assert ed["pri"][e] == np.float32(3.0e38) and ed["tau"] == np.float32(3.0e38)
    assert checker_edges("strip32-E129-V66")["E"] == 129 and checker_edges("fan64-E128-V65")["E"] == 128
    assert [len(sc.by_name(n).pos) for n in ("grid17x15-V255", "grid16x16-V256", "grid16x16-ear-V257")] == [255, 256, 257]


def test_nan_guard_of_the_placement():
    """Coordinates of 1e25 (simplify_cases.HUGE): the adjugate products of the solve overflow.  Where they give inf - inf the guard takes the best of the
    midpoint and the two end points by Q -- the position is then one of the three as binary32 and the priority is an ordinary finite one; the guard IS
    reachable from finite input.  Where they give a plain inf the guard does not apply and the position is not finite; on these two meshes the priority
    is then NaN or +inf, never a candidate, so no collapse carries such a position into the mesh.  That is an observation on these inputs, not a
    property of the rule: DESIGN.md section 3.9 states the limit (coordinates beyond 1e24)."""
    guarded = infinite = 0
    unit = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32) * np.float32(1e25)      # this one overflows to plain inf
    for pos, tri in (sc.HUGE, (unit, sc.HUGE[1])):
        ed = orc.simplify_stage_edges(pos, tri)
        for e, k in enumerate(ed["ukey"]):
            v0, v1 = int(k) >> 32, int(k) & 0xFFFFFFFF
            mid = (0.5 * (pos[v0].astype(np.float64) + pos[v1].astype(np.float64))).astype(np.float32)
            x = ed["x"][e]
            assert not np.isnan(x).any()
            if not np.isfinite(x).all():
                infinite += 1
                assert not ed["pri"][e] <= np.float32(3.0e38), "a candidate with a position that is not finite"
            elif any(np.array_equal(x, p) for p in (mid, pos[v0], pos[v1])):
                guarded += 1
                q = [sx.Fr(float(a)) + sx.Fr(float(b)) for a, b in zip(ed["Q"][v0], ed["Q"][v1])]
                val = [sx.q_value(q, [sx.Fr(float(t)) for t in p]) for p in (x, mid, pos[v0], pos[v1])]
                assert val[0] == min(val), "the guard did not take the best of the three"
    assert guarded == 9 and infinite == 9, (guarded, infinite)


@pytest.mark.parametrize("wc", sc.winner_cases(), ids=lambda w: w[0])
def test_checker_winners_stage_meets_the_rule(wc):
    name, (pos, tri), pri, tau, rnd = wc
    alive = np.ones(len(tri), np.uint8)
    ed = orc.simplify_stage_edges(pos, tri, alive)
    assert ed["E"] == len(pri)
    w = orc.simplify_stage_winners(len(pos), tri, alive, pri, tau, rnd)
    winners = sx.check_winners(len(pos), tri, alive, ed["ukey"], ed["ucnt"], pri, np.float32(tau), rnd, w["passes"], w["taken"], w["counters"])
    want = {"islands-no-candidate": 0, "islands-one-winner-in-wave-0": 1, "islands-32-winners-in-wave-0": 32, "islands96-64-winners-in-one-wave": 64, "islands-winners-only-in-the-last-partial-wave": 10,
            "islands-every-edge-tied": 70}.get(name)
    if want is not None:
        assert len(winners) == want
    if name == "islands96-64-winners-in-one-wave":
        assert winners == list(range(192, 256)), "one whole wave of k_winners: lanes 0 .. 63 of the fourth"
    if name == "islands-32-winners-in-wave-0":
        assert all(e < 64 for e in winners)
    if name == "islands-winners-only-in-the-last-partial-wave":
        assert all(e >= 192 for e in winners)


@pytest.mark.parametrize("case", sc.STAGE_CASES, ids=repr)
def test_checker_winners_and_collapse_on_the_cases_own_priorities(case):
    """The winner rule on the priorities the edges stage gave (rounds 0 and 1), and the collapse of those winners against the direct statement."""
    ed = checker_edges(case.name)
    assert ed["E"] > 0
    for rnd in (0, 1):
        w = orc.simplify_stage_winners(len(case.pos), case.tri, case.alive, ed["pri"], ed["tau"], rnd)
        ids = sx.check_winners(len(case.pos), case.tri, case.alive, ed["ukey"], ed["ucnt"], ed["pri"], ed["tau"], rnd, w["passes"], w["taken"], w["counters"])
        got = orc.simplify_stage_collapse(case.pos, case.tri, case.alive, ed["Q"], ids, ed["x"])
        want = sx.collapse(case.pos, case.tri, case.alive, ed["Q"], ed["ukey"], ids, ed["x"])
        for k in ("pos", "tri", "alive", "Q", "vdel"):
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (k, rnd)


@pytest.mark.parametrize("name", ["grid5x4-planar0-bw1-opt1-thr0.3", "rough12", "bumpy12-checker-only", "crease5x5", "fan64-E128-V65", "strip32-E129-V66"])
def test_one_rounds_winners_do_not_change_each_other(name):
    """The independence claim itself: collapse one round's winners one at a time, in two different orders; after each collapse the edges stage of the
    intermediate mesh gives every REMAINING winner the same priority, position and link verdict, to the bit."""
    c, ed = sc.by_name(name), checker_edges(name)
    w = orc.simplify_stage_winners(len(c.pos), c.tri, c.alive, ed["pri"], ed["tau"], 0)
    ids = [int(e) for e in np.nonzero(w["passes"])[0]]
    assert len(ids) >= 2
    key_of = {e: int(ed["ukey"][e]) for e in ids}
    for order in (ids, ids[::-1]):
        pos, tri, alive, Q = c.pos, c.tri, c.alive, ed["Q"]
        cur, left = ed, list(order)
        while left:
            e = left.pop(0)
            now = [int(k) for k in cur["ukey"]].index(key_of[e])
            got = orc.simplify_stage_collapse(pos, tri, alive, Q, [now], cur["x"])
            pos, tri, alive, Q = got["pos"], got["tri"], got["alive"], got["Q"]
            if not left:
                break
            cur = orc.simplify_stage_edges(pos, tri, alive, Q, scale=ed["scale"], **c.oracle_kw)
            keys = [int(k) for k in cur["ukey"]]
            for r in left:
                j = keys.index(key_of[r])
                assert cur["pri"][j:j + 1].view(np.uint32)[0] == ed["pri"][r:r + 1].view(np.uint32)[0], (e, r)
                assert np.array_equal(cur["x"][j].view(np.uint32), ed["x"][r].view(np.uint32)), (e, r)
                assert cur["ucnt"][j] == ed["ucnt"][r]


@pytest.mark.parametrize("case", sc.SOUP_CASES, ids=repr)
def test_soups_run_through_the_checker(case):
    """Soups are held to the checker alone (the link test counts per corner, which is the count of distinct common neighbours only where every edge has
    at most two consistently oriented faces); here: the stages terminate and stay in range on them."""
    ed = checker_edges(case.name)
    assert ed["E"] > 0
    if case.name in ("soup-three-faces-on-an-edge", "soup-face-twice"):
        assert not sx.well_formed(sx.live_faces(case.tri, case.alive))
    if case.name == "soup-flipped-pair":      # two faces on every edge, and a third "common neighbour" that is the opposite vertex of both: rejected
        assert np.isinf(ed["pri"]).all()
    assert not np.isnan(ed["pri"]).any() and np.isfinite(ed["x"]).all()


def test_whole_runs_of_the_checker_are_the_composition_of_its_stages():
    """or_simplify_rounds against the stage calls driven round by round (simplify_cases.run_rounds), and the two named paths of the round loop: a budget
    that cuts inside the last round's winners, dead faces squeezed out before the last round.  Also the soups that stall."""
    for name, (pos, tri), target in sc.whole_run_cases():
        p, t, alive, vdel, log = sc.run_rounds(STAGES, pos, tri, target)
        ox, _, ot, ost = orc.simplify_rounds(pos, tri, target_perc=0.0, target_faces=target, auto_clean=0)
        assert ost["rounds"] == len(log) and ost["collapses"] == sum(r["take"] for r in log), (name, log)
        assert np.array_equal(ox.view(np.uint32), p[vdel == 0].view(np.uint32)), name
        remap = np.cumsum(vdel == 0) - 1
        assert np.array_equal(ot, remap[t[alive != 0]]), name
        if name.endswith("cut"):
            assert 0 < log[-1]["take"] < log[-1]["winners"], log
        else:
            assert any(r["squeezed"] for r in log[:-1]) and len(log) >= 2, log
    # the flipped pair: every edge has two faces that the link test rejects; two rounds without winners, no collapse
    c = sc.by_name("soup-flipped-pair")
    st = orc.simplify_rounds(c.pos, c.tri, target_perc=0.0, target_faces=1)[3]
    assert (st["rounds"], st["collapses"]) == (2, 0)
    log = sc.run_rounds(STAGES, c.pos, c.tri, 1)[4]
    assert [r["winners"] for r in log] == [0, 0]
    # a tetrahedron to one face: three rounds and one collapse
    st = orc.simplify_rounds(*sc.TETRA, target_perc=0.0, target_faces=1)[3]
    assert (st["rounds"], st["collapses"]) == (3, 1)


# ---- the host filter's numbers for the same edges (simplify.cpp through sf_simplify_probe_edge) -----------------------------------------------------
def host_probe(case, v0, v1):
    from scannet_amd import _abi, meshclean
    from scannet_amd.segmentator import Mesh
    L = _abi.lib()
    p = meshclean._stage_params(case.params)
    L.sf_simplify_probe_edge.argtypes = [C.c_void_p, C.POINTER(meshclean.SfSimplifyParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float),
                                         C.POINTER(C.c_double)]
    if not hasattr(case, "_mesh"):
        case._mesh = Mesh.from_arrays(case.pos, case.tri)
    q, x, pri, scale = np.zeros(10, np.float64), np.zeros(3, np.float32), C.c_float(0), C.c_double(0)
    _abi.check(L.sf_simplify_probe_edge(case._mesh._h, C.byref(p), v0, v1, q.ctypes.data, x.ctypes.data, C.byref(pri), C.byref(scale)))
    return q, x, np.float32(pri.value), scale.value


def against_host(case, ed):
    """Every edge the link test accepts: Q(v0) + Q(v1), position and priority equal the host filter's, bit for bit (both compile simplify_math.h with
    contraction off, and the host adds a vertex's face quadrics in the same order)."""
    for e in np.nonzero(np.isfinite(ed["pri"]))[0]:
        v0, v1 = int(ed["ukey"][e]) >> 32, int(ed["ukey"][e]) & 0xFFFFFFFF
        q, x, pri, scale = host_probe(case, v0, v1)
        assert scale == ed["scale"]
        assert np.array_equal((ed["Q"][v0] + ed["Q"][v1]).view(np.uint64), q.view(np.uint64)), "summed quadric of edge (%d, %d)" % (v0, v1)
        assert np.array_equal(ed["x"][e].view(np.uint32), x.view(np.uint32)), "position of edge (%d, %d): %s, host %s" % (v0, v1, ed["x"][e], x)
        assert ed["pri"][e] == pri, "priority of edge (%d, %d): %r, host %r" % (v0, v1, ed["pri"][e], pri)


HOST_CASES = [c for c in sc.ALL_CASES if not c.soup and c.alive.all()]


@pytest.mark.parametrize("case", HOST_CASES, ids=repr)
def test_checker_first_round_equals_the_host_filter(case):
    against_host(case, checker_edges(case.name))


if __name__ == "__main__":
    worst = {"q": (0.0, None), "x": (0.0, None), "pri": (0.0, None), "eval": (0.0, None), "unsure": (0.0, None)}
    for case in NOT_SOUP:
        f = against_statement(case, checker_edges(case.name))
        for k, v in f.items():
            if v > worst[k][0]:
                worst[k] = (v, case.name)
    print(worst)
