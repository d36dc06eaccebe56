"""The marching-cubes stage without a GPU: on every case of tests/mc_cases.py
  * oracle/mc_oracle.c's entry over blocks (or_mc_extract_blocks) equals the statement tests/mc_exact.py to the bit: keys, position bits, colours, indices;
  * the independent float64 evaluation oracle/spec_literal_mc.py (with the ownership mask) has exactly the statement's vertex key set and triangle count.
    No cube is flagged or left out: every decision (w > 0, |sdf| <= thresh, sdf < 0) compares the same float32 values in all parties, so there are no
    ties and the share of cases left out is zero;
  * colours lie within 0.5 + 1e-3 levels of the unrounded float64 colour, positions within mc_exact.position_bound(g, voxel) =
    voxel * 2^-24 * (2 + 2(|g| + 1)) * (1 + 2^-20) + 2^-149 per coordinate (derivation: tests/mc_exact.py), which is 9.6e-7 m at |g| = 800, voxel 0.01;
  * what each case expects beyond that (mc_cases.Case.expect): exactly the stated cubes carry triangles, a perturbation drops exactly the cubes that
    touch it and changes no other byte, a ghost's cubes are not meshed and the rest is the all-owned mesh, zero-area triangles are emitted;
  * closure from the mesh arrays alone (no case table): on all-cases every triangle side whose surrounding cubes all carry triangles is matched by
    sides in the opposite direction, one to one (two to two where two sheets touch along a face segment: 0.3 % of the sides);
  * beyond the key range every party refuses the volume, and the arithmetic of the unguarded key shows why: two different grid edges, one key.

Largest deviation of the statement from the float64 evaluation per group of cases, measured (position as a share of the bound / colour levels):
  all-cases 0.775 / 0.50001   gates 0.777 / 0.50000   neighbour 0.731 / 0.50001   zeros 0.741 / 0.49999   colour 0.701 / 0.50000 (all-pairs: 0.5 exactly)
  key-range 0.722 / 0.49999 (|g| = 2^19: 4.5e-4 m of a bound of 6.25e-4 m = 1/16 voxel, float32's ulp there)   prefix 0.698 / 0.49992   dense-checker-3 0.750 / 0.50000
The device-sized dense checker (13^3 blocks on 256 CUs) belongs to the GPU module; here the same builder runs at 3^3 blocks.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import spec_literal_mc as lit
from tests import mc_cases as mc
from tests import mc_exact as mx

U64 = np.uint64
_statement, _oracle = {}, {}


def statement(case):
    if case.name not in _statement:
        _statement[case.name] = mx.mesh(case.coords, case.voxels, case.owned, case.voxel_size, case.thresh_factor)
    return _statement[case.name]


def oracle_mesh(case):
    if case.name not in _oracle:
        _oracle[case.name] = orc.mc_extract_blocks(case.oracle_params(orc), case.coords, case.voxels, case.owned)
    return _oracle[case.name]


def assert_same_mesh(got, want, what, tkeys=True):
    for k in ("keys", "col", "idx") + (("tkeys",) if tkeys and "tkeys" in got and "tkeys" in want else ()):
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
    gp, wp = np.ascontiguousarray(got["pos"], np.float32).view(np.uint32), np.ascontiguousarray(want["pos"], np.float32).view(np.uint32)
    assert np.array_equal(gp, wp), (what, "pos", int((gp != wp).sum()))


def cube_keys(origins):
    return np.unique(mx.edge_key(np.asarray(origins, np.int64).reshape(-1, 3), 0) >> U64(2))


def _triangle_keys(m):
    return m["keys"][m["idx"].astype(np.int64)] if len(m["idx"]) else np.zeros((0, 3), U64)


def _assert_part_of(m, base, keep, what):
    """m is base restricted to base's triangles `keep`: the same triangles by key, and every vertex of m is base's vertex of that key, byte for byte"""
    assert np.array_equal(m["tkeys"], base["tkeys"][keep]), what
    assert np.array_equal(_triangle_keys(m), _triangle_keys(base)[keep]), what
    assert np.array_equal(m["keys"], np.unique(_triangle_keys(base)[keep])), what
    at = np.searchsorted(base["keys"], m["keys"])
    assert np.array_equal(base["keys"][at], m["keys"]), what
    assert np.array_equal(base["pos"][at].view(np.uint32), np.ascontiguousarray(m["pos"], np.float32).view(np.uint32)) and np.array_equal(base["col"][at], m["col"]), what


def check_expectations(case, m, mesh_of):
    """m: dict(keys, pos, col, idx, tkeys) of `case` by some party; mesh_of(base case) the same party's mesh of a base case"""
    e = case.expect
    got = np.unique(m["tkeys"] >> U64(3))
    if "cubes" in e:
        assert np.array_equal(got, cube_keys(e["cubes"])), (case.name, len(got), len(e["cubes"]))
    if e.get("empty"):
        assert len(m["idx"]) == 0 and len(m["keys"]) == 0 and len(m["pos"]) == 0
    if "same_as" in e:
        assert_same_mesh(m, mesh_of(e["same_as"]), case.name)
    if "dropped" in e:
        base, origins = mesh_of(e["dropped"][0]), e["dropped"][1]
        gone = cube_keys(origins)
        assert np.isin(gone, base["tkeys"] >> U64(3)).all() and len(gone) > 0
        _assert_part_of(m, base, ~np.isin(base["tkeys"] >> U64(3), gone), case.name)
        assert np.isfinite(m["pos"]).all()
    if "restrict" in e:
        base, ghosts = mesh_of(e["restrict"][0]), np.asarray(e["restrict"][1], np.int64)
        origin = mx.decode_key((base["tkeys"] >> U64(3)) << U64(2))[0]
        in_ghost = np.zeros(len(origin), bool)
        for gb in ghosts:
            in_ghost |= ((origin >> 3) == gb).all(1)
        assert in_ghost.any() and not in_ghost.all()
        _assert_part_of(m, base, ~in_ghost, case.name)
        mine = mx.decode_key((m["tkeys"] >> U64(3)) << U64(2))[0] >> 3
        for gb in ghosts:
            assert not (mine == gb).all(1).any(), "a cube of a ghost block was meshed"
    if "degenerate" in e:
        for origin in e["degenerate"]:
            tri = np.nonzero((m["tkeys"] >> U64(3)) == cube_keys(origin)[0])[0]
            assert len(tri) >= 1, (case.name, origin)
            for t in tri:
                v = m["idx"][t].astype(np.int64)
                p = np.ascontiguousarray(m["pos"][v], np.float32).view(np.uint32)
                assert (p == p[0]).all() and len(set(m["keys"][v].tolist())) == 3, (case.name, origin, m["pos"][v])


def literal_deviation(case, m):
    """the float64 evaluation against mesh m -> (largest position deviation as a share of the bound, largest colour deviation in levels)"""
    order = np.lexsort((case.coords[:, 2], case.coords[:, 1], case.coords[:, 0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        ev = lit.evaluate(case.coords[order], case.voxels[order], case.voxel_size, case.thresh_factor, mx.NTRI, owned=case.owned[order])
    assert np.array_equal(ev["keys"], m["keys"]), (case.name, len(ev["keys"]), len(m["keys"]))
    assert ev["n_tris"] == len(m["idx"]), (case.name, ev["n_tris"], len(m["idx"]))
    if not len(m["keys"]):
        return 0.0, 0.0
    g, _ = mx.decode_key(m["keys"])
    share = np.abs(m["pos"].astype(np.float64) - ev["pos"]) / mx.position_bound(g, case.voxel_size)
    dcol = np.abs(m["col"].astype(np.float64) - ev["col"])
    assert share.max() <= 1.0, (case.name, share.max())
    assert dcol.max() <= 0.5 + 1e-3, (case.name, dcol.max())
    return float(share.max()), float(dcol.max())


@pytest.mark.parametrize("case", mc.cases(), ids=repr)
def test_oracle_statement_and_literal_agree(case):
    if "key_range" in case.expect:
        axis, bad = case.expect["key_range"]
        for party, err in ((lambda: statement(case), mx.KeyRangeError), (lambda: oracle_mesh(case), orc.KeyRangeError)):
            with pytest.raises(err) as info:
                party()
            assert info.value.block[axis] == bad
        return
    s, o = statement(case), oracle_mesh(case)
    assert_same_mesh(o, s, case.name)
    check_expectations(case, s, statement)
    share, dcol = literal_deviation(case, s)
    print("%s: %d blocks (%d owned), %d vertices, %d triangles; float64 evaluation: position %.3f of the bound, colour %.5f levels"
          % (case.name, len(case.coords), case.owned.sum(), len(s["keys"]), len(s["idx"]), share, dcol))
    if hasattr(case, "edge"):
        key, byte = case.edge
        assert s["col"][np.searchsorted(s["keys"], key), 0] == byte
    if hasattr(case, "n_tris"):
        assert (len(s["idx"]), len(s["keys"])) == (case.n_tris, case.n_verts)


def test_all_cases_reach_every_configuration_in_every_halo_class():
    c = mc.by_name("all-cases")
    assert c.table.shape == (8, 256) and (c.table > 0).all()
    s = statement(c)
    # and the meshed cubes of the statement show it too: the configuration of a cube is not in the mesh, its class and triangle count are
    origin = mx.decode_key((s["tkeys"] >> U64(3)) << U64(2))[0]
    cls = ((origin[:, 0] & 7) == 7) | (((origin[:, 1] & 7) == 7) << 1) | (((origin[:, 2] & 7) == 7) << 2)
    assert (np.bincount(cls, minlength=8) > 254 * 1).all()
    print("all-cases: fewest cubes of one configuration in one class:", int(c.table.min()), "per class:", c.table.min(1))


def assert_closed(m, what):
    n, bad, twice = mx.unclosed_sides(m["keys"], m["idx"], m["tkeys"])
    assert n > 0.9 * 3 * len(m["idx"]), (what, n)
    assert len(bad) == 0, (what, bad[:5])
    assert twice < 0.01 * n, (what, twice, n)
    return n, twice


def test_statement_mesh_of_all_cases_closes():
    n, twice = assert_closed(statement(mc.by_name("all-cases")), "statement")
    print("all-cases: %d sides with all their cubes meshed, every one matched; %d directed sides occur twice" % (n, twice))


def test_a_broken_index_does_not_close():
    """the closure check is not vacuous: one swapped index pair opens the mesh"""
    s = dict(statement(mc.by_name("gates-base")))
    assert_closed(s, "intact")
    idx = s["idx"].copy()
    idx[100, [0, 1]] = idx[100, [1, 0]]
    s["idx"] = idx
    assert len(mx.unclosed_sides(s["keys"], s["idx"], s["tkeys"])[1]) > 0


def test_unguarded_key_beyond_the_range_merges_two_edges():
    """The key as DESIGN 3.7 states it, without the range guard: the y field of voxel 2^19 (block 65536) carries into the x field."""
    def raw(gx, gy, gz, axis):
        b = 1 << 19
        return (((gx + b) & 0xFFFFFFFF) << 42 | ((gy + b) & 0xFFFFFFFF) << 22 | ((gz + b) & 0xFFFFFFFF) << 2 | axis) & 0xFFFFFFFFFFFFFFFF
    assert raw(0, 1 << 19, 5, 1) == raw(1, -(1 << 19), 5, 1)             # one block beyond on y: another edge's key
    assert raw(3, 6, 1 << 19, 2) == raw(3, 7, -(1 << 19), 2)             # one block beyond on z: its carry lands in the y field
    assert raw(0, (1 << 19) - 1, 5, 1) != raw(1, -(1 << 19), 5, 1)
    assert mx.BLOCK_MIN == -65536 and mx.BLOCK_MAX == 65535


def test_position_bound_stays_within_the_room_tests_tolerance():
    assert mx.position_bound(800, 0.01) <= 1e-6 < mx.position_bound(900, 0.01)
    assert abs(mx.position_bound(1 << 19, 0.01) / 0.01 - 1.0 / 16.0) < 1e-3     # twice the half-ulp of 1/32 voxel there
