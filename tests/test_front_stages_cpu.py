"""The fusion front chain without a GPU: the statement tests/front_exact.py against itself and against the oracle's stage entries, on every case of
tests/front_cases.py.

  * fma32 (binary64 product, TwoSum, round to odd) is fmaf: held to the rational fma_exact on random, cancelling and half-way operands.
  * Self-checks of the walk on every allocation case: it starts at the block of p0, moves one block along one axis per step (6-connected), never against
    its step on any axis, stays in the box of the blocks of p0 and p1, and visits at most 1024 blocks.
  * oracle/tsdf_oracle.c or_stage_alloc (births of every sequence), or_stage_frustum (both frustum_modes, every pose and lattice of the compaction
    cases) and or_depth_to_float (with the integration-distance gate the kernels apply in the pre-pass) against the statement, to the bit.
  * The witnesses the cases claim: depth values that hit each gate exactly, colour pixels outside and on the last row and column, coordinates below
    zero and on both sides of it, the fill of the 128-slot table, frames that name nothing.
  * check_directory on a hand-built sound dump and on one violation per rule: each rule rejects its own violation and no other rule fires.

Expected values of the GPU module (tests/test_front_stages.py) come from here: expected_births is the oracle's, for speed; the smallest cases are
held to the statement there as well.

Run time of this module: 4 s for its 126 tests on 16 CPU threads (the births of a 32-frame sequence: 0.3 s by the statement); nothing is cached beyond
the oracle's births per sequence."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import front_cases as fc
from tests import front_exact as fx

F32 = np.float32
_births = {}


def expected_births(case):
    """[{coords: birth} after pass 1, after pass 2, ...] of an allocation case, by or_stage_alloc; sequences shared between cases are walked once."""
    key = getattr(case, "seq", None) or case.name
    n_max = {"wall32": 32}.get(key)
    if key not in _births:
        vol = orc.Volume(fc.oracle_params(orc, case.p))
        out, present, seq = [], {}, 1
        passes = case.passes if n_max is None else [(fc.wall(fc.SEQ_W, fc.SEQ_H, 32), fc.walk_poses(32), 0, 0)]
        for depth, poses, _, _ in passes:
            for j in range(len(depth)):
                for b in map(tuple, vol.stage_alloc(depth[j], poses[j]).tolist()):
                    present[b] = seq + j
            seq += len(depth)
            out.append(dict(present))
        _births[key] = out
    if n_max is None:
        return _births[key]
    n = len(case.passes[0][0])                      # a prefix of the shared sequence, and nothing new in the passes that repeat it
    first = {b: s for b, s in _births[key][0].items() if s <= n}
    return [first] * len(case.passes)


def stated_births(case):
    k = fx.derive(case.p)
    out, present, seq = [], {}, 1
    for depth, poses, _, _ in case.passes:
        present = fx.births(k, poses, depth, seq, present)
        seq += len(depth)
        out.append(present)
    return out


# ---- fma ------------------------------------------------------------------------------------------------------------------------------------------------
def test_fma32_is_one_rounding_of_the_exact_sum():
    rng = np.random.default_rng(5)
    n = 3000
    a, b, c = (rng.standard_normal(n).astype(F32) * F32(2.0) ** rng.integers(-20, 20, n).astype(F32) for _ in range(3))
    c[:1000] = (-(a[:1000].astype(np.float64) * b[:1000])).astype(F32)              # cancellation: the result is the product's rounding error
    # half-way cases: a b = an odd multiple of 2^-24 relative to c's ulp, so that the exact sum lies exactly between two floats, +- one bit far below
    a[1000:1400], b[1000:1400] = F32(1 + 2.0 ** -12), F32(1 + 2.0 ** -12)            # 1 + 2^-11 + 2^-24: 25 bits
    c[1000:1400] = (rng.integers(1, 1 << 10, 400) * 2.0 ** -11).astype(F32) * rng.choice([-1, 1], 400).astype(F32)
    got = fx.fma32(a, b, c)
    want = np.array([fx.fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.uint32) & 0x7FFFFFFF, want.view(np.uint32) & 0x7FFFFFFF) and np.array_equal(got, want)
    with np.errstate(all="ignore"):
        twice = (a * b + c).astype(F32)
    assert (got != twice).sum() > 500                                                # two roundings are another function on these operands


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in fc.ALLOC_CASES if not c.name.startswith(("ray-n", "cube5-n"))] + [c for c in fc.ALLOC_CASES if c.name == "ray-n32-g16-h0"], ids=repr)
def test_walks_are_connected_monotone_and_boxed(case):
    k = fx.derive(case.p)
    seen = 0
    for depth, poses, _, _ in case.passes[:1]:
        for j in range(len(depth)):
            rs = fx.ray_setup(k, fx.frame_setup(k, poses[j]), fx.prepass(k, depth[j]))
            ray, visit, b = fx.walk(rs)
            if len(ray) == 0:
                continue
            order = np.lexsort((visit, ray))
            ray, visit, b = ray[order], visit[order], b[order]
            first = np.r_[True, ray[1:] != ray[:-1]]
            assert np.array_equal(b[first], rs.cur[ray[first]]) and (visit[first] == 0).all()                      # starts at the block of p0
            d = b[1:] - b[:-1]
            same = ~first[1:]
            assert (np.abs(d[same]).sum(1) == 1).all()                                                                 # 6-connected
            assert (d[same] * rs.step[ray[1:][same]] >= 0).all()                                                       # never against the step
            lo, hi = np.minimum(rs.cur, rs.end)[ray], np.maximum(rs.cur, rs.end)[ray]
            assert ((b >= lo) & (b <= hi)).all()                                                                       # inside the box of p0's and p1's blocks
            assert visit.max() < fx.MAX_WALK
            seen += len(ray)
    assert (seen == 0) == bool(getattr(case, "empty", False)) or case.name == "empty-band"


# ---- the oracle's entries against the statement ---------------------------------------------------------------------------------------------------------
UNIQUE_SEQUENCES = [c for c in fc.ALLOC_CASES if getattr(c, "seq", None) is None] + [c for c in fc.ALLOC_CASES if c.name in ("ray-n32-g16-h0", "three-passes-brick1")]


@pytest.mark.parametrize("case", UNIQUE_SEQUENCES, ids=repr)
def test_oracle_stage_alloc_is_the_statement(case):
    want, got = stated_births(case), expected_births(case)
    assert len(want) == len(got)
    for w, g in zip(want, got):
        assert w == g, (len(w), len(g))
    last = want[-1]
    coords = np.array(sorted(last), np.int64).reshape(-1, 3)
    if getattr(case, "empty", False):
        assert not last
    else:
        assert len(last) > 0
    if getattr(case, "negative", False):
        assert (coords < 0).any(1).all()
    if getattr(case, "ties", None):
        k = fx.derive(case.p)
        depth, poses, _, _ = case.passes[0]
        rs = fx.ray_setup(k, fx.frame_setup(k, poses[0]), fx.prepass(k, depth[0]))
        axes = ["xyz".index(a) for a in case.ties]
        assert len(rs.pixel) == 1 and len(last) >= 6
        for q in (rs.tmax, rs.tdelta, rs.cur, rs.bound):
            assert len({q[0, a].tolist() for a in axes}) == 1 and np.isfinite(q[0, axes[0]])
    if getattr(case, "straddles", False):
        assert all({-1, 0} <= set(coords[:, a].tolist()) for a in range(3))
    if getattr(case, "fill", None):
        assert case.fill[0] <= len(last) <= case.fill[1], len(last)
    if getattr(case, "relaxed", None) == "table":
        assert len(last) > fx.derive(case.p).total_slots
    if getattr(case, "relaxed", None) == "heap":
        assert len(last) > case.p.num_sdf_blocks
    if getattr(case, "repeat", False):
        assert want[0] == want[1] == want[2]
    assert len(last) <= case.p.num_sdf_blocks or getattr(case, "relaxed", None)


@pytest.mark.parametrize("mode", (0, 1))
def test_oracle_stage_frustum_is_the_statement(mode):
    p = fc.compact_params(mode)
    k, op = fx.derive(p), fc.oracle_params(orc, p)
    poses = fc.compact_poses(32)
    blocks = np.concatenate([fc.lattice(k, poses[0]), fc.plane_blocks(k, poses[0]), fc.plane_blocks(k, poses[31])])
    inside = 0
    for pose in poses:
        want = fx.in_frustum(k, fx.frame_setup(k, pose), blocks)
        assert np.array_equal(orc.stage_frustum(op, pose, blocks), want)
        inside += int(want.sum())
    assert 0 < inside < 32 * len(blocks)


def test_plane_blocks_sit_on_either_side_of_every_plane():
    k = fx.derive(fc.compact_params(0))
    pose = fc.compact_poses(1)[0]
    b = fc.plane_blocks(k, pose)
    m = fx.plane_margins(k, fx.frame_setup(k, pose), b)
    bs = 8 * float(k.voxel)
    for q in range(6):
        alone = np.delete(m, q, 1).min(1) >= 0
        assert (alone & (m[:, q] >= 0)).any() and (alone & (m[:, q] < 0)).any(), q
    inside = fx.in_frustum(k, fx.frame_setup(k, pose), b)
    assert np.array_equal(inside, (m[:, :2] > 0).all(1) & (m[:, 2:] >= 0).all(1)) and 0 < inside.sum() < len(b)
    assert np.abs(m[:, :2]).min() < bs                                               # within a block of the z planes


@pytest.mark.parametrize("case", fc.PREPASS_CASES, ids=repr)
def test_prepass_statement_and_oracle(case):
    k, op = fx.derive(case.p), fc.oracle_params(orc, case.p)
    for frame in case.depth:
        want = fx.prepass(k, frame)
        got = orc.depth_to_float(op, fx.resample(k, frame))
        got[~(got < op.max_integration_dist)] = -np.inf          # the kernels gate the integration distance in the pre-pass, or_depth_to_float in the rule
        assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
    v = case.depth[0].astype(F32) / k.shift
    for name in getattr(case, "hits", ()):
        assert (v == {"dmin": k.dmin, "dmax": k.dmax, "maxd": k.maxd}[name]).any(), name
    if getattr(case, "hits", ()):
        d = fx.prepass(k, case.depth[0]).ravel()
        u = case.depth[0].ravel()
        assert d[0] == -np.inf and np.isfinite(d[u[v.ravel() == k.dmin]]).all()
        if "dmax" in case.hits:
            at = int(u[v.ravel() == k.dmax][0])
            assert np.isfinite(d[at]) and d[at + 1] == -np.inf
        if "maxd" in case.hits:
            at = int(u[v.ravel() == k.maxd][0])
            assert d[at] == -np.inf and np.isfinite(d[at - 1])
    if getattr(case, "outside", False):
        kx = (np.arange(k.W).astype(F32) - k.mx) / k.fx
        ky = (np.arange(k.H).astype(F32) - k.my) / k.fy
        u = (fx.fma32(kx, k.cfx, k.cmx) + F32(0.5)).astype(np.float64)
        w = (fx.fma32(ky, k.cfy, k.cmy) + F32(0.5)).astype(np.float64)
        assert (u < 0).any() and (u >= k.cW).any() and (w < 0).any() and (w >= k.cH).any()
        assert (u.astype(int) == k.cW - 1).any() and (w.astype(int) == k.cH - 1).any() and ((u > -1) & (u < 0)).sum() >= 0
        packed = fx.colour_lookup(k, case.rgb[0])
        assert (packed == 0).any() and (packed != 0).any()
    if case.name.startswith("resampled"):
        assert not np.array_equal(fx.resample(k, case.depth[0]), case.depth[0][:k.H, :k.W])


# ---- check_directory ------------------------------------------------------------------------------------------------------------------------------------
def sound_dump(k, blocks, freed=()):
    """A dump as a sequence of insertions leaves it (by hand: linear probing from the home slot, slots handed out 0, 1, 2, ...), then `freed` of the blocks
    released the way a collection with a rebuilt table leaves them."""
    key = np.full(k.total_slots, fx.KEY_EMPTY, np.uint64)
    ptr = np.full(k.total_slots, -1, np.int32)
    birth = np.full(k.total_slots, 0xFFFFFFFF, np.uint32)
    bkeys = np.full(k.num_blocks, fx.KEY_EMPTY, np.uint64)
    bentry = np.zeros(k.num_blocks, np.int32)
    for i, b in enumerate(blocks):
        at = fx.home_slot(k, *b)
        while key[at] != fx.KEY_EMPTY:
            at = (at + 1) % k.total_slots
        key[at], ptr[at], birth[at] = fx.pack_key(*b), i, 1 + i % 3
        bkeys[i], bentry[i] = key[at], at
    n = len(blocks)
    heap = np.arange(k.num_blocks - 1, -1, -1).astype(np.int32)
    cnt = np.zeros(48, np.int32)
    cnt[fx.C_HEAP_FREE], cnt[fx.C_HIGH_WATER], cnt[fx.C_SLOTS_USED] = k.num_blocks - n, n, n
    return {"key": key, "ptr": ptr, "birth": birth, "heap": heap, "block_keys": bkeys, "block_entry": bentry, "block_flags": np.zeros(k.num_blocks, np.uint8), "counters": cnt}


def _dir_case():
    p = fc.params(16, 16, num_sdf_blocks=64, hash_num_buckets=16, hash_bucket_size=2)
    k = fx.derive(p)
    rng = np.random.default_rng(3)
    blocks = [tuple(b) for b in np.unique(rng.integers(-4, 5, (40, 3)), axis=0).tolist()][:28]
    return k, blocks, sound_dump(k, blocks)


def test_check_directory_accepts_a_sound_dump_with_wrapped_chains():
    k, blocks, d = _dir_case()
    assert fx.check_directory(d, k) == []
    assert fx.dump_births(d) == {b: 1 + i % 3 for i, b in enumerate(blocks)}
    used = np.nonzero(d["key"] != fx.KEY_EMPTY)[0]
    assert any(s < fx.home_slot(k, *fx.unpack_key(d["key"][s])) for s in used)      # 28 of 32 slots: some chain wrapped at total_slots
    assert any(min(b) < 0 for b in blocks) and all(fx.unpack_key(fx.pack_key(*b)) == b for b in blocks)


@pytest.mark.parametrize("rule", fx.RULES)
def test_check_directory_rejects_each_violation_by_its_own_rule(rule):
    k, blocks, d = _dir_case()
    key, ptr, bkeys, bentry, heap, cnt = d["key"], d["ptr"], d["block_keys"], d["block_entry"], d["heap"], d["counters"]
    used = np.nonzero(key != fx.KEY_EMPTY)[0]
    relaxed = False
    if rule == "tombstone":                     # a tombstone where an EMPTY belongs: a free slot of the table
        key[np.nonzero(key == fx.KEY_EMPTY)[0][0]] = fx.KEY_TOMB
    elif rule == "duplicate-key":               # the same key once more, behind its first entry, without a tile
        e = np.nonzero(key == fx.KEY_EMPTY)[0][0]
        key[e] = key[used[0]]
        cnt[fx.C_ALLOC_FAIL], relaxed = 1, True                                           # (as an orphan it is accounted for: only the key is wrong)
    elif rule == "unreachable":                 # an entry moved to a free slot: the EMPTY it leaves behind ends the look-up before the key is met
        s, t = used[0], np.nonzero(key == fx.KEY_EMPTY)[0][0]
        key[t], ptr[t], key[s], ptr[s] = key[s], ptr[s], fx.KEY_EMPTY, -1
        bentry[ptr[t]] = t
    elif rule == "entry-slot":                  # two directory entries swapped: ptr and block_entry still form a bijection, the keys disagree
        bkeys[0], bkeys[1] = bkeys[1], bkeys[0]
    elif rule == "heap-partition":              # a live slot also on the free list
        heap[0] = 3
    elif rule == "slots-used":
        cnt[fx.C_SLOTS_USED] += 1
    elif rule == "heap-free":                   # one more free slot than there is: the list's stretch grows by a slot that is live
        cnt[fx.C_HEAP_FREE] += 1
        heap[cnt[fx.C_HEAP_FREE] - 1] = heap[0]
    elif rule == "high-water":
        cnt[fx.C_HIGH_WATER] = len(blocks) - 1
    elif rule == "orphan":                      # an entry claimed without a tile that no failure accounts for
        e = np.nonzero(key == fx.KEY_EMPTY)[0][0]
        key[e] = fx.pack_key(100, 100, 100)
        home = fx.home_slot(k, 100, 100, 100)
        at = home
        while key[at] != fx.KEY_EMPTY and at != e:
            at = (at + 1) % k.total_slots
        key[e] = fx.KEY_EMPTY
        key[at] = fx.pack_key(100, 100, 100)
        relaxed = True
    got = fx.check_directory(d, k, relaxed=relaxed)
    want = {"heap-free": ["heap-free", "heap-partition"], "duplicate-key": ["duplicate-key"]}.get(rule, [rule])
    assert got == want, got
    if rule == "orphan":
        assert fx.check_directory(d, k, relaxed=False) == ["orphan"]
        cnt[fx.C_ALLOC_FAIL] = 1
        assert fx.check_directory(d, k, relaxed=True, failures_are_orphans=True) == []
        cnt[fx.C_ALLOC_FAIL] = 2
        assert fx.check_directory(d, k, relaxed=True) == [] and fx.check_directory(d, k, relaxed=True, failures_are_orphans=True) == ["orphan"]


# ---- compaction -----------------------------------------------------------------------------------------------------------------------------------------
def test_masks_follow_births_and_ghosts():
    k = fx.derive(fc.compact_params(0))
    poses = fc.compact_poses(8)
    blocks, ghost = fc.compact_directory(k, 257)
    assert len(np.unique(blocks, axis=0)) == 257
    free = fx.masks(k, poses, 10, blocks, np.zeros(257), np.zeros(257, bool))
    assert (free != 0).any() and (free == 0).any() and len(set(free.tolist())) > 4
    birth = 10 + np.arange(257) % 12                                                   # born before, inside and after the pass
    m = fx.masks(k, poses, 12, blocks, birth, ghost)
    for i in range(257):
        d = max(0, int(birth[i]) - 12)
        assert m[i] == (0 if ghost[i] or d >= 8 else int(free[i]) & ~((1 << d) - 1) & 0xFF)
    s = fx.mask_summary(m, 8)
    assert s["length"] == int((m != 0).sum()) == s["tiles"] and s["last"] == int(((m >> 7) & 1).sum()) and s["total"] == sum(bin(int(v)).count("1") for v in m)
    assert (fx.masks(k, poses, 12, blocks, birth + 40, ghost) == 0).all()              # 32 or more after seq0: never listed
