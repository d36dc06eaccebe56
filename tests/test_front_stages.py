"""The front chain of a fusion pass, kernel by kernel: k_prepass, k_alloc<5 | 6, MULTI>, k_alloc_ray<MULTI> (with and without the fused pre-pass),
k_compactify, k_compactify_few, and the block maintenance k_gc, k_rehash, k_import (scannet_amd/csrc/fuser_prepass.hip, fuser_alloc.hip, fuser_compact.hip,
fuser_blocks.hip).

Three parties:
  * the HIP kernels through the stage hooks of include/scanfuse_internal.h (fusion.Fuser.stage_prepass / _alloc / _compact / _live / _dump), each of which
    runs ONE stage of a pass through the launcher run_batch uses for it;
  * the oracle's stage entries (oracle/tsdf_oracle.c or_stage_alloc, or_stage_frustum, or_depth_to_float), which tests/test_front_stages_cpu.py (default
    suite) holds to the statement on every case;
  * tests/front_exact.py, the statement: numpy.float32 arrays with one rounding per operation, sets of coordinates, a dictionary {coords: birth}.

This module (-m gpu): every case of tests/front_cases.py through the hooks, to the bit -- floats and texels; {coords: birth} of the dumped table (slots
and list order are scheduling: compared by coordinates; within a workgroup's stretch the list is ascending); masks, list length, last-frame count and
the two sums; check_directory after every allocation pass and after garbage collection, reset, import and re-import, and exhaust -> deintegrate ->
collect -> integrate; the product (integrate_batch_device) against the composition of the hooks.  Expected values are the oracle's, for speed; cases
of fewer than 3 000 blocks are held to the statement directly as well.  There is no tolerance anywhere.

Findings.
  1. A block claimed in the table while the heap is empty (give_block_quiet's failure path) stayed counted in C_SLOTS_USED: after an exhausted pass
     sf_stats.hash_slots_used exceeded blocks_allocated by the number of failures, although no such block exists (case heap-too-small, rule slots-used).
     Fixed in scannet_amd/csrc/fuser_device.h: the failure path takes the count back; such an entry is counted in alloc_failures and nowhere else.
  2. Not a defect, a precondition now written down: k_compactify_few reads no birth stamp for a pass of ONE frame (a one-frame pass only meets blocks
     its own frame or an earlier one asked for).  sf_fuser_stage_compact documents it and the n == 1 cases keep every birth <= seq0.

Out of scope: the grid-stride loop of k_compactify (it starts above num_cus x 8 x 1024 directory entries: an 8 GiB voxel pool); stream hand-over and
overlap between passes (tests/test_gpu_tsdf.py runs the scheduling matrix); the integrate kernels (tests/test_gpu_integrate_cuts.py,
tests/test_gpu_weight_record.py); everything the measurement and test set-up owns (bench.py, conftest.py, the pytest settings).

One-line mutations of the front chain (values and predicates only; never the hash probe loop, a compare-and-swap, the heap pop, a queue, LDS or global
index, a loop bound or a barrier), each built into a scratch copy of the library and run under this module once on the MI355X; the test ids that failed
under it (133 ids when mutations 0-9 and 13-21 ran, 141 with the eight tie-* cases that 10-12 then ran under; "product" =
test_gpu_product_is_the_composition_of_the_hooks):
   0. finding 1 taken back (the failure path keeps its slot counted)      2: test_gpu_alloc_stage[heap-too-small], test_gpu_directory_after_collect_reset_and_exhaustion
   1. k_prepass: v < depth_min as <=                     6: test_gpu_prepass_stage[all-u16-shift1000], [-far], [all-u16-shift777.5], two raw-colour cases whose random depths hold a 100;
                                                         test_gpu_alloc_stage[ray-gates]
   2. k_prepass: !(v < max distance) as !(v <=)          5: test_gpu_prepass_stage[all-u16-shift1000], [all-u16-shift777.5], [frames-n32-17x9]; test_gpu_alloc_stage[ray-gates],
                                                         [all-beyond-max-distance]
   3. k_prepass: raw colour's u without + 0.5f           2: test_gpu_prepass_stage[rgb-own-size-31x23], [rgb-resampled-input-size]
   4. k_prepass: the resample's column without + 0.5f    2: test_gpu_prepass_stage[resampled-40x30-to-17x9], [rgb-resampled-input-size]
   5. fused pre-pass: v < depth_min as <=                1: test_gpu_alloc_stage[ray-fused-gates] (added for it: the fused case had no value on a gate)
   6. world_to_block: q - 0.5f as q + 0.5f               74: every allocation case that allocates but the ties, diag111 and +y views, nine-levels and heap-too-small; compact_births; product
   7. k_alloc_ray: the block face at + 0.5 voxel         62: every case through k_alloc_ray (59); compact_births; product
   8. k_alloc: the block face at + 0.5 voxel             17: every case through k_alloc<5> and k_alloc<6>
   9. k_alloc_ray: lo < hi as <=                         1: test_gpu_alloc_stage[empty-band]
  10. ray_walk_bits: tmx < tmy as <=                     1: test_gpu_alloc_stage[tie-xy-ray]
  11. ray_walk_bits: tmz < tmy as <=                     2: test_gpu_alloc_stage[tie-xyz-ray], [tie-yz-ray]
  12. k_alloc: tmz < tmy as <=                           2: test_gpu_alloc_stage[tie-xyz-cube5], [tie-yz-cube5]
      (10-12 passed every case of the first list: no walk there meets an exact tie.  The eight tie-* cases were added for them.)
  13. k_alloc_ray's scan: the centre line read back with >> 11 for >> 12 (the walk's map unchanged; the range test keeps every bit inside the bitmap)
                                                         60: every case through k_alloc_ray but ray-window-too-small and table-128; compact_births; product
  14. block_in_frustum: zfar + radius as zfar - radius   7: test_gpu_compact_stage[0-255 .. 0-2049]; compact_births
  15. block_in_frustum, mode 1: nx x 0.9                 6: test_gpu_compact_stage[1-255 .. 1-2049]
  16. block_in_frustum: >= -yr[1] as >= yr[1]            84: 74 of test_gpu_alloc_stage, test_gpu_compact_stage[0-255 .. 0-2049], compact_births, the maintenance test, product
  17. k_compactify: d >= 32 as d > 32                    1: test_gpu_compact_births (n 32, seq0 9: the blocks born in frame 41)
  18. k_compactify_few: ~((1 << d) - 1) as ~(1 << d)     1: test_gpu_compact_births (n 4, seq0 6)
  19. k_compactify: ghosts listed                        13: test_gpu_compact_stage[*-255 .. *-2049] (12), compact_births
  20. k_alloc_ray: every queued key born in frame 0      52: every multi-frame case through k_alloc_ray (48), the refusal test's last pass, compact_births, product
  21. k_compactify: birth > seq0 as birth > seq0 + 1     1: test_gpu_compact_births
No mutated run faulted or hung.

Run time on the MI355X (--durations=0): the module takes 5.5 s; the slowest five are test_gpu_prepass_stage[all-u16-shift1000] 0.30 s, [jpeg-444-17x9] 0.23 s
(the first use of the JPEG kernels), test_gpu_alloc_stage[ray-window-too-small] 0.13 s, [ray-n32-g4-h1] 0.08 s and test_gpu_compact_births 0.08 s."""
import numpy as np
import pytest

from oracle import oracle as orc
from scannet_amd import calibrate, fusion
from scannet_amd._abi import ScanfuseError
from tests import front_cases as fc
from tests import front_exact as fx
from tests import test_front_stages_cpu as cpu

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- pre-pass -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.PREPASS_CASES, ids=repr)
def test_gpu_prepass_stage(case):
    """k_prepass: the gates, the resample, raw colour at every alignment, colour at its own size, JPEG planes."""
    k = fx.derive(case.p)
    rgb, jpeg = getattr(case, "rgb", None), None
    cw, ch = (k.cW, k.cH) if k.cW else (k.W, k.H)
    if hasattr(case, "jpeg"):
        jpeg = fc.jpeg_streams(case)
        pictures = [calibrate.jpeg_decode(s, cw, ch) for s in jpeg]         # sf_jpeg_decode: the host decoder's bytes
    else:
        pictures = rgb
    with fusion.Fuser(case.p, device=0) as f:
        depthf, texel = f.stage_prepass(case.depth, rgb=rgb, misalign=getattr(case, "misalign", 0), jpeg=jpeg)
    want = np.stack([fx.prepass(k, frame).ravel() for frame in case.depth])
    assert np.array_equal(_bits(depthf), _bits(want)), case.name
    if pictures is None:
        assert texel is None
        return
    want_t = np.stack([fx.texels(want[j], fx.colour_lookup(k, pictures[j]).ravel()) for j in range(len(want))])
    assert np.array_equal(texel, want_t), (case.name, int((texel != want_t).sum()))
    assert ((want_t >> np.uint64(32)) != 0).any()


# ---- allocation -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.ALLOC_CASES, ids=repr)
def test_gpu_alloc_stage(case):
    """The front chain up to the allocation: the blocks and their births, the counters' deltas, the directory's invariants after every pass."""
    k = fx.derive(case.p)
    want = cpu.expected_births(case)
    relaxed = getattr(case, "relaxed", None)
    probed = []
    with fusion.Fuser(case.p, device=0, **case.tune) as f:
        for (depth, poses, head, fuse_pre), w in zip(case.passes, want):
            r = f.stage_alloc(depth, poses, head=head, fuse_pre=fuse_pre, want_depth=True)
            dump = f.stage_dump()
            got = fx.dump_births(dump)
            print("%s: %d blocks (%d stated), direct %d, probed %d, failed %d" % (case.name, len(got), len(w), r["direct"], r["probed"], r["failed"]))
            assert np.array_equal(_bits(r["depthf"]), _bits(np.stack([fx.prepass(k, fr).ravel() for fr in depth])))
            probed.append(r["probed"])
            if relaxed:
                assert r["failed"] > 0 and 0 < len(got) < len(w)
                assert all(w.get(b) == s for b, s in got.items())                 # a subset of the statement's set, every birth as stated
                assert fx.check_directory(dump, k, relaxed=True, failures_are_orphans=relaxed == "heap") == []
                if relaxed == "heap":
                    assert len(got) == case.p.num_sdf_blocks and dump["counters"][fx.C_HEAP_FREE] == 0
            else:
                assert got == w, (len(got), len(w), sorted(set(got) ^ set(w))[:4], [(b, got[b], w[b]) for b in got if b in w and got[b] != w[b]][:4])
                assert r["failed"] == 0
                assert fx.check_directory(dump, k) == []
            assert (r["direct"] > 0) == bool(getattr(case, "direct", False)), r
            if getattr(case, "fill", None):
                used = np.nonzero(dump["key"] != fx.KEY_EMPTY)[0]
                assert any(s < fx.home_slot(k, *fx.unpack_key(dump["key"][s])) for s in used), "no chain wrapped at total_slots"
        st = f.stats()
        assert st["blocks_allocated"] == len(got) == st["hash_slots_used"]
    if getattr(case, "repeat", False) and case.brick:
        assert probed[2] < probed[0] and probed[2] <= probed[1], probed
    if not relaxed and len(want[-1]) < 3000:
        assert cpu.stated_births(case)[-1] == got                                  # the smallest cases against the statement itself


def test_gpu_hooks_refuse_what_they_cannot_run():
    p = fc.params(fc.SEQ_W, fc.SEQ_H)
    depth, poses = fc.wall(fc.SEQ_W, fc.SEQ_H, 2), fc.walk_poses(2)
    lost = poses.copy()
    lost[1, :] = -np.inf
    with fusion.Fuser(p, device=0) as f:
        calls = [lambda: f.stage_alloc(depth, poses, fuse_pre=True),                                   # two frames never fuse the pre-pass
                 lambda: f.stage_alloc(depth, lost),
                 lambda: f.stage_alloc(np.zeros((33, fc.SEQ_H, fc.SEQ_W), np.uint16), np.tile(poses[:1], (33, 1))),
                 lambda: f.stage_compact(lost, 1),
                 lambda: f.stage_compact(np.tile(poses[:1], (33, 1)), 1),
                 lambda: f.stage_prepass(depth, rgb=np.zeros((2, fc.SEQ_H, fc.SEQ_W, 3), np.uint8), misalign=8),
                 lambda: f.stage_prepass(depth, misalign=1)]
        for call in calls:
            with pytest.raises(ScanfuseError) as e:
                call()
            assert e.value.code == -1
        f.tune(alloc_ray=0)
        with pytest.raises(ScanfuseError) as e:
            f.stage_alloc(depth[:1], poses[:1], fuse_pre=True)                                         # the cube window never does
        assert e.value.code == -1
        d = f.stage_dump()
        assert (d["key"] == fx.KEY_EMPTY).all() and d["counters"][fx.C_SLOTS_USED] == 0                # nothing was launched
        f.tune(alloc_ray=1)
        assert f.stage_alloc(depth, poses)["failed"] == 0                                              # ... and the sequence numbers did not move
        assert set(fx.dump_births(f.stage_dump()).values()) == {1, 2}


# ---- compaction -----------------------------------------------------------------------------------------------------------------------------------------
def _listed(dump, r):
    keys = dump["block_keys"][r["slots"]]
    assert (keys != fx.KEY_EMPTY).all() and len(set(r["slots"].tolist())) == len(r["slots"])
    return {fx.unpack_key(kk): int(m) for kk, m in zip(keys, r["masks"])}


def _ascending_per_stretch(slots, stretch):
    s = np.asarray(slots, np.int64)
    g = s // stretch
    change = np.nonzero(g[1:] != g[:-1])[0]
    assert len(change) + 1 == len(set(g.tolist())) or len(s) == 0, "a workgroup's entries are not contiguous in the list"
    assert ((s[1:] > s[:-1]) | (g[1:] != g[:-1])).all()


def _oracle_masks(p, poses, seq0, blocks, birth, ghost):
    op = fc.oracle_params(orc, p)
    m = np.zeros(len(blocks), np.uint32)
    for j, pose in enumerate(poses):
        inside = orc.stage_frustum(op, pose, blocks) & (np.asarray(birth) <= seq0 + j) & ~np.asarray(ghost, bool)
        m |= inside.astype(np.uint32) << np.uint32(j)
    return m


def _check_compaction(f, p, k, poses, seq0, blocks, birth, ghost, stated):
    n = len(poses)
    dump = f.stage_dump()
    r = f.stage_compact(poses, seq0)
    want = _oracle_masks(p, poses, seq0, blocks, birth, ghost)
    if stated:
        assert np.array_equal(want, fx.masks(k, poses, seq0, blocks, birth, ghost))
    assert _listed(dump, r) == {tuple(b): int(m) for b, m in zip(blocks.tolist(), want) if m}, (n, seq0)
    s = fx.mask_summary(want, n)
    assert {q: r[q] for q in ("length", "last", "total", "tiles")} == s, (r, s)
    _ascending_per_stretch(r["slots"], 256 if n > 4 else 2048)
    return s


@pytest.mark.parametrize("hw", fc.HIGH_WATER)
@pytest.mark.parametrize("mode", (0, 1))
def test_gpu_compact_stage(mode, hw):
    """k_compactify (n > 4: the 8 / 16 / 32 frames-per-lane-group layouts) and k_compactify_few (its stretches of 8 x 256 entries) on directories of exactly
    hw entries made with import_blocks: blocks on either side of every plane, ghosts among them; and sf_compact_live with and without ghosts."""
    p = fc.compact_params(mode)
    k = fx.derive(p)
    blocks, ghost = fc.compact_directory(k, hw)
    with fusion.Fuser(p, device=0) as f:
        if hw:
            f.import_blocks(blocks[~ghost], np.zeros((int((~ghost).sum()), 4096), np.uint8), ghost=False)
            f.import_blocks(blocks[ghost], np.zeros((int(ghost.sum()), 4096), np.uint8), ghost=True)
        dump = f.stage_dump()
        assert dump["counters"][fx.C_HIGH_WATER] == hw and fx.check_directory(dump, k) == []
        assert fx.dump_births(dump) == {tuple(b): 0 for b in blocks.tolist()}
        listed = 0
        for n in fc.COMPACT_N:
            s = _check_compaction(f, p, k, fc.compact_poses(n), 7, blocks, np.zeros(hw), ghost, stated=hw <= 257)
            listed += s["length"]
        assert listed > 0 or hw < 255
        for with_ghosts in (True, False):
            live = f.stage_live(with_ghosts)
            want = {tuple(b) for b, g in zip(blocks.tolist(), ghost) if with_ghosts or not g}
            assert {fx.unpack_key(kk) for kk in dump["block_keys"][live]} == want and len(live) == len(want)
            _ascending_per_stretch(live, 2048)
        # a re-import changes flags, not the table
        if hw >= 255:
            f.import_blocks(blocks[:40], np.zeros((40, 4096), np.uint8), ghost=True)
            d2 = f.stage_dump()
            assert fx.check_directory(d2, k) == [] and np.array_equal(d2["key"], dump["key"]) and np.array_equal(d2["ptr"], dump["ptr"])
            assert len(f.stage_live(False)) == hw - 40 - int(ghost[40:].sum())


def test_gpu_compact_births():
    """birth <= seq0 + j: blocks born before, inside and 32 or more frames after the first frame of the pass."""
    p = fc.params(fc.SEQ_W, fc.SEQ_H)
    k = fx.derive(p)
    depth, poses = fc.wall(fc.SEQ_W, fc.SEQ_H, 32), fc.walk_poses(32)
    late = fc.walk_poses(2, eye=(0.5, -0.1, 0.2))
    vol = orc.Volume(fc.oracle_params(orc, p))
    birth = {}
    with fusion.Fuser(p, device=0, alloc_group=4) as f:
        f.stage_alloc(depth[:8], poses[:8])                                                        # births 1 .. 8
        f.stage_alloc(np.zeros_like(depth), poses)                                                 # 32 frames that name nothing: 9 .. 40
        f.stage_alloc(depth[8:10], late)                                                           # births 41, 42
        for seq, d, q in [(1 + j, depth[j], poses[j]) for j in range(8)] + [(41 + j, depth[8 + j], late[j]) for j in range(2)]:
            for b in map(tuple, vol.stage_alloc(d, q).tolist()):
                birth[b] = seq
        cand = fc.lattice(k, poses[0], reach=0)
        cand = cand[fx.in_frustum(k, fx.frame_setup(k, poses[0]), cand)]
        extra = np.array([b for b in cand[::max(1, len(cand) // 400)].tolist() if tuple(b) not in birth][:300], np.int32)
        assert len(extra) == 300
        f.import_blocks(extra[:200], np.zeros((200, 4096), np.uint8), ghost=False)                   # birth 0
        f.import_blocks(extra[200:], np.zeros((100, 4096), np.uint8), ghost=True)
        dump = f.stage_dump()
        for b in extra.tolist():
            birth[tuple(b)] = 0
        assert fx.dump_births(dump) == birth and fx.check_directory(dump, k) == []
        assert {41, 42} <= set(birth.values()) and set(range(1, 9)) <= set(birth.values())
        blocks = np.array(sorted(birth), np.int32)
        b_arr = np.array([birth[tuple(b)] for b in blocks.tolist()])
        ghost = np.array([tuple(b) in set(map(tuple, extra[200:].tolist())) for b in blocks.tolist()])
        for n, seq0 in ((1, 50), (4, 6), (4, 43), (5, 1), (8, 38), (9, 41), (16, 0), (17, 30), (32, 0), (32, 9), (32, 10), (32, 11)):
            use = np.concatenate([poses[:max(n - 2, 0)], late])[:n] if n > 1 else late[:1]
            s = _check_compaction(f, p, k, use, seq0, blocks, b_arr, ghost, stated=True)
            print("n %d seq0 %d: %s" % (n, seq0, s))
            assert s["length"] > 0


# ---- maintenance ----------------------------------------------------------------------------------------------------------------------------------------
def test_gpu_directory_after_collect_reset_and_exhaustion():
    """k_gc + k_rehash leave no tombstone and births of 0; reset leaves the state create leaves; a heap that ran out, emptied and collected serves again."""
    p = fc.params(16, 16, num_sdf_blocks=64)
    k = fx.derive(p)
    depth, poses = fc.wall(16, 16, 4, 1000, 500, 2), fc.walk_poses(4)
    with fusion.Fuser(p, device=0) as f:
        # import: every other block observed (kept by a collection), the others empty (freed)
        blocks = np.array([(x, y, 3) for x in range(-3, 4) for y in range(-2, 3)], np.int32)
        vox = np.zeros((len(blocks), 512), fusion.VOXEL_DTYPE)
        vox["sdf"][::2], vox["w"][::2] = 0.01, 1
        f.import_blocks(blocks, vox, ghost=False)
        assert fx.check_directory(f.stage_dump(), k) == []
        assert f.garbage_collect() == len(blocks) // 2
        d = f.stage_dump()
        assert fx.check_directory(d, k) == [] and not (d["key"] == fx.KEY_TOMB).any()
        assert fx.dump_births(d) == {tuple(b): 0 for b in blocks[::2].tolist()}
        f.reset()
        d = f.stage_dump()
        assert fx.check_directory(d, k) == [] and (d["key"] == fx.KEY_EMPTY).all() and (d["block_keys"] == fx.KEY_EMPTY).all()
        assert d["counters"][fx.C_HEAP_FREE] == 64 and not d["counters"][1:].any() and np.array_equal(d["heap"], np.arange(63, -1, -1))
        # exhaust -> deintegrate -> collect -> integrate again
        for j in range(4):
            f.integrate(depth[j], poses[j])
        d = f.stage_dump()
        assert d["counters"][fx.C_ALLOC_FAIL] > 0 and d["counters"][fx.C_HEAP_FREE] == 0
        assert fx.check_directory(d, k, relaxed=True, failures_are_orphans=True) == []
        for j in range(4):
            f.deintegrate(depth[j], poses[j])
        assert f.garbage_collect() == 64
        d = f.stage_dump()
        assert fx.check_directory(d, k, relaxed=True) == [] and d["counters"][fx.C_HEAP_FREE] == 64 and (d["key"] == fx.KEY_EMPTY).all()
        small = np.zeros((16, 16), np.uint16)
        small[4:8, 4:8] = 800
        f.integrate(small, poses[0])
        d = f.stage_dump()
        got = fx.dump_births(d)
        assert fx.check_directory(d, k, relaxed=True) == [] and 0 < len(got) < 64
        assert set(got) == set(fx.births(k, poses[:1], small[None], 9))


# ---- the product ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (5, 20))
def test_gpu_product_is_the_composition_of_the_hooks(n):
    """sf_fuser_integrate_batch_device (one pass; two passes with a head pass) ends in the {coords: birth} the hooks' composition ends in."""
    import torch
    p = fc.params(fc.SEQ_W, fc.SEQ_H)
    k = fx.derive(p)
    depth, poses = fc.wall(fc.SEQ_W, fc.SEQ_H, n), fc.walk_poses(n)
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    pose16 = np.ascontiguousarray(poses, F32)
    with fusion.Fuser(p, device=0) as f:
        f.integrate_batch_device(d_depth, fc.SEQ_W * fc.SEQ_H * 2, pose16)
        f.sync()
        product = f.stage_dump()
        assert f.stats()["alloc_failures"] == 0
    with fusion.Fuser(p, device=0) as f:
        cuts = [n] if n <= 8 else [(n + 1) // 2, n - (n + 1) // 2]                 # the passes integrate_batch_device cuts a call of n frames into
        at = 0
        for i, m in enumerate(cuts):
            f.stage_alloc(depth[at:at + m], poses[at:at + m], head=(i == 0 and len(cuts) > 1))
            at += m
        hooks = f.stage_dump()
    full = cpu.expected_births(next(c for c in fc.ALLOC_CASES if c.name == "ray-n32-g16-h0"))[0]
    want = {b: s for b, s in full.items() if s <= n}                              # the call's frames are the first n of the shared sequence
    assert fx.dump_births(product) == want and fx.dump_births(hooks) == want
    assert fx.check_directory(product, k) == [] and fx.check_directory(hooks, k) == []
