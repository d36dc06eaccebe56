"""Marching cubes on the GPU (scannet_amd/csrc/mc.hip: k_mc's count and emit pass, the two radix sorts, k_flag_heads, k_weld, k_gather_tris and the host
side of sf_fuser_extract_mesh), case by case.

Three parties, no tolerance between them:
  * the HIP path: Fuser.import_blocks (owned blocks and ghosts) -> extract_mesh().arrays(keys=True) and face_keys();
  * oracle/mc_oracle.c's entry over blocks (or_mc_extract_blocks), which tests/test_mc_stages_cpu.py (default suite) holds to the statement on every case;
  * tests/mc_exact.py, the statement in numpy; cases below 3 000 blocks are compared with it directly as well.
keys, position bits, colours (alpha 255), triangle indices and cube keys are equal; counts() and sf_fuser_mc_timing [9..11] agree with the arrays; what a
case expects beyond equality (tests/mc_cases.py: the exact cubes, what a perturbation drops, ghosts, zero-area triangles) is checked on the GPU mesh;
the closure check of tests/mc_exact.py runs on the GPU mesh of all-cases.

Findings.
  1. Edge-key overflow: confirmed by arithmetic (tests/test_mc_stages_cpu.py::test_unguarded_key_beyond_the_range_merges_two_edges) and by mutation 12:
     a block beyond +-65536 took part in the mesh and its vertices got keys of other grid edges.  The count pass now reports such a block and
     sf_fuser_extract_mesh refuses the volume with SF_ERR_CAPACITY naming it (cases key-range-beyond-*); DESIGN 3.7 states the range.
  2. sf_params.mc_max_triangles is not applied, on purpose; include/scanfuse.h no longer promises a limit (test_gpu_mc_max_triangles_is_not_applied).
  3. Denormals: not reproduced.  The kernel keeps them (zeros-signs: the smallest negative denormal is inside, dl = thresh / dh = -denormal gives mu == 1,
     bit-equal to the CPU parties); nothing was changed.
  Also: sf_fuser_mc_timing [9] (live blocks) stayed 0 when no triangle came out of live blocks; it is now set on that return too (zeros-all-*).

One-line mutations of mc.hip (values and predicates only; never an index, a loop bound, a barrier, a scan offset or a buffer size), built into a scratch
copy of the library and run under this module once each on the MI355X; the test ids that failed (of 56; "[x]" = test_gpu_case[x]):
   1. classify: d[i] < 0.0f as <=                        1: [zeros-signs]
   2. classify: fabsf(d) <= thresh as <                  5: [gates-thresh-on-f10-v0.01], [gates-thresh-on-f10-v0.004], [gates-thresh-on-f2.5-v0.01], [zeros-signs],
                                                         [colour-all-pairs] (the last two hold |sdf| == thresh by construction)
   3. classify: the weight gate removed                  54: all but [zeros-all-positive] and the closure test (an absent neighbour then reads as sdf 0, w 0: valid)
   4. load_tile: s >= 0 as s > 0                         52: all but the three [zeros-all-*] and the closure test (every fuser has a block in slot 0, which
                                                         then cannot read itself); test_gpu_neighbour_in_directory_slot_zero among them
   5. mu taken from the other end of the edge            51: all but [zeros-all-*], [colour-all-pairs] (mu = 1/2 there) and the closure test
   6. host_tables: edge orientation > as <               53: all but [zeros-all-*]
   7. colour without + 0.5f                              52: all but [zeros-all-*] and the closure test
   8. colour unfused (mu * (ch - cl) + cl, two roundings) 7: [colour-fused-differs], [all-cases], the three [gates-thresh-*-f2.5-v0.01], the dense checker,
                                                         test_gpu_order_and_reuse
   9. the axis == 0 / axis == 1 branches swapped         51: all but [zeros-all-*], [colour-all-pairs] (only z-edges there) and the closure test
  10. k_flag_heads flagging every entry                  52: all but [zeros-all-*] and [prefix-single-cubes] (no edge there is shared); the closure test fails
  11. sf_compact_live(..., 1): ghosts meshed             8: the seven [neighbour-ghost-*] and [neighbour-ghost-surrounded]
  12. finding 1 taken back (no refusal)                  2: [key-range-beyond-high-y], [key-range-beyond-low-z]
The unmutated scratch library passed all 56.  No mutated or unmutated run faulted or hung.

Run time on the MI355X (--durations=0): the module takes 8.5 s; the slowest five are test_gpu_case[all-cases] 2.59 s (2 s of it the numpy statement of
800 k triangles), test_gpu_mesh_of_all_cases_closes 2.09 s (numpy over 2.4 M sides), the dense checker 1.93 s (13^3 blocks, 4.4 M triangles, the
oracle included), test_gpu_order_and_reuse 0.08 s and test_gpu_case[colour-all-pairs] 0.07 s.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from scannet_amd import fusion
from scannet_amd._abi import ScanfuseError
from tests import mc_cases as mc
from tests import mc_exact as mx
from tests import test_mc_stages_cpu as cpu

pytestmark = pytest.mark.gpu
U64 = np.uint64
_gpu = {}


def extract(f, n_owned):
    """one extraction -> the canonical dict; counts() and the timing record agree with the arrays"""
    m = f.extract_mesh()
    xyz, rgba, tris, keys = m.arrays(keys=True)
    tkeys = m.face_keys()
    t = f.mc_timing()
    assert m.counts() == (len(keys), len(tris)) == (t["vertices"], t["triangles"]), (m.counts(), t)
    assert t["blocks"] == n_owned, (t, n_owned)
    assert (rgba[:, 3] == 255).all() and len(xyz) == len(keys) and len(tkeys) == len(tris)
    return dict(keys=keys, pos=xyz, col=np.ascontiguousarray(rgba[:, :3]), idx=tris.astype(np.int32), tkeys=tkeys)


def gpu_mesh(case):
    if case.name not in _gpu:
        with fusion.Fuser(case.params(), device=0) as f:
            case.fill(f)
            _gpu[case.name] = extract(f, int(case.owned.sum()))
    return _gpu[case.name]


@pytest.mark.parametrize("case", mc.cases(), ids=repr)
def test_gpu_case(case):
    if "key_range" in case.expect:
        axis, bad = case.expect["key_range"]
        with fusion.Fuser(case.params(), device=0) as f:
            case.fill(f)
            with pytest.raises(ScanfuseError) as info:
                f.extract_mesh()
            assert info.value.code == -6 and str(bad) in str(info.value), info.value          # SF_ERR_CAPACITY, the block named
            f.reset()
            ok = mc.by_name("gates-base")
            ok.fill(f)                                                                        # the fuser is not left broken
            cpu.assert_same_mesh(extract(f, 8), cpu.oracle_mesh(ok), "after the refusal", tkeys=False)
        return
    m = gpu_mesh(case)
    print("%s: %d blocks (%d owned) -> %d vertices, %d triangles" % (case.name, len(case.coords), case.owned.sum(), len(m["keys"]), len(m["idx"])))
    cpu.assert_same_mesh(m, cpu.oracle_mesh(case), case.name + " vs oracle")
    assert len(case.coords) < 3000
    cpu.assert_same_mesh(m, cpu.statement(case), case.name + " vs statement")
    assert not np.isnan(m["pos"]).any()
    cpu.check_expectations(case, m, gpu_mesh)
    if hasattr(case, "edge"):
        assert m["col"][np.searchsorted(m["keys"], case.edge[0]), 0] == case.edge[1]


def test_gpu_mesh_of_all_cases_closes():
    n, twice = cpu.assert_closed(gpu_mesh(mc.by_name("all-cases")), "gpu")
    print("all-cases on the GPU: %d sides with all their cubes meshed, every one matched; %d directed sides occur twice" % (n, twice))


def _dense_case():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = mc.dense_n(cus)
    assert n ** 3 > 8 * cus >= (n - 1) ** 3
    return mc.dense_checker(n), cus


def test_gpu_dense_checker_grid_stride_and_chunked_download():
    """More live blocks than k_mc has workgroups (the grid-stride loop, 4 triangles in every cube) and arrays longer than one 16 MiB download chunk with
    a partial last chunk.  Expected values: the oracle entry only."""
    case, cus = _dense_case()
    chunk = 16 << 20
    with fusion.Fuser(case.params(), device=0) as f:
        case.fill(f)
        m = extract(f, len(case.coords))
    assert len(case.coords) > 8 * cus
    assert (len(m["idx"]), len(m["keys"])) == (case.n_tris, case.n_verts)
    for name, nbytes in (("tri", m["idx"].size * 4), ("pos", m["pos"].size * 4), ("keys", m["keys"].size * 8)):
        assert nbytes > chunk and nbytes % chunk != 0, (name, nbytes)
    print("%s: %d CUs, %d blocks, %d triangles, %d vertices; tri %.1f, pos %.1f, keys %.1f chunks" % (
        case.name, cus, len(case.coords), len(m["idx"]), len(m["keys"]), m["idx"].size * 4 / chunk, m["pos"].size * 4 / chunk, m["keys"].size * 8 / chunk))
    want = orc.mc_extract_blocks(case.oracle_params(orc), case.coords, case.voxels, case.owned)
    cpu.assert_same_mesh(m, want, case.name)


def test_gpu_order_and_reuse():
    """The mesh does not depend on the order of the import (directory slots and the live list are scheduling), nor on what the fuser extracted before:
    three orders, a garbage collection in between, twice in a row, and small / large / small on one fuser (bounce buffers and events reused)."""
    big, small = mc.by_name("all-cases"), mc.by_name("gates-base")
    want, want_small = cpu.oracle_mesh(big), cpu.oracle_mesh(small)
    rng = np.random.default_rng(5)
    n = len(big.coords)
    with fusion.Fuser(big.params(), device=0) as f:
        small.fill(f)
        cpu.assert_same_mesh(extract(f, 8), want_small, "small first", tkeys=False)
        f.reset()
        big.fill(f, order=np.arange(n)[::-1])
        a = extract(f, n)
        cpu.assert_same_mesh(a, want, "reversed order", tkeys=False)
        cpu.assert_same_mesh(extract(f, n), a, "twice in a row")
        f.garbage_collect()
        big.fill(f, order=rng.permutation(n))
        cpu.assert_same_mesh(extract(f, n), a, "imported again after a collection")
        f.reset()
        small.fill(f)
        cpu.assert_same_mesh(extract(f, 8), want_small, "small again", tkeys=False)
    with fusion.Fuser(big.params(), device=0) as f:
        big.fill(f, order=rng.permutation(n))
        cpu.assert_same_mesh(extract(f, n), a, "another order, another fuser")


def _slot_of_blocks(f):
    d = f.stage_dump()
    live = np.nonzero(d["block_keys"] != U64(0xFFFFFFFFFFFFFFFF))[0]
    k = d["block_keys"][live].astype(np.int64)
    c = np.stack([(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], 1)
    return live, np.where(c >= (1 << 20), c - (1 << 21), c)


def test_gpu_neighbour_in_directory_slot_zero():
    """hash_lookup's `s >= 0`: slot 0 is a block like any other.  The heap holds exactly the 27 blocks, so slot 0 is taken; which block sits there is read
    from the directory, and it is made one that lower neighbours read through their halo."""
    case = mc.by_name("neighbour-base-3x3x3")
    first = int(np.nonzero((case.coords == 1).all(1))[0][0])                    # block (1, 1, 1)
    last = int(np.nonzero((case.coords == (1, 1, 0)).all(1))[0][0])
    with fusion.Fuser(case.params(num_sdf_blocks=27), device=0) as f:
        f.import_blocks(case.coords[[first]], case.voxels[[first]], ghost=False)
        slots, _ = _slot_of_blocks(f)
        assert len(slots) == 1
        rest = [i for i in range(27) if i not in (first, last)]
        f.import_blocks(case.coords[rest], case.voxels[rest], ghost=False)
        if slots[0] != 0:
            assert 0 not in _slot_of_blocks(f)[0]                               # the heap hands out slot 0 last
        f.import_blocks(case.coords[[last]], case.voxels[[last]], ghost=False)
        slots, coords = _slot_of_blocks(f)
        assert len(slots) == 27 and slots[0] == 0
        at0 = coords[0]
        assert tuple(at0) in ((1, 1, 1), (1, 1, 0)), at0
        m = extract(f, 27)
    # the cubes of block (0, 0, 0) that read the block in slot 0 through the halo: lx == ly == 7, and lz == 7 for (1,1,1) / lz < 7 for (1,1,0)
    origin = mx.decode_key((m["tkeys"] >> U64(3)) << U64(2))[0]
    through = (origin[:, 0] == 7) & (origin[:, 1] == 7) & ((origin[:, 2] == 7) if at0[2] == 1 else ((origin[:, 2] >= 0) & (origin[:, 2] < 7)))
    assert through.any(), "no meshed cube reads the block in slot 0"
    print("slot 0 holds block", at0, "read by", int(through.sum()), "triangles of block (0, 0, 0)")
    cpu.assert_same_mesh(m, cpu.oracle_mesh(case), "slot 0")
    cpu.assert_same_mesh(m, cpu.statement(case), "slot 0 vs statement")


def test_gpu_mc_max_triangles_is_not_applied():
    case = mc.by_name("gates-base")
    got = []
    for limit in (0, 1):
        with fusion.Fuser(case.params(mc_max_triangles=limit), device=0) as f:
            case.fill(f)
            got.append(extract(f, 8))
    cpu.assert_same_mesh(got[0], got[1], "mc_max_triangles 0 and 1")
    cpu.assert_same_mesh(got[0], cpu.oracle_mesh(case), "mc_max_triangles")
    assert len(got[1]["idx"]) > 1
