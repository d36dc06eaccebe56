"""The GPU mesh clean, kernel by kernel (scannet_amd/csrc/clean_gpu.hip: the four clean.mlx filters as sorts, a round-by-round resolution of the greedy
clustering and a lock-free union-find).

Three parties:
  * the HIP kernels through the stage hooks of include/scanfuse_internal.h (meshclean.clean_stage_merge / _faces / _components / _compact), each of which
    runs ONE of the four helpers that sf_mesh_clean_gpu is the composition of;
  * the host filter scannet_amd/csrc/clean.cpp and the restatement oracle/clean_oracle.py, which tests/test_clean_stages_cpu.py (default suite) holds to
    the statement on every case;
  * tests/clean_exact.py, the statement: brute force over all pairs in numpy.float32, frozensets, breadth-first search.

This module (-m gpu): every case of tests/clean_cases.py through the hooks, to the byte against the statement -- target, verdicts, triples, root, sizes, keep,
counters, used, remap, gathered arrays; error codes where a case names one; the k_settle launch count, 1 <= launches <= max depth + 1 (the kernel's racy
reads can only settle a vertex earlier), exactly 1 where no vertex has a lower neighbour; the occupied cells against the grid formula; the whole cases
through the product against statement and host filter, and the product against the composition of the hooks.  There is no tolerance anywhere.

Findings: none in the code -- the statement, the host filter, the restatement and the device agree on every case.  chain130 and chain130-reversed take 130
launches (the bound is tight), one-cell-300 127 of at most 127, apart130 one.

One-line mutations of clean_gpu.hip (values and predicates only, never an address, a bound or a loop count), each built into a scratch copy of the library
and run under this module once on the device; the tests that failed under it (counts are test ids of this module, 161 in all; "whole" =
test_gpu_whole_cases_through_the_product, which fails wherever the stage's error reaches the product's arrays or statistics):
   1. dist < radius as <=                          6: test_gpu_merge_stage[cells], [cells-mirrored] (the "at r" neighbours that sit exactly at r), [rounding]; whole on the same three
   2. the distance as fmaf(ez, ez, fmaf(ey, ey, ex * ex))   2: test_gpu_merge_stage[rounding], whole[rounding] -- the 80 + 80 disagreement pairs are the only inputs that can tell
   3. the distance summed as ex2 + (ey2 + ez2)     2: the same two
   4. ti == i && dropped                           18: test_gpu_merge_stage[chain7], [chain130], [chain130-reversed], [absorbed-neighbour-only], [one-cell-300], [cloud-V64], [-V255],
                                                   [-V256], [-V257]; whole on the same nine
   5. i < best dropped                             14: test_gpu_merge_stage[chain130-evens-first], [two-centres], [one-cell-300], [cloud-V64], [-V255], [-V256], [-V257]; whole on the same
   6. the cell sort's end bit 63 as 60             2: test_gpu_merge_stage[keys-alias-bits-60-62] (targets 5, 6, 7: the runs of keys equal in their low 60 bits interleave), whole on it
   7. << 42 as << 41 in pack_cell                  2: test_gpu_merge_stage[keys-2300m-xyz], [keys-minus-2300m-xyz], by the occupied-cell count alone (17 for 18: two cells share a
                                                   key).  No target can change: every look-up goes through the same function of the cell, a shared key only puts the members of two
                                                   cells into one run in index order, and the distance test decides as before
   8. side always -1                               28: test_gpu_merge_stage[cells*] (all four), [r1e-6-box-1m], [-3m], [rounding], [chain130-reversed], [cloud-V63] .. [-V257]; whole on the same
   9. k_pos_keys without + 0.0f                    4: test_gpu_merge_stage[r0-signed-zeros], [r0-subnormals]; whole on both
  10. k_run_heads without the kz comparison        18: test_gpu_merge_stage[r0-runs-1-2-70], [r0-xy-equal-z-differs], [r0-subnormals], [r0-lattice-V63] .. [-V257]; whole on the same
  11. k_remap_faces without a == c                 52: test_gpu_faces_stage[degenerate-ac], [ids-from-65536], [ids-near-the-limit], [through-target], [all-degenerate], [F1-degenerate],
                                                   [random-F*] (four); 42 of whole
  12. sort3 without its third exchange             49: test_gpu_faces_stage[six-corner-orders], [three-and-four-copies], [lower-two-agree], [highest-agrees], [ids-near-the-limit],
                                                   [through-target], [all-but-one-duplicate], [random-F*] (four); 38 of whole
  13. k_dup_flags without the k2 comparison        42: test_gpu_faces_stage[lower-two-agree], [through-target], [random-F*] (four); 36 of whole
  14. k_edge_keys emitting (a, b) for (c, a)       43: test_gpu_components_stage[grids-touching-in-a-vertex*] (both), [third-edge-of-one], [-of-both], [-chain], [random-F*] (three); 35 of whole
  15. k_link hooking the smaller root under the larger   20: test_gpu_components_stage on every case with a component of two faces or more (all but islands257* and F1); root is invisible in
                                                   the product's output, so whole passes
  16. size < min_faces as <=                       22: test_gpu_components_stage[strip2000-shuffled], [grids-touching-in-a-vertex-shuffled], [sizes-6-7-8-1-min1], [-min6], [-min7], [-min8],
                                                   [islands257], [F1], [third-edge-*] (three); 11 of whole
  17. k_count_merged testing threadIdx.x == 0      38: test_gpu_merge_stage on every case with a merged vertex outside the first wave of a block, [count-lanes-from-64] and
                                                   [count-last-partial-wave] among them (19); whole on the same
  18. k_gather_vertices reading colour at w        24: test_gpu_compact_stage[V63-last-unused-colour] .. [V300-last-unused-colour] (seven); 17 of whole (the cases with colour)
  19. k_mark_used leaving out c                    23: test_gpu_compact_stage[V63 .. V300]-last-unused-colour and -last-used (fourteen); 9 of whole
side < 0.5 as <= 0.5 was run too: none failed, and none can.  It differs for a point exactly in the middle of its cell, which then looks at the lower
neighbour cells instead of the upper ones.  A neighbour within r is strictly closer than half a cell (2 r (1 + 1e-5)) on every axis, so it lies in the
point's own cell either way: the choice of side adds nothing there."""
import numpy as np
import pytest

from scannet_amd import meshclean
from scannet_amd._abi import ScanfuseError
from scannet_amd.segmentator import Mesh
from tests import clean_cases as cc
from tests import clean_exact as cx
from tests import test_clean_stages_cpu as cpu

pytestmark = pytest.mark.gpu

GPU_STAGES = (lambda pos, r: meshclean.clean_stage_merge(pos, r)["target"], meshclean.clean_stage_faces, meshclean.clean_stage_components,
              meshclean.clean_stage_compact)


@pytest.mark.parametrize("case", cc.MERGE_CASES, ids=repr)
def test_gpu_merge_stage(case):
    """radius > 0: k_cell_keys, the cell sort, the run-length encode, the scan, the k_settle rounds; radius == 0: k_pos_keys, k_iota, both sorts, k_gather64,
    k_run_heads, the max-scan, k_targets_from_heads; k_count_merged on both paths.  Or the error the case names, from the hook and from the product."""
    if case.error is not None:
        with pytest.raises(ScanfuseError) as e:
            meshclean.clean_stage_merge(case.pos, case.r)
        assert e.value.code == case.error
        with pytest.raises(ScanfuseError) as e:
            meshclean.clean(Mesh.from_arrays(case.pos, np.zeros((0, 3), np.uint32)), float(case.r), 0, gpu=0)
        assert e.value.code == case.error
        return
    got = meshclean.clean_stage_merge(case.pos, case.r)
    want = cpu.stated_target(case.name)
    cpu._same({"target": got["target"], "merged": got["merged"]}, {"target": want, "merged": int((want != np.arange(len(want))).sum())}, case.name)
    if case.r > 0:
        depth = cpu.stated_depth(case.name)
        print("%s: %d launches, max depth %d" % (case.name, got["launches"], depth))
        assert 1 <= got["launches"] <= depth + 1, (got["launches"], depth)
        assert got["cells"] == cc.occupied_cells(case.pos, case.r)
    else:
        assert (got["launches"], got["cells"]) == (0, 0)


@pytest.mark.parametrize("case", cc.FACE_CASES, ids=repr)
def test_gpu_faces_stage(case):
    """k_remap_faces, k_face_keys, k_iota, the two sorts, k_gather64, k_dup_flags and both selects."""
    cpu._same(meshclean.clean_stage_faces(case.nv, case.tri, case.target), cx.faces(case.tri, case.target), case.name)


@pytest.mark.parametrize("case", cc.COMP_CASES, ids=repr)
def test_gpu_components_stage(case):
    """k_edge_keys, the sort, k_iota, k_link, k_roots, k_component_flags: a component's root is its lowest face."""
    cpu._same(meshclean.clean_stage_components(case.tri, case.min_faces), cx.components(case.tri, case.min_faces), case.name)


@pytest.mark.parametrize("case", cc.COMPACT_CASES, ids=repr)
def test_gpu_compact_stage(case):
    """k_mark_used, the scan, k_gather_vertices, k_remap_tris."""
    cpu._same(meshclean.clean_stage_compact(case.pos, case.col, case.tri), cx.compact(case.pos, case.col, case.tri), case.name)


@pytest.mark.parametrize("w", cpu.WHOLE, ids=lambda w: w[0])
def test_gpu_whole_cases_through_the_product(w):
    """sf_mesh_clean_gpu: arrays and every statistic against the statement and the host filter, and against the composition of the four hooks."""
    name, pos, col, tri, r, mf = w
    sx, sc, stri, sst, _ = cpu.stated_whole(name)
    got, st = cpu.host_clean(pos, col, tri, r, mf, gpu=0)
    cpu._arrays_same(got, (sx, sc, stri), name)
    assert st == sst, (st, sst)
    host, hst = cpu.host_clean(pos, col, tri, r, mf)
    cpu._arrays_same(got, host, name + " host")
    assert st == hst
    cpos, ccol, ctri, cst = cc.run_stages(GPU_STAGES, pos, col, tri, r, mf)
    cpu._arrays_same(got, (cpos, ccol, ctri), name + " composed")
    assert cst == st
