"""The object-task data on the GPU: the kernels of scannet_amd/csrc/object_voxels.hip against the brute-force checker
tests/object_voxels_checker.c, the exact statement tests/object_voxels_exact.py and the host path, byte for byte; the key / fill stage alone against a
numpy grouping; host and device destinations; the whole stage on a small synthetic room; bin/objectvoxels --device=0 against --host."""
import os
import subprocess

import numpy as np
import pytest

from scannet_amd import freespace, fusion, object_voxels as ov
from tests import freespace_cases as fc
from tests import object_voxels_cases as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker():
    L = oc.build_checker()
    if L is None:
        pytest.skip("needs gcc")
    return L


@pytest.mark.parametrize("name", oc.CASE_NAMES)
def test_device_equals_checker_exact_statement_and_host_path(checker, name):
    case = oc.case(name)
    got, total = case.library(device=0)
    assert oc.same(got, case.answer(checker)) == [], name
    assert oc.same(got, case.exact()) == [], name
    host, host_total = case.library()
    assert oc.same(got, host) == [] and total == host_total
    if name != "empty":
        occ = got[0][:, 0]
        assert len(occ) >= 1 and (occ.reshape(len(occ), -1).sum(1) > 0).all() and (occ == 0).any()    # the case is not idle
    if name == "many":                                                # paging on the device
        for first, cap, n in ((5, 7, 7), (60, 10, 3), (63, 4, 0)):
            page, t = case.library(device=0, first=first, max_objects=cap)
            assert t == total and oc.same(page, tuple(w[first:first + n] for w in got)) == []
        assert case.library(device=0, first=0, max_objects=0)[1] == total


def _numpy_groups(case):
    """DESIGN.md section 4n in numpy: the object of every counted face, 0 elsewhere"""
    t = case.tris.astype(np.int64)
    a, b, c = (case.vobj[t[:, k]] for k in range(3))
    obj = np.where(b == c, b, a)
    ok = (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2]) & np.isfinite(case.xyz[t]).all((1, 2))
    return np.where(ok, obj, 0).astype(np.uint32)


@pytest.mark.parametrize("name", ["shared", "big", "many", "skipped_all", "degenerate"])
def test_key_and_fill_stage_alone(name):
    """k_ov_key, k_ov_scan, k_ov_fill through the internal hook: the object of every face, per-object counts, their exclusive scan, and every object's
    list as a set (the order within an object is free)."""
    case = oc.case(name)
    nobj = len(case.cls)
    want = _numpy_groups(case)
    fobj, counts, offsets, lst = ov.stage_faces(case.xyz, case.tris, case.vobj, nobj, device=0)
    assert np.array_equal(fobj, want) and (want > 0).sum() >= 5
    want_counts = np.bincount(want, minlength=nobj + 1)
    want_counts[0] = 0
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(want_counts)[:-1]])) and len(lst) == want_counts.sum()
    for o in range(1, nobj + 1):
        got = lst[offsets[o]:offsets[o] + counts[o]]
        assert len(set(got.tolist())) == len(got) and set(got.tolist()) == set(np.nonzero(want == o)[0].tolist()), o
    hf, hc, ho, hl = ov.stage_faces(case.xyz, case.tris, case.vobj, nobj)       # the host path groups the same sets
    assert np.array_equal(hf, fobj) and np.array_equal(hc, counts) and np.array_equal(ho, offsets) and np.array_equal(np.sort(hl), np.sort(lst))


def test_device_destinations():
    """The five outputs written straight into device memory (torch tensors) hold the bytes of the host destinations."""
    import torch
    case = oc.case("known_half")
    want, total = case.library(device=0)
    n = 2
    out = (torch.full((n, 2, 30, 30, 30), 7, dtype=torch.uint8, device="cuda:0"), torch.full((n,), 7, dtype=torch.uint8, device="cuda:0"),
           torch.full((n,), 7, dtype=torch.int32, device="cuda:0"), torch.zeros((n, 3), dtype=torch.float32, device="cuda:0"),
           torch.zeros((n,), dtype=torch.float32, device="cuda:0"))
    got, t = case.library(device=0, first=0, max_objects=n, out=out)
    torch.cuda.synchronize()
    assert t == total == 1
    assert oc.same(tuple(o[:1].cpu().numpy() for o in got), want) == []
    assert (out[0][1] == 7).all() and int(out[1][1]) == 7             # beyond the objects there are, nothing is written


def test_whole_stage_on_a_synthetic_room(checker):
    """32 frames of the empty room at 64 x 48: the 5 cm grid of freespace.carve_sens and the mesh of a fuser with the stage's parameters and box; objects
    by height band and x band.  The device's arrays equal the checker's and the host path's; a room seen from inside knows cells it does not occupy."""
    W, H = 64, 48
    sd = fc.make_sens(fc.room_frames(32, W, H), W, H)
    fp = freespace.default_params(voxel_size=0.05)
    grid = freespace.carve_sens(sd, fp)
    sp, lo_b, hi_b = freespace.plan(sd, fp)
    with fusion.Fuser(sp, device=0) as f:
        f.allocate_box(lo_b, hi_b)
        f.run(sd)
        mesh = f.extract_mesh()
        xyz, _, tris = mesh.arrays()
        mesh.close()
    assert len(tris) > 5000
    band = np.clip(np.floor(xyz[:, 2] / 0.5), 0, 5).astype(np.uint32)                   # six bands of half a metre
    vobj = 1 + 2 * band + (xyz[:, 0] > 3.0)                                             # objectIds 0 .. 11
    cls = np.array([1, 3, 4, -1, 5, 9, 13, 18, 20, -1, 22, 30], np.int32)
    case = oc.Case("room", xyz, tris, vobj, cls, grid=grid)
    got, total = case.library(device=0)
    want = case.answer(checker)
    assert oc.same(got, want) == []
    assert oc.same(got, case.library()[0]) == []
    assert total >= 6 and set(got[1]) <= set(cls[cls >= 0].tolist())
    occ, known = got[0][:, 0].astype(bool), got[0][:, 1].astype(bool)
    assert occ.sum() > 200 * total and (known & ~occ).sum() > 1000 and (~known).sum() > 1000
    assert ov.kernel_us()["raster"] > 0


def test_tool_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    paths, xyz, tris, grid = oc.write_scene_files(tmp_path)
    outs = {}
    for name, flag in (("host", "--host"), ("device", "--device=0")):
        os.makedirs(str(tmp_path / name))
        prefix = str(tmp_path / name / "scene")
        r = subprocess.run(oc.tool_args(paths, prefix, flag, "--all-objects", "--print-stats"), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        assert ("path: " + name) in r.stdout and "4 objects" in r.stdout
        outs[name] = [open(prefix + s, "rb").read() for s in (".objects.data.npy", ".objects.label.npy", ".objects.id.npy", ".objects.names.txt")]
    assert outs["host"] == outs["device"] and all(len(b) > 30 for b in outs["host"])
