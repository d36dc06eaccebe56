"""The voxel-task data without a GPU: the host path of scannet_amd/csrc/voxel_labels.cpp against the brute-force checker
tests/voxel_labels_checker.c -- bit for bit on `face`, on the bits of `dist2` and on every label array -- and against analytic answers; the sampler
against plain numpy indexing; the refusals, the read-back, the struct layout, the tool, and the host code once under AddressSanitizer / UBSan as a
stand-alone program (tests/voxel_labels_host_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, freespace, voxel_labels as vl
from tests import voxel_labels_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker():
    L = vc.build_checker()
    if L is None:
        pytest.skip("needs gcc")
    return L


def _host(case):
    face, d2 = vl.nearest_faces(case.header(), case.xyz, case.tris, case.band)
    return (face, d2) + vl.labels(face, case.tris, case.vlabel, case.vinst)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("face", "dist2", "label", "instance", "byte_label")):
        assert vc.same_bits(g, w), "%s: %s differs at %d nodes" % (what, name, int((g != w).sum()) if g.shape == w.shape else -1)


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_host_path_equals_the_checker(checker, name):
    case = vc.case(name)
    want = case.answer(checker)
    got = _host(case)
    assert_same(got, want, name)
    if name not in ("empty_mesh", "empty_grid"):
        assert (want[0] >= 0).sum() > 20                              # the case is not idle
    if name == "many":
        counts, _, _ = vl.bins(case.header(), case.xyz, case.tris, case.band)
        assert counts[0, 0, 1] >= 1000 and (counts[0, :, 2:4] == 0).all() and counts[0, 1, 4] > 0   # eight chunks in one tile; empty tiles between


def test_analytic_plane(checker):
    """A 2 m square at the height of 2.5 nodes over 1/16 m voxels, band 2: a node 0.5 or 1.5 nodes from it has dist2 == dz^2 exactly, the triangle that
    holds its foot point wins, and on the shared diagonal x + y = 1 the lower index does."""
    case = vc.plane_case()
    face, d2 = vl.nearest_faces(case.header(), case.xyz, case.tris, case.band)
    nx, ny, nz = case.dims
    z, y, x = np.meshgrid(*(np.arange(case.lo[a], case.lo[a] + n, dtype=np.float32) * np.float32(case.voxel) for a, n in ((2, nz), (1, ny), (0, nx))),
                          indexing="ij")
    dz = z - np.float32(vc.PLANE_H)
    near = np.abs(dz) <= np.float32(2.0 / 16.0)
    assert near.sum() == 4 * nx * ny
    assert np.array_equal(d2[near], (dz * dz)[near])                  # dyadic: exact
    assert np.isposinf(d2[~near]).all() and (face[~near] == -1).all()
    side = x + y                                                      # exact as well
    assert (face[near & (side <= 1)] == 0).all() and (face[near & (side > 1)] == 1).all()
    assert (near & (side == 1)).sum() >= 4 * 10 and (near & (side > 1)).sum() > 100
    assert_same((face, d2), case.answer(checker)[:2], "plane")


def test_coincident_triangles_the_lower_index_wins(checker):
    for order, first in ((0, 5), (1, 9)):
        case = vc.coincident_case(order)
        face, d2, label, inst, bl = _host(case)
        hit = face >= 0
        assert hit.sum() > 20 and (face[hit] == 0).all()
        assert (label[hit] == first).all() and (bl[hit] == first).all() and (label[~hit] == 0).all()


def test_skipped_faces_change_nothing(checker):
    base, both = vc.skipped_cases()
    fb, db = vl.nearest_faces(base.header(), base.xyz, base.tris, base.band)
    fa, da = vl.nearest_faces(both.header(), both.xyz, both.tris, both.band)
    assert vc.same_bits(fa, fb) and vc.same_bits(da, db) and (fb >= 0).sum() > 200
    n = len(base.tris)
    for i, what in enumerate(vc.SKIPPED):                              # each one alone beside the base mesh
        tris = np.concatenate([both.tris[:n], both.tris[n + i:n + i + 1]])
        f1, d1 = vl.nearest_faces(both.header(), both.xyz, tris, both.band)
        assert vc.same_bits(f1, fb) and vc.same_bits(d1, db), what
    # the good triangle of the first entry, named properly, is not skipped
    nv = len(base.xyz)
    tris = np.concatenate([both.tris[:n], np.array([[nv, nv + 1, nv + 2]], np.uint32)])
    f2, _ = vl.nearest_faces(both.header(), both.xyz, tris, both.band)
    assert (f2 == n).sum() > 5


def test_unaligned_grid_and_far_vertex(checker):
    case = vc.unaligned_case()
    face = _host(case)[0]
    assert set(np.unique(face)) == {-1, 0, 1}
    z, y, x = np.nonzero(face == 0)
    assert x.min() >= 0 and x.max() <= 7 and y.max() <= 7 and z.max() <= 7          # one tile
    z, y, x = np.nonzero(face == 1)
    assert len({(a // 8, b // 8, c // 8) for a, b, c in zip(x, y, z)}) >= 4          # several
    # a valid face with a vertex a thousand kilometres away: clamped before any index is made; host equals checker
    far = vc.Case("far", case.dims, case.lo, case.voxel, np.concatenate([case.xyz, [[1e6, 2e6, -1e6]]]), [(0, 1, 2), (3, 4, 6)])
    assert_same(_host(far), far.answer(checker), "far")


def test_face_majority_rule_all_eight_patterns():
    """(a, b, c) over two values: the value two vertices share; three different values: the first vertex's.  Labels and instances apart."""
    tris = np.arange(27).reshape(9, 3)
    pats = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 1, 1), (1, 2, 2), (2, 1, 2), (2, 2, 1), (2, 2, 2), (5, 6, 7)]
    want = [1, 1, 1, 1, 2, 2, 2, 2, 5]
    vlabel = np.array(pats, np.uint16).reshape(-1) * 10
    vinst = np.array(pats[::-1], np.uint8).reshape(-1)
    face = np.arange(-1, 9, dtype=np.int32)
    label, inst, bl = vl.labels(face, tris, vlabel, vinst)
    assert list(label) == [0] + [10 * w for w in want] and list(bl) == [0] + [10 * w for w in want]
    assert list(inst) == [0] + [5, 2, 2, 2, 2, 1, 1, 1, 1]
    assert (vl.labels(face, tris, vlabel)[1] == 0).all()              # no vertex instances: zeros


def test_byte_label_mapping():
    tris = np.arange(12).reshape(4, 3)
    vlabel = np.repeat(np.array([0, 254, 255, 300], np.uint16), 3)
    label, _, bl = vl.labels(np.array([-1, 0, 1, 2, 3], np.int32), tris, vlabel)
    assert list(label) == [0, 0, 254, 255, 300] and list(bl) == [0, 255, 254, 255, 255]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", vc.SAMPLER_CONFIGS, ids=lambda c: "nz%d_%dx%dx%d_z%s_s%d" % c)
def test_sampler_equals_numpy_indexing(cfg):
    nz, wx, wy, wz, z0, stride = cfg
    grid, bl = vc.sampler_grid(nz, seed=nz + wx)
    p = vl.default_params(wx=wx, wy=wy, wz=wz, z0=z0, stride=stride)
    want = vc.numpy_samples(grid, bl, wx, wy, wz, z0, stride)
    data, label, xy, total = vl.sample_columns(grid, bl, p)
    assert total == len(want[2]) == vl.count_columns(grid, bl, p)
    assert vc.same_bits(data, want[0]) and vc.same_bits(label, want[1]) and vc.same_bits(xy, want[2])
    if z0 == 25:
        assert total == 0
        return
    assert total > 10 and np.isneginf(data).any()                     # windows hang over the border
    assert ((xy[:, 0] < wx // 2) | (xy[:, 0] >= grid.value.shape[2] - wx // 2)).any() and (xy[:, 1] < wy // 2).any()
    # paging: a page in the middle, the last (short) one, one past the end
    d, l, c, t = vl.sample_columns(grid, bl, p, first=3, max_samples=4)
    assert t == total and vc.same_bits(d, want[0][3:7]) and vc.same_bits(l, want[1][3:7]) and vc.same_bits(c, want[2][3:7])
    d, l, c, t = vl.sample_columns(grid, bl, p, first=total - 2, max_samples=5)
    assert len(d) == 2 and vc.same_bits(d, want[0][-2:]) and vc.same_bits(c, want[2][-2:])
    d, l, c, t = vl.sample_columns(grid, bl, p, first=total + 3, max_samples=5)
    assert len(d) == 0 and t == total


def test_sampler_no_selected_column_and_empty_grid():
    grid, bl = vc.sampler_grid(20, seed=2)
    only = np.where(bl == 255, 255, 0).astype(np.uint8)
    data, label, xy, total = vl.sample_columns(grid, only)
    assert total == 0 and data.shape == (0, 1, 62, 31, 31) and label.shape == (0, 62) and xy.shape == (0, 2)
    empty = freespace.Grid(np.zeros((0, 0, 0), np.float32), np.zeros((0, 0, 0), np.uint8), 0.05, (0, 0, 0))
    assert vl.sample_columns(empty, np.zeros((0, 0, 0), np.uint8))[3] == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals and the read-back
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _refused(call, code=-1):
    with pytest.raises(_abi.ScanfuseError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_come_before_anything_is_written():
    case = vc.unaligned_case()
    h = case.header()
    face = np.full((case.dims[2], case.dims[1], case.dims[0]), 77, np.int32)
    d2 = np.full(face.shape, 5.0, np.float32)

    def search(hd=h, tris=case.tris, band=case.band, device=None):
        vl.nearest_faces(hd, case.xyz, tris, band, device, face_out=face, dist2_out=d2)
    bad = case.tris.copy()
    bad[1, 2] = len(case.xyz)
    _refused(lambda: search(tris=bad))                                # a face index >= nv
    for band in (0.0, -1.0, np.nan, np.inf):
        _refused(lambda: search(band=band))
    for voxel in (0.0, -0.05, np.nan, np.inf):
        hd = case.header()
        hd.voxel_size = voxel
        _refused(lambda: search(hd=hd))
    hd = case.header()
    hd.nx = -1
    _refused(lambda: search(hd=hd))
    hd = vl.header((1 << 21, 1 << 21, 1 << 21), 0.05, (0, 0, 0))     # 2^63 nodes
    _refused(lambda: search(hd=hd))
    hd = vl.header(case.dims, 0.05, (1 << 23, 0, 0))                  # node coordinates binary32 cannot hold
    _refused(lambda: search(hd=hd))
    assert (face == 77).all() and (d2 == 5.0).all()
    grid, bl = vc.sampler_grid(20, seed=1)
    for over in (dict(wx=30), dict(wy=0), dict(wx=-3), dict(wz=0), dict(stride=0), dict(wx=(1 << 31) - 1, wy=(1 << 31) - 1, wz=1 << 20)):
        _refused(lambda: vl.sample_columns(grid, bl, vl.default_params(**over), max_samples=0))
    _refused(lambda: vl.labels(np.array([2], np.int32), case.tris, case.vlabel))          # a face that is not there
    _refused(lambda: vl.labels(np.array([0], np.int32), case.tris, case.vlabel[:4]))      # a vertex that is not there


def test_no_gpu_is_a_device_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    case = vc.unaligned_case()
    _refused(lambda: vl.nearest_faces(case.header(), case.xyz, case.tris, case.band, device=0), -5)
    grid, bl = vc.sampler_grid(20, seed=1)
    _refused(lambda: vl.sample_columns(grid, bl, device=0), -5)
    _refused(lambda: vl.bins(case.header(), case.xyz, case.tris, case.band, device=0), -5)


def test_read_back_at_the_mesh_vertices(checker, tmp_path):
    """The two-box scene: freespace.lookup over the label grid, at the mesh's own vertices, gives back their labels; label_scan holds the four grids, its
    samples are the sampler's, and save_npy writes them."""
    case, grid = vc.two_box_scene()
    scan = vl.label_scan(grid, case.xyz, case.tris, case.vlabel, case.vinst)
    want = case.answer(checker)
    assert_same((scan.face, want[1], scan.label, scan.instance, scan.byte_label), want, "two_box")
    assert np.array_equal(scan.lookup(case.xyz), case.vlabel) and np.array_equal(scan.lookup(case.xyz, "instance"), case.vinst)
    assert np.array_equal(freespace.lookup((scan.byte_label, grid.world2grid), case.xyz), case.vlabel)
    data, label, xy, total = scan.samples()
    assert total > 50 and ((label != 0) & (label != 255)).any(axis=1).all()
    paths = scan.save_npy(str(tmp_path / "scene"))
    assert [os.path.basename(p) for p in paths] == ["scene.label.npy", "scene.instance.npy", "scene.samples.data.npy", "scene.samples.label.npy"]
    assert np.array_equal(np.load(paths[0]), scan.label) and np.array_equal(np.load(paths[1]), scan.instance)
    assert vc.same_bits(np.load(paths[2]), data) and vc.same_bits(np.load(paths[3]), label) and data.shape[1:] == (1, 62, 31, 31)


def test_struct_layout_matches_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(sf_voxlabel_params), offsetof(sf_voxlabel_params, wx), offsetof(sf_voxlabel_params, z0),
         offsetof(sf_voxlabel_params, z0_default), offsetof(sf_voxlabel_params, stride), offsetof(sf_voxlabel_params, reserved));
  return 0;
}'''
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = str(tmp_path / "vl_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P = vl.SfVoxlabelParams
    assert got == [C.sizeof(P), P.wx.offset, P.z0.offset, P.z0_default.offset, P.stride.offset, P.reserved.offset]
    p = vl.default_params()
    assert (p.band, p.wx, p.wy, p.wz, p.z0_default, p.stride) == (vc.BAND, 31, 31, 62, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------------------------------------------------------------------------
def python_products(paths, case, grid, device=None, **over):
    from scannet_amd import project
    inst, label, _ = project.vertex_ids(paths["segs"], paths["agg"], paths["tsv"], len(case.xyz))
    scan = vl.label_scan(grid, case.xyz, case.tris, label, inst, vl.default_params(**over), device)
    return scan, label


def test_tool_host_equals_python(tmp_path):
    paths, case, grid = vc.write_scene_files(tmp_path)
    scan, vlabel = python_products(paths, case, grid, stride=2)
    assert sorted(np.unique(vlabel)) == [2, 3]                        # chair, table: 1-based lines of the label map
    want = scan.save_npy(str(tmp_path / "py"))
    prefix = str(tmp_path / "tool")
    ids = str(tmp_path / "ids.txt")
    r = subprocess.run(vc.tool_args(paths, prefix, "--host", "--stride=2", "--print-stats", "--ids-out=" + ids), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert "nodes" in r.stdout and "samples" in r.stdout
    for w in want:
        got = prefix + w[len(str(tmp_path / "py")):]
        assert open(got, "rb").read() == open(w, "rb").read(), got
    # the per-vertex read-back, one id per line (util_3d.export_ids)
    assert [int(x) for x in open(ids).read().split("\n") if x] == [int(v) for v in scan.lookup(case.xyz)]
    assert open(ids).read().endswith("\n")
    # a page of samples, a small window, a band
    r = subprocess.run(vc.tool_args(paths, prefix + "2", "--host", "--window=5x5x7", "--z0=1", "--max-samples=3", "--band=1.5"), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    scan2, _ = python_products(paths, case, grid, wx=5, wy=5, wz=7, z0=1, band=1.5)
    d, l, _, _ = scan2.samples(0, 3)
    assert vc.same_bits(np.load(prefix + "2.samples.data.npy"), d) and vc.same_bits(np.load(prefix + "2.samples.label.npy"), l)
    assert np.array_equal(np.load(prefix + "2.label.npy"), scan2.label)
    # refusals: an even window, a missing file; nothing is written
    r = subprocess.run(vc.tool_args(paths, prefix + "3", "--host", "--window=4x5x7"), capture_output=True, text=True)
    assert r.returncode == 1 and "(-1)" in r.stderr and not os.path.exists(prefix + "3.label.npy")
    r = subprocess.run(vc.tool_args(dict(paths, ply=paths["ply"] + ".none"), prefix + "3", "--host"), capture_output=True, text=True)
    assert r.returncode == 1 and not os.path.exists(prefix + "3.label.npy")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the host code under AddressSanitizer / UBSan, as a program of its own
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_host_code_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "voxel_labels_host_san")
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "voxel_labels_host_main.cpp"),
           os.path.join(ROOT, "scannet_amd", "csrc", "voxel_labels.cpp"), "-lpthread"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.strip() == "voxel labels host: ok"
