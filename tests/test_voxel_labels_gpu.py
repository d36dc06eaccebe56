"""The voxel-task data on the GPU: the kernels of scannet_amd/csrc/voxel_labels.hip against the brute-force checker
tests/voxel_labels_checker.c and against the host path, bit for bit; the bin stage alone against numpy; host and device destinations; the whole stage
on a small synthetic room; bin/voxellabels --device=0 against --host."""
import os
import subprocess

import numpy as np
import pytest

from scannet_amd import freespace, fusion, voxel_labels as vl
from tests import freespace_cases as fc
from tests import voxel_labels_cases as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker():
    L = vc.build_checker()
    if L is None:
        pytest.skip("needs gcc")
    return L


def _same(got, want, what):
    for g, w, name in zip(got, want, ("face", "dist2", "label", "instance", "byte_label")):
        assert vc.same_bits(g, w), "%s: %s differs at %d nodes" % (what, name, int((g != w).sum()) if g.shape == w.shape else -1)


@pytest.mark.parametrize("name", vc.CASE_NAMES + ["far"])
def test_device_equals_the_checker_and_the_host_path(checker, name):
    if name == "far":      # a valid face with a vertex a thousand kilometres away: clamped in float before any tile index is made
        u = vc.unaligned_case()
        case = vc.Case("far", u.dims, u.lo, u.voxel, np.concatenate([u.xyz, [[1e6, 2e6, -1e6]]]), [(0, 1, 2), (3, 4, 6)])
    else:
        case = vc.case(name)
    face, d2 = vl.nearest_faces(case.header(), case.xyz, case.tris, case.band, device=0)
    got = (face, d2) + vl.labels(face, case.tris, case.vlabel, case.vinst)
    _same(got, case.answer(checker), name)
    hf, hd = vl.nearest_faces(case.header(), case.xyz, case.tris, case.band)
    assert vc.same_bits(face, hf) and vc.same_bits(d2, hd)
    f_only, none = vl.nearest_faces(case.header(), case.xyz, case.tris, case.band, device=0, dist2=False)     # dist2 is optional
    assert none is None and vc.same_bits(f_only, face)


def _numpy_bins(case):
    """The tiles of every face, from DESIGN.md section 4m in float32 numpy: {tile index: set of faces}, counts [tz, ty, tx]."""
    f32 = np.float32
    v = case.xyz[case.tris.astype(np.int64)]                              # [nf, 3 vertices, 3]
    a, ab, ac = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]

    def dot(p, q):
        return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]
    with np.errstate(all="ignore"):
        det = dot(ab, ab) * dot(ac, ac) - dot(ab, ac) * dot(ab, ac)
        t = f32(case.band) * f32(case.voxel)
        lo, hi = v.min(1) - t, v.max(1) + t
        t0, t1 = [], []
        for k in range(3):
            n, l = case.dims[k], f32(case.lo[k])
            g0 = np.minimum(np.maximum(np.floor(lo[:, k] / f32(case.voxel) - l) - f32(1), f32(0)), f32(n))
            g1 = np.minimum(np.maximum(np.ceil(hi[:, k] / f32(case.voxel) - l) + f32(1), f32(-1)), f32(n - 1))
            t0.append(g0.astype(np.int64))
            t1.append(g1.astype(np.int64))
    tr = case.tris
    ok = (tr[:, 0] != tr[:, 1]) & (tr[:, 0] != tr[:, 2]) & (tr[:, 1] != tr[:, 2]) & np.isfinite(v).all((1, 2)) & (det > 0) & np.isfinite(det)
    tiles = tuple((n + 7) // 8 for n in case.dims)
    counts = np.zeros(tiles[::-1], np.uint32)
    sets = {}
    for f in np.nonzero(ok)[0]:
        if any(t1[k][f] < t0[k][f] for k in range(3)):
            continue
        for z in range(t0[2][f] // 8, t1[2][f] // 8 + 1):
            for y in range(t0[1][f] // 8, t1[1][f] // 8 + 1):
                for x in range(t0[0][f] // 8, t1[0][f] // 8 + 1):
                    counts[z, y, x] += 1
                    sets.setdefault((z, y, x), set()).add(int(f))
    return counts, sets


@pytest.mark.parametrize("name", ["unaligned", "many", "skipped_all", "soup"])
def test_bin_stage_alone(name):
    """k_vl_count, k_vl_scan, k_vl_fill through the internal hook: per-tile counts equal a numpy count, the offsets are their exclusive scan, and each
    tile's list is the expected set (the order within a tile is free)."""
    case = vc.case(name)
    want_counts, want_sets = _numpy_bins(case)
    counts, offsets, lst = vl.bins(case.header(), case.xyz, case.tris, case.band, device=0)
    assert np.array_equal(counts, want_counts)
    flat = counts.reshape(-1).astype(np.int64)
    assert np.array_equal(offsets.reshape(-1), np.concatenate([[0], np.cumsum(flat)[:-1]])) and len(lst) == flat.sum()
    tz, ty, tx = counts.shape
    for (z, y, x), s in want_sets.items():
        o = int(offsets[z, y, x])
        got = lst[o:o + int(counts[z, y, x])]
        assert len(set(got.tolist())) == len(got) and set(got.tolist()) == s, (z, y, x)
    hc, ho, hl = vl.bins(case.header(), case.xyz, case.tris, case.band)                # the host path bins the same sets
    assert np.array_equal(hc, counts) and np.array_equal(ho, offsets)
    assert np.array_equal(np.sort(hl), np.sort(lst))


def test_device_destinations():
    """face / dist2 and the sample arrays written straight into device memory (torch tensors) hold the bytes of the host destinations."""
    import torch
    case = vc.soup_case()
    nx, ny, nz = case.dims
    face_t = torch.full((nz, ny, nx), 7, dtype=torch.int32, device="cuda:0")
    d2_t = torch.zeros((nz, ny, nx), dtype=torch.float32, device="cuda:0")
    vl.nearest_faces(case.header(), case.xyz, case.tris, case.band, device=0, face_out=face_t, dist2_out=d2_t)
    torch.cuda.synchronize()
    face, d2 = vl.nearest_faces(case.header(), case.xyz, case.tris, case.band, device=0)
    assert vc.same_bits(face_t.cpu().numpy(), face) and vc.same_bits(d2_t.cpu().numpy(), d2)
    grid, bl = vc.sampler_grid(70, seed=5)
    p = vl.default_params(stride=2)
    data, label, xy, total = vl.sample_columns(grid, bl, p, device=0, first=2, max_samples=6)
    assert len(data) == 6
    out = (torch.zeros((6, 1, 62, 31, 31), dtype=torch.float32, device="cuda:0"), torch.zeros((6, 62), dtype=torch.uint8, device="cuda:0"),
           torch.zeros((6, 2), dtype=torch.int32, device="cuda:0"))
    _, _, _, t2 = vl.sample_columns(grid, bl, p, device=0, first=2, max_samples=6, out=out)
    torch.cuda.synchronize()
    assert t2 == total
    assert vc.same_bits(out[0].cpu().numpy(), data) and vc.same_bits(out[1].cpu().numpy(), label) and vc.same_bits(out[2].cpu().numpy(), xy)


@pytest.mark.parametrize("cfg", vc.SAMPLER_CONFIGS, ids=lambda c: "nz%d_%dx%dx%d_z%s_s%d" % c)
def test_device_sampler_equals_numpy_indexing(cfg):
    nz, wx, wy, wz, z0, stride = cfg
    grid, bl = vc.sampler_grid(nz, seed=nz + wx)
    p = vl.default_params(wx=wx, wy=wy, wz=wz, z0=z0, stride=stride)
    want = vc.numpy_samples(grid, bl, wx, wy, wz, z0, stride)
    data, label, xy, total = vl.sample_columns(grid, bl, p, device=0)
    assert total == len(want[2]) == vl.count_columns(grid, bl, p, device=0)
    assert vc.same_bits(data, want[0]) and vc.same_bits(label, want[1]) and vc.same_bits(xy, want[2])
    if total == 0:
        return
    d, l, c, t = vl.sample_columns(grid, bl, p, device=0, first=3, max_samples=4)
    assert t == total and vc.same_bits(d, want[0][3:7]) and vc.same_bits(l, want[1][3:7]) and vc.same_bits(c, want[2][3:7])
    d, l, c, t = vl.sample_columns(grid, bl, p, device=0, first=total - 2, max_samples=5)
    assert len(d) == 2 and vc.same_bits(d, want[0][-2:])
    assert len(vl.sample_columns(grid, bl, p, device=0, first=total + 3, max_samples=5)[0]) == 0
    only = np.where(bl == 255, 255, 0).astype(np.uint8)                    # no selected column
    assert vl.sample_columns(grid, only, p, device=0)[3] == 0


def test_whole_stage_on_a_synthetic_room(checker):
    """32 frames of the empty room at 64 x 48: the 5 cm grid of freespace.carve_sens, the mesh of a fuser with the stage's parameters and box, labels by
    height band.  The device's label grids equal the checker's; every sampled column's label holds a task label; the vertices read their labels back."""
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
    vlabel = (1 + np.clip(np.floor(xyz[:, 2] / 0.5), 0, 5)).astype(np.uint16)          # six bands of half a metre
    vinst = (1 + (xyz[:, 0] > 3.0)).astype(np.uint8)
    scan = vl.label_scan(grid, xyz, tris, vlabel, vinst, device=0)
    nz, ny, nx = grid.value.shape
    case = vc.Case("room", (nx, ny, nz), grid.lo_voxel, grid.voxel_size, xyz, tris)
    case.vlabel, case.vinst = vlabel, vinst
    want = case.answer(checker)
    _same((scan.face, want[1], scan.label, scan.instance, scan.byte_label), want, "room")
    hit = scan.face >= 0
    assert hit.sum() > 20000 and set(np.unique(scan.label[hit])) <= set(range(1, 7)) and len(np.unique(scan.label[hit])) >= 5
    # a surface leaves no hole: every vertex's nearest node carries a label, and it is a label of the vertex's own band or of a neighbouring one
    back = scan.lookup(xyz).astype(np.int64)
    assert (back > 0).all() and (np.abs(back - vlabel) <= 1).all()
    # only a vertex within a node and a half of a band boundary (half a node to its nearest node, a face of at most one node beyond) can read the
    # neighbouring band: 5 boundaries x 2 x 0.075 m of 3 m of wall, a quarter at the most
    assert (back == vlabel).mean() >= 0.75
    p = vl.default_params(stride=8)
    data, label, xy, total = vl.sample_columns(grid, scan.byte_label, p, device=0)
    assert total > 20 and ((label != 0) & (label != 255)).any(axis=1).all()
    hdata, hlabel, hxy, htotal = vl.sample_columns(grid, scan.byte_label, p)
    assert htotal == total and vc.same_bits(data, hdata) and vc.same_bits(label, hlabel) and vc.same_bits(xy, hxy)
    z0 = -int(grid.lo_voxel[2])
    k = min(61, nz - 1 - z0)
    assert np.array_equal(data[:, 0, :k + 1, 15, 15], np.stack([grid.value[z0:z0 + k + 1, y, x] for x, y in xy]))   # the centre column is the grid's


def test_tool_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    paths, case, grid = vc.write_scene_files(tmp_path)
    outs = {}
    for name, flag in (("host", "--host"), ("device", "--device=0")):
        prefix = str(tmp_path / name)
        ids = prefix + ".ids.txt"
        r = subprocess.run(vc.tool_args(paths, prefix, flag, "--stride=2", "--ids-out=" + ids, "--print-stats"), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        assert ("path: " + name) in r.stdout
        outs[name] = [open(prefix + s, "rb").read() for s in (".label.npy", ".instance.npy", ".samples.data.npy", ".samples.label.npy", ".ids.txt")]
    assert outs["host"] == outs["device"] and all(len(b) > 100 for b in outs["host"])
