"""The free-space stage without a GPU: the checker tests/freespace_checker.c against analytic answers, the plan against the
checker's restatement and against what the checker finds outside it, the grid file, the refusal to run without a GPU, and the host code once under
AddressSanitizer / UBSan as a stand-alone program (tests/freespace_host_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, freespace, fusion, synth
from tests import freespace_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 120
VOXEL = 0.05


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    L = fc.build_checker(tmp_path_factory.mktemp("fs"))
    if L is None:
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    return L


def _params(width=W, height=H, **over):
    fx, fy, mx, my = synth.intrinsics(width, height)
    return fusion.default_params(depth_width=width, depth_height=height, fx=fx, fy=fy, mx=mx, my=my, voxel_size=VOXEL, **over)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the checker against analytic answers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_checker_plane_known_answers(checker):
    """One 2 m plane frame at the identity pose: the state of every lattice node that projects inside the image follows from its camera z alone."""
    sp = _params()
    lo, dims = np.array([-36, -30, -4], np.int32), np.array([72, 60, 58], np.int32)
    vol = fc.Volume(checker, fc.checker_params(sp), lo, dims)
    assert vol.integrate(synth.plane_frame(W, H, 2000), np.eye(4, dtype=np.float32))
    sdf, w = vol.export()
    task, w1 = vol.export(task=True)
    assert np.array_equal(w, w1)
    v32 = np.float32(VOXEL)
    gz, gy, gx = np.meshgrid(*(np.arange(lo[a], lo[a] + dims[a]) for a in (2, 1, 0)), indexing="ij")
    x, y, z = (g.astype(np.float32) * v32 for g in (gx, gy, gz))     # the rule's own world coordinates: exact products of float32
    z64 = z.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = x.astype(np.float64) / z64 * sp.fx + sp.mx
        v = y.astype(np.float64) / z64 * sp.fy + sp.my
    # "projects inside the image": the rule casts (int)(u + 0.5) and accepts (-1, W); 0.1 of a pixel either side of that edge is left to neither set
    inside = (z64 > 0) & (u > -1.4) & (u < W - 0.6) & (v > -1.4) & (v < H - 0.6)
    outside = (z64 <= 0) | (u < -1.6) | (u > W - 0.4) | (v < -1.6) | (v > H - 0.4)
    t = np.float32(np.float64(np.float32(0.02)) * 2.0 + np.float64(np.float32(0.06)))    # fmaf(trunc_scale, 2, trunc_base), one rounding
    s = 2.0 - z64                                                                        # exact in binary32 as well wherever |s| <= t (Sterbenz)
    front, band, behind = inside & (s > t), inside & (s > -np.float64(t)) & (s <= t), inside & (s <= -np.float64(t))
    assert front.sum() > 10000 and band.sum() > 2000 and behind.sum() > 2000 and outside.sum() > 20000
    assert (w[front] == 1).all() and (sdf[front] == t).all()                             # in front by more than the truncation: +trunc, exactly
    assert (w[band] == 1).all() and np.abs(sdf[band].astype(np.float64) - s[band]).max() <= 1e-6
    assert (w[behind] == 0).all() and (sdf[behind] == 0).all()                           # at or beyond the truncation behind the plane: never touched
    assert (w[outside] == 0).all()
    # the task volume: voxel units where something was observed, -inf elsewhere (provider.lua:80-97 reads "known" as value >= -1)
    assert np.array_equal(task[w > 0], sdf[w > 0] / v32) and np.isneginf(task[w == 0]).all()
    assert (task[front] == t / v32).all() and (task[w > 0] >= -1.0 * (t / v32)).all()
    vol.close()


@pytest.fixture(scope="module")
def room(checker):
    """The noise-free empty room, 160 x 120, 48 poses of the walk, 5 cm voxels, fused by the checker into the plan's box enlarged by one ring of blocks."""
    frames = fc.room_frames(48, W, H)
    sd = fc.make_sens(frames, W, H)
    fp = freespace.default_params(voxel_size=VOXEL)
    sp, lo_b, hi_b = freespace.plan(sd, fp)
    lo = (lo_b.astype(np.int64) - 1) * 8
    dims = (hi_b.astype(np.int64) - lo_b + 3) * 8
    vol = fc.Volume(checker, fc.checker_params(sp), lo, dims)
    for d, pose in frames:
        assert vol.integrate(d, pose)
    sdf, w = vol.export()
    vol.close()
    return dict(frames=frames, sens=sd, fuser_params=sp, lo_block=lo_b, hi_block=hi_b, lo=lo, dims=dims, sdf=sdf, weight=w)


def test_checker_room_known_space(room):
    """Nothing further than 0.15 m outside a wall is known (0.15 > trunc(4 m) = 0.14); at least half of what lies further than 0.15 m inside is.
    On the 5 cm lattice "further than 0.15 m" is "at least 4 nodes": the walls of the 6 x 4 x 3 m room are the nodes 0 and 120, 80, 60."""
    lo, dims, w = room["lo"], room["dims"], room["weight"]
    walls = np.array([round(r / VOXEL) for r in synth.ROOM])
    g = [np.arange(lo[a], lo[a] + dims[a]) for a in range(3)]
    out = [(g[a] < -3) | (g[a] > walls[a] + 3) for a in range(3)]
    ins = [(g[a] > 3) & (g[a] < walls[a] - 3) for a in range(3)]
    outside = out[2][:, None, None] | out[1][None, :, None] | out[0][None, None, :]
    inside = ins[2][:, None, None] & ins[1][None, :, None] & ins[0][None, None, :]
    known = w > 0
    assert outside.sum() > 10 * inside.sum() > 0
    assert not known[outside].any(), int(known[outside].sum())
    share = known[inside].mean()
    print("known share of the voxels more than 0.15 m inside the room: %.3f of %d" % (share, inside.sum()))
    assert share >= 0.5


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _ring_is_unknown(w):
    inner = np.zeros(w.shape, bool)
    inner[8:-8, 8:-8, 8:-8] = True
    return not (w[~inner] > 0).any(), int((w[inner] > 0).sum())


def test_plan_matches_the_checker_and_bounds_the_room(checker, room):
    sp, lo_b, hi_b = room["fuser_params"], room["lo_block"], room["hi_block"]
    poses = np.stack([p for _, p in room["frames"]])
    fx, fy, mx, my = synth.intrinsics(W, H)
    lo_c, hi_c, blocks, R = fc.plan(checker, W, H, fx, fy, mx, my, poses, VOXEL)
    assert np.array_equal(lo_c, lo_b) and np.array_equal(hi_c, hi_b)
    assert blocks == np.prod(hi_b.astype(np.int64) - lo_b + 1) and sp.num_sdf_blocks >= blocks
    assert sp.hash_num_buckets * sp.hash_bucket_size >= 2 * blocks
    assert 5.0 < R < 5.2                                              # zfar 4.14 m x sqrt(1 + (81 / 144.47)^2 + (61 / 144.47)^2)
    assert sp.voxel_size == float(np.float32(VOXEL)) and sp.gc_enabled == 0 and sp.color_width == 0 and (sp.depth_width, sp.depth_height) == (W, H)
    ok, known = _ring_is_unknown(room["weight"])
    assert ok and known > 100000
    # every other frame, lost poses among them, and the integration size of the shipped parameter file
    poses2 = poses.copy()
    poses2[4] = poses2[10] = -np.inf
    frames2 = [(d, poses2[i]) for i, (d, _) in enumerate(room["frames"])]
    sd2 = fc.make_sens(frames2, W, H)
    sp2, lo2, hi2 = freespace.plan(sd2, freespace.default_params(voxel_size=0.1, every=2))
    lo_c, hi_c, blocks, _ = fc.plan(checker, W, H, fx, fy, mx, my, poses2, 0.1, every=2)
    assert np.array_equal(lo_c, lo2) and np.array_equal(hi_c, hi2)


def test_plan_bounds_a_camera_that_looks_out_of_the_box(checker):
    """Two cameras turned 30 degrees (and one pitched down) in front of a plane at 3.99 m, just inside the integration distance: their frusta leave the
    box of the camera centres by almost the whole reach.  The checker, over the plan's box and one more ring of blocks, updates nothing in the ring."""
    a = np.deg2rad(30.0)
    yaw = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    pitch = np.array([[1, 0, 0, 0], [0, np.cos(a), -np.sin(a), 0], [0, np.sin(a), np.cos(a), 0], [0, 0, 0, 1]])
    T0, T1 = yaw.copy(), yaw @ pitch
    T0[:3, 3] = (0.3, -0.2, 0.1)
    T1[:3, 3] = (0.9, 0.4, 0.2)
    frames = [(synth.plane_frame(W, H, 3990), T0.astype(np.float32)), (synth.plane_frame(W, H, 3990), T1.astype(np.float32))]
    sd = fc.make_sens(frames, W, H)
    sp, lo_b, hi_b = freespace.plan(sd, freespace.default_params(voxel_size=VOXEL))
    fx, fy, mx, my = synth.intrinsics(W, H)
    lo_c, hi_c, _, R = fc.plan(checker, W, H, fx, fy, mx, my, np.stack([T0, T1]), VOXEL)
    assert np.array_equal(lo_c, lo_b) and np.array_equal(hi_c, hi_b)
    lo = (lo_b.astype(np.int64) - 1) * 8
    dims = (hi_b.astype(np.int64) - lo_b + 3) * 8
    vol = fc.Volume(checker, fc.checker_params(sp), lo, dims)
    for d, pose in frames:
        assert vol.integrate(d, pose)
    _, w = vol.export()
    vol.close()
    ok, known = _ring_is_unknown(w)
    assert ok and known > 100000
    # the bound is not idle: along the image corners the known voxels lie well beyond zfar = 4.14 m from the nearer camera centre, and none beyond R
    gz, gy, gx = np.nonzero(w > 0)
    pts = (np.stack([gx, gy, gz], 1) + lo) * VOXEL
    far = np.minimum(np.linalg.norm(pts - T0[:3, 3], axis=1), np.linalg.norm(pts - T1[:3, 3], axis=1)).max()
    assert 4.5 < far <= R + 1e-3, (far, R)


def test_plan_refuses_a_box_beyond_max_blocks(room):
    with pytest.raises(_abi.ScanfuseError) as e:
        freespace.plan(room["sens"], freespace.default_params(voxel_size=VOXEL, max_blocks=1000))
    n = int(np.prod(room["hi_block"].astype(np.int64) - room["lo_block"] + 1))
    assert e.value.code == -6 and str(n) in str(e.value)               # SF_ERR_CAPACITY, with the count
    lost = fc.make_sens([(synth.plane_frame(W, H), fc.NEG_INF_POSE)] * 3, W, H)
    with pytest.raises(_abi.ScanfuseError) as e:
        freespace.plan(lost, freespace.default_params())
    assert e.value.code == -1                                          # SF_ERR_INVALID_ARG: no valid pose


# ---------------------------------------------------------------------------------------------------------------------------------------------
# grid files
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _grid():
    rng = np.random.default_rng(5)
    w = rng.integers(0, 4, (6, 5, 7)).astype(np.uint8)
    value = np.where(w > 0, rng.normal(0, 1.5, w.shape), -np.inf).astype(np.float32)
    return freespace.Grid(value, w, VOXEL, (-9, 3, -2), frames_used=48)


def _expected_bytes(g):
    nz, ny, nx = g.value.shape
    head = b"SFGRID1\0" + np.array([nx, ny, nz], "<i4").tobytes() + np.array([g.voxel_size], "<f4").tobytes() + g.lo_voxel.astype("<i4").tobytes()
    head += g.world2grid.astype("<f4").tobytes() + np.array([g.frames_used], "<u8").tobytes()
    return head + g.value.astype("<f4").tobytes() + g.weight.tobytes()


def test_grid_file_round_trip(tmp_path):
    g = _grid()
    path = str(tmp_path / "a.grid")
    g.save(path)
    raw = open(path, "rb").read()
    assert raw == _expected_bytes(g)                                   # the layout, field by field
    r = freespace.load_grid(path)
    assert np.array_equal(r.value, g.value) and np.array_equal(r.weight, g.weight) and np.array_equal(r.lo_voxel, g.lo_voxel)
    assert np.array_equal(r.world2grid, g.world2grid) and r.frames_used == 48 and r.voxel_size == g.voxel_size
    assert np.array_equal(r.known, g.weight > 0)
    r.save(str(tmp_path / "b.grid"))
    assert open(str(tmp_path / "b.grid"), "rb").read() == raw          # byte for byte
    m = g.world2grid
    assert m[0, 0] == np.float32(1) / np.float32(VOXEL) and m[0, 3] == 9.5 and m[1, 3] == -2.5 and m[2, 3] == 2.5 and m[3, 3] == 1
    grid_npy, w2g_npy = g.save_npy(str(tmp_path / "scene0000_00"))
    assert np.array_equal(np.load(grid_npy), g.value) and np.array_equal(np.load(w2g_npy), g.world2grid)
    empty = freespace.Grid(np.zeros((0, 0, 0), np.float32), np.zeros((0, 0, 0), np.uint8), VOXEL, (0, 0, 0))
    empty.save(str(tmp_path / "e.grid"))
    assert freespace.load_grid(str(tmp_path / "e.grid")).value.shape == (0, 0, 0)


@pytest.mark.parametrize("case", ["magic", "negative", "short", "long", "size", "nan", "inf", "header_only", "empty"])
def test_grid_file_malformed_is_a_format_error(tmp_path, case):
    raw = bytearray(_expected_bytes(_grid()))
    if case == "magic":
        raw[0:8] = b"SFGRID2\0"
    elif case == "negative":
        raw[12:16] = np.array([-5], "<i4").tobytes()
    elif case == "short":
        raw = raw[:-1]
    elif case == "long":
        raw += b"\0"
    elif case == "size":
        raw[16:20] = np.array([7], "<i4").tobytes()
    elif case == "nan":
        raw[20:24] = np.array([np.nan], "<f4").tobytes()
    elif case == "inf":
        raw[20:24] = np.array([np.inf], "<f4").tobytes()
    elif case == "header_only":
        raw = raw[:108]
    elif case == "empty":
        raw = raw[:0]
    path = str(tmp_path / "bad.grid")
    open(path, "wb").write(bytes(raw))
    with pytest.raises(_abi.ScanfuseError) as e:
        freespace.load_grid(path)
    assert e.value.code == -3                                          # SF_ERR_FORMAT


def test_lookup_is_the_reference_helpers_read():
    """export_semantic_label_grid_for_evaluation.py:40-47 in plain numpy: world2grid, floor, clamp, grid[z, y, x]."""
    g = _grid()
    rng = np.random.default_rng(8)
    nz, ny, nx = g.value.shape
    nodes = np.stack([rng.integers(-2, nx + 2, 300), rng.integers(-2, ny + 2, 300), rng.integers(-2, nz + 2, 300)], 1)
    verts = ((nodes + g.lo_voxel) * VOXEL + rng.uniform(-0.4, 0.4, (300, 3)) * VOXEL).astype(np.float32)   # within 0.4 voxels of a lattice node
    got = freespace.lookup(g, verts)
    want = np.empty(300, np.float32)
    for i, p in enumerate(verts):
        q = g.world2grid @ np.array([p[0], p[1], p[2], 1.0], np.float32)
        x, y, z = (int(np.clip(np.floor(q[a]), 0, n - 1)) for a, n in ((0, nx), (1, ny), (2, nz)))
        want[i] = g.value[z, y, x]
    assert np.array_equal(got, want)
    # floor(g) is the NEAREST node: the vertex reads the node it was scattered around (clamped into the grid)
    near = np.clip(nodes, 0, [nx - 1, ny - 1, nz - 1])
    assert np.array_equal(got, g.value[near[:, 2], near[:, 1], near[:, 0]])
    assert np.array_equal(freespace.lookup((g.value, g.world2grid), verts), got)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# no GPU, no grid
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_no_gpu_is_a_device_error_and_writes_nothing(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    frames = [(synth.plane_frame(64, 48), np.eye(4, dtype=np.float32))] * 2
    sd = fc.make_sens(frames, 64, 48)
    with pytest.raises(_abi.ScanfuseError) as e:
        freespace.carve_sens(sd)
    assert e.value.code == -5 and "no CPU fallback" in str(e.value)    # SF_ERR_DEVICE
    path = str(tmp_path / "scan.sens")
    sd.save(path)
    r = subprocess.run([os.path.join(ROOT, "bin", "freespace"), path], capture_output=True, text=True)
    assert r.returncode == 1 and "(-5)" in r.stderr and r.stdout == ""
    assert sorted(os.listdir(str(tmp_path))) == ["scan.sens"]


def test_struct_layouts_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(sf_freespace_params), offsetof(sf_freespace_params, params_file), sizeof(sf_freespace_stats),
         offsetof(sf_freespace_stats, seconds_plan), sizeof(sf_grid_header), offsetof(sf_grid_header, world2grid), offsetof(sf_grid_header, frames_used));
  return 0;
}'''
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = str(tmp_path / "fs_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, S, G = freespace.SfFreespaceParams, freespace.SfFreespaceStats, freespace.SfGridHeader
    assert got == [C.sizeof(P), P.params_file.offset, C.sizeof(S), S.seconds_plan.offset, C.sizeof(G), G.world2grid.offset, G.frames_used.offset]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the host code under AddressSanitizer / UBSan, as a program of its own
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_host_code_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "freespace_host_san")
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "freespace_host_main.cpp"),
           os.path.join(ROOT, "scannet_amd", "csrc", "freespace.cpp"), "-lpthread"]
    subprocess.run(cmd, check=True)
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.strip() == "freespace host: ok"
