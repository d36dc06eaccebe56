"""Global alignment of keyframes by joint dense depth alignment (DESIGN.md "Global alignment"; scannet_amd/csrc/align.hip).

BundleFusion's solver is not in the reference tree, so the rule is pinned the way the tracker's is:
  * without a GPU: tests/align_checker.c restates the solver in C; a planar scene converges to the truth, the furnished room stays within the
    tracker's bound, the structural cases (thin pairs, unconnected and lost frames, a singular system, refused arguments), sf_align_pairs against a
    numpy restatement, sf_align_spread against the checker, the parameter surface, the tool's refusals, the kernels' resources;
  * -m gpu: sf_fuser_align_system and sf_fuser_align against the checker bit for bit, the volume untouched, stream order, the correction loop
    align_and_reintegrate, bin/depthsensing --track --align.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, synth
from tests import solver_scenes as ss
from tests.solver_scenes import DRIFT_R, DRIFT_T, WALK_TOTAL, f32, perturb, pose_error, random_poses, worst_pose_error as worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "depthsensing")
FIXTURE = os.path.join(ROOT, "tests", "golden", "zParametersBundlingScanNet.txt")
SF_ERR_INVALID_ARG = -1
W, H = 320, 240
# On noise-free planes the residual at the true poses is zero up to rounding and the 1 mm depth step: the truth is the solver's fixed point
# (the bound test_track.py::test_checker_room_corner_converges uses on this scene)
CORNER_T_BOUND, CORNER_R_BOUND = 1e-3, 1e-3    # metres, radians
# the project's bound for tracked poses on the furnished room (DESIGN.md "Camera tracking")
ROOM_T_BOUND, ROOM_R_BOUND = 0.015, 0.005


@pytest.fixture(scope="module")
def chk():
    """tests/align_checker.c is there to be compiled; the tests reach it through tests/solver_scenes.py."""
    if not ss.checkers_available():
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    return ss.align_lib()


def frame_of(W_=W, H_=H):
    return ss.align_frame(W_, H_)


def fuser_params(voxel=0.008, W_=W, H_=H):
    return ss.fuser_params(W_, H_, ss.NO_COLOUR, voxel, num_sdf_blocks=1 << 17)


def cpu_align(depth, poses, pairs, a, fr=None):
    """The depth-only alignment (no pictures): the colour term's result fields are 0."""
    rc, out, res = ss.cpu_align(depth, poses, pairs, a, fr or frame_of())
    assert rc != 0 or (res.colour_correspondences == 0 and res.colour_rms_first == 0.0 and res.colour_rms_last == 0.0)
    return rc, out, res


def cpu_system(depth, poses, pairs, a, fr=None):
    """The depth-only systems (no pictures): 29 sums per pair, the colour term's two are 0."""
    rc, sys = ss.cpu_align_system(depth, poses, pairs, a, fr or frame_of())
    assert not sys[:, 29:].any()
    return rc, np.ascontiguousarray(sys[:, :29])


def res_tuple(r):
    """The depth term's fields of sf_align_result."""
    return ss.align_res_tuple(r)[:8]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Scenes (rendered once per module)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corner():
    """Test 1's input: 6 noise-free views of the room corner along a 50 cm arc about the vertical through it (10 cm of arc per keyframe), all looking
    at the corner."""
    return ss.corner_arc(6, W, H, metres=0.1)


@pytest.fixture(scope="module")
def room():
    """Test 2's input: 8 views of the furnished room 10 cm apart, sensor noise 2."""
    boxes = synth.clutter_boxes()
    truth = [synth.trajectory_pose(10 * k, WALK_TOTAL) for k in range(8)]
    depth = np.stack([synth.render_room_depth(p, W, H, noise_frame=10 * k, noise=2, boxes=boxes).reshape(-1) for k, p in enumerate(truth)])
    return depth, np.stack(truth).astype(np.float32), ss.drifted(truth)


@pytest.fixture(scope="module")
def corner_cpu(chk, corner):
    """The checker's answer on test 1's input (shared with the GPU tests)."""
    from scannet_amd import fusion
    depth, truth, start = corner
    a = fusion.default_align_params()
    pairs, count = fusion.align_pairs(start, a)
    assert count == len(pairs)
    rc, out, res = cpu_align(depth, start, pairs, a)
    assert rc == 0
    return pairs, out, res


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: convergence on the checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_checker_planar_scene_converges_to_the_truth(corner, corner_cpu):
    depth, truth, start = corner
    pairs, out, res = corner_cpu
    e0 = pose_error(start[5], truth[5])
    assert e0[0] > 0.039 and e0[1] > 0.019
    et, er = worst(out, truth)
    print("corner: worst %.3f mm / %.3f mrad, %s" % (et * 1e3, er * 1e3, res.as_dict()))
    assert res.status == 0 and res.frames_unconnected == 0 and res.frames_rejected == 0, res.as_dict()
    assert len(pairs) == 30 and res.pairs_used == 30
    assert et < CORNER_T_BOUND and er < CORNER_R_BOUND, (et, er, res.as_dict())
    assert out[0].tobytes() == start[0].reshape(16).tobytes()   # the fixed frame
    assert all(o[12:].tolist() == [0.0, 0.0, 0.0, 1.0] for o in out)


def test_checker_furnished_scene_stays_within_the_trackers_bound(chk, room):
    from scannet_amd import fusion
    depth, truth, start = room
    e0 = pose_error(start[7], truth[7])
    assert e0[0] > 0.055 and e0[1] > 0.027
    a = fusion.default_align_params()
    pairs, count = fusion.align_pairs(start, a)
    assert count == len(pairs)
    rc, out, res = cpu_align(depth, start, pairs, a)
    assert rc == 0
    et, er = worst(out, truth)
    print("room: worst %.3f mm / %.3f mrad, %s" % (et * 1e3, er * 1e3, res.as_dict()))
    assert res.status == 0 and res.frames_unconnected == 0 and res.frames_rejected == 0, res.as_dict()
    assert et < ROOM_T_BOUND and er < ROOM_R_BOUND, (et, er, res.as_dict())
    assert res.rms_last < res.rms_first, res.as_dict()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: structure
# ---------------------------------------------------------------------------------------------------------------------------------------------
def structure_cases(corner):
    return ss.structure_cases(corner, W, H)


def check_structure(name, poses, out, res):
    if name == "thin":
        assert res.status == 0 and res.pairs_used == 2 and res.frames_unconnected == 1 and res.iterations >= 1, res.as_dict()
        assert out[2].tobytes() == poses[2].tobytes()
        assert out[1].tobytes() != poses[1].tobytes()
    elif name == "lost":
        assert res.status == 0 and res.pairs_used == 2 and res.frames_unconnected == 0, res.as_dict()
        assert np.isneginf(out[1]).all()
        assert out[2].tobytes() != poses[2].tobytes()
    else:
        assert res.status == 1 and res.iterations == 0, res.as_dict()
        assert out.tobytes() == poses.tobytes()


@pytest.mark.parametrize("name", ["thin", "lost", "planes"])
def test_checker_structure(chk, corner, name):
    from scannet_amd import fusion
    depth, poses, pairs = structure_cases(corner)[name]
    rc, out, res = cpu_align(depth, poses, pairs, fusion.default_align_params())
    assert rc == 0
    check_structure(name, poses, out, res)


def test_nothing_connected_is_status_2(chk, corner):
    from scannet_amd import fusion
    depth, truth, start = corner
    a = fusion.default_align_params(min_pair_correspondences=W * H)   # more than a level-1 image holds
    rc, out, res = cpu_align(depth[:3], start[:3], np.array([[0, 1], [1, 2]], np.int32), a)
    assert rc == 0 and res.status == 2 and res.frames_unconnected == 2 and res.pairs_used == 0
    assert out.tobytes() == start[:3].tobytes()


REFUSED = [("one_frame", dict(K=1)), ("fixed_out_of_range", dict(fixed_frame=3)), ("fixed_negative", dict(fixed_frame=-1)), ("no_pairs", dict(P=0)),
           ("self_pair", dict(pairs=[[0, 1], [2, 2]])), ("pair_out_of_range", dict(pairs=[[0, 3]])), ("level_4", dict(level=4))]


@pytest.mark.parametrize("name,case", REFUSED)
def test_refused_arguments(chk, corner, name, case):
    """Refused by the checker and, before the fuser is looked at, by the C ABI: the same with or without a GPU."""
    from scannet_amd import fusion
    depth, truth, start = corner
    K = case.get("K", 3)
    pairs = np.array(case.get("pairs", [[0, 1], [1, 0]]), np.int32)
    P = case.get("P", len(pairs))
    a = fusion.default_align_params(**{k: v for k, v in case.items() if k in ("fixed_frame", "level")})
    poses = np.ascontiguousarray(start[:3], np.float32).reshape(3, 16)
    d = np.ascontiguousarray(depth[:3])
    out = np.zeros_like(poses)
    res = fusion.SfAlignResult()
    fr = frame_of()
    assert chk.al_align(C.byref(fr), d.ctypes.data, None, K, poses.ctypes.data, pairs.ctypes.data, P, C.byref(a), out.ctypes.data, C.byref(res)) == -1
    sys = np.zeros((max(P, 1), 31))
    assert chk.al_system(C.byref(fr), d.ctypes.data, None, K, poses.ctypes.data, pairs.ctypes.data, P, C.byref(a), sys.ctypes.data) == -1
    L = _abi.lib()
    PP, RP = C.POINTER(fusion.SfAlignParams), C.POINTER(fusion.SfAlignResult)
    L.sf_fuser_align.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, PP, C.c_void_p, RP]
    L.sf_fuser_align_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, PP, C.c_void_p, RP]
    L.sf_fuser_align_system.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, PP, C.c_void_p]
    assert L.sf_fuser_align(None, d.ctypes.data, K, poses.ctypes.data, pairs.ctypes.data, P, C.byref(a), out.ctypes.data, C.byref(res)) == SF_ERR_INVALID_ARG
    assert "NULL fuser" not in L.sf_last_error().decode()
    assert L.sf_fuser_align_device(None, d.ctypes.data, W * H * 2, K, poses.ctypes.data, pairs.ctypes.data, P, C.byref(a), out.ctypes.data,
                                   C.byref(res)) == SF_ERR_INVALID_ARG
    assert "NULL fuser" not in L.sf_last_error().decode()
    assert L.sf_fuser_align_system(None, d.ctypes.data, K, poses.ctypes.data, pairs.ctypes.data, P, C.byref(a), sys.ctypes.data) == SF_ERR_INVALID_ARG
    assert "NULL fuser" not in L.sf_last_error().decode()
    good = fusion.default_align_params()
    gp = np.array([[0, 1]], np.int32)
    assert L.sf_fuser_align(None, d.ctypes.data, 3, poses.ctypes.data, gp.ctypes.data, 1, C.byref(good), out.ctypes.data, C.byref(res)) == SF_ERR_INVALID_ARG
    assert "NULL fuser" in L.sf_last_error().decode()


def test_checker_refuses_a_size_that_is_no_level(chk, corner):
    from scannet_amd import fusion
    depth, truth, start = corner
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    for dw, dh in ((100, 60), (80, 0), (20, 15)):
        rc, _, _ = cpu_align(depth[:2], start[:2], pairs, fusion.default_align_params(down_width=dw, down_height=dh))
        assert rc == -1, (dw, dh)
    # 80 x 60 is level 2 of 320 x 240, whatever `level` says
    a = fusion.default_align_params(down_width=80, down_height=60, level=0)
    rc, s1 = cpu_system(depth[:2], start[:2], pairs, a)
    rc2, s2 = cpu_system(depth[:2], start[:2], pairs, fusion.default_align_params(level=2))
    assert rc == 0 and rc2 == 0 and s1.tobytes() == s2.tobytes() and s1[0, 28] > 1000


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: sf_align_pairs and sf_align_spread (host only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def numpy_pairs(poses, max_dist, max_angle):
    """The rule of sf_align_pairs in float64."""
    P = poses.astype(np.float64).reshape(-1, 4, 4)
    out = []
    for i in range(len(P)):
        for j in range(i + 1, len(P)):
            take = j == i + 1
            if not take:
                d = P[j, :3, 3] - P[i, :3, 3]
                dist = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                M = P[i, :3, :3].T @ P[j, :3, :3]
                v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
                th = np.arctan2(0.5 * np.sqrt(v @ v), 0.5 * (np.trace(M) - 1.0))
                take = dist <= max_dist and th <= max_angle
            if take:
                out += [(i, j), (j, i)]
    return np.array(out, np.int32).reshape(-1, 2)


def test_align_pairs_equals_numpy(chk):
    from scannet_amd import fusion
    poses = random_poses(40, 7)
    a = fusion.default_align_params()
    want = numpy_pairs(poses, float(np.float32(a.pair_max_dist)), float(np.float32(a.pair_max_angle)))
    assert 2 * 39 < len(want) < 40 * 39     # the distance rule adds pairs and leaves pairs out
    got, count = fusion.align_pairs(poses, a)
    assert count == len(want) and np.array_equal(got, want)
    cap = len(want) // 2 + 1               # odd: the capacity falls between the two pairs of a couple
    got, count = fusion.align_pairs(poses, a, capacity=cap)
    assert count == len(want) and np.array_equal(got, want[:cap])
    out = np.zeros((count, 2), np.int32)
    n = C.c_uint64(0)
    p16 = np.ascontiguousarray(poses).reshape(-1, 16)
    assert chk.al_pairs(p16.ctypes.data, len(p16), C.byref(a), out.ctypes.data, count, C.byref(n)) == 0
    assert n.value == count and np.array_equal(out, want)
    # a frame without a finite pose is in no pair
    p16[3, 7] = np.nan
    p16[10] = -np.inf
    got, _ = fusion.align_pairs(p16, a)
    assert len(got) and not np.isin(got, [3, 10]).any()


def test_align_spread_equals_the_checker(chk):
    from scannet_amd import fusion
    n = 50
    poses = np.stack([synth.trajectory_pose(3 * i, WALK_TOTAL) for i in range(n)]).astype(np.float32).reshape(n, 16)
    keys = np.arange(2, n, 7, dtype=np.uint64)             # 2, 9, 16, ..., 44: frames 0 and 1 lie before the first keyframe
    for lost in (0, 12, 13, 30, 23):                        # before the first keyframe, between keyframes, at a keyframe (23)
        poses[lost] = -np.inf
    assert 23 in keys
    new = np.stack([perturb(poses[int(k)].reshape(4, 4), 0.004 * q, rad=0.002 * q) if np.isfinite(poses[int(k)]).all() else poses[int(k)].reshape(4, 4)
                    for q, k in enumerate(keys)]).astype(np.float32).reshape(-1, 16)
    new[5] = np.nan                                        # keyframe 37 came back without a pose: its frames follow keyframe 30
    got = fusion.align_spread(poses, keys, new)
    want = np.empty_like(poses)
    assert chk.al_spread(poses.ctypes.data, n, keys.ctypes.data, len(keys), new.ctypes.data, want.ctypes.data) == 0
    assert got.tobytes() == want.tobytes()
    for lost in (0, 12, 13, 30, 23):
        assert np.isneginf(got[lost]).all()
    for q, k in enumerate(keys):
        if q != 5 and int(k) != 23:
            assert got[int(k)].tobytes() == new[q].tobytes()
    # frames before the first keyframe take its correction; frames behind the lost keyframe 23 keep following keyframe 16
    D = new[0].reshape(4, 4).astype(np.float64) @ np.linalg.inv(poses[2].reshape(4, 4).astype(np.float64))
    assert np.allclose(got[1].reshape(4, 4), D @ poses[1].reshape(4, 4), atol=1e-5)
    D = new[2].reshape(4, 4).astype(np.float64) @ np.linalg.inv(poses[16].reshape(4, 4).astype(np.float64))
    assert np.allclose(got[25].reshape(4, 4), D @ poses[25].reshape(4, 4), atol=1e-5)
    # identical new poses: nothing moves beyond rounding, and lost frames stay lost
    same = fusion.align_spread(poses, keys, poses[keys.astype(np.int64)])
    fin = np.isfinite(poses).all(axis=1)
    assert np.allclose(same[fin], poses[fin], atol=1e-6) and np.isneginf(same[~fin]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: parameters and layouts
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_align_params_default_and_file(tmp_path):
    from scannet_amd import fusion
    a = fusion.default_align_params()
    assert (a.level, a.down_width, a.down_height, a.max_iters) == (1, 0, 0, 8)
    assert (a.dist_thres, a.normal_thres, a.depth_min, a.depth_max, a.early_out) == (f32(0.15), f32(0.7), 0.0, 0.0, f32(1e-5))
    assert (a.min_pair_correspondences, a.fixed_frame) == (500, 0)
    assert (a.pair_max_dist, a.pair_max_angle, a.max_translation, a.max_rotation) == (f32(1.0), f32(0.6), f32(0.5), f32(0.5))
    b = fusion.load_align_params(FIXTURE)
    assert (b.dist_thres, b.normal_thres, b.depth_min, b.depth_max) == (f32(0.15), f32(0.95), f32(0.5), f32(4.0))
    assert (b.down_width, b.down_height, b.max_iters) == (80, 60, 3)
    assert (b.level, b.early_out, b.min_pair_correspondences, b.pair_max_dist) == (1, f32(1e-5), 500, f32(1.0))   # no key of the file
    plain = tmp_path / "plain.txt"
    plain.write_text("s_SDFVoxelSize = 0.010f;\ns_denseDepthMax = 3.5f;\n")
    c = fusion.load_align_params(plain)
    assert c.depth_max == f32(3.5)
    c.depth_max = 0.0
    assert bytes(c) == bytes(fusion.default_align_params())
    bad = tmp_path / "bad.txt"
    for text in ("s_denseDistThresh = far;\n", "s_denseNormalThresh = nan;\n", "s_downsampledWidth = ;\n"):
        bad.write_text(text)
        with pytest.raises(_abi.ScanfuseError):
            fusion.load_align_params(bad)


def test_the_fixture_is_the_reference_file():
    text = open(FIXTURE).read()
    for key in ("s_denseDistThresh = 0.15f", "s_denseNormalThresh = 0.95f", "s_submapSize = 10", "s_numGlobalNonLinIterations = 3", "s_downsampledWidth = 80"):
        assert key in text, key


def test_align_structs_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sf_align_params), offsetof(sf_align_params, dist_thres), offsetof(sf_align_params, early_out),
         offsetof(sf_align_params, fixed_frame), offsetof(sf_align_params, max_rotation), offsetof(sf_align_params, reserved), sizeof(sf_align_result),
         offsetof(sf_align_result, frames_rejected), offsetof(sf_align_result, correspondences), offsetof(sf_align_result, rms_last));
  return 0;
}'''
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = str(tmp_path / "al_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    from scannet_amd import fusion
    P, R = fusion.SfAlignParams, fusion.SfAlignResult
    assert got == [C.sizeof(P), P.dist_thres.offset, P.early_out.offset, P.fixed_frame.offset, P.max_rotation.offset, P.reserved.offset, C.sizeof(R),
                   R.frames_rejected.offset, R.correspondences.offset, R.rms_last.offset]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the tool's refusals, the kernels' resources
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_depthsensing_refuses_align_without_track_and_with_ranks(tmp_path):
    if not os.path.exists(TOOL):
        pytest.skip("bin/depthsensing is built by build()")
    (tmp_path / "p.txt").write_text("s_SDFVoxelSize = 0.010f;\n")
    (tmp_path / "t.txt").write_text("s_maxLevels = 3;\n")
    base = [str(tmp_path / "p.txt"), str(tmp_path / "t.txt"), str(tmp_path / "none.sens")]
    for flag in ("--align", "--align=4"):
        r = subprocess.run([TOOL] + base + [flag], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--track" in r.stderr and "--align" in r.stderr, r.stderr
    r = subprocess.run([TOOL, "--ranks", "2", "--share-gpu"] + base + ["--align"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--track" in r.stderr, r.stderr
    r = subprocess.run([TOOL, "--ranks", "2", "--share-gpu"] + base + ["--track", "--align"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--ranks" in r.stderr, r.stderr
    r = subprocess.run([TOOL] + base + ["--track", "--align=0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0


def test_align_kernels_live_in_registers():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kr = ss.kernel_resources()
    rows = kr.kernels(os.path.join(ROOT, "scannet_amd", "libscanfuse.so"))
    every = [(kr.short(n), r) for r, n in zip(rows, kr.demangle([r["name"] for r in rows]))]
    mine = [(s, r) for s, r in every if s.startswith("k_align_")]
    assert {s.split("<")[0] for s, _ in mine} == {"k_align_prep", "k_align_assoc", "k_align_final"}
    assert len([s for s, _ in mine if s.startswith("k_align_prep<")]) == 4   # one per level
    # one association body per solver, instantiated without and with the colour row; nothing else associates
    assert sorted(s for s, _ in every if "assoc" in s) == ["k_align_assoc<false>", "k_align_assoc<true>", "k_track_assoc<false>", "k_track_assoc<true>"]
    assert sorted(s for s, _ in mine if "final" in s) == ["k_align_final<false>", "k_align_final<true>"]
    for s, r in mine:
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (s, r)
        assert r["lds"] <= 160 * 1024, (s, r["lds"])
    assoc = [r for s, r in mine if s == "k_align_assoc<false>"][0]
    assert assoc["lds"] == 464


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernels against the checker, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_fuser(room):
    """A fuser holding 10 fused frames of the furnished room."""
    from scannet_amd import fusion
    f = fusion.Fuser(fuser_params(), device=0)
    boxes = synth.clutter_boxes()
    for i in range(10):
        pose = synth.trajectory_pose(i, WALK_TOTAL)
        assert f.integrate(synth.render_room_depth(pose, W, H, noise_frame=i, noise=2, boxes=boxes), pose)
    f.sync()
    yield f
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1, 2])
def test_gpu_systems_bit_exact(chk, room, gpu_fuser, level):
    """K = 4, P = 7: both directions of three pairs and one pair of frames that face away from each other.  Level 2 is 80 x 60 = 4 800 pixels, 18.75
    workgroups: the last one is partial."""
    from scannet_amd import fusion
    depth, truth, start = room
    d = depth[[0, 2, 5, 7]]
    poses = start[[0, 2, 5, 7]].copy()
    back = poses[3].copy()
    back[:3, 0] *= -1.0   # turned half a turn about the image's y axis: the camera looks the other way
    back[:3, 2] *= -1.0
    poses[3] = back
    pairs = np.array([[0, 1], [1, 0], [1, 2], [2, 1], [0, 2], [2, 0], [0, 3]], np.int32)
    a = fusion.default_align_params(level=level)
    rc, want = cpu_system(d, poses, pairs, a)
    assert rc == 0
    got = gpu_fuser.align_system(d, poses, pairs, a)
    assert got.shape == (7, 29) and got.tobytes() == want.tobytes(), (level, np.abs(got - want).max())
    assert (want[:4, 28] > 1000 >> (2 * level)).all() and (want[4:6, 28] > 0).all(), want[:, 28]   # the comparison is not of empty systems
    assert not want[6].any()


@pytest.mark.gpu
def test_gpu_buffers_grow_on_demand_and_never_go_stale(chk, room):
    """One fuser's alignment buffers through their three states: made for K = 2, P = 2 at level 2 (80 x 60: a partial last workgroup), every one of them
    grown for K = 4, P = 7 at level 0, and the small problem again in the larger buffers."""
    from scannet_amd import fusion
    depth, truth, start = room
    small = (depth[:2], start[:2], np.array([[0, 1], [1, 0]], np.int32), fusion.default_align_params(level=2))
    big = (depth[[0, 2, 5, 7]], start[[0, 2, 5, 7]], np.array([[0, 1], [1, 0], [1, 2], [2, 1], [0, 2], [2, 0], [0, 3]], np.int32),
           fusion.default_align_params(level=0))
    want = {}
    for name, (d, poses, pairs, a) in (("small", small), ("big", big)):
        rc, want[name] = cpu_system(d, poses, pairs, a)
        assert rc == 0 and (want[name][:2, 28] > 1000 >> (2 * a.level)).all(), want[name][:, 28]   # the comparison is not of empty systems
    with fusion.Fuser(fuser_params(), device=0) as f:
        for step, (name, (d, poses, pairs, a)) in enumerate((("small", small), ("big", big), ("small", small))):
            got = f.align_system(d, poses, pairs, a)
            assert got.shape == want[name].shape and got.tobytes() == want[name].tobytes(), (step, name, np.abs(got - want[name]).max())


@pytest.mark.gpu
def test_gpu_a_size_that_is_no_level_is_refused(room, gpu_fuser):
    from scannet_amd import fusion
    depth, truth, start = room
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    with pytest.raises(_abi.ScanfuseError):
        gpu_fuser.align(depth[:2], start[:2], pairs, fusion.default_align_params(down_width=100, down_height=60))
    out, res = gpu_fuser.align(depth[:2], start[:2], pairs, fusion.default_align_params(down_width=80, down_height=60, level=0))
    out2, res2 = gpu_fuser.align(depth[:2], start[:2], pairs, fusion.default_align_params(level=2))
    assert out.tobytes() == out2.tobytes() and res_tuple(res) == res_tuple(res2) and res.status == 0


@pytest.mark.gpu
def test_gpu_solve_bit_exact_and_leaves_the_volume_alone(corner, corner_cpu, gpu_fuser):
    import torch
    from scannet_amd import fusion
    depth, truth, start = corner
    pairs, want, want_res = corner_cpu
    f = gpu_fuser
    before, st0 = ss.volume_digest(f), f.stats()
    a = fusion.default_align_params()
    out, res = f.align(depth, start, pairs, a)
    assert res_tuple(res) == res_tuple(want_res), (res.as_dict(), want_res.as_dict())
    assert out.tobytes() == want.tobytes()
    et, er = worst(out, truth)
    assert et < CORNER_T_BOUND and er < CORNER_R_BOUND
    d = torch.from_numpy(depth.astype(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    out2, res2 = f.align_device(d, W * H * 2, start, pairs, a)
    assert out2.tobytes() == out.tobytes() and res_tuple(res2) == res_tuple(res)
    assert ss.volume_digest(f) == before and f.stats() == st0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["thin", "lost", "planes"])
def test_gpu_structure_bit_exact(chk, corner, gpu_fuser, name):
    from scannet_amd import fusion
    depth, poses, pairs = structure_cases(corner)[name]
    a = fusion.default_align_params()
    rc, want, want_res = cpu_align(depth, poses, pairs, a)
    out, res = gpu_fuser.align(depth, poses, pairs, a)
    assert rc == 0 and res_tuple(res) == res_tuple(want_res) and out.tobytes() == want.tobytes()
    check_structure(name, poses, out, res)


@pytest.mark.gpu
def test_gpu_align_sees_queued_work_and_leaves_it_intact(corner, corner_cpu):
    """An align right after an un-synchronised integrate: the same answer, and the integrate's effect is in the volume afterwards."""
    from scannet_amd import fusion
    depth, truth, start = corner
    pairs, want, want_res = corner_cpu
    boxes = synth.clutter_boxes()
    frames = [(synth.render_room_depth(synth.trajectory_pose(i, WALK_TOTAL), W, H, noise_frame=i, noise=2, boxes=boxes), synth.trajectory_pose(i, WALK_TOTAL))
              for i in range(3)]
    with fusion.Fuser(fuser_params(), device=0) as a, fusion.Fuser(fuser_params(), device=0) as b:
        for d, pose in frames:
            assert a.integrate(d, pose)
            out, res = a.align(depth, start, pairs)      # queued behind the integrate, not waited for
            assert out.tobytes() == want.tobytes() and res_tuple(res) == res_tuple(want_res)
            assert b.integrate(d, pose)
            b.sync()
        assert a.stats()["frames_integrated"] == 3
        assert ss.volume_digest(a) == ss.volume_digest(b)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the loop and the tool
# ---------------------------------------------------------------------------------------------------------------------------------------------
LOOP_N, LOOP_STEP = 24, 3     # 24 frames 3 cm apart; keyframes every 4: 12 cm


def _loop_scan(tmp_path, poses_in_file):
    from scannet_amd import sens
    K = synth.intrinsic_matrix(W, H)
    boxes = synth.clutter_boxes()
    truth = [synth.trajectory_pose(LOOP_STEP * i, WALK_TOTAL) for i in range(LOOP_N)]
    sd = sens.SensorData.create(0, 0, W, H, K, K, sensor_name="StructureSensor")
    for i, t in enumerate(truth):
        sd.add_frame(synth.render_room_depth(t, W, H, noise_frame=i, noise=2, boxes=boxes), poses_in_file[i], timestamp_depth=i)
    path = str(tmp_path / "scan.sens")
    sd.save(path)
    sd.close()
    return path, truth


@pytest.mark.gpu
def test_gpu_align_and_reintegrate(tmp_path):
    """Test 2's drift scaled to 24 frames: frame i starts i / 23 x (56 mm, 28 mrad) off the truth."""
    from scannet_amd import fusion, sens
    truth = [synth.trajectory_pose(LOOP_STEP * i, WALK_TOTAL) for i in range(LOOP_N)]
    start = np.stack([perturb(t, 7 * DRIFT_T * i / (LOOP_N - 1), rad=7 * DRIFT_R * i / (LOOP_N - 1)) if i else t for i, t in enumerate(truth)]).astype(np.float32)
    path, _ = _loop_scan(tmp_path, start)
    sd = sens.SensorData(path)
    clean = synth.render_room_depth(truth[-1], W, H, noise=0, boxes=synth.clutter_boxes()).astype(np.float32) / 1000.0
    with fusion.Fuser(fuser_params(0.008), device=0) as f:
        for i in range(LOOP_N):
            assert f.integrate(sd.frames[i].decompress_depth(), start[i])

        def model():
            return f.raycast(truth[-1], normals=False, color=False)[0]

        d_before = model()
        integrated = np.ascontiguousarray(start.reshape(LOOP_N, 16))
        held = integrated.copy()
        target, res, stats = fusion.align_and_reintegrate(f, sd, integrated, every=4)
        assert res.status == 0 and res.frames_unconnected == 0 and res.frames_rejected == 0, res.as_dict()
        assert integrated.tobytes() == target.tobytes()
        moved = int((held != target).any(axis=1).sum())   # the frames of the fixed keyframe 0 stay where they are
        assert stats["frames_moved"] == moved and moved >= LOOP_N - 4, (stats, moved)
        for k in range(0, LOOP_N, 4):
            et, er = pose_error(target[k].reshape(4, 4), truth[k])
            assert et < ROOM_T_BOUND and er < ROOM_R_BOUND, (k, et, er)
        d_after = model()
        ok = (d_before > 0) & (d_after > 0) & (clean > 0)   # the pixels both models and the scene have
        print("hits: %d before, %d after, %d shared with the scene" % ((d_before > 0).sum(), (d_after > 0).sum(), ok.sum()))
        assert ok.sum() > 0.25 * W * H
        e_before, e_after = float(np.abs(d_before[ok] - clean[ok]).mean()), float(np.abs(d_after[ok] - clean[ok]).mean())
        print("model error at frame 23: %.2f mm before, %.2f mm after" % (e_before * 1e3, e_after * 1e3))
        assert e_after < e_before, (e_before, e_after)
    sd.close()


@pytest.mark.gpu
def test_gpu_depthsensing_track_align(tmp_path):
    from scannet_amd import fusion, sens
    truth = [synth.trajectory_pose(LOOP_STEP * i, WALK_TOTAL) for i in range(LOOP_N)]
    path, _ = _loop_scan(tmp_path, [truth[0]] + [np.eye(4, dtype=np.float32)] * (LOOP_N - 1))   # the converter's identity poses after frame 0
    params = tmp_path / "zParametersScanNet.txt"
    params.write_text("s_SDFVoxelSize = 0.008f;\ns_hashNumSDFBlocks = 131072;\ns_hashNumBuckets = 500000;\n")
    tracking = tmp_path / "zParametersTrackingDefault.txt"
    tracking.write_text("s_maxLevels = 3;\ns_maxOuterIter = 10 5 4;\n")
    out_sens = tmp_path / "out.sens"
    r = subprocess.run([TOOL, str(params), str(tracking), path, "--track", "--align=4", "--write-sens=%s" % out_sens], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Aligned" in r.stdout, r.stdout
    assert os.path.getsize(str(tmp_path / "scan_vh.ply")) > 1000
    # the same in Python
    sd = sens.SensorData(path)
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.load_params(params, base=fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my))
    t = fusion.load_track_params(tracking)
    with fusion.Fuser(gp, device=0) as f:
        poses, _ = fusion.track_and_fuse(f, [sd.frames[i].decompress_depth() for i in range(LOOP_N)], truth[0], params=t)
        integrated = np.ascontiguousarray(np.stack(poses).astype(np.float32).reshape(LOOP_N, 16))
        target, res, _ = fusion.align_and_reintegrate(f, sd, integrated, every=4)
    sd.close()
    got = sens.SensorData(str(out_sens))
    assert len(got.frames) == LOOP_N
    for i in range(LOOP_N):
        assert np.asarray(got.frames[i].camera_to_world, np.float32).tobytes() == target[i].tobytes(), i
    got.close()
