"""Camera tracking against the fused volume (DESIGN.md "Camera tracking"; scannet_amd/csrc/track.hip).

The upstream tracker is not in the reference tree, so the rule is pinned here the way the ray cast is:
  * without a GPU: tests/track_checker.c restates the tracker in C; with the CPU oracle fusing and tests/raycast_checker.c rendering, the whole
    chain runs on the CPU: a room corner converges from a 2 cm / 2 degree guess, degenerate and empty inputs are lost, and a 30-frame
    track-and-fuse loop over the furnished room follows the true trajectory; the parameter surface of the C ABI;
  * -m gpu: sf_fuser_track_system and sf_fuser_track against the checker bit for bit, the volume untouched, the GPU loop reproducing the CPU chain
    (poses and volume bytes), stream order, the lost cases, bin/depthsensing --track.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, synth
from tests import solver_scenes as ss
from tests.solver_scenes import f32, perturb, pose_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "depthsensing")
SF_ERR_INVALID_ARG = -1
W, H = 320, 240
LOOP_FRAMES, LOOP_TOTAL = ss.LOOP_FRAMES, ss.WALK_TOTAL   # the walk's 12 m perimeter in 1200 frames: 1 cm per frame
# Bounds measured on the CPU chain (DESIGN.md "Camera tracking") and fixed with margin: the corner converged to 0.095 mm / 0.08 mrad, the loop's
# worst frame was 7.4 mm / 1.8 mrad off
CORNER_T_BOUND, CORNER_R_BOUND = 1e-3, 1e-3   # metres, radians
LOOP_T_BOUND, LOOP_R_BOUND = 0.015, 0.005


@pytest.fixture(scope="module")
def chk():
    """tests/raycast_checker.c and tests/track_checker.c are there to be compiled."""
    if not ss.checkers_available():
        pytest.skip("needs gcc and a CPU with fused multiply-add")


def params_pair(oracle, W=W, H=H, voxel=0.004, **over):
    """Oracle and fuser parameters of the same camera and volume."""
    from scannet_amd import fusion
    op = ss.oracle_params(oracle, W, H, voxel)
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, voxel_size=voxel, fx=fx, fy=fy, mx=mx, my=my, num_sdf_blocks=1 << 18)
    for k, v in over.items():
        setattr(gp, k, v)
    return op, gp


def cpu_track(vol, op, depth, guess, t, ref=None, model=None):
    """The depth-only tracker on the CPU (no picture) over an oracle volume or exported blocks -> (pose [4,4] f32, result)."""
    code, pose, res = ss.cpu_track(vol, op, depth, guess, t, ref=ref, model=model)
    assert code == 0 and res.colour_correspondences == 0 and res.colour_rms_residual == 0.0
    return pose, res


def cpu_system(vol, op, depth, level, T, Tref, t):
    """The depth-only system (no picture): 29 sums, the colour term's two are 0."""
    code, sys, mask = ss.cpu_system(vol, op, depth, level, T, Tref, t)
    assert code == 0 and sys[29] == 0.0 and sys[30] == 0.0
    return sys[:29], mask


def res_tuple(r):
    """The depth term's fields of sf_track_result."""
    return ss.track_res_tuple(r)[:5]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
corner_truth = ss.corner_truth


def corner_frames():
    """The truth and two nearby views, noise free."""
    return ss.corner_frames(W, H)


def oracle_corner(oracle):
    op, _ = params_pair(oracle)
    vol = oracle.Volume(op, threads=8)
    for d, p in corner_frames():
        vol.integrate(d, p)
    return op, vol


def plane_pose():
    return np.eye(4, dtype=np.float32)


def loop_frames():
    return ss.loop_frames(W, H)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the chain oracle -> raycast_checker -> track_checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_checker_room_corner_converges(chk, oracle):
    from scannet_amd import fusion
    op, vol = oracle_corner(oracle)
    truth = corner_truth()
    depth = corner_frames()[0][0]
    t = fusion.default_track_params()
    for dt, deg, axis in ((0.02, 2.0, (0.3, -0.5, 0.8)), (0.02, -2.0, (1.0, 0.2, -0.1)), (0.015, 1.5, (0.0, 1.0, 0.3))):
        guess = perturb(truth, dt, deg=deg, axis=axis)
        e0 = pose_error(guess, truth)
        assert e0[0] > 0.01 and e0[1] > 0.02
        pose, res = cpu_track(vol, op, depth, guess, t, ref=truth)
        assert res.tracked == 1 and res.lost_reason == 0, res_tuple(res)
        et, er = pose_error(pose, truth)
        assert et < CORNER_T_BOUND and er < CORNER_R_BOUND, (et, er, res_tuple(res))
        assert res.correspondences > 0.5 * W * H and res.rms_residual < 2e-3
        assert pose[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    vol.close()


def test_checker_single_plane_is_lost(chk, oracle):
    from scannet_amd import fusion
    op, _ = params_pair(oracle)
    vol = oracle.Volume(op, threads=8)
    plane = synth.plane_frame(W, H)
    vol.integrate(plane, plane_pose())
    guess = perturb(plane_pose(), 0.01, deg=1.0)
    pose, res = cpu_track(vol, op, plane, guess, fusion.default_track_params(), ref=plane_pose())
    assert res.tracked == 0 and res.lost_reason == 3, res_tuple(res)
    assert np.isneginf(pose).all()
    vol.close()


def test_checker_empty_zero_and_nonfinite_are_lost(chk, oracle):
    from scannet_amd import fusion
    t = fusion.default_track_params()
    op, vol = oracle_corner(oracle)
    truth = corner_truth()
    depth = corner_frames()[0][0]
    pose, res = cpu_track(vol, op, np.zeros_like(depth), truth, t)
    assert res.tracked == 0 and res.lost_reason == 3 and np.isneginf(pose).all(), res_tuple(res)   # nothing at the coarsest level
    for bad in (np.nan, np.inf, -np.inf):
        g = truth.copy()
        g[1, 3] = bad
        pose, res = cpu_track(vol, op, depth, g, t, ref=truth)
        assert res.tracked == 0 and res.lost_reason == 1 and np.isneginf(pose).all()
        pose, res = cpu_track(None, op, depth, truth, t, ref=g, model=ss.missed_model(op))   # nothing is cast at a reference that is not finite
        assert res.tracked == 0 and res.lost_reason == 1 and np.isneginf(pose).all()
    vol.close()
    empty = oracle.Volume(op, threads=8)
    pose, res = cpu_track(empty, op, depth, truth, t)
    assert res.tracked == 0 and res.lost_reason == 3 and np.isneginf(pose).all(), res_tuple(res)
    empty.close()


def cpu_loop(oracle, t=None):
    """The track-and-fuse loop on the CPU: frame 0 at its true pose, every later frame tracked from the last pose and fused where it tracked."""
    from scannet_amd import fusion
    t = t or fusion.default_track_params()
    op, _ = params_pair(oracle)
    vol = oracle.Volume(op, threads=8)
    poses, results = [], []
    frames = loop_frames()
    last = frames[0][1]
    for k, (d, truth) in enumerate(frames):
        if k == 0:
            pose, res = truth, None
        else:
            pose, res = cpu_track(vol, op, d, last, t)
            if not res.tracked:
                poses.append(pose)
                results.append(res)
                continue
        vol.integrate(d, pose)
        last = pose
        poses.append(pose)
        results.append(res)
    return op, vol, frames, poses, results


@pytest.fixture(scope="module")
def cpu_loop_run(chk, oracle):
    op, vol, frames, poses, results = cpu_loop(oracle)
    coords, vox = vol.export()
    vol.close()
    return frames, poses, results, coords, vox


def test_checker_track_and_fuse_loop(cpu_loop_run):
    frames, poses, results, _, _ = cpu_loop_run
    errs = [pose_error(p, truth) for p, (_, truth) in zip(poses[1:], frames[1:])]
    assert all(r.tracked for r in results[1:]), [res_tuple(r) for r in results[1:] if not r.tracked]
    et = max(e[0] for e in errs)
    er = max(e[1] for e in errs)
    assert et < LOOP_T_BOUND and er < LOOP_R_BOUND, (et, er)
    # the guess (the previous pose) was off by the walk's step: the tracker did move the pose
    steps = [pose_error(frames[k][1], frames[k - 1][1])[0] for k in range(1, LOOP_FRAMES)]
    assert min(steps) > 0.008


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the parameter surface of the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_track_params_default_and_file(tmp_path):
    from scannet_amd import fusion
    t = fusion.default_track_params()
    assert t.levels == 3 and list(t.max_iters) == [10, 5, 4, 4]
    assert list(t.dist_thres) == [f32(0.15)] * 4 and list(t.normal_thres) == [f32(0.7)] * 4
    assert (t.early_out, t.min_correspondences, t.max_translation, t.max_rotation) == (f32(1e-5), 1000, f32(0.3), f32(0.5))
    assert bytes(t.raycast) == bytes(fusion.default_raycast_params())
    path = tmp_path / "zParametersTrackingDefault.txt"
    path.write_text("s_maxLevels = 2;\ns_maxOuterIter = 7 3;\t// finest first\ns_distThres = 0.1f 0.2f 0.3f;\ns_normalThres = 0.9f;\n"
                    "s_residualEarlyOut = 0.001f;\ns_minCorrespondences = 500;\ns_maxTranslation = 0.5f;\ns_maxRotation = 0.25f;\n"
                    "s_renderDepthMax = 3.0f;\n")
    t = fusion.load_track_params(path)
    assert t.levels == 2 and list(t.max_iters) == [7, 3, 4, 4]
    assert list(t.dist_thres) == [f32(0.1), f32(0.2), f32(0.3), f32(0.15)]
    assert list(t.normal_thres) == [f32(0.9), f32(0.7), f32(0.7), f32(0.7)]
    assert (t.early_out, t.min_correspondences, t.max_translation, t.max_rotation) == (f32(0.001), 500, f32(0.5), f32(0.25))
    assert t.raycast.depth_max == f32(6.0)   # the ray-cast keys are the ray-cast loader's
    plain = tmp_path / "plain.txt"
    plain.write_text("s_SDFVoxelSize = 0.010f;\n")
    assert bytes(fusion.load_track_params(plain)) == bytes(fusion.default_track_params())
    bad = tmp_path / "bad.txt"
    for text in ("s_distThres = far;\n", "s_maxRotation = inf;\n", "s_normalThres = nan;\n", "s_maxOuterIter = 1 2 3 4 5;\n", "s_maxLevels = ;\n"):
        bad.write_text(text)
        with pytest.raises(_abi.ScanfuseError):
            fusion.load_track_params(bad)


BAD_TRACK = [("levels", 0, "levels"), ("levels", 5, "levels"), ("max_iters", [0], "max_iters"), ("max_iters", [10, 101], "max_iters"),
             ("dist_thres", [0.0], "dist_thres"), ("dist_thres", [float("nan")], "dist_thres"), ("dist_thres", [0.1, float("inf")], "dist_thres"),
             ("normal_thres", [1.5], "normal_thres"), ("normal_thres", [float("nan")], "normal_thres"), ("early_out", -1.0, "early_out"),
             ("early_out", float("inf"), "early_out"), ("min_correspondences", 5, "min_correspondences"),
             ("max_translation", 0.0, "motion"), ("max_rotation", float("nan"), "motion"), ("max_translation", float("inf"), "motion")]


@pytest.mark.parametrize("field,value,words", BAD_TRACK)
def test_invalid_track_params_are_refused(field, value, words):
    """Checked before the fuser is looked at: the same refusal with or without a GPU."""
    from scannet_amd import fusion
    L = _abi.lib()
    args = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fusion.SfTrackParams), C.c_void_p, C.POINTER(fusion.SfTrackResult)]
    L.sf_fuser_track.argtypes = args
    L.sf_fuser_track_device.argtypes = args
    t = fusion.default_track_params(**{field: value})
    depth = np.zeros(16, np.uint16)
    pose = np.eye(4, dtype=np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    res = fusion.SfTrackResult()
    for fn in (L.sf_fuser_track, L.sf_fuser_track_device):
        assert fn(None, depth.ctypes.data, pose.ctypes.data, None, C.byref(t), out.ctypes.data, C.byref(res)) == SF_ERR_INVALID_ARG
        assert words in L.sf_last_error().decode()
    good = fusion.default_track_params()
    assert L.sf_fuser_track(None, depth.ctypes.data, pose.ctypes.data, None, C.byref(good), out.ctypes.data, C.byref(res)) == SF_ERR_INVALID_ARG
    assert "NULL fuser" in L.sf_last_error().decode()
    # the tracker's ray cast is the integration camera's: a size or intrinsics of its own are refused
    for k, v in (("width", 160), ("fx", 300.0)):
        t = fusion.default_track_params()
        setattr(t.raycast, k, v)
        assert L.sf_fuser_track(None, depth.ctypes.data, pose.ctypes.data, None, C.byref(t), out.ctypes.data, C.byref(res)) == SF_ERR_INVALID_ARG
        assert "integration camera" in L.sf_last_error().decode()


def test_track_structs_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sf_track_params), offsetof(sf_track_params, normal_thres), offsetof(sf_track_params, max_rotation),
         offsetof(sf_track_params, raycast), offsetof(sf_track_params, reserved), sizeof(sf_track_result), offsetof(sf_track_result, rms_residual),
         offsetof(sf_track_result, lost_reason));
  return 0;
}'''
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = str(tmp_path / "tk_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    from scannet_amd import fusion
    P, R = fusion.SfTrackParams, fusion.SfTrackResult
    assert got == [C.sizeof(P), P.normal_thres.offset, P.max_rotation.offset, P.raycast.offset, P.reserved.offset, C.sizeof(R),
                   R.rms_residual.offset, R.lost_reason.offset]


def test_depthsensing_refuses_track_with_ranks(tmp_path):
    if not os.path.exists(TOOL):
        pytest.skip("bin/depthsensing is built by build()")
    (tmp_path / "p.txt").write_text("s_SDFVoxelSize = 0.010f;\n")
    (tmp_path / "t.txt").write_text("s_maxLevels = 3;\n")
    r = subprocess.run([TOOL, "--ranks", "2", "--share-gpu", str(tmp_path / "p.txt"), str(tmp_path / "t.txt"), str(tmp_path / "none.sens"), "--track"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--track" in r.stderr and "--ranks" in r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernels against the checker, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _room_pair(oracle, n, voxel, W_=W, H_=H, **table):
    """The furnished room's walk fused by the oracle and by a fuser, n frames at 1 cm per frame."""
    from scannet_amd import fusion
    op, gp = params_pair(oracle, W_, H_, voxel, **table)
    vol = oracle.Volume(op, threads=8)
    f = fusion.Fuser(gp, device=0)
    boxes = synth.clutter_boxes()
    for i in range(n):
        pose = synth.trajectory_pose(i, LOOP_TOTAL)
        d = synth.render_room_depth(pose, W_, H_, noise_frame=i, noise=2, boxes=boxes)
        vol.integrate(d, pose)
        assert f.integrate(d, pose)
    f.sync()
    return op, vol, f


def _pairs():
    t0, t5 = synth.trajectory_pose(5, LOOP_TOTAL), synth.trajectory_pose(8, LOOP_TOTAL)
    return [("same", t5, t5), ("guess_off", perturb(t5, 0.02, deg=2.0), t5), ("ref_elsewhere", t5, t0), ("both_off", perturb(t5, 0.01, deg=-1.0, axis=(1, 0, 0)), perturb(t5, 0.005, deg=0.5))]


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [0.004, 0.001])
def test_gpu_system_bit_exact_every_level(chk, oracle, voxel):
    """At 4 mm the fuser's volume is the oracle's; at 1 mm (a table of 4 M blocks) the checker reads the fuser's own exported blocks."""
    from scannet_amd import fusion
    table = {} if voxel == 0.004 else {"num_sdf_blocks": 1 << 22, "hash_num_buckets": 1 << 22}
    op, vol, f = _room_pair(oracle, 10 if voxel == 0.004 else 3, voxel, **table)
    try:
        blocks = f.export_blocks()
        if voxel == 0.004:
            oc, ov = vol.export()
            assert np.array_equal(oc, blocks[0]) and ov.tobytes() == blocks[1].tobytes()
        else:
            assert f.stats()["alloc_failures"] == 0
        boxes = synth.clutter_boxes()
        depth = synth.render_room_depth(synth.trajectory_pose(8, LOOP_TOTAL), W, H, noise_frame=8, noise=2, boxes=boxes)
        t = fusion.default_track_params()
        for name, T, Tref in _pairs():
            for level in range(t.levels):
                want, wmask = cpu_system(blocks, op, depth, level, T, Tref, t)
                got, gmask = f.track_system(depth, level, T, Tref, t, mask=True)
                assert np.array_equal(gmask, wmask), (name, level, int((gmask != wmask).sum()))
                assert got.tobytes() == want.tobytes(), (name, level, got, want)
                assert want[28] > 100, (name, level, want[28])
    finally:
        vol.close()
        f.close()


@pytest.mark.gpu
def test_gpu_buffers_are_remade_for_more_levels(chk, oracle):
    """One fuser's tracking buffers through their three states: made for one level, re-made when three are asked for (level 2 is 80 x 60 = 4 800 pixels =
    18.75 workgroups: the last one is partial), and kept when one level is asked for again."""
    from scannet_amd import fusion
    op, gp = params_pair(oracle)
    frames = corner_frames()
    depth, truth = frames[0]
    T = perturb(truth, 0.01, deg=1.0)
    with fusion.Fuser(gp, device=0) as f:
        for d, p in frames:
            assert f.integrate(d, p)
        f.sync()
        blocks = f.export_blocks()
        want = {}
        for step, (levels, level) in enumerate(((1, 0), (3, 2), (1, 0))):
            t = fusion.default_track_params(levels=levels)
            if (levels, level) not in want:
                want[levels, level] = cpu_system(blocks, op, depth, level, T, truth, t)
            wsys, wmask = want[levels, level]
            got, gmask = f.track_system(depth, level, T, truth, t, mask=True)
            assert np.array_equal(gmask, wmask), (step, int((gmask != wmask).sum()))
            assert got.tobytes() == wsys.tobytes(), (step, got, wsys)
            assert wsys[28] > 100, (step, wsys[28])


@pytest.fixture(scope="module")
def gpu_room10(oracle):
    op, vol, f = _room_pair(oracle, 10, 0.004)
    yield op, vol, f
    vol.close()
    f.close()


@pytest.mark.gpu
def test_gpu_track_bit_exact_and_leaves_the_volume_alone(chk, gpu_room10):
    from scannet_amd import fusion
    op, vol, f = gpu_room10
    boxes = synth.clutter_boxes()
    truth = synth.trajectory_pose(10, LOOP_TOTAL)
    depth = synth.render_room_depth(truth, W, H, noise_frame=10, noise=2, boxes=boxes)
    before, st0 = ss.volume_digest(f), f.stats()
    t = fusion.default_track_params()
    for guess, ref in ((synth.trajectory_pose(9, LOOP_TOTAL), None), (perturb(truth, 0.02, deg=2.0), truth), (perturb(truth, 0.01, deg=-1.0), None)):
        want_pose, want_res = cpu_track(vol, op, depth, guess, t, ref=ref)
        pose, res = f.track(depth, guess, ref=ref, params=t)
        pose2, res2 = f.track(depth, guess, ref=ref, params=t)
        assert res_tuple(res) == res_tuple(want_res), (res_tuple(res), res_tuple(want_res))
        assert want_res.tracked == 1
        assert pose.tobytes() == want_pose.tobytes()
        assert pose2.tobytes() == pose.tobytes() and res_tuple(res2) == res_tuple(res)
        et, er = pose_error(pose, truth)
        assert et < LOOP_T_BOUND and er < LOOP_R_BOUND
    assert ss.volume_digest(f) == before and f.stats() == st0


@pytest.mark.gpu
def test_gpu_track_device_equals_host(gpu_room10):
    import torch
    op, vol, f = gpu_room10
    truth = synth.trajectory_pose(10, LOOP_TOTAL)
    depth = synth.render_room_depth(truth, W, H, noise_frame=10, noise=2, boxes=synth.clutter_boxes())
    guess = synth.trajectory_pose(9, LOOP_TOTAL)
    d = torch.from_numpy(depth.astype(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    p1, r1 = f.track_device(d, guess)
    p0, r0 = f.track(depth, guess)
    assert p1.tobytes() == p0.tobytes() and res_tuple(r1) == res_tuple(r0)


@pytest.mark.gpu
def test_gpu_loop_reproduces_the_cpu_chain(cpu_loop_run, oracle):
    from scannet_amd import fusion
    frames, cpu_poses, cpu_results, coords, vox = cpu_loop_run
    _, gp = params_pair(oracle)
    with fusion.Fuser(gp, device=0) as f:
        poses, results = fusion.track_and_fuse(f, [d for d, _ in frames], frames[0][1])
        f.sync()
        for k in range(1, LOOP_FRAMES):
            assert poses[k].tobytes() == np.asarray(cpu_poses[k], np.float32).tobytes(), k
            r = cpu_results[k]
            assert results[k]["iterations"] == list(r.iterations) and results[k]["correspondences"] == r.correspondences, k
        gc, gv = f.export_blocks()
        assert np.array_equal(gc, coords) and gv.tobytes() == vox.tobytes()


@pytest.mark.gpu
def test_gpu_track_sees_a_queued_integrate(oracle):
    """A track queued right after integrate_device sees that frame: the same answer as on a fuser that was synchronised in between."""
    import torch
    from scannet_amd import fusion
    _, gp = params_pair(oracle)
    boxes = synth.clutter_boxes()
    frames = [(synth.render_room_depth(synth.trajectory_pose(i, LOOP_TOTAL), W, H, noise_frame=i, noise=2, boxes=boxes), synth.trajectory_pose(i, LOOP_TOTAL))
              for i in range(4)]
    with fusion.Fuser(gp, device=0) as a, fusion.Fuser(gp, device=0) as b:
        for k, (d, pose) in enumerate(frames[:3]):
            dd = torch.from_numpy(d.astype(np.int16)).to("cuda:0")
            torch.cuda.synchronize()
            assert a.integrate_device(dd, pose)
            pa, ra = a.track(frames[k + 1][0], pose)     # queued behind the integrate, not waited for
            assert b.integrate(d, pose)
            b.sync()
            pb, rb = b.track(frames[k + 1][0], pose)
            assert ra.tracked == 1 and pa.tobytes() == pb.tobytes() and res_tuple(ra) == res_tuple(rb), k
            a.sync()
            del dd
        assert ss.volume_digest(a) == ss.volume_digest(b)


@pytest.mark.gpu
def test_gpu_lost_cases(oracle):
    from scannet_amd import fusion
    _, gp = params_pair(oracle)
    truth = corner_truth()
    depth = corner_frames()[0][0]
    with fusion.Fuser(gp, device=0) as f:
        pose, res = f.track(depth, truth)                   # empty volume
        assert pose is None and res.lost_reason == 3
        for d, p in corner_frames():
            assert f.integrate(d, p)
        pose, res = f.track(np.zeros_like(depth), truth)    # zero depth
        assert pose is None and res.lost_reason == 3
        g = truth.copy()
        g[0, 0] = np.nan
        pose, res = f.track(depth, g)                       # non-finite guess
        assert pose is None and res.lost_reason == 1
        pose, res = f.track(depth, truth, ref=np.full((4, 4), -np.inf, np.float32))
        assert pose is None and res.lost_reason == 1
        out = np.zeros(16, np.float32)
        L = _abi.lib()
        r = fusion.SfTrackResult()
        t = fusion.default_track_params()
        L.sf_fuser_track.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(fusion.SfTrackParams), C.c_void_p, C.POINTER(fusion.SfTrackResult)]
        assert L.sf_fuser_track(f._h, depth.ctypes.data, g.ctypes.data, None, C.byref(t), out.ctypes.data, C.byref(r)) == 0
        assert np.isneginf(out).all()
        pose, res = f.track(depth, perturb(truth, 0.02, deg=2.0), ref=truth)
        assert res.tracked == 1
        et, er = pose_error(pose, truth)
        assert et < CORNER_T_BOUND and er < CORNER_R_BOUND
    with fusion.Fuser(gp, device=0) as f:
        plane = synth.plane_frame(W, H)
        assert f.integrate(plane, plane_pose())
        pose, res = f.track(plane, perturb(plane_pose(), 0.01, deg=1.0), ref=plane_pose())
        assert pose is None and res.lost_reason == 3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU: bin/depthsensing --track
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_depthsensing_track(tmp_path):
    from scannet_amd import sens
    K = synth.intrinsic_matrix(W, H)
    sd = sens.SensorData.create(0, 0, W, H, K, K, sensor_name="StructureSensor")
    frames = loop_frames()
    for i, (d, pose) in enumerate(frames):
        sd.add_frame(d, pose if i == 0 else np.eye(4, dtype=np.float32), timestamp_depth=i)   # the converter's identity poses after frame 0
    path = str(tmp_path / "scan.sens")
    sd.save(path)
    sd.close()
    params = tmp_path / "zParametersScanNet.txt"
    params.write_text("s_SDFVoxelSize = 0.004f;\ns_hashNumSDFBlocks = 262144;\ns_hashNumBuckets = 500000;\n")
    (tmp_path / "zParametersTrackingDefault.txt").write_text("s_maxLevels = 3;\ns_maxOuterIter = 10 5 4;\n")
    out_sens = tmp_path / "tracked.sens"
    r = subprocess.run([TOOL, str(params), str(tmp_path / "zParametersTrackingDefault.txt"), path, "--track", "--write-sens=%s" % out_sens],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "tracked" in r.stdout and "lost" in r.stdout
    assert os.path.getsize(str(tmp_path / "scan_vh.ply")) > 1000
    got = sens.SensorData(str(out_sens))
    assert len(got.frames) == LOOP_FRAMES
    for i, (_, truth) in enumerate(frames):
        et, er = pose_error(got.frames[i].camera_to_world, truth)
        assert et < LOOP_T_BOUND and er < LOOP_R_BOUND, (i, et, er)
    got.close()
    r2 = subprocess.run([TOOL, "--ranks", "2", "--share-gpu", str(params), str(tmp_path / "zParametersTrackingDefault.txt"), path, "--track"],
                        capture_output=True, text=True, timeout=120)
    assert r2.returncode != 0 and "--track" in r2.stderr and "--ranks" in r2.stderr
