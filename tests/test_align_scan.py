"""The scan alignment on the GPU: k_group_solve alone against the stand-alone program of tests/align_group_solve_main.cpp, one batched
call over a mix of groups against sf_fuser_align* on every group alone, the scan call against the composition of the public calls and against the
hierarchy on the CPU checker, and bin/depthsensing's scan path against Python's -- all byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, synth
from tests import align_scan_cases as cases
from tests import solver_scenes as ss

W, H = cases.W, cases.H
TOOL = os.path.join(cases.ROOT, "bin", "depthsensing")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chk():
    if not ss.checkers_available():
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    return ss.align_lib()


@pytest.fixture(scope="module")
def fuser():
    """A fuser holding 4 fused frames of the furnished room: the calls must leave them alone."""
    from scannet_amd import fusion
    f = fusion.Fuser(ss.fuser_params(W, H, ss.NO_COLOUR, 0.008, num_sdf_blocks=1 << 17), device=0)
    boxes = synth.clutter_boxes()
    for i in range(4):
        pose = synth.trajectory_pose(i, ss.WALK_TOTAL)
        assert f.integrate(synth.render_room_depth(pose, W, H, noise_frame=i, noise=2, boxes=boxes), pose)
    f.sync()
    yield f
    f.close()


def res_all(r):
    return ss.align_res_tuple(r)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. The kernel alone: its records are the stand-alone program's.  This is the test of the device's double-precision sqrt and division
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_gpu_group_solve_kernel_equals_the_program(chk, tmp_path):
    if not cases.have_gxx():
        pytest.skip("needs g++")
    problems, min_corr = cases.stage_problems()
    want = cases.run_program(cases.build_program(tmp_path, False), tmp_path, problems, min_corr)
    gf, pf, masks, local, sys = cases.stage_arrays(problems)
    G, M = len(problems), int(gf[-1])
    xi, status, used, conn, sums = np.full((M, 6), np.nan), np.full(G, -1, np.int32), np.full(G, -1, np.int32), np.zeros(G, np.uint32), np.full((G, 4), np.nan)
    L = _abi.lib()
    L.sf_align_group_solve_stage.argtypes = [C.c_int, C.c_uint64] + [C.c_void_p] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 5
    _abi.check(L.sf_align_group_solve_stage(0, G, ss.ptr(gf), ss.ptr(pf), ss.ptr(local), ss.ptr(masks), ss.ptr(sys), sys.shape[1], min_corr, ss.ptr(xi), ss.ptr(status),
                                            ss.ptr(used), ss.ptr(conn), ss.ptr(sums)))
    got = (xi, status, used, conn, sums)
    print("status %s used %s conn %s" % (status.tolist(), used.tolist(), conn.tolist()))
    bad = np.flatnonzero((xi.view(np.uint64) != want[0].view(np.uint64)).any(axis=1))
    print("member slots whose update differs: %s; largest difference %.3g" % (bad.tolist(), float(np.abs(xi - want[0]).max()) if len(bad) else 0.0))
    assert sorted(set(status.tolist())) == [0, 1, 2]
    for k, (g, w) in enumerate(zip(cases.records_bytes(*got), cases.records_bytes(*want))):
        assert g == w, ("xi status used conn sums".split()[k], got[k], want[k])
    # the 29-value layout: the same problems without the colour sums
    sys29 = np.ascontiguousarray(sys[:, :29])
    xi2 = np.full((M, 6), np.nan)
    _abi.check(L.sf_align_group_solve_stage(0, G, ss.ptr(gf), ss.ptr(pf), ss.ptr(local), ss.ptr(masks), ss.ptr(sys29), 29, min_corr, ss.ptr(xi2), ss.ptr(status),
                                            ss.ptr(used), ss.ptr(conn), ss.ptr(sums)))
    assert xi2.tobytes() == want[0].tobytes() and status.tobytes() == want[1].tobytes() and not sums[:, 2:].any()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. One batched call over a mix of groups against sf_fuser_align on every group alone
# ---------------------------------------------------------------------------------------------------------------------------------------------
def mixed_groups():
    """-> (depth [K, H*W], [(name, frames, poses [n,16])])."""
    d16, t16, s16 = cases.arc(16)
    s16 = s16.reshape(16, 16)
    t16 = t16.astype(np.float32)
    st = ss.structure_cases(cases.arc(6), W, H)
    depth = np.concatenate([d16, st["thin"][0], st["planes"][0], st["lost"][0]])
    far = np.stack([t16[8], ss.perturb(t16[9], 0.008, rad=0.004), ss.perturb(t16[10], 0.06, rad=0.03)]).astype(np.float32)
    groups = [("arc2", [0, 1], s16[0:2]),
              ("arc3", [2, 3, 4], ss.drifted(list(t16[2:5]))),
              ("arc4_at_the_truth", [4, 5, 6, 7], t16[4:8]),          # frame 4 is in two groups; ends after one iteration
              ("arc16", list(range(16)), s16),
              ("one_member", [9], s16[9:10]),
              ("thin", [16, 17, 18], st["thin"][1]),
              ("thin_nothing_connected", [18, 16], st["thin"][1][[2, 0]]),   # the thin frame first: both pairs are dropped, status 2 in the kernel's first run
              ("planes", [19, 20], st["planes"][1]),
              ("lost", [21, 22, 23], st["lost"][1]),
              ("last_member_far", [8, 9, 10], far)]
    return depth, [(n, fr, np.ascontiguousarray(p, np.float32).reshape(-1, 16)) for n, fr, p in groups]


def check_groups_against_single_calls(f, depth, groups, a, rgb=None):
    from scannet_amd import fusion
    members = np.concatenate([fr for _, fr, _ in groups]).astype(np.int32)
    first = np.concatenate([[0], np.cumsum([len(fr) for _, fr, _ in groups])]).astype(np.int32)
    poses = np.concatenate([p for _, _, p in groups])
    out, res = f.align_groups(depth, members, first, poses, a, rgb=rgb)
    seen = {}
    for g, (name, fr, p) in enumerate(groups):
        mine = out[first[g]:first[g + 1]]
        if len(fr) == 1:
            assert res_all(res[g]) == (2, 0, 0, 0, 0, 0) + (np.float32(0).tobytes(),) * 2 + (0,) + (np.float32(0).tobytes(),) * 2 and mine.tobytes() == p.tobytes()
            continue
        pairs, count = fusion.align_pairs(p, a)
        assert count == len(pairs) <= 240
        want, want_res = f.align(depth[fr], p, pairs, a, rgb=None if rgb is None else rgb[fr])
        print("%s: %s" % (name, want_res.as_dict()))
        assert res_all(res[g]) == res_all(want_res), (name, res[g].as_dict(), want_res.as_dict())
        assert mine.tobytes() == want.tobytes(), name
        seen[name] = want_res
    return seen


def test_gpu_groups_equal_single_calls(fuser):
    from scannet_amd import fusion
    depth, groups = mixed_groups()
    before, st0 = ss.volume_digest(fuser), fuser.stats()
    a = fusion.default_align_params(max_translation=0.05)
    seen = check_groups_against_single_calls(fuser, depth, groups, a)
    assert seen["arc2"].status == 0 and seen["arc16"].status == 0 and seen["arc16"].pairs_used > 100
    assert seen["arc4_at_the_truth"].status == 0 and seen["arc4_at_the_truth"].iterations < seen["arc16"].iterations     # groups end in different iterations
    assert seen["thin"].status == 0 and seen["thin"].frames_unconnected == 1
    assert seen["thin_nothing_connected"].status == 2 and seen["thin_nothing_connected"].iterations == 0 and seen["thin_nothing_connected"].frames_unconnected == 1
    assert seen["planes"].status == 1 and seen["lost"].status == 0
    assert seen["last_member_far"].status == 0 and seen["last_member_far"].frames_rejected == 1
    assert ss.volume_digest(fuser) == before and fuser.stats() == st0
    # refused: a fixed frame that is not the first, a member that is no frame, a group of 17
    for bad in (dict(params=fusion.default_align_params(fixed_frame=1)), dict(members=[0, 24]), dict(members=list(range(17)), first=[0, 17])):
        with pytest.raises(_abi.ScanfuseError):
            fuser.align_groups(depth, bad.get("members", [0, 1]), bad.get("first", [0, 2]), np.zeros((len(bad.get("members", [0, 1])), 16), np.float32), bad.get("params"))


@pytest.mark.parametrize("variant", ["working_weight", "weight_0_no_pictures"])
def test_gpu_groups_equal_single_calls_with_pictures(variant):
    from scannet_amd import fusion
    depth, rgb, truth, start = ss.wall_scene(4)
    start = start.reshape(4, 16)
    groups = [("all4", [0, 1, 2, 3], start), ("pair", [1, 2], start[1:3]), ("one", [3], start[3:4]), ("three", [0, 2, 3], start[[0, 2, 3]])]
    photo = variant == "working_weight"
    a = fusion.default_align_params(colour_weight=fusion.ALIGN_COLOUR_WEIGHT if photo else 0.0, level=ss.ALIGN_LEVEL)
    with fusion.Fuser(ss.fuser_params(ss.W, ss.H, ss.WALL_CAMERA), device=0) as f:
        seen = check_groups_against_single_calls(f, depth, groups, a, rgb=rgb if photo else None)
    if photo:
        assert seen["all4"].status == 0 and seen["all4"].colour_correspondences > 0
    else:
        assert seen["all4"].status == 1 and seen["all4"].colour_correspondences == 0    # depth alone is singular on the wall


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. The scan call against the composition of the public calls and against the CPU chain
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.SHAPES))
def test_gpu_scan_equals_the_public_calls_and_the_cpu_chain(chk, fuser, name):
    from scannet_amd import fusion
    depth, truth, start, g, t = cases.shape_input(name)
    a = fusion.default_align_params()
    sp = fusion.default_align_scan_params(group_size=g, top_frames=t)
    before, st0 = ss.volume_digest(fuser), fuser.stats()
    out, res = fuser.align_scan(depth, start, a, sp)
    assert ss.volume_digest(fuser) == before and fuser.stats() == st0
    # the composition of the public calls, with the library's own plan
    plan = fusion.align_scan_plan(start, a, sp)

    def solve(d, p, pairs):
        return fuser.align(d, p, pairs, a)

    pub, groups, top, top_res = cases.chain(depth, start, a, g, t, solve, lambda p: fusion.align_pairs(p, a)[0],
                                            lambda p, new: fusion.align_spread(p, np.zeros(1, np.uint64), np.asarray(new, np.float32).reshape(1, 16)))
    first = plan["group_first"]
    assert [fr for _, fr, _ in groups] == [plan["members"][first[k]:first[k + 1]].tolist() for k in range(len(first) - 1)] and top == plan["top"].tolist()
    assert out.tobytes() == pub.tobytes(), name
    assert res_all(res.top) == res_all(top_res), (res.top.as_dict(), top_res.as_dict())
    solved = [r for _, _, r in groups if r is not None]
    assert res.levels == plan["levels"] and res.groups == len(groups)
    assert list(res.groups_status) == [sum(r.status == 0 for r in solved), sum(r.status == 1 for r in solved), sum(r.status == 2 for r in solved) + len(groups) - len(solved)]
    assert res.max_iterations == max(r.iterations for r in solved + [top_res])
    assert res.frames_unconnected == sum(r.frames_unconnected for r in solved + [top_res]) and res.frames_rejected == sum(r.frames_rejected for r in solved + [top_res])
    assert res.correspondences == sum(r.correspondences for r in solved + [top_res])
    # the CPU chain of tests/test_align_scan_cpu.py
    cpu, cpu_groups, cpu_top, cpu_top_res = cases.shape_chain(name)
    assert out.tobytes() == cpu.tobytes(), name
    assert res_all(res.top) == res_all(cpu_top_res)
    assert res.groups_status[0] == len(solved) and res.top.status == 0
    # a top that takes every frame: the call is one sf_fuser_align
    live = np.flatnonzero(cases.finite(start))
    flat, flat_res = fuser.align_scan(depth, start, a, fusion.default_align_scan_params(group_size=g, top_frames=16))
    pairs, count = fusion.align_pairs(start[live], a)
    want, want_res = fuser.align(depth[live], start[live], pairs, a)
    assert count == len(pairs) and flat_res.levels == 0 and flat_res.groups == 0 and res_all(flat_res.top) == res_all(want_res)
    assert flat[live].tobytes() == want.tobytes() and flat[~cases.finite(start)].tobytes() == start[~cases.finite(start)].tobytes()


@pytest.mark.parametrize("lost", [(5,), (0, 5)], ids=["frame_5_lost", "frames_0_and_5_lost"])
def test_gpu_scan_without_a_level_makes_the_maps_of_every_frame(lost):
    """No grouping level and lost frames that are not the last: the top's frames are addressed by their own indices, up to K - 1, so the maps of all K
    frames must be this call's.  The fuser is fresh and its map buffers hold the same views in reverse order from a grouped call before."""
    from scannet_amd import fusion
    depth, truth, start = cases.arc(12)
    start = start.reshape(12, 16).copy()
    a = fusion.default_align_params()
    with fusion.Fuser(ss.fuser_params(W, H, ss.NO_COLOUR, 0.008, num_sdf_blocks=1 << 17), device=0) as f:
        f.align_scan(np.ascontiguousarray(depth[::-1]), np.ascontiguousarray(start[::-1]), a, fusion.default_align_scan_params(group_size=4, top_frames=3))
        start[list(lost)] = -np.inf
        live = np.flatnonzero(cases.finite(start))
        out, res = f.align_scan(depth, start, a, fusion.default_align_scan_params(group_size=4, top_frames=12))
    with fusion.Fuser(ss.fuser_params(W, H, ss.NO_COLOUR, 0.008, num_sdf_blocks=1 << 17), device=0) as f:
        pairs, count = fusion.align_pairs(start[live], a)
        want, want_res = f.align(depth[live], start[live], pairs, a)
    assert count == len(pairs) and res.levels == 0 and res.groups == 0 and want_res.status == 0 and want_res.frames_unconnected == 0
    assert res_all(res.top) == res_all(want_res), (res.top.as_dict(), want_res.as_dict())
    assert out[live].tobytes() == want.tobytes() and out[list(lost)].tobytes() == start[list(lost)].tobytes()
    assert out[live[0]].tobytes() == start[live[0]].tobytes() and (out[live[1:]] != start[live[1:]]).any(axis=1).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. The tool
# ---------------------------------------------------------------------------------------------------------------------------------------------
LOOP_N, LOOP_STEP = 24, 3     # the loop of tests/test_align.py::test_gpu_depthsensing_track_align: 24 frames 3 cm apart


def test_gpu_depthsensing_scan_path(tmp_path):
    from scannet_amd import fusion, sens
    K = synth.intrinsic_matrix(W, H)
    boxes = synth.clutter_boxes()
    truth = [synth.trajectory_pose(LOOP_STEP * i, ss.WALK_TOTAL) for i in range(LOOP_N)]
    sd = sens.SensorData.create(0, 0, W, H, K, K, sensor_name="StructureSensor")
    for i, t in enumerate(truth):
        sd.add_frame(synth.render_room_depth(t, W, H, noise_frame=i, noise=2, boxes=boxes), truth[0] if i == 0 else np.eye(4, dtype=np.float32), timestamp_depth=i)
    path = str(tmp_path / "scan.sens")
    sd.save(path)
    sd.close()
    params = tmp_path / "zParametersScanNet.txt"
    params.write_text("s_SDFVoxelSize = 0.008f;\ns_hashNumSDFBlocks = 131072;\ns_hashNumBuckets = 500000;\n")
    tracking = tmp_path / "zParametersTrackingDefault.txt"
    tracking.write_text("s_maxLevels = 3;\ns_maxOuterIter = 10 5 4;\n")
    out_sens = tmp_path / "out.sens"
    r = subprocess.run([TOOL, str(params), str(tracking), path, "--track", "--align=2", "--align-group=3", "--align-top=3", "--write-sens=%s" % out_sens],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Aligned")]
    assert len(line) == 1 and "Aligned 12 keyframes (every 2) in 2 levels of groups of 3 under a top of at most 3" in line[0] and ": 6 groups, " in line[0], r.stdout
    assert any(ln.startswith("Top level: status 0") for ln in r.stdout.splitlines()), r.stdout
    # the same in Python
    sd = sens.SensorData(path)
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.load_params(params, base=fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my))
    t = fusion.load_track_params(tracking)
    with fusion.Fuser(gp, device=0) as f:
        poses, _ = fusion.track_and_fuse(f, [sd.frames[i].decompress_depth() for i in range(LOOP_N)], truth[0], params=t)
        integrated = np.ascontiguousarray(np.stack(poses).astype(np.float32).reshape(LOOP_N, 16))
        target, res, _ = fusion.align_and_reintegrate(f, sd, integrated, every=2, group=3, top=3)
    sd.close()
    assert isinstance(res, fusion.SfAlignScanResult) and res.levels == 2 and res.groups == 6 and res.top.status == 0, res.as_dict()
    got = sens.SensorData(str(out_sens))
    assert len(got.frames) == LOOP_N
    for i in range(LOOP_N):
        assert np.asarray(got.frames[i].camera_to_world, np.float32).tobytes() == target[i].tobytes(), i
    got.close()
    # without the new flags and within the solver's limits the tool says what it always said
    r = subprocess.run([TOOL, str(params), str(tracking), path, "--track", "--align=4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Aligned")]
    assert len(line) == 1 and re.fullmatch(r"Aligned 6 keyframes \(every 4\) over \d+ pairs in [0-9.]+ ms: status 0, \d+ iterations, \d+ pairs and \d+ correspondences in the "
                                           r"last system, rms [0-9.]+ -> [0-9.]+ m, \d+ unconnected, \d+ rejected", line[0]), r.stdout
    assert "Top level" not in r.stdout and "levels" not in r.stdout
