"""Axis alignment without a GPU (scannet_amd/csrc/axis_align.cpp): the host path against tests/axis_align_checker.c bit for
bit, stage by stage and end to end; known answers on the noise-free room; the up vector's two sources; bin/alignment on a scan folder; the ABI."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, alignment, meshclean, sens
from scannet_amd.segmentator import Mesh
from tests import alignment_cases as ac

ROOT = ac.ROOT
SF_ERR_DEVICE = -5

pytestmark = pytest.mark.skipif(not ac.have_gcc(), reason="needs gcc for tests/axis_align_checker.c")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return ac.Checker(tmp_path_factory.mktemp("aac"))


def _cleaned(xyz, tris, p):
    m = Mesh.from_arrays(xyz, tris)
    c, st = meshclean.clean(m, p.merge_distance, p.min_piece_faces)
    cx, _, ct = c.arrays()
    m.close()
    c.close()
    return cx, ct, st


@pytest.fixture(scope="module")
def cases(checker):
    """name -> the case with everything the tests share: the host estimate and the checker's, computed once"""
    out = {}
    for name, (xyz, tris), over, poses in (("room", ac.room()[:2], ac.ROOM_PARAMS, ac.room_trajectory()),
                                           ("clutter", ac.clutter(), ac.CLUTTER_PARAMS, ac.room_trajectory()),
                                           ("ceiling", ac.ceiling_room(), ac.ROOM_PARAMS, ac.room_trajectory())):
        p = alignment.default_params(**over)
        sd = ac.make_sens(poses)
        mesh = Mesh.from_arrays(xyz, tris)
        T, st = alignment.estimate(mesh, sd, params=p)
        cx, ct, cst = _cleaned(xyz, tris, p)
        up, src, _ = ac.stage_up(sd)
        cT, cres = checker.estimate(cx, ct, checker.up(poses), p)
        out[name] = dict(xyz=xyz, tris=tris, p=p, poses=poses, T=T, st=st, cx=cx, ct=ct, up=up, cT=cT, cres=cres)
        mesh.close()
        sd.close()
    return out


@pytest.mark.parametrize("name", ["room", "clutter", "ceiling"])
def test_host_estimate_is_the_checkers_bits(cases, name):
    c = cases[name]
    assert c["st"]["vertices"] == len(c["cx"]) and c["st"]["faces"] == len(c["ct"])
    assert np.array_equal(ac.bits(c["T"]), ac.bits(c["cT"])), (c["T"], c["cT"])
    st, res = c["st"], c["cres"]
    assert (st["clusters_founded"], st["clusters_after_small"], st["clusters_kept"]) == (res.founded, res.after_small, res.kept)
    assert st["floor_found"] == (1 if res.floor >= 0 else 0) and st["floor_inliers"] == res.floor_inliers
    assert st["gpu_batches"] == st["gpu_dirty_evaluations"] == st["gpu_fallback_rescans"] == 0


@pytest.mark.parametrize("name", ["room", "clutter"])
def test_host_stages_are_the_checkers_bits(cases, checker, name):
    """normals, the per-vertex cluster index, the table after the sort and removeSmallClusters, the behind counts (the second filter is a mask over
    them), the covariance sums of the first kept cluster -- on the cleaned mesh after the up rotation, where the rule computes them"""
    c = cases[name]
    p = c["p"]
    up = c["up"]
    M = np.eye(4, dtype=np.float32)
    M[2, :3] = up   # any rotation serves the comparison; rows x and y of the rule are checked through the 16 floats above
    xyz_h, bb_h = ac.stage_transform(c["cx"], M)
    xyz_c, bb_c = checker.transform(c["cx"], M)
    assert np.array_equal(ac.bits(xyz_h), ac.bits(xyz_c)) and np.array_equal(ac.bits(bb_h), ac.bits(bb_c))
    n_h, n_c = ac.stage_normals(xyz_h, c["ct"]), checker.normals(xyz_c, c["ct"])
    assert np.array_equal(ac.bits(n_h), ac.bits(n_c))
    assert np.abs(np.linalg.norm(n_c, axis=1) - 1).max() < 1e-5
    pl_h, pl_c = ac.stage_planes(xyz_h, n_h, p), checker.planes(xyz_c, n_c, p)
    assert ac.same_planes(pl_h, pl_c)
    assert len(pl_c["ids"]) >= 3
    if name == "clutter":
        assert pl_c["founded"] >= 1100, pl_c["founded"]      # the table spans more than one chunk of 1024
        kept = pl_c["behind"] <= p.behind_max
        assert kept.any() and not kept.all()                  # the second filter removes some and keeps some
    for i in range(min(3, len(pl_c["ids"]))):
        cid, rep = int(pl_c["ids"][i]), pl_c["table"][i, :4]
        s_h = ac.stage_cov(xyz_h, pl_h["index"], cid, rep, p.floor_inlier_dist)
        s_c = checker.cov(xyz_c, pl_c["index"], cid, rep, p.floor_inlier_dist)
        assert np.array_equal(ac.bits(s_h), ac.bits(s_c)) and s_c[0] > 0


def test_known_answers_on_the_noise_free_room(cases):
    """The room is exact up to the fp32 rounding of its coordinates, so the aligned frame is known: the floor at z = 0, min x = min y = 0, walls on
    the axes, a rigid transform.  Bound: 1e-4 m and 1e-4 rad -- fp32's 6e-8 x 10 m of coordinates x a chain of at most six transforms is about
    4e-6 m, with a wide margin over it.  Largest deviations seen (host path): floor |z| 5.6e-7 m, min x 1.8e-7 m, min y 4.5e-7 m, wall normal off
    its axis 1.2e-7 rad, |R R^T - I| 1.5e-7, |det - 1| 4.8e-8 (the test prints them)."""
    c = cases["room"]
    xyz, tris, floor, walls = ac.room()
    T = c["T"].astype(np.float64)
    q = xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    R = T[:3, :3]
    dev = {"floor": np.abs(q[floor, 2]).max(), "minx": abs(q[:, 0].min()), "miny": abs(q[:, 1].min()), "rigid": np.abs(R @ R.T - np.eye(3)).max(), "det": abs(np.linalg.det(R) - 1)}
    worst = 0.0
    for mask, n in walls:
        n_aligned = R @ ac.ROOM_R @ np.asarray(n, np.float64)            # the wall's normal in the aligned frame
        assert abs(n_aligned[2]) < 1e-4
        worst = max(worst, float(np.arcsin(min(1.0, np.abs(n_aligned[:2]).min()))))   # angle to the nearer horizontal axis
        assert np.ptp(q[mask] @ n_aligned) < 1e-4                        # and its vertices lie in one plane across that normal
    dev["wall"] = worst
    print("largest deviations:", dev)
    assert q[floor, 2].size > 1000 and q[:, 2].min() > -1e-4
    assert all(v < 1e-4 for v in dev.values()), dev
    assert T[3].tolist() == [0, 0, 0, 1]
    assert c["st"]["floor_found"] == 1 and c["st"]["up_source"] == 0
    assert c["st"]["vertices"] < len(xyz)                                # the table left with the small pieces, the borders were merged


def test_no_floor_is_the_identity_for_step_five_and_still_completes(cases):
    c = cases["ceiling"]
    assert c["st"]["floor_found"] == 0 and c["cres"].floor == -1 and c["st"]["floor_inliers"] == 0
    assert c["st"]["clusters_kept"] >= 5                                 # the ceiling and the walls are there; none of them looks up
    T = c["T"].astype(np.float64)
    q = c["xyz"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert abs(q[:, 0].min()) < 1e-4 and abs(q[:, 1].min()) < 1e-4 and abs(q[:, 2].min()) < 1e-4
    up = c["up"].astype(np.float64)
    assert np.abs(T[2, :3] - up).max() < 1e-6                            # z is still the up vector of step 2: nothing turned it


# ---- the up vector ----------------------------------------------------------------------------------------------------------------------------------
def _pose(R, t=(0, 0, 0)):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = R
    m[:3, 3] = t
    return m


def test_up_vector_from_views_with_a_lost_frame(checker):
    """two cameras whose ups (camera -y) are +z and +x: the mean of (0,0,1) and (1,0,0), divided by ALL THREE frames and normalised, is (1,0,1) / sqrt 2"""
    up_z = np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]])                # camera y -> world -z
    up_x = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])                # camera y -> world -x
    lost = np.full((4, 4), -np.inf, np.float32)
    poses = [_pose(up_z), lost, _pose(up_x)]
    sd = ac.make_sens(poses)
    up, src, _ = ac.stage_up(sd)
    assert src == 0
    assert np.abs(up - np.array([1, 0, 1]) / np.sqrt(2)).max() < 1e-6
    assert np.array_equal(ac.bits(up), ac.bits(checker.up(poses)))
    sd.apply_transform(np.eye(4, dtype=np.float32) * 2)                  # ... and a lost pose stays lost under a transform
    m = np.zeros(16, np.float32)
    v = C.c_int(1)
    _abi.check(_abi.lib().sf_sens_pose(sd._h, 1, m.ctypes.data_as(C.c_void_p), C.byref(v)))
    assert np.all(np.isneginf(m))
    sd.close()


@pytest.mark.parametrize("with_gravity,expect", [(11, 1), (10, 0)])
def test_gravity_takes_over_above_ten_records(checker, with_gravity, expect):
    """11 IMU records that carry gravity switch the source, 10 do not; records with time stamp 0 are dropped before anything else -- here five of them
    carry a gravity that would count, and one that would be the closest record of frame 0"""
    poses = [_pose(np.eye(3)), _pose(ac.rotation((0, 0, 1), 0.5))]
    stamps = [1000, 2000]
    g = np.array([0.6, 0.8, 0.0])                                        # camera frame; swapped to (0.8, 0.6, 0) by the rule
    imu = [ac.imu_record((0, 0, 9.0), 0) for _ in range(5)]
    imu += [ac.imu_record(g * 9.81, 900 + 100 * i) for i in range(with_gravity)]
    imu += [ac.imu_record((0, 0, 0), 5000 + i) for i in range(3)]        # valid stamps, no gravity: not counted
    sd = ac.make_sens(poses, stamps, imu)
    up, src, none = ac.stage_up(sd)
    assert src == expect and none == 0
    if expect:
        per_frame = [sd.find_closest_imu_frame(i)[1]["gravity"] for i in range(2)]
        assert np.array_equal(ac.bits(up), ac.bits(checker.up(poses, per_frame)))
        want = poses[0][:3, :3] @ [0.8, 0.6, 0] + poses[1][:3, :3] @ [0.8, 0.6, 0]
        assert np.abs(up - want / np.linalg.norm(want)).max() < 1e-6
    else:
        assert np.array_equal(ac.bits(up), ac.bits(checker.up(poses)))
    sd.close()


# ---- bin/alignment ----------------------------------------------------------------------------------------------------------------------------------
def _run(*args):
    return subprocess.run([ac.TOOL] + [str(a) for a in args], capture_output=True, text=True)


def _poses_of(path):
    sd = sens.SensorData(path)
    out = np.zeros((sd.num_frames, 16), np.float32)
    v = C.c_int(0)
    for i in range(sd.num_frames):
        _abi.check(_abi.lib().sf_sens_pose(sd._h, i, out[i].ctypes.data_as(C.c_void_p), C.byref(v)))
    sd.close()
    return out


@pytest.fixture(scope="module")
def aligned_folder(tmp_path_factory):
    """a scan folder, what it held before, and the tool's first run on it (the reference's constants: the room's faces are large enough for them)"""
    xyz, tris, _, _ = ac.room()
    poses = [np.eye(4, dtype=np.float32)] + ac.room_trajectory()[1:] + [np.full((4, 4), -np.inf, np.float32)]
    d = ac.write_scan_folder(tmp_path_factory.mktemp("scans"), "scene0000_00", xyz, tris, poses)
    before = ac.folder_bytes(d)
    keep = str(tmp_path_factory.mktemp("orig") / "scene0000_00")
    shutil.copytree(d, keep)
    r = _run(d, "--print-transform")
    return d, keep, before, r


def test_tool_aligns_every_ply_and_every_pose(aligned_folder):
    d, keep, before, r = aligned_folder
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "aligning: " + d and len(lines) == 5
    T = np.array([[float(x) for x in ln.split()] for ln in lines[1:]], np.float32)
    assert open(os.path.join(d, "processed.txt")).read() == "valid = true\nheapFreeCount = 12345\nnumValidOptTransforms = 7\nnumTransforms = 9\naligned = true\n"
    for name in ("scene0000_00.ply", "scene0000_00_vh_clean.ply"):      # the same transform on copies, through the library's own calls
        m = Mesh.read(os.path.join(keep, name))
        alignment.apply_transform(m, T)
        want = m.arrays()
        m.close()
        m = Mesh.read(os.path.join(d, name))
        got = m.arrays()
        m.close()
        for a, b in zip(want, got):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    sd = sens.SensorData(os.path.join(keep, "scene0000_00.sens"))
    sd.apply_transform(T)
    out = os.path.join(keep, "expect.sens")
    sd.save(out)
    sd.close()
    assert open(out, "rb").read() == open(os.path.join(d, "scene0000_00.sens"), "rb").read()
    assert np.all(np.isneginf(_poses_of(os.path.join(d, "scene0000_00.sens"))[-1]))
    assert sorted(os.listdir(d)) == sorted(before)                       # nothing left behind


def test_tool_second_run_skips_and_force_lands_on_the_same_poses(aligned_folder):
    d, keep, before, _ = aligned_folder
    first = ac.folder_bytes(d)
    r = _run(d)
    assert r.returncode == 0 and r.stderr == ""
    assert r.stdout == "aligning: %s\nreconstruction is already aligned %s\n\t -> skipping folder\n" % (d, d)
    assert ac.folder_bytes(d) == first
    poses1 = _poses_of(os.path.join(d, "scene0000_00.sens"))
    r = _run(d, "--force")
    assert r.returncode == 0 and r.stderr == ""
    assert r.stdout == "aligning: %s\nalready found a previous alignment -> reverting to original\n" % d
    poses2 = _poses_of(os.path.join(d, "scene0000_00.sens"))
    fin = np.isfinite(poses1)
    assert np.array_equal(fin, np.isfinite(poses2)) and np.abs(poses1[fin] - poses2[fin]).max() < 1e-5


def test_tool_gates(tmp_path):
    xyz, tris = ac.room()[0][:3], np.array([[0, 1, 2]], np.uint32)
    poses = [np.eye(4, dtype=np.float32)]
    d = ac.write_scan_folder(tmp_path, "invalid", xyz, tris, poses, valid=False)
    before = ac.folder_bytes(d)
    r = _run(d)
    assert (r.returncode, r.stderr, r.stdout) == (0, "", "aligning: %s\nreconstruction was invalid for %s\n\t -> skipping folder\n" % (d, d))
    assert ac.folder_bytes(d) == before
    d = ac.write_scan_folder(tmp_path, "unprocessed", xyz, tris, poses, processed=False)
    r = _run(d)
    assert (r.returncode, r.stderr, r.stdout) == (0, "", "aligning: %s\nno reconstruction available for %s\n\t -> skipping folder\n" % (d, d))
    lost = [np.full((4, 4), -np.inf, np.float32)]
    d = ac.write_scan_folder(tmp_path, "lost", xyz, tris, lost)
    before = ac.folder_bytes(d)
    r = _run(d)
    assert r.returncode == 0 and r.stderr == "" and "error can't revert due to an invalid transform in the first frame\n\tskipping folder \n" in r.stdout
    assert ac.folder_bytes(d) == before


def test_tool_reports_a_missing_floor(tmp_path):
    xyz, tris = ac.ceiling_room()
    d = ac.write_scan_folder(tmp_path, "ceiling", xyz, tris, [np.eye(4, dtype=np.float32)] + ac.room_trajectory()[1:])
    r = _run(d)
    assert (r.returncode, r.stderr, r.stdout) == (0, "", "aligning: %s\ncould not find a horizontal plane\n" % d)
    assert open(os.path.join(d, "processed.txt")).read().endswith("aligned = true\n")


def test_align_scan_mirror(tmp_path):
    xyz, tris, _, _ = ac.room()
    d = ac.write_scan_folder(tmp_path, "s", xyz, tris, [np.eye(4, dtype=np.float32)] + ac.room_trajectory()[1:], aligned=False)
    st = alignment.align_scan(d)
    assert st["outcome"] == "aligned" and st["floor_found"] == 1 and st["reverted"] == 0
    assert alignment.align_scan(d)["outcome"] == "aligned already"
    st2 = alignment.align_scan(d, force=True)
    assert st2["outcome"] == "aligned" and st2["reverted"] == 1


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sf_axis_align_params), offsetof(sf_axis_align_params, min_cluster_points), offsetof(sf_axis_align_params, floor_inlier_dist),
         sizeof(sf_axis_align_stats), offsetof(sf_axis_align_stats, up_source), offsetof(sf_axis_align_stats, gpu_batches), offsetof(sf_axis_align_stats, outcome),
         offsetof(sf_axis_align_stats, transform), offsetof(sf_axis_align_stats, seconds));
  return 0;
}'''
    exe = str(tmp_path / "aa_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, S = alignment.SfAxisAlignParams, alignment.SfAxisAlignStats
    assert got == [C.sizeof(P), P.min_cluster_points.offset, P.floor_inlier_dist.offset, C.sizeof(S), S.up_source.offset, S.gpu_batches.offset, S.outcome.offset,
                   S.transform.offset, S.seconds.offset]
    p = alignment.default_params()
    assert (p.min_piece_faces, p.gravity_min_records, p.min_cluster_points, p.behind_max) == (5000, 10, 500, 100)
    assert [round(v, 6) for v in (p.merge_distance, p.cluster_normal_thresh, p.cluster_dist_thresh, p.behind_dist, p.floor_normal_z, p.floor_inlier_dist)] == [0.0005, 0.9, 0.05, 0.1, 0.8, 0.05]


def test_device_path_needs_a_device_and_bad_arguments_are_refused(tmp_path):
    import torch
    xyz, tris = ac.clutter(40)
    mesh, sd = Mesh.from_arrays(xyz, tris), ac.make_sens([np.eye(4, dtype=np.float32)])
    if not torch.cuda.is_available():
        with pytest.raises(_abi.ScanfuseError) as e:
            alignment.estimate(mesh, sd, device=0)
        assert e.value.code == SF_ERR_DEVICE
        with pytest.raises(_abi.ScanfuseError) as e:
            ac.stage_transform(xyz, np.eye(4), device=0)
        assert e.value.code == SF_ERR_DEVICE
    with pytest.raises(_abi.ScanfuseError) as e:
        alignment.estimate(mesh, sd, params=alignment.default_params(behind_dist=float("nan")))
    assert e.value.code == -1
    with pytest.raises(_abi.ScanfuseError) as e:
        alignment.estimate(mesh, ac.make_sens([]))
    assert e.value.code == -1
    for bad in (63, 2048, 100):
        with pytest.raises(_abi.ScanfuseError):
            ac.tune_batch(bad)
    mesh.close()
    sd.close()
