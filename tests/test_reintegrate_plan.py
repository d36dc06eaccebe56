"""The host-only half of re-integration (no GPU): the trajectory manager's planner sf_reint_plan against a float64 numpy restatement of its rule,
the three parameter-file keys (Server/tools/recons/zParametersScanNet.txt:25-28; tests/golden/zParametersScanNet.txt is that file), the layout of the
two new structs against their ctypes mirrors, and what the compiler gave k_reintegrate (DESIGN.md section 4d states the register figure)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, fusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOST = np.full(16, -np.inf, np.float32)


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _trajectory(rng, n=200):
    """n camera-to-world poses (float32 [n,16]): random rotations, positions in a 6 m cube."""
    out = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        out[i, :3, :3] = _rot(rng.normal(size=3), rng.uniform(0, np.pi))
        out[i, :3, 3] = rng.uniform(-3, 3, 3)
        out[i, 3, 3] = 1
    return out.reshape(n, 16)


def _perturb(pose16, rng, angle, shift):
    p = pose16.reshape(4, 4).astype(np.float64)
    q = p.copy()
    q[:3, :3] = _rot(rng.normal(size=3), angle) @ p[:3, :3]
    d = rng.normal(size=3)
    q[:3, 3] = p[:3, 3] + shift * d / np.linalg.norm(d)
    return q.astype(np.float32).reshape(16)


def _dist2(a, b):
    """d2 = |t_b - t_a|^2 + theta^2 in float64 from the float32 poses; theta = atan2(sin, cos) of M = R_a^T R_b, sin from M's antisymmetric part, cos
    from its trace (include/scanfuse.h)."""
    A, B = a.reshape(4, 4).astype(np.float64), b.reshape(4, 4).astype(np.float64)
    d2 = 0.0
    for r in range(3):
        dt = B[r, 3] - A[r, 3]
        d2 += dt * dt
    M = [[(A[0, i] * B[0, j] + A[1, i] * B[1, j]) + A[2, i] * B[2, j] for j in range(3)] for i in range(3)]
    x, y, z = M[2][1] - M[1][2], M[0][2] - M[2][0], M[1][0] - M[0][1]
    sn = 0.5 * np.sqrt((x * x + y * y) + z * z)
    cs = 0.5 * (((M[0][0] + M[1][1]) + M[2][2]) - 1.0)
    th = np.arctan2(sn, cs)
    return float(d2 + th * th)


def _plan_numpy(integrated, target, max_fixes, top_n, thresh):
    """The rule of include/scanfuse.h, restated: +inf when exactly one pose is lost; both lost: no candidate; candidates d2 > thresh; order d2
    descending, then index ascending; first top_n, of those first max_fixes."""
    cand = []
    for i, (a, b) in enumerate(zip(integrated, target)):
        la, lb = bool(np.all(a == -np.inf)), bool(np.all(b == -np.inf))
        if la and lb:
            continue
        d2 = np.inf if (la or lb) else _dist2(a, b)
        if d2 > thresh:
            cand.append((-d2, i))
    cand.sort()
    return [i for _, i in cand][:top_n][:max_fixes]


def _drifted(seed, n=200, moved=120):
    rng = np.random.default_rng(seed)
    target = _trajectory(rng, n)
    integrated = target.copy()
    for i in rng.choice(n, moved, replace=False):
        integrated[i] = _perturb(target[i], rng, rng.uniform(0.001, 0.1), rng.uniform(0.001, 0.2))
    return integrated, target


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("max_fixes,top_n", [(30, 30), (30, 12), (7, 30), (500, 500), (0, 30), (30, 0)])
def test_plan_matches_the_numpy_restatement(seed, max_fixes, top_n):
    integrated, target = _drifted(seed)
    r = fusion.default_reint_params(max_frame_fixes=max_fixes, top_n_active=top_n)
    got = fusion.plan_reintegration(integrated, target, r)
    want = _plan_numpy(integrated, target, max_fixes, top_n, 0.0)
    assert list(got) == want
    assert len(want) == min(max_fixes, top_n, 120)


def test_plan_defaults_are_the_files():
    r = fusion.default_reint_params()
    assert (r.max_frame_fixes, r.top_n_active, r.min_pose_dist_sqrt) == (30, 30, 0.0)
    integrated, target = _drifted(5)
    assert list(fusion.plan_reintegration(integrated, target)) == _plan_numpy(integrated, target, 30, 30, 0.0)


def test_plan_threshold_excludes_small_changes():
    integrated, target = _drifted(11)
    full = _plan_numpy(integrated, target, 10 ** 6, 10 ** 6, 0.0)
    assert len(full) == 120
    # a threshold between the 40th and the 41st largest distance: exactly 40 candidates remain
    def dist2(i):
        return _dist2(integrated[i], target[i])
    thresh = np.float32(0.5 * (dist2(full[39]) + dist2(full[40])))
    r = fusion.default_reint_params(max_frame_fixes=200, top_n_active=200, min_pose_dist_sqrt=float(thresh))
    got = list(fusion.plan_reintegration(integrated, target, r))
    assert got == _plan_numpy(integrated, target, 200, 200, float(thresh)) == full[:40]


def test_plan_breaks_exact_ties_by_frame_index():
    rng = np.random.default_rng(21)
    target = _trajectory(rng, 200)
    integrated = target.copy()
    # the same pure translation given to six frames with IDENTICAL poses: the distances are equal bit for bit
    for i in (150, 17, 90, 3, 199, 42):
        target[i] = target[0]
        integrated[i] = target[0]
        integrated[i][3] += np.float32(0.25)
    integrated[60] = _perturb(target[60], rng, 0.3, 0.5)    # one larger, one smaller
    integrated[61] = _perturb(target[61], rng, 0.001, 0.01)
    got = list(fusion.plan_reintegration(integrated, target, fusion.default_reint_params()))
    assert got == [60, 3, 17, 42, 90, 150, 199, 61] == _plan_numpy(integrated, target, 30, 30, 0.0)
    got = list(fusion.plan_reintegration(integrated, target, fusion.default_reint_params(top_n_active=4)))
    assert got == [60, 3, 17, 42]


def test_plan_lost_frames_come_first_and_both_lost_never():
    integrated, target = _drifted(31)
    integrated[10] = LOST          # lost -> tracked: must be put in
    target[150] = LOST             # tracked -> lost: must be taken out
    integrated[77] = LOST          # lost in both: never a candidate
    target[77] = LOST
    integrated[5] = LOST
    r = fusion.default_reint_params(max_frame_fixes=200, top_n_active=200, min_pose_dist_sqrt=1e9)   # no finite distance passes this
    assert list(fusion.plan_reintegration(integrated, target, r)) == [5, 10, 150]
    got = list(fusion.plan_reintegration(integrated, target, fusion.default_reint_params()))
    assert got[:3] == [5, 10, 150] and 77 not in got and len(got) == 30
    assert got == _plan_numpy(integrated, target, 30, 30, 0.0)
    everything = list(fusion.plan_reintegration(integrated, target, fusion.default_reint_params(max_frame_fixes=200, top_n_active=200)))
    assert 77 not in everything and everything == _plan_numpy(integrated, target, 200, 200, 0.0)


def test_plan_capacity_and_identical_trajectories():
    integrated, target = _drifted(41)
    with pytest.raises(_abi.ScanfuseError) as e:
        fusion.plan_reintegration(integrated, target, fusion.default_reint_params(), capacity=29)
    assert e.value.code == -7   # SF_ERR_BOUNDS
    assert len(fusion.plan_reintegration(integrated, target, fusion.default_reint_params(), capacity=30)) == 30
    assert len(fusion.plan_reintegration(target, target)) == 0
    assert len(fusion.plan_reintegration(target, target.copy(), fusion.default_reint_params(max_frame_fixes=200, top_n_active=200))) == 0
    assert len(fusion.plan_reintegration(np.zeros((0, 16), np.float32), np.zeros((0, 16), np.float32))) == 0
    with pytest.raises(_abi.ScanfuseError):
        fusion.plan_reintegration(integrated, target, fusion.default_reint_params(max_frame_fixes=-1))


def test_parameter_file_keys(tmp_path):
    r = fusion.load_reint_params(os.path.join(ROOT, "tests", "golden", "zParametersScanNet.txt"),
                                 base=fusion.default_reint_params(max_frame_fixes=1, top_n_active=2, min_pose_dist_sqrt=3.0))
    assert (r.max_frame_fixes, r.top_n_active, r.min_pose_dist_sqrt) == (30, 30, 0.0)
    p = tmp_path / "some.txt"
    p.write_text("s_topNActive = 12;\t//only this one\ns_SDFVoxelSize = 0.010f;\n")
    r = fusion.load_reint_params(p, base=fusion.default_reint_params(max_frame_fixes=5, min_pose_dist_sqrt=0.25))
    assert (r.max_frame_fixes, r.top_n_active, r.min_pose_dist_sqrt) == (5, 12, 0.25)
    p.write_text("s_maxFrameFixes = 8;\ns_minPoseDistSqrt = 0.0625f;\n")
    r = fusion.load_reint_params(p)
    assert (r.max_frame_fixes, r.top_n_active, r.min_pose_dist_sqrt) == (8, 30, 0.0625)
    p.write_text("s_maxFrameFixes = many;\n")
    with pytest.raises(_abi.ScanfuseError):
        fusion.load_reint_params(p)


def test_struct_layouts_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(sf_reint_params), offsetof(sf_reint_params, min_pose_dist_sqrt), offsetof(sf_reint_params, reserved),
         sizeof(sf_reint_stats), offsetof(sf_reint_stats, passes), offsetof(sf_reint_stats, seconds_total));
  return 0;
}'''
    exe = str(tmp_path / "sf_reint_layout_check")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, S = fusion.SfReintParams, fusion.SfReintStats
    assert got == [C.sizeof(P), P.min_pose_dist_sqrt.offset, P.reserved.offset, C.sizeof(S), S.passes.offset, S.seconds_total.offset]
    assert C.sizeof(P) == 32


def test_reintegrate_kernels_live_in_registers():
    """Every k_reintegrate variant: no private memory, no spills, LDS within a CU's, and no more vector registers than DESIGN.md 4d states -- the
    figure that gives five waves per SIMD, k_integrate's occupancy."""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernels(os.path.join(ROOT, "scannet_amd", "libscanfuse.so"))
    for r, n in zip(rows, kr.demangle([r["name"] for r in rows])):
        r["short"] = kr.short(n)
    mine = [r for r in rows if r["short"].startswith("k_reintegrate<")]
    assert len(mine) == 11, [r["short"] for r in mine]
    assert {"k_reintegrate<0, true, 2, true>", "k_reintegrate<2, true, 2, true>"} <= {r["short"] for r in mine}   # the shipped parameters: x-row layout
    for r in mine:
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (r["short"], r["scratch"], r["vspill"], r["sspill"])
        assert r["lds"] <= 160 * 1024, (r["short"], r["lds"])
    m = re.search(r"k_reintegrate[^\n]*?at most (\d+) vector registers", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert m, "DESIGN.md 4d states the register figure"
    stated = int(m.group(1))
    assert stated <= 96                                                   # 512 // 96 = 5 waves per SIMD
    assert max(r["vgpr"] + r["agpr"] for r in mine) == stated
    # the k_integrate instantiations did not move when their update bodies went into a shared header
    integ = [r for r in rows if r["short"].startswith("k_integrate<")]
    assert len(integ) >= 20 and max(r["vgpr"] + r["agpr"] for r in integ) <= 96
