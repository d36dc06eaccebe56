"""The scan alignment without a GPU: the plan against a Python restatement of its rule, the group solve of scannet_amd/csrc/align_solve.h
-- run by a stand-alone program the way the kernel maps it onto lanes, plain and under the address and undefined-behaviour sanitizers -- against a
Python restatement of the solve, bit for bit, and the hierarchy itself on the CPU checker: how close to the truth it ends."""
import ctypes as C

import numpy as np
import pytest

from scannet_amd import _abi
from tests import align_scan_cases as cases
from tests import solver_scenes as ss

SF_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def chk():
    if not ss.checkers_available():
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    return ss.align_lib()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. The plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pose_sets():
    holes = ss.random_poses(23, 5).reshape(23, 16).copy()
    holes[[0, 7, 8, 22]] = -np.inf
    near = ss.random_poses(100, 9, spread=0.4, turn=0.25)   # nearly all within 1 m and 0.6 rad of one another: far more than 4 096 pairs
    return {"random_40": ss.random_poses(40, 1), "random_7": ss.random_poses(7, 2), "arc_13": cases.arc(13)[2], "holes_23": holes, "near_100": near}


def library_plan(poses, a, g, t, **cap):
    from scannet_amd import fusion
    return fusion.align_scan_plan(poses, a, fusion.default_align_scan_params(group_size=g, top_frames=t), **cap)


@pytest.mark.parametrize("name", ["random_40", "random_7", "arc_13", "holes_23", "near_100"])
def test_plan_equals_the_rule(name):
    from scannet_amd import fusion
    poses = np.asarray(pose_sets()[name], np.float32).reshape(-1, 16)
    a = fusion.default_align_params()
    live = [int(k) for k in np.flatnonzero(cases.finite(poses))]
    for g in (2, 3, 4, 16):
        for t in (2, 3, 4, 256):
            groups, top, levels = cases.python_plan(poses, a, g, t, lambda p: fusion.align_pairs(p, a, capacity=0)[1])
            got = library_plan(poses, a, g, t)
            first = got["group_first"]
            mine = [(int(got["group_level"][k]), [int(x) for x in got["members"][first[k]:first[k + 1]]]) for k in range(len(first) - 1)]
            assert mine == groups and got["top"].tolist() == top and got["levels"] == levels, (name, g, t)
            assert got["counts"] == (sum(len(fr) for _, fr in groups), len(groups), len(top))
            # every live frame is in exactly one level-0 group (when there is a level), every first member of level l in one group of level l + 1 or the top
            if levels:
                assert sorted(x for lv, fr in groups if lv == 0 for x in fr) == live
            for lv in range(levels):
                firsts = sorted(fr[0] for l2, fr in groups if l2 == lv)
                above = sorted(x for l2, fr in groups if l2 == lv + 1 for x in fr) if lv + 1 < levels else sorted(top)
                assert firsts == above, (name, g, t, lv)
            assert all(1 <= len(fr) <= g for _, fr in groups) and 0 < len(top) <= max(t, 0) or not live


def test_plan_takes_one_more_level_when_the_top_would_have_too_many_pairs():
    from scannet_amd import fusion
    poses = pose_sets()["near_100"]
    a = fusion.default_align_params()
    assert fusion.align_pairs(poses, a, capacity=0)[1] > 4096
    got = library_plan(poses, a, 16, 256)
    assert got["levels"] == 1 and got["counts"] == (100, 7, 7) and got["top"].tolist() == [0, 16, 32, 48, 64, 80, 96]
    assert library_plan(poses[:60], a, 16, 256)["levels"] == 0   # 3 540 pairs: the top takes them


def test_plan_capacities_and_argument_errors():
    from scannet_amd import fusion
    poses = ss.random_poses(40, 1)
    a = fusion.default_align_params()
    full = library_plan(poses, a, 4, 3)
    part = library_plan(poses, a, 4, 3, members_capacity=5, groups_capacity=2, top_capacity=1)
    assert part["counts"] == full["counts"] == (50, 13, 3) and part["levels"] == full["levels"] == 2
    assert part["members"].tolist() == full["members"][:5].tolist() and part["top"].tolist() == full["top"][:1].tolist()
    assert part["group_first"].tolist() == full["group_first"][:3].tolist() and part["group_level"].tolist() == full["group_level"][:2].tolist()
    none = library_plan(poses, a, 4, 3, members_capacity=0, groups_capacity=0, top_capacity=0)
    assert none["counts"] == (50, 13, 3)
    for g, t in ((1, 3), (17, 3), (4, 1), (4, 257)):
        with pytest.raises(_abi.ScanfuseError):
            library_plan(poses, a, g, t)
    L = _abi.lib()
    sp = fusion.default_align_scan_params()
    assert (sp.group_size, sp.top_frames) == (16, 256)
    n = C.c_uint64(0)
    lv = C.c_int32(0)
    L.sf_align_scan_plan.restype = C.c_int
    assert L.sf_align_scan_plan(None, 0, None, C.byref(sp), None, 0, None, None, 0, None, 0, C.byref(n), C.byref(n), C.byref(n), C.byref(lv)) == SF_ERR_INVALID_ARG
    assert L.sf_align_scan_plan(poses.ctypes.data_as(C.c_void_p), 40, C.byref(a), C.byref(sp), None, 3, None, None, 0, None, 0, C.byref(n), C.byref(n), C.byref(n),
                                C.byref(lv)) == SF_ERR_INVALID_ARG


def test_scan_structs_match_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    from scannet_amd import fusion
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(sf_align_scan_params), offsetof(sf_align_scan_params, top_frames), sizeof(sf_align_scan_result),
         offsetof(sf_align_scan_result, groups_status), offsetof(sf_align_scan_result, frames_rejected), offsetof(sf_align_scan_result, correspondences),
         offsetof(sf_align_scan_result, top), offsetof(sf_align_scan_result, reserved));
  return 0;
}'''
    exe = str(tmp_path / "scan_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(cases.ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, R = fusion.SfAlignScanParams, fusion.SfAlignScanResult
    assert got == [C.sizeof(P), P.top_frames.offset, C.sizeof(R), R.groups_status.offset, R.frames_rejected.offset, R.correspondences.offset, R.top.offset,
                   R.reserved.offset]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. The solve arithmetic: the stand-alone program, plain and sanitized, against Python floats
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_group_solve_program_equals_python_floats(chk, tmp_path, sanitize):
    if not cases.have_gxx():
        pytest.skip("needs g++")
    problems, min_corr = cases.stage_problems()
    want = cases.python_records_arrays(problems, min_corr)
    exe = cases.build_program(tmp_path, sanitize)
    got = cases.run_program(exe, tmp_path, problems, min_corr)
    names = [p[0] for p in problems]
    status = dict(zip(names, want[1]))
    assert status["arc2"] == status["arc4"] == status["arc16"] == 0 and status["thin"] == 2 and status["planes"] == 1, status
    assert status["thin_one_left"] == 0 and status["spd_1e-6_1e6"] == 0 and status["spd_member_2_invalid"] == 0 and status["spd_16"] == 0, status
    assert dict(zip(names, want[3]))["thin_one_left"] == 0b011 and dict(zip(names, want[3]))["spd_member_2_invalid"] == 0b11011
    assert np.abs(want[0]).max() > 1e-4      # the comparison is not of zeros
    for k, (g, w) in enumerate(zip(cases.records_bytes(*got), cases.records_bytes(*want))):
        assert g == w, ("xi status used conn sums".split()[k], got[k], want[k])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. The CPU chain: groups under a top on the checker, against the truth
# ---------------------------------------------------------------------------------------------------------------------------------------------
T_BOUND, R_BOUND = 2e-3, 1e-3    # metres, radians: the flat solve of the same views ends 1.36 mm / 0.52 mrad off


@pytest.mark.parametrize("name", sorted(cases.SHAPES))
def test_checker_chain_ends_at_the_truth(chk, name):
    depth, truth, start, g, t = cases.shape_input(name)
    out, groups, top, top_res = cases.shape_chain(name)
    live = np.flatnonzero(cases.finite(start))
    assert top_res is not None and top_res.status == 0, top_res.as_dict()
    for lv, frames, res in groups:
        assert (res is None and len(frames) == 1) or res.status == 0, (lv, frames, res.as_dict())
    levels = 1 + max(lv for lv, _, _ in groups)
    assert levels == (2 if name == "12_by_2_by_2_under_3" else 1) and len(top) <= t
    if name == "13_by_4_under_4":
        assert [fr for _, fr, _ in groups][-1] == [12]
    errs = [ss.pose_error(out[k].reshape(4, 4), truth[k]) for k in live]
    et, er = max(e[0] for e in errs), max(e[1] for e in errs)
    e0 = max(ss.pose_error(start[k].reshape(4, 4), truth[k])[0] for k in live)
    print("%s: start %.1f mm, worst %.3f mm / %.3f mrad" % (name, e0 * 1e3, et * 1e3, er * 1e3))
    assert e0 > 0.08
    assert et < T_BOUND and er < R_BOUND, (name, et, er)
    dead = np.flatnonzero(~cases.finite(start))
    assert out[dead].tobytes() == start[dead].tobytes()
    assert out[live[0]].tobytes() == start[live[0]].tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The kernel's resources
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_group_solve_kernel_lives_in_lds_and_registers():
    import os
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kr = ss.kernel_resources()
    rows = kr.kernels(os.path.join(cases.ROOT, "scannet_amd", "libscanfuse.so"))
    mine = [r for r, n in zip(rows, kr.demangle([r["name"] for r in rows])) if kr.short(n) == "k_group_solve"]
    assert len(mine) == 1
    assert mine[0]["scratch"] == 0 and mine[0]["vspill"] == 0 and 32760 < mine[0]["lds"] <= 64 * 1024, mine[0]
