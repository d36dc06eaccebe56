"""Ray casting of the fused volume (DESIGN.md "Ray casting"; scannet_amd/csrc/raycast.hip).

The semantics are unpinned -- the upstream ray caster is not in the reference tree -- so they are pinned here the way oracle/tsdf_oracle.c is:
  * without a GPU: tests/raycast_checker.c, a C restatement of the rule over the blocks sf_fuser_export_blocks writes (its own sorted-key look-up,
    not the product's hash table), against analytic answers on a plane fused by the CPU oracle; the ray-cast parameter surface of the C ABI;
  * -m gpu: k_raycast against the checker bit for bit (depth, normal and colour bytes) on the plane, the furnished room at 4 mm, a 1 mm volume,
    other sizes and intrinsics, batches, -inf poses, a deintegrated and garbage-collected volume; the volume and the stream order untouched by a ray
    cast; a sanity check against the analytic room; bin/depthsensing --render-depth.
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tests", "raycast_checker.c")
TOOL = os.path.join(ROOT, "bin", "depthsensing")
SF_ERR_INVALID_ARG = -1
PLANE_RGB = (200, 120, 41)
NORMAL_Z = np.array([0.0, 0.0, -1.0])   # gradient of the plane's sdf (2 - z): it grows towards the camera


def f32(x):
    return np.float32(x)


def _has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


class RcArgs(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("mx", C.c_float), ("my", C.c_float),
                ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("ray_increment_factor", C.c_float), ("thres_sample_dist_factor", C.c_float), ("thres_dist_factor", C.c_float),
                ("refine_iters", C.c_int32), ("voxel_size", C.c_float), ("trunc_base", C.c_float)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("gcc") is None or not _has_fma():
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    so = str(tmp_path_factory.mktemp("rc") / "libraycast_checker.so")
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, CHECKER, "-lm"], check=True)
    L = C.CDLL(so)
    L.rc_raycast.restype = C.c_int64
    L.rc_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(RcArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def ray_intrinsics(W, H, fW, fH, fx, fy, mx, my):
    """The intrinsics sf_raycast_params' zeros stand for: the fuser's, scaled by width / W and height / H, in float."""
    sx, sy = f32(W) / f32(fW), f32(H) / f32(fH)
    return f32(fx) * sx, f32(fy) * sy, f32(mx) * sx, f32(my) * sy


def rc_args(W, H, K, voxel=0.004, trunc_base=0.06, **over):
    a = RcArgs(W, H, K[0], K[1], K[2], K[3], 0.1, 6.0, 0.8, 50.5, 50.0, 3, voxel, trunc_base)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def check_cast(L, coords, vox, args, pose):
    H, W = args.height, args.width
    depth = np.empty((H, W), np.float32)
    nrm = np.empty((H, W, 3), np.float32)
    rgb = np.empty((H, W, 3), np.uint8)
    coords = np.ascontiguousarray(coords, np.int32)
    vox = np.ascontiguousarray(vox)
    pose = np.ascontiguousarray(pose, np.float32).reshape(16)
    L.rc_raycast(coords.ctypes.data, vox.ctypes.data, len(coords), C.byref(args), pose.ctypes.data, depth.ctypes.data, nrm.ctypes.data, rgb.ctypes.data)
    return depth, nrm, rgb


def plane_truth(pose, W, H, K, z_plane=2.0, inset=0.064, half=None):
    """Analytic depth along camera z where each pixel's ray meets the plane z = z_plane (world), and whether that point lies `inset` metres inside
    the region the identity-pose plane frame fused (half = its half extents at z_plane)."""
    fx, fy, mx, my = (float(k) for k in K)
    u = (np.arange(W, dtype=np.float64) - mx) / fx
    v = (np.arange(H, dtype=np.float64) - my) / fy
    c = np.stack(np.broadcast_arrays(u[None, :], v[:, None], np.ones((H, W))), -1)
    R = pose[:3, :3].astype(np.float64)
    o = pose[:3, 3].astype(np.float64)
    w = c @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = (z_plane - o[2]) / w[..., 2]
    X = o[None, None, :] + lam[..., None] * w
    inside = (lam > 0) & (np.abs(X[..., 0]) <= half[0] - inset) & (np.abs(X[..., 1]) <= half[1] - inset)
    return lam, inside


def yawed(dx, yaw_deg):
    """camToWorld: the identity camera moved dx metres along its x axis and turned yaw_deg about its (vertical) y axis."""
    t = np.radians(yaw_deg)
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(t), np.sin(t), -np.sin(t), np.cos(t)
    m[0, 3] = dx
    return m


PLANE_HALF = ((319.5 / 577.87) * 2.0, (239.5 / 577.87) * 2.0)   # the identity plane frame's extent at 2 m (pixel centres 0 and W - 1)


def assert_plane_answers(depth, nrm, rgb, pose, W, H, K, color=True):
    lam, inside = plane_truth(pose, W, H, K, half=PLANE_HALF)
    hit = np.isfinite(depth)
    assert hit[inside].all(), "%d pixels inside the fused region missed" % int((~hit & inside).sum())
    assert np.abs(depth[hit] - lam[hit]).max() < 1e-4          # a hit is never at a wrong depth, border or not
    assert np.isneginf(depth[~hit]).all()
    assert np.isneginf(nrm[~hit]).all() and (rgb[~hit] == 0).all()
    good = hit & inside
    assert np.abs(nrm[good] - NORMAL_Z).max() < 1e-4
    ok_n = np.isneginf(nrm[hit]).all(-1) | (np.abs(nrm[hit] - NORMAL_Z).max(-1) < 1e-4)
    assert ok_n.all()
    if color:
        assert (rgb[hit] == np.array(PLANE_RGB, np.uint8)).all()
    return int(hit.sum()), int(good.sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the checker against analytic answers
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_plane(oracle):
    p = oracle.default_params()
    vol = oracle.Volume(p, threads=8)
    rgb = np.empty((480, 640, 3), np.uint8)
    rgb[...] = PLANE_RGB
    vol.integrate(synth.plane_frame(), np.eye(4, dtype=np.float32), rgb=rgb)
    coords, vox = vol.export()
    vol.close()
    return coords, vox


@pytest.mark.parametrize("pose_name", ["same", "shifted_yawed"])
def test_checker_plane_known_answers(checker, oracle_plane, pose_name):
    coords, vox = oracle_plane
    W, H = 160, 120
    K = ray_intrinsics(W, H, 640, 480, 577.87, 577.87, 319.5, 239.5)
    pose = np.eye(4, dtype=np.float32) if pose_name == "same" else yawed(0.3, 10.0)
    depth, nrm, rgb = check_cast(checker, coords, vox, rc_args(W, H, K), pose)
    hits, good = assert_plane_answers(depth, nrm, rgb, pose, W, H, K)
    assert good > 0.6 * W * H and hits >= good


def test_checker_misses(checker, oracle_plane):
    coords, vox = oracle_plane
    K = ray_intrinsics(80, 60, 640, 480, 577.87, 577.87, 319.5, 239.5)
    away = synth.yaw_pose(0, 0, 0, 0)   # world z up: the camera looks along world +x, parallel to the plane
    back = yawed(0.0, 180.0)             # looking straight away from the plane
    for pose in (away, back):
        depth, nrm, rgb = check_cast(checker, coords, vox, rc_args(80, 60, K), pose)
        assert np.isneginf(depth).all() and np.isneginf(nrm).all() and (rgb == 0).all()
    nan_pose = np.eye(4, dtype=np.float32)
    nan_pose[1, 3] = np.nan
    depth, nrm, rgb = check_cast(checker, coords, vox, rc_args(80, 60, K), nan_pose)
    assert np.isneginf(depth).all() and np.isneginf(nrm).all() and (rgb == 0).all()
    empty_c, empty_v = np.zeros((0, 3), np.int32), np.zeros((0, 4096), np.uint8)
    depth, nrm, rgb = check_cast(checker, empty_c, empty_v, rc_args(80, 60, K), np.eye(4, dtype=np.float32))
    assert np.isneginf(depth).all() and np.isneginf(nrm).all() and (rgb == 0).all()


def test_checker_thresholds_and_depth_range(checker, oracle_plane):
    coords, vox = oracle_plane
    K = ray_intrinsics(80, 60, 640, 480, 577.87, 577.87, 319.5, 239.5)
    eye = np.eye(4, dtype=np.float32)
    depth, _, _ = check_cast(checker, coords, vox, rc_args(80, 60, K, depth_max=1.5), eye)
    assert np.isneginf(depth).all()                     # the plane lies beyond the render range
    depth, _, _ = check_cast(checker, coords, vox, rc_args(80, 60, K, thres_dist_factor=1e-6), eye)
    assert np.isneginf(depth).all()                     # |s_b| < thres_dist_factor * delta fails everywhere
    depth, _, _ = check_cast(checker, coords, vox, rc_args(80, 60, K, refine_iters=1), eye)
    assert np.isfinite(depth).mean() > 0.6 and np.abs(depth[np.isfinite(depth)] - 2.0).max() < 1e-4   # linear sdf: one step is exact


# ---------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the parameter surface of the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_raycast_params_default_and_file(tmp_path):
    from scannet_amd import fusion
    r = fusion.default_raycast_params()
    assert (r.width, r.height, r.fx, r.fy, r.mx, r.my) == (0, 0, 0.0, 0.0, 0.0, 0.0)
    assert (r.depth_min, r.depth_max) == (f32(0.1), f32(6.0))
    assert (r.ray_increment_factor, r.thres_sample_dist_factor, r.thres_dist_factor, r.refine_iters) == (f32(0.8), f32(50.5), f32(50.0), 3)
    path = tmp_path / "zParametersScanNet.txt"
    path.write_text("s_SDFVoxelSize = 0.010f;\ns_rayCastWidth = 320;\t//should be same as integration except if rendering video\n"
                    "s_rayCastHeight = 240;\ns_renderDepthMax = 5.5f;\ns_renderDepthMin = 0.25f;\ns_SDFRayIncrementFactor = 0.5f;\n"
                    "s_SDFRayThresSampleDistFactor = 40.5f;\ns_SDFRayThresDistFactor = 30.0f;\n")
    r = fusion.load_raycast_params(path)
    assert (r.width, r.height) == (320, 240)
    assert (r.depth_min, r.depth_max) == (f32(0.25), f32(5.5))
    assert (r.ray_increment_factor, r.thres_sample_dist_factor, r.thres_dist_factor, r.refine_iters) == (f32(0.5), f32(40.5), f32(30.0), 3)
    plain = tmp_path / "plain.txt"
    plain.write_text("s_SDFVoxelSize = 0.010f;\ns_sensorDepthMax = 4.0f;\n")
    r = fusion.load_raycast_params(plain)
    d = fusion.default_raycast_params()
    assert bytes(r) == bytes(d)
    # sf_params is not touched by the ray-cast keys, and the ray-cast loader ignores the fusion keys
    p = fusion.load_params(path)
    assert p.voxel_size == f32(0.010) and p.depth_max == f32(6.0)
    bad = tmp_path / "bad.txt"
    bad.write_text("s_renderDepthMax = deep;\n")
    with pytest.raises(_abi.ScanfuseError):
        fusion.load_raycast_params(bad)
    for text in ("s_renderDepthMax = inf;\n", "s_renderDepthMin = nan;\n", "s_SDFRayIncrementFactor = 1e60f;\n"):   # not finite as a float
        bad.write_text(text)
        with pytest.raises(_abi.ScanfuseError):
            fusion.load_raycast_params(bad)


@pytest.mark.parametrize("field,value,words", [("refine_iters", 0, "refine_iters"), ("refine_iters", 9, "refine_iters"),
                                               ("depth_min", 6.0, "depth range"), ("depth_max", 0.05, "depth range"),
                                               ("ray_increment_factor", 0.0, "increment"), ("ray_increment_factor", -0.8, "increment"),
                                               ("width", -1, "image"), ("height", 240, "image"),
                                               ("depth_max", float("inf"), "depth range"), ("depth_min", float("-inf"), "depth range"),
                                               ("depth_min", float("nan"), "depth range"), ("ray_increment_factor", float("inf"), "increment"),
                                               ("ray_increment_factor", float("nan"), "increment"), ("thres_dist_factor", float("nan"), "threshold"),
                                               ("thres_sample_dist_factor", float("inf"), "threshold")])
def test_invalid_raycast_params_are_refused(field, value, words):
    """Checked before the fuser is looked at: the same refusal with or without a GPU (tests below repeat it on a real fuser)."""
    from scannet_amd import fusion
    L = _abi.lib()
    L.sf_fuser_raycast.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(fusion.SfRaycastParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.sf_fuser_raycast_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(fusion.SfRaycastParams), C.c_void_p, C.c_void_p, C.c_void_p]
    r = fusion.default_raycast_params(**{field: value})
    pose = np.eye(4, dtype=np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    assert L.sf_fuser_raycast(None, pose.ctypes.data, C.byref(r), out.ctypes.data, None, None) == SF_ERR_INVALID_ARG
    assert words in L.sf_last_error().decode()
    assert L.sf_fuser_raycast_device(None, pose.ctypes.data, 1, C.byref(r), out.ctypes.data, None, None) == SF_ERR_INVALID_ARG
    assert words in L.sf_last_error().decode()
    good = fusion.default_raycast_params()
    assert L.sf_fuser_raycast(None, pose.ctypes.data, C.byref(good), out.ctypes.data, None, None) == SF_ERR_INVALID_ARG
    assert "NULL fuser" in L.sf_last_error().decode()


def test_raycast_params_layout_matches_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "scanfuse.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(sf_raycast_params), offsetof(sf_raycast_params, refine_iters), offsetof(sf_raycast_params, thres_dist_factor));
  return 0;
}'''
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = str(tmp_path / "rc_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", exe, "-"], input=src, text=True, check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    from scannet_amd import fusion
    R = fusion.SfRaycastParams
    assert got == [C.sizeof(R), R.refine_iters.offset, R.thres_dist_factor.offset]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU: k_raycast against the checker, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _same_bits(got, want, what):
    for g, w, name in zip(got, want, ("depth", "normals", "rgb")):
        if g is None:
            continue
        if g.tobytes() != w.tobytes():
            bad = np.argwhere((g.view(np.uint8) != w.view(np.uint8)).reshape(g.shape[0], g.shape[1], -1).any(-1))
            y, x = bad[0]
            raise AssertionError("%s %s: %d pixels differ, first (%d, %d): gpu %r checker %r" % (what, name, len(bad), x, y, g[y, x], w[y, x]))


def _gpu_vs_checker(checker, f, pose, params, what):
    """f.raycast against the checker on f's own export_blocks(); returns the GPU images."""
    got = f.raycast(pose, params)
    W, H = f.raycast_size(params)
    p = f.params
    assert p.integration_width == 0   # the fuser's intrinsics are sf_params' own (no resampling in these tests)
    if params.fx == 0 and params.fy == 0 and params.mx == 0 and params.my == 0:
        K = ray_intrinsics(W, H, p.depth_width, p.depth_height, p.fx, p.fy, p.mx, p.my)
    else:
        K = (params.fx, params.fy, params.mx, params.my)
    coords, vox = f.export_blocks()
    a = rc_args(W, H, K, voxel=p.voxel_size, trunc_base=p.trunc_base, depth_min=params.depth_min, depth_max=params.depth_max,
                ray_increment_factor=params.ray_increment_factor, thres_sample_dist_factor=params.thres_sample_dist_factor,
                thres_dist_factor=params.thres_dist_factor, refine_iters=params.refine_iters)
    want = check_cast(checker, coords, vox, a, pose)
    _same_bits(got, want, what)
    return got, K


def _volume_digest(f):
    c, v = f.export_blocks()
    return hashlib.sha256(c.tobytes() + v.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def gpu_plane():
    from scannet_amd import fusion
    f = fusion.Fuser(fusion.default_params(num_sdf_blocks=1 << 17), device=0)
    rgb = np.empty((480, 640, 3), np.uint8)
    rgb[...] = PLANE_RGB
    assert f.integrate(synth.plane_frame(), np.eye(4, dtype=np.float32), rgb=rgb)
    yield f
    f.close()


@pytest.mark.gpu
def test_gpu_plane_bit_exact_and_analytic(checker, gpu_plane, oracle_plane):
    from scannet_amd import fusion
    f = gpu_plane
    oc, ov = oracle_plane
    gc, gv = f.export_blocks()
    assert np.array_equal(oc, gc) and ov.tobytes() == gv.tobytes()   # the GPU fused the oracle's volume: the plane answers carry over
    K = (f32(577.87), f32(577.87), f32(319.5), f32(239.5))
    for pose in (np.eye(4, dtype=np.float32), yawed(0.3, 10.0)):
        (depth, nrm, rgb), _ = _gpu_vs_checker(checker, f, pose, fusion.default_raycast_params(), "plane")
        assert depth.shape == (480, 640)
        hits, good = assert_plane_answers(depth, nrm, rgb, pose, 640, 480, K)
        assert good > 0.6 * 640 * 480
    for pose in (synth.yaw_pose(0, 0, 0, 0), yawed(0.0, 180.0)):
        depth, nrm, rgb = f.raycast(pose)
        assert np.isneginf(depth).all() and np.isneginf(nrm).all() and (rgb == 0).all()


@pytest.mark.gpu
def test_gpu_empty_volume_and_invalid_params():
    from scannet_amd import fusion
    with fusion.Fuser(fusion.default_params(num_sdf_blocks=1 << 12), device=0) as f:
        depth, nrm, rgb = f.raycast(np.eye(4, dtype=np.float32), fusion.default_raycast_params(width=64, height=48))
        assert np.isneginf(depth).all() and np.isneginf(nrm).all() and (rgb == 0).all()
        for over in ({"refine_iters": 0}, {"refine_iters": 9}, {"depth_min": 7.0}, {"ray_increment_factor": 0.0}, {"width": -4, "height": 3},
                     {"depth_max": float("inf")}, {"depth_min": float("-inf")}, {"fx": float("nan"), "fy": 1.0},
                     {"ray_increment_factor": 1e-9}, {"depth_max": 1e6}):   # the last two: a ray would take 1e10 / 2e7 samples
            with pytest.raises(_abi.ScanfuseError) as e:
                f.raycast(np.eye(4, dtype=np.float32), fusion.default_raycast_params(**over))
            assert e.value.code == SF_ERR_INVALID_ARG
            with pytest.raises(_abi.ScanfuseError):
                f.raycast_size(fusion.default_raycast_params(**over))
        # the bound on the samples of a ray: 65 536, counted at the image's farthest corner (rho = 1.2155 at 640 x 480, fx = 577.87)
        assert f.raycast_size(fusion.default_raycast_params(depth_max=0.1 + 65536 * 0.048 / 1.22)) == (640, 480)
        with pytest.raises(_abi.ScanfuseError) as e:
            f.raycast_size(fusion.default_raycast_params(depth_max=0.1 + 65536 * 0.048 / 1.21))
        assert "samples" in str(e.value)
        assert f.raycast_size(fusion.default_raycast_params(width=200, height=150)) == (200, 150)


def _room_rgb(i, W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(xx + 5 * i) % 256, (yy * 2 + 3 * i) % 256, (xx + yy + 7 * i) % 256], -1).astype(np.uint8)


N_ROOM = 200


@pytest.fixture(scope="module")
def gpu_room():
    """The furnished room, noisy RGB-D stream, 200 frames of the walk, 4 mm."""
    from scannet_amd import fusion
    f = fusion.Fuser(fusion.default_params(), device=0)
    boxes = synth.clutter_boxes()
    for i in range(N_ROOM):
        pose = synth.trajectory_pose(i, N_ROOM)
        d = synth.render_room_depth(pose, 640, 480, noise_frame=i, noise=2, boxes=boxes)
        assert f.integrate(d, pose, rgb=_room_rgb(i, 640, 480))
    f.sync()
    yield f
    f.close()


def _room_poses():
    low = synth.yaw_pose(3.0, 2.0, 0.12, 0.3)   # 12 cm above the floor, level: the lower image corners graze it
    return {
        "integrated_0": synth.trajectory_pose(0, N_ROOM), "integrated_100": synth.trajectory_pose(100, N_ROOM),
        "between_10.5": synth.trajectory_pose(10.5, N_ROOM), "between_120.5": synth.trajectory_pose(120.5, N_ROOM),
        "outside": synth.yaw_pose(-1.0, 2.0, 1.5, 0.0), "grazing_floor": low,
        "centre_up": synth.yaw_pose(3.0, 2.0, 2.4, 2.0), "integrated_150": synth.trajectory_pose(150, N_ROOM),
    }


@pytest.mark.gpu
def test_gpu_room_eight_poses_bit_exact(checker, gpu_room):
    from scannet_amd import fusion
    f = gpu_room
    small = fusion.default_raycast_params(width=320, height=240)
    hit_share = {}
    for name, pose in _room_poses().items():
        (depth, nrm, rgb), _ = _gpu_vs_checker(checker, f, pose, small, name)
        hit_share[name] = float(np.isfinite(depth).mean())
    # the full default size once (the fuser's own intrinsics, no scaling)
    _gpu_vs_checker(checker, f, _room_poses()["integrated_0"], fusion.default_raycast_params(), "integrated_0 640x480")
    assert hit_share["integrated_0"] > 0.9 and hit_share["between_10.5"] > 0.9, hit_share
    assert hit_share["grazing_floor"] > 0.2, hit_share   # fused frames dropped the floor where they saw it below ~7 degrees (synth's sensor holes)


@pytest.mark.gpu
def test_gpu_room_sizes_file_and_intrinsics(checker, gpu_room, tmp_path):
    from scannet_amd import fusion
    f = gpu_room
    path = tmp_path / "zParametersScanNet.txt"
    path.write_text("s_rayCastWidth = 320;\ns_rayCastHeight = 240;\ns_renderDepthMax = 6.0f;\ns_renderDepthMin = 0.1f;\n"
                    "s_SDFRayIncrementFactor = 0.8f;\ns_SDFRayThresSampleDistFactor = 50.5f;\ns_SDFRayThresDistFactor = 50.0f;\n")
    r = fusion.load_raycast_params(path)
    pose = synth.trajectory_pose(40, N_ROOM)
    (d320, _, _), _ = _gpu_vs_checker(checker, f, pose, r, "file 320x240")
    assert d320.shape == (240, 320)
    explicit = fusion.default_raycast_params(width=200, height=150, fx=180.0, fy=175.5, mx=97.25, my=76.0, refine_iters=5, depth_max=4.0)
    (d, n, c), _ = _gpu_vs_checker(checker, f, pose, explicit, "explicit intrinsics")
    assert d.shape == (150, 200) and np.isfinite(d).mean() > 0.5
    assert d[np.isfinite(d)].max() <= 4.0


@pytest.mark.gpu
def test_gpu_batch_equals_single_calls(gpu_room):
    import torch
    from scannet_amd import fusion
    f = gpu_room
    r = fusion.default_raycast_params(width=160, height=120)
    n = 32
    poses = np.stack([synth.trajectory_pose(i * 6.25 + 0.5, N_ROOM).reshape(16) for i in range(n)]).astype(np.float32)
    lost = [3, 17, 25, 31]
    poses[[3, 17, 31]] = -np.inf          # "tracking lost"
    poses[25, 7] = np.nan                 # anything that is not a number in the first three rows: a lost pose too
    dd = torch.empty((n, 120, 160), dtype=torch.float32, device="cuda:0")
    dn = torch.empty((n, 120, 160, 3), dtype=torch.float32, device="cuda:0")
    dc = torch.empty((n, 120, 160, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    f.raycast_device(poses, dd, dn, dc, params=r)
    f.sync()
    bd, bn, bc = dd.cpu().numpy(), dn.cpu().numpy(), dc.cpu().numpy()
    for i in range(n):
        if i in lost:
            assert np.isneginf(bd[i]).all() and np.isneginf(bn[i]).all() and (bc[i] == 0).all()
            continue
        d, nr, c = f.raycast(poses[i], r)
        assert d.tobytes() == bd[i].tobytes() and nr.tobytes() == bn[i].tobytes() and c.tobytes() == bc[i].tobytes(), i
        assert np.isfinite(d).mean() > 0.5
    # depth only, into one buffer: the same depth bits
    dd2 = torch.empty((n, 120, 160), dtype=torch.float32, device="cuda:0")
    f.raycast_device(poses, dd2, None, None, params=r)
    f.sync()
    assert dd2.cpu().numpy().tobytes() == bd.tobytes()


@pytest.mark.gpu
def test_gpu_raycast_leaves_the_volume_alone(gpu_room):
    from scannet_amd import fusion
    f = gpu_room
    before, st0 = _volume_digest(f), f.stats()
    for pose in _room_poses().values():
        f.raycast(pose, fusion.default_raycast_params(width=160, height=120))
    assert _volume_digest(f) == before and f.stats() == st0


def _plane_fuser():
    from scannet_amd import fusion
    return fusion.Fuser(fusion.default_params(num_sdf_blocks=1 << 17), device=0)


@pytest.mark.gpu
def test_gpu_stream_order_integrate_raycast_integrate():
    """A ray cast queued between two frames sees the first (and only the first) and changes nothing the second computes."""
    from scannet_amd import fusion
    boxes = synth.clutter_boxes()
    frames = [(synth.render_room_depth(synth.trajectory_pose(i, 40), 320, 240, noise_frame=i, noise=2, boxes=boxes), synth.trajectory_pose(i, 40))
              for i in range(6)]
    K = synth.intrinsics(320, 240)
    gp = fusion.default_params(depth_width=320, depth_height=240, fx=K[0], fy=K[1], mx=K[2], my=K[3])   # a heap that never runs out: which blocks
    r = fusion.default_raycast_params()                                                                  # an exhausted heap refuses is a race
    with fusion.Fuser(gp, device=0) as a, fusion.Fuser(gp, device=0) as b, fusion.Fuser(gp, device=0) as c:
        import torch
        buf = torch.empty((len(frames), 240, 320), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for k, (d, pose) in enumerate(frames):
            assert a.integrate(d, pose) and b.integrate(d, pose) and c.integrate(d, pose)
            a.raycast_device(pose, buf[k], params=r)        # queued, not waited for
            want = c.raycast(pose, r)[0]                    # synchronous, on a volume that saw the same frames
            a.sync()
            assert buf[k].cpu().numpy().tobytes() == want.tobytes(), k
        assert a.stats()["alloc_failures"] == 0
        assert _volume_digest(a) == _volume_digest(b) == _volume_digest(c)
        assert a.stats()["blocks_allocated"] == b.stats()["blocks_allocated"]


@pytest.mark.gpu
def test_gpu_after_deintegrate_and_garbage_collect(checker):
    from scannet_amd import fusion
    with _plane_fuser() as f:
        eye = np.eye(4, dtype=np.float32)
        near = synth.plane_frame(depth_mm=1500)
        assert f.integrate(synth.plane_frame(), eye)
        assert f.integrate(near, yawed(0.1, 5.0))
        assert f.deintegrate(near, yawed(0.1, 5.0))
        assert f.garbage_collect() > 0
        for pose in (eye, yawed(0.3, 10.0)):
            (depth, _, _), _ = _gpu_vs_checker(checker, f, pose, fusion.default_raycast_params(width=320, height=240), "after gc")
            fin = np.isfinite(depth)
            assert fin.mean() > 0.5


@pytest.mark.gpu
def test_gpu_one_millimetre(checker):
    """A plane 1 m away seen from two poses, fused at 1 mm voxels (~70 k blocks at 160 x 120)."""
    from scannet_amd import fusion
    W, H = 160, 120
    K = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=K[0], fy=K[1], mx=K[2], my=K[3], voxel_size=0.001, num_sdf_blocks=1 << 19)
    Kf = tuple(f32(k) for k in K)
    with fusion.Fuser(gp, device=0) as f:
        eye, turned = np.eye(4, dtype=np.float32), yawed(0.05, 3.0)
        assert f.integrate(synth.plane_frame(W, H, 1000), eye)
        lam, _ = plane_truth(turned, W, H, Kf, z_plane=1.0, half=(1.0, 1.0))
        assert f.integrate(np.rint(lam * 1000.0).astype(np.uint16), turned)
        assert f.stats()["alloc_failures"] == 0
        (depth, nrm, _), _ = _gpu_vs_checker(checker, f, eye, fusion.default_raycast_params(), "1 mm")
        hit = np.isfinite(depth)
        assert hit.mean() > 0.6 and np.abs(depth[hit] - 1.0).max() < 1e-3
        _gpu_vs_checker(checker, f, yawed(0.02, 1.5), fusion.default_raycast_params(width=120, height=90), "1 mm moved")


@pytest.mark.gpu
def test_gpu_room_against_ground_truth():
    """Noise-free room at an integrated pose: the ray-cast depth agrees with the analytic depth within 2 voxels + 1 mm on >= 95 % of the pixels whose
    analytic depth lies in [0.5, 3.5] m."""
    from scannet_amd import fusion
    boxes = synth.clutter_boxes()
    with fusion.Fuser(fusion.default_params(), device=0) as f:
        for i in range(0, N_ROOM, 2):
            pose = synth.trajectory_pose(i, N_ROOM)
            assert f.integrate(synth.render_room_depth(pose, 640, 480, boxes=boxes), pose)
        for i in (40, 130):
            pose = synth.trajectory_pose(i, N_ROOM)
            truth = synth.render_room_depth(pose, 640, 480, boxes=boxes).astype(np.float64) / 1000.0
            depth = f.raycast(pose, normals=False, color=False)[0].astype(np.float64)
            band = (truth >= 0.5) & (truth <= 3.5)
            err = np.where(np.isfinite(depth), np.abs(depth - truth), np.inf)
            ok = err[band] <= 2 * 0.004 + 0.001
            assert ok.mean() >= 0.95, (i, ok.mean(), np.isfinite(depth[band]).mean(), np.median(err[band][np.isfinite(err[band])]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# GPU: bin/depthsensing --render-depth
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _small_scan(tmp_path, n, W, H):
    from scannet_amd import sens
    K = synth.intrinsic_matrix(W, H)
    sd = sens.SensorData.create(0, 0, W, H, K, K, sensor_name="StructureSensor")
    boxes = synth.clutter_boxes()
    for i in range(n):
        pose = synth.trajectory_pose(i * 4, 200)
        if i == 10:
            pose = np.full((4, 4), -np.inf, np.float32)   # tracking lost: no image for this frame
            d = synth.render_room_depth(synth.trajectory_pose(i * 4, 200), W, H, noise_frame=i, boxes=boxes)
        else:
            d = synth.render_room_depth(pose, W, H, noise_frame=i, boxes=boxes)
        sd.add_frame(d, pose, timestamp_depth=i)
    path = str(tmp_path / "scan.sens")
    sd.save(path)
    sd.close()
    params = tmp_path / "zParametersScanNet.txt"
    params.write_text("s_SDFVoxelSize = 0.010f;\ns_SDFTruncation = 0.06f;\ns_SDFTruncationScale = 0.02f;\ns_hashNumSDFBlocks = 200000;\n"
                      "s_hashNumBuckets = 100000;\ns_renderDepthMax = 6.0f;\n")
    (tmp_path / "t.txt").write_text("// tracking\n")
    return [str(params), str(tmp_path / "t.txt"), path]


@pytest.mark.gpu
def test_gpu_depthsensing_render_depth(tmp_path):
    from scannet_amd import fusion, sens
    L = _abi.lib()
    W, H, n = 160, 120, 23
    plain_dir, flag_dir = tmp_path / "plain", tmp_path / "flag"
    plain_dir.mkdir()
    flag_dir.mkdir()
    args_p = _small_scan(plain_dir, n, W, H)
    args_f = [args_p[0], args_p[1], args_p[2], str(flag_dir / "scan_vh.ply")]
    out_png = tmp_path / "d"
    r0 = subprocess.run([TOOL] + args_p, capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and r0.stderr == "", r0.stderr
    r1 = subprocess.run([TOOL] + args_f + ["--render-depth=%s" % out_png, "--render-every=5"], capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0 and r1.stderr == "", r1.stderr
    assert open(str(plain_dir / "scan_vh.ply"), "rb").read() == open(str(flag_dir / "scan_vh.ply"), "rb").read()
    want_frames = [i for i in range(0, n, 5) if i != 10]
    assert sorted(os.listdir(str(out_png))) == sorted("%d.png" % i for i in want_frames)
    # the same volume in Python: the file's parameters, fused by sf_fuse_run as the tool does it
    p = fusion.load_params(args_p[0])
    sd = sens.SensorData(args_p[2])
    p.depth_width, p.depth_height = W, H
    K = sd.intrinsic_depth
    p.fx, p.fy, p.mx, p.my = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    p.depth_shift = sd.depth_shift
    r = fusion.load_raycast_params(args_p[0])
    L.sf_png_read.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    with fusion.Fuser(p, device=0) as f:
        f.run(sd)
        for i in want_frames:
            assert sd.frames[i].valid_pose
            depth = f.raycast(sd.frames[i].camera_to_world, r, normals=False, color=False)[0]
            v = depth * f32(1000.0)
            want = np.where(depth > 0, np.minimum(np.floor(v.astype(np.float64) + 0.5), 65535), 0).astype(np.uint16)
            w, h, ch, bits, data = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_int(), C.c_void_p()
            _abi.check(L.sf_png_read(str(out_png / ("%d.png" % i)).encode(), C.byref(w), C.byref(h), C.byref(ch), C.byref(bits), C.byref(data)))
            assert (w.value, h.value, ch.value, bits.value) == (W, H, 1, 16)
            got = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint16)), shape=(H, W)).copy()
            L.sf_free.argtypes = [C.c_void_p]
            L.sf_free(data)
            assert np.array_equal(got, want), i
            assert (got > 0).mean() > 0.5
    sd.close()
    r2 = subprocess.run([TOOL, "--ranks", "2", "--share-gpu"] + args_p + ["--render-depth=%s" % (tmp_path / "e")], capture_output=True, text=True, timeout=120)
    assert r2.returncode != 0 and "--render-depth" in r2.stderr and "--ranks" in r2.stderr
    assert not os.path.exists(str(tmp_path / "e"))


def test_checker_sample_bound(checker, oracle_plane):
    """A ray takes at most K = ceil((depth_max - depth_min) * rho_max / delta) + 2 samples, and K above 65 536 is refused (the library's rule)."""
    coords, vox = oracle_plane
    K = ray_intrinsics(80, 60, 640, 480, 577.87, 577.87, 319.5, 239.5)
    a = rc_args(80, 60, K, ray_increment_factor=1e-9)
    out = np.zeros((60, 80), np.float32)
    pose = np.eye(4, dtype=np.float32).reshape(16)
    assert checker.rc_raycast(coords.ctypes.data, vox.ctypes.data, len(coords), C.byref(a), pose.ctypes.data, out.ctypes.data, None, None) == -1
    assert (out == 0).all()
    # the longest march allowed still finds the plane
    depth, _, _ = check_cast(checker, coords, vox, rc_args(80, 60, K, depth_max=3.0, ray_increment_factor=0.8), np.eye(4, dtype=np.float32))
    assert np.isfinite(depth).mean() > 0.6
