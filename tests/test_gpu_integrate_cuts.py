"""The instruction cuts of k_integrate's frame loop (scannet_amd/csrc/fuser_fuse.h), bit for bit against the oracle:

  * the integration-distance gate applied once per pixel by the pre-pass (k_prepass, and the conversion fused into k_alloc_ray) instead of per voxel and frame;
  * the new voxel written under its update mask by the instruction that produces it, instead of computed for all eight voxels and selected;
  * "in front of the camera" decided once per lane from the two end voxels of its x-row, voxel by voxel only in a wave the camera plane cuts;
  * the reciprocal of the camera-space depth: one Newton step where the device's reciprocal seed allows it, two where not.

Three scenes of four 64 x 48 frames, each fused by every kernel the cuts touch -- passes of 2 and of 4 frames with and without colour (the x-row kernels, 8 and
5 waves per SIMD), one frame per launch with colour (k_integrate with per-row write-back) and without (k_integrate_pipe) --, then one deintegration and one
re-integration.  The oracle fuses each scene once per colour setting; every schedule is compared with that one export.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_tsdf import _DeviceFrames, _assert_same, _mk

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 4
BLOCKS = 1 << 16


def _rgb(k):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(5 * xx + 40 * k) % 256, (7 * yy + 90 * k + 1) % 256, (3 * xx + 2 * yy + 11 * k) % 256], -1).astype(np.uint8)


def _shift(k):
    p = np.eye(4, dtype=np.float32)
    p[:3, 3] = (0.011 * k, -0.006 * k, 0.004 * k)
    return p


def _look(centre, forward):
    """camToWorld of a camera at `centre` looking along `forward` (columns: camera x, y, z)."""
    z = np.asarray(forward, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross((0.0, 1.0, 0.0), z)
    x /= np.linalg.norm(x)
    p = np.eye(4)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = x, np.cross(z, x), z, centre
    return p.astype(np.float32)


def _scene(name):
    depth = np.zeros((N, H, W), np.uint16)
    poses = [None] * N
    for k in range(N):
        if name == "gate":
            # a near wall, and patches on both sides of the integration distance (depth shift 1000, max_integration_dist 4.0: 3999 is fused, 4000 and 4001 are
            # not), between the gate and depth_max (6.0), beyond depth_max, and without a measurement
            d = np.full((H, W), 1500 + 3 * k, np.uint16)
            for i, v in enumerate((3999, 4000, 4001, 5000, 0, 6500)):
                d[4 + k:11 + k, 3 + 10 * i:10 + 10 * i] = v
            d[30:36, 8:56:3] = (3999, 4001, 0, 4000) * 4   # ... and pixel by pixel
            depth[k], poses[k] = d, _shift(k)
        elif name == "tilted":
            # a plane tilted against the block grid: the edge of the truncation band cuts blocks obliquely
            yy, xx = np.mgrid[0:H, 0:W]
            depth[k], poses[k] = (900 + 4 * xx + 3 * yy + 7 * k).astype(np.uint16), _shift(k)
        else:
            # frame 0 puts a wall's band at z = 1; the other frames look from INSIDE that band, along a direction with a world-x component: their camera
            # plane cuts x-rows of blocks frame 0 allocated
            if k == 0:
                depth[k], poses[k] = np.full((H, W), 1000, np.uint16), np.eye(4, dtype=np.float32)
            else:
                depth[k], poses[k] = np.full((H, W), 1500 - 100 * k, np.uint16), _look(CUT_CENTRES[k], (1.0, 0.2 * k - 0.3, 0.3))
    return depth, np.stack(poses).reshape(N, 16), np.stack([_rgb(k) for k in range(N)])


CUT_CENTRES = {1: (0.0142, 0.0221, 1.0103), 2: (-0.1018, 0.0502, 0.9861), 3: (0.0863, -0.0418, 1.0142)}   # (inside the box of a block's voxel centres, not in the one-voxel gap between two blocks')
SCENES = ("gate", "tilted", "cut")
_cache = {}


def _reference(oracle, name, colour):
    """(frames, oracle volume holding the scene's four frames, its export): made once per scene and colour setting, never changed by a test."""
    key = (name, colour)
    if key not in _cache:
        depth, poses, rgb = _scene(name)
        op, _ = _mk(oracle, W, H, num_sdf_blocks=BLOCKS)
        vol = oracle.Volume(op, threads=4)
        last = 0
        for k in range(N):
            last = vol.integrate(depth[k], poses[k].reshape(4, 4), rgb=rgb[k] if colour else None)
        _cache[key] = (depth, poses, rgb, last, vol.export())
    return _cache[key]


def _assert_export(ref, fuser):
    oc, ov = ref
    gc, gv = fuser.export_blocks()
    assert np.array_equal(oc, gc), "allocated block sets differ"
    same = ov.view(np.uint8).reshape(len(oc), 512, 8) == gv.view(np.uint8).reshape(len(gc), 512, 8)
    if not same.all():
        b, v = np.argwhere(~same.all(-1))[0]
        raise AssertionError("%d voxels differ; first: block %s voxel %d oracle %s gpu %s" % ((~same.all(-1)).sum(), oc[b], v, ov[b, v], gv[b, v]))
    return gc, gv


SCHEDULES = {"pass2_wide": dict(batch=2, tail_wide=1), "pass2": dict(batch=2, tail_wide=0), "pass4_wide": dict(batch=4, tail_wide=1), "pass4": dict(batch=4, tail_wide=0),
             "one": dict(batch=1)}


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("name", SCENES)
def test_every_changed_kernel_matches_the_oracle(oracle, name, schedule, colour):
    from scannet_amd import fusion
    depth, poses, rgb, last, ref = _reference(oracle, name, colour)
    _, gp = _mk(oracle, W, H, num_sdf_blocks=BLOCKS)
    dev = _DeviceFrames(depth, rgb if colour else None)
    try:
        with fusion.Fuser(gp, **SCHEDULES[schedule]) as f:
            dev.fuse(f, poses, 0, N)
            st = f.stats()
            assert st["frames_integrated"] == N and st["alloc_failures"] == 0 and st["last_frame_blocks"] == last
            coords, vox = _assert_export(ref, f)
    finally:
        dev.close()
    touched = vox["w"] > 0
    if name == "gate":
        assert touched.any()
    if name == "tilted":
        # the case the predicated write-back is about: lanes that update one voxel of a pair and not the other, rows of which only some update
        mixed = touched.any(1) & ~touched.all(1)
        assert mixed.sum() > 100, "no block with touched and untouched voxels"
        pairs = touched.reshape(len(vox), 256, 2)
        assert (pairs[:, :, 0] != pairs[:, :, 1]).any(), "no voxel pair of which only one voxel was updated"
    if name == "cut":
        _assert_camera_plane_cuts_a_live_block(coords, poses, gp.voxel_size)


def _assert_camera_plane_cuts_a_live_block(coords, poses, voxel):
    """For each of the frames that look from inside the band: the block that holds the camera centre is allocated (frame 0 made it) and is live in that frame --
    its centre is nearer to the camera centre than the radius of its bounding sphere, so the conservative frustum test (|a . p| <= |a| |p| for each side plane,
    pz > -radius) admits it -- and some x-row of it (a lane's eight voxels) has voxels on both sides of the camera plane."""
    for k in range(1, N):
        pose = poses[k].reshape(4, 4).astype(np.float64)
        Ti = np.linalg.inv(pose)
        c = pose[:3, 3]
        lo, hi = coords * 8 * voxel, (coords * 8 + 7) * voxel
        inside = np.all((lo <= c) & (c <= hi), axis=1)
        assert inside.sum() == 1, "frame %d: the block around the camera centre is not allocated" % k
        b = coords[inside][0]
        centre = (b * 8 + 3.5) * voxel
        assert np.linalg.norm(centre - c) < 4.0 * np.sqrt(3.0) * voxel
        z, y, x = np.mgrid[0:8, 0:8, 0:8]
        pcz = Ti[2, 0] * (b[0] * 8 + x) * voxel + Ti[2, 1] * (b[1] * 8 + y) * voxel + Ti[2, 2] * (b[2] * 8 + z) * voxel + Ti[2, 3]
        cut_rows = (pcz.min(-1) < -voxel / 4) & (pcz.max(-1) > voxel / 4)
        assert cut_rows.any(), "frame %d: no x-row of the block has voxels on both sides of the camera plane" % k


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_deintegrate_and_reintegrate_match_the_oracle(oracle, name, colour):
    """One frame taken out again (k_integrate<-1>), then one frame moved to another pose in a mixed-sign pass (k_reintegrate): the oracle's deintegrate / integrate."""
    from scannet_amd import fusion
    depth, poses, rgb, _, _ = _reference(oracle, name, colour)
    op, gp = _mk(oracle, W, H, num_sdf_blocks=BLOCKS)
    vol = oracle.Volume(op, threads=4)
    col = (lambda k: rgb[k]) if colour else (lambda k: None)
    with fusion.Fuser(gp) as f:
        for k in range(N):
            p = poses[k].reshape(4, 4)
            vol.integrate(depth[k], p, rgb=col(k))
            assert f.integrate(depth[k], p, rgb=col(k))
        p = poses[1].reshape(4, 4)
        vol.deintegrate(depth[1], p, rgb=col(1))
        assert f.deintegrate(depth[1], p, rgb=col(1))
        _assert_same(vol, f)
        old = poses[2].reshape(4, 4)
        new = old.copy()
        new[:3, 3] += np.float32(0.013)
        vol.deintegrate(depth[2], old, rgb=col(2))
        vol.integrate(depth[2], new, rgb=col(2))
        assert f.reintegrate(depth[2], old, new, rgb=col(2))
        _assert_same(vol, f)


def test_recip_one_step_is_exact_on_this_device():
    """1 / pcz by ONE Newton step from v_rcp_f32 is correctly rounded exactly when the hardware's seed is one of the two floats either side of 1 / b (and, for the
    all-ones mantissa, the upper one): tools/check_division.c part (4).  The device self-test runs all 2^32 bit patterns.  Where recip_rn ships as one step it
    must report no mismatch; where it ships as two, the two-step form is what has to be exact (sf_selftest_division), and the patterns the one step gets wrong
    are printed for the record."""
    from scannet_amd import _abi
    L = _abi.lib()
    n, shipped = C.c_uint64(1), C.c_int(-1)
    pats = (C.c_uint32 * 16)()
    L.sf_selftest_recip_one_step.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_int)]
    _abi.check(L.sf_selftest_recip_one_step(0, C.byref(n), pats, 16, C.byref(shipped)))
    print("one Newton step: %d mismatches over all normal b with a normal reciprocal; shipped: %d; some of them: %s"
          % (n.value, shipped.value, " ".join("%08x" % p for p in sorted(pats[:min(16, n.value)]))))
    assert shipped.value in (0, 1)
    if shipped.value:
        assert n.value == 0
    else:
        a, b, c = C.c_uint64(1), C.c_uint64(1), C.c_uint64(1)
        L.sf_selftest_division.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _abi.check(L.sf_selftest_division(0, C.byref(a), C.byref(b), C.byref(c)))
        assert a.value == 0
