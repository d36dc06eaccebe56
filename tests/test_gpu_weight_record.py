"""The per-weight records of the multi-frame integrate kernels (scannet_amd/csrc/fuser_internal.h fill_weight_records, fuser_fuse.h fuse_update): a pass of
several frames with the shipped parameters reads (float)w, (float)(w + 1), 1 / (w + 1) and the {new weight, "first observation"} word of a voxel from one
16-byte LDS record instead of computing them per voxel and frame.  Held here:

  * the table itself, word for word, for all 256 weights;
  * a dwell of 300 frames on one view: every weight from 0 through the saturation at 255 and 44 frames beyond, with a black first colour frame (a black voxel
    that HAS a weight is not a first observation), a saturated patch and a pattern that changes every frame;
  * 40 frames of a camera that steps sideways over a tilted plane: the lanes of one wave hold different weights, voxels are first observed late;
  * the kernels that keep the float table (colour_first, a small weight_max, one frame per launch) over the same scene.

Every comparison is byte for byte with oracle.Volume: the block set and all 512 x 8 bytes of every block.  The oracle fuses each scene once per parameter
set; what the scenes are meant to contain is asserted on the oracle's own exports.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_tsdf import _DeviceFrames, _mk

pytestmark = pytest.mark.gpu

W, H = 64, 48
BLOCKS = 1 << 16
N_DWELL, N_MIXED = 300, 40


def test_table_is_the_statement_of_its_four_words():
    from scannet_amd import _abi
    L = _abi.lib()
    out = np.zeros((256, 4), np.uint32)
    L.sf_selftest_weight_records.argtypes = [C.c_int, C.c_void_p]
    _abi.check(L.sf_selftest_weight_records(0, out.ctypes.data_as(C.c_void_p)))
    w = np.arange(256, dtype=np.uint32)
    want = np.zeros((256, 4), np.uint32)
    want[:, 0] = w.astype(np.float32).view(np.uint32)
    want[:, 1] = (w + 1).astype(np.float32).view(np.uint32)
    want[:, 2] = (np.float32(1) / (w + 1).astype(np.float32)).view(np.uint32)
    want[:, 3] = (np.minimum(w + 1, 255) << 24) | np.where(w == 0, 0x00FFFFFF, 0).astype(np.uint32)
    bad = np.argwhere(out != want)
    assert len(bad) == 0, "weight %d word %d: device %08x, statement %08x" % (bad[0][0], bad[0][1], out[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pattern(k):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(5 * xx + 40 * k) % 256, (7 * yy + 90 * k + 1) % 256, (3 * xx + 2 * yy + 11 * k) % 256], -1).astype(np.uint8)


def _dwell():
    """One pose, a wall at 1.2 m whose depth ripples by a few millimetres from frame to frame (every mean is a different quotient).  Colour: frame 0 black,
    a 255-saturated patch in every seventh frame, a black patch that stays, a pattern that changes every frame."""
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([1200 + (3 * xx + 5 * yy + 7 * k) % 9 - 4 for k in range(N_DWELL)]).astype(np.uint16)
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(16), (N_DWELL, 1))
    rgb = np.stack([_pattern(k) for k in range(N_DWELL)])
    rgb[0] = 0
    rgb[3::7, 10:20, 12:30] = 255
    rgb[:, 30:40, 40:56] = 0
    return depth, poses, rgb


def _mixed():
    """The `tilted` scene of tests/test_gpu_integrate_cuts.py, 40 frames long: 11 mm sideways per frame over a plane tilted against the block grid."""
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([900 + 4 * xx + 3 * yy + 7 * k for k in range(N_MIXED)]).astype(np.uint16)
    poses = np.tile(np.eye(4, dtype=np.float32), (N_MIXED, 1, 1))
    for k in range(N_MIXED):
        poses[k, :3, 3] = (0.011 * k, -0.006 * k, 0.004 * k)
    return depth, poses.reshape(N_MIXED, 16), np.stack([_pattern(k) for k in range(N_MIXED)])


SCENES = {"dwell": _dwell, "mixed": _mixed}
_frames, _refs = {}, {}


def _scene(name):
    if name not in _frames:
        _frames[name] = SCENES[name]()
    return _frames[name]


def _weights_by_voxel(export):
    """{block coordinate: the 512 weights of the block}, as one sorted key array and the weights in its order."""
    coords, vox = export
    key = (coords[:, 0].astype(np.int64) << 42) + (coords[:, 1].astype(np.int64) << 21) + coords[:, 2].astype(np.int64)
    order = np.argsort(key)
    return key[order], vox["w"][order], vox[order]


def _reference(oracle, name, colour, snapshots=(), **over):
    """(last frame's block count, the oracle's export after the whole scene, {frames fused: export} for `snapshots`): made once per scene and parameter set,
    never changed by a test."""
    key = (name, colour, tuple(sorted(over.items())))
    if key not in _refs:
        depth, poses, rgb = _scene(name)
        op, _ = _mk(oracle, W, H, num_sdf_blocks=BLOCKS, **over)
        vol = oracle.Volume(op, threads=8)
        last, snaps = 0, {}
        for k in range(len(depth)):
            last = vol.integrate(depth[k], poses[k].reshape(4, 4), rgb=rgb[k] if colour else None)
            if k + 1 in snapshots:
                snaps[k + 1] = vol.export()
        _refs[key] = (last, vol.export(), snaps)
        vol.close()
    return _refs[key]


def _assert_export(ref, fuser):
    oc, ov = ref
    gc, gv = fuser.export_blocks()
    assert np.array_equal(oc, gc), "allocated block sets differ"
    same = ov.view(np.uint8).reshape(len(oc), 512, 8) == gv.view(np.uint8).reshape(len(gc), 512, 8)
    if not same.all():
        b, v = np.argwhere(~same.all(-1))[0]
        raise AssertionError("%d voxels differ; first: block %s voxel %d oracle %s gpu %s" % ((~same.all(-1)).sum(), oc[b], v, ov[b, v], gv[b, v]))


def _fuse_and_compare(oracle, name, colour, tune, ref, last, **over):
    from scannet_amd import fusion
    depth, poses, rgb = _scene(name)
    _, gp = _mk(oracle, W, H, num_sdf_blocks=BLOCKS, **over)
    dev = _DeviceFrames(depth, rgb if colour else None)
    try:
        with fusion.Fuser(gp, **tune) as f:
            dev.fuse(f, poses, 0, len(depth))
            st = f.stats()
            assert st["frames_integrated"] == len(depth) and st["alloc_failures"] == 0 and st["last_frame_blocks"] == last
            _assert_export(ref, f)
    finally:
        dev.close()


SCHEDULES = {"pass32": dict(batch=32, tail_wide=0), "pass32_wide": dict(batch=32, tail_wide=1), "pass4": dict(batch=4)}


def _dwell_reference(oracle, colour):
    """The dwell's reference, and that the scene holds what it is for -- counted on the oracle's exports."""
    last, ref, snaps = _reference(oracle, "dwell", colour, snapshots=(1, 254, 255, 256))
    assert ref[1]["w"].max() == 255
    # the steps 254 -> 255 (the last increment) -> 255 (the first saturated update): the same voxel after 254, 255 and 256 frames
    k254, w254, _ = _weights_by_voxel(snaps[254])
    k255, w255, _ = _weights_by_voxel(snaps[255])
    k256, w256, _ = _weights_by_voxel(snaps[256])
    assert np.array_equal(k254, k255) and np.array_equal(k255, k256), "the dwell allocates no block after frame 254"
    assert ((w254 == 254) & (w255 == 255) & (w256 == 255)).sum() >= 1000
    if colour:
        _, _, v1 = _weights_by_voxel(snaps[1])
        assert ((v1["w"] > 0) & (v1["r"] == 0) & (v1["g"] == 0) & (v1["b"] == 0)).sum() >= 100, "frame 0 leaves black voxels that have a weight"
    return last, ref


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_dwell_through_saturation(oracle, schedule, colour):
    last, ref = _dwell_reference(oracle, colour)
    _fuse_and_compare(oracle, "dwell", colour, SCHEDULES[schedule], ref, last)


def _mixed_reference(oracle, colour, **over):
    last, ref, _ = _reference(oracle, "mixed", colour, **over)
    if not over:
        w = np.sort(ref[1]["w"], axis=1)
        distinct = 1 + (w[:, 1:] != w[:, :-1]).sum(1)
        assert (distinct >= 8).sum() >= 200, "blocks whose voxels hold eight or more different weights"
    return last, ref


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_mixed_records_in_one_wave(oracle, schedule, colour):
    last, ref = _mixed_reference(oracle, colour)
    _fuse_and_compare(oracle, "mixed", colour, SCHEDULES[schedule], ref, last)


@pytest.mark.parametrize("over", [dict(colour_first=1), dict(weight_max=7, weight_sample=2)], ids=["colour_first", "weight_max7_sample2"])
def test_other_parameters_keep_their_kernels(oracle, over):
    """colour_first 1 ("first" by the colour bytes) and a generic weight limit: k_integrate variants that keep the float table."""
    last, ref = _mixed_reference(oracle, True, **over)
    _fuse_and_compare(oracle, "mixed", True, {}, ref, last, **over)


@pytest.mark.parametrize("colour", [True, False], ids=["rows_variant", "pipe"])
def test_one_frame_per_launch_keeps_its_kernels(oracle, colour):
    """batch 1: k_integrate with per-row write-back (colour) and k_integrate_pipe (geometry only)."""
    last, ref = _mixed_reference(oracle, colour)
    _fuse_and_compare(oracle, "mixed", colour, dict(batch=1), ref, last)
