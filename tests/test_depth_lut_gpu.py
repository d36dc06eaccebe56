"""The depth-distortion table's kernels (scannet_amd/csrc/depth_lut.hip) on the GPU: k_lut_accumulate / k_lut_finish /
k_lut_apply against the CPU checker and the host path, bit for bit, over the shapes at which the kernels take another path."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, depth_lut, filter2d
from tests import depth_lut_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "calibrate_depth")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not dc.have_checker(), reason="no gcc for the checker")]


def run(seq, device, split=None):
    with depth_lut.Estimator(seq["W"], seq["H"], seq["K"], seq["n_slices"], seq["max_depth"], seq["bitshift"], device=device) as e:
        a = 0
        for n in (split or [len(seq["depths"])]):
            e.add(seq["depths"][a:a + n], seq["poses"][a:a + n])
            a += n
        assert a == len(seq["depths"])
        acc, div, n, used = e.sums()
        table, _ = e.finish()
    return acc, div, table, n, used


def same(a, b):
    return all(np.array_equal(dc.bits(x), dc.bits(y)) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("bitshift", [True, False])
def test_small_case_is_the_checker_and_the_host_path(bitshift):
    seq = dc.sequence("small", bitshift)
    want = dc.checker_case("small", bitshift)
    dev, host = run(seq, 0), run(seq, -1)
    assert dev[3:] == (9, 8) and host[3:] == (9, 8)
    assert same(dev, want) and same(host, want)
    assert (want[1] != 0).sum() > 200
    gold = json.load(open(dc.GOLDEN))["small/" + ("shift" if bitshift else "noshift")]
    assert dict(acc=dc.digest(dev[0]), div=dc.digest(dev[1]), table=dc.digest(dev[2])) == gold


def test_batch_boundaries_do_not_change_the_bits():
    B = depth_lut.max_batch()
    seq = dc.repeat(dc.sequence("small"), 2 * B + 1)
    want = dc.checker_run(seq)
    for split in (None, [1] * (2 * B + 1), [B, B + 1]):
        assert same(run(seq, 0, split), want), split


@pytest.mark.parametrize("name", ["small_50x38", "small_10x2"])
def test_shapes_off_the_workgroup_tile(name):
    seq = dc.sequence(name)
    want = dc.checker_case(name)
    assert same(run(seq, 0), want)
    if name == "small_10x2":        # the stripe takes 4 of the 5 columns
        t = want[2]
        assert t.shape == (5, 1, 5) and all(np.array_equal(dc.bits(t[:, :, x]), dc.bits(t[:, :, 0])) for x in range(1, 5))


@pytest.mark.parametrize("ns", [1, 2, 32, 33, 64, 65, 128])     # 32 | 33 and 64 | 65: the workgroup size changes; 128: the largest the LDS budget allows
def test_slice_counts(ns):
    name = "small_s%d" % ns
    seq = dc.sequence(name)
    want = dc.checker_case(name)
    got = run(seq, 0)
    assert same(got, want)
    if ns == 1:
        assert (got[2] == 1.0).all() and not got[1].any()
    if ns >= 32:
        assert (want[1] != 0).any(axis=(1, 2)).sum() >= 10          # many slices take samples


def test_too_many_slices_is_refused_before_any_launch():
    K = dc.intrinsics(48, 36)
    L = depth_lut._lib()
    h = C.c_void_p()
    rc = L.sf_lut_estimator_create(48, 36, float(K[0]), float(K[1]), float(K[2]), float(K[3]), 129, 5.0, 1, 0, C.byref(h))
    assert rc == -9 and not h.value and b"LDS" in L.sf_last_error()


def test_real_shape_once():
    seq = dc.sequence("real")
    want = dc.checker_case("real")
    got = run(seq, 0)
    assert got[3:] == (3, 3) and same(got, want)
    gold = json.load(open(dc.GOLDEN))["real/shift"]
    assert dict(acc=dc.digest(got[0]), div=dc.digest(got[1]), table=dc.digest(got[2])) == gold


def test_device_images_and_kernel_time():
    """sf_lut_estimator_add_device on images that live on the device, with the launches timed."""
    seq = dc.sequence("small")
    want = dc.checker_case("small")
    L = depth_lut._lib()
    n, px = len(seq["depths"]), seq["W"] * seq["H"]
    d = C.c_void_p()
    _abi.check(L.sf_device_malloc(0, n * px * 2, C.byref(d)))
    try:
        _abi.check(L.sf_device_upload(d, seq["depths"].ctypes.data, n * px * 2))
        with depth_lut.Estimator(seq["W"], seq["H"], seq["K"], seq["n_slices"], seq["max_depth"], True, device=0) as e:
            ptr = (C.c_void_p * n)(*[d.value + k * px * 2 for k in range(n)])
            us = C.c_float(-1.0)
            poses = np.ascontiguousarray(seq["poses"], np.float32)
            _abi.check(L.sf_lut_estimator_add_device(e._h, n, ptr, poses.ctypes.data, C.byref(us)))
            assert us.value > 0
            odd = (C.c_void_p * 1)(d.value + 2)
            assert L.sf_lut_estimator_add_device(e._h, 1, odd, poses.ctypes.data, None) == -1      # not 4-byte aligned: refused, not launched
            got = e.sums()[:2] + (e.finish()[0],)
        assert same(got, want)
    finally:
        L.sf_device_free(d)


@pytest.mark.parametrize("bitshift", [True, False])
def test_apply_is_the_checker_and_the_host_path(bitshift):
    seq = dc.sequence("small", bitshift)
    table = dc.checker_case("small", bitshift)[2]
    want = dc.checker_apply((table, 5.0), seq["depths"], bitshift)
    assert np.array_equal(depth_lut.apply((table, 5.0), seq["depths"], bitshift, device=0), want)
    assert np.array_equal(depth_lut.apply((table, 5.0), seq["depths"], bitshift, device=-1), want)
    assert not np.array_equal(want, seq["depths"])
    # a 24 x 18 table on 50 x 38 images: the resolution does not divide the image
    big = dc.sequence("small_50x38", bitshift)["depths"]
    want = dc.checker_apply((table, 5.0), big, bitshift)
    assert np.array_equal(depth_lut.apply((table, 5.0), big, bitshift, device=0), want)
    assert np.array_equal(depth_lut.apply((table, 5.0), big, bitshift, device=-1), want)


def test_apply_clamps_past_65535():
    table = np.full((5, 18, 24), 0.01, np.float32)           # a multiplier of 100
    table[0] = 1.0
    d = np.zeros((1, 36, 48), np.uint16)
    d[0, :, :24] = 4000
    d[0, :, 24:] = 500
    want = dc.checker_apply((table, 5.0), d, False)
    got = depth_lut.apply((table, 5.0), d, False, device=0)
    assert np.array_equal(got, want) and np.array_equal(depth_lut.apply((table, 5.0), d, False, device=-1), want)
    assert (got[0, :, :24] == 65535).all() and (got[0, :, 24:] < 65535).all()


def test_tool_on_the_device_and_on_the_host_write_the_same_bytes(tmp_path):
    seq = dc.sequence("small")
    out = {}
    for mode in ("--device=0", "--host"):
        root = str(tmp_path / mode.strip("-").replace("=", ""))
        conf = dc.write_sequence(root, seq, filter2d.png_write_gray)
        lut = os.path.join(root, "out.lut")
        r = subprocess.run([TOOL, conf, "-e", lut, "-a", lut, "-s", "5", "-l", "--root=" + root, mode], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        names = ["out.lut"] + ["depth/frame-%04d.png" % k for k in range(9)] + ["slice_%03d.png" % z for z in range(5)]
        out[mode] = [open(os.path.join(root, n), "rb").read() for n in names]
    assert out["--device=0"] == out["--host"]
    want = os.path.join(str(tmp_path), "want.lut")
    depth_lut.save_lut(want, (dc.checker_run(dict(seq, poses=depth_lut.load_config(conf, root=root)["plane_poses"]))[2], 5.0))
    assert out["--host"][0] == open(want, "rb").read()
