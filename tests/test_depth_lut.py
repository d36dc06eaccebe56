"""The depth-distortion table without a GPU: the checker against a float64 evaluation of the rule, the host path against the
checker bit for bit, known answers, the round trip estimate -> apply, the files, the tool with --host, and what the compiler gave the kernels."""
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, calibrate, depth_lut, filter2d
from tests import depth_lut_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "calibrate_depth")
HOST = -1

pytestmark = pytest.mark.skipif(not dc.have_checker(), reason="no gcc for the checker")


def host_run(seq, split=None):
    with depth_lut.Estimator(seq["W"], seq["H"], seq["K"], seq["n_slices"], seq["max_depth"], seq["bitshift"], device=HOST) as e:
        if split is None:
            e.add(seq["depths"], seq["poses"])
        else:
            a = 0
            for n in split:
                e.add(seq["depths"][a:a + n], seq["poses"][a:a + n])
                a += n
            assert a == len(seq["depths"])
        acc, div, n, used = e.sums()
        table, md = e.finish()
    assert md == seq["max_depth"]
    return acc, div, table, n, used


# ---- the checker against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "roundtrip"])
def test_checker_agrees_with_the_rule_in_float64(name):
    seq = dc.sequence(name)
    acc, div, _ = dc.checker_case(name)
    m64, cnt = dc.rule_float64(seq)
    known = div != 0
    assert np.array_equal(known, ~np.isnan(m64)), "the sets of unknown cells differ"
    assert known.sum() > 100
    m32 = (acc[known] / div[known]).astype(np.float64)
    rel = np.abs(m32 - m64[known]) / np.abs(m64[known])
    bound = (cnt[known] + 8) * 2.0 ** -23      # sequential binary32 sums of k terms plus the few operations per term
    print("worst relative error / bound: %.3g" % (rel / bound).max())
    assert (rel <= bound).all()


# ---- the host path against the checker -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bitshift", [True, False])
def test_host_path_is_the_checker_bit_for_bit(bitshift):
    seq = dc.sequence("small", bitshift)
    acc, div, table = dc.checker_case("small", bitshift)
    hacc, hdiv, htable, n, used = host_run(seq)
    assert (n, used) == (9, 8)                       # the 30-degree image is skipped
    assert np.array_equal(dc.bits(hacc), dc.bits(acc)) and np.array_equal(dc.bits(hdiv), dc.bits(div))
    assert np.array_equal(dc.bits(htable), dc.bits(table))
    assert (div != 0).sum() > 200
    out = depth_lut.apply((htable, 5.0), seq["depths"], bitshift, device=HOST)
    assert np.array_equal(out, dc.checker_apply((table, 5.0), seq["depths"], bitshift))
    assert not np.array_equal(out, seq["depths"])


def test_host_path_threads_and_calls_do_not_change_the_bits():
    seq = dc.repeat(dc.sequence("roundtrip"), 150)   # enough work for the threaded rows
    acc, div, table = dc.checker_run(seq)
    for split in (None, [1] * 150, [64, 86]):
        hacc, hdiv, htable, _, _ = host_run(seq, split)
        assert np.array_equal(dc.bits(hacc), dc.bits(acc)) and np.array_equal(dc.bits(hdiv), dc.bits(div)) and np.array_equal(dc.bits(htable), dc.bits(table))


def test_golden_digests():
    gold = json.load(open(dc.GOLDEN))
    for name, want in gold.items():
        case, _, shift = name.partition("/")
        acc, div, table = dc.checker_case(case, shift != "noshift")
        got = dict(acc=dc.digest(acc), div=dc.digest(div), table=dc.digest(table))
        assert got == want, name
        seq = dc.sequence(case, shift != "noshift")
        hacc, hdiv, htable, _, _ = host_run(seq)
        assert dict(acc=dc.digest(hacc), div=dc.digest(hdiv), table=dc.digest(htable)) == want, name
    assert {"small/shift", "small/noshift", "roundtrip/shift"} <= set(gold)


def test_filter_is_the_checkers():
    for tilt, about in [(0, "y"), (10, "x"), (24.9, "y"), (25.1, "y"), (30, "x"), (-40, "y"), (89, "x")]:
        T = dc.plane_pose(2.0, tilt, about)
        seq = dict(dc.sequence("small"))
        seq["depths"], seq["poses"] = seq["depths"][:1], T[None]
        _, _, _, n, used = host_run(seq)
        assert (n, used) == (1, int(dc.checker_filter(T))), tilt
        assert dc.checker_filter(T) == (abs(tilt) < 25.0), tilt


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------
def _exact_sequence(extra=()):
    W, H = 48, 36
    K = dc.intrinsics(W, H)
    poses = [dc.plane_pose(d) for d in (1.25, 2.5, 3.75, 5.5)]      # millimetres that a fronto-parallel plane gives exactly
    depths = [np.full((H, W), dc.shift_in(np.uint16(1000 * d)) if d < 8 else 0, np.uint16) for d in (1.25, 2.5, 3.75, 5.5)]
    for T, img in extra:
        poses.append(T)
        depths.append(img)
    return dict(W=W, H=H, K=K, n_slices=5, max_depth=5.0, bitshift=True, depths=np.stack(depths), poses=np.stack(poses).astype(np.float32))


def test_fronto_parallel_plane_gives_one():
    seq = _exact_sequence()
    acc, div, table, _, used = host_run(seq)
    assert used == 4
    has = div != 0
    assert has[1].all() and has[2].all() and has[3].all() and not has[0].any() and not has[4].any()   # 5.5 m is beyond the table, slice 0 takes nothing
    ulp = np.abs(dc.bits(table[1:4]).astype(np.int64) - int(np.float32(1.0).view(np.uint32)))
    assert ulp.max() <= 2
    assert (table[0] == 1.0).all() and (table[4] == 1.0).all()
    # a tilted image, and an all-zero one, change nothing
    W, H, K = seq["W"], seq["H"], seq["K"]
    T30 = dc.plane_pose(2.0, 30.0)
    more = _exact_sequence([(T30, dc.observe(T30, W, H, K)), (dc.plane_pose(2.0), np.zeros((H, W), np.uint16))])
    acc2, div2, table2, n2, used2 = host_run(more)
    assert (n2, used2) == (6, 5)
    assert np.array_equal(dc.bits(acc2), dc.bits(acc)) and np.array_equal(dc.bits(div2), dc.bits(div)) and np.array_equal(dc.bits(table2), dc.bits(table))


def test_stripe_copies_column_xres_minus_5():
    seq = dc.sequence("small")
    acc, div, table = dc.checker_case("small")
    _, _, htable, _, _ = host_run(seq)
    xres = table.shape[2]
    with np.errstate(all="ignore"):
        m = np.where(div != 0, acc / div, np.float32(1.0))
    for x in range(xres - 4, xres):
        assert np.array_equal(dc.bits(htable[:, :, x]), dc.bits(m[:, :, xres - 5]))
    assert not np.array_equal(m[:, :, xres - 4:], htable[:, :, xres - 4:])       # the stripe is not what the data alone would give
    # a cell that is unknown at xres - 5 makes its stripe 1.0, whatever the stripe's own data
    holes = dict(seq)
    d = seq["depths"].copy()
    d[:, 6:8, 2 * (xres - 5):2 * (xres - 5) + 2] = 0
    holes["depths"] = d
    hacc, hdiv, t2, _, _ = host_run(holes)
    assert (hdiv[:, 3, xres - 5] == 0).all() and (hdiv[1:, 3, xres - 4:] != 0).any()
    assert (t2[:, 3, xres - 5:] == 1.0).all()


def test_reciprocal_forms_agree():
    """1.0f / s against (float)(1.0 / (double)s) on 10^6 hashed s, powers of two and their neighbours among them."""
    i = np.arange(1_000_000, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)
    u = (h & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    u = u[(u >> 23) != 255]                                             # finite
    s = u.view(np.float32)
    pw = (np.arange(1, 254, dtype=np.uint32) << 23)
    edge = np.concatenate([pw, pw + 1, pw - 1, pw + 2, pw - 2]).view(np.float32)
    s = np.ascontiguousarray(np.concatenate([s, edge, np.float32([1e-3, 0.01, 0.45, 4.3, 7.0])]))
    s = s[s > 0]
    assert len(s) >= 1_000_000 - 10_000
    assert dc.checker().dl_recip_differ(s.ctypes.data, len(s)) == 0
    with np.errstate(all="ignore"):
        assert np.array_equal(dc.bits(np.float32(1.0) / s), dc.bits((1.0 / s.astype(np.float64)).astype(np.float32)))


# ---- round trip ------------------------------------------------------------------------------------------------------------------------------
def test_round_trip_restores_the_truth_within_3_mm():
    seq = dc.sequence("roundtrip")
    acc, div, table = dc.checker_case("roundtrip")
    assert (div[1:14] != 0).all(), "a cell of slices 1..13 is unknown: the case does not meet its own condition"
    lut = depth_lut.estimate(seq["depths"], seq["poses"], seq["K"], 15, 5.0, True, device=HOST)
    assert np.array_equal(dc.bits(lut[0]), dc.bits(table))
    out = dc.shift_out(depth_lut.apply(lut, seq["depths"], True, device=HOST)).astype(np.float64)
    obs = dc.shift_out(seq["depths"])
    depth32 = obs.astype(np.float32) * np.float32(0.001)
    zi = np.minimum(depth32 * (np.float32(15) / np.float32(5.0)), np.float32(14.0))
    inside = (zi >= 1) & (zi < 13) & (obs > 0)
    truth = np.stack([1000.0 * dc.true_depth(T, seq["W"], seq["H"], seq["K"]) for T in seq["poses"]])
    err = np.abs(out - truth)[inside]
    print("pixels %d, worst %.3f mm" % (inside.sum(), err.max()))
    assert inside.sum() > 0.5 * obs.size
    assert err.max() <= 3.0
    assert np.abs(obs.astype(np.float64) - truth)[inside].max() > 10.0      # the observation itself was 3 % off


# ---- files -----------------------------------------------------------------------------------------------------------------------------------
def test_files_parse_and_convert(tmp_path):
    seq = dc.sequence("small")
    conf = dc.write_sequence(str(tmp_path), seq, filter2d.png_write_gray)
    c = depth_lut.load_config(conf, root=str(tmp_path))
    assert c["n_images"] == 9 and c["image_names"] == ["frame-%04d.png" % k for k in range(9)]
    assert c["K"] == tuple(float(v) for v in seq["K"])
    assert np.array_equal(c["depth_to_color"], dc.D2C.astype(np.float32))
    F = np.diag([1.0, -1.0, -1.0, 1.0])
    raw = np.loadtxt(str(tmp_path / "plane_poses.txt")).reshape(-1, 4, 4)
    want = np.linalg.inv(F @ dc.D2C.astype(np.float32).astype(np.float64) @ F) @ raw.astype(np.float32).astype(np.float64)
    assert np.abs(c["plane_poses"] - want).max() <= 1e-6
    assert np.abs(c["plane_poses"] - seq["poses"]).max() <= 1e-5
    # relative to the current directory, as the reference reads them
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        assert depth_lut.load_config("calib.conf")["n_images"] == 9
    finally:
        os.chdir(cwd)


def _rc(fn):
    try:
        fn()
    except _abi.ScanfuseError as e:
        return e.code
    return 0


def test_bad_files_return_error_codes(tmp_path):
    seq = dc.sequence("small")
    root = str(tmp_path)
    conf = dc.write_sequence(root, seq, filter2d.png_write_gray)
    good = open(conf).read()
    lut = os.path.join(root, "o.lut")
    run = lambda: depth_lut.calibrate_depth(conf, estimate_path=lut, n_slices=5, root=root, device=HOST)
    assert _rc(run) == 0
    lines = good.splitlines()
    # plane_poses before n_images
    open(conf, "w").write("\n".join([lines[1], lines[3], lines[2]] + lines[4:]) + "\n")
    assert _rc(run) == -3
    # a missing parameters file, a missing configuration
    open(conf, "w").write(good.replace("parameters.txt", "nothing.txt"))
    assert _rc(run) == -2
    assert _rc(lambda: depth_lut.load_config(os.path.join(root, "none.conf"))) == -2
    # n_images larger than the scan lines
    open(conf, "w").write(good.replace("n_images 9", "n_images 10"))
    assert _rc(run) == -3
    # a truncated poses file
    open(conf, "w").write(good)
    poses = open(os.path.join(root, "plane_poses.txt")).read()
    open(os.path.join(root, "plane_poses.txt"), "w").write(poses[:len(poses) // 2])
    assert _rc(run) == -3
    open(os.path.join(root, "plane_poses.txt"), "w").write(poses)
    assert _rc(run) == 0
    # mixed image sizes, odd image sizes, a missing image, a truncated image, an 8-bit image
    name = os.path.join(root, "depth_raw", "frame-0003.png")
    keep = open(name, "rb").read()
    filter2d.png_write_gray(name, np.zeros((36, 50), np.uint16))
    assert _rc(run) == -3
    for k in range(9):
        filter2d.png_write_gray(os.path.join(root, "depth_raw", "frame-%04d.png" % k), np.zeros((35, 47), np.uint16))
    assert _rc(run) == -1
    for k in range(9):
        filter2d.png_write_gray(os.path.join(root, "depth_raw", "frame-%04d.png" % k), seq["depths"][k])
    open(name, "wb").write(keep[:len(keep) // 2])
    assert _rc(run) < 0
    filter2d.png_write_gray(name, np.zeros((36, 48), np.uint8))
    assert _rc(run) == -3
    os.remove(name)
    assert _rc(run) == -2
    # neither -e nor -a; a truncated table
    assert _rc(lambda: depth_lut.calibrate_depth(conf, root=root, device=HOST)) == -1
    open(name, "wb").write(keep)
    assert _rc(run) == 0
    blob = open(lut, "rb").read()
    open(lut, "wb").write(blob[:100])
    assert _rc(lambda: depth_lut.calibrate_depth(conf, apply_path=lut, root=root, device=HOST)) == -3


def test_estimator_refuses_bad_parameters():
    K = dc.intrinsics(48, 36)
    mk = lambda *a, **k: (lambda: depth_lut.Estimator(*a, device=HOST, **k).close())
    assert _rc(mk(48, 36, K)) == 0
    assert _rc(mk(47, 36, K)) == -1 and _rc(mk(48, 35, K)) == -1 and _rc(mk(8, 36, K)) == -1
    assert _rc(mk(10, 2, K)) == 0
    assert _rc(mk(48, 36, K, n_slices=0)) == -1 and _rc(mk(48, 36, K, max_depth=0.0)) == -1
    assert _rc(mk(48, 36, K, n_slices=128)) == 0
    assert _rc(mk(48, 36, K, n_slices=129)) == -9          # SF_ERR_PARAM: the bound of the kernel's LDS holds on both paths
    assert _rc(mk(48, 36, (0.0, 1.0, 1.0, 1.0))) == -1
    t = (np.ones((2, 40, 60), np.float32), 5.0)
    assert _rc(lambda: depth_lut.apply(t, np.zeros((1, 36, 48), np.uint16), device=HOST)) == -1   # finer than the image


# ---- the .lut file -----------------------------------------------------------------------------------------------------------------------------
def test_lut_file_round_trips(tmp_path):
    _, _, table = dc.checker_case("small")
    a, b, c = str(tmp_path / "a.lut"), str(tmp_path / "b.lut"), str(tmp_path / "c.lut")
    depth_lut.save_lut(a, (table, 5.0))
    calibrate.write_lut(b, table, 5.0)
    assert open(a, "rb").read() == open(b, "rb").read()
    back = depth_lut.load_lut(a)
    assert back[1] == 5.0 and np.array_equal(dc.bits(back[0]), dc.bits(table))
    depth_lut.save_lut(c, back)
    assert open(c, "rb").read() == open(a, "rb").read()


# ---- the tool ----------------------------------------------------------------------------------------------------------------------------------
def test_tool_host(tmp_path):
    seq = dict(dc.sequence("small"))
    seq["depths"], seq["poses"] = seq["depths"][[0, 1, 2, 3, 5, 6]], seq["poses"][[0, 1, 2, 3, 5, 6]]      # 6 images, the tilted one among them
    root = str(tmp_path)
    conf = dc.write_sequence(root, seq, filter2d.png_write_gray)
    lut = os.path.join(root, "out.lut")
    r = subprocess.run([TOOL, conf, "-e", lut, "-a", lut, "-s", "5", "-d", "5", "-v", "-l", "--root=" + root, "--host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    c = depth_lut.load_config(conf, root=root)
    want = depth_lut.estimate(seq["depths"], c["plane_poses"], c["K"], 5, 5.0, True, device=HOST)
    ref = os.path.join(root, "want.lut")
    depth_lut.save_lut(ref, want)
    assert open(lut, "rb").read() == open(ref, "rb").read()
    fixed = depth_lut.apply(want, seq["depths"], True, device=HOST)
    for k in range(6):
        assert np.array_equal(filter2d.png_read(os.path.join(root, "depth", "frame-%04d.png" % k)), fixed[k])
    # -v: the bin table (z_bin = 1: bins of a metre) and the skipped image; -l: one picture per slice
    assert "Depth Bins:" in r.stdout and "\tBin   0 (0.000 - 1.000) :   1" in r.stdout and "\tBin   1 (1.000 - 2.000) :   2" in r.stdout
    assert "Will use 5/6 images for calibration" in r.stdout and "Skipped images: \n\t frame-0004.png" in r.stdout
    for z in range(5):
        img = filter2d.png_read(os.path.join(root, "slice_%03d.png" % z))
        assert img.shape == (18, 24, 3) and img.dtype == np.uint8
    # without -e or -a: the usage, non-zero
    r = subprocess.run([TOOL, conf, "--host"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "usage" in r.stderr
    r = subprocess.run([TOOL, os.path.join(root, "none.conf"), "-e", lut, "--host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "configuration" in r.stderr


# ---- the kernels in the shipped code object --------------------------------------------------------------------------------------------------------
def test_kernels_use_no_private_memory():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernels(os.path.join(ROOT, "scannet_amd", "libscanfuse.so"))
    names = [kr.short(n) for n in kr.demangle([r["name"] for r in rows])]
    mine = [(n, r) for n, r in zip(names, rows) if n.split("<")[0] in ("k_lut_accumulate", "k_lut_finish", "k_lut_apply")]
    assert {n for n, _ in mine} == {"k_lut_accumulate<256>", "k_lut_accumulate<128>", "k_lut_accumulate<64>", "k_lut_finish", "k_lut_apply"}
    for n, r in mine:
        assert r["scratch"] == 0 and r["vspill"] == 0, n
        assert r["lds"] <= 160 * 1024, n                       # static; the accumulate kernel's dynamic LDS is bounded below
    # the dynamic LDS of k_lut_accumulate at the largest n_slices each workgroup size serves: 64 KiB, so two workgroups share a CU's 160 KiB
    for block, ns in ((256, 32), (128, 64), (64, 128)):
        assert block * 2 * 4 * ns <= 64 * 1024 <= 160 * 1024 // 2
