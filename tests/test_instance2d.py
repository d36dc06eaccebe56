"""The 2-D instance task without a GPU: the host plan and the host overlaps against the brute-force checker
tests/instance2d_checker.c, count for count; the thresholds against numpy's, bit for bit; the AP against the section restated in numpy
(tests/instance2d_cases.py::ap_from_the_rule) and against curves worked by hand; the order of images and predictions; bin/evaluate instance2d
against what the reference's script said about the same files (tests/golden/instance2d_golden.json); the refusals; and the host code once under
AddressSanitizer / UBSan as a stand-alone program (tests/instance2d_host_main.cpp)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, evaluation as ev, filter2d
from tests import instance2d_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "evaluate")
SIZES = ((1, 1), (15, 1), (17, 3), (67, 45), (128, 96))   # width x height
NAN = float("nan")


@pytest.fixture(scope="module")
def checker():
    L = ic.build_checker()
    if L is None:
        pytest.skip("needs gcc")
    return L


def same_plan(got, plans):
    count, ids, px = got
    want = ic.plan_arrays(plans, ids.shape[1])
    return np.array_equal(count, want[0]) and np.array_equal(ids, want[1]) and np.array_equal(px, want[2])


# ---- the counts ----

@pytest.mark.parametrize("dtype", (np.uint8, np.uint16, np.uint32))
def test_host_plan_and_overlaps_equal_the_checker(checker, dtype):
    seen = 0
    for (w, h) in SIZES:
        for batch in (1, 3, 17):
            gt, masks, mask_image, _, _ = ic.image_batch(1000 + w + batch, batch, w, h, dtype, n_inst=6 if batch == 17 else 12, masks_per_image=2)
            plans = ic.check_plan(checker, gt)
            got = ev.image_plan(gt)
            assert same_plan(got, plans), (w, h, batch)
            seen += int(got[0].sum())
            capacity = got[1].shape[1]
            want = ic.check_table(checker, gt, plans, masks, mask_image, capacity)
            table = ev.overlaps_images(gt, got[0], got[1], masks, mask_image)
            assert table.dtype == np.uint32 and np.array_equal(table, want), (w, h, batch)
            roomy = ev.image_plan(gt, capacity=capacity + 3)                                   # a larger capacity: the same entries, the rest untouched
            assert same_plan(roomy, plans)
            assert np.array_equal(ev.overlaps_images(gt, roomy[0], roomy[1], masks, mask_image), ic.check_table(checker, gt, plans, masks, mask_image, capacity + 3))
    assert (seen > 100) == (dtype != np.uint8)   # bytes hold no instance id: images of void and of nothing


def test_images_of_no_instance_of_one_id_and_of_an_id_per_pixel(checker):
    none = np.zeros((2, 45, 67), np.uint16)
    none[0, 3:9] = 39
    none[1, :, 5] = 2999
    count, ids, px = ev.image_plan(none)
    assert count.tolist() == [0, 0] and ids.shape == (2, 0)
    masks = np.ones((2, 45 * 67), np.uint8)
    assert ev.overlaps_images(none, count, ids, masks, [0, 1]).tolist() == [[6 * 67, 45 * 67], [0, 45 * 67]]
    one = np.full((1, 96, 128), 7001, np.uint16)
    count, ids, px = ev.image_plan(one)
    assert count.tolist() == [1] and ids.tolist() == [[7001]] and px.tolist() == [[96 * 128]]
    half = np.zeros((1, 96 * 128), np.uint8)
    half[0, ::2] = 200
    assert ev.overlaps_images(one, count, ids, half, [0]).tolist() == [[96 * 64, 0, 96 * 64]]
    each = ic.distinct_ids_image(128, 96)
    plans = ic.check_plan(checker, each)
    got = ev.image_plan(each)
    assert got[0].tolist() == [128 * 96] and same_plan(got, plans) and (got[2] == 1).all()
    masks = np.zeros((2, 128 * 96), np.uint8)
    masks[0, 5::7] = 1
    masks[1, :100] = 255
    assert np.array_equal(ev.overlaps_images(each, got[0], got[1], masks, [0, 0]), ic.check_table(checker, each, plans, masks, [0, 0], 128 * 96))


def test_plan_capacity_too_small_writes_nothing():
    gt = np.zeros((2, 4, 8), np.uint16)
    gt[0, 0, :3] = (5001, 5002, 7001)
    gt[1, 0, 0] = 5001
    L = ev._lib()
    v = np.array(ev.INSTANCE_IDS, np.int32)
    count, ids, px = np.full(2, 77, np.uint32), np.full((2, 2), -7, np.int32), np.full((2, 2), 7, np.uint32)
    rc = L.sf_eval_image_plan(ev._ptr(gt), 2, 2, 8, 4, ev._ptr(v), len(v), 2, -1, ev._ptr(count), ev._ptr(ids), ev._ptr(px))
    assert rc == -7
    with pytest.raises(_abi.ScanfuseError) as e:
        _abi.check(rc)
    assert e.value.code == -7 and "image 0 holds 3" in str(e.value)
    assert (count == 77).all() and (ids == -7).all() and (px == 7).all()


def test_refused_arguments():
    gt = np.zeros((1, 4, 4), np.uint16)
    for bad in ((0, 5), (5, 1000), (5, 5), (-1,), ()):
        with pytest.raises((_abi.ScanfuseError, ValueError)) as e:
            ev.image_plan(gt, valid_ids=bad)
        assert not isinstance(e.value, _abi.ScanfuseError) or e.value.code == -1
    with pytest.raises(_abi.ScanfuseError):
        ev.InstanceAP2D(valid_ids=(1000,), names=("x",))
    count, ids, _ = ev.image_plan(gt)
    masks = np.zeros((1, 16), np.uint8)
    with pytest.raises(_abi.ScanfuseError) as e:
        ev.overlaps_images(gt, count, ids, masks, [1])                         # a mask over an image that is not there
    assert e.value.code == -1
    with pytest.raises(_abi.ScanfuseError):
        ev.overlaps_images(gt, np.array([2], np.uint32), np.array([[7001, 5001]], np.int32), masks, [0])   # ids that do not ascend
    with pytest.raises(_abi.ScanfuseError):
        ev.overlaps_images(gt, np.array([3], np.uint32), np.array([[5001, 7001]], np.int32), masks, [0])   # a count above the capacity


def test_no_silent_fallback_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    gt = np.zeros((1, 4, 4), np.uint16)
    for call in (lambda: ev.image_plan(gt, device=0), lambda: ev.overlaps_images(gt, [0], np.zeros((1, 0), np.int32), np.ones((1, 16), np.uint8), [0], device=0)):
        with pytest.raises(_abi.ScanfuseError) as e:
            call()
        assert e.value.code == -5


# ---- the AP ----

def test_thresholds_are_numpys_bit_for_bit():
    th = ev.ap2d_thresholds()
    want = np.arange(0.5, 1., 0.05)
    assert len(th) == 10 and th.tobytes() == want.tobytes()
    assert th[6:].tolist() == [0.8000000000000003, 0.8500000000000003, 0.9000000000000004, 0.9500000000000004] and 0.25 not in th


def score(images, **kw):
    with ev.InstanceAP2D(**kw) as acc:
        for im in images:
            acc.add(im.gt[None], im.masks, np.zeros(len(im.labels), np.uint32), im.labels, im.confs)
        return acc.finish()


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize("seed", (11, 12, 13))
def test_ap_equals_the_rule_restated_in_numpy(seed):
    gt, masks, mask_image, labels, confs = ic.image_batch(seed, 6, 128, 96, np.uint16, n_inst=10, masks_per_image=8)
    images = ic.images_of(gt, masks, mask_image, labels, confs)
    want = ic.ap_from_the_rule(images)
    with ev.InstanceAP2D() as acc:
        acc.add(gt, masks, mask_image, labels, confs)       # the whole batch in one call
        got = acc.finish()
    assert np.isfinite(want).sum() >= 30 and (want[np.isfinite(want)] > 0).any()
    assert np.array_equal(np.isnan(got["ap"]), np.isnan(want))
    # fewer than 200 terms in [0, 1] per dot product and mean: DESIGN.md section 4o's bound
    assert np.nanmax(np.abs(got["ap"] - want)) <= 1e-12
    cls, avg = ic.averages_from_the_rule(got["ap"])
    assert np.allclose([got["classes"][n]["ap"] for n in ev.INSTANCE_NAMES], cls[:, 0], rtol=0, atol=1e-12, equal_nan=True)
    assert same([got["classes"][n]["ap50%"] for n in ev.INSTANCE_NAMES], cls[:, 1])
    assert abs(got["all_ap"] - avg[0]) <= 1e-12 and abs(got["all_ap_50%"] - avg[1]) <= 1e-12
    assert same(score(images)["ap"], got["ap"])               # image by image: the same bits


def chair(rows):
    """A 40 x 40 image of one chair over rows [0, rows)."""
    gt = np.zeros((40, 40), np.uint16)
    gt[:rows] = 5001
    return gt


def rows_mask(a, b, cols=40):
    m = np.zeros((40, 40), np.uint8)
    m[a:b, :cols] = 1
    return m.reshape(-1)


def test_second_match_by_hand():
    # a chair of 1600 pixels, two predictions that exceed every threshold up to 0.9: 1600 / 1600 with 0.4 and 1560 / 1600 = 0.975 with 0.8.
    # The instance keeps 0.8 (true), 0.4 becomes a false positive.  Sorted scores (0.4: false, 0.8: true): precision 1/2, 1, then the artificial 1;
    # recall 1, 1, 0.  Step widths 0.5 * (a[j] - a[j + 2]) over a = [1, 1, 1, 0, 0]: 0, 0.5, 0.5.  AP = 0.5 * 0 + 1 * 0.5 + 1 * 0.5 = 1.
    im = ic.Image(chair(40), [rows_mask(0, 40), rows_mask(0, 39)], [5, 5], [0.4, 0.8])
    ap = score([im])["ap"][2]
    assert ap.tolist() == [1.0] * 10
    # the better-placed one carries the lower score: at 0.95 only it is left (0.975 against 0.9500000000000004), at 1600 / 1600 with 0.9 both stay
    im = ic.Image(chair(40), [rows_mask(0, 36), rows_mask(0, 39)], [5, 5], [0.9, 0.3])   # 0.9 and 0.975
    ap = score([im])["ap"][2]
    # up to 0.85: both match, true at 0.9 and a false positive at 0.3: precision [1/2, 1, 1], recall [1, 1, 0] -> 1.  At 0.9000000000000004 the first
    # (1440 / 1600 = 0.9) no longer exceeds it: it is an unmatched prediction (nothing to ignore: a false positive at 0.9), the instance is matched
    # by 0.3: scores (0.3: true, 0.9: false): precision [1/2, 0, 1], recall [1, 0, 0]; a = [1, 1, 0, 0, 0]: widths 0.5, 0.5, 0 -> 0.25.
    assert ap.tolist() == [1.0] * 8 + [0.25, 0.25]
    assert same(ic.ap_from_the_rule([im])[2], ap)


def test_small_instance_ignore_by_hand():
    gt = np.zeros((40, 40), np.uint16)
    gt[0] = gt[1] = 6001
    gt[2, :19] = 6001                                         # a sofa of 99 pixels
    gt[10:30] = 5001                                          # a chair of 800
    small = (gt == 6001).astype(np.uint8).reshape(-1)
    # the small sofa is no ground truth: the class has none (NaN), the prediction on it counts nowhere; the averages are the chair's
    got = score([ic.Image(gt, [small, rows_mask(10, 30)], [6, 5], [0.9, 0.5])])
    assert np.isnan(got["ap"][3]).all() and got["ap"][2].tolist() == [1.0] * 10 and got["all_ap"] == 1.0 and got["all_ap_50%"] == 1.0
    assert score([ic.Image(gt, [small, rows_mask(10, 30)], [6, 5], [0.9, 0.5])], min_region_size=99)["ap"][3].tolist() == [1.0] * 10
    # the small instance as a second chair, and a chair prediction of 40 pixels inside it (no minimum size for predictions): its overlap 40 / 99
    # exceeds no threshold, all of its pixels lie on a small instance, so it is ignored: the chairs stay at 1
    gt[gt == 6001] = 5002
    inside = rows_mask(0, 1)
    im = ic.Image(gt, [inside, rows_mask(10, 30)], [5, 5], [0.9, 0.5])
    assert score([im])["ap"][2].tolist() == [1.0] * 10
    # with 99 as the minimum the small chair is ground truth that nothing matches (one hard false negative) and the prediction a false positive:
    # scores (0.5: true, 0.9: false): precision [1/2, 0, 1], recall [1/2, 0, 0]; a = [1/2, 1/2, 0, 0, 0]: widths 1/4, 1/4, 0 -> 1/8
    assert score([im], min_region_size=99)["ap"][2].tolist() == [0.125] * 10
    assert same(ic.ap_from_the_rule([im], min_region=99)[2], [0.125] * 10)


def test_void_ignore_exactly_at_and_just_above_the_threshold_by_hand():
    # a chair matched exactly by a prediction of score 0.2, and a second chair prediction of 2000 pixels and score 0.9 that touches no instance:
    # k of its pixels lie on void (raw value 5), the rest on nothing.  k / 2000 <= threshold: a false positive above the match: scores (0.2: true,
    # 0.9: false): precision [1/2, 0, 1], recall [1, 0, 0]; a = [1, 1, 0, 0, 0]: widths 1/2, 1/2, 0 -> 1/4.  k / 2000 > threshold: ignored, the
    # match alone -> 1.  The thresholds 0.5 and 0.55 are the doubles nearest to 0.5 and 0.55, as are 1000 / 2000 and 1100 / 2000.
    gt = np.zeros((96, 128), np.uint16)
    gt[:20] = 5001
    gt[30:40] = 5                                             # 1280 void pixels
    good = (gt == 5001).astype(np.uint8).reshape(-1)
    for k, ignored_at in ((1000, 0), (1001, 1), (1100, 1), (1101, 2)):
        m = np.zeros(96 * 128, np.uint8)
        m[30 * 128:30 * 128 + k] = 255
        m[50 * 128:50 * 128 + 2000 - k] = 255
        im = ic.Image(gt, [good, m], [5, 5], [0.2, 0.9])
        assert score([im])["ap"][2].tolist() == [1.0] * ignored_at + [0.25] * (10 - ignored_at), k
        assert same(ic.ap_from_the_rule([im])[2], score([im])["ap"][2])


def test_order_of_images_and_predictions_does_not_matter():
    gt, masks, mask_image, labels, confs = ic.image_batch(21, 5, 67, 45, np.uint16, n_inst=8, masks_per_image=9)
    images = ic.images_of(gt, masks, mask_image, labels, confs)
    first = score(images)
    assert np.isfinite(first["ap"]).any()
    rng = np.random.default_rng(5)
    for _ in range(3):
        shuffled = []
        for b in rng.permutation(len(images)):
            im = images[b]
            order = rng.permutation(len(im.labels))
            shuffled.append(ic.Image(im.gt, im.masks[order], im.labels[order], im.confs[order]))
        again = score(shuffled)
        assert again["ap"].tobytes() == first["ap"].tobytes()
        assert np.float64(again["all_ap"]).tobytes() == np.float64(first["all_ap"]).tobytes()


def test_the_3d_accumulator_and_the_2d_one_share_their_curve():
    # a case on which the two rules coincide (every prediction of 100 pixels or more and inside instances of its class, no second visit): the nine
    # thresholds 0.5 .. 0.9 are the same doubles in both, and so must the APs be, through sf_eval_ap_finish and sf_eval_ap2d_finish
    gt = np.zeros((40, 40), np.uint16)
    gt[:20] = 5001
    gt[20:] = 5002
    masks = [rows_mask(0, 20), rows_mask(2, 20), rows_mask(20, 34), rows_mask(20, 40, 30)]   # 1, 0.9 on the first; 0.7 and 0.75 on the second
    labels, confs = [5, 5, 5, 5], [0.9, 0.3, 0.6, 0.6]
    two = score([ic.Image(gt, masks, labels, confs)])["ap"]
    with ev.InstanceAP() as acc:
        acc.add(gt.reshape(-1).astype(np.int32), np.stack(masks), labels, confs)
        three = acc.finish()["ap"]
    assert same(two[:, :9], three[:, :9]) and 0 < two[2, 5] < 1 and len(set(two[2].tolist())) >= 2   # the curve is no constant


# ---- the files ----

def _tool(*args):
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "instance2d_golden.json")))


def test_files_against_the_reference(tmp_path, golden):
    pred_path, gt_path, sha = ic.write_file_case(str(tmp_path))
    assert sha == golden["inputs_sha256"]
    rc, out, err = _tool("instance2d", "--pred_path", pred_path, "--gt_path", gt_path, "--host")
    assert rc == 0 and err == "", err
    assert out == "\n" + "\n".join(golden["table"]) + "\n\n"                                     # printResults, line for line
    lines = open(os.path.join(pred_path, "semantic_instance.txt")).read().splitlines()
    assert lines[0].split(",") == golden["header"] and len(lines) == 19
    worst = 0.0
    for line, want in zip(lines[1:], golden["rows"]):
        name, cid, ap, ap50 = line.split(",")
        assert (name, int(cid)) == (want[0], want[1])
        for got, ref in ((float(ap), want[2]), (float(ap50), want[3])):
            assert np.isnan(got) == (ref is None)
            if ref is not None:
                worst = max(worst, abs(got - ref))
    assert worst <= 1e-12, worst
    # the second run leaves the result file of the first out, and writes the same bytes; so does the library call
    first = open(os.path.join(pred_path, "semantic_instance.txt"), "rb").read()
    rc, out2, err = _tool("instance2d", "--pred_path", pred_path, "--gt_path", gt_path)
    assert rc == 0 and out2 == out and open(os.path.join(pred_path, "semantic_instance.txt"), "rb").read() == first
    os.remove(os.path.join(pred_path, "semantic_instance.txt"))
    other = str(tmp_path / "elsewhere.txt")
    assert ev.evaluate_instance2d_dir(pred_path, gt_path, other) == out and open(other, "rb").read() == first
    assert not os.path.exists(os.path.join(pred_path, "semantic_instance.txt"))
    # and the rule restated in numpy says the same about these images
    cls, _ = ic.averages_from_the_rule(ic.ap_from_the_rule(ic.file_case_images()))
    for want, row in zip(golden["rows"], cls):
        assert (want[2] is None) == np.isnan(row[0]) and (want[2] is None or abs(want[2] - row[0]) <= 1e-12)


def test_refusals_name_their_file(tmp_path):
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    (pred / "masks").mkdir(parents=True)
    (pred / "sub").mkdir()
    gt.mkdir()
    img = np.zeros((12, 20), np.uint16)
    img[2:10, 2:18] = 5001
    mask = (img != 0).astype(np.uint8)
    filter2d.png_write_gray(str(gt / "a.png"), img)
    filter2d.png_write_gray(str(pred / "masks" / "m.png"), mask)
    run = lambda: _tool("instance2d", "--pred_path", pred, "--gt_path", gt, "--host")   # noqa: E731

    def refused(text, *needles, code=2):
        (pred / "a.txt").write_text(text)
        rc, out, err = run()
        assert rc == code and out == "" and err.startswith("ERROR: ") and err.count("\n") == 1, (text, err)
        for n in needles:
            assert n in err, (n, err)
    rc, out, err = _tool("instance2d", "--pred_path", pred, "--gt_path", gt)
    assert rc == 2 and "No result files found" in err
    (pred / "a.txt").write_text("masks/m.png 5 0.5\n")
    rc, out, err = run()
    assert rc == 0 and "chair          :          1.000          1.000" in out
    refused("masks/m.png 5\n", "a.txt", "Expected content")
    refused("masks/m.png  5 0.5\n", "a.txt", "Expected content")                        # two blanks: four fields
    refused("masks/m.png 5 0.5\n\n", "a.txt", "Expected content")                       # an empty line
    refused("/masks/m.png 5 0.5\n", "a.txt", "relative path")
    refused("../gt/a.png 5 0.5\n", "a.txt", "outside of prediction path")
    refused("masks/../../pred_other/m.png 5 0.5\n", "a.txt", "outside of prediction path")
    refused("masks/m.png 5 nan\n", "a.txt", "numbers")
    refused("masks/m.png inf 0.5\n", "a.txt", "numbers")
    refused("masks/m.png 5 0_5\n", "a.txt", "numbers")
    refused("masks/m.png 5 0x1p-1\n", "a.txt", "numbers")
    refused("masks/gone.png 5 0.5\n", "gone.png")
    filter2d.png_write_gray(str(pred / "masks" / "small.png"), mask[:, :19].copy())
    refused("masks/small.png 5 0.5\n", "small.png", "19 x 12", "a.png")
    filter2d.png_write_gray(str(pred / "masks" / "deep.png"), mask.astype(np.uint16))
    refused("masks/deep.png 5 0.5\n", "deep.png", "16 bits")
    (pred / "masks" / "cut.png").write_bytes((pred / "masks" / "m.png").read_bytes()[:60])
    refused("masks/cut.png 5 0.5\n", "cut.png")
    (pred / "a.txt").write_text("masks/cut.png 13 0.5\nmasks/m.png 5 1\n")               # a dropped label: its mask is never opened
    assert run()[0] == 0
    (pred / "sub" / "a.txt").write_text("../masks/m.png 5 0.5\n")                        # two lists for a.png
    rc, out, err = run()
    assert rc == 2 and "sub/a.txt" in err and "share" in err
    (pred / "sub" / "a.txt").unlink()
    (pred / "b.txt").write_text("masks/m.png 5 0.5\n")
    rc, out, err = run()
    assert rc == 2 and "b.txt" in err and "does not match any gt file" in err
    rgb = np.zeros((12, 20, 3), np.uint8)
    try:
        from PIL import Image
    except ImportError:
        return
    Image.fromarray(rgb).save(str(gt / "b.png"))
    rc, out, err = run()
    assert rc == 2 and "b.png" in err and "channels" in err


def test_host_code_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "instance2d_host")
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "instance2d_host_main.cpp")] + \
          [os.path.join(ROOT, "scannet_amd", "csrc", f) for f in ("evaluation.cpp", "instance2d.cpp", "instance2d_files.cpp", "png.cpp", "zlib_codec.cpp")] + ["-lpthread"]
    subprocess.run(cmd, check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.strip() == "instance2d host: ok"
