"""The benchmark's scores without a GPU: the host path of scannet_amd/csrc/evaluation.cpp against the brute-force checker
tests/evaluation_checker.c, count for count; the AP against the section restated in numpy (tests/evaluation_cases.py::ap_from_the_rule) within
1e-12 -- fewer than 200 terms in [0, 1] summed in binary64 in an order numpy does not fix stay under 1e-13 --; the resize rule against Pillow; hand-written
answers; the refusals; and the host code once under AddressSanitizer / UBSan as a stand-alone program (tests/evaluation_host_main.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, evaluation as ev
from tests import evaluation_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.uint8, np.int16, np.int32, np.int8, np.uint16, np.uint32)


@pytest.fixture(scope="module")
def checker():
    L = ec.build_checker()
    if L is None:
        pytest.skip("needs gcc")
    return L


@pytest.mark.parametrize("n", ec.LABEL_SIZES)
def test_confusion_3d_host_equals_the_checker(checker, n):
    for k, dtype in enumerate(DTYPES if n in (17, 300007) else DTYPES[n % 3::3]):
        gt, pred = ec.label_case(100 + k, n, dtype)
        got, oor = ev.confusion(gt, pred).numpy()
        want = ec.check_confusion_3d(checker, gt, pred)
        assert np.array_equal(got, want), (n, dtype)
        assert oor == 0
        if n == 300007:                                               # the case is not idle: valid and unknown columns, skipped elements
            assert 0 < got.sum() < n and got[:, 40].sum() > 0 and (np.diag(got) > 0).sum() >= 10
            assert got[[0, 13, 40]].sum() == 0 and got[:, [0, 13]].sum() == 0


def test_confusion_one_key_and_alternating_keys(checker):
    got, _ = ev.confusion(*ec.same_key_case()).numpy()
    assert got[5, 7] == 70000 and got.sum() == 70000
    gt, pred = ec.alternating_case()
    got, _ = ev.confusion(gt, pred).numpy()
    assert got[1, 2] == 35001 and got[2, 39] == 35000 and got.sum() == 70001
    assert np.array_equal(got, ec.check_confusion_3d(checker, gt, pred))


def test_confusion_2d_counts_every_element_and_sets_large_ids_aside(checker):
    for dtype in (np.uint8, np.uint16, np.int32):
        gt, pred = ec.label_case(7, 5001, dtype)
        got, oor = ev.confusion(gt, pred, mode=ev.MODE_2D).numpy()
        want, woor = ec.check_confusion_2d(checker, gt, pred)
        assert np.array_equal(got, want) and oor == woor
        assert oor > 50 and got.sum() + oor == 5001 and got[0].sum() > 0 and got[13].sum() > 0


def test_wider_types_and_mixed_types_read_the_same_values(checker):
    gt, pred = ec.label_case(3, 4000, np.int16)
    want = ev.confusion(gt, pred).numpy()[0]
    assert np.array_equal(ev.confusion(gt.astype(np.int64), pred.astype(np.int64)).numpy()[0], want)
    assert np.array_equal(ev.confusion(gt.astype(np.int32), pred).numpy()[0], want)
    big = np.array([1, 1, 1], np.int64), np.array([1, 2 ** 32 + 1, -2 ** 40], np.int64)     # 2^32 + 1 is not class 1
    got = ev.confusion(*big).numpy()[0]
    assert got[1, 1] == 1 and got[1, 40] == 2


def test_accumulation_equals_one_call(checker):
    gt, pred = ec.label_case(11, 9000, np.uint8)
    acc = None
    for a, b in ((0, 1), (1, 4097), (4097, 9000)):
        acc = ev.confusion(gt[a:b], pred[a:b], into=acc)
    assert np.array_equal(acc.numpy()[0], ev.confusion(gt, pred).numpy()[0])


def test_iou_against_the_checker_and_by_hand(checker):
    gt, pred = ec.label_case(5, 20000, np.uint8)
    conf = ev.confusion(gt, pred).numpy()[0]
    iou, tp, denom = ev.iou(conf)
    wiou, wtp, wdenom = ec.check_iou(checker, conf)
    assert iou.tobytes() == wiou.tobytes() and np.array_equal(tp, wtp) and np.array_equal(denom, wdenom)
    assert not np.isnan(iou).any() and (iou > 0.3).all() and (iou < 1).all()
    # by hand, classes 1 and 3 (dim 5): row 2 is no valid class, so its column entries are no false positives
    m = np.array([[0, 0, 0, 0, 0], [0, 6, 1, 2, 1], [0, 9, 9, 9, 9], [0, 3, 0, 4, 5], [0, 0, 0, 0, 0]], np.uint64)
    iou, tp, denom = ev.iou(m, [1, 3])
    assert list(tp) == [6, 4] and list(denom) == [6 + 4 + 3, 4 + 8 + 2] and iou[0] == 6 / 13 and iou[1] == 4 / 14


def test_a_class_without_ground_truth_or_prediction_has_iou_nan(checker):
    gt = np.array([1, 1, 2, 0], np.uint8)
    pred = np.array([1, 2, 2, 3], np.uint8)
    iou, tp, denom = ev.iou(ev.confusion(gt, pred))
    assert iou[0] == 0.5 and iou[1] == 0.5 and np.isnan(iou[2:]).all() and (denom[2:] == 0).all()
    assert "%5.3f" % iou[2] == "  nan"                                 # what the tables print there


SIZES = ((1296, 968), (1280, 960), (1000, 750), (641, 481), (640, 480), (320, 240))


def test_resize_rule_equals_pillow():
    """The prediction is Pillow's resize of the ground truth (640 x 480, so the size check lets it through): every pixel lies on the diagonal iff the
    library picks Pillow's source pixel.  Neighbours differ in the pattern, along x by 1 and along y by 7 (mod 41)."""
    Image = pytest.importorskip("PIL.Image")
    for w, h in SIZES:
        yy, xx = np.mgrid[0:h, 0:w]
        src = ((xx + 7 * yy) % 41).astype(np.uint8)
        want = np.ascontiguousarray(np.array(Image.fromarray(src).resize((640, 480), Image.NEAREST)))
        got, oor = ev.confusion_images(src[None], want[None]).numpy()
        assert got.sum() == np.trace(got) == 640 * 480 and oor == 0, (w, h)


def test_confusion_images_host_equals_the_checker(checker):
    for seed, gsize, psize, dtype in ((1, (1296, 968), (640, 480), np.uint8), (2, (1296, 968), (1296, 968), np.uint16), (3, (641, 481), (641, 481), np.uint8),
                                      (4, (320, 240), (320, 240), np.int32)):
        gt, pred = ec.image_case(seed, 2, gsize, psize, dtype)
        got, oor = ev.confusion_images(gt, pred).numpy()
        want, woor = ec.check_confusion_images(checker, gt, pred)
        assert np.array_equal(got, want) and oor == woor == 0 and got.sum() == 2 * 640 * 480
        assert np.trace(got) > got.sum() // 2 and (got > 0).sum() > 200
    gt, pred = ec.image_case(5, 1, (1296, 968), (640, 480), np.uint8, top=60)     # ids of 41 and more
    got, oor = ev.confusion_images(gt, pred).numpy()
    want, woor = ec.check_confusion_images(checker, gt, pred)
    assert np.array_equal(got, want) and oor == woor and oor > 10000 and got.sum() + oor == 640 * 480


def test_image_size_check_of_the_reference():
    g = np.zeros((1, 968, 1296), np.uint8)
    ev.confusion_images(g, np.zeros((1, 480, 640), np.uint8))
    ev.confusion_images(g, np.zeros((1, 100, 1296), np.uint8))         # :240 compares the widths only
    with pytest.raises(_abi.ScanfuseError) as e:
        ev.confusion_images(g, np.zeros((1, 484, 648), np.uint8))
    assert e.value.code == -1 and "648 x 484" in str(e.value)


def test_instance_plan_equals_the_checker(checker):
    for seed in (1, 2):
        s = ec.instance_scan(seed)
        iid, verts, slot = ev.instance_plan(s.gt_ids)
        wid, wverts, wslot = ec.check_plan(checker, s.gt_ids)
        assert np.array_equal(iid, wid) and np.array_equal(verts, wverts) and np.array_equal(slot, wslot)
        assert len(iid) >= 15 and (verts < 100).any() and (slot == len(iid)).sum() > 500 and (np.diff(iid) > 0).all()
    gt = np.array([0, 1001, 2005, 13001, 40001, -3001, 999, 0], np.int32)       # no instance at all: every vertex is void
    iid, verts, slot = ev.instance_plan(gt)
    assert len(iid) == 0 and (slot == 0).all()
    iid, verts, slot = ev.instance_plan(np.array([3001, 3001, 3000, 39999, 3001, 5], np.int32))
    assert list(iid) == [3000, 3001, 39999] and list(verts) == [1, 3, 1] and list(slot) == [1, 1, 0, 2, 1, 3]


@pytest.mark.parametrize("G", (0, 1, 65, 300))
def test_overlaps_host_equals_the_checker(checker, G):
    rng = np.random.default_rng(G)
    n = 5003
    slot = ec.runs(rng, n, np.arange(G + 1), 30).astype(np.uint32)
    for P in (0, 1, 33):
        wide = np.zeros((P, n + 37), np.uint8)
        masks = wide[:, 5:5 + n]                                       # rows further apart than n, and off every alignment
        for p in range(P):
            a = int(rng.integers(0, n - 10))
            masks[p, a:a + int(rng.integers(1, 900))] = rng.choice([1, 2, 255])
            masks[p, rng.integers(0, n, size=20)] = 1
        got = ev.instance_overlaps(slot, G, masks)
        want = ec.check_overlaps(checker, slot, G, np.ascontiguousarray(masks))
        assert got.shape == (P, G + 2) and np.array_equal(got, want)
        if P:
            assert (got[:, G + 1] == (masks != 0).sum(1)).all() and got[:, G + 1].min() >= 1 and (got[:, :G + 1].sum(1) == got[:, G + 1]).all()


def test_overlaps_a_slot_above_g_is_void():
    got = ev.instance_overlaps(np.array([0, 1, 2, 7, 2 ** 32 - 1], np.uint32), 2, np.ones((1, 5), np.uint8))
    assert got.tolist() == [[1, 1, 3, 5]]


def test_ap_thresholds_are_numpys():
    assert ev.ap_thresholds().tobytes() == np.append(np.arange(0.5, 0.95, 0.05), 0.25).tobytes()


@pytest.fixture(scope="module")
def scans():
    return [ec.instance_scan(seed) for seed in (21, 22, 23)]


def test_ap_equals_the_rule_restated(scans):
    with ev.InstanceAP() as acc:
        for s in scans:
            acc.add(s.gt_ids, s.masks, s.labels, s.confs)
        got = acc.finish()
    want = ec.ap_from_the_rule(scans)
    assert np.array_equal(np.isnan(got["ap"]), np.isnan(want))
    live = ~np.isnan(want)
    assert np.abs(got["ap"][live] - want[live]).max() <= 1e-12
    # the cases are not idle: classes with and without ground truth, APs strictly between 0 and 1, AP25 >= AP50 somewhere strictly
    assert live.any(1).sum() == 5 and ((want[live] > 0) & (want[live] < 1)).sum() >= 10 and (want[:, 9][live[:, 9]] > want[:, 0][live[:, 0]]).any()
    cls, avg = ec.averages_from_the_rule(want)
    for i, name in enumerate(ev.INSTANCE_NAMES):
        for j, key in enumerate(("ap", "ap50%", "ap25%")):
            a, b = got["classes"][name][key], cls[i, j]
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12
    assert max(abs(got["all_ap"] - avg[0]), abs(got["all_ap_50%"] - avg[1]), abs(got["all_ap_25%"] - avg[2])) <= 1e-12


def test_ap_does_not_depend_on_the_order_of_scans(scans):
    out = []
    for order in ((0, 1, 2), (2, 0, 1)):
        with ev.InstanceAP() as acc:
            for i in order:
                acc.add(scans[i].gt_ids, scans[i].masks, scans[i].labels, scans[i].confs)
            out.append(acc.finish()["ap"])
    assert out[0].tobytes() == out[1].tobytes()


def _one_scan_ap(gt, masks, labels, confs, min_region=2):
    s = ec.Scan(gt, masks, labels, confs)
    with ev.InstanceAP(min_region_size=min_region) as acc:
        acc.add(s.gt_ids, s.masks, s.labels, s.confs)
        got = acc.finish()["ap"]
    want = ec.ap_from_the_rule([s], min_region=min_region)
    live = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~live) and (not live.any() or np.abs(got[live] - want[live]).max() <= 1e-12)
    return got


def test_ap_by_hand_and_the_second_match_of_an_instance():
    gt = np.array([3001] * 10 + [3002] * 10 + [0] * 10, np.int32)
    exact = np.zeros((2, 30), np.uint8)
    exact[0, :10] = 1
    exact[1, 10:20] = 1
    ap = _one_scan_ap(gt, exact, [3, 3], [0.9, 0.8])
    assert (ap[0] == 1.0).all() and np.isnan(ap[1:]).all()             # cabinet: both found at every overlap; no other class has ground truth
    # two predictions over instance 3001 with IoU 1.0 and 0.9; nothing for 3002.  At thresholds below 0.9 the second one is a false positive that carries
    # the LOWER of the two scores, at 0.9 (0.9 > 0.9000000000000004 fails) it does not match and, overlapping no instance enough and no void, is a false
    # positive with its own score
    two = np.zeros((2, 30), np.uint8)
    two[0, :10] = 1
    two[1, :9] = 1
    ap = _one_scan_ap(gt, two, [3, 3], [0.6, 0.7])
    # scores (0.6 false, 0.7 true) with one missed instance: thresholds 0.6 -> p 1/2, r 1/2; 0.7 -> p 1, r 1/2: AP = 0.5 * 0.5 * 0 + 1 * 0.25 + 1 * 0.25
    assert abs(ap[0, 0] - 0.5) <= 1e-12 and abs(ap[0, 9] - 0.5) <= 1e-12
    # at 0.9: the first (0.6) matches, the second (0.7) is a plain false positive: thresholds 0.6 -> p 1/2, r 1/2; 0.7 -> p 0, r 0; the artificial point
    # p 1, r 0.  Step widths 0.5 * (r[j - 1] - r[j + 1]) with the ends repeated: 0.25, 0.25, 0: AP = 0.5 * 0.25 + 0 * 0.25 + 1 * 0
    assert abs(ap[0, 8] - 0.125) <= 1e-12


def test_ap_dropped_predictions_and_empty_sides():
    gt = np.array([3001] * 200 + [4001] * 200 + [1001] * 100, np.int32)
    masks = np.zeros((4, 500), np.uint8)
    masks[0, :200] = 255                                               # cabinet, exact
    masks[1, 200:299] = 1                                              # bed, 99 vertices: dropped for size
    masks[2, 200:400] = 1                                              # label 13: dropped for its label
    masks[3, 400:500] = 2                                              # a chair over void: ignored as a false positive, but chairs have no ground truth
    ap = _one_scan_ap(gt, masks, [3, 4, 13, 5], [0.5, 0.5, 0.5, 0.5], min_region=100)
    assert (ap[0] == 1.0).all() and (ap[1] == 0.0).all() and np.isnan(ap[2:]).all()
    ap = _one_scan_ap(gt, np.zeros((0, 500), np.uint8), [], [], min_region=100)      # P = 0
    assert (ap[:2] == 0.0).all() and np.isnan(ap[2:]).all()
    ap = _one_scan_ap(np.zeros(300, np.int32), np.ones((1, 300), np.uint8), [3], [0.5], min_region=100)   # G = 0
    assert np.isnan(ap).all()
    with ev.InstanceAP() as acc:                                       # no scan at all
        out = acc.finish()
        assert np.isnan(out["ap"]).all() and np.isnan(out["all_ap"])


def test_refusals():
    L = ev._lib()
    a = np.zeros(8, np.uint8)
    conf, oor = np.zeros(41 * 41, np.uint64), np.zeros(1, np.uint64)
    valid = ec.LABEL_IDS
    P = ev._ptr
    assert L.sf_eval_confusion(P(a), P(a), 3, 8, P(valid), 20, 0, -1, P(conf), P(oor)) == -1 and b"3 bytes" in L.sf_last_error()
    assert L.sf_eval_confusion(P(a), P(a), 1, 8, P(valid), 20, 2, -1, P(conf), P(oor)) == -1
    assert L.sf_eval_confusion(P(a), P(a), 1, 8, P(valid), 20, 1, -1, P(conf), None) == -1
    assert L.sf_eval_confusion(P(a), P(a), 1, 8, P(valid), 0, 0, -1, P(conf), P(oor)) == -1
    for bad in ([1, 1], [62], [-1]):
        with pytest.raises(_abi.ScanfuseError):
            ev.confusion(a, a, valid_ids=bad)
    ev.confusion(a, a, valid_ids=[61])
    with pytest.raises(_abi.ScanfuseError):
        ev.iou(np.zeros((3, 3), np.uint64), [5])
    slot = np.zeros(8, np.uint32)
    table = np.zeros(4, np.uint32)
    assert L.sf_eval_instance_overlaps(P(slot), 8, 0, P(a), 2, 7, -1, P(table)) == -1 and b"stride" in L.sf_last_error()
    with pytest.raises(_abi.ScanfuseError) as e:
        with ev.InstanceAP() as acc:
            acc.add_scan([3001], [10], [3], [0.5], np.array([[5, 0, 6]], np.uint32))
    assert "add up" in str(e.value)
    with pytest.raises(_abi.ScanfuseError):
        with ev.InstanceAP() as acc:
            acc.add_scan([3002, 3001], [10, 10], [], [], np.zeros((0, 4), np.uint32))
    assert conf.sum() == 0 and oor[0] == 0                             # a refusal writes nothing


def test_no_silent_fallback_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    a = np.ones(100, np.uint8)
    for call in (lambda: ev.confusion(a, a, device=0), lambda: ev.confusion_images(np.zeros((1, 480, 640), np.uint8), np.zeros((1, 480, 640), np.uint8), device=0),
                 lambda: ev.instance_overlaps(np.zeros(100, np.uint32), 1, a[None], device=0)):
        with pytest.raises(_abi.ScanfuseError) as e:
            call()
        assert e.value.code == -5


def test_host_code_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "evaluation_host")
    cmd = ["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "evaluation_host_main.cpp"),
           os.path.join(ROOT, "scannet_amd", "csrc", "evaluation.cpp")] + [os.path.join(ROOT, "scannet_amd", "csrc", f) for f in
                                                                             ("evaluation_files.cpp", "annotations.cpp", "png.cpp", "zlib_codec.cpp")] + ["-lpthread"]
    subprocess.run(cmd, check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.strip() == "evaluation host: ok"


# ---- bin/evaluate and the *_dir functions on the benchmark's files, against what the reference's scripts said (tests/golden/evaluation_golden.json,
# written by tests/golden/make_evaluation_golden.py) ----

TOOL = os.path.join(ROOT, "bin", "evaluate")


@pytest.fixture(scope="module")
def golden():
    import json
    return json.load(open(os.path.join(ROOT, "tests", "golden", "evaluation_golden.json")))


def _tool(*args):
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


def test_tool_label3d_writes_the_references_bytes(tmp_path, golden):
    pred_path, gt_path, sha = ec.write_label_dirs(str(tmp_path))
    assert sha == golden["label3d"]["inputs_sha256"]                  # the same inputs the reference saw
    rc, out, err = _tool("label3d", "--pred_path", pred_path, "--gt_path", gt_path, "--host")
    assert rc == 0 and err == ""
    got = open(os.path.join(pred_path, "semantic_label_evaluation.txt")).read()     # the script's default name
    assert got == golden["label3d"]["result_file"]
    assert ec.label_table(out) == golden["label3d"]["table"]
    assert "nan" not in got                                            # every class has a denominator: the reference could print them all
    other = str(tmp_path / "elsewhere.txt")
    assert ev.evaluate_label_dir(pred_path, gt_path, other) == out.replace(os.path.join(pred_path, "semantic_label_evaluation.txt"), other)
    assert open(other).read() == got                                   # the result file in pred_path was left out of the second run


def test_tool_instance3d_equals_the_reference(tmp_path, golden):
    pred_path, gt_path, sha, scans = ec.write_instance_dirs(str(tmp_path))
    assert sha == golden["instance3d"]["inputs_sha256"] and all(len(s.labels) >= 1 for s in scans)
    rc, out, err = _tool("instance3d", "--pred_path", pred_path, "--gt_path", gt_path, "--host")
    assert rc == 0 and err == ""
    rows = [ln.split(",") for ln in open(os.path.join(pred_path, "semantic_instance_evaluation.txt")).read().splitlines()]
    assert rows[0] == golden["instance3d"]["header"] and len(rows) == 19
    live = 0
    for got, want in zip(rows[1:], golden["instance3d"]["rows"]):
        assert got[0] == want[0] and int(got[1]) == want[1]
        for a, b in zip(got[2:], want[2:]):
            if b is None:
                assert a == "nan"
            else:
                assert abs(float(a) - b) <= 1e-12
                live += 1
    assert live >= 15
    assert ec.instance_table(out) == golden["instance3d"]["table"]
    # the numbers in the file parse back to what the accumulator holds
    with ev.InstanceAP() as acc:
        for s in scans:
            acc.add(s.gt_ids, s.masks, s.labels, s.confs)
        cls = acc.finish()["classes"]
    for got in rows[1:]:
        for a, key in zip(got[2:], ("ap", "ap50%", "ap25%")):
            assert a == "nan" if np.isnan(cls[got[0]][key]) else float(a) == cls[got[0]][key]
    rc, out2, err = _tool("instance3d", "--pred_path", pred_path, "--gt_path", gt_path, "--min-region=100000", "--output_file", tmp_path / "big.txt")
    assert rc == 0 and err == "" and open(tmp_path / "big.txt").read().count("nan") == 54      # no instance is that large: no ground truth anywhere


def test_tool_instance3d_refuses_masks_outside_the_prediction_path(tmp_path):
    pred_path, gt_path = tmp_path / "pred", tmp_path / "gt"
    (pred_path / "pred_mask").mkdir(parents=True)
    gt_path.mkdir()
    (tmp_path / "outside.txt").write_text("1\n" * 4)
    (pred_path / "pred_mask" / "m.txt").write_text("1\n" * 4)
    (gt_path / "scene.txt").write_text("3001\n" * 4)
    for line, word in (("../outside.txt 3 0.5", "outside of prediction path"), ("pred_mask/../../outside.txt 3 0.5", "outside of prediction path"),
                       ("%s 3 0.5" % (tmp_path / "outside.txt"), "relative path"), ("pred_mask/m.txt 3", "Expected (per line)"),
                       ("pred_mask/m.txt x 0.5", "must be numbers"), ("pred_mask/missing.txt 3 0.5", "unable to load"), ("pred_mask/m.txt 3 0.5\npred_mask/m.txt", "Expected")):
        (pred_path / "scene.txt").write_text(line + "\n")
        rc, out, err = _tool("instance3d", "--pred_path", pred_path, "--gt_path", gt_path)
        assert rc == 2 and out == "" and word in err and err.count("\n") == 1, (line, err)
    (pred_path / "scene.txt").write_text("pred_mask/./m.txt 3.0 0.5\npred_mask/missing.txt 13 0.5\n")      # a mask of no valid class is never opened
    rc, out, err = _tool("instance3d", "--pred_path", pred_path, "--gt_path", gt_path, "--min-region=2")
    assert rc == 0 and err == "" and "cabinet        :          1.000          1.000          1.000" in out


def test_tool_refuses_broken_text_files(tmp_path):
    pred_path, gt_path = tmp_path / "pred", tmp_path / "gt"
    pred_path.mkdir()
    gt_path.mkdir()
    assert _tool("label3d", "--pred_path", pred_path, "--gt_path", gt_path)[2] == "ERROR: No result files found.\n"
    (pred_path / "a.txt").write_text("1\n2\n3\n")
    assert "does not match any gt file" in _tool("label3d", "--pred_path", pred_path, "--gt_path", gt_path)[2]
    for text, word in (("1\n2\n", "does not match number of vertices"), ("1\n2\nx\n", "line 3 is no integer"), ("1\n\n3\n", "line 2 is no integer"),
                       ("1\n2\n3.0\n", "no integer"), ("1\n2\n" + "9" * 30 + "\n", "no integer")):
        (gt_path / "a.txt").write_text(text)
        rc, out, err = _tool("label3d", "--pred_path", pred_path, "--gt_path", gt_path)
        assert rc == 2 and out == "" and word in err, (text, err)
    (gt_path / "a.txt").write_text(" 1\n2 \r\n-3")                     # spaces, a carriage return, no line end at the end of the file
    rc, out, err = _tool("label3d", "--pred_path", pred_path, "--gt_path", gt_path)
    assert rc == 0 and err == "" and "wall          : 1.000   (     1/1     )" in out and "floor         : 1.000" in out and "cabinet       :   nan   (     0/0     )" in out
    assert _tool("nothing")[0] == 2 and _tool("label3d", "--pred_path", pred_path)[0] == 2


def test_tool_label2d_on_png_files(tmp_path, checker):
    from scannet_amd import filter2d
    pred_path, gt_path = tmp_path / "pred", tmp_path / "gt"
    pred_path.mkdir()
    gt_path.mkdir()
    gt, pred = ec.image_case(50, 2, (1296, 968), (640, 480), np.uint8)
    gt16, pred_full = ec.image_case(51, 1, (1296, 968), (1296, 968), np.uint16)
    filter2d.png_write_gray(str(gt_path / "0.png"), gt[0])
    filter2d.png_write_gray(str(pred_path / "0.png"), pred[0])
    filter2d.png_write_gray(str(gt_path / "1.png"), gt[1])
    filter2d.png_write_gray(str(pred_path / "1.png"), pred[1])
    filter2d.png_write_gray(str(gt_path / "2.png"), gt16[0])          # 16-bit ground truth, as bin/filter2dannotations writes the label frames
    filter2d.png_write_gray(str(pred_path / "2.png"), pred_full[0].astype(np.uint8))
    rc, out, err = _tool("label2d", "--pred_path", pred_path, "--gt_path", gt_path, "--host")
    assert rc == 0 and err == ""
    want = ec.check_confusion_images(checker, gt, pred)[0] + ec.check_confusion_images(checker, gt16, pred_full)[0]
    iou = ec.check_iou(checker, want)[0]
    text = open(pred_path / "semantic_label.txt").read()
    lines = text.split("\n")
    assert lines[0] == "iou scores" and lines[1] == "wall          (1 ): %5.3f" % iou[0] and lines[20] == "otherfurniture(39): %5.3f" % iou[19]
    # evalPixelLevelSemanticLabeling.py:167-173 as it stands: the heading row has no line end, and the matrix is read at the classes' positions
    assert lines[22] == "confusion matrix" and lines[23].startswith("\twall          (1 )\tfloor         (2 )") and lines[23].count("\t") == 40
    assert lines[23].endswith("otherfurniture(39)wall          (1 )" + "".join("\t%5.3f" % want[0, c] for c in range(20)))
    assert lines[24] == "floor         (2 )" + "".join("\t%5.3f" % want[1, c] for c in range(20)) and len(lines) == 44
    assert "Score Average : %5.3f" % np.nanmean(iou) in out and "wall          : %5.3f" % iou[0] in out
    rc, out, err = _tool("label2d", "--pred_path", pred_path, "--gt_path", gt_path)                     # the result file of the first run is left out
    assert rc == 0 and open(pred_path / "semantic_label.txt").read() == text
    big = gt[0].copy()
    big[100:200, 100:300] = 41
    filter2d.png_write_gray(str(gt_path / "1.png"), big)
    rc, out, err = _tool("label2d", "--pred_path", pred_path, "--gt_path", gt_path)
    assert rc == 2 and "1.png" in err and "41 or more" in err
    filter2d.png_write_gray(str(gt_path / "1.png"), gt[1])
    filter2d.png_write_gray(str(pred_path / "1.png"), pred[1][:, :600])
    assert "Invalid image size" in _tool("label2d", "--pred_path", pred_path, "--gt_path", gt_path)[2]
    (pred_path / "1.png").write_bytes(open(pred_path / "0.png", "rb").read()[:300])                    # a truncated PNG
    rc, out, err = _tool("label2d", "--pred_path", pred_path, "--gt_path", gt_path)
    assert rc == 2 and "Unable to load" in err and out == ""


# ---- export: the ground truth of a scan in the evaluation format (3d_helpers/export_train_mesh_for_evaluation.py) ----

def _export_scan(tmp_path):
    """The labelled boxes of tests/object_voxels_cases.py::write_scene_files as a scan folder, with three vertices no group holds and a fifth group
    that lists segment 11 again (a later group overwrites) -> (scan_path, label map, label_ids, instance_ids as DESIGN.md section 4o states them)."""
    import json
    from tests import object_voxels_cases as oc
    paths = oc.write_scene_files(tmp_path)[0]
    scan = tmp_path / "scene0042_00"
    scan.mkdir()
    seg = json.load(open(paths["segs"]))["segIndices"] + [99, 99, 98]
    groups = json.load(open(paths["agg"]))["segGroups"] + [{"id": 4, "objectId": 7, "segments": [11], "label": "table"}]
    json.dump({"params": {}, "sceneId": "scene0042_00", "segIndices": seg}, open(scan / "scene0042_00_vh_clean_2.0.010000.segs.json", "w"))
    json.dump({"sceneId": "scene0042_00", "appId": "test", "segGroups": groups}, open(scan / "scene0042_00.aggregation.json", "w"))
    tsv = tmp_path / "labels.combined.tsv"
    nyu40 = {"office chair": 5, "table": 7, "chair": 5, "thing": 40, "lamp": 35}
    tsv.write_text("id\traw_category\tcategory\tcount\tnyu40id\tnyu40class\n" + "".join("%d\t%s\tx\t1\t%d\ty\n" % (i, k, v) for i, (k, v) in enumerate(nyu40.items())))
    label, inst = np.zeros(len(seg), np.uint32), np.zeros(len(seg), np.uint32)
    for g in groups:                                                   # file order, a later group overwrites
        at = np.isin(seg, g["segments"])
        label[at], inst[at] = nyu40[g["label"]], g["objectId"] + 1
    return scan, tsv, label, inst


def test_tool_export_writes_the_evaluation_format(tmp_path):
    scan, tsv, label, inst = _export_scan(tmp_path)
    assert sorted(set(inst)) == [0, 1, 2, 3, 6, 8] and (label[inst == 8] == 7).all() and (inst == 8).sum() == 4 and (inst == 0).sum() == 3
    got_label, got_inst = ev.export_ids(scan / "scene0042_00_vh_clean_2.0.010000.segs.json", scan / "scene0042_00.aggregation.json", tsv)
    assert np.array_equal(got_label, label) and np.array_equal(got_inst, inst)
    out = tmp_path / "out"
    (out / "gt").mkdir(parents=True)
    (out / "pred").mkdir()
    args = ("export", "--scan_path", scan, "--label_map_file", tsv)
    rc, stdout, err = _tool(*args, "--type", "label", "--output_file", out / "labels.txt")
    assert (rc, stdout, err) == (0, "", "")
    assert open(out / "labels.txt").read() == "".join("%d\n" % i for i in label)          # util_3d.export_ids
    rc, stdout, err = _tool(*args, "--type", "instance-gt", "--output_file", out / "gt" / "scene0042_00.txt")
    assert (rc, stdout, err) == (0, "", "")
    assert open(out / "gt" / "scene0042_00.txt").read() == "".join("%d\n" % (l * 1000 + i if i else 0) for l, i in zip(label, inst))
    rc, stdout, err = _tool(*args, "--type", "instance", "--output_file", str(scan) + "/../out/pred/scene0042_00.txt")
    assert (rc, stdout, err) == (0, "", "")
    # util_3d.export_instance_ids_for_eval: numbered by the position among the sorted distinct ids (0 is there: the first object is _1)
    want = ["pred_mask/scene0042_00_%d.txt %d 1.000000" % (k, label[inst == i][0]) for k, i in enumerate(sorted(set(inst))) if i]
    assert open(out / "pred" / "scene0042_00.txt").read().splitlines() == want and len(want) == 5
    for k, i in enumerate(sorted(set(inst))):
        if i:
            assert open(out / "pred" / "pred_mask" / ("scene0042_00_%d.txt" % k)).read() == "".join("%d\n" % (j == i) for j in inst)
    ev.export_ground_truth(scan, tsv, "instance", out / "pred" / "scene0042_00.txt")      # again, over an existing pred_mask/
    # the exported ground truth scored against itself: every class that occurs is found at every overlap; label 40 is no class and is dropped
    rc, stdout, err = _tool("instance3d", "--pred_path", out / "pred", "--gt_path", out / "gt", "--min-region=2")
    assert rc == 0 and err == ""
    assert "chair          :          1.000          1.000          1.000" in stdout and "table          :          1.000          1.000          1.000" in stdout
    assert stdout.count("nan") == 16 * 3 and "average        :          1.000          1.000          1.000" in stdout
    rc, stdout, err = _tool("label3d", "--pred_path", out / "gt", "--gt_path", out / "gt")            # and the label export is a label file
    (out / "lp").mkdir()
    (out / "lg").mkdir()
    ev.export_ground_truth(str(scan) + "/", tsv, "label", out / "lp" / "s.txt")                       # a trailing slash names the same scan
    ev.export_ground_truth(scan, tsv, "label", out / "lg" / "s.txt")
    text = ev.evaluate_label_dir(out / "lp", out / "lg")
    assert "chair         : 1.000   (    12/12    )" in text and "table         : 1.000   (    12/12    )" in text


def test_export_refusals(tmp_path):
    scan, tsv, label, inst = _export_scan(tmp_path)
    segs, agg = scan / "scene0042_00_vh_clean_2.0.010000.segs.json", scan / "scene0042_00.aggregation.json"
    rc, out, err = _tool("export", "--scan_path", scan, "--label_map_file", tsv, "--type", "panoptic", "--output_file", tmp_path / "x.txt")
    assert rc == 2 and "panoptic" in err and not (tmp_path / "x.txt").exists()
    assert _tool("export", "--scan_path", scan, "--label_map_file", tsv, "--type", "label")[0] == 2
    rc, out, err = _tool("export", "--scan_path", tmp_path / "scene0043_00", "--label_map_file", tsv, "--type", "label", "--output_file", tmp_path / "x.txt")
    assert rc == 2 and "scene0043_00_vh_clean_2.0.010000.segs.json" in err
    short = tmp_path / "short.tsv"
    short.write_text("id\traw_category\tnyu40id\n1\tchair\t5\n2\ttable\t7\n3\toffice chair\t5\n")
    with pytest.raises(_abi.ScanfuseError) as e:
        ev.export_ids(segs, agg, short)
    assert e.value.code == -3 and '"thing"' in str(e.value)
    short.write_text("id\traw_category\tnyu40class\n1\tchair\tchair\n")
    with pytest.raises(_abi.ScanfuseError) as e:
        ev.export_ids(segs, agg, short)
    assert e.value.code == -3 and "nyu40id" in str(e.value)
    short.write_text("id\traw_category\tnyu40id\n1\tchair\t\n")
    with pytest.raises(_abi.ScanfuseError) as e:
        ev.export_ids(segs, agg, short)
    assert e.value.code == -3 and "line 2" in str(e.value)
    L = ev._lib()
    n = __import__("ctypes").c_uint64(0)
    small = np.full(5, 77, np.uint32)
    args = (os.fsencode(str(segs)), os.fsencode(str(agg)), os.fsencode(str(tsv)))
    assert L.sf_eval_export_ids(*args, 5, ev._ptr(small), None, __import__("ctypes").byref(n)) == -7 and n.value == len(label) and (small == 77).all()


def test_prediction_file_numbers_are_read_as_python_reads_them(tmp_path):
    pred_path, gt_path = tmp_path / "pred", tmp_path / "gt"
    (pred_path / "pred_mask").mkdir(parents=True)
    gt_path.mkdir()
    (pred_path / "pred_mask" / "m.txt").write_text("1\n" * 4)
    (gt_path / "scene.txt").write_text("3001\n" * 4)

    def python_reads(text):
        try:
            float(text)
            return True
        except ValueError:
            return False
    assert all(python_reads(v) for v in ("3.0", "5e-1", "+3", "inf", "-Infinity")) and not any(python_reads(v) for v in ("0x3", "0x1p-1", "nan(1)"))
    # the stated differences from float(): a NaN confidence, an infinite label (int() of it raises in the reference) and digit groups are refused
    for label, conf, ok in (("3", "0.5", True), ("3.0", "5e-1", True), ("+3", "inf", True), ("3", "-Infinity", True), ("0x3", "0.5", False), ("3", "0x1p-1", False),
                            ("3", "nan", False), ("3", "nan(1)", False), ("inf", "0.5", False), ("3", "1_0", False)):
        (pred_path / "scene.txt").write_text("pred_mask/m.txt %s %s\n" % (label, conf))
        rc, out, err = _tool("instance3d", "--pred_path", pred_path, "--gt_path", gt_path, "--min-region=2")
        assert (rc == 0) == ok and (ok or "must be numbers" in err), (label, conf, err)
