"""The benchmark's scores on the GPU: the kernels of scannet_amd/csrc/evaluation.hip against the brute-force checker
tests/evaluation_checker.c and the host path, count for count: k_eval_confusion at the sizes around a 16-byte vector and a workgroup, at every element
width, from pointers off a 16-byte boundary, on one key and on alternating keys; k_eval_confusion_images on a batch; k_eval_overlaps with more bins
than its LDS holds; accumulation in a matrix that stays on the device; torch tensors in and out."""
import numpy as np
import pytest
import torch

from scannet_amd import evaluation as ev
from tests import evaluation_cases as ec

pytestmark = pytest.mark.gpu

OV_BINS = 4096   # k_eval_overlaps' LDS bins (evaluation.hip)


@pytest.fixture(scope="module")
def checker():
    L = ec.build_checker()
    if L is None:
        pytest.skip("needs gcc")
    return L


def dev(a):
    """numpy -> a tensor on the GPU with the same bits (torch has no arithmetic on uint16 / uint32: the signed twin carries them)"""
    a = np.ascontiguousarray(a)
    twin = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(twin) if twin else a).to("cuda:0")


@pytest.mark.parametrize("dtype", (np.uint8, np.int16, np.int32))
def test_confusion_3d_device_equals_checker_and_host(checker, dtype):
    for n in ec.LABEL_SIZES:
        gt, pred = ec.label_case(200 + n % 7, n, dtype)
        want = ec.check_confusion_3d(checker, gt, pred)
        got, oor = ev.confusion(gt, pred, device=0).numpy()             # host arrays through the device
        assert np.array_equal(got, want) and oor == 0, (n, dtype)
        assert np.array_equal(ev.confusion(gt, pred).numpy()[0], want)
        counts = ev.confusion(dev(gt), dev(pred))                       # tensors: nothing leaves the device
        assert counts.on_device and counts.matrix.is_cuda and counts.matrix.shape == (41, 41)
        assert np.array_equal(counts.numpy()[0], want), (n, dtype)
        if n == 300007:
            assert 0 < got.sum() < n and got[:, 40].sum() > 0 and (np.diag(got) > 0).sum() == 20   # negative and huge predictions went to column 40


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16, np.uint32))
def test_confusion_from_pointers_off_a_16_byte_boundary(checker, dtype):
    gt, pred = ec.label_case(31, 9000, dtype)
    dg, dp = dev(gt), dev(pred)
    for a, b in ((1, 1), (1, 0), (0, 3), (5, 2)):                      # slices: both off by the same, and by different amounts
        n = 8000
        g, p = dg[a:a + n], dp[b:b + n]
        assert g.data_ptr() % 16 == (a * gt.itemsize) % 16
        want = ec.check_confusion_3d(checker, gt[a:a + n], pred[b:b + n])
        assert np.array_equal(ev.confusion(g, p).numpy()[0], want), (dtype, a, b)
    for n in (1, 3, 17):                                                # shorter than the way to the boundary, and just past it
        assert np.array_equal(ev.confusion(dg[1:1 + n], dp[1:1 + n]).numpy()[0], ec.check_confusion_3d(checker, gt[1:1 + n], pred[1:1 + n]))


def test_confusion_one_key_and_alternating_keys(checker):
    gt, pred = ec.same_key_case()
    got = ev.confusion(dev(gt), dev(pred)).numpy()[0]
    assert got[5, 7] == 70000 and got.sum() == 70000
    for dtype in (np.uint8, np.uint16, np.uint32):
        gt, pred = ec.alternating_case(dtype)
        got = ev.confusion(dev(gt), dev(pred)).numpy()[0]
        assert got[1, 2] == 35001 and got[2, 39] == 35000 and got.sum() == 70001


def test_confusion_2d_mode_on_the_device(checker):
    for dtype in (np.uint8, np.int16, np.int32):
        gt, pred = ec.label_case(7, 5001, dtype)
        want, woor = ec.check_confusion_2d(checker, gt, pred)
        got, oor = ev.confusion(dev(gt), dev(pred), mode=ev.MODE_2D).numpy()
        assert np.array_equal(got, want) and oor == woor and oor > 50


def test_confusion_images_batch(checker):
    for psize, dtype in (((640, 480), np.uint8), ((1296, 968), np.uint8), ((1296, 968), np.uint16)):
        gt, pred = ec.image_case(40, 3, (1296, 968), psize, dtype)
        want, woor = ec.check_confusion_images(checker, gt, pred)
        got, oor = ev.confusion_images(dev(gt), dev(pred)).numpy()
        assert np.array_equal(got, want) and oor == woor == 0 and got.sum() == 3 * 640 * 480, (psize, dtype)
        host, hoor = ev.confusion_images(gt, pred).numpy()
        assert np.array_equal(got, host) and hoor == 0
    gt, pred = ec.image_case(41, 1, (1296, 968), (640, 480), np.uint8, top=60)      # ids of 41 and more
    want, woor = ec.check_confusion_images(checker, gt, pred)
    got, oor = ev.confusion_images(gt, pred, device=0).numpy()
    assert np.array_equal(got, want) and oor == woor and oor > 10000
    got, oor = ev.confusion_images(dev(gt), dev(pred)).numpy()
    assert np.array_equal(got, want) and oor == woor


def _masks(rng, P, n, pad):
    wide = np.zeros((P, n + pad), np.uint8)
    masks = wide[:, 5:5 + n] if pad else wide                          # rows further apart than n, off every alignment
    for p in range(P):
        a = int(rng.integers(0, max(1, n - 10)))
        masks[p, a:a + int(rng.integers(1, 900))] = rng.choice([1, 2, 255])
        masks[p, rng.integers(0, n, size=20)] = 2
    return wide, masks


@pytest.mark.parametrize("G", (0, 1, 65, 300, OV_BINS + 1000))
def test_overlaps_device_equals_checker_and_host(checker, G):
    rng = np.random.default_rng(G)
    n = 70003                                                           # three spans of vertices, not a multiple of 16
    slot = ec.runs(rng, n, np.arange(G + 1), 30).astype(np.uint32)
    if G > OV_BINS:
        slot[:G + 1] = np.arange(G + 1)                                 # every bin of every pass is hit by the first mask
    for P in (0, 1, 33):
        wide, masks = _masks(rng, P, n, 37)
        if P and G > OV_BINS:
            masks[0, :G + 1] = 1
        want = ec.check_overlaps(checker, slot, G, np.ascontiguousarray(masks))
        assert np.array_equal(ev.instance_overlaps(slot, G, masks), want)
        assert np.array_equal(ev.instance_overlaps(slot, G, masks, device=0), want), (G, P)
        dslot, dwide = dev(slot), dev(wide)
        table = ev.instance_overlaps(dslot, G, dwide[:, 5:5 + n])       # a view: the stride stays n + 37
        assert table.is_cuda and np.array_equal(table.cpu().numpy().view(np.uint32), want), (G, P)
        if P:
            assert want[:, G + 1].min() >= 1 and (want[:, :G + 1].sum(1) == want[:, G + 1]).all()
    if G > OV_BINS:
        assert (want[0, :G + 1] >= 1).all() and want[0, OV_BINS:].sum() > 1000


def test_accumulation_in_a_matrix_that_stays_on_the_device(checker):
    gt, pred = ec.label_case(11, 9000, np.uint8)
    dg, dp = dev(gt), dev(pred)
    acc = None
    for a, b in ((0, 1), (1, 4097), (4097, 9000)):
        acc = ev.confusion(dg[a:b], dp[a:b], into=acc)
    assert acc.on_device and np.array_equal(acc.numpy()[0], ec.check_confusion_3d(checker, gt, pred))
    iou = ev.iou(acc)[0]
    assert iou.tobytes() == ec.check_iou(checker, acc.numpy()[0])[0].tobytes()


def test_tensors_in_and_a_tensor_out_on_the_current_stream(checker):
    gt, pred = ec.label_case(12, 100000, np.int32)
    want = ec.check_confusion_3d(checker, gt, pred)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.from_numpy(gt).to("cuda:0", non_blocking=False)
        p = (g + 0)                                                     # made on stream s: the count must be ordered behind it
        p.copy_(torch.from_numpy(pred))
        counts = ev.confusion(g, p)
        total = counts.matrix.sum()                                     # consumed on the device, behind the kernel
    s.synchronize()
    assert counts.matrix.device.type == "cuda" and counts.matrix.dtype == torch.int64
    assert int(total) == int(want.sum()) and np.array_equal(counts.numpy()[0], want)
    wide = ev.confusion(g.to(torch.int64), p.to(torch.int64))           # int64 tensors are narrowed on the device
    assert np.array_equal(wide.numpy()[0], want)


def test_ap_with_masks_on_the_device():
    scans = [ec.instance_scan(seed) for seed in (21, 22)]
    out = []
    for on_device in (False, True):
        with ev.InstanceAP() as acc:
            for s in scans:
                acc.add(s.gt_ids, dev(s.masks) if on_device else s.masks, s.labels, s.confs)
            out.append(acc.finish()["ap"])
    assert out[0].tobytes() == out[1].tobytes() and (~np.isnan(out[0])).sum() >= 30


def test_tool_on_the_device_writes_the_bytes_of_the_host_path(tmp_path):
    import os
    import subprocess
    from scannet_amd import filter2d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "bin", "evaluate")
    label = ec.write_label_dirs(str(tmp_path))[:2]
    inst = ec.write_instance_dirs(str(tmp_path))[:2]
    pix = (str(tmp_path / "pix_pred"), str(tmp_path / "pix_gt"))
    os.makedirs(pix[0])
    os.makedirs(pix[1])
    gt, pred = ec.image_case(50, 2, (1296, 968), (640, 480), np.uint8)
    for i in range(2):
        filter2d.png_write_gray(os.path.join(pix[1], "%d.png" % i), gt[i])
        filter2d.png_write_gray(os.path.join(pix[0], "%d.png" % i), pred[i])
    for mode, (pred_path, gt_path) in (("label3d", label), ("instance3d", inst), ("label2d", pix)):
        files, texts = [], []
        for how in ("--host", "--device=0"):
            out = str(tmp_path / ("%s%s.txt" % (mode, how)))
            r = subprocess.run([tool, mode, "--pred_path", pred_path, "--gt_path", gt_path, "--output_file", out, how], capture_output=True, text=True)
            assert r.returncode == 0 and r.stderr == "", (mode, how, r.stderr)
            files.append(open(out, "rb").read())
            texts.append(r.stdout.replace(out, ""))
        assert files[0] == files[1] and len(files[0]) > 500 and texts[0] == texts[1], mode


def test_device_calls_keep_the_current_device_and_a_refusal_writes_nothing():
    import ctypes as C
    L = ev._lib()
    before = torch.cuda.current_device()
    slot = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    masks = torch.ones((2, 64), dtype=torch.uint8, device="cuda:0")
    table = torch.full((2, 3), 7, dtype=torch.int32, device="cuda:0")
    rc = L.sf_eval_instance_overlaps_device(C.c_void_p(slot.data_ptr() + 1), 60, 1, C.c_void_p(masks.data_ptr()), 2, 64, None, C.c_void_p(table.data_ptr()))
    torch.cuda.synchronize()
    assert rc == -1 and b"aligned" in L.sf_last_error() and (table == 7).all()           # refused before the table was zeroed
    host = np.zeros(64, np.uint32)
    rc = L.sf_eval_instance_overlaps_device(host.ctypes.data_as(C.c_void_p), 64, 1, C.c_void_p(masks.data_ptr()), 2, 64, None, C.c_void_p(table.data_ptr()))
    assert rc == -1 and b"not device memory" in L.sf_last_error() and (table == 7).all()
    got = ev.instance_overlaps(slot, 1, masks)
    assert got.cpu().tolist() == [[64, 0, 64], [64, 0, 64]] and torch.cuda.current_device() == before
    if torch.cuda.device_count() > 1:                                   # tensors on another device than the current one
        g = torch.ones(1000, dtype=torch.uint8, device="cuda:1")
        counts = ev.confusion(g, g)
        assert torch.cuda.current_device() == before and counts.numpy()[0][1, 1] == 1000
