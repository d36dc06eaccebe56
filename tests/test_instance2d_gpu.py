"""The 2-D instance task on the GPU: k_eval_image_ids with k_eval_image_compact and k_eval_overlaps_images
(scannet_amd/csrc/evaluation.hip) against the brute-force checker tests/instance2d_checker.c and the host path, count for count: at the sizes around
a 16-byte vector and a span, at every pixel width, from pointers off a 16-byte boundary, with mask rows further apart than an image, with more
instances than the LDS table and the LDS id list hold, on one id (the contention case), with ids outside the counter range; tensors in and out on
a side stream; the current device; a refused call; and bin/evaluate instance2d --device=0 against --host."""
import os
import subprocess

import numpy as np
import pytest
import torch

from scannet_amd import _abi, evaluation as ev
from tests import instance2d_cases as ic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "evaluate")
SIZES = ((1, 1), (15, 1), (17, 3), (67, 45), (128, 96))
ID_TABLE, OI_LIST = 1024, 2048   # entries of k_eval_image_ids' LDS table, ids of one pass of k_eval_overlaps_images (evaluation.hip)


@pytest.fixture(scope="module")
def checker():
    L = ic.build_checker()
    if L is None:
        pytest.skip("needs gcc")
    return L


def dev(a):
    """numpy -> a tensor on the GPU with the same bits (torch has no arithmetic on uint16 / uint32: the signed twin carries them)"""
    a = np.ascontiguousarray(a)
    twin = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(twin) if twin else a).to("cuda:0")


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def same_plan(got, plans, capacity):
    want = ic.plan_arrays(plans, capacity)
    count, ids, px = (host(t) if torch.is_tensor(t) else t for t in got)
    return np.array_equal(count, want[0]) and np.array_equal(ids.view(np.int32), want[1]) and np.array_equal(px, want[2])


def both_ways(checker, gt, masks, mask_image, gt_t=None, masks_t=None):
    """The plan and the table of a batch through the device, from host arrays and from tensors, against the checker.  -> the checker's plans"""
    plans = ic.check_plan(checker, gt)
    capacity = max([len(p[0]) for p in plans] + [0])
    want = ic.check_table(checker, gt, plans, masks, mask_image, capacity)
    got = ev.image_plan(gt, device=0)                                                   # host arrays through the device
    assert got[1].shape[1] == capacity and same_plan(got, plans, capacity)
    assert np.array_equal(ev.overlaps_images(gt, got[0], got[1], masks, mask_image, device=0), want)
    gt_t = dev(gt) if gt_t is None else gt_t
    masks_t = dev(masks) if masks_t is None else masks_t
    count, ids, px = ev.image_plan(gt_t, capacity=capacity)                             # tensors: nothing leaves the device
    assert count.is_cuda and ids.is_cuda and px.is_cuda and same_plan((count, ids, px), plans, capacity)
    table = ev.overlaps_images(gt_t, count, ids, masks_t, dev(np.asarray(mask_image, np.uint32)))
    assert table.is_cuda and tuple(table.shape) == (len(mask_image), capacity + 2)
    assert np.array_equal(host(table), want)
    return plans


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16, np.uint32))
def test_device_plan_and_overlaps_equal_checker_and_host(checker, dtype):
    for (w, h) in SIZES:
        for batch in (1, 3, 17):
            gt, masks, mask_image, _, _ = ic.image_batch(1000 + w + batch, batch, w, h, dtype, n_inst=6 if batch == 17 else 12, masks_per_image=2)
            plans = both_ways(checker, gt, masks, mask_image)
            host_plan = ev.image_plan(gt)
            assert same_plan(host_plan, plans, host_plan[1].shape[1])


def test_a_640_by_480_pair(checker):
    gt, masks, mask_image, _, _ = ic.image_batch(77, 2, 640, 480, np.uint16, n_inst=30, masks_per_image=3)
    plans = both_ways(checker, gt, masks, mask_image)
    assert min(len(p[0]) for p in plans) >= 10


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16, np.uint32))
def test_pointers_off_a_16_byte_boundary_and_a_wide_mask_stride(checker, dtype):
    w, h, batch = 67, 45, 3
    gt, masks, mask_image, _, _ = ic.image_batch(31, batch, w, h, dtype, masks_per_image=3)
    n, P = w * h, len(mask_image)
    for goff, moff in ((1, 1), (3, 0), (0, 5), (7, 13)):                               # in pixels of the ground truth, in bytes of the masks
        flat = torch.zeros(goff + batch * n, dtype=dev(gt).dtype, device="cuda:0")
        flat[goff:] = dev(gt).reshape(-1)
        gt_t = flat[goff:].view(batch, h, w)
        mflat = torch.zeros(moff + P * n, dtype=torch.uint8, device="cuda:0")
        mflat[moff:] = dev(masks).reshape(-1)
        masks_t = mflat[moff:].view(P, n)
        assert gt_t.data_ptr() % 16 == (goff * gt.itemsize) % 16 and masks_t.data_ptr() % 16 == moff % 16
        both_ways(checker, gt, masks, mask_image, gt_t, masks_t)
    wide = torch.full((P, n + 37), 9, dtype=torch.uint8, device="cuda:0")              # rows 37 bytes further apart, set bytes between them
    wide[:, :n] = dev(masks)
    both_ways(checker, gt, masks, mask_image, None, wide[:, :n])
    wide_np = np.full((P, n + 37), 9, np.uint8)
    wide_np[:, :n] = masks
    plans = ic.check_plan(checker, gt)
    count, ids, _ = ev.image_plan(gt)
    assert np.array_equal(ev.overlaps_images(gt, count, ids, wide_np[:, :n], mask_image, device=0), ic.check_table(checker, gt, plans, masks, mask_image, ids.shape[1]))


@pytest.mark.parametrize("instances", (0, 1, 65, 300, 5000))
def test_instance_counts_up_to_beyond_the_lds_table_and_list(checker, instances):
    w, h = 128, 64
    if instances == 5000:
        gt = ic.distinct_ids_image(w, h)                      # every pixel its own id: 8192 of them, over the 18 classes
        assert w * h > 4 * ID_TABLE and w * h > 2 * OI_LIST   # the table overflows into the range passes, the list takes several passes
    else:
        gt = np.zeros((1, h, w), np.uint32)
        flat = gt.reshape(-1)
        per = (w * h) // max(instances, 1)
        for k in range(instances):                            # runs of `per` pixels, ids over the classes and out of order along the image
            flat[k * per:(k + 1) * per] = int(ic.INSTANCE_IDS[(7 * k) % 18]) * 1000 + 1 + k // 18
    rng = np.random.default_rng(instances)
    masks = np.zeros((3, w * h), np.uint8)
    masks[0] = 1
    masks[1, rng.random(w * h) < 0.3] = 255
    masks[2, 1000:1017] = 2
    plans = both_ways(checker, gt, masks, [0, 0, 0])
    assert len(plans[0][0]) == (8192 if instances == 5000 else instances)


def test_images_without_a_mask_and_with_33(checker):
    gt, _, _, _, _ = ic.image_batch(5, 4, 67, 45, np.uint16, masks_per_image=1)
    rng = np.random.default_rng(9)
    mask_image = np.array([2] * 33 + [0, 3, 0], np.uint32)    # image 1 has no mask, image 2 has 33; the rows are not sorted by image
    masks = (rng.random((len(mask_image), 67 * 45)) < 0.4).astype(np.uint8) * rng.choice([1, 2, 255], size=(len(mask_image), 1)).astype(np.uint8)
    both_ways(checker, gt, masks, mask_image)


def test_one_id_and_mask_values_2_and_255():
    gt = np.full((1, 480, 640), 7001, np.uint16)              # the contention case: every run of every lane is the same id
    count, ids, px = ev.image_plan(dev(gt), capacity=4)
    assert host(count).tolist() == [1] and host(ids)[0, 0] == 7001 and host(px)[0, 0] == 640 * 480
    masks = np.zeros((2, 640 * 480), np.uint8)
    masks[0, ::3] = 2
    masks[1, 5::2] = 255
    table = host(ev.overlaps_images(dev(gt), count, ids, dev(masks), dev(np.array([0, 0], np.uint32))))
    want = [int((masks[0] != 0).sum()), int((masks[1] != 0).sum())]
    assert table[:, 0].tolist() == want and table[:, 5].tolist() == want and not table[:, 1:5].any()


def test_ids_at_or_above_the_counter_range(checker):
    gt = np.zeros((1, 45, 67), np.uint32)
    flat = gt.reshape(-1)
    values = [39999, 40000, 40001, 65535, 999999, 1000000, 5001 + 2 ** 20, 2 ** 31 + 5001, 2 ** 32 - 1, 39001, 5001, 39]
    for k, v in enumerate(values):
        flat[k * 200:(k + 1) * 200] = v
    masks = np.ones((1, 45 * 67), np.uint8)
    plans = both_ways(checker, gt, masks, [0])
    assert plans[0][0].tolist() == [5001, 39001, 39999] and plans[0][1].tolist() == [200, 200, 200]
    gt16 = np.full((1, 45, 67), 65535, np.uint16)
    gt16[0, 0, :9] = 40000
    gt16[0, 1, :9] = 39123
    assert both_ways(checker, gt16, masks, [0])[0][0].tolist() == [39123]


def test_tensors_on_a_side_stream_and_the_current_device(checker):
    gt, masks, mask_image, labels, confs = ic.image_batch(3, 3, 128, 96, np.uint16, masks_per_image=4)
    plans = ic.check_plan(checker, gt)
    capacity = max(len(p[0]) for p in plans)
    want = ic.check_table(checker, gt, plans, masks, mask_image, capacity)
    before = torch.cuda.current_device()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        gt_t, masks_t, mi_t = dev(gt), dev(masks), dev(mask_image)
        count, ids, px = ev.image_plan(gt_t, capacity=capacity)
        table = ev.overlaps_images(gt_t, count, ids, masks_t, mi_t)
    side.synchronize()
    assert torch.cuda.current_device() == before
    assert same_plan((count, ids, px), plans, capacity) and np.array_equal(host(table), want)
    with ev.InstanceAP2D() as a, ev.InstanceAP2D() as b:
        a.add(dev(gt), dev(masks), mask_image, labels, confs, capacity=capacity)
        b.add(gt, masks, mask_image, labels, confs)
        assert a.finish()["ap"].tobytes() == b.finish()["ap"].tobytes()


def test_a_refused_device_call_writes_nothing():
    L = ev._lib()
    gt = dev(np.full((1, 8, 8), 5001, np.uint16))
    v = np.array(ev.INSTANCE_IDS, np.int32)
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
    ids = torch.full((1, 2), -7, dtype=torch.int32, device="cuda:0")
    px = torch.full((1, 2), 7, dtype=torch.int32, device="cuda:0")
    scratch = torch.full((40000,), 5, dtype=torch.int32, device="cuda:0")
    table = torch.full((1, 4), 9, dtype=torch.int32, device="cuda:0")
    masks = torch.ones((1, 64), dtype=torch.uint8, device="cuda:0")
    image = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    p = ev._ptr
    bad_ids = np.array([5, 1000], np.int32)
    host_gt = np.zeros((1, 8, 8), np.uint16)
    plan_calls = (
        lambda: L.sf_eval_image_plan_device(p(gt), 3, 1, 8, 8, p(v), len(v), 2, None, p(scratch), p(count), p(ids), p(px)),               # pixels of 3 bytes
        lambda: L.sf_eval_image_plan_device(p(gt), 2, 1, 8, 8, p(bad_ids), 2, 2, None, p(scratch), p(count), p(ids), p(px)),            # a class id of 1000
        lambda: L.sf_eval_image_plan_device(p(host_gt), 2, 1, 8, 8, p(v), len(v), 2, None, p(scratch), p(count), p(ids), p(px)),        # host memory
        lambda: L.sf_eval_image_plan_device(p(gt), 2, 1, 8, 8, p(v), len(v), 2, None, C_void(scratch.data_ptr() + 4), p(count), p(ids), p(px)),   # scratch off 16 bytes
        lambda: L.sf_eval_image_plan_device(p(gt), 2, 1, 1 << 16, 1 << 16, p(v), len(v), 2, None, p(scratch), p(count), p(ids), p(px)),  # 2^32 pixels
    )
    for call in plan_calls:
        assert call() == -1
    overlap_calls = (
        lambda: L.sf_eval_overlaps_images_device(p(gt), 2, 1, 8, 8, p(v), len(v), 2, p(count), p(ids), p(masks), 1, 63, p(image), None, p(table)),   # a stride below an image
        lambda: L.sf_eval_overlaps_images_device(p(gt), 2, 1, 8, 8, p(v), len(v), 2, p(count), p(ids), p(np.ones((1, 64), np.uint8)), 1, 64, p(image), None, p(table)),
        lambda: L.sf_eval_overlaps_images_device(p(gt), 2, 1, 8, 8, p(bad_ids), 2, 2, p(count), p(ids), p(masks), 1, 64, p(image), None, p(table)),
    )
    for call in overlap_calls:
        assert call() == -1
    torch.cuda.synchronize()
    assert (count == 77).all() and (ids == -7).all() and (px == 7).all() and (scratch == 5).all() and (table == 9).all()
    with pytest.raises(_abi.ScanfuseError):
        _abi.check(plan_calls[2]())


def C_void(address):
    import ctypes
    return ctypes.c_void_p(address)


def test_tool_on_the_device_writes_the_bytes_of_the_host(tmp_path):
    pred_path, gt_path, _ = ic.write_file_case(str(tmp_path))
    outs = []
    for how in ("--host", "--device=0"):
        out_file = str(tmp_path / ("result" + how.strip("-=0") + ".txt"))
        r = subprocess.run([TOOL, "instance2d", "--pred_path", pred_path, "--gt_path", gt_path, "--output_file", out_file, how], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        outs.append((r.stdout, open(out_file, "rb").read()))
    assert outs[0] == outs[1] and "chair" in outs[0][0]
