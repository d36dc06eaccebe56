"""Measures the 2-D instance task on one GPU and prints the table kept in profiles/instance2d.txt: the plan kernels and the
overlaps kernel on inputs that already sit in device memory, beside a device-to-device copy of the same bytes in the same run; the host path on
the same inputs; the composition the 3-D entry points offer (sf_eval_instance_plan on the host and one sf_eval_instance_overlaps_device call per
image over a 4-byte slot image); and bin/evaluate instance2d with --host and --device=0 on a directory of such images.  Every figure is the median
of 5 repeats after one warm-up, with the fastest and the slowest repeat beside it.

    python tools/instance2d_bench.py [--out FILE] [--images 64] [--tool-images 16]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scannet_amd import evaluation as ev, filter2d  # noqa: E402
from tools.evaluation_bench import REPEATS, device_ms, row, wall  # noqa: E402

W, H, INSTANCES, MASKS = 1296, 968, 30, 20
CLASSES = (3, 4, 5, 7, 8, 9, 12, 14, 39)


def images(rng, batch):
    """-> (gt uint16 [B, H, W], boxes per image): large uniform regions -- about INSTANCES rectangles of instances over a background of 0, wall and
    floor values and void (raw class ids)."""
    gt = np.zeros((batch, H, W), np.uint16)
    boxes = []
    for b in range(batch):
        gt[b, :H // 3] = 1
        gt[b, 2 * H // 3:] = 2
        gt[b, H // 3:H // 2, :W // 4] = 5
        mine = []
        for k in range(INSTANCES):
            x0, y0 = int(rng.integers(0, W - 80)), int(rng.integers(0, H - 80))
            x1, y1 = min(W, x0 + int(rng.integers(60, 400))), min(H, y0 + int(rng.integers(60, 300)))
            label = int(rng.choice(CLASSES))
            gt[b, y0:y1, x0:x1] = label * 1000 + k + 1
            mine.append((x0, y0, x1, y1, label))
        boxes.append(mine)
    return gt, boxes


def masks_of(rng, boxes):
    """MASKS masks per image: an instance's rectangle moved by a few pixels.  -> (masks uint8 [P, H * W], mask_image, labels, confs)"""
    P = len(boxes) * MASKS
    masks = np.zeros((P, H, W), np.uint8)
    mask_image, labels = np.zeros(P, np.uint32), np.zeros(P, np.int32)
    for b, mine in enumerate(boxes):
        for k in range(MASKS):
            x0, y0, x1, y1, label = mine[int(rng.integers(0, len(mine)))]
            dx, dy = int(rng.integers(-20, 21)), int(rng.integers(-20, 21))
            masks[b * MASKS + k, max(0, y0 + dy):max(0, y1 + dy), max(0, x0 + dx):max(0, x1 + dx)] = 255 if k % 2 else 1
            mask_image[b * MASKS + k], labels[b * MASKS + k] = b, label
    return masks.reshape(P, H * W), mask_image, labels, rng.random(P)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--tool-images", type=int, default=16)
    opt = ap.parse_args()
    B = opt.images
    lines = ["instance2d: median of %d repeats after a warm-up; %s; torch %s" % (REPEATS, torch.cuda.get_device_name(0), torch.__version__), ""]
    rng = np.random.default_rng(1)
    gt, boxes = images(rng, B)
    masks, mask_image, labels, confs = masks_of(rng, boxes)
    P, n = masks.shape
    to = lambda a: torch.from_numpy(a).to("cuda:0")
    dg, dm, di = to(gt.view(np.int16)), to(masks), to(mask_image.view(np.int32))
    verdict = {}

    count, ids, px = ev.image_plan(gt)
    capacity = ids.shape[1]
    lines.append("%d images of %d x %d at 16 bits (%.0f MB), %d .. %d instances each; %d masks (%.0f MB), %.1f %% of their bytes set" % (
        B, W, H, gt.nbytes / 1e6, count.min(), count.max(), P, masks.nbytes / 1e6, 100.0 * np.count_nonzero(masks) / masks.size))
    dcount, dids, dpx = ev.image_plan(dg, capacity=capacity)
    assert np.array_equal(dcount.cpu().numpy().view(np.uint32), count) and np.array_equal(dids.cpu().numpy(), ids) and np.array_equal(dpx.cpu().numpy().view(np.uint32), px)
    table = ev.overlaps_images(gt, count, ids, masks, mask_image)
    assert np.array_equal(ev.overlaps_images(dg, dcount, dids, dm, di).cpu().numpy().view(np.uint32), table)

    lines.append("the plan (ids and pixel counts of every image)")
    cg = torch.empty_like(dg)
    k = device_ms(lambda: ev.image_plan(dg, capacity=capacity))
    c = device_ms(lambda: cg.copy_(dg))
    h = wall(lambda: ev.image_plan(gt, capacity=capacity))
    d = wall(lambda: ev.image_plan(gt, capacity=capacity, device=0))
    lines += [row("  k_eval_image_ids + k_eval_image_compact (with the counters' memset), device-resident", k, gt.nbytes),
              row("  device copy of the images (rate: bytes read)", c, gt.nbytes), row("  host path (at most 16 threads)", h),
              row("  host arrays through the device (copy, count, read back)", d), ""]
    verdict["plan, device-resident kernels against the host path"] = (k, h)
    verdict["plan from host arrays"] = (d, h)
    del cg

    lines.append("the overlaps (a table row per mask)")
    cm = torch.empty_like(dm)
    k_ov = device_ms(lambda: ev.overlaps_images(dg, dcount, dids, dm, di))
    c = device_ms(lambda: cm.copy_(dm))
    del cm
    h_ov = wall(lambda: ev.overlaps_images(gt, count, ids, masks, mask_image))
    d_ov = wall(lambda: ev.overlaps_images(gt, count, ids, masks, mask_image, device=0))
    lines += [row("  k_eval_overlaps_images (with the table's memset), device-resident", k_ov, masks.nbytes), row("  device copy of the masks (rate: bytes read)", c, masks.nbytes),
              row("  host path", h_ov), row("  host arrays through the device", d_ov), ""]
    verdict["overlaps, device-resident kernel against the host path"] = (k_ov, h_ov)
    verdict["overlaps from host arrays"] = (d_ov, h_ov)

    # what the 3-D entry points offer for the same work: a host-made slot image per image, then a launch per image
    lines.append("the per-image composition of the 3-D entry points")
    flat = gt.reshape(B, n).astype(np.int32)
    plans = [None] * B

    def host_plans():
        for b in range(B):
            plans[b] = ev.instance_plan(flat[b])
    hp = wall(host_plans)
    slots = [to(p[2].view(np.int32)) for p in plans]
    per_image = [dm[b * MASKS:(b + 1) * MASKS] for b in range(B)]

    def launches():
        for b in range(B):
            ev.instance_overlaps(slots[b], len(plans[b][0]), per_image[b])
    for b in range(B):
        G = len(plans[b][0])
        got = ev.instance_overlaps(slots[b], G, per_image[b]).cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:, :G], table[b * MASKS:(b + 1) * MASKS, :G]) and np.array_equal(got[:, G + 1], table[b * MASKS:(b + 1) * MASKS, capacity + 1])
    kl = device_ms(launches)
    lines += [row("  sf_eval_instance_plan on the host, %d images (ids, counts and a 4-byte slot image each)" % B, hp),
              row("  %d sf_eval_instance_overlaps_device calls over resident slot images" % B, kl, masks.nbytes), ""]
    verdict["batched overlaps kernel against %d per-image launches (both device-resident)" % B] = (k_ov, kl)
    verdict["device plan against the host plan of the composition"] = (k, hp)
    del slots, per_image, dm, dg

    T = min(opt.tool_images, B)
    work = tempfile.mkdtemp(prefix="instance2d_bench_")
    try:
        pred_path, gt_path = os.path.join(work, "pred"), os.path.join(work, "gt")
        os.makedirs(os.path.join(pred_path, "masks"))
        os.makedirs(gt_path)
        for b in range(T):
            filter2d.png_write_gray(os.path.join(gt_path, "frame%03d.png" % b), gt[b])
            text = ""
            for k in range(MASKS):
                p = b * MASKS + k
                rel = "masks/frame%03d_%02d.png" % (b, k)
                filter2d.png_write_gray(os.path.join(pred_path, rel), masks[p].reshape(H, W))
                text += "%s %d %r\n" % (rel, int(labels[p]), float(confs[p]))
            open(os.path.join(pred_path, "frame%03d.txt" % b), "w").write(text)
        tool = os.path.join(ROOT, "bin", "evaluate")
        lines.append("bin/evaluate instance2d, wall time of the process (%d images of %d x %d with %d masks each, as PNG files)" % (T, W, H, MASKS))
        t, outs = {}, {}
        for how in ("--host", "--device=0"):
            out_file = os.path.join(work, "out" + how.strip("-=0") + ".txt")
            t[how] = wall(lambda: subprocess.run([tool, "instance2d", "--pred_path", pred_path, "--gt_path", gt_path, "--output_file", out_file, how], check=True,
                                                 capture_output=True))
            outs[how] = open(out_file, "rb").read()
            lines.append(row("  instance2d %s" % how, t[how]))
        assert outs["--host"] == outs["--device=0"]
        verdict["bin/evaluate instance2d"] = (t["--device=0"], t["--host"])
    finally:
        shutil.rmtree(work, ignore_errors=True)
    lines += ["", "the standing rule: the device (first figure) is the default only where its slowest repeat beats the other's fastest"]
    for name, (d, h) in verdict.items():
        lines.append("  %-78s max %9.3f ms against min %9.3f ms -> %s" % (name, d[2], h[1], "the first" if d[2] < h[1] else "the second"))
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        open(opt.out, "w").write(text)


if __name__ == "__main__":
    main()
