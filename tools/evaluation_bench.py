"""Measures the benchmark's scores on one GPU and prints the table kept in profiles/evaluation.txt: the two counting kernels on
inputs that already sit in device memory, beside a device-to-device copy of the same bytes in the same run; the host path on the same inputs; and
bin/evaluate's three modes with --host and --device=0 on the file cases of tests/evaluation_cases.py.  Every figure is the median of 5 repeats after
one warm-up, with the fastest and the slowest repeat beside it.

    python tools/evaluation_bench.py [--out FILE] [--labels 50000000]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scannet_amd import evaluation as ev, filter2d  # noqa: E402
from tests import evaluation_cases as ec  # noqa: E402

REPEATS = 5


def stats(times):
    t = sorted(times)
    return t[len(t) // 2], t[0], t[-1]


def wall(fn):
    fn()
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def device_ms(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def row(name, s, bytes_read=None):
    rate = "" if bytes_read is None else "  %7.1f GB/s" % (bytes_read / s[0] / 1e6)
    return "%-58s %9.3f ms  (min %9.3f, max %9.3f)%s" % (name, s[0], s[1], s[2], rate)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--labels", type=int, default=50_000_000)
    opt = ap.parse_args()
    lines = ["evaluation: median of %d repeats after a warm-up; %s; torch %s" % (REPEATS, torch.cuda.get_device_name(0), torch.__version__), ""]
    to = lambda a: torch.from_numpy(a).to("cuda:0")
    verdict = {}

    rng = np.random.default_rng(1)
    n = opt.labels
    gt64 = ec.runs(rng, n, ec.ALL_IDS, 40)
    pred64 = np.where(rng.random(n) < 0.2, ec.runs(rng, n, ec.ALL_IDS, 10), gt64)
    lines.append("confusion, 3-D mode, %d labels in runs of about 40" % n)
    for dtype, tdtype in ((np.uint8, None), (np.int16, None), (np.int32, None)):
        gt, pred = gt64.astype(dtype), pred64.astype(dtype)
        dg, dp = to(gt), to(pred)
        cg, cp = torch.empty_like(dg), torch.empty_like(dp)
        counts = ev.confusion(dg, dp)
        assert np.array_equal(counts.numpy()[0], ev.confusion(gt, pred).numpy()[0])
        width = gt.itemsize
        k = device_ms(lambda: ev.confusion(dg, dp, into=counts))
        c = device_ms(lambda: (cg.copy_(dg), cp.copy_(dp)))
        h = wall(lambda: ev.confusion(gt, pred))
        d = wall(lambda: ev.confusion(gt, pred, device=0))
        lines += [row("  %d-byte: k_eval_confusion, device-resident (rate: bytes read)" % width, k, 2 * n * width), row("          device copy of the same bytes (rate: bytes read)", c, 2 * n * width),
                  row("          host path (at most 16 threads)", h), row("          host arrays through the device (copy, count, read back)", d)]
        verdict["confusion %d-byte from host arrays" % width] = (d, h)
        del dg, dp, cg, cp
    lines.append("")

    B = 16
    gt, pred = ec.image_case(2, B, (1296, 968), (1296, 968), np.uint8)
    dg, dp = to(gt), to(pred)
    cg, cp = torch.empty_like(dg), torch.empty_like(dp)
    counts = ev.confusion_images(dg, dp)
    assert np.array_equal(counts.numpy()[0], ev.confusion_images(gt, pred).numpy()[0])
    lines.append("confusion, 2-D mode, %d pairs of 1296 x 968 bytes, resized to 640 x 480 inside the kernel" % B)
    k = device_ms(lambda: ev.confusion_images(dg, dp, into=counts))
    c = device_ms(lambda: (cg.copy_(dg), cp.copy_(dp)))
    h = wall(lambda: ev.confusion_images(gt, pred))
    d = wall(lambda: ev.confusion_images(gt, pred, device=0))
    lines += [row("  k_eval_confusion_images, device-resident", k), row("  device copy of both batches (rate: bytes read)", c, 2 * gt.size), row("  host path", h),
              row("  host arrays through the device", d), ""]
    verdict["images from host arrays"] = (d, h)
    del dg, dp, cg, cp

    nv, G, P = 150_000, 60, 100
    slot = ec.runs(rng, nv, np.arange(G + 1), 1500).astype(np.uint32)
    masks = np.zeros((P, nv), np.uint8)
    for p in range(P):
        a = int(rng.integers(0, nv - 4000))
        masks[p, a:a + int(rng.integers(200, 4000))] = 1
    ds, dm = to(slot.view(np.int32)), to(masks)
    cm = torch.empty_like(dm)
    assert np.array_equal(ev.instance_overlaps(ds, G, dm).cpu().numpy().view(np.uint32), ev.instance_overlaps(slot, G, masks))
    lines.append("overlaps, %d masks over %d vertices, %d instances" % (P, nv, G))
    k = device_ms(lambda: ev.instance_overlaps(ds, G, dm))
    c = device_ms(lambda: cm.copy_(dm))
    h = wall(lambda: ev.instance_overlaps(slot, G, masks))
    d = wall(lambda: ev.instance_overlaps(slot, G, masks, device=0))
    lines += [row("  k_eval_overlaps (with the table's memset), device-resident", k, masks.size), row("  device copy of the masks (rate: bytes read)", c, masks.size), row("  host path", h),
              row("  host arrays through the device", d), ""]
    verdict["overlaps from host arrays"] = (d, h)

    work = tempfile.mkdtemp(prefix="evaluation_bench_")
    label = ec.write_label_dirs(work)[:2]
    inst = ec.write_instance_dirs(work)[:2]
    pix = (os.path.join(work, "pix_pred"), os.path.join(work, "pix_gt"))
    os.makedirs(pix[0])
    os.makedirs(pix[1])
    gt, pred = ec.image_case(50, 8, (1296, 968), (640, 480), np.uint8)
    for i in range(len(gt)):
        filter2d.png_write_gray(os.path.join(pix[1], "%d.png" % i), gt[i])
        filter2d.png_write_gray(os.path.join(pix[0], "%d.png" % i), pred[i])
    tool = os.path.join(ROOT, "bin", "evaluate")
    lines.append("bin/evaluate, wall time of the process (3 scans of 5000 vertices; 3 scans of 6000 vertices with 30 masks; 8 image pairs)")
    for mode, (pp, gp) in (("label3d", label), ("instance3d", inst), ("label2d", pix)):
        t = {}
        for how in ("--host", "--device=0"):
            t[how] = wall(lambda: subprocess.run([tool, mode, "--pred_path", pp, "--gt_path", gp, "--output_file", os.path.join(work, "out.txt"), how], check=True,
                                                 capture_output=True))
            lines.append(row("  %-10s %s" % (mode, how), t[how]))
        verdict["bin/evaluate " + mode] = (t["--device=0"], t["--host"])
    lines += ["", "the standing rule: the device is the default only where its slowest repeat beats the host's fastest"]
    for name, (d, h) in verdict.items():
        lines.append("  %-40s device max %9.3f ms, host min %9.3f ms -> default: %s" % (name, d[2], h[1], "device" if d[2] < h[1] else "host"))
    text = "\n".join(lines) + "\n"
    print(text)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        open(opt.out, "w").write(text)


if __name__ == "__main__":
    main()
