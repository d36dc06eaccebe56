#!/usr/bin/env python3
"""Whole-call time of sf_fuser_align_device: the furnished room, 640 x 480, K = 64 keyframes 10 cm apart at level 1 with the default pair list,
their poses drifted k x (2 mm, 1 mrad) so that the solver has something to do.  One warm-up call, then 7 timed calls: min / median / max.

    python tools/align_bench.py                  # the table below, on stdout
    python tools/align_bench.py --profile DIR    # the same command under rocprofv3 --kernel-trace --stats (a run of its own), per-kernel device time appended

The numbers in profiles/align.txt are this tool's output (DESIGN.md "Global alignment").
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, K, STEP_CM, REPEATS = 640, 480, 64, 10, 7


def drift(pose, dt, rad, axis=(0.3, -0.5, 0.8), tdir=(0.6, 0.64, -0.48)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(rad) * Kx + (1 - np.cos(rad)) * Kx @ Kx
    out = np.eye(4)
    out[:3, :3] = R @ pose[:3, :3].astype(np.float64)
    out[:3, 3] = R @ pose[:3, 3].astype(np.float64) + dt * np.asarray(tdir, np.float64) / np.linalg.norm(tdir)
    return out.astype(np.float32)


def run(calls):
    import torch
    from scannet_amd import fusion, synth
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, voxel_size=0.004, fx=fx, fy=fy, mx=mx, my=my)
    with fusion.Fuser(gp, device=0) as f:
        d = torch.zeros((K, H * W), dtype=torch.int16, device="cuda:0")
        truth = synth.render_scan_device(d.data_ptr(), W * H * 2, 0, K, 1200 // STEP_CM, W, H)   # the 12 m walk in 120 frames: 10 cm per frame
        torch.cuda.synchronize()
        start = np.stack([drift(t.reshape(4, 4), 0.002 * k, 0.001 * k) if k else t.reshape(4, 4) for k, t in enumerate(truth)]).astype(np.float32)
        a = fusion.default_align_params()
        pairs, count = fusion.align_pairs(start, a)
        assert count == len(pairs), (count, len(pairs))
        times, res, out = [], None, None
        for i in range(calls + 1):   # the first call allocates the work buffers: warm-up
            t0 = time.perf_counter()
            out, res = f.align_device(d, W * H * 2, start, pairs, a)
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        err0 = max(float(np.linalg.norm(s.reshape(4, 4)[:3, 3] - t.reshape(4, 4)[:3, 3])) for s, t in zip(start, truth))
        err1 = max(float(np.linalg.norm(o.reshape(4, 4)[:3, 3] - t.reshape(4, 4)[:3, 3])) for o, t in zip(out, truth))
    t = sorted(times)
    print("sf_fuser_align_device: furnished room, %d x %d, K = %d keyframes %d cm apart, level %d (%d x %d), %d pairs" % (W, H, K, STEP_CM, a.level, W >> a.level, H >> a.level, len(pairs)))
    print("whole call, %d calls after a warm-up: min %.2f ms, median %.2f ms, max %.2f ms" % (len(t), t[0], t[len(t) // 2], t[-1]))
    print("iterations %d, pairs in the last system %d, correspondences %d, rms %.5f -> %.5f m, status %d, unconnected %d, rejected %d" % (
        res.iterations, res.pairs_used, res.correspondences, res.rms_first, res.rms_last, res.status, res.frames_unconnected, res.frames_rejected))
    print("per iteration: %.2f ms (median call / iterations, preparation included)" % (t[len(t) // 2] / max(1, res.iterations)))
    print("worst keyframe translation error: %.1f mm at the start, %.1f mm after" % (err0 * 1e3, err1 * 1e3))


def profile(outdir):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__), "--calls", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print("rocprofv3 failed (%d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        return r.returncode
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    print("per-kernel device time (rocprofv3 --kernel-trace --stats, a run of its own: warm-up + 1 call):")
    for row in rows:
        name = row.get("Name", "")
        if "k_align" in name or "k_synth" in name:
            print("  %-60s calls %6s  total %10.1f us  average %9.1f us" % (name[:60], row.get("Calls"), float(row.get("TotalDurationNs", 0)) / 1e3,
                                                                            float(row.get("AverageNs", 0)) / 1e3))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=REPEATS)
    ap.add_argument("--profile", metavar="DIR")
    args = ap.parse_args()
    if args.profile:
        sys.exit(profile(args.profile))
    run(args.calls)
