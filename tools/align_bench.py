#!/usr/bin/env python3
"""Whole-call time of sf_fuser_align_device: the furnished room, 640 x 480, K = 64 keyframes 10 cm apart at level 1 with the default pair list,
their poses drifted k x (2 mm, 1 mrad) so that the solver has something to do.  One warm-up call, then 7 timed calls: min / median / max.

    python tools/align_bench.py                  # the table below, on stdout
    python tools/align_bench.py --profile DIR    # the same command under rocprofv3 --kernel-trace --stats (a run of its own), per-kernel device time appended
    python tools/align_bench.py --colour         # the depth-only call, then sf_fuser_align_rgbd_device with the colour term on the same frames, poses and pairs
                                                 # (a sinusoid texture painted on by world position); --profile DIR goes with it
    python tools/align_bench.py --scan           # sf_fuser_align_scan_device on the 558 keyframes of the 5 578-frame walk (stride 10) against the same groups
                                                 # and top solved through one sf_fuser_align_device call each; --profile DIR goes with it

The numbers in profiles/align.txt and, with --colour, profiles/align_colour.txt are this tool's output (DESIGN.md "Global alignment", 4e and 4f); with
--scan, profiles/align_scan.txt.
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


def paint(depth, pose, fx, fy, mx, my):
    """RGB8 [H*W*3] of one frame: a sum of sinusoids at each pixel's world position (wavelengths of 16 .. 64 level-1 pixels at 2.5 m)."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = depth.reshape(H, W).astype(np.float64) / 1000.0
    cam = np.stack([(xx - mx) / fx * d, (yy - my) / fy * d, d], -1)
    p = np.asarray(pose, np.float64).reshape(4, 4)
    wp = cam @ p[:3, :3].T + p[:3, 3]
    X, Y = wp[..., 0] + 0.7 * wp[..., 2], wp[..., 1] - 0.7 * wp[..., 2]
    foot = 2.5 / (fx / 2)
    out = []
    for amps in ((0.06, 0.10, 0.12, 0.12), (0.05, 0.12, 0.10, 0.14), (0.10, 0.06, 0.14, 0.08)):
        v = np.full(X.shape, 0.5)
        for (lam, th, ph), a in zip(((16.0, 0.3, 0.0), (24.0, 1.9, 1.0), (40.0, 2.6, 2.0), (64.0, 1.1, 4.0)), amps):
            v = v + a * np.sin(2 * np.pi * (X * np.cos(th) + Y * np.sin(th)) / (lam * foot) + ph)
        out.append(v)
    return np.clip(np.rint(np.stack(out, -1) * 255.0), 0, 255).astype(np.uint8).reshape(-1)


def run(calls, colour=False):
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
        if colour:
            host = d.cpu().numpy().view(np.uint16)
            c = torch.from_numpy(np.stack([paint(host[k], truth[k], fx, fy, mx, my) for k in range(K)])).to("cuda:0")
            torch.cuda.synchronize()
            ac = fusion.default_align_params(colour_weight=fusion.ALIGN_COLOUR_WEIGHT)
            ctimes = []
            for i in range(calls + 1):
                t0 = time.perf_counter()
                cout, cres = f.align_device(d, W * H * 2, start, pairs, ac, d_rgb=c, rgb_stride_bytes=W * H * 3)
                if i:
                    ctimes.append((time.perf_counter() - t0) * 1e3)
        err0 = max(float(np.linalg.norm(s.reshape(4, 4)[:3, 3] - t.reshape(4, 4)[:3, 3])) for s, t in zip(start, truth))
        err1 = max(float(np.linalg.norm(o.reshape(4, 4)[:3, 3] - t.reshape(4, 4)[:3, 3])) for o, t in zip(out, truth))
    t = sorted(times)
    print("sf_fuser_align_device: furnished room, %d x %d, K = %d keyframes %d cm apart, level %d (%d x %d), %d pairs" % (W, H, K, STEP_CM, a.level, W >> a.level, H >> a.level, len(pairs)))
    print("whole call, %d calls after a warm-up: min %.2f ms, median %.2f ms, max %.2f ms" % (len(t), t[0], t[len(t) // 2], t[-1]))
    print("iterations %d, pairs in the last system %d, correspondences %d, rms %.5f -> %.5f m, status %d, unconnected %d, rejected %d" % (
        res.iterations, res.pairs_used, res.correspondences, res.rms_first, res.rms_last, res.status, res.frames_unconnected, res.frames_rejected))
    print("per iteration: %.2f ms (median call / iterations, preparation included)" % (t[len(t) // 2] / max(1, res.iterations)))
    print("worst keyframe translation error: %.1f mm at the start, %.1f mm after" % (err0 * 1e3, err1 * 1e3))
    if colour:
        ct = sorted(ctimes)
        errc = max(float(np.linalg.norm(o.reshape(4, 4)[:3, 3] - t.reshape(4, 4)[:3, 3])) for o, t in zip(cout, truth))
        print("sf_fuser_align_rgbd_device: the same frames, poses and pairs with %d x %d pictures, colour_weight %g" % (W, H, ac.colour_weight))
        print("whole call, %d calls after a warm-up: min %.2f ms, median %.2f ms, max %.2f ms" % (len(ct), ct[0], ct[len(ct) // 2], ct[-1]))
        print("iterations %d, pairs in the last system %d, correspondences %d (%d with a colour row), rms %.5f -> %.5f m, colour rms %.5f -> %.5f, status %d, "
              "unconnected %d, rejected %d" % (cres.iterations, cres.pairs_used, cres.correspondences, cres.colour_correspondences, cres.rms_first, cres.rms_last,
                                               cres.colour_rms_first, cres.colour_rms_last, cres.status, cres.frames_unconnected, cres.frames_rejected))
        print("per iteration: %.2f ms (median call / iterations, preparation included)" % (ct[len(ct) // 2] / max(1, cres.iterations)))
        print("worst keyframe translation error: %.1f mm after" % (errc * 1e3))


SCAN_FRAMES, SCAN_STRIDE = 5578, 10


def scan_input():
    """The 558 keyframes in HBM and their drifted poses: keyframe k stands for frame 10 k of the 5 578-frame walk -> (fuser parameters, tensor, start [K,16])."""
    import torch
    from scannet_amd import fusion, synth
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, voxel_size=0.004, fx=fx, fy=fy, mx=mx, my=my)
    KS = (SCAN_FRAMES + SCAN_STRIDE - 1) // SCAN_STRIDE
    d = torch.zeros((KS, H * W), dtype=torch.int16, device="cuda:0")
    truth = synth.render_scan_device(d.data_ptr(), W * H * 2, 0, KS, KS, W, H)
    torch.cuda.synchronize()
    start = np.stack([drift(t.reshape(4, 4), 0.0005 * k, 0.00025 * k) if k else t.reshape(4, 4) for k, t in enumerate(truth)]).astype(np.float32).reshape(KS, 16)
    return gp, d, start


def run_scan_batched(calls):
    """The batched call alone, for the kernel trace: a warm-up and `calls` calls."""
    from scannet_amd import fusion
    gp, d, start = scan_input()
    with fusion.Fuser(gp, device=0) as f:
        for i in range(calls + 1):
            t0 = time.perf_counter()
            out, res = f.align_scan_device(d, W * H * 2, start)
            print("call %d: %.2f ms, %s" % (i, (time.perf_counter() - t0) * 1e3, res.as_dict()))
    return 0


def run_scan(calls):
    """The batched scan call against the only way the solver could do the same before it: one sf_fuser_align_device call per group and one for the top,
    the corrections carried down by sf_align_spread.  Both run in this process, alternating."""
    from scannet_amd import fusion
    gp, d, start = scan_input()
    KS = len(start)
    with fusion.Fuser(gp, device=0) as f:
        a, sp = fusion.default_align_params(), fusion.default_align_scan_params()
        plan = fusion.align_scan_plan(start, a, sp)
        first, members, top = plan["group_first"], plan["members"], plan["top"]
        groups = [members[first[g]:first[g + 1]] for g in range(len(first) - 1)]
        gpairs = [fusion.align_pairs(start[g], a)[0] for g in groups]
        tpairs = fusion.align_pairs(start[top], a)[0]
        stride = W * H * 2

        def per_group():
            out = start.copy()
            solved = []
            for g, pairs in zip(groups, gpairs):
                step = int(g[1] - g[0]) if len(g) > 1 else 1
                assert len(g) < 2 or (np.diff(g) == step).all()
                solved.append(f.align_device(d.data_ptr() + int(g[0]) * stride, step * stride, start[g], pairs, a)[0] if len(g) > 1 else start[g].copy())
            step = int(top[1] - top[0])
            assert (np.diff(top) == step).all()
            out[top], tres = f.align_device(d.data_ptr() + int(top[0]) * stride, step * stride, start[top], tpairs, a)
            for lv in range(plan["levels"] - 1, -1, -1):
                for k, g in enumerate(groups):
                    if plan["group_level"][k] == lv and len(g) > 1:
                        out[g[1:]] = fusion.align_spread(solved[k], np.zeros(1, np.uint64), out[g[:1]])[1:]
            return out, tres

        bt, pt, res, out, ref = [], [], None, None, None
        for i in range(calls + 1):   # the first round allocates the work buffers: warm-up
            t0 = time.perf_counter()
            out, res = f.align_scan_device(d, stride, start, a, sp)
            t1 = time.perf_counter()
            ref, tres = per_group()
            t2 = time.perf_counter()
            if i:
                bt.append((t1 - t0) * 1e3)
                pt.append((t2 - t1) * 1e3)
        same = out.tobytes() == ref.tobytes()
    b, p = sorted(bt), sorted(pt)
    print("sf_fuser_align_scan_device: furnished room, %d x %d, %d keyframes (every %d-th of %d frames), level %d (%d x %d), group_size %d, top_frames %d" % (
        W, H, KS, SCAN_STRIDE, SCAN_FRAMES, a.level, W >> a.level, H >> a.level, sp.group_size, sp.top_frames))
    print("levels %d, groups %d (status 0 / 1 / 2: %s), pairs per iteration %d in the groups and %d in the top of %d, iterations at most %d (top %d)" % (
        res.levels, res.groups, list(res.groups_status), sum(len(x) for x in gpairs), len(tpairs), len(top), res.max_iterations, res.top.iterations))
    print("batched call, %d calls after a warm-up: min %.2f ms, median %.2f ms, max %.2f ms" % (len(b), b[0], b[len(b) // 2], b[-1]))
    print("one sf_fuser_align_device call per group and for the top (%d calls), alternating with it: min %.2f ms, median %.2f ms, max %.2f ms" % (
        sum(len(g) > 1 for g in groups) + 1, p[0], p[len(p) // 2], p[-1]))
    print("slowest batched repeat / fastest per-group repeat: %.3f; identical poses: %s" % (b[-1] / p[0], same))
    print("unconnected %d, rejected %d, correspondences %d; top: status %d, rms %.5f -> %.5f m" % (
        res.frames_unconnected, res.frames_rejected, res.correspondences, res.top.status, res.top.rms_first, res.top.rms_last))
    return 0 if same else 1


def profile(outdir, colour=False, scan=False):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__), "--calls", "1"]
    if colour:
        cmd.append("--colour")
    if scan:
        cmd += ["--scan", "--batched-only"]
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
        if "k_align" in name or "k_photo" in name or "k_synth" in name or "k_group" in name:
            print("  %-60s calls %6s  total %10.1f us  average %9.1f us" % (name[:60], row.get("Calls"), float(row.get("TotalDurationNs", 0)) / 1e3,
                                                                            float(row.get("AverageNs", 0)) / 1e3))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=REPEATS)
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--colour", action="store_true")
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--batched-only", action="store_true", help="--scan without the per-group comparator (the profiled run)")
    args = ap.parse_args()
    if args.profile:
        sys.exit(profile(args.profile, args.colour, args.scan))
    if args.scan:
        sys.exit(run_scan_batched(args.calls) if args.batched_only else run_scan(args.calls))
    run(args.calls, args.colour)
