"""Camera-tracking throughput (DESIGN.md "Camera tracking"): frames per second of sf_fuser_track_device on the furnished synthetic room at 4 mm, at
320x240 and 640x480, for tracking alone (each frame tracked from the previous frame's true pose against a volume of the first frames) and for the
track-and-fuse loop (each frame tracked from the last tracked pose and fused there).  Default tracking parameters; the walk moves 1 cm per frame.

    python tools/track_bench.py [--frames 60] [--sizes 320x240,640x480]

One JSON line per measurement on stdout.  No gate: bench.py is the project's yardstick, this is the record behind the DESIGN.md figure.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scannet_amd import fusion, synth  # noqa: E402

TOTAL = 1200   # frames of the walk's 12 m perimeter: 1 cm per frame
SEED_FRAMES = 20


def err(a, b):
    a, b = np.asarray(a, np.float64).reshape(4, 4), np.asarray(b, np.float64).reshape(4, 4)
    c = (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), float(np.arccos(np.clip(c, -1.0, 1.0)))


def run(torch, W, H, n):
    frames = torch.empty((SEED_FRAMES + n, H, W), dtype=torch.uint16, device="cuda:0")
    poses = synth.render_scan_device(frames.data_ptr(), W * H * 2, 0, SEED_FRAMES + n, TOTAL, W, H)
    torch.cuda.synchronize()
    fx, fy, mx, my = synth.intrinsics(W, H)
    p = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my)
    t = fusion.default_track_params()
    fp = lambda k: frames[k].data_ptr()   # noqa: E731
    out = []
    # track alone: a volume of the first SEED_FRAMES frames, the frames after it tracked from the previous frame's true pose
    with fusion.Fuser(p, device=0) as f:
        f.integrate_batch_device(frames.data_ptr(), W * H * 2, poses[:SEED_FRAMES])
        f.sync()
        f.track_device(fp(SEED_FRAMES), poses[SEED_FRAMES - 1], params=t)   # workspace made
        iters, worst, lost = [], 0.0, 0
        t0 = time.perf_counter()
        for k in range(SEED_FRAMES, SEED_FRAMES + n):
            pose, res = f.track_device(fp(k), poses[k - 1], params=t)
            iters.append(sum(res.iterations))
            if pose is None:
                lost += 1
            else:
                worst = max(worst, err(pose, poses[k])[0])
        dt = time.perf_counter() - t0
        out.append({"mode": "track", "width": W, "height": H, "frames": n, "frames_per_s": round(n / dt, 1), "ms_per_frame": round(dt * 1e3 / n, 3),
                    "iterations_mean": round(float(np.mean(iters)), 2), "lost": lost, "worst_translation_error_m": round(worst, 5)})
    # track + integrate: frame 0 at its true pose, every later frame tracked from the last tracked pose and fused there
    with fusion.Fuser(p, device=0) as f:
        f.integrate_device(fp(0), poses[0])
        f.track_device(fp(1), poses[0], params=t)
        last, iters, worst, lost = poses[0], [], 0.0, 0
        t0 = time.perf_counter()
        for k in range(1, SEED_FRAMES + n):
            pose, res = f.track_device(fp(k), last, params=t)
            iters.append(sum(res.iterations))
            if pose is None:
                lost += 1
                continue
            f.integrate_device(fp(k), pose)
            last = pose
            worst = max(worst, err(pose, poses[k])[0])
        f.sync()
        dt = time.perf_counter() - t0
        m = SEED_FRAMES + n - 1
        out.append({"mode": "track+integrate", "width": W, "height": H, "frames": m, "frames_per_s": round(m / dt, 1), "ms_per_frame": round(dt * 1e3 / m, 3),
                    "iterations_mean": round(float(np.mean(iters)), 2), "lost": lost, "worst_translation_error_m": round(worst, 5)})
    del frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--sizes", default="320x240,640x480")
    args = ap.parse_args()
    import torch
    for s in args.sizes.split(","):
        W, H = (int(x) for x in s.split("x"))
        for line in run(torch, W, H, args.frames):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
