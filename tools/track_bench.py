"""Camera-tracking throughput (DESIGN.md "Camera tracking"): frames per second of sf_fuser_track_device on the furnished synthetic room at 4 mm, at
320x240 and 640x480, for tracking alone (each frame tracked from the previous frame's true pose against a volume of the first frames) and for the
track-and-fuse loop (each frame tracked from the last tracked pose and fused there).  Default tracking parameters; the walk moves 1 cm per frame.

    python tools/track_bench.py [--frames 60] [--sizes 320x240,640x480] [--colour]

--colour: the same walk with a texture painted on by world position, fused with colour, tracked alone by sf_fuser_track_device and by
sf_fuser_track_rgbd_device at fusion.TRACK_COLOUR_WEIGHT, one after the other on the same fuser in the same run; the time of an iteration (launches,
kernels, the read-back and the host's solve) is the slope between a run at the default iteration counts and a run at one iteration per level.  The lines
go to stdout and, with a header, to profiles/track_colour.txt.

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


def paint(depth, pose, W, H):
    """RGB8 [H, W, 3]: three sinusoids of the pixel's world position, 0.3 m to 0.8 m long, so that walls, floor and furniture all carry a gradient."""
    fx, fy, mx, my = synth.intrinsics(W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    d = depth.astype(np.float64) / 1000.0
    cam = np.stack([(xx - mx) / fx * d, (yy - my) / fy * d, d], -1)
    p = np.asarray(pose, np.float64).reshape(4, 4)
    wp = cam @ p[:3, :3].T + p[:3, 3]
    a, b = wp[..., 0] + 0.7 * wp[..., 2], wp[..., 1] - 0.7 * wp[..., 2]
    ch = [0.5 + 0.2 * np.sin(2 * np.pi * a / lam + ph) + 0.2 * np.sin(2 * np.pi * b / (1.3 * lam) + 2 * ph) for lam, ph in ((0.3, 0.0), (0.5, 1.0), (0.8, 2.0))]
    return np.clip(np.rint(np.stack(ch, -1) * 255.0), 0, 255).astype(np.uint8)


def run_colour(torch, W, H, n):
    frames = torch.empty((SEED_FRAMES + n, H, W), dtype=torch.uint16, device="cuda:0")
    poses = synth.render_scan_device(frames.data_ptr(), W * H * 2, 0, SEED_FRAMES + n, TOTAL, W, H)
    torch.cuda.synchronize()
    host = frames.cpu().numpy()
    pics = torch.from_numpy(np.stack([paint(host[k], poses[k], W, H) for k in range(SEED_FRAMES + n)])).to("cuda:0")
    torch.cuda.synchronize()
    fx, fy, mx, my = synth.intrinsics(W, H)
    p = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my)
    out = []
    with fusion.Fuser(p, device=0) as f:
        for k in range(SEED_FRAMES):
            f.integrate_device(frames[k].data_ptr(), poses[k], d_rgb=pics[k].data_ptr())
        f.sync()
        for mode, weight in (("track", None), ("track_rgbd", fusion.TRACK_COLOUR_WEIGHT)):
            ms = {}
            for name, over in (("default", {}), ("one_iteration", dict(max_iters=[1, 1, 1, 1]))):
                t = fusion.default_track_params(**over)
                if weight is not None:
                    t.colour_weight = weight
                rgb = (lambda k: pics[k].data_ptr()) if weight is not None else (lambda k: None)
                f.track_device(frames[SEED_FRAMES].data_ptr(), poses[SEED_FRAMES - 1], params=t, d_rgb=rgb(SEED_FRAMES))   # workspace made
                iters, worst, lost, ccorr = [], 0.0, 0, []
                t0 = time.perf_counter()
                for k in range(SEED_FRAMES, SEED_FRAMES + n):
                    pose, res = f.track_device(frames[k].data_ptr(), poses[k - 1], params=t, d_rgb=rgb(k))
                    iters.append(sum(res.iterations))
                    ccorr.append(res.colour_correspondences)
                    if pose is None:
                        lost += 1
                    else:
                        worst = max(worst, err(pose, poses[k])[0])
                dt = time.perf_counter() - t0
                ms[name] = (dt * 1e3 / n, float(np.mean(iters)))
                if name == "default":
                    line = {"mode": mode, "width": W, "height": H, "frames": n, "frames_per_s": round(n / dt, 1), "ms_per_frame": round(dt * 1e3 / n, 3),
                            "iterations_mean": round(float(np.mean(iters)), 2), "lost": lost, "worst_translation_error_m": round(worst, 5),
                            "colour_correspondences_mean": round(float(np.mean(ccorr)), 1)}
            (ma, ia), (mb, ib) = ms["default"], ms["one_iteration"]
            line["us_per_iteration"] = round((ma - mb) / max(ia - ib, 1e-9) * 1e3, 2)
            line["ms_per_frame_outside_iterations"] = round(mb - ib * (ma - mb) / max(ia - ib, 1e-9), 3)
            out.append(line)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--sizes", default="320x240,640x480")
    ap.add_argument("--colour", action="store_true")
    args = ap.parse_args()
    import torch
    if args.colour:
        lines = []
        for s in args.sizes.split(","):
            W, H = (int(x) for x in s.split("x"))
            for line in run_colour(torch, W, H, args.frames):
                print(json.dumps(line), flush=True)
                lines.append(json.dumps(line))
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "track_colour.txt")
        with open(path, "w") as fh:
            fh.write("# tools/track_bench.py --colour --frames %d --sizes %s on %s: the furnished room at 4 mm with a painted texture, 1 cm per frame,\n"
                     "# tracking alone, depth only (track) and with the colour term at weight %g (track_rgbd), same fuser, same run (DESIGN.md 4g).\n"
                     "# us_per_iteration: the slope between the default iteration counts and one iteration per level (launches, kernels, read-back, solve).\n"
                     % (args.frames, args.sizes, torch.cuda.get_device_name(0), fusion.TRACK_COLOUR_WEIGHT))
            fh.write("\n".join(lines) + "\n")
        return
    for s in args.sizes.split(","):
        W, H = (int(x) for x in s.split("x"))
        for line in run(torch, W, H, args.frames):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
