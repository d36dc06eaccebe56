"""Re-integration cost: 32 corrected frames of the configs[1] stream (640x480 RGB-D, 4 mm voxels, the furnished room of
bench.py) in a volume built from 400 frames, re-integrated
  (a) by ONE sf_fuser_reintegrate_batch_device call (two mixed-sign passes of 16 frames), and
  (b) by the 64 single device calls that do the same without it: sf_fuser_deintegrate_device + sf_fuser_integrate_device per frame,
on the same frames and poses.  The corrected frames are every 12th of the 400; the volume holds them about 1 degree / 3 cm off (seeded).  Every repeat
starts from the same volume (reset, fuse the 400 frames, synchronise) and is timed by the wall clock between two synchronisations; one warm-up of each
way, then the repeats alternate.  Both ways leave the same volume: the blocks of the two are compared once, untimed.

    python tools/reintegrate_bench.py [--repeats 5] [--frames 400] [--fixes 32] [--once a|b]

One JSON line per way and a summary line on stdout.  --once runs a single untimed-by-us pass of one way (for a profiler around the process).
No gate: bench.py is the project's yardstick, this is the record behind the DESIGN.md / README figures.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scannet_amd import fusion, synth  # noqa: E402

W, H, TOTAL = 640, 480, 5578


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def perturbed(pose, rng):
    p = np.array(pose, np.float64).reshape(4, 4)
    q = p.copy()
    q[:3, :3] = rot(rng.normal(size=3), np.deg2rad(1.0)) @ p[:3, :3]
    q[:3, 3] = p[:3, 3] + rng.normal(size=3) * 0.03 / np.sqrt(3)
    return q.astype(np.float32).reshape(16)


def colour_tensor(torch, n):
    """bench.py's synthetic RGB frame per depth frame (gradients that move with the frame index under a per-pixel texture)."""
    yy = torch.arange(H, device="cuda", dtype=torch.int32).view(1, H, 1)
    xx = torch.arange(W, device="cuda", dtype=torch.int32).view(1, 1, W)
    tex = ((xx * 7919 + yy * 104729) >> 3) & 31
    k = torch.arange(0, n, device="cuda", dtype=torch.int32).view(-1, 1, 1)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    out[..., 0] = ((xx * 255 // W + 5 * k + tex) % 256).to(torch.uint8)
    out[..., 1] = ((yy * 255 // H + 3 * k + tex) % 256).to(torch.uint8)
    out[..., 2] = ((xx + yy + 7 * k + tex) % 256).to(torch.uint8)
    out[:, : H // 8] = 0
    out[:, H // 2: H // 2 + H // 16, : W // 3] = 255
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--fixes", type=int, default=32)
    ap.add_argument("--once", choices=["a", "b"], default=None)
    args = ap.parse_args()
    import torch
    n, m = args.frames, args.fixes
    stride, cstride = W * H * 2, W * H * 3
    frames = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    true = np.ascontiguousarray(synth.render_scan_device(frames.data_ptr(), stride, 0, n, TOTAL, W, H, noise=2, scene=1, seed=0), np.float32).reshape(n, 16)
    rgb = colour_tensor(torch, n)
    pick = np.arange(m) * (n // m)
    rng = np.random.default_rng(7)
    held = true.copy()
    for k in pick:
        held[k] = perturbed(true[k], rng)
    sub_d = frames[torch.as_tensor(pick, device="cuda")].contiguous()
    sub_c = rgb[torch.as_tensor(pick, device="cuda")].contiguous()
    torch.cuda.synchronize()
    old, new = np.ascontiguousarray(held[pick]), np.ascontiguousarray(true[pick])
    p = fusion.default_params()   # configs[1]: 4 mm, 2^19 buckets, 2^20 blocks

    def build(f):
        f.reset()
        f.integrate_batch_device(frames.data_ptr(), stride, held, rgb.data_ptr(), cstride)
        f.sync()
        torch.cuda.synchronize()

    def way_a(f):
        f.reintegrate_batch_device(sub_d.data_ptr(), stride, old, new, d_rgb=sub_c.data_ptr(), rgb_stride_bytes=cstride)

    def way_b(f):
        for k in range(m):
            f.deintegrate_device(sub_d[k].data_ptr(), old[k], d_rgb=sub_c[k].data_ptr())
            f.integrate_device(sub_d[k].data_ptr(), new[k], d_rgb=sub_c[k].data_ptr())

    def timed(f, way):
        build(f)
        t0s = f.stats()
        t0 = time.perf_counter()
        way(f)
        f.sync()
        dt = time.perf_counter() - t0
        t1s = f.stats()
        return dt, t1s["total_pass_tiles"] - t0s["total_pass_tiles"], t1s["total_frame_blocks"] - t0s["total_frame_blocks"]

    with fusion.Fuser(p, device=0) as f:
        if args.once:
            build(f)
            (way_a if args.once == "a" else way_b)(f)
            f.sync()
            print(json.dumps({"once": args.once, "fixes": m}))
            return
        # the same volume either way (untimed; also the warm-up of each)
        timed(f, way_a)
        ca, va = f.export_blocks()
        timed(f, way_b)
        cb, vb = f.export_blocks()
        same = bool(np.array_equal(ca, cb) and np.array_equal(va.view(np.uint8), vb.view(np.uint8)))
        ta, tb, tiles_a, tiles_b, blocks = [], [], 0, 0, 0
        for _ in range(args.repeats):
            dt, tiles_a, blocks = timed(f, way_a)
            ta.append(dt)
            dt, tiles_b, _ = timed(f, way_b)
            tb.append(dt)

    def line(name, t, tiles):
        t = sorted(t)
        return {"way": name, "fixes": m, "repeats": len(t), "ms_min": round(t[0] * 1e3, 3), "ms_median": round(t[len(t) // 2] * 1e3, 3), "ms_max": round(t[-1] * 1e3, 3),
                "frames_per_s_median": round(m / t[len(t) // 2], 1), "total_pass_tiles": int(tiles)}
    print(json.dumps(line("a: sf_fuser_reintegrate_batch_device", ta, tiles_a)), flush=True)
    print(json.dumps(line("b: 64 single device calls", tb, tiles_b)), flush=True)
    print(json.dumps({"same_volume": same, "blocks_in_volume": int(len(ca)), "sum_of_blocks_per_operation": int(blocks),
                      "a_slowest_faster_than_b_fastest": bool(max(ta) < min(tb)), "speedup_median": round(sorted(tb)[len(tb) // 2] / sorted(ta)[len(ta) // 2], 2),
                      "speedup_worst_case": round(min(tb) / max(ta), 2), "tiles_ratio_b_over_a": round(tiles_b / max(1, tiles_a), 2)}), flush=True)


if __name__ == "__main__":
    main()
