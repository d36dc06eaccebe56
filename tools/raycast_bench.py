"""Ray-cast throughput (DESIGN.md "Ray casting"): images per second of sf_fuser_raycast_device on the furnished synthetic room fused at 4 mm and at 1 mm,
at 640x480 and 320x240, one pose per call and 32 poses per call.  Depth, normals and colour are all written.  Poses are the fused frames' own.

    python tools/raycast_bench.py [--voxels 4mm,1mm] [--calls 40]

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

VOXELS = {   # fused frames of the walk, total frames of the walk (consecutive frames), table size (bench.py's CONFIGS)
    "4mm": dict(voxel_size=0.004, hash_num_buckets=1 << 19, num_sdf_blocks=1 << 20, frames=400, total=400),
    "1mm": dict(voxel_size=0.001, hash_num_buckets=1 << 22, num_sdf_blocks=1 << 25, frames=128, total=5578),
}


def fuse(torch, cfg, W=640, H=480):
    frames = torch.empty((cfg["frames"], H, W), dtype=torch.uint16, device="cuda:0")
    poses = synth.render_scan_device(frames.data_ptr(), W * H * 2, 0, cfg["frames"], cfg["total"], W, H)
    p = fusion.default_params(voxel_size=cfg["voxel_size"], hash_num_buckets=cfg["hash_num_buckets"], num_sdf_blocks=cfg["num_sdf_blocks"])
    f = fusion.Fuser(p, device=0)
    f.integrate_batch_device(frames.data_ptr(), W * H * 2, poses)
    f.sync()
    del frames
    return f, poses


def measure(torch, f, poses, W, H, n, calls):
    r = fusion.default_raycast_params(width=W, height=H)
    d = torch.empty((n, H, W), dtype=torch.float32, device="cuda:0")
    nr = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda:0")
    c = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    sel = lambda k: poses[(np.arange(n) * 7 + k * n) % len(poses)]   # noqa: E731 -- a different set of fused poses per call
    for k in range(3):
        f.raycast_device(sel(k), d, nr, c, params=r)
    f.sync()
    t0 = time.perf_counter()
    for k in range(calls):
        f.raycast_device(sel(k), d, nr, c, params=r)
    f.sync()
    dt = time.perf_counter() - t0
    hit = float(torch.isfinite(d).float().mean().item())
    return {"images_per_s": round(calls * n / dt, 1), "ms_per_image": round(dt * 1e3 / (calls * n), 4), "calls": calls, "hit_share_last_call": round(hit, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", default="4mm,1mm")
    ap.add_argument("--calls", type=int, default=40)
    args = ap.parse_args()
    import torch
    for name in args.voxels.split(","):
        cfg = VOXELS[name]
        f, poses = fuse(torch, cfg)
        blocks = f.stats()["blocks_allocated"]
        for W, H in ((640, 480), (320, 240)):
            for n in (1, 32):
                calls = args.calls if n == 32 else args.calls * 8
                out = {"voxel": name, "blocks": blocks, "fused_frames": cfg["frames"], "width": W, "height": H, "poses_per_call": n}
                out.update(measure(torch, f, poses, W, H, n, calls))
                print(json.dumps(out), flush=True)
        f.close()


if __name__ == "__main__":
    main()
