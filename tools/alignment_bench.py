#!/usr/bin/env python3
"""Time per stage of the axis alignment (sf_axis_align_estimate) on a scan-sized mesh, host path against device path.

The mesh is the furnished synthetic room fused on the GPU and extracted by marching cubes, at 1 cm voxels and -- the larger case -- at 5 mm; the
trajectory is the walk that was fused.  Per mesh and path: one warm-up call, then --repeats timed calls; the table shows the median of each stage
and, for the whole call, the median with the spread (min .. max) of the repeats.  The device path's clustering is split into its two kernels by a
further call under sf_axis_align_tune("profile", 1) (HIP events round every launch; that call is not part of the timed repeats).

  python tools/alignment_bench.py [--frames 400] [--repeats 5] [--voxels 0.01 0.005] [--out profiles/alignment.txt]
needs a GPU."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def room_scan(frames, voxel):
    import torch
    from scannet_amd import fusion, synth
    W, H = 640, 480
    dev = torch.empty((frames, H, W), dtype=torch.int16, device="cuda")
    poses = synth.render_scan_device(dev.data_ptr(), W * H * 2, 0, frames, 5578, W, H, noise=2, scene=1, seed=0)
    p = fusion.default_params(voxel_size=voxel)
    with fusion.Fuser(p, device=0) as f:
        f.integrate_batch_device(dev.data_ptr(), W * H * 2, poses)
        mesh = f.extract_mesh()
    del dev
    torch.cuda.empty_cache()
    return mesh, np.asarray(poses, np.float32).reshape(-1, 4, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxels", type=float, nargs="+", default=[0.01, 0.005])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scannet_amd import _abi, alignment, sens
    L = _abi.lib()
    L.sf_axis_align_tune.argtypes = [C.c_char_p, C.c_int]
    lines = ["command: python tools/alignment_bench.py " + " ".join(sys.argv[1:]),
             "sf_axis_align_estimate, reference constants; seconds, median of %d repeats after one warm-up call; whole call: median (min .. max)" % a.repeats, ""]
    for voxel in a.voxels:
        mesh, poses = room_scan(a.frames, voxel)
        k = np.eye(4, dtype=np.float32)
        sd = sens.SensorData.create(4, 4, 4, 4, k, k)
        for i, m in enumerate(poses):
            sd.add_frame(np.zeros((4, 4), np.uint16), camera_to_world=m, timestamp_color=i, timestamp_depth=i)
        nv, nf = mesh.counts()
        results = {}
        for name, device in (("host", -1), ("device", 0)):
            T, st = alignment.estimate(mesh, sd, device=device)   # warm-up
            runs, walls = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                T, st = alignment.estimate(mesh, sd, device=device)
                walls.append(time.perf_counter() - t0)
                runs.append(st)
            results[name] = (T, runs, walls)
        _abi.check(L.sf_axis_align_tune(b"profile", 1))
        _, prof = alignment.estimate(mesh, sd, device=0)
        _abi.check(L.sf_axis_align_tune(b"profile", 0))
        st = results["host"][1][0]
        same = np.array_equal(results["host"][0].view(np.uint32), results["device"][0].view(np.uint32))
        lines.append("voxel %g m, %d frames: mesh %d vertices %d faces; working mesh %d vertices; %d clusters founded, %d after the size filter, %d kept; floor found %d (%d inliers); "
                     "transforms bit-identical: %s" % (voxel, a.frames, nv, nf, st["vertices"], st["clusters_founded"], st["clusters_after_small"], st["clusters_kept"],
                                                       st["floor_found"], st["floor_inliers"], same))
        lines.append("  %-16s %10s %10s" % ("stage", "host", "device"))
        for stage in alignment.SECONDS:
            med = [statistics.median(r["seconds"][stage] for r in results[n][1]) for n in ("host", "device")]
            lines.append("  %-16s %10.4f %10.4f" % (stage, med[0], med[1]))
        lines.append("  %-16s %10s %10.4f   (k_aa_match summed over the batches, HIP events)" % ("  match", "", prof["gpu_seconds_match"]))
        lines.append("  %-16s %10s %10.4f   (k_aa_commit)" % ("  commit", "", prof["gpu_seconds_commit"]))
        for n in ("host", "device"):
            w = results[n][2]
            lines.append("  whole call, %-6s %.4f (%.4f .. %.4f)" % (n, statistics.median(w), min(w), max(w)))
        d = results["device"][1][0]
        lines.append("  device path: %d batches, %d dirty re-evaluations, %d fallback rescans" % (d["gpu_batches"], d["gpu_dirty_evaluations"], d["gpu_fallback_rescans"]))
        lines.append("")
        mesh.close()
        sd.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
