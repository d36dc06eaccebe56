#!/usr/bin/env python3
"""Times of the free-space stage on the benchmark's scan: the 5 578-frame 640 x 480 walk through the furnished room (hashed noise),
written as a .sens by this library, at 5 cm and at 2 cm voxels.

  (a) the stage end to end (sf_freespace_sens on the opened file): frames per second, and the seconds of each step
  (b) sf_fuser_allocate_box against importing the same box of zero blocks through sf_fuser_import_blocks (4 KiB of host zeros per block), on an empty volume
  (c) k_export_dense over the box of the known voxels (task volume + weights, device destination): bytes read + bytes written over the kernel time (HIP
      events around the launch), beside the HBM peak and beside a plain device copy that moves the same number of bytes, timed in the same run
  (d) the device time sf_fuse_run's allocation kernels take in the stage, where every block they look for exists already: from a run of bin/freespace of
      its own under rocprofv3 --kernel-trace --stats (skipped with --no-trace)

One warm-up, then --repeats timed runs of each; median with min .. max.

  python tools/freespace_bench.py [--frames 5578] [--repeats 5] [--voxels 0.05 0.02] [--out profiles/freespace.txt] [--work DIR] [--no-trace]
needs a GPU."""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12     # bytes per second, MI355X
W, H = 640, 480


def med(v, fmt="%.3f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (statistics.median(v), min(v), max(v))


def say(msg):
    print(msg, file=sys.stderr, flush=True)


def write_scan(path, n):
    """The benchmark's stream (bench.py: scene 1, noise 2) rendered on the device and written with this library's writer."""
    import torch
    from scannet_amd import sens, synth
    frames = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    poses = synth.render_scan_device(frames.data_ptr(), W * H * 2, 0, n, n, W, H, noise=synth.NOISE_DEFAULT, scene=synth.SCENE_DEFAULT, seed=0)
    host = frames.cpu().numpy().view(np.uint16)
    del frames
    torch.cuda.empty_cache()
    K = synth.intrinsic_matrix(W, H)
    sd = sens.SensorData.create(0, 0, W, H, K, K, depth_compression=1, sensor_name="StructureSensor")
    sd.add_depth_frames(host, np.asarray(poses, np.float32).reshape(-1, 4, 4))
    sd.save(path)
    sd.close()


def trace(tool, scan, voxel, work):
    """bin/freespace under rocprofv3 --kernel-trace --stats, a run of its own -> (device seconds by kernel-name prefix, the stage's own seconds line)."""
    out = os.path.join(work, "trace_%g" % voxel)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", tool, scan, "-o", os.path.join(work, "traced.grid"),
           "--voxel=%g" % voxel, "--print-stats"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, "rocprofv3 failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-500:].replace("\n", " | "))
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    tot = {}
    for row in rows:
        name = row.get("Name", "")
        key = next((k for k in ("k_alloc_box", "k_alloc", "k_integrate", "k_prepass", "k_compactify", "k_inflate", "k_export_dense", "k_known_bounds") if k in name), "other")
        tot[key] = tot.get(key, 0.0) + float(row.get("TotalDurationNs", 0)) / 1e9
    seconds = [ln for ln in r.stdout.splitlines() if ln.startswith("seconds:")]
    return tot, seconds[0] if seconds else ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5578)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxels", type=float, nargs="+", default=[0.05, 0.02])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freespace.txt"))
    ap.add_argument("--work", default=None)
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    import torch
    from scannet_amd import _abi, freespace, fusion, sens
    if not torch.cuda.is_available():
        raise SystemExit("tools/freespace_bench.py needs a GPU: nothing here is measured without one")
    L = _abi.lib()
    work = a.work or tempfile.mkdtemp(prefix="freespace_bench_")
    os.makedirs(work, exist_ok=True)
    scan = os.path.join(work, "scan.sens")
    t0 = time.perf_counter()
    write_scan(scan, a.frames)
    say("scan written in %.1f s (%.0f MB)" % (time.perf_counter() - t0, os.path.getsize(scan) / 1e6))
    sd = sens.SensorData(scan)
    lines = ["free-space stage: %d frames of %d x %d (furnished room, hashed noise), .sens of %.0f MB; one warm-up, %d repeats, median (min .. max)" % (
        a.frames, W, H, os.path.getsize(scan) / 1e6, a.repeats), "device: %s; host threads: %d" % (torch.cuda.get_device_name(0), _abi.usable_cpus()), ""]
    for voxel in a.voxels:
        fp = freespace.default_params(voxel_size=voxel)
        sp, lo_b, hi_b = freespace.plan(sd, fp)
        nblk = int(np.prod(hi_b.astype(np.int64) - lo_b + 1))
        lines += ["=== voxel %g m: box of blocks %s .. %s = %d blocks (%.2f GiB of voxels), heap %d, table %d x %d" % (
            voxel, [int(v) for v in lo_b], [int(v) for v in hi_b], nblk, nblk * 4096 / 2 ** 30, sp.num_sdf_blocks, sp.hash_num_buckets, sp.hash_bucket_size), ""]

        # (a) the stage end to end
        runs = []
        for r in range(a.repeats + 1):
            grid, st = freespace.carve_sens(sd, fp, stats=True)
            say("voxel %g stage run %d: %.3f s" % (voxel, r, st["seconds_total"]))
            if r:
                runs.append(st)
        lines += ["(a) sf_freespace_sens, the file open: %d frames used, grid %d x %d x %d, %d known voxels (%d free, %d near)" % (
            st["frames_used"], grid.value.shape[2], grid.value.shape[1], grid.value.shape[0], st["known"], st["free_voxels"], st["near_voxels"]),
            "    frames per second, end to end: %s" % med([s["frames_used"] / s["seconds_total"] for s in runs], "%.0f"),
            "    frames per second of the sf_fuse_run step alone: %s" % med([s["frames_used"] / s["seconds_fuse"] for s in runs], "%.0f")]
        for k in ("plan", "create", "allocate", "fuse", "bounds", "export", "total"):
            lines.append("    seconds %-9s %s" % (k, med([s["seconds_" + k] for s in runs], "%.4f")))
        lines.append("")
        del grid

        # (b) allocate_box against an import of zero blocks, each on an empty volume
        g = np.meshgrid(*(np.arange(lo_b[k], hi_b[k] + 1, dtype=np.int32) for k in range(3)), indexing="ij")
        coords = np.ascontiguousarray(np.stack([v.reshape(-1) for v in g], 1))
        zeros = np.zeros((nblk, 4096), np.uint8)
        t_alloc, t_import = [], []
        with fusion.Fuser(sp) as f:
            for r in range(a.repeats + 1):
                f.reset()
                t0 = time.perf_counter()
                made = f.allocate_box(lo_b, hi_b)
                t1 = time.perf_counter() - t0
                assert made == nblk
                f.reset()
                t0 = time.perf_counter()
                f.import_blocks(coords, zeros, ghost=False)
                t2 = time.perf_counter() - t0
                assert f.stats()["blocks_allocated"] == nblk
                if r:
                    t_alloc.append(t1)
                    t_import.append(t2)
            lines += ["(b) the box on an empty volume, wall seconds of the call (both end in a device synchronise)",
                      "    sf_fuser_allocate_box:                        %s" % med(t_alloc, "%.5f"),
                      "    sf_fuser_import_blocks of %d zero blocks: %s   (%.2f GB of host zeros)" % (nblk, med(t_import, "%.5f"), nblk * 4096 / 1e9),
                      "    ratio import / allocate_box (medians): %.0f x" % (statistics.median(t_import) / statistics.median(t_alloc)), ""]
            del zeros, coords

            # (c) k_export_dense over the box of the known voxels, on the fused volume
            f.reset()
            f.allocate_box(lo_b, hi_b)
            f.run(sd, decode_threads=4)
            lo, hi, known = f.known_bounds()
            dims = hi - lo + 1
            nb = [(int(hi[k]) >> 3) - (int(lo[k]) >> 3) + 1 for k in range(3)]
            rd, wr = nb[0] * nb[1] * nb[2] * 4096, int(np.prod(dims.astype(np.int64))) * 5
            f.profile(True)
            us_k, us = [], _abi.C.c_float(0)
            for r in range(a.repeats + 1):
                out = f.export_dense(lo, dims, task=True, device=True)
                _abi.check(L.sf_fuser_export_dense_kernel_us(_abi.C.byref(us)))
                if r:
                    us_k.append(us.value)
            f.profile(False)
            del out
            src = torch.empty((rd + wr) // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            us_c = []
            for r in range(a.repeats + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    us_c.append(e0.elapsed_time(e1) * 1e3)
            del src, dst
            lines += ["(c) k_export_dense, region %d x %d x %d voxels (%d x %d x %d blocks, all allocated), sdf / voxel + weight to device arrays" % (
                dims[0], dims[1], dims[2], nb[0], nb[1], nb[2]),
                "    bytes: %d read (4 096 per block) + %d written (5 per voxel) = %.1f MB" % (rd, wr, (rd + wr) / 1e6),
                "    kernel us: %s" % med(us_k, "%.1f"),
                "    TB/s: %s   = %.1f %% of the %.1f TB/s HBM peak (median)" % (
                    med([(rd + wr) / (u * 1e-6) / 1e12 for u in us_k]), (rd + wr) / (statistics.median(us_k) * 1e-6) / HBM_PEAK * 100.0, HBM_PEAK / 1e12),
                "    a device copy of %.1f MB (the same bytes read + written), us: %s   TB/s: %s" % (
                    (rd + wr) / 2e6, med(us_c, "%.1f"), med([(rd + wr) / (u * 1e-6) / 1e12 for u in us_c])), ""]

        # (d) the allocation walk in a stage where every block exists
        if not a.no_trace:
            tot, line = trace(os.path.join(ROOT, "bin", "freespace"), scan, voxel, work)
            if tot is None:
                lines += ["(d) not measured: %s" % line, ""]
            else:
                fuse = float(line.split("fuse")[1].split(",")[0]) if "fuse" in line else float("nan")
                lines += ["(d) bin/freespace under rocprofv3 --kernel-trace --stats (a run of its own; the tool's own %s)" % line,
                          "    device seconds by kernel: " + ", ".join("%s %.4f" % kv for kv in sorted(tot.items(), key=lambda kv: -kv[1])),
                          "    the allocation kernels (k_alloc*): %.4f s = %.1f %% of the sf_fuse_run step's %.4f s; they run on the front stream beside k_integrate," % (
                              tot.get("k_alloc", 0.0), tot.get("k_alloc", 0.0) / fuse * 100.0, fuse),
                          "    and in this stage they find every block they name in the table: a lead (a fuser switch that skips the walk), not taken up here", ""]
        say("voxel %g done" % voxel)
    sd.close()
    if not a.work:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
