#!/usr/bin/env python3
"""Time of the depth-distortion table estimate on a sequence of the sensor's size: 600 synthetic 640 x 480 images of planes
between 0.45 m and 4.3 m (tilted up to 12 degrees, observed 3 % long, hashed noise of +-3 mm so that the PNG files compress as a sensor's do), 15 slices.

  (a) k_lut_accumulate alone on device-resident images (sf_lut_estimator_add_device with kernel_us: HIP events around the launches)
  (b) the host path (sf_lut_estimator_add, device -1) on the CPUs this process may use
  (c) bin/calibrate_depth end to end from PNG files, `-e` then `-a`, with --device=0 and with --host

One warm-up, then --repeats timed runs of each; median with min .. max.  The decision rule for the tool's default is printed with the numbers.

  python tools/depth_lut_bench.py [--images 600] [--repeats 5] [--out profiles/depth_lut.txt] [--work DIR]
needs a GPU."""
import argparse
import ctypes as C
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


def med(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def sequence(n):
    from tests import depth_lut_cases as dc
    W, H = 640, 480
    K = dc.intrinsics(W, H)
    rng = np.random.default_rng(5578)
    poses, depths = [], []
    for k in range(n):
        T = dc.plane_pose(0.45 + (4.3 - 0.45) * k / max(1, n - 1), 12.0 * np.sin(1.7 * k), "xy"[k % 2])
        mm = np.rint(1030.0 * dc.true_depth(T, W, H, K)) + rng.integers(-3, 4, (H, W))
        mm = np.where((mm > 0) & (mm < 8192), mm, 0).astype(np.uint16)
        poses.append(T)
        depths.append(dc.shift_in(mm))
    return dict(W=W, H=H, K=K, n_slices=15, max_depth=5.0, bitshift=True, depths=np.ascontiguousarray(np.stack(depths)), poses=np.ascontiguousarray(np.stack(poses), np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_lut.txt"))
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    from scannet_amd import _abi, depth_lut, filter2d
    from tests import depth_lut_cases as dc
    L = depth_lut._lib()
    seq = sequence(a.images)
    n, px = a.images, 640 * 480
    lines = ["depth-distortion table estimate: %d images of 640 x 480, 15 slices, max depth 5 m; one warm-up, %d repeats, median (min .. max)" % (n, a.repeats),
             "host threads: %d" % _abi.usable_cpus(), ""]

    # (a) the kernel on device-resident images
    d = C.c_void_p()
    _abi.check(L.sf_device_malloc(0, n * px * 2, C.byref(d)))
    _abi.check(L.sf_device_upload(d, seq["depths"].ctypes.data, n * px * 2))
    ptr = (C.c_void_p * n)(*[d.value + k * px * 2 for k in range(n)])
    us_all, dev_table = [], None
    for r in range(a.repeats + 1):
        with depth_lut.Estimator(640, 480, seq["K"], 15, 5.0, True, device=0) as e:
            us = C.c_float(0)
            _abi.check(L.sf_lut_estimator_add_device(e._h, n, ptr, seq["poses"].ctypes.data, C.byref(us)))
            if r:
                us_all.append(us.value)
            else:
                dev_table = e.finish()[0]
    L.sf_device_free(d)
    per = [u / n for u in us_all]
    share = [614400.0 / (u * 1e-6) / HBM_PEAK * 100.0 for u in per]
    lines += ["(a) k_lut_accumulate, device-resident images, %d per launch" % depth_lut.max_batch(),
              "    us per image: %s" % med(per), "    share of the HBM peak (614 400 B read per image, %.1f TB/s): %s %%" % (HBM_PEAK / 1e12, med(share)), ""]

    print("kernel done", file=sys.stderr, flush=True)
    # (b) the host path
    t_all, host_table = [], None
    for r in range(a.repeats + 1):
        with depth_lut.Estimator(640, 480, seq["K"], 15, 5.0, True, device=-1) as e:
            t0 = time.perf_counter()
            e.add(seq["depths"], seq["poses"])
            t = time.perf_counter() - t0
            if r:
                t_all.append(t)
            else:
                host_table = e.finish()[0]
    same = np.array_equal(dc.bits(dev_table), dc.bits(host_table))
    lines += ["(b) the host path, sf_lut_estimator_add on host images", "    us per image: %s" % med([t / n * 1e6 for t in t_all]), "    seconds per sequence: %s" % med(t_all),
              "    table bits device == host: %s" % same, ""]

    print("host path done", file=sys.stderr, flush=True)
    # (c) the tool from PNG files
    work = a.work or tempfile.mkdtemp(prefix="depth_lut_bench_")
    conf = dc.write_sequence(work, seq, filter2d.png_write_gray)
    size = sum(os.path.getsize(os.path.join(work, "depth_raw", f)) for f in os.listdir(os.path.join(work, "depth_raw")))
    tool = os.path.join(ROOT, "bin", "calibrate_depth")
    res, last, blobs = {}, {}, {}
    for mode in ("--device=0", "--host"):
        ts = []
        for r in range(a.repeats + 1):
            lut = os.path.join(work, "bench.lut")
            t0 = time.perf_counter()
            p = subprocess.run([tool, conf, "-e", lut, "-a", lut, "-v", "--root=" + work, mode], capture_output=True, text=True)
            t = time.perf_counter() - t0
            if p.returncode != 0:
                raise RuntimeError(p.stderr)
            print("tool %s run %d: %.3f s" % (mode, r, t), file=sys.stderr, flush=True)
            if r:
                ts.append(t)
            last[mode] = p.stdout.strip().splitlines()[-1]
        res[mode] = ts
        blobs[mode] = open(lut, "rb").read() + open(os.path.join(work, "depth", "frame-0007.png"), "rb").read()
    lines += ["(c) bin/calibrate_depth <conf> -e t.lut -a t.lut from %d PNG files (%.1f MB, %.0f kB each), wall seconds of the process" % (n, size / 1e6, size / n / 1e3)]
    for mode in res:
        lines += ["    %-11s %s" % (mode, med(res[mode])), "                %s" % last[mode]]
    lines += ["    same bytes (table, a corrected image): %s" % (blobs["--device=0"] == blobs["--host"]), ""]
    dev_wins = max(res["--device=0"]) < min(res["--host"])
    lines += ["decision: the slowest device repeat (%.3f s) %s the fastest host repeat (%.3f s): the default of the tool and of estimate() is %s" % (
        max(res["--device=0"]), "beats" if dev_wins else "does not beat", min(res["--host"]), "the device" if dev_wins else "the host path; --device=N is opt-in")]
    if not a.work:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
