#!/usr/bin/env python3
"""Times of the voxel-task data on the furnished room of the benchmark (640 x 480, hashed noise), at 5 cm and at 2 cm voxels: the
grid is the free-space stage's, the meshes are a fuser's marching-cubes mesh with the stage's parameters ("undecimated") and that mesh through
clean.mlx's filters and the quadric decimation ("decimated"); labels are six height bands.

  (a) the nearest-face search, sf_voxlabel_nearest_faces from host arrays to host arrays: the device (wall seconds of the call, copies included, and the
      device microseconds of its bin and search launches) against the host path on the CPUs this process may use (at most 16), for both meshes
  (b) k_vl_sample into device arrays: bytes read + bytes written over the kernel time (HIP events around the launch), beside the HBM peak and beside a
      plain device copy that moves the same number of bytes, timed in the same run
  (c) bin/voxellabels end to end, from files to files, --host against --device=0 (at most --samples samples)

One warm-up, then --repeats timed runs of each; median with min .. max.  The last lines state which path the measurement makes the default.

  python tools/voxel_labels_bench.py [--frames 600] [--repeats 5] [--voxels 0.05 0.02] [--samples 1024] [--out profiles/voxel_labels.txt] [--work DIR]
needs a GPU."""
import argparse
import json
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


def med(v, fmt="%.4f"):
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


def bands(xyz):
    return (1 + np.clip(np.floor(xyz[:, 2] / 0.5), 0, 5)).astype(np.uint16)


def timed(fn, repeats):
    out = []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        res = fn()
        t = time.perf_counter() - t0
        if r:
            out.append(t)
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--voxels", type=float, nargs="+", default=[0.05, 0.02])
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_labels.txt"))
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    import torch
    from scannet_amd import _abi, freespace, fusion, meshclean, sens, voxel_labels as vl
    if not torch.cuda.is_available():
        raise SystemExit("tools/voxel_labels_bench.py needs a GPU: nothing here is measured without one")
    work = a.work or tempfile.mkdtemp(prefix="voxel_labels_bench_")
    os.makedirs(work, exist_ok=True)
    scan = os.path.join(work, "scan.sens")
    write_scan(scan, a.frames)
    sd = sens.SensorData(scan)
    lines = ["voxel-task data: %d frames of %d x %d (furnished room, hashed noise); one warm-up, %d repeats, median (min .. max); %s" % (
        a.frames, W, H, a.repeats, time.strftime("%Y-%m-%d", time.gmtime())),
        "device: %s; host threads: at most %d" % (torch.cuda.get_device_name(0), min(16, _abi.usable_cpus())), ""]
    verdicts = []
    for voxel in a.voxels:
        fp = freespace.default_params(voxel_size=voxel)
        grid = freespace.carve_sens(sd, fp)
        sp, lo_b, hi_b = freespace.plan(sd, fp)
        with fusion.Fuser(sp, device=0) as f:
            f.allocate_box(lo_b, hi_b)
            f.run(sd)
            full = f.extract_mesh()
        cleaned, _ = meshclean.clean(full, gpu=0)
        small, _ = meshclean.simplify(cleaned, gpu=0)
        cleaned.close()
        meshes = {}
        for name, m in (("decimated", small), ("undecimated", full)):
            xyz, _, tris = m.arrays()
            meshes[name] = (xyz, tris)
        nz, ny, nx = grid.value.shape
        lines += ["=== voxel %g m: grid %d x %d x %d = %d nodes" % (voxel, nx, ny, nz, grid.value.size), ""]

        # (a) the nearest-face search
        for name, (xyz, tris) in meshes.items():
            us = []

            def dev():
                r = vl.nearest_faces(grid, xyz, tris, device=0, dist2=False)[0]
                us.append(vl.kernel_us())
                return r
            t_dev, face_d = timed(dev, a.repeats)
            t_host, face_h = timed(lambda: vl.nearest_faces(grid, xyz, tris, dist2=False)[0], a.repeats)
            assert np.array_equal(face_d, face_h), "device and host disagree"
            us = us[1:]
            lines += ["(a) nearest faces, %s mesh: %d vertices, %d faces; %d nodes with a face; device and host bytes equal" % (
                name, len(xyz), len(tris), int((face_h >= 0).sum())),
                "    device, wall seconds of the call: %s" % med(t_dev),
                "      of which device us: bins %s, search %s" % (med([u["bins"] for u in us], "%.0f"), med([u["nearest"] for u in us], "%.0f")),
                "    host path, wall seconds:          %s" % med(t_host),
                "    host / device (medians): %.1f x" % (statistics.median(t_host) / statistics.median(t_dev)), ""]
            say("voxel %g %s: device %.4f host %.4f" % (voxel, name, statistics.median(t_dev), statistics.median(t_host)))

        # (b) k_vl_sample into device arrays
        xyz, tris = meshes["decimated"]
        scan_l = vl.label_scan(grid, xyz, tris, bands(xyz))
        stride = 1
        while vl.count_columns(grid, scan_l.byte_label, vl.default_params(stride=stride)) > a.samples:
            stride += 1
        p = vl.default_params(stride=stride)
        total = vl.count_columns(grid, scan_l.byte_label, p)
        out = (torch.empty((total, 1, p.wz, p.wy, p.wx), dtype=torch.float32, device="cuda"), torch.empty((total, p.wz), dtype=torch.uint8, device="cuda"),
               torch.empty((total, 2), dtype=torch.int32, device="cuda"))
        us_k = []
        for r in range(a.repeats + 1):
            vl.sample_columns(grid, scan_l.byte_label, p, device=0, max_samples=total, out=out)
            if r:
                us_k.append(vl.kernel_us()["sample"])
        moved = 2 * out[0].numel() * 4
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
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
        del src, dst, out
        lines += ["(b) k_vl_sample: %d samples (stride %d) of %d x %d x %d into device arrays" % (total, stride, p.wx, p.wy, p.wz),
                  "    bytes: %.1f MB read (clamped loads, one per element) + %.1f MB written" % (moved / 2e6, moved / 2e6),
                  "    kernel us: %s" % med(us_k, "%.1f"),
                  "    TB/s: %s   = %.1f %% of the %.1f TB/s HBM peak (median)" % (
                      med([moved / (u * 1e-6) / 1e12 for u in us_k], "%.3f"), moved / (statistics.median(us_k) * 1e-6) / HBM_PEAK * 100.0, HBM_PEAK / 1e12),
                  "    a device copy of %.1f MB (the same bytes read + written), us: %s   TB/s: %s" % (
                      moved / 2e6, med(us_c, "%.1f"), med([moved / (u * 1e-6) / 1e12 for u in us_c], "%.3f")), ""]

        # (c) the tool, from files to files
        d = os.path.join(work, "tool_%g" % voxel)
        os.makedirs(d, exist_ok=True)
        grid.save(os.path.join(d, "scan.grid"))
        small.write_ply(os.path.join(d, "mesh.ply"))
        seg = [int(v) for v in bands(xyz)]
        json.dump({"params": {}, "sceneId": "room", "segIndices": seg}, open(os.path.join(d, "segs.json"), "w"))
        json.dump({"sceneId": "room", "appId": "bench", "segGroups": [{"id": k, "objectId": k, "segments": [k + 1], "label": "band%d" % k} for k in range(6)]},
                  open(os.path.join(d, "agg.json"), "w"))
        open(os.path.join(d, "labels.tsv"), "w").write("id\tcategory\tcount\n" + "".join("%d\tband%d\t1\n" % (k, k) for k in range(6)))
        base = [os.path.join(ROOT, "bin", "voxellabels"), os.path.join(d, "scan.grid"), os.path.join(d, "mesh.ply"), "--segs=" + os.path.join(d, "segs.json"),
                "--aggregation=" + os.path.join(d, "agg.json"), "--label-map=" + os.path.join(d, "labels.tsv"), "--stride=%d" % stride,
                "--max-samples=%d" % a.samples]
        t_tool = {}
        for flag in ("--host", "--device=0"):
            def run():
                r = subprocess.run(base + ["-o", os.path.join(d, "out" + flag.strip("-").replace("=", ""))] + [flag], capture_output=True, text=True)
                assert r.returncode == 0, r.stderr
            t_tool[flag], _ = timed(run, a.repeats)
        same = all(open(os.path.join(d, "outhost" + s), "rb").read() == open(os.path.join(d, "outdevice0" + s), "rb").read()
                   for s in (".label.npy", ".instance.npy", ".samples.data.npy", ".samples.label.npy"))
        wins = max(t_tool["--device=0"]) < min(t_tool["--host"])
        verdicts.append(wins)
        lines += ["(c) bin/voxellabels, decimated mesh, files to files, wall seconds of the process (outputs byte-equal: %s)" % same,
                  "    --host:     %s" % med(t_tool["--host"]),
                  "    --device=0: %s" % med(t_tool["--device=0"]),
                  "    the device's slowest repeat %s the host path's fastest" % ("beats" if wins else "does not beat"), ""]
        full.close()
        small.close()
        say("voxel %g done" % voxel)
    lines += ["default path: the device is the default of the tool and of label_scan only if its slowest repeat beats the host path's fastest, end to end, at every",
              "voxel size measured: %s -> %s" % (verdicts, "the device qualifies" if all(verdicts) else "the host path stays the default, --device=N is opt-in"), ""]
    sd.close()
    if not a.work:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
