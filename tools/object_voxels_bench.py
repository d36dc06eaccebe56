#!/usr/bin/env python3
"""Times of the object-task data on the furnished room of the benchmark (640 x 480, hashed noise): the grid is the free-space
stage's at 5 cm, the meshes are a fuser's marching-cubes mesh with the stage's parameters ("undecimated") and that mesh through clean.mlx's filters
and the quadric decimation ("decimated"); the objects are six height bands times four quadrants of the floor plan, 24 in all, each with a class.

  (a) sf_objvox_voxelize from host arrays to host arrays, for both meshes: the device (wall seconds of the call, copies included, and the device
      microseconds of its launches: grouping and cubes, k_ov_raster, k_ov_emit) against the host path on the CPUs this process may use (at most 16)
  (b) bin/objectvoxels end to end, from files to files, --host against --device=0, on the decimated mesh

One warm-up, then --repeats timed runs of each; median with min .. max.  The last lines state which path the measurement makes the default.

  python tools/object_voxels_bench.py [--frames 600] [--repeats 5] [--out profiles/object_voxels.txt] [--work DIR]
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
W, H = 640, 480
CLASS_IDS = [1, 3, 4, 5, 9, 13, 18, 20, 22, 30, 31, 35, 39, 42, 47, 48, 49]     # Tasks/Benchmark/classes_ObjClassification-ShapeNetCore55.txt


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


def objects(xyz):
    """objectId 0 .. 23 per vertex: six height bands of half a metre, four quadrants around the mesh's centre"""
    band = np.clip(np.floor(xyz[:, 2] / 0.5), 0, 5).astype(np.int64)
    cx, cy = np.median(xyz[:, 0]), np.median(xyz[:, 1])
    return band * 4 + 2 * (xyz[:, 1] > cy) + (xyz[:, 0] > cx)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_voxels.txt"))
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    import torch
    from scannet_amd import _abi, freespace, fusion, meshclean, object_voxels as ov, sens
    if not torch.cuda.is_available():
        raise SystemExit("tools/object_voxels_bench.py needs a GPU: nothing here is measured without one")
    work = a.work or tempfile.mkdtemp(prefix="object_voxels_bench_")
    os.makedirs(work, exist_ok=True)
    scan = os.path.join(work, "scan.sens")
    write_scan(scan, a.frames)
    sd = sens.SensorData(scan)
    lines = ["object-task data: %d frames of %d x %d (furnished room, hashed noise), 5 cm grid; one warm-up, %d repeats, median (min .. max); %s" % (
        a.frames, W, H, a.repeats, time.strftime("%Y-%m-%d", time.gmtime())),
        "device: %s; host threads: at most %d" % (torch.cuda.get_device_name(0), min(16, _abi.usable_cpus())), ""]
    fp = freespace.default_params(voxel_size=0.05)
    grid = freespace.carve_sens(sd, fp)
    sp, lo_b, hi_b = freespace.plan(sd, fp)
    with fusion.Fuser(sp, device=0) as f:
        f.allocate_box(lo_b, hi_b)
        f.run(sd)
        full = f.extract_mesh()
    cleaned, _ = meshclean.clean(full, gpu=0)
    small, _ = meshclean.simplify(cleaned, gpu=0)
    cleaned.close()
    cls = np.array([CLASS_IDS[k % len(CLASS_IDS)] for k in range(24)], np.int32)

    # (a) the call
    for name, m in (("decimated", small), ("undecimated", full)):
        xyz, _, tris = m.arrays()
        vobj = (objects(xyz) + 1).astype(np.uint32)
        us = []

        def dev():
            r = ov.voxelize(xyz, tris, vobj, cls, grid, device=0)
            us.append(ov.kernel_us())
            return r
        t_dev, got_d = timed(dev, a.repeats)
        t_host, got_h = timed(lambda: ov.voxelize(xyz, tris, vobj, cls, grid), a.repeats)
        assert np.array_equal(got_d.data, got_h.data) and got_d.origin.tobytes() == got_h.origin.tobytes(), "device and host disagree"
        us = us[1:]
        lines += ["(a) sf_objvox_voxelize, %s mesh: %d vertices, %d faces; %d objects kept, %d cells occupied, %d known; device and host bytes equal" % (
            name, len(xyz), len(tris), len(got_h), int(got_h.data[:, 0].sum()), int(got_h.data[:, 1].sum())),
            "    device, wall seconds of the call: %s" % med(t_dev),
            "      of which device us: grouping and cubes %s, raster %s, emit %s" % tuple(med([u[k] for u in us], "%.0f") for k in ("group", "raster", "emit")),
            "    host path, wall seconds:          %s" % med(t_host),
            "    host / device (medians): %.2f x" % (statistics.median(t_host) / statistics.median(t_dev)), ""]
        say("%s: device %.4f host %.4f" % (name, statistics.median(t_dev), statistics.median(t_host)))

    # (b) the tool, from files to files
    xyz, _, tris = small.arrays()
    d = os.path.join(work, "tool")
    os.makedirs(d, exist_ok=True)
    grid.save(os.path.join(d, "scan.grid"))
    small.write_ply(os.path.join(d, "mesh.ply"))
    json.dump({"params": {}, "sceneId": "room", "segIndices": [int(v) for v in objects(xyz)]}, open(os.path.join(d, "segs.json"), "w"))
    json.dump({"sceneId": "room", "appId": "bench", "segGroups": [{"id": k, "objectId": k, "segments": [k], "label": "thing%d" % k} for k in range(24)]},
              open(os.path.join(d, "agg.json"), "w"))
    open(os.path.join(d, "labels.tsv"), "w").write("id\traw_category\tShapeNetCore55\n" + "".join("%d\tthing%d\t%d\n" % (k, k, cls[k]) for k in range(24)))
    open(os.path.join(d, "classes.txt"), "w").write("".join("%d\tclass%d\n" % (c, c) for c in CLASS_IDS))
    base = [os.path.join(ROOT, "bin", "objectvoxels"), os.path.join(d, "mesh.ply"), os.path.join(d, "scan.grid"), "--segs=" + os.path.join(d, "segs.json"),
            "--aggregation=" + os.path.join(d, "agg.json"), "--label-map=" + os.path.join(d, "labels.tsv"), "--classes=" + os.path.join(d, "classes.txt")]
    t_tool = {}
    for flag in ("--host", "--device=0"):
        def run():
            r = subprocess.run(base + ["-o", os.path.join(d, "out" + flag.strip("-").replace("=", ""))] + [flag], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
        t_tool[flag], _ = timed(run, a.repeats)
    same = all(open(os.path.join(d, "outhost" + s), "rb").read() == open(os.path.join(d, "outdevice0" + s), "rb").read()
               for s in (".objects.data.npy", ".objects.label.npy", ".objects.id.npy"))
    wins = max(t_tool["--device=0"]) < min(t_tool["--host"])
    lines += ["(b) bin/objectvoxels, decimated mesh, files to files, wall seconds of the process (outputs byte-equal: %s)" % same,
              "    --host:     %s" % med(t_tool["--host"]),
              "    --device=0: %s" % med(t_tool["--device=0"]),
              "    the device's slowest repeat %s the host path's fastest" % ("beats" if wins else "does not beat"), "",
              "default path: the device is the default of the tool and of object_scan only if its slowest repeat beats the host path's fastest, end to end:",
              "%s" % ("the device qualifies" if wins else "the host path stays the default, --device=N is opt-in"), ""]
    full.close()
    small.close()
    sd.close()
    if not a.work:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
