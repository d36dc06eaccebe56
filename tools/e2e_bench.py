#!/usr/bin/env python3
"""End-to-end timing of the drop-in stage chain on one MI355X (numbers for DESIGN.md section 5; not bench.py's metric):
.sens on disk -> threaded inflate -> pinned ring -> H2D -> fusion (PCIe-inclusive frames/s) -> marching cubes -> PLY ->
clean -> Segmentator.  The stream is the config-2 walk rendered on the GPU, written with this repo's .sens writer.

  python tools/e2e_bench.py [--frames 1500] [--voxel 0.004] [--threads 0] [--out gpurun_out/e2e.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scannet_amd import _abi, fusion, meshclean, segmentator, sens, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--total", type=int, default=5578)
    ap.add_argument("--voxel", type=float, default=0.004)
    ap.add_argument("--blocks", type=int, default=1 << 20)
    ap.add_argument("--buckets", type=int, default=1 << 19)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--dir", default="/tmp/sf_e2e")
    ap.add_argument("--out", default="")
    ap.add_argument("--color", choices=["none", "raw", "jpeg"], default="none", help="store a synthetic 640x480 colour frame per depth frame")
    ap.add_argument("--gpu-decimate", action="store_true", help="the decimate stage on the GPU (sf_mesh_simplify_gpu) instead of the sequential filter")
    ap.add_argument("--gpu-clean", action="store_true", help="the cleaning filters on the GPU (sf_mesh_clean_gpu: same output) instead of the host filters")
    ap.add_argument("--fuse-only", action="store_true", help="stop after the fusion stage")
    ap.add_argument("--no-prepare", action="store_true", help="do not call sf_fuse_run_prepare before the first fuser is created (A/B of the first run's set-up)")
    ap.add_argument("--scene", type=int, default=synth.SCENE_DEFAULT, help="0 = empty box room, 1 = furnished (default)")
    ap.add_argument("--noise", type=int, default=synth.NOISE_DEFAULT, help="1 = the LCG ramp of rounds 1-2, 2 = hashed per pixel (default)")
    ap.add_argument("--smooth-pictures", action="store_true", help="--color jpeg: the smooth pictures of rounds 1-4 (77-110 KB at 1296x968) instead of synth.textured_pictures (~200 KB)")
    ap.add_argument("--color-res", default="", help="WxH of the colour frames when it differs from the depth size (ScanNet: 1296x968)")
    a = ap.parse_args()
    W, H = 640, 480
    os.makedirs(a.dir, exist_ok=True)
    path = os.path.join(a.dir, "scene_e2e.sens")
    L = _abi.lib()
    # render on the GPU, pull to the host, write a real .sens (zlib depth)
    t0 = time.perf_counter()
    nbytes = a.frames * W * H * 2
    dptr = C.c_void_p()
    _abi.check(L.sf_device_malloc(0, nbytes, C.byref(dptr)))
    poses = np.zeros((a.frames, 16), np.float32)
    poses = synth.render_scan_device(dptr.value, W * H * 2, 0, a.frames, a.total, W, H, noise=a.noise, scene=a.scene)
    depth = np.zeros((a.frames, H, W), np.uint16)
    _abi.check(L.sf_device_download(depth.ctypes.data_as(C.c_void_p), dptr, nbytes))
    L.sf_device_free(dptr)
    K = synth.intrinsic_matrix(W, H)
    cw, ch = (W, H) if a.color != "none" else (0, 0)
    KC = K
    if a.color != "none" and a.color_res:
        cw, ch = (int(v) for v in a.color_res.lower().split("x"))
        KC = synth.intrinsic_matrix(cw, ch)
    sd = sens.SensorData.create(cw, ch, W, H, KC, K, color_compression=2 if a.color == "jpeg" else 0, depth_compression=1, sensor_name="StructureSensor")
    yy, xx = np.mgrid[0:(ch or H), 0:(cw or W)]
    blobs = []
    if a.color == "jpeg":
        from scannet_amd import calibrate
        if a.smooth_pictures:
            for k in range(8):   # eight distinct encoded frames, cycled (encoding thousands of frames would dominate the set-up)
                img = np.stack([(xx + 8 * k) % 256, (yy * 2) % 256, (128 + 100 * np.sin(xx / 30.0) * np.cos(yy / 20.0 + k))], -1).astype(np.uint8)
                blobs.append(calibrate.jpeg_encode(img, 90, True))
        else:
            blobs = [calibrate.jpeg_encode(img, 90, True) for img in synth.textured_pictures(cw or W, ch or H)]
    if a.color == "none":
        sd.add_depth_frames(depth, poses.reshape(-1, 4, 4))   # threaded deflate
    for i in range(a.frames if a.color != "none" else 0):
        color = None
        if a.color == "raw":
            color = np.stack([(xx + i) % 256, (yy * 2) % 256, np.full_like(xx, (i * 3) % 256)], -1).astype(np.uint8)
        elif a.color == "jpeg":
            color = blobs[i % 8]
        sd.add_frame(depth[i], poses[i].reshape(4, 4), color=color, timestamp_depth=33333 * i)
    sd.save(path)
    sd.close()
    t_write = time.perf_counter() - t0
    res = {"frames": a.frames, "sens_bytes": os.path.getsize(path), "compressed_bytes_per_frame": os.path.getsize(path) // a.frames, "scene": a.scene, "noise": a.noise,
           "write_s": round(t_write, 2), "voxel": a.voxel, "host_cores": os.cpu_count()}

    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=a.voxel, num_sdf_blocks=a.blocks,
                               hash_num_buckets=a.buckets)
    if a.color != "none" and a.color_res:
        gp.color_width, gp.color_height = cw, ch
        gp.cfx, gp.cfy, gp.cmx, gp.cmy = synth.intrinsics(cw, ch)
    sd = sens.SensorData(path)
    # the same scan fused twice by two fusers: sf_fuse_run keeps its streams and its pinned pool for the next run of the process (a dataset
    # rebuild fuses 1513 scans per process); the first run creates them.  Both rates are reported; the stages below continue from the second.
    if not a.no_prepare:
        fusion.Fuser.prepare_run(sd, gp, 0)   # as bin/depthsensing does (sf_fuse_run_prepare): the first run finds its streams and rings made
    with fusion.Fuser(gp) as f0:
        rs0 = f0.run(sd, decode_threads=a.threads)
    with fusion.Fuser(gp) as f:
        rs = f.run(sd, decode_threads=a.threads)
        st = f.stats()
        res["fuse"] = {"frames_per_s_end_to_end": round(rs["frames_total"] / rs["seconds_total"], 1), "seconds": round(rs["seconds_total"], 3),
                       "decode_threads": rs["decode_threads"], "decode_cpu_s": round(rs["seconds_decode_cpu"], 2),
                       "decode_ms_per_frame_per_thread": round(1e3 * rs["seconds_decode_cpu"] / max(rs["frames_total"], 1), 3),
                       "blocks": st["blocks_allocated"], "alloc_failures": st["alloc_failures"],
                       "voxel_tiles_GB": round(st["blocks_allocated"] * 4096 / 1e9, 2)}
        res["fuse"]["color_fused"] = rs["color_fused"]
        res["fuse"]["first_run_of_the_process"] = {"frames_per_s_end_to_end": round(rs0["frames_total"] / rs0["seconds_total"], 1), "seconds": round(rs0["seconds_total"], 3)}
        if a.fuse_only:
            print(json.dumps(res))
            if a.out:
                open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
            return
        t0 = time.perf_counter()
        mesh = f.extract_mesh()
        res["marching_cubes_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        mesh = f.extract_mesh()   # once more: the first call pays for the kernels' code objects and the pinned staging
        res["marching_cubes_second_call_s"] = round(time.perf_counter() - t0, 3)
        res["marching_cubes_phases_ms"] = f.mc_timing()
    nv, nf = mesh.counts()
    res["mesh"] = {"vertices": nv, "faces": nf}
    ply = os.path.join(a.dir, "scene_e2e_vh.ply")
    t0 = time.perf_counter()
    mesh.write_ply(ply)
    res["ply_write_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    cleaned, cst = meshclean.clean(mesh, gpu=0 if a.gpu_clean else None)
    res["clean_where"] = "gpu" if a.gpu_clean else "host"
    res["clean_s"] = round(time.perf_counter() - t0, 3)
    res["clean"] = {k: cst[k] for k in ("vertices_out", "faces_out", "components_in", "components_removed")}
    cply = os.path.join(a.dir, "scene_e2e_vh_clean.ply")
    cleaned.write_ply(cply)
    # the decimate stage: quadric edge collapse to 20 % twice, each followed by the cleaning filters (simplify.mlx)
    cur = cleaned
    for k in (1, 2):
        t0 = time.perf_counter()
        simp, sst = meshclean.simplify(cur, gpu=0 if a.gpu_decimate else None)
        t1 = time.perf_counter()
        cur, _ = meshclean.clean(simp, min_component_faces=1000, gpu=0 if a.gpu_clean else None)
        res["decimate%d_s" % k] = round(time.perf_counter() - t0, 3)
        res["decimate%d" % k] = {"faces_in": sst["faces_in"], "faces_out": cur.counts()[1], "collapses": sst["collapses"], "rounds": sst["rounds"],
                                 "collapse_s": round(t1 - t0, 3), "where": "gpu" if a.gpu_decimate else "host"}
    cply = os.path.join(a.dir, "scene_e2e_vh_clean_2.ply")
    cur.write_ply(cply)
    t0 = time.perf_counter()
    nseg = segmentator.segment_to_json(cply)
    res["segment_s"] = round(time.perf_counter() - t0, 3)
    res["segments"] = nseg
    ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "segmentator_ref")
    if os.path.exists(ref):
        # the reference binary on a COPY of the same mesh (it names its output after the input, so it would overwrite ours): timed AND compared
        import shutil
        import subprocess
        refdir = os.path.join(a.dir, "reference_segmentator")
        os.makedirs(refdir, exist_ok=True)
        rply = os.path.join(refdir, os.path.basename(cply))
        shutil.copyfile(cply, rply)
        t0 = time.perf_counter()
        subprocess.run([ref, rply], capture_output=True)
        res["segment_reference_binary_s"] = round(time.perf_counter() - t0, 3)
        name = os.path.basename(cply)[:-4] + ".0.010000.segs.json"
        ours = json.load(open(os.path.join(a.dir, name)))
        theirs = json.load(open(os.path.join(refdir, name)))
        res["segment_identical_to_reference"] = ours["segIndices"] == theirs["segIndices"] and ours["params"] == theirs["params"]
        if not res["segment_identical_to_reference"]:
            raise SystemExit("segIndices differ from the reference binary's on %s" % cply)
    print(json.dumps(res))
    if a.out:
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
