#!/usr/bin/env python3
"""Time of the mesh render (sf_renderer_run) on a scan-sized mesh, device path against host path.

The mesh is the furnished synthetic room fused on the GPU at 1 cm voxels, extracted by marching cubes, then cleaned and decimated twice as
scannet_amd/shard.py's finish_scan does it (the `<id>_vh_clean_2.ply` of the pipeline), with hashed vertex colours: as it is, without its
ceiling (see coloured()), and -- the larger case -- the cleaned mesh before decimation without its ceiling.  640 x 480, 16 samples, `path` at
depth 8 and `ao`.  Per integrator: one warm-up call, then --repeats timed calls of one view (wall time of sf_renderer_run with its download, and
the kernel by HIP events), the same for 32 views in one launch, and the host path on the CPUs this process may use.  The tree's build time is the
wall time of sf_renderer_set_mesh on the host path.

  python tools/render_bench.py [--frames 400] [--repeats 5] [--host-repeats 5] [--out profiles/render.txt]
  python tools/render_bench.py --kernel-only        # one view per integrator and nothing else: the command to put behind rocprofv3 --kernel-trace --stats
needs a GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def room_mesh(frames, voxel):
    import torch
    from scannet_amd import fusion, meshclean, synth
    W, H = 640, 480
    dev = torch.empty((frames, H, W), dtype=torch.int16, device="cuda")
    poses = synth.render_scan_device(dev.data_ptr(), W * H * 2, 0, frames, 5578, W, H, noise=2, scene=1, seed=0)
    with fusion.Fuser(fusion.default_params(voxel_size=voxel), device=0) as f:
        f.integrate_batch_device(dev.data_ptr(), W * H * 2, poses)
        mesh = f.extract_mesh()
    del dev
    torch.cuda.empty_cache()
    raw = mesh.counts()
    cleaned, _ = meshclean.clean(mesh, meshclean.CLEAN_MLX_MERGE_DISTANCE, 7500, gpu=0)
    cur = cleaned
    for _ in range(2):
        simp, _ = meshclean.simplify(cur, gpu=0)
        cur, _ = meshclean.clean(simp, meshclean.CLEAN_MLX_MERGE_DISTANCE, meshclean.CLEAN_LORES_MIN_COMPONENT, gpu=0)
    return [("decimated", coloured(cur, False)), ("decimated, ceiling removed", coloured(cur, True)), ("cleaned only, ceiling removed", coloured(cleaned, True))], raw


def coloured(mesh, open_top):
    """The mesh with hashed vertex colours; open_top: without the faces of the ceiling (every corner within 15 cm of the top).  The synthetic room is a
    closed box scanned from inside, so every face looks inwards and the default view from above meets the back of the ceiling, which ends a path at
    once; a real scan has no ceiling and the view looks into the room."""
    from scannet_amd.segmentator import Mesh
    xyz, _, tris = mesh.arrays()
    if open_top:
        tris = np.ascontiguousarray(tris[~(xyz[tris, 2] > xyz[:, 2].max() - 0.15).all(1)])
    i = np.arange(len(xyz), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(24)
    rgba = np.stack([40 + ((i >> np.uint64(8 * k)) & np.uint64(255)) * np.uint64(200) // np.uint64(255) for k in range(3)] + [np.full(len(xyz), 255, np.uint64)], -1)
    return Mesh.from_arrays(xyz, tris, rgba.astype(np.uint8))


def host_threads():
    """sf::usable_cpus(): the hardware concurrency capped by the cgroup's CPU quota."""
    n = os.cpu_count() or 1
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, -(-int(q) // int(period))))
    except (OSError, ValueError):
        pass
    return n


def timed(f, repeats):
    f()   # warm-up
    walls, kernels = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        k = f()
        walls.append(time.perf_counter() - t0)
        kernels.append(k * 1e-6)
    return walls, kernels


def spread(v):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scannet_amd import render
    meshes, raw = room_mesh(a.frames, a.voxel)
    lines = ["command: python tools/render_bench.py " + " ".join(sys.argv[1:]),
             "furnished room, %d frames at %g m: marching cubes %d vertices %d faces, cleaned, and decimated twice as scannet_amd/shard.py does" % (a.frames, a.voxel, raw[0], raw[1]),
             "640 x 480, 16 samples; seconds, median (min .. max) of the repeats after one warm-up call; the host path runs %d threads" % host_threads(), ""]
    for s in lines:
        print(s, flush=True)

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for label, mesh in meshes[1:2] if a.kernel_only else meshes:
        nv, nf = mesh.counts()
        emit("== %s: %d vertices, %d faces" % (label, nv, nf))
        if not a.kernel_only:
            builds = []
            for _ in range(a.repeats):
                with render.Renderer(render.default_params(), -1) as r:
                    t0 = time.perf_counter()
                    r.set_mesh(mesh)
                    builds.append(time.perf_counter() - t0)
                    n_nodes = len(r.nodes()[0])
            emit("tree: %d nodes, built on one host thread in %s" % (n_nodes, spread(builds)))
        images = {}
        for integ in ("path", "ao"):
            p = render.default_params(integrator=integ)
            cams = [render.camera(mesh, p, theta=11.25 * i) for i in range(32)]
            with render.Renderer(p, 0) as r:
                r.set_mesh(mesh)

                def one(r=r, cams=cams):
                    images[integ] = r.run(cams[0])
                    return r.kernel_us

                if a.kernel_only:
                    one()
                    continue
                w, k = timed(one, a.repeats)
                img = images[integ][0]
                emit("%-4s picture: mean alpha %.3f, mean RGB on the mesh %.3f" % (integ, img[..., 3].mean(), img[..., :3][img[..., 3] > 0].mean()))
                emit("%-4s device,  1 view  per launch: call %s   kernel %s" % (integ, spread(w), spread(k)))

                def many(r=r, cams=cams):
                    r.run(cams)
                    return r.kernel_us

                w, k = timed(many, a.repeats)
                emit("%-4s device, 32 views per launch: call %s   kernel %s   = %.4f per view" % (integ, spread(w), spread(k), statistics.median(k) / 32))
            with render.Renderer(p, -1) as h:
                h.set_mesh(mesh)
                host = {}

                def one_host(h=h, cams=cams):
                    host["image"] = h.run(cams[0])
                    return h.kernel_us

                w, k = timed(one_host, a.host_repeats)
                emit("%-4s host path, 1 view: call %s   bits equal to the device's: %s" % (integ, spread(w), np.array_equal(host["image"].view(np.uint32), images[integ].view(np.uint32))))
        emit("")
    if a.out and not a.kernel_only:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
