"""End-to-end on the GPU: .sens -> threaded decode -> fusion -> mesh -> PLY -> Segmentator, through the library
entry point and through the two drop-in executables (the `improve` and `segment` stages of Server/scan_processor.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_sens(path, n, W, H, total, invalid=()):
    from scannet_amd import sens
    K = synth.intrinsic_matrix(W, H)
    sd = sens.SensorData.create(0, 0, W, H, K, K, sensor_name="StructureSensor")
    frames = []
    for i in range(n):
        pose = synth.trajectory_pose(i * 7, total)
        d = synth.render_room_depth(pose, W, H, noise_frame=i)
        if i in invalid:
            pose = np.full((4, 4), -np.inf, np.float32)
        sd.add_frame(d, pose, timestamp_depth=i)
        frames.append((d, pose))
    sd.save(path)
    return frames


def test_fuse_run_matches_frame_by_frame(oracle, tmp_path):
    from scannet_amd import fusion, sens
    W, H = 320, 240
    p = str(tmp_path / "scene.sens")
    frames = _write_sens(p, 40, W, H, 1200, invalid=(3, 17))
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.008, num_sdf_blocks=1 << 17)
    sd = sens.SensorData(p)
    with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b:
        st = a.run(sd, decode_threads=5)
        assert (st["frames_total"], st["frames_integrated"], st["frames_skipped"]) == (40, 38, 2)
        for d, pose in frames:
            b.integrate(d, pose)
        ca, va = a.export_blocks()
        cb, vb = b.export_blocks()
        assert np.array_equal(ca, cb) and np.array_equal(va.view(np.uint8), vb.view(np.uint8))
        assert a.stats()["frames_skipped"] == 2
        # sub-range + wrong resolution
        with fusion.Fuser(gp) as c:
            assert c.run(sd, first=10, last=20, decode_threads=2)["frames_total"] == 10
        gp2 = fusion.default_params(depth_width=W + 8, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, num_sdf_blocks=1 << 12)
        with fusion.Fuser(gp2) as d2:
            with pytest.raises(Exception, match="created for"):
                d2.run(sd)


def _recompress_depth_frames(path, which, how):
    """Rewrite a .sens (v4 layout, sensorData.h:1250-1290 / :580-598) with the depth blobs of the frames in `which` replaced by how(raw bytes)."""
    import struct
    import zlib
    b = open(path, "rb").read()
    o = 4
    (n,) = struct.unpack_from("<Q", b, o)
    o += 8 + n + 4 * 64 + 4 + 4
    cw, ch, dw, dh = struct.unpack_from("<IIII", b, o)
    o += 16 + 4
    (nf,) = struct.unpack_from("<Q", b, o)
    o += 8
    out = bytearray(b[:o])
    for i in range(nf):
        head = b[o:o + 64 + 16]
        cs, ds = struct.unpack_from("<QQ", b, o + 80)
        col = b[o + 96:o + 96 + cs]
        dep = b[o + 96 + cs:o + 96 + cs + ds]
        o += 96 + cs + ds
        if i in which:
            dep = how(zlib.decompress(dep))
        out += head + struct.pack("<QQ", cs, len(dep)) + col + dep
    out += b[o:]
    open(path, "wb").write(bytes(out))


@pytest.mark.parametrize("where", ["gpu", "host"])
def test_fuse_run_inflates_depth_on_the_gpu_or_on_the_host(tmp_path, where, monkeypatch):
    """sf_fuse_run sends zlib depth frames to the GPU compressed (the writer's one fixed-Huffman block: csrc/inflate_gpu.hip) and inflates what
    the device does not take on the host threads -- here every fifth frame is recompressed by python's zlib (dynamic blocks) and one is stored
    (level 0) -- or everything on the host (SF_INFLATE_HOST): the same voxels as integrating the decoded frames one by one.  A frame whose stream
    inflates to the wrong size fails the run on either path."""
    import zlib
    from scannet_amd import fusion, sens
    from tests import deflate_tools as dt
    W, H = 320, 240
    p = str(tmp_path / "scene.sens")
    frames = _write_sens(p, 70, W, H, 1200, invalid=(9,))
    _recompress_depth_frames(p, set(range(0, 70, 5)) - {35}, lambda raw: zlib.compress(raw, 6))
    _recompress_depth_frames(p, {35}, lambda raw: zlib.compress(raw, 0))
    if where == "host":
        monkeypatch.setenv("SF_INFLATE_HOST", "1")
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.008, num_sdf_blocks=1 << 17)
    sd = sens.SensorData(p)
    with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b:
        st = a.run(sd, decode_threads=3)
        assert (st["frames_total"], st["frames_integrated"], st["frames_skipped"]) == (70, 69, 1)
        for d, pose in frames:
            b.integrate(d, pose)
        ca, va = a.export_blocks()
        cb, vb = b.export_blocks()
        assert np.array_equal(ca, cb) and np.array_equal(va.view(np.uint8), vb.view(np.uint8))
    short = str(tmp_path / "short.sens")
    _write_sens(short, 12, W, H, 1200)
    short_tokens = list(range(250)) * 4 + [(258, 1000)] * 591 + [(118, 1000)]                # one fixed block that inflates to four bytes less than a frame
    assert len(dt.apply_tokens(short_tokens)) == W * H * 2 - 4
    _recompress_depth_frames(short, {7}, lambda raw: dt.zlib_stream(short_tokens))
    with fusion.Fuser(gp) as c:
        with pytest.raises(Exception, match="inflate"):
            c.run(sens.SensorData(short), decode_threads=2)


DROP_IN_GOLDEN = os.path.join(ROOT, "tests", "golden", "drop_in_segmentator_golden.json")


def _mesh_sha256(path):
    from scannet_amd import segmentator
    import hashlib
    h = hashlib.sha256()
    for a in segmentator.Mesh.read(path).arrays():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _drop_in_clean_mesh(tmp_path):
    """The `improve` stage by the drop-in executables: `depthsensing p1 p2 scene0000_00.sens` -> scene0000_00_vh.ply, `meshclean ... -s clean.mlx` ->
    scene0000_00_vh_clean.ply (also what tests/golden/make_drop_in_golden.py records the reference Segmentator on).  Returns (params, ply, clean ply)."""
    W, H = 320, 240
    sens_path = str(tmp_path / "scene0000_00.sens")
    _write_sens(sens_path, 30, W, H, 1200)
    params = tmp_path / "zParametersScanNet.txt"
    # the fusion keys of Server/tools/recons/zParametersScanNet.txt:34-35,47-52 (values only: nothing under /root/reference is read by a GPU test)
    params.write_text("s_sensorDepthMin = 0.1f;\ns_sensorDepthMax = 6.0f;\ns_SDFVoxelSize = 0.010f;\ns_SDFMarchingCubeThreshFactor = 10.0f;\ns_SDFTruncation = 0.06f;\n"
                      "s_SDFTruncationScale = 0.02f;\ns_SDFMaxIntegrationDistance = 4.0f;\ns_SDFIntegrationWeightSample = 1;\ns_SDFIntegrationWeightMax = 99999999;\n"
                      "s_hashNumSDFBlocks = 200000;\n")
    (tmp_path / "zParametersTrackingDefault.txt").write_text("// tracking parameters are not used by the fusion stage\n")
    out = subprocess.run([os.path.join(ROOT, "bin", "depthsensing"), str(params), str(tmp_path / "zParametersTrackingDefault.txt"), sens_path],
                         capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert out.stderr == ""
    ply = str(tmp_path / "scene0000_00_vh.ply")
    assert os.path.getsize(ply) > 100000
    assert "Integrated 30 frames" in out.stdout and "written to" in out.stdout
    # meshlabserver -i X_vh.ply -o X_vh_clean.ply -m vc -s clean.mlx (scan_processor.py:143)
    mlx = tmp_path / "clean.mlx"
    mlx.write_text('<!DOCTYPE FilterScript>\n<FilterScript>\n <filter name="Merge Close Vertices">\n  <Param name="Threshold" value="0.0010689" type="RichAbsPerc"/>\n </filter>\n'
                   ' <filter name="Remove Duplicate Faces"/>\n <filter name="Remove Isolated pieces (wrt Face Num.)">\n  <Param name="MinComponentSize" value="7500" type="RichInt"/>\n </filter>\n'
                   ' <filter name="Remove Unreferenced Vertex"/>\n</FilterScript>\n')
    clean_ply = str(tmp_path / "scene0000_00_vh_clean.ply")
    cl = subprocess.run([os.path.join(ROOT, "bin", "meshclean"), "-i", ply, "-o", clean_ply, "-m", "vc", "-s", str(mlx)], capture_output=True, text=True)
    assert cl.returncode == 0 and cl.stderr == "", cl.stderr
    return params, ply, clean_ply


def test_drop_in_executables(tmp_path):
    """`depthsensing p1 p2 scan.sens` -> scan_vh.ply, then `segmentator scan_vh.ply` -> scan_vh.0.010000.segs.json;
    stderr stays empty (Server/util.py:42-44 logs stderr as an error)."""
    import hashlib
    params, ply, clean_ply = _drop_in_clean_mesh(tmp_path)
    from scannet_amd import segmentator
    nv0, nf0 = segmentator.Mesh.read(ply).counts()
    nv, nf = segmentator.Mesh.read(clean_ply).counts()
    assert 10000 < nf <= nf0 and nv <= nv0
    seg = subprocess.run([os.path.join(ROOT, "bin", "segmentator"), clean_ply], capture_output=True, text=True)
    assert seg.returncode == 0 and seg.stderr == ""
    js = json.load(open(str(tmp_path / "scene0000_00_vh_clean.0.010000.segs.json")))
    assert js["params"] == {"kThresh": 0.01, "segMinVerts": 20} and js["sceneId"] == "/scene0000_00_vh_clean"
    assert len(js["segIndices"]) == nv
    # north_star: "bit-exact on segIndices for a fixed kThresh" -- the REFERENCE Segmentator on the very mesh the GPU extracted and cleaned: same
    # segIndices, same file bytes.  Its bytes on this mesh are recorded in tests/golden/drop_in_segmentator_golden.json (make_drop_in_golden.py); where
    # oracle/_ref/segmentator_ref is built (compiled from the reference's own sources by oracle/Makefile) it runs here as well
    # (segmentator.cpp:253-287 writes beside its input, so it gets a copy of the mesh in a directory of its own)
    ours = open(str(tmp_path / "scene0000_00_vh_clean.0.010000.segs.json"), "rb").read()
    gold = json.load(open(DROP_IN_GOLDEN))
    regen = "regenerate with tests/golden/make_drop_in_golden.py (needs the reference build and a GPU)"
    assert _mesh_sha256(clean_ply) == gold["mesh_sha256"], "fusion, meshing or cleaning changed the mesh the reference's bytes were recorded on: " + regen
    assert hashlib.sha256(ours).hexdigest() == gold["segs_json_sha256"] and len(ours) == gold["segs_json_bytes"], \
        "bin/segmentator's segs.json differs from the reference's on this mesh (or the golden is stale: %s)" % regen
    assert len(set(js["segIndices"])) == gold["num_segments"] > 10          # a real over-segmentation, not one label
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "segmentator_ref")
    if os.path.exists(ref_bin):
        ref_dir = tmp_path / "ref"
        ref_dir.mkdir()
        shutil.copy(clean_ply, str(ref_dir / "scene0000_00_vh_clean.ply"))
        rr = subprocess.run([ref_bin, str(ref_dir / "scene0000_00_vh_clean.ply")], capture_output=True, text=True)
        assert rr.returncode == 0, rr.stderr
        theirs = open(str(ref_dir / "scene0000_00_vh_clean.0.010000.segs.json"), "rb").read()
        assert json.loads(theirs)["segIndices"] == js["segIndices"]
        assert ours == theirs
    # failure protocol: non-zero exit and a message on stderr
    bad = subprocess.run([os.path.join(ROOT, "bin", "depthsensing"), str(params), str(params), str(tmp_path / "missing.sens")], capture_output=True, text=True)
    assert bad.returncode != 0 and "could not open" in bad.stderr


def test_depthsensing_honours_the_shipped_integration_size(tmp_path):
    """The shipped parameter file integrates at s_integrationWidth x s_integrationHeight = 320 x 240 whatever the sensor delivers
    (zParametersScanNet.txt:20-21): `depthsensing` on a 640x480 .sens must say so and write the mesh a fuser created with
    integration_width / height = 320 / 240 produces from the same frames."""
    from scannet_amd import fusion, segmentator
    W, H = 640, 480
    sens_path = str(tmp_path / "scan.sens")
    frames = _write_sens(sens_path, 12, W, H, 600)
    params = tmp_path / "zParametersScanNet.txt"
    params.write_text("s_integrationWidth = 320;\ns_integrationHeight = 240;\ns_SDFVoxelSize = 0.010f;\ns_SDFTruncation = 0.06f;\n"
                      "s_SDFTruncationScale = 0.02f;\ns_hashNumSDFBlocks = 200000;\ns_hashNumBuckets = 100000;\n")
    (tmp_path / "t.txt").write_text("// tracking\n")
    out = subprocess.run([os.path.join(ROOT, "bin", "depthsensing"), str(params), str(tmp_path / "t.txt"), sens_path], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    assert "resampled to s_integrationWidth x s_integrationHeight = 320 x 240" in out.stdout
    got = segmentator.Mesh.read(str(tmp_path / "scan_vh.ply")).arrays()
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.load_params(str(params), fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my))
    assert (gp.integration_width, gp.integration_height, gp.depth_width) == (320, 240, 640)
    with fusion.Fuser(gp) as f:
        for d, pose in frames:
            f.integrate(d, pose)
        want = f.extract_mesh().arrays()
    assert len(want[2]) > 10000
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def _room_frames(n, W, H, total, stride=9):
    out = []
    for i in range(n):
        pose = synth.trajectory_pose(i * stride, total)
        out.append((synth.render_room_depth(pose, W, H, noise_frame=i), pose))
    return out


def test_slab_partition_matches_one_gpu():
    """configs[4] in miniature: the block space cut into 3 slabs along x, three fusers see every frame and fuse only their
    slab, boundary layers are exchanged as ghost blocks, the slab meshes concatenate into the one-fuser mesh byte for byte."""
    from scannet_amd import fusion, partition
    W, H = 320, 240
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.01, num_sdf_blocks=1 << 17)
    frames = _room_frames(24, W, H, 1200, stride=40)
    with fusion.Fuser(gp) as whole:
        for d, pose in frames:
            whole.integrate(d, pose)
        ref = whole.extract_mesh().arrays(keys=True)
        wc, wv = whole.export_blocks()
    world = 3
    planes = partition.planes_from_poses([p for _, p in frames], gp.voxel_size, gp.max_integration_dist, world)
    # the room spans x in [0, 6] m: put the inner planes inside it so that every slab owns surface
    planes[1], planes[2] = int(2.0 / 0.08), int(4.0 / 0.08)
    fusers = [fusion.Fuser(gp) for _ in range(world)]
    try:
        for r, f in enumerate(fusers):
            f.set_slab(0, planes[r], planes[r + 1])
            for d, pose in frames:
                f.integrate(d, pose)
        # the slabs partition the one-GPU block set, voxels bit-identical
        owned = [f.export_blocks() for f in fusers]
        assert sum(len(c) for c, _ in owned) == len(wc)
        allc = np.concatenate([c for c, _ in owned]); allv = np.concatenate([v for _, v in owned])
        order = np.lexsort((allc[:, 2], allc[:, 1], allc[:, 0]))
        assert np.array_equal(allc[order], wc) and np.array_equal(allv[order].view(np.uint8), wv.view(np.uint8))
        for r, (c, _) in enumerate(owned):
            assert len(c) > 100 and c[:, 0].min() >= planes[r] and c[:, 0].max() < planes[r + 1]
        # boundary exchange (in-process stand-in for the all-gather), then mesh per slab
        layers = [f.export_blocks_where(0, planes[r], planes[r] + 1) if r > 0 else (np.zeros((0, 3), np.int32), np.zeros((0, 512), fusion.VOXEL_DTYPE))
                  for r, f in enumerate(fusers)]
        gather = lambda c, v: ([l[0] for l in layers], [l[1] for l in layers])
        sent_got = [partition.exchange_boundary_layers(f, planes, r, gather=gather) for r, f in enumerate(fusers)]
        assert sent_got[0][1] > 0 and sent_got[1][1] > 0 and sent_got[2][1] == 0 and sent_got[1][0] == sent_got[0][1]
        for f, (c, _) in zip(fusers, owned):   # ghosts are not exported as owned blocks, not fused, not garbage-collected
            assert len(f.export_blocks_where(-1, 0, 0)[0]) == len(c)
        parts = [f.extract_mesh().arrays(keys=True) for f in fusers]
        xyz, rgba, tris, keys = partition.merge_slab_meshes(parts)
        assert np.array_equal(keys, ref[3]) and np.array_equal(xyz.view(np.uint32), ref[0].view(np.uint32))
        assert np.array_equal(rgba, ref[1]) and np.array_equal(tris, ref[2])
        # another frame after the exchange: ghosts stay untouched, owned blocks keep matching
        d, pose = frames[3]
        for f in fusers:
            f.integrate(d, pose)
        g0 = fusers[0].export_blocks_where(0, planes[1], planes[1] + 1, include_ghosts=True)
        assert np.array_equal(g0[1].view(np.uint8), layers[1][1].view(np.uint8))
    finally:
        for f in fusers:
            f.close()


@pytest.mark.parametrize("thickness", [4, 16])
def test_stripe_partition_device_resident_exchange_matches_one_gpu(thickness):
    """configs[4] with STRIPES (sf_fuser_set_stripes): block layers dealt round-robin to three fusers, so every frame's blocks spread over
    all of them.  The boundary exchange never touches host memory: sf_fuser_export_boundary into device buffers (torch tensors stand in
    for the all-gather output), sf_fuser_import_ghosts filters on the device.  Owned blocks partition the one-GPU block set bit for bit;
    the merged mesh (vertices by edge key, faces by cube key) is the one-GPU mesh byte for byte."""
    import torch
    from scannet_amd import fusion, partition
    W, H = 320, 240
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.01, num_sdf_blocks=1 << 17)
    frames = _room_frames(24, W, H, 1200, stride=40)
    with fusion.Fuser(gp) as whole:
        for d, pose in frames:
            whole.integrate(d, pose)
        ref = whole.extract_mesh()
        ref_arr, ref_fk = ref.arrays(keys=True), ref.face_keys()
        wc, wv = whole.export_blocks()
    world, origin = 3, -7
    fusers = [fusion.Fuser(gp) for _ in range(world)]
    try:
        for r, f in enumerate(fusers):
            f.set_stripes(0, origin, thickness, world, r)
            for d, pose in frames:
                f.integrate(d, pose)
        owned = [f.export_blocks() for f in fusers]
        assert sum(len(c) for c, _ in owned) == len(wc) and min(len(c) for c, _ in owned) > 0.2 * len(wc) / world
        allc = np.concatenate([c for c, _ in owned]); allv = np.concatenate([v for _, v in owned])
        order = np.lexsort((allc[:, 2], allc[:, 1], allc[:, 0]))
        assert np.array_equal(allc[order], wc) and np.array_equal(allv[order].view(np.uint8), wv.view(np.uint8))
        for r, (c, _) in enumerate(owned):
            assert all(partition.owner_of(x, origin, thickness, world) == r for x in np.unique(c[:, 0]))
        # exchange on the device
        payload = []
        for f in fusers:
            n = f.count_boundary()
            c = torch.empty((max(n, 1), 3), dtype=torch.int32, device="cuda")
            v = torch.empty((max(n, 1), 4096), dtype=torch.uint8, device="cuda")
            assert f.export_boundary(c, v) == n and n > 0
            payload.append((c[:n], v[:n]))
            cn, vn = f.export_boundary()                     # the host form returns the same blocks
            assert np.array_equal(np.sort(cn.view([("", cn.dtype)] * 3), axis=0), np.sort(c[:n].cpu().numpy().view([("", cn.dtype)] * 3), axis=0))
            assert all(partition.owner_of(x - 1, origin, thickness, world) != partition.owner_of(x, origin, thickness, world) for x in np.unique(cn[:, 0]))
        got = [sum(f.import_ghosts(c, v) for q, (c, v) in enumerate(payload) if q != r) for r, f in enumerate(fusers)]
        assert min(got) > 0
        for f, (c, _) in zip(fusers, owned):                 # ghosts are not owned blocks
            assert len(f.export_blocks_where(-1, 0, 0)[0]) == len(c)
        parts = []
        for f in fusers:
            m = f.extract_mesh()
            parts.append(m.arrays(keys=True) + (m.face_keys(),))
        xyz, rgba, tris, keys = partition.merge_slab_meshes(parts)
        assert np.array_equal(keys, ref_arr[3]) and np.array_equal(xyz.view(np.uint32), ref_arr[0].view(np.uint32))
        assert np.array_equal(rgba, ref_arr[1]) and np.array_equal(tris, ref_arr[2])
        assert np.all(np.diff(ref_fk.astype(np.int64)) >= 0)
    finally:
        for f in fusers:
            f.close()


def test_exchange_boundary_over_the_nccl_backend_on_one_gpu(tmp_path):
    """partition.exchange_boundary through torch.distributed with the nccl (= RCCL) backend, world size 1: the device export and the
    all-gather of device tensors run as they do on 8 GPUs (the import of the other ranks' layers is covered above)."""
    import socket
    import torch
    import torch.distributed as dist
    from scannet_amd import fusion, partition
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        W, H = 160, 120
        fx, fy, mx, my = synth.intrinsics(W, H)
        gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.02, num_sdf_blocks=1 << 15)
        with fusion.Fuser(gp) as f:
            f.set_stripes(0, 0, 2, 2, 0)     # this rank plays rank 0 of 2: it owns every other pair of layers
            for d, pose in _room_frames(4, W, H, 400, stride=30):
                f.integrate(d, pose)
            sent, got = partition.exchange_boundary(f)
            assert sent == f.count_boundary() and sent > 0 and got == 0
    finally:
        dist.destroy_process_group()


def _smooth_image(W, H, k):
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 255 // W + 9 * k) % 256, (yy * 255 // H), (128 + 100 * np.sin(xx / 11.0 + k) * np.cos(yy / 7.0))], -1)
    img[H // 4: H // 2, W // 3: 2 * W // 3] = (200, 30 + 20 * k, 60)
    return np.clip(img, 0, 255).astype(np.uint8)


def test_jpeg_gpu_reconstruction_equals_the_host_decoder():
    """sf_jpeg_decode_gpu (Huffman on the host, IDCT + chroma upsampling + colour conversion on the GPU: what sf_fuse_run does with
    colour frames) returns the bytes of the host decoder: 4:4:4, 4:2:2, 4:2:0, grey, sizes that are not multiples of the MCU."""
    import io
    from PIL import Image
    from scannet_amd import calibrate
    cases = 0
    for (W, H) in ((136, 104), (133, 99), (64, 48), (17, 9)):
        img = _smooth_image(W, H, cases)
        blobs = []
        for sub in (0, 1, 2):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG", quality=88, subsampling=sub)
            blobs.append(buf.getvalue())
        buf = io.BytesIO()
        Image.fromarray(img[..., 0]).save(buf, format="JPEG", quality=80)          # one component
        blobs.append(buf.getvalue())
        blobs.append(calibrate.jpeg_encode(img, 92, True))
        blobs.append(calibrate.jpeg_encode(img, 75, False))
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=85, subsampling=2, restart_marker_blocks=3)   # DRI / RSTn
        blobs.append(buf.getvalue())
        for b in blobs:
            host = calibrate.jpeg_decode(b, W, H)
            gpu = calibrate.jpeg_decode(b, W, H, device=0)
            assert np.array_equal(host, gpu), "%dx%d case %d: %d bytes differ" % (W, H, cases, (host != gpu).sum())
            cases += 1
    assert cases == 28
    W, H = 1296, 968                                   # ScanNet's colour size, 4:2:0 and 4:2:2
    img = _smooth_image(W, H, 3)
    img = np.clip(img.astype(np.int32) + np.random.default_rng(0).integers(-9, 10, img.shape), 0, 255).astype(np.uint8)   # busy blocks too
    for sub, q in ((True, 90), (False, 97)):
        b = calibrate.jpeg_encode(img, q, sub)
        assert np.array_equal(calibrate.jpeg_decode(b, W, H), calibrate.jpeg_decode(b, W, H, device=0))
    with pytest.raises(Exception):
        calibrate.jpeg_decode(b"\xff\xd8 not a jpeg", 8, 8, device=0)


def test_gpu_inflate_equals_zlib():
    """sf_zlib_inflate_gpu -- the depth frames' inflate as sf_fuse_run does it (csrc/inflate_gpu.hip: 1024 lanes tokenise a frame from guessed
    chunk starts iterated to their fixed point, a 256-lane workgroup copies in 1024-byte groups with the window in LDS) -- returns zlib's bytes: the
    streams of THIS LIBRARY's writer (one final fixed-Huffman block, as the reference's; the reference writer's own bytes are the next test) on depth
    frames, noise, constants; token lists no match finder would produce (runs that copy themselves, chains of short near matches, the longest distance, distances around the group size); corrupt
    streams fail with the host inflater's verdict; dynamic / multi-block streams are refused (the pipeline inflates those on the host)."""
    import zlib
    from scannet_amd import sens
    from scannet_amd._abi import ScanfuseError
    from tests import deflate_tools as dt
    from tests.test_inflate_lanes import token_cases
    rng = np.random.default_rng(0)
    frames = [synth.render_room_depth(synth.trajectory_pose(37 * k, 1200), 640, 480, noise_frame=k).tobytes() for k in range(4)]
    frames += [bytes(614400), rng.integers(0, 65536, 307200, dtype=np.uint16).tobytes(), (np.arange(76800, dtype=np.uint16) // 7).tobytes(), b"\x01\x02\x03\x04" * 25, b"abcd"]
    for raw in frames:
        z = sens.zlib_deflate(raw)
        assert zlib.decompress(z) == raw
        assert sens.zlib_inflate(z, len(raw), device=0) == raw
    for name, tokens in token_cases().items():
        want = dt.apply_tokens(tokens)
        pad = (-len(want)) % 4
        z = dt.zlib_stream(tokens + [0] * pad)
        assert sens.zlib_inflate(z, len(want) + pad, device=0) == want + bytes(pad), name
    lits = [int(v) for v in rng.integers(0, 256, 4000)]
    for bad, word in ((dt.zlib_stream(lits, end=False), "code"),      # "no end-of-block code", or the trailer read as tokens holds "an invalid code" first (dt.zlib_stream(lits[:2000] + [("sym", 286)] + lits[2000:]), "invalid code"),
                      (dt.zlib_stream(lits[:2000] + [("sym", 257), ("dist", 30)] + lits[2000:]), "invalid code"),
                      (dt.zlib_stream(lits[:10] + [(5, 11)] + lits[10:3995]), "in front of the output"), (dt.zlib_stream(lits + [1, 2, 3, 4]), "expected size")):
        with pytest.raises(ScanfuseError) as ei:
            sens.zlib_inflate(bad, 4000, device=0)
        assert word in str(ei.value), (word, str(ei.value))
        with pytest.raises(ScanfuseError):
            sens.zlib_inflate(bad, 4000)                     # the host inflater agrees
    for foreign in (zlib.compress(bytes(lits), 6), dt.zlib_stream(lits, header=(0, 1))):
        with pytest.raises(ScanfuseError) as ei:
            sens.zlib_inflate(foreign, 4000, device=0)
        assert "sf_zlib_inflate" in str(ei.value)
    # mutated streams: the device's verdict is the host inflater's -- the same bytes, or both refuse (and nothing faults)
    raw = synth.render_room_depth(synth.trajectory_pose(11, 1200), 320, 240, noise_frame=5).tobytes()
    z = bytearray(sens.zlib_deflate(raw))
    agree = [0, 0]
    for k in range(120):
        m = bytearray(z)
        if k % 4 == 0:
            i = int(rng.integers(2, len(m) - 4)); m[i] ^= 1 << int(rng.integers(0, 8))
        elif k % 4 == 1:
            i = int(rng.integers(2, len(m) - 4)); m[i] = int(rng.integers(0, 256))
        elif k % 4 == 2:
            m = m[: int(rng.integers(8, len(m)))]
        else:
            i = int(rng.integers(2, len(m) - 40)); m[i:i + 8] = bytes(rng.integers(0, 256, 8, dtype=np.uint8))
        m = bytes(m)
        try:
            host = sens.zlib_inflate(m, len(raw))
            host = host if len(host) == len(raw) else None
        except ScanfuseError:
            host = None
        try:
            dev = sens.zlib_inflate(m, len(raw), device=0)
        except ScanfuseError as e:
            if "goes to sf_zlib_inflate" in str(e):
                continue            # no longer one final fixed block: the pipeline hands it to the host inflater
            dev = None
        assert (dev is None) == (host is None) and dev == host, k
        agree[dev is None] += 1
    assert agree[0] >= 3 and agree[1] >= 40, agree


def _reference_written_frames(oracle, n_room, W=640, H=480, step=173, total=5578):
    """(frames [n, H, W] u16, poses [n, 4, 4]): furnished-room frames of the configs[1] walk with hashed noise, then a constant-zero, a constant and a noise frame."""
    rng = np.random.default_rng(9)
    poses = [synth.trajectory_pose((step * k) % total, total) for k in range(n_room)]
    frames = [synth.render_room_depth(poses[k], W, H, noise_frame=k, noise=2, boxes=synth.clutter_boxes()) for k in range(n_room)]
    return frames, poses, rng


def test_gpu_inflate_on_the_reference_writers_streams(oracle):
    """The bytes real ScanNet files hold: depth frames compressed by the REFERENCE writer (oracle/_ref/libref_sens.so = sensorData.h compiled where it
    lies: SensorData::createFrame -> compressDepth -> stb::stbi_zlib_compress(.., quality 8), sensorData.h:659-670, stb_image_write.h:721-823) --
    16 furnished 640x480 frames of the configs[1] walk, zeros, a constant, noise, a ramp -- through sf_zlib_inflate_gpu: zlib.decompress's bytes,
    which are the frames.  These are not the streams this library's writer makes (other matches, ~9 % more bytes)."""
    import zlib
    from scannet_amd import sens
    if not oracle.ref_sens_available() or not hasattr(oracle.ref_sens(), "ref_sens_add_frames_mt"):
        pytest.skip("oracle/_ref/libref_sens.so not built (needs /root/reference)")
    W, H = 640, 480
    frames, poses, rng = _reference_written_frames(oracle, 16)
    frames += [np.zeros((H, W), np.uint16), np.full((H, W), 2000, np.uint16), rng.integers(0, 65536, (H, W), dtype=np.uint16), (np.arange(W * H, dtype=np.uint32) // 7).astype(np.uint16).reshape(H, W)]
    P = np.stack(poses + [np.eye(4, dtype=np.float32)] * 4)
    blobs = oracle.ref_write_sens(None, np.stack(frames), P, synth.intrinsic_matrix(W, H), want_blobs=True)
    differ = 0
    for raw, z in zip(frames, blobs):
        raw = raw.tobytes()
        want = zlib.decompress(z)
        assert want == raw
        assert sens.zlib_inflate(z, len(raw), device=0) == want
        differ += z != sens.zlib_deflate(raw)
    assert differ >= 17, differ          # the reference's streams, not ours
    assert 300_000 < np.mean([len(z) for z in blobs[:16]]) < 520_000   # real-entropy depth: 0.5-0.85 of the pixels' bytes


def test_fuse_run_on_a_reference_written_sens_matches_the_oracle(oracle, tmp_path):
    """A whole .sens written by the reference writer (initDefault + createFrame per frame + saveToFile through libref_sens.so) -> sf_fuse_run with the
    device's inflate -> the volume oracle.Volume builds from the same frames (NOT the frame-by-frame GPU path: the checker is the CPU restatement),
    block set and voxels bit for bit; every depth frame was inflated on the device; the reference's own reader returns the frames the file was written from."""
    import ctypes as C
    from scannet_amd import fusion, sens
    if not oracle.ref_sens_available() or not hasattr(oracle.ref_sens(), "ref_sens_add_frames_mt"):
        pytest.skip("oracle/_ref/libref_sens.so not built (needs /root/reference)")
    W, H = 640, 480
    n = 40
    frames, poses, _ = _reference_written_frames(oracle, n, step=9)       # 40 consecutive-ish frames of the walk: two passes (32 + 8) of the batched schedule
    poses[7] = np.full((4, 4), -np.inf, np.float32)                         # tracking lost (sensorData.h:382): skipped
    p = str(tmp_path / "reference.sens")
    oracle.ref_write_sens(p, np.stack(frames), np.stack(poses), synth.intrinsic_matrix(W, H))
    R = oracle.ref_sens()
    h = R.ref_sens_open(p.encode())
    out = np.zeros((H, W), np.uint16)
    assert R.ref_sens_decode_depth(h, 5, out.ctypes.data_as(C.c_void_p)) == 0 and np.array_equal(out, frames[5])
    R.ref_sens_close(h)
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, num_sdf_blocks=1 << 18)
    op = oracle.default_params(W, H)
    ovol = oracle.Volume(op, threads=8)
    for i in range(n):
        if i != 7:
            ovol.integrate(frames[i], poses[i])
    sd = sens.SensorData(p)
    assert sd.depth_compression_type == "zlib_ushort" and sd.num_frames == n
    with fusion.Fuser(gp) as f:
        st = f.run(sd, decode_threads=3)
        assert (st["frames_total"], st["frames_integrated"], st["frames_skipped"]) == (n, n - 1, 1)
        assert (st["depth_inflated_on_device"], st["depth_inflated_on_host"]) == (n - 1, 0)
        gc, gv = f.export_blocks()
    oc, ov = ovol.export()
    assert np.array_equal(oc, gc), "allocated block sets differ"
    assert np.array_equal(ov.view(np.uint8), gv.view(np.uint8)), "voxels differ"


def test_a_corrupt_depth_frame_is_fused_as_no_measurement_not_as_stale_pixels(tmp_path):
    """a depth frame the device's inflate gives up on used to leave its slot's previous pixels (the frame NB batches earlier) to be fused
    under the new pose while the failure travelled to the host.  Now the copy kernel zero-fills such a frame (depth 0 = no measurement) and the run
    fails with SF_ERR_FORMAT: the volume is bit for bit what the file's other frames give."""
    from scannet_amd import fusion, sens
    from tests import deflate_tools as dt
    W, H = 320, 240
    good = str(tmp_path / "good.sens")
    frames = _write_sens(good, 100, W, H, 1200)
    bad = str(tmp_path / "bad.sens")
    import shutil
    shutil.copy(good, bad)
    short_tokens = list(range(250)) * 4 + [(258, 1000)] * 591 + [(118, 1000)]                # inflates to four bytes less than a frame: the device reports IL_ST_SIZE
    _recompress_depth_frames(bad, {70}, lambda raw: dt.zlib_stream(short_tokens))
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.008, num_sdf_blocks=1 << 17)
    with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b:
        with pytest.raises(Exception, match="inflate: depth frame 70"):
            a.run(sens.SensorData(bad), decode_threads=2)
        for i, (d, pose) in enumerate(frames):
            if i != 70:
                b.integrate(d, pose)
        ca, va = a.export_blocks()
        cb, vb = b.export_blocks()
    # the failure is read back when the run ends: every other frame of the file was fused, frame 70 as a frame without a single measurement
    assert np.array_equal(ca, cb), "the failed run's block set is not that of the file's valid frames: stale pixels were fused"
    assert np.array_equal(va.view(np.uint8), vb.view(np.uint8))


def test_jpeg_gpu_entropy_decoding_equals_the_host_decoder():
    """sf_jpeg_decode_gpu_huffman -- headers on the host, Huffman decoding by 1024 lanes per picture (csrc/jpeg_huff_gpu.hip: speculative chunk
    states iterated to their fixed point, prefix sums, a second decode that writes) and reconstruction on the GPU: what sf_fuse_run does with a
    colour frame -- returns the host decoder's bytes.  4:4:4 / 4:2:2 / 4:2:0 / 4:4:0 / grey, optimised (per-picture) Huffman tables, sizes
    that are not multiples of the MCU, one-MCU and one-chunk pictures, q 30 (short chunks, many rounds) to q 100 (every coefficient coded),
    noise (long codes), ScanNet's 1296x968.  Restart intervals are refused (sf_fuse_run decodes those on the host); corrupt streams fail."""
    import io
    from PIL import Image
    from scannet_amd import calibrate
    from scannet_amd._abi import ScanfuseError
    from tests import jpeg_tools
    rng = np.random.default_rng(11)
    cases = 0
    for (W, H) in ((136, 104), (133, 99), (64, 48), (17, 9), (1, 1), (8, 8), (1296, 968)):
        img = _smooth_image(W, H, cases)
        noisy = np.clip(img.astype(np.int32) + rng.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
        blobs = []
        for sub in (0, 1, 2):
            for q, opt, pic in ((88, False, img), (30, True, img), (100, False, noisy), (95, True, noisy)):
                if W > 1000 and (q == 100 or sub == 0):
                    continue
                buf = io.BytesIO()
                Image.fromarray(pic).save(buf, format="JPEG", quality=q, subsampling=sub, optimize=opt)
                blobs.append(buf.getvalue())
        buf = io.BytesIO()
        Image.fromarray(noisy[..., 0]).save(buf, format="JPEG", quality=80)          # one component
        blobs.append(buf.getvalue())
        blobs.append(calibrate.jpeg_encode(img, 92, True))
        blobs.append(calibrate.jpeg_encode(noisy, 75, False))
        if W < 1000:
            blobs.append(jpeg_tools.encode(noisy, ((1, 2), (1, 1), (1, 1)), qstep=3))          # 4:4:0
            blobs.append(jpeg_tools.encode(img, ((1, 1), (2, 2), (2, 2)), qstep=5))            # chroma finer than luma
        for b in blobs:
            host = calibrate.jpeg_decode(b, W, H)
            gpu = calibrate.jpeg_decode(b, W, H, device=0, device_huffman=True)
            assert np.array_equal(host, gpu), "%dx%d case %d: %d bytes differ" % (W, H, cases, (host != gpu).sum())
            cases += 1
    assert cases == 6 * 17 + 9
    W, H = 136, 104
    img = _smooth_image(W, H, 2)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=85, subsampling=2, restart_marker_blocks=3)   # DRI / RSTn: the host's
    with pytest.raises(ScanfuseError) as ei:
        calibrate.jpeg_decode(buf.getvalue(), W, H, device=0, device_huffman=True)
    assert "restart" in str(ei.value)
    good = calibrate.jpeg_encode(img, 90, True)
    cut = good[: len(good) * 2 // 3] + b"\xff\xd9"                   # the segment ends before the picture does
    with pytest.raises(ScanfuseError):
        calibrate.jpeg_decode(cut, W, H, device=0, device_huffman=True)
    with pytest.raises(ScanfuseError):
        calibrate.jpeg_decode(b"\xff\xd8 not a jpeg", 8, 8, device=0, device_huffman=True)


def test_jpeg_gpu_reconstruction_identical_to_the_reference_decoder(oracle, tmp_path):
    """The GPU reconstruction against the REFERENCE's decoder itself (SensorData::decompressColorAlloc -> stb_image, compiled from the
    reference's sources into oracle/_ref/libref_sens.so, which travels with the snapshot): integer work, identical bytes.  4:4:4 / 4:2:2
    (stb's last-column rule) / 4:2:0 / 4:4:0 / grey, odd sizes, restart intervals, and ScanNet's 1296x968."""
    import ctypes as C
    import io
    from PIL import Image
    from scannet_amd import calibrate, sens
    from tests import jpeg_tools
    if not oracle.ref_sens_available():
        pytest.skip("oracle/_ref/libref_sens.so absent")
    R = oracle.ref_sens()

    def ref_decode(blob, W, H):
        sd = sens.SensorData.create(W, H, 8, 8, np.eye(4), np.eye(4), color_compression=2, depth_compression=0)
        sd.add_frame(np.zeros((8, 8), np.uint16), np.eye(4), color=blob)
        p = str(tmp_path / "c.sens")
        sd.save(p)
        h = R.ref_sens_open(p.encode())
        ref = np.zeros((H, W, 3), np.uint8)
        assert R.ref_sens_decode_color(h, 0, ref.ctypes.data_as(C.c_void_p)) == 0
        R.ref_sens_close(h)
        return ref

    rng = np.random.default_rng(5)
    n = 0
    for (W, H) in ((136, 104), (133, 99), (17, 9), (1, 1), (1296, 968)):
        img = np.clip(_smooth_image(W, H, n).astype(np.int32) + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
        blobs = []
        for sub in (0, 1, 2):
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG", quality=90 if W > 1000 else 70 + 10 * sub, subsampling=sub, **({"restart_marker_blocks": 5} if sub == 1 else {}))
            blobs.append(buf.getvalue())
        if W < 1000:
            blobs.append(jpeg_tools.encode(img, ((1, 2), (1, 1), (1, 1)), qstep=3))
            blobs.append(jpeg_tools.encode(img[..., 0], ((1, 1),), qstep=2, restart=2))
            blobs.append(jpeg_tools.encode(img, ((1, 1), (2, 2), (2, 2)), qstep=5))
        for b in blobs:
            gpu = calibrate.jpeg_decode(b, W, H, device=0)
            assert np.array_equal(gpu, ref_decode(b, W, H)), (W, H, n)
            n += 1
    assert n == 27


@pytest.mark.parametrize("kind", ["raw", "jpeg", "jpeg_gpu_huffman", "jpeg_host_huffman", "jpeg_host"])
def test_fuse_run_with_colour_matches_frame_by_frame(tmp_path, kind, monkeypatch):
    """Colour at its own resolution through the threaded pipeline -- raw; JPEG as sf_fuse_run takes it by default (entropy decoding on the device, on the
    batch's side stream: the pictures travel as prepared segments in a pinned slot sized for THOSE; a picture the device does not take -- here every
    second one has another sampling layout than the scan's first -- is decoded by its host thread into a pageable buffer of its own); the same forced
    (SF_JPEG_GPU_HUFFMAN); JPEG entropy-decoded by the host threads and reconstructed on the GPU (SF_JPEG_HOST_HUFFMAN); JPEG decoded on the host
    altogether (SF_JPEG_HOST): the same voxels, colours included, as integrating the host-decoded frames one by one.  One frame has no pose, one no colour."""
    from scannet_amd import calibrate, fusion, sens
    W, H, CW, CH = 160, 120, 324, 242
    n = 37
    K = synth.intrinsic_matrix(W, H)
    KC = np.eye(4, dtype=np.float32)
    KC[0, 0], KC[1, 1], KC[0, 2], KC[1, 2] = 340.3, 338.1, 160.2, 119.7
    sd = sens.SensorData.create(CW, CH, W, H, KC, K, color_compression=2 if kind.startswith("jpeg") else 0, depth_compression=1)
    frames = []
    for i in range(n):
        pose = synth.trajectory_pose(i * 9, 1200)
        d = synth.render_room_depth(pose, W, H, noise_frame=i)
        img = _smooth_image(CW, CH, i)
        if i == 5:
            pose = np.full((4, 4), -np.inf, np.float32)
        color = None if i == 11 else (calibrate.jpeg_encode(img, 90, i % 2 == 0) if kind.startswith("jpeg") else img)
        if i == 16 and kind.startswith("jpeg"):   # a PROGRESSIVE picture in the scan (the reference decodes those too): no device path takes it, its host thread decodes it
            import io
            from PIL import Image
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="JPEG", quality=90, subsampling=2, progressive=True)
            color = buf.getvalue()
            assert b"\xff\xc2" in color
        sd.add_frame(d, pose, color=color, timestamp_depth=i)
        frames.append((d, pose))
    p = str(tmp_path / "c.sens")
    sd.save(p)
    sd.close()
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.016, num_sdf_blocks=1 << 16)
    gp.color_width, gp.color_height, gp.cfx, gp.cfy, gp.cmx, gp.cmy = CW, CH, 340.3, 338.1, 160.2, 119.7
    if kind == "jpeg_host":
        monkeypatch.setenv("SF_JPEG_HOST", "1")
    if kind == "jpeg_gpu_huffman":
        monkeypatch.setenv("SF_JPEG_GPU_HUFFMAN", "1")
    if kind == "jpeg_host_huffman":
        monkeypatch.setenv("SF_JPEG_HOST_HUFFMAN", "1")
    s = sens.SensorData(p)
    with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b:
        rs = a.run(s, decode_threads=5)
        assert rs["frames_total"] == n and rs["color_fused"] == 1
        if kind in ("jpeg", "jpeg_gpu_huffman"):      # frames 0, 2, 4, ... share the first frame's layout (5 has no pose); the odd ones fall back to their host thread
            assert rs["jpeg_entropy_on_device"] == 18 and rs["jpeg_entropy_on_host"] == 17, rs     # ... and frame 16 is progressive
        elif kind.startswith("jpeg"):
            assert rs["jpeg_entropy_on_device"] == 0 and rs["jpeg_entropy_on_host"] == 35, rs
        for i, (d, pose) in enumerate(frames):
            if i == 5:
                continue
            rgb = None if i == 11 else s.frames[i].decompress_color()
            assert b.integrate(d, pose, rgb=rgb)
        ca, va = a.export_blocks()
        cb, vb = b.export_blocks()
        oa, ob = np.lexsort(ca.T[::-1]), np.lexsort(cb.T[::-1])
        assert np.array_equal(ca[oa], cb[ob])
        assert np.array_equal(va[oa], vb[ob]), "voxels (sdf, weight, colour) differ"
        assert len(ca) > 500


def _write_small_scan(path, n, colour, mixed_layouts, lost, nocol):
    """Depth 160x120 (zlib) with colour 324x242 -- None, "raw" or "jpeg" (4:2:0, every second picture 4:4:4 when mixed_layouts) -- frame `lost` without a
    pose, frame `nocol` without colour: the (depth, pose) pairs and the fuser parameters."""
    from scannet_amd import calibrate, fusion, sens
    W, H, CW, CH = 160, 120, 324, 242
    K = synth.intrinsic_matrix(W, H)
    KC = np.eye(4, dtype=np.float32)
    KC[0, 0], KC[1, 1], KC[0, 2], KC[1, 2] = 340.3, 338.1, 160.2, 119.7
    if colour is None:
        sd = sens.SensorData.create(0, 0, W, H, K, K, depth_compression=1)
    else:
        sd = sens.SensorData.create(CW, CH, W, H, KC, K, color_compression=2 if colour == "jpeg" else 0, depth_compression=1)
    frames = []
    for i in range(n):
        pose = synth.trajectory_pose(i * 7, 1200)
        d = synth.render_room_depth(pose, W, H, noise_frame=i)
        if i == lost:
            pose = np.full((4, 4), -np.inf, np.float32)
        img = _smooth_image(CW, CH, i)
        color = None
        if colour is not None and i != nocol:
            color = calibrate.jpeg_encode(img, 90, not (mixed_layouts and i % 2)) if colour == "jpeg" else img
        sd.add_frame(d, pose, color=color, timestamp_depth=i)
        frames.append((d, pose))
    sd.save(path)
    sd.close()
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.016, num_sdf_blocks=1 << 16)
    if colour is not None:
        gp.color_width, gp.color_height, gp.cfx, gp.cfy, gp.cmx, gp.cmy = CW, CH, 340.3, 338.1, 160.2, 119.7
    return frames, gp


def _assert_run_equals_frame_by_frame(a, b, s, frames, colour):
    """Fuser `a` ran the scan `s`; `b` integrates the host-decoded frames one by one: the same blocks, byte for byte."""
    for i, (d, pose) in enumerate(frames):
        if not np.isfinite(pose[0, 0]):
            continue
        has_colour = colour and s.frames[i].color_size_bytes > 0
        assert b.integrate(d, pose, rgb=s.frames[i].decompress_color() if has_colour else None)
    ca, va = a.export_blocks()
    cb, vb = b.export_blocks()
    oa, ob = np.lexsort(ca.T[::-1]), np.lexsort(cb.T[::-1])
    assert np.array_equal(ca[oa], cb[ob])
    assert np.array_equal(va[oa].view(np.uint8), vb[ob].view(np.uint8)), "voxels (sdf, weight, colour) differ"
    assert len(ca) > 500


@pytest.mark.parametrize("colour", [None, "raw", "jpeg"])
def test_fuse_run_reuses_its_ring_slots(tmp_path, colour):
    """A run whose ring slots come round: 45 frames in batches of 4 are 12 batches over 6 slots (8 with JPEG colour), so every slot is refilled while the
    copies, the side-stream work and the pre-pass of its previous batch may still be in flight (`consumed` / `landed`).  Depth only (the device inflates),
    raw colour, and JPEG colour as taken by default -- pictures of two sampling layouts alternate, so every batch mixes prepared segments with pictures
    their host threads decode, and the packed copy is never taken.  One frame has no pose, one no colour."""
    from scannet_amd import fusion, sens
    n = 45
    p = str(tmp_path / "ring.sens")
    frames, gp = _write_small_scan(p, n, colour, mixed_layouts=True, lost=5, nocol=11)
    s = sens.SensorData(p)
    with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b:
        a.tune(batch=4)
        rs = a.run(s, decode_threads=5)
        assert (rs["frames_total"], rs["frames_integrated"], rs["frames_skipped"]) == (n, n - 1, 1), rs
        assert rs["color_fused"] == (1 if colour else 0)
        assert rs["depth_inflated_on_device"] == n - 1 and rs["depth_inflated_on_host"] == 0, rs
        if colour == "jpeg":
            assert rs["jpeg_entropy_on_device"] > 0 and rs["jpeg_entropy_on_host"] > 0, rs
            assert rs["jpeg_entropy_on_device"] + rs["jpeg_entropy_on_host"] == n - 2, rs
        _assert_run_equals_frame_by_frame(a, b, s, frames, colour)


@pytest.mark.parametrize("entropy", ["host", "device"])
def test_fuse_run_with_jpeg_colour_and_no_side_stream(tmp_path, entropy, monkeypatch):
    """JPEG colour when depth is not inflated on the device (SF_INFLATE_HOST): the batch has no side stream, and the pictures of a sub-batch are reconstructed
    on the fuser's input stream in front of its pre-pass.  By default the host threads entropy-decode; with SF_JPEG_GPU_HUFFMAN the device does that there too,
    out of the small pinned slot -- all pictures share one layout, so the second batch (five frames, all with pose and colour) takes the packed two-copy
    path and the first (a frame without pose, one without colour) the copy per frame."""
    from scannet_amd import fusion, sens
    n = 37
    p = str(tmp_path / "noside.sens")
    frames, gp = _write_small_scan(p, n, "jpeg", mixed_layouts=False, lost=5, nocol=11)
    monkeypatch.setenv("SF_INFLATE_HOST", "1")
    if entropy == "device":
        monkeypatch.setenv("SF_JPEG_GPU_HUFFMAN", "1")
    s = sens.SensorData(p)
    with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b:
        rs = a.run(s, decode_threads=5)
        assert (rs["frames_total"], rs["frames_integrated"], rs["frames_skipped"]) == (n, n - 1, 1) and rs["color_fused"] == 1, rs
        assert rs["depth_inflated_on_device"] == 0, rs
        assert rs["jpeg_entropy_on_device"] == (n - 2 if entropy == "device" else 0), rs
        assert rs["jpeg_entropy_on_device"] + rs["jpeg_entropy_on_host"] == n - 2, rs
        _assert_run_equals_frame_by_frame(a, b, s, frames, colour=True)


@pytest.mark.parametrize("res", ["own", "same"])
@pytest.mark.parametrize("layout", ["420", "444", "grey"])
def test_fuse_run_converts_the_looked_up_pixels_from_the_jpeg_planes(tmp_path, res, layout, monkeypatch):
    """Round 6: when every colour frame of a batch is a picture the device reconstructs, sf_fuse_run stops at the component planes (k_jpeg_idct) and the fuser's
    pre-pass upsamples and converts the ONE pixel per depth pixel it looks up (k_prepass, YccPicture) -- no RGB image per picture.  A scan whose pictures all share
    one layout (4:2:0 with the triangle filters, 4:4:4, grey), colour at its own resolution (the look-up under the depth pixel's ray, odd sizes) or at the depth
    resolution, a frame count and an image size that leave partial batches and partial workgroups: the same voxels, colours included, as integrating the
    host-decoded frames one by one, and as the run that writes the RGB images out (SF_JPEG_RGB_IMAGE=1)."""
    import io
    from PIL import Image
    from scannet_amd import fusion, sens
    W, H = 160, 120
    CW, CH = (323, 241) if res == "own" else (W, H)
    n = 45
    K = synth.intrinsic_matrix(W, H)
    fx, fy, mx, my = synth.intrinsics(W, H)
    KC = np.eye(4, dtype=np.float32)
    if res == "own":
        KC[0, 0], KC[1, 1], KC[0, 2], KC[1, 2] = 340.3, 338.1, 160.2, 119.7
    else:
        KC[:] = K
    sd = sens.SensorData.create(CW, CH, W, H, KC, K, color_compression=2, depth_compression=1)
    frames = []
    for i in range(n):
        pose = synth.trajectory_pose(i * 7, 1200)
        d = synth.render_room_depth(pose, W, H, noise_frame=i)
        img = _smooth_image(CW, CH, i)
        buf = io.BytesIO()
        if layout == "grey":
            Image.fromarray(img[..., 1]).save(buf, format="JPEG", quality=88)
        else:
            Image.fromarray(img).save(buf, format="JPEG", quality=88, subsampling=2 if layout == "420" else 0)
        sd.add_frame(d, pose, color=buf.getvalue(), timestamp_depth=i)
        frames.append((d, pose))
    p = str(tmp_path / "y.sens")
    sd.save(p)
    sd.close()
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.016, num_sdf_blocks=1 << 16)
    if res == "own":
        gp.color_width, gp.color_height, gp.cfx, gp.cfy, gp.cmx, gp.cmy = CW, CH, 340.3, 338.1, 160.2, 119.7
    s = sens.SensorData(p)
    with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b, fusion.Fuser(gp) as c:
        rs = a.run(s, decode_threads=3)
        assert rs["frames_total"] == n and rs["color_fused"] == 1 and rs["jpeg_entropy_on_device"] == n, rs
        monkeypatch.setenv("SF_JPEG_RGB_IMAGE", "1")
        rc = c.run(s, decode_threads=3)
        monkeypatch.delenv("SF_JPEG_RGB_IMAGE")
        assert rc["jpeg_entropy_on_device"] == n
        for i, (d, pose) in enumerate(frames):
            assert b.integrate(d, pose, rgb=s.frames[i].decompress_color())
        ca, va = a.export_blocks()
        cb, vb = b.export_blocks()
        cc, vc = c.export_blocks()
        oa, ob, oc = np.lexsort(ca.T[::-1]), np.lexsort(cb.T[::-1]), np.lexsort(cc.T[::-1])
        assert np.array_equal(ca[oa], cb[ob]) and np.array_equal(ca[oa], cc[oc])
        assert np.array_equal(va[oa], vb[ob]), "voxels (sdf, weight, colour) differ from the host-decoded frames'"
        assert np.array_equal(va[oa], vc[oc]), "voxels differ from the RGB-image run's"
        assert len(ca) > 500 and (va["r"] > 0).any()


def test_shard_main_runs_the_whole_chain(tmp_path, capsys, monkeypatch):
    """python -m scannet_amd.shard on two small scans (one process, no process group): the GPU part of the second scan runs while host
    threads clean, decimate (twice) and segment the first; every output file of the reference's improve / decimate / segment stages."""
    from scannet_amd import segmentator, shard
    paths = []
    for k, n in enumerate((24, 16)):
        p = str(tmp_path / ("scene%d.sens" % k))
        _write_sens(p, n, 320, 240, 1200)
        paths.append(p)
    lst = tmp_path / "scans.txt"
    lst.write_text("\n".join(paths) + "\n")
    monkeypatch.setenv("SF_HOST_WORKERS", "2")
    shard.main([str(lst)])
    out = capsys.readouterr().out
    assert out.count("rank 0:") == 2
    for p in paths:
        base = os.path.splitext(p)[0]
        for suffix in ("_vh.ply", "_vh_clean.ply", "_vh_clean_2.ply", "_vh_clean_2.0.010000.segs.json"):
            assert os.path.getsize(base + suffix) > 0, suffix
        hi = segmentator.Mesh.read(base + "_vh_clean.ply").counts()[1]
        lo = segmentator.Mesh.read(base + "_vh_clean_2.ply").counts()[1]
        assert hi > 20000 and lo < 0.06 * hi          # 20 % of 20 %, minus what cleanLoRes drops
        segs = json.load(open(base + "_vh_clean_2.0.010000.segs.json"))
        assert len(segs["segIndices"]) == segmentator.Mesh.read(base + "_vh_clean_2.ply").counts()[0]
    # the cleaning filters ran on the GPU (the default of the tool): with --host-clean every file is byte for byte the same
    first = {p: {sfx: open(os.path.splitext(p)[0] + sfx, "rb").read() for sfx in ("_vh_clean.ply", "_vh_clean_2.ply", "_vh_clean_2.0.010000.segs.json")} for p in paths}
    shard.main([str(lst), "--host-clean"])
    capsys.readouterr()
    for p in paths:
        for sfx, blob in first[p].items():
            assert open(os.path.splitext(p)[0] + sfx, "rb").read() == blob, (p, sfx)
    # --gpu-decimate is the default spelled out (accepted for old command lines): the same files again
    shard.main([str(lst), "--gpu-decimate"])
    capsys.readouterr()
    for p in paths:
        for sfx, blob in first[p].items():
            assert open(os.path.splitext(p)[0] + sfx, "rb").read() == blob, (p, sfx)
    # --host-decimate pins the SEQUENTIAL filter (the restatement of MeshLab's greedy collapse, what rounds 1-3 shipped as the default): the cleaned mesh is
    # the same file, the decimated one has other triangles than the GPU's rounds -- and is exactly what the library's host filters give for the two scripts
    from scannet_amd import meshclean
    shard.main([str(lst), "--host-decimate"])
    capsys.readouterr()
    for p in paths:
        base = os.path.splitext(p)[0]
        assert open(base + "_vh_clean.ply", "rb").read() == first[p]["_vh_clean.ply"]
        host2 = open(base + "_vh_clean_2.ply", "rb").read()
        assert host2 != first[p]["_vh_clean_2.ply"]
        hi = segmentator.Mesh.read(base + "_vh_clean.ply").counts()[1]
        lo = segmentator.Mesh.read(base + "_vh_clean_2.ply").counts()[1]
        assert 0 < lo < 0.06 * hi
        m1, st1 = meshclean.simplify(segmentator.Mesh.read(base + "_vh_clean.ply"))          # the sequential filter, twice, as the stage runs simplify.mlx
        m2, st2 = meshclean.simplify(m1)
        assert st1["rounds"] == 0 and st2["rounds"] == 0 and abs(m2.counts()[1] - lo) <= max(8, lo // 10)   # cleanLoRes.mlx may drop small components behind it
    with pytest.raises(SystemExit):
        shard.main([str(lst), "--no-such-flag"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# configs[4] with REAL fusers in separate processes (the exchange had only run with real fusers at world size 1 and with a
# fake fuser at world size 2).  Two or three processes share GPU 0 -- RCCL refuses two ranks on one device, so the process group is gloo and
# the payload is staged through host memory; everything else is the multi-GPU path: one fuser per process with its stripes, every frame seen
# by every rank, partition.exchange_boundary (ring shift to the neighbour that needs the layers), marching cubes per rank, merge by key.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _partition_worker(rank, world, port, out_dir, mode, thickness):
    import sys
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from scannet_amd import fusion, partition
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        W, H = 320, 240
        fx, fy, mx, my = synth.intrinsics(W, H)
        gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.01, num_sdf_blocks=1 << 17)
        frames = _room_frames(24, W, H, 1200, stride=40)
        with fusion.Fuser(gp) as f:
            f.set_stripes(0, -7, thickness, world, rank)
            for d, pose in frames:
                f.integrate(d, pose)
            oc, ov = f.export_blocks()
            sent, got = partition.exchange_boundary(f, mode=mode)
            assert len(f.export_blocks_where(-1, 0, 0)[0]) == len(oc)      # ghosts are not owned blocks
            m = f.extract_mesh()
            xyz, rgba, tris, keys = m.arrays(keys=True)
            np.savez(os.path.join(out_dir, "part%d.npz" % rank), xyz=xyz, rgba=rgba, tris=tris, keys=keys, fk=m.face_keys(), oc=oc, ov=ov.view(np.uint8),
                     sent=sent, got=got, bytes_in=partition.exchange_boundary.last_bytes)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,mode,thickness", [(2, "neighbour", 4), (3, "neighbour", 16), (2, "all_gather", 16)])
def test_real_fusers_in_separate_processes_exchange_and_merge(tmp_path, world, mode, thickness):
    import socket
    import torch.multiprocessing as mp
    from scannet_amd import fusion, partition
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_partition_worker, args=(world, port, str(tmp_path), mode, thickness), nprocs=world, join=True)
    W, H = 320, 240
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, fx=fx, fy=fy, mx=mx, my=my, voxel_size=0.01, num_sdf_blocks=1 << 17)
    with fusion.Fuser(gp) as whole:
        for d, pose in _room_frames(24, W, H, 1200, stride=40):
            whole.integrate(d, pose)
        ref = whole.extract_mesh().arrays(keys=True)
        wc, wv = whole.export_blocks()
    parts = [np.load(str(tmp_path / ("part%d.npz" % r))) for r in range(world)]
    # the ranks' owned blocks partition the one-fuser volume, bit for bit
    allc = np.concatenate([p["oc"] for p in parts]); allv = np.concatenate([p["ov"] for p in parts])
    order = np.lexsort((allc[:, 2], allc[:, 1], allc[:, 0]))
    assert np.array_equal(allc[order], wc) and np.array_equal(allv[order].reshape(len(wc), -1), wv.view(np.uint8).reshape(len(wc), -1))
    # every rank sent its boundary and received ghosts; with the ring shift exactly the wanted blocks travelled
    assert all(int(p["sent"]) > 0 and int(p["got"]) > 0 for p in parts)
    if mode == "neighbour":
        assert all(int(p["bytes_in"]) == 4108 * int(p["got"]) for p in parts)
        assert sum(int(p["got"]) for p in parts) == sum(int(p["sent"]) for p in parts)
    # the merged mesh is the one-fuser mesh, byte for byte
    xyz, rgba, tris, keys = partition.merge_slab_meshes([(p["xyz"], p["rgba"], p["tris"], p["keys"], p["fk"]) for p in parts])
    assert np.array_equal(keys, ref[3]) and np.array_equal(xyz.view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(rgba, ref[1]) and np.array_equal(tris, ref[2])


def test_bench_with_two_ranks_sharing_one_gpu():
    """A BARE `python bench.py --gpus 2 ...` (no launcher in the command: bench.py re-executes itself under torch.distributed.run) runs two ranks:
    one process per rank, barriers, max over ranks, the roofline window on every rank, the partition's ring shift and the merged-mesh check --
    on a one-GPU box `--share-gpu` puts both ranks on GPU 0 over gloo.  A pass that only rank 0 enters hangs the job; a --gpus that is parsed and
    never read measures one GPU (round 3).  The rates mean nothing here.  --full: the roofline window, the exchange and the prefix check are
    measured beside the metric, which a plain run leaves out."""
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    import tempfile
    for extra in (["--full", "--steps", "64", "--warmup", "5", "--repeats", "3", "--no-pmc"], ["--full", "--config", "partition", "--scan-frames", "600"]):
        detail = os.path.join(tempfile.mkdtemp(prefix="sf_bench_"), "detail.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu"] + extra,
                           capture_output=True, text=True, cwd=ROOT, timeout=600, env=dict(env, SF_BENCH_DETAIL=detail))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-1500:]          # rank 0 prints ONE line
        line = json.loads(lines[0])                       # ... the compact record (< 4 KB, the last line of stdout); the full measurement is in the detail file
        assert len(lines[0]) < 4096 and r.stdout.rstrip().splitlines()[-1] == lines[0] and line["detail"] == detail
        j = json.load(open(detail))
        assert line["value"] == j["value"] and line["n_gpus"] == 2 and line["process_group"] == "gloo"
        assert j["n_gpus"] == 2 and j["value"] > 0 and j["unit"] == "frames/s" and j["process_group"] == "gloo"
        if "partition" in extra:
            assert j["exchange"]["mode"] == "neighbour" and j["exchange"]["boundary_blocks_sent_total"] == j["exchange"]["ghost_blocks_received_total"] > 0
            pc = j["prefix_check"]
            assert pc["sha256_equal"] and pc["faces"] > 10000 and pc["boundary_blocks_sent"] == pc["ghost_blocks_received"] > 0
        else:
            assert j["repeats"]["n"] == 3 and j["roofline"]["launches"] > 0
            assert len(j["per_rank_frames_per_s"]) == 2 and min(j["per_rank_frames_per_s"]) > 0
            assert j["config"]["rgbd"] is True and j["value_rgbd"] == j["value"]


def test_a_plain_bench_run_is_lean(tmp_path):
    """`python bench.py --gpus 1 --steps N --warmup W` does what its headline figure needs and nothing else: the contract's keys, the dumped
    volume, no leg beside the metric (those sit behind --full) -- and at most 30 s of the whole run, from start to exit, lie outside its
    N + W steps."""
    import sys
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    detail, dump = str(tmp_path / "detail.json"), str(tmp_path / "dump")
    n, w = 20, 5
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(n), "--warmup", str(w), "--dump-outputs", dump],
                       capture_output=True, text=True, cwd=ROOT, timeout=600, env=dict(env, SF_BENCH_DETAIL=detail))
    wall = time.perf_counter() - t0
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 4096 and r.stdout.rstrip().splitlines()[-1] == lines[0]
    line = json.loads(lines[0])
    assert line["metric"].startswith("RGB-D frames/sec integrated") and line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == n and line["warmup"] == w and line["value"] > 0 and line["ms_per_step"] > 0 and line["roofline"] is None
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1.0      # one GPU: frames/s x ms per frame
    j = json.load(open(detail))
    assert j["value"] == line["value"] and j["repeats"]["n"] == 1 and j["config"]["rgbd"] is True and j["config"]["alloc_failures"] == 0
    for leg in ("cpu_baseline", "parity", "parity_depth_only", "end_to_end", "end_to_end_rgbd", "roofline_single_frame", "roofline_depth_only",
                "roofline_out_of_cache", "value_depth_only"):
        assert leg not in j, leg
    coords = np.load(os.path.join(dump, "block_coords.npy"))
    assert len(coords) == j["config"]["blocks_live_end"] > 0 and np.load(os.path.join(dump, "sample_weight.npy")).max() > 0
    outside = wall - (n + w) * line["ms_per_step"] * 1e-3
    print("plain bench run: %.1f s from start to exit, %.1f s outside its %d steps" % (wall, outside, n + w))
    assert outside <= 30.0, outside


def test_bench_refuses_more_ranks_than_gpus_and_a_mismatched_launcher():
    """`--gpus N` on a node with fewer GPUs refuses (unless --share-gpu); a launcher that started a different number of ranks than --gpus names is
    refused too -- no line with the wrong n_gpus can come out."""
    import sys
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "4", "--warmup", "1"], capture_output=True, text=True, cwd=ROOT, timeout=300, env=env)
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout) and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"], capture_output=True, text=True, cwd=ROOT, timeout=300,
                       env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout) and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_match_upstream_tool_finds_the_switches_a_mesh_was_fused_with(tmp_path):
    """tools/match_upstream.py: a `_vh.ply` fused with a known switch combination is handed in as "the reference binary's output";
    the tool fuses the same .sens under every combination and must rank the right one first with nothing unmatched."""
    import sys
    from scannet_amd import fusion, sens
    W, H, N = 160, 120, 24
    K = synth.intrinsic_matrix(W, H)
    sd = sens.SensorData.create(W, H, W, H, K, K, color_compression=0, depth_compression=1, sensor_name="StructureSensor")
    rng = np.random.default_rng(4)
    for i in range(N):
        pose = synth.trajectory_pose(11 * i, 1200)
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rgb[:, : W // 3] = 0
        sd.add_frame(synth.render_room_depth(pose, W, H, noise_frame=i), pose, color=rgb, timestamp_depth=i)
    path = str(tmp_path / "scan.sens")
    sd.save(path)
    params = str(tmp_path / "p.txt")
    open(params, "w").write("s_SDFVoxelSize = 0.02f;\ns_hashNumSDFBlocks = 32768;\ns_hashNumBuckets = 16384;\ns_SDFIntegrationWeightMax = 99999999;\n")
    truth = dict(frustum_mode=1, colour_round=1, colour_first=0, weight_mode=0, weight_wrap=0)
    p = fusion.load_params(params)
    fx, fy, mx, my = synth.intrinsics(W, H)
    p.depth_width, p.depth_height, p.fx, p.fy, p.mx, p.my = W, H, fx, fy, mx, my
    for k, v in truth.items():
        setattr(p, k, v)
    with fusion.Fuser(p) as f:
        f.run(sens.SensorData(path))
        f.extract_mesh().write_ply(str(tmp_path / "ref_vh.ply"))
    out = str(tmp_path / "rank.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "match_upstream.py"), path, str(tmp_path / "ref_vh.ply"), "--params", params,
                        "--fix", "weight_mode=0", "--fix", "weight_wrap=0", "--json", out], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    rank = json.load(open(out))
    assert len(rank) == 8
    assert rank[0]["switches"] == truth and rank[0]["score"]["unmatched"] == 0.0 and rank[0]["score"]["mean_m"] == 0.0 and rank[0]["score"]["colour"] == 0.0
    # the other frustum rule and the other rounding are visibly worse
    assert rank[-1]["score"]["unmatched"] > 0 or rank[-1]["score"]["colour"] > 0
    assert "s_scanfuseFrustumMode = 1;" in r.stdout and "s_scanfuseColourRound = 1;" in r.stdout
