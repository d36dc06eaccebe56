"""Re-integration on the MI355X (`-m gpu`): sf_fuser_reintegrate_batch_device / sf_fuser_reintegrate / sf_fuse_update_trajectory against the oracle's
Volume.deintegrate / .integrate called in sequence, bit for bit.  Inputs are seeded / closed-form (scannet_amd/synth.py)."""
import ctypes as C

import numpy as np
import pytest

from scannet_amd import synth

pytestmark = pytest.mark.gpu

W, H = 320, 240
LOST = np.full((4, 4), -np.inf, np.float32)


def _gparams(voxel=0.008, **over):
    from scannet_amd import fusion
    fx, fy, mx, my = synth.intrinsics(W, H)
    gp = fusion.default_params(depth_width=W, depth_height=H, voxel_size=voxel, fx=fx, fy=fy, mx=mx, my=my, num_sdf_blocks=over.pop("num_sdf_blocks", 1 << 17))
    for k, v in over.items():
        setattr(gp, k, v)
    return gp


def _mk(oracle, voxel=0.008, **over):
    gp = _gparams(voxel, **over)
    op = oracle.default_params(W, H, voxel)
    op.fx, op.fy, op.mx, op.my = gp.fx, gp.fy, gp.mx, gp.my
    for k, v in over.items():
        if hasattr(op, k):
            setattr(op, k, v)
    return op, gp


def _colour_under_the_depth_rays(gp, big):
    """What the pre-pass looks up for colour at its own resolution (nearest pixel under the depth pixel's ray, black outside), in numpy, for the oracle:
    tests/test_gpu_tsdf.py::test_colour_at_its_own_resolution."""
    CW, CH = gp.color_width, gp.color_height
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    u = (((xs - np.float32(gp.mx)) / np.float32(gp.fx)).astype(np.float64) * np.float64(np.float32(gp.cfx)) + np.float64(np.float32(gp.cmx))).astype(np.float32) + np.float32(0.5)
    v = (((ys - np.float32(gp.my)) / np.float32(gp.fy)).astype(np.float64) * np.float64(np.float32(gp.cfy)) + np.float64(np.float32(gp.cmy))).astype(np.float32) + np.float32(0.5)
    ok = (u >= 0) & (u < CW) & (v >= 0) & (v < CH)
    iu, iv = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
    return np.where(ok[None, ..., None], big[:, iv, iu], 0).astype(np.uint8)


def _assert_same(ovol, fuser):
    oc, ov = ovol.export()
    gc, gv = fuser.export_blocks()
    assert len(oc) == len(gc), "block count differs: oracle %d gpu %d" % (len(oc), len(gc))
    assert np.array_equal(oc, gc), "allocated block sets differ"
    same = ov.view(np.uint8).reshape(len(oc), -1) == gv.view(np.uint8).reshape(len(gc), -1)
    if not same.all():
        bad = np.argwhere(~same.reshape(len(oc), 512, 8).all(-1))
        b, v = bad[0]
        raise AssertionError("%d voxels differ; first: block %s voxel %d oracle %s gpu %s" % (len(bad), oc[b], v, ov[b, v], gv[b, v]))


class _Device:
    """Frames (and colour frames) resident in HBM for the *_device entry points."""

    def __init__(self, depth, rgb=None):
        from scannet_amd import _abi
        self.L = _abi.lib()
        self.depth = np.ascontiguousarray(depth, np.uint16)
        self.stride = self.depth[0].nbytes
        self.d = C.c_void_p()
        _abi.check(self.L.sf_device_malloc(0, self.depth.nbytes, C.byref(self.d)))
        _abi.check(self.L.sf_device_upload(self.d, self.depth.ctypes.data_as(C.c_void_p), self.depth.nbytes))
        self.c, self.cstride = None, 0
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, np.uint8)
            self.cstride = rgb[0].nbytes
            self.c = C.c_void_p()
            _abi.check(self.L.sf_device_malloc(0, rgb.nbytes, C.byref(self.c)))
            _abi.check(self.L.sf_device_upload(self.c, rgb.ctypes.data_as(C.c_void_p), rgb.nbytes))

    def frame(self, k):
        return self.d.value + k * self.stride, (self.c.value + k * self.cstride if self.c else None)

    def close(self):
        self.L.sf_device_free(self.d)
        if self.c:
            self.L.sf_device_free(self.c)


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _perturbed(pose, rng, degrees=1.0, sigma=0.03):
    """The issue's perturbation: a `degrees` rotation about a random axis left-multiplied on R, a translation normal(3) * sigma / sqrt(3) m."""
    p = np.array(pose, np.float64).reshape(4, 4)
    q = p.copy()
    q[:3, :3] = _rot(rng.normal(size=3), np.deg2rad(degrees)) @ p[:3, :3]
    q[:3, 3] = p[:3, 3] + rng.normal(size=3) * sigma / np.sqrt(3)
    return q.astype(np.float32)


def _room(indices, total=1200, colour=False, csize=None, seed=3):
    rng = np.random.default_rng(seed)
    poses = [synth.trajectory_pose(i, total).astype(np.float32) for i in indices]
    depth = np.stack([synth.render_room_depth(p, W, H, noise_frame=i) for p, i in zip(poses, indices)])
    rgb = None
    if colour:
        ch, cw = csize if csize else (H, W)
        rgb = rng.integers(0, 256, (len(indices), ch, cw, 3), dtype=np.uint8)
        rgb[:, ::7] //= 3   # some structure besides noise
    return depth, np.stack(poses), rgb


def _sequence(vol, depth, rgb, old, new):
    """The contract's sequence on the oracle (or on a Fuser: same method names): deintegrate at the old pose, integrate at the new one, lost poses skipped."""
    last = None
    for k in range(len(depth)):
        c = None if rgb is None else rgb[k]
        if old[k].reshape(-1)[0] != -np.inf:
            last = vol.deintegrate(depth[k], old[k], rgb=c)
        if new[k].reshape(-1)[0] != -np.inf:
            last = vol.integrate(depth[k], new[k], rgb=c)
    return last


def _core_case():
    idx = list(range(0, 1200, 50))
    depth, true, _ = _room(idx)
    rng = np.random.default_rng(7)
    drift = np.stack([_perturbed(p, rng) for p in true])
    return depth, true, drift


def test_core_two_passes_match_the_oracle_sequence(oracle):
    """24 frames fused at poses about 1 degree / 3 cm off, then all 24 corrected in one call: two mixed-sign passes (16 + 8 frames).  Before anything
    is compared the oracle alone must show that the case exercises both halves: a + slot allocated, a - slot emptied voxels."""
    from scannet_amd import fusion
    depth, true, drift = _core_case()
    op, gp = _mk(oracle)
    ovol = oracle.Volume(op, threads=8)
    for k in range(len(depth)):
        ovol.integrate(depth[k], drift[k])
    c0, v0 = ovol.export()
    last = _sequence(ovol, depth, None, drift, true)
    c1, v1 = ovol.export()
    assert len(c1) > len(c0), "no + slot allocated a block"
    key0 = {tuple(c): i for i, c in enumerate(c0)}
    rows = np.array([key0.get(tuple(c), -1) for c in c1])
    kept = rows >= 0
    emptied = int(((v0["w"][rows[kept]] > 0) & (v1["w"][kept] == 0)).sum())
    assert emptied > 0, "no - slot took a voxel back to weight 0"
    print("blocks %d -> %d, %d voxels emptied" % (len(c0), len(c1), emptied))
    dev = _Device(depth)
    try:
        with fusion.Fuser(gp) as f:
            f.integrate_batch_device(dev.d.value, dev.stride, drift)
            f.reintegrate_batch_device(dev.d.value, dev.stride, drift, true)
            st = f.stats()
            assert st["frames_integrated"] == 24 + 48 and st["frames_skipped"] == 0 and st["alloc_failures"] == 0
            assert st["last_frame_blocks"] == last and st["blocks_allocated"] == len(c1)
            _assert_same(ovol, f)
            # the volume serves its readers as any other: one assertion each (they read the tiles compared above)
            d, _, _ = f.raycast(true[0], color=False)
            assert np.isfinite(d).mean() > 0.5
            assert f.extract_mesh().counts()[1] > 1000
    finally:
        dev.close()


@pytest.mark.parametrize("case", ["rgb", "rgb_own_size", "preset1", "preset2", "weight_sample3", "batch6"])
def test_colour_presets_and_generic_bodies(oracle, case):
    """The same correction with colour (at depth size and at its own), under the two upstream presets (colour_first, colour_round, weight_wrap,
    block-centre frustum; preset 1 also the depth-dependent weight), with weight_sample 3 (table division, generic weight) and in passes of 6 slots."""
    from scannet_amd import fusion, _abi
    over = {}
    csize = None
    if case == "rgb_own_size":
        csize = (300, 400)
        over = dict(color_width=400, color_height=300, cfx=620.5, cfy=618.25, cmx=199.5, cmy=149.75)   # narrower than the depth camera: a black rim
    if case == "weight_sample3":
        over = dict(weight_sample=3)
    idx = list(range(0, 1200, 100))
    depth, true, rgb = _room(idx, colour=True, csize=csize)
    rng = np.random.default_rng(17)
    drift = np.stack([_perturbed(p, rng) for p in true])
    op, gp = _mk(oracle, **over)
    if case in ("preset1", "preset2"):
        which = 1 if case == "preset1" else 2
        _abi.check(_abi.lib().sf_params_upstream_preset(C.byref(gp), which))
        for k in ("frustum_mode", "colour_round", "colour_first", "weight_mode", "weight_wrap"):
            setattr(op, k, getattr(gp, k))
        gp.weight_max = op.weight_max = 99999999
    ovol = oracle.Volume(op, threads=8)
    orgb = _colour_under_the_depth_rays(gp, rgb) if case == "rgb_own_size" else rgb
    for k in range(len(depth)):
        ovol.integrate(depth[k], drift[k], rgb=orgb[k])
    last = _sequence(ovol, depth, orgb, drift, true)
    dev = _Device(depth, rgb)
    try:
        with fusion.Fuser(gp, **({"batch": 6} if case == "batch6" else {})) as f:
            f.integrate_batch_device(dev.d.value, dev.stride, drift, d_rgb=dev.c.value, rgb_stride_bytes=dev.cstride)
            f.reintegrate_batch_device(dev.d.value, dev.stride, drift, true, d_rgb=dev.c.value, rgb_stride_bytes=dev.cstride)
            assert f.stats()["last_frame_blocks"] == last
            _assert_same(ovol, f)
            assert (f.export_blocks()[1]["r"] > 0).any()
    finally:
        dev.close()


def _mixed_case():
    """Large pose jumps (blocks born in the middle of a pass), frames that only enter (old lost), only leave (new lost) or do neither, and a frame
    (k = 5) whose OLD view is the region an earlier + slot of the same pass (k = 3's new pose) has just allocated."""
    idx = [0, 300, 600, 900, 1, 905, 301, 601, 2, 1100, 302, 3]
    depth, true, _ = _room(idx)
    rng = np.random.default_rng(23)
    drift = np.stack([_perturbed(p, rng, 1.5, 0.05) for p in true])
    old, new = drift.copy(), true.copy()
    fused = np.ones(len(idx), bool)
    old[3] = synth.trajectory_pose(450, 1200)      # frame 3 was fused far away from where it belongs: its new view allocates
    old[1] = LOST; fused[1] = False                # never integrated: add
    old[9] = LOST; fused[9] = False
    new[6] = LOST                                  # lost now: remove
    new[10] = LOST
    old[7] = LOST; new[7] = LOST; fused[7] = False  # neither
    old[5] = true[3]                               # frame 5 sits (wrongly) in frame 3's true view
    return depth, old, new, fused


@pytest.mark.parametrize("batch", [32, 5, 1])
def test_mixed_validity_and_births_inside_a_pass(oracle, batch):
    from scannet_amd import fusion
    depth, old, new, fused = _mixed_case()
    op, gp = _mk(oracle)
    ovol = oracle.Volume(op, threads=8)
    for k in np.flatnonzero(fused):
        ovol.integrate(depth[k], old[k])
    n0 = ovol.num_blocks
    last = _sequence(ovol, depth, None, old, new)
    assert ovol.num_blocks > n0
    dev = _Device(depth)
    try:
        with fusion.Fuser(gp, batch=batch) as f:
            for k in np.flatnonzero(fused):
                f.integrate_device(dev.frame(k)[0], old[k])
            f.reintegrate_batch_device(dev.d.value, dev.stride, old, new)
            st = f.stats()
            assert st["frames_skipped"] == 6 and st["frames_integrated"] == int(fused.sum()) + 9 + 9
            assert st["last_frame_blocks"] == last
            _assert_same(ovol, f)
    finally:
        dev.close()


@pytest.mark.parametrize("colour", [False, True])
def test_equals_the_fusers_own_sequence_stats_included(colour):
    """A second Fuser runs the frame-by-frame calls of the parent commit's API: the same blocks, the same voxels and every sf_stats field but
    total_pass_tiles -- and fewer tiles moved."""
    from scannet_amd import fusion
    depth, old, new, fused = _mixed_case()
    rgb = np.random.default_rng(5).integers(0, 256, (len(depth), H, W, 3), dtype=np.uint8) if colour else None
    gp = _gparams()
    dev = _Device(depth, rgb)
    try:
        with fusion.Fuser(gp) as a, fusion.Fuser(gp) as b:
            for f in (a, b):
                for k in np.flatnonzero(fused):
                    d, c = dev.frame(k)
                    f.integrate_device(d, old[k], d_rgb=c)
            a.reintegrate_batch_device(dev.d.value, dev.stride, old, new, d_rgb=dev.c.value if colour else None, rgb_stride_bytes=dev.cstride)
            for k in range(len(depth)):
                d, c = dev.frame(k)
                b.deintegrate_device(d, old[k], d_rgb=c)
                b.integrate_device(d, new[k], d_rgb=c)
            sa, sb = a.stats(), b.stats()
            for key in sa:
                if key != "total_pass_tiles":
                    assert sa[key] == sb[key], (key, sa[key], sb[key])
            assert sa["total_pass_tiles"] < sb["total_pass_tiles"]
            ca, va = a.export_blocks()
            cb, vb = b.export_blocks()
            assert np.array_equal(ca, cb) and np.array_equal(va.view(np.uint8), vb.view(np.uint8))
            # one host frame through sf_fuser_reintegrate on both: the pair of host calls on the other
            k = 4
            c = None if rgb is None else rgb[k]
            assert a.reintegrate(depth[k], new[k], old[k], rgb=c)
            assert b.deintegrate(depth[k], new[k], rgb=c) and b.integrate(depth[k], old[k], rgb=c)
            assert not a.reintegrate(depth[k], LOST, LOST)
            ca, va = a.export_blocks()
            cb, vb = b.export_blocks()
            assert np.array_equal(ca, cb) and np.array_equal(va.view(np.uint8), vb.view(np.uint8))
    finally:
        dev.close()


def test_weights_at_the_clamp(oracle):
    """A static view fused 300 times saturates the 8-bit weight; deintegration is then no inverse of integration (255 - 1 + 1 is 255, but the mean has
    moved).  The oracle defines the answer for a re-integration of 20 of those frames; the mixed-sign pass must give it."""
    from scannet_amd import fusion
    pose = synth.trajectory_pose(0, 1200).astype(np.float32)
    n = 300
    depth = np.stack([synth.render_room_depth(pose, W, H, noise_frame=k) for k in range(8)])
    depth = depth[np.arange(n) % 8]
    poses = np.repeat(pose[None], n, 0)
    op, gp = _mk(oracle)
    ovol = oracle.Volume(op, threads=8)
    for k in range(n):
        ovol.integrate(depth[k], pose)
    assert ovol.export()[1]["w"].max() == 255
    pick = np.arange(0, 200, 10)
    rng = np.random.default_rng(29)
    new = np.stack([_perturbed(pose, rng, 0.5, 0.01) for _ in pick])
    _sequence(ovol, depth[pick], None, poses[pick], new)
    dev = _Device(depth)
    try:
        with fusion.Fuser(gp) as f:
            f.integrate_batch_device(dev.d.value, dev.stride, poses)
            sub = _Device(depth[pick])
            try:
                f.reintegrate_batch_device(sub.d.value, sub.stride, poses[pick], new)
                _assert_same(ovol, f)
            finally:
                sub.close()
    finally:
        dev.close()


@pytest.mark.parametrize("colour", [False, True])
def test_update_trajectory_on_a_sens_file(oracle, tmp_path, colour):
    """About 120 frames written through the sf_sens_* writer (zlib depth, RAW colour or none), fused with a drifted trajectory, then updated to the true one
    with the default parameters, a step at a time: after every step the volume is the oracle's driven by the same plan; at the end nothing is left to
    move, the trajectory is the target and the frame counter shows that nothing was reset or fused again."""
    from scannet_amd import fusion, sens
    n = 120
    idx = [10 * k for k in range(n)]
    depth, true, rgb = _room(idx, colour=colour)
    rng = np.random.default_rng(31)
    drift = true.copy()
    moved = sorted(rng.choice(np.setdiff1d(np.arange(n), [7, 11, 13]), 70, replace=False))
    for k in moved:
        drift[k] = _perturbed(true[k], rng, rng.uniform(0.2, 1.5), rng.uniform(0.005, 0.04))
    target = true.copy()
    drift[7] = LOST       # enters
    target[11] = LOST     # leaves
    drift[13] = LOST      # lost in both
    target[13] = LOST
    fx, fy, mx, my = synth.intrinsics(W, H)
    K = np.array([[fx, 0, mx, 0], [0, fy, my, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    sd = sens.SensorData.create(W if colour else 0, H if colour else 0, W, H, K, K, color_compression=0, depth_compression=1)
    for k in range(n):
        sd.add_frame(depth[k], drift[k], color=rgb[k] if colour else None)
    path = str(tmp_path / "drift.sens")
    sd.save(path)
    sd.close()
    sd = sens.SensorData(path)
    op, gp = _mk(oracle)
    ovol = oracle.Volume(op, threads=8)
    for k in range(n):
        if drift[k][0, 0] != -np.inf:
            ovol.integrate(depth[k], drift[k], rgb=rgb[k] if colour else None)
    with fusion.Fuser(gp) as f:
        for k in range(n):
            f.integrate(depth[k], drift[k], rgb=rgb[k] if colour else None)
        _assert_same(ovol, f)
        fused0 = f.stats()["frames_integrated"]
        assert fused0 == n - 2
        cur = drift.reshape(n, 16).copy()
        tgt = target.reshape(n, 16)
        steps = frames = ops = 0
        while True:
            plan = fusion.plan_reintegration(cur, tgt)
            before = cur.copy()
            out, st = f.update_trajectory(sd, cur, tgt, max_steps=1, colour=colour, decode_threads=4)
            assert out is cur or np.shares_memory(out, cur)
            if len(plan) == 0:
                assert st["steps"] == 0 and np.array_equal(before, cur)
                break
            assert st["steps"] == 1 and st["frames_moved"] + st["frames_added"] + st["frames_removed"] == len(plan) and st["passes"] >= 1
            c = rgb[plan] if colour else None
            _sequence(ovol, depth[plan], c, before[plan].reshape(-1, 4, 4), tgt[plan].reshape(-1, 4, 4))
            ops += int((before[plan, 0] != -np.inf).sum() + (tgt[plan, 0] != -np.inf).sum())
            assert np.array_equal(cur[plan], tgt[plan])
            rest = np.setdiff1d(np.arange(n), plan)
            assert np.array_equal(cur[rest], before[rest])
            _assert_same(ovol, f)
            steps += 1
            frames += len(plan)
            assert steps < 10
        assert steps == 3 and frames == 72          # 70 moved + one that enters + one that leaves, 30 per step
        assert np.array_equal(cur, tgt)
        assert len(fusion.plan_reintegration(cur, tgt)) == 0
        assert f.stats()["frames_integrated"] == fused0 + ops == fused0 + 2 * 70 + 2   # nothing reset, nothing fused twice
    sd.close()
