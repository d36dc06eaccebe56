"""The free-space stage on the GPU: sf_fuser_allocate_box, sf_fuser_known_bounds and sf_fuser_export_dense against export_blocks and
numpy, the fused box against the dense checker tests/freespace_checker.c bit for bit, and the stage and its tool against the checker over the plan's box."""
import os
import subprocess

import numpy as np
import pytest

from scannet_amd import _abi, freespace, fusion, synth
from tests import freespace_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
VOXEL = 0.05
ROOM_LO, ROOM_HI = (-1, -1, -1), (15, 10, 8)     # blocks of 0.4 m around the 6 x 4 x 3 m room: 17 x 12 x 10
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    L = fc.build_checker(tmp_path_factory.mktemp("fsg"))
    if L is None:
        pytest.skip("needs gcc and a CPU with fused multiply-add")
    return L


def _params(width=W, height=H, blocks=1 << 14, **over):
    fx, fy, mx, my = synth.intrinsics(width, height)
    kw = dict(depth_width=width, depth_height=height, fx=fx, fy=fy, mx=mx, my=my, voxel_size=VOXEL, num_sdf_blocks=blocks, hash_num_buckets=1 << 15)
    kw.update(over)
    return fusion.default_params(**kw)


def _box_coords(lo, hi):
    g = np.meshgrid(*(np.arange(lo[a], hi[a] + 1) for a in range(3)), indexing="ij")
    c = np.stack([v.reshape(-1) for v in g], 1).astype(np.int32)
    return c[np.lexsort((c[:, 2], c[:, 1], c[:, 0]))]


def _scatter(coords, vox, lo, dims):
    """export_blocks' blocks scattered into the dense region [lo, lo + dims): (sdf bits uint32, weight, rgb), zeros where no block is."""
    lo, dims = np.asarray(lo, np.int64), np.asarray(dims, np.int64)
    bits = np.zeros((dims[2], dims[1], dims[0]), np.uint32)
    w = np.zeros(bits.shape, np.uint8)
    rgb = np.zeros(bits.shape + (3,), np.uint8)
    blo, bhi = lo // 8, (lo + dims - 1) // 8
    pick = np.nonzero(((coords >= blo) & (coords <= bhi)).all(1))[0]
    for i in pick:
        b = vox[i].reshape(8, 8, 8)                      # [z][y][x]
        o = coords[i].astype(np.int64) * 8 - lo          # where voxel (0, 0, 0) of the block lands in the region
        s = [slice(max(0, -o[a]), min(8, dims[a] - o[a])) for a in range(3)]
        d = [slice(o[a] + s[a].start, o[a] + s[a].stop) for a in range(3)]
        part = b[s[2], s[1], s[0]]
        bits[d[2], d[1], d[0]] = part["sdf"].view(np.uint32)
        w[d[2], d[1], d[0]] = part["w"]
        rgb[d[2], d[1], d[0]] = np.stack([part["r"], part["g"], part["b"]], -1)
    return bits, w, rgb


def _bytes(coords, vox):
    return coords.tobytes() + vox.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# allocation
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_allocate_box_on_an_empty_volume():
    with fusion.Fuser(_params()) as f:
        lo, hi = (-3, -2, 4), (5, 1, 6)                  # across negative coordinates: 9 x 4 x 3
        assert f.allocate_box(lo, hi) == 108
        coords, vox = f.export_blocks()
        assert np.array_equal(coords, _box_coords(lo, hi)) and not vox.view(np.uint8).any()
        st = f.stats()
        assert st["blocks_allocated"] == 108 and st["hash_slots_used"] == 108 and st["alloc_failures"] == 0 and st["high_water"] == 108
        assert f.allocate_box(lo, hi) == 0               # a second call: nothing new, nothing changed
        assert _bytes(*f.export_blocks()) == _bytes(coords, vox) and f.stats()["blocks_allocated"] == 108
        assert f.allocate_box((7, 7, 7), (7, 7, 7)) == 1  # one block
        assert f.allocate_box((-3, -2, 4), (6, 1, 6)) == 12   # one more layer in x: only that layer is new
        assert len(f.export_blocks()[0]) == 121
        for bad_lo, bad_hi in (((1, 0, 0), (0, 5, 5)), ((0, 0, 3), (5, 5, 2))):
            with pytest.raises(_abi.ScanfuseError) as e:
                f.allocate_box(bad_lo, bad_hi)
            assert e.value.code == -1                     # hi < lo
        with pytest.raises(_abi.ScanfuseError) as e:
            f.allocate_box((0, 0, 0), (2047, 1023, 1023))   # 2^31 blocks
        assert e.value.code == -1
        with pytest.raises(_abi.ScanfuseError) as e:
            f.allocate_box((0, 0, 1 << 20), (0, 0, 1 << 20))   # beyond the 21 bits of a key
        assert e.value.code == -1
        assert len(f.export_blocks()[0]) == 121
        f.set_slab(0, 0, 4)
        with pytest.raises(_abi.ScanfuseError) as e:
            f.allocate_box((0, 0, 0), (1, 1, 1))
        assert e.value.code == -4                         # SF_ERR_UNSUPPORTED while a partition is set
        f.set_slab(-1, 0, 0)
        f.reset()
        assert len(f.export_blocks()[0]) == 0 and f.allocate_box(lo, hi) == 108


def test_allocate_box_onto_a_fused_volume_and_a_heap_too_small():
    rgb = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    with fusion.Fuser(_params()) as f:                    # which blocks the frame allocates: the heap below is sized from them
        assert f.integrate(synth.plane_frame(W, H, 1000), EYE, rgb=rgb)
        c0 = f.export_blocks()[0]
    lo, hi = c0.min(0) - (1, 1, 2), c0.max(0) + (1, 1, 0)
    box = _box_coords(lo, hi)
    assert 0 < len(c0) < len(box) < 1000
    with fusion.Fuser(_params(blocks=len(box))) as f:
        assert f.integrate(synth.plane_frame(W, H, 1000), EYE, rgb=rgb)
        c0, v0 = f.export_blocks()
        assert (v0["w"] > 0).any() and (v0["r"] > 0).any()
        free0 = f.stats()["heap_free"]
        assert len(box) - len(c0) == free0 < len(box)     # the missing blocks just fit, the whole box would not: only what is missing counts
        assert f.allocate_box(lo, hi) == len(box) - len(c0)
        c1, v1 = f.export_blocks()
        assert np.array_equal(c1, box)                    # the union (the fused blocks all lie inside this box)
        old = (c1[:, None, :] == c0[None, :, :]).all(2).any(1)
        assert np.array_equal(v1[old].view(np.uint8), v0.view(np.uint8)) and not v1[~old].view(np.uint8).any()
        # a heap that cannot hold the box: refused before anything changes
        before, st0 = _bytes(c1, v1), f.stats()
        with pytest.raises(_abi.ScanfuseError) as e:
            f.allocate_box(lo - (0, 0, 40), hi)
        assert e.value.code == -6                         # SF_ERR_CAPACITY
        st1 = f.stats()
        assert _bytes(*f.export_blocks()) == before and st1["heap_free"] == st0["heap_free"] and st1["alloc_failures"] == st0["alloc_failures"] == 0
        # the volume still fuses: the same frame again doubles the weights of the old blocks
        assert f.integrate(synth.plane_frame(W, H, 1000), EYE, rgb=rgb)
        c2, v2 = f.export_blocks()
        assert np.array_equal(c2, box) and np.array_equal(v2[old]["w"], v0["w"] * 2)


def test_fusing_into_a_box_leaves_ordinary_fusion_alone(oracle):
    """Allocate the box, then integrate: every block oracle.Volume allocates for the same frames has the oracle's bytes in the fuser.  The views are
    chosen so that this is exact: a box block exists from the first frame on and so also takes the free-space updates of frames BEFORE the one whose
    truncation band makes the oracle allocate it -- which is the feature.  Two cameras back to back (and the first frame twice) share no block near a wall,
    so every oracle block is born in the first frame that can update it."""
    op = oracle.default_params(W, H, VOXEL)
    fx, fy, mx, my = synth.intrinsics(W, H)
    op.fx, op.fy, op.mx, op.my = fx, fy, mx, my
    ovol = oracle.Volume(op, threads=4)
    poses = [synth.yaw_pose(3.0, 2.0, 1.5, 0.0), synth.yaw_pose(3.0, 2.0, 1.5, 0.0), synth.yaw_pose(3.0, 2.0, 1.5, np.pi)]
    rng = np.random.default_rng(4)
    with fusion.Fuser(_params()) as f:
        assert f.allocate_box(ROOM_LO, ROOM_HI) == 17 * 12 * 10
        for pose in poses:
            pose = np.asarray(pose, np.float32)
            d = synth.render_room_depth(pose, W, H)
            rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            ovol.integrate(d, pose, rgb=rgb)
            assert f.integrate(d, pose, rgb=rgb)
        oc, ov = ovol.export()
        gc, gv = f.export_blocks()
        assert f.stats()["alloc_failures"] == 0
    ovol.close()
    assert len(oc) > 100 and (ov["w"] == 2).any() and (ov["w"] == 1).any()
    index = {tuple(c): i for i, c in enumerate(gc)}
    rows = np.array([index.get(tuple(c), -1) for c in oc])
    assert (rows >= 0).all()
    assert np.array_equal(gv[rows].view(np.uint8), ov.view(np.uint8))
    extra = np.ones(len(gc), bool)
    extra[rows] = False
    assert (gv[extra]["w"] > 0).any()                     # free space: known voxels in blocks ordinary fusion never allocates


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dense export
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coloured_volume():
    """A plane at 1 m seen from the origin, with colour, twice, and a box of empty blocks beside it: blocks either side of every axis' zero."""
    rng = np.random.default_rng(6)
    f = fusion.Fuser(_params())
    for k in range(2):
        assert f.integrate(synth.plane_frame(W, H, 1000 + 20 * k), EYE, rgb=rng.integers(1, 256, (H, W, 3), dtype=np.uint8))
    f.allocate_box((-2, -1, 0), (0, 0, 1))
    coords, vox = f.export_blocks()
    yield f, coords, vox
    f.close()


REGIONS = {"one": ((1, -2, 20), (1, 1, 1)), "unaligned": ((-5, -3, 14), (13, 9, 17)), "half_outside": ((-20, -40, 16), (40, 37, 9)),
           "outside": ((100, 100, 100), (11, 3, 5)), "far_negative": ((-2000000000, 5, 5), (9, 2, 2)),
           "far_positive": ((2147483600, 2147483640, 0), (40, 7, 2))}      # up to the last voxel index 32 bits hold


@pytest.mark.parametrize("region", sorted(REGIONS))
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_export_dense_is_the_scatter_of_export_blocks(coloured_volume, region, device):
    f, coords, vox = coloured_volume
    lo, dims = REGIONS[region]
    bits, w, rgb = _scatter(coords, vox, lo, dims)
    if region in ("one", "unaligned", "half_outside"):
        assert (w > 0).any()
    if region == "half_outside":
        assert (w[:, :16] == 0).all() and (w[:, 24:] > 0).any()
    if region in ("outside", "far_negative", "far_positive"):
        assert not bits.any() and not w.any()

    def host(a):
        return a.cpu().numpy() if device else a

    sdf0, w0, rgb0 = (host(a) for a in f.export_dense(lo, dims, rgb=True, device=device))
    assert sdf0.shape == (dims[2], dims[1], dims[0]) and sdf0.dtype == np.float32
    assert np.array_equal(sdf0.view(np.uint32), bits) and np.array_equal(w0, w) and np.array_equal(rgb0, rgb)
    sdf1, w1 = (host(a) for a in f.export_dense(lo, dims, task=True, device=device))
    with np.errstate(divide="ignore"):
        want = np.where(w > 0, bits.view(np.float32) / np.float32(VOXEL), np.float32(-np.inf)).astype(np.float32)
    assert np.array_equal(sdf1.view(np.uint32), want.view(np.uint32)) and np.array_equal(w1, w)
    again = [host(a) for a in f.export_dense(lo, dims, rgb=True, device=device)]
    assert again[0].tobytes() == sdf0.tobytes() and again[1].tobytes() == w0.tobytes() and again[2].tobytes() == rgb0.tobytes()
    assert _bytes(*f.export_blocks()) == _bytes(coords, vox)          # an export changes nothing


def test_export_dense_refuses_bad_regions(coloured_volume):
    f = coloured_volume[0]
    L = _abi.lib()
    lo = np.zeros(3, np.int32)
    for dims in ((0, 4, 4), (4, -1, 4), (1 << 14, 1 << 14, 1 << 12), (2147483647, 1, 1)):
        d = np.array(dims, np.int32)
        lo[0] = 2 if dims[0] == 2147483647 else 0       # the last: fewer than 2^40 voxels, but its last voxel index would be 2^31
        rc = L.sf_fuser_export_dense(f._h, lo.ctypes.data, d.ctypes.data, 0, None, None, None, 0)
        assert rc == -1, dims
    assert L.sf_fuser_export_dense(f._h, lo.ctypes.data, np.array([4, 4, 4], np.int32).ctypes.data, 2, None, None, None, 0) == -1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the whole rule: the fused box against the dense checker, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_case(checker, sp, frames, mode, lo_block=ROOM_LO, hi_block=ROOM_HI):
    """frames: [(depth at the input size, pose)] -> the fuser's and the checker's (sdf, weight) over the box."""
    lo = np.array(lo_block) * 8
    dims = (np.array(hi_block) - np.array(lo_block) + 1) * 8
    cp = fc.checker_params(sp)
    vol = fc.Volume(checker, cp, lo, dims)
    resample = (cp.width, cp.height) != (sp.depth_width, sp.depth_height)
    for d, pose in frames:
        vol.integrate(fc.resample(d, cp.width, cp.height) if resample else d, pose)
    want = vol.export() + vol.export(task=True)
    vol.close()
    with fusion.Fuser(sp) as f:
        f.allocate_box(lo_block, hi_block)
        if mode == "single":
            for d, pose in frames:
                assert f.integrate(d, pose) == (pose[0, 0] != -np.inf)
        else:
            import torch
            px = sp.depth_width * sp.depth_height
            stride = (px * 2 + 15) // 16 * 16                         # the device frames 16-byte aligned
            buf = np.zeros((len(frames), stride // 2), np.uint16)
            for i, (d, _) in enumerate(frames):
                buf[i, :px] = d.reshape(-1)
            d_depth = torch.from_numpy(buf.view(np.int16)).cuda()
            f.integrate_batch_device(d_depth, stride, np.stack([p for _, p in frames]))
        got = f.export_dense(lo, dims) + f.export_dense(lo, dims, task=True)
        st = f.stats()
    assert st["alloc_failures"] == 0
    assert st["frames_integrated"] == sum(1 for _, p in frames if p[0, 0] != -np.inf)
    return got, want


def _assert_bits(got, want):
    for g, w, name in zip(got, want, ("sdf", "weight", "task volume", "weight")):
        if g.dtype == np.float32:
            same = g.view(np.uint32) == w.view(np.uint32)
        else:
            same = g == w
        if not same.all():
            z, y, x = np.argwhere(~same)[0]
            raise AssertionError("%s: %d voxels differ; first at [%d, %d, %d]: fuser %r checker %r" % (name, (~same).sum(), z, y, x, g[z, y, x], w[z, y, x]))
    assert (want[1] > 0).sum() > 1000


def _cycle(frames, n):
    out = [frames[i % len(frames)] for i in range(n)]
    if n >= 3:
        out[n // 2] = (out[n // 2][0], fc.NEG_INF_POSE)               # tracking lost in the middle
    return out


@pytest.fixture(scope="module")
def room8():
    return fc.room_frames(8, W, H)


@pytest.mark.parametrize("n,mode", [(1, "batch"), (32, "batch"), (33, "batch"), (65, "batch"), (33, "single")])
def test_whole_rule_room(checker, room8, n, mode):
    got, want = _run_case(checker, _params(), _cycle(room8, n), mode)
    _assert_bits(got, want)
    if n == 65:
        assert want[1].max() >= 8


@pytest.mark.parametrize("n,mode", [(33, "batch"), (5, "single")])
def test_whole_rule_noise(checker, n, mode):
    """Hashed-noise depth, zeros and out-of-range values among it: every ray ends somewhere else, the truncation bands of neighbouring pixels overlap."""
    poses = [np.asarray(synth.trajectory_pose(i * 50, 400), np.float32) for i in range(4)]
    frames = [(fc.noise_depth(W, H, 10 + i), poses[i]) for i in range(4)]
    got, want = _run_case(checker, _params(blocks=1 << 16), _cycle(frames, n), mode)
    _assert_bits(got, want)


@pytest.mark.parametrize("case", ["50x38", "intrinsics", "integration_size"])
def test_whole_rule_other_cameras(checker, case):
    if case == "50x38":                                               # no multiple of the pre-pass's 8 pixels per lane, rows of an odd length
        w, h, sp = 50, 38, _params(50, 38)
    elif case == "intrinsics":                                        # off-centre principal point, fx != fy
        w, h, sp = W, H, _params(fx=70.0, fy=52.0, mx=25.25, my=30.5)
    else:                                                             # 160 x 120 frames integrated at 64 x 48
        w, h, sp = 160, 120, _params(160, 120, integration_width=W, integration_height=H)
    intr = (sp.fx, sp.fy, sp.mx, sp.my)
    frames = []
    for i in range(6):
        pose = np.asarray(synth.trajectory_pose(i * 66, 400), np.float32)
        frames.append((_render(pose, w, h, intr), pose))
    got, want = _run_case(checker, sp, _cycle(frames, 33), "batch")
    _assert_bits(got, want)


def _render(pose, w, h, intr):
    """The empty room through a camera with the intrinsics `intr`: synth.render_room_depth's picture is of synth.intrinsics(w, h), so the frame is a
    plausible depth image, not a consistent one -- the rule is per pixel and does not care."""
    d = synth.render_room_depth(pose, w, h)
    return d if tuple(intr) == tuple(np.float32(v) for v in synth.intrinsics(w, h)) else np.ascontiguousarray(d[::-1, ::-1])


@pytest.mark.parametrize("wrap", [0, 1])
def test_weight_saturation_and_wrap(checker, wrap):
    """300 identical frames: the 8-bit weight stays at 255, or -- weight_wrap = 1 with the shipped weightMax -- wraps at 256 and starts again."""
    sp = _params(weight_wrap=wrap, weight_max=99999999 if wrap else 255)
    frames = [(synth.plane_frame(W, H, 1500), EYE)] * 300
    got, want = _run_case(checker, sp, frames, "batch", lo_block=(-3, -2, 0), hi_block=(2, 1, 4))
    _assert_bits(got, want)
    assert int(want[1].max()) == (300 - 256 if wrap else 255)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# known bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_known_bounds_is_numpy_over_export_blocks(room8):
    with fusion.Fuser(_params()) as f:
        assert f.known_bounds() == (None, None, 0)                    # an empty volume
        f.allocate_box(ROOM_LO, ROOM_HI)
        assert f.known_bounds() == (None, None, 0)                    # blocks, but nothing observed
        for k, (d, pose) in enumerate(room8[:3]):
            assert f.integrate(d, pose)
            coords, vox = f.export_blocks()
            b, v = np.nonzero(vox["w"] > 0)
            g = coords[b].astype(np.int64) * 8 + np.stack([v & 7, (v >> 3) & 7, v >> 6], 1)
            lo, hi, known = f.known_bounds()
            assert known == len(b) > 1000
            assert np.array_equal(lo, g.min(0)) and np.array_equal(hi, g.max(0))
    with fusion.Fuser(_params()) as f:                                # without a box: one block's corner voxel, at negative coordinates
        c = np.array([[-4, 2, -1]], np.int32)
        v = np.zeros((1, 512), fusion.VOXEL_DTYPE)
        v["w"][0, 7 * 64 + 0 * 8 + 7] = 3
        f.import_blocks(c, v, ghost=False)
        lo, hi, known = f.known_bounds()
        assert known == 1 and list(lo) == list(hi) == [-32 + 7, 16, -8 + 7]
        f.import_blocks(np.array([[9, 9, 9]], np.int32), v, ghost=True)   # a ghost is somebody else's block
        assert f.known_bounds()[2] == 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_stage_and_tool(checker, tmp_path):
    """A 40-frame synthetic .sens (one pose lost): sf_freespace_sens is the checker over the plan's box, cropped to the box of the known voxels;
    bin/freespace writes the same bytes to the default path; --every=2 fuses 20 frames."""
    voxel = 0.1
    frames = fc.room_frames(40, W, H)
    frames[7] = (frames[7][0], fc.NEG_INF_POSE)
    sd = fc.make_sens(frames, W, H)
    path = str(tmp_path / "scene0000_00.sens")
    sd.save(path)
    fp = freespace.default_params(voxel_size=voxel)
    sp, lo_b, hi_b = freespace.plan(sd, fp)
    grid, st = freespace.carve_sens(sd, fp, stats=True)
    lo, dims = lo_b.astype(np.int64) * 8, (hi_b.astype(np.int64) - lo_b + 1) * 8
    vol = fc.Volume(checker, fc.checker_params(sp), lo, dims)
    for d, pose in frames:
        vol.integrate(d, pose)
    task, w = vol.export(task=True)
    vol.close()
    z, y, x = np.nonzero(w > 0)
    k_lo, k_hi = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    assert np.array_equal(grid.lo_voxel, lo + k_lo) and grid.value.shape == tuple((k_hi - k_lo + 1)[::-1])
    crop = (slice(k_lo[2], k_hi[2] + 1), slice(k_lo[1], k_hi[1] + 1), slice(k_lo[0], k_hi[0] + 1))
    assert np.array_equal(grid.value.view(np.uint32), task[crop].view(np.uint32)) and np.array_equal(grid.weight, w[crop])
    assert grid.frames_used == 39 and grid.voxel_size == float(np.float32(voxel)) and np.array_equal(grid.world2grid, freespace.world2grid(np.float32(voxel), grid.lo_voxel))
    assert st["known"] == len(x) and st["free_voxels"] + st["near_voxels"] == st["known"] and st["free_voxels"] > 0 and st["near_voxels"] > 0
    assert st["box_blocks"] == np.prod(hi_b.astype(np.int64) - lo_b + 1) and st["frames_used"] == 39 and st["seconds_total"] > 0
    # the world position of every known node reads that node's value back: world2grid on the stage's own grid
    kz, ky, kx = np.nonzero(grid.known)
    world = ((np.stack([kx, ky, kz], 1) + grid.lo_voxel) * np.float64(grid.voxel_size)).astype(np.float32)
    assert np.array_equal(freespace.lookup(grid, world).view(np.uint32), grid.value[kz, ky, kx].view(np.uint32))
    ref = str(tmp_path / "library.grid")
    grid.save(ref)
    exe = os.path.join(ROOT, "bin", "freespace")
    r = subprocess.run([exe, path, "--voxel=0.1", "--print-stats"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    out = str(tmp_path / "scene0000_00.grid")                          # the .sens path with .grid in place of .sens
    assert open(out, "rb").read() == open(ref, "rb").read()
    assert "%d known" % st["known"] in r.stdout
    back = freespace.load_grid(out)
    assert np.array_equal(back.value.view(np.uint32), grid.value.view(np.uint32)) and np.array_equal(back.weight, grid.weight)
    out2 = str(tmp_path / "half.grid")
    r = subprocess.run([exe, path, "-o", out2, "--voxel=0.1", "--every=2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    half = freespace.load_grid(out2)
    assert half.frames_used == 20 and half.known.sum() > 0
    vol = fc.Volume(checker, fc.checker_params(sp), lo, dims)          # frames 0, 2, 4, ... lie inside the box planned for all of them
    for d, pose in frames[::2]:
        vol.integrate(d, pose)
    task2, w2 = vol.export(task=True)
    vol.close()
    o = half.lo_voxel - lo
    nz, ny, nx = half.value.shape
    crop2 = (slice(o[2], o[2] + nz), slice(o[1], o[1] + ny), slice(o[0], o[0] + nx))
    assert np.array_equal(half.value.view(np.uint32), task2[crop2].view(np.uint32)) and (w2 > 0).sum() == half.known.sum()
