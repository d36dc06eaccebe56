"""Cases of the fusion front chain (tests/test_front_stages_cpu.py, tests/test_front_stages.py): every case names the branch of
scannet_amd/csrc/fuser_prepass.hip / fuser_alloc.hip / fuser_compact.hip it exists for and the witness that a run got there.  Images are 16x16 to 48x32
(33x17 and 17x9: ragged pixel tiles, W*H no multiple of 8), heaps hold at most 2^15 blocks.

Witnesses that no device counter gives -- "rays left the ray-space window", "the window map was refreshed", "nine windows would be needed" -- rest on the
coarse float64 models at the end of this module, asserted when the cases are built, with at least two blocks of margin."""
import numpy as np

from scannet_amd import fusion
from tests import front_exact as fx

F32 = np.float32


# ---- parameters, poses, scenes --------------------------------------------------------------------------------------------------------------------------
def params(W, H, fx_=250.0, **over):
    """The shipped parameters at a small image; fx 250 keeps the ray-space window (k_alloc_ray) the fuser's own choice at 4 mm voxels."""
    kw = dict(depth_width=W, depth_height=H, fx=fx_, fy=fx_ + 3.0, mx=(W - 1) / 2.0 + 0.25, my=(H - 1) / 2.0 - 0.25, num_sdf_blocks=1 << 13, hash_num_buckets=1 << 12,
              hash_bucket_size=4)
    kw.update(over)
    return fusion.default_params(**kw)


def oracle_params(orc, p):
    """oracle.OrParams of the INTEGRATION camera of sf_params p."""
    k = fx.derive(p)
    op = orc.OrParams(k.W, k.H, float(k.fx), float(k.fy), float(k.mx), float(k.my), p.depth_shift, p.depth_min, p.depth_max, p.voxel_size, p.trunc_base, p.trunc_scale,
                      p.max_integration_dist, 1, 255, 10.0)
    op.frustum_mode = p.frustum_mode
    return op


def look(eye, direction, roll=0.0):
    """camToWorld (16 floats) of a camera at `eye` looking along `direction`; axis-aligned directions give entries of exactly 0 and +-1."""
    z = np.asarray(direction, np.float64)
    z = z / np.linalg.norm(z)
    h = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(h, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    if roll:
        x, y = np.cos(roll) * x + np.sin(roll) * y, -np.sin(roll) * x + np.cos(roll) * y
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    m[np.abs(m) < 1e-15] = 0.0
    return m.astype(F32).reshape(16)


def wall(W, H, n, base_mm=1500, step_mm=700, drift_mm=4, holes=True):
    """n frames of a tilted wall with a depth step down the middle columns (a pixel tile then holds two clusters of rays) and a few holes; all differ."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint16)
    for j in range(n):
        d = base_mm + 3 * xx + 2 * yy + drift_mm * j + np.where((xx > W // 3) & (xx < W // 2), step_mm, 0)
        if holes:
            d = np.where((xx * 7 + yy * 13 + j) % 29 == 0, 0, d)
        out[j] = d
    return out


def walk_poses(n, eye=(0.3, -0.2, 0.1), direction=(0, 0, 1), move=(0.004, 0.002, 0.001), yaw=0.0):
    """n poses: the camera drifts by `move` per frame and turns by `yaw` radians per frame about the world's y axis."""
    out = []
    for j in range(n):
        d = np.asarray(direction, np.float64)
        a = yaw * j
        rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        out.append(look(np.asarray(eye, np.float64) + j * np.asarray(move), rot @ d if yaw else d))
    return np.array(out, F32)


class Case:
    def __init__(self, name, branch, witness, **kw):
        self.name, self.branch, self.witness = name, branch, witness
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


# ---- pre-pass -------------------------------------------------------------------------------------------------------------------------------------------
def _all_values():
    return np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)


def _frames(W, H, n, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 7000, (n, H, W)).astype(np.uint16)
    d[rng.random((n, H, W)) < 0.1] = 0
    return d


def _picture(w, h, n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 9 + yy * 5) % 256, (xx * 3 + yy * 11 + 40) % 256, (xx * yy + 7) % 256], -1)
    return ((base[None] + rng.integers(0, 24, (n, h, w, 3))) % 256).astype(np.uint8)


def _prepass_cases():
    out = []
    small = dict(num_sdf_blocks=256, hash_num_buckets=64, hash_bucket_size=2)
    # all 65 536 values; shift 1000: 100 / 1000 rounds to depth_min's own bits, 6000 / 1000 = depth_max, 4000 / 1000 = max_integration_dist
    out.append(Case("all-u16-shift1000", "every gate of k_prepass at the shipped shift", "values at depth_min (kept), at max_integration_dist (dropped)",
                    p=params(256, 256, **small), depth=_all_values(), hits=("dmin", "maxd")))
    out.append(Case("all-u16-shift1000-far", "the depth_max gate: max_integration_dist above it", "a value at depth_max (kept), the next one dropped",
                    p=params(256, 256, max_integration_dist=8.0, **small), depth=_all_values(), hits=("dmin", "dmax")))
    odd = float(F32(777.5))
    q = lambda u: float(F32(u) / F32(odd))
    out.append(Case("all-u16-shift777.5", "the gates at a shift that is no power of ten", "values at all three bounds",
                    p=params(256, 256, depth_shift=odd, depth_min=q(80), depth_max=q(5000), max_integration_dist=q(3100), **small), depth=_all_values(),
                    hits=("dmin", "maxd")))
    for n in (1, 2, 32):
        out.append(Case("frames-n%d-17x9" % n, "blockIdx.y = frame; the ragged last lane (153 pixels)", "n planes that all differ",
                        p=params(17, 9, **small), depth=_frames(17, 9, n, 10 + n)))
    out.append(Case("resampled-40x30-to-17x9", "integration_width: the nearest resample", "source columns and rows skipped",
                    p=params(40, 30, integration_width=17, integration_height=9, **small), depth=_frames(40, 30, 3, 20)))
    for (W, H) in ((16, 16), (17, 9)):
        for mis in range(8):
            out.append(Case("rgb-%dx%d-misaligned%d" % (W, H, mis), "the 8-byte loads of aligned colour (misalign 0, 16x16) and the byte loop",
                            "pictures at %d bytes past an aligned address, frame stride %d bytes" % (mis, W * H * 3),
                            p=params(W, H, **small), depth=_frames(W, H, 3, 30 + mis), rgb=_picture(W, H, 3, 40 + mis), misalign=mis))
    own = dict(color_width=31, color_height=23, cfx=260.0, cfy=390.0, cmx=15.5, cmy=11.2)
    out.append(Case("rgb-own-size-31x23", "colour at its own size: the ray-slope look-up", "pixels outside (black) and on the last row and column",
                    p=params(33, 17, **own, **small), depth=_frames(33, 17, 2, 50), rgb=_picture(31, 23, 2, 51), misalign=0, outside=True))
    out.append(Case("rgb-resampled-input-size", "colour at the INPUT size of a resampled depth stream", "the colour camera is the input camera",
                    p=params(40, 30, integration_width=17, integration_height=9, **small), depth=_frames(40, 30, 2, 52), rgb=_picture(40, 30, 2, 53), misalign=3))
    for name, samp in (("444", ((1, 1), (1, 1), (1, 1))), ("422", ((2, 1), (1, 1), (1, 1))), ("420", ((2, 2), (1, 1), (1, 1))), ("grey", None)):
        out.append(Case("jpeg-%s-17x9" % name, "JPEG planes at the depth size: YccPicture.pixel", "odd size: partial MCUs",
                        p=params(17, 9, **small), depth=_frames(17, 9, 2, 60), jpeg=samp, picture=_picture(17, 9, 2, 61)))
        out.append(Case("jpeg-%s-own-31x23" % name, "JPEG planes at their own size: the look-up dealt across the workgroup", "pixels outside and inside",
                        p=params(33, 17, **own, **small), depth=_frames(33, 17, 2, 62), jpeg=samp, picture=_picture(31, 23, 2, 63)))
    return out


def jpeg_streams(case):
    from tests import jpeg_tools
    if case.jpeg is None:
        return [jpeg_tools.encode(pic[..., 1], qstep=3) for pic in case.picture]
    return [jpeg_tools.encode(pic, sampling=case.jpeg, qstep=3) for pic in case.picture]


# ---- allocation -----------------------------------------------------------------------------------------------------------------------------------------
SEQ_W, SEQ_H = 33, 17


def _alloc_cases():
    out = []
    p = params(SEQ_W, SEQ_H)
    depth, poses = wall(SEQ_W, SEQ_H, 32), walk_poses(32)
    # one 32-frame sequence, its prefixes: the births of the first n frames do not depend on the frames behind them
    for n in (1, 2, 4, 5, 16, 17, 32):
        for group in (1, 4, 16):
            for head in (0, 1):
                kern = "k_alloc_ray<%s>" % ("true" if min(group if not head else min(group, 4), n) > 1 else "false")
                out.append(Case("ray-n%d-g%d-h%d" % (n, group, head), "%s, %d workgroup layers" % (kern, -(-n // min(group if not head else min(group, 4), n))),
                                "direct == 0", p=p, tune=dict(alloc_group=group), passes=[(depth[:n], poses[:n], head, 0)], seq="wall32"))
    out.append(Case("ray-fused-prepass", "k_alloc_ray<false> with fuse_depth16", "the float depth comes back from the kernel; direct == 0", p=p, tune={},
                    passes=[(depth[:1], poses[:1], 0, 1)], seq="wall32"))
    gates = depth[:1].copy()
    gates[0, 0, :4], gates[0, 1, :4], gates[0, 2, :2] = (100, 99, 4000, 3999), (101, 6000, 6001, 1), (65535, 3998)
    out.append(Case("ray-fused-gates", "the gates of the fused pre-pass (k_alloc_ray's own copy of k_prepass's)", "pixels at depth_min and at max_integration_dist, one unit either side",
                    p=p, tune={}, passes=[(gates, poses[:1], 0, 1)]))
    out.append(Case("ray-gates", "the same frame through k_prepass + k_alloc_ray<false>", "the same blocks", p=p, tune={}, passes=[(gates, poses[:1], 0, 0)]))
    for n in (1, 5, 17):
        for brick in (0, 1):
            out.append(Case("cube5-n%d-brick%d" % (n, brick), "k_alloc<5, %s>, presence cache %s" % ("true" if n > 1 else "false", "on" if brick else "off"), "direct == 0",
                            p=p, tune=dict(alloc_ray=0, brick_cache=brick), passes=[(depth[:n], poses[:n], 0, 0)], seq="wall32"))
    # 1.5 mm voxels: the 64^3 window, one frame per workgroup
    p15 = params(16, 16, voxel_size=0.0015, num_sdf_blocks=1 << 15, hash_num_buckets=1 << 14)
    out.append(Case("cube6-n3", "k_alloc<6, false>", "direct == 0", p=p15, tune={}, passes=[(wall(16, 16, 3, 900, 90), walk_poses(3), 0, 0)]))
    # the six orientations of the ray-space window, a diagonal that ties its axis choice, negative coordinates, the origin inside the pencil
    views = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1), "diag111": (1, 1, 1)}
    for name, d in views.items():
        for ray in (1, 0):
            out.append(Case("view%s-%s" % (name, "ray" if ray else "cube5"), "window axis and sign %s (%s)" % (name, "k_alloc_ray<true>" if ray else "k_alloc<5, true>"), "direct == 0",
                            p=p, tune=dict(alloc_ray=ray), passes=[(wall(SEQ_W, SEQ_H, 4, 1200), walk_poses(4, eye=(0.3, -0.2, 0.1), direction=d), 0, 0)]))
    # exact ties of the walk: the ray of the pixel AT the principal point runs along the camera's z axis; with equal components of that axis and of the camera
    # centre its end points, first blocks, tmax and tdelta are the same numbers on the tied axes -- every step of the walk meets the tie-break
    pt = params(16, 16, mx=8.0, my=8.0)
    one = np.zeros((1, 16, 16), np.uint16)
    one[0, 8, 8] = 1500
    for name, d, eye in (("xyz", (1, 1, 1), (0.3, 0.3, 0.3)), ("xy", (1, 1, 0), (0.3, 0.3, 0.1)), ("yz", (0, 1, 1), (0.1, 0.3, 0.3)), ("xz", (1, 0, 1), (0.3, 0.1, 0.3))):
        for ray in (1, 0):
            out.append(Case("tie-%s-%s" % (name, "ray" if ray else "cube5"), "the walk's tie-break: x if strictly smallest, else z if below y, else y (%s)" % ("ray_walk_bits" if ray else "k_alloc"),
                            "tmax equal on the tied axes at every step", p=pt, tune=dict(alloc_ray=ray), passes=[(one, walk_poses(1, eye=eye, direction=d), 0, 0)], ties=name))
    out.append(Case("negative-coordinates", "block coordinates below zero: the arithmetic shift, the 21-bit key fields", "every block has a negative coordinate",
                    p=p, tune={}, passes=[(wall(SEQ_W, SEQ_H, 4, 1200), walk_poses(4, eye=(-7.3, -5.2, -9.1), direction=(0.1, -0.2, -1)), 0, 0)], negative=True))
    out.append(Case("across-the-origin", "coordinates of both signs in one tile: rounding half away from zero on both sides", "blocks at -1 and 0 on every axis",
                    p=p, tune={}, passes=[(wall(SEQ_W, SEQ_H, 4, 1000, holes=False), walk_poses(4, eye=(-0.05, 0.03, -1.1), direction=(0, 0, 1), move=(0.002, -0.002, 0)), 0, 0)],
                    straddles=True))
    # a camera that turns: the map of a 16-frame group cannot hold the sweep
    out.append(Case("turning-camera", "k_alloc_ray<true>: n_map < group, a fresh map and a cleared s_done inside the group", "model: the tile centre at max distance sweeps > 11 blocks",
                    p=p, tune=dict(alloc_group=16), passes=[(wall(SEQ_W, SEQ_H, 16, 600, 100), walk_poses(16, yaw=0.012), 0, 0)], sweeps=True))
    # the ray-space window forced on a pencil it cannot hold
    pw = params(16, 16, fx_=40.0, voxel_size=0.0015, num_sdf_blocks=1 << 15, hash_num_buckets=1 << 14)
    far = wall(16, 16, 2, 3300, 400, 30, holes=False)
    out.append(Case("ray-window-too-small", "k_alloc_ray: rays outside the window, the LDS set's 32-probe give-up, the full queue, direct()",
                    "model: the pencil is > 18 blocks wide and > 258 slabs deep; direct > 0", p=pw, tune=dict(alloc_ray=1, alloc_group=2),
                    passes=[(far, walk_poses(2), 0, 0)], direct=True, leaves=True))
    # nine clusters of rays, each further than a window from the next
    # (0.5 mm voxels; a truncation of 5 mm + 2 % keeps every ray shorter than the window, so that a round holds exactly one level)
    p05 = params(16, 16, fx_=600.0, voxel_size=0.0005, trunc_base=0.005, trunc_scale=0.02, num_sdf_blocks=1 << 13)
    nine = np.zeros((1, 16, 16), np.uint16)
    for i in range(9):
        nine[0, 1 + i, 3 + i % 3] = 300 + 440 * i
    out.append(Case("nine-levels-cube6", "k_alloc<6, false>: the eight re-anchoring rounds run out, the last round's LDS set", "model: nine levels > 66 blocks apart",
                    p=p05, tune={}, passes=[(nine, walk_poses(1, eye=(0.01, 0.01, 0.01)), 0, 0)], levels=True))
    # frames that name nothing
    zero = np.zeros((2, SEQ_H, SEQ_W), np.uint16)
    out.append(Case("all-invalid", "no active lane", "nothing allocated", p=p, tune={}, passes=[(zero, walk_poses(2), 0, 0)], empty=True))
    out.append(Case("all-beyond-max-distance", "d >= max_integration_dist", "nothing allocated", p=p, tune={}, passes=[(zero + 4000, walk_poses(2), 0, 0)], empty=True))
    out.append(Case("empty-band", "lo >= hi: a truncation of zero", "nothing allocated", p=params(SEQ_W, SEQ_H, trunc_base=0.0, trunc_scale=0.0), tune={},
                    passes=[(wall(SEQ_W, SEQ_H, 2), walk_poses(2), 0, 0)], empty=True))
    # the same frames again
    for brick in (0, 1):
        out.append(Case("three-passes-brick%d" % brick, "found entries: note_birth keeps the earlier birth; brick_note / brick_known_row", "passes 2, 3: nothing new" +
                        ("; pass 3 probes less than pass 1" if brick else ""), p=p, tune=dict(alloc_ray=0, brick_cache=brick),
                        passes=[(depth[:5], poses[:5], 0, 0)] * 3, seq="wall32", repeat=True, brick=brick))
    # a table of 64 x 2 slots, nearly full
    ptab = params(16, 16, num_sdf_blocks=256, hash_num_buckets=64, hash_bucket_size=2)
    out.append(Case("table-128-nearly-full", "probe chains that wrap at total_slots", "100..127 of 128 slots used; an entry sits below its home",
                    p=ptab, tune={}, passes=[(wall(16, 16, 6, 1000, 0, 2, holes=False), walk_poses(6, move=(0.012, 0.0, 0.004)), 0, 0)], fill=(100, 127)))
    out.append(Case("table-too-small", "hash_find_or_claim gives up after MAX_PROBES: C_ALLOC_FAIL", "failed > 0, a subset is inserted",
                    p=ptab, tune={}, passes=[(wall(16, 16, 8, 1000, 500, 2), walk_poses(8, move=(0.02, 0.01, 0.004)), 0, 0)], relaxed="table"))
    pheap = params(16, 16, num_sdf_blocks=64)
    out.append(Case("heap-too-small", "give_block_quiet without a block: the pop undone, the failure counted", "failed == orphans > 0, heap_free == 0",
                    p=pheap, tune={}, passes=[(wall(16, 16, 4, 1000, 500, 2), walk_poses(4), 0, 0)], relaxed="heap"))
    return out


# ---- compaction -----------------------------------------------------------------------------------------------------------------------------------------
def lattice(k, pose, reach=3):
    """Candidate blocks around the frustum of `pose`: the blocks the far and near part of the view volume touch, +- reach."""
    F = fx.frame_setup(k, pose)
    bs = 8.0 * float(k.voxel)
    pts = []
    for z in (0.0, float(F.zfar)):
        for u in (-1.5, k.W - 0.5):
            for v in (-1.5, k.H - 0.5):
                c = np.array([(u - float(k.mx)) / float(k.fx) * z, (v - float(k.my)) / float(k.fy) * z, z])
                pts.append(np.asarray(pose, np.float64).reshape(4, 4)[:3, :3] @ c + np.asarray(pose, np.float64).reshape(4, 4)[:3, 3])
    pts = np.array(pts) / bs
    lo, hi = np.floor(pts.min(0)).astype(int) - reach, np.ceil(pts.max(0)).astype(int) + reach
    g = np.mgrid[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].reshape(3, -1).T
    return g


def plane_blocks(k, pose, each=3):
    """Of the lattice: per plane of the frustum (frustum_mode 0) the `each` blocks nearest the plane on either side -- on, just inside, just outside."""
    g = lattice(k, pose)
    m = fx.plane_margins(k, fx.frame_setup(k, pose), g).astype(np.float64)
    pick = []
    for q in range(6):
        others = np.delete(m, q, 1).min(1) >= 0            # decided by this plane alone
        inside = np.nonzero(others & (m[:, q] >= 0))[0]
        outside = np.nonzero(others & (m[:, q] < 0))[0]
        pick += inside[np.argsort(m[inside, q])[:each]].tolist() + outside[np.argsort(-m[outside, q])[:each]].tolist()
    return g[sorted(set(pick))]


COMPACT_N = (1, 4, 5, 8, 9, 16, 17, 32)
HIGH_WATER = (0, 1, 255, 256, 257, 2047, 2048, 2049)


def compact_directory(k, m, seed=0):
    """m blocks for a directory of exactly m entries: the plane blocks of the first two poses of compact_poses, then lattice blocks at random; every fifth a ghost."""
    poses = compact_poses(32)
    first = np.concatenate([plane_blocks(k, poses[0]), plane_blocks(k, poses[31])])
    g = lattice(k, poses[0], reach=1)
    rng = np.random.default_rng(seed)
    rest = g[rng.permutation(len(g))]
    allb = np.unique(np.concatenate([first, rest]), axis=0, return_index=True)[1]
    blocks = np.concatenate([first, rest])[np.sort(allb)][:m]
    assert len(blocks) == m, (len(blocks), m)
    ghost = (np.arange(m) % 5) == 4
    return blocks.astype(np.int32), ghost


def compact_poses(n):
    return walk_poses(n, eye=(0.2, 0.1, -0.3), direction=(0.05, -0.02, 1), move=(0.01, 0.004, 0.002), yaw=0.004)


def compact_params(mode):
    return params(24, 16, fx_=60.0, frustum_mode=mode, num_sdf_blocks=4096, max_integration_dist=1.0)


# ---- the float64 models behind the coverage claims ------------------------------------------------------------------------------------------------------
def model_sweep_blocks(k, poses):
    """How far (blocks, largest axis) the centre of the image's first pixel tile at max_integration_dist moves between the first and the last pose."""
    bs = 8.0 * float(k.voxel)
    pts = []
    for pose in (poses[0], poses[-1]):
        m = np.asarray(pose, np.float64).reshape(4, 4)
        c = np.array([(7.5 - float(k.mx)) / float(k.fx), (7.5 - float(k.my)) / float(k.fy), 1.0]) * float(k.maxd)
        pts.append((m[:3, :3] @ c + m[:3, 3]) / bs)
    return float(np.abs(pts[1] - pts[0]).max())


def model_pencil(k, depth_mm):
    """(width, depth) in blocks of a 16-pixel tile's pencil of rays at the given depth: what the 16 x 256 ray-space window would have to hold."""
    bs = 8.0 * float(k.voxel)
    z = depth_mm / 1000.0
    return 16.0 * z / float(k.fx) / bs, z / bs


def model_level_gaps(k, levels_mm):
    """The smallest gap (blocks along the view axis) between the truncation bands of consecutive depth levels."""
    bs = 8.0 * float(k.voxel)
    band = lambda d: (d - (float(k.tbase) + float(k.tscale) * d), d + (float(k.tbase) + float(k.tscale) * d))
    z = sorted(levels_mm)
    return min((band(b / 1000.0)[0] - band(a / 1000.0)[1]) / bs for a, b in zip(z, z[1:]))


PREPASS_CASES = _prepass_cases()
ALLOC_CASES = _alloc_cases()

for _c in ALLOC_CASES:
    _k = fx.derive(_c.p)
    if getattr(_c, "sweeps", False):
        assert model_sweep_blocks(_k, _c.passes[0][1]) > 9.0 + 2.0, model_sweep_blocks(_k, _c.passes[0][1])
    elif _c.name.startswith("ray-n"):
        assert model_sweep_blocks(_k, _c.passes[0][1]) < 9.0 - 2.0                                    # ... and nowhere else
    if getattr(_c, "leaves", False):
        w, d = model_pencil(_k, float(_c.passes[0][0].max()))
        assert w > 16 + 2 and d > 256 + 2, (w, d)
    if getattr(_c, "levels", False):
        lv = sorted(set(_c.passes[0][0].ravel().tolist()) - {0})
        assert len(lv) == 9 and model_level_gaps(_k, lv) > 64 + 2, (lv, model_level_gaps(_k, lv))
