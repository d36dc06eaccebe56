"""TEST INFRASTRUCTURE -- the cases of the marching-cubes pin (tests/test_mc_stages_cpu.py, tests/test_mc_stages.py): blocks written voxel by voxel,
not fused from frames, so that they reach what a fused room never does.  A case is (coords int32 [n,3], voxels VOXEL_DTYPE [n,512], owned bool [n],
voxel_size, thresh_factor); owned blocks go into the fuser with import_blocks(ghost=False), the others with ghost=True.

Every builder ASSERTS its own coverage from the arrays it wrote (cube configurations by plain sign arithmetic, never through the statement), so that a
changed seed cannot hollow a case out.  `expect` carries what the tests check beyond equality of the parties:
    cubes      the exact set of cube origins [k,3] that carry triangles
    dropped    (base case, cube origins): the mesh is the base's without exactly these cubes, everything else the same bytes
    same_as    base case: the same mesh, byte for byte
    restrict   (base case, ghost block coords): the base's mesh restricted to the cubes of owned blocks
    empty      no triangle although blocks are live
    degenerate cube origins whose triangles have three vertices equal in position and distinct in key
    key_range  block the refusal names: every party refuses the volume

colour-fused-differs is one edge found by a search over 2^24 random (dl, dh, cl, ch) with dl in (0, thresh), dh in (-thresh, 0) (numpy default_rng
(2024), 30 hits): dl = 0x3D245164, dh = 0xBD8187A7, red 175 -> 32: the single rounding of the fma gives byte 119, a separately rounded product 120.
"""
import itertools

import numpy as np

from scannet_amd import fusion
from scannet_amd.fusion import VOXEL_DTYPE
from tests import mc_exact as mx

F32 = np.float32
CORNERS = mx.CORNERS
CLASS_NAMES = ("interior", "+x", "+y", "xy", "+z", "xz", "yz", "xyz")     # bit 0: lx == 7, bit 1: ly == 7, bit 2: lz == 7
CHECKER = 0b01011010


class Case:
    def __init__(self, name, coords, voxels, owned=None, voxel_size=0.01, thresh_factor=10.0, **expect):
        self.name = name
        self.coords = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
        self.voxels = np.ascontiguousarray(voxels, VOXEL_DTYPE).reshape(len(self.coords), 512)
        self.owned = np.ones(len(self.coords), bool) if owned is None else np.asarray(owned, bool)
        self.voxel_size, self.thresh_factor = voxel_size, thresh_factor
        self.expect = expect

    def __repr__(self):
        return self.name

    @property
    def thresh(self):
        return F32(self.thresh_factor) * F32(self.voxel_size)

    def params(self, **over):
        """a small table and heap: the directory twice the blocks"""
        nb = 64
        while nb < 2 * len(self.coords):
            nb *= 2
        kw = dict(voxel_size=self.voxel_size, mc_thresh_factor=self.thresh_factor, num_sdf_blocks=nb, hash_num_buckets=nb, hash_bucket_size=2)
        kw.update(over)
        return fusion.default_params(**kw)

    def oracle_params(self, orc):
        p = orc.default_params(voxel=self.voxel_size)
        p.mc_thresh_factor = self.thresh_factor
        return p

    def fill(self, f, order=None):
        """import into a fuser: owned blocks as its own, the others as ghosts"""
        idx = np.arange(len(self.coords)) if order is None else np.asarray(order)
        own = idx[self.owned[idx]]
        gh = idx[~self.owned[idx]]
        if len(own):
            f.import_blocks(self.coords[own], self.voxels[own], ghost=False)
        if len(gh):
            f.import_blocks(self.coords[gh], self.voxels[gh], ghost=True)


# ---- dense bricks -----------------------------------------------------------------------------------------------------------------------------------------
def random_dense(rng, shape, thresh, lo_frac=0.02):
    """D[X, Y, Z]: sdf of random sign and magnitude in (lo_frac, 0.98) * thresh, random colours, w in 1 .. 255"""
    D = np.zeros(shape, VOXEL_DTYPE)
    mag = (F32(lo_frac) + rng.random(shape, dtype=np.float32) * F32(0.98 - lo_frac)) * F32(thresh)
    D["sdf"] = np.where(rng.random(shape) < 0.5, -mag, mag).astype(F32)
    for ch in "rgb":
        D[ch] = rng.integers(0, 256, shape)
    D["w"] = rng.integers(1, 256, shape)
    assert (np.abs(D["sdf"]) < thresh).all() and (D["sdf"] != 0).all()
    return D


def blocks_of(D, lo):
    """dense D[X, Y, Z] (every extent a multiple of 8) with its lowest block at block coordinates lo -> (coords [n,3], voxels [n,512])"""
    nx, ny, nz = (s // 8 for s in D.shape)
    vox = D.reshape(nx, 8, ny, 8, nz, 8).transpose(0, 2, 4, 5, 3, 1).reshape(-1, 512)
    coords = np.array(list(itertools.product(range(nx), range(ny), range(nz))), np.int64) + np.asarray(lo, np.int64)
    return coords.astype(np.int32), np.ascontiguousarray(vox)


def cube_cases(D):
    """configuration of every cube of a dense brick whose 8 corners lie in it: [X-1, Y-1, Z-1]"""
    inside = D["sdf"] < 0
    sx, sy, sz = (s - 1 for s in D.shape)
    case = np.zeros((sx, sy, sz), np.int64)
    for i, (ox, oy, oz) in enumerate(CORNERS):
        case |= inside[ox:ox + sx, oy:oy + sy, oz:oz + sz].astype(np.int64) << i
    return case


def set_config(D, origin, config):
    for i, off in enumerate(CORNERS):
        p = tuple(np.asarray(origin) + off)
        m = np.abs(D["sdf"][p])
        D["sdf"][p] = -m if (config >> i) & 1 else m


def touching(p, shape):
    """origins of the cubes of a dense brick that have voxel p as a corner"""
    out = []
    for d in itertools.product((0, 1), repeat=3):
        o = np.asarray(p) - d
        if (o >= 0).all() and (o + 1 < np.asarray(shape)).all():
            out.append(o)
    return np.array(out, np.int64)


def _meshed(D, lo):
    """origins (global voxel coordinates) of the cubes of a solid, all-valid dense brick that carry triangles"""
    case = cube_cases(D)
    o = np.argwhere((case != 0) & (case != 255))
    return o + 8 * np.asarray(lo, np.int64)


# ---- all-cases --------------------------------------------------------------------------------------------------------------------------------------------
def all_cases(seed=11):
    """8x8x8 blocks at -4 .. 3: every one of the 256 configurations in every one of the 8 halo classes, on pairwise disjoint cubes (local origins in
    {1, 3, 5, 7}^3: the intervals [1,2] [3,4] [5,6] [7,8] do not meet)."""
    rng = np.random.default_rng(seed)
    c = Case("all-cases", *blocks_of(random_dense(rng, (64, 64, 64), F32(10) * F32(0.01)), (-4, -4, -4)))
    D = _dense_of(c, (-4, -4, -4), (8, 8, 8))
    for cls in range(8):
        loc = [(7,) if (cls >> a) & 1 else (1, 3, 5) for a in range(3)]
        blk = [range(7) if (cls >> a) & 1 else range(8) for a in range(3)]      # the +1 neighbour must exist
        cand = np.array([np.array(b) * 8 + np.array(l) for b in itertools.product(*blk) for l in itertools.product(*loc)])
        pick = cand[rng.permutation(len(cand))[:256]]
        assert len(pick) == 256
        for config, origin in enumerate(pick):
            set_config(D, origin, config)
    c.coords, c.voxels = blocks_of(D, (-4, -4, -4))
    case = cube_cases(D)
    o = np.argwhere(np.ones_like(case, bool))
    cls = ((o[:, 0] & 7) == 7) | (((o[:, 1] & 7) == 7) << 1) | (((o[:, 2] & 7) == 7) << 2)
    table = np.bincount(cls * 256 + case.ravel(), minlength=8 * 256).reshape(8, 256)
    assert (table > 0).all(), "all-cases: a configuration is missing in a halo class"
    c.expect["cubes"] = _meshed(D, (-4, -4, -4))
    c.table = table
    return c


def _dense_of(case, lo, nblocks):
    nx, ny, nz = nblocks
    assert len(case.coords) == nx * ny * nz
    return np.ascontiguousarray(case.voxels.reshape(nx, ny, nz, 8, 8, 8).transpose(0, 5, 1, 4, 2, 3).reshape(8 * nx, 8 * ny, 8 * nz))


# ---- gates ------------------------------------------------------------------------------------------------------------------------------------------------
def _brick2(rng, voxel=0.01, factor=10.0):
    return random_dense(rng, (16, 16, 16), F32(factor) * F32(voxel))


def gates(seed=12):
    out = []
    rng = np.random.default_rng(seed)
    D0 = _brick2(rng)
    base = Case("gates-base", *blocks_of(D0, (0, 0, 0)), cubes=_meshed(D0, (0, 0, 0)))
    out.append(base)

    def perturbed(name, D, points, **kw):
        t = np.unique(np.concatenate([touching(p, D.shape) for p in points]), axis=0)
        case0 = cube_cases(D0 if "base_dense" not in kw else kw.pop("base_dense"))
        t = t[(case0[tuple(t.T)] != 0) & (case0[tuple(t.T)] != 255)]
        assert len(t) >= 4 * len(points), name              # the perturbed voxels sit on meshed cubes
        return Case(name, *blocks_of(D, (0, 0, 0)), dropped=(kw.pop("base", base), t), **kw)
    for name, p in (("gates-w0-interior", (3, 4, 5)), ("gates-w0-low-face", (8, 3, 3)), ("gates-w0-corner-of-xyz-neighbour", (8, 8, 8))):
        D = D0.copy()
        D["w"][p] = 0
        out.append(perturbed(name, D, [p]))
    for factor, voxel in ((10.0, 0.01), (10.0, 0.004), (2.5, 0.01)):
        t = F32(factor) * F32(voxel)
        Db = _brick2(rng, voxel, factor)
        tag = "f%g-v%g" % (factor, voxel)
        b = Case("gates-thresh-base-" + tag, *blocks_of(Db, (0, 0, 0)), voxel_size=voxel, thresh_factor=factor, cubes=_meshed(Db, (0, 0, 0)))
        A, B = (5, 6, 7), (8, 12, 3)
        on, off = Db.copy(), Db.copy()
        on["sdf"][A], on["sdf"][B] = t, -t                                                  # |sdf| == thresh: kept
        off["sdf"][A], off["sdf"][B] = np.nextafter(t, F32(np.inf)), -np.nextafter(t, F32(np.inf))
        assert abs(on["sdf"][A]) == t and abs(on["sdf"][B]) == t and off["sdf"][A] > t and off["sdf"][B] < -t
        out += [b, Case("gates-thresh-on-" + tag, *blocks_of(on, (0, 0, 0)), voxel_size=voxel, thresh_factor=factor, cubes=_meshed(on, (0, 0, 0))),
                perturbed("gates-thresh-above-" + tag, off, [A, B], base=b, base_dense=Db, voxel_size=voxel, thresh_factor=factor)]
    D = D0.copy()
    pts = [(2, 2, 2), (8, 7, 11), (13, 8, 5)]
    for p, v in zip(pts, (np.nan, np.inf, -np.inf)):
        D["sdf"][p] = v
        assert D["w"][p] > 0
    out.append(perturbed("gates-nan-inf", D, pts))
    D = D0.copy()
    D["w"][3, 4, 5], D["w"][8, 8, 8], D["w"][7, 8, 3], D["w"][12, 1, 8] = 1, 255, 1, 255
    out.append(Case("gates-w1-w255", *blocks_of(D, (0, 0, 0)), same_as=base))
    return out


# ---- missing neighbour ------------------------------------------------------------------------------------------------------------------------------------
def missing_neighbour(seed=13):
    out = []
    rng = np.random.default_rng(seed)
    D0 = _brick2(rng)
    coords, vox = blocks_of(D0, (0, 0, 0))
    base = Case("neighbour-base", coords, vox, cubes=_meshed(D0, (0, 0, 0)))
    out.append(base)
    allc = _meshed(D0, (0, 0, 0))
    for i in range(1, 8):
        nbc = np.array([i & 1, (i >> 1) & 1, i >> 2])
        at = int(np.nonzero((coords == nbc).all(1))[0][0])
        # cubes with a corner in block nbc
        reads = np.zeros(len(allc), bool)
        for off in CORNERS:
            reads |= (((allc + off) >> 3) == nbc).all(1)
        of_origin = ((allc >> 3) == 0).all(1) & reads
        want = {1: 64, 2: 8, 3: 1}[bin(i).count("1")]
        cls = np.array([(allc[:, a] & 7) == 7 for a in range(3) if (i >> a) & 1]).all(0)
        assert np.array_equal(of_origin, ((allc >> 3) == 0).all(1) & cls) and want - 2 <= of_origin.sum() <= want, (i, of_origin.sum())
        keep = np.arange(8) != at
        out.append(Case("neighbour-absent-%s" % CLASS_NAMES[i], coords[keep], vox[keep], dropped=(base, allc[reads])))
        out.append(Case("neighbour-ghost-%s" % CLASS_NAMES[i], coords, vox, owned=keep, restrict=(base, nbc[None, :])))
    D = random_dense(rng, (24, 24, 24), F32(10) * F32(0.01))
    c3, v3 = blocks_of(D, (-1, -1, -1))
    b3 = Case("neighbour-base-3x3x3", c3, v3, cubes=_meshed(D, (-1, -1, -1)))
    out += [b3, Case("neighbour-ghost-surrounded", c3, v3, owned=~(c3 == 0).all(1), restrict=(b3, np.zeros((1, 3), np.int64)))]
    return out


# ---- zeros ------------------------------------------------------------------------------------------------------------------------------------------------
def zeros(seed=14):
    rng = np.random.default_rng(seed)
    t = F32(10) * F32(0.01)
    den = F32(-1e-45)
    assert den < 0 and den == np.nextafter(F32(0), F32(-1)) and F32(-0.0) == 0 and not (F32(-0.0) < 0)
    D = _brick2(rng)
    half = F32(0.5) * t

    def plant(origin, values):
        """corner i of the cube gets values[i]; the voxels around it stay as they are"""
        for i, off in enumerate(CORNERS):
            D["sdf"][tuple(np.asarray(origin) + off)] = values[i]
    cubes = {}
    # +0 and -0 are outside: a cube of them among positive corners has no triangle
    plant((1, 1, 1), [F32(0.0), F32(-0.0), half, F32(0.0), F32(-0.0), half, half, half]); cubes["none"] = [(1, 1, 1)]
    # the smallest negative denormal is inside.  Corner 6 = (1,1,1) is the high end of its three edges: dl = thresh, dh = -denormal -> mu == 1
    plant((4, 1, 1), [half, half, t, half, half, t, den, t]); cubes["mu1"] = (4, 1, 1)
    # corner 0 is the low end of its three edges: dl = +0 outside, dh < 0 -> mu == 0 (and -0 likewise: mu == -0)
    plant((1, 4, 1), [F32(0.0), -half, -half, -half, -half, -half, -half, -half]); cubes["mu0"] = (1, 4, 1)
    plant((4, 4, 1), [F32(-0.0), -half, -half, -half, -half, -half, -half, -half]); cubes["mu-0"] = (4, 4, 1)
    # a denormal inside corner at the low end: mu = denormal / thresh, a denormal or zero: the position is the corner's
    plant((1, 1, 4), [den, t, t, t, t, t, t, t]); cubes["den-lo"] = (1, 1, 4)
    assert (t / (t - den)) == 1 and (F32(0.0) / (F32(0.0) - (-half))) == 0
    case = cube_cases(D)
    assert case[1, 1, 1] == 0 and case[4, 1, 1] == 1 << 6 and case[1, 4, 1] == 254 and case[4, 4, 1] == 254 and case[1, 1, 4] == 1
    deg = np.array([cubes[k] for k in ("mu1", "mu0", "mu-0", "den-lo")], np.int64)
    # the literal float64 evaluation divides by (dl - dh) too: every planted value is exact in float64
    out = [Case("zeros-signs", *blocks_of(D, (0, 0, 0)), cubes=_meshed(D, (0, 0, 0)), degenerate=deg)]
    for name, sdf, w in (("zeros-all-positive", half, 7), ("zeros-all-negative", -half, 7), ("zeros-all-w0", None, 0)):
        E = _brick2(rng)
        if sdf is not None:
            E["sdf"] = sdf
        E["w"] = w
        out.append(Case(name, *blocks_of(E, (0, 0, 0)), empty=True, cubes=np.zeros((0, 3), np.int64)))
    return out


# ---- colour -----------------------------------------------------------------------------------------------------------------------------------------------
def colour(seed=15):
    rng = np.random.default_rng(seed)
    t = F32(10) * F32(0.01)
    D = random_dense(rng, (160, 160, 8), t)
    D["sdf"][:, :, :4], D["sdf"][:, :, 4:] = t, -t                       # dl = t, dh = -t on every z-edge between z = 3 and z = 4: mu == 1/2
    assert t / (t - (-t)) == F32(0.5)
    lo = np.stack([D[ch][:, :, 3] for ch in "rgb"], -1)
    hi = np.stack([D[ch][:, :, 4] for ch in "rgb"], -1)
    pair = np.arange(65536)
    lo.reshape(-1)[:65536], hi.reshape(-1)[:65536] = pair >> 8, pair & 255
    for q, ch in enumerate("rgb"):
        D[ch][:, :, 3], D[ch][:, :, 4] = lo[..., q], hi[..., q]
    got = np.stack([D[ch][:, :, 3].astype(np.int64) * 256 + D[ch][:, :, 4] for ch in "rgb"], -1)
    # every z-edge between z = 3 and z = 4 survives: the edge at (x, y) belongs to the cube at (min(x, 158), min(y, 158), 3), whose neighbours exist
    assert len(np.unique(got)) == 65536, "colour: a (cl, ch) pair is missing"
    o = np.argwhere(np.ones((159, 159), bool))
    slab = Case("colour-all-pairs", *blocks_of(D, (-10, -10, 0)), cubes=np.concatenate([o, np.full((len(o), 1), 3)], 1) + np.array([-80, -80, 0]))
    E = _brick2(rng)
    for ch in "rgb":
        E[ch] = rng.choice(np.array([0, 1, 254, 255], np.uint8), E.shape)
    ends = Case("colour-extremes-random-mu", *blocks_of(E, (0, 0, 0)), cubes=_meshed(E, (0, 0, 0)))
    G = _brick2(rng)
    dl, dh = np.array([0x3D245164], np.uint32).view(F32)[0], np.array([0xBD8187A7], np.uint32).view(F32)[0]
    G["sdf"][5, 5, 5], G["sdf"][5, 5, 6], G["r"][5, 5, 5], G["r"][5, 5, 6] = dl, dh, 175, 32
    mu = dl / (dl - dh)
    fused = F32(np.float64(mu) * (32.0 - 175.0) + 175.0)
    unfused = F32(mu * F32(32.0 - 175.0)) + F32(175.0)
    assert 0 < dl < t and -t < dh < 0 and int(fused + F32(0.5)) == 119 and int(unfused + F32(0.5)) == 120
    one = Case("colour-fused-differs", *blocks_of(G, (0, 0, 0)), cubes=_meshed(G, (0, 0, 0)))
    one.edge = (mx.edge_key(np.array([5, 5, 5]), 2), 119)
    return [slab, ends, one]


# ---- key range --------------------------------------------------------------------------------------------------------------------------------------------
def key_range(seed=16):
    out = []
    rng = np.random.default_rng(seed)
    for a in range(3):
        for name, b0 in (("low", mx.BLOCK_MIN), ("high", mx.BLOCK_MAX - 1)):
            D = _brick2(rng)
            lo = [0, 0, 0]
            lo[a] = b0
            c = Case("key-range-%s-%s" % (name, "xyz"[a]), *blocks_of(D, lo), cubes=_meshed(D, lo))
            g = c.expect["cubes"][:, a]
            assert (g.min() == -(1 << 19)) if name == "low" else (g.max() + 1 == (1 << 19) - 1)     # the extreme cube is meshed
            out.append(c)
    for name, a, b0, bad in (("beyond-high-y", 1, mx.BLOCK_MAX, mx.BLOCK_MAX + 1), ("beyond-low-z", 2, mx.BLOCK_MIN - 1, mx.BLOCK_MIN - 1)):
        D = _brick2(rng)
        lo = [0, 0, 0]
        lo[a] = b0
        c = Case("key-range-" + name, *blocks_of(D, lo), key_range=(a, bad))
        out.append(c)
    return out


# ---- prefix extremes --------------------------------------------------------------------------------------------------------------------------------------
def prefix_extremes(seed=17):
    """One meshed cube per block at cube 0, cube 511, lane 63 of wave 0 and lane 0 of wave 1 (cube index = lz * 64 + ly * 8 + lx): only the cube's 8
    corners have w > 0.  Then an empty block between two full of checkerboard cubes (4 triangles each)."""
    rng = np.random.default_rng(seed)
    t = F32(10) * F32(0.01)
    spots = {"cube0": (0, 0, 0), "cube511": (7, 7, 7), "wave0-lane63": (7, 7, 0), "wave1-lane0": (0, 0, 1)}
    assert [z * 64 + y * 8 + x for x, y, z in spots.values()] == [0, 511, 63, 64]
    coords, vox, cubes = [], [], []
    for k, (name, l) in enumerate(spots.items()):
        for rep in range(2):
            D = random_dense(rng, (16, 16, 16), t)
            D["w"] = 0
            lo = (4 * k, 4 * rep, 0)
            for off in CORNERS:
                D["w"][tuple(np.asarray(l) + off)] = 200
            set_config(D, l, CHECKER)
            c, v = blocks_of(D, lo)
            coords.append(c); vox.append(v); cubes.append(np.asarray(l) + 8 * np.asarray(lo))
    one = Case("prefix-single-cubes", np.concatenate(coords), np.concatenate(vox), cubes=np.array(cubes, np.int64))
    D = random_dense(rng, (24, 8, 8), t)
    x, y, z = np.meshgrid(np.arange(24), np.arange(8), np.arange(8), indexing="ij")
    D["sdf"] = np.where((x + y + z) & 1, -1, 1) * np.abs(D["sdf"])
    D["sdf"][8:16] = np.abs(D["sdf"][8:16])
    D["sdf"][7], D["sdf"][16] = np.abs(D["sdf"][7]), np.abs(D["sdf"][16])        # the middle block's neighbours end in a positive layer: it stays empty
    case = cube_cases(D)
    assert set(np.unique(case[:6, :, :])) == {CHECKER, CHECKER ^ 255} and (case[7:15] == 0).all()
    assert mx.NTRI[CHECKER] == 4 and mx.NTRI[CHECKER ^ 255] == 4
    cz, vz = blocks_of(D, (0, 0, 0))
    # single row of blocks: the cubes at ly == 7 or lz == 7 lack a neighbour
    m = _meshed(D, (0, 0, 0))
    m = m[(m[:, 1] < 7) & (m[:, 2] < 7)]
    assert not ((m[:, 0] >= 8) & (m[:, 0] < 16)).any() and (m[:, 0] < 8).sum() > 300 and (m[:, 0] >= 16).sum() > 300
    return [one, Case("prefix-empty-between-checkers", cz, vz, cubes=m)]


# ---- dense checker ----------------------------------------------------------------------------------------------------------------------------------------
def dense_n(num_cus):
    n = 1
    while n ** 3 <= 8 * num_cus:
        n += 1
    return n


def dense_checker(n, seed=18):
    """n^3 blocks, a sign checkerboard on every voxel: 4 triangles in every cube"""
    rng = np.random.default_rng(seed)
    D = random_dense(rng, (8 * n,) * 3, F32(10) * F32(0.01), lo_frac=0.1)
    x, y, z = np.meshgrid(*(np.arange(8 * n),) * 3, indexing="ij")
    D["sdf"] = (np.where((x + y + z) & 1, -1, 1) * np.abs(D["sdf"])).astype(F32)
    c = Case("dense-checker-%d" % n, *blocks_of(D, (-(n // 2),) * 3))
    c.n_tris = 4 * (8 * n - 1) ** 3
    c.n_verts = 3 * (8 * n - 1) * (8 * n) ** 2          # every grid edge of the (8n)^3 voxels changes sign and belongs to a cube
    return c


_cache = {}


def cases():
    """every case but the device-sized dense checker; built once"""
    if "all" not in _cache:
        _cache["all"] = [all_cases()] + gates() + missing_neighbour() + zeros() + colour() + key_range() + prefix_extremes() + [dense_checker(3)]
    return _cache["all"]


def by_name(name):
    return next(c for c in cases() if c.name == name)
