"""TEST INFRASTRUCTURE -- the statement of the marching-cubes stage in numpy: float32 arrays with ONE rounding per operation, integer
keys, sorts.  It shares no code with oracle/mc_oracle.c or scannet_amd/csrc/mc.hip; the case table comes from the committed header through the parsing
of tests/test_mc_tables.py (which verifies the table from first principles).

    mesh(coords, voxels, owned, voxel_size, thresh_factor) -> dict(keys u64 [nv], pos f32 [nv,3], col u8 [nv,3], idx i32 [nt,3], tkeys u64 [nt])

The rules, one by one:
  * thresh = float32(thresh_factor) * float32(voxel_size), the float32 product;
  * only cubes whose lowest voxel lies in a block with owned[i] are meshed; every block given is readable as a neighbour (a ghost is a block that is
    read and not meshed);
  * a cube takes part iff its 8 corner voxels exist, have w > 0 and |sdf| <= thresh.  NaN fails the comparison, +-inf exceeds every thresh: such a
    corner drops its cubes and no non-finite number reaches an output;
  * a corner is inside iff sdf < 0 in IEEE float32 with denormals kept: +0, -0 are outside, the smallest negative denormal is inside;
  * vertex on the grid edge (lo, hi), lo the end with the smaller coordinate: mu = dl / (dl - dh) (two roundings); position float32(g) * voxel on the
    two other axes and (float32(g_lo) + mu) * voxel on the edge's axis (two roundings); colour (u8)(fma(mu, ch - cl, cl) + 0.5f): the fma is ONE rounding
    of the exact value -- mu has 24 significant bits, ch - cl at most 9, so mu * (ch - cl) + cl is exact in float64 and is rounded to float32 once;
  * mu == 0 and mu == 1 happen (dl == +-0, or dh a denormal that dl - dh absorbs): the vertices of such a triangle coincide in position and differ in
    key; the triangle is emitted;
  * the vertex is identified by the key of its grid edge, 20 bits per voxel coordinate around 2^19 and 2 bits of axis; vertices ascending by key,
    triangles by (cube key, table order);
  * KEY RANGE: a block takes part when it is owned or is the +1 neighbour of an owned block.  Every block that takes part lies in -65536 .. 65535 on
    every axis (voxels -2^19 .. 2^19 - 1), else KeyRangeError names it: beyond, the y and z fields of the key spill into the field above.

Deviation of a float64 evaluation (oracle/spec_literal_mc.py) from this statement, derived from the three groups of roundings, u = 2^-24:
  mu:       fl(dl - dh) and the division, |mu32 - mu| <= 2u(1 + u) since mu <= 1;
  the sum:  fl(g + mu32) = (g + mu32)(1 + e), |g + mu32| <= |g| + 1;
  product:  one more factor (1 + e) on a value of at most (|g| + 1)(1 + u) * voxel.
  |pos32 - pos64| <= voxel * u * (2 + 2(|g| + 1)) * (1 + 2^-20) + 2^-149 = position_bound(g, voxel)   [second-order terms and the denormal spacing]
It scales with |g|: 9.6e-7 m at |g| = 800, voxel 0.01 (the room of test_gpu_mesh_matches_the_literal_marching_cubes spans |g| < 800: within its 1e-6 m),
6.25e-4 m = 1/16 voxel at |g| = 2^19, voxel 0.01, where float32 positions have an ulp of 1/16 voxel (the sum and the product round there).
Colour: 255 * 2u from mu, 255u from the fma's rounding, 255u from + 0.5f: within 0.5 + 1e-3 levels of the unrounded float64 colour.
"""
import numpy as np

from tests import test_mc_tables as tab

F32 = np.float32
KEY_BIAS = 1 << 19
BLOCK_MIN, BLOCK_MAX = -(KEY_BIAS >> 3), (KEY_BIAS >> 3) - 1
CORNERS = np.asarray(tab.CORNERS, np.int64)            # [8, 3] (x, y, z)
NTRI = np.asarray(tab.NTRI, np.int64)
TRIS = np.asarray(tab.TRIS, np.int64)
_a, _b = np.asarray(tab.EDGES)[:, 0], np.asarray(tab.EDGES)[:, 1]
EDGE_AXIS = np.argmax(CORNERS[_a] != CORNERS[_b], 1)
_swap = CORNERS[_a, EDGE_AXIS] > CORNERS[_b, EDGE_AXIS]
EDGE_LO, EDGE_HI = np.where(_swap, _b, _a), np.where(_swap, _a, _b)
assert ((CORNERS[_a] != CORNERS[_b]).sum(1) == 1).all() and (CORNERS[EDGE_HI, EDGE_AXIS] - CORNERS[EDGE_LO, EDGE_AXIS] == 1).all()


class KeyRangeError(ValueError):
    def __init__(self, block):
        super().__init__("block (%d, %d, %d) lies outside the edge-key range" % tuple(block))
        self.block = tuple(int(c) for c in block)


def position_bound(g, voxel):
    """see the module docstring; g = |grid coordinate| (array or scalar), voxel in metres"""
    u = 2.0 ** -24
    return float(F32(voxel)) * u * (2.0 + 2.0 * (np.abs(np.asarray(g, np.float64)) + 1.0)) * (1.0 + 2.0 ** -20) + 2.0 ** -149


def edge_key(g, axis):
    """g int64 [..., 3] inside the key range"""
    g = np.asarray(g, np.int64) + KEY_BIAS
    assert ((g >= 0) & (g < (1 << 20))).all()
    return ((g[..., 0] << 42) | (g[..., 1] << 22) | (g[..., 2] << 2) | np.asarray(axis, np.int64)).astype(np.uint64)


def decode_key(keys):
    """-> (g int64 [n,3], axis [n]) of vertex keys; cube keys (tkeys >> 3) decode with decode_key(cube << 2)"""
    k = np.asarray(keys, np.uint64).astype(np.int64)
    g = np.stack([(k >> 42) & 0xFFFFF, (k >> 22) & 0xFFFFF, (k >> 2) & 0xFFFFF], -1) - KEY_BIAS
    return g, k & 3


def _block_index(coords):
    c = np.asarray(coords, np.int64)
    k = ((c[:, 0] + (1 << 20)) << 42) | ((c[:, 1] + (1 << 20)) << 21) | (c[:, 2] + (1 << 20))
    order = np.argsort(k, kind="stable")
    sk = k[order]
    assert (sk[1:] != sk[:-1]).all(), "a block is given twice"

    def find(q):
        q = np.asarray(q, np.int64)
        kq = ((q[:, 0] + (1 << 20)) << 42) | ((q[:, 1] + (1 << 20)) << 21) | (q[:, 2] + (1 << 20))
        at = np.minimum(np.searchsorted(sk, kq), len(sk) - 1)
        return np.where(sk[at] == kq, order[at], -1)
    return find


def _soup(c, V, nb, voxel, thresh):
    """The triangle soup of owned blocks c [m,3] with neighbour indices nb [m,8] (-1: absent) into V [n,8,8,8] (z, y, x)."""
    m = len(c)
    sdf = np.zeros((m, 9, 9, 9), F32)
    w = np.zeros((m, 9, 9, 9), np.uint8)
    rgb = np.zeros((m, 9, 9, 9, 3), np.uint8)
    for i in range(8):
        dx, dy, dz = i & 1, (i >> 1) & 1, i >> 2
        rows = np.nonzero(nb[:, i] >= 0)[0]
        if not len(rows):
            continue
        dst = tuple(slice(8, 9) if d else slice(0, 8) for d in (dz, dy, dx))
        src = tuple(slice(0, 1) if d else slice(0, 8) for d in (dz, dy, dx))
        blk = V[nb[rows, i]][(slice(None),) + src]
        sub = (rows[:, None, None, None],) + tuple(np.arange(9)[s].reshape(sh) for s, sh in zip(dst, ((-1, 1, 1), (1, -1, 1), (1, 1, -1))))
        sdf[sub] = blk["sdf"]
        w[sub] = blk["w"]                                   # an absent neighbour leaves w = 0: its voxels do not exist
        for q, ch in enumerate("rgb"):
            rgb[sub + (q,)] = blk[ch]
    with np.errstate(invalid="ignore"):
        valid = (w > 0) & (np.abs(sdf) <= thresh)           # NaN compares false
        inside = sdf < F32(0.0)
    ok = np.ones((m, 8, 8, 8), bool)
    case = np.zeros((m, 8, 8, 8), np.int64)
    for i in range(8):
        ox, oy, oz = CORNERS[i]
        ok &= valid[:, oz:oz + 8, oy:oy + 8, ox:ox + 8]
        case |= inside[:, oz:oz + 8, oy:oy + 8, ox:ox + 8].astype(np.int64) << i
    bi, lz, ly, lx = np.nonzero(ok & (NTRI[case] > 0))
    cs = case[bi, lz, ly, lx]
    nt = NTRI[cs]
    rep = np.repeat(np.arange(len(bi)), nt)
    t = np.arange(len(rep)) - np.repeat(np.cumsum(nt) - nt, nt)
    l = np.stack([lx, ly, lz], 1)[rep]                                         # [T, 3] local cube origin
    g = c[bi[rep]] * 8 + l
    tkeys = ((edge_key(g, 0) >> np.uint64(2)) << np.uint64(3)) | t.astype(np.uint64)
    e = TRIS[cs[rep][:, None], 3 * t[:, None] + np.arange(3)[None, :]]         # [T, 3] cube edges
    assert (e >= 0).all()
    a, b, axis = EDGE_LO[e], EDGE_HI[e], EDGE_AXIS[e]
    la, lb = l[:, None, :] + CORNERS[a], l[:, None, :] + CORNERS[b]            # [T, 3, 3] tile coordinates of the end points
    B = bi[rep][:, None]
    dl, dh = sdf[B, la[..., 2], la[..., 1], la[..., 0]], sdf[B, lb[..., 2], lb[..., 1], lb[..., 0]]
    assert ((dl < 0) != (dh < 0)).all()
    mu = dl / (dl - dh)                                                        # float32: two roundings
    gl = c[bi[rep]][:, None, :] * 8 + la
    pos = gl.astype(F32)
    onaxis = np.arange(3)[None, None, :] == axis[..., None]
    pos = np.where(onaxis, pos + mu[..., None], pos) * voxel                   # float32 sum, float32 product
    cl = rgb[B, la[..., 2], la[..., 1], la[..., 0]].astype(np.float64)
    ch = rgb[B, lb[..., 2], lb[..., 1], lb[..., 0]].astype(np.float64)
    fused = (mu.astype(np.float64)[..., None] * (ch - cl) + cl).astype(F32)    # exact in float64, ONE rounding
    col = (fused + F32(0.5)).astype(np.int64).astype(np.uint8)                 # values in [0.5, 255.5]: the C cast truncates
    return tkeys, edge_key(gl, axis).reshape(-1), pos.reshape(-1, 3).astype(F32), col.reshape(-1, 3)


def mesh(coords, voxels, owned, voxel_size, thresh_factor, chunk=128):
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    n = len(coords)
    owned = np.ones(n, bool) if owned is None else np.asarray(owned, bool)
    V = np.asarray(voxels).reshape(n, 8, 8, 8)
    voxel = F32(voxel_size)
    thresh = F32(thresh_factor) * voxel
    find = _block_index(coords) if n else None
    own = np.nonzero(owned)[0]
    c = coords[own]
    nb = np.stack([find(c + np.array([i & 1, (i >> 1) & 1, i >> 2])) for i in range(8)], 1) if len(own) else np.zeros((0, 8), np.int64)
    for i in range(8):
        q = c + np.array([i & 1, (i >> 1) & 1, i >> 2])
        out = ((q < BLOCK_MIN) | (q > BLOCK_MAX)).any(1) & (nb[:, i] >= 0)
        if out.any():
            raise KeyRangeError(q[np.nonzero(out)[0][0]])
    parts = [_soup(c[s:s + chunk], V, nb[s:s + chunk], voxel, thresh) for s in range(0, len(own), chunk)]
    if not parts or not sum(len(p[0]) for p in parts):
        return dict(keys=np.zeros(0, np.uint64), pos=np.zeros((0, 3), F32), col=np.zeros((0, 3), np.uint8), idx=np.zeros((0, 3), np.int32),
                    tkeys=np.zeros(0, np.uint64))
    tkeys, vkeys, pos, col = (np.concatenate([p[i] for p in parts]) for i in range(4))
    uk, first, inv = np.unique(vkeys, return_index=True, return_inverse=True)
    # an edge is shared by up to four cubes, which read the same two voxels: every copy of a vertex is the same bytes
    assert np.array_equal(pos[first][inv].view(np.uint32), pos.view(np.uint32)) and np.array_equal(col[first][inv], col)
    order = np.argsort(tkeys, kind="stable")
    assert (np.diff(tkeys[order].astype(np.int64)) > 0).all()
    return dict(keys=uk, pos=pos[first], col=col[first], idx=inv.reshape(-1, 3)[order].astype(np.int32), tkeys=tkeys[order])


def unclosed_sides(keys, idx, tkeys):
    """Closure of a mesh, from its arrays alone (no case table).  A triangle side joins two vertices = two grid edges; the cubes that hold both are its
    surrounding cubes (one for a side inside a cube, two for a side on a cube face).  Of every side whose surrounding cubes all carry triangles:
    -> (number of such sides, the sides that are not matched one to one by a side in the opposite direction [k, 2] vertex ids,
        how many directed sides occur twice -- two sheets touching along a face segment, each direction then twice)."""
    g, axis = decode_key(keys)
    hi = g.copy()
    hi[np.arange(len(g)), axis] += 1
    idx = np.asarray(idx, np.int64)
    a, b = idx.reshape(-1), idx[:, [1, 2, 0]].reshape(-1)
    lo_box = np.minimum(g[a], g[b])                      # g is each edge's lower end
    hi_box = np.maximum(hi[a], hi[b])
    cubes = np.unique(np.asarray(tkeys, np.uint64) >> np.uint64(3))
    closed = np.ones(len(a), bool)
    some = np.zeros(len(a), bool)
    for d in range(8):
        cgrid = lo_box - np.array([d & 1, (d >> 1) & 1, d >> 2])
        rows = np.nonzero((cgrid + 1 >= hi_box).all(1))[0]            # the cube [cgrid, cgrid + 1]^3 holds both edges
        want = edge_key(cgrid[rows], 0) >> np.uint64(2)
        at = np.minimum(np.searchsorted(cubes, want), len(cubes) - 1)
        closed[rows] &= cubes[at] == want
        some[rows] = True
    assert some.all()
    nv = np.int64(len(keys))
    fwd, back = a * nv + b, b * nv + a
    ids, cnt = np.unique(fwd, return_counts=True)

    def count_of(q):
        at = np.minimum(np.searchsorted(ids, q), len(ids) - 1)
        return np.where(ids[at] == q, cnt[at], 0)
    nf, nb = count_of(fwd), count_of(back)
    bad = closed & ((nf != nb) | (nf > 2))
    twice = int((closed & (nf == 2)).sum())
    return int(closed.sum()), np.stack([a[bad], b[bad]], 1), twice
