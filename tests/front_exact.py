"""The front chain of a fusion pass stated directly (tests/test_front_stages_cpu.py, tests/test_front_stages.py), independent of the kernels of
scannet_amd/csrc/fuser_prepass.hip, fuser_alloc.hip, fuser_compact.hip, fuser_blocks.hip and of oracle/tsdf_oracle.c: no window, no bitmap, no queue, no hash
set, no lane groups -- arrays of numpy.float32 with one rounding per operation, sets of coordinates, and a dictionary {coords: birth}.

  fma          fmaf(a, b, c) is ONE rounding of the exact a b + c.  fma_exact states it through rational arithmetic (tests/clean_exact.py round32); fma32 is the
               same function on arrays: the product of two binary32 values is exact in binary64, the sum is taken with its exact error (TwoSum) and rounded
               to odd, and 53 >= 2 x 24 + 2 bits make the final rounding to binary32 the single rounding asked for.  The CPU module holds fma32 to fma_exact.
  derive       what sf_fuser_create makes of sf_params: the integration camera of a resampled input, the colour camera
  frame_setup  DESIGN 3.2: the inverse of the pose in double, the plane constants, zfar -- each rounded once to binary32
  pre-pass     u16 / shift and the FOUR gates (0, below depth_min, above depth_max, not below max_integration_dist); the nearest resample; the ray-slope
               colour look-up with black outside and the + 0.5f truncation; the packed texel {depth bits | r | g << 8 | b << 16 in the high word}
  rays, walk   DESIGN 3.4: world_to_block rounds half away from zero, then an arithmetic shift; the walk takes x if strictly smallest, else z if below y, else
               y, and ends when the axis that MOVED reaches one past its last block; at most 1024 visits
  in_frustum   DESIGN 3.3 (frustum_mode 0: bounding sphere against four planes and the z range) and 6b (frustum_mode 1: the centre in NDC x 0.95)
  births       a block is born in the first frame of the sequence that names it while it does not exist
  masks        bit j iff the block is in frame j's frustum and birth <= seq0 + j; ghosts are never listed; list length, last-frame count, the two sums
  check_directory   the invariants of table, heap and directory, each rule under its own name
Parameters are any object with the fields of sf_params (scannet_amd._abi.SfParams)."""
from fractions import Fraction
from types import SimpleNamespace
import math

import numpy as np

from tests.clean_exact import round32

F32 = np.float32
NINF = F32(-np.inf)
KEY_EMPTY = 0xFFFFFFFFFFFFFFFF
KEY_TOMB = KEY_EMPTY - 1
MAX_WALK = 1024       # visits of one ray's walk
MAX_PROBES = 4096     # slots a look-up reads before it gives up
C_HEAP_FREE, C_HIGH_WATER, C_ALLOC_FAIL, C_SLOTS_USED = 0, 2, 3, 4   # counter words (scannet_amd/csrc/fuser_internal.h enum Counter)


# ---- fused multiply-add ---------------------------------------------------------------------------------------------------------------------------------
def fma_exact(a, b, c):
    """fmaf of three finite binary32 scalars: the exact rational a b + c, rounded once (ties to even)."""
    q = Fraction(float(F32(a))) * Fraction(float(F32(b))) + Fraction(float(F32(c)))
    return round32(q) if q >= 0 else F32(-round32(-q))


def fma32(a, b, c):
    """fmaf on binary32 arrays (broadcast): see the module docstring.  Non-finite sums are passed through as binary64 computes them."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        up = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        odd = np.where((err != 0) & even, up, s)
        return np.where(np.isfinite(s), odd, s).astype(F32)


# ---- what sf_fuser_create derives -----------------------------------------------------------------------------------------------------------------------
def derive(p):
    k = SimpleNamespace()
    k.W, k.H = int(p.depth_width), int(p.depth_height)
    k.fx, k.fy, k.mx, k.my = F32(p.fx), F32(p.fy), F32(p.mx), F32(p.my)
    k.inW = k.inH = 0
    k.rsx = k.rsy = F32(1)
    iw, ih = int(p.integration_width), int(p.integration_height)
    resample = iw > 0 and ih > 0 and (iw != k.W or ih != k.H)
    if resample:
        k.inW, k.inH, k.W, k.H = k.W, k.H, iw, ih
        k.rsx, k.rsy = F32(k.inW - 1) / F32(k.W - 1), F32(k.inH - 1) / F32(k.H - 1)
        k.fx, k.fy = F32(p.fx) * (F32(k.W) / F32(k.inW)), F32(p.fy) * (F32(k.H) / F32(k.inH))
        k.mx, k.my = F32(p.mx) * (F32(k.W - 1) / F32(k.inW - 1)), F32(p.my) * (F32(k.H - 1) / F32(k.inH - 1))
    k.shift, k.dmin, k.dmax, k.maxd = F32(p.depth_shift), F32(p.depth_min), F32(p.depth_max), F32(p.max_integration_dist)
    k.voxel, k.tbase, k.tscale = F32(p.voxel_size), F32(p.trunc_base), F32(p.trunc_scale)
    own = p.color_width > 0 and p.color_height > 0
    k.cW, k.cH = (int(p.color_width), int(p.color_height)) if own else (0, 0)
    k.cfx, k.cfy, k.cmx, k.cmy = F32(p.cfx), F32(p.cfy), F32(p.cmx), F32(p.cmy)
    if resample and not own:   # colour at the INPUT depth size: its own size as far as the integration camera is concerned
        k.cW, k.cH, k.cfx, k.cfy, k.cmx, k.cmy = k.inW, k.inH, F32(p.fx), F32(p.fy), F32(p.mx), F32(p.my)
    k.frustum_mode = int(p.frustum_mode)
    k.num_buckets, k.bucket_size, k.num_blocks = int(p.hash_num_buckets), int(p.hash_bucket_size), int(p.num_sdf_blocks)
    k.total_slots = k.num_buckets * k.bucket_size
    return k


# ---- DESIGN 3.2 -----------------------------------------------------------------------------------------------------------------------------------------
def frame_setup(k, pose):
    """pose: 16 floats, row-major camToWorld.  T, Ti: rows 0..2 (12 values each)."""
    m = [float(F32(v)) for v in np.asarray(pose).reshape(16)]
    a00, a01, a02, t0, a10, a11, a12, t1, a20, a21, a22, t2 = m[:12]
    c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
    det = a00 * c00 + a01 * c01 + a02 * c02
    inv = [c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det,
           c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det,
           c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det]
    F = SimpleNamespace(T=np.array(m[:12], F32), Ti=np.zeros(12, F32))
    for r in range(3):
        F.Ti[4 * r:4 * r + 3] = inv[3 * r:3 * r + 3]
        F.Ti[4 * r + 3] = -(inv[3 * r] * t0 + inv[3 * r + 1] * t1 + inv[3 * r + 2] * t2)
    rad = 4.0 * math.sqrt(3.0) * float(k.voxel)
    F.radius = F32(rad)
    fx, fy, mx, my = float(k.fx), float(k.fy), float(k.mx), float(k.my)
    xl, xh = mx + 1.5, (float(k.W) - 0.5) - mx      # the voxel rule's (int)(u + 0.5f) truncates (-1, 0) to pixel 0: the lower planes sit at -1.5
    yl, yh = my + 1.5, (float(k.H) - 0.5) - my
    F.xa, F.xc = (F32(fx), F32(-fx)), (F32(xl), F32(xh))
    F.xr = (F32(rad * math.sqrt(fx * fx + xl * xl)), F32(rad * math.sqrt(fx * fx + xh * xh)))
    F.ya, F.yc = (F32(fy), F32(-fy)), (F32(yl), F32(yh))
    F.yr = (F32(rad * math.sqrt(fy * fy + yl * yl)), F32(rad * math.sqrt(fy * fy + yh * yh)))
    F.zfar = F32(k.maxd + fma_exact(k.tscale, k.maxd, k.tbase))
    return F


# ---- DESIGN 3.3 / 6b ------------------------------------------------------------------------------------------------------------------------------------
def camera_point(k, F, blocks):
    """The block centres in camera space, three binary32 arrays."""
    b = np.asarray(blocks, np.int64).reshape(-1, 3)
    c = [((8 * b[:, i]).astype(F32) + F32(3.5)) * k.voxel for i in range(3)]
    M = F.Ti
    return [fma32(M[4 * r], c[0], fma32(M[4 * r + 1], c[1], fma32(M[4 * r + 2], c[2], M[4 * r + 3]))) for r in range(3)]


def in_frustum(k, F, blocks):
    px, py, pz = camera_point(k, F, blocks)
    with np.errstate(all="ignore"):
        if k.frustum_mode == 1:
            zn = ((pz - k.dmin) / (k.dmax - k.dmin)) * F32(0.95)
            ok = (zn >= 0) & (zn <= 1) & (pz > 0)
            u = (px * k.fx) / pz + k.mx
            v = (py * k.fy) / pz + k.my
            wm1, hm1 = F32(k.W - 1), F32(k.H - 1)
            nx = ((F32(2) * u - wm1) / wm1) * F32(0.95)
            ny = ((hm1 - F32(2) * v) / hm1) * F32(0.95)
            return ok & (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1)
        ok = (pz > -F.radius) & (pz < F.zfar + F.radius)
        for a, c, r, q in ((F.xa[0], F.xc[0], F.xr[0], px), (F.xa[1], F.xc[1], F.xr[1], px), (F.ya[0], F.yc[0], F.yr[0], py), (F.ya[1], F.yc[1], F.yr[1], py)):
            ok &= fma32(a, q, c * pz) >= -r
        return ok


def plane_margins(k, F, blocks):
    """frustum_mode 0: per block the six signed margins (>= 0 inside; the two z tests are strict), for the cases that look for blocks on a plane."""
    px, py, pz = camera_point(k, F, blocks)
    out = [pz + F.radius, (F.zfar + F.radius) - pz]
    for a, c, r, q in ((F.xa[0], F.xc[0], F.xr[0], px), (F.xa[1], F.xc[1], F.xr[1], px), (F.ya[0], F.yc[0], F.yr[0], py), (F.ya[1], F.yc[1], F.yr[1], py)):
        out.append(fma32(a, q, c * pz) + r)
    return np.stack(out, 1)


# ---- pre-pass -------------------------------------------------------------------------------------------------------------------------------------------
def resample(k, frame):
    """One input frame (inH x inW) -> the integration image (H x W), nearest; a source position outside reads 0."""
    if k.inW == 0:
        return np.asarray(frame, np.uint16).reshape(k.H, k.W)
    src = np.asarray(frame, np.uint16).reshape(k.inH, k.inW)
    xi = (np.arange(k.W).astype(F32) * k.rsx + F32(0.5)).astype(np.int64)
    yi = (np.arange(k.H).astype(F32) * k.rsy + F32(0.5)).astype(np.int64)
    ok = (yi < k.inH)[:, None] & (xi < k.inW)[None, :]
    return np.where(ok, src[np.minimum(yi, k.inH - 1)[:, None], np.minimum(xi, k.inW - 1)[None, :]], 0).astype(np.uint16)


def depth_to_float(k, u16):
    u = np.asarray(u16, np.uint16)
    v = u.astype(F32) / k.shift
    bad = (u == 0) | (v < k.dmin) | (v > k.dmax) | ~(v < k.maxd)
    return np.where(bad, NINF, v).astype(F32)


def prepass(k, frame):
    """One input frame -> the float depth image H x W."""
    return depth_to_float(k, resample(k, frame))


def colour_lookup(k, rgb):
    """rgb: the colour picture (cH x cW x 3, or H x W x 3 where the fuser has no colour size) -> r | g << 8 | b << 16 per integration pixel, uint32 H x W."""
    if k.cW == 0:
        c = np.asarray(rgb, np.uint8).reshape(k.H, k.W, 3).astype(np.uint32)
        return c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)
    c = np.asarray(rgb, np.uint8).reshape(k.cH, k.cW, 3).astype(np.uint32)
    kx = (np.arange(k.W).astype(F32) - k.mx) / k.fx
    ky = (np.arange(k.H).astype(F32) - k.my) / k.fy
    u = fma32(kx, k.cfx, k.cmx) + F32(0.5)
    v = fma32(ky, k.cfy, k.cmy) + F32(0.5)
    ok = ((v >= 0) & (v < F32(k.cH)))[:, None] & ((u >= 0) & (u < F32(k.cW)))[None, :]
    ui, vi = np.clip(u.astype(np.int64), 0, k.cW - 1), np.clip(v.astype(np.int64), 0, k.cH - 1)     # the cast truncates
    px = c[vi[:, None], ui[None, :]]
    return np.where(ok, px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16), 0).astype(np.uint32)


def texels(depthf, packed):
    return np.asarray(depthf, F32).view(np.uint32).astype(np.uint64) | (np.asarray(packed, np.uint32).astype(np.uint64) << np.uint64(32))


# ---- DESIGN 3.4 -----------------------------------------------------------------------------------------------------------------------------------------
def world_to_block(k, w):
    with np.errstate(all="ignore"):
        q = np.asarray(w, F32) / k.voxel
        vi = np.where(q >= 0, q + F32(0.5), q - F32(0.5)).astype(np.int64)      # round half away from zero: the cast truncates
    return vi >> 3                                                              # arithmetic shift: floor division by 8


def ray_setup(k, F, depthf):
    """The rays of one frame's valid pixels: pixel index, end points p0 / p1, first block, step, one-past-the-last block, tmax, tdelta."""
    d = np.asarray(depthf, F32).reshape(k.H, k.W)
    yy, xx = np.nonzero((d != NINF) & (d < k.maxd))
    d = d[yy, xx]
    t = fma32(k.tscale, d, k.tbase)
    lo, hi = np.minimum(k.maxd, d - t), np.minimum(k.maxd, d + t)
    keep = lo < hi
    yy, xx, lo, hi = yy[keep], xx[keep], lo[keep], hi[keep]
    kx, ky = (xx.astype(F32) - k.mx) / k.fx, (yy.astype(F32) - k.my) / k.fy
    T = F.T

    def point(z):
        cx, cy = kx * z, ky * z
        return np.stack([fma32(T[4 * r], cx, fma32(T[4 * r + 1], cy, fma32(T[4 * r + 2], z, T[4 * r + 3]))) for r in range(3)], 1)
    p0, p1 = point(lo), point(hi)
    with np.errstate(all="ignore"):
        dirv = p1 - p0
        cur, end = world_to_block(k, p0), world_to_block(k, p1)
        step = np.where(dirv > 0, 1, np.where(dirv < 0, -1, 0)).astype(np.int64)
        nb = cur + (step > 0)
        plane = ((8 * nb).astype(F32) - F32(0.5)) * k.voxel
        bsize = F32(8) * k.voxel
        tmax = np.where(step == 0, F32(np.inf), (plane - p0) / dirv).astype(F32)
        tdelta = np.where(step == 0, F32(np.inf), (step.astype(F32) * bsize) / dirv).astype(F32)
    return SimpleNamespace(pixel=yy * k.W + xx, p0=p0, p1=p1, cur=cur, end=end, step=step, bound=end + step, tmax=tmax, tdelta=tdelta)


def walk(rs):
    """Every ray's walk at once -> (ray index, visit number, block) of every visit, in visit order per ray."""
    n = len(rs.pixel)
    cur, tmax = rs.cur.copy(), rs.tmax.copy()
    alive = np.arange(n)
    rays, visits, blocks = [], [], []
    for it in range(MAX_WALK):
        if len(alive) == 0:
            break
        rays.append(alive)
        visits.append(np.full(len(alive), it))
        blocks.append(cur[alive].copy())
        tm = tmax[alive]
        c = np.where((tm[:, 0] < tm[:, 1]) & (tm[:, 0] < tm[:, 2]), 0, np.where(tm[:, 2] < tm[:, 1], 2, 1))
        cur[alive, c] += rs.step[alive, c]
        done = cur[alive, c] == rs.bound[alive, c]
        with np.errstate(all="ignore"):
            tmax[alive, c] = tmax[alive, c] + rs.tdelta[alive, c]
        alive = alive[~done]
    if not rays:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.int64)
    return np.concatenate(rays), np.concatenate(visits), np.concatenate(blocks)


def frame_blocks(k, F, depthf):
    """The blocks one frame names: visited by some ray's walk and inside the frame's frustum -> int64 [m, 3], sorted, unique."""
    _, _, b = walk(ray_setup(k, F, depthf))
    if len(b) == 0:
        return b
    b = np.unique(b, axis=0)
    return b[in_frustum(k, F, b)]


def births(k, poses, frames, seq0, present=None):
    """{(x, y, z): birth} after the frames of a sequence, from `present` (a dictionary of the same kind, left unchanged)."""
    out = dict(present or {})
    for j, (pose, frame) in enumerate(zip(poses, frames)):
        for b in map(tuple, frame_blocks(k, frame_setup(k, pose), prepass(k, frame)).tolist()):
            out.setdefault(b, seq0 + j)
    return out


# ---- compaction -----------------------------------------------------------------------------------------------------------------------------------------
def masks(k, poses, seq0, blocks, birth, ghost):
    """Frame masks of a directory (blocks [m, 3], birth [m], ghost [m]) for the n poses of a pass -> uint32 [m]; 0 = not listed."""
    blocks = np.asarray(blocks, np.int64).reshape(-1, 3)
    m = np.zeros(len(blocks), np.uint32)
    birth = np.asarray(birth, np.int64)
    for j, pose in enumerate(poses):
        inside = in_frustum(k, frame_setup(k, pose), blocks) & (birth <= seq0 + j) & ~np.asarray(ghost, bool)
        m |= inside.astype(np.uint32) << np.uint32(j)
    return m


def mask_summary(m, n):
    m = np.asarray(m, np.uint32)
    listed = m[m != 0]
    pop = int(sum(bin(int(v)).count("1") for v in listed))
    return {"length": int(len(listed)), "last": int(((listed >> np.uint32(n - 1)) & 1).sum()), "total": pop, "tiles": int(len(listed))}


# ---- table, heap, directory -----------------------------------------------------------------------------------------------------------------------------
def pack_key(x, y, z):
    return ((x & 0x1FFFFF) << 42) | ((y & 0x1FFFFF) << 21) | (z & 0x1FFFFF)


def unpack_key(key):
    def s21(v):
        return v - (1 << 21) if v & (1 << 20) else v
    key = int(key)
    return s21((key >> 42) & 0x1FFFFF), s21((key >> 21) & 0x1FFFFF), s21(key & 0x1FFFFF)


def home_slot(k, x, y, z):
    """Where a block's probe sequence starts: its bucket's first slot."""
    h = ((x * 73856093) ^ (y * 19349669) ^ (z * 83492791)) & 0xFFFFFFFF
    return (h % k.num_buckets) * k.bucket_size


def dump_births(dump):
    """{coords: birth} of every block that has a tile."""
    key, ptr, birth = dump["key"], dump["ptr"], dump["birth"]
    return {unpack_key(key[s]): int(birth[s]) for s in np.nonzero((key != KEY_EMPTY) & (key != KEY_TOMB) & (ptr >= 0))[0]}


RULES = ("tombstone", "duplicate-key", "unreachable", "entry-slot", "heap-partition", "slots-used", "heap-free", "high-water", "orphan")


def check_directory(dump, k, relaxed=False, failures_are_orphans=False):
    """The names of the rules a dump violates (sorted; empty = sound).  relaxed: the volume ran out of table or heap -- entries claimed without a tile
    ("orphans") may exist, and then C_ALLOC_FAIL counts at least as many failures (exactly as many where the table never filled: failures_are_orphans)."""
    key, ptr = np.asarray(dump["key"], np.uint64), np.asarray(dump["ptr"], np.int64)
    bkeys, bentry = np.asarray(dump["block_keys"], np.uint64), np.asarray(dump["block_entry"], np.int64)
    heap, cnt = np.asarray(dump["heap"], np.int64), np.asarray(dump["counters"], np.int64)
    nb, total = k.num_blocks, k.total_slots
    assert len(key) == total and len(bkeys) == nb
    bad = set()
    if (key == KEY_TOMB).any():
        bad.add("tombstone")
    used = np.nonzero((key != KEY_EMPTY) & (key != KEY_TOMB))[0]
    if len(np.unique(key[used])) != len(used):
        bad.add("duplicate-key")
    for s in used.tolist():                       # every key is met from its home before any EMPTY
        kk = int(key[s])
        at = home_slot(k, *unpack_key(kk))
        for _ in range(MAX_PROBES):
            if int(key[at]) == kk:
                break
            if int(key[at]) == KEY_EMPTY:
                bad.add("unreachable")
                break
            at = at + 1 if at + 1 < total else 0
        else:
            bad.add("unreachable")
    tiled = used[ptr[used] >= 0]
    orphans = len(used) - len(tiled)
    live = np.nonzero(bkeys != KEY_EMPTY)[0]
    p = ptr[tiled]
    if (p >= nb).any() or len(np.unique(p)) != len(p) or len(tiled) != len(live):
        bad.add("entry-slot")
    else:
        if (bkeys[p] != key[tiled]).any() or (bentry[p] != tiled).any():
            bad.add("entry-slot")
        e = bentry[live]
        if ((e < 0) | (e >= total)).any() or (key[np.clip(e, 0, total - 1)] != bkeys[live]).any() or (ptr[np.clip(e, 0, total - 1)] != live).any():
            bad.add("entry-slot")
    hf = int(cnt[C_HEAP_FREE])
    if not 0 <= hf <= nb or sorted(heap[:max(hf, 0)].tolist() + live.tolist()) != list(range(nb)):
        bad.add("heap-partition")
    if int(cnt[C_SLOTS_USED]) != len(live):
        bad.add("slots-used")
    if hf + len(live) != nb:
        bad.add("heap-free")
    if len(live) and int(cnt[C_HIGH_WATER]) <= int(live.max()):
        bad.add("high-water")
    fails = int(cnt[C_ALLOC_FAIL])
    if (orphans and not relaxed) or orphans > fails or (failures_are_orphans and orphans != fails):
        bad.add("orphan")
    return sorted(bad)
