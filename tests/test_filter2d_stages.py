"""2-D annotation filter, stage by stage (scannet_amd/csrc/filter2d.hip; AnnotationTools/Filter2dAnnotations/filter.cu).

Three parties:
  * the HIP kernels, one per call through the stage hooks of include/scanfuse_internal.h (scannet_amd.filter2d.stage_* / selftest_gauss);
  * the checker oracle/filter2d_oracle.c, the float restatement the kernels are held to bit for bit;
  * a float64 numpy statement of the same filters, written here from the definitions in filter.cu (bilateral :210-247, validity-aware bilinear
    resample :514-560, nearest resample :647-665, vote :1020-1059) and sharing no code with either.

CPU part: the checker against the float64 statement on the very inputs the GPU tests use.  Float maps agree within FLOAT_BOUND; vote labels agree
on every pixel whose two strongest bins the float64 statement separates by more than VOTE_MARGIN, and at most 1 % of an image may fail to.
GPU part (-m gpu): every kernel against the checker's matching or_f2d_* function, bit for bit, at the shapes where a kernel can go wrong (smaller than
the window, one tile, a ragged second tile, holes, an all-invalid image, the real ScanNet geometry for the resamples), the device's gauss_r / gauss_d2
against the checker's over every distance the pipeline can form, and the refusal of a radius the frame path could not launch.

One thing no test here can see, by construction: the spatial table exp(-(dx^2 + dy^2) / (2 sigma^2)) is symmetric in (dx, dy), and x*x + y*y is the same
binary32 number either way round, so a transposed s_gd index reads the same bits.  What IS order-dependent is the order of the taps in the float32
running sums (column by column in the bilateral filter, row by row in the vote); the non-symmetric images below change bits when it is exchanged."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from oracle import oracle as orc
from scannet_amd import filter2d

MINF = np.float32(-np.inf)

# Largest relative difference of a float map between the checker and the float64 statement, measured on the CPU over every bilateral and resample
# case below: 1.51e-06 (bilateral, "50x37 holes" at sigma_d 6; "17x33 skew" 1.28e-06; the resamples stay under 2.1e-07).  Most of it is not the
# running sum but the definition's float `cur - center`: half an ulp of a 0.7 value (3e-8), through the derivative d / sigma_r^2 of the range
# Gaussian's exponent at a difference d of 0.2, is 6e-7 per tap.  The bound is the measured figure with a margin of 4 for the freedom a float32 running
# sum over up to 625 taps has in the order of its additions.  Not derived from any GPU output.
FLOAT_MEASURED = 1.51e-06
FLOAT_BOUND = 4 * FLOAT_MEASURED
# A vote bin is such a float32 running sum of products of three rounded Gaussians; each of the two strongest bins is off by at most FLOAT_BOUND
# relative, so their order can differ from the float64 statement's only when they lie within 2 * FLOAT_BOUND of each other.
VOTE_MARGIN = 2 * FLOAT_BOUND


# ---------------------------------------------------------------------------------------------------------------- the float64 statement
def _g64(sigma, sq):
    s = float(np.float32(sigma))           # the filters take sigma as a float
    return np.exp(-np.asarray(sq, np.float64) / (2.0 * s * s))


def _shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    h, w = a.shape
    b = np.full((h, w), fill, a.dtype)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return b


def ref_bilateral(img, sigma_d, sigma_r):
    a = np.asarray(img, np.float64)
    r = int(math.ceil(2.0 * sigma_d))
    num, den = np.zeros(a.shape), np.zeros(a.shape)
    ok_c = a != -np.inf
    c = np.where(ok_c, a, 0.0)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            t = _shifted(a, dx, dy, -np.inf)
            ok = ok_c & (t != -np.inf)
            v = np.where(ok, t, 0.0)
            wgt = np.where(ok, _g64(sigma_d, dx * dx + dy * dy) * _g64(sigma_r, (v - c) ** 2), 0.0)
            num += wgt * v
            den += wgt
    return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), -np.inf)


def _source_positions(n_out, n_in):
    """Where output index i samples the source, as filter.cu:550-558 types it: float index times float scale (the POSITION is a binary32 quantity by
    definition; everything computed from the samples is binary64 here), and the nearest source index the write is conditional on."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1)
    pos = np.arange(n_out, dtype=np.float32) * scale
    near = (pos + np.float32(0.5)).astype(np.int64)
    return pos.astype(np.float64), near


def ref_resample_float(img, initial):
    a, out = np.asarray(img, np.float64), np.asarray(initial, np.float64).copy()
    ih, iw = a.shape
    oh, ow = out.shape
    fx, nx = _source_positions(ow, iw)
    fy, ny = _source_positions(oh, ih)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    al, be = (fx - x0)[None, :], (fy - y0)[:, None]

    def row(yi):                                   # one source row's blend over the taps that exist and are valid -> (value, took part)
        s, wsum = np.zeros((oh, ow)), np.zeros((oh, ow))
        for xi, wt in ((x0, 1.0 - al), (x0 + 1, al)):
            inside = ((xi >= 0) & (xi < iw))[None, :] & ((yi >= 0) & (yi < ih))[:, None]
            v = a[np.clip(yi, 0, ih - 1)[:, None], np.clip(xi, 0, iw - 1)[None, :]]
            ok = inside & (v != -np.inf)
            s += np.where(ok, wt * np.where(ok, v, 0.0), 0.0)
            wsum += np.where(ok, wt, 0.0)
        took = wsum > 0.0
        return s / np.where(took, wsum, 1.0), took
    p0, t0 = row(y0)
    p1, t1 = row(y0 + 1)
    ss = np.where(t0, (1.0 - be) * p0, 0.0) + np.where(t1, be * p1, 0.0)
    ww = np.where(t0, 1.0 - be, 0.0) + np.where(t1, be, 0.0)
    val = np.where(ww > 0.0, ss / np.where(ww > 0.0, ww, 1.0), -np.inf)
    write = (nx < iw)[None, :] & (ny < ih)[:, None]
    return np.where(write, val, out)


def ref_resample_uchar(img, initial):
    a, out = np.asarray(img), np.asarray(initial).copy()
    _, nx = _source_positions(out.shape[1], a.shape[1])
    _, ny = _source_positions(out.shape[0], a.shape[0])
    write = (nx < a.shape[1])[None, :] & (ny < a.shape[0])[:, None]
    picked = a[np.minimum(ny, a.shape[0] - 1)[:, None], np.minimum(nx, a.shape[1] - 1)[None, :]]
    return np.where(write, picked, out)


def ref_vote(inst, depth, inten, to_idx, to_inst, radius, sigma_d, sigma_r, scale):
    """-> (labels, the strongest bin's vote, the second strongest's) in float64."""
    d, it = np.asarray(depth, np.float64), np.asarray(inten, np.float64)
    h, w = d.shape
    idx = np.asarray(to_idx)[np.asarray(inst)].astype(np.int64)
    votes = np.zeros((h, w, 80))
    yy, xx = np.mgrid[0:h, 0:w]
    inside0 = np.ones((h, w), bool)
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            inside = _shifted(inside0, j, i, False)
            dn, im, b = _shifted(d, j, i, -np.inf), _shifted(it, j, i, 0.0), _shifted(idx, j, i, 255)
            both = (d != -np.inf) & (dn != -np.inf)
            doff = np.where(both, np.abs(np.where(both, d, 0.0) - np.where(both, dn, 0.0)), 0.0)
            io = np.abs(it - im) * float(np.float32(scale))
            wgt = _g64(sigma_d, i * i + j * j) * _g64(sigma_r, doff * doff) * _g64(sigma_r, io * io)
            use = inside & (b < 80)
            votes[yy[use], xx[use], b[use]] += wgt[use]
    order = np.sort(votes, axis=2)
    top, second = order[..., -1], order[..., -2]
    first = np.argmax(votes, axis=2)                                     # the lowest bin among equals, as the strict > of the scan keeps it
    return np.where(top > 0.0, np.asarray(to_inst)[first], 0).astype(np.uint8), top, second


# ---------------------------------------------------------------------------------------------------------------- the checker, as functions
def chk_bilateral(img, sd, sr):
    a = np.ascontiguousarray(img, np.float32)
    out = np.empty_like(a)
    orc.f2d_lib().or_f2d_bilateral(out.ctypes.data, a.ctypes.data, sd, sr, a.shape[1], a.shape[0])
    return out


def _chk_resample(fn, dtype, img, initial):
    a, out = np.ascontiguousarray(img, dtype), np.ascontiguousarray(initial, dtype).copy()
    fn(out.ctypes.data, out.shape[1], out.shape[0], a.ctypes.data, a.shape[1], a.shape[0])
    return out


def chk_resample_float(img, initial):
    return _chk_resample(orc.f2d_lib().or_f2d_resample_float, np.float32, img, initial)


def chk_resample_uchar(img, initial):
    return _chk_resample(orc.f2d_lib().or_f2d_resample_uchar, np.uint8, img, initial)


def chk_vote(inst, depth, inten, to_idx, to_inst, radius, sd, sr, scale):
    i, d, n = np.ascontiguousarray(inst, np.uint8), np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(inten, np.float32)
    out = np.empty_like(i)
    orc.f2d_lib().or_f2d_vote(out.ctypes.data, i.ctypes.data, d.ctypes.data, n.ctypes.data, to_idx.ctypes.data, to_inst.ctypes.data, radius, i.shape[1], i.shape[0],
                              sd, sr, scale)
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rel(a, ref):
    """Largest relative difference of a float map from the float64 statement; -inf must sit exactly where the statement has it."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    hole = ref == -np.inf
    assert np.array_equal(a == -np.inf, hole), "validity differs"
    assert np.isfinite(a[~hole]).all() and (np.abs(ref[~hole]) > 0).all()
    return float((np.abs(a[~hole] - ref[~hole]) / np.abs(ref[~hole])).max()) if (~hole).any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- inputs, shared by both parts
BILATERAL_SIGMAS = ((6.0, 0.1), (2.0, 0.1))


@functools.lru_cache(None)
def _bilateral_images():
    rng = np.random.default_rng(21)

    def noisy(w, h):   # values a few sigma_r apart, so that the range weights differ from tap to tap
        return (0.5 + 0.2 * rng.random((h, w)) + 0.004 * np.arange(w)[None, :]).astype(np.float32)
    yy, xx = np.mgrid[0:33, 0:17]
    skew = (0.4 + 0.011 * xx + 0.0007 * yy * yy + 0.05 * rng.random((33, 17))).astype(np.float32)    # nothing symmetric about it
    holes = noisy(50, 37)
    holes[rng.random((37, 50)) < 0.15] = MINF
    holes[11, :] = MINF                                                                             # one all-invalid row
    holes[20:24, 30:36] = MINF
    cases = {"2x2": noisy(2, 2), "5x7": noisy(5, 7), "16x16": noisy(16, 16), "17x33 skew": skew, "50x37 holes": holes,
             "50x37 all invalid": np.full((37, 50), MINF, np.float32)}
    for a in cases.values():
        a.setflags(write=False)
    return cases


@functools.lru_cache(None)
def _resample_cases():
    """name -> (source float image, source label image, (ow, oh))."""
    rng = np.random.default_rng(22)

    def pair(w, h, holes=0.0):
        f = (1.0 + 0.01 * np.arange(w)[None, :] + 0.02 * np.arange(h)[:, None] + 0.3 * rng.random((h, w))).astype(np.float32)
        if holes:
            f[rng.random((h, w)) < holes] = MINF
        return f, rng.integers(0, 256, (h, w), dtype=np.uint8)
    up = pair(16, 12)
    # 16 x 12 -> 31 x 23 puts every second output row / column exactly between two source rows / columns.  Source rows 2, 6 and 7 are all holes: the
    # vertical blend is left with the upper row only (output rows 3, 11), the lower row only (5, 15), or neither (12, 13; and 4, 14, which sit exactly
    # on a missing row while the row below has weight 0)
    up[0][2, :] = MINF
    up[0][6:8, :] = MINF
    up[0][9, 3:9] = MINF
    up[0][0, 0] = MINF
    cases = {"identity 16x12": (*pair(16, 12, 0.1), (16, 12)), "up 16x12 -> 31x23": (*up, (31, 23)), "down 97x61 -> 32x24": (*pair(97, 61, 0.2), (32, 24)),
             "side of 2: 9x7 -> 2x2": (*pair(9, 7, 0.1), (2, 2)), "side of 2: 2x2 -> 19x18": (*pair(2, 2), (19, 18)),
             "depth 640x480 -> 320x240": (*pair(640, 480, 0.05), (320, 240)), "colour 1296x968 -> 320x240": (*pair(1296, 968, 0.05), (320, 240)),
             "labels 320x240 -> 1296x968": (*pair(320, 240, 0.05), (1296, 968))}
    for f, l, _ in cases.values():
        f.setflags(write=False)
        l.setflags(write=False)
    return cases


def _sentinel(dtype, wh):
    """An output no kernel would produce by accident: a pixel that was skipped keeps it, and nothing else has it."""
    return np.full((wh[1], wh[0]), 173 if dtype == np.uint8 else -12345.0, dtype)


VOTE_PARAMS = ((12, 10.0), (10, 4.0))      # (radius, intensity scale) of the two passes, Filter2dAnnotations.cpp:290-291; sigma_d 5, sigma_r 0.1


@functools.lru_cache(None)
def _vote_scenes():
    """name -> (instance, depth, intensity, to_idx, to_inst, {(y, x): expected output} for pixels with a known answer)."""
    rng = np.random.default_rng(23)
    scenes = {}
    # 40 x 40: all 80 bins in use.  Instance v (1 .. 78) -> bin v, instance 0 -> bin 0, instance 255 -> bin 79; 100 .. 120 have no bin.
    to_idx = np.full(256, 255, np.uint8)
    to_inst = np.zeros(80, np.uint8)
    for b in range(79):
        to_idx[b], to_inst[b] = b, b
    to_idx[255], to_inst[79] = 79, 255
    inst = np.repeat(np.repeat(rng.permutation(100)[:100].reshape(10, 10), 4, 0), 4, 1)
    inst = np.where(inst < 79, inst, np.where(inst < 90, 255, inst + 10)).astype(np.uint8)           # 79 .. 89 -> 255 (bin 79), 90 .. 99 -> 100 .. 109 (no bin)
    speck = rng.random((40, 40)) < 0.1
    inst[speck] = rng.integers(0, 79, speck.sum())
    yy, xx = np.mgrid[0:40, 0:40]
    depth = (1.2 + 0.004 * xx + 0.002 * yy + np.where(xx > 22, 0.15, 0.0) + 0.002 * rng.random((40, 40))).astype(np.float32)
    depth[rng.random((40, 40)) < 0.05] = MINF
    depth[17, 9] = depth[30, 30] = MINF                                                              # centres without depth
    inten = (0.3 + 0.3 * (yy > 18) + 0.05 * rng.random((40, 40))).astype(np.float32)
    assert set(np.unique(to_idx[inst])) >= set(range(80)) and (to_idx[inst] == 255).any() and (inst == 255).any()
    scenes["40x40 all 80 bins"] = (inst, depth, inten, to_idx, to_inst, {})
    # 16 x 16: mapped labels in one corner only; the far corner's window (x, y >= 3 at radius 12, >= 5 at radius 10) holds none -> 0
    inst = np.full((16, 16), 200, np.uint8)
    inst[0:3, 0:3] = rng.integers(1, 5, (3, 3))
    inst[5, 9] = 255
    depth = (2.0 + 0.01 * rng.random((16, 16))).astype(np.float32)
    depth[4, 4] = MINF
    inten = (0.5 + 0.02 * rng.random((16, 16))).astype(np.float32)
    to_idx2 = np.full(256, 255, np.uint8)
    to_inst2 = np.full(80, 255, np.uint8)
    for k, v in enumerate((0, 1, 2, 3, 4)):
        to_idx2[v], to_inst2[k] = k, v
    scenes["16x16 one mapped corner"] = (inst, depth, inten, to_idx2, to_inst2, {(15, 15): 0, (15, 14): 0, (14, 15): 0})
    # 33 x 18: labels and intensity mirrored about column 16.  Column 13 is instance 9 (bin 3), column 19 instance 4 (bin 7), nothing else has a
    # bin: a centre pixel (16, y) gets ONE tap of each bin per row, at -3 and +3, so the two bins accumulate the same float32 numbers in the same
    # order wherever the two range weights are equal.  The depths are dyadic: column 13 at 2.0, column 19 at 2.0625, the centre column at 2.03125 in
    # rows 4, 9, 13 (both differences 0.03125 exactly: a tie, and the lower bin 3 = instance 9 must win although instance 4 is the smaller value)
    # and at 2.0 elsewhere (column 13 wins clearly).  Three tied pixels of 594 stay under the 1 % the float64 comparison may set aside.
    inst = np.full((18, 33), 201, np.uint8)
    inst[:, 13], inst[:, 19] = 9, 4
    half = 0.4 + 0.1 * rng.random((18, 17))
    inten = np.concatenate([half[:, :16], half[:, 16:17], half[:, 15::-1]], axis=1).astype(np.float32)
    depth = np.full((18, 33), 2.0, np.float32)
    depth[:, 19] = 2.0625
    depth[[4, 9, 13], 16] = 2.03125
    depth[6, 2] = MINF
    to_idx3 = np.full(256, 255, np.uint8)
    to_inst3 = np.full(80, 255, np.uint8)
    to_idx3[9], to_inst3[3], to_idx3[4], to_inst3[7] = 3, 9, 7, 4
    assert np.array_equal(inten, inten[:, ::-1])
    scenes["33x18 mirrored tie"] = (inst, depth, inten, to_idx3, to_inst3, {(4, 16): 9, (9, 16): 9, (13, 16): 9, (5, 16): 9, (0, 27): 4})
    for s in scenes.values():
        for a in s[:5]:
            a.setflags(write=False)
    return scenes


@functools.lru_cache(None)
def _chk_vote_cached(name, radius, scale):
    inst, depth, inten, to_idx, to_inst, _ = _vote_scenes()[name]
    out = chk_vote(inst, depth, inten, to_idx, to_inst, radius, 5.0, 0.1, scale)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU: checker vs float64
def test_checker_gaussians_against_float64():
    L = orc.f2d_lib()
    u = 2.0 ** -24      # the argument of exp carries one float rounding (dist * dist, or the float quotient of gaussD), the result another
    for sigma, d in ((0.1, 0.0), (0.1, 0.05), (0.1, 0.3), (0.1, 1.0), (5.0, 7.0)):
        arg = float(np.float32(d)) ** 2 / (2.0 * float(np.float32(sigma)) ** 2)
        assert abs(L.or_f2d_gauss_r(sigma, d) - math.exp(-arg)) <= 1.01 * u * (1 + arg) * math.exp(-arg), (sigma, d)
    for sigma in (2.0, 5.0, 6.0):
        for x, y in ((0, 0), (1, 0), (0, 1), (-12, 12), (3, -7)):
            arg = (x * x + y * y) / (2.0 * sigma * sigma)
            assert abs(L.or_f2d_gauss_d2(sigma, x, y) - math.exp(-arg)) <= 1.01 * u * (1 + arg) * math.exp(-arg), (sigma, x, y)
            assert L.or_f2d_gauss_d2(sigma, x, y) == L.or_f2d_gauss_d2(sigma, y, x)
    assert L.or_f2d_gauss_r(0.1, 0.0) == 1.0 and L.or_f2d_gauss_r(0.1, 65.535) == 0.0 and L.or_f2d_gauss_d2(5.0, 0, 0) == 1.0
    # the array forms are the scalar ones
    d = np.linspace(0, 3, 50, dtype=np.float32)
    out = np.empty_like(d)
    L.or_f2d_gauss_r_n(0.1, d.ctypes.data, out.ctypes.data, d.size)
    assert all(out[i] == L.or_f2d_gauss_r(0.1, float(d[i])) for i in range(d.size))


def test_checker_float_maps_against_float64():
    """Measured here (CPU only): see FLOAT_MEASURED above; the assertion is the bound, the print is the measurement."""
    worst = {}
    for sd, sr in BILATERAL_SIGMAS:
        for name, img in _bilateral_images().items():
            worst["bilateral %s sigma_d %g" % (name, sd)] = _rel(chk_bilateral(img, sd, sr), ref_bilateral(img, sd, sr))
    for name, (f, _, wh) in _resample_cases().items():
        init = _sentinel(np.float32, wh)
        got, ref = chk_resample_float(f, init), ref_resample_float(f, init)
        assert not (ref == init[0, 0]).any(), "every output pixel of these geometries is written"
        worst["resample " + name] = _rel(got, ref)
    for k, v in worst.items():
        print("%-48s %.3g" % (k, v))
    assert max(worst.values()) <= FLOAT_BOUND, max(worst.items(), key=lambda kv: kv[1])


def test_checker_label_resample_against_float64():
    for name, (_, lab, wh) in _resample_cases().items():
        init = _sentinel(np.uint8, wh)
        assert np.array_equal(chk_resample_uchar(lab, init), ref_resample_uchar(lab, init)), name


@pytest.mark.parametrize("radius,scale", VOTE_PARAMS)
def test_checker_vote_against_float64(radius, scale):
    for name, (inst, depth, inten, to_idx, to_inst, known) in _vote_scenes().items():
        got = _chk_vote_cached(name, radius, scale)
        ref, top, second = ref_vote(inst, depth, inten, to_idx, to_inst, radius, 5.0, 0.1, scale)
        close = (top > 0.0) & (top - second <= VOTE_MARGIN * top)
        print("%-28s radius %d: %d of %d pixels set aside, %d labels differ among them" % (name, radius, close.sum(), close.size, (got != ref)[close].sum()))
        assert close.sum() <= 0.01 * close.size, name
        assert np.array_equal(got[~close], ref[~close]), name
        for (y, x), want in known.items():
            assert got[y, x] == want, (name, y, x)
        assert (top > 0.0).any() and (name != "16x16 one mapped corner" or (top == 0.0).any())
        if "tie" in name:
            assert close[[4, 9, 13], 16].all(), "the float64 statement sees the tie as a tie"


# ---------------------------------------------------------------------------------------------------------------- GPU: kernel vs checker, bit for bit
def _gauss_dists():
    rng = np.random.default_rng(24)
    depth = (np.arange(65536, dtype=np.float32) * np.float32(0.001))                                 # every millimetre difference, as metres
    step = np.arange(256, dtype=np.float32) / np.float32(255.0)
    u16 = rng.integers(0, 65536, (2, 1 << 19)).astype(np.float32) * np.float32(0.001)
    formed = np.abs(u16[0] - u16[1])                                                                 # what |dc - d| looks like: differences of two converted depths
    inten = np.abs(rng.random(1 << 19, dtype=np.float32) - rng.random(1 << 19, dtype=np.float32)) * np.where(rng.random(1 << 19) < 0.5, np.float32(4.0), np.float32(10.0))
    return np.concatenate([depth, step * np.float32(4.0), step * np.float32(10.0), formed, inten.astype(np.float32)])


@pytest.mark.gpu
def test_gpu_gaussians_bit_for_bit():
    """gauss_r's three-operation quotient and the LDS exp table against the checker's division and constant table: sigma_r 0.1 over 0 .. 65.535 m in
    millimetres (the exponent runs from 0 through the subnormal results to 0), the intensity steps times both scales, 2^20 random distances; gauss_d2
    at sigma_d 2, 5, 6 over [-12, 12]^2."""
    L = orc.f2d_lib()
    d = _gauss_dists()
    assert d.size == 65536 + 512 + (1 << 20) and np.isfinite(d * d).all()
    want = np.empty_like(d)
    L.or_f2d_gauss_r_n(0.1, d.ctypes.data, want.ctypes.data, d.size)
    got, _ = filter2d.selftest_gauss(0.1, dist=d)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%d of %d differ, first at dist %r: %r != %r" % (bad.size, d.size, d[bad[0]], got[bad[0]], want[bad[0]])
    sub = want[(want > 0) & (want < np.finfo(np.float32).tiny)]
    assert sub.size > 0 and (want == 0).any() and (want == 1).any(), "the sweep reaches the subnormal results and 0"
    dy, dx = [a.ravel().astype(np.int32) for a in np.mgrid[-12:13, -12:13]]
    for sigma in (2.0, 5.0, 6.0):
        want = np.empty(dx.size, np.float32)
        L.or_f2d_gauss_d2_n(sigma, dx.ctypes.data, dy.ctypes.data, want.ctypes.data, dx.size)
        _, got = filter2d.selftest_gauss(sigma, dx=dx, dy=dy)
        assert _same_bits(got, want), sigma
    both = filter2d.selftest_gauss(5.0, dist=d[:700], dx=np.resize(dx, 700), dy=np.resize(dy, 700))          # both groups in one launch, n not a multiple of 256
    L.or_f2d_gauss_r_n(5.0, d.ctypes.data, want.ctypes.data, 625)
    assert _same_bits(both[0][:625], want) and both[1][624] == L.or_f2d_gauss_d2(5.0, 12, 12)


@pytest.mark.gpu
@pytest.mark.parametrize("dwh,cwh", [((13, 11), (31, 17)), ((37, 23), (7, 5)), ((16, 16), (16, 16))])
def test_gpu_prepare_bit_for_bit(dwh, cwh):
    rng = np.random.default_rng(25)
    dn, cn = dwh[0] * dwh[1], cwh[0] * cwh[1]
    depth = rng.integers(0, 65536, dn).astype(np.uint16)
    depth[:6] = (0, 1, 65535, 0, 65535, 1)
    depth[-1] = 0
    rgb = rng.integers(0, 256, (cn, 3), dtype=np.uint8)
    rgb[:3] = ((0, 0, 0), (255, 255, 255), (255, 0, 1))
    d, i = filter2d.stage_prepare(depth, rgb)
    want_d = np.where(depth == 0, MINF, depth.astype(np.float32) * np.float32(0.001)).astype(np.float32)                    # Filter2dAnnotations.cpp:245-256
    c = rgb.astype(np.float32)
    want_i = (np.float32(0.299) * c[:, 0] + np.float32(0.587) * c[:, 1] + np.float32(0.114) * c[:, 2]) * (np.float32(1.0) / np.float32(255.0))   # :232-243
    assert _same_bits(d, want_d) and _same_bits(i, want_i)
    assert d[0] == MINF and d[1] == np.float32(0.001) and d[2] == np.float32(65535) * np.float32(0.001) and i[0] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("sd,sr", BILATERAL_SIGMAS)
def test_gpu_bilateral_bit_for_bit(sd, sr):
    for name, img in _bilateral_images().items():
        got, want = filter2d.stage_bilateral(img, sd, sr), chk_bilateral(img, sd, sr)
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), "%s: %d of %d pixels differ, first at %s" % (name, diff.sum(), diff.size, np.argwhere(diff)[0])
        if name.endswith("all invalid"):
            assert (got == MINF).all()


@pytest.mark.gpu
def test_gpu_resamples_bit_for_bit():
    """Each case twice, over a sentinel and over -inf: a pixel the kernel skipped would keep the one and the other; none may (every output pixel of
    these geometries has a source), and what is written does not depend on what was there."""
    for name, (f, lab, wh) in _resample_cases().items():
        over_sentinel = filter2d.stage_resample_float(f, _sentinel(np.float32, wh))
        assert _same_bits(over_sentinel, chk_resample_float(f, _sentinel(np.float32, wh))), name
        assert not (over_sentinel == -12345.0).any(), name
        assert _same_bits(filter2d.stage_resample_float(f, np.full((wh[1], wh[0]), MINF, np.float32)), over_sentinel), name
        init8 = _sentinel(np.uint8, wh)
        assert _same_bits(filter2d.stage_resample_uchar(lab, init8), chk_resample_uchar(lab, init8)), name
        assert _same_bits(filter2d.stage_resample_uchar(lab, 255 - init8), chk_resample_uchar(lab, init8)), name
    f, lab, _ = _resample_cases()["identity 16x12"]
    assert _same_bits(filter2d.stage_resample_float(f, _sentinel(np.float32, (16, 12))), f)
    assert _same_bits(filter2d.stage_resample_uchar(lab, _sentinel(np.uint8, (16, 12))), lab)


@pytest.mark.gpu
@pytest.mark.parametrize("radius,scale", VOTE_PARAMS)
def test_gpu_vote_bit_for_bit(radius, scale):
    for name, (inst, depth, inten, to_idx, to_inst, known) in _vote_scenes().items():
        got = filter2d.stage_vote(inst, depth, inten, to_idx, to_inst, radius, 5.0, 0.1, scale)
        want = _chk_vote_cached(name, radius, scale)
        assert np.array_equal(got, want), "%s: %d of %d pixels differ, first at %s" % (name, (got != want).sum(), got.size, np.argwhere(got != want)[:1])
        for (y, x), v in known.items():
            assert got[y, x] == v, (name, y, x)
    assert 255 in _chk_vote_cached("40x40 all 80 bins", radius, scale), "bin 79 (instance 255) wins somewhere"


@pytest.mark.gpu
def test_gpu_to_label_bit_for_bit():
    rng = np.random.default_rng(26)
    lut = rng.integers(256, 65536, 256).astype(np.uint16)
    lut[0], lut[255] = 0, 65535
    inst = rng.integers(0, 256, 1000, dtype=np.uint8)
    inst[:2] = (0, 255)
    want = np.empty(1000, np.uint16)
    orc.f2d_lib().or_f2d_to_label(want.ctypes.data, inst.ctypes.data, lut.ctypes.data, 1000, 1)
    assert np.array_equal(filter2d.stage_to_label(inst, lut), want) and np.array_equal(want, lut[inst]) and (want > 255).any()


@pytest.mark.gpu
def test_gpu_hooks_refuse_what_the_frame_path_cannot_launch():
    """Radius 35 is the largest whose table fits the vote kernel's 100 KiB beside the histogram; 36 is an error, not a launch."""
    inst, depth, inten, to_idx, to_inst, _ = _vote_scenes()["16x16 one mapped corner"]
    assert filter2d.MAX_RADIUS == 35
    got = filter2d.stage_vote(inst, depth, inten, to_idx, to_inst, 35, 5.0, 0.1, 4.0)
    assert np.array_equal(got, chk_vote(inst, depth, inten, to_idx, to_inst, 35, 5.0, 0.1, 4.0))
    with pytest.raises(Exception, match="radius"):
        filter2d.stage_vote(inst, depth, inten, to_idx, to_inst, 36, 5.0, 0.1, 4.0)
    with pytest.raises(Exception, match="radius"):
        filter2d.stage_vote(inst, depth, inten, to_idx, to_inst, -1, 5.0, 0.1, 4.0)
    with pytest.raises(Exception, match="radius"):
        filter2d.stage_bilateral(depth, 17.75, 0.1)                                                   # ceil(35.5) = 36
    small = np.ones((2, 1), np.float32)
    with pytest.raises(Exception, match="at least 2"):
        filter2d.stage_resample_float(small, np.zeros((4, 4), np.float32))
