"""Pins for the CPU TSDF oracle (oracle/tsdf_oracle.c).

The reference holds no TSDF code, tests or golden vectors (SURVEY.md sections 0, 4, 8c: "parity
unpinned"), so the oracle is pinned by analytic known answers on the reference's own conventions:
depth/depthShift (sensorData.h:968-977), K^-1 unprojection without y flip (sensorData.h:1568-1579),
-inf poses skipped (sensorData.h:382) and the zParametersScanNet.txt:34-35,47-53 constants.
"""
import os

import numpy as np
import pytest

from scannet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x):
    return np.float32(x)


def test_depth_prepass(oracle):
    p = oracle.default_params(8, 2)
    d = np.array([[0, 50, 99, 100, 101, 2000, 6000, 6001], [7000, 65535, 1, 1234, 4000, 4001, 3999, 100]], np.uint16)
    out = oracle.depth_to_float(p, d)
    exp = d.astype(np.float32) / np.float32(1000.0)
    bad = (d == 0) | (exp < np.float32(0.1)) | (exp > np.float32(6.0))
    assert np.array_equal(np.isneginf(out), bad)
    assert np.array_equal(out[~bad], exp[~bad])
    assert out[0, 5] == np.float32(2.0)


@pytest.fixture(scope="module")
def plane_volume(oracle):
    p = oracle.default_params()
    vol = oracle.Volume(p, threads=8)
    n = vol.integrate(synth.plane_frame(), np.eye(4, dtype=np.float32))
    return p, vol, n


def test_plane_known_answer(oracle, plane_volume):
    p, vol, n = plane_volume
    coords, vox = vol.export()
    # SURVEY 8d worked example: ~26k blocks for the 2 m plane at 4 mm
    assert 20000 < vol.num_blocks < 34000
    assert n == vol.num_blocks  # everything allocated by this frame is in its frustum
    voxel = f32(0.004)
    t = np.float32(np.float32(0.02) * np.float32(2.0) + np.float32(0.06))
    # z range of allocated blocks covers [2 - t, 2 + t]
    zmin = (coords[:, 2].min() * 8) * 0.004
    zmax = (coords[:, 2].max() * 8 + 7) * 0.004
    assert zmin <= 2.0 - float(t) + 0.004 and zmax >= 2.0 + float(t) - 0.004
    assert zmin > 2.0 - float(t) - 0.04 and zmax < 2.0 + float(t) + 0.04
    # analytic voxel values: identity pose => pc = voxel centre exactly, d = 2.0 exactly
    l = np.arange(8)
    gz = (coords[:, 2, None] * 8 + l[None, :]).astype(np.float32) * voxel  # [n,8]
    gy = (coords[:, 1, None] * 8 + l[None, :]).astype(np.float32) * voxel
    gx = (coords[:, 0, None] * 8 + l[None, :]).astype(np.float32) * voxel
    Z = np.broadcast_to(gz[:, :, None, None], (len(coords), 8, 8, 8)).reshape(len(coords), 512)
    Y = np.broadcast_to(gy[:, None, :, None], (len(coords), 8, 8, 8)).reshape(len(coords), 512)
    X = np.broadcast_to(gx[:, None, None, :], (len(coords), 8, 8, 8)).reshape(len(coords), 512)
    fx, fy, mx, my = (f32(v) for v in synth.intrinsics())
    with np.errstate(divide="ignore", invalid="ignore"):
        rz = f32(1.0) / Z
        # fmaf(pc.x*fx, rz, mx): emulate the fused op in float64 (exact product of two f32 fits in f64)
        u = ((X * fx).astype(np.float64) * rz.astype(np.float64) + np.float64(mx)).astype(np.float32) + f32(0.5)
        v = ((Y * fy).astype(np.float64) * rz.astype(np.float64) + np.float64(my)).astype(np.float32) + f32(0.5)
    # pixel = (int)(... + 0.5f), then the image test: a C cast truncates towards zero, so (-1, 0) is pixel 0
    inside = (Z > 0) & (u > -1) & (u < 640) & (v > -1) & (v < 480)
    sdf = f32(2.0) - Z
    upd = inside & (sdf > -t)
    exp = np.where(upd, np.minimum(sdf, t), f32(0)).astype(np.float32)
    assert np.array_equal(vox["w"], upd.astype(np.uint8))
    assert np.array_equal(vox["sdf"], exp)
    assert upd.sum() > 5_000_000


def test_running_mean_and_deintegrate(oracle):
    p = oracle.default_params()
    vol = oracle.Volume(p, threads=8)
    I = np.eye(4, dtype=np.float32)
    a, b = synth.plane_frame(depth_mm=2000), synth.plane_frame(depth_mm=2010)
    vol.integrate(a, I)
    c1, v1 = vol.export()
    vol.integrate(b, I)
    c2, v2 = vol.export()
    assert v2["w"].max() == 2
    # blocks of frame a keep their identity; weights add up where both frames touch
    both = (v2["w"] == 2)
    assert both.sum() > 1_000_000
    vol.deintegrate(b, I)
    c3, v3 = vol.export()
    assert np.array_equal(c2, c3)
    # after removing b the voxels touched by a are back to a's values (weights exact, sdf <= 1e-5)
    idx = {tuple(c): i for i, c in enumerate(c3)}
    sel = np.array([idx[tuple(c)] for c in c1])
    assert np.array_equal(v3["w"][sel], v1["w"])
    assert np.abs(v3["sdf"][sel] - v1["sdf"]).max() <= 1e-5
    # voxels only b touched are reset to zero
    rest = np.ones(len(c3), bool)
    rest[sel] = False
    assert (v3["w"][rest] == 0).all() and (v3["sdf"][rest] == 0).all()
    vol.deintegrate(a, I)
    _, v4 = vol.export()
    assert (v4["w"] == 0).all() and (v4["sdf"] == 0).all()
    # everything is now empty => GC frees every block
    assert vol.garbage_collect() == len(c3)
    assert vol.num_blocks == 0


def test_weight_saturates_and_invalid_pose(oracle):
    p = oracle.default_params(160, 120)
    p.fx = p.fy = 577.87 / 4
    p.weight_max = 3
    vol = oracle.Volume(p)
    I = np.eye(4, dtype=np.float32)
    d = synth.plane_frame(160, 120, 1500)
    for _ in range(5):
        vol.integrate(d, I)
    _, v = vol.export()
    assert v["w"].max() == 3
    n = vol.num_blocks
    bad = np.full((4, 4), -np.inf, np.float32)
    assert vol.integrate(d, bad) == -1
    assert vol.num_blocks == n


def test_colour_average(oracle):
    p = oracle.default_params(160, 120)
    p.fx = p.fy = 577.87 / 4
    vol = oracle.Volume(p)
    I = np.eye(4, dtype=np.float32)
    d = synth.plane_frame(160, 120, 1500)
    c0 = np.full((120, 160, 3), (10, 200, 31), np.uint8)
    c1 = np.full((120, 160, 3), (21, 100, 30), np.uint8)
    vol.integrate(d, I, rgb=c0)
    vol.integrate(d, I, rgb=c1)
    _, v = vol.export()
    m = v["w"] == 2
    assert m.any()
    # (v.color + c) / 2 per channel, integer division: (10 + 21) / 2 = 15, (31 + 30) / 2 = 30
    assert (v["r"][m] == 15).all() and (v["g"][m] == 150).all() and (v["b"][m] == 30).all()


def test_room_mesh_on_walls(oracle):
    """Marching cubes on a few frames of the config-2 room: vertices lie on the room's planes."""
    W, H = 160, 120
    p = oracle.default_params(W, H, voxel=0.02)
    p.fx = p.fy = 577.87 / 4
    vol = oracle.Volume(p, threads=8)
    for depth, pose in synth.room_stream(6, total_frames=60, width=W, height=H):
        assert vol.integrate(depth, pose) > 0
    m = vol.extract_mesh()
    pos, idx = m["pos"], m["idx"]
    assert len(pos) > 1000 and len(idx) > 1000
    assert np.all(np.diff(m["keys"].astype(np.int64)) > 0)  # canonical order, welded
    rx, ry, rz = synth.ROOM
    dist = np.min(np.abs(np.stack([pos[:, 0], pos[:, 0] - rx, pos[:, 1], pos[:, 1] - ry, pos[:, 2], pos[:, 2] - rz])), 0)
    # depth is quantised to mm and sampled at the nearest pixel: a few mm of error at grazing angles
    assert np.percentile(dist, 99) < 0.02
    assert idx.min() >= 0 and idx.max() < len(pos)
    # every edge is shared by at most two triangles (manifold) and interior edges appear in opposite directions
    e = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]])
    fw = set(map(tuple, e))
    assert len(fw) == len(e)  # no directed edge twice => consistent orientation


def test_plane_mesh_known_answer(oracle, plane_volume):
    p, vol, _ = plane_volume
    m = vol.extract_mesh()
    pos, idx = m["pos"], m["idx"]
    assert len(pos) > 100000
    assert np.abs(pos[:, 2] - 2.0).max() < 1e-6
    # normals point from inside (behind the surface) to outside (towards the camera): -z
    a, b, c = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
    n = np.cross(b - a, c - a)
    assert (n[:, 2] <= 0).all() and (n[:, 2] < 0).sum() > 0.9 * len(idx)


def _golden():
    import importlib.util
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_tsdf_golden", os.path.join(here, "make_tsdf_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, json.load(open(os.path.join(here, "tsdf_golden.json")))


@pytest.mark.parametrize("case", [0, 1, 2, 3, 4, 5])
def test_oracle_matches_committed_digests(oracle, case):
    """tests/golden/tsdf_golden.json freezes the oracle's output (voxels + canonical mesh) on small seeded scenarios."""
    mod, gold = _golden()
    name, size, voxel, idx, colour, deint, opts = mod.SCENARIOS[case]

    def factory(W, H, vx, **switches):
        p = oracle.default_params(W, H, vx)
        p.fx, p.fy, p.mx, p.my = synth.intrinsics(W, H)
        for k, v in switches.items():
            setattr(p, k, v)
        vol = oracle.Volume(p, threads=4)
        raw = vol.extract_mesh

        def extract():
            m = raw()
            return m["pos"], m["col"], m["idx"].astype(np.int32), m["keys"]
        vol.extract_mesh = extract
        return vol

    assert mod.run(factory, name, size, voxel, idx, colour, deint, opts) == gold[name]


def _births(volume_after_each_frame_coords):
    """coords exported after every frame -> (final coords, first frame index at which each block exists)."""
    final = volume_after_each_frame_coords[-1]
    key = lambda c: (c[:, 0].astype(np.int64) << 42) | ((c[:, 1].astype(np.int64) & 0x1FFFFF) << 21) | (c[:, 2].astype(np.int64) & 0x1FFFFF)
    kf = key(final)
    birth = np.full(len(final), len(volume_after_each_frame_coords), np.int64)
    for k in range(len(volume_after_each_frame_coords) - 1, -1, -1):
        birth[np.isin(kf, key(volume_after_each_frame_coords[k]))] = k
    return final, birth


def spec_literal_check(frames, coords, birth, vox, params, sample=None, seed=0):
    """The fp32 volume `vox` (VOXEL_DTYPE [n,512]) against the float64 literal evaluation of SURVEY App. C (oracle/spec_literal.py).
    Returns a dict of what was measured; asserts the north-star tolerance (1e-4 m on TSDF values) and weight equality away from ties."""
    from oracle import spec_literal
    if sample is not None and sample < len(coords):
        pick = np.sort(np.random.default_rng(seed).choice(len(coords), sample, replace=False))
        coords, birth, vox = coords[pick], birth[pick], vox[pick]
    sdf, w, tie = spec_literal.evaluate(frames, coords, birth, **params)
    ok = ~tie
    wrong_w = ok & (w != vox["w"])
    seen = ok & (w > 0)
    err = np.abs(sdf - vox["sdf"].astype(np.float64))
    out = {"voxels": int(ok.size), "ties": int(tie.sum()), "tie_frac": float(tie.mean()), "observed": int(seen.sum()),
           "weight_mismatches": int(wrong_w.sum()), "max_abs_sdf_err_m": float(err[seen].max()) if seen.any() else 0.0,
           "mean_abs_sdf_err_m": float(err[seen].mean()) if seen.any() else 0.0}
    assert out["observed"] > 0.2 * ok.sum(), out
    eps_px = 1e-6 * max(params["width"], params["height"])
    assert out["tie_frac"] < 6 * eps_px * len(frames) + 0.002, out   # discontinuities within rounding distance of their threshold are rare ...
    assert out["weight_mismatches"] == 0, out              # ... and away from them every voxel saw exactly the same frames
    assert out["max_abs_sdf_err_m"] < 1e-4, out            # the north-star tolerance; fp32 lands around 1e-6
    # inside the tie set the two may differ by whole observations -- but only there; count them for the record
    out["tie_weight_mismatches"] = int((tie & (w != vox["w"])).sum())
    return out


def test_oracle_within_tolerance_of_the_literal_specification(oracle):
    """The fp32 oracle (fused multiply-adds, reciprocal projection: DESIGN.md 3.5 -- the forms the HIP kernel shares) against the float64,
    division-form, statement-by-statement evaluation of SURVEY App. C: equal weights away from pixel-rounding / threshold ties, TSDF values
    within 1e-4 m.  The same check runs on the HIP volume at 640x480 in tests/test_gpu_tsdf.py."""
    W, H = 160, 120
    p = oracle.default_params(W, H, voxel=0.008)
    fx, fy, mx, my = synth.intrinsics(W, H)
    p.fx, p.fy, p.mx, p.my = fx, fy, mx, my
    vol = oracle.Volume(p, threads=8)
    frames, after = [], []
    for i in (0, 1, 2, 150, 151, 300):
        pose = synth.trajectory_pose(i, 1200)
        d = synth.render_room_depth(pose, W, H, noise_frame=i)
        vol.integrate(d, pose)
        frames.append((d, pose))
        after.append(vol.export()[0])
    coords, vox = vol.export()
    final, birth = _births(after)
    assert np.array_equal(final, coords)
    res = spec_literal_check(frames, coords, birth, vox, dict(voxel=0.008, fx=fx, fy=fy, mx=mx, my=my, width=W, height=H), sample=6000)
    assert res["max_abs_sdf_err_m"] < 2e-5


def _mc_table_counts():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "mc_tables.h")).read()
    body = re.search(r"MC_NUM_TRIS[^=]*=\s*\{(.*?)\};", text, re.S).group(1)
    return np.array([int(x) for x in re.findall(r"\d+", body)])


def spec_literal_mc_check(coords, vox, mesh, voxel, thresh_factor=10.0):
    """A canonical mesh (dict with keys / pos / col / idx) against the independent float64 marching cubes of oracle/spec_literal_mc.py over
    the same volume: the same vertices (grid edges), positions within 1e-6 m, colours within one level (round-half-up of a float32 against
    a float64 interpolation), the same number of triangles."""
    from oracle import spec_literal_mc
    ref = spec_literal_mc.evaluate(coords, vox, voxel, thresh_factor, _mc_table_counts())
    assert len(ref["keys"]) > 0 and np.array_equal(ref["keys"], mesh["keys"]), (len(ref["keys"]), len(mesh["keys"]))
    assert np.abs(ref["pos"] - mesh["pos"].astype(np.float64)).max() < 1e-6
    want = np.floor(ref["col"] + 0.5)
    assert np.abs(want - mesh["col"].astype(np.float64)).max() <= 1.0
    assert (want == mesh["col"]).mean() > 0.999
    assert ref["n_tris"] == len(mesh["idx"])
    return dict(vertices=len(ref["keys"]), triangles=ref["n_tris"], max_pos_err=float(np.abs(ref["pos"] - mesh["pos"]).max()))


def test_oracle_mesh_matches_the_literal_marching_cubes(oracle):
    """The restated marching cubes (mc_oracle.c; the HIP mesh is byte-identical to it, tests/test_gpu_tsdf.py) against an independent float64
    evaluation of DESIGN.md 3.7 on a coloured, noisy room volume: vertex set, positions, colours, triangle count."""
    W, H = 160, 120
    p = oracle.default_params(W, H, voxel=0.02)
    p.fx = p.fy = 577.87 / 4
    vol = oracle.Volume(p, threads=8)
    rng = np.random.default_rng(3)
    for i, (depth, pose) in enumerate(synth.room_stream(8, total_frames=60, width=W, height=H)):
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert vol.integrate(depth, pose, rgb) > 0
    coords, vox = vol.export()
    res = spec_literal_mc_check(coords, vox, vol.extract_mesh(), 0.02)
    assert res["vertices"] > 3000 and res["triangles"] > 5000, res


# ---------------------------------------------------------------------------------------------------------------------------------------
# upstream-conformance switches (include/scanfuse.h sf_params::frustum_mode / colour_round / colour_first / weight_mode)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _small(oracle, **over):
    p = oracle.default_params(160, 120)
    p.fx = p.fy = 577.87 / 4
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_colour_round_half_up_is_the_float_formula_upstream_writes():
    """colour_round 1 is stated upstream as (uchar)(0.5f * c0 + 0.5f * c1 + 0.5f); the kernels compute (a + b + 1) >> 1 on packed bytes.  All
    65 536 byte pairs: the float expression, the integer one and the packed-word one ((a & b) + ((a ^ b) >> 1) + ((a ^ b) & 1)) agree."""
    a, b = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32))
    f = (np.float32(0.5) * a.astype(np.float32) + np.float32(0.5) * b.astype(np.float32) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(f, ((a + b + 1) >> 1).astype(np.uint8))
    x = a ^ b
    assert np.array_equal(f, ((a & b) + ((x & 0xFE) >> 1) + (x & 1)).astype(np.uint8))
    assert np.array_equal(((a + b) // 2).astype(np.uint8), ((a & b) + ((x & 0xFE) >> 1)).astype(np.uint8))   # colour_round 0


def test_colour_switches(oracle):
    I = np.eye(4, dtype=np.float32)
    d = synth.plane_frame(160, 120, 1500)
    c0 = np.full((120, 160, 3), (10, 200, 31), np.uint8)
    c1 = np.full((120, 160, 3), (21, 100, 30), np.uint8)
    black = np.zeros((120, 160, 3), np.uint8)
    vol = oracle.Volume(_small(oracle, colour_round=1))
    vol.integrate(d, I, rgb=c0)
    vol.integrate(d, I, rgb=c1)
    _, v = vol.export()
    m = v["w"] == 2
    assert m.any() and (v["r"][m] == 16).all() and (v["g"][m] == 150).all() and (v["b"][m] == 31).all()   # (10 + 21 + 1) >> 1, (31 + 30 + 1) >> 1
    # colour_first: a black accumulated colour is "no colour yet" upstream -- black, then c1: weight rule averages, colour rule copies
    for first, want in ((0, (10, 50, 15)), (1, (21, 100, 30))):
        vol = oracle.Volume(_small(oracle, colour_first=first))
        vol.integrate(d, I, rgb=black)
        vol.integrate(d, I, rgb=c1)
        _, v = vol.export()
        m = v["w"] == 2
        assert m.any() and (v["r"][m] == want[0]).all() and (v["g"][m] == want[1]).all() and (v["b"][m] == want[2]).all(), first


def test_depth_dependent_weight(oracle):
    """weight_mode 1 (VoxelHashing): (uchar)max(ws * 1.5 * (1 - (d - dmin) / (dmax - dmin)), 1).  ws = 10 at d = 1.5 m: 15 * (1 - 1.4 / 5.9) =
    11.44 -> 11; at 5 m (beyond the integration distance nothing is fused) -- and with the SHIPPED ws = 1 the rule gives 1 at every depth."""
    I = np.eye(4, dtype=np.float32)
    for ws, mm, want in ((10, 1500, 11), (10, 3900, 5), (1, 500, 1), (1, 3900, 1), (4, 200, 5)):
        vol = oracle.Volume(_small(oracle, weight_mode=1, weight_sample=ws))
        vol.integrate(synth.plane_frame(160, 120, mm), I)
        _, v = vol.export()
        z01 = (np.float32(mm) / np.float32(1000) - np.float32(0.1)) / (np.float32(6.0) - np.float32(0.1))
        assert want == int(max(np.float32(ws) * np.float32(1.5) * (np.float32(1) - z01), np.float32(1)))
        assert set(np.unique(v["w"])) == {0, want}, (ws, mm, np.unique(v["w"]))
    # integrate then deintegrate with the same weights empties the volume
    vol = oracle.Volume(_small(oracle, weight_mode=1, weight_sample=10))
    a = synth.plane_frame(160, 120, 1500)
    vol.integrate(a, I)
    vol.deintegrate(a, I)
    _, v = vol.export()
    assert (v["w"] == 0).all() and (v["sdf"] == 0).all()


def test_block_centre_frustum(oracle):
    """frustum_mode 1: the allocated set is the sphere-mode set restricted to the blocks whose CENTRE projects inside 0.95 x NDC, and border
    blocks the sphere test keeps are dropped -- checked against the float64 statement in oracle/spec_literal.py away from ties."""
    from oracle import spec_literal
    W, H = 160, 120
    fx, fy, mx, my = synth.intrinsics(W, H)
    pose = synth.trajectory_pose(7, 400)
    d = synth.render_room_depth(pose, W, H, noise_frame=7)
    sets = []
    for mode in (0, 1):
        p = oracle.default_params(W, H, voxel=0.01)
        p.fx, p.fy, p.mx, p.my = fx, fy, mx, my
        p.frustum_mode = mode
        vol = oracle.Volume(p, threads=4)
        n = vol.integrate(d, pose)
        assert n == vol.num_blocks
        sets.append(vol.export())
    (c0, v0), (c1, v1) = sets
    k = lambda c: {tuple(r) for r in c}
    assert k(c1) < k(c0) and 0.9 * len(c0) < len(c1) < len(c0), (len(c0), len(c1))   # the rays stay inside the image: only the 2.5 % border ring goes
    inside, near = spec_literal.centre_in_frustum(c0, np.linalg.inv(pose.astype(np.float64)), voxel=0.01, fx=fx, fy=fy, mx=mx, my=my, width=W, height=H,
                                                  dmin=0.1, dmax=6.0)
    want = {tuple(r) for r in c0[inside & ~near]}
    maybe = {tuple(r) for r in c0[near]}
    assert want <= k(c1) <= (want | maybe) and len(maybe) < 0.01 * len(c0)
    # the voxels of a block both modes hold are the same voxels
    idx0 = {tuple(r): i for i, r in enumerate(c0)}
    sel = np.array([idx0[tuple(r)] for r in c1])
    assert np.array_equal(v0[sel].view(np.uint8), v1.view(np.uint8))


def test_switched_semantics_within_tolerance_of_the_literal_specification(oracle):
    """The float64 literal evaluator with the same switches (block-centre frustum, depth-dependent weight at VoxelHashing's own ws = 10)."""
    W, H = 160, 120
    p = oracle.default_params(W, H, voxel=0.008)
    fx, fy, mx, my = synth.intrinsics(W, H)
    p.fx, p.fy, p.mx, p.my = fx, fy, mx, my
    p.frustum_mode, p.weight_mode, p.weight_sample = 1, 1, 10
    vol = oracle.Volume(p, threads=8)
    frames, after = [], []
    for i in (0, 1, 2, 150, 151, 300):
        pose = synth.trajectory_pose(i, 1200)
        d = synth.render_room_depth(pose, W, H, noise_frame=i)
        vol.integrate(d, pose)
        frames.append((d, pose))
        after.append(vol.export()[0])
    coords, vox = vol.export()
    final, birth = _births(after)
    assert np.array_equal(final, coords)
    res = spec_literal_check(frames, coords, birth, vox, dict(voxel=0.008, fx=fx, fy=fy, mx=mx, my=my, width=W, height=H, frustum_mode=1, weight_mode=1,
                                                             weight_sample=10), sample=6000)
    assert res["max_abs_sdf_err_m"] < 2e-5
    assert vox["w"].max() > 20   # several observations of weight > 1 each


def test_weight_wrap(oracle):
    """weight_wrap 1 (upstream's `uchar weight` with the shipped s_SDFIntegrationWeightMax = 99999999): the 256th observation wraps the weight
    to 0 and the mean restarts -- 256 observations of a plane at 1500 mm, then 44 of one at 1510 mm: the weight reads 44 and the sdf is the mean
    of the last 44 observations only (the first 256 are forgotten); the saturating default keeps 255 and the long memory."""
    I = np.eye(4, dtype=np.float32)
    a, b = synth.plane_frame(160, 120, 1500), synth.plane_frame(160, 120, 1510)
    vol = oracle.Volume(_small(oracle, weight_wrap=1, weight_max=99999999))
    sat = oracle.Volume(_small(oracle, weight_max=99999999))
    for i in range(300):
        d = a if i < 256 else b
        vol.integrate(d, I)
        sat.integrate(d, I)
    _, v = vol.export()
    _, s = sat.export()
    assert v["w"].max() == 44 and s["w"].max() == 255
    # voxels observed by all 300 frames: the wrapped volume holds exactly plane b's values (as if fused 44 times from empty), the saturated one does not
    ref = oracle.Volume(_small(oracle))
    for i in range(44):
        ref.integrate(b, I)
    rc, rv = ref.export()
    vc, _ = vol.export()
    idx = {tuple(c): i for i, c in enumerate(vc)}
    sel = np.array([idx[tuple(c)] for c in rc])
    full = (rv["w"] == 44) & (v["w"][sel] == 44)
    assert full.sum() > 10000
    assert np.abs(v["sdf"][sel][full] - rv["sdf"][full]).max() < 1e-6


@pytest.mark.parametrize("colour_round,colour_first", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_colour_rule_against_the_literal_evaluation(oracle, colour_round, colour_first):
    """The colour half of the voxel update against the literal evaluator (integers: no tolerance), in all four switch positions, on frames with
    random colours and a black band; voxels whose geometry sits on a decision boundary (the evaluator's `tie`) are left out."""
    from oracle import spec_literal
    W, H = 160, 120
    p = oracle.default_params(W, H, voxel=0.01)
    fx, fy, mx, my = synth.intrinsics(W, H)
    p.fx, p.fy, p.mx, p.my = fx, fy, mx, my
    p.colour_round, p.colour_first = colour_round, colour_first
    vol = oracle.Volume(p, threads=8)
    rng = np.random.default_rng(17)
    frames, after = [], []
    for i in (0, 1, 2, 3, 40, 41, 42, 2):
        pose = synth.trajectory_pose(i, 400)
        d = synth.render_room_depth(pose, W, H, noise_frame=i)
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rgb[:, : W // 3] = 0
        vol.integrate(d, pose, rgb=rgb)
        frames.append((d, pose, rgb))
        after.append(vol.export()[0])
    coords, vox = vol.export()
    final, birth = _births(after)
    assert np.array_equal(final, coords)
    pick = np.sort(np.random.default_rng(1).choice(len(coords), 4000, replace=False))
    sdf, w, tie, col = spec_literal.evaluate(frames, coords[pick], birth[pick], voxel=0.01, fx=fx, fy=fy, mx=mx, my=my, width=W, height=H,
                                             colour_round=colour_round, colour_first=colour_first, return_colour=True)
    ok = ~tie & (w > 0)
    assert ok.sum() > 100000 and np.array_equal(w[ok], vox["w"][pick][ok])
    got = np.stack([vox["r"][pick], vox["g"][pick], vox["b"][pick]], -1).astype(np.int64)
    assert np.array_equal(got[ok], col[ok])
    assert (w[ok] >= 3).sum() > 10000          # several blends per voxel, so the rounding direction matters


def test_reference_unprojection_form_against_the_ray_slope_form(oracle):
    """SURVEY 8a row a6 pinned to IN-TREE code: the reference unprojects a depth pixel as K^-1 . (x d, y d, d) (filter.cu:74-91 on the float4x4
    class of cuda_SimpleMatrixUtil.h -- compiled from /root/reference into oracle/_ref/libref_unproject.so); the fusion kernels and
    oracle/tsdf_oracle.c use the ray-slope form ((x - mx) / fx) d, ((y - my) / fy) d, d (one division per column / row, tabulated).  Same
    convention (pixel centres at integers, no y flip, z = the depth itself), and over EVERY pixel of a 640x480 image and the sensor's depth range
    the two differ by rounding only: bounded here far inside the 1e-4 m of the north star."""
    if not oracle.ref_unproject_available():
        pytest.skip("oracle/_ref/libref_unproject.so not built (needs /root/reference)")
    W, H = 640, 480
    fx, fy, mx, my = (np.float32(v) for v in synth.intrinsics(W, H))
    K = np.array([[fx, 0, mx, 0], [0, fy, my, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    inv = oracle.ref_intrinsics_inverse(K)
    assert inv[2].tolist() == [0, 0, 1, 0] and inv[3].tolist() == [0, 0, 0, 1] and inv[0, 1] == 0 and inv[1, 0] == 0
    assert abs(float(inv[0, 0]) * float(fx) - 1) < 1e-6 and abs(float(inv[0, 2]) + float(mx) / float(fx)) < 1e-6
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    kx, ky = (xs - mx) / fx, (ys - my) / fy          # csrc/fuser_prepass.hip k_ray_tables / fuser_alloc.hip k_alloc: true float32 divisions
    worst, worst_rel = 0.0, 0.0
    rng = np.random.default_rng(4)
    depths = [0.1, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 3.999, 4.0, 5.0, 6.0] + list(rng.uniform(0.1, 6.0, 9))
    for dval in depths:
        d = np.full((H, W), np.float32(dval), np.float32)
        d[0, 0] = -np.inf
        ref = oracle.ref_unproject(K, d)
        ours = np.stack([kx * d, ky * d, d], -1).astype(np.float32)
        assert np.all(np.isneginf(ref[0, 0])), "an invalid pixel stays invalid (filter.cu:83)"
        assert np.array_equal(ref[..., 2][1:], d[1:]), "camera-space z is the depth itself"
        diff = np.abs(ref[1:].astype(np.float64) - ours[1:].astype(np.float64))
        worst = max(worst, float(diff.max()))
        worst_rel = max(worst_rel, float((diff[..., :2] / np.float64(dval)).max()))
    # conventions: +x to the right of the principal point, +y BELOW it (no flip), both forms
    d = np.full((H, W), np.float32(2.0), np.float32)
    ref = oracle.ref_unproject(K, d)
    assert ref[300, 500, 0] > 0 and ref[300, 500, 1] > 0 and ref[100, 100, 0] < 0 and ref[100, 100, 1] < 0
    assert worst < 2e-6 and worst_rel < 5e-7, (worst, worst_rel)   # metres; measured 7.2e-7 m, 1.9e-7 of the depth
    print("a6: max |K^-1 form - ray-slope form| = %.3g m, %.3g of the depth" % (worst, worst_rel))


def test_conformance_packet_is_reproducible(oracle):
    """conformance/digests.json (tools/conformance_packet.py; INTEGRATION.md "Conformance packet"): the packet's input is closed-form, so its
    first frames and the oracle's volume / mesh after the 40-frame walk come out again, here for the two presets (SURVEY App. C = 00000, the
    VoxelHashing preset = 11111); all 32 combinations on all 300 frames are reproduced by the HIP path in tests/test_gpu_tsdf.py."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("conformance_packet", os.path.join(ROOT, "tools", "conformance_packet.py"))
    cp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cp)
    want = json.load(open(os.path.join(ROOT, "conformance", "digests.json")))
    assert want["switch_order"] == list(cp.SWITCHES) and len(want["combinations"]) == 32
    assert len({v["full"]["mesh_sha256"] for v in want["combinations"].values()}) == 32, "every switch must be observable on the packet's scan"
    fr = cp.frames("walk")
    for name in ("00000", "11111"):
        sw = dict(zip(cp.SWITCHES, (int(c) for c in name)))
        got = cp.run_oracle(oracle, fr, sw, threads=8)
        assert got["walk"] == want["combinations"][name]["walk"], name
