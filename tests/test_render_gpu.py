"""The mesh render on the GPU: k_render against the brute-force checker tests/render_checker.c and against the host path on the float
bits of every pixel, batches against single launches, image sizes that are no multiple of the 8x8 tile, k_render_rays on the rays built from the
tree's boxes, a renderer that changes its mesh, and bin/render on the device against --host."""
import os
import subprocess

import numpy as np
import pytest

from scannet_amd import render
from scannet_amd.segmentator import Mesh
from tests import render_cases as rc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not rc.have_checker(), reason="needs gcc and a CPU with fused multiply-add for tests/render_checker.c")]

DEV = 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "bin", "render")


@pytest.mark.parametrize("name", ["floor", "lattice", "room", "ao", "inside"])
def test_kernel_matches_the_checker_and_the_host_path(name):
    ref, got = rc.checker_images(name), rc.product_images(name, DEV)
    assert np.array_equal(rc.bits(got), rc.bits(ref)), "%d of %d floats differ from the checker" % ((rc.bits(got) != rc.bits(ref)).sum(), ref.size)
    assert np.array_equal(rc.bits(got), rc.bits(rc.product_images(name, -1)))
    if name == "inside":
        assert np.all(got[..., :3] == 0) and np.all(got[..., 3] == 1)


def test_three_cameras_in_one_launch_equal_three_launches():
    c = rc.case("room")
    cams = [render.camera(c["mesh"], c["p"], theta=th) for th in (0.0, 120.0, 240.0)]
    with render.Renderer(c["p"], DEV) as r:
        r.set_mesh(c["mesh"])
        batch = r.run(cams)
        single = np.concatenate([r.run(cam) for cam in cams])
    assert np.array_equal(rc.bits(batch), rc.bits(single))
    assert np.array_equal(rc.bits(batch[:2]), rc.bits(rc.checker_images("room")))
    assert not np.array_equal(batch[1], batch[2])


@pytest.mark.parametrize("size", [(33, 25), (7, 5)])
@pytest.mark.parametrize("samples", [1, 3, 16])
def test_odd_sizes_and_sample_counts(size, samples):
    c = rc.case("lattice")
    p = render.default_params(width=size[0], height=size[1], samples=samples, max_depth=3)
    cam = render.camera(c["mesh"], p, theta=25.0, world_up=(0.1, 0.2, 1.0))
    images = []
    for device in (-1, DEV):
        with render.Renderer(p, device) as r:
            r.set_mesh(c["mesh"])
            images.append(r.run(cam))
    assert images[0].shape == (1, size[1], size[0], 4)
    assert np.array_equal(rc.bits(images[0]), rc.bits(images[1]))
    L, out = rc.checker(), np.zeros((size[1], size[0], 4), np.float32)
    cf = rc.camera_floats(cam)
    L.rk_render(rc._p(c["xyz"]), rc._p(c["rgba"]), len(c["xyz"]), rc._p(c["tris"]), len(c["tris"]), rc._p(cf), size[0], size[1], samples, 3, 0, 0, rc._p(out))
    assert np.array_equal(rc.bits(images[1][0]), rc.bits(out))


def test_ray_batch_kernel_on_the_adversarial_rays():
    c = rc.case("room")
    with render.Renderer(c["p"], DEV) as r:
        r.set_mesh(c["mesh"])
        boxes, _ = r.nodes()
        rays = np.concatenate([rc.box_rays(boxes), rc.hashed_rays(c)])
        got = r.rays(rays)
    ref = rc.checker_rays(c, rays)
    bad = np.flatnonzero((got[0] != ref[0]) | (rc.bits(got[1]) != rc.bits(ref[1])).any(1))
    assert len(bad) == 0, (len(bad), rays[bad[:3]], got[0][bad[:3]], ref[0][bad[:3]])


def test_a_renderer_changes_its_mesh():
    small, big = rc.case("lattice"), rc.case("room")
    p = render.default_params(width=33, height=25, samples=2, max_depth=2, pixel_centre=1)
    assert [getattr(p, k) for k in ("width", "height", "samples", "max_depth", "pixel_centre")] == [getattr(small["p"], k) for k in ("width", "height", "samples", "max_depth", "pixel_centre")]
    with render.Renderer(p, DEV) as r, render.Renderer(p, -1) as h:
        r.set_mesh(small["mesh"])
        first = r.run(small["cameras"][0])
        r.set_mesh(big["mesh"])
        h.set_mesh(big["mesh"])
        cam = render.camera(big["mesh"], p)
        assert np.array_equal(rc.bits(r.run(cam)), rc.bits(h.run(cam)))
        r.set_mesh(small["mesh"])
        again = r.run(small["cameras"][0])
    assert np.array_equal(rc.bits(first), rc.bits(again))
    assert np.array_equal(rc.bits(first), rc.bits(rc.checker_images("lattice")))


def test_tool_on_the_device_writes_the_host_bytes(tmp_path):
    c = rc.case("room")
    ply = str(tmp_path / "room_vh_clean_2.ply")
    c["mesh"].write_ply(ply)
    args = ["--width", "64", "--height", "48", "--samples", "4", "--max-depth", "3", "--theta", "200"]
    outs = []
    for extra in (["--host"], ["--device=%d" % DEV], []):
        out = str(tmp_path / ("out%d.png" % len(outs)))
        r = subprocess.run([TOOL, ply, "-o", out, "--thumb"] + args + extra, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        outs.append(open(out, "rb").read() + open(out[:-4] + "_thumb.png", "rb").read())
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) > 1000
