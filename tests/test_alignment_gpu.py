"""The kernels of the axis alignment (scannet_amd/csrc/axis_align.hip), each alone at the smallest shapes at which it can go wrong,
bitwise against tests/axis_align_checker.c; then the estimate and bin/alignment --gpu against the host path."""
import shutil
import subprocess

import numpy as np
import pytest

from scannet_amd import alignment
from scannet_amd.segmentator import Mesh
from tests import alignment_cases as ac

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ac.have_gcc(), reason="needs gcc for tests/axis_align_checker.c")]

DEV = 0


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return ac.Checker(tmp_path_factory.mktemp("aac"))


@pytest.fixture(scope="module")
def clutter_points(checker):
    """the "clutter" case as the clustering sees it: positions and the checker's normals"""
    xyz, tris = ac.clutter()
    return xyz, checker.normals(xyz, tris)


@pytest.fixture()
def default_batch():
    yield
    ac.tune_batch(1024)


def test_normals_high_valence_unreferenced_and_odd_count(checker):
    """about 2 k faces: a 30 x 30 grid, a fan of 80 faces round one hub (valence above 64: the lane's walk is longer than a wave is wide), one vertex
    no face names (it keeps (0, 0, 0)); 1043 vertices, no multiple of 64"""
    rng = np.random.default_rng(1)
    gx, gt = ac.grid((0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), 30, 30)
    gx[:, 2] = rng.uniform(-0.02, 0.02, len(gx))
    ang = np.linspace(0, 2 * np.pi, 80, endpoint=False)
    rim = np.stack([5 + np.cos(ang), np.sin(ang), rng.uniform(-0.1, 0.1, 80)], -1)
    fan = np.array([[0, 1 + i, 1 + (i + 1) % 80] for i in range(80)])
    xyz, tris = ac.join([(gx, gt), (np.concatenate([[[5.0, 0, 0.3]], rim]), fan), (np.array([[9.0, 9, 9]]), np.zeros((0, 3), int))])
    xyz = np.ascontiguousarray(xyz.astype(np.float32))
    assert len(tris) == 1880 and len(xyz) == 1043 and len(xyz) % 64 != 0
    assert np.bincount(tris.ravel(), minlength=len(xyz)).max() == 80
    got, want = ac.stage_normals(xyz, tris, DEV), checker.normals(xyz, tris)
    assert np.array_equal(ac.bits(got), ac.bits(want))
    assert np.all(got[-1] == 0) and np.abs(np.linalg.norm(got[:-1], axis=1) - 1).max() < 1e-5


@pytest.mark.parametrize("batch", [256, 1024])
def test_clustering_partial_last_batch_and_founders_inside_a_batch(checker, clutter_points, default_batch, batch):
    """2 * 256 + 37 vertices of "clutter": at batch 256 two full batches and a partial one, at the default one partial batch; nearly every third vertex
    founds a cluster inside its batch and the two after it join that cluster while it is dirty"""
    xyz, nrm = (a[:2 * 256 + 37].copy() for a in clutter_points)
    p = alignment.default_params(min_cluster_points=1, behind_max=100)
    ac.tune_batch(batch)
    got, want = ac.stage_planes(xyz, nrm, p, DEV), checker.planes(xyz, nrm, p)
    assert ac.same_planes(got, want)
    assert got["batches"] == -(-len(xyz) // batch) and got["dirty"] > 0
    assert want["founded"] > 100 and len(want["ids"]) == want["founded"]       # min_cluster_points 1: the whole table, sorted


def test_clustering_across_chunks(checker, clutter_points):
    """the whole case: more than 1024 clusters, so the match kernel's table spans two chunks and a vertex's lowest match may lie in either"""
    xyz, nrm = clutter_points
    p = alignment.default_params(**ac.CLUTTER_PARAMS)
    got, want = ac.stage_planes(xyz, nrm, p, DEV), checker.planes(xyz, nrm, p)
    assert want["founded"] >= 1100
    assert ac.same_planes(got, want)


def test_fallback_rescan_on_the_adversarial_triple(checker, default_batch):
    """Batch 64.  Vertex 0 founds cluster 0 (normal n0 = +z); vertex 1, 40 degrees to one side, founds cluster 1; 62 far-away vertices fill the batch.
    In the second batch vertex 64 (25 degrees to the other side, dot 0.906) joins cluster 0 and turns its representative by 12.5 degrees; vertex 65 (25
    degrees towards cluster 1) passed cluster 0 in the snapshot (dot 0.906) and fails the moved representative (37.5 degrees, dot 0.79): the snapshot match
    is dirty and fails, no dirty cluster before it passes, so the commit scans the table again and finds the clean cluster 1 (15 degrees)."""
    def n(deg):
        a = np.radians(deg)
        return [np.sin(a), 0.0, np.cos(a)]
    far = [[10.0 + i, 50.0, 0.0] for i in range(62)]
    xyz = np.array([[0, 0, 0], [0.004, 0, 0]] + far + [[0, 0.004, 0], [0.004, 0.004, 0]], np.float32)
    nrm = np.array([n(0), n(-40)] + [[0.0, 1.0, 0.0]] * 62 + [n(25), n(-25)], np.float32)
    assert np.ptp(xyz[[0, 1, 64, 65]], axis=0).max() < 0.01
    p = alignment.default_params(min_cluster_points=1)
    want = checker.planes(xyz, nrm, p)
    assert want["index"][[0, 1, 64, 65]].tolist() == [0, 1, 0, 1]              # on the checker first: the triple does what it was built for
    ac.tune_batch(64)
    got = ac.stage_planes(xyz, nrm, p, DEV)
    assert ac.same_planes(got, want)
    assert got["fallbacks"] > 0 and got["dirty"] > 0, got


def test_behind_counts_at_the_limit(checker):
    """cluster A (z = 0, looking up) has exactly 100 vertices further than 0.1 behind it and stays; cluster C (z = 10, looking down) has 101 and goes"""
    rng = np.random.default_rng(2)
    def plane(n, z):
        return np.stack([rng.uniform(0, 1, n), rng.uniform(0, 1, n), np.full(n, z)], -1)
    side = lambda n, z: np.stack([np.zeros(n), rng.uniform(0, 1, n), np.full(n, z)], -1)   # on the plane x = 0, looking along +x
    xyz = np.concatenate([plane(300, 0.0), plane(300, 10.0), side(100, -1.0), side(101, 11.0)]).astype(np.float32)
    nrm = np.concatenate([np.tile([0, 0, 1.0], (300, 1)), np.tile([0, 0, -1.0], (300, 1)), np.tile([1.0, 0, 0], (201, 1))]).astype(np.float32)
    p = alignment.default_params(min_cluster_points=50, behind_max=100)
    want = checker.planes(xyz, nrm, p)
    assert want["ids"].tolist() == [0, 1, 2] and want["counts"].tolist() == [300, 300, 201]
    assert want["behind"].tolist() == [100, 101, 0]                            # kept at the limit, removed one above it
    got = ac.stage_planes(xyz, nrm, p, DEV)
    assert ac.same_planes(got, want)
    reps = np.concatenate([want["table"][:, :4]] * 400)[:1030]                 # the kernel alone, on more planes than one chunk holds
    assert np.array_equal(ac.stage_behind(xyz, reps, p.behind_dist, DEV), checker.behind(xyz, reps, p.behind_dist))
    assert np.array_equal(checker.behind(xyz, reps, p.behind_dist)[:3], [100, 101, 0])


def test_cov_three_blocks_and_an_empty_set(checker):
    """2 * 256 + 100 vertices: the inliers of cluster 1 lie in all three blocks of 256, the last one partial; vertices of another cluster and outliers
    of this one lie between them.  Then a cluster nobody belongs to: ten zeros."""
    rng = np.random.default_rng(3)
    nv = 2 * 256 + 100
    xyz = np.stack([rng.uniform(-3, 3, nv), rng.uniform(-3, 3, nv), rng.normal(0, 0.03, nv)], -1).astype(np.float32)
    index = rng.integers(0, 2, nv).astype(np.uint32)
    rep = np.array([0, 0, 1, 0.001], np.float32)
    want = checker.cov(xyz, index, 1, rep, 0.05)
    inl = (index == 1) & (np.abs(xyz[:, 2] + np.float32(0.001)) < 0.05)
    assert want[0] == inl.sum() and all(inl[b:b + 256].any() for b in (0, 256, 512)) and (~inl & (index == 1)).any()
    assert np.array_equal(ac.bits(ac.stage_cov(xyz, index, 1, rep, 0.05, DEV)), ac.bits(want))
    assert np.array_equal(ac.stage_cov(xyz, index, 7, rep, 0.05, DEV), np.zeros(10)) and np.array_equal(checker.cov(xyz, index, 7, rep, 0.05), np.zeros(10))


@pytest.mark.parametrize("nv", [1000, 2048 * 256 + 77])
def test_transform_extremes_at_the_first_and_last_vertex(checker, nv):
    """the bounding box's corners are the first and the last vertex; the larger size makes the kernel's 2048 workgroups take a second stride"""
    rng = np.random.default_rng(4)
    xyz = rng.uniform(-5, 5, (nv, 3)).astype(np.float32)
    xyz[0], xyz[-1] = (-7.5, -8.25, -9.0), (7.5, 8.25, 9.0)
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = ac.rotation((0, 0, 1), 0.0)                                    # axes kept, so the extremes stay where they were put ...
    M[:3, 3] = (0.5, -0.25, 2.0)
    got, gbox = ac.stage_transform(xyz, M, DEV)
    want, wbox = checker.transform(xyz, M)
    assert np.array_equal(ac.bits(got), ac.bits(want)) and np.array_equal(ac.bits(gbox), ac.bits(wbox))
    assert np.array_equal(wbox, np.concatenate([want[0], want[-1]]))
    M[:3, :3] = ac.rotation((1, 2, 3), 1.1).astype(np.float32)                 # ... and a general matrix
    got, gbox = ac.stage_transform(xyz, M, DEV)
    want, wbox = checker.transform(xyz, M)
    assert np.array_equal(ac.bits(got), ac.bits(want)) and np.array_equal(ac.bits(gbox), ac.bits(wbox))


@pytest.mark.parametrize("name", ["room", "clutter"])
def test_estimate_on_the_device_is_the_host_paths_bits(name):
    xyz, tris = ac.room()[:2] if name == "room" else ac.clutter()
    p = alignment.default_params(**(ac.ROOM_PARAMS if name == "room" else ac.CLUTTER_PARAMS))
    mesh, sd = Mesh.from_arrays(xyz, tris), ac.make_sens(ac.room_trajectory())
    Th, sh = alignment.estimate(mesh, sd, params=p)
    Tg, sg = alignment.estimate(mesh, sd, device=DEV, params=p)
    mesh.close()
    sd.close()
    assert np.array_equal(ac.bits(Tg), ac.bits(Th))
    for k in ("vertices", "faces", "clusters_founded", "clusters_after_small", "clusters_kept", "floor_points", "floor_inliers", "floor_found", "up_source"):
        assert sg[k] == sh[k], k
    assert sg["gpu_batches"] == -(-sg["vertices"] // 1024) and sh["gpu_batches"] == 0


def test_tool_on_the_device_writes_the_host_runs_bytes(tmp_path):
    xyz, tris, _, _ = ac.room()
    poses = [np.eye(4, dtype=np.float32)] + ac.room_trajectory()[1:]
    host = ac.write_scan_folder(tmp_path / "h", "scene", xyz, tris, poses)
    dev = str(tmp_path / "d" / "scene")
    shutil.copytree(host, dev)
    rh = subprocess.run([ac.TOOL, host], capture_output=True, text=True)
    rd = subprocess.run([ac.TOOL, dev, "--gpu=%d" % DEV], capture_output=True, text=True)
    assert (rh.returncode, rh.stderr, rd.returncode, rd.stderr) == (0, "", 0, "")
    assert rd.stdout == "aligning: %s\n" % dev
    fh, fd = ac.folder_bytes(host), ac.folder_bytes(dev)
    assert sorted(fh) == sorted(fd) == ["processed.txt", "scene.ply", "scene.sens", "scene_vh_clean.ply"]
    for n in fh:
        assert fh[n] == fd[n], n
    rd = subprocess.run([ac.TOOL, dev, "--gpu=%d" % DEV, "--force"], capture_output=True, text=True)   # the revert goes through k_aa_transform too
    rh = subprocess.run([ac.TOOL, host, "--force"], capture_output=True, text=True)
    assert (rh.returncode, rh.stderr, rd.returncode, rd.stderr) == (0, "", 0, "")
    assert ac.folder_bytes(host) == ac.folder_bytes(dev)
