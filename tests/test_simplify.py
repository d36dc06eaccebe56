"""Decimate stage: "Quadric Edge Collapse Decimation" of simplify.mlx (scannet_amd/csrc/simplify.cpp).
PARITY UNPINNED against MeshLab (not in the reference tree, no version pinned): the filter is checked through the properties
the algorithm guarantees -- face budget, planarity and border of flat regions, closedness and Euler characteristic of a closed
surface, geometric error bounds, determinism -- plus the shipped script and the meshlabserver-compatible CLI."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from scannet_amd import meshclean
from scannet_amd.segmentator import Mesh
from tests import meshes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the same filters and values as Server/tools/meshclean/simplify.mlx:3-24 (tooltips dropped)
SIMPLIFY_MLX = """<!DOCTYPE FilterScript>
<FilterScript>
 <filter name="Quadric Edge Collapse Decimation">
  <Param value="0" type="RichInt" name="TargetFaceNum"/>
  <Param value="0.2" type="RichFloat" name="TargetPerc"/>
  <Param value="0.3" type="RichFloat" name="QualityThr"/>
  <Param value="false" type="RichBool" name="PreserveBoundary"/>
  <Param value="1" type="RichFloat" name="BoundaryWeight"/>
  <Param value="false" type="RichBool" name="PreserveNormal"/>
  <Param value="false" type="RichBool" name="PreserveTopology"/>
  <Param value="true" type="RichBool" name="OptimalPlacement"/>
  <Param value="false" type="RichBool" name="PlanarQuadric"/>
  <Param value="false" type="RichBool" name="QualityWeight"/>
  <Param value="true" type="RichBool" name="AutoClean"/>
  <Param value="false" type="RichBool" name="Selected"/>
 </filter>
 <filter name="Merge Close Vertices">
  <Param min="0" max="0.106888" name="Threshold" value="0.0010689" type="RichAbsPerc"/>
 </filter>
 <filter name="Remove Duplicate Faces"/>
 <filter name="Remove Isolated pieces (wrt Face Num.)">
  <Param name="MinComponentSize" value="1000" type="RichInt"/>
 </filter>
 <filter name="Remove Unreferenced Vertex"/>
</FilterScript>
"""


def _plane(n, noise=0.0, seed=1):
    xs = np.linspace(0, 1, n, dtype=np.float32)
    X, Y = np.meshgrid(xs, xs, indexing="xy")
    Z = (noise * np.random.default_rng(seed).standard_normal(X.shape)).astype(np.float32)
    v = np.stack([X, Y, Z], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.uint32)


def _icosphere(sub):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(sub):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (v[a] + v[b]) / 2
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.uint32)


def _edge_counts(tris):
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64), axis=1)
    _, cnt = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    return cnt


def test_plane_stays_planar_and_keeps_its_border():
    v, t = _plane(120)
    out, st = meshclean.simplify(Mesh.from_arrays(v, t))
    xyz, _, tris = out.arrays()
    assert st["faces_in"] == len(t) and st["target_faces"] == int(len(t) * 0.2)
    assert st["faces_out"] == len(tris) <= st["target_faces"] and st["faces_out"] >= st["target_faces"] - 2
    assert np.abs(xyz[:, 2]).max() == 0.0                      # flat stays exactly flat (no spikes: the rank-deficient case)
    assert xyz[:, :2].min() >= -1e-6 and xyz[:, :2].max() <= 1 + 1e-6
    # border quadrics keep the outline: the square's area survives within 0.1 %
    a, b, c = xyz[tris[:, 0]], xyz[tris[:, 1]], xyz[tris[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert abs(area.sum() - 1.0) < 1e-3 and area.min() > 0
    # orientation preserved: every normal still points to +z
    assert (np.cross(b - a, c - a)[:, 2] > 0).all()


def test_closed_surface_stays_closed():
    v, t = _icosphere(5)  # 20480 faces
    out, st = meshclean.simplify(Mesh.from_arrays(v, t))
    xyz, _, tris = out.arrays()
    assert len(tris) == st["faces_out"] == int(len(t) * 0.2)
    assert (_edge_counts(tris) == 2).all()                    # still a closed 2-manifold edge-wise
    assert len(xyz) - len(tris) * 3 // 2 + len(tris) == 2     # Euler characteristic of a sphere
    r = np.linalg.norm(xyz, axis=1)
    assert abs(r - 1).max() < 2e-3                             # 5x fewer faces, radial error well under the sagitta of the input
    a, b, c = xyz[tris[:, 0]], xyz[tris[:, 1]], xyz[tris[:, 2]]
    n = np.cross(b - a, c - a)
    assert (np.einsum("ij,ij->i", n, (a + b + c)) > 0).all()   # no flipped face


def test_heightfield_error_and_determinism():
    v, t = meshes.bumpy(120, creases=True)
    m = Mesh.from_arrays(v, t)
    out1, st1 = meshclean.simplify(m)
    out2, st2 = meshclean.simplify(m)
    x1, _, t1 = out1.arrays()
    x2, _, t2 = out2.arrays()
    assert np.array_equal(x1.view(np.uint32), x2.view(np.uint32)) and np.array_equal(t1, t2) and st1 == st2
    assert st1["faces_out"] <= st1["target_faces"]
    # every output vertex lies close to the input surface (input spacing 0.02, relief up to 0.3)
    used = np.unique(t)
    d, _ = cKDTree(v[used]).query(x1)
    assert d.max() < 0.02 and np.median(d) < 0.01
    # AutoClean: the 7 unreferenced vertices of the input are gone, no degenerate faces remain
    assert len(x1) == len(np.unique(t1)) and (t1[:, 0] != t1[:, 1]).all() and (t1[:, 1] != t1[:, 2]).all() and (t1[:, 0] != t1[:, 2]).all()


def test_parameters_and_edge_cases():
    v, t = _plane(30)
    m = Mesh.from_arrays(v, t)
    out, st = meshclean.simplify(m, target_perc=0.0, target_faces=100)
    assert st["target_faces"] == 100 and st["faces_out"] <= 100
    out, st = meshclean.simplify(m, target_perc=1.0)           # nothing to do
    assert st["collapses"] == 0 and st["faces_out"] == len(t)
    out, st = meshclean.simplify(m, optimal_placement=0)       # subset placement: output vertices are input vertices
    xyz = out.arrays()[0]
    assert set(map(tuple, xyz.view(np.uint32))) <= set(map(tuple, v.view(np.uint32)))
    for unsupported in ("preserve_boundary", "preserve_normal", "preserve_topology", "quality_weight"):
        with pytest.raises(Exception, match="not implemented"):
            meshclean.simplify(m, **{unsupported: 1})
    with pytest.raises(Exception):
        meshclean.simplify(m, target_perc=1.5)
    # colours travel with the surviving vertex
    rgba = np.zeros((len(v), 4), np.uint8)
    rgba[:, 0] = np.arange(len(v)) % 251
    rgba[:, 3] = 255
    out, _ = meshclean.simplify(Mesh.from_arrays(v, t, rgba))
    _, c, _ = out.arrays()
    assert (c[:, 3] == 255).all() and c[:, 0].max() <= 250
    # empty mesh, faces with a repeated vertex
    out, st = meshclean.simplify(Mesh.from_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)))
    assert out.counts() == (0, 0)
    out, st = meshclean.simplify(Mesh.from_arrays(v[[0, 1, 30]], np.array([[0, 1, 1], [0, 1, 2]], np.uint32)), target_perc=1.0)
    assert st["faces_out"] == 1


def test_script_params_behind_markup_in_attributes(tmp_path):
    """MeshLab writes every Param with a tooltip that may hold markup -- "&lt;br>", "&#xa;", a bare '>' -- and not always after name= (the shipped
    simplify.mlx puts QualityThr's tooltip before it).  Every value must be read, not left at its default: each one below differs from the default."""
    tip = 'tooltip="first line&lt;br>second line&#xa; values > 0 &lt; 1 &lt;b>bold&lt;/b>"'
    params = [("TargetFaceNum", "5000", "RichInt"), ("TargetPerc", "0.35", "RichFloat"), ("QualityThr", "0.45", "RichFloat"),
              ("PreserveBoundary", "true", "RichBool"), ("BoundaryWeight", "2.5", "RichFloat"), ("PreserveNormal", "true", "RichBool"),
              ("PreserveTopology", "true", "RichBool"), ("OptimalPlacement", "false", "RichBool"), ("PlanarQuadric", "true", "RichBool"),
              ("QualityWeight", "true", "RichBool"), ("AutoClean", "false", "RichBool")]
    lines = ['<!DOCTYPE FilterScript>', '<FilterScript>', ' <filter name="Quadric Edge Collapse Decimation">']
    lines += ['  <Param value="%s" %s type="%s" name="%s" description="d&lt;i>"/>' % (v, tip, t, n) for n, v, t in params]
    lines += [' </filter>', ' <filter name="Merge Close Vertices">',
              '  <Param min="0" max="0.1" %s description="x > y" name="Threshold" value="0.0021" type="RichAbsPerc"/>' % tip, ' </filter>',
              ' <filter name="Remove Duplicate Faces"/>', ' <filter name="Remove Isolated pieces (wrt Face Num.)">',
              '  <Param description="n:" name="MinComponentSize" %s value="333" type="RichInt"/>' % tip, ' </filter>',
              ' <filter name="Remove Unreferenced Vertex"/>', '</FilterScript>']
    path = tmp_path / "markup.mlx"
    path.write_text("\n".join(lines) + "\n")
    s = meshclean.load_script(str(path))
    sp = s.simplify_params
    assert s.simplify == 1 and sp.target_faces == 5000 and abs(sp.target_perc - 0.35) < 1e-7 and abs(sp.quality_thr - 0.45) < 1e-7
    assert abs(sp.boundary_weight - 2.5) < 1e-7
    assert (sp.preserve_boundary, sp.preserve_normal, sp.preserve_topology, sp.optimal_placement, sp.planar_quadric, sp.quality_weight,
            sp.auto_clean) == (1, 1, 1, 0, 1, 1, 0)
    assert (s.merge_close_vertices, s.remove_duplicate_faces, s.remove_small_components, s.remove_unreferenced) == (1, 1, 1, 1)
    assert abs(s.merge_distance - 0.0021) < 1e-9 and s.min_component_faces == 333


def test_shipped_script_and_cli(tmp_path):
    path = str(tmp_path / "simplify.mlx")
    open(path, "w").write(SIMPLIFY_MLX)
    for p in (path, str(tmp_path / "mine.mlx")):
        if p != path:
            open(p, "w").write(SIMPLIFY_MLX)
        s = meshclean.load_script(p)
        sp = s.simplify_params
        assert s.simplify == 1 and abs(sp.target_perc - 0.2) < 1e-7 and abs(sp.quality_thr - 0.3) < 1e-7 and sp.target_faces == 0
        assert (sp.preserve_boundary, sp.preserve_normal, sp.preserve_topology, sp.optimal_placement, sp.planar_quadric, sp.quality_weight,
                sp.auto_clean) == (0, 0, 0, 1, 0, 0, 1) and sp.boundary_weight == 1.0
        assert (s.merge_close_vertices, s.remove_duplicate_faces, s.remove_small_components, s.remove_unreferenced) == (1, 1, 1, 1)
        assert abs(s.merge_distance - 0.0010689) < 1e-9 and s.min_component_faces == 1000
    bad = tmp_path / "late.mlx"
    bad.write_text(SIMPLIFY_MLX.replace('<filter name="Quadric Edge Collapse Decimation">', '<filter name="Remove Duplicate Faces"/>\n <filter name="Quadric Edge Collapse Decimation">', 1))
    with pytest.raises(Exception, match="first filter"):
        meshclean.load_script(str(bad))
    # the decimate stage as Server/scan_processor.py:144-145 runs it: two passes, each to 20 %
    v, t = _icosphere(6)  # 81920 faces
    v = (v * 0.5).astype(np.float32)
    src = str(tmp_path / "scene_vh_clean.ply")
    Mesh.from_arrays(v, t, np.full((len(v), 4), 200, np.uint8)).write_ply(src)
    exe = os.path.join(ROOT, "bin", "meshclean")
    names = [src, str(tmp_path / "scene_vh_clean_1.ply"), str(tmp_path / "scene_vh_clean_2.ply")]
    for a, b in zip(names, names[1:]):
        r = subprocess.run([exe, "-i", a, "-o", b, "-m", "vc", "-s", path], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and "Quadric Edge Collapse Decimation" in r.stdout and "Mesh saved as" in r.stdout
    x1, c1, t1 = Mesh.read(names[1]).arrays()
    x2, c2, t2 = Mesh.read(names[2]).arrays()
    assert len(t1) == 16384 and len(t2) == 3276
    assert (c2 == 200).all()
    assert abs(np.linalg.norm(x2, axis=1) - 0.5).max() < 5e-3
    # the python mirror of the same call
    st = meshclean.clean_file(names[0], str(tmp_path / "again.ply"), path)
    assert st["simplify"]["faces_out"] == 16384 and st["faces_out"] == 16384
    assert np.array_equal(Mesh.read(str(tmp_path / "again.ply")).arrays()[0], x1)
