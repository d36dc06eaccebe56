#!/usr/bin/env python3
"""Regenerates tests/golden/drop_in_segmentator_golden.json: the REFERENCE Segmentator binary (oracle/_ref/segmentator_ref, see oracle/Makefile) on
the cleaned mesh the drop-in executables make in tests/test_gpu_pipeline.py::test_drop_in_executables -- so that the test holds bin/segmentator
against the reference's bytes where the reference is not built.  Needs the GPU (bin/depthsensing) and the reference build:

    python tests/golden/make_drop_in_golden.py [OUT.json]
"""
import hashlib
import json
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_gpu_pipeline as t  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "segmentator_ref")
if not os.path.exists(REF):
    raise SystemExit("oracle/_ref/segmentator_ref is not built (make -C oracle ref)")
out_path = sys.argv[1] if len(sys.argv) > 1 else t.DROP_IN_GOLDEN
with tempfile.TemporaryDirectory() as d:
    _, _, clean_ply = t._drop_in_clean_mesh(pathlib.Path(d))
    ref_dir = os.path.join(d, "ref")
    os.mkdir(ref_dir)
    shutil.copy(clean_ply, os.path.join(ref_dir, "scene0000_00_vh_clean.ply"))
    subprocess.run([REF, os.path.join(ref_dir, "scene0000_00_vh_clean.ply")], check=True, capture_output=True)
    segs = open(os.path.join(ref_dir, "scene0000_00_vh_clean.0.010000.segs.json"), "rb").read()
    out = {"generator": "tests/golden/make_drop_in_golden.py (oracle/_ref/segmentator_ref, reference Segmentator, -std=c++11 -O2)",
           "mesh_sha256": t._mesh_sha256(clean_ply), "segs_json_sha256": hashlib.sha256(segs).hexdigest(), "segs_json_bytes": len(segs),
           "num_segments": len(set(json.loads(segs)["segIndices"]))}
json.dump(out, open(out_path, "w"), indent=1)
open(out_path, "a").write("\n")
print("wrote", out_path, out)
