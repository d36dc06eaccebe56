#!/usr/bin/env python3
"""Regenerates tests/golden/depth_lut_golden.json: SHA-256 digests of the sums and the finished table that the CPU checker of the
depth-distortion table (tests/depth_lut_checker.c) gives on the named cases of tests/depth_lut_cases.py.  The reference
binary cannot be built here, so these are not reference vectors: they freeze the rule's executable form, so that neither the checker nor the
host path nor the kernels can drift silently.

    python tests/golden/make_depth_lut_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import depth_lut_cases as dc  # noqa: E402

CASES = [("small", True), ("small", False), ("small_50x38", True), ("small_10x2", True), ("real", True), ("roundtrip", True)]

if __name__ == "__main__":
    out = {}
    for name, shift in CASES:
        acc, div, table = dc.checker_case(name, shift)
        out["%s/%s" % (name, "shift" if shift else "noshift")] = dict(acc=dc.digest(acc), div=dc.digest(div), table=dc.digest(table))
    json.dump(out, open(dc.GOLDEN, "w"), indent=1, sort_keys=True)
    print(dc.GOLDEN, len(out))
