#!/usr/bin/env python3
"""Regenerates tests/golden/solver_checker.json: SHA-256 digests of what the CPU restatements of the tracker and of the global alignment
(tests/track_checker.c and tests/align_checker.c over tests/solver_rules.h) say on the small cases of tests/solver_scenes.py, and of each case's
inputs.  The checkers are the specification's executable form and every GPU bit is held to them, so these digests keep them from drifting:
tests/test_track_colour.py and tests/test_align_colour.py (test_checker_reproduces_the_recorded_digests) compare against the file.

The file was first recorded from the four separate checkers that preceded the two (depth-only and with colour, per solver), so it also shows that
folding them into one set of rules changed no bit.  A change of a rule changes it on purpose: regenerate and say so.

    python tests/golden/make_solver_checker_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402
from tests import solver_scenes as ss  # noqa: E402


def main():
    oracle.lib()
    out = {}
    for name in ss.CASE_NAMES:
        out[name] = ss.run_case(name, oracle)
        print(name, out[name]["inputs"][:16], len(out[name]["outputs"]), "outputs")
    with open(ss.GOLDEN, "w") as f:
        json.dump({"cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", ss.GOLDEN)


if __name__ == "__main__":
    main()
