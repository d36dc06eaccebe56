"""Writes tests/golden/instance2d_golden.json: what the reference's own 2-D instance evaluation says about the file case of
tests/instance2d_cases.py (write_file_case).

    python tests/golden/make_instance2d_golden.py /path/to/ScanNet

The three scripts (2d_evaluation/evalInstanceLevelSemanticLabeling.py, instances2dict.py, instance.py) are Python 2.  They are translated with
lib2to3 into a temporary directory and run there, with that directory on PYTHONPATH and np.float / np.bool set from outside, on the case written as
files.  The script's gtInstances.json cache lands in the same temporary directory.  Nothing of the translated text is kept: only the recorded result
file, the table and the hash of the inputs go into the JSON."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import instance2d_cases as ic  # noqa: E402

RUNNER = """import sys, runpy
import numpy as np
np.float, np.bool = float, bool
sys.argv = sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
"""
SCRIPTS = ("evalInstanceLevelSemanticLabeling.py", "instances2dict.py", "instance.py")


def translate(reference, work):
    dst = os.path.join(work, "2d_evaluation")
    os.makedirs(dst)
    for name in SCRIPTS:
        shutil.copy(os.path.join(reference, "BenchmarkScripts", "2d_evaluation", name), os.path.join(dst, name))
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", dst], check=True, capture_output=True)
    open(os.path.join(work, "runner.py"), "w").write(RUNNER)
    return dst


def run(work, dst, pred_path, gt_path, output_file):
    env = dict(os.environ, PYTHONPATH=dst)
    r = subprocess.run([sys.executable, os.path.join(work, "runner.py"), os.path.join(dst, SCRIPTS[0]), "--pred_path", pred_path, "--gt_path", gt_path,
                        "--output_file", output_file], capture_output=True, text=True, env=env, cwd=work)
    if r.returncode != 0:
        raise SystemExit("%s failed:\n%s\n%s" % (SCRIPTS[0], r.stdout[-2000:], r.stderr[-4000:]))
    return r.stdout


def main():
    reference = sys.argv[1]
    work = tempfile.mkdtemp(prefix="instance2d_golden_")
    try:
        dst = translate(reference, work)
        pred_path, gt_path, sha = ic.write_file_case(work)
        out = os.path.join(work, "instance2d_result.txt")
        stdout = run(work, dst, pred_path, gt_path, out)
        rows = [ln.split(",") for ln in open(out).read().splitlines()]
        golden = {"inputs_sha256": sha, "header": rows[0], "rows": [[r[0], int(r[1]), float(r[2]), float(r[3])] for r in rows[1:]], "table": ic.result_table(stdout)}
        text = json.dumps(golden, indent=1).replace("NaN", "null")
        open(os.path.join(ROOT, "tests", "golden", "instance2d_golden.json"), "w").write(text + "\n")
        print("instance2d:", len(golden["rows"]), "classes")
        print("\n".join(golden["table"]))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
