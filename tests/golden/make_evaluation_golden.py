"""Writes tests/golden/evaluation_golden.json: what the reference's own 3-D evaluation scripts say about the file cases of
tests/evaluation_cases.py (write_label_dirs, write_instance_dirs).

    python tests/golden/make_evaluation_golden.py /path/to/ScanNet

The scripts are Python 2.  They are translated with lib2to3 into a temporary directory, the `try:` block the translation leaves empty gets a `pass`,
empty stand-in modules serve for plyfile and imageio (neither is used by the two scripts), np.float / np.bool / np.int are set from outside, and the
scripts are run there on the cases written as files.  Nothing of the translated text is kept: only the recorded outputs and the hashes of the inputs
(so that a drift of numpy's generator fails the test instead of comparing different inputs) go into the JSON."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import evaluation_cases as ec  # noqa: E402

RUNNER = """import sys, runpy
import numpy as np
np.float, np.bool, np.int = float, bool, int
sys.argv = sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
"""


def translate(reference, work):
    src = os.path.join(reference, "BenchmarkScripts")
    dst = os.path.join(work, "BenchmarkScripts")
    os.makedirs(os.path.join(dst, "3d_evaluation"))
    for rel in ("util.py", "util_3d.py", "3d_evaluation/evaluate_semantic_label.py", "3d_evaluation/evaluate_semantic_instance.py"):
        shutil.copy(os.path.join(src, rel), os.path.join(dst, rel))
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", dst], check=True, capture_output=True)
    for dirpath, _, files in os.walk(dst):
        for fn in files:
            if fn.endswith(".py"):
                path = os.path.join(dirpath, fn)
                text = open(path).read()
                text = re.sub(r"(\n[ \t]*)try:\n(\s*)except", lambda m: "%stry:%s    pass\n%sexcept" % (m.group(1), m.group(1), m.group(2)), text)
                open(path, "w").write(text)
    for stand_in in ("plyfile", "imageio"):
        open(os.path.join(dst, stand_in + ".py"), "w").write("PlyData = PlyElement = None\n")
    open(os.path.join(work, "runner.py"), "w").write(RUNNER)
    return dst


def run(work, dst, script, pred_path, gt_path, output_file):
    env = dict(os.environ, PYTHONPATH=dst)
    r = subprocess.run([sys.executable, os.path.join(work, "runner.py"), os.path.join(dst, "3d_evaluation", script), "--pred_path", pred_path, "--gt_path", gt_path,
                        "--output_file", output_file], capture_output=True, text=True, env=env, cwd=work)
    if r.returncode != 0:
        raise SystemExit("%s failed:\n%s\n%s" % (script, r.stdout[-2000:], r.stderr[-4000:]))
    return r.stdout


def main():
    reference = sys.argv[1]
    work = tempfile.mkdtemp(prefix="evaluation_golden_")
    try:
        dst = translate(reference, work)
        pred_path, gt_path, sha = ec.write_label_dirs(work)
        out = os.path.join(work, "label_result.txt")
        stdout = run(work, dst, "evaluate_semantic_label.py", pred_path, gt_path, out)
        golden = {"label3d": {"inputs_sha256": sha, "result_file": open(out).read(), "table": ec.label_table(stdout)}}
        pred_path, gt_path, sha, _ = ec.write_instance_dirs(work)
        out = os.path.join(work, "instance_result.txt")
        stdout = run(work, dst, "evaluate_semantic_instance.py", pred_path, gt_path, out)
        rows = [ln.split(",") for ln in open(out).read().splitlines()]
        golden["instance3d"] = {"inputs_sha256": sha, "header": rows[0], "rows": [[r[0], int(r[1]), float(r[2]), float(r[3]), float(r[4])] for r in rows[1:]],
                                "table": ec.instance_table(stdout)}
        text = json.dumps(golden, indent=1).replace("NaN", "null")
        open(os.path.join(ROOT, "tests", "golden", "evaluation_golden.json"), "w").write(text + "\n")
        print("label3d:", len(golden["label3d"]["result_file"]), "bytes; instance3d:", len(golden["instance3d"]["rows"]), "classes")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
