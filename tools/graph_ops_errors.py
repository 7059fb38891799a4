#!/usr/bin/env python3
"""The record of tests/test_gpu_graph_ops.py: the measured error, the bound and their ratio of every case of the graph-side and
temporal entries on the MI355X (bounds: tests/graph_ops_cases.py -- 0 = bit-equal, derived for ufnd_node_features, 3 x the float32
restatement's own distance from float64 for the composite entries; the tests hold every ratio to 1), the worst ratio per entry and
output first.  Runs the test file in a child process and collects the figures every test prints before it asserts.

    python tools/graph_ops_errors.py [--out profiles/graph_ops_errors.txt] [--log FILE] [--parent-log FILE --parent-name COMMIT] [--note FILE]

--log FILE: summarise the kept output of an earlier `pytest tests/test_gpu_graph_ops.py -m gpu -s` run on the MI355X instead of running one.
--parent-log FILE: the same file's kept output with another commit's library loaded; its cases with a ratio above 1 are listed under
a heading that names the commit.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
NUM = r"([-+.\de]+|inf|nan)"
LINE = re.compile(rf"GRAPH_OPS_ERR (\S+) (\S+) (\S+) gpu={NUM} bound={NUM} ratio={NUM}")
CONTROL = re.compile(r"GRAPH_OPS_CONTROL (.*)")


def rows_of(text):
    return [(e, c, k, float(g), float(b), float(r)) for e, c, k, g, b, r in LINE.findall(text)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--parent-log", default=None)
    ap.add_argument("--parent-name", default="parent")
    ap.add_argument("--note", default=None)
    a = ap.parse_args()
    if a.log:
        r = subprocess.CompletedProcess([], 0, stdout=Path(a.log).read_text(), stderr="")
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_graph_ops.py", "-m", "gpu", "-s", "-q", "-p", "no:cacheprovider"], cwd=str(REPO),
                           capture_output=True, text=True, timeout=900)
    rows = rows_of(r.stdout)
    if not rows:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-2000:])
        raise SystemExit("graph_ops_errors.py: the GPU tests printed no figures (no MI355X?)")
    worst = {}
    for e, c, k, g, b, ratio in rows:
        key = (e.split(".")[0], re.sub(r"\d+$", "", k) if k.startswith("running_") else k)
        if key not in worst or ratio > worst[key][0]:
            worst[key] = (ratio, c, k, g, b)
    lines = ["Graph-side and temporal entries on the MI355X against float64 (tests/test_gpu_graph_ops.py): error / bound, the tests hold every case to 1",
             "(ratio 0 with bound 0: bit-equal; the loss of the pretrain step is judged over the whole table, see tests/graph_ops_cases.py)", "",
             "worst case per entry and output (running_mean / running_var: over the layers)"]
    for (e, k), (ratio, c, kk, g, b) in sorted(worst.items()):
        lines.append(f"  {e:16s} {k:14s} {ratio:8.3g}   at {c} {kk} (gpu {g:.3e}, bound {b:.3e})")
    lines += [f"  gcn_pretrain     loss           {float(x):8.3g}   over the table (max relative error / 3 x the restatement's)"
              for x in re.findall(rf"GRAPH_OPS_ERR gcn_pretrain table loss ratio={NUM}", r.stdout)]
    lines += ["", "negative controls of the dropout sites (share of the elements outside the bound; the tests ask for 0.25)"]
    lines += ["  " + m for m in CONTROL.findall(r.stdout)]
    if a.parent_log:
        bad = [x for x in rows_of(Path(a.parent_log).read_text()) if not x[5] <= 1.0]
        lines += ["", f"the same cases with the library of {a.parent_name} (the backward products used A_norm, not A_norm^T): {len(bad)} outputs above 1, "
                      f"all on directed or asymmetrically weighted graphs: {all(any(d in x[1] for d in ('directed', 'asym')) for x in bad)}"]
        lines += [f"  {e:16s} {c:44s} {k:12s} gpu={g:.3e} bound={b:.3e} ratio={ratio:.3g}" for e, c, k, g, b, ratio in bad]
    lines += ["", "every case"]
    lines += [f"  {e:24s} {c:44s} {k:14s} gpu={g:.3e} bound={b:.3e} ratio={ratio:.3g}" for e, c, k, g, b, ratio in rows]
    if a.note:
        lines += ["", Path(a.note).read_text().rstrip()]
    lines += ["", f"pytest: {r.stdout.strip().splitlines()[-1]}"]
    text = "\n".join(lines) + "\n"
    print(text[:6000], end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    if r.returncode != 0:
        raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
