"""The record of tests/audio_ops_cases.py and tests/conv_rows_cases.py: per op and case group the worst error / bound of the float32
restatement and the best error / bound of every mutant (CPU), and -- with --gpu, on the MI355X -- the worst error / bound of the
kernel itself and the case it came from.

    python tools/audio_ops_errors.py [--gpu] [--before LOG] [--out profiles/audio_ops_errors.txt]

--before LOG: the printed lines of tests/test_gpu_audio_ops.py from a GPU run of an EARLIER build (pytest -s); its statistics-kernel
lines are copied under a heading of their own, so that a change of those kernels keeps its before and after side by side.
Without --gpu the kernel lines are left out: nothing measured on a CPU is ever written under a GPU heading."""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests import audio_ops_cases as A  # noqa: E402
from tests import conv_rows_cases as R  # noqa: E402

STAT_OPS = ("wave_normalize", "w2v2_conv0")


def group_of(op, case) -> str:
    return f"{op} {case[0]}" if op in STAT_OPS else op


def cpu_ratios(op, mutant=None):
    """{case group: (worst error / bound, case)} of the restatement (or a mutant of it)"""
    out = {}
    for case in A.OPS[op].cases:
        inp = A.OPS[op].make(case)
        with np.errstate(invalid="ignore"):
            r = max(A.check(op, case, inp, A.OPS[op].restate(case, inp, mutant)).values())
        g = group_of(op, case)
        if g not in out or r > out[g][0]:
            out[g] = (r, case)
    return out


def conv_rows_groups(measure):
    out = {}
    for c in R.CASES:
        r = measure(c)
        g = f"conv1d_rows {c.family} tile {c.want}" + (" xcd_cols 2" if c.xcd == 2 else "")
        if g not in out or r > out[g][0]:
            out[g] = (r, c.id)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--before", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["error / bound per op and case group (bounds: tests/audio_ops_cases.py, tests/conv_rows_cases.py; 0 = bit-equal where the bound is 0, "
             "inf = a bit differs there)", ""]
    if a.gpu:
        import torch
        from tests import test_gpu_audio_ops as T
        prop = torch.cuda.get_device_properties(0)
        lines.append(f"kernel on the GPU ({prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs; worst over the group's cases)")
        for g, (r, cid) in conv_rows_groups(lambda c: T.measure_conv_rows(c)[0]).items():
            lines.append(f"  {g:44s} {r:10.3g}   at {cid}")
        for op in sorted(A.OPS):
            groups = {}
            for case in A.OPS[op].cases:
                r = max(T.measure(op, case).values())
                g = group_of(op, case)
                if g not in groups or r > groups[g][0]:
                    groups[g] = (r, case)
            for g, (r, case) in groups.items():
                lines.append(f"  {g:44s} {r:10.3g}   at {A.case_id(case)}")
        lines.append("")
    if a.before:
        lines.append("the statistics kernels of the build before (sums about a chunk's FIRST value), same cases, same bounds, on the GPU")
        for ln in Path(a.before).read_text().splitlines():
            ln = ln.lstrip(".F")
            if ln.startswith(STAT_OPS) and "worst error / bound" in ln:
                lines.append("  " + ln)
        lines.append("")
    lines.append("float32 restatement on the CPU (worst over the group's cases and two summation orders for conv1d_rows; must be <= 1)")

    def emulated(c):
        inp = R.make(c)
        refs = R.reference(c, inp)
        return max(max(R.check(c, inp, R.emulate(c, inp, o), refs).values()) for o in (0, 1))
    for g, (r, cid) in conv_rows_groups(emulated).items():
        lines.append(f"  {g:44s} {r:10.3g}   at {cid}")
    for op in sorted(A.OPS):
        for g, (r, case) in cpu_ratios(op).items():
            lines.append(f"  {g:44s} {r:10.3g}   at {A.case_id(case)}")
    lines += ["", f"mutants on the CPU (per case group; a mutant must reach {A.MUTANT_FACTOR:g} or inf on at least one group of its op; pivot_sensitive: "
              "tests/test_audio_ops_cases.py)"]
    for m in R.MUTANTS:
        c = R.BY_ID[R.KILLS[m]]
        inp = R.make(c)
        r = max(R.check(c, inp, R.emulate(c, inp, 0, m)).values())
        lines.append(f"  {'conv1d_rows':16s} {m:34s} {r:10.3g}   at {c.id}")
    for op in sorted(A.OPS):
        for m in A.OPS[op].mutants:
            for g, (r, case) in cpu_ratios(op, m).items():
                if op in STAT_OPS or r >= A.MUTANT_FACTOR or math.isinf(r):
                    lines.append(f"  {g:34s} {m:34s} {r:10.3g}   at {A.case_id(case)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
