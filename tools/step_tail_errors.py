"""The record of tests/step_tail_cases.py: per op the worst error / bound of the float32 restatement and the best error / bound of
every mutant (CPU), and -- with --gpu, on the MI355X -- the worst error / bound of the kernels themselves and the case it came from.

    python tools/step_tail_errors.py [--gpu] [--out profiles/step_tail_errors.txt]
    python tools/step_tail_errors.py --gpu --shifted-only --lib PATH      one line: the shifted cross-entropy cases on another build

Without --gpu the kernel lines are left out: nothing measured on a CPU is ever written under a GPU heading.  --parent-lib PATH
--parent-name COMMIT adds, under a heading that names the commit, the worst error / bound of that build's cross-entropy kernels on
the shifted cases (measured in a child process: one process loads one library)."""
from __future__ import annotations

import argparse
import math
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests import step_tail_cases as S  # noqa: E402

NOTES = """notes on shares above 0.5 (why a correct kernel attains them)
  step_census      0.5: the one rounded output is grad_norm = float32(sqrt(S)), allowed one float32 ulp; a correctly rounded value is
                   up to half an ulp away.  Everything else in the family is bit-equal.
  adamw_rounded    m and v reach ~1 where g = 0 (the eps elements): m' = fma(m, b1, 0) and v' = fma(v, b2, 0) are ONE rounding each,
                   and the bound there is u |m b1| (u |v b2|) -- a single correctly rounded operation attains u of its result when the
                   result lies just above a power of two.
  cross_entropy    loss_rows reach ~1 on rows with a gap of 8 to 16: S = 1 + exp(-gap) is rounded at u S (one addition), and
                   log(S) ~ exp(-gap) carries that absolute error whole; the bound's d_S / S term is this one rounding and nothing else
                   of its size.  (torch's log_softmax forms the same sum.)
"""


def cpu_ratio(op, mutant=None):
    worst, where = 0.0, None
    cases = S.OPS[op].cases if mutant is None else S.designated_cases(op, mutant)
    for case in cases:
        inp = S.OPS[op].make(case)
        r = max(S.check(op, case, inp, S.OPS[op].restate(case, inp, mutant)).values())
        if r > worst:
            worst, where = r, case
        if worst == math.inf:
            break
    return worst, where


def shifted_line():
    from tests import test_gpu_step_tail as G
    r, case, key = G.worst_of("cross_entropy", G.shifted_cases())
    return f"  {'cross_entropy (shifted)':26s} {r:10.3g}   at {S.case_id(case)} ({key})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="load this libultrafnd_hip.so instead of the package's")
    ap.add_argument("--shifted-only", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-name", default="parent")
    a = ap.parse_args()
    if a.lib:
        from ultrafnd_git_amd import _lib as L
        L.LIB_PATH = Path(a.lib).resolve()
    if a.shifted_only:
        assert a.gpu
        print("SHIFTED" + shifted_line())
        return
    lines = ["error / bound per op (bounds: tests/step_tail_cases.py; 0 = bit-equal where the bound is 0, inf = a bit differs there)", ""]
    if a.gpu:
        import torch
        from tests import test_gpu_step_tail as G
        prop = torch.cuda.get_device_properties(0)
        lines.append(f"kernels on the GPU ({prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs; worst over the op's cases; "
                     "the two-launch and the four-launch form bit-identical on every optimizer case)")
        for op in sorted(S.OPS):
            r, case, key = G.worst_of(op)
            lines.append(f"  {op:26s} {r:10.3g}   at {S.case_id(case)} ({key})")
        lines.append(shifted_line())
        lines.append("")
        if a.parent_lib:
            out = subprocess.run([sys.executable, __file__, "--gpu", "--shifted-only", "--lib", a.parent_lib], capture_output=True, text=True, cwd=str(REPO),
                                 timeout=300)      # (expiry raises: a hung child fails the tool)
            got = [ln[len("SHIFTED"):] for ln in out.stdout.splitlines() if ln.startswith("SHIFTED")]
            assert out.returncode == 0 and len(got) == 1, (out.returncode, out.stderr[-2000:])
            lines += [f"the cross-entropy kernels of {a.parent_name} (lse = max + logf(S), then lse - l_c and __expf(l_c - lse)) on the shifted cases, same GPU",
                      got[0], ""]
    lines.append("float32 restatement on the CPU (worst over the op's cases; must be <= 1)")
    for op in sorted(S.OPS):
        r, case = cpu_ratio(op)
        lines.append(f"  {op:26s} {r:10.3g}   at {S.case_id(case) if case is not None else '-'}")
    lines += ["", f"mutants on the CPU (best over their designated cases, up to the first bit-unequal one; must be >= {S.MUTANT_FACTOR:g})"]
    for op in sorted(S.OPS):
        for m in S.OPS[op].mutants:
            r, case = cpu_ratio(op, m)
            lines.append(f"  {op:18s} {m:38s} {r:10.3g}   at {S.case_id(case)}")
    lines += ["", NOTES.rstrip()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
