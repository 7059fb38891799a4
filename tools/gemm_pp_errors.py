"""The record of tests/gemm_pp_cases.py (the persistent bf16 GEMM, tile id 64): per case the worst |error| / bound of the float32
restatement on the CPU (cases of at most 15 tiles) and the error / bound every mutant reaches, and -- with --log, from the MI355X -- the
figures tests/test_gpu_gemm_pp_cases.py printed for the kernel itself: the worst ratio of each case over its two launches, the count of
unequal elements in the exact family and whether the two launches left the same bits.

    python tools/gemm_pp_errors.py [--log pytest.log] [--out profiles/gemm_pp_errors.txt]

--log takes the output of `pytest tests/test_gpu_gemm_pp_cases.py -m gpu -s`.  Without it the kernel lines are left out: nothing
measured on a CPU is ever written under a GPU heading.  Nothing is asserted from this record."""
from __future__ import annotations

import argparse
import re
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests import gemm_bf16_cases as G  # noqa: E402
from tests import gemm_pp_cases as P  # noqa: E402


def _line(cid, r, key, ne, extra=""):
    return f"  {cid:72s} {r:10.3g} ({key})" + ("" if ne is None else f"   unequal {ne}") + extra


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["worst |error| / bound per case of the persistent bf16 GEMM (table: tests/gemm_pp_cases.py; bounds and data families:",
             "tests/gemm_bf16_cases.py; 0 = bit-equal where the bound is 0, inf = a bit differs there or a sentinel was overwritten; the bf16",
             "output's figure is the fraction of the fp32 bound needed to explain the stored value)", ""]
    if a.log:
        text = Path(a.log).read_text().splitlines()
        pat = re.compile(r"^\.?(\S+): worst error / bound (\S+) \((\w+)\)(?:; unequal elements (\d+))?; runs bit-equal (\w+)")
        seen = {}
        for ln in text:
            m = pat.match(ln)
            if m:
                seen[m.group(1)] = (float(m.group(2)), m.group(3), None if m.group(4) is None else int(m.group(4)), m.group(5))
        ids = [c.id for c in P.CASES] + [lc.id for lc in P.LIVE_CASES]
        assert set(ids) <= set(seen), "the log does not hold every case"
        cus = next((ln.lstrip(".") for ln in text if "CUs: coverage gaps" in ln), "")
        lines.append("kernel on the GPU (MI355X; the figures tests/test_gpu_gemm_pp_cases.py printed: two launches per case on fresh buffers)")
        lines += [_line(i, *seen[i][:3], extra=f"   runs bit-equal {seen[i][3]}") for i in ids]
        lines += ["", f"  cases with unequal elements: {sum(1 for i in ids if seen[i][2])} of {sum(1 for i in ids if seen[i][2] is not None)} bit-exact ones",
                  f"  cases whose two launches differ: {sum(1 for i in ids if seen[i][3] != 'True')}", f"  worst ratio: {max(seen[i][0] for i in ids):.3g}",
                  f"  {cus}", ""]
        lines.append("tile counts per workgroup the stamps build reported against the host mirror of the walk")
        lines += ["  " + ln.lstrip(".") for ln in text if "workgroups that differ" in ln and "print" not in ln] + [""]
    lines.append("float32 restatement on the CPU, stored along the walk of 256 CUs, two summation orders (must be <= 1; cases of at most 15 tiles)")
    for c in P.SMALL:
        inp = P.make(c)
        refs = P.reference(c, inp)
        best = (-1.0, "", None)
        for order in (0, 1):
            got = P.emulate_pp(c, inp, order)
            ratios = P.check(c, inp, got, refs)
            key = max(ratios, key=lambda k: ratios[k])
            if ratios[key] > best[0]:
                best = (ratios[key], key, P.unequal(c, got, refs) if P.is_bit_exact(c) else None)
        lines.append(_line(c.id, *best))
    lines += ["", f"mutants on the CPU, the worst error / bound over the cases of at most 15 tiles (inf on a bit-exact case, >= {G.MUTANT_FACTOR:g} otherwise)"]
    from tests.test_gemm_pp_cases import KILLERS
    for m in P.MUTANTS:
        worst = (0.0, "-")
        if m in KILLERS:
            for c in P.SMALL:
                if KILLERS[m](c):
                    inp = P.make(c)
                    worst = max(worst, (max(P.check(c, inp, P.emulate_pp(c, inp, 0, m)).values()), c.id))
        else:
            for lc in P.LIVE_CASES:
                if lc.case.guard != "no" and lc.live % P.BM:
                    inp = P.make_live(lc, P.make(lc.case))
                    worst = max(worst, (max(P.check_live(lc, inp, P.emulate_pp(lc.case, inp, 0, m, live_rows=lc.m_live), 256).values()), lc.id))
        lines.append(f"  {m:48s} {worst[0]:10.3g}   at {worst[1]}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
