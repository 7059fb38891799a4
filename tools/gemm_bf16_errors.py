"""The record of tests/gemm_bf16_cases.py: per case the worst |error| / bound of the float32 restatement on the CPU (and, for the exact
family, the count of unequal elements), the error / bound every mutant reaches on the case that kills it, and -- with --gpu, on the
MI355X -- the same two figures of the kernel itself.

    python tools/gemm_bf16_errors.py [--gpu | --log pytest.log] [--out profiles/gemm_bf16_errors.txt]

--log collects the ratios that `pytest tests/test_gpu_gemm_bf16.py -m gpu -s` printed on the MI355X instead of launching again.
Without --gpu or --log the kernel lines are left out: nothing measured on a CPU is ever written under a GPU heading."""
from __future__ import annotations

import argparse
import re
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from tests import gemm_bf16_cases as G  # noqa: E402


def _line(c, r, key, ne):
    return f"  {c.id:62s} {r:10.3g} ({key})" + ("" if ne is None else f"   unequal {ne}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--log", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["worst |error| / bound per case (bounds and data families: tests/gemm_bf16_cases.py; 0 = bit-equal where the bound is 0, inf = a bit",
             "differs there or a sentinel was overwritten; the bf16 output's figure is the fraction of the fp32 bound needed to explain the stored value)", ""]
    if a.gpu:
        import torch
        from tests import test_gpu_gemm_bf16 as T
        prop = torch.cuda.get_device_properties(0)
        lines.append(f"kernel on the GPU ({prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs)")
        worst = {}
        for c in G.CASES:
            r, key, ne = T.measure(c)
            lines.append(_line(c, r, key, ne))
            fam = (c.family, c.entry if c.ln == "none" else c.ln)
            if not c.refuse and r >= worst.get(fam, (-1.0, ""))[0]:
                worst[fam] = (r, c.id)
        lines += ["", "  worst per (family, form):"] + [f"    {f[0]:8s} {f[1]:6s} {r:10.3g}   {cid}" for f, (r, cid) in sorted(worst.items())]
        lines.append("")
    if a.log:
        pat = re.compile(r"^\.?(\S+): worst error / bound (\S+) \((\w+)\)(?:; unequal elements (\d+))?")
        seen = {}
        for ln in Path(a.log).read_text().splitlines():
            m = pat.match(ln)
            if m and m.group(1) in G.BY_ID:
                seen[m.group(1)] = (float(m.group(2)), m.group(3), None if m.group(4) is None else int(m.group(4)))
        assert set(seen) == set(G.BY_ID), "the log does not hold every case"
        lines.append("kernel on the GPU (MI355X; the figures tests/test_gpu_gemm_bf16.py printed, one launch per case)")
        lines += [_line(c, *seen[c.id]) for c in G.CASES]
        live = [c for c in G.CASES if not c.refuse]
        lines += ["", f"  exact cases with unequal elements: {sum(1 for c in live if seen[c.id][2])} of {sum(1 for c in live if seen[c.id][2] is not None)}",
                  f"  worst ratio: {max(seen[c.id][0] for c in live):.3g}", ""]
    lines.append("float32 restatement on the CPU, two summation orders (must be <= 1; cases above 1,100 rows: one order)")
    for c in G.CASES:
        if c.refuse:
            continue
        inp = G.make(c)
        refs = G.reference(c, inp)
        best = (-1.0, "", None)
        for order in ((0, 1) if c.M <= 1100 else (1,)):
            got = G.emulate(c, inp, order)
            ratios = G.check(c, inp, got, refs)
            key = max(ratios, key=lambda k: ratios[k])
            if ratios[key] > best[0]:
                best = (ratios[key], key, G.unequal(c, got, refs) if G.is_bit_exact(c) else None)
        lines.append(_line(c, *best))
    lines += ["", f"mutants on the CPU, each on the case that kills it (must be inf on a bit-exact case, >= {G.MUTANT_FACTOR:g} otherwise)"]
    for m in G.MUTANTS:
        c = G.BY_ID[G.KILLS[m]]
        inp = G.make(c)
        r = max(G.check(c, inp, G.emulate(c, inp, 0, m)).values())
        lines.append(f"  {m:34s} {r:10.3g}   at {c.id}")
    m = G.measure_act_errors()
    lines += ["", "float32 restatements of the activation functions against float64 over |x| <= %g (ACT_ABS / GRAD_ABS of the bounds)" % G.ACT_RANGE,
              f"  gelu_fast {m[G.ACT_GELU]:.3g}   quick_gelu_fast {m[G.ACT_QUICK_GELU]:.3g}   gelu_grad {m[G.ACT_GELU_BWD]:.3g}   quick_gelu_grad {m[G.ACT_QUICK_GELU_BWD]:.3g}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
