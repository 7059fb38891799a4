"""Which bf16 rounding of the trainable-encoder backward carries the error on the outlier-shaped 4-layer BERT (CPU only).

The text encoder's gradients through oracle/encoders_bf16.py with all rounding points active, with only the Linear GEMM operands
rounded, and with all active but one attention-internal point, each against the fp32 autograd of oracle/encoders_ref.py: the
relative L2 error of the query / key weight gradients (all layers together), the worst of them per tensor, and the worst tensor
overall; then each GEMM-operand point alone.  DESIGN.md section 9 holds the table for gains 5 and 20.

    python tests/encoder_bf16_ablation.py [--gain 20] [--gain 5]
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from oracle import encoders_bf16 as EB  # noqa: E402
from oracle import encoders_ref as E  # noqa: E402
from tests.helpers import grad_rel_errors, outlier_text_problem, qk_weight_rel_l2  # noqa: E402


def rows():
    yield "all points", EB.ALL
    yield "GEMM operands only", EB.GEMM_OPERANDS
    for p in EB.ATTENTION_INTERNAL:
        yield f"all but {p}", tuple(q for q in EB.ALL if q != p)
    yield "all but every attention-internal point", tuple(q for q in EB.ALL if q not in EB.ATTENTION_INTERNAL)
    for p in EB.GEMM_OPERANDS:
        yield f"{p} only", (p,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gain", type=float, action="append")
    gains = ap.parse_args().gain or [20.0, 5.0]
    for gain in gains:
        w, ids, mask, seed = outlier_text_problem(gain)
        _, ref = E.text_feature_grads(w, ids, mask, seed)
        print(f"gain {gain:g}")
        print(f"| rounding points | q/k weight grads, rel. L2 | worst q/k tensor | worst tensor (above floor) |")
        print("|---|---|---|---|")
        for name, pts in rows():
            _, got = EB.text_feature_grads(w, ids, mask, seed, points=pts)
            per, worst, wk = grad_rel_errors(got, ref)
            qk = {k: v[0] for k, v in per.items() if k.endswith(("query.weight", "key.weight"))}
            qk_worst = max(qk, key=qk.get)
            print(f"| {name} | {qk_weight_rel_l2(got, ref):.3g} | {qk[qk_worst]:.3g} ({qk_worst.replace('encoder.layer.', 'L')}) | "
                  f"{worst:.3g} ({wk.replace('encoder.layer.', 'L')}) |", flush=True)


if __name__ == "__main__":
    main()
