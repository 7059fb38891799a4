#!/usr/bin/env python3
"""Time per call of explain.input_attribution at the step's geometry -- full-depth encoders, B = 32, L = 128, F = 1 -- next to
what reaching the same layer cost before the data-gradient pass existed: forward_train + the full backward() (every weight
gradient) of the same shapes.  Writes profiles/token_explain_throughput.txt.

Device events around windows of >= 0.5 s after a warm-up of every shape; five windows per row, alternated over the rows; the
median and the spread are reported.

    token_explain_throughput.py [--layers N]       (--layers: a shallower rehearsal; the committed numbers are full depth)
"""
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import torch

from ultrafnd_git_amd.arena import FlatArena
from ultrafnd_git_amd.classifier import DeepTruthClassifier
from ultrafnd_git_amd.encoder_train import TextBackprop, VisualBackprop
from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
from ultrafnd_git_amd.explain import input_attribution
from ultrafnd_git_amd.fusion import CrossModalTransformer

DEV = torch.device("cuda", torch.cuda.current_device())
B, LQ, FR, STEPS, WINDOWS = 32, 128, 1, 16, 5
layers = int(sys.argv[sys.argv.index("--layers") + 1]) if "--layers" in sys.argv else 12
torch.manual_seed(0)
fusion, clf = CrossModalTransformer().to(DEV).eval(), DeepTruthClassifier().to(DEV).eval()


def encoders():
    return BertTextEncoder(layers=layers).to(DEV), ClipVisualEncoder(layers=layers).to(DEV)


tenc, venc = encoders()                     # frozen: the explanation's operand copies
tenc2, venc2 = encoders()                   # bound to an arena: the training step's forward_train + backward
bound = []
for cls, enc in ((TextBackprop, tenc2), (VisualBackprop, venc2)):
    bp = cls(enc)
    arena = FlatArena([list(g) for g in bp.groups()], [], DEV)
    bp.bind(arena, "")
    arena.ensure_grad()
    bound.append(bp)
tbp, vbp = bound
g = torch.Generator().manual_seed(1)
lens = torch.randint(16, LQ + 1, (B,), generator=g)
batch = {"input_ids": torch.randint(0, tenc.vocab, (B, LQ), generator=g).to(DEV),
         "attention_mask": (torch.arange(LQ)[None, :] < lens[:, None]).to(torch.int32).to(DEV),
         "frames": torch.randn(B, FR, 3, 224, 224, generator=g).to(DEV), "audio_features": torch.randn(B, 128, generator=g).to(DEV),
         "temporal_features": torch.randn(B, 256, generator=g).to(DEV), "gnn_feat": torch.randn(B, 128, generator=g).to(DEV),
         "aux": torch.rand(B, 2, generator=g).to(DEV)}
dt, dv = torch.randn(B, 768, generator=g).to(DEV), torch.randn(B, 512, generator=g).to(DEV)


def full_text():
    tbp.forward_train(batch["input_ids"], batch["attention_mask"])
    tbp.backward(dt)


def full_visual():
    vbp.forward_train(batch["frames"])
    vbp.backward(dv)


def data_text():
    tbp.forward_saved(batch["input_ids"], batch["attention_mask"])
    tbp.input_grad(dt)


def data_visual():
    vbp.forward_saved(batch["frames"])
    vbp.input_grad(dv)


ROWS = (("input_attribution grad_x_input (both encoders, head, reductions)", lambda: input_attribution(fusion, clf, tenc, venc, batch)),
        (f"input_attribution integrated_gradients, {STEPS} steps (+ the delta forward)",
         lambda: input_attribution(fusion, clf, tenc, venc, batch, method="integrated_gradients", steps=STEPS)),
        ("text: forward_saved + input_grad (data gradient only)", data_text),
        ("text: forward_train + backward (every weight gradient)", full_text),
        ("vision: forward_saved + input_grad (data gradient only)", data_visual),
        ("vision: forward_train + backward (every weight gradient)", full_visual))


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


calls = {}
for name, fn in ROWS:                       # warm-up of every shape, then the calls a 0.5 s window takes
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls[name] = max(3, int(0.5 / max(time.perf_counter() - t0, 1e-5)) + 1)
res = {name: [] for name, _ in ROWS}
for _ in range(WINDOWS):                    # alternated: every round times every row once
    for name, fn in ROWS:
        res[name].append(window(fn, calls[name]))
lines = [f"token / image-patch attribution, {layers}-layer encoders, B = {B}, L = {LQ}, F = {FR} on {torch.cuda.get_device_name(DEV)}",
         f"ms per call: median of {WINDOWS} alternated windows of >= 0.5 s (device events), [min .. max], calls per window"]
med = {}
for name, _ in ROWS:
    med[name] = statistics.median(res[name])
    lines.append(f"  {name}: {med[name]:.3f} ms [{min(res[name]):.3f} .. {max(res[name]):.3f}], {calls[name]} calls")
names = [n for n, _ in ROWS]
lines.append(f"  data-gradient pass / full backward: text {med[names[2]] / med[names[3]]:.2f}, vision {med[names[4]] / med[names[5]]:.2f}")
lines.append(f"  integrated_gradients ({STEPS} steps) / grad_x_input: {med[names[1]] / med[names[0]]:.2f}")
text = "\n".join(lines) + "\n"
print(text, end="")
if layers == 12:
    (REPO / "profiles" / "token_explain_throughput.txt").write_text(text)
