#!/usr/bin/env python3
"""Time per call of the explanation paths at B = 256 (device events, warm-up, windows of >= 0.5 s), and the design question
behind explain_shap: the 16 gradients of the smooth-grad walk as ONE 4,096-row ufnd_classifier_input_grad call against 16
sequential 256-row calls of the same entry, alternated in the same process.

    explain_throughput.py                      timings (three rounds of every measurement, alternated)
    explain_throughput.py --trace              one pass for `rocprofv3 --kernel-trace --output-format csv -d DIR -- python ... --trace`:
                                               each path once, separated by a sentinel launch (step_advance_kernel)
    explain_throughput.py --launches TRACE.csv launches per call from that run's *_kernel_trace.csv
"""
import csv
import ctypes as C
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

SENTINEL = "step_advance_kernel"
PHASES = ("feature_importance (B=256)", "explain_shap (B=256 -> 4,096 rows; incl. its torch plumbing: padded copies, std, randn, D2H)",
          "modality_attribution (B=256; incl. torch's row sums and stack)", "ufnd_classifier_input_grad, 4,096 rows in one call",
          "ufnd_classifier_input_grad, 16 calls of 256 rows")


def launches(path: str) -> None:
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seg, segs = [], []
    for r in rows:
        if SENTINEL in r["Kernel_Name"]:
            segs.append(seg)
            seg = []
        else:
            seg.append(r["Kernel_Name"])
    for name, s in zip(PHASES, segs[1:]):          # (segs[0]: set-up and warm-up)
        other = sum(1 for k in s if "at::" in k or "rocclr" in k)      # torch's own kernels and the runtime's buffer copies
        print(f"launches per call: {name}: {len(s)} ({len(s) - other} of this library, {other} of torch and the runtime's copies)")


if len(sys.argv) > 2 and sys.argv[1] == "--launches":
    launches(sys.argv[2])
    sys.exit(0)

import torch

from ultrafnd_git_amd import _lib as L
from ultrafnd_git_amd.classifier import DeepTruthClassifier
from ultrafnd_git_amd.explain import modality_attribution
from ultrafnd_git_amd.fusion import CrossModalTransformer
from ultrafnd_git_amd.state import StepStateBuffer

DEV = torch.device("cuda")
B, N = 256, 16
torch.manual_seed(0)
fusion, clf = CrossModalTransformer().to(DEV).eval(), DeepTruthClassifier().to(DEV).eval()
feats = {"text_features": torch.randn(B, 768, device=DEV), "audio_features": torch.randn(B, 128, device=DEV),
         "visual_features": torch.randn(B, 512, device=DEV), "temporal_features": torch.randn(B, 256, device=DEV),
         "gnn_feat": torch.randn(B, 128, device=DEV)}
aux = torch.rand(B, 2, device=DEV)
with torch.no_grad():
    fused = fusion(feats)["fused"]
noise = torch.randn(N, B, 514, device=DEV)

# the walk's 4,096 rows as plain tensors, for the batched-against-sequential comparison on the entry itself
d, s = clf.dims(), L.stream_ptr(DEV)
X = torch.cat([fused, aux], dim=1)
sigma = 0.1 * X.std(dim=0).clamp_min(1e-6)
pts = [X]
for i in range(N - 1):
    pts.append(pts[-1] + noise[i] * sigma)
P = torch.stack(pts).reshape(N * B, 514)
PF, PA = P[:, :512].contiguous(), P[:, 512:].contiguous()
ws_all = torch.empty(L.lib().ufnd_clf_workspace_floats(C.byref(d), N * B), dtype=torch.float32, device=DEV)
ws_one = torch.empty(L.lib().ufnd_clf_workspace_floats(C.byref(d), B), dtype=torch.float32, device=DEV)
gx = torch.empty(N * B, 516, device=DEV)
lg, pr = torch.empty(N * B, 2, device=DEV), torch.empty(N * B, 2, device=DEV)
state = StepStateBuffer(DEV)
sentinel_state = StepStateBuffer(DEV)


def input_grad(ws, row0, rows):
    L.check(L.lib().ufnd_classifier_input_grad(C.byref(d), C.byref(clf.param_table()), PF[row0:].data_ptr(), 512, PA[row0:].data_ptr(), rows, 0,
                                               L.TARGET_PROB, 1, ws.data_ptr(), gx[row0:].data_ptr(), 516, lg[row0:].data_ptr(), pr[row0:].data_ptr(),
                                               state.ptr, s), "ufnd_classifier_input_grad")


def batched():
    input_grad(ws_all, 0, N * B)


def sequential():
    for i in range(N):
        input_grad(ws_one, i * B, B)


PATHS = (lambda: clf.feature_importance(fused, aux), lambda: clf.explain_shap(fused, aux, noise=noise),
         lambda: modality_attribution(fusion, clf, feats, aux), batched, sequential)

batched()
g_b = gx.clone()
sequential()
print(f"batched vs sequential gradients: max-abs difference {(g_b - gx).abs().max().item():.2e}")

if "--trace" in sys.argv:
    for fn in PATHS:
        fn()
    torch.cuda.synchronize()
    for fn in PATHS:
        sentinel_state.advance()
        fn()
        torch.cuda.synchronize()
    sentinel_state.advance()
    torch.cuda.synchronize()
    sys.exit(0)


def timed(fn, window_s=0.5):
    """ms per call over a window of at least `window_s` seconds (device events around the whole window)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(5, int(window_s / max(time.perf_counter() - t0, 1e-5)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


res = {name: [] for name in PHASES}
for rnd in range(3):                       # alternated: every round times every path once
    for name, fn in zip(PHASES, PATHS):
        res[name].append(timed(fn))
for name in PHASES:
    ms = [m for m, _ in res[name]]
    print(f"{name}: {min(ms) * 1e3:.1f} us per call (three windows: {', '.join(f'{m * 1e3:.1f}' for m in ms)}; {res[name][0][1]} calls per window)")
b, q = min(m for m, _ in res[PHASES[3]]), min(m for m, _ in res[PHASES[4]])
print(f"16 gradients of 256 rows: batched {b * 1e3:.1f} us, sequential {q * 1e3:.1f} us -> batched / sequential = {b / q:.2f}")
