#!/usr/bin/env python3
"""Throughput of the audio encoder (ultrafnd_git_amd/audio.py) on one MI355X: one process, one GPU.

    audio_throughput.py                 clips/s and ms per call at B = 32 for 1-s and 5-s clips (12 layers), against, on the same
                                        device and the same weights, HF's Wav2Vec2Model at batch 1 in fp32 (the reference's call
                                        pattern, one clip per call) and HF's Wav2Vec2Model batched in bf16.  Device events
                                        around windows of >= 0.5 s after warm-up, three windows per path, alternated; median.
    audio_throughput.py --trace         a warmed pass of five native calls (B = 32, 5-s clips) for a run of its own under
                                        `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python ... --trace`
    audio_throughput.py --kernels CSV   read that run's kernel trace: time per stage of the LAST call, the conv stack's share,
                                        and the achieved fraction of the bf16 MFMA roof of conv layers 1-4

Run it under a `timeout`.  profiles/audio_encoder_throughput.txt holds the output of the three modes.

Dense-FLOP definition (conv layers 1-4): 2 * (B * S_out rows the launch computes) * 512 * 1536 per layer -- every row of the slab
is computed, valid or tail -- over the layer's kernel time, against 2.5 PFLOP/s dense bf16.  The useful share (valid frames only)
is printed beside it.
"""
import csv
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

B, LAYERS, SECONDS = 32, 12, (1, 5)
ROOF = 2.5e15
CONV_KERNELS, CONV_STRIDES = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)


def frames(n):
    out = []
    for k, s in zip(CONV_KERNELS, CONV_STRIDES):
        n = (n - k) // s + 1
        out.append(n)
    return out


def stage_of(names):
    """Stage of every kernel of ONE forward call, by its place in the launch sequence (audio.py: _run)."""
    out, gemm_seen, ln_seen = [], 0, 0
    for nm in names:
        if "frames_kernel" in nm:
            st = "frame counts / key mask"
        elif "wave_partials" in nm or "wave_apply" in nm:
            st = "wave normalise"
        elif "conv0_" in nm:
            st = "conv0 + GroupNorm + GELU"
        elif "pos_pack" in nm:
            st = "positional conv (pack, 16 GEMMs, add, LayerNorm)"
        elif "pos_add" in nm:
            st = "positional conv (pack, 16 GEMMs, add, LayerNorm)"
        elif "gemm_bf16_kernel" in nm:
            gemm_seen += 1
            if gemm_seen <= 4:
                st = "conv layers 1-4 (overlapping-row GEMM)"
            elif gemm_seen <= 6:
                st = "conv layers 5-6 (overlapping-row GEMM)"
            elif gemm_seen == 7:
                st = "feature projection (LayerNorm + GEMM)"
            elif gemm_seen <= 23:
                st = "positional conv (pack, 16 GEMMs, add, LayerNorm)"
            else:
                st = "encoder layers: GEMMs"
        elif "layernorm_kernel" in nm:
            ln_seen += 1
            if ln_seen == 1:
                st = "feature projection (LayerNorm + GEMM)"
            elif ln_seen == 2:
                st = "positional conv (pack, 16 GEMMs, add, LayerNorm)"
            else:
                st = "encoder layers: LayerNorms"
        elif "attention_kernel" in nm:
            st = "encoder layers: attention"
        elif "meanpool_kernel" in nm or "nt16_kernel" in nm:
            st = "mean-pool + projection"
        else:
            st = "other (torch / runtime)"
        out.append(st)
    return out


def kernels(path):
    rows = list(csv.DictReader(open(path)))
    key = {k.lower(): k for k in rows[0]}
    name, t0, t1 = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    rows.sort(key=lambda r: int(r[t0]))
    starts = [i for i, r in enumerate(rows) if "frames_kernel" in r[name]]
    if not starts:
        raise SystemExit("no audio forward call in this trace")
    call = rows[starts[-1]:]
    st = stage_of([r[name] for r in call])
    tot = {}
    for r, s in zip(call, st):
        tot[s] = tot.get(s, 0) + int(r[t1]) - int(r[t0])
    busy = sum(tot.values())
    wall = int(call[-1][t1]) - int(call[0][t0])
    n = 16000 * SECONDS[-1]
    T = frames(n)
    S1 = (T[0] + 63) // 64 * 64
    print(f"# last native call of the trace: B = {B}, {SECONDS[-1]}-s clips, {LAYERS} layers; {len(call)} kernels, kernel time {busy / 1e6:.3f} ms, "
          f"first start to last end {wall / 1e6:.3f} ms")
    for s, v in sorted(tot.items(), key=lambda kv: -kv[1]):
        print(f"  {s:52s} {v / 1e3:10.1f} us  {100.0 * v / busy:5.1f} %")
    conv = sum(v for s, v in tot.items() if s.startswith("conv"))
    print(f"conv stack (conv0 + layers 1-6): {100.0 * conv / busy:.1f} % of the call's kernel time")
    g = [int(r[t1]) - int(r[t0]) for r, s in zip(call, st) if s.startswith("conv layers 1-4")]
    dense = sum(2.0 * B * (S1 >> (i + 1)) * 512 * 1536 for i in range(4))
    useful = sum(2.0 * B * T[i + 1] * 512 * 1536 for i in range(4))
    print(f"conv layers 1-4: {sum(g) / 1e3:.1f} us for {dense / 1e9:.1f} dense GFLOP (2 x B S_out x 512 x 1536 per layer, every slab row) -> "
          f"{dense / (sum(g) * 1e-9) / 1e12:.0f} TFLOP/s = {dense / (sum(g) * 1e-9) / ROOF:.3f} of the 2.5 PFLOP/s dense bf16 MFMA roof "
          f"(valid frames only: {useful / 1e9:.1f} GFLOP, {useful / (sum(g) * 1e-9) / ROOF:.3f}); per layer us: {', '.join(f'{x / 1e3:.1f}' for x in g)}")


if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    kernels(sys.argv[2])
    sys.exit(0)

import torch

from ultrafnd_git_amd.audio import Wav2Vec2AudioEncoder

if not torch.cuda.is_available():
    raise SystemExit("audio_throughput.py: no HIP device (timings are taken on the GPU only)")
DEV = torch.device("cuda")


def clips(seconds):
    g = torch.Generator().manual_seed(seconds)
    return 0.1 * torch.randn(B, 16000 * seconds, generator=g)


def timed(fn, window_s=0.5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(2, int(window_s / max(time.perf_counter() - t0, 1e-5)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


enc = Wav2Vec2AudioEncoder(layers=LAYERS).to(DEV)

if "--trace" in sys.argv:
    x = clips(SECONDS[-1]).to(DEV)
    for _ in range(5):
        enc(x)
    torch.cuda.synchronize()
    sys.exit(0)

from transformers import Wav2Vec2Config, Wav2Vec2Model

cfg = Wav2Vec2Config(num_hidden_layers=LAYERS)
sd = {k: v for k, v in enc.state_dict().items() if not k.startswith("proj.")}
hf32 = Wav2Vec2Model(cfg).eval()
hf32.load_state_dict(sd, strict=False)
hf32 = hf32.to(DEV)
hf16 = Wav2Vec2Model(cfg).eval()
hf16.load_state_dict(sd, strict=False)
hf16 = hf16.to(DEV, torch.bfloat16)
proj_w, proj_b = enc.state_dict()["proj.weight"].to(DEV), enc.state_dict()["proj.bias"].to(DEV)
prop = torch.cuda.get_device_properties(0)
print(f"# tools/audio_throughput.py on one {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}: B = {B}, {LAYERS} layers, seeded weights; "
      "device events over windows of >= 0.5 s after warm-up, three windows per path (alternated), median.  Clips are device-resident; "
      "the HF paths get clips normalised beforehand (their normalisation runs on the CPU in the reference and is not timed).")


def normed(x):
    return (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-7)


with torch.no_grad():
    for sec in SECONDS:
        x = clips(sec).to(DEV)
        xn = normed(x)
        xn16 = xn.to(torch.bfloat16)

        def native():
            return enc(x)

        def hf_batch1():      # the reference's call pattern: one clip per forward, mean over time, projection
            return [torch.addmm(proj_b, hf32(xn[i:i + 1]).last_hidden_state.mean(dim=1), proj_w.T) for i in range(B)]

        def hf_bf16():
            return torch.addmm(proj_b, hf16(xn16).last_hidden_state.float().mean(dim=1), proj_w.T)

        a, r1, r16 = native().clone(), torch.cat(hf_batch1()), hf_bf16()
        print(f"{sec}-s clips: features native vs HF fp32 batch-1 max-abs {float((a - r1).abs().max()):.2e} (|feature| max {float(r1.abs().max()):.2f}); "
              f"HF bf16 batched vs HF fp32 {float((r16 - r1).abs().max()):.2e}")
        paths = (("native Wav2Vec2AudioEncoder (incl. normalisation, pool, projection)", native), ("HF Wav2Vec2Model fp32, batch 1 x 32", hf_batch1),
                 ("HF Wav2Vec2Model bf16, one batch of 32", hf_bf16))
        res = {nm: [] for nm, _ in paths}
        for _ in range(3):
            for nm, fn in paths:
                res[nm].append(timed(fn))
        for nm, _ in paths:
            ms = [m for m, _ in res[nm]]
            med = statistics.median(ms)
            print(f"{sec}-s clips, B={B}: {nm}: {med:.2f} ms per {B} clips = {B / med * 1e3:.0f} clips/s = {B * sec / med * 1e3:.0f} s of audio per s "
                  f"(three windows: {', '.join(f'{m:.2f}' for m in ms)}; {res[nm][0][1]} calls per window)", flush=True)
