#!/usr/bin/env python3
"""In-kernel phase times of the fused projection + attention kernel over sample tiles (diagnostics library, GPU box), for a bench
group of 128 samples (lengths uniform in [16, 128]): median over workgroups and launches of prologue (entry -> first K-step landed),
K loop, projection epilogue (-> LDS images), attention (-> end), in us of s_memrealtime (100 MHz); the slowest workgroup's attention
and the launch span.   usage: text_tile_stamps.py [--ln] [--seed N]"""
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import torch

from _diaglib import check as dcheck, diag
from ultrafnd_git_amd import _lib as L
from ultrafnd_git_amd.encoders import TEXT_TILE_INTS, text_tiles

dev = "cuda"
B, heads, H = 128, 12, 768
seed = int(sys.argv[sys.argv.index("--seed") + 1]) if "--seed" in sys.argv else 0
g = torch.Generator().manual_seed(seed)
lens = torch.randint(16, 129, (B,), generator=g)
mask = (torch.arange(128)[None] < lens[:, None]).to(torch.int32).to(dev)
x = torch.randn(B * 128, H, generator=g).to(dev)
W = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(dev).bfloat16()
bias = torch.randn(3 * H, generator=g).to(dev)
ctx = torch.empty(B * 128, H, dtype=torch.bfloat16, device=dev)
i32 = dict(dtype=torch.int32, device=dev)
cu, row_src = torch.zeros(B + 1, **i32), torch.zeros(B * 128, **i32)
tiles, ntiles = torch.zeros((B + 1) // 2, TEXT_TILE_INTS, **i32), torch.zeros(1, **i32)
s = L.stream_ptr(torch.device(dev))
L.check(L.lib().ufnd_text_pack_tiles(mask.data_ptr(), B, 128, cu.data_ptr(), row_src.data_ptr(), tiles.data_ptr(), ntiles.data_ptr(), None, None, s),
        "ufnd_text_pack_tiles")
torch.cuda.synchronize()
nt = int(ntiles.item())
assert nt == len(text_tiles(lens.tolist()))
ln = None
if "--ln" in sys.argv:
    xs = x.view(B * 128, 24, 32)
    st = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).contiguous()
    cs = W.float().sum(1).contiguous()
    ln = L.GemmLn()
    ln.a_stats, ln.colsum, ln.a_parts, ln.a_eps, ln.r_eps, ln.width = st.data_ptr(), cs.data_ptr(), 24, 1e-12, 1e-12, H
ngrid, nblk = tiles.shape[0] * heads, nt * heads
xs_rot = [x.bfloat16().clone() for _ in range(8)]
rows = []
for it in range(16):
    stt = torch.zeros(ngrid, 10, dtype=torch.int64, device=dev)
    dcheck(diag().ufnd_diag_qkv_attention_tiles_stamps(xs_rot[it % 8].data_ptr(), W.data_ptr(), bias.data_ptr(), tiles.data_ptr(), ntiles.data_ptr(),
                                                       ctx.data_ptr(), tiles.shape[0], heads, C.byref(ln) if ln is not None else None, stt.data_ptr(), s),
           "stamps")
    torch.cuda.synchronize()
    if it >= 4:
        rows.append(stt[:nblk].clone())      # (the first nt * heads workgroups of the grid are the live ones)
st_ = torch.stack(rows).double()             # (launch, block, 10)
rt = st_[..., 1::2] * 0.01                   # realtime, us: entry, first landed, loop done, end, epilogue done
pro = (rt[..., 1] - rt[..., 0]).median().item()
loop = (rt[..., 2] - rt[..., 1]).median().item()
epi = (rt[..., 4] - rt[..., 2]).median().item()
att = rt[..., 3] - rt[..., 4]
tot = rt[..., 3] - rt[..., 0]
span = (rt[..., 3].max(dim=1).values - rt[..., 0].min(dim=1).values).median().item()
units = tiles[:nt, 2].float()
print(f"fused projection + attention over sample tiles, {B} samples, {int(lens.sum())} live rows, {nt} tiles x {heads} heads = {nblk} workgroups"
      f"{' LN-folded' if ln is not None else ''} ({units.mean().item():.1f} units per tile, at most {int(units.max().item())}): per workgroup "
      f"prologue {pro:.2f} us, K loop {loop:.2f} us, projection epilogue {epi:.2f} us, attention + store {att.median().item():.2f} us "
      f"(slowest {att.max().item():.2f}), total {tot.median().item():.2f} us (slowest {tot.max().item():.2f}); "
      f"launch span (first entry -> last end) {span:.2f} us")
