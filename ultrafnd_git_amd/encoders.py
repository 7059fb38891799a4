"""Frozen, forward-only encoders that produce the `text` (B,768) and `visual` (B,512) inputs of
the fusion step, MI355X-native.

  BertTextEncoder   replaces BERTContextEncoder.encode's model call + pooling
                    (src/core_blocks/text_blocks.py:71-101): BertModel(...).last_hidden_state
                    -> masked mean-pool -> L2-norm, batched over (B, L) instead of one
                    string at a time.  Tokenisation stays outside (ids/mask in), there is
                    no tokenizer vocabulary offline.
  ClipVisualEncoder the ViT-B/32 @224 geometry the reference points at
                    (configs/model_configs/semantic.yaml:2): pooled -> bias-free projection ->
                    L2-norm; multi-frame = mean over frames, L2-norm again
                    (text_blocks.py:126-128 idiom).

Weights keep the third-party `state_dict` names so real checkpoints load unchanged; fp32
masters are converted once to bf16 MFMA operands (Q/K/V stacked into one (3H,H) matrix).
Every Linear is `ufnd_gemm_bf16` with fused bias / GELU / residual epilogues; the residual
stream and all LayerNorm / softmax statistics stay fp32.  No CPU path.

LayerNorm folding (`fold_ln=True`, the default): no LayerNorm kernel runs between two Linears.
The GEMM that produces a residual-stream row also writes its bf16 rounding and partial
{sum, sum of squares}; the Linear that consumes LayerNorm(row) multiplies the UN-normalised bf16
row by W * gamma and applies  rstd (acc - mean colsum) + (b + W beta)  in its epilogue
(`ufnd_gemm_bf16_ln`); BERT's post-LN residual LayerNorm(row) * gamma + beta is evaluated on the fly
in the epilogue of the GEMM that adds it.  `fold_ln=False` keeps one LayerNorm kernel per LayerNorm.

Residual stream dtype (`residual_dtype`, folded encoders only).  "fp32": the stream is kept in fp32 next to the bf16
rounding the consumers read -- a residual GEMM moves 4 B in and 4 + 2 B out per element.  "bf16" (default): the rounding IS the stream
-- the residual operand is the bf16 copy the previous GEMM wrote for its consumer, no fp32 copy is written (except by the last
layer, for the final LayerNorm), 2 B in and 2 B out per element: 125 -> 53 MB per out-projection launch at 16,384 rows.  The
stream then carries 8 significant bits per layer; row statistics are still taken from the fp32 sums before rounding.
Measured at BASELINE's sizes (tests/test_gpu_fullsize.py): BERT features 9.9e-4 max-abs against 1.1e-3 with the fp32 stream,
hidden states 9.3e-3 against 8.7e-3 relative RMS after 12 layers; ViT (pre-LN: the stream is never re-normalised) features
7.4e-4 against 5.8e-4, hidden 8.7e-3 against 5.4e-3; end-to-end logits 3.2e-5 against 2.7e-5 (bound 1e-3) -- for
out-projection launches 49 -> 31 us and FFN2 100 -> 83 us at 16,384 rows, the step +7 %.
"""
from __future__ import annotations

import ctypes
import warnings
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L

ACT_NONE, ACT_GELU, ACT_QUICK_GELU = 0, 1, 2


def _bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 device tensor -> bf16 copy through the library's own cast kernel."""
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    L.check(L.lib().ufnd_cast_bf16(t.data_ptr(), out.data_ptr(), t.numel(), L.stream_ptr(t.device)), "ufnd_cast_bf16")
    return out


def dropout_prob(name: str, p) -> float:
    """A dropout probability of the trainable encoders (HF config names), refused by name outside [0, 1)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name}={p!r}: a dropout probability in [0, 1)")
    return p


def text_slot_bins(n_rows) -> list:
    """The slot bins ufnd_text_pack_bins computes on the device, from the per-sample row counts n_b (1 + the last kept position,
    0 for an all-masked sample; n_b <= 128): a list of bins, each four slots (b, s) -- slot s of sample b -- or None (empty).
    Sample b takes ceil(n_b / 32) contiguous slots.  Full bins first: [4], [3 + 1], [2 + 2], [the odd 2 + 1 + 1], [1 x 4]; then
    the partial ones: [3 alone], [the odd 2 (+ 1)], [the last 1-3 1-slot samples]; samples in ascending order within a class."""
    cls = {c: [b for b, n in enumerate(n_rows) if (int(n) + 31) // 32 == c] for c in (1, 2, 3, 4)}
    one, two, three = cls[1], cls[2], cls[3]
    p = min(len(one), len(three))
    ones = one[p:]
    u = min(2, len(ones)) if len(two) % 2 else 0
    slots = lambda *bs: [(b, s) for b in bs for s in range((int(n_rows[b]) + 31) // 32)]
    full = [slots(b) for b in cls[4]] + [slots(three[k], one[k]) for k in range(p)]
    full += [slots(two[k], two[k + 1]) for k in range(0, len(two) - 1, 2)]
    odd = slots(two[-1], *ones[:u]) if len(two) % 2 else None
    rest = ones[u:]
    if odd is not None and u == 2:
        full.append(odd)
    full += [slots(*rest[k:k + 4]) for k in range(0, len(rest) - len(rest) % 4, 4)]
    part = [slots(b) for b in three[p:]]
    if odd is not None and u < 2:
        part.append(odd)
    if len(rest) % 4:
        part.append(slots(*rest[len(rest) - len(rest) % 4:]))
    return [x + [None] * (4 - len(x)) for x in full + part]


def text_slot_bin_count(n_rows) -> int:
    """len(text_slot_bins(n_rows)): the workgroup rows the fused Q/K/V + attention runs over slot bins."""
    return len(text_slot_bins(n_rows))


SUPPORTED_HIDDEN = (256, 512, 768, 1024)      # the widths the row kernels are instantiated for (csrc/rowwise.hpp: h_ok, NI_LAUNCH)
MAX_PROJECTION = 1024                         # ufnd_l2norm_frames' widest row


def check_geometry(hidden=None, heads=None, intermediate=None, projection_dim=None) -> None:
    """The frozen encoders' constructor arguments against what their kernels are built for, each given as (argument name, value):
    a ValueError that names the argument and the supported values, instead of a C-ABI refusal at the first launch (DESIGN.md's
    geometry table).  heads is checked against hidden: the attention kernels are built for a head dimension of 64."""
    if hidden is not None and hidden[1] not in SUPPORTED_HIDDEN:
        raise ValueError(f"{hidden[0]}={hidden[1]!r}: one of {SUPPORTED_HIDDEN}, the widths the row kernels are built for")
    if heads is not None and hidden[1] != heads[1] * 64:
        raise ValueError(f"{heads[0]}={heads[1]!r}: {hidden[0]} // 64 = {hidden[1] // 64}, head_dim must be 64 ({hidden[0]} == {heads[0]} * 64)")
    if intermediate is not None and (intermediate[1] < 64 or intermediate[1] % 64):
        raise ValueError(f"{intermediate[0]}={intermediate[1]!r}: a positive multiple of 64 (the bf16 GEMM's N and K)")
    if projection_dim is not None and (projection_dim[1] < 64 or projection_dim[1] % 64 or projection_dim[1] > MAX_PROJECTION):
        raise ValueError(f"{projection_dim[0]}={projection_dim[1]!r}: a multiple of 64 from 64 to {MAX_PROJECTION} (the projection GEMM's N; "
                         "the L2 normalisation's widest row)")


TEXT_TILE_ROWS, TEXT_TILE_SAMPLES, TEXT_TILE_MAX_B = 256, 16, 512      # ufnd_text_pack_tiles (UFND_TEXT_TILE_*)
TEXT_TILE_INTS, TEXT_TILE_UNIT0, TEXT_TILE_ROWMAP, TEXT_TILE_KBIAS = 576, 36, 64, 320


def text_tiles(n_rows) -> list:
    """The sample tiles ufnd_text_pack_tiles computes on the device, from the per-sample row counts n_b (n_b <= 128): a list of tiles,
    each a list of (b, r0) -- sample b's rows 0 .. n_b - 1 are tile rows r0 .. r0 + n_b - 1 -- in placement order.  First-fit-decreasing:
    samples in descending n_b (ties: ascending b) go to the first tile with n_b of its 256 rows free and fewer than 16 samples; samples
    with n_b = 0 take no rows.  The 16-sample cap can only bind where samples of fewer than 16 rows meet (17 samples of 16 rows or more
    do not fit 256 rows): for longer samples this IS first-fit-decreasing."""
    tiles, used = [], []
    for b in sorted((b for b, n in enumerate(n_rows) if int(n) > 0), key=lambda b: (-int(n_rows[b]), b)):
        n = int(n_rows[b])
        if n > 128:
            raise ValueError(f"text_tiles: n_b={n} (samples of at most 128 rows)")
        for t, u in enumerate(used):
            if u + n <= TEXT_TILE_ROWS and len(tiles[t]) < TEXT_TILE_SAMPLES:
                break
        else:
            t = len(tiles)
            tiles.append([])
            used.append(0)
        tiles[t].append((b, used[t]))
        used[t] += n
    return tiles


def text_tile_count(n_rows) -> int:
    """len(text_tiles(n_rows)): the workgroup rows the fused Q/K/V + attention runs over sample tiles."""
    return len(text_tiles(n_rows))


class _EncoderBase(nn.Module):
    """Weight store with third-party key names + lazily packed bf16 operands + per-shape buffers."""

    # Largest |mean| / std of a row whose LayerNorm may be folded into the next GEMM.  Folding rounds the UN-normalised
    # row to bf16, so its error relative to the normalised output is about (1 + |mean|/std) * 2^-9: at 4 it is still
    # below the bf16 floor of the materialised path; beyond, the encoder falls back to one LayerNorm kernel per LayerNorm.
    FOLD_GUARD_MAX = 4.0

    def __init__(self, hidden: int, heads: int, fold_ln: bool, residual_dtype: str):
        super().__init__()
        if residual_dtype not in ("fp32", "bf16"):
            raise ValueError(f"residual_dtype={residual_dtype!r}: 'fp32' or 'bf16'")
        if hidden != heads * 64:
            raise ValueError("head_dim must be 64 (hidden == heads * 64)")
        self.hidden, self.heads, self.fold_ln, self.residual_dtype = hidden, heads, fold_ln, residual_dtype
        # GEMM tile per Linear ("qkv", "out", "ffn1", "ffn2"): -1 = the library's own choice for the shape.  Set by the
        # trainer when the encoder runs on a compute-unit partition (a launch wants about one tile per CU it may use).
        self.tiles: Dict[str, int] = {}
        # ... and the tiles a pass chose for its own live-row launches (BertTextEncoder.live_tiles), which `tiles` overrides
        self._live_tiles: Dict[str, int] = {}
        self._guard: Optional[torch.Tensor] = None      # device float: largest |mean| / std any folded LayerNorm has seen
        self._w: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self._packed: Optional[dict] = None
        self._layer_keys: Dict[int, dict] = {}
        self._bufs: Dict[Tuple, dict] = {}
        self.weights_version = 0      # bumped whenever the packed operands are invalidated (captured graphs name them)

    @staticmethod
    def _seeded_init():
        """init(shape, std=0.02): the constructors' placeholder weights, drawn in call order from one generator seeded with 0."""
        g = torch.Generator().manual_seed(0)

        def init(shape, std=0.02):
            return torch.randn(shape, generator=g) * std
        return init

    # ---- the layer table: the third-party names of a layer's tensors, and the operands packed from them
    LAYER_PREFIX: str                  # "...{}." : the prefix of layer i's keys
    LAYER_NAMES: Dict[str, list]       # name -> the key suffixes behind it

    def layer_keys(self, i: int) -> Dict[str, list]:
        """The state_dict keys of layer i: qkv_w / qkv_b (query, key, value: stacked row-wise into one Linear), o_w / o_b, w1 / b1, w2 / b2
        (the four Linears) and g1 / b1n, g2 / b2n (the two LayerNorms, in the order they run), each a list of keys.  Built once per
        layer: a pass that formats a dozen strings per layer pays for them in host time."""
        k = self._layer_keys.get(i)
        if k is None:
            P = self.LAYER_PREFIX.format(i)
            k = self._layer_keys[i] = {name: [P + sfx for sfx in sfxs] for name, sfxs in self.LAYER_NAMES.items()}
        return k

    def _pack_layers(self, extra=None) -> list:
        """The layers' operands: bf16 MFMA weights (Q/K/V stacked into one (3H, H) matrix), fp32 biases and LayerNorm parameters.
        extra(layers, wq, w1): called per layer, right after layers[-1] is built, with the fp32 stacked Q/K/V weight and FFN1 weight
        while they are at hand -- where BERT and the ViT add their folded forms on top."""
        w, layers = self._w, []
        for i in range(self.layers):
            k = self.layer_keys(i)
            wq = torch.cat([w[n] for n in k["qkv_w"]], 0)
            layers.append({"wqkv": _bf16(wq), "bqkv": torch.cat([w[n] for n in k["qkv_b"]], 0).contiguous(),
                           "wo": _bf16(w[k["o_w"][0]]), "bo": w[k["o_b"][0]], "g1": w[k["g1"][0]], "b1": w[k["b1n"][0]],
                           "w1": _bf16(w[k["w1"][0]]), "bi": w[k["b1"][0]], "w2": _bf16(w[k["w2"][0]]), "b2": w[k["b2"][0]],
                           "g2": w[k["g2"][0]], "b2n": w[k["b2n"][0]]})
            if extra is not None:
                extra(layers, wq, w[k["w1"][0]])
        return layers

    # ---- state_dict with the third-party names
    def state_dict(self, *args, **kwargs):
        return OrderedDict((k, v.detach().clone()) for k, v in self._w.items())

    def load_state_dict(self, sd, strict: bool = True):
        missing = [k for k in self._w if k not in sd]
        unexpected = [k for k in sd if k not in self._w]
        if strict and missing:
            raise RuntimeError(f"missing keys: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        for k in self._w:
            if k in sd:
                if tuple(sd[k].shape) != tuple(self._w[k].shape):
                    raise RuntimeError(f"shape mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(self._w[k].shape)}")
                self._w[k].copy_(sd[k].to(self._w[k].device, torch.float32))
        self._packed = None
        self.weights_version += 1
        return missing, unexpected

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        for k in self._w:
            self._w[k] = fn(self._w[k]).float()
        self._packed = None
        self._bufs.clear()
        self.weights_version += 1
        return self

    @property
    def device(self) -> torch.device:
        return next(iter(self._w.values())).device

    def _require_hip(self):
        if self.device.type != "cuda":
            raise L.UltrafndHipError(f"{type(self).__name__} runs on a HIP device only: call .to('cuda') (no CPU fallback)")

    def _strict(self, run):
        """forward(strict=True), the offline feature builder's mode (encode_fields; caches for the reference-style training mode): run()
        with the more faithful fp32 residual stream whatever the in-step default is -- the bf16 stream's speed only matters inside the
        train step -- then the fold guard is read (one host sync) and, if it tripped, run() repeated with materialised
        LayerNorms."""
        rd, self.residual_dtype = self.residual_dtype, "fp32"
        try:
            if self.fold_ln:
                out = run()
                if not self.check_fold():
                    return out
            return run()
        finally:
            self.residual_dtype = rd

    def _fold_parts(self, M: int) -> int:
        """The {sum, sumsq} partials per row (an even count) that the GEMMs of an M-row pass write for its folded LayerNorms, or 0 when
        the pass cannot fold: fold_ln is off, or the two GEMM widths that produce a residual-stream row disagree on the count."""
        p1 = L.lib().ufnd_gemm_bf16_stat_parts(M, self.hidden, self.hidden)
        p2 = L.lib().ufnd_gemm_bf16_stat_parts(M, self.hidden, self.inter)
        return p1 if (self.fold_ln and p1 > 0 and p1 == p2 and p1 % 2 == 0) else 0

    # ---- thin wrappers over the C ABI
    # m_live (BertTextEncoder's packed pass): the device address of an int holding how many of the operands' rows are live.  With it a
    # Linear / LayerNorm computes the first *m_live rows of its capacity-sized operands only (include/ultrafnd_hip.h,
    # ufnd_gemm_bf16_live): same launches, same shapes (the tile: _tile_for).  None: every row.
    def _tile_for(self, which, m_live) -> int:
        """The GEMM tile of a Linear's launch: the `tiles` entry, else (a live-row launch) the running pass's own choice, else -1."""
        t = self.tiles.get(which)
        if t is None and m_live is not None:
            t = self._live_tiles.get(which)
        return -1 if t is None else t

    def _gemm(self, A, W, bias, out_bf16=None, out_f32=None, residual=None, act=ACT_NONE, which=None, m_live=None):
        M = A.shape[0]
        N, K = W.shape
        L.check(L.lib().ufnd_gemm_bf16_live(A.data_ptr(), W.data_ptr(), L.ptr(bias), L.ptr(residual), L.ptr(out_bf16),
                                            L.ptr(out_f32), M, N, K, A.stride(0), W.stride(0),
                                            residual.stride(0) if residual is not None else 0,
                                            out_bf16.stride(0) if out_bf16 is not None else 0,
                                            out_f32.stride(0) if out_f32 is not None else 0, act, self._tile_for(which, m_live),
                                            m_live, L.stream_ptr(A.device)), "ufnd_gemm_bf16_live")

    def _gemm_ln(self, A, W, bias, out_bf16=None, out_f32=None, residual=None, act=ACT_NONE, a_stats=None, colsum=None,
                 r_stats=None, r_gamma=None, r_beta=None, out_stats=None, eps=1e-5, which=None, residual_bf16=None, m_live=None):
        """ufnd_gemm_bf16_ln: a_stats / r_stats / out_stats are (M, parts, 2) fp32 tensors."""
        M = A.shape[0]
        N, K = W.shape
        ln = L.GemmLn()
        ln.a_stats, ln.colsum = L.ptr(a_stats), L.ptr(colsum)
        ln.r_stats, ln.r_gamma, ln.r_beta = L.ptr(r_stats), L.ptr(r_gamma), L.ptr(r_beta)
        ln.out_stats = L.ptr(out_stats)
        ln.a_parts = a_stats.shape[1] if a_stats is not None else 0
        ln.r_parts = r_stats.shape[1] if r_stats is not None else 0
        ln.a_eps = ln.r_eps = eps
        ln.width = self.hidden
        ln.tile_cfg = self._tile_for(which, m_live)
        if residual_bf16 is not None:
            ln.residual_bf16, ln.ldrb = residual_bf16.data_ptr(), residual_bf16.stride(0)
        if a_stats is not None:      # fold guard: the launch reports the largest |mean| / std among the rows it folds
            ln.guard = self._guard_buf(A.device).data_ptr()
        L.check(L.lib().ufnd_gemm_bf16_ln_live(A.data_ptr(), W.data_ptr(), L.ptr(bias), L.ptr(residual), L.ptr(out_bf16),
                                               L.ptr(out_f32), M, N, K, A.stride(0), W.stride(0),
                                               residual.stride(0) if residual is not None else 0,
                                               out_bf16.stride(0) if out_bf16 is not None else 0,
                                               out_f32.stride(0) if out_f32 is not None else 0, act, ctypes.byref(ln),
                                               m_live, L.stream_ptr(A.device)), "ufnd_gemm_bf16_ln_live")

    def _guard_buf(self, dev) -> torch.Tensor:
        """The fold guard's slots (UFND_FOLD_GUARD_SLOTS floats): every folded GEMM launch -- inside captured graphs too -- leaves
        the largest |mean| / std among the rows it folds in them (one atomicMax per workgroup, ufnd_gemm_ln.guard), so every
        row of every batch is looked at by the kernel that folds it; the host reads the slots when it chooses to (check_fold)."""
        if self._guard is None or self._guard.device != dev:
            self._guard = torch.zeros(L.FOLD_GUARD_SLOTS, dtype=torch.float32, device=dev)
        return self._guard

    def fold_ratio(self) -> float:
        """Largest |mean| / std over the rows that went through a folded LayerNorm since the last reset (synchronises)."""
        return 0.0 if self._guard is None else float(self._guard.max().cpu())

    def check_fold(self, reset: bool = True, ratio: Optional[float] = None) -> bool:
        """The fold guard: True (and folding switched off for every later call, buffers rebuilt) when a folded row's
        |mean| / std exceeded FOLD_GUARD_MAX.  Every folded GEMM evaluates the guard on the device (inside captured graphs
        too); this reads it: `strict=True` forwards after each batch (which is then
        repeated unfolded), the trainer after every encoder pass through an asynchronous copy (`ratio=` hands that value in,
        so that nothing synchronises)."""
        r = self.fold_ratio() if ratio is None else float(ratio)
        if reset and self._guard is not None:
            self._guard.zero_()
        if self.fold_ln and r > self.FOLD_GUARD_MAX:
            warnings.warn(f"{type(self).__name__}: a residual-stream row with |mean|/std = {r:.1f} (> {self.FOLD_GUARD_MAX}) went through a "
                          "folded LayerNorm; switching to materialised LayerNorms (fold_ln=False)")
            self.fold_ln = False
            self._bufs.clear()
            return True
        return False

    @staticmethod
    def _fold(W, b, gamma, beta):
        """LayerNorm(x; gamma, beta) W^T + b  ==  rstd (x W'^T - mean colsum) + b'  with
        W' = bf16(W * gamma), colsum = row sums of the ROUNDED W', b' = b + W beta."""
        Wp = _bf16(W * gamma[None, :])
        # (W * beta).sum(1), not W @ beta: packing is one-off setup, but it was the only vendor-BLAS call (rocblas gemv) of the tree
        return Wp, Wp.float().sum(1).contiguous(), (b + (W * beta[None, :]).sum(1)).contiguous()

    def _ln(self, x, ldx, gamma, beta, out_bf16, out_f32, M, H, eps, m_live=None):
        if m_live is not None:      # (its own entry: ufnd_layernorm_live refuses a NULL count)
            L.check(L.lib().ufnd_layernorm_live(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), L.ptr(out_bf16),
                                                L.ptr(out_f32), M, H, eps, m_live, L.stream_ptr(x.device)), "ufnd_layernorm_live")
            return
        L.check(L.lib().ufnd_layernorm(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), L.ptr(out_bf16),
                                       L.ptr(out_f32), M, H, eps, L.stream_ptr(x.device)), "ufnd_layernorm")

    def _qkv_attn(self, A, W, bias, mask_i32, ctx, B, Lq, heads, a_stats=None, colsum=None, eps=1e-5, cu=None, bins=None, nbins=None, tiles=None,
                  ntiles=None):
        """Fused Q/K/V projection (+ folded LayerNorm of A) + attention, one launch per layer.  cu: sample b's rows are
        cu[b] .. cu[b+1] of the packed pass (None: the padded batch); bins, nbins (ufnd_text_pack_bins, with cu): one workgroup per
        bin of up to four samples and head pair (None: one per sample and head pair); tiles, ntiles (ufnd_text_pack_tiles, instead of
        cu and bins; the key mask is the table's): one workgroup per 256-row tile of whole samples and head.  Samples of Lq <= 64 rows (the ViT's 50) take
        the short-sample geometry, ufnd_qkv_attention_bf16_vit: 256 // Lq whole samples and one head per workgroup, no key mask."""
        ln = None
        if a_stats is not None:
            ln = L.GemmLn()
            ln.a_stats, ln.colsum, ln.a_parts, ln.a_eps, ln.r_eps, ln.width = a_stats.data_ptr(), colsum.data_ptr(), a_stats.shape[1], eps, eps, self.hidden
            ln.guard = self._guard_buf(A.device).data_ptr()
        if Lq <= 64:
            if mask_i32 is not None or cu is not None or bins is not None:
                raise L.UltrafndHipError("_qkv_attn: the short-sample kernel (Lq <= 64) takes no key mask, cu or bins")
            L.check(L.lib().ufnd_qkv_attention_bf16_vit(A.data_ptr(), W.data_ptr(), L.ptr(bias), ctx.data_ptr(), B, Lq, heads, A.stride(0),
                                                        W.stride(0), ctypes.byref(ln) if ln is not None else None, L.stream_ptr(A.device)),
                    "ufnd_qkv_attention_bf16_vit")
            return
        if tiles is not None:
            L.check(L.lib().ufnd_qkv_attention_bf16_tiles(A.data_ptr(), W.data_ptr(), L.ptr(bias), tiles.data_ptr(), ntiles.data_ptr(), ctx.data_ptr(),
                                                          tiles.shape[0], heads, A.stride(0), W.stride(0),
                                                          ctypes.byref(ln) if ln is not None else None, L.stream_ptr(A.device)),
                    "ufnd_qkv_attention_bf16_tiles")
            return
        L.check(L.lib().ufnd_qkv_attention_bf16_bins(A.data_ptr(), W.data_ptr(), L.ptr(bias), L.ptr(mask_i32), L.ptr(cu), L.ptr(bins),
                                                     L.ptr(nbins), ctx.data_ptr(), B, Lq, heads, A.stride(0), W.stride(0),
                                                     ctypes.byref(ln) if ln is not None else None, L.stream_ptr(A.device)),
                "ufnd_qkv_attention_bf16_bins")

    # ---- the layer loops.  `attend(A, W, bias, **fold)` is the pass's own: a layer's Q/K/V projection of A (folded: of LayerNorm(A),
    # fold = a_stats, colsum) and its attention into b["ctx"] -- one fused launch (_qkv_attn), or _two_launch around an attention entry
    def _two_launch(self, b, entry: str, operands: tuple, B: int, Lq: int, live=None):
        """attend as two launches: the projection GEMM into b["qkv"], then the attention entry(b["qkv"], *operands, b["ctx"], B, Lq,
        heads, stream).  operands: the tensors (or None) the entry takes between qkv and ctx -- (key_mask,) for the padded forms,
        (cu_seqlens, key_mask) for the packed ones.  The call's arguments are put together here, once per pass."""
        fn = getattr(L.lib(), entry)
        call = (b["qkv"].data_ptr(), *(L.ptr(t) for t in operands), b["ctx"].data_ptr(), B, Lq, self.heads, L.stream_ptr(self.device))

        def attend(A, W, bias, a_stats=None, colsum=None):
            if a_stats is None:
                self._gemm(A, W, bias, out_bf16=b["qkv"], which="qkv", m_live=live)
            else:
                self._gemm_ln(A, W, bias, out_bf16=b["qkv"], a_stats=a_stats, colsum=colsum, eps=self.eps, which="qkv", m_live=live)
            L.check(fn(*call), entry)
        return attend

    def _post_ln_layers(self, layers, b, attend, M: int, live=None, tail=None) -> None:
        """Post-LN layers (BERT, wav2vec2, RoBERTa) with one LayerNorm kernel per LayerNorm, over the work buffers' M rows (live: the
        first *live of them).  Leaves last_hidden_state in b["xf"] (and its bf16 rounding in b["xb"]).
        tail(res_bf16, res_f32, stats): past its attention the last layer runs over the class rows only -- the call gathers them from
        b["ctx"] and the given residual-side buffers into compact buffers of the same names (the copies: "rb", "rf", "rst") and
        returns those; last_hidden_state's class rows are then in the returned buffers' "xf"."""
        H, eps = self.hidden, self.eps
        for i, ly in enumerate(layers):
            attend(b["xb"], ly["wqkv"], ly["bqkv"])
            r, res = b, b["xf"]
            if tail is not None and i == len(layers) - 1:
                r = tail(None, b["xf"], None)
                res, M, live = r["rf"], r["y"].shape[0], None
            self._gemm(r["ctx"], ly["wo"], ly["bo"], out_f32=r["y"], residual=res, which="out", m_live=live)
            self._ln(r["y"], H, ly["g1"], ly["b1"], r["x1b"], r["x1f"], M, H, eps, m_live=live)
            self._gemm(r["x1b"], ly["w1"], ly["bi"], out_bf16=r["h"], act=ACT_GELU, which="ffn1", m_live=live)
            self._gemm(r["h"], ly["w2"], ly["b2"], out_f32=r["y"], residual=r["x1f"], which="ffn2", m_live=live)
            self._ln(r["y"], H, ly["g2"], ly["b2n"], r["xb"], r["xf"], M, H, eps, m_live=live)

    def _pre_ln_blocks(self, layers, b, attend, M: int, act: int, live=None, tail=None) -> None:
        """Pre-LN blocks (both CLIP towers) with one LayerNorm kernel per LayerNorm, on the fp32 residual stream b["xf"] (M rows; live:
        the first *live of them).  tail(): the buffers the last layer runs over past its attention (the ViT's class-token rows)."""
        H, eps = self.hidden, self.eps
        for i, ly in enumerate(layers):
            self._ln(b["xf"], H, ly["g1"], ly["b1"], b["hb"], None, M, H, eps, m_live=live)
            attend(b["hb"], ly["wqkv"], ly["bqkv"])
            r = tail() if (tail is not None and i == len(layers) - 1) else b
            xf = r["xf"]
            self._gemm(r["ctx"], ly["wo"], ly["bo"], out_f32=xf, residual=xf, which="out", m_live=live)
            self._ln(xf, xf.stride(0), ly["g2"], ly["b2n"], r["hb"], None, xf.shape[0], H, eps, m_live=live)
            self._gemm(r["hb"], ly["w1"], ly["bi"], out_bf16=r["m"], act=act, which="ffn1", m_live=live)
            self._gemm(r["m"], ly["w2"], ly["b2"], out_f32=xf, residual=xf, which="ffn2", m_live=live)


def _live_ptr(cu: torch.Tensor) -> int:
    """The device address of a packed pass's live row count: the last entry of its cu_seqlens (B + 1 int32), which the pack kernel
    writes.  The m_live of the wrappers above."""
    return cu.data_ptr() + 4 * (cu.numel() - 1)


# CLIP's layer names, vision and text tower alike
_CLIP_LAYER = {"qkv_w": [f"self_attn.{n}.weight" for n in ("q_proj", "k_proj", "v_proj")],
               "qkv_b": [f"self_attn.{n}.bias" for n in ("q_proj", "k_proj", "v_proj")],
               "o_w": ["self_attn.out_proj.weight"], "o_b": ["self_attn.out_proj.bias"], "g1": ["layer_norm1.weight"], "b1n": ["layer_norm1.bias"],
               "w1": ["mlp.fc1.weight"], "b1": ["mlp.fc1.bias"], "w2": ["mlp.fc2.weight"], "b2": ["mlp.fc2.bias"],
               "g2": ["layer_norm2.weight"], "b2n": ["layer_norm2.bias"]}


# =============================================================================================
class BertTextEncoder(_EncoderBase):
    LAYER_PREFIX = "encoder.layer.{}."
    LAYER_NAMES = {"qkv_w": [f"attention.self.{n}.weight" for n in ("query", "key", "value")],
                   "qkv_b": [f"attention.self.{n}.bias" for n in ("query", "key", "value")],
                   "o_w": ["attention.output.dense.weight"], "o_b": ["attention.output.dense.bias"],
                   "g1": ["attention.output.LayerNorm.weight"], "b1n": ["attention.output.LayerNorm.bias"],
                   "w1": ["intermediate.dense.weight"], "b1": ["intermediate.dense.bias"], "w2": ["output.dense.weight"], "b2": ["output.dense.bias"],
                   "g2": ["output.LayerNorm.weight"], "b2n": ["output.LayerNorm.bias"]}

    def __init__(self, layers: int = 12, hidden: int = 768, heads: int = 12, intermediate: int = 3072,
                 vocab_size: int = 30522, max_position: int = 512, type_vocab: int = 2, eps: float = 1e-12,
                 fold_ln: bool = True, residual_dtype: str = "bf16", hidden_dropout_prob: float = 0.0,
                 attention_probs_dropout_prob: float = 0.0):
        check_geometry(hidden=("hidden", hidden), heads=("heads", heads), intermediate=("intermediate", intermediate))
        super().__init__(hidden, heads, fold_ln, residual_dtype)
        # train-mode dropout (HF BertConfig names): applied only by encoder_train.TextBackprop.forward_train and its backward, never
        # by forward() / encode_fields, whatever the module's mode
        self.hidden_dropout_prob = dropout_prob("hidden_dropout_prob", hidden_dropout_prob)
        self.attention_probs_dropout_prob = dropout_prob("attention_probs_dropout_prob", attention_probs_dropout_prob)
        # 128-token samples: Q/K/V projection + attention of a layer as ONE launch (ufnd_qkv_attention_bf16); bit-identical
        # to the two-launch form, which every other length uses
        self.fuse_qkv_attention = True
        # the packed pass's fused launch over sample tiles (ufnd_text_pack_tiles: whole samples in 256-row tiles, one head per workgroup);
        # False: over slot bins (ufnd_text_pack_bins), which batches of more than TEXT_TILE_MAX_B samples use either way.  Bit-identical.
        self.text_sample_tiles = True
        # ... from this many slot-bin workgroups (B x heads / 2) on.  The tile form wins by cutting the launch's rounds and its CU-time;
        # a batch whose slot bins get a compute unit each (256: one round either way) stays on them -- measured at B = 32, 12 heads:
        # the tile workgroup is the longer one, the step 1 % slower (profiles/text_tile_pack_summary.md).
        self.text_tile_min_grid = 257
        # the packed L = 128 pass's out-projection and FFN2 (N = 768, residual + row statistics) from text_narrow_min_rows capacity rows on:
        # the 256x128 tile (2) instead of the library's choice for the capacity, 256x192 (22).  The library sizes 64 x 4 = 256 workgroups
        # for 16,384 rows; the 34 to 40 live row panels of a batch of 16- to 128-token samples give 136 to 160 of them, 204 to 240 of
        # 256x128 -- one round either way, each workgroup a third shorter (FFN2 74 -> 50 us, out-projection 29 -> 21 us per launch).
        # Above 42 live panels (66 % of the capacity) the 256x128 launch spills into a second round; measured crossover and the
        # full-length batch (+2.8 % there): DESIGN.md's bf16 GEMM section, profiles/text_narrow_tile_summary.md.  22 restores the library's choice; a
        # `tiles` entry for the op wins over this.  Bit-identical rows either way: a row does not depend on the tile that computed it.
        self.text_narrow_tile = 2
        self.text_narrow_min_rows = 8192
        self.layers, self.inter, self.vocab, self.eps = layers, intermediate, vocab_size, eps
        self.max_position = max_position
        w, init = self._w, self._seeded_init()
        w["embeddings.word_embeddings.weight"] = init((vocab_size, hidden))
        w["embeddings.position_embeddings.weight"] = init((max_position, hidden))
        w["embeddings.token_type_embeddings.weight"] = init((type_vocab, hidden))
        w["embeddings.LayerNorm.weight"] = torch.ones(hidden)
        w["embeddings.LayerNorm.bias"] = torch.zeros(hidden)
        for i in range(layers):
            P = f"encoder.layer.{i}."
            for n in ("query", "key", "value"):
                w[P + f"attention.self.{n}.weight"] = init((hidden, hidden))
                w[P + f"attention.self.{n}.bias"] = torch.zeros(hidden)
            w[P + "attention.output.dense.weight"] = init((hidden, hidden))
            w[P + "attention.output.dense.bias"] = torch.zeros(hidden)
            w[P + "attention.output.LayerNorm.weight"] = torch.ones(hidden)
            w[P + "attention.output.LayerNorm.bias"] = torch.zeros(hidden)
            w[P + "intermediate.dense.weight"] = init((intermediate, hidden))
            w[P + "intermediate.dense.bias"] = torch.zeros(intermediate)
            w[P + "output.dense.weight"] = init((hidden, intermediate))
            w[P + "output.dense.bias"] = torch.zeros(hidden)
            w[P + "output.LayerNorm.weight"] = torch.ones(hidden)
            w[P + "output.LayerNorm.bias"] = torch.zeros(hidden)

    def _fold_layer(self, layers, wq, w1) -> None:
        # folded forms: intermediate.dense consumes LayerNorm_1; the NEXT layer's Q/K/V consume LayerNorm_2
        ly = layers[-1]
        ly["w1f"], ly["cs1"], ly["bif"] = self._fold(w1, ly["bi"], ly["g1"], ly["b1"])
        if len(layers) > 1:
            prev = layers[-2]
            ly["wqkvf"], ly["csqkv"], ly["bqkvf"] = self._fold(wq, ly["bqkv"], prev["g2"], prev["b2n"])

    def _pack(self):
        if self._packed is None:
            self._packed = {"layers": self._pack_layers(self._fold_layer)}
        return self._packed

    def _workbufs(self, B: int, Lq: int) -> dict:
        key = (B, Lq)
        if key not in self._bufs:
            dev, M, H = self.device, B * Lq, self.hidden
            bf, f32 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.float32, device=dev)
            self._bufs[key] = {"xb": torch.empty(M, H, **bf), "xf": torch.empty(M, H, **f32), "y": torch.empty(M, H, **f32),
                               "x1b": torch.empty(M, H, **bf), "x1f": torch.empty(M, H, **f32),
                               "qkv": torch.empty(M, 3 * H, **bf), "ctx": torch.empty(M, H, **bf),
                               "h": torch.empty(M, self.inter, **bf), "feat": torch.empty(B, H, **f32),
                               # packed pass (ufnd_text_pack): cu_seqlens (B + 1; cu[B] = the live row count) and row -> (b, pos)
                               "cu": torch.zeros(B + 1, dtype=torch.int32, device=dev), "row_src": torch.zeros(M, dtype=torch.int32, device=dev),
                               # (L <= 128: ufnd_text_pack_bins) the fused Q/K/V + attention's slot bins and their count
                               "bins": torch.zeros(B, 8, dtype=torch.int32, device=dev), "nbins": torch.zeros(1, dtype=torch.int32, device=dev)}
            if Lq <= 128 and B <= TEXT_TILE_MAX_B:      # (ufnd_text_pack_tiles) its sample tiles and their count
                self._bufs[key].update({"tiles": torch.zeros((B + 1) // 2, TEXT_TILE_INTS, dtype=torch.int32, device=dev),
                                        "ntiles": torch.zeros(1, dtype=torch.int32, device=dev)})
            p1 = self._fold_parts(M)
            if p1:
                # one statistics buffer per folded LayerNorm of the pass (st[2i]: layer i's attention half, st[2i+1]: its
                # feed-forward half); every buffer is read by a folded GEMM, which reports its rows' |mean| / std (fold guard)
                self._bufs[key].update({"y2": torch.empty(M, H, **f32), "y1b": torch.empty(M, H, **bf), "y2b": torch.empty(M, H, **bf),
                                        "st": torch.zeros(2 * self.layers, M, p1, 2, **f32)})
                self._guard_buf(dev)
        return self._bufs[key]

    def _check_length(self, Lq: int) -> None:
        if Lq > self.max_position:
            raise RuntimeError(f"sequence length {Lq} exceeds max_position_embeddings {self.max_position}")

    def _fuses(self, Lq: int) -> bool:
        """Whether an L-token pass runs a layer's Q/K/V projection + attention as one launch (two otherwise)."""
        return bool(self.fuse_qkv_attention and Lq == 128 and self.heads % 2 == 0)

    def live_tiles(self, packed: bool, B: int, Lq: int) -> Dict[str, int]:
        """The tiles a (B, L) pass names for its own live-row launches (text_narrow_tile, above): fixed by the pass's form and shape
        alone, so a captured pass never reads the live row count back.  N = 768 only: the width the choice was measured at."""
        if packed and Lq == 128 and B * Lq >= self.text_narrow_min_rows and self.hidden == 768:
            return {"out": self.text_narrow_tile, "ffn2": self.text_narrow_tile}
        return {}

    def _pass(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool, n_layers: Optional[int] = None, pool: bool = True,
              tail=None) -> dict:
        """One pass over a (B, L) batch: embeddings, the first n_layers layers (all by default) and, with pool, the pooled features.
        packed: over the rows ufnd_text_pack keeps, their count on the device (forward's unpad paragraph); otherwise over all B L rows.
        Returns the work buffers: last_hidden_state in "xf" (packed: its live rows), the features in "feat".  A packed, folded pass that
        pools never writes "xf": one kernel normalises the last layer's sums and pools them (ufnd_ln_masked_meanpool_l2_live).
        tail(b, cu, B, L): the layer loops' tail for this pass (a sequence classifier's class rows; never with pool)."""
        self._require_hip()
        dev = self.device
        B, Lq = input_ids.shape
        self._check_length(Lq)
        ids = input_ids.to(dev, torch.int64).contiguous()
        mask = attention_mask.to(dev, torch.int32).contiguous()
        p, b = self._pack(), self._workbufs(B, Lq)
        M = B * Lq
        fuse = self._fuses(Lq)
        cu = b["cu"] if packed else None                 # packed rows: sample b's are cu[b] .. cu[b+1] ...
        live = _live_ptr(cu) if packed else None         # ... and cu[B], their count, stays on the device: the pack kernel writes it
        self._live_tiles = self.live_tiles(packed, B, Lq)
        tiled = packed and fuse and self.text_sample_tiles and "tiles" in b and B * (self.heads // 2) >= self.text_tile_min_grid
        self._pack_embed(ids, mask, b, B, Lq, packed, fuse, tiled, live)
        layers = p["layers"] if n_layers is None else p["layers"][:max(1, int(n_layers))]
        ln_pool = pool and packed and "st" in b
        if tiled:
            attend = lambda A, W, bias, **fold: self._qkv_attn(A, W, bias, None, b["ctx"], B, Lq, self.heads, eps=self.eps, tiles=b["tiles"],
                                                               ntiles=b["ntiles"], **fold)
        elif fuse:
            bins, nbins = (b["bins"], b["nbins"]) if packed else (None, None)
            attend = lambda A, W, bias, **fold: self._qkv_attn(A, W, bias, mask, b["ctx"], B, Lq, self.heads, eps=self.eps, cu=cu, bins=bins,
                                                               nbins=nbins, **fold)
        elif packed:
            attend = self._two_launch(b, "ufnd_attention_bf16_varlen_masked", operands=(cu, mask), B=B, Lq=Lq, live=live)
        else:
            attend = self._two_launch(b, "ufnd_attention_bf16", operands=(mask,), B=B, Lq=Lq)
        tail = None if tail is None else tail(b, cu, B, Lq)
        if "st" in b:
            self._layers_folded(layers, b, attend, M, live, final_ln=not ln_pool, tail=tail)
        else:
            self._post_ln_layers(layers, b, attend, M, live, tail=tail)
        H, s = self.hidden, L.stream_ptr(dev)
        if ln_pool:       # bit-identical to the final LayerNorm into "xf" + the pooling below
            L.check(L.lib().ufnd_ln_masked_meanpool_l2_live(b["y2"].data_ptr(), layers[-1]["g2"].data_ptr(), layers[-1]["b2n"].data_ptr(), self.eps,
                                                            mask.data_ptr(), b["cu"].data_ptr(), b["feat"].data_ptr(), B, Lq, H, s),
                    "ufnd_ln_masked_meanpool_l2_live")
        elif pool and packed:
            L.check(L.lib().ufnd_masked_meanpool_l2_live(b["xf"].data_ptr(), mask.data_ptr(), b["cu"].data_ptr(), b["feat"].data_ptr(), B, Lq, H, s),
                    "ufnd_masked_meanpool_l2_live")
        elif pool:
            L.check(L.lib().ufnd_masked_meanpool_l2(b["xf"].data_ptr(), mask.data_ptr(), b["feat"].data_ptr(), B, Lq, H, s), "ufnd_masked_meanpool_l2")
        return b

    def _pack_rows(self, mask, b, B: int, Lq: int, fuse: bool, tiled: bool) -> None:
        """The packed pass's tables from the mask: cu_seqlens, row_src and, for the fused Q/K/V + attention, its slot bins / sample tiles."""
        s = L.stream_ptr(self.device)
        cu = b["cu"]
        if tiled:                # (+ the sample tiles: the fused Q/K/V + attention runs one workgroup per 256-row tile of whole samples and head;
                                 #  the slot bins stay current too: either launch form may follow this pack)
            L.check(L.lib().ufnd_text_pack_tiles(mask.data_ptr(), B, Lq, cu.data_ptr(), b["row_src"].data_ptr(), b["tiles"].data_ptr(),
                                                 b["ntiles"].data_ptr(), b["bins"].data_ptr(), b["nbins"].data_ptr(), s), "ufnd_text_pack_tiles")
        elif fuse:               # (+ the slot bins: the fused Q/K/V + attention runs one workgroup per bin of up to four samples)
            L.check(L.lib().ufnd_text_pack_bins(mask.data_ptr(), B, Lq, cu.data_ptr(), b["row_src"].data_ptr(), b["bins"].data_ptr(),
                                                b["nbins"].data_ptr(), s), "ufnd_text_pack_bins")
        else:
            L.check(L.lib().ufnd_text_pack(mask.data_ptr(), B, Lq, cu.data_ptr(), b["row_src"].data_ptr(), s), "ufnd_text_pack")

    def _embed_outs(self, b) -> tuple:
        """The embedding kernel's (bf16, fp32) outputs: with the folded bf16 stream nothing reads the fp32 copy."""
        return b["xb"].data_ptr(), None if ("st" in b and self.residual_dtype == "bf16") else b["xf"].data_ptr()

    def _pack_embed(self, ids, mask, b, B: int, Lq: int, packed: bool, fuse: bool, tiled: bool, live) -> None:
        """The pass's first launches: the packed pass's tables, then the embeddings into the residual stream."""
        w, H, s = self._w, self.hidden, L.stream_ptr(self.device)
        if packed:
            self._pack_rows(mask, b, B, Lq, fuse, tiled)
        tables = [w["embeddings." + n].data_ptr() for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                                                            "LayerNorm.weight", "LayerNorm.bias")]
        outs = self._embed_outs(b)
        if packed:
            L.check(L.lib().ufnd_bert_embed_live(ids.data_ptr(), b["row_src"].data_ptr(), live, *tables, *outs, B * Lq, Lq, H, self.vocab, self.eps, s),
                    "ufnd_bert_embed_live")
        else:
            L.check(L.lib().ufnd_bert_embed(ids.data_ptr(), *tables, *outs, B, Lq, H, self.vocab, self.eps, s), "ufnd_bert_embed")

    def _layers_folded(self, layers, b, attend, M: int, live=None, final_ln: bool = True, tail=None) -> None:
        """The layers without a LayerNorm kernel between Linears (module docstring).  y1 / y2 are the
        PRE-LayerNorm sums of the attention and the feed-forward halves (fp32 + bf16 + row statistics).  final_ln=False leaves the
        last layer's sums in y2 and their LayerNorm to the caller.  tail: as _post_ln_layers' (the compact buffers carry "st1" / "st2",
        the last layer's statistics over the class rows alone: statistics are indexed by row number)."""
        H, eps = self.hidden, self.eps
        st = b["st"]
        rb = self.residual_dtype == "bf16"
        prev, r = None, b
        for i, ly in enumerate(layers):
            st1, st2 = st[2 * i], st[2 * i + 1]
            last = i == len(layers) - 1
            if prev is None:      # layer 0 consumes the embeddings' own (materialised) LayerNorm
                attend(b["xb"], ly["wqkv"], ly["bqkv"])
                res_b, res_f, stp, rg, rbeta = b["xb"], b["xf"], None, None, None
            else:
                stp = st[2 * i - 1]           # the previous layer's feed-forward half
                attend(b["y2b"], ly["wqkvf"], ly["bqkvf"], a_stats=stp, colsum=ly["csqkv"])
                res_b, res_f, rg, rbeta = b["y2b"], b["y2"], prev["g2"], prev["b2n"]
            if last and tail is not None:      # (K / V and the attention needed every row; nothing past them does)
                r = tail(res_b if rb else None, None if rb else res_f, stp)
                res_b, res_f, stp = r["rb"], r["rf"], (r["rst"] if stp is not None else None)
                st1, st2, M, live = r["st1"], r["st2"], r["y"].shape[0], None
            y1, y2 = r["y"], r["y2"]
            self._gemm_ln(r["ctx"], ly["wo"], ly["bo"], out_f32=None if rb else y1, out_bf16=r["y1b"], residual=None if rb else res_f,
                          residual_bf16=res_b if rb else None, r_stats=stp, r_gamma=rg, r_beta=rbeta, out_stats=st1,
                          eps=eps, which="out", m_live=live)
            self._gemm_ln(r["y1b"], ly["w1f"], ly["bif"], out_bf16=r["h"], act=ACT_GELU, a_stats=st1, colsum=ly["cs1"], eps=eps, which="ffn1",
                          m_live=live)
            self._gemm_ln(r["h"], ly["w2"], ly["b2"], out_f32=y2 if (last or not rb) else None, out_bf16=r["y2b"], residual=None if rb else y1,
                          residual_bf16=r["y1b"] if rb else None, r_stats=st1, r_gamma=ly["g1"], r_beta=ly["b1"], out_stats=st2, eps=eps,
                          which="ffn2", m_live=live)      # (the last layer's fp32 sums feed the final, materialised LayerNorm)
            prev = ly
        if final_ln:
            self._ln(r["y2"], H, prev["g2"], prev["b2n"], None, r["xf"], M, H, eps, m_live=live)       # last_hidden_state is materialised once (fp32 only: no GEMM reads it)

    @torch.no_grad()
    def last_hidden_state(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, n_layers: Optional[int] = None) -> torch.Tensor:
        """BertModel(input_ids, attention_mask).last_hidden_state -> (B, L, H) fp32 (a view of an
        internal buffer, valid until the next call with the same shape).  n_layers: stop after that many layers (the
        hidden state BertModel reports as hidden_states[n_layers]; per-layer localisation in the parity tests)."""
        b = self._pass(input_ids, attention_mask, packed=False, n_layers=n_layers, pool=False)
        return b["xf"].view(*input_ids.shape, self.hidden)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, unpad: bool = True, strict: bool = False) -> torch.Tensor:
        """Batched BERTContextEncoder.encode: (B,L) ids/mask -> (B,768) L2-normalised features.
        strict=True is the offline feature builder's mode: fp32 residual stream (whatever `residual_dtype` says), the fold guard checked
        after the pass (one host sync) and, if it tripped, the batch repeated with materialised LayerNorms; not for hipGraph capture.
        unpad=True (default): the encoder runs over packed rows -- sample b keeps its positions 0 .. its last kept position, so only
        trailing padding is dropped (holes stay rows, masked as keys).  Padded positions never reach the pooling (text_blocks.py:82-86)
        and every kept row is computed exactly as in the padded batch: bit-identical features for every mask, while the work drops
        with the padding fraction.  The row count stays on the device (ufnd_text_pack) and every launch keeps its padded geometry:
        no host sync, hipGraph-capturable, a replay follows the ids / mask its buffers hold.  unpad=False: the padded computation."""
        if strict:
            return self._strict(lambda: self.forward(input_ids, attention_mask, unpad=unpad))
        return self._pass(input_ids, attention_mask, packed=unpad)["feat"]

    encode_batch = forward

    @torch.no_grad()
    def encode_fields(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, part_valid: torch.Tensor,
                      chunk: int = 1024, unpad: bool = True) -> torch.Tensor:
        """Batched BERTContextEncoder.encode_fields (text_blocks.py:108-128).
        input_ids / attention_mask (N, M, L): the tokenised parts of N records in the reference's
        order [title, ocr, up to 10 comments] (M <= 12); part_valid (N, M): 1 where the part exists
        (the reference skips empty strings).  Every existing part goes through the encoder in one
        batched pass (the reference runs <= 12 batch-1 forwards per record), then the per-record mean
        of the part vectors is L2-normalised.  Returns (N, 768); zero rows for records without parts."""
        self._require_hip()
        dev = self.device
        N, Mx, Lq = input_ids.shape
        valid = part_valid.to(dev, torch.int32).contiguous()
        ids = input_ids.to(dev, torch.int64).reshape(N * Mx, Lq)
        mask = attention_mask.to(dev, torch.int32).reshape(N * Mx, Lq)
        rows = torch.nonzero(valid.reshape(-1), as_tuple=False).flatten()
        parts = torch.zeros(N * Mx, self.hidden, dtype=torch.float32, device=dev)
        for s0 in range(0, rows.numel(), chunk):
            r = rows[s0:s0 + chunk]
            parts[r] = self.forward(ids[r], mask[r], unpad=unpad, strict=True)      # (texts are short against max_length: skip the padding)
        out = torch.empty(N, self.hidden, dtype=torch.float32, device=dev)
        L.check(L.lib().ufnd_field_mean_l2(parts.data_ptr(), valid.data_ptr(), out.data_ptr(), N, Mx, self.hidden,
                                           L.stream_ptr(dev)), "ufnd_field_mean_l2")
        return out


# =============================================================================================
class ClipVisualEncoder(_EncoderBase):
    LAYER_PREFIX, LAYER_NAMES = "vision_model.encoder.layers.{}.", _CLIP_LAYER

    def __init__(self, layers: int = 12, hidden: int = 768, heads: int = 12, intermediate: int = 3072, patch: int = 32,
                 image: int = 224, projection_dim: int = 512, eps: float = 1e-5, fold_ln: bool = True, residual_dtype: str = "bf16",
                 attention_dropout: float = 0.0):
        check_geometry(hidden=("hidden", hidden), heads=("heads", heads), intermediate=("intermediate", intermediate),
                       projection_dim=("projection_dim", projection_dim))
        # ufnd_vit_patchify copies 8-pixel runs of whole patches; the patch GEMM's K = 3 patch^2 is a multiple of 64 with them
        if patch < 8 or patch % 8:
            raise ValueError(f"patch={patch!r}: a positive multiple of 8 (the patch GEMM's K = 3 patch^2 is then a multiple of 64)")
        if image < patch or image % patch:
            raise ValueError(f"image={image!r}: a positive multiple of patch={patch}")
        super().__init__(hidden, heads, fold_ln, residual_dtype)
        # train-mode dropout on the attention probabilities (HF CLIPVisionConfig name; CLIP has no hidden-state dropout): applied only by
        # encoder_train.VisualBackprop.forward_train and its backward
        self.attention_dropout = dropout_prob("attention_dropout", attention_dropout)
        self.layers, self.inter = layers, intermediate
        self.patch, self.image, self.proj, self.eps = patch, image, projection_dim, eps
        self.n_patches = (image // patch) ** 2
        # samples of at most 64 tokens: Q/K/V projection + attention of a layer as ONE launch (ufnd_qkv_attention_bf16_vit); bit-identical
        # to the two-launch form (off: a GEMM into qkv and an attention launch per layer)
        self.fuse_qkv_attention = True
        # the embeddings read the class-token row of each frame only (CLIPVisionModelWithProjection pools last_hidden_state[:, 0]): past
        # its attention the last layer runs over those N rows, not over all N T (forward, image_embeds; hidden_state keeps every row).
        # A row's arithmetic does not depend on the launch it is part of, so the features are bit-identical (off: all rows)
        self.cls_tail = True
        w, V, init = self._w, "vision_model.", self._seeded_init()
        w[V + "embeddings.class_embedding"] = init((hidden,))
        w[V + "embeddings.patch_embedding.weight"] = init((hidden, 3, patch, patch))
        w[V + "embeddings.position_embedding.weight"] = init((self.n_patches + 1, hidden))
        w[V + "pre_layrnorm.weight"], w[V + "pre_layrnorm.bias"] = torch.ones(hidden), torch.zeros(hidden)
        for i in range(layers):
            P = V + f"encoder.layers.{i}."
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                w[P + f"self_attn.{n}.weight"] = init((hidden, hidden))
                w[P + f"self_attn.{n}.bias"] = torch.zeros(hidden)
            w[P + "layer_norm1.weight"], w[P + "layer_norm1.bias"] = torch.ones(hidden), torch.zeros(hidden)
            w[P + "mlp.fc1.weight"], w[P + "mlp.fc1.bias"] = init((intermediate, hidden)), torch.zeros(intermediate)
            w[P + "mlp.fc2.weight"], w[P + "mlp.fc2.bias"] = init((hidden, intermediate)), torch.zeros(hidden)
            w[P + "layer_norm2.weight"], w[P + "layer_norm2.bias"] = torch.ones(hidden), torch.zeros(hidden)
        w[V + "post_layernorm.weight"], w[V + "post_layernorm.bias"] = torch.ones(hidden), torch.zeros(hidden)
        w["visual_projection.weight"] = init((projection_dim, hidden))

    def _fold_layer(self, layers, wq, w1) -> None:
        ly = layers[-1]
        ly["wqkvf"], ly["csqkv"], ly["bqkvf"] = self._fold(wq, ly["bqkv"], ly["g1"], ly["b1"])
        ly["w1f"], ly["cs1"], ly["bif"] = self._fold(w1, ly["bi"], ly["g2"], ly["b2n"])

    def _pack(self):
        if self._packed is None:
            w = self._w
            self._packed = {"layers": self._pack_layers(self._fold_layer),
                            "wpatch": _bf16(w["vision_model.embeddings.patch_embedding.weight"].reshape(self.hidden, -1)),
                            "wproj": _bf16(w["visual_projection.weight"])}
        return self._packed

    def _workbufs(self, B: int, Fr: int) -> dict:
        key = (B, Fr)
        if key not in self._bufs:
            dev, H, N = self.device, self.hidden, B * Fr
            T = self.n_patches + 1
            M = N * T
            bf, f32 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.float32, device=dev)
            self._bufs[key] = {"patches": torch.empty(N * self.n_patches, 3 * self.patch ** 2, **bf),
                               "pe": torch.empty(N * self.n_patches, H, **f32), "xf": torch.empty(M, H, **f32),
                               "hb": torch.empty(M, H, **bf), "qkv": torch.empty(M, 3 * H, **bf),
                               "ctx": torch.empty(M, H, **bf), "m": torch.empty(M, self.inter, **bf),
                               "pooled": torch.empty(N, H, **bf), "e": torch.empty(N, self.proj, **f32),
                               "feat": torch.empty(B, self.proj, **f32)}
            p1 = self._fold_parts(M)
            if p1:
                # st0: the assembled embeddings' statistics; st[2i] / st[2i+1]: layer i's attention / feed-forward half
                # stc: the last layer's two statistics buffers over the class-token rows alone (_cls_rows; statistics are indexed by
                # row number, so a strided view of st will not do)
                self._bufs[key].update({"st0": torch.zeros(M, 2, 2, **f32), "st": torch.zeros(2 * self.layers, M, p1, 2, **f32),
                                        "stc": torch.zeros(2, N, p1, 2, **f32)})
                self._guard_buf(dev)
            else:
                self._bufs[key]["hc"] = torch.empty(N, H, **bf)      # (_cls_rows: the last layer_norm2 of the class-token rows)
        return self._bufs[key]

    @torch.no_grad()
    def image_embeds(self, frames: torch.Tensor) -> torch.Tensor:
        """frames (N,3,S,S) fp32 -> un-normalised projected embeddings (N, 512)
        (CLIPVisionModelWithProjection.image_embeds)."""
        return self._run(frames[:, None], cls_tail=self.cls_tail)[0]

    @torch.no_grad()
    def hidden_state(self, frames: torch.Tensor, n_layers: Optional[int] = None) -> torch.Tensor:
        """The residual stream after `n_layers` layers (all by default), (N, 50, H) fp32: CLIPVisionModel's hidden_states[n_layers]
        (per-layer localisation in the parity tests)."""
        if frames.dim() == 4:
            frames = frames[:, None]
        _, b = self._run(frames, n_layers)
        N = frames.shape[0] * frames.shape[1]
        return b["xf"].view(N, self.n_patches + 1, self.hidden)

    def _fuses(self) -> bool:
        """Whether a pass runs a layer's Q/K/V projection + attention as one launch (samples of at most 64 tokens; two otherwise)."""
        return bool(self.fuse_qkv_attention and self.n_patches + 1 <= 64)

    def _embed(self, fr, p, b, N) -> None:
        """Patchify, patch GEMM, then class token + positions + pre-LayerNorm into the residual stream (folded: hb and its statistics st0)."""
        w, V, s = self._w, "vision_model.", L.stream_ptr(self.device)
        L.check(L.lib().ufnd_vit_patchify(fr.data_ptr(), b["patches"].data_ptr(), N, self.image, self.patch, s), "ufnd_vit_patchify")
        self._gemm(b["patches"], p["wpatch"], None, out_f32=b["pe"])
        L.check(L.lib().ufnd_vit_assemble(b["pe"].data_ptr(), w[V + "embeddings.class_embedding"].data_ptr(),
                                          w[V + "embeddings.position_embedding.weight"].data_ptr(),
                                          w[V + "pre_layrnorm.weight"].data_ptr(), w[V + "pre_layrnorm.bias"].data_ptr(),
                                          None if ("st0" in b and self.residual_dtype == "bf16") else b["xf"].data_ptr(),      # (bf16 stream: hb is the stream)
                                          L.ptr(b["hb"]) if "st0" in b else None, L.ptr(b.get("st0")),
                                          N, self.n_patches, self.hidden, self.eps, s), "ufnd_vit_assemble")

    def _cls_rows(self, b, N) -> dict:
        """The work buffers over the class-token rows alone, as the last layer past its attention takes them: N-row views of ctx / hb /
        xf with row stride T H, the first N rows of m, the statistics in stc.  Unfolded, hb only carries layer_norm2's output to FFN1
        and ufnd_layernorm writes dense rows: the compact hc stands in for it."""
        T = self.n_patches + 1
        r = {k: b[k].view(N, T * self.hidden)[:, :self.hidden] for k in ("ctx", "hb", "xf")}
        r["m"] = b["m"][:N]
        if "stc" in b:
            r["st1"], r["st2"] = b["stc"][0], b["stc"][1]
        else:
            r["hb"] = b["hc"]
        return r

    def _blocks_folded(self, layers, b, attend, tail=None) -> None:
        """Pre-LN blocks without LayerNorm kernels: hb is the bf16 rounding of the residual stream xf, st* the row statistics its
        LayerNorms need (module docstring).  tail (_cls_rows): the last layer's out-projection, FFN1 and FFN2 over the class-token rows only."""
        eps, stA, st = self.eps, b["st0"], b["st"]
        rb = self.residual_dtype == "bf16"       # the stream is hb itself, updated in place (a tile reads exactly what it rewrites)
        for i, ly in enumerate(layers):
            st1, st2 = st[2 * i], st[2 * i + 1]
            last = i == len(layers) - 1
            attend(b["hb"], ly["wqkvf"], ly["bqkvf"], a_stats=stA, colsum=ly["csqkv"])
            r = b
            if last and tail is not None:      # (K / V and the attention needed every row; nothing past them does)
                r = tail()
                st1, st2 = r["st1"], r["st2"]
            self._gemm_ln(r["ctx"], ly["wo"], ly["bo"], out_f32=None if rb else r["xf"], out_bf16=r["hb"], residual=None if rb else r["xf"],
                          residual_bf16=r["hb"] if rb else None, out_stats=st1, eps=eps, which="out")
            self._gemm_ln(r["hb"], ly["w1f"], ly["bif"], out_bf16=r["m"], act=ACT_QUICK_GELU, a_stats=st1, colsum=ly["cs1"], eps=eps, which="ffn1")
            self._gemm_ln(r["m"], ly["w2"], ly["b2"], out_f32=r["xf"] if (last or not rb) else None, out_bf16=r["hb"],
                          residual=None if rb else r["xf"], residual_bf16=r["hb"] if rb else None, out_stats=st2, eps=eps, which="ffn2")
            stA = st2

    def _pooled_projection(self, p, b, N) -> None:
        """post-LN on the CLS rows (row stride T*H), bias-free projection into b["e"]."""
        w, V, H = self._w, "vision_model.", self.hidden
        self._ln(b["xf"], (self.n_patches + 1) * H, w[V + "post_layernorm.weight"], w[V + "post_layernorm.bias"], b["pooled"], None, N, H, self.eps)
        self._gemm(b["pooled"], p["wproj"], None, out_f32=b["e"])

    def _run(self, frames5: torch.Tensor, n_layers: Optional[int] = None, cls_tail: bool = False):
        """One pass over (B, F) frames: (the (B F, projection_dim) embeddings, the work buffers).  cls_tail: the caller reads the
        embeddings only, so the last layer may leave every row but the class tokens' behind its attention (hidden_state: never)."""
        self._require_hip()
        B, Fr = frames5.shape[:2]
        if tuple(frames5.shape[2:]) != (3, self.image, self.image):
            raise RuntimeError(f"frames: expected (B,F,3,{self.image},{self.image}), got {tuple(frames5.shape)}")
        fr = L.f32c(frames5.to(self.device)).view(B * Fr, 3, self.image, self.image)
        p, b = self._pack(), self._workbufs(B, Fr)
        layers = p["layers"] if n_layers is None else p["layers"][:max(1, int(n_layers))]
        N, T = B * Fr, self.n_patches + 1
        self._embed(fr, p, b, N)
        if self._fuses():
            attend = lambda A, W, bias, **fold: self._qkv_attn(A, W, bias, None, b["ctx"], N, T, self.heads, eps=self.eps, **fold)
        else:
            attend = self._two_launch(b, "ufnd_attention_bf16", operands=(None,), B=N, Lq=T)      # (no key mask: every patch is a key)
        tail = (lambda: self._cls_rows(b, N)) if cls_tail else None
        if "st0" in b:
            self._blocks_folded(layers, b, attend, tail)
        else:
            self._pre_ln_blocks(layers, b, attend, N * T, ACT_QUICK_GELU, tail=tail)
        self._pooled_projection(p, b, N)
        return b["e"], b

    @torch.no_grad()
    def forward(self, frames: torch.Tensor, strict: bool = False) -> torch.Tensor:
        """frames (B,F,3,224,224) or (B,3,224,224) -> (B,512) features.  strict: as BertTextEncoder.forward."""
        if frames.dim() == 4:
            frames = frames[:, None]
        if strict:
            return self._strict(lambda: self.forward(frames))
        B, Fr = frames.shape[:2]
        e, b = self._run(frames, cls_tail=self.cls_tail)
        L.check(L.lib().ufnd_l2norm_frames(e.data_ptr(), b["feat"].data_ptr(), B, Fr, self.proj, L.stream_ptr(self.device)),
                "ufnd_l2norm_frames")
        return b["feat"]

    @torch.no_grad()
    def encode_frames(self, frames_u8: torch.Tensor, lengths=None, layout: Optional[str] = None) -> torch.Tensor:
        """Decoded uint8 frames (B,F,H,W,3) / (B,F,3,H,W), or a 4-D image batch, on the device -> (B,512) features: the checkpoint's
        image preprocessing at this encoder's `image` size (video.clip_preprocess, bit-exact to CLIPImageProcessor's Pillow backend),
        then forward().  lengths: frames at or past a clip's length repeat its last valid frame."""
        from .video import clip_preprocess
        return self.forward(clip_preprocess(frames_u8, lengths, layout, image_size=self.image)["pixel_values"])
