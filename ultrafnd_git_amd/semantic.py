"""The CLIP text tower and the text-image semantic analyzer, MI355X-native.

  ClipTextEncoder          transformers.CLIPTextModelWithProjection (the ViT-B/32 text geometry: hidden 512, 8 heads, 12 pre-LN
                           quick-GELU layers, 77 positions, bias-free projection to 512), frozen and forward-only: the other half of
                           the CLIP model whose vision tower is encoders.ClipVisualEncoder.  (B, L) ids / mask -> (B, 512)
                           L2-normalised features in the joint text-image space.  Tokenisation stays outside (ids / mask in), there
                           is no tokenizer vocabulary offline.
  SemanticForgeryAnalyzer  the reference's module of that name (src/models/semantic_forgery.py): title and OCR through the text
                           tower, Linear(512, D) -> GELU each, then semantic_text, semantic_image and the L2-normalised
                           semantic_gap.  With `frames` the image side is the vision tower, which the reference only imitates with
                           "text as a proxy for vision"; either way the CLIP similarity of the two sides is returned too.

Weights keep HF's `state_dict` names, so a CLIPTextModelWithProjection checkpoint loads with strict=True.

Causal skipping and the live-row pass.  CLIP's text tower attends causally and pools ONE row per sample, the EOS
position e(b).  Under a causal mask no row after e(b) can influence row e(b), so the packed pass (`packed=True`, the default) keeps
rows 0 .. e(b) of each sample and nothing else -- exactly, not approximately: every kept row is computed as in the padded batch
and the features are bit-identical.  The row count stays on the device (ufnd_clip_text_pack) and every launch keeps its padded
geometry: no host sync, hipGraph-capturable.  Inside the attention a workgroup stops at the key block that holds its last query.

Precondition (not checked on the hot path): L <= max_position_embeddings and attention_mask[:, 0] == 1, so that every query sees a
key; rows whose every visible key is masked are unspecified.  No CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .encoders import _CLIP_LAYER, ACT_QUICK_GELU, ClipVisualEncoder, _bf16, _EncoderBase, _live_ptr, check_geometry


class ClipTextEncoder(_EncoderBase):
    LAYER_PREFIX, LAYER_NAMES = "text_model.encoder.layers.{}.", _CLIP_LAYER

    def __init__(self, vocab_size: int = 49408, hidden_size: int = 512, intermediate_size: int = 2048, projection_dim: int = 512,
                 num_hidden_layers: int = 12, num_attention_heads: int = 8, max_position_embeddings: int = 77, hidden_act: str = "quick_gelu",
                 layer_norm_eps: float = 1e-5, attention_dropout: float = 0.0, pad_token_id: int = 1, bos_token_id: int = 49406,
                 eos_token_id: int = 49407):
        """The arguments are CLIPTextConfig's.  eos_token_id selects the pooled position by HF's rule: 2 (the legacy configs) pools the
        first position of the largest id, anything else the first position equal to eos_token_id.  attention_dropout is a training-time
        setting of a model that is frozen here: accepted, never applied."""
        if hidden_act != "quick_gelu":
            raise ValueError(f"hidden_act={hidden_act!r}: ClipTextEncoder is built for CLIP's 'quick_gelu'")
        check_geometry(hidden=("hidden_size", hidden_size), heads=("num_attention_heads", num_attention_heads),
                       intermediate=("intermediate_size", intermediate_size), projection_dim=("projection_dim", projection_dim))
        if num_hidden_layers < 1:
            raise ValueError(f"num_hidden_layers={num_hidden_layers} (>= 1)")
        super().__init__(hidden_size, num_attention_heads, fold_ln=False, residual_dtype="fp32")      # the plain (unfolded-LayerNorm) layer form
        self.layers, self.inter, self.vocab, self.proj, self.eps = num_hidden_layers, intermediate_size, vocab_size, projection_dim, layer_norm_eps
        self.max_position, self.eos_token_id = max_position_embeddings, int(eos_token_id)
        self.pad_token_id, self.bos_token_id = pad_token_id, bos_token_id
        w, T, init = self._w, "text_model.", self._seeded_init()
        w[T + "embeddings.token_embedding.weight"] = init((vocab_size, hidden_size))
        w[T + "embeddings.position_embedding.weight"] = init((max_position_embeddings, hidden_size))
        for i in range(num_hidden_layers):
            P = T + f"encoder.layers.{i}."
            for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
                w[P + f"self_attn.{n}.weight"] = init((hidden_size, hidden_size))
                w[P + f"self_attn.{n}.bias"] = torch.zeros(hidden_size)
            w[P + "layer_norm1.weight"], w[P + "layer_norm1.bias"] = torch.ones(hidden_size), torch.zeros(hidden_size)
            w[P + "mlp.fc1.weight"], w[P + "mlp.fc1.bias"] = init((intermediate_size, hidden_size)), torch.zeros(intermediate_size)
            w[P + "mlp.fc2.weight"], w[P + "mlp.fc2.bias"] = init((hidden_size, intermediate_size)), torch.zeros(hidden_size)
            w[P + "layer_norm2.weight"], w[P + "layer_norm2.bias"] = torch.ones(hidden_size), torch.zeros(hidden_size)
        w[T + "final_layer_norm.weight"], w[T + "final_layer_norm.bias"] = torch.ones(hidden_size), torch.zeros(hidden_size)
        w["text_projection.weight"] = init((projection_dim, hidden_size))

    def _pack(self):
        if self._packed is None:
            # (HF scales q by 1 / sqrt(64) before Q K^T; the attention kernel scales the scores: the same product)
            self._packed = {"layers": self._pack_layers(), "wproj": _bf16(self._w["text_projection.weight"])}
        return self._packed

    def _workbufs(self, B: int, Lq: int) -> dict:
        key = (B, Lq)
        if key not in self._bufs:
            dev, M, H = self.device, B * Lq, self.hidden
            bf, f32, i32 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
            self._bufs[key] = {"xb": torch.empty(M, H, **bf), "xf": torch.empty(M, H, **f32), "hb": torch.empty(M, H, **bf),
                               "qkv": torch.empty(M, 3 * H, **bf), "ctx": torch.empty(M, H, **bf), "m": torch.empty(M, self.inter, **bf),
                               "lh": torch.empty(M, H, **f32), "pooled": torch.empty(B, H, **bf), "emb": torch.empty(B, self.proj, **f32),
                               "feat": torch.empty(B, self.proj, **f32),
                               # ufnd_clip_text_pack: the pooled positions, cu_seqlens (B + 1; cu[B] = the live row count), row -> (b, pos)
                               "e": torch.zeros(B, **i32), "cu": torch.zeros(B + 1, **i32), "row_src": torch.zeros(M, **i32)}
        return self._bufs[key]

    def _run(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool, n_layers: Optional[int] = None, pool: bool = True) -> dict:
        """One pass over a (B, L) batch: pooled positions, embeddings, the first n_layers layers (all by default; 0: none) and, with pool,
        final_layer_norm on the pooled rows, the projection ("emb") and its L2 normalisation ("feat").  Returns the work buffers; the
        residual stream is "xf" (packed: its live rows, in ufnd_clip_text_pack's order)."""
        self._require_hip()
        dev = self.device
        if input_ids.dim() != 2 or tuple(attention_mask.shape) != tuple(input_ids.shape):
            raise ValueError(f"input_ids {tuple(input_ids.shape)} / attention_mask {tuple(attention_mask.shape)}: expected two (B, L) tensors")
        B, Lq = input_ids.shape
        if Lq > self.max_position:
            raise RuntimeError(f"sequence length {Lq} exceeds max_position_embeddings {self.max_position}")
        ids = input_ids.to(dev, torch.int64).contiguous()
        mask = attention_mask.to(dev, torch.int32).contiguous()
        p, b, w, lib = self._pack(), self._workbufs(B, Lq), self._w, L.lib()
        M, H, s, T = B * Lq, self.hidden, L.stream_ptr(dev), "text_model."
        live = _live_ptr(b["cu"]) if packed else None      # packed: every launch runs over the live rows, their count on the device
        L.check(lib.ufnd_clip_text_pack(ids.data_ptr(), B, Lq, self.eos_token_id, b["e"].data_ptr(), b["cu"].data_ptr(), b["row_src"].data_ptr(), s),
                "ufnd_clip_text_pack")
        tables = (w[T + "embeddings.token_embedding.weight"].data_ptr(), w[T + "embeddings.position_embedding.weight"].data_ptr())
        if packed:
            L.check(lib.ufnd_clip_text_embed_live(ids.data_ptr(), b["row_src"].data_ptr(), live, *tables, b["xb"].data_ptr(),
                                                  b["xf"].data_ptr(), M, Lq, H, self.vocab, self.max_position, s), "ufnd_clip_text_embed_live")
        else:
            L.check(lib.ufnd_clip_text_embed(ids.data_ptr(), *tables, b["xb"].data_ptr(), b["xf"].data_ptr(), B, Lq, H, self.vocab, self.max_position, s),
                    "ufnd_clip_text_embed")
        layers = p["layers"] if n_layers is None else p["layers"][:max(0, int(n_layers))]
        if packed:
            attend = self._two_launch(b, "ufnd_attention_bf16_causal_varlen", operands=(b["cu"], mask), B=B, Lq=Lq, live=live)
        else:
            attend = self._two_launch(b, "ufnd_attention_bf16_causal", operands=(mask,), B=B, Lq=Lq)
        self._pre_ln_blocks(layers, b, attend, M, ACT_QUICK_GELU, live=live)
        if pool:
            L.check(lib.ufnd_clip_text_pool(b["xf"].data_ptr(), b["e"].data_ptr(), b["cu"].data_ptr() if packed else None,
                                            w[T + "final_layer_norm.weight"].data_ptr(), w[T + "final_layer_norm.bias"].data_ptr(), b["pooled"].data_ptr(),
                                            B, Lq, H, self.eps, s), "ufnd_clip_text_pool")
            self._gemm(b["pooled"], p["wproj"], None, out_f32=b["emb"])
            L.check(lib.ufnd_l2norm_frames(b["emb"].data_ptr(), b["feat"].data_ptr(), B, 1, self.proj, s), "ufnd_l2norm_frames")      # x / (||x|| + 1e-9)
        return b

    @torch.no_grad()
    def pooled_positions(self, input_ids: torch.Tensor) -> torch.Tensor:
        """e(b), the pooled (EOS) position of each sample by HF's rule for this encoder's eos_token_id: (B,) int32 (a copy)."""
        return self._run(input_ids, torch.ones_like(input_ids), packed=True, n_layers=0, pool=False)["e"].clone()

    @torch.no_grad()
    def last_hidden_state(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool = False, n_layers: Optional[int] = None) -> torch.Tensor:
        """(B, L, H) fp32 (a copy).  n_layers=None: CLIPTextModel's last_hidden_state (final_layer_norm applied); n_layers=k: its
        hidden_states[k], the residual stream after k layers (0: the embeddings), for per-layer localisation in the tests.  The packed
        pass computes rows 0 .. e(b) of each sample; the others are zero (reads the live row count: one host sync)."""
        b = self._run(input_ids, attention_mask, packed=packed, n_layers=n_layers, pool=False)
        B, Lq = input_ids.shape
        src = b["xf"]
        if n_layers is None:
            w, T = self._w, "text_model."
            self._ln(b["xf"], self.hidden, w[T + "final_layer_norm.weight"], w[T + "final_layer_norm.bias"], None, b["lh"], B * Lq, self.hidden, self.eps,
                     m_live=_live_ptr(b["cu"]) if packed else None)
            src = b["lh"]
        if not packed:
            return src.view(B, Lq, self.hidden).clone()
        n = int(b["cu"][B].item())
        out = torch.zeros(B * Lq, self.hidden, dtype=torch.float32, device=self.device)
        out[b["row_src"][:n].long()] = src[:n]
        return out.view(B, Lq, self.hidden)

    @torch.no_grad()
    def pooled(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool = True) -> torch.Tensor:
        """final_layer_norm of row e(b) as the projection GEMM reads it (rounded to bf16): (B, H) fp32 (a copy; for the tests)."""
        return self._run(input_ids, attention_mask, packed=packed)["pooled"].float()

    @torch.no_grad()
    def text_embeds(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool = True) -> torch.Tensor:
        """CLIPTextModelWithProjection.text_embeds: the un-normalised projected features (B, projection_dim) (a view of an internal
        buffer, valid until the next call with the same shape)."""
        return self._run(input_ids, attention_mask, packed=packed)["emb"]

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool = True) -> torch.Tensor:
        """(B, L) ids / mask -> (B, projection_dim) features x / (||x|| + 1e-9), the reference's l2n(get_text_features(...)) (a view of
        an internal buffer, valid until the next call with the same shape).  packed=True: the live-row pass (module docstring),
        bit-identical to packed=False, the padded computation."""
        return self._run(input_ids, attention_mask, packed=packed)["feat"]


@dataclass
class SemanticConfig:
    """The reference's SemanticConfig (src/models/semantic_forgery.py:21-27).  model_name / use_fast name a checkpoint and a tokenizer,
    which stay outside this package; dropout is never applied (SemanticForgeryAnalyzer)."""
    model_name: str = "openai/clip-vit-base-patch32"
    proj_dim: int = 512
    dropout: float = 0.3
    use_fast: bool = True
    max_length: int = 64


class SemanticForgeryAnalyzer(nn.Module):
    """The reference's text-visual semantic consistency module on the GPU.

    forward(batch) takes token ids instead of strings (tokenise with the CLIP tokenizer, truncation to cfg.max_length):
      title_ids / title_mask (B, L)       the title
      ocr_ids / ocr_mask (B, L')          the OCR text, the reference's "text as a proxy for vision" image side; or
      frames (B, 3, S, S) / (B, F, 3, S, S)   the frames themselves: the image side is l2n(ClipVisualEncoder.image_embeds), for several
                                          frames their mean, L2-normalised again
    and returns the reference's semantic_text, semantic_image, semantic_gap (B, proj_dim) plus clip_similarity (B,), the cosine of the two
    sides in CLIP's joint space (CLIPModel's logits_per_text diagonal without logit_scale), and semantic_conflict = 1 - (cos + 1) / 2.

    Always eval-mode arithmetic: the reference's Dropout(0.3) behind each projection is a training-time regulariser of a module it never
    trains (no optimizer sees these parameters, fusion keeps them as dead tensors), so it is not applied in any mode.
    Parameters: text_proj.0.{weight,bias}, vision_proj.0.{weight,bias}, the reference's names."""

    def __init__(self, cfg: Optional[SemanticConfig] = None, device="cuda", text_encoder: Optional[ClipTextEncoder] = None,
                 visual_encoder: Optional[ClipVisualEncoder] = None):
        super().__init__()
        self.cfg = cfg or SemanticConfig()
        if self.cfg.proj_dim % 32 or self.cfg.proj_dim < 32:
            raise ValueError(f"proj_dim={self.cfg.proj_dim}: a multiple of 32")
        # construction order == the reference's, so the RNG stream matches
        self.text_proj = nn.Sequential(nn.Linear(512, self.cfg.proj_dim))
        self.vision_proj = nn.Sequential(nn.Linear(512, self.cfg.proj_dim))
        self.out_dim = self.cfg.proj_dim
        self.text_encoder = text_encoder if text_encoder is not None else ClipTextEncoder()
        self.visual_encoder = visual_encoder      # built on first use with frames
        if self.text_encoder.proj != 512:
            raise ValueError(f"text encoder projects to {self.text_encoder.proj}, the head takes 512")
        self.to(device)

    @classmethod
    def from_fusion(cls, fusion, **kwargs) -> "SemanticForgeryAnalyzer":
        """An analyzer whose head IS fusion.semantic: the four `semantic.*` tensors a reference checkpoint carries through
        CrossModalTransformer (shared modules, shared storage)."""
        sem = fusion.semantic
        D = sem.text_proj[0].out_features
        dev = sem.text_proj[0].weight.device
        self = cls(SemanticConfig(proj_dim=D), device=dev, **kwargs)
        self.text_proj, self.vision_proj = sem.text_proj, sem.vision_proj
        return self

    def _ids(self, batch: Dict[str, torch.Tensor], name: str):
        ids, mask = batch[name + "_ids"], batch.get(name + "_mask")
        if mask is None:
            raise KeyError(f"{name}_mask")
        if ids.shape[1] > self.cfg.max_length:
            raise ValueError(f"{name}_ids: {ids.shape[1]} tokens, max_length={self.cfg.max_length} (tokenise with truncation)")
        return ids, mask

    @torch.no_grad()
    def head(self, text_feat: torch.Tensor, image_feat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The head alone on (B, 512) fp32 features of the two sides (the reference's forward past encode_text)."""
        wt, bt, wi, bi = self.text_proj[0].weight, self.text_proj[0].bias, self.vision_proj[0].weight, self.vision_proj[0].bias
        dev = L.require_hip(text_feat, image_feat, wt, bt, wi, bi)
        t, i = L.f32c(text_feat), L.f32c(image_feat)
        B, D = t.shape[0], wt.shape[0]
        if tuple(t.shape) != (B, 512) or tuple(i.shape) != (B, 512):
            raise ValueError(f"features: expected two (B, 512) tensors, got {tuple(t.shape)} and {tuple(i.shape)}")
        ws = torch.empty(2, B, D, dtype=torch.float32, device=dev)
        out = torch.empty(3, B, D, dtype=torch.float32, device=dev)
        sc = torch.empty(2, B, dtype=torch.float32, device=dev)
        s = L.stream_ptr(dev)
        L.check(L.lib().ufnd_semantic_head(t.data_ptr(), i.data_ptr(), wt.data_ptr(), bt.data_ptr(), wi.data_ptr(), bi.data_ptr(), ws.data_ptr(),
                                           out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), B, D, 512, s), "ufnd_semantic_head")
        L.check(L.lib().ufnd_clip_similarity(t.data_ptr(), i.data_ptr(), sc[0].data_ptr(), sc[1].data_ptr(), B, 512, s), "ufnd_clip_similarity")
        return {"semantic_text": out[0], "semantic_image": out[1], "semantic_gap": out[2], "clip_similarity": sc[0], "semantic_conflict": sc[1]}

    @torch.no_grad()
    def forward(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        txt = self.text_encoder(*self._ids(batch, "title")).clone()      # (the encoder's buffer is reused by the OCR pass)
        if batch.get("frames") is not None:
            if self.visual_encoder is None:
                self.visual_encoder = ClipVisualEncoder().to(txt.device)
            img = self.visual_encoder(batch["frames"])
        elif batch.get("ocr_ids") is not None:
            img = self.text_encoder(*self._ids(batch, "ocr"))
        else:
            raise KeyError("batch needs ocr_ids / ocr_mask or frames for the image side")
        return self.head(txt, img)
