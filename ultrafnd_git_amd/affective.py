"""The RoBERTa emotion classifier and AffectiveForensics, MI355X-native.

  RobertaEmotionClassifier  transformers.RobertaForSequenceClassification in the geometry the reference names
                            (configs/model_configs/affective.yaml: 6 post-LN layers, hidden 768, 12 heads, 7 labels), frozen and
                            forward-only: (B, L) ids / mask -> (B, num_labels) logits.  It runs on BertTextEncoder's machinery -- the
                            one layer table, the one post-LN layer loop with folded LayerNorms, the packed live-row pass, the fused
                            Q/K/V + attention tiles -- and adds RoBERTa's embedding rule (position ids counted over the non-pad ids
                            and offset by the pad id), the classification head (dense -> tanh -> out_proj on the <s> row, all fp32)
                            and the class-row tail below.  Tokenisation stays outside (ids / mask in), there is no tokenizer
                            vocabulary offline.
  AffectiveForensics        the reference's module of that name (src/models/affective_forensics.py), batched: softmax, the label
                            grouping into fear / anger / joy, text_intensity, the RMS-energy audio arousal, intensity and valence,
                            as device tensors.  The lexicon fallback and the librosa.pyin arousal branch are not built.

Weights keep HF's `state_dict` names, so a RobertaForSequenceClassification checkpoint loads with strict=True.

The class-row tail (`cls_tail`).  A sequence classifier reads one row per sample, the <s> row.  Keys and values need every row, so a
layer's attention runs over all of them; past the LAST layer's attention nothing but the B class rows is read.  ufnd_gather_class_rows
copies those rows -- stream row cu[b] of the packed pass, row b L of the padded one -- of ctx, the residual and (folded) its
statistics partials into compact B-row buffers, and the out-projection, FFN1, FFN2 and the final LayerNorm run on B rows.  A row's
arithmetic does not depend on the launch it is part of, so the logits are bit-identical to the all-rows pass.

A sample whose mask keeps nothing has no rows in the packed pass; its features count as zero in both passes (the head's text_valid),
so packed and padded logits agree for it too.  No host synchronisation, fixed launch geometry: a call is hipGraph-capturable; the
returned tensors are internal buffers, valid until the next call with the same shape.  No CPU path.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional, Sequence

import torch

from . import _lib as L
from .encoders import BertTextEncoder, check_geometry

# the reference's substring rules (affective_forensics.py:94-97), in group order: 0 fear, 1 anger, 2 joy
GROUP_RULES = (("fear", "anx", "worr", "scare"), ("anger", "annoy", "mad", "rage"), ("joy", "happi", "delight", "amuse"))
# the seven labels of the emotion model the reference names, in id order -- recalled, not verified offline; a default only
DEFAULT_ID2LABEL = ("anger", "disgust", "fear", "joy", "neutral", "sadness", "surprise")


def group_table(names: Sequence[str]) -> list:
    """The head's group entry per label, from the reference's substring rules on the lower-cased names: -1 none, 0 fear, 1 anger,
    2 joy; a name that matches several groups counts in each, as in the reference: 4 + m with m = bit 0 fear | bit 1 anger | bit 2 joy."""
    out = []
    for n in names:
        n = str(n).lower()
        hits = [g for g, keys in enumerate(GROUP_RULES) if any(k in n for k in keys)]
        out.append(-1 if not hits else hits[0] if len(hits) == 1 else 4 + sum(1 << g for g in hits))
    return out


class RobertaEmotionClassifier(BertTextEncoder):
    LAYER_PREFIX = "roberta.encoder.layer.{}."

    def __init__(self, num_hidden_layers: int = 6, hidden_size: int = 768, num_attention_heads: int = 12, intermediate_size: int = 3072,
                 vocab_size: int = 50265, max_position_embeddings: int = 514, type_vocab_size: int = 1, layer_norm_eps: float = 1e-5,
                 pad_token_id: int = 1, num_labels: int = 7, fold_ln: bool = True, residual_dtype: str = "bf16"):
        """The arguments are RobertaConfig's, plus fold_ln / residual_dtype as the other encoders take them."""
        if not 1 <= num_labels <= 32 or num_hidden_layers < 1 or pad_token_id < 0 or max_position_embeddings - pad_token_id - 1 < 1:
            raise ValueError(f"num_labels={num_labels} (1 .. 32), num_hidden_layers={num_hidden_layers} (>= 1), pad_token_id={pad_token_id}, "
                             f"max_position_embeddings={max_position_embeddings}")
        check_geometry(hidden=("hidden_size", hidden_size), heads=("num_attention_heads", num_attention_heads),
                       intermediate=("intermediate_size", intermediate_size))
        super().__init__(layers=num_hidden_layers, hidden=hidden_size, heads=num_attention_heads, intermediate=intermediate_size,
                         vocab_size=vocab_size, max_position=max_position_embeddings, type_vocab=type_vocab_size, eps=layer_norm_eps,
                         fold_ln=fold_ln, residual_dtype=residual_dtype)
        self.pad_token_id, self.num_labels = int(pad_token_id), int(num_labels)
        # past its attention the last layer runs over the B class rows only (module docstring); bit-identical logits (off: all rows)
        self.cls_tail = True
        init = self._seeded_init()
        w = OrderedDict(("roberta." + k, v) for k, v in self._w.items())
        w["classifier.dense.weight"], w["classifier.dense.bias"] = init((hidden_size, hidden_size)), torch.zeros(hidden_size)
        w["classifier.out_proj.weight"], w["classifier.out_proj.bias"] = init((num_labels, hidden_size)), torch.zeros(num_labels)
        self._w = w

    def load_state_dict(self, sd, strict: bool = True):
        unexpected = [k for k in sd if k not in self._w]
        if strict and unexpected:
            raise RuntimeError(f"unexpected keys: {unexpected[:5]}{'...' if len(unexpected) > 5 else ''}")
        return super().load_state_dict(sd, strict)

    def _check_length(self, Lq: int) -> None:
        most = self.max_position - self.pad_token_id - 1      # position ids run to L + pad_token_id
        if Lq > most:
            raise RuntimeError(f"sequence length {Lq} exceeds max_position_embeddings - pad_token_id - 1 = {most}")

    def _workbufs(self, B: int, Lq: int) -> dict:
        fresh = (B, Lq) not in self._bufs
        b = super()._workbufs(B, Lq)
        if fresh:
            dev, H, C = self.device, self.hidden, self.num_labels
            bf, f32, i32 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
            b.update({"pos": torch.zeros(B * Lq, **i32), "valid": torch.zeros(B, **i32), "head_ws": torch.empty(B, H, **f32),
                      "logits": torch.empty(B, C, **f32), "class_probs": torch.empty(B, C, **f32), "probs": torch.empty(B, 3, **f32),
                      "text_intensity": torch.empty(B, **f32), "intensity": torch.empty(B, **f32), "valence": torch.empty(B, **f32)})
            # the class rows' compact buffers: the gathered copies (ctx, rb / rf: the residual, rst: its statistics) and what the last
            # layer writes past its attention, under the work buffers' names
            c = {"ctx": torch.empty(B, H, **bf), "rb": torch.empty(B, H, **bf), "rf": torch.empty(B, H, **f32), "y": torch.empty(B, H, **f32),
                 "x1b": torch.empty(B, H, **bf), "x1f": torch.empty(B, H, **f32), "h": torch.empty(B, self.inter, **bf),
                 "xb": torch.empty(B, H, **bf), "xf": torch.empty(B, H, **f32)}
            if "st" in b:
                p1 = b["st"].shape[2]
                if self._fold_parts(B) != p1:      # (tests/test_gpu_vit_cls_tail.py: the GEMMs' partial count does not depend on the row count)
                    raise L.UltrafndHipError(f"the GEMMs write {self._fold_parts(B)} statistics partials at {B} rows and {p1} at {B * Lq}")
                c.update({"y1b": torch.empty(B, H, **bf), "y2": torch.empty(B, H, **f32), "y2b": torch.empty(B, H, **bf),
                          "rst": torch.zeros(B, p1, 2, **f32), "st1": torch.zeros(B, p1, 2, **f32), "st2": torch.zeros(B, p1, 2, **f32)})
            b["cls"] = c
        return b

    def _pack_embed(self, ids, mask, b, B: int, Lq: int, packed: bool, fuse: bool, tiled: bool, live) -> None:
        """Position ids by HF's rule, then LayerNorm(word + position + token_type[0]).  The packed pass without the fused attention gets
        cu_seqlens / row_src from the position-id launch; with it (L == 128) the text pass's own pack entry writes them with the slot
        bins / sample tiles, and the position-id launch follows."""
        w, H, s, lib = self._w, self.hidden, L.stream_ptr(self.device), L.lib()
        own = packed and not fuse
        if packed and fuse:
            self._pack_rows(mask, b, B, Lq, fuse, tiled)
        L.check(lib.ufnd_roberta_pack(ids.data_ptr(), mask.data_ptr(), B, Lq, self.pad_token_id, b["cu"].data_ptr() if own else None,
                                      b["row_src"].data_ptr() if own else None, b["pos"].data_ptr(), b["valid"].data_ptr(), s), "ufnd_roberta_pack")
        tables = [w["roberta.embeddings." + n].data_ptr() for n in ("word_embeddings.weight", "position_embeddings.weight",
                                                                      "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")]
        outs, geom = self._embed_outs(b), (Lq, H, self.vocab, self.max_position, self.pad_token_id, self.eps, s)
        if packed:
            L.check(lib.ufnd_roberta_embed_live(ids.data_ptr(), b["pos"].data_ptr(), b["row_src"].data_ptr(), live, *tables, *outs, B * Lq, *geom),
                    "ufnd_roberta_embed_live")
        else:
            L.check(lib.ufnd_roberta_embed(ids.data_ptr(), b["pos"].data_ptr(), *tables, *outs, B, *geom), "ufnd_roberta_embed")

    def _gather(self, b, cu, B: int, Lq: int, ctx=None, rb=None, rf=None, st=None) -> None:
        """ufnd_gather_class_rows: each argument a (source, destination) pair or None."""
        flat = [L.ptr(t) for pair in (ctx, rb, rf, st) for t in (pair if pair is not None else (None, None))]
        L.check(L.lib().ufnd_gather_class_rows(L.ptr(cu), *flat, B, Lq, self.hidden, st[0].shape[1] * 2 if st is not None else 0, B * Lq,
                                               L.stream_ptr(self.device)), "ufnd_gather_class_rows")

    def _tail(self, b, cu, B: int, Lq: int):
        """The layer loops' tail: gather the class rows of ctx and of the residual side the loop names into the compact buffers."""
        c = b["cls"]

        def tail(res_bf16, res_f32, stats):
            self._gather(b, cu, B, Lq, ctx=(b["ctx"], c["ctx"]), rb=None if res_bf16 is None else (res_bf16, c["rb"]),
                         rf=None if res_f32 is None else (res_f32, c["rf"]), st=None if stats is None else (stats, c["rst"]))
            return c
        return tail

    def _classify(self, input_ids, attention_mask, packed: bool, group: Optional[torch.Tensor] = None, arousal: Optional[torch.Tensor] = None) -> dict:
        """The pass, the class rows of last_hidden_state in b["cls"]["xf"], then the head.  With group (the int32 table), AffectiveForensics'
        outputs are written too."""
        b = self._pass(input_ids, attention_mask, packed=packed, pool=False, tail=self._tail if self.cls_tail else None)
        B, Lq = input_ids.shape
        c, w = b["cls"], self._w
        if not self.cls_tail:
            self._gather(b, b["cu"] if packed else None, B, Lq, rf=(b["xf"], c["xf"]))
        extra = [b[k].data_ptr() if group is not None else None for k in ("probs", "text_intensity", "intensity", "valence")]
        L.check(L.lib().ufnd_emotion_head(c["xf"].data_ptr(), w["classifier.dense.weight"].data_ptr(), w["classifier.dense.bias"].data_ptr(),
                                          w["classifier.out_proj.weight"].data_ptr(), w["classifier.out_proj.bias"].data_ptr(), L.ptr(group),
                                          b["valid"].data_ptr(), L.ptr(arousal), b["head_ws"].data_ptr(), b["logits"].data_ptr(),
                                          b["class_probs"].data_ptr(), *extra, B, self.hidden, self.num_labels, L.stream_ptr(self.device)),
                "ufnd_emotion_head")
        return b

    @torch.no_grad()
    def logits(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool = True) -> torch.Tensor:
        """RobertaForSequenceClassification(input_ids, attention_mask).logits -> (B, num_labels) fp32.  packed (default): over the rows
        the mask keeps up to each sample's last kept position, bit-identical to the padded pass."""
        return self._classify(input_ids, attention_mask, packed)["logits"]

    forward = encode_batch = logits

    @torch.no_grad()
    def probs(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, packed: bool = True) -> torch.Tensor:
        """softmax(logits) -> (B, num_labels) fp32."""
        return self._classify(input_ids, attention_mask, packed)["class_probs"]

    @torch.no_grad()
    def last_hidden_state(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, n_layers: Optional[int] = None) -> torch.Tensor:
        """RobertaModel's last_hidden_state -> (B, L, H) fp32, every row, the padded pass (a view of an internal buffer).  n_layers=k:
        hidden_states[k], k >= 1 (per-layer localisation in the parity tests); embeddings() is hidden_states[0]."""
        return self._pass(input_ids, attention_mask, packed=False, n_layers=n_layers, pool=False)["xf"].view(*input_ids.shape, self.hidden)

    @torch.no_grad()
    def embeddings(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """RobertaModel's hidden_states[0] -> (B, L, H) fp32 (a fresh tensor)."""
        self._require_hip()
        B, Lq = input_ids.shape
        self._check_length(Lq)
        dev = self.device
        ids, mask = input_ids.to(dev, torch.int64).contiguous(), attention_mask.to(dev, torch.int32).contiguous()
        b = dict(self._workbufs(B, Lq))
        b["xf"] = torch.empty(B * Lq, self.hidden, dtype=torch.float32, device=dev)
        b.pop("st", None)      # (so that _embed_outs names the fp32 rows)
        self._pack_embed(ids, mask, b, B, Lq, False, False, False, None)
        return b["xf"].view(B, Lq, self.hidden)

    def encode_fields(self, *args, **kwargs):
        raise NotImplementedError("RobertaEmotionClassifier is a sequence classifier: logits / probs / last_hidden_state")


@torch.no_grad()
def audio_arousal(audio: torch.Tensor, audio_lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """clip(sigmoid(5 mean(x^2)), 0, 1) per clip (the reference's RMS-energy branch, affective_forensics.py:127-128): audio (B, T) fp32 on
    a HIP device, audio_lengths (B) the valid samples of each clip (None: T) -> (B,) fp32 (out, or a fresh tensor).  A clip is
    computed as if alone; a clip without samples gives sigmoid(0) = 0.5."""
    x = L.f32c(audio)
    dev = L.require_hip(x, out)
    if x.dim() != 2:
        raise ValueError(f"audio {tuple(audio.shape)}: expected (B, T)")
    B, T = x.shape
    lens = None if audio_lengths is None else audio_lengths.to(dev, torch.int32).contiguous()
    if lens is not None and lens.numel() != B:
        raise ValueError(f"audio_lengths holds {lens.numel()} entries for {B} clips")
    if T == 0:      # (clips without samples: length 0 of a one-sample row)
        x, T, lens = torch.zeros(B, 1, dtype=torch.float32, device=dev), 1, torch.zeros(B, dtype=torch.int32, device=dev)
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    L.check(L.lib().ufnd_audio_arousal(x.data_ptr(), L.ptr(lens), out.data_ptr(), B, T, L.stream_ptr(dev)), "ufnd_audio_arousal")
    return out


class AffectiveForensics:
    """Batched AffectiveForensics.analyze (src/models/affective_forensics.py:130-148) on pre-tokenised text.

    classifier: a RobertaEmotionClassifier (default: the reference's geometry with placeholder weights -- load a checkpoint).
    id2label: the label names in id order, or a dict id -> name.  The default is the seven labels of the emotion model the reference
    names -- anger, disgust, fear, joy, neutral, sadness, surprise -- an order recalled from that model's card and NOT verified on
    an offline machine: pass the checkpoint's own config.id2label.  The reference's substring rules are applied to the names once,
    here, on the host (group_table)."""

    def __init__(self, classifier: Optional[RobertaEmotionClassifier] = None, id2label=None, device="cuda"):
        self.device = torch.device(device)
        self.classifier = (classifier if classifier is not None else RobertaEmotionClassifier()).to(self.device)
        C = self.classifier.num_labels
        if id2label is None:
            id2label = DEFAULT_ID2LABEL
        if isinstance(id2label, dict):      # (the reference: labels.get(i, str(i)); HF configs key by int, their JSON by str)
            id2label = [id2label.get(i, id2label.get(str(i), str(i))) for i in range(C)]
        if len(id2label) != C:
            raise ValueError(f"id2label names {len(id2label)} labels, the classifier has {C}")
        self.labels = [str(n) for n in id2label]
        self.groups = group_table(self.labels)
        self._group_dev = torch.tensor(self.groups, dtype=torch.int32, device=self.device)
        self._arousal: Dict[int, torch.Tensor] = {}

    def audio_arousal(self, audio: torch.Tensor, audio_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """audio_arousal (above) on this module's device, into an internal buffer per batch size."""
        B = audio.shape[0]
        out = self._arousal.get(B)
        if out is None:
            out = self._arousal[B] = torch.empty(B, dtype=torch.float32, device=self.device)
        return audio_arousal(audio.to(self.device), audio_lengths, out=out)

    @torch.no_grad()
    def analyze_batch(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, audio: Optional[torch.Tensor] = None,
                      audio_lengths: Optional[torch.Tensor] = None, packed: bool = True) -> Dict[str, torch.Tensor]:
        """class_probs (B, C), probs (B, 3) = [fear, anger, joy] / (f + a + j + 1e-9), text_intensity, arousal, intensity, valence (B,).
        A sample whose mask row is all zero is the reference's `if not text`: probs 0, text_intensity 0.5.  audio=None: arousal 0.5."""
        B = input_ids.shape[0]
        if audio is None:
            arousal = None
        else:
            arousal = self.audio_arousal(audio, audio_lengths)
            if arousal.shape[0] != B:
                raise ValueError(f"audio holds {arousal.shape[0]} clips for {B} texts")
        b = self.classifier._classify(input_ids, attention_mask, packed, group=self._group_dev, arousal=arousal)
        out = {k: b[k] for k in ("class_probs", "probs", "text_intensity", "intensity", "valence")}
        out["arousal"] = arousal if arousal is not None else torch.full((B,), 0.5, dtype=torch.float32, device=self.device)
        return out

    def get_emotion_intensity(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, audio: Optional[torch.Tensor] = None,
                              audio_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.analyze_batch(input_ids, attention_mask, audio, audio_lengths)["intensity"]
