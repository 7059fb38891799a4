"""The geometry table of tests/test_gpu_encoder_geometry.py, shared with the CPU tests that hold it to its purpose
(tests/test_encoder_geometry_census.py: every form of the pass is reached; the tests/test_*_ref.py files: every input is admissible).

The four frozen encoders take their geometry as constructor arguments, and the form of a pass changes with it: folded LayerNorms with
8, 16 or 24 statistics partials per row or, at hidden 1024, the unfolded fallback; fused Q/K/V + attention or two launches; the
class-row tails over folded or unfolded buffers; row kernels with NI = hidden / 256 = 1 .. 4.  Every case has 2 layers, a vocabulary
of 512, seeded weights with a non-trivial affine everywhere (each family's case_weights) and 3 to 5 samples.

The form a case takes is READ from the encoder (form_of, below: _workbufs' statistics buffers, _fuses), never restated here.
Nothing in this file touches a GPU: an encoder built on the CPU answers every question about its dispatch.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

LAYERS, VOCAB = 2, 512
# (hidden, heads, intermediate).  640 is a multiple of 64 and 128 but not of 192 or 256; 768 is the control
WIDTHS = ((256, 4, 640), (512, 8, 2048), (768, 12, 3072), (1024, 16, 4096))
PROJ = {256: 192, 512: 512, 1024: 1024}      # projection_dim where the class has one (768: the class's default)
LABELS = {256: 1, 512: 32, 768: 7, 1024: 7}  # num_labels of the RoBERTa cases: 1, 7 and 32
FORMS = {"folded-bf16": (True, "bf16"), "folded-fp32": (True, "fp32"), "unfolded": (False, "fp32")}


# ---------------------------------------------------------------------------------------------------------------------
# BertTextEncoder / RobertaEmotionClassifier
@dataclass(frozen=True)
class TextCase:
    kind: str                 # "bert" | "roberta"
    hidden: int
    heads: int
    inter: int
    L: int                    # 40: two-launch attention; 128: the fused forms
    fold_ln: bool = True
    residual_dtype: str = "bf16"

    @property
    def id(self) -> str:
        return f"{self.kind}-h{self.hidden}-L{self.L}-{'fold' if self.fold_ln else 'nofold'}-{self.residual_dtype}"

    @property
    def lengths(self) -> Tuple[int, ...]:
        """prefix masks: one row, the 16-row MFMA tile and its neighbour, L - 1 and L, in one batch"""
        return (1, 16, 17, self.L - 1, self.L)

    @property
    def labels(self) -> int:
        return LABELS[self.hidden]


def _text_cases(kind: str):
    out = []
    for h, nh, it in WIDTHS:
        for L in (40, 128):
            out.append(TextCase(kind, h, nh, it, L))
        if h in (768, 1024):      # the other residual dtype: folded with the fp32 stream at 768, the unfolded fallback under both names at 1024
            out.append(TextCase(kind, h, nh, it, 40, residual_dtype="fp32"))
    out.append(TextCase(kind, 768, 12, 3072, 40, fold_ln=False, residual_dtype="fp32"))      # unfolded by request, at the control width
    return tuple(out)


BERT_CASES = _text_cases("bert")
ROBERTA_CASES = _text_cases("roberta")
FIELDS_WIDTHS = (256, 1024)      # encode_fields once at each


def text_encoder(c: TextCase):
    """The case's encoder on the CPU, with the family's test weights loaded."""
    from tests import affective_ref as AR
    if c.kind == "bert":
        from ultrafnd_git_amd.encoders import BertTextEncoder
        enc = BertTextEncoder(layers=LAYERS, hidden=c.hidden, heads=c.heads, intermediate=c.inter, vocab_size=VOCAB, max_position=128,
                              fold_ln=c.fold_ln, residual_dtype=c.residual_dtype)
        enc.load_state_dict(text_weights(c.kind, c.hidden, c.heads, c.inter))
        return enc
    from ultrafnd_git_amd.affective import RobertaEmotionClassifier
    enc = RobertaEmotionClassifier(num_hidden_layers=LAYERS, hidden_size=c.hidden, num_attention_heads=c.heads, intermediate_size=c.inter,
                                   vocab_size=VOCAB, max_position_embeddings=AR.MAX_POS, num_labels=c.labels, fold_ln=c.fold_ln,
                                   residual_dtype=c.residual_dtype)
    enc.load_state_dict(text_weights(c.kind, c.hidden, c.heads, c.inter))
    return enc


@functools.lru_cache(maxsize=None)
def text_weights(kind: str, hidden: int, heads: int, inter: int):
    from tests import affective_ref as AR
    if kind == "bert":
        from ultrafnd_git_amd.encoders import BertTextEncoder
        sd = BertTextEncoder(layers=LAYERS, hidden=hidden, heads=heads, intermediate=inter, vocab_size=VOCAB, max_position=128).state_dict()
        sd = AR.case_weights({**sd, "classifier.dense.weight": torch.zeros(1), "classifier.out_proj.weight": torch.zeros(1)})
        return {k: v for k, v in sd.items() if not k.startswith("classifier.")}
    from ultrafnd_git_amd.affective import RobertaEmotionClassifier
    return AR.case_weights(RobertaEmotionClassifier(num_hidden_layers=LAYERS, hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter,
                                                    vocab_size=VOCAB, max_position_embeddings=AR.MAX_POS, num_labels=LABELS[hidden]).state_dict())


def text_batch(c: TextCase):
    """(ids, mask), both (5, L) int64: prefix masks of the case's lengths.  RoBERTa: <s> words </s>, pad after (affective_ref.make_batch);
    BERT: id 101 % VOCAB in column 0, words after, and words (never read) behind the mask too."""
    from tests import affective_ref as AR
    if c.kind == "roberta":
        return AR.make_batch(c.lengths, c.L, seed=c.hidden + c.L, vocab=VOCAB)
    g = torch.Generator().manual_seed(c.hidden + c.L)
    ids = torch.randint(0, VOCAB, (len(c.lengths), c.L), generator=g)
    ids[:, 0] = 101
    mask = (torch.arange(c.L)[None, :] < torch.tensor(c.lengths)[:, None]).long()
    return ids, mask


# ---------------------------------------------------------------------------------------------------------------------
# ClipVisualEncoder
@dataclass(frozen=True)
class VitCase:
    hidden: int
    heads: int
    inter: int
    patch: int = 32
    image: int = 224
    fold_ln: bool = True
    residual_dtype: str = "bf16"

    @property
    def tokens(self) -> int:
        return (self.image // self.patch) ** 2 + 1

    @property
    def proj(self) -> int:
        return PROJ.get(self.hidden, 512)

    @property
    def id(self) -> str:
        return f"vit-h{self.hidden}-T{self.tokens}-p{self.patch}-{'fold' if self.fold_ln else 'nofold'}-{self.residual_dtype}"


# tokens: (patch, image).  17: the patch GEMM's K = 192; 65: the first count past the fused form
VIT_TOKENS = {2: (32, 32), 5: (32, 64), 17: (8, 32), 50: (32, 224), 65: (32, 256), 197: (16, 224)}
VIT_CASES = tuple([VitCase(h, nh, it) for h, nh, it in WIDTHS]
                  + [VitCase(768, 12, 3072, *VIT_TOKENS[t]) for t in (2, 5, 17, 65, 197)]
                  + [VitCase(1024, 16, 4096, *VIT_TOKENS[65]), VitCase(256, 4, 640, *VIT_TOKENS[197])]      # the two cross cases
                  + [VitCase(768, 12, 3072, residual_dtype="fp32"), VitCase(768, 12, 3072, fold_ln=False, residual_dtype="fp32"),
                     VitCase(1024, 16, 4096, residual_dtype="fp32"), VitCase(768, 12, 3072, *VIT_TOKENS[65], fold_ln=False, residual_dtype="fp32")])
VIT_BATCHES = ((1, 1), (3, 1), (2, 2))      # (B, F): N = 1 and N = 3 frames, and one batch of two clips of two frames
VIT_HF_PINS = (VitCase(256, 4, 640, *VIT_TOKENS[197]), VitCase(768, 12, 3072, *VIT_TOKENS[17]))      # the two geometries HF pins the yardstick at


@functools.lru_cache(maxsize=None)
def vit_weights(hidden: int, heads: int, inter: int, patch: int, image: int, proj: int):
    from tests import vit_ref as VR
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    return VR.case_weights(ClipVisualEncoder(layers=LAYERS, hidden=hidden, heads=heads, intermediate=inter, patch=patch, image=image,
                                             projection_dim=proj).state_dict())


def vit_encoder(c: VitCase):
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    enc = ClipVisualEncoder(layers=LAYERS, hidden=c.hidden, heads=c.heads, intermediate=c.inter, patch=c.patch, image=c.image,
                            projection_dim=c.proj, fold_ln=c.fold_ln, residual_dtype=c.residual_dtype)
    enc.load_state_dict(vit_weights(c.hidden, c.heads, c.inter, c.patch, c.image, c.proj))
    return enc


def vit_frames(c: VitCase, B: int, Fr: int) -> torch.Tensor:
    from tests import vit_ref as VR
    return VR.make_frames(B, Fr, c.image, seed=c.hidden + c.tokens + 10 * B + Fr)


# ---------------------------------------------------------------------------------------------------------------------
# ClipTextEncoder
@dataclass(frozen=True)
class ClipTextCase:
    hidden: int
    heads: int
    inter: int
    proj: int
    L: int = 77
    max_pos: int = 77
    e_list: Tuple[int, ...] = (1, 15, 16, 63, 64, 76)

    @property
    def id(self) -> str:
        return f"cliptext-h{self.hidden}-L{self.L}"

    @property
    def batches(self):
        """the pooled positions, in batches of at most five samples"""
        e = self.e_list
        return (e,) if len(e) <= 5 else (e[:len(e) // 2], e[len(e) // 2:])


LONG_E = (127, 128, 191, 192)      # the long tower's pooled positions: the key-block / query-workgroup edges from both sides, and L - 1
CLIP_TEXT_CASES = tuple([ClipTextCase(h, nh, it, PROJ.get(h, 768)) for h, nh, it in WIDTHS]
                        + [ClipTextCase(512, 8, 2048, 512, L, 248, tuple(sorted({e for e in LONG_E if e < L} | {L - 1}))) for L in (128, 129, 193, 248)])
EOS_RULES = (VOCAB - 1, 2)      # "the first position equal to eos_token_id" and the legacy argmax rule


@functools.lru_cache(maxsize=None)
def clip_text_weights(hidden: int, heads: int, inter: int, proj: int, max_pos: int):
    from tests import clip_text_ref as CR
    from ultrafnd_git_amd.semantic import ClipTextEncoder
    return CR.case_weights(ClipTextEncoder(vocab_size=VOCAB, hidden_size=hidden, intermediate_size=inter, projection_dim=proj, num_hidden_layers=LAYERS,
                                           num_attention_heads=heads, max_position_embeddings=max_pos).state_dict())


def clip_text_encoder(c: ClipTextCase, eos: int):
    from ultrafnd_git_amd.semantic import ClipTextEncoder
    enc = ClipTextEncoder(vocab_size=VOCAB, hidden_size=c.hidden, intermediate_size=c.inter, projection_dim=c.proj, num_hidden_layers=LAYERS,
                          num_attention_heads=c.heads, max_position_embeddings=c.max_pos, eos_token_id=eos)
    enc.load_state_dict(clip_text_weights(c.hidden, c.heads, c.inter, c.proj, c.max_pos))
    return enc


def clip_text_batch(c: ClipTextCase, k: int):
    """(ids, mask) of the case's k-th batch: EOS (VOCAB - 1, which both pooling rules find) at the pooled position, a prefix mask."""
    from tests import clip_text_ref as CR
    e = c.batches[k]
    return CR.make_ids(e, c.L, seed=c.hidden + c.L + k, vocab=VOCAB), CR.prefix_mask(e, c.L)


# ---------------------------------------------------------------------------------------------------------------------
# the form a case takes, read from the encoder
def form_of(enc, B: int, L: Optional[int] = None) -> dict:
    """What the encoder does with a (B, L) batch (text) or (B, F) frames (ViT; L is then F), read from its own dispatch:
      parts   the {sum, sumsq} partials per row of its folded LayerNorms (0: unfolded -- one LayerNorm kernel per LayerNorm)
      form    the mirror's name for it (FORMS): "unfolded", or "folded-" + the residual dtype
      fused   Q/K/V projection + attention as one launch
      tail    which buffers the last layer's class-row tail runs over: "folded" | "unfolded" | None (no tail)
      ni      the row kernels' NI = hidden / 256"""
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    b = enc._workbufs(B, L)
    vit = isinstance(enc, ClipVisualEncoder)
    folded = ("st0" in b) if vit else ("st" in b)
    parts = int(b["st"].shape[2]) if folded else 0
    tail = None
    if getattr(enc, "cls_tail", False):
        if vit:
            r = enc._cls_rows(b, B * L)
            tail = "folded" if "st1" in r else "unfolded"
            assert (tail == "unfolded") == (r["hb"] is b.get("hc")), "the unfolded tail runs over the compact hc buffer"
        else:
            tail = "folded" if "st1" in b["cls"] else "unfolded"
    fused = enc._fuses() if vit else enc._fuses(L)
    return {"parts": parts, "form": "folded-" + enc.residual_dtype if folded else "unfolded", "fused": bool(fused), "tail": tail,
            "ni": enc.hidden // 256}


# ---------------------------------------------------------------------------------------------------------------------
# the float64 yardstick and the bf16-operand mirror of a case, computed once and shared (never modified by a test)
@functools.lru_cache(maxsize=None)
def text_ref_mirror(c: TextCase, form: str, bf16: bool = True):
    """(float64 yardstick, mirror in `form`) on the case's batch.  RoBERTa: the installed RobertaForSequenceClassification in float64;
    BERT: oracle/encoders_ref in float64 (embeddings, hidden states, features)."""
    from oracle import encoders_ref as E
    from tests import affective_ref as AR
    ids, mask = text_batch(c)
    sd = text_weights(c.kind, c.hidden, c.heads, c.inter)
    if c.kind == "roberta":
        ref = AR.reference(AR.hf_model(sd, LAYERS, vocab=VOCAB, labels=c.labels, hidden=c.hidden, heads=c.heads, inter=c.inter), ids, mask)
        return ref, AR.mirror(sd, ids, mask, LAYERS, bf16=bf16, form=form, heads=c.heads)
    w = {k: v.double() for k, v in sd.items()}
    col: dict = {}
    with torch.no_grad():
        last = E.bert_last_hidden_state(w, ids, mask, heads=c.heads, collect=col)
        ref = {"embed": col[0], "layers": [col[k] for k in range(1, LAYERS + 1)], "feature": E.masked_meanpool_l2(last, mask)}
        assert torch.equal(ref["feature"], E.text_features(w, ids, mask, heads=c.heads))
    return ref, AR.bert_mirror(sd, ids, mask, LAYERS, bf16=bf16, form=form, heads=c.heads)


@functools.lru_cache(maxsize=None)
def vit_ref_mirror(c: VitCase, B: int, Fr: int, form: str, bf16: bool = True):
    from tests import vit_ref as VR
    sd, frames = vit_weights(c.hidden, c.heads, c.inter, c.patch, c.image, c.proj), vit_frames(c, B, Fr)
    return VR.reference(sd, frames, c.heads), VR.mirror(sd, frames, LAYERS, c.heads, bf16=bf16, form=form)


@functools.lru_cache(maxsize=None)
def clip_text_ref_mirror(c: ClipTextCase, eos: int, k: int, bf16: bool = True):
    from tests import clip_text_ref as CR
    sd = clip_text_weights(c.hidden, c.heads, c.inter, c.proj, c.max_pos)
    ids, mask = clip_text_batch(c, k)
    model = CR.hf_model(sd, LAYERS, eos, vocab=VOCAB, hidden=c.hidden, heads=c.heads, inter=c.inter, proj=c.proj, max_pos=c.max_pos, attn="sdpa")
    return CR.reference(model, ids, mask), CR.mirror(sd, ids, mask, LAYERS, eos, bf16=bf16, heads=c.heads)


def fields_batch(hidden: int):
    """encode_fields' input at a width: (ids, mask, part_valid) of 3 records of up to 4 parts of 40 tokens -- prefix masks of 1 to 40
    tokens, three, two and no existing parts."""
    g = torch.Generator().manual_seed(hidden)
    ids = torch.randint(0, VOCAB, (3, 4, 40), generator=g)
    lens = torch.tensor([[40, 7, 16, 1], [17, 39, 1, 1], [5, 5, 5, 5]])
    mask = (torch.arange(40)[None, None, :] < lens[:, :, None]).long()
    return ids, mask, torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0]])


@functools.lru_cache(maxsize=None)
def fields_ref_mirror(hidden: int, form: str, bf16: bool = True):
    """(float64 yardstick, mirror in `form`) of encode_fields on fields_batch(hidden), both (3, H): the per-record mean of the existing
    parts' features, L2-normalised (oracle/encoders_ref.field_mean_l2); a record without parts is a zero row."""
    from oracle import encoders_ref as E
    from tests import affective_ref as AR
    c = next(x for x in BERT_CASES if x.hidden == hidden)
    sd = text_weights(c.kind, c.hidden, c.heads, c.inter)
    ids, mask, valid = fields_batch(hidden)
    N, Mx, Lq = ids.shape
    rows = valid.reshape(-1).bool()
    fi, fm = ids.reshape(-1, Lq)[rows], mask.reshape(-1, Lq)[rows]
    with torch.no_grad():
        parts_ref = E.text_features({k: v.double() for k, v in sd.items()}, fi, fm, heads=c.heads)
    parts_mir = AR.bert_mirror(sd, fi, fm, LAYERS, bf16=bf16, form=form, heads=c.heads)["feature"]

    def records(parts):
        full = torch.zeros(N * Mx, hidden, dtype=torch.float64)
        full[rows] = parts
        out = torch.zeros(N, hidden, dtype=torch.float64)
        for n in range(N):
            if valid[n].any():
                out[n] = E.field_mean_l2(full.view(N, Mx, hidden)[n][valid[n].bool()])
        return out
    return records(parts_ref), records(parts_mir)


def stages(ref: dict, mir: dict, rows=None):
    """[(stage name, mirror's value, yardstick's value)] over the bf16 stages both dicts hold ("embed" excluded where it is fp32-only:
    the caller names it); rows: a boolean (B, L) selection of the hidden states' rows."""
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    out = [(f"layer{k + 1}", sel(mir["layers"][k]), sel(ref["layers"][k])) for k in range(len(ref["layers"]))]
    return out + [(n, mir[n], ref[n]) for n in ("pooled", "image_embeds", "text_embeds", "logits", "class_probs", "feature") if n in ref]
