"""TEST INFRASTRUCTURE for ultrafnd_git_amd/affective.py (CPU, float64).

  reference(model, ids, mask)   the yardstick: the installed transformers.RobertaForSequenceClassification in float64, built from a
                                local RobertaConfig with the encoder's own (seeded) weights -- never from_pretrained, nothing touches
                                the network.
  mirror(sd, ids, mask, ...)    the same arithmetic written out in float64 torch, with operands rounded to bf16 exactly where the
                                product rounds them (bf16=True): the GEMM weights, every GEMM A operand (the LayerNorm outputs -- in
                                the folded forms the UN-normalised row, with W * gamma rounded -- ctx, the GELU output), q / k / v, the
                                attention probabilities before P V and, with the bf16 residual stream, the residual operand.  LayerNorm /
                                softmax statistics, the embedding sum, the last layer's sums and the whole head stay unrounded.  With
                                bf16=False it is the yardstick itself (tests/test_affective_ref.py holds it to HF).
  position_ids                  HF's create_position_ids_from_input_ids (modeling_roberta.py), restated.
  head_ref / arousal_ref        the head chain (tanh head, softmax, the reference's grouping and formulas:
                                src/models/affective_forensics.py:92-101,130-148) and the RMS-energy arousal (:127-128), float64.
  head_bounds / arousal_bound   their fp32 rounding bounds, derived beside the code.

reference / mirror return the same dict of checkpoints: "embed" (B, L, H), "layers" [hidden_states[1], ...], "logits" (B, C),
"class_probs" (B, C).

Bounds.  Every comparison of the GPU against float64 that carries bf16 roundings is held to BOUND_FACTOR x the mirror's own error
against float64 on that same input, per criterion (audio_ref.criteria / bounds_from_mirror, the project's convention); the bound never
comes from the code under test.  fp32-only stages: FP32_BOUNDS, head_bounds and arousal_bound.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from tests.audio_ref import BF16_U, BOUND_FACTOR, EPS32, MIRROR_SANITY, bounds_from_mirror, criteria, mirror_within_sanity  # noqa: F401

HIDDEN, HEADS, INTER, LABELS, MAX_POS, PAD = 768, 12, 3072, 7, 514, 1
VOCAB = 300          # the tests' small vocabulary: id 0 is <s>, PAD = 1, 2 is </s>, 3 .. VOCAB - 1 are words
FORMS = {"folded-bf16": (True, "bf16"), "folded-fp32": (True, "fp32"), "unfolded": (False, "fp32")}
# the reference's substring rules (affective_forensics.py:94-97), restated: group 0 fear, 1 anger, 2 joy
RULES = (("fear", "anx", "worr", "scare"), ("anger", "annoy", "mad", "rage"), ("joy", "happi", "delight", "amuse"))
DEFAULT_LABELS = ("anger", "disgust", "fear", "joy", "neutral", "sadness", "surprise")

# fp32-only stage: the embeddings.  word + position + token_type: two fp32 additions (2 eps of the sum's scale); LayerNorm over H = 768:
# mean and variance from fixed fp32 trees (their relative errors are a few eps each thanks to the cancellation-free two-pass form: <= 8
# eps of the normalised value together with rsqrt), the subtraction, two products and the addition of beta (4 eps): <= 16 eps relative
# to the largest |embedding|; doubled for the two-pass variance's dependence on the rounded mean.
FP32_BOUNDS = {"embed": 32 * EPS32}
LAMBDA = 6.0         # head_bounds: the confidence parameter of the probabilistic rounding bound


def position_ids(ids: torch.Tensor, pad: int = PAD) -> torch.Tensor:
    """cumsum(ids != pad) * (ids != pad) + pad, over the ids (not the attention mask)."""
    keep = (ids != pad).long()
    return torch.cumsum(keep, dim=1) * keep + pad


def make_batch(lengths: Sequence[int], L: int, seed: int = 0, holes: Sequence[tuple] = (), vocab: int = VOCAB, pad: int = PAD):
    """(ids, mask), both (B, L) int64: sample b = <s>, words, </s> over its first lengths[b] positions (length 0: all pad, mask 0;
    1: <s> alone), pad after.  holes: (b, l) positions that hold the pad id while the mask stays 1 -- a pad in the middle: the
    position ids skip it, the attention keeps it."""
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    ids = torch.randint(3, vocab, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lengths):
        assert 0 <= n <= L
        ids[b, n:] = pad
        mask[b, :n] = 1
        if n >= 1:
            ids[b, 0] = 0
        if n >= 2:
            ids[b, n - 1] = 2
    for b, l in holes:
        assert 0 < l < lengths[b] - 1
        ids[b, l] = pad
    return ids, mask


def case_weights(sd: Dict[str, torch.Tensor], seed: int = 23) -> Dict[str, torch.Tensor]:
    """The tests' weights from a classifier's seeded state_dict: a non-trivial affine everywhere (the constructor leaves gamma = 1,
    beta = 0, bias = 0), and a head whose logits spread over a few units (std 0.02 weights alone would give a flat softmax)."""
    sd = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        if "LayerNorm" in k and k.endswith(".weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
    sd["classifier.dense.weight"] = sd["classifier.dense.weight"] * 2.0
    sd["classifier.out_proj.weight"] = sd["classifier.out_proj.weight"] * 8.0
    return sd


def hf_model(sd: Dict[str, torch.Tensor], layers: int, vocab: int = VOCAB, labels: int = LABELS, hidden: int = HIDDEN, heads: int = HEADS,
             inter: int = INTER, max_pos: int = MAX_POS):
    from transformers import RobertaConfig, RobertaForSequenceClassification
    cfg = RobertaConfig(vocab_size=vocab, num_hidden_layers=layers, hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter,
                        max_position_embeddings=max_pos, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=PAD, num_labels=labels,
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_act="gelu")
    cfg._attn_implementation = "eager"
    m = RobertaForSequenceClassification(cfg).double().eval()
    m.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    return m


@torch.no_grad()
def reference(model, ids: torch.Tensor, mask: torch.Tensor) -> dict:
    out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    hs = out.hidden_states
    return {"embed": hs[0], "layers": list(hs[1:]), "logits": out.logits, "class_probs": torch.softmax(out.logits, dim=-1)}


def _rb(t: torch.Tensor, on: bool) -> torch.Tensor:
    return t.to(torch.bfloat16).double() if on else t


def _post_ln_stack(w: Dict[str, torch.Tensor], prefix: str, x: torch.Tensor, mask: torch.Tensor, layers: int, bf16: bool, form: str, heads: int,
                   eps: float) -> list:
    """hidden_states[1 ..] of the post-LN layers `prefix`{i}. (BERT's and RoBERTa's names) over the embeddings x, in the given form."""
    fold, stream = FORMS[form]
    fold, sb = fold and bf16, (stream == "bf16") and bf16
    B, L, H = x.shape
    keep = (mask != 0)[:, None, None, :]

    def lin(a, name):
        return _rb(a, bf16) @ _rb(w[name + ".weight"], bf16).T + w[name + ".bias"]

    def ln(y, name):      # exact LayerNorm of the fp32 row
        return F.layer_norm(y, (H,), w[name + ".weight"], w[name + ".bias"], eps)

    def ln_of_rounded(y, name):      # the folded forms' view: the rounded row, the unrounded row's statistics
        mu, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
        return (_rb(y, True) - mu) / torch.sqrt(var + eps), w[name + ".weight"], w[name + ".bias"]

    def lin_ln(y, ln_name, name):      # Linear(LayerNorm(y))
        if not fold:
            return lin(ln(y, ln_name), name)
        n, gamma, beta = ln_of_rounded(y, ln_name)
        W = w[name + ".weight"]
        return n @ _rb(W * gamma[None, :], True).T + (w[name + ".bias"] + W @ beta)

    def residual(y, ln_name):
        if not sb:
            return ln(y, ln_name)
        n, gamma, beta = ln_of_rounded(y, ln_name)
        return n * gamma + beta

    hs = []
    y_prev, prev_ln = None, None      # the previous layer's feed-forward sums and the LayerNorm that follows them
    for i in range(layers):
        P = prefix + f"{i}."
        if y_prev is None:      # layer 0 reads the embeddings' materialised LayerNorm
            qkv = [lin(x, P + f"attention.self.{n}") for n in ("query", "key", "value")]
            res = _rb(x, sb)
        else:
            qkv = [lin_ln(y_prev, prev_ln, P + f"attention.self.{n}") for n in ("query", "key", "value")]
            res = residual(y_prev, prev_ln)
        q, k, v = (_rb(t, bf16).view(B, L, heads, 64).transpose(1, 2) for t in qkv)
        s = (q @ k.transpose(2, 3) * 0.125).masked_fill(~keep, float("-inf"))
        p = torch.softmax(s, dim=-1)
        ctx = _rb((_rb(p, bf16) @ v).transpose(1, 2).reshape(B, L, H), bf16)
        y1 = lin(ctx, P + "attention.output.dense") + res
        a = F.gelu(lin_ln(y1, P + "attention.output.LayerNorm", P + "intermediate.dense"))
        y2 = lin(_rb(a, bf16), P + "output.dense") + residual(y1, P + "attention.output.LayerNorm")
        y_prev, prev_ln = y2, P + "output.LayerNorm"
        hs.append(ln(y2, prev_ln))      # hidden_states[i + 1], as last_hidden_state(n_layers = i + 1) materialises it: from the fp32 sums
    return hs


@torch.no_grad()
def mirror(sd: Dict[str, torch.Tensor], ids: torch.Tensor, mask: torch.Tensor, layers: int, bf16: bool = True, form: str = "folded-bf16",
           heads: int = HEADS, eps: float = 1e-5, pad: int = PAD) -> dict:
    """form: which of the encoder's three forms is mirrored (FORMS).  A LayerNorm's consumer GEMM reads, unfolded, the rounded LayerNorm
    output against the rounded weight; folded, the rounded un-normalised row against the rounded W * gamma, normalised with the
    statistics of the unrounded row.  The residual operand is LayerNorm of the fp32 row, or (bf16 stream) of its rounding.  The
    geometry is the weights' own (H from the word embeddings) and `heads`."""
    w = {k: v.double() for k, v in sd.items()}
    E = "roberta.embeddings."
    H = w[E + "word_embeddings.weight"].shape[1]
    x = w[E + "word_embeddings.weight"][ids] + w[E + "position_embeddings.weight"][position_ids(ids, pad)] + w[E + "token_type_embeddings.weight"][0]
    x = F.layer_norm(x, (H,), w[E + "LayerNorm.weight"], w[E + "LayerNorm.bias"], eps)
    hs = _post_ln_stack(w, "roberta.encoder.layer.", x, mask, layers, bf16, form, heads, eps)
    feat = hs[-1][:, 0]
    t = torch.tanh(feat @ w["classifier.dense.weight"].T + w["classifier.dense.bias"])
    logits = t @ w["classifier.out_proj.weight"].T + w["classifier.out_proj.bias"]
    return {"embed": x, "layers": hs, "logits": logits, "class_probs": torch.softmax(logits, dim=-1)}


@torch.no_grad()
def bert_mirror(sd: Dict[str, torch.Tensor], ids: torch.Tensor, mask: torch.Tensor, layers: int, bf16: bool = True, form: str = "folded-bf16",
                heads: int = 12, eps: float = 1e-12) -> dict:
    """BertTextEncoder's pass: the same layers under BERT's names, with BERT's position rule (position l is row l) and the masked
    mean-pool + L2 normalisation of the reference (text_blocks.py:82-100; fp32 in the product, unrounded here).  Returns "embed",
    "layers" and "feature" (B, H).  With bf16=False it is oracle/encoders_ref.text_features in float64."""
    w = {k: v.double() for k, v in sd.items()}
    E = "embeddings."
    B, L = ids.shape
    H = w[E + "word_embeddings.weight"].shape[1]
    x = w[E + "word_embeddings.weight"][ids] + w[E + "position_embeddings.weight"][:L][None] + w[E + "token_type_embeddings.weight"][0]
    x = F.layer_norm(x, (H,), w[E + "LayerNorm.weight"], w[E + "LayerNorm.bias"], eps)
    hs = _post_ln_stack(w, "encoder.layer.", x, mask, layers, bf16, form, heads, eps)
    m = (mask != 0).double()[:, :, None]
    rep = (hs[-1] * m).sum(dim=1) / m.sum(dim=1).clamp_min(1e-6)
    return {"embed": x, "layers": hs, "feature": rep / (rep.norm(dim=-1, keepdim=True) + 1e-9)}


# ---- the head chain and the arousal, float64
def group_masks(names: Sequence[str]) -> torch.Tensor:
    """(3, C) 0/1: row g marks the labels the reference's rule g picks (a label may be in several rows)."""
    low = [str(n).lower() for n in names]
    return torch.tensor([[1.0 if any(k in n for k in keys) else 0.0 for n in low] for keys in RULES], dtype=torch.float64)


def group_table(names: Sequence[str]) -> list:
    """The int32 table the head entry takes: -1 none, 0 / 1 / 2 one group, 4 + bitmask for several."""
    gm = group_masks(names)
    out = []
    for c in range(gm.shape[1]):
        hits = [g for g in range(3) if gm[g, c] > 0]
        out.append(-1 if not hits else hits[0] if len(hits) == 1 else 4 + sum(1 << g for g in hits))
    return out


def post_ref(logits, names: Sequence[str], valid=None, arousal=None) -> Dict[str, torch.Tensor]:
    """Everything after the logits: softmax, group sums, normalisation by f + a + j + 1e-9, text_intensity, intensity, valence."""
    lg = torch.as_tensor(logits).double()
    B = lg.shape[0]
    p = torch.softmax(lg, dim=-1)
    g3 = p @ group_masks(names).T
    probs = g3 / (g3.sum(-1, keepdim=True) + 1e-9)
    if valid is not None:
        probs = probs * (torch.as_tensor(valid).double()[:, None] != 0)
    f, a, j = probs[:, 0], probs[:, 1], probs[:, 2]
    ti = torch.clamp(torch.sigmoid(2.5 * (f + a - 0.5 * j)), 0.0, 1.0)
    ar = torch.full((B,), 0.5, dtype=torch.float64) if arousal is None else torch.as_tensor(arousal).double()
    return {"class_probs": p, "probs": probs, "text_intensity": ti, "arousal": ar, "intensity": torch.clamp(0.6 * ti + 0.4 * ar, 0.0, 1.0),
            "valence": torch.clamp(0.5 + 0.5 * (j - 0.5 * (f + a)), 0.0, 1.0)}


def head_ref(x, wd, bd, wo, bo, names: Sequence[str], valid=None, arousal=None) -> Dict[str, torch.Tensor]:
    """logits = tanh(x Wd^T + bd) Wo^T + bo (RobertaClassificationHead, eval mode), then post_ref.  valid == 0: the features count as 0."""
    x, wd, bd, wo, bo = (torch.as_tensor(t).double() for t in (x, wd, bd, wo, bo))
    if valid is not None:
        x = x * (torch.as_tensor(valid).double()[:, None] != 0)
    logits = torch.tanh(x @ wd.T + bd) @ wo.T + bo
    return dict(post_ref(logits, names, valid, arousal), logits=logits)


def head_bounds(x, wd, bd, wo, bo, valid=None, logits_slack: float = 0.0, arousal_err: float = 0.0) -> Dict[str, float]:
    """max-abs bounds of the fp32 head's outputs, from rounding (eps = 2^-24), the largest over the batch rows.  Two H = 768-term
    sums in sequence: the worst-case n eps bounds, chained (every rounding of every term aligned, twice), come to 0.1 on a logit and
    check nothing.  The sums are held to the probabilistic bound instead (Higham & Mary, "A new approach to probabilistic rounding error
    analysis", SIAM J. Sci. Comput. 41(5), 2019): roundings as independent zero-mean variables give |error| <= LAMBDA sqrt(n) eps sum |terms| except with probability 2 n
    exp(-LAMBDA^2 / 2) -- 3e-5 per sum at LAMBDA = 6 -- and independent errors e_j with |e_j| <= d_j give |sum_j w_j e_j| <=
    sqrt(sum_j (w_j d_j)^2) at the same confidence.
      z_j   an H-term fma chain + bias: dz_j = LAMBDA sqrt(H + 2) eps S_j, S_j = sum_k |x_k Wd_jk| + |bd_j|
      t_j   tanh has slope <= 1 and tanhf is good to a few ulp of a value below 1: dt_j = dz_j + 4 eps
      l_c   sum_j t_j Wo_cj + bo_c in a fixed tree: dl_c = sqrt(sum_j (Wo_cj dt_j)^2) + LAMBDA sqrt(H + 2) eps (sum_j |t_j Wo_cj| +
            |bo_c|)  [+ logits_slack: a known offset of the logits the caller adds]
      p_c   softmax: a shift of the logits by at most d = max_c dl_c changes p_c by a factor within exp(+-2 d); l - max costs eps |l - max|
            on the exponent, expf 4 eps, the C-term sum C eps, the division 1 eps:  rp = 2 d + (range + C + 5) eps  relative, p <= 1
      groups  sums of <= C probabilities (C eps), f + a + j + 1e-9 (3 eps), the division (1 eps): the normalised probs carry
            rn = 2 (rp + C eps) + 4 eps  relative, probs <= 1
      text_intensity  raw = f + a - 0.5 j: 2 rn + 3 eps; sigmoid(2.5 raw) has slope 2.5 / 4; expf, the addition and the division 8 eps
      intensity  0.6 d_ti + 0.4 arousal_err + 4 eps;   valence  0.5 (rn + 0.5 * 2 rn) + 4 eps = rn + 4 eps"""
    x, wd, bd, wo, bo = (torch.as_tensor(t).double() for t in (x, wd, bd, wo, bo))
    if valid is not None:
        x = x * (torch.as_tensor(valid).double()[:, None] != 0)
    n_eps = LAMBDA * math.sqrt(wd.shape[0] + 2) * EPS32
    S = x.abs() @ wd.abs().T + bd.abs()
    t = torch.tanh(x @ wd.T + bd)
    dt = n_eps * S + 4 * EPS32
    lg = t @ wo.T + bo
    dl = torch.sqrt((dt * dt) @ (wo * wo).T) + n_eps * (t.abs() @ wo.abs().T + bo.abs()) + logits_slack
    return dict(post_bounds(lg, dl.max(-1).values, arousal_err), logits=float(dl.max()))


def post_bounds(logits, d=0.0, arousal_err: float = 0.0) -> Dict[str, float]:
    """head_bounds from the softmax on: logits (B, C) known to within d (a number or one per row)."""
    lg = torch.as_tensor(logits).double()
    C = lg.shape[1]
    rng = lg.max(-1).values - lg.min(-1).values
    rp = 2 * torch.as_tensor(d).double() + (rng + C + 5) * EPS32
    rn = 2 * (rp + C * EPS32) + 4 * EPS32
    d_ti = 0.625 * (2 * rn + 3 * EPS32) + 8 * EPS32
    return {"class_probs": float(rp.max()), "probs": float(rn.max()), "text_intensity": float(d_ti.max()),
            "intensity": float((0.6 * d_ti + 0.4 * arousal_err + 4 * EPS32).max()), "valence": float((rn + 4 * EPS32).max())}


def arousal_ref(wave) -> float:
    """clip(sigmoid(5 mean(x^2)), 0, 1); an empty clip: sigmoid(0) (the reference is never handed one: np.mean of nothing is nan)."""
    x = torch.as_tensor(wave).double().flatten()
    en = float((x * x).mean()) if x.numel() else 0.0
    return min(1.0, max(0.0, 1.0 / (1.0 + math.exp(-5.0 * en))))


def arousal_bound(wave) -> float:
    """The fp32 kernel's bound.  All terms of sum x^2 are non-negative, so the error of the sum is relative: each of the 256 threads adds
    ceil(n / 256) squares in sequence (fma: one rounding per term), then an 8-level fixed tree, the division by n:
    (ceil(n / 256) + 10) eps of the mean.  sigmoid(5 m) has slope 5 / 4: 1.25 m times that; the product, expf, the addition and the
    division: 8 eps of a value below 1."""
    x = torch.as_tensor(wave).double().flatten()
    n = x.numel()
    en = float((x * x).mean()) if n else 0.0
    return 1.25 * en * (math.ceil(n / 256) + 10) * EPS32 + 8 * EPS32
