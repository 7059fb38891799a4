"""TEST INFRASTRUCTURE for ultrafnd_git_amd/semantic.py (CPU, float64).

  reference(model, ids, mask)   the yardstick: the installed transformers.CLIPTextModelWithProjection in float64, built from a config
                                with the encoder's own (seeded) weights -- never from_pretrained, nothing touches the network.
  mirror(sd, ids, mask, ...)    the same arithmetic written out in float64 torch, with operands rounded to bf16 exactly where the
                                product rounds them (bf16=True): the GEMM weights, every GEMM A operand (the two LayerNorm outputs,
                                ctx, the quick-GELU output, the pooled final_layer_norm row), q / k / v, the attention probabilities
                                before P V.  The residual stream, the LayerNorm / softmax statistics, the embedding sum and the L2
                                normalisation stay unrounded.  With bf16=False it is the yardstick itself (tests/test_clip_text_ref.py
                                holds it to HF).
  head_ref / similarity_ref     the reference's head (src/models/semantic_forgery.py: Linear -> exact GELU, l2n) and CLIP's cosine, float64.
  causal_attn_ref_bound         the causal attention op alone: float64 reference and the elementwise bound from the kernel's roundings.

reference / mirror return the same dict of checkpoints: "embed" (B, L, 512), "layers" [hidden_states[1], ...], "pooled" (B, 512: the
final_layer_norm of row e(b), as the projection reads it: the mirror's is rounded to bf16), "text_embeds" (B, P), "feature" (B, P).

Bounds.  Every comparison of the GPU against float64 is held to BOUND_FACTOR x the mirror's own error against float64 on that same
input, per criterion (audio_ref.criteria / bounds_from_mirror, the project's convention); the bound never comes from the code under
test.  fp32-only stages: FP32_BOUNDS and head_bounds, derived beside their constants.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from tests import frozen_ops_cases as FO
from tests.audio_ref import BF16_U, BOUND_FACTOR, EPS32, MIRROR_SANITY, bounds_from_mirror, criteria, mirror_within_sanity  # noqa: F401

HIDDEN, HEADS, INTER, PROJ, MAX_POS = 512, 8, 2048, 512, 77
# the tests' small vocabulary: ids 3 .. VOCAB - 2 are words; VOCAB - 1 is the EOS of the "first position equal to eos_token_id" rule and
# the largest id of the legacy argmax rule (eos_token_id == 2)
VOCAB = 512
EOS = VOCAB - 1
# the lengths of the attention-op test (the issue's list): one row, two, the 16-row MFMA tile and its neighbours, the 32-query wave
# tile, the 64-key block / 64-query workgroup edge from both sides, CLIP's own 77
# ... and, past the tower's own 77 (long-context towers: max_position_embeddings = 248), the second and third key-block / query-workgroup
# edges from both sides and 248 itself (four key blocks, the last ragged)
ATTN_LENGTHS = (1, 2, 16, 17, 32, 33, 63, 64, 65, 77, 127, 128, 129, 191, 192, 193, 248)
ATTN_HEADS = (4, 8, 16)      # the head counts of the widths 256, 512 and 1024
# the pooled positions of the stage tests at L = 77: row 1, the tile edges 15 | 16, the key-block / workgroup edge 63 | 64, the last row
STAGE_E = (1, 15, 16, 63, 64, 76)
STAGE_BATCHES = ((1, 15, 16, 63, 64), (76, 1, 64, 16, 63))      # ... spread over two batches of B = 5
FULL_DEPTH_E = (76, 9, 33, 64)                                    # 12 layers once, B = 4
CAUSAL_J = (1, 15, 16, 31, 32, 63, 64, 76)

# fp32-only stages: bounds from rounding, relative to the largest magnitude of the float64 result (max-abs / max|ref|).
#   embed    token row + position row: ONE fp32 addition of two fp32 values, <= 1 eps of the sum
#   cosine   three 512-term fp32 sums of products in a fixed tree (depth <= 8 per lane + 6 wave steps; bounded by the plain n-term
#            bound, 514 eps of sum |t_k i_k| <= 514 eps ||t|| ||i||), two square roots, two additions of 1e-9, a product and a
#            division (8 eps): <= (3 * 514 + 8) eps in units of the cosine's range 1; the conflict score halves it
FP32_BOUNDS = {"embed": 1 * EPS32, "cosine": (3 * 514 + 8) * EPS32}


def make_ids(e_list, L: int, seed: int = 0, eos: int = EOS, pad: Optional[int] = None, vocab: int = VOCAB) -> torch.Tensor:
    """(B, L) int64 ids: row b = words (ids 3 .. vocab - 2) up to position e_list[b] - 1, `eos` at e_list[b], then `pad` (default:
    eos itself, CLIP's own padding habit, so that "first position" matters).  With eos == vocab - 1 both HF rules pool e_list[b]."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 1, (len(e_list), L), generator=g)
    for b, e in enumerate(e_list):
        ids[b, e] = eos
        ids[b, e + 1:] = eos if pad is None else pad
    return ids


def prefix_mask(e_list, L: int) -> torch.Tensor:
    """(B, L) int64 attention mask: ones up to and including e_list[b]."""
    return (torch.arange(L)[None, :] <= torch.tensor(list(e_list))[:, None]).long()


def pooled_positions(ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """HF's rule (modeling_clip.py, CLIPTextTransformer.forward), restated."""
    if eos_token_id == 2:
        return ids.to(torch.int).argmax(dim=-1)
    return (ids.to(torch.int) == eos_token_id).int().argmax(dim=-1)


def case_weights(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The tests' weights from an encoder's seeded state_dict: a non-trivial affine everywhere (the constructor leaves gamma = 1,
    beta = 0, bias = 0)."""
    sd = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(11)
    for k, v in sd.items():
        if "layer_norm" in k and k.endswith(".weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
    return sd


def hf_model(sd: Dict[str, torch.Tensor], layers: int, eos_token_id: int = EOS, vocab: int = VOCAB, hidden: int = HIDDEN, heads: int = HEADS,
             inter: int = INTER, proj: int = PROJ, max_pos: int = MAX_POS, attn: str = "eager"):
    """attn: HF's attention implementation.  Its "eager" softmax runs in float32 whatever the model's dtype (modeling_clip.py,
    eager_attention_forward: softmax(..., dtype=torch.float32)), which leaves the float64 model about one fp32 unit roundoff per layer
    away from float64; "sdpa" keeps the model's dtype throughout (the geometry table's yardstick, tests/encoder_geometry_cases.py)."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    cfg = CLIPTextConfig(vocab_size=vocab, num_hidden_layers=layers, eos_token_id=eos_token_id, hidden_size=hidden, num_attention_heads=heads,
                         intermediate_size=inter, projection_dim=proj, max_position_embeddings=max_pos)
    cfg._attn_implementation = attn
    m = CLIPTextModelWithProjection(cfg).double().eval()
    m.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    return m


def _l2n(x: torch.Tensor) -> torch.Tensor:
    return x / (x.norm(dim=-1, keepdim=True) + 1e-9)


@torch.no_grad()
def reference(model, ids: torch.Tensor, mask: torch.Tensor) -> dict:
    out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    hs = out.hidden_states
    e = pooled_positions(ids, model.config.eos_token_id)
    pooled = out.last_hidden_state[torch.arange(ids.shape[0]), e]
    return {"embed": hs[0], "layers": list(hs[1:]), "pooled": pooled, "text_embeds": out.text_embeds, "feature": _l2n(out.text_embeds)}


def _rb(t: torch.Tensor, on: bool) -> torch.Tensor:
    return t.to(torch.bfloat16).double() if on else t


@torch.no_grad()
def mirror(sd: Dict[str, torch.Tensor], ids: torch.Tensor, mask: torch.Tensor, layers: int, eos_token_id: int = EOS, bf16: bool = True,
           heads: int = HEADS, eps: float = 1e-5) -> dict:
    w = {k: v.double() for k, v in sd.items()}
    T = "text_model."
    B, L = ids.shape
    H = w[T + "embeddings.position_embedding.weight"].shape[1]
    x = w[T + "embeddings.token_embedding.weight"][ids] + w[T + "embeddings.position_embedding.weight"][:L][None]
    embed = x.clone()
    vis = (torch.arange(L)[None, :] <= torch.arange(L)[:, None])[None] & (mask != 0)[:, None, :]      # (B, q, k)

    def lin(a, name):
        y = _rb(a, bf16) @ _rb(w[name + ".weight"], bf16).T
        return y + w[name + ".bias"] if name + ".bias" in w else y

    hs = []
    for i in range(layers):
        P = T + f"encoder.layers.{i}."
        h = F.layer_norm(x, (H,), w[P + "layer_norm1.weight"], w[P + "layer_norm1.bias"], eps)
        q, k, v = (_rb(lin(h, P + f"self_attn.{n}"), bf16).view(B, L, heads, 64).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        s = (q @ k.transpose(2, 3) * 0.125).masked_fill(~vis[:, None], float("-inf"))
        p = torch.softmax(s, dim=-1)
        ctx = _rb((_rb(p, bf16) @ v).transpose(1, 2).reshape(B, L, H), bf16)
        x = x + lin(ctx, P + "self_attn.out_proj")
        h = F.layer_norm(x, (H,), w[P + "layer_norm2.weight"], w[P + "layer_norm2.bias"], eps)
        a = lin(h, P + "mlp.fc1")
        x = x + lin(_rb(a * torch.sigmoid(1.702 * a), bf16), P + "mlp.fc2")
        hs.append(x.clone())
    e = pooled_positions(ids, eos_token_id)
    pooled = _rb(F.layer_norm(x[torch.arange(B), e], (H,), w[T + "final_layer_norm.weight"], w[T + "final_layer_norm.bias"], eps), bf16)
    te = lin(pooled, "text_projection")
    return {"embed": embed, "layers": hs, "pooled": pooled, "text_embeds": te, "feature": _l2n(te)}


# ---- the head and the similarity, float64
def head_ref(t, i, wt, bt, wi, bi) -> Dict[str, torch.Tensor]:
    t, i, wt, bt, wi, bi = (torch.as_tensor(a).double() for a in (t, i, wt, bt, wi, bi))
    tp, ip = F.gelu(t @ wt.T + bt), F.gelu(i @ wi.T + bi)
    return {"semantic_text": _l2n(tp), "semantic_image": _l2n(ip), "semantic_gap": _l2n(tp - ip)}


def head_bounds(t, i, wt, bt, wi, bi) -> Dict[str, float]:
    """max-abs bounds of the fp32 head's three outputs, from rounding.  With S_j = sum_k |w_jk x_k| + |b_j| (the scale of a 512-term fma
    chain + bias: its error is <= 514 eps S_j), GELU's slope <= 1.13 and erff good to a few ulp (<= 4 eps |y_j| on the output), the
    un-normalised vector y carries ||dy|| <= 1.13 * 514 eps ||S|| + 4 eps ||y||; x / (||x|| + 1e-9) turns a perturbation dy into at most
    2 ||dy|| / ||y|| (the direction's change plus the norm's), and the norm (a 512..D-term sum, sqrt, the division) adds <= (D + 8) eps
    relative.  The gap subtracts two such vectors: their errors add, one more eps for the subtraction.  Per output the bound is the
    largest over the batch rows."""
    t, i, wt, bt, wi, bi = (torch.as_tensor(a).double() for a in (t, i, wt, bt, wi, bi))
    D = wt.shape[0]
    St, Si = t.abs() @ wt.abs().T + bt.abs(), i.abs() @ wi.abs().T + bi.abs()
    yt, yi = F.gelu(t @ wt.T + bt), F.gelu(i @ wi.T + bi)
    dt = 1.13 * 514 * EPS32 * St.norm(dim=-1) + 4 * EPS32 * yt.norm(dim=-1)
    di = 1.13 * 514 * EPS32 * Si.norm(dim=-1) + 4 * EPS32 * yi.norm(dim=-1)
    dg = dt + di + EPS32 * (yt - yi).norm(dim=-1)
    tail = (D + 8) * EPS32
    return {"semantic_text": float((2 * dt / yt.norm(dim=-1) + tail).max()), "semantic_image": float((2 * di / yi.norm(dim=-1) + tail).max()),
            "semantic_gap": float((2 * dg / (yt - yi).norm(dim=-1) + tail).max())}


def similarity_ref(t, i):
    t, i = torch.as_tensor(t).double(), torch.as_tensor(i).double()
    cos = (t * i).sum(-1) / ((t.norm(dim=-1) + 1e-9) * (i.norm(dim=-1) + 1e-9))
    return cos, 1.0 - (cos + 1.0) / 2.0


# ---- the causal attention op alone (numpy, the conventions of tests/frozen_ops_cases.py)
def attn_inputs(B: int, L: int, heads: int, seed: int):
    """(B L, 3 H) bf16 bit patterns: q, k of unit scale (scores of a few units, a peaked softmax), v of unit scale."""
    g = np.random.default_rng([seed, B, L, heads])
    return FO.bf16_bits(g.standard_normal((B * L, 3 * heads * 64)).astype(np.float32))


def attn_prefix_mask(B: int, L: int) -> np.ndarray:
    """(B, L) int32 key mask: sample b keeps the keys 0 .. n_b - 1 with n_b spread from 1 to L (key 0 always: the precondition)."""
    n = [max(1, (L * (b + 1)) // (B + 1)) for b in range(B)]
    return (np.arange(L)[None, :] < np.asarray(n)[:, None]).astype(np.int32)


def causal_attn_ref_bound(qkv_bits, mask, B: int, L: int, heads: int):
    """float64 causal softmax attention of the bf16 operands (key k visible to query q iff k <= q and the mask keeps it; an invisible
    key has probability 0) and the elementwise bound: frozen_ops_cases.attn_ref_bound's derivation, its maxima taken over the keys a
    query sees.  With A_id = sum_j P_ij |V_jd|, T_ij = sum_d |q_id k_jd|, nblk = ceil(L / 64):
      delta_i = 8 u max_j T_ij + 4 u max_j |s_ij| + 2^-23      relative error of an unnormalised p_ij (64-term fp32 dot product, the
                                                               scaling and the subtraction of the maximum, v_exp_f32 at 1 ulp)
      e1 = (2 delta_i + (L + 2 nblk + 24) u) A + BF A          p's error in the numerator and in l, the P V sum, one rescale per key
                                                               block, l's own sum, 1 / l and the product; P rounded to bf16 in the
                                                               numerator only
      bound = e1 + BF (|ref| + e1)                             the output's rounding to bf16
    Rows (B L, H), the kernel's ctx layout."""
    x = FO.bf16_f32(qkv_bits).astype(np.float64).reshape(B, L, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    s = np.einsum("bhid,bhjd->bhij", q, k) * 0.125
    T = np.einsum("bhid,bhjd->bhij", np.abs(q), np.abs(k))
    keep = np.ones((B, L), dtype=bool) if mask is None else mask != 0
    live = (np.tril(np.ones((L, L), dtype=bool))[None] & keep[:, None, :])[:, None]      # (B, 1, q, k)
    assert live.any(-1).all(), "precondition: every query sees a key"
    sm = np.where(live, s, -np.inf)
    p = np.exp(sm - sm.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhij,bhjd->bhid", p, v)
    A = np.einsum("bhij,bhjd->bhid", p, np.abs(v))
    delta = 8 * FO.U * np.where(live, T, 0).max(-1, keepdims=True) + 4 * FO.U * np.where(live, np.abs(s), 0).max(-1, keepdims=True) + FO.HW_ULP
    nblk = -(-L // FO.KB)
    e1 = (2 * delta + (L + 2 * nblk + 24) * FO.U) * A + FO.BF * A
    bound = e1 + FO.BF * (np.abs(ref) + e1)
    merge = lambda t: t.transpose(0, 2, 1, 3).reshape(B * L, heads * 64)
    return merge(ref), merge(bound)
