"""Cases, float64 references, derived error bounds, a float32 restatement and mutants of the attention backward
(csrc/attention_bwd.hip: attn_delta_kernel, attention_bwd_kernel<PASS, DROP>) and of the training forwards that feed it
(ufnd_attention_bf16_lse[_dropout]: ctx and lse).  Shared by tests/test_attention_bwd_cases.py (CPU: the coverage list, every
restatement inside its bound, every mutant outside) and tests/test_gpu_attention_bwd.py (GPU: every case through the C ABI).

The definition (header of attention_bwd.hip), per (sample, head), head_dim 64, m = the dropout multipliers (1 without dropout):
    S = Q K^T / 8 (+ key mask),  P = softmax(S),  O = (m o P) V,  lse = log2 sum_j 2^(S_ij log2 e)
    delta_i = sum_d dO_id O_id,  dP = m o (dO V^T),  dS = P o (dP - delta) / 8,  dQ = dS K,  dK = dS^T Q,  dV = (m o P)^T dO
A sample without a live key: every score IS the mask constant, so P = 1 / L over all L keys (HF's finfo.min arithmetic, DESIGN.md
sections 2 and 4) and lse is the constant the forward documents, -3e38 (its ulp is 2e31: adding log2 L changes nothing).

Comparison (`judge`): an output g of a case with reference r and error bound e (both float64, e >= 0: the error BEFORE the final
rounding to bf16) must lie in [RNE(r - e), RNE(r + e)], RNE = round to nearest even to bf16.  e = 0 is bit equality with RNE(r).
lse is fp32: the same with the rounding to fp32.  The figure reported beside the verdict is the share of e that was needed: the
distance from r to the nearest real that rounds to g, over e.

EXACT families (e = 0 everywhere).  Operands are small integers or multiples of 1/4, so every fp32 partial sum is exact in any
order and the only roundings are the kernel's own to bf16, which the reference repeats where they are not the identity:
  census_q0  Q = 0, K_j = e_(j mod 64): S = 0, P = 1 / n over the n live keys, n a power of two.  V_j = v_j in EVERY channel (so
             dP_ij = a_i v_j for every query, not only those of one channel), v_j in 1 .. 242 mostly distinct with an integer mean
             vbar over the live keys; dO_i = a_i e_(i mod 64), a_i in +-{1, 2, 4}.  Then O = vbar, delta_i = a_i vbar,
               dV_j[d] = (1 / n) sum_(i = d mod 64) a_i                 (counts the queries of every key; all keys alike)
               dQ_i[d] = (a_i / 8 n) sum_(j = d mod 64, live) (v_j - vbar)    (weighs every key distinctly)
               dK = 0;  dS = a_i (v_j - vbar) / 8 n has |v_j - vbar| < 256 and a power-of-two a_i: exact in bf16.
  census_k0  K = 0, Q_i = e_(i mod 64): dK_j[d] = ((v_j - vbar) / 8 n) sum_(i = d mod 64) a_i, dQ = 0.
  either with dropout p = 0.5 (multiplier 2, exact): O_i = (2 / n) sum_(kept j) v_j is rounded to bf16 by the forward and
             dS_ij = (2 m_ij a_i v_j - a_i bf16(O_i)) / 8 n by the backward; both are roundings of values that are EXACT in fp32
             (integers below 2^11 against multiples of 2^-9), so they are known: the reference applies them (`kernel_roundings`),
             and dQ / dK are exact sums of those bf16 numbers, dV_j[d] = (2 / n) sum_(i = d mod 64, (i, j) kept) a_i.
             One wrong keep bit at one (q, k) changes a sum.
  select     k_j in {-4, 4}^64, q_i = 4 k_pi(i): the selected score is 512 nats = 738.7 in base 2, every other live score is at
             least SELECT_MARGIN_LOG2 = 150 below it in base 2 (checked on the CPU for every case) -- exp2 of anything under
             -149 is exactly 0 in fp32, so P is the 0/1 matrix of pi.  (The forward's l may be 1 + 2e-5 -- its fused
             multiply-add sees the rounding of score x log2 e -- so P_(i pi(i)) is within 1e-4 of 1: it rounds to bf16 1, and
             ctx to V_pi(i).)  dO and V are multiples of 1/4 below 4: delta_i = dO_i . V_pi(i) = dP_(i pi(i)) in any order, so
             dS = 0, dQ = dK = 0 and dV_j = sum_(pi(i) = j) dO_i to the bit.
The float32 restatement of an exact case must reproduce the reference bit for bit (it sums in NumPy's order, not the kernel's): that
is the CPU evidence for "exact in any order".

ROUNDED family: normal bf16 operands; the scores' standard deviation is about 0.5 ("flat") or 4 ("peaked").  Census cases whose
live count is not a power of two (P = exp2(-log2f(n)) is off by hardware ulps) and the fully masked sample at L = 50 are judged
by the same bound.  The bound is derived from the kernel's rounding points (`reference`, beside the code); no term comes from a
kernel's output.  u = 2^-24 one fp32 operation, BF = 2^-8 one rounding to bf16 (tests/frozen_ops_cases.py: half a bf16 ulp
reaches 2^-8 of the value -- 1 + 2^-8 is an exact tie --, so the 2^-9 of an average rounding would fail a correctly rounded
two-term sum), HW = 2^-23 v_exp_f32 / v_log_f32 (1 ulp, CDNA ISA reference).
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from tests import dropout_mirror as DM
from tests.frozen_ops_cases import BF, HW_ULP, MUTANT_FACTOR, U, bf16_bits, bf16_f32, bf16_round  # noqa: F401

NEG_MASK = np.float32(-3.0e38)          # the mask constant of attention.hip / attention_bwd.hip; the lse of a fully masked row
DEAD_LSE = -1.0e30                      # the forward's own test of such a row: m_run > -1.0e30f
LOG2E = 1.44269504088896340736
SELECT_MARGIN_LOG2 = 150.0              # base-2 units after the 1/8 scale: exp2(x <= -150) == 0 in fp32 (least subnormal 2^-149)
WB, OB = 64, 128                        # rows of a walked block / of an owned block
DELTA_HEADS_PER_PASS = 8                # attn_delta_kernel: 8 lanes per head, 8 heads per wave-pass
DROP_SEED, DROP_STEP, DROP_TAG = 0xA77E, 11, 257 + 3 * 4

MASK_KINDS = ("none", "ones", "prefix", "holes", "last", "first", "block64", "own128", "dead")
SELECT_KINDS = ("reversal", "stride", "many_to_one", "avoid_masked")


class Case(NamedTuple):
    family: str          # census_q0 | census_k0 | select | rounded
    B: int
    L: int
    heads: int
    mask: str            # MASK_KINDS: the kind of sample 0; the other samples rotate through the kinds ("dead": sample 1 is dead)
    p: float = 0.0       # dropout probability: 0, 0.5 (exact) or 0.1
    variant: str = ""    # select: SELECT_KINDS; rounded: flat | peaked


def case_id(c: Case) -> str:
    return "-".join(str(x) for x in c if x != "")


# ---------------------------------------------------------------------------------------------------------------------
# key masks
_ROT = ("prefix", "holes", "last", "first", "ones", "block64", "own128")


def mask_row(kind: str, L: int, pow2: bool) -> np.ndarray:
    m = np.ones(L, dtype=np.int32)
    if kind == "block64" and L <= 2 * WB:
        kind = "holes"
    if kind == "own128" and L <= OB:
        kind = "prefix"
    if kind == "prefix":
        m[max(1, 2 * L // 3):] = 0
    elif kind == "holes":                   # single keys and a run, never the last key
        m[1::3] = 0
        m[L // 2:L // 2 + L // 8] = 0
        m[L - 1] = 1
    elif kind == "last":
        m[:L - 1] = 0
    elif kind == "first":
        m[1:] = 0
    elif kind == "block64":                 # a fully masked walked block between live ones
        m[WB:2 * WB] = 0
    elif kind == "own128":                  # every key of one owned block: the second where there are three, else the first
        if L > 2 * OB:
            m[OB:2 * OB] = 0
        else:
            m[:OB] = 0
    elif kind == "dead":
        m[:] = 0
    if pow2 and kind != "dead":             # thin the live keys to a power of two; the first and the last live key stay
        live = np.flatnonzero(m)
        extra = live.size - (1 << (live.size.bit_length() - 1))
        if extra:
            inner = live[1:-1]
            m[inner[np.linspace(0, inner.size - 1, extra).round().astype(int)]] = 0
            assert np.flatnonzero(m).size == live.size - extra
    return m


def sample_kinds(c: Case) -> List[str]:
    if c.mask == "dead":
        return [("holes", "dead", "prefix")[b % 3] for b in range(c.B)]
    if c.mask in ("none", "ones"):
        return [c.mask] * c.B if c.mask == "none" else ["ones"] + [_ROT[b % len(_ROT)] for b in range(1, c.B)]
    i = _ROT.index(c.mask)
    return [_ROT[(i + b) % len(_ROT)] for b in range(c.B)]


def case_mask(c: Case) -> Optional[np.ndarray]:
    """(B, L) int32, or None for the null pointer.  Census cases thin the live keys to a power of two unless the kind is none / ones."""
    if c.mask == "none":
        return None
    pow2 = c.family.startswith("census")
    return np.stack([mask_row(k, c.L, pow2 and k != "ones") for k in sample_kinds(c)])


def is_exact(c: Case) -> bool:
    """Bit equality is asked of: select; a census whose every sample has a power-of-two live count (a dead one: L) and p in {0, 0.5}."""
    if c.family == "select":
        return True
    if c.family == "rounded" or c.p not in (0.0, 0.5):
        return False
    m = case_mask(c)
    n = [c.L] * c.B if m is None else [int(r.sum()) or c.L for r in m]
    return all(x & (x - 1) == 0 for x in n)


def grid_size(c: Case) -> int:
    return -(-c.L // OB) * c.heads * c.B


# ---------------------------------------------------------------------------------------------------------------------
# the case table
L_ALL = (1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 320, 513)
L_LONG = 1100
HEADS_AT_65 = (1, 3, 8, 9, 12, 17)
GRIDS = (1, 3, 7, 8, 9, 15, 18)
DROP_L = (1, 2, 5, 63, 66, 129, 255)


def _cases() -> List[Case]:
    out: List[Case] = []
    exact_fams = ("census_q0", "census_k0", "select")
    masks = ("prefix", "holes", "none", "last", "first", "ones", "block64", "own128")
    for i, L in enumerate(L_ALL):                       # every length: one exact probe, one rounded case; B and heads in {1, 2}
        fam = exact_fams[i % 3]
        mk = masks[i % len(masks)]
        if fam != "select" and mk in ("none", "ones") and L & (L - 1):
            mk = "holes"                                # the exact census needs a power-of-two live count
        B, heads = 1 + (i % 2), 1 + ((i // 2) % 2)
        out.append(Case(fam, B, L, heads, mk, 0.0, SELECT_KINDS[(i // 3) % 4] if fam == "select" else ""))
        rB, rh = (3 - B, 3 - heads) if L <= 320 else (1, 1)      # (the float64 reference of the test is L^2 x 64 per head and sample)
        out.append(Case("rounded", rB, L, rh, masks[(i + 3) % len(masks)], 0.0, ("flat", "peaked")[i % 2]))
    # the blocked kinds where a block can be masked, in every family
    out += [Case("census_q0", 1, 193, 1, "block64"), Case("census_k0", 1, 257, 2, "own128"), Case("census_k0", 1, 129, 1, "own128"),
            Case("select", 1, 320, 1, "own128", 0.0, "avoid_masked"), Case("select", 2, 129, 1, "block64", 0.0, "avoid_masked"),
            Case("select", 1, 191, 2, "none", 0.0, "stride"), Case("select", 1, 257, 1, "holes", 0.0, "many_to_one"),
            Case("select", 1, 65, 1, "ones", 0.0, "reversal"),
            Case("rounded", 1, 193, 1, "block64", 0.0, "peaked"), Case("rounded", 1, 320, 1, "own128", 0.0, "flat"),
            Case("census_q0", 1, 64, 1, "none"), Case("census_k0", 1, 256, 1, "ones"),              # exact with the null pointer / all ones
            Case("census_q0", 1, 65, 1, "none"), Case("census_k0", 2, 127, 1, "ones")]               # n no power of two: the rounded bound
    # heads at L = 65: the delta kernel's 8-heads-per-pass boundary and its h < heads guard, seen through dQ (K free) and dK (Q free)
    for i, h in enumerate(HEADS_AT_65):
        out.append(Case(("census_q0", "census_k0")[i % 2], 1, 65, h, ("holes", "prefix")[i % 2]))
    out += [Case("census_q0", 1, 65, 9, "prefix"), Case("census_q0", 1, 65, 17, "holes"),
            Case("rounded", 1, 65, 9, "holes", 0.0, "flat"), Case("rounded", 1, 65, 17, "prefix", 0.0, "peaked")]
    # grids of 7, 15 and 18 workgroups (1, 3, 8, 9 are above), B = 3 with a different mask per sample
    out += [Case("census_k0", 1, 33, 7, "holes"), Case("census_q0", 3, 17, 5, "prefix"), Case("census_k0", 3, 129, 3, "last"),
            Case("select", 3, 65, 3, "holes", 0.0, "avoid_masked"), Case("rounded", 3, 129, 3, "first", 0.0, "flat")]
    # the fully masked sample (sample 1): bit-exact at powers of two, rounded at L = 50; with dropout too
    out += [Case("census_q0", 2, 64, 2, "dead"), Case("census_k0", 3, 256, 1, "dead"), Case("census_q0", 2, 50, 1, "dead"),
            Case("rounded", 2, 50, 2, "dead", 0.0, "flat"), Case("rounded", 2, 128, 1, "dead", 0.0, "peaked"),
            Case("census_k0", 2, 128, 1, "dead", 0.5), Case("rounded", 2, 50, 1, "dead", 0.1, "flat")]
    # dropout: p = 0.5 exact (L % 4 in 0 .. 3), p = 0.1 rounded
    for i, L in enumerate(DROP_L + (64,)):
        out.append(Case(("census_q0", "census_k0")[i % 2], 1 + (i % 2), L, 2 - (i % 2), ("holes", "prefix")[i % 2] if L & (L - 1) else "none", 0.5))
    for i, L in enumerate(DROP_L):
        out.append(Case("rounded", 2 - (i % 2), L, 1 + (i % 2), ("none", "holes", "prefix")[i % 3], 0.1, ("peaked", "flat")[i % 2]))
    # nob = 9
    out += [Case("census_q0", 1, L_LONG, 1, "holes"), Case("rounded", 1, L_LONG, 1, "prefix", 0.0, "flat")]
    assert len(set(out)) == len(out)
    return out


CASES: List[Case] = _cases()


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def _seed(*ints) -> np.random.Generator:
    return np.random.default_rng([20] + list(ints))


def _pack(q, k, v) -> np.ndarray:
    """(B, heads, L, 64) x 3 -> (B L, 3 H) bf16 bits (the fused q | k | v rows)"""
    B, heads, L, _ = q.shape
    return bf16_bits(np.stack([q, k, v], 0).transpose(1, 3, 0, 2, 4).reshape(B * L, 3 * heads * 64))


def _merge(x) -> np.ndarray:
    """(B, heads, L, 64) -> (B L, H)"""
    B, heads, L, _ = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B * L, heads * 64)


def _split_rows(bits, B, L, heads, parts):
    x = bf16_f32(bits).astype(np.float64).reshape(B, L, parts, heads, 64)
    return tuple(x[:, :, i].transpose(0, 2, 1, 3) for i in range(parts))


def live_keys(c: Case, mask) -> np.ndarray:
    return np.ones((c.B, c.L), dtype=bool) if mask is None else mask != 0


def census_values(c: Case, mask) -> np.ndarray:
    """v_j (B, L): 1 .. 241 by a stride of 37 modulo 241 (distinct over any 241 consecutive keys), then + 1 on the first r live keys so
    that the live keys' sum is a multiple of their count (a dead sample: of L)."""
    base = (np.arange(c.L) * 37) % 241 + 1
    v = np.tile(base, (c.B, 1)).astype(np.int64)
    live = live_keys(c, mask)
    for b in range(c.B):
        idx = np.flatnonzero(live[b]) if live[b].any() else np.arange(c.L)
        n = idx.size
        if n & (n - 1) == 0:
            v[b, idx[:(-int(v[b, idx].sum())) % n]] += 1
            assert v[b, idx].sum() % n == 0
    return v


def census_signs(c: Case) -> np.ndarray:
    """a_i (B, heads, L) in +-{1, 2, 4}: differs between neighbours, between the 64-row blocks and between heads"""
    i = np.arange(c.L)[None, None, :]
    h = np.arange(c.heads)[None, :, None]
    b = np.arange(c.B)[:, None, None]
    t = (5 * i + i // 64 + 3 * h + b) % 6
    return np.array([1.0, -2.0, 4.0, -1.0, 2.0, -4.0])[t]


def permutation(c: Case, mask) -> np.ndarray:
    """pi (B, heads, L) of a selection case"""
    L = c.L
    i = np.arange(L)
    live = live_keys(c, mask)
    pi = np.zeros((c.B, c.heads, L), dtype=np.int64)
    for b in range(c.B):
        idx = np.flatnonzero(live[b]) if live[b].any() else i
        for h in range(c.heads):
            if c.variant == "reversal":
                t = (idx.size - 1 - i) % idx.size
            elif c.variant == "stride":             # 67 crosses the 64- and the 128-row blocks at every step (gcd with n removed)
                s = 67 + h
                while math.gcd(s, idx.size) != 1:
                    s += 1
                t = (i * s + b) % idx.size
            elif c.variant == "many_to_one":        # 5 queries per key, the keys a stride apart
                t = ((i // 5) * 29 + h) % idx.size
            else:                                   # avoid_masked: a stride over the live keys only
                t = (i * 3 + h + b) % idx.size
            pi[b, h] = idx[t]
    return pi


def make(c: Case) -> Dict:
    """qkv (B L, 3 H) and dctx (B L, H) as bf16 bits, mask (B, L) int32 or None, dm (B, heads, L, L) float32 multipliers or None"""
    B, L, heads = c.B, c.L, c.heads
    mask = case_mask(c)
    rng = _seed(CASES.index(c) if c in CASES else 0, B, L, heads)
    shape = (B, heads, L, 64)
    onehot = (np.arange(L)[:, None] % 64 == np.arange(64)[None, :]).astype(np.float64)
    out: Dict = dict(mask=mask, dm=None)
    if c.family.startswith("census"):
        tag = np.broadcast_to(onehot, shape)
        zero = np.zeros(shape)
        v = np.broadcast_to(census_values(c, mask)[:, None, :, None].astype(np.float64), shape)
        q, k = (zero, tag) if c.family == "census_q0" else (tag, zero)
        do = census_signs(c)[..., None] * onehot
    elif c.family == "select":
        k = rng.choice([-4.0, 4.0], shape)
        pi = permutation(c, mask)
        q = 4.0 * np.take_along_axis(k, pi[..., None], axis=2)
        v = rng.integers(-15, 16, shape) / 4.0
        do = rng.integers(-15, 16, shape) / 4.0
        out["pi"] = pi
    else:
        # |q . k| / 8 has the standard deviation sq sk: 0.5 (flat) or 4 (peaked)
        sq, sk = (0.7, 0.7) if c.variant == "flat" else (2.0, 2.0)
        q, k = rng.normal(0, sq, shape), rng.normal(0, sk, shape)
        v, do = rng.normal(0, 1.0, shape), rng.normal(0, 1.0, shape)
    out["qkv"] = _pack(q, k, v)
    out["dctx"] = bf16_bits(_merge(np.asarray(do, dtype=np.float64)))
    if c.p > 0:
        lp = (L + 3) // 4 * 4
        out["dm"] = DM.multipliers(DROP_SEED + L, DROP_STEP, DROP_TAG, c.p, B * heads * L, L, lp).reshape(B, heads, L, L)
    return out


def select_margin_log2(c: Case, inp) -> float:
    """The least (selected score - any other LIVE score of the row) in base-2 units after the 1/8 scale, over the live samples."""
    q, k, _ = _split_rows(inp["qkv"], c.B, c.L, c.heads, 3)
    s = np.einsum("bhid,bhjd->bhij", q, k) * 0.125 * LOG2E
    live = live_keys(c, inp["mask"])
    sel = np.take_along_axis(s, inp["pi"][..., None], axis=3)
    other = np.where(live[:, None, None, :], s, -np.inf)
    np.put_along_axis(other, inp["pi"][..., None], -np.inf, axis=3)
    gap = sel[..., 0] - other.max(-1)
    gap = gap[live.any(-1)]
    return float(gap.min()) if gap.size and c.L > 1 else math.inf


# ---------------------------------------------------------------------------------------------------------------------
# float64 -> bf16, round to nearest even WITHOUT a double rounding through fp32
def rne_bf16(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
    d = x - f.astype(np.float64)
    tie = ((f.view(np.uint32) & 0xFFFF) == 0x8000) & (d != 0) & np.isfinite(f)
    f = np.where(tie, np.nextafter(f, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)), f)
    return bf16_round(f).astype(np.float64)


def _cell(got, fp32: bool):
    """[lo, hi]: the reals that round (to nearest) to the stored value `got` -- halfway to its two neighbours in the output format"""
    if fp32:
        g = np.asarray(got, dtype=np.float32)
        dn, up = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        g, dn, up = (t.astype(np.float64) for t in (g, dn, up))
        return (g + dn) / 2, (g + up) / 2
    bits = bf16_bits(np.asarray(got, dtype=np.float32)).astype(np.int64)
    mag, neg = bits & 0x7FFF, (bits >> 15) != 0
    a = bf16_f32(mag.astype(np.uint16)).astype(np.float64)
    away = bf16_f32(np.minimum(mag + 1, 0x7F80).astype(np.uint16)).astype(np.float64)
    toward = np.where(mag > 0, bf16_f32(np.maximum(mag - 1, 0).astype(np.uint16)).astype(np.float64), -away)
    lo, hi = (a + toward) / 2, (a + away) / 2
    return np.where(neg, -hi, lo), np.where(neg, -lo, hi)


def judge(got, ref, e, fp32: bool = False) -> Tuple[float, int]:
    """(worst share of the bound that was needed, number of elements outside).  bf16 outputs: the allowed set is
    [RNE(ref - e), RNE(ref + e)]; fp32 outputs (lse): the same with the rounding to fp32.  The share of an element is d / e, d = the
    distance from ref to the nearest real that rounds to `got` (0 if ref itself does): the least error before the output rounding
    that explains `got`; inf where e = 0 and d > 0 (a bit differs), and for a NaN.  An element outside always has a share above 1."""
    got, ref, e = (np.asarray(a, dtype=np.float64) for a in (got, ref, e))
    assert got.shape == ref.shape == e.shape, (got.shape, ref.shape, e.shape)
    if fp32:
        lo, hi = (ref - e).astype(np.float32).astype(np.float64), (ref + e).astype(np.float32).astype(np.float64)
    else:
        lo, hi = rne_bf16(ref - e), rne_bf16(ref + e)
    bad = ~((got >= lo) & (got <= hi))          # (a NaN compares false)
    clo, chi = _cell(np.nan_to_num(got, nan=0.0), fp32)
    d = np.maximum(0.0, np.maximum(clo - ref, ref - chi))
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(d == 0, 0.0, d / e)
    share = np.where(np.isnan(got), np.inf, share)
    # `bad` decides; the clamp only absorbs the rounding noise of d / e for an element just inside (and lifts one just outside above 1)
    share = np.where(bad, np.maximum(share, np.nextafter(1.0, 2.0)), np.minimum(share, 1.0))
    return float(share.max()) if share.size else 0.0, int(bad.sum())


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference and the bound
def reference(c: Case, inp) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """{ctx (B L, H), lse (B L, heads), dqkv (B L, 3 H)}: (float64 reference, error bound before the output rounding; zeros for an
    exact case).

    Exact cases repeat the kernel's three internal roundings to bf16 (m o P, dS, and the ctx that delta reads): there they act on
    values that are exact in fp32, so they are part of the definition; without dropout they are the identity
    (tests/test_attention_bwd_cases.py checks that).

    The bound, with T_ij = sum_d |q_id k_jd|, TP_ij = sum_d |dO_id v_jd|, nblk = ceil(L / 64), x = -ln P_ij:
      df_i  = 8 u max_j T_ij + 4 u max_j |s_ij| + HW              an unnormalised forward p, relative (frozen_ops_cases.attn_ref_bound)
      el_i  = 2 df_i + (L + 2 nblk + 24) u                        l's own sum, relative
      lse   : el_i / ln 2 + HW (|log2 l| + 1) + 2 u |lse|         v_log_f32, the addition of m          (log2 units; the lse bound)
      eP_ij = 8 u T_ij + 3 u |s_ij| + u x_ij + HW + ln 2 (lse bound)      the recomputed P = exp2(s log2 e - lse), relative: the 64-term
                                                                  dot product / 8, the scaling, the subtraction, v_exp_f32, lse
      ctx   : e1 = (el_i + 2 df_i + 4 u) A + BF A, A = sum_j (m P)_ij |v_jd|     (frozen_ops_cases: P rounded to bf16 in the numerator)
      eO    = e1 + BF (|O| + e1)                                  the bf16 ctx that delta reads
      eD_i  = sum_d |dO_id| eO_id + 16 u sum_d |dO_id O_id|       delta: 8 products per lane, 3 shuffles
      eS_ij = BF (|dS_ij| + f) + f,  f = |dS_ij| (eP_ij + 3 u) + (P_ij / 8) (66 u m_ij TP_ij + eD_i + u (|dP_ij| + |delta_i|))
                                                                  dS before and after its rounding to bf16
      dQ_id : sum_j eS_ij |k_jd| + (L + 64) u sum_j (|dS_ij| + eS_ij) |k_jd|       the form-2 sum: depth <= L + 64
      dK_jd : sum_i eS_ij |q_id| + (L + 64) u sum_i (|dS_ij| + eS_ij) |q_id|
      dV_jd : sum_i (BF (Pm_ij + g) + g) |dO_id| + (L + 64) u sum_i Pm_ij |dO_id|,  g = Pm_ij (eP_ij + 2 u),  Pm = m o P
      + L 2^-120 everywhere: an operand below the least normal bf16 may be flushed by the matrix unit.
    The first term of dQ contains the issue's two: BF sum |dS K| and BF sum_d |dO O| sum_j P_ij |K_jd| / 8."""
    B, L, heads = c.B, c.L, c.heads
    q, k, v = _split_rows(inp["qkv"], B, L, heads, 3)
    (do,) = _split_rows(inp["dctx"], B, L, heads, 1)
    live = live_keys(c, inp["mask"])
    dead = ~live.any(-1)
    dm = np.ones((B, heads, L, L)) if inp["dm"] is None else inp["dm"].astype(np.float64)
    exact = is_exact(c)
    r16 = rne_bf16 if exact else (lambda x: x)

    s = np.einsum("bhid,bhjd->bhij", q, k) * 0.125
    s = np.where(dead[:, None, None, None], 0.0, s)
    lv = (live | dead[:, None])[:, None, None, :]
    sm = np.where(lv, s, -np.inf)
    mx = sm.max(-1, keepdims=True)
    pe = np.exp(sm - mx)
    l = pe.sum(-1, keepdims=True)
    P = pe / l
    with np.errstate(invalid="ignore"):
        x = np.where(lv, mx + np.log(l) - sm, 0.0)                   # -ln P, finite where P underflows
    lse = ((mx + np.log(l)) * LOG2E)[..., 0]                         # (B, heads, L)
    lse = np.where(dead[:, None, None], float(NEG_MASK), lse)
    Pm = r16(P * dm)
    O = np.einsum("bhij,bhjd->bhid", Pm, v)
    delta = (do * r16(O)).sum(-1, keepdims=True)
    dP = np.einsum("bhid,bhjd->bhij", do, v) * dm
    dS = r16(P * (dP - delta) * 0.125)
    dQ = np.einsum("bhij,bhjd->bhid", dS, k)
    dK = np.einsum("bhij,bhid->bhjd", dS, q)
    dV = np.einsum("bhij,bhid->bhjd", Pm, do)
    dqkv = np.concatenate([_merge(dQ), _merge(dK), _merge(dV)], axis=1)
    lse_rows = lse.transpose(0, 2, 1).reshape(B * L, heads)
    if exact:
        # census: lse = log2 n, an integer.  select: lse = 512 log2 e up to the roundings of log2 e, of the scale and of the product, and
        # to the forward's l in [1, 1 + 2^-15]: 6 u |lse|
        e_lse = 6 * U * np.abs(lse_rows) * (lse_rows > DEAD_LSE) if c.family == "select" else np.zeros_like(lse_rows)
        return {"ctx": (_merge(O), np.zeros((B * L, heads * 64))), "lse": (lse_rows, e_lse), "dqkv": (dqkv, np.zeros_like(dqkv))}

    aq, ak, av, ado = np.abs(q), np.abs(k), np.abs(v), np.abs(do)
    T = np.where(lv, np.einsum("bhid,bhjd->bhij", aq, ak), 0.0)
    TP = np.einsum("bhid,bhjd->bhij", ado, av)
    nblk = -(-L // WB)
    df = 8 * U * T.max(-1, keepdims=True) + 4 * U * np.where(lv, np.abs(s), 0.0).max(-1, keepdims=True) + HW_ULP
    el = 2 * df + (L + 2 * nblk + 24) * U
    e_lse = el / math.log(2) + HW_ULP * (np.abs(np.log2(l)) + 1) + 2 * U * np.abs(lse[..., None])
    e_lse = np.where(dead[:, None, None, None], 0.0, e_lse)           # the documented constant, to the bit
    eP = 8 * U * T + 3 * U * np.abs(s) + U * x + HW_ULP + math.log(2) * e_lse
    A = np.einsum("bhij,bhjd->bhid", Pm, av)
    e1 = (el + 2 * df + 4 * U) * A + BF * A
    eO = e1 + BF * (np.abs(O) + e1)
    eD = (ado * eO).sum(-1, keepdims=True) + 16 * U * (ado * np.abs(O)).sum(-1, keepdims=True)
    f = np.abs(dS) * (eP + 3 * U) + (P / 8) * (66 * U * dm * TP + eD + U * (np.abs(dP) + np.abs(delta)))
    eS = BF * (np.abs(dS) + f) + f
    depth = (L + 64) * U
    floor = L * 2.0 ** -120
    eQ = np.einsum("bhij,bhjd->bhid", eS + depth * (np.abs(dS) + eS), ak) + floor
    eK = np.einsum("bhij,bhid->bhjd", eS + depth * (np.abs(dS) + eS), aq) + floor
    g = Pm * (eP + 2 * U)
    eV = np.einsum("bhij,bhid->bhjd", BF * (Pm + g) + g + depth * Pm, ado) + floor
    e_dqkv = np.concatenate([_merge(eQ), _merge(eK), _merge(eV)], axis=1)
    return {"ctx": (_merge(O), _merge(e1) + floor), "lse": (lse_rows, e_lse[..., 0].transpose(0, 2, 1).reshape(B * L, heads)),
            "dqkv": (dqkv, e_dqkv)}


# ---------------------------------------------------------------------------------------------------------------------
# the float32 restatement (the kernel's rounding points, NumPy's summation order, no blocks) and its mutants
MUTANTS = ("walked_tail_block_dropped", "walked_block_visited_twice", "clamped_rows_not_silenced", "key_mask_shifted_by_one",
           "mask_of_sample_0_for_every_sample", "delta_of_head_h_plus_1", "delta_skipped_for_heads_ge_8", "form2_half_tiles_exchanged",
           "owned_tiles_swapped", "scale_missing", "pass2_nibble_indexed_by_key", "lp4_is_L_shr_2", "fully_masked_row_p_is_one")
DROPOUT_MUTANTS = ("pass2_nibble_indexed_by_key", "lp4_is_L_shr_2")
# mutants of the walk over the other side's 64-row blocks: at L <= 64 "a block" is everything, so they must ALSO be seen where the walk
# has several blocks and the mutant loses, doubles or leaks a few rows among hundreds
WALK_MUTANTS = ("walked_tail_block_dropped", "walked_block_visited_twice", "clamped_rows_not_silenced")


def mutant_applies(mutant: str, c: Case) -> bool:
    """False where the mutant cannot change the case's result (saves the CPU test the run)."""
    if mutant in DROPOUT_MUTANTS:
        return c.p > 0
    if mutant in ("key_mask_shifted_by_one", "mask_of_sample_0_for_every_sample"):
        return c.mask != "none" and (mutant == "key_mask_shifted_by_one" or c.B > 1)
    if mutant == "delta_of_head_h_plus_1":
        return c.heads > 1
    if mutant == "delta_skipped_for_heads_ge_8":
        return c.heads > DELTA_HEADS_PER_PASS
    if mutant == "fully_masked_row_p_is_one":
        return c.mask == "dead"
    if mutant == "clamped_rows_not_silenced":
        return c.L % WB != 0
    return True


def _f(a):
    return np.asarray(a, dtype=np.float32)


def restate(c: Case, inp, mutant: Optional[str] = None) -> Dict[str, np.ndarray]:
    """{ctx, lse, dqkv} in fp32 arithmetic with the kernel's roundings: bf16(m o p) in the forward's numerator and in dV, bf16(dS),
    the bf16 ctx in delta, bf16 outputs.  A mutant changes the BACKWARD only (ctx and lse stay right)."""
    B, L, heads = c.B, c.L, c.heads
    q, k, v = (_f(t) for t in _split_rows(inp["qkv"], B, L, heads, 3))
    do = _f(_split_rows(inp["dctx"], B, L, heads, 1)[0])
    live = live_keys(c, inp["mask"])
    one = np.float32(1)
    dm = np.ones((B, heads, L, L), dtype=np.float32) if inp["dm"] is None else inp["dm"]
    c2 = np.float32(0.125) * np.float32(LOG2E)

    def scores(lv):
        s2 = np.einsum("bhid,bhjd->bhij", q, k).astype(np.float32) * c2
        return np.where(lv[:, None, None, :], s2, NEG_MASK).astype(np.float32)

    # forward (ufnd_attention_bf16_lse[_dropout])
    sc = scores(live)
    m = sc.max(-1, keepdims=True)
    p = np.exp2(sc - m, dtype=np.float32)
    l = p.sum(-1, keepdims=True, dtype=np.float32)
    lse = (m + np.log2(l, dtype=np.float32)).astype(np.float32)
    o = np.einsum("bhij,bhjd->bhid", bf16_round(p * dm), v).astype(np.float32) * (one / l)
    ctx = bf16_round(o)

    # backward
    lb = live
    if mutant == "key_mask_shifted_by_one":
        lb = np.roll(live, 1, axis=-1)
    elif mutant == "mask_of_sample_0_for_every_sample":
        lb = np.broadcast_to(live[:1], live.shape)
    scb = sc if lb is live else scores(lb)
    with np.errstate(over="ignore", invalid="ignore"):
        P = np.exp2(scb - lse, dtype=np.float32)
    if mutant != "fully_masked_row_p_is_one":
        P = np.where(lse > np.float32(DEAD_LSE), P, one / np.float32(L)).astype(np.float32)
    delta = (do * ctx).sum(-1, keepdims=True, dtype=np.float32)
    if mutant == "delta_of_head_h_plus_1":
        delta = np.roll(delta, -1, axis=1)
    elif mutant == "delta_skipped_for_heads_ge_8":
        delta = delta.copy()
        delta[:, DELTA_HEADS_PER_PASS:] = 0
    dm1 = dm2 = dm
    if mutant == "lp4_is_L_shr_2" and c.p > 0:
        dm1 = dm2 = DM.multipliers(DROP_SEED + L, DROP_STEP, DROP_TAG, c.p, B * heads * L, L, 4 * (L >> 2)).reshape(B, heads, L, L)
    elif mutant == "pass2_nibble_indexed_by_key" and c.p > 0:      # keep(4 (q >> 2) + (k & 3), 4 (k >> 2) + (q & 3)); out of range: dropped
        qi, ki = np.arange(L)[:, None], np.arange(L)[None, :]
        q2, k2 = 4 * (qi >> 2) + (ki & 3), 4 * (ki >> 2) + (qi & 3)
        ok = (q2 < L) & (k2 < L)
        dm2 = np.where(ok, dm[:, :, np.minimum(q2, L - 1), np.minimum(k2, L - 1)], np.float32(0))
    scale = one if mutant == "scale_missing" else np.float32(0.125)
    dP = np.einsum("bhid,bhjd->bhij", do, v).astype(np.float32)
    dS1 = bf16_round(P * (dP * dm1 - delta) * scale)               # pass 1 (dQ)
    dS2 = dS1 if dm2 is dm1 else bf16_round(P * (dP * dm2 - delta) * scale)      # pass 2 (dK)
    Pm2 = bf16_round(P * dm2)                                      # pass 2 (dV)

    w = np.ones(L, dtype=np.float32)                               # how often the walk visits a row of the other side
    nwb = -(-L // WB)
    if mutant == "walked_tail_block_dropped":
        w[WB * (nwb - 1):] = 0
    elif mutant == "walked_block_visited_twice":
        w[WB * (nwb // 2):WB * (nwb // 2 + 1)] = 2
    elif mutant == "clamped_rows_not_silenced":
        w[L - 1] += WB * nwb - L                                   # the clamped copies of row L - 1, taken as that row
    z = np.arange(L)                                               # the form-2 image row that meets walked row x
    if mutant == "form2_half_tiles_exchanged":
        z = np.minimum(z ^ 16, L - 1)
    dQ = np.einsum("bhij,bhjd->bhid", dS1 * w[None, None, None, :], k[:, :, z]).astype(np.float32)
    dK = np.einsum("bhij,bhid->bhjd", dS2 * w[None, None, :, None], q[:, :, z]).astype(np.float32)
    dV = np.einsum("bhij,bhid->bhjd", Pm2 * w[None, None, :, None], do[:, :, z]).astype(np.float32)
    if mutant == "owned_tiles_swapped":
        src = np.arange(L) ^ 16
        sw = lambda t: np.where((src < L)[None, None, :, None], t[:, :, np.minimum(src, L - 1)], np.float32(0))
        dQ, dK, dV = sw(dQ), sw(dK), sw(dV)
    dqkv = bf16_round(np.concatenate([_merge(dQ), _merge(dK), _merge(dV)], axis=1))
    return {"ctx": _merge(ctx), "lse": lse[..., 0].transpose(0, 2, 1).reshape(B * L, heads), "dqkv": dqkv}


def check(c: Case, got: Dict[str, np.ndarray], refs) -> Dict[str, Tuple[float, int]]:
    """{output: (worst error / allowance, elements outside)}"""
    assert set(got) == set(refs) == {"ctx", "lse", "dqkv"}
    return {key: judge(got[key], refs[key][0], refs[key][1], fp32=(key == "lse")) for key in ("ctx", "lse", "dqkv")}


def caught(c: Case, res: Dict[str, Tuple[float, int]]) -> bool:
    """A mutant is caught by a case if a bit-equality breaks (exact case) or the bound is left by MUTANT_FACTOR."""
    r, n = res["dqkv"]
    return (is_exact(c) and n > 0) or r >= MUTANT_FACTOR
