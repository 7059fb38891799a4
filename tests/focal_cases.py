"""Cases, float64 reference, derived error bounds, float32 restatement and mutants of the raw-data trainer's criterion:
ufnd_softmax_focal (softmax_focal_kernel in csrc/tier_a.hip) -- FocalLoss(alpha, gamma), optionally under mixup_criterion.  Shared by
tests/test_focal_cases.py (CPU: the restatement stays inside the bound on every case, every mutant leaves it, the table reaches
what it names) and tests/test_gpu_focal_mixup.py (GPU: every case through the C ABI).  The conventions are those of
tests/step_tail_cases.py, whose cross-entropy section this extends: U, HW_ULP, TINY, DIV, block_sum_f32, worst_ratio are its own.

The kernel, per row (l0, l1) and label y, from ce_row's (n0, n1, p0, p1) (n_c = -log p_c = logf(S) - d_c, p_c = e_c / S,
d_c = l_c - max, e_c = __expf(d_c), S = e0 + e1):
    pt = p_y, q = p_(1-y), ce = n_y                            q is the OTHER class's probability, never 1 - pt
    w  = 1 (gamma 0) | q (gamma 1) | q q (gamma 2) | powf(q, gamma)
    dw = 0           | 1           | 2 q           | gamma powf(q, gamma - 1)
    fl = (alpha w) ce
    k  = w + (dw pt) ce                                        (1 for gamma 0)
    g_c = (alpha k) (p_c - [c == y])
without mixup    row = fl,                            G_c = g_c
with mixup       row = mix0 fl(ya) + mix1 fl(yb),     G_c = mix0 g_c(ya) + mix1 g_c(yb)         (mix = fl32(lam), fl32(1 - lam))
    loss_rows = row, d_logits = G / float(B), loss = block_sum(row) / float(B)
every operation rounded on its own (contraction is off in the kernel), in the order written.

Bounds.  u = 2^-24 per fp32 operation; a division is 5 u, logf 2 u (HIP's single-precision table), v_exp_f32 HW_ULP; a result
below 2^-126 may be flushed: TINY absolute per operation that can underflow.  From the cross-entropy section, with gap = |l0 - l1|:
    rho_e = 3 u gap + HW_ULP for the losing class (0 for the winner: exp(0) = 1), d_e = e rho_e + TINY,
    d_S = d_e0 + d_e1 + u S,  d_ls = d_S / S + 2 u |ls|,  d_n = d_ls + u |d_c| + u |n_c|,  d_p = p (rho_e + d_S / S + 5 u) + TINY.
d_n does NOT vanish with n: logf(S) is exactly 0 once the loser's exponential is below 2^-24, where the true n_winner is that
exponential -- the u S in d_S carries it.  That absolute u is what the `alpha q^gamma` term of the bound's form is made of.
powf is OCML's: POW = 4 u here -- twice the 1 ulp HIP's table lists for it, that figure being a measured maximum over sampled
arguments, not a promise.  With r_q = d_q / q (the relative error of q):
    w:   gamma 1: d_w = d_q;  gamma 2: w (2 r_q + u) + TINY;  else w (gamma r_q + POW) + TINY
    dw:  gamma 1: 0;          gamma 2: dw r_q + TINY;         else dw ((gamma - 1) r_q + POW + u) + TINY
    a = dw pt:  d_a = d_dw pt + dw d_pt + u a + TINY;     t = a ce:  d_t = d_a ce + a d_ce + u t + TINY;     k = w + t:  d_k = d_w + d_t + u k
    alpha w: d = alpha d_w + u alpha w + TINY;            fl:  d_fl = d_(alpha w) ce + alpha w d_ce + u |fl| + TINY
    alpha k: d = alpha d_k + u alpha k;   diff_c = p_c - [c == y]: d = d_p + u |diff|;   g_c: d_g = d_(alpha k) |diff| + alpha k d_diff + u |g| + TINY
    mixed:   d_row = mix0 d_fl(a) + mix1 d_fl(b) + u (|mix0 fl(a)| + |mix1 fl(b)|) + u |row| + 3 TINY, the gradient alike
    d_logits: d_G / B + 5 u |G / B| + TINY;    loss: (sum d_row + D u sum |row|) / B + 5 u |loss| + TINY,  D = ceil(B / 256) + 8.
Collected into the form  c u (|fl| + alpha q^gamma)  and  c' u (|d| + alpha gamma q^gamma):  the relative part is dominated by
gamma r_q with r_q = (3 gap + 2 + 6 + 1) u for a winning label (q is the loser's probability), so on the device
    c(gap, gamma) = gamma (3 gap + 9) + 12,        c'(gap, gamma) = c + gamma + 8
-- at gap <= 1 and gamma <= 5 that is c <= 72 where a restatement with correctly rounded exp / log stays at 8.2: the difference is
__expf's argument product (d log2(e), rounded: a relative 3 u gap in the result) and powf.  tests/test_focal_cases.py asserts that
the term-by-term bounds below stay under these closed forms on every row of the table.  No term comes from the kernel's output.

Exact rows.  At |gap| = 100 the loser's exponential is below the denormals of fp32: __expf returns 0, S = 1, q = 0 and n_winner = 0
exactly, so a row whose label(s) name the winner has loss and gradient exactly 0 for every gamma >= 1 -- also where an exponential
keeps its denormal 3.8e-44 (NumPy's does): n_winner is still 0, and q times anything of q's size underflows.  At gamma = 0 the
loser's gradient entry IS that exponential, zero or denormal: those rows are held to their TINY bound, not to 0.  `zero_rows`
(bound 0) holds |loss_row| + |d0| + |d1| of the exact rows.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from tests.frozen_ops_cases import HW_ULP, MUTANT_FACTOR, U, Op, case_id, worst_ratio  # noqa: F401
from tests.step_tail_cases import DIV, TINY, _d, _f, _f32, block_sum_f32

POW = 4 * U
FOCAL_B = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
GAPS = (0.0, 1e-3, -1e-3, 1.0, -1.0, 12.0, -12.0, 30.0, -30.0, 100.0, -100.0)      # l0 - l1: positive = class 0 wins
OFFSETS = (0.0, 1e3, -1e3)
LABELS = ("mixed", "all0", "all1")
LABELS_B = (None, "same", "reversed", "random")      # None: no mixup (labels_b = NULL)
LAMS = (1.0, 0.0, 0.5, 1e-9, "beta")
ALPHA_GAMMA = ((1.0, 2.0), (0.25, 2.0), (1.0, 1.0), (1.0, 3.5), (1.0, 5.0), (1.0, 0.0))
MUTANTS = ("q_as_one_minus_pt", "pt_ce_term_missing", "gamma_minus_one_for_gamma", "lam_and_one_minus_lam_swapped", "mean_over_2B",
           "labels_b_ignored", "alpha_missing_from_gradient")


def _seed(*ints):
    return np.random.default_rng([20261021] + [int(i) for i in ints])


def _cases():
    """B x (alpha, gamma) x labels; the offset, the labels_b set and lam rotate (19 steps per batch size: coprime to 3, 4 and 5), then
    every (alpha, gamma) meets every labels_b set and every lam at the multi-sweep batch"""
    out, i = [], 0
    for B in FOCAL_B:
        for ag in ALPHA_GAMMA:
            for labels in LABELS:
                out.append((B, ag, labels, OFFSETS[i % 3], LABELS_B[i % 4], LAMS[i % 5]))
                i += 1
        i += 1
    for j, ag in enumerate(ALPHA_GAMMA):
        for lb in LABELS_B[1:]:
            for lam in LAMS:
                out.append((257, ag, "mixed", OFFSETS[j % 3], lb, lam))
        out.append((257, ag, "mixed", OFFSETS[(j + 1) % 3], None, 1.0))
    return sorted(set(out), key=lambda c: (c[0], c[1], c[2], c[3], str(c[4]), str(c[5])))


def mix_of(lam):
    """(fl32(lam), fl32(1 - lam)): the difference in double, rounded once -- what HeadStep.stage_draw writes"""
    return np.array([lam, 1.0 - lam], dtype=np.float64).astype(np.float32)


def _make(case):
    B, ag, labels, offset, lb, lam = case
    rng = _seed(B, ALPHA_GAMMA.index(ag), LABELS.index(labels), OFFSETS.index(offset), LABELS_B.index(lb), LAMS.index(lam))
    start = int(rng.integers(0, len(GAPS)))                 # the rows walk through every gap, starting anywhere (B = 1, 2 see two of them)
    gap = np.array([GAPS[(start + r) % len(GAPS)] for r in range(B)])
    lg = _f32(np.stack([np.full(B, offset), offset - gap], 1))
    ya = {"mixed": rng.integers(0, 2, B), "all0": np.zeros(B, int), "all1": np.ones(B, int)}[labels].astype(np.int64)
    yb = None if lb is None else {"same": ya.copy(), "reversed": ya[::-1].copy(), "random": rng.integers(0, 2, B).astype(np.int64)}[lb]
    if lb == "reversed" and labels != "mixed":              # (a reversal of equal labels is the same labels: flip it, so that ya != yb somewhere)
        yb = 1 - ya
    lam_v = float(rng.beta(0.2, 0.2)) if lam == "beta" else float(lam)
    return dict(logits=lg, labels_a=ya, labels_b=yb, mix=None if lb is None else mix_of(lam_v), gap=gap)


# ---------------------------------------------------------------------------------------------------------------------
def focal_f32(logits, ya, yb, mix, alpha, gamma, mutant=None):
    """the kernel, operation by operation in float32"""
    B = ya.size
    alpha, gamma, one, zero = _f(alpha), _f(gamma), _f(1), _f(0)
    l0, l1 = logits[:, 0], logits[:, 1]
    if mutant == "gamma_minus_one_for_gamma" and gamma >= 1:
        gamma = gamma - one
    with np.errstate(all="ignore"):
        mx = np.maximum(l0, l1)
        d0, d1 = l0 - mx, l1 - mx
        e0, e1 = np.exp(d0), np.exp(d1)
        S = e0 + e1
        ls = np.log(S)
        n0, n1, p0, p1 = ls - d0, ls - d1, e0 / S, e1 / S

        def row(y):
            pt, q, n = np.where(y == 1, p1, p0), np.where(y == 1, p0, p1), np.where(y == 1, n1, n0)
            if mutant == "q_as_one_minus_pt":
                q = one - pt
            if gamma == 0:
                w = k = np.ones(B, dtype=np.float32)
            else:
                if gamma == 2:
                    w, dw = q * q, _f(2) * q
                elif gamma == 1:
                    w, dw = q, np.ones(B, dtype=np.float32)
                else:
                    w, dw = np.power(q, gamma), gamma * np.power(q, gamma - one)
                k = w if mutant == "pt_ce_term_missing" else w + (dw * pt) * n
            ak = k if mutant == "alpha_missing_from_gradient" else alpha * k
            return (alpha * w) * n, ak * (p0 - np.where(y == 0, one, zero)), ak * (p1 - np.where(y == 1, one, zero))

        fl, g0, g1 = row(ya)
        if yb is not None:
            lam, mb = (mix[1], mix[0]) if mutant == "lam_and_one_minus_lam_swapped" else (mix[0], mix[1])
            fb, h0, h1 = row(ya if mutant == "labels_b_ignored" else yb)
            fl, g0, g1 = lam * fl + mb * fb, lam * g0 + mb * h0, lam * g1 + mb * h1
        Bf = _f(2 * B if mutant == "mean_over_2B" else B)
        fl = fl.astype(np.float32)
        d = np.stack([g0 / Bf, g1 / Bf], 1).astype(np.float32)
        loss = block_sum_f32(fl) / Bf
    return dict(loss_rows=fl, loss=np.array([loss]), d_logits=d)


def zero_mask(inp, gamma):
    """rows at |gap| = 100 whose label(s) name the winner, gamma >= 1: loss and gradient are exactly 0"""
    win = (inp["gap"] < 0).astype(np.int64)
    m = (np.abs(inp["gap"]) >= 100) & (inp["labels_a"] == win) & (gamma >= 1)
    return m if inp["labels_b"] is None else m & (inp["labels_b"] == win)


def with_zero_rows(case, inp, out):
    m = zero_mask(inp, case[1][1])
    d = np.asarray(out["d_logits"], dtype=np.float64).reshape(-1, 2)
    out = dict(out)
    out["zero_rows"] = np.where(m, np.abs(np.asarray(out["loss_rows"], dtype=np.float64)) + np.abs(d[:, 0]) + np.abs(d[:, 1]), 0.0)
    return out


def _restate(case, inp, mutant=None):
    return with_zero_rows(case, inp, focal_f32(inp["logits"], inp["labels_a"], inp["labels_b"], inp["mix"], case[1][0], case[1][1], mutant))


# ---------------------------------------------------------------------------------------------------------------------
def rows_ref_bound(logits, y, alpha, gamma):
    """float64 (fl, d_fl, g (B, 2), d_g, q) of every row for the labels y; the derivation is in the module docstring"""
    B = y.size
    alpha, gamma = _d(alpha), _d(gamma)
    l = logits.astype(np.float64)
    l0, l1 = l[:, 0], l[:, 1]
    mx = np.maximum(l0, l1)
    gap = np.abs(l0 - l1)
    d = np.stack([l0 - mx, l1 - mx], 1)
    e = np.exp(d)
    S = e.sum(1)
    ls = np.log1p(e.min(1))                                # S = 1 + the loser's exponential (1 + 1 at gap 0): nothing is lost at 1e-44
    n = ls[:, None] - d
    p = e / S[:, None]
    lose = d < 0
    rho_e = np.where(lose, 3 * U * gap[:, None] + HW_ULP, 0.0)
    d_e = e * rho_e + np.where(lose, TINY, 0.0)
    d_S = d_e.sum(1) + U * S
    d_ls = d_S / S + 2 * U * np.abs(ls)
    d_n = d_ls[:, None] + U * np.abs(d) + U * np.abs(n)
    d_p = p * (rho_e + (d_S / S)[:, None] + DIV) + TINY
    r, yi = np.arange(B), y.astype(int)
    pt, q, ce = p[r, yi], p[r, 1 - yi], n[r, yi]
    d_pt, d_q, d_ce = d_p[r, yi], d_p[r, 1 - yi], d_n[r, yi]
    if gamma == 0:
        w, d_w, k, d_k = np.ones(B), np.zeros(B), np.ones(B), np.zeros(B)
    else:
        r_q = d_q / np.maximum(q, 1e-300)
        if gamma == 1:
            w, d_w, dw, d_dw = q, d_q, np.ones(B), np.zeros(B)
        elif gamma == 2:
            w, dw = q * q, 2 * q
            d_w, d_dw = w * (2 * r_q + U) + TINY, dw * r_q + TINY
        else:
            w, dw = q ** gamma, gamma * q ** (gamma - 1)
            d_w, d_dw = w * (gamma * r_q + POW) + TINY, dw * ((gamma - 1) * r_q + POW + U) + TINY
        a = dw * pt
        d_a = d_dw * pt + dw * d_pt + U * a + TINY
        t = a * ce
        d_t = d_a * ce + a * d_ce + U * t + TINY
        k = w + t
        d_k = d_w + d_t + U * k
    aw = alpha * w
    d_aw = alpha * d_w + U * aw + TINY
    fl = aw * ce
    d_fl = d_aw * ce + aw * d_ce + U * fl + TINY
    ak = alpha * k
    d_ak = alpha * d_k + U * ak
    onehot = np.stack([yi == 0, yi == 1], 1).astype(np.float64)
    diff = p - onehot
    d_diff = d_p + U * np.abs(diff)
    g = ak[:, None] * diff
    d_g = d_ak[:, None] * np.abs(diff) + ak[:, None] * d_diff + U * np.abs(g) + TINY
    return fl, d_fl, g, d_g, q


def focal_ref_bound(logits, ya, yb, mix, alpha, gamma):
    B = ya.size
    fl, d_fl, g, d_g, _ = rows_ref_bound(logits, ya, alpha, gamma)
    if yb is not None:
        m0, m1 = float(mix[0]), float(mix[1])
        fb, d_fb, h, d_h, _ = rows_ref_bound(logits, yb, alpha, gamma)
        d_fl = m0 * d_fl + m1 * d_fb + U * (np.abs(m0 * fl) + np.abs(m1 * fb)) + U * np.abs(m0 * fl + m1 * fb) + 3 * TINY
        d_g = m0 * d_g + m1 * d_h + U * (np.abs(m0 * g) + np.abs(m1 * h)) + U * np.abs(m0 * g + m1 * h) + 3 * TINY
        fl, g = m0 * fl + m1 * fb, m0 * g + m1 * h
    D = -(-B // 256) + 8
    dl = g / B
    d_dl = d_g / B + DIV * np.abs(dl) + TINY
    loss = fl.sum() / B
    d_loss = (d_fl.sum() + D * U * np.abs(fl).sum()) / B + DIV * abs(loss) + TINY
    return dict(loss_rows=(fl, d_fl), loss=(np.array([loss]), np.array([d_loss])), d_logits=(dl, d_dl))


def _reference(case, inp):
    out = focal_ref_bound(inp["logits"], inp["labels_a"], inp["labels_b"], inp["mix"], case[1][0], case[1][1])
    out["zero_rows"] = (np.zeros(case[0]), np.zeros(case[0]))
    return out


def closed_form(gap, gamma):
    """(c, c') of the module docstring"""
    c = gamma * (3 * gap + 9) + 12
    return c, c + gamma + 8


OPS: Dict[str, Op] = {"focal": Op(_cases(), _make, _reference, _restate, MUTANTS)}


def check(case, inp, got: Dict[str, np.ndarray], refs=None) -> Dict[str, float]:
    """error / bound of every output of a case"""
    refs = _reference(case, inp) if refs is None else refs
    assert set(refs) == set(got), (case, sorted(refs), sorted(got))
    return {k: worst_ratio(np.asarray(got[k], dtype=np.float64).reshape(np.shape(refs[k][0])), *refs[k]) for k in refs}


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/recipe.npz: the reference's own FocalLoss / mixup_criterion in fp32 (tests/golden/make_golden_recipe.py)
def reference_error(logits, y, alpha, gamma):
    """(d_rows, d_g (R, 2)): how far the REFERENCE's fp32 evaluation may lie from the float64 value, per row.  It forms
    ce = F.cross_entropy (log_softmax in fp32: d_ce = 4 u (1 + ce)), pt = exp(-ce) (1 ulp of a number below 1, plus pt d_ce) and then
    1 - pt, exact as a subtraction but carrying pt's absolute error: delta = 4 u (1 + ce) on q, i.e. a relative delta / q that is 100 %
    once q is near 2^-24.  Through the power (convex for gamma >= 1: the upper side is the larger deviation):
        d(q^gamma) = (q + delta)^gamma - q^gamma,      d(gamma q^(gamma-1)) = gamma ((q + delta)^(gamma-1) - q^(gamma-1)),
    d_rows = alpha (d(q^gamma) ce + (q + delta)^gamma d_ce) + 4 u |fl|; autograd's gradient is alpha k (softmax - onehot) with
    k = q^gamma + gamma q^(gamma-1) pt ce from the same fp32 q: d_k = d(q^gamma) + d(gamma q^(gamma-1)) pt ce + gamma (q + delta)^(gamma-1)
    (delta ce + pt d_ce) + 8 u k, softmax - onehot within 4 u."""
    alpha, gamma = _d(alpha), _d(gamma)
    fl, _, g, _, q = rows_ref_bound(logits, y, alpha, gamma)
    l = logits.astype(np.float64)
    mx = l.max(1)
    d = l - mx[:, None]
    e = np.exp(d)
    ls = np.log1p(e.min(1))
    p = e / e.sum(1)[:, None]
    r, yi = np.arange(y.size), y.astype(int)
    ce, pt = (ls[:, None] - d)[r, yi], p[r, yi]
    diff = p - np.stack([yi == 0, yi == 1], 1)
    d_ce = 4 * U * (1 + ce)
    delta = 4 * U * (1 + ce)
    hi = q + delta
    if gamma == 0:
        dW, dDW, Whi, DWhi = np.zeros_like(q), np.zeros_like(q), np.ones_like(q), np.zeros_like(q)
    else:
        dW, Whi = hi ** gamma - q ** gamma, hi ** gamma
        dDW, DWhi = gamma * (hi ** (gamma - 1) - q ** (gamma - 1)), gamma * hi ** (gamma - 1)
    d_rows = alpha * (dW * ce + Whi * d_ce) + 4 * U * np.abs(fl) + TINY
    k_hi = Whi + DWhi * pt * ce
    d_k = dW + dDW * pt * ce + DWhi * (delta * ce + pt * d_ce) + 8 * U * k_hi
    d_g = alpha * (d_k[:, None] * np.abs(diff) + k_hi[:, None] * 4 * U) + TINY
    return d_rows, d_g


def fixture_checks(z, k, got_rows, got_mean, got_d, mixed):
    """error / (device bound + reference error) of the rows, the mean and the moderate-gap gradient of fixture entry k.
    got_rows, got_mean: ufnd_softmax_focal over all R rows; got_d: its d_logits over the moderate rows alone (B = their number)."""
    alpha, gamma = (float(v) for v in z["focal/alpha_gamma"][k])
    lg, ya, yb, m = z["focal/logits"], z["focal/labels_a"], z["focal/labels_b"], z["focal/moderate"]
    mix = mix_of(float(z["focal/lam"])) if mixed else None
    sfx = "_mixed" if mixed else ""

    def tol(rows):
        dev = focal_ref_bound(lg[rows], ya[rows], yb[rows] if mixed else None, mix, alpha, gamma)
        ra, ga = reference_error(lg[rows], ya[rows], alpha, gamma)
        if mixed:
            rb, gb = reference_error(lg[rows], yb[rows], alpha, gamma)
            ra, ga = float(mix[0]) * ra + float(mix[1]) * rb, float(mix[0]) * ga + float(mix[1]) * gb
        return dev, ra + 4 * U * np.abs(dev["loss_rows"][0]), ga / len(rows) + 4 * U * np.abs(dev["d_logits"][0])
    every = np.arange(ya.size)
    dev, d_rows, _ = tol(every)
    out = {"rows": worst_ratio(np.asarray(got_rows, np.float64), z[f"focal/{k}/rows{sfx}"].astype(np.float64), dev["loss_rows"][1] + d_rows),
           "mean": worst_ratio(np.asarray([got_mean], np.float64), np.asarray([z[f"focal/{k}/mean{sfx}"]], np.float64),
                               dev["loss"][1] + d_rows.mean() + 8 * U * np.abs(dev["loss_rows"][0]).mean())}
    dev, _, d_g = tol(m)
    out["d"] = worst_ratio(np.asarray(got_d, np.float64).reshape(-1, 2), z[f"focal/{k}/d{sfx}"].astype(np.float64), dev["d_logits"][1] + d_g)
    return out
