"""Cases, float64 references, derived error bounds, float32 restatements and mutants of the end of the training step:
cross-entropy (softmax_ce_kernel / softmax_ce_ws_kernel in csrc/tier_a.hip) and everything in csrc/optim.hip
(grad_accumulate_kernel, sumsq_kernel, norm_finalize_kernel, adamw_kernel, step_advance_kernel, sumsq_advance_kernel,
adamw_clip_kernel).  Shared by tests/test_step_tail_cases.py (CPU: every restatement stays inside its bound and is bit-equal
on the exact cases, every mutant is caught, the table reaches every grid class) and tests/test_gpu_step_tail.py (GPU: every
case through the C ABI).  The layout is that of tests/frozen_ops_cases.py, whose U, HW_ULP, MUTANT_FACTOR and worst_ratio
are used here: an `Op` has `cases`, `make`, `reference -> {output: (ref float64, bound float64)}`, `restate(case, inputs,
mutant)` and its mutants; a bound of 0 means bit equality.

Grids (recomputed here from the launchers' formulas, and asserted by the CPU test to be reached class by class), n4 = n / 4:
  AdamW and accumulate: blocks = clamp(ceil(n4 / 512), 1, 2048), stride = 256 blocks; a pair loop `i + stride < n4` that handles
  elements i and i + stride, then a tail loop.  Norm: blocks = clamp(ceil(n4 / 1024), 1, 1024), a plain grid-stride loop, one
  fp32 partial per block; the finalize adds the partials in float64, thread k taking partials k, k + 256, ...

Exact families (bound 0):
  accumulate      overwrite copies bits (NaN payloads, -0.0: compared as uint32); add is ONE IEEE addition per element, so it
                  equals NumPy's float32 dst + src bit for bit.
  step_census     integers throughout: g = ga + gb with |ga|, |gb| <= 7 (so |g| <= 14 <= 15), p, m in [-8, 8], v in [0, 8];
                  lr = 0, beta1 = 0.5, beta2 = 0.75, eps = 1, grad_scale = 1, max_norm = 0.  A block of the norm sees at most
                  ceil(n / 1024 blocks) <= 8212 floats of at most 14^2: its sum stays below 1.7e6 < 2^24, every partial is a whole
                  number and their float64 sum is the integer sum of squares: a float4 read twice or not at all changes it by a
                  whole number at any n.  m' = 0.5 m + 0.5 g and v' = 0.75 v + 0.25 g^2 are exact, p keeps its bits (step_size =
                  0 / bc1 = 0, decay = 1 - 0 = 1, denom >= eps = 1 is finite).  Only grad_norm is rounded: float32(sqrt(S)) --
                  one float32 ulp is allowed.
  norm_select     a one-hot gradient of value 3: the sum of squares is 9 wherever it is read, sqrt(9) = 3, and 3 |grad_scale| is
                  exact for grad_scale in {1, 0.5, -0.25}.
  adamw_zero_grad g = m = v = 0: mq = vq = 0, denom = fma(0, inv_bc2, eps) = eps, 0 / eps = 0, p' = fma(-step_size, 0, p decay)
                  = float32(p decay) -- one rounding, and decay = float32(1 - float32(lr wd)).
  counters        step and micro are integers; bc1 and bc2_sqrt are float32 roundings of a double-precision pow / sqrt (below).

Rounded families.  u = 2^-24 (U) per fp32 operation; a division is HIP's promised 2.5 ulp = 5 u (HIP programming guide, "HIP
math API", single-precision table; tests/gemm_bf16_cases.py uses the same figure); sqrtf and logf are 1 ulp = 2 u in the same
table; v_exp_f32 is 1 ulp = HW_ULP (CDNA ISA reference).  A fused multiply-add rounds once.  Second-order terms (products of
two errors, below 1e-6 of the bound) are left out.
  norm            one thread adds (sweeps) group sums, each group ((s0 + s1) + s2) + s3 of four squares: depth sweeps + 4; the
                  wave's six levels and the block's two follow: the partial is within (sweeps + 12) u of itself, all terms being
                  positive.  The float64 finalize adds nothing visible; the square root halves the relative error; its rounding
                  to float32 and the product with |grad_scale| are u each:     rho_n = (sweeps + 12) u / 2 + 2 u.
  clip_coef       min(1, max_norm / (norm + 1e-6)): the addition u, the division 5 u; min is 1-Lipschitz, so the same bound
                  holds on both sides of the threshold:                        rho_c = rho_n + 6 u  (0 when max_norm <= 0).
  bc1, bc2_sqrt   1 - pow(beta, t) and its sqrt in double (errors ~1e-16, up to 1e-13 relative after the cancellation at t = 1),
                  carried as ONE rounding to float32:                          rho_bc = u (1 + 1e-5).
  AdamW           per element, with gs = grad_scale clip_coef (u), gq = g gs (u): rho_g = 2 u + rho_c;
                  decay = 1 - lr wd: d_decay = u lr wd + u |decay|;  pq = p decay: d_pq = |p| d_decay + u |pq|;
                  mq = fma(m, b1, (1 - b1) gq): d_m = |b| (2 u + rho_g) + u (|a| + |b|), a = m b1, b = (1 - b1) gq -- the sum of
                  magnitudes, because a and b may cancel;
                  vq = fma(v, b2, ((1 - b2) gq) gq): d_v = e (3 u + 2 rho_g) + u (c + e), c = v b2, e = (1 - b2) gq^2;
                  s = sqrtf(vq): d_s = d_v / (2 s) + 2 u s  (d_v = 0 where vq = 0);
                  inv = 1 / bc2_sqrt: rho_inv = 5 u + rho_bc;  denom = fma(s, inv, eps): d_den = s inv rho_inv + d_s inv + u denom;
                  q = mq / denom: d_q = d_m / denom + |q| d_den / denom + 5 u |q|;
                  step_size = lr / bc1: rho_ss = 5 u + rho_bc;
                  p' = fma(-step_size, q, pq): d_p = step_size (d_q + |q| rho_ss) + d_pq + u (|pq| + step_size |q|).
  cross-entropy   per row, gap = |l0 - l1|, d_c = l_c - max (0 for the winner, -gap for the loser: u gap), e_c = __expf(d_c) =
                  v_exp_f32(d_c log2(e)): the product and the constant cost 2 u |d_c|, the input u |d_c|, the instruction HW_ULP:
                  rho_e = 3 u gap + HW_ULP for the loser, and exp(0) = 1 exactly for the winner.  A result below 2^-126 may be
                  flushed: TINY = 2^-126 absolute.  S = e0 + e1 in [1, 2]: d_S = e_lose rho_e + TINY + u S.
                  ls = logf(S): d_ls = d_S / S + 2 u |ls|.   n_c = ls - d_c: d_n = d_ls + u |d_c| + u |n_c|.
                  p_c = e_c / S: d_p = p_c (rho_e,c + d_S / S + 5 u) + TINY.
                  NOTHING here scales with |max|: the bound is a function of the gap alone, which is what the shifted cases
                  (the same logits + 1024) hold the kernels to.
                  loss row (weighted form) lr = ((1 - eps) wy) n_y + (0.5 eps) (w0 n0 + w1 n1):
                  d_lr = (1-eps) wy d_ny + 3 u |A| + 0.5 eps (w0 d_n0 + w1 d_n1) + 3 u |B| + u |lr|; the plain form is n_y alone.
                  W = sum of w[y_i] over depth D = ceil(B / 256) + 8, all positive: rho_W = D u (0 for the plain form: float(B)).
                  loss_rows = lr / W: d = d_lr / W + |row| (rho_W + 5 u).
                  state->loss = sum(lr) / W: d = (sum d_lr + D u sum |lr|) / W + |loss| (rho_W + 5 u).
                  d_logits_c = (p_c k - [c = y] (1 - eps) wy - 0.5 eps w_c) / W, k = (1 - eps) wy + 0.5 eps (w0 + w1) (5 u k; exact
                  1 in the plain form): d_num = d_p k + p_c d_k + u T1 + 2 u T2 + u T3 + 2 u (T1 + T2 + T3), then
                  d = d_num / W + |d_logits| (rho_W + 5 u) + TINY.
No term of any bound comes from a kernel's output.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple

import numpy as np

from tests.frozen_ops_cases import HW_ULP, MUTANT_FACTOR, U, Op, case_id, worst_ratio  # noqa: F401

ADAMW_PER_BLOCK, ADAMW_CAP = 512, 2048      # ufnd_adamw_step, ufnd_clip_adamw_step (launch 2), ufnd_grad_accumulate
NORM_PER_BLOCK, NORM_CAP = 1024, 1024       # ufnd_grad_norm, ufnd_clip_adamw_step (launch 1)
TINY = 2.0 ** -126
DIV = 5 * U                                 # 2.5 ulp
SENTINEL_F32 = 12345.678
PARTIALS_FLOATS = NORM_CAP
HALF_CAP = ADAMW_CAP * 256                  # 524,288: one sweep of the capped AdamW grid

ONE_BLOCK = (1, 63, 64, 65, 255, 256, 257)
ADAMW_STEP = (511, 512, 513)
NORM_STEP = (1023, 1024, 1025)
FINALIZE_BLOCKS = (255, 256, 257, 1023)
FINALIZE = tuple(b * NORM_PER_BLOCK for b in FINALIZE_BLOCKS)
CAPS = (2 * HALF_CAP, 2 * HALF_CAP + 1, 3 * HALF_CAP - 1, 3 * HALF_CAP + 1, 4 * HALF_CAP + 5)
SIZE_CLASSES = {"one_block": ONE_BLOCK, "adamw_block_step": ADAMW_STEP, "norm_block_step": NORM_STEP, "finalize_stride": FINALIZE,
                "caps": CAPS}
ALL_SIZES = ONE_BLOCK + ADAMW_STEP + NORM_STEP + FINALIZE + CAPS
SMALL_SIZES = ONE_BLOCK + ADAMW_STEP + NORM_STEP
LARGE_FLOATS = 1_000_000


def adamw_grid(n4):
    """(blocks, stride in float4, sweeps) of the AdamW / accumulate launch"""
    want = (n4 + ADAMW_PER_BLOCK - 1) // ADAMW_PER_BLOCK
    blocks = min(max(want, 1), ADAMW_CAP)
    return blocks, blocks * 256, -(-n4 // (blocks * 256))


def norm_grid(n4):
    want = (n4 + NORM_PER_BLOCK - 1) // NORM_PER_BLOCK
    blocks = min(max(want, 1), NORM_CAP)
    return blocks, blocks * 256, -(-n4 // (blocks * 256))


def pair_and_tail(n4):
    """(float4 handled by the pair loop, float4 handled by the tail loop) of the AdamW / accumulate kernels"""
    _, stride, _ = adamw_grid(n4)
    x = np.arange(n4)
    sweep = x // stride
    tail = (sweep % 2 == 0) & (x + stride >= n4)
    return int(n4 - tail.sum()), int(tail.sum())


class HP(NamedTuple):
    lr: float = 2e-4
    wd: float = 1e-4
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    max_norm: float = 5.0
    gs: float = 1.0


CENSUS_HP = HP(lr=0.0, wd=1e-4, b1=0.5, b2=0.75, eps=1.0, max_norm=0.0, gs=1.0)


def _seed(*ints):
    return np.random.default_rng([20261018] + [int(i) for i in ints])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f(x):
    return np.float32(x)


def _d(x):
    """the float64 value of the float32 the kernel is given"""
    return float(np.float32(x))


def bits(a):
    """float32 -> its uint32 bit patterns as float64 (exact), for bit comparisons that tell NaN payloads and -0.0 apart"""
    return _f32(a).view(np.uint32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# which float4 the AdamW / accumulate grid visits how often (the mutants are wrong loops)
GRID_MUTANTS = ("last_float4_skipped", "pair_second_skipped", "tail_sweep_dropped_at_cap", "element_updated_twice")


def adamw_visits(n4, mutant=None):
    v = np.ones(n4, dtype=np.int8)
    if mutant not in GRID_MUTANTS:
        return v
    blocks, stride, _ = adamw_grid(n4)
    if mutant == "last_float4_skipped":
        v[-1] = 0
    elif mutant == "element_updated_twice":
        v[n4 // 2] = 2
    else:
        x = np.arange(n4)
        sweep = x // stride
        if mutant == "pair_second_skipped":
            odd = np.flatnonzero(sweep & 1)
            if odd.size:
                v[odd[-1]] = 0
        else:      # tail_sweep_dropped_at_cap: a thread that ran the pair loop skips its tail element.  The mutant does not look at
            v[(sweep >= 2) & (sweep % 2 == 0) & (x + stride >= n4)] = 0      # the block count: only a capped grid HAS a third sweep
    return v


def _apply(vis, old, once, twice):
    if vis is None:
        return once
    vv = np.repeat(vis, 4)
    return np.where(vv == 0, old, np.where(vv == 2, twice, once))


def acc_f32(dst, src, overwrite, mutant=None):
    ow = overwrite and mutant != "accumulate_adds_on_overwrite"
    with np.errstate(invalid="ignore", over="ignore"):
        once = src.copy() if ow else dst + src
        if mutant not in GRID_MUTANTS:
            return once
        twice = once if ow else once + src
    return _apply(adamw_visits(dst.size // 4, mutant), dst, once, twice)


def sumsq_partials_f32(g, mutant=None):
    """the per-block fp32 partials in the kernel's order: a thread's sweeps in sequence, a tree over the wave, (w0 + w1) + (w2 + w3)"""
    n4 = g.size // 4
    blocks, stride, sweeps = norm_grid(n4)
    q = g.reshape(n4, 4)
    s4 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    if mutant == "last_float4_skipped":
        s4[-1] = 0
    elif mutant == "element_updated_twice":
        s4[n4 // 2] *= _f(2)
    pad = np.zeros(sweeps * stride, dtype=np.float32)
    pad[:n4] = s4
    t = pad.reshape(sweeps, stride)
    acc = np.zeros(stride, dtype=np.float32)
    for k in range(sweeps):
        acc = acc + t[k]
    x = acc.reshape(blocks, 4, 64)
    for _ in range(6):
        x = x[..., 0::2] + x[..., 1::2]
    sh = x[..., 0]
    return (sh[:, 0] + sh[:, 1]) + (sh[:, 2] + sh[:, 3])


def finalize_f32(partials, hp: HP, t, mutant=None):
    """grad_norm, clip_coef, bc1, bc2_sqrt as the finalize (or launch 2 of the fused form) derives them for step t"""
    ps = partials[:256] if mutant == "finalize_first_256_partials" else partials[:1] if mutant == "finalize_reads_one_partial" else partials
    S = float(np.sum(ps.astype(np.float64)))
    total = _f(math.sqrt(S)) * (_f(1) if mutant == "norm_without_grad_scale" else np.abs(_f(hp.gs)))
    coef = _f(1)
    if hp.max_norm > 0:
        coef = min(_f(1), _f(hp.max_norm) / (total + (_f(0) if mutant == "clip_without_1e-6" else _f(1e-6))))
    if mutant == "bias_corrections_at_t_minus_1":
        t = t - 1
    bc1 = _f(1.0 - _d(hp.b1) ** t)
    bc2 = _f(math.sqrt(1.0 - _d(hp.b1 if mutant == "beta1_in_second_correction" else hp.b2) ** t))
    return _f(total), _f(coef), bc1, bc2


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.float64(b) + np.asarray(c, np.float64)).astype(np.float32)


def adamw_f32(p, g, m, v, hp: HP, coef, bc1, bc2, mutant=None):
    lr, wd, b1, b2, eps = _f(hp.lr), _f(hp.wd), _f(hp.b1), _f(hp.b2), _f(hp.eps)
    with np.errstate(all="ignore"):
        decay = _f(1) - lr * wd
        gsv = (np.abs(_f(hp.gs)) if mutant == "update_with_abs_grad_scale" else _f(hp.gs)) * coef
        step_size, inv = lr / bc1, _f(1) / bc2

        def once(p, m, v):
            gq, pq = g * gsv, p * decay
            if mutant == "weight_decay_folded_into_gradient":
                gq, pq = gq + wd * p, p
            mq = _fma(m, b1, (_f(1) - b1) * gq)
            vq = _fma(v, b2, ((_f(1) - b2) * gq) * gq)
            if mutant == "eps_inside_sqrt":
                denom = np.sqrt(vq * inv * inv + eps)
            else:
                denom = _fma(np.sqrt(vq), inv, eps)
            return _fma(mq / denom, -step_size, pq), mq, vq

        o = once(p, m, v)
        if mutant not in GRID_MUTANTS:
            return o
        vis = adamw_visits(p.size // 4, mutant)
        tw = once(*o) if (vis == 2).any() else o
        return tuple(_apply(vis, old, a, b) for old, a, b in zip((p, m, v), o, tw))


def step_f32(p, g, m, v, hp: HP, step0, micro0, mutant=None):
    """one optimizer step (either form: they agree bit for bit) -> every output the GPU test reads back"""
    t = step0 + 1
    partials = sumsq_partials_f32(g, mutant)
    total, coef, bc1, bc2 = finalize_f32(partials, hp, t, mutant)
    pn, mn, vn = adamw_f32(p, g, m, v, hp, coef, bc1, bc2, mutant)
    step = step0 + (2 if mutant == "step_advanced_twice" else 1)
    micro = micro0 if mutant == "micro_not_reset" else 0
    return dict(p=pn, m=mn, v=vn, grad_norm=np.array([total]), clip_coef=np.array([coef]), bc1=np.array([bc1]), bc2_sqrt=np.array([bc2]),
                step=np.array([float(step)]), micro=np.array([float(micro)]), partials=partials)


# ---------------------------------------------------------------------------------------------------------------------
# float64 references and bounds of the optimizer
def rho_norm(n4):
    return (norm_grid(n4)[2] + 12) * U / 2 + 2 * U


RHO_BC = U * (1 + 1e-5)


def scalars_ref(g, hp: HP, t):
    """{grad_norm, clip_coef, bc1, bc2_sqrt: (ref, bound)} and rho_c"""
    gs, mx = _d(hp.gs), _d(hp.max_norm)
    g64 = g.astype(np.float64)
    norm = math.sqrt(float(np.dot(g64, g64))) * abs(gs)
    rn = rho_norm(g.size // 4)
    coef, rc = 1.0, 0.0
    if mx > 0:
        coef, rc = min(1.0, mx / (norm + _d(1e-6))), rn + 6 * U
    bc1 = 1.0 - _d(hp.b1) ** t
    bc2 = math.sqrt(1.0 - _d(hp.b2) ** t)
    one = lambda r, b: (np.array([r]), np.array([b]))
    return dict(grad_norm=one(norm, norm * rn), clip_coef=one(coef, coef * rc), bc1=one(bc1, bc1 * RHO_BC), bc2_sqrt=one(bc2, bc2 * RHO_BC)), rc


def adamw_ref_bound(p, g, m, v, hp: HP, t):
    """{p, m, v, scalars: (ref, bound)} of one step in float64 (the derivation is in the module docstring)"""
    sc, rc = scalars_ref(g, hp, t)
    lr, wd, b1, b2, eps, gs = (_d(x) for x in (hp.lr, hp.wd, hp.b1, hp.b2, hp.eps, hp.gs))
    coef, bc1, bc2 = sc["clip_coef"][0][0], sc["bc1"][0][0], sc["bc2_sqrt"][0][0]
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    rho_g = 2 * U + rc
    decay = 1.0 - lr * wd
    d_decay = U * lr * wd + U * abs(decay)
    gq = g * (gs * coef)
    pq = p * decay
    d_pq = np.abs(p) * d_decay + U * np.abs(pq)
    a, b = m * b1, (1.0 - b1) * gq
    mq = a + b
    d_m = np.abs(b) * (2 * U + rho_g) + U * (np.abs(a) + np.abs(b))
    c, e = v * b2, (1.0 - b2) * gq * gq
    vq = c + e
    d_v = e * (3 * U + 2 * rho_g) + U * (c + e)
    s = np.sqrt(vq)
    d_s = np.where(vq > 0, d_v / (2 * np.where(vq > 0, s, 1.0)), 0.0) + 2 * U * s
    inv, rho_inv = 1.0 / bc2, DIV + RHO_BC
    denom = s * inv + eps
    d_den = s * inv * rho_inv + d_s * inv + U * denom
    q = mq / denom
    d_q = d_m / denom + np.abs(q) * d_den / denom + DIV * np.abs(q)
    ss, rho_ss = lr / bc1, DIV + RHO_BC
    pn = pq - ss * q
    d_p = ss * (d_q + np.abs(q) * rho_ss) + d_pq + U * (np.abs(pq) + ss * np.abs(q))
    out = dict(sc)
    out.update(p=(pn, d_p), m=(mq, d_m), v=(vq, d_v))
    return out


def _exact(d):
    return {k: (np.asarray(a, dtype=np.float64), np.zeros(np.shape(a))) for k, a in d.items()}


# ------------------------------------------------------------------ accumulate
def _acc_cases():
    out = []
    for i, n4 in enumerate(SMALL_SIZES):
        out.append((n4, "bits", i % 2 == 0))
        out.append((n4, "add", i % 2 == 1))
    return out


def _acc_make(case):
    n4, kind, _ = case
    n = 4 * n4
    rng = _seed(1, n4, kind == "add")
    src = _f32(rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 7, n))
    dst = _f32(rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 7, n))
    if kind == "bits":       # NaNs with payloads, both infinities, both zeros: spread over the first, the last and inner elements
        special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
        for k, s in enumerate(special):
            src[(k * 37 + (n - 1) * (k % 2)) % n] = s
        src[n - 1] = special[1]
        if n > 1:
            src[0] = special[5]
    else:
        src[n - 1], dst[0] = np.float32(np.inf), np.float32(-0.0)
        src[0] = np.float32(-0.0) if n > 1 else src[0]
        if n > 8:
            src[5], dst[5] = np.float32(1e38), np.float32(3e38)      # overflows to +inf
    return dict(dst=dst, src=src, micro0=3)


def _acc_restate(case, inp, mutant=None):
    _, kind, with_state = case
    out = acc_f32(inp["dst"], inp["src"], kind == "bits", mutant)
    return dict(dst_bits=bits(out), micro=np.array([float(inp["micro0"] + (1 if with_state else 0))]))


def _acc_reference(case, inp):
    return _exact(_acc_restate(case, inp))


# ------------------------------------------------------------------ step_census
def _census_cases():
    return [(n4, 148 if i % 3 == 1 else 64) for i, n4 in enumerate(ALL_SIZES)]


def _census_make(case):
    n4, _ = case
    n = 4 * n4
    rng = _seed(2, n4)
    i8 = lambda lo, hi: rng.integers(lo, hi + 1, n, dtype=np.int8).astype(np.float32)
    return dict(ga=i8(-7, 7), gb=i8(-7, 7), p=i8(-8, 8), m=i8(-8, 8), v=i8(0, 8), hp=CENSUS_HP, step0=0)


def _census_restate(case, inp, mutant=None):
    n = inp["ga"].size
    junk = np.full(n, SENTINEL_F32, dtype=np.float32)
    g = acc_f32(junk, inp["ga"], True, mutant)
    g = acc_f32(g, inp["gb"], False, mutant)
    if mutant in GRID_MUTANTS:      # the optimizer sees a correct gradient: one wrong loop at a time
        g_ok = inp["ga"] + inp["gb"]
    else:
        g_ok = g
    o = step_f32(inp["p"], g_ok, inp["m"], inp["v"], inp["hp"], inp["step0"], 2, mutant)
    o["partials_sum"] = np.array([float(np.sum(o.pop("partials").astype(np.float64)))])
    o["g"] = g
    return o


def _census_reference(case, inp):
    g = inp["ga"].astype(np.float64) + inp["gb"].astype(np.float64)
    S = float(np.dot(g, g))
    m, v = inp["m"].astype(np.float64), inp["v"].astype(np.float64)
    out = _exact(dict(g=g, partials_sum=[S], p=inp["p"], m=0.5 * m + 0.5 * g, v=0.75 * v + 0.25 * g * g, clip_coef=[1.0], bc1=[0.5],
                      bc2_sqrt=[0.5], step=[1.0], micro=[0.0]))
    norm = math.sqrt(S)
    out["grad_norm"] = (np.array([norm]), np.array([float(np.spacing(np.float32(norm)))]))      # one float32 ulp
    return out


# ------------------------------------------------------------------ norm_select
SELECT_SCALES = (1.0, 0.5, -0.25)
SELECT_SIZES = (1, 65, 257, 1025, 257 * NORM_PER_BLOCK, 2 * HALF_CAP + 1)


def select_positions(n4):
    """float indices: the first, the last, and both sides of every sweep edge and of the edges of blocks 0/1, 255/256 and the last"""
    blocks, stride, sweeps = norm_grid(n4)
    n = 4 * n4
    pos = {0, n - 1}
    for s in range(1, sweeps):
        pos |= {4 * s * stride - 1, 4 * s * stride}
    for b in (1, 256, blocks - 1):
        if 0 < b < blocks:
            pos |= {4 * 256 * b - 1, 4 * 256 * b}
    return sorted(x for x in pos if 0 <= x < n)


def _select_make(case):
    return dict(pos=select_positions(case[0]))


def _select_restate(case, inp, mutant=None):
    n4 = case[0]
    out = np.zeros((len(inp["pos"]), len(SELECT_SCALES)))
    g = np.zeros(4 * n4, dtype=np.float32)
    for i, x in enumerate(inp["pos"]):
        g[x] = 3.0
        partials = sumsq_partials_f32(g, mutant)
        g[x] = 0.0
        for j, gs in enumerate(SELECT_SCALES):
            out[i, j] = finalize_f32(partials, HP(gs=gs, max_norm=0.0), 1, mutant)[0]
    return dict(grad_norm=out)


def _select_reference(case, inp):
    ref = np.tile(3.0 * np.abs(np.array(SELECT_SCALES)), (len(inp["pos"]), 1))
    return _exact(dict(grad_norm=ref))


# ------------------------------------------------------------------ norm_clip (rounded)
NORM_SIZES = (65, 1025, 3 * 1024 + 1, 200_003)
NORM_SCALES = (1e-4, 1.0, 1e3)
NORM_GS = (1.0, 1.0 / 3.0, -0.25)
CLIP_KINDS = {"below": (5.0, 5.0 * (1 - 1e-3)), "above": (5.0, 5.0 * (1 + 1e-3)), "just_below": (5.0, 5.0 * (1 - 1e-6)),
              "just_above": (5.0, 5.0 * (1 + 1e-6)), "tiny": (5e-6, 1e-5), "off": (0.0, 7.0)}      # (max_norm, the gradient's norm)


def _norm_cases():
    out = [(n4, sc, gs, 0.0, None) for n4 in NORM_SIZES for sc in NORM_SCALES for gs in NORM_GS]
    out += [(65 if i % 2 else 1025, 1.0, 1.0, mx, kind) for i, (kind, (mx, _)) in enumerate(CLIP_KINDS.items())]
    return out


def _norm_make(case):
    n4, scale, gs, _, kind = case
    rng = _seed(3, n4, int(math.log10(scale)) + 10, int(abs(gs) * 1000))
    g = rng.normal(0, scale, 4 * n4)
    if kind is not None:
        g *= CLIP_KINDS[kind][1] / math.sqrt(float(np.dot(g, g)))
    return dict(g=_f32(g))


def _norm_hp(case):
    return HP(gs=case[2], max_norm=case[3])


def _norm_restate(case, inp, mutant=None):
    total, coef, _, _ = finalize_f32(sumsq_partials_f32(inp["g"], mutant), _norm_hp(case), 1, mutant)
    return dict(grad_norm=np.array([total]), clip_coef=np.array([coef]))


def _norm_reference(case, inp):
    sc, _ = scalars_ref(inp["g"], _norm_hp(case), 1)
    return dict(grad_norm=sc["grad_norm"], clip_coef=sc["clip_coef"])


# ------------------------------------------------------------------ adamw_zero_grad
ZERO_HPS = (HP(), HP(lr=1e-2, wd=0.1))


def _zero_cases():
    return [(n4, k) for n4 in (1, 65, 257, 513) for k in range(len(ZERO_HPS))]


def _zero_make(case):
    n4, k = case
    n = 4 * n4
    z = np.zeros(n, dtype=np.float32)
    return dict(p=_f32(_seed(4, n4).normal(0, 1, n)), g=z, m=z.copy(), v=z.copy(), hp=ZERO_HPS[k], step0=0)


def _step_restate(case, inp, mutant=None):
    o = step_f32(inp["p"], inp["g"], inp["m"], inp["v"], inp["hp"], inp["step0"], 2, mutant)
    o.pop("partials")
    return o


def _zero_reference(case, inp):
    hp = inp["hp"]
    sc, _ = scalars_ref(inp["g"], hp, 1)
    decay = _f(1) - _f(hp.lr) * _f(hp.wd)
    out = _exact(dict(p=inp["p"] * decay, m=inp["m"], v=inp["v"], step=[1.0], micro=[0.0], grad_norm=[0.0], clip_coef=[1.0]))
    out.update(bc1=sc["bc1"], bc2_sqrt=sc["bc2_sqrt"])
    return out


# ------------------------------------------------------------------ adamw_rounded
#                 hyper-parameters                             gradient scale (a decade inside the array starts here)
ADAMW_HPS = {"trainer_clip_active": (HP(), 0.1), "trainer_clip_inactive": (HP(), 1e-3), "no_weight_decay": (HP(wd=0.0), 1e-3),
             "large_lr_wd": (HP(lr=1e-2, wd=0.1), 1e-2), "negative_grad_scale": (HP(gs=-0.25), 0.4)}
ADAMW_T = (1, 2, 3, 100_000)
ADAMW_SIZES = (257, 513, 2053)
EPS_ELEMENTS = 64      # elements with g = 0, v = 0, m != 0: the denominator is eps


def _adamw_cases():
    out, i = [], 0
    for name in ADAMW_HPS:
        for t in ADAMW_T:
            out.append((ADAMW_SIZES[i % 3], name, t))
            i += 1
        i += 1
    return out


def _adamw_make(case):
    n4, name, t = case
    hp, gscale = ADAMW_HPS[name]
    n = 4 * n4
    rng = _seed(5, n4, t, len(name))
    g = rng.normal(0, 1, n) * gscale * 10.0 ** rng.uniform(0, 1, n)
    p = rng.normal(0, 1, n)
    m = rng.normal(0, 1, n) * gscale * 3
    v = (rng.normal(0, 1, n) * gscale * 3) ** 2
    idx = rng.choice(n, EPS_ELEMENTS, replace=False)
    g[idx], v[idx] = 0.0, 0.0
    m[idx] = rng.choice([-1.0, 1.0], EPS_ELEMENTS) * rng.uniform(1e-9, 1e-7, EPS_ELEMENTS)      # |m| / eps of order 1: the update stays finite
    return dict(p=_f32(p), g=_f32(g), m=_f32(m), v=_f32(v), hp=hp, step0=t - 1, eps_idx=idx)


def _adamw_reference(case, inp):
    out = adamw_ref_bound(inp["p"], inp["g"], inp["m"], inp["v"], inp["hp"], case[2])
    out.update(_exact(dict(step=[float(case[2])], micro=[0.0])))
    return out


# ------------------------------------------------------------------ counters
COUNTER_RUNS = ((0, 3), (99_999, 1))      # (state->step at the start, optimizer steps taken)


def _counter_make(case):
    n = 4 * 65
    rng = _seed(6, case[0])
    return dict(p=_f32(rng.normal(0, 1, n)), g=_f32(rng.normal(0, 0.01, n)), m=_f32(rng.normal(0, 0.01, n)),
                v=_f32(rng.normal(0, 0.01, n) ** 2), hp=HP())


def _counter_restate(case, inp, mutant=None):
    """every step is preceded by two accumulate calls with the state (micro 0 -> 2); the step must return it to 0"""
    step0, steps = case
    p, m, v = inp["p"], inp["m"], inp["v"]
    rows = {k: [] for k in ("step", "micro_before", "micro", "bc1", "bc2_sqrt")}
    step, micro = step0, 0
    for _ in range(steps):
        micro += 2
        rows["micro_before"].append(float(micro))
        o = step_f32(p, inp["g"], m, v, inp["hp"], step, micro, mutant)
        p, m, v, step, micro = o["p"], o["m"], o["v"], int(o["step"][0]), int(o["micro"][0])
        for k in ("step", "micro", "bc1", "bc2_sqrt"):
            rows[k].append(float(o[k][0]))
    return {k: np.array(a) for k, a in rows.items()}


def _counter_reference(case, inp):
    step0, steps = case
    t = np.arange(step0 + 1, step0 + steps + 1, dtype=np.float64)
    bc1 = 1.0 - _d(HP().b1) ** t
    bc2 = np.sqrt(1.0 - _d(HP().b2) ** t)
    out = _exact(dict(step=t, micro_before=np.full(steps, 2.0), micro=np.zeros(steps)))
    out.update(bc1=(bc1, bc1 * RHO_BC), bc2_sqrt=(bc2, bc2 * RHO_BC))
    return out


# ------------------------------------------------------------------ cross-entropy
CE_B = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000)
CE_LABELS = ("mixed", "all0", "all1")
CE_ENTRIES = (None, (1.0, 1.0, 0.0), (1.0, 1.0, 0.05), (0.7, 1.9, 0.0), (0.6, 1.4, 0.05), (1.0, 1.0, 0.5))      # None = ufnd_softmax_ce
CE_LOGITS = ("randn2", "equal", "gap20", "gap90", "gap120", "one_of_each", "grid", "grid_shifted")
CE_SHIFT = 1024.0
CE_MUTANTS = ("ce_mean_over_B", "smoothing_eps_not_halved", "smoothing_missing_from_d_logits", "row_max_not_subtracted",
              "lse_rounded_at_the_common_magnitude")


def _ce_cases():
    """B x labels x entry, the logit set rotating; every `grid` case is repeated as `grid_shifted` (the same rows + 1024)"""
    kinds = [k for k in CE_LOGITS if k != "grid_shifted"]
    out, i = [], 0
    for B in CE_B:
        for labels in CE_LABELS:
            for entry in CE_ENTRIES:
                out.append((B, labels, entry, kinds[i % len(kinds)]))
                i += 1
        i += 1      # (19 steps per batch size: coprime to the 7 sets, so every entry meets every set)
    # every entry meets the shift pair and the widest gaps at a multi-sweep batch
    out += [(257, "mixed", entry, kind) for entry in CE_ENTRIES for kind in ("grid", "gap90", "gap120", "one_of_each", "equal")]
    out += [c[:3] + ("grid_shifted",) for c in out if c[3] == "grid"]
    return sorted(set(out), key=lambda c: (c[0], c[1], str(c[2]), c[3]))


def ce_logits(kind, B, rng):
    sign = rng.choice([-1.0, 1.0], B)
    base = rng.normal(0, 2, B)
    both = lambda gap: np.stack([base + sign * gap / 2, base - sign * gap / 2], 1)
    if kind == "randn2":
        lg = rng.normal(0, 2, (B, 2))
    elif kind == "equal":
        lg = np.stack([base, base], 1)
    elif kind.startswith("gap"):
        lg = both(float(kind[3:]))
    elif kind == "one_of_each":
        rows = [rng.normal(0, 2, (B, 2)), np.stack([base, base], 1), both(20.0), both(90.0), both(120.0)]
        lg = np.stack([rows[r % 5][r] for r in range(B)], 0)
    else:      # multiples of 2^-10 with |l| <= 8: exact in fp32 with 1024 added as well
        lg = rng.integers(-8 * 1024, 8 * 1024 + 1, (B, 2)) / 1024.0
        if kind == "grid_shifted":
            lg = lg + CE_SHIFT
    return _f32(lg)


def _ce_make(case):
    B, labels, _, kind = case
    rng = _seed(7, B, CE_LABELS.index(labels), CE_LOGITS.index("grid" if kind == "grid_shifted" else kind))      # the shifted case draws the same rows
    lg = ce_logits(kind, B, rng)
    y = {"mixed": rng.integers(0, 2, B), "all0": np.zeros(B, int), "all1": np.ones(B, int)}[labels].astype(np.int64)
    return dict(logits=lg, labels=y)


def _ce_w(entry):
    return (1.0, 1.0, 0.0) if entry is None else entry


def block_sum_f32(x):
    """one 256-thread block's sum in the kernels' order: thread k adds x[k], x[k + 256], ...; a tree over each wave; (w0 + w1) + (w2 + w3)"""
    sweeps = -(-x.size // 256)
    pad = np.zeros(sweeps * 256, dtype=np.float32)
    pad[:x.size] = x
    t = pad.reshape(sweeps, 256)
    acc = np.zeros(256, dtype=np.float32)
    for k in range(sweeps):
        acc = acc + t[k]
    w = acc.reshape(4, 64)
    for _ in range(6):
        w = w[:, 0::2] + w[:, 1::2]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def ce_f32(logits, y, entry, mutant=None):
    """both kernels, operation by operation in float32"""
    B = y.size
    w0, w1, eps = (_f(x) for x in _ce_w(entry))
    l0, l1 = logits[:, 0], logits[:, 1]
    one = _f(1)
    with np.errstate(all="ignore"):
        mx = np.maximum(l0, l1)
        if mutant == "row_max_not_subtracted":
            mx = np.zeros_like(mx)
        d0, d1 = l0 - mx, l1 - mx
        e0, e1 = np.exp(d0), np.exp(d1)
        S = e0 + e1
        ls = np.log(S)
        if mutant == "lse_rounded_at_the_common_magnitude":      # the kernels before this file existed
            lse = mx + ls
            n0, n1, p0, p1 = lse - l0, lse - l1, np.exp(l0 - lse), np.exp(l1 - lse)
        else:
            n0, n1, p0, p1 = ls - d0, ls - d1, e0 / S, e1 / S
        wy = np.where(y == 1, w1, w0).astype(np.float32)
        ny = np.where(y == 1, n1, n0)
        if entry is None:
            lr, W = ny, _f(B)
            k = one
            t2, t30, t31 = one, _f(0), _f(0)
        else:
            half = _f(0.5) * (eps if mutant != "smoothing_eps_not_halved" else _f(2) * eps)
            lr = (one - eps) * wy * ny + half * (w0 * n0 + w1 * n1)
            W = _f(B) if mutant == "ce_mean_over_B" else block_sum_f32(wy)
            k = (one - eps) * wy + half * (w0 + w1)
            t2 = (one - eps) * wy
            t30, t31 = half * w0, half * w1
            if mutant == "smoothing_missing_from_d_logits":
                t30, t31 = _f(0), _f(0)
        d = np.stack([(p0 * k - np.where(y == 0, t2, _f(0)) - t30) / W, (p1 * k - np.where(y == 1, t2, _f(0)) - t31) / W], 1).astype(np.float32)
        rows = (lr / W).astype(np.float32) if entry is not None else lr.astype(np.float32)
        loss = block_sum_f32(lr.astype(np.float32)) / W
    out = dict(loss_rows=rows, loss=np.array([loss]), d_logits=d)
    if entry is None:
        out["d_sum"] = d[:, 0].astype(np.float64) + d[:, 1].astype(np.float64)
    return out


def _ce_restate(case, inp, mutant=None):
    return ce_f32(inp["logits"], inp["labels"], case[2], mutant)


def ce_ref_bound(logits, y, entry):
    B = y.size
    w0, w1, eps = (_d(x) for x in _ce_w(entry))
    l = logits.astype(np.float64)
    if l.min() >= CE_SHIFT - 8:
        l = l - CE_SHIFT       # exact: the shifted rows ARE the unshifted rows + 1024, and softmax does not see the shift
    l0, l1 = l[:, 0], l[:, 1]
    mx = np.maximum(l0, l1)
    gap = np.abs(l0 - l1)
    d = np.stack([l0 - mx, l1 - mx], 1)
    e = np.exp(d)
    S = e.sum(1)
    ls = np.log(S)
    n = ls[:, None] - d                                   # -log p_c
    p = e / S[:, None]
    lose = d < 0
    rho_e = np.where(lose, 3 * U * gap[:, None] + HW_ULP, 0.0)
    d_e = e * rho_e + np.where(lose, TINY, 0.0)
    d_S = d_e.sum(1) + U * S
    d_ls = d_S / S + 2 * U * np.abs(ls)
    d_n = d_ls[:, None] + U * np.abs(d) + U * np.abs(n)
    d_p = p * (rho_e + (d_S / S)[:, None] + DIV) + TINY
    D = -(-B // 256) + 8
    yi = y.astype(int)
    r = np.arange(B)
    wy = np.where(yi == 1, w1, w0)
    onehot = np.stack([yi == 0, yi == 1], 1).astype(np.float64)
    wc = np.array([w0, w1])
    if entry is None:
        lr, d_lr, W, rho_W = n[r, yi], d_n[r, yi], float(B), 0.0
        k, d_k, T2, d_T2, T3, d_T3 = 1.0, 0.0, onehot, 0.0, np.zeros((B, 2)), 0.0
    else:
        A = (1 - eps) * wy * n[r, yi]
        Bq = 0.5 * eps * (w0 * n[:, 0] + w1 * n[:, 1])
        lr = A + Bq
        d_lr = (1 - eps) * wy * d_n[r, yi] + 3 * U * np.abs(A) + 0.5 * eps * (w0 * d_n[:, 0] + w1 * d_n[:, 1]) + 3 * U * np.abs(Bq) + U * np.abs(lr)
        W, rho_W = float(wy.sum()), D * U
        k = ((1 - eps) * wy + 0.5 * eps * (w0 + w1))[:, None]
        d_k = 5 * U * k
        T2 = onehot * ((1 - eps) * wy)[:, None]
        d_T2 = 2 * U * T2
        T3 = np.broadcast_to(0.5 * eps * wc, (B, 2))
        d_T3 = U * T3
    rows = lr / W if entry is not None else lr
    d_rows = d_lr / W + np.abs(rows) * (rho_W + DIV) if entry is not None else d_lr
    loss = lr.sum() / W
    d_loss = (d_lr.sum() + D * U * np.abs(lr).sum()) / W + abs(loss) * (rho_W + DIV)
    T1 = p * k
    num = T1 - T2 - T3
    d_num = d_p * k + p * d_k + U * T1 + d_T2 + d_T3 + 2 * U * (T1 + T2 + T3)
    dl = num / W
    d_dl = d_num / W + np.abs(dl) * (rho_W + DIV) + TINY
    out = dict(loss_rows=(rows, d_rows), loss=(np.array([loss]), np.array([d_loss])), d_logits=(dl, d_dl))
    if entry is None:
        out["d_sum"] = (np.zeros(B), d_dl.sum(1))
    return out


def _ce_reference(case, inp):
    return ce_ref_bound(inp["logits"], inp["labels"], case[2])


STEP_MUTANTS = ("bias_corrections_at_t_minus_1", "beta1_in_second_correction", "eps_inside_sqrt", "weight_decay_folded_into_gradient",
                "update_with_abs_grad_scale", "norm_without_grad_scale", "step_advanced_twice", "micro_not_reset")

OPS: Dict[str, Op] = {
    "accumulate": Op(_acc_cases(), _acc_make, _acc_reference, _acc_restate,
                     ("accumulate_adds_on_overwrite", "last_float4_skipped", "pair_second_skipped", "element_updated_twice")),
    "step_census": Op(_census_cases(), _census_make, _census_reference, _census_restate,
                      GRID_MUTANTS + ("finalize_first_256_partials", "finalize_reads_one_partial", "accumulate_adds_on_overwrite", "step_advanced_twice", "micro_not_reset")),
    "norm_select": Op([(n4,) for n4 in SELECT_SIZES], _select_make, _select_reference, _select_restate,
                      ("last_float4_skipped", "element_updated_twice", "finalize_first_256_partials", "norm_without_grad_scale")),
    "norm_clip": Op(_norm_cases(), _norm_make, _norm_reference, _norm_restate, ("norm_without_grad_scale", "clip_without_1e-6")),
    "adamw_zero_grad": Op(_zero_cases(), _zero_make, _zero_reference, _step_restate, ("weight_decay_folded_into_gradient",)),
    "adamw_rounded": Op(_adamw_cases(), _adamw_make, _adamw_reference, _step_restate, STEP_MUTANTS),
    "counters": Op([tuple(r) for r in COUNTER_RUNS], _counter_make, _counter_reference, _counter_restate,
                   ("step_advanced_twice", "micro_not_reset", "bias_corrections_at_t_minus_1", "beta1_in_second_correction")),
    "cross_entropy": Op(_ce_cases(), _ce_make, _ce_reference, _ce_restate, CE_MUTANTS),
}
EXACT_OPS = ("accumulate", "norm_select", "adamw_zero_grad")      # every output of every case has bound 0 (bc1 / bc2_sqrt aside)

# Mutants of the large cases run only where they are caught (the CPU suite's run time): mutant -> the n4 at which to look.
DESIGNATED = {
    ("step_census", "last_float4_skipped"): (1, 257, CAPS[1]),
    ("step_census", "pair_second_skipped"): (257, 513, CAPS[1]),
    ("step_census", "tail_sweep_dropped_at_cap"): (CAPS[1], CAPS[2], CAPS[3], CAPS[4]),
    ("step_census", "element_updated_twice"): (65, CAPS[0]),
    ("step_census", "finalize_first_256_partials"): (FINALIZE[2], FINALIZE[3]),
    ("step_census", "finalize_reads_one_partial"): (1025,),
    ("step_census", "accumulate_adds_on_overwrite"): (64,),
    ("step_census", "step_advanced_twice"): (63,),
    ("step_census", "micro_not_reset"): (63,),
    ("norm_select", "last_float4_skipped"): (1, 65),
    ("norm_select", "element_updated_twice"): (1,),
    ("norm_select", "finalize_first_256_partials"): (FINALIZE[2],),
    ("norm_select", "norm_without_grad_scale"): (1,),
}

# Why every size class is in the table: class -> (op, mutant, the class is the mutant's ONLY catcher among that op's cases).
CLASS_NEEDED_BY = {
    "one_block": ("step_census", "last_float4_skipped", False),             # the last float4 in a partly filled wave of a single block (63, 65, 255, 257); 257 holds the one-pair loop
    "adamw_block_step": ("step_census", "pair_second_skipped", False),      # 513: the first pair of a two-block grid (511 and 512 have none: asserted)
    "norm_block_step": ("step_census", "finalize_reads_one_partial", False),    # 1025: the first launch with two partials (1023 and 1024 have one: asserted)
    "finalize_stride": ("step_census", "finalize_first_256_partials", False),   # 257 and 1023 blocks: a thread of the finalize reads a second partial
    "caps": ("step_census", "tail_sweep_dropped_at_cap", True),             # the mutant acts wherever a third sweep has a tail; the grid formula gives one only at the cap
}


def designated_cases(op, mutant):
    cases = OPS[op].cases
    want = DESIGNATED.get((op, mutant))
    return cases if want is None else [c for c in cases if c[0] in want]


def is_large(op, case):
    return op in ("step_census", "norm_select", "norm_clip") and 4 * case[0] > LARGE_FLOATS


def check(op: str, case, inp, got: Dict[str, np.ndarray], refs=None) -> Dict[str, float]:
    """error / bound of every output of a case; refs = a reference(case, inp) computed earlier"""
    refs = OPS[op].reference(case, inp) if refs is None else refs
    assert set(refs) == set(got), (op, case, sorted(refs), sorted(got))
    out = {}
    for k in refs:
        ref, bound = refs[k]
        out[k] = worst_ratio(np.asarray(got[k], dtype=np.float64).reshape(np.shape(ref)), ref, bound)
    return out
