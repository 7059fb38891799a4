"""Case lists of tests/test_gpu_encoder_bwd_ops.py, shared with tests/test_encoder_bwd_coverage.py (tests only).

The op-level tests of the trainable-encoder backward are only worth their run time if their shapes reach the code paths of the
real step: the split-K weight gradient at 2 and 4 slices and with a ragged last slice, the LayerNorm backward's partials at 1 and
at the 256-block cap, attention in its 2-wave form and over several query / key blocks.  Those paths are chosen by the library
(wgrad_cfg / wgrad_slices, ln_bwd_blocks, QB and nob), so the CPU coverage test reads them back through host-only queries and
fails when a policy change moves the cases off them.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple


class WgradCase(NamedTuple):
    M: int                 # tokens
    N: int                 # out_features (dY columns)
    K: int                 # in_features (X columns)
    strided: bool = False  # lddy > N, ldx > K, ldt > Mp


# the real step: bench.py defaults (B = 32, L = 128: 4,096 text tokens; one frame: 32 x 50 = 1,600 ViT tokens) x the four Linears
_REAL = [WgradCase(m, n, k) for m in (4096, 1600) for (n, k) in ((2304, 768), (768, 768), (3072, 768), (768, 3072))]
WGRAD_CASES = _REAL + [
    WgradCase(16384, 2304, 768),          # L = 512 (configs[3]) Q/K/V
    WgradCase(4097, 768, 768),            # one token past the real text step: a 1-token last K-step
    WgradCase(1599, 768, 768),            # one short of the ViT step
    WgradCase(65, 2304, 768),             # two K-steps, the second with one token
    WgradCase(1, 768, 768),               # a single token
    WgradCase(1600, 2304, 768, True),     # strided operands, as the encoders pass them
    WgradCase(4097, 768, 3072, True),
    WgradCase(1600, 40, 768),             # 8 <= N < 64: the workspace query must size it (it returned 0)
]

PARTIALS_NBLK = (1, 15, 16, 17, 64, 255, 256)
PARTIALS_H = (16, 40, 768)

# LayerNorm backward rows (block count 1 .. 256: ufnd_layernorm_bwd_blocks) and the row stride (50 H: the ViT's CLS rows)
LN_H = 768
LN_CASES = [(m, LN_H) for m in (1, 37, 1600, 2040, 2041, 4096, 16384)] + [(37, 50 * LN_H), (300, 50 * LN_H)]

HIDDEN_M = (1, 37, 1600, 4096, 4097)

# attention: the 2-wave form (L <= 64), one and several 128-query blocks forward, one and several 128-key blocks backward
ATTN_LENGTHS = (1, 2, 50, 63, 64, 65, 77, 128, 129, 200, 256, 512)
ATTN_P = (0.1, 0.5)
ATTN_QB = 128                             # queries per forward workgroup (csrc/attention.hip QB)
ATTN_KB = 128                             # keys per backward workgroup (csrc/attention_bwd.hip nob)


def pad64(m: int) -> int:
    return (m + 63) // 64 * 64


def wgrad_id(c: WgradCase) -> str:
    return f"M{c.M}_N{c.N}_K{c.K}" + ("_strided" if c.strided else "")


def wgrad_slices(lib, c: WgradCase) -> Tuple[int, int, int]:
    """(S, per, nk): the slice count the library sizes the slab workspace for, K-steps per slice, 64-token K-steps in all.
    Slice s owns K-steps [s per, min((s + 1) per, nk)) -- the split of wgrad_slices (every slice at least one K-step)."""
    mp = pad64(c.M)
    floats = lib.ufnd_gemm_bf16_wgrad_workspace_floats(c.N, c.K, mp)
    assert floats > 0 and floats % (c.N * c.K) == 0, (c, floats)
    S = floats // (c.N * c.K)
    nk = mp // 64
    per = (nk + S - 1) // S
    assert (nk + per - 1) // per == S, (c, S, per, nk)
    return S, per, nk
