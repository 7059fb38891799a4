"""CPU: the case lists of tests/test_gpu_encoder_bwd_ops.py (tests/encoder_bwd_cases.py) still reach the code paths they are there
for, read from the library's host-only queries.  A change of the slice policy, the LayerNorm block count or the attention block
sizes that moves the cases off those paths fails here, and the cases have to be chosen again."""
from tests import encoder_bwd_cases as C


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def test_weight_gradient_cases_reach_every_slice_count_and_a_ragged_last_slice():
    lib = _lib()
    seen, ragged = set(), []
    for c in C.WGRAD_CASES:
        S, per, nk = C.wgrad_slices(lib, c)
        seen.add(S)
        if S > 1 and nk % per:
            ragged.append((C.wgrad_id(c), S, per, nk - (S - 1) * per))
    print(f"slice counts {sorted(seen)}; ragged last slices {ragged}")
    assert {1, 2, 4} <= seen, seen
    assert ragged, "no case splits the tokens into slices of unequal length"
    # the real ViT step (1,600 tokens): 25 K-steps in two slices of 13 and 12
    assert C.wgrad_slices(lib, C.WgradCase(1600, 768, 768)) == (2, 13, 25)


def test_workspace_query_sizes_every_width_linear_wgrad_accepts():
    lib = _lib()
    for n in (8, 16, 40, 56, 64, 72):
        for k, mp in ((64, 64), (768, 1600 // 64 * 64 + 64), (768, 16384)):
            f = lib.ufnd_gemm_bf16_wgrad_workspace_floats(n, k, mp)
            assert f > 0 and f % (n * k) == 0, (n, k, mp, f)
    assert lib.ufnd_gemm_bf16_wgrad_workspace_floats(64, 768, 100) == 0       # tokens not padded to 64: not a shape the entries take
    assert lib.ufnd_gemm_bf16_wgrad_workspace_floats(64, 700, 128) == 0       # K_in not a multiple of 64


def test_layernorm_cases_reach_one_block_and_the_block_cap():
    lib = _lib()
    blocks = {lib.ufnd_layernorm_bwd_blocks(m) for m, _ in C.LN_CASES}
    assert {1, 255, 256} <= blocks, blocks
    assert lib.ufnd_layernorm_bwd_blocks(2040) == 255 and lib.ufnd_layernorm_bwd_blocks(2041) == 256
    assert lib.ufnd_layernorm_bwd_blocks(16384) == 256
    for m, _ in C.LN_CASES:
        assert lib.ufnd_layernorm_bwd_workspace_floats(m, C.LN_H) == lib.ufnd_layernorm_bwd_blocks(m) * 2 * C.LN_H
    assert any(ld > h for _, ld in C.LN_CASES for h in (C.LN_H,))


def test_partials_cases_cross_the_sixteen_row_groups():
    assert {1, 15, 16, 17, 256} <= set(C.PARTIALS_NBLK)
    assert any(h % 16 for h in C.PARTIALS_H) and min(C.PARTIALS_H) == 16


def test_attention_lengths_cross_every_kernel_form():
    Ls = C.ATTN_LENGTHS
    assert any(l <= 64 for l in Ls) and any(64 < l <= C.ATTN_QB for l in Ls)          # the 2-wave form; one 4-wave query block
    assert any(l > C.ATTN_QB for l in Ls) and any(l > 2 * C.ATTN_KB for l in Ls)     # several query blocks; several key blocks
    assert any(l % 4 for l in Ls) and any(l % 64 == 1 for l in Ls)                  # Lp != L (mask rows padded to 4); a 1-row tail
    assert max(Ls) == 512 and 256 in Ls
