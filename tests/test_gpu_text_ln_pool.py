"""ufnd_ln_masked_meanpool_l2_live -- the packed text pass's final LayerNorm and masked mean-pool in one kernel -- against the two
launches it replaces, ufnd_layernorm_live into an fp32 buffer and ufnd_masked_meanpool_l2_live over it: the pooled, L2-normalised
rows bit for bit at H = 768.  Samples of 0 (fully masked), 1, 4, 5, 33 and L rows -- below, at and past the four token groups and
the eight rows a group has in flight -- in every position of the batch, a mask with holes, and NaN in every row past the live
count, which neither form may read."""
import itertools

import pytest
import torch

DEV = "cuda"
gpu = pytest.mark.gpu
H, EPS = 768, 1e-12


def _run_both(lens, L_, holes=False):
    from ultrafnd_git_amd import _lib as L
    lib, B = L.lib(), len(lens)
    g = torch.Generator().manual_seed(100 * L_ + sum((i + 1) * n for i, n in enumerate(lens)) + holes)
    mask = torch.zeros(B, L_, dtype=torch.int32)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
        if holes and n > 2:      # holes stay rows of the packed pass (the last kept position bounds the sample), masked in the pool
            mask[b, 1:n - 1] = (torch.rand(n - 2, generator=g) < 0.6).int()
    live = int(sum(lens))
    y = torch.full((B * L_, H), float("nan"))
    y[:live] = torch.randn(live, H, generator=g) * 1.7 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    y, mask, gamma, beta = y.to(DEV), mask.to(DEV), gamma.to(DEV), beta.to(DEV)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    row_src = torch.zeros(B * L_, dtype=torch.int32, device=DEV)
    s = L.stream_ptr(y.device)
    L.check(lib.ufnd_text_pack(mask.data_ptr(), B, L_, cu.data_ptr(), row_src.data_ptr(), s), "ufnd_text_pack")
    assert cu.tolist() == [0] + list(itertools.accumulate(lens))
    xf = torch.full((B * L_, H), float("nan"), device=DEV)
    want = torch.full((B, H), float("nan"), device=DEV)
    got = torch.full((B, H), float("nan"), device=DEV)
    L.check(lib.ufnd_layernorm_live(y.data_ptr(), H, gamma.data_ptr(), beta.data_ptr(), None, xf.data_ptr(), B * L_, H, EPS,
                                    cu.data_ptr() + 4 * B, s), "ufnd_layernorm_live")
    L.check(lib.ufnd_masked_meanpool_l2_live(xf.data_ptr(), mask.data_ptr(), cu.data_ptr(), want.data_ptr(), B, L_, H, s),
            "ufnd_masked_meanpool_l2_live")
    L.check(lib.ufnd_ln_masked_meanpool_l2_live(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), EPS, mask.data_ptr(), cu.data_ptr(),
                                                got.data_ptr(), B, L_, H, s), "ufnd_ln_masked_meanpool_l2_live")
    torch.cuda.synchronize()
    assert torch.isfinite(want).all(), lens
    for b, n in enumerate(lens):      # (a fully masked sample pools to zeros; any other to a unit row)
        assert abs(float(want[b].norm()) - (1.0 if n else 0.0)) < 1e-5, (lens, b)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (lens, L_, holes)


@gpu
@pytest.mark.parametrize("L_", [8, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_fused_ln_pool_equals_the_two_launches(B, L_):
    lengths = [n for n in (0, 1, 4, 5, 33, L_) if n <= L_]
    for k in range(len(lengths)):      # every length in every position of the batch
        lens = [lengths[(k + 2 * i) % len(lengths)] for i in range(B)]
        _run_both(lens, L_)
    _run_both([L_] * B, L_, holes=True)
    _run_both([lengths[-2]] + [L_] * (B - 1), L_, holes=True)


def test_refusals():
    """Argument checks (no launch, so no GPU)."""
    from ultrafnd_git_amd import _lib as L
    f = L.lib().ufnd_ln_masked_meanpool_l2_live
    buf = torch.zeros(4096, dtype=torch.float32)
    p = buf.data_ptr()
    assert p % 16 == 0
    assert f(None, p, p, EPS, p, p, p, 1, 8, H, None) == 1 and b"null argument" in L.lib().ufnd_last_error()
    assert f(p, p, p, EPS, p, p, p, 1, 8, 640, None) == 1 and b"H=640" in L.lib().ufnd_last_error()
    assert f(p + 4, p, p, EPS, p, p, p, 1, 8, H, None) == 1 and b"alignment" in L.lib().ufnd_last_error()
