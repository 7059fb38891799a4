"""GPU: tile 2 (256x128, 8 waves as 4x2, A and W rings 3 slots deep) at the shapes and epilogues of the packed text pass's N = 768
residual GEMMs -- BertTextEncoder.text_narrow_tile names it for the out-projection and FFN2 -- through ufnd_gemm_bf16_ex /
ufnd_gemm_bf16_ln and their live-row entries with an explicit tile.

  - a row does not depend on the tile that computed it: outputs and row statistics are bit for bit those of tile 22 (256x192, the
    library's choice for these shapes at the capacity) at N = 768 and of tile 16 (128x128, the only other forward production tile
    whose width divides 128) at N = 128;
  - both tiles stay inside the float64 reference's bounds of tests/gemm_bf16_cases.py (the bounds its table applies to tile 22: derived
    there, none from a GPU result), on inputs with NaN pads and outputs filled with sentinels (G.check: a damaged sentinel is inf);
  - the live-row entries at capacity 512: live rows equal the capacity-sized launch bit for bit, rows at or past the count keep the
    sentinel, operand rows past it (NaN here) reach nothing;
  - every launch runs twice and must give equal bits.

K = 64 is a K loop with no refill, K = 192 a ring that wraps once, K = 768 the out-projection's."""
import numpy as np
import pytest

from tests import gemm_bf16_cases as G
from tests.test_gpu_gemm_bf16 import launch

pytestmark = pytest.mark.gpu

TILE = 2
PARTNER = {768: 22, 128: 16}
MS = (1, 255, 256, 257, 512)
NS = (128, 768)
KS = (64, 192, 768)
CAPACITY = 512
COUNTS = (0, 1, 255, 256, 257, 512)
EPILOGUES = ("plain", "bias", "fold-gelu", "res-stats", "rln-stats")


def case(epi: str, tile: int, M: int, N: int, K: int) -> G.Case:
    if epi == "plain":
        return G._mk("ex", tile, M, N, K, "rounded", bias=False)
    if epi == "bias":
        return G._mk("ex", tile, M, N, K, "rounded")
    if epi == "fold-gelu":      # (partials of the K columns: the production count K / 32 where it is even)
        return G._mk("ln", tile, M, N, K, "rounded", ln="fold", act=G.ACT_GELU, parts=K // 32, guard="yes")
    if epi == "res-stats":
        return G._mk("ln", tile, M, N, K, "rounded", ln="plain", res="bf16", outs="bf16", out_stats=True)
    assert epi == "rln-stats"
    return G._mk("ln", tile, M, N, K, "rounded", ln="rln", parts=N // 32, res="bf16", outs="bf16", out_stats=True)


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a: dict, b: dict, names=("of", "ob", "ostats")) -> list:
    """the outputs among `names` whose whole buffers (sentinels included) differ"""
    return [n for n in names if n in a and not np.array_equal(_bits(a[n]), _bits(b[n]))]


def _twice(c: G.Case, inp: dict, m_live=None) -> dict:
    rc, err, got = launch(c, inp, m_live)
    assert rc == 0, (c.id, m_live, err)
    rc, err, again = launch(c, inp, m_live)
    assert rc == 0, (c.id, m_live, err)
    assert not _same(got, again, ("of", "ob", "ostats", "guard")), (c.id, m_live, "two runs differ", _same(got, again, ("of", "ob", "ostats", "guard")))
    return got


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_tile_2_equals_its_partner_and_float64(epi, N, K):
    other = PARTNER[N]
    for M in MS:
        c = case(epi, TILE, M, N, K)
        co = c._replace(tile=other, want=other)      # (the same inputs: they are drawn from c's id)
        inp = G.make(c)
        refs = G.reference(c, inp)
        got, goto = _twice(c, inp), _twice(co, inp)
        assert not _same(got, goto), (c.id, f"tile {TILE} and tile {other} differ", _same(got, goto))
        for cc, g in ((c, got), (co, goto)):
            ratios = G.check(cc, inp, g, refs)
            worst = max(ratios, key=lambda k: ratios[k])
            print(f"{cc.id} tile {cc.tile}: worst error / bound {ratios[worst]:.3g} ({worst})")
            assert ratios[worst] <= 1.0, (cc.id, cc.tile, ratios)


def _poisoned(c: G.Case, inp: dict, T: int) -> dict:
    """inp with NaN in every operand row at or past T"""
    out = dict(inp)
    for name, nan in (("A", G.NAN_BF16), ("resb", G.NAN_BF16), ("res", np.float32(np.nan)), ("a_stats", np.float32(np.nan)),
                      ("r_stats", np.float32(np.nan))):
        if name in inp:
            out[name] = inp[name].copy()
            out[name][T:] = nan
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("epi", EPILOGUES)
def test_tile_2_live_rows(epi, N, K):
    c = case(epi, TILE, CAPACITY, N, K)
    inp = G.make(c)
    full = _twice(c, inp)
    assert max(G.check(c, inp, full).values()) <= 1.0, c.id
    for T in COUNTS:
        got = _twice(c, _poisoned(c, inp, T), m_live=T)
        for n in ("of", "ob", "ostats"):
            if n not in got:
                continue
            want = inp[n].copy()                       # the sentinels ...
            want[G.PRE:G.PRE + T] = full[n][G.PRE:G.PRE + T]      # ... and the capacity-sized launch's live rows (pad columns: sentinels in both)
            assert np.array_equal(_bits(got[n]), _bits(want)), (c.id, n, "m_live", T, "live rows differ or dead rows written")
        if "guard" in got:      # the dead rows' statistics are NaN: a workgroup that read one reports +inf
            assert np.isfinite(got["guard"]).all() and got["guard"].max() <= full["guard"].max(), (c.id, "guard", T)
            assert (got["guard"].max() > 0) == (T > 0), (c.id, "guard", T)
