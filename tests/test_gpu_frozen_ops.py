"""The frozen encoders' non-GEMM kernels, op by op through the C ABI, against the float64 references and derived bounds of
tests/frozen_ops_cases.py (the cases, the derivations and the CPU evidence that the bounds can tell a wrong kernel from a
rounded one are there and in tests/test_frozen_ops_cases.py).

Every output buffer is filled with a sentinel and is two rows (or eight elements) longer than the kernel may write: an
unwritten element fails the comparison, an overwritten tail fails in `back`.  Each test prints its worst
error / bound; tools/frozen_ops_errors.py collects them into profiles/frozen_ops_errors.txt.

ufnd_act_bf16: the acceptance 2^-8 |ref| + 1e-6 is absolute in the far negative tail ON PURPOSE.  At x = -5.5 the exact GELU is
-1.0e-7 and the kernel's polynomial (|erf error| <= 1.5e-7, times |x| / 2) is off by up to 4e-7 before the rounding: hundreds of
bf16 ulps of a number that small, 2e-7 in absolute terms, invisible in anything the result is added to.  Do not turn the
absolute term into a relative one.
"""
import numpy as np
import pytest
import torch

from tests import frozen_ops_cases as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 2          # sentinel rows behind every output
_SENT16 = np.array([F.SENTINEL_BF16], dtype=np.uint16).view(np.int16)[0]


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


def _s():
    return _lib().stream_ptr(torch.device(DEV))


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def out_f32(rows, cols):
    return torch.full((rows + TAIL, cols), F.SENTINEL_F32, dtype=torch.float32, device=DEV)


def out_bf16(rows, cols):
    return torch.full((rows + TAIL, cols), int(_SENT16), dtype=torch.int16, device=DEV)


def back(t, rows):
    """the first `rows` rows of an output (bf16 as float32 values); the sentinel rows behind them must be untouched"""
    a = t.cpu().numpy()
    tail = a[rows:]
    if a.dtype == np.int16:
        assert (tail.view(np.uint16) == F.SENTINEL_BF16).all(), "wrote behind its output"
        return F.bf16_f32(a[:rows].view(np.uint16))
    assert (tail == np.float32(F.SENTINEL_F32)).all(), "wrote behind its output"
    return a[:rows]


def _ok(rc, what):
    _lib().check(rc, what)


# ---------------------------------------------------------------------------------------------------------------------
# one launch per case: inputs of tests/frozen_ops_cases.py -> {output name: array}
def run_layernorm(case, inp):
    H, M, ldx, kind, eps, _ = case
    L = _lib()
    x, g, b = dev(inp["x"]), dev(inp["gamma"]), dev(inp["beta"])
    of = out_f32(M, H) if kind in ("both", "f32") else None
    ob = out_bf16(M, H) if kind in ("both", "bf16") else None
    _ok(L.lib().ufnd_layernorm(x.data_ptr(), ldx, g.data_ptr(), b.data_ptr(), L.ptr(ob), L.ptr(of), M, H, eps, _s()), "ufnd_layernorm")
    return {k: back(t, M) for k, t in (("of", of), ("ob", ob)) if t is not None}


def run_bert_embed(case, inp):
    H, B, Lq, form, out = case
    L = _lib()
    t = {k: dev(inp[k]) for k in ("ids", "word", "pos", "type0", "gamma", "beta")}
    M = B * Lq
    of = out_f32(M, H) if out == "f32" else None
    ob = out_bf16(M, H) if out == "bf16" else None
    ln = form == "ln"
    _ok(L.lib().ufnd_bert_embed(t["ids"].data_ptr(), t["word"].data_ptr(), t["pos"].data_ptr(), t["type0"].data_ptr(),
                                t["gamma"].data_ptr() if ln else None, t["beta"].data_ptr() if ln else None, L.ptr(ob), L.ptr(of), B, Lq, H,
                                F.EMB_VOCAB, inp["eps"], _s()), "ufnd_bert_embed")
    return {k: back(v, M) for k, v in (("of", of), ("ob", ob)) if v is not None}


def run_vit_assemble(case, inp):
    H, N, P, variant = case
    L = _lib()
    t = {k: dev(inp[k]) for k in ("pe", "cls", "pos", "gamma", "beta")}
    M = N * (P + 1)
    of = out_f32(M, H) if variant != "ln_bf16" else None
    ob = out_bf16(M, H) if variant == "ln_bf16" else None
    st = out_f32(M, 4) if variant == "ln_stats" else None
    ln = variant != "raw"
    _ok(L.lib().ufnd_vit_assemble(t["pe"].data_ptr(), t["cls"].data_ptr(), t["pos"].data_ptr(), t["gamma"].data_ptr() if ln else None,
                                  t["beta"].data_ptr() if ln else None, L.ptr(of), L.ptr(ob), L.ptr(st), N, P, H, inp["eps"], _s()), "ufnd_vit_assemble")
    got = {k: back(v, M) for k, v in (("of", of), ("ob", ob), ("stats", st)) if v is not None}
    if st is not None:
        assert (got["stats"][:, 2:] == 0).all() and not np.signbit(got["stats"][:, 2:]).any()      # the two zeros are +0 exactly
    return got


def run_vit_patchify(case, inp):
    image, patch, N = case
    L = _lib()
    G = image // patch
    fr = dev(inp["frames"])
    o = out_bf16(N * G * G, 3 * patch * patch)
    _ok(L.lib().ufnd_vit_patchify(fr.data_ptr(), o.data_ptr(), N, image, patch, _s()), "ufnd_vit_patchify")
    return {"patches": back(o, N * G * G)}


def run_masked_meanpool_l2(case, inp):
    H, Lq = case
    L = _lib()
    B = inp["mask"].shape[0]
    h, m = dev(inp["hidden"]), dev(inp["mask"])
    o = out_f32(B, H)
    _ok(L.lib().ufnd_masked_meanpool_l2(h.data_ptr(), m.data_ptr(), o.data_ptr(), B, Lq, H, _s()), "ufnd_masked_meanpool_l2")
    return {"out": back(o, B)}


def run_l2norm_frames(case, inp):
    B, Fr, D = case
    L = _lib()
    e = dev(inp["e"])
    o = out_f32(B, D)
    _ok(L.lib().ufnd_l2norm_frames(e.data_ptr(), o.data_ptr(), B, Fr, D, _s()), "ufnd_l2norm_frames")
    return {"out": back(o, B)}


def run_field_mean_l2(case, inp):
    N, Mx, D = case
    L = _lib()
    p, v = dev(inp["parts"]), dev(inp["valid"])
    o = out_f32(N, D)
    _ok(L.lib().ufnd_field_mean_l2(p.data_ptr(), v.data_ptr(), o.data_ptr(), N, Mx, D, _s()), "ufnd_field_mean_l2")
    return {"out": back(o, N)}


def run_cast_bf16(n, inp):
    L = _lib()
    x = dev(inp["x"])
    o = torch.full((n + 8,), int(_SENT16), dtype=torch.int16, device=DEV)
    _ok(L.lib().ufnd_cast_bf16(x.data_ptr(), o.data_ptr(), n, _s()), "ufnd_cast_bf16")
    bits = o.cpu().numpy().view(np.uint16)
    assert (bits[n:] == F.SENTINEL_BF16).all(), "wrote behind its output"
    want = F.bf16_bits(inp["x"])
    nan = np.isnan(inp["x"])
    assert np.array_equal(bits[:n][~nan], want[~nan]), "bits differ (the sign of zero included)"
    return {"out": F.bf16_f32(bits[:n])}


def run_act_bf16(case, inp):
    act, n = case
    L = _lib()
    x = dev(inp["x"])
    o = torch.full((n + 8,), int(_SENT16), dtype=torch.int16, device=DEV)
    _ok(L.lib().ufnd_act_bf16(x.data_ptr(), o.data_ptr(), n, act, _s()), "ufnd_act_bf16")
    bits = o.cpu().numpy().view(np.uint16)
    assert (bits[n:] == F.SENTINEL_BF16).all(), "wrote behind its output"
    return {"out": F.bf16_f32(bits[:n])}


def run_gather_rows(case, inp):
    L = _lib()
    B = len(F.GATHER_IDX)
    idx = dev(inp["idx"])
    src = [dev(s) for s in inp["src"]]
    dst = [torch.full((B + TAIL, s.shape[1]), 0xA5, dtype=torch.uint8, device=DEV) for s in src]
    items = (L.GatherItem * len(src))(*[L.GatherItem(s.data_ptr(), d.data_ptr(), s.shape[1], s.shape[0]) for s, d in zip(src, dst)])
    assert len(src) == F.GATHER_MAX_ITEMS
    _ok(L.lib().ufnd_gather_rows(idx.data_ptr(), B, items, len(src), _s()), "ufnd_gather_rows")
    got = {}
    for i, d in enumerate(dst):
        a = d.cpu().numpy()
        assert (a[B:] == 0xA5).all(), f"item {i}: wrote behind its {B} rows"
        got[f"dst{i}"] = a[:B]
    return got


def run_attention(case, inp):
    B, Lq, heads, _ = case
    L = _lib()
    qkv = dev(inp["qkv"])
    mask = None if inp["mask"] is None else dev(inp["mask"])
    ctx = out_bf16(B * Lq, heads * 64)
    _ok(L.lib().ufnd_attention_bf16(qkv.data_ptr(), L.ptr(mask), ctx.data_ptr(), B, Lq, heads, _s()), "ufnd_attention_bf16")
    return {"ctx": back(ctx, B * Lq)}


RUN = {"layernorm": run_layernorm, "bert_embed": run_bert_embed, "vit_assemble": run_vit_assemble, "vit_patchify": run_vit_patchify,
       "masked_meanpool_l2": run_masked_meanpool_l2, "l2norm_frames": run_l2norm_frames, "field_mean_l2": run_field_mean_l2,
       "cast_bf16": run_cast_bf16, "act_bf16": run_act_bf16, "gather_rows": run_gather_rows, "attention_select": run_attention,
       "attention_census": run_attention, "attention_general": run_attention}
assert set(RUN) == set(F.OPS)


def worst_of(op, cases=None):
    """(worst error / bound, case, output) of an op's kernel over its cases"""
    worst = (-1.0, None, None)
    for case in (F.OPS[op].cases if cases is None else cases):
        inp = F.OPS[op].make(case)
        got = RUN[op](case, inp)
        for k, r in F.check(op, case, inp, got).items():
            if r > worst[0]:
                worst = (r, case, k)
    return worst


ATTN_OPS = ("attention_select", "attention_census", "attention_general")
PARAMS = [(op, None) for op in sorted(F.OPS) if op not in ATTN_OPS] + [(op, g) for op in ATTN_OPS for g in F.ATTN_GRID]


@pytest.mark.parametrize("op,grid", PARAMS, ids=[op if g is None else f"{op}-{F.case_id(g)}" for op, g in PARAMS])
def test_kernel_against_float64(op, grid):
    cases = None if grid is None else [c for c in F.OPS[op].cases if c[:3] == grid]
    r, case, key = worst_of(op, cases)
    print(f"{op}: worst error / bound {r:.3g} at {case} ({key})")
    assert r <= 1.0, (op, r, case, key)


# ---------------------------------------------------------------------------------------------------------------------
def _rejected(rc, word):
    msg = _lib().lib().ufnd_last_error()
    assert rc == 1 and msg and word in msg, (rc, msg, word)


def test_entries_reject_what_their_kernels_cannot_do():
    """Host-side rejections (nothing is launched): an output 4 bytes off its 16-B (fp32) / 8-B (bf16) alignment, H = 384, D = 1025,
    patch = 12, act = 0."""
    L = _lib()
    lib, s = L.lib(), _s()
    H, M = 256, 4
    x, g, b = torch.zeros(M, H, device=DEV), torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    x384, g384 = torch.zeros(M, 384, device=DEV), torch.ones(384, device=DEV)
    of, ob = out_f32(M, 512), out_bf16(M, 512)
    ids, src, live = torch.zeros(M, dtype=torch.int64, device=DEV), torch.arange(M, dtype=torch.int32, device=DEV), torch.full((1,), M, dtype=torch.int32, device=DEV)
    word, pos = torch.zeros(8, 384, device=DEV), torch.zeros(M, 384, device=DEV)
    X, G, Bt, I, S, Lv, W, P_ = (t.data_ptr() for t in (x, g, b, ids, src, live, word, pos))
    for o_f, o_b in ((of.data_ptr() + 4, None), (None, ob.data_ptr() + 4), (of.data_ptr(), ob.data_ptr() + 4), (of.data_ptr() + 4, ob.data_ptr())):
        _rejected(lib.ufnd_layernorm(X, H, G, Bt, o_b, o_f, M, H, 1e-5, s), b"layernorm: alignment")
        _rejected(lib.ufnd_layernorm_live(X, H, G, Bt, o_b, o_f, M, H, 1e-5, Lv, s), b"layernorm_live: alignment")
        _rejected(lib.ufnd_bert_embed(I, W, P_, G, G, Bt, o_b, o_f, 1, M, H, 8, 1e-5, s), b"bert_embed: alignment")
        _rejected(lib.ufnd_bert_embed_live(I, S, Lv, W, P_, G, G, Bt, o_b, o_f, M, M, H, 8, 1e-5, s), b"bert_embed_live: alignment")
        _rejected(lib.ufnd_vit_assemble(X, G, P_, G, Bt, o_f, o_b, None, 1, M - 1, H, 1e-5, s), b"vit_assemble: alignment")
    O, Ob = of.data_ptr(), ob.data_ptr()
    X3, G3 = x384.data_ptr(), g384.data_ptr()
    _rejected(lib.ufnd_layernorm(X3, 384, G3, G3, Ob, O, M, 384, 1e-5, s), b"H=384")
    _rejected(lib.ufnd_layernorm_live(X3, 384, G3, G3, Ob, O, M, 384, 1e-5, Lv, s), b"H=384")
    _rejected(lib.ufnd_bert_embed(I, W, P_, G3, G3, G3, Ob, O, 1, M, 384, 8, 1e-5, s), b"H=384")
    _rejected(lib.ufnd_bert_embed_live(I, S, Lv, W, P_, G3, G3, G3, Ob, O, M, M, 384, 8, 1e-5, s), b"H=384")
    _rejected(lib.ufnd_vit_assemble(X3, G3, P_, G3, G3, O, Ob, None, 1, M - 1, 384, 1e-5, s), b"H=384")
    e = torch.zeros(2 * 1025, device=DEV)
    valid = torch.ones(2, dtype=torch.int32, device=DEV)
    _rejected(lib.ufnd_l2norm_frames(e.data_ptr(), O, 1, 2, 1025, s), b"D=1025")
    _rejected(lib.ufnd_field_mean_l2(e.data_ptr(), valid.data_ptr(), O, 1, 2, 1025, s), b"D=1025")
    fr = torch.zeros(3 * 48 * 48, device=DEV)
    _rejected(lib.ufnd_vit_patchify(fr.data_ptr(), Ob, 1, 48, 12, s), b"patch=12")
    _rejected(lib.ufnd_act_bf16(Ob, Ob, 8, 0, s), b"act=0")
    torch.cuda.synchronize()
    assert (of.cpu().numpy() == np.float32(F.SENTINEL_F32)).all() and (ob.cpu().numpy() == _SENT16).all()      # nothing was launched
