"""The audio encoder's own kernels, op by op through the C ABI, against the float64 references and derived per-element bounds of
tests/audio_ops_cases.py and tests/conv_rows_cases.py (the cases, the derivations and the CPU evidence that the bounds tell a wrong
kernel from a rounded one are there and in tests/test_audio_ops_cases.py / tests/test_conv_rows_cases.py).

ufnd_conv1d_rows_bf16: every case of the table; the exact family must be bit-equal.  ufnd_w2v2_frames, ufnd_w2v2_pos_pack and
ufnd_w2v2_pos_add: bit equality of whole buffers.  ufnd_wave_normalize and ufnd_w2v2_conv0: per element, on smooth clips, clicks at
and beside a chunk's first value, a DC-heavy and a constant clip; a clip alone equals its row of a ragged batch bit for bit.  Every
output is filled with a sentinel and is longer than the kernel may write.  Each test prints its worst error / bound;
tools/audio_ops_errors.py collects them into profiles/audio_ops_errors.txt."""
import numpy as np
import pytest
import torch

from tests import audio_ops_cases as A
from tests import conv_rows_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
_SENT16 = int(np.array([A.SENT_BF16], dtype=np.uint16).view(np.int16)[0])


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


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def filled(shape, dtype):
    sent = {torch.float32: float(A.SENT_F32), torch.int16: _SENT16, torch.int32: int(A.SENT_I32)}[dtype]
    return torch.full(shape, sent, dtype=dtype, device=DEV)


def _ok(rc, what):
    _lib().check(rc, what)


def _sentinel(a):
    return {np.dtype(np.float32): A.SENT_F32, np.dtype(np.uint16): A.SENT_BF16, np.dtype(np.int32): A.SENT_I32}[a.dtype]


def untouched(a) -> bool:
    return bool((a == _sentinel(a)).all())


# ---------------------------------------------------------------------------------------------------------------------
# ufnd_conv1d_rows_bf16
def launch_conv_rows(c: R.Case, inp: dict) -> dict:
    L = _lib()
    t = {k: dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}

    def p(name, ld=0):
        return None if name not in t else t[name].data_ptr() + inp["pre"].get(name, 0) * ld * t[name].element_size()
    _ok(L.lib().ufnd_conv1d_rows_bf16(p("A"), p("W"), p("bias"), p("ob", c.ldo), p("of", c.ldf), c.M, c.N, c.K, c.lda, c.ldw, c.ldo, c.ldf, c.act,
                                      _s()), "ufnd_conv1d_rows_bf16")
    torch.cuda.synchronize()
    return {k: host(t[k]) for k in ("of", "ob") if k in t}


def measure_conv_rows(c: R.Case):
    """(worst error / bound, the output it is on, unequal elements or None outside the exact family)"""
    inp = R.make(c)
    refs = R.reference(c, inp)
    got = launch_conv_rows(c, inp)
    ratios = R.check(c, inp, got, refs)
    key = max(ratios, key=lambda k: ratios[k])
    return ratios[key], key, (R.unequal(c, got, refs) if R.is_bit_exact(c) else None)


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_conv1d_rows_against_float64(case):
    r, key, ne = measure_conv_rows(case)
    print(f"conv1d_rows {case.id}: worst error / bound {r:.3g} ({key})" + ("" if ne is None else f"; unequal elements {ne}") + f"   [{case.edge}]")
    assert r <= 1.0, (case.id, r, key)
    assert ne in (None, 0), (case.id, ne)


# ---------------------------------------------------------------------------------------------------------------------
# one launch per case: inputs of tests/audio_ops_cases.py -> {output name: array}
def run_frames(case, inp):
    L = _lib()
    S, B = case[1], inp["lengths"].size
    n = dev(inp["lengths"])
    fr, km = filled((B + 8,), torch.int32), filled((B * S + 8,), torch.int32)
    _ok(L.lib().ufnd_w2v2_frames(n.data_ptr(), fr.data_ptr(), km.data_ptr(), B, S, _s()), "ufnd_w2v2_frames")
    fr, km = host(fr), host(km)
    assert untouched(fr[B:]) and untouched(km[B * S:]), "wrote behind its output"
    return {"frames": fr[:B], "key_mask": km[:B * S].reshape(B, S)}


def run_pos_pack(case, inp):
    L = _lib()
    B, S, _ = case
    Mp = B * (S + A.POS_K) + A.POS_K
    x, fr = dev(inp["x"]), dev(inp["frames"])
    packed = filled((A.POS_G * Mp * A.POS_C + 64,), torch.int16)
    _ok(L.lib().ufnd_w2v2_pos_pack(x.data_ptr(), fr.data_ptr(), packed.data_ptr(), B, S, _s()), "ufnd_w2v2_pos_pack")
    bits = host(packed)
    assert untouched(bits[-64:]), "wrote behind its output"
    return {"packed": bits[:-64].reshape(A.POS_G, Mp, A.POS_C)}


def run_pos_add(case, inp):
    L = _lib()
    B, S, _ = case
    x, conv, fr = dev(inp["x"]), dev(inp["conv"]), dev(inp["frames"])
    y = filled((B * S + A.TAIL, A.HID), torch.float32)
    _ok(L.lib().ufnd_w2v2_pos_add(x.data_ptr(), conv.data_ptr(), fr.data_ptr(), y.data_ptr(), B, S, _s()), "ufnd_w2v2_pos_add")
    y = host(y)
    assert untouched(y[B * S:]), "wrote behind its output"
    return {"y": y[:B * S]}


def run_pos_conv(case, inp):
    """pack -> one overlapping-row GEMM per group (lda = 48, K = 6,144, N = 64, GELU, fp32 out) -> add: the encoder's own sequence"""
    L = _lib()
    B, S, _ = case
    Sp = S + A.POS_K
    Mp = B * Sp + A.POS_K
    xb, x, fr, wg, bg = (dev(inp[k]) for k in ("xb", "x", "frames", "wg", "bg"))
    packed = filled((A.POS_G, Mp, A.POS_C), torch.int16)
    pconv = filled((A.POS_G, B * Sp, 64), torch.float32)
    y = filled((B * S + A.TAIL, A.HID), torch.float32)
    _ok(L.lib().ufnd_w2v2_pos_pack(xb.data_ptr(), fr.data_ptr(), packed.data_ptr(), B, S, _s()), "ufnd_w2v2_pos_pack")
    for g in range(A.POS_G):
        _ok(L.lib().ufnd_conv1d_rows_bf16(packed[g].data_ptr(), wg[g].data_ptr(), bg[g].data_ptr(), None, pconv[g].data_ptr(), B * Sp, 64,
                                          A.POS_K * A.POS_C, A.POS_C, A.POS_K * A.POS_C, 0, 64, 1, _s()), "ufnd_conv1d_rows_bf16")
    _ok(L.lib().ufnd_w2v2_pos_add(x.data_ptr(), pconv.data_ptr(), fr.data_ptr(), y.data_ptr(), B, S, _s()), "ufnd_w2v2_pos_add")
    y = host(y)
    assert untouched(y[B * S:]), "wrote behind its output"
    return {"y": y[:B * S]}


def wave_normalize(wave: np.ndarray, lengths: np.ndarray) -> np.ndarray:
    """(B, n_max) result of one launch; everything past each length must still hold the sentinel"""
    L = _lib()
    B, n_max = wave.shape
    nws = 3 * B * -(-n_max // A.WCH)
    w, n = dev(wave), dev(lengths)
    out, ws = filled((B + A.TAIL, n_max), torch.float32), filled((nws + 8,), torch.float32)
    _ok(L.lib().ufnd_wave_normalize(w.data_ptr(), n.data_ptr(), out.data_ptr(), ws.data_ptr(), B, n_max, _s()), "ufnd_wave_normalize")
    out, ws = host(out), host(ws)
    assert untouched(out[B:]) and untouched(ws[nws:]), "wrote behind its output / its workspace"
    for b, k in enumerate(lengths.tolist()):
        assert untouched(out[b, k:]), f"row {b}: wrote past its {k} samples"
    return out[:B]


def run_wave_normalize(case, inp):
    _, lengths = case
    out = wave_normalize(inp["wave"], inp["lengths"])
    got = {f"out{b}": out[b, :n].copy() for b, n in enumerate(lengths)}
    if len(lengths) > 1:      # a clip alone is its batch row, bit for bit
        for b, n in enumerate(lengths):
            alone = wave_normalize(inp["wave"][b:b + 1, :n], inp["lengths"][b:b + 1])[0]
            assert np.array_equal(alone.view(np.uint32), got[f"out{b}"].view(np.uint32)), f"clip of {n} samples: alone and in the batch differ"
    return got


def conv0(inp, wave: np.ndarray, lengths: np.ndarray, S1: int):
    L = _lib()
    B, n_max = wave.shape
    nws = 3 * B * A.C0 * -(-S1 // A.FCH) + 2 * B * A.C0
    t = {k: dev(inp[k]) for k in ("w", "gamma", "beta")}
    w, n = dev(wave), dev(lengths)
    ob, of = filled((B * S1 + A.TAIL, A.C0), torch.int16), filled((B * S1 + A.TAIL, A.C0), torch.float32)
    ws = filled((nws + 8,), torch.float32)
    _ok(L.lib().ufnd_w2v2_conv0(w.data_ptr(), n.data_ptr(), t["w"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), ob.data_ptr(),
                                of.data_ptr(), ws.data_ptr(), B, n_max, S1, A.CONV0_EPS, _s()), "ufnd_w2v2_conv0")
    ob, of, ws = host(ob), host(of), host(ws)
    # (the header does not say what a slab's rows past T1 hold: nothing is asserted about them)
    assert untouched(ob[B * S1:]) and untouched(of[B * S1:]) and untouched(ws[nws:]), "wrote behind its output / its workspace"
    rows = [(b * S1, b * S1 + A.conv0_T1(k)) for b, k in enumerate(lengths.tolist())]
    return [of[lo:hi].copy() for lo, hi in rows], [ob[lo:hi].copy() for lo, hi in rows]


def run_conv0(case, inp):
    _, lengths, extra = case
    S1 = A.conv0_S1(lengths, extra)
    of, ob = conv0(inp, inp["wave"], inp["lengths"], S1)
    if len(lengths) > 1:
        for b, n in enumerate(lengths):
            f1, b1 = conv0(inp, inp["wave"][b:b + 1, :n], inp["lengths"][b:b + 1], A.conv0_S1((n,), extra))
            assert np.array_equal(f1[0].view(np.uint32), of[b].view(np.uint32)) and np.array_equal(b1[0], ob[b]), \
                f"clip of {n} samples: alone and in the batch differ"
    got = {f"of{b}": v for b, v in enumerate(of)}
    got.update({f"ob{b}": A.bf16_f32(v) for b, v in enumerate(ob)})
    return got


RUN = {"w2v2_frames": run_frames, "w2v2_pos_pack": run_pos_pack, "w2v2_pos_add": run_pos_add, "w2v2_pos_conv": run_pos_conv,
       "wave_normalize": run_wave_normalize, "w2v2_conv0": run_conv0}
assert set(RUN) == set(A.OPS)


def measure(op, case):
    """{output: error / bound} of one case on the GPU"""
    inp = A.OPS[op].make(case)
    got = RUN[op](case, inp)
    torch.cuda.synchronize()
    return A.check(op, case, inp, got)


def group_of(op, case) -> str:
    """the case groups the record is kept by: the data kind for the statistics kernels, the op itself otherwise"""
    return f"{op} {case[0]}" if op in ("wave_normalize", "w2v2_conv0") else op


PARAMS = [(op, c) for op in sorted(A.OPS) for c in A.OPS[op].cases]
EXACT_OPS = ("w2v2_frames", "w2v2_pos_pack", "w2v2_pos_add")


@pytest.mark.parametrize("op,case", PARAMS, ids=[f"{op}-{A.case_id(c)}" for op, c in PARAMS])
def test_kernel_against_float64(op, case):
    ratios = measure(op, case)
    key = max(ratios, key=lambda k: ratios[k])
    print(f"{group_of(op, case)}: worst error / bound {ratios[key]:.3g} at {A.case_id(case)} ({key})")
    assert ratios[key] <= 1.0, (op, case, ratios)
    if op in EXACT_OPS or case[0] == "constant" and op == "wave_normalize":
        assert ratios[key] == 0.0, (op, case, ratios)
