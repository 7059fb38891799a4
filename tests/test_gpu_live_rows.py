"""GPU: the live-row entries of the packed text pass (include/ultrafnd_hip.h, the packed-rows block above ufnd_text_pack), called
directly through the C ABI.  The frozen text encoder runs every launch at its padded capacity and reads the live row count T from
the device; these tests hold each entry to its contract at the row counts, capacities and masks where such kernels go wrong:

  - live rows are bit-identical to the capacity-sized (padded) call on the same operands;
  - outputs past T keep whatever they held (the persistent GEMM: past the end of the last live 256-row panel);
  - operand rows past T (NaN / Inf here) never reach a live row;
  - counts below 0 or above the capacity are clamped; the fold guard looks at live rows only.

Output buffers are prefilled with a NaN bit pattern (SENT16 / SENT32) and compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PP = 64                     # UFND_GEMM_TILE_PERSISTENT
PANEL = 256                 # the persistent GEMM's row panel
SENT16 = 0x7FA5             # bf16 NaN with a payload no kernel writes
SENT32 = 0x7FC0DEAD         # fp32 NaN with a payload no kernel writes


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _sent_f32(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _untouched(t):
    """every element still holds the sentinel"""
    return bool((_bits(t) == (SENT16 if t.dtype == torch.bfloat16 else SENT32)).all())


def _split_stats(x, parts):
    M, H = x.shape
    xs = x.view(M, parts, H // parts)
    return torch.stack([xs.sum(2), (xs * xs).sum(2)], 2).contiguous()


def _guard_ref(st, T, width, eps):
    """float64 max over rows < T of |mean| / sqrt(var + eps) of a statistics buffer (M, parts, 2)"""
    if T <= 0:
        return 0.0
    s = st[:T].double()
    mean = s[..., 0].sum(1) / width
    var = (s[..., 1].sum(1) / width - mean * mean).clamp_min(0)
    return float((mean.abs() / (var + eps).sqrt()).max())


def _poison(t, T, k):
    """a copy of t whose rows T.. hold NaN (k even) or +Inf (k odd)"""
    t = t.clone()
    if T < t.shape[0]:
        t[max(T, 0):] = float("nan") if k % 2 == 0 else float("inf")
    return t


def _pack_np(mask):
    """numpy restatement of ufnd_text_pack: (cu, row_src[:T])"""
    B, L = mask.shape
    nz = mask != 0
    last = np.where(nz.any(1), L - np.argmax(nz[:, ::-1], axis=1), 0).astype(np.int64)
    cu = np.zeros(B + 1, dtype=np.int64)
    cu[1:] = np.cumsum(last)
    src = np.concatenate([b * L + np.arange(last[b]) for b in range(B)]) if cu[-1] else np.zeros(0, np.int64)
    return cu, src


def _pack(mask_d):
    """ufnd_text_pack on the device: (cu, row_src) with row_src sized to the capacity"""
    L = _lib()
    B, Lq = mask_d.shape
    cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    src = torch.full((B * Lq,), -7, dtype=torch.int32, device=DEV)
    L.check(L.lib().ufnd_text_pack(mask_d.data_ptr(), B, Lq, cu.data_ptr(), src.data_ptr(), L.stream_ptr(mask_d.device)), "ufnd_text_pack")
    return cu, src


def _counts(cap, bm, seed, extra=()):
    g = np.random.default_rng(seed)
    c = {-5, 0, 1, bm - 1, bm, bm + 1, 255, 256, 257, cap - 1, cap, cap + 100} | set(int(x) for x in g.integers(2, cap, 8)) | set(extra)
    return sorted(x for x in c if x <= cap + 100)


# ------------------------------------------------------------------------------------------------------------------ ufnd_text_pack
PACK_CASES = [(B, L) for B in (1, 7, 1024, 1025, 3000, 16384) for L in (1, 40, 128, 256, 512) if B * L <= 1 << 21]


def test_text_pack_against_numpy():
    L = _lib()
    g = torch.Generator().manual_seed(3)
    for B, Lq in PACK_CASES:
        masks = []
        m = (torch.rand(B, Lq, generator=g) < 0.6).int()          # random with holes
        m[0] = 0                                                   # all-masked first and last samples
        m[-1] = 0
        masks.append(("holes", m))
        lens = torch.randint(0, Lq + 1, (B,), generator=g)
        m = (torch.arange(Lq)[None] < lens[:, None]).int() * torch.randint(-3, 4, (B, Lq), generator=g, dtype=torch.int32)   # non-{0,1} values
        masks.append(("values", m))
        masks.append(("all-masked", torch.zeros(B, Lq, dtype=torch.int32)))
        masks.append(("full", torch.ones(B, Lq, dtype=torch.int32)))
        for what, m in masks:
            cu_np, src_np = _pack_np(m.numpy())
            cu, src = _pack(m.to(DEV).contiguous())
            torch.cuda.synchronize()
            T = int(cu_np[-1])
            tag = (f"ufnd_text_pack B={B} L={Lq} mask={what} T={T}")
            assert np.array_equal(cu.cpu().numpy(), cu_np), tag
            s = src.cpu().numpy()
            assert np.array_equal(s[:T], src_np), tag
            assert (s[T:] == -7).all(), tag + ": row_src past T written"
    # a batch past the kernel's shared-memory scan is refused with a message, nothing launched
    m = torch.ones(16385, 1, dtype=torch.int32, device=DEV)
    cu = torch.zeros(16386, dtype=torch.int32, device=DEV)
    src = torch.zeros(16385, dtype=torch.int32, device=DEV)
    rc = L.lib().ufnd_text_pack(m.data_ptr(), 16385, 1, cu.data_ptr(), src.data_ptr(), L.stream_ptr(m.device))
    assert rc != 0 and b"B=16385" in L.lib().ufnd_last_error(), L.lib().ufnd_last_error()
    torch.cuda.synchronize()
    assert int(cu.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------------- live-row GEMMs
class _Gemm:
    """One GEMM call (mode plain / fold / res / rln) at capacity M, its operands clean and with poisoned dead rows."""

    def __init__(self, M, N, mode, act, tile, seed, pp=False, K=768):
        L = _lib()
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.mode, self.act, self.tile, self.pp = M, N, K, mode, act, tile, pp
        x = (torch.randn(M, K, generator=g) * 1.3 + 0.2)
        self.A = x.to(DEV).bfloat16()
        self.W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).bfloat16()
        self.bias = torch.randn(N, generator=g).to(DEV)
        self.res = self.rb = self.st = self.rst = None
        if mode == "plain" and not pp:
            self.res = torch.randn(M, N, generator=g).to(DEV)
        if mode == "fold":
            self.st = _split_stats(x.to(DEV), 24)
            self.colsum = self.W.float().sum(1).contiguous()
        if mode in ("res", "rln"):
            r = (torch.randn(M, N, generator=g) * 1.5 - 0.2).to(DEV)
            if mode == "rln":
                self.rst = _split_stats(r, 12)
                self.gamma, self.beta = (1 + 0.2 * torch.randn(N, generator=g)).to(DEV), (0.1 * torch.randn(N, generator=g)).to(DEV)
            if pp or mode == "res":
                self.rb = r.bfloat16()
            else:
                self.res = r
        self.guard = torch.zeros(L.FOLD_GUARD_SLOTS, device=DEV)
        self.m_live = torch.zeros(1, dtype=torch.int32, device=DEV)

    def operands(self, T=None, k=0):
        ops = {"A": self.A, "res": self.res, "rb": self.rb, "st": self.st, "rst": self.rst}
        if T is not None:
            ops = {n: (_poison(t, T, k) if t is not None else None) for n, t in ops.items()}
        return ops

    def outputs(self):
        M, N = self.M, self.N
        o = {"ob": _sent_bf16(M, N), "of": None if self.pp or self.mode != "plain" else _sent_f32(M, N)}
        o["ost"] = _sent_f32(M, N // 32, 2) if self.mode in ("res", "rln") else None
        return o

    def launch(self, ops, out, live, tile=None):
        """live: False = the capacity-sized product entry, True = the _live entry with self.m_live"""
        L = _lib()
        M, N, K = self.M, self.N, self.K
        tile = self.tile if tile is None else tile
        mp = self.m_live.data_ptr() if live else None
        s = L.stream_ptr(self.A.device)
        ldr = N if ops["res"] is not None else 0
        ldf = N if out["of"] is not None else 0
        args = (ops["A"].data_ptr(), self.W.data_ptr(), self.bias.data_ptr(), L.ptr(ops["res"]), out["ob"].data_ptr(), L.ptr(out["of"]),
                M, N, K, K, K, ldr, N, ldf, self.act)
        if self.mode == "plain":
            if live:
                return L.lib().ufnd_gemm_bf16_live(*args, tile, mp, s)
            return L.lib().ufnd_gemm_bf16_ex(*args, tile, s)
        ln = L.GemmLn()
        ln.a_eps = ln.r_eps = 1e-5
        ln.tile_cfg = tile
        if self.mode == "fold":
            ln.width = K
            ln.a_stats, ln.colsum, ln.a_parts, ln.guard = ops["st"].data_ptr(), self.colsum.data_ptr(), 24, self.guard.data_ptr()
        else:
            ln.width = N
            ln.out_stats = out["ost"].data_ptr()
            if ops["rb"] is not None:
                ln.residual_bf16, ln.ldrb = ops["rb"].data_ptr(), N
            if self.mode == "rln":
                ln.r_stats, ln.r_gamma, ln.r_beta, ln.r_parts = ops["rst"].data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), 12
        if live:
            return L.lib().ufnd_gemm_bf16_ln_live(*args, C.byref(ln), mp, s)
        return L.lib().ufnd_gemm_bf16_ln(*args, C.byref(ln), s)

    def reference(self, tile=None):
        out = self.outputs()
        rc = self.launch(self.operands(), out, False, tile)
        assert rc == 0, (self.tag(tile), _lib().lib().ufnd_last_error())
        torch.cuda.synchronize()
        assert torch.isfinite(out["ob"].float()).all(), self.tag(tile)
        return out

    def tag(self, tile=None, count=None, T=None):
        tile = self.tile if tile is None else tile
        kind = "persistent" if self.pp else f"tile {tile}"
        return f"ufnd_gemm_bf16_{'live' if self.mode == 'plain' else 'ln_live'} {kind} mode={self.mode} act={self.act} M={self.M} N={self.N} m_live={count} (T={T})"

    def check_count(self, ref, count, k, tile=None, reps=1):
        """one device count: live rows == ref, dead rows untouched, the fold guard == float64 over live rows"""
        L = _lib()
        T = min(max(count, 0), self.M)
        tag = self.tag(tile, count, T)
        # the persistent kernel stores whole panels: the ragged last live panel may be written past T
        D = min(-(-T // PANEL) * PANEL, self.M) if self.pp else T
        ops = self.operands(T, k)
        if self.mode == "fold":
            ops["st"][T:] = float("nan") if k % 2 == 0 else 1e30      # NaN or huge statistics in dead rows
        self.m_live.fill_(count)
        for rep in range(reps):      # (persistent form: fresh outputs every time, as tests/test_gpu_gemm_pp.py does)
            out = self.outputs()
            self.guard.zero_()
            rc = self.launch(ops, out, True, tile)
            assert rc == 0, (tag, L.lib().ufnd_last_error())
            torch.cuda.synchronize()
            for n in ("ob", "of", "ost"):
                if out[n] is None:
                    continue
                got, want = _bits(out[n][:T]), _bits(ref[n][:T])
                assert torch.equal(got, want), (tag, n, rep, "live rows differ", int((got != want).sum()))
                assert _untouched(out[n][D:]), (tag, n, rep, "dead rows written")
            if self.mode == "fold":
                want = _guard_ref(self.st, T, self.K, 1e-5)
                got = float(self.guard.max())
                assert abs(got - want) <= 1e-3 * max(want, 1.0), (tag, "fold guard", got, want)


def _exported_tiles():
    L = _lib()
    out = []
    for t in range(L.lib().ufnd_gemm_bf16_tile_count()):
        bm, bn, ln = C.c_int(), C.c_int(), C.c_int()
        if L.lib().ufnd_gemm_bf16_tile_info(t, C.byref(bm), C.byref(bn), C.byref(ln)):
            out.append((t, bm.value, bn.value, ln.value))
    return out


def test_gemm_live_every_exported_tile():
    """Every exported one-tile kernel at a ragged capacity (2 bm + 37): plain (bias, act 0/1/2, fp32 residual, both outputs), folded
    LayerNorm with the guard, bf16 residual with statistics out, residual through a LayerNorm with statistics out."""
    L = _lib()
    tiles = _exported_tiles()
    assert len(tiles) >= 4
    for i, (t, bm, bn, ln_aware) in enumerate(tiles):
        M = 2 * bm + 37
        N = 2304 if 2304 % bn == 0 else bn * 6
        modes = [("plain", i % 3, N)]
        if ln_aware:
            modes += [("fold", 1 + i % 2, N)]
            if 768 % bn == 0:
                modes += [("res", 0, 768), ("rln", 0, 768)]
        for mode, act, n in modes:
            case = _Gemm(M, n, mode, act, t, seed=100 + t)
            if mode in ("res", "rln"):
                out = case.outputs()
                rc = case.launch(case.operands(), out, False)
                if rc != 0:      # a tile whose wave columns are not whole 32-column groups has no statistics epilogue
                    assert b"out_stats" in L.lib().ufnd_last_error(), (t, L.lib().ufnd_last_error())
                    continue
            ref = case.reference()
            for k, count in enumerate(_counts(M, bm, seed=t)):
                case.check_count(ref, count, k)


# (M, N, mode, act): forced persistent launches, all accepted at the capacity (at least 8 tiles)
PP_CASES = [
    (2048, 3072, "fold", 1),      # FFN1 shape: 192 tiles
    (2048, 128, "plain", 0),      # one column tile per panel: live tile counts 0 .. 8, below the 8 workgroups
    (2048, 384, "plain", 2),      # three per panel: 3, 6, ..., 21 live tiles against 24 workgroups
    (2048, 768, "res", 0),
    (2048, 768, "rln", 0),
    (2048, 2304, "fold", 0),      # folded Q/K/V
]


@pytest.mark.parametrize("M,N,mode,act", PP_CASES)
def test_gemm_live_persistent(M, N, mode, act):
    """(the reference is the same kernel at full capacity; against float64: tests/test_gpu_gemm_pp_cases.py, the LiveCase table of tests/gemm_pp_cases.py)"""
    case = _Gemm(M, N, mode, act, PP, seed=M + N + act, pp=True)
    ref = case.reference()
    extra = [PANEL * p + d for p in range(1, 8) for d in (0, 1, 77)]      # every live panel count, whole and ragged
    for k, count in enumerate(_counts(M, PANEL, seed=N, extra=extra)):
        case.check_count(ref, count, k, reps=2)


def test_gemm_live_automatic_choice():
    """tile_cfg < 0: a folded GELU call with enough tiles goes to the persistent form, a ragged plain one to a one-tile kernel."""
    big = _Gemm(8192, 3072, "fold", 1, -1, seed=5, pp=True)
    ref = big.reference()
    for k, count in enumerate(_counts(8192, PANEL, seed=1, extra=(PANEL * 3 + 5, 8192 - 300))):
        big.check_count(ref, count, k)
    small = _Gemm(1000, 2304, "plain", 1, -1, seed=6)
    ref = small.reference()
    for k, count in enumerate(_counts(1000, 128, seed=2)):
        small.check_count(ref, count, k)


@pytest.mark.parametrize("tile,M,T", [(22, 2 * 256 + 37, 2 * 256 + 20), (16, 2 * 128 + 37, 128 + 50), (PP, 2048, 5 * PANEL + 77)])
def test_fold_guard_sees_an_outlier_in_the_last_live_row(tile, M, T):
    """Negative control of the live-row guard: an outlier row at T - 1 (inside a ragged tile / panel) shows up, one at T does not."""
    pp = tile == PP
    case = _Gemm(M, 3072 if pp else 2304, "fold", 1, tile, seed=T, pp=pp)
    x = (case.A.float()).clone()
    for row, seen in ((T - 1, True), (T, False)):
        xo = x.clone()
        xo[row] += 40.0
        case.st = _split_stats(xo, 24)
        case.m_live.fill_(T)
        out = case.outputs()
        case.guard.zero_()
        rc = case.launch(case.operands(), out, True)
        assert rc == 0, _lib().lib().ufnd_last_error()
        torch.cuda.synchronize()
        got, live, outlier = float(case.guard.max()), _guard_ref(case.st, T, 768, 1e-5), _guard_ref(case.st[row:row + 1], 1, 768, 1e-5)
        tag = (case.tag(count=T, T=T), "outlier row", row)
        assert abs(got - live) <= 1e-3 * max(live, 1.0), (tag, got, live)
        assert (abs(got - outlier) <= 1e-3 * outlier) == seen and outlier > 10, (tag, got, outlier)


def test_gemm_live_capture_follows_the_device_count():
    """A _live and an _ln_live launch captured into one graph: the count rewritten between replays (larger, smaller, 0, the
    capacity, past it) -- each replay equals an eager call."""
    L = _lib()
    plain = _Gemm(2 * 256 + 37, 2304, "plain", 1, 22, seed=41)
    fold = _Gemm(2048, 3072, "fold", 1, PP, seed=42, pp=True)
    fold.m_live = plain.m_live
    po, fo = plain.outputs(), fold.outputs()
    pops, fops = plain.operands(), fold.operands()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plain.m_live.fill_(300)
        assert plain.launch(pops, po, True) == 0 and fold.launch(fops, fo, True) == 0
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert plain.launch(pops, po, True) == 0 and fold.launch(fops, fo, True) == 0
    for count in (300, 1700, 40, 0, 2048, 5000):
        for o in (po, fo):
            for t in o.values():
                if t is not None:
                    _bits(t).fill_(SENT16 if t.dtype == torch.bfloat16 else SENT32)
        plain.m_live.fill_(count)
        graph.replay()
        torch.cuda.synchronize()
        pe, fe = plain.outputs(), fold.outputs()
        assert plain.launch(pops, pe, True) == 0 and fold.launch(fops, fe, True) == 0
        torch.cuda.synchronize()
        for what, o, e in (("one-tile", po, pe), ("persistent", fo, fe)):
            for n in o:
                if o[n] is not None:
                    assert torch.equal(_bits(o[n]), _bits(e[n])), ("captured", what, n, "m_live", count)
    del graph


# ------------------------------------------------------------------------------------------------------- the other live kernels
def _mask_with_edges(B, Lq, seed, lo=1):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, Lq + 1, (B,), generator=g)
    m = (torch.arange(Lq)[None] < lens[:, None]).int()
    m[0] = 0                                  # all-masked first sample
    if B > 2:
        m[1] = 0
        m[1, 0] = 1                           # length 1
        m[2] = 1                              # full length
    if B > 4:
        m[3, Lq // 4: Lq // 2] = 0            # a hole
        m[4] = 0                              # all-masked middle sample
    if B > 5 and Lq > 70:
        m[5] = 1
        m[5, :70] = 0                         # the first 64-key block wholly masked
    return m


def test_bert_embed_and_layernorm_live():
    """ufnd_bert_embed_live = ufnd_bert_embed rows gathered by row_src (ids out of range included); ufnd_layernorm_live =
    ufnd_layernorm on the live rows (ldx > H); dead rows untouched, at every count."""
    L = _lib()
    g = torch.Generator().manual_seed(12)
    H, vocab, eps = 768, 1000, 1e-12
    word = torch.randn(vocab, H, generator=g).to(DEV)
    pos = torch.randn(512, H, generator=g).to(DEV)
    type0 = torch.randn(H, generator=g).to(DEV)
    gamma, beta = (1 + 0.2 * torch.randn(H, generator=g)).to(DEV), (0.1 * torch.randn(H, generator=g)).to(DEV)
    s = L.stream_ptr(word.device)
    for B, Lq in ((7, 77), (3, 512), (40, 40)):
        ids = torch.randint(0, vocab, (B, Lq), generator=g)
        ids[0, :5] = torch.tensor([-5, vocab, vocab + 10, -1, 2 ** 40])
        ids[2, -3:] = torch.tensor([-(2 ** 40), vocab - 1, vocab * 3])
        ids = ids.to(DEV).contiguous()
        mask = _mask_with_edges(B, Lq, B).to(DEV).contiguous()
        mask[2, 0] = 1
        cu, src = _pack(mask)
        M = B * Lq
        fb, ff = torch.empty(M, H, dtype=torch.bfloat16, device=DEV), torch.empty(M, H, device=DEV)
        L.check(L.lib().ufnd_bert_embed(ids.data_ptr(), word.data_ptr(), pos.data_ptr(), type0.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                        fb.data_ptr(), ff.data_ptr(), B, Lq, H, vocab, eps, s), "ufnd_bert_embed")
        torch.cuda.synchronize()
        T = int(cu[-1])
        # counts past T (up to the clamp at the capacity) read row_src[T:]: give those rows valid tokens too
        src[T:] = torch.arange(M - T, device=DEV, dtype=torch.int32) * 7 % M
        rs = src.long()
        for count in sorted({-5, 0, 1, 3, T - 1, T, M, M + 100} | ({T // 2} if T > 2 else set())):
            n = min(max(count, 0), M)
            lc = torch.tensor([count], dtype=torch.int32, device=DEV)
            lb, lf = _sent_bf16(M, H), _sent_f32(M, H)
            L.check(L.lib().ufnd_bert_embed_live(ids.data_ptr(), src.data_ptr(), lc.data_ptr(), word.data_ptr(), pos.data_ptr(), type0.data_ptr(),
                                                 gamma.data_ptr(), beta.data_ptr(), lb.data_ptr(), lf.data_ptr(), M, Lq, H, vocab, eps, s),
                    "ufnd_bert_embed_live")
            torch.cuda.synchronize()
            tag = f"ufnd_bert_embed_live B={B} L={Lq} m_live={count} (T={T})"
            assert torch.equal(_bits(lb[:n]), _bits(fb[rs[:n]])) and torch.equal(_bits(lf[:n]), _bits(ff[rs[:n]])), tag
            assert _untouched(lb[n:]) and _untouched(lf[n:]), tag + ": dead rows written"
        # LayerNorm over the live rows of a wider fp32 buffer (ldx = H + 64), dead rows poisoned
        ldx = H + 64
        xw = (torch.randn(M, ldx, generator=g) * 2 + 0.3).to(DEV)
        ob, of = torch.empty(M, H, dtype=torch.bfloat16, device=DEV), torch.empty(M, H, device=DEV)
        L.check(L.lib().ufnd_layernorm(xw.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), ob.data_ptr(), of.data_ptr(), M, H, eps, s), "ufnd_layernorm")
        for k, count in enumerate(sorted({-5, 0, 1, 3, T, M - 1, M, M + 100})):
            n = min(max(count, 0), M)
            xp = _poison(xw, n, k)
            lc = torch.tensor([count], dtype=torch.int32, device=DEV)
            lb, lf = _sent_bf16(M, H), _sent_f32(M, H)
            L.check(L.lib().ufnd_layernorm_live(xp.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), lb.data_ptr(), lf.data_ptr(), M, H, eps,
                                                lc.data_ptr(), s), "ufnd_layernorm_live")
            torch.cuda.synchronize()
            tag = f"ufnd_layernorm_live capacity={M} ldx={ldx} m_live={count}"
            assert torch.equal(_bits(lb[:n]), _bits(ob[:n])) and torch.equal(_bits(lf[:n]), _bits(of[:n])), tag
            assert _untouched(lb[n:]) and _untouched(lf[n:]), tag + ": dead rows written"


MEANPOOL_BOUND = 6e-8      # 2.3e-8 measured against float64 on MI355X (unit-norm rows): about 2.5x


def test_masked_meanpool_live():
    """ufnd_masked_meanpool_l2_live over packed rows (dead rows NaN) = ufnd_masked_meanpool_l2 over the padded layout, bit for bit;
    close to float64; an all-masked sample gives exact zeros."""
    L = _lib()
    g = torch.Generator().manual_seed(8)
    H = 768
    worst = 0.0
    for B, Lq in ((9, 40), (6, 128), (5, 512), (1500, 16)):
        mask = _mask_with_edges(B, Lq, Lq).to(DEV).contiguous()
        mask[-1] = 0                                               # all-masked last sample
        cu, src = _pack(mask)
        T = int(cu[-1])
        M = B * Lq
        hid = (torch.randn(M, H, generator=g) + 0.3).to(DEV)
        packed = torch.full((M, H), float("nan"), device=DEV)
        packed[:T] = hid[src[:T].long()]
        want, got = torch.empty(B, H, device=DEV), _sent_f32(B, H)
        s = L.stream_ptr(hid.device)
        L.check(L.lib().ufnd_masked_meanpool_l2(hid.data_ptr(), mask.data_ptr(), want.data_ptr(), B, Lq, H, s), "ufnd_masked_meanpool_l2")
        L.check(L.lib().ufnd_masked_meanpool_l2_live(packed.data_ptr(), mask.data_ptr(), cu.data_ptr(), got.data_ptr(), B, Lq, H, s),
                "ufnd_masked_meanpool_l2_live")
        torch.cuda.synchronize()
        tag = f"ufnd_masked_meanpool_l2_live B={B} L={Lq} T={T}"
        assert torch.equal(_bits(got), _bits(want)), (tag, (got - want).abs().max().item())
        empty = (mask == 0).all(1)
        assert torch.equal(_bits(got[empty]), torch.zeros_like(_bits(got[empty]))), tag + ": all-masked sample is not exact zeros"
        m = mask.double().view(B, Lq, 1)
        mean = (hid.double().view(B, Lq, H) * m).sum(1) / m.sum(1).clamp_min(1)
        ref = mean / mean.norm(dim=1, keepdim=True).clamp_min(1e-12)
        err = (got.double() - ref).abs().max().item()
        worst = max(worst, err)
        assert err <= MEANPOOL_BOUND, (tag, err)
    print(f"masked meanpool (live): max-abs error vs float64 {worst:.3e} (bound {MEANPOOL_BOUND:.1e})")


def _attn_ref64(qkv, mask, cu, B, heads):
    """float64 attention of the packed rows: sample b's queries and keys are its rows cu[b] .. cu[b+1], keys masked by mask[b]"""
    H = heads * 64
    out = torch.zeros(qkv.shape[0], H, dtype=torch.float64, device=DEV)
    for b in range(B):
        r0, r1 = int(cu[b]), int(cu[b + 1])
        if r1 == r0:
            continue
        n = r1 - r0
        x = qkv[r0:r1].double().view(n, 3, heads, 64)
        sc = torch.einsum("qhd,khd->hqk", x[:, 0], x[:, 1]) * 0.125
        sc = sc.masked_fill(mask[b, :n][None, None, :] == 0, float("-inf"))
        out[r0:r1] = torch.einsum("hqk,khd->qhd", torch.softmax(sc, -1), x[:, 2]).reshape(n, H)
    return out


@pytest.mark.parametrize("Lq", [1, 40, 64, 77, 200, 256, 512])
def test_attention_varlen_masked(Lq):
    """ufnd_attention_bf16_varlen_masked over packed rows (dead rows NaN): bit-identical to the padded ufnd_attention_bf16 on live
    rows -- also at L <= 64, where the padded form runs the 2-wave kernel and the varlen form the 4-wave one: the per-query arithmetic
    is the same -- within 3e-2 of float64, and ctx rows past T untouched."""
    L = _lib()
    heads, H = 12, 768
    B = {1: 5, 40: 9, 64: 9, 77: 9, 200: 7, 256: 7, 512: 6}[Lq]
    g = torch.Generator().manual_seed(Lq)
    mask = _mask_with_edges(B, Lq, Lq + 1).to(DEV).contiguous() if Lq > 1 else torch.tensor([[0], [1], [1], [0], [1]], dtype=torch.int32, device=DEV)
    cu, src = _pack(mask)
    T, M = int(cu[-1]), B * Lq
    qkv = (torch.randn(M, 3 * H, generator=g) * 1.5).to(DEV).bfloat16()
    packed = torch.full((M, 3 * H), float("nan"), dtype=torch.bfloat16, device=DEV)
    packed[:T] = qkv[src[:T].long()]
    ctx_pad, ctx = torch.empty(M, H, dtype=torch.bfloat16, device=DEV), _sent_bf16(M, H)
    s = L.stream_ptr(qkv.device)
    L.check(L.lib().ufnd_attention_bf16(qkv.data_ptr(), mask.data_ptr(), ctx_pad.data_ptr(), B, Lq, heads, s), "ufnd_attention_bf16")
    L.check(L.lib().ufnd_attention_bf16_varlen_masked(packed.data_ptr(), cu.data_ptr(), mask.data_ptr(), ctx.data_ptr(), B, Lq, heads, s),
            "ufnd_attention_bf16_varlen_masked")
    torch.cuda.synchronize()
    tag = f"ufnd_attention_bf16_varlen_masked max_len={Lq} B={B} T={T}"
    want = ctx_pad[src[:T].long()]
    assert torch.equal(_bits(ctx[:T]), _bits(want)), (tag, int((_bits(ctx[:T]) != _bits(want)).sum()))
    assert _untouched(ctx[T:]), tag + ": rows past T written"
    ref = _attn_ref64(packed[:T], mask, cu.cpu(), B, heads)
    err = (ctx[:T].double() - ref).abs().max().item()
    assert err <= 3e-2, (tag, err)


@pytest.mark.parametrize("with_ln", [False, True])
def test_qkv_attention_packed(with_ln):
    """The fused Q/K/V + attention launch over packed rows (dead rows of X and of the statistics NaN): ctx rows equal the padded
    launch's, rows past T untouched; empty samples first and in the middle, full-length ones, holes."""
    L = _lib()
    B, Lq, heads, H = 11, 128, 12, 768
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(B * Lq, H, generator=g) * 1.3 + 0.1).to(DEV)
    Wf = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(3 * H, generator=g)).to(DEV)
    mask = _mask_with_edges(B, Lq, 5).to(DEV).contiguous()
    mask[-2] = 1                                                   # full-length, then a short last sample
    mask[-1] = 0
    mask[-1, :33] = 1
    cu, src = _pack(mask)
    T, M = int(cu[-1]), B * Lq
    rs = src[:T].long()
    guard = torch.zeros(L.FOLD_GUARD_SLOTS, device=DEV)

    def gemm_ln(stats):
        if not with_ln:
            return None
        ln = L.GemmLn()
        ln.a_stats, ln.colsum, ln.a_parts, ln.a_eps, ln.r_eps, ln.width = stats.data_ptr(), cs.data_ptr(), 24, 1e-12, 1e-12, H
        ln.guard = guard.data_ptr()
        return ln
    if with_ln:
        gm, bt = (1 + 0.2 * torch.randn(H, generator=g)).to(DEV), (0.1 * torch.randn(H, generator=g)).to(DEV)
        W = (Wf * gm[None, :]).bfloat16()
        cs = W.float().sum(1).contiguous()
        b2 = (bias + Wf @ bt).contiguous()
    else:
        W, b2 = Wf.bfloat16(), bias
    st = _split_stats(x, 24)
    xb = x.bfloat16()
    xp = torch.full((M, H), float("nan"), dtype=torch.bfloat16, device=DEV)
    xp[:T] = xb[rs]
    stp = torch.full_like(st, float("nan"))
    stp[:T] = st[rs]
    ctx_pad, ctx = torch.empty(M, H, dtype=torch.bfloat16, device=DEV), _sent_bf16(M, H)
    s = L.stream_ptr(x.device)
    ln = gemm_ln(st)
    L.check(L.lib().ufnd_qkv_attention_bf16(xb.data_ptr(), W.data_ptr(), b2.data_ptr(), mask.data_ptr(), ctx_pad.data_ptr(), B, Lq, heads, H, H,
                                            C.byref(ln) if ln is not None else None, s), "ufnd_qkv_attention_bf16")
    guard.zero_()
    ln = gemm_ln(stp)
    L.check(L.lib().ufnd_qkv_attention_bf16_packed(xp.data_ptr(), W.data_ptr(), b2.data_ptr(), mask.data_ptr(), cu.data_ptr(), ctx.data_ptr(),
                                                   B, Lq, heads, H, H, C.byref(ln) if ln is not None else None, s), "ufnd_qkv_attention_bf16_packed")
    torch.cuda.synchronize()
    tag = f"ufnd_qkv_attention_bf16_packed fold={with_ln} B={B} T={T}"
    assert torch.equal(_bits(ctx[:T]), _bits(ctx_pad[rs])), (tag, int((_bits(ctx[:T]) != _bits(ctx_pad[rs])).sum()))
    assert _untouched(ctx[T:]), tag + ": rows past T written"
    if with_ln:      # the guard saw the live rows' statistics only (the dead rows are NaN: they would report +inf)
        want = _guard_ref(st[rs], T, H, 1e-12)
        assert abs(float(guard.max()) - want) <= 1e-3 * max(want, 1.0), (tag, float(guard.max()), want)


# -------------------------------------------------------------------------------------- out_stats sizing (ufnd_gemm_bf16_stat_parts)
@pytest.mark.parametrize("M", [6400, 16384, 25600, 65536])
def test_stat_parts_follow_the_dispatch(M):
    """The encoders size out_stats with ufnd_gemm_bf16_stat_parts(M, 768, 768) at their capacity; the automatic RES_LN call of
    that shape (persistent at 65,536 rows) must write exactly M x parts x 2 floats, the float64 partial sums of its output."""
    L = _lib()
    N = K = 768
    parts = L.lib().ufnd_gemm_bf16_stat_parts(M, N, K)
    assert parts > 0 and N % parts == 0
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, K, generator=g).to(DEV).bfloat16()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV).bfloat16()
    bias = torch.randn(N, generator=g).to(DEV)
    r = (torch.randn(M, N, generator=g) * 1.5 - 0.2).to(DEV)
    rb = r.bfloat16()
    rst = _split_stats(rb.float(), 12)
    gamma, beta = (1 + 0.2 * torch.randn(N, generator=g)).to(DEV), (0.1 * torch.randn(N, generator=g)).to(DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    buf = torch.full((M * parts * 2 + 64,), float("nan"), device=DEV)      # exactly M parts 2 floats, then a NaN canary
    buf[M * parts * 2:] = 12345.0
    ln = L.GemmLn()
    ln.r_stats, ln.r_gamma, ln.r_beta, ln.r_parts, ln.out_stats = rst.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 12, buf.data_ptr()
    ln.residual_bf16, ln.ldrb = rb.data_ptr(), N
    ln.a_eps = ln.r_eps = 1e-12
    ln.width, ln.tile_cfg = N, -1
    L.check(L.lib().ufnd_gemm_bf16_ln(A.data_ptr(), W.data_ptr(), bias.data_ptr(), None, out.data_ptr(), None, M, N, K, K, K, 0, N, 0, 0,
                                      C.byref(ln), L.stream_ptr(A.device)), "ufnd_gemm_bf16_ln")
    torch.cuda.synchronize()
    assert bool((buf[M * parts * 2:] == 12345.0).all()), f"out_stats written past M x {parts} x 2 floats at M={M}"
    ost = buf[:M * parts * 2].view(M, parts, 2)
    # the statistics are of the fp32 output row before its bf16 rounding: recompute it in float64
    v = A.double() @ W.double().t() + bias.double()
    rr = rb.double()
    mean = rr.mean(1, keepdim=True)
    rstd = 1.0 / ((rr * rr).mean(1, keepdim=True) - mean * mean + 1e-12).sqrt()
    v = v + (rr - mean) * rstd * gamma.double() + beta.double()
    want = torch.stack([v.view(M, parts, -1).sum(2), (v * v).view(M, parts, -1).sum(2)], 2)
    err = (ost.double() - want).abs() / (want.abs() + N // parts)
    assert torch.isfinite(ost).all() and err.max().item() <= 1e-3, (M, parts, err.max().item())
