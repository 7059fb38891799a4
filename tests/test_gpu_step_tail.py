"""The end of the training step, entry by entry through the C ABI (ufnd_softmax_ce, ufnd_softmax_ce_weighted, ufnd_grad_accumulate,
ufnd_grad_norm, ufnd_adamw_step, ufnd_step_advance, ufnd_clip_adamw_step), against the float64 references and derived bounds of
tests/step_tail_cases.py (the cases, the derivations and the CPU evidence that the bounds tell a wrong kernel from a rounded one
are there and in tests/test_step_tail_cases.py).

Every device buffer -- inputs, outputs, the partials, the step state -- lies between two sentinel pads, and the pointer handed to
the entry is `lo` floats into the allocation (64, or 148 = 4 x 37: a sub-range of a larger arena, 16-B aligned and no more, as
FusedAdamW.fold(lo, hi) calls it).  Reading a buffer back asserts its pads; read-only inputs must keep their bits; of the state only
the fields an entry owns may change.  Every optimizer case runs in the two-launch form (ufnd_clip_adamw_step) and in the four-launch
form (ufnd_grad_norm + ufnd_adamw_step + ufnd_step_advance) from the same inputs, and the two must leave identical bits in p, m, v,
step, micro, grad_norm, clip_coef, bc1 and bc2_sqrt.  Each test prints its worst error / bound; tools/step_tail_errors.py collects
them into profiles/step_tail_errors.txt.

The shifted cross-entropy cases (logits + 1024, held to the bound of the unshifted rows) failed on the kernels that formed
max + logf(S) - l_c: worst error / bound 1.0e+03 (profiles/step_tail_errors.txt).
"""
import numpy as np
import pytest
import torch

from tests import step_tail_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BACK = 64                                   # sentinel elements behind every buffer
_SENT = np.float32(S.SENTINEL_F32)
_SENT_I64 = 0x5A5A5A5A5A5A5A5A
_SENT_U8 = 0xA5
STATE_OUT = ("step", "micro", "grad_norm", "clip_coef", "bc1", "bc2_sqrt", "loss")


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L


def _s():
    return _lib().stream_ptr(torch.device(DEV))


def _ok(rc, what):
    _lib().check(rc, what)


class Buf:
    """`data` between two sentinel pads on the device; `ptr` points at the data"""

    def __init__(self, data, lo=64):
        data = np.ascontiguousarray(data)
        self.lo, self.n, self.orig = lo, data.size, data
        sent = {np.dtype(np.float32): _SENT, np.dtype(np.int64): _SENT_I64, np.dtype(np.uint8): _SENT_U8}[data.dtype]
        self.sent = np.array([sent], dtype=data.dtype)[0]
        full = np.full(lo + data.size + BACK, self.sent, dtype=data.dtype)
        full[lo:lo + data.size] = data.ravel()
        self.t = torch.from_numpy(full).to(DEV)
        self.ptr = self.t.data_ptr() + lo * data.itemsize
        assert self.ptr % 16 == 0

    def read(self):
        a = self.t.cpu().numpy()
        assert (a[:self.lo] == self.sent).all() and (a[self.lo + self.n:] == self.sent).all(), "wrote outside its buffer"
        return a[self.lo:self.lo + self.n]

    def unchanged(self):
        got, want = self.read(), self.orig.ravel()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), "a read-only input changed"


def fresh(n, lo=64):
    return Buf(np.full(n, _SENT, dtype=np.float32), lo)


class State(Buf):
    """a ufnd_step_state between pads, initialised through StepStateBuffer"""

    def __init__(self, hp: S.HP = S.HP(), step=0, micro=0, loss=None):
        from ultrafnd_git_amd.state import StepStateBuffer
        L = _lib()
        sb = StepStateBuffer(torch.device(DEV), seed=1234, lr=hp.lr, weight_decay=hp.wd, betas=(hp.b1, hp.b2), eps=hp.eps, max_norm=hp.max_norm,
                             grad_scale=hp.gs)
        sb.set_u64("step", step)
        st = sb.read()
        assert st.step == step and st.lr == np.float32(hp.lr)
        st.micro = micro
        for k in ("grad_norm", "clip_coef", "bc1", "bc2_sqrt", "loss"):      # outputs start at a value no case produces
            setattr(st, k, -77.0)
        if loss is not None:
            st.loss = loss
        st.reserved[0], st.reserved[1] = 3.25, -4.5
        self.L = L
        super().__init__(np.frombuffer(bytes(st), dtype=np.uint8).copy(), lo=64)

    def get(self, may_change):
        """the struct; every field outside `may_change` must hold its bits"""
        raw = self.read()
        now = self.L.StepState.from_buffer_copy(raw.tobytes())
        for name, _ in self.L.StepState._fields_:
            f = getattr(self.L.StepState, name)
            if name not in may_change:
                assert np.array_equal(raw[f.offset:f.offset + f.size], self.orig[f.offset:f.offset + f.size]), f"state->{name} changed"
        return now


def _scalars(st):
    return {k: np.array([float(getattr(st, k))]) for k in ("step", "micro", "grad_norm", "clip_coef", "bc1", "bc2_sqrt")}


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
def optimizer_step(p, g, m, v, hp, step0, micro0, lo=64, form="two"):
    """one optimizer step in one form, on fresh buffers -> its outputs"""
    lib, s = _lib().lib(), _s()
    n = p.size
    P, G, M, V = Buf(p, lo), Buf(g, lo), Buf(m, lo), Buf(v, lo)
    part = fresh(S.PARTIALS_FLOATS, 64)
    st = State(hp, step0, micro0)
    if form == "two":
        _ok(lib.ufnd_clip_adamw_step(P.ptr, G.ptr, M.ptr, V.ptr, n, part.ptr, st.ptr, s), "ufnd_clip_adamw_step")
    else:
        _ok(lib.ufnd_grad_norm(G.ptr, n, part.ptr, st.ptr, s), "ufnd_grad_norm")
        _ok(lib.ufnd_adamw_step(P.ptr, G.ptr, M.ptr, V.ptr, n, st.ptr, s), "ufnd_adamw_step")
        _ok(lib.ufnd_step_advance(st.ptr, s), "ufnd_step_advance")
    torch.cuda.synchronize()
    G.unchanged()
    now = st.get(("step", "micro", "grad_norm", "clip_coef", "bc1", "bc2_sqrt"))
    out = dict(p=P.read().copy(), m=M.read().copy(), v=V.read().copy(), **_scalars(now))
    pt = part.read()
    nb = S.norm_grid(n // 4)[0]
    assert (pt[nb:] == _SENT).all(), "a partial behind the launch's block count was written"
    out["partials"] = pt[:nb].copy()
    return out


def both_forms(p, g, m, v, hp, step0, micro0, lo=64):
    """the two-launch form's outputs, after the four-launch form has produced the same bits from the same inputs"""
    two = optimizer_step(p, g, m, v, hp, step0, micro0, lo, "two")
    four = optimizer_step(p, g, m, v, hp, step0, micro0, lo, "four")
    for k in two:
        assert _same_bits(two[k], four[k]), f"the two-launch and the four-launch form differ in {k}"
    return two


def run_accumulate(case, inp):
    n4, kind, with_state = case
    lib, s = _lib().lib(), _s()
    dst, src = Buf(inp["dst"], 148 if n4 % 2 else 64), Buf(inp["src"], 64 if n4 % 2 else 148)
    st = State(S.HP(), step=5, micro=inp["micro0"])
    _ok(lib.ufnd_grad_accumulate(dst.ptr, src.ptr, 4 * n4, 1 if kind == "bits" else 0, st.ptr if with_state else None, s), "ufnd_grad_accumulate")
    torch.cuda.synchronize()
    src.unchanged()
    now = st.get(("micro",))       # no other field of the state may change
    return dict(dst_bits=S.bits(dst.read()), micro=np.array([float(now.micro)]))


def run_step_census(case, inp):
    n4, lo = case
    lib, s = _lib().lib(), _s()
    n = 4 * n4
    ga, gb, g = Buf(inp["ga"], lo), Buf(inp["gb"], lo), fresh(n, lo)
    st = State(inp["hp"], inp["step0"], 0)
    _ok(lib.ufnd_grad_accumulate(g.ptr, ga.ptr, n, 1, st.ptr, s), "ufnd_grad_accumulate")
    _ok(lib.ufnd_grad_accumulate(g.ptr, gb.ptr, n, 0, st.ptr, s), "ufnd_grad_accumulate")
    torch.cuda.synchronize()
    ga.unchanged(), gb.unchanged()
    micro = st.get(("micro",)).micro
    assert micro == 2
    gnp = g.read().copy()
    del ga, gb, g
    out = both_forms(inp["p"], gnp, inp["m"], inp["v"], inp["hp"], inp["step0"], micro, lo)
    out["partials_sum"] = np.array([float(np.sum(out.pop("partials").astype(np.float64)))])
    out["g"] = gnp
    return out


def run_norm_select(case, inp):
    """every probe through ufnd_grad_norm AND through the fused ufnd_clip_adamw_step (its own sum-of-squares loop and finalize), on the
    same gradient buffer; p, m and v are dummies that the fused launch may move"""
    n4 = case[0]
    n = 4 * n4
    lib, s = _lib().lib(), _s()
    G, part = Buf(np.zeros(n, dtype=np.float32), 148), fresh(S.PARTIALS_FLOATS)
    P, M, V = (Buf(np.zeros(n, dtype=np.float32), 148) for _ in range(3))
    data = G.t[G.lo:G.lo + G.n]
    out = np.zeros((len(inp["pos"]), len(S.SELECT_SCALES)))
    for i, x in enumerate(inp["pos"]):
        data[x] = 3.0
        four = [State(S.HP(gs=gs, max_norm=0.0)) for gs in S.SELECT_SCALES]
        two = [State(S.HP(gs=gs, max_norm=0.0)) for gs in S.SELECT_SCALES]
        for st in four:
            _ok(lib.ufnd_grad_norm(G.ptr, n, part.ptr, st.ptr, s), "ufnd_grad_norm")
        for st in two:
            _ok(lib.ufnd_clip_adamw_step(P.ptr, G.ptr, M.ptr, V.ptr, n, part.ptr, st.ptr, s), "ufnd_clip_adamw_step")
        torch.cuda.synchronize()
        data[x] = 0.0
        for j, (a, b) in enumerate(zip(four, two)):
            na = a.get(("grad_norm", "clip_coef", "bc1", "bc2_sqrt"))
            nb = b.get(("step", "micro", "grad_norm", "clip_coef", "bc1", "bc2_sqrt"))
            assert na.clip_coef == 1.0 and nb.clip_coef == 1.0 and nb.step == 1
            assert _same_bits([na.grad_norm], [nb.grad_norm]), ("the forms differ in grad_norm", x, na.grad_norm, nb.grad_norm)
            out[i, j] = nb.grad_norm
    G.unchanged()
    part.read(), P.read(), M.read(), V.read()
    return dict(grad_norm=out)


def run_norm_clip(case, inp):
    """through both forms (the fused one repeats the sum-of-squares loop and the clip expression): p, m, v are small dummies"""
    n = inp["g"].size
    rng = np.random.default_rng(n)
    p, m = (rng.normal(0, 1, n).astype(np.float32) for _ in range(2))
    v = (rng.normal(0, 1, n) ** 2).astype(np.float32)
    out = both_forms(p, inp["g"], m, v, S.HP(gs=case[2], max_norm=case[3]), 0, 0, 148)
    return dict(grad_norm=out["grad_norm"], clip_coef=out["clip_coef"])


def run_step(case, inp):
    out = both_forms(inp["p"], inp["g"], inp["m"], inp["v"], inp["hp"], inp["step0"], 2, 148 if case[0] % 2 else 64)
    out.pop("partials")
    return out


def run_counters(case, inp):
    step0, steps = case
    lib, s = _lib().lib(), _s()
    n = inp["p"].size
    per_form = {}
    for form in ("two", "four"):
        st = State(inp["hp"], step0, 0)
        bufs = tuple(Buf(inp[k]) for k in ("p", "g", "m", "v"))
        scratch = fresh(n)
        rows = {k: [] for k in ("step", "micro_before", "micro", "bc1", "bc2_sqrt")}
        for _ in range(steps):
            _ok(lib.ufnd_grad_accumulate(scratch.ptr, bufs[1].ptr, n, 1, st.ptr, s), "ufnd_grad_accumulate")
            _ok(lib.ufnd_grad_accumulate(scratch.ptr, bufs[1].ptr, n, 0, st.ptr, s), "ufnd_grad_accumulate")
            torch.cuda.synchronize()
            rows["micro_before"].append(float(st.get(STATE_OUT).micro))
            o = _step_on(bufs, st, form, n)
            for k in ("step", "micro", "bc1", "bc2_sqrt"):
                rows[k].append(float(o[k][0]))
        per_form[form] = ({k: np.array(a) for k, a in rows.items()}, [b.read().copy() for b in bufs])
    (r2, b2), (r4, b4) = per_form["two"], per_form["four"]
    for k in r2:
        assert _same_bits(r2[k], r4[k]), f"forms differ in {k}"
    for a, b, k in zip(b2, b4, "pgmv"):
        assert _same_bits(a, b), f"forms differ in {k} after {steps} steps"
    return r2


def _step_on(bufs, st, form, n):
    lib, s = _lib().lib(), _s()
    P, G, M, V = bufs
    part = fresh(S.PARTIALS_FLOATS)
    if form == "two":
        _ok(lib.ufnd_clip_adamw_step(P.ptr, G.ptr, M.ptr, V.ptr, n, part.ptr, st.ptr, s), "ufnd_clip_adamw_step")
    else:
        _ok(lib.ufnd_grad_norm(G.ptr, n, part.ptr, st.ptr, s), "ufnd_grad_norm")
        _ok(lib.ufnd_adamw_step(P.ptr, G.ptr, M.ptr, V.ptr, n, st.ptr, s), "ufnd_adamw_step")
        _ok(lib.ufnd_step_advance(st.ptr, s), "ufnd_step_advance")
    torch.cuda.synchronize()
    part.read()
    G.unchanged()
    return _scalars(st.get(("step", "micro", "grad_norm", "clip_coef", "bc1", "bc2_sqrt")))


def _ce_call(entry, lg, y, B, rows, d, st):
    lib, s = _lib().lib(), _s()
    rp, dp = (None if rows is None else rows.ptr), (None if d is None else d.ptr)
    if entry is None:
        _ok(lib.ufnd_softmax_ce(lg.ptr, y.ptr, B, rp, dp, st.ptr, s), "ufnd_softmax_ce")
    else:
        _ok(lib.ufnd_softmax_ce_weighted(lg.ptr, y.ptr, B, entry[0], entry[1], entry[2], rp, dp, st.ptr, s), "ufnd_softmax_ce_weighted")
    torch.cuda.synchronize()
    lg.unchanged(), y.unchanged()
    return st.get(("loss",)).loss


def run_cross_entropy(case, inp):
    B, _, entry, _ = case
    lg, y = Buf(inp["logits"], 148 if B % 2 else 64), Buf(inp["labels"])
    rows, d = fresh(B), fresh(2 * B)
    loss = _ce_call(entry, lg, y, B, rows, d, State())
    full_rows, full_d = rows.read().copy(), d.read().copy()
    # the null arms: state->loss keeps its bits, and the output that is still asked for keeps its bits
    for want_rows, want_d in ((False, True), (True, False), (False, False)):
        r2, d2 = (fresh(B) if want_rows else None), (fresh(2 * B) if want_d else None)
        loss2 = _ce_call(entry, lg, y, B, r2, d2, State(loss=-5.0))
        assert _same_bits([loss2], [loss]), ("state->loss differs with a null output", want_rows, want_d, loss2, loss)
        assert r2 is None or _same_bits(r2.read(), full_rows)
        assert d2 is None or _same_bits(d2.read(), full_d)
    out = dict(loss_rows=full_rows, loss=np.array([float(loss)]), d_logits=full_d.reshape(B, 2))
    if entry is None:
        out["d_sum"] = out["d_logits"][:, 0].astype(np.float64) + out["d_logits"][:, 1].astype(np.float64)
    return out


RUN = {"accumulate": run_accumulate, "step_census": run_step_census, "norm_select": run_norm_select, "norm_clip": run_norm_clip,
       "adamw_zero_grad": run_step, "adamw_rounded": run_step, "counters": run_counters, "cross_entropy": run_cross_entropy}
assert set(RUN) == set(S.OPS)


def worst_of(op, cases=None, verbose=False):
    """(worst error / bound, case, output) of an op's kernels over its cases"""
    worst = (-1.0, None, None)
    for case in (S.OPS[op].cases if cases is None else cases):
        inp = S.OPS[op].make(case)
        got = RUN[op](case, inp)
        for k, r in S.check(op, case, inp, got).items():
            if verbose:
                print(f"  {op} {S.case_id(case)} {k}: {r:.3g}")
            if r > worst[0]:
                worst = (r, case, k)
    return worst


def shifted_cases():
    return [c for c in S.OPS["cross_entropy"].cases if c[3] == "grid_shifted"]


def _params():
    out = []
    for op in sorted(S.OPS):
        if op == "step_census":
            out += [(op, cl) for cl in S.SIZE_CLASSES]
        elif op == "cross_entropy":
            out += [(op, B) for B in S.CE_B]
        elif op == "norm_select":
            out += [(op, n4) for n4 in S.SELECT_SIZES if 4 * n4 > S.LARGE_FLOATS] + [(op, None)]
        else:
            out.append((op, None))
    return out


def _cases_of(op, part):
    cases = S.OPS[op].cases
    if op == "step_census":
        return [c for c in cases if c[0] in S.SIZE_CLASSES[part]]
    if op == "cross_entropy":
        return [c for c in cases if c[0] == part]
    if op == "norm_select":
        return [c for c in cases if (c[0] == part if part is not None else 4 * c[0] <= S.LARGE_FLOATS)]
    return cases


@pytest.mark.parametrize("op,part", _params(), ids=[op if part is None else f"{op}-{part}" for op, part in _params()])
def test_entry_against_float64(op, part):
    r, case, key = worst_of(op, _cases_of(op, part))
    print(f"{op}: worst error / bound {r:.3g} at {case} ({key})")
    assert r <= 1.0, (op, r, case, key)


def test_weighted_entry_with_unit_weights_is_the_plain_entry():
    """ufnd_softmax_ce_weighted(1, 1, 0) against ufnd_softmax_ce on the same rows: both lie within the bound of the same reference,
    so they differ by at most the sum of their bounds (loss_rows: the weighted entry's are the plain entry's / B)."""
    worst = 0.0
    for B in S.CE_B:
        for kind in ("randn2", "one_of_each", "grid_shifted"):
            plain, unit = (B, "mixed", None, kind), (B, "mixed", (1.0, 1.0, 0.0), kind)
            inp = S.OPS["cross_entropy"].make(plain)
            a, b = run_cross_entropy(plain, inp), run_cross_entropy(unit, inp)
            ra, rb = S.OPS["cross_entropy"].reference(plain, inp), S.OPS["cross_entropy"].reference(unit, inp)
            for k in ("loss_rows", "loss", "d_logits"):
                div = float(B) if k == "loss_rows" else 1.0      # the weighted entry's rows are divided by the weight sum (here B), the plain entry's are not
                shape = ra[k][0].shape
                worst = max(worst, S.worst_ratio(np.asarray(b[k], np.float64).reshape(shape), np.asarray(a[k], np.float64).reshape(shape) / div,
                                                 ra[k][1] / div + rb[k][1]))
    print(f"weighted(1, 1, 0) against plain: worst difference / (sum of the bounds) {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_one_non_finite_gradient_pins_the_present_behaviour(bad):
    """One NaN (or +inf) among 2052 gradients, max_norm = 5, both forms.  The published norm is NaN (+inf).  fminf(1, max_norm / NaN)
    is 1 and max_norm / inf is 0, so the clip coefficient is 1 (0): with the NaN every other element takes its ordinary unclipped
    update; with the +inf every other gradient is scaled to 0 (its moments decay, its parameter moves by the old momentum) and the
    bad one becomes inf * 0 = NaN.  In both cases exactly ONE element of p, m and v turns non-finite -- unlike clip_grad_norm_,
    where the NaN norm multiplies, and poisons, every gradient."""
    n4, k = 513, 4 * 300 + 1
    rng = np.random.default_rng(77)
    n = 4 * n4
    p, g, m, v = (rng.normal(0, 1, n).astype(np.float32) for _ in range(4))
    v = v * v
    g[k] = bad
    out = both_forms(p, g, m, v, S.HP(), 0, 0)
    norm, coef = out["grad_norm"][0], out["clip_coef"][0]
    if np.isnan(bad):
        assert np.isnan(norm) and coef == 1.0
    else:
        assert norm == np.inf and coef == 0.0
    others = np.arange(n) != k
    for name in ("p", "m", "v"):
        assert not np.isfinite(out[name][k]) and np.isfinite(out[name][others]).all(), name
    g_ok = g.copy()
    g_ok[k] = 0.0
    hp = S.HP(max_norm=0.0, gs=float(coef))       # the other elements: an ordinary step at the published coefficient
    refs = S.adamw_ref_bound(p, g_ok, m, v, hp, 1)
    for name in ("p", "m", "v"):
        assert S.worst_ratio(out[name][others], refs[name][0][others], refs[name][1][others]) <= 1.0, name
    assert out["step"][0] == 1 and out["micro"][0] == 0
