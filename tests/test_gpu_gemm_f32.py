"""GPU: every form of the fp32 skinny-GEMM family (csrc/gemm_f32.hip) op by op against float64, through the diagnostics
library's ufnd_diag_gemm_f32_nt / _nn / _tn (the product launchers with a caller-made problem array; they report the kernel
instantiation they launched).  The cases are tests/gemm_f32_cases.py; tests/test_gemm_f32_cases.py keeps them on their forms.

  exact       operands are multiples of 1/4 in [-2, 2]: every partial sum is exact in fp32 in any order, so Z, Y (act 0), the
              summed ksplit / nsplit partials, dW, db and out (no actZ) must be BIT-equal to float64 rounded once.
  random      normal operands against the fp32 FMA-chain bound (L + 8) 2^-24 (|A| @ |B| + |bias or add|), L the contraction
              length (8: the cross-wave LDS adds and the epilogue add).  ksplit / nsplit partials are summed in float64 on
              the host, so split launches are held to the same bound.
  activation  Y = gelu(Z) and out = S gelu'(z) against float64 erf-GELU.  The error of the device's erff / __expf cannot be
              derived; it was measured over this table on an MI355X (the same figure on every form of a family to three digits
              or so: the epilogues share gelu_f / gelu_grad_f):
                  GELU output      max |Y - gelu64(Z)|                 3.831e-07    bound 1.532e-06
                  GELU' factor     max (|out - S gelu'64(z)| - 2^-23 |out|) / |S|   1.317e-07    bound 5.268e-07
              The bounds are four times the measurements (the table samples the argument range at a few thousand points),
              far below the caps, the project's criteria TOL_OUT = 2e-5 (absolute, outputs) and TOL_GRAD = 5e-4 (relative,
              gradient factors).  In the factor's error one fp32 rounding of the result (2^-23 |out|: the final add) is taken
              off first, and where a mask follows, the rounding of its multiplication.
  dropout     multipliers rebuilt by tests/dropout_mirror at the documented element index (nt: m N + n whatever ldy is; nn:
              m drop_ld + k whatever ldo is): kept elements bit-equal to fp32(exact) * 1/(1-p), dropped ones 0.  Negative
              controls: the next step's masks, and the index built with the output's stride.
  bounds      every output buffer is NaN-filled with pad columns and a guard band, every input has NaN in its pad columns, in
              rows past M and between segments: nothing outside the logical panel may change, no NaN may come in.
  batch       row 0 computed alone is bit-equal to row 0 inside 33 and 65 rows.
"""
import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import gemm_f32_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, STEP = 0x5EED_0F_F32_6E33, 11
TOL_OUT, TOL_GRAD = 2e-5, 5e-4
MEASURED_GELU, MEASURED_GRAD = 3.831e-07, 1.317e-07          # MI355X, over the table (module docstring)
BOUND_GELU = min(TOL_OUT, 4 * MEASURED_GELU)
BOUND_GRAD = min(TOL_GRAD, 4 * MEASURED_GRAD)
EPS = 2.0 ** -24
NAN_BITS = 0x7FC00000
GUARD = 64
GEN_ROWS = 65           # operands are drawn for at least this many rows (the batch-invariance variants reuse them)


def _D():
    from tools import _diaglib
    return _diaglib


def gelu64(x):
    x = torch.from_numpy(np.asarray(x, dtype=np.float64))
    return (0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))).numpy()


def gelu_grad64(x):
    x = torch.from_numpy(np.asarray(x, dtype=np.float64))
    return (0.5 * (1.0 + torch.erf(x / np.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# operands (float64 arrays holding fp32-representable values), drawn once per (case, problem, mode)
_OPS = {}


def _draw(g, shape, mode):
    if mode == "exact":
        return g.integers(-8, 9, size=shape).astype(np.float64) / 4.0
    return g.standard_normal(shape).astype(np.float32).astype(np.float64)


def operands(case, i, mode):
    key = (case.id, i, mode)
    if key not in _OPS:
        p, g = case.probs[i], np.random.default_rng([G.CASES.index(case), i, mode == "exact"])
        M = max(p["M"], GEN_ROWS)
        if case.kind == "nt":
            o = {"X": _draw(g, (M, p["K"]), mode), "W": _draw(g, (p["N"], p["K"]), mode), "bias": _draw(g, (p["N"],), mode)}
        elif case.kind == "nn":
            o = {"dY": _draw(g, (M, p["N"]), mode), "W": _draw(g, (p["N"], p["K"]), mode), "add": _draw(g, (M, p["K"]), mode),
                 "actZ": g.integers(-96, 97, size=(M, p["K"])).astype(np.float64) / 16.0,          # [-6, 6] in steps of 1/16
                 "flat": np.where(g.integers(0, 2, size=(M, p["K"])) == 1, 8.0, 0.0)}              # gelu'(0) = 1/2, gelu'(8) = 1 in fp32
        else:
            o = {"dY": _draw(g, (M, p["N"]), mode), "X": _draw(g, (M, p["K"]), mode)}
        _OPS[key] = o
    return _OPS[key]


# ---------------------------------------------------------------------------------------------------------------------
# device buffers: NaN everywhere, the logical panel filled in
class Buf:
    def __init__(self, floats, a8=False):
        self.off = 2 if a8 else 0
        self.flat = torch.full((self.off + floats + GUARD,), float("nan"), dtype=torch.float32)
        self.dev = None

    def put(self, data, ld, seg_rows=0, seg=0):
        """rows of `data` at row stride ld (in segments of seg_rows rows, seg floats apart)"""
        d = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))
        rows, cols = d.shape
        if seg_rows:
            for s in range(rows // seg_rows):
                v = self.flat[self.off + s * seg: self.off + s * seg + seg_rows * ld].view(seg_rows, ld)
                v[:, :cols] = d[s * seg_rows:(s + 1) * seg_rows]
        else:
            self.flat[self.off: self.off + rows * ld].view(rows, ld)[:, :cols] = d
        return self

    def up(self):
        self.dev = self.flat.to(DEV)
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() + 4 * self.off

    def back(self, rows, cols, ld, slabs=1):
        """-> (float32 array (slabs, rows, cols), True when everything outside those panels still holds the NaN fill)"""
        h = self.dev.cpu()
        bits = h.view(torch.int32).clone()
        body = h[self.off: self.off + slabs * rows * ld].view(slabs, rows, ld)
        out = body[:, :, :cols].clone().numpy()
        bits[self.off: self.off + slabs * rows * ld].view(slabs, rows, ld)[:, :, :cols] = NAN_BITS
        return out, bool((bits == NAN_BITS).all())


def _state(step=STEP):
    from ultrafnd_git_amd.state import StepStateBuffer
    st = StepStateBuffer(torch.device(DEV), seed=SEED)
    st.set_u64("step", step)
    return st


def run(case, mode, variant=None, step=STEP, zkey="actZ"):
    """Launch a case (variant: field overrides for every problem).  -> (form, [per-problem dict of outputs + `clean`], [problems])"""
    D = _D()
    probs = [dict(p, **(variant or {})) for p in case.probs]
    bufs = []
    for i, p in enumerate(probs):
        o, M, N, K, b = operands(case, i, mode), p["M"], p["N"], p["K"], {}
        if case.kind == "nt":
            b["X"] = Buf((M + 2) * p["ldx"]).put(o["X"][:M], p["ldx"])
            b["W"] = Buf(N * p["ldw"], p["a8"]).put(o["W"], p["ldw"])
            b["bias"] = Buf(N).put(o["bias"][None, :], N)
            b["Y"] = Buf(p["ksplit"] * M * N if p["ksplit"] > 1 else M * p["ldy"])
            b["Z"] = Buf(M * p["ldz"])
        elif case.kind == "nn":
            b["dY"] = Buf((M + 2) * p["lddy"]).put(o["dY"][:M], p["lddy"])
            b["W"] = Buf(N * p["ldw"], p["a8"]).put(o["W"], p["ldw"])
            b["out"] = Buf(p["nsplit"] * M * p["ldo"])
            b["actZ"] = Buf((M + 2) * p["ldz"]).put(o[zkey][:M], p["ldz"])
            b["add"] = Buf((M + 2) * p["ldadd"]).put(o["add"][:M], p["ldadd"])
        else:
            sr = p["seg_rows"]
            nseg = M // sr if sr else 1
            b["dY"] = Buf(nseg * p["seg_dy"] if sr else (M + 2) * p["lddy"]).put(o["dY"][:M], p["lddy"], sr, p["seg_dy"])
            b["X"] = Buf(nseg * p["seg_x"] if sr else (M + 2) * p["ldx"], p["a8"]).put(o["X"][:M], p["ldx"], sr, p["seg_x"])
            b["dW"] = Buf(N * p["ldw"], p["a8"])
            b["db"] = Buf(N)
        for v in b.values():
            v.up()
        bufs.append(b)
    shadow = G.Case(case.id, case.kind, probs)
    structs = G.make_probs(D, shadow, addr=lambda name, i: bufs[i][name].ptr)
    st = _state(step)
    form, grid = D.gemm_f32_launch(case.kind, structs, st.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    planned = D.gemm_f32_plan(case.kind, G.make_probs(D, shadow))
    assert planned[1:3] == (form, grid), (case.id, planned, form, grid)      # made-up addresses and real ones choose alike
    outs = []
    for p, b in zip(probs, bufs):
        M, N, K, r = p["M"], p["N"], p["K"], {}
        if case.kind == "nt":
            if p["ksplit"] > 1:
                r["Yparts"], c1 = b["Y"].back(M, N, N, p["ksplit"])
            else:
                y, c1 = b["Y"].back(M, N, p["ldy"])
                r["Y"] = y[0]
            z, c2 = b["Z"].back(M, N if p["Z"] and p["ksplit"] == 1 else 0, p["ldz"])
            r["Z"] = z[0] if p["Z"] and p["ksplit"] == 1 else None
            r["clean"] = c1 and c2
        elif case.kind == "nn":
            o, r["clean"] = b["out"].back(M, K, p["ldo"], p["nsplit"])
            r["out"] = o if p["nsplit"] > 1 else o[0]
        else:
            w, c1 = b["dW"].back(N, K, p["ldw"])
            d, c2 = b["db"].back(1, N if p["db"] else 0, N)
            r["dW"], r["db"], r["clean"] = w[0], (d[0, 0] if p["db"] else None), c1 and c2
        outs.append(r)
    return form, outs, probs


def reference(case, i, p, mode):
    """float64: (the sum, the sum plus bias / add, |A| @ |B| + |bias or add|, contraction length)"""
    o, M = operands(case, i, mode), p["M"]
    if case.kind == "nt":
        S, mag, extra = o["X"][:M] @ o["W"].T, np.abs(o["X"][:M]) @ np.abs(o["W"]).T, (o["bias"][None, :] if p["bias"] and p["ksplit"] == 1 else 0.0)
    elif case.kind == "nn":
        S, mag, extra = o["dY"][:M] @ o["W"], np.abs(o["dY"][:M]) @ np.abs(o["W"]), (o["add"][:M] if p["add"] and p["nsplit"] == 1 else 0.0)
    else:
        S, mag, extra = o["dY"][:M].T @ o["X"][:M], np.abs(o["dY"][:M]).T @ np.abs(o["X"][:M]), 0.0
    return S, S + extra, mag + np.abs(extra), G.contraction(case.kind, p)


def _bits(a):
    return (np.asarray(a, dtype=np.float32) + np.float32(0.0)).view(np.uint32)      # (+ 0: -0 and +0 are the same answer)


def _sum_partials(parts, mode):
    """The consumer's sum of the ksplit / nsplit partial slabs.  Exact operands: in fp32, slab after slab (every partial sum is
    exact, so this is too).  Random operands: in float64, so that the host adds no rounding of its own and the bound stays the
    kernels' (L + 8) 2^-24 (...) with L the whole contraction length."""
    if mode == "exact":
        total = parts[0].copy()
        for s in range(1, len(parts)):
            total = total + parts[s]
        return total
    return parts.astype(np.float64).sum(0)


def _linear_outputs(case, i, p, r, mode):
    """[(name, device result, float64 reference, magnitude, L)] of the outputs that are linear in the operands"""
    S, lin, mag, L = reference(case, i, p, mode)
    o = operands(case, i, mode)
    if case.kind == "nt":
        if p["ksplit"] > 1:
            return [("Y partials summed", _sum_partials(r["Yparts"], mode), lin, mag, L)]
        out = [("Y", r["Y"], lin, mag, L)]
        if p["Z"]:
            out.append(("Z", r["Z"], lin, mag, L))
        return out
    if case.kind == "nn":
        if p["nsplit"] > 1:
            return [("out partials summed", _sum_partials(r["out"], mode), lin, mag, L)]
        return [("out", r["out"], lin, mag, L)]
    out = [("dW", r["dW"], lin, mag, L)]
    if p["db"]:
        out.append(("db", r["db"], o["dY"][:p["M"]].sum(0), np.abs(o["dY"][:p["M"]]).sum(0), L))
    return out


LINEAR = {"nt": {"act": 0, "drop": 0.0}, "nn": {"actZ": False, "drop": 0.0}, "tn": {}}


def test_exact_operands_give_bit_equal_linear_outputs_and_nothing_else_is_written():
    """(a) + (e): every case with its activation and mask switched off (the choice of the form looks at neither)."""
    per_form = {}
    for case in G.CASES:
        form, outs, probs = run(case, "exact", LINEAR[case.kind])
        for i, (p, r) in enumerate(zip(probs, outs)):
            assert r["clean"], f"{case.id}[{i}] ({form}): an element outside the logical panel was written"
            for name, got, ref, _, _ in _linear_outputs(case, i, p, r, "exact"):
                assert not np.isnan(got).any(), f"{case.id}[{i}] ({form}) {name}: NaN (an element not written, or a pad read)"
                want = ref.astype(np.float32)
                assert (want.astype(np.float64) == ref).all()
                bad = _bits(got) != _bits(want)
                assert not bad.any(), f"{case.id}[{i}] ({form}) {name}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0]}"
                per_form[form] = per_form.get(form, 0) + got.size
    for f in _D().GEMM_F32_FORMS:
        print(f"exact  {f:11s} {per_form.get(f, 0):8d} elements bit-equal to float64")
    assert set(per_form) == set(_D().GEMM_F32_FORMS)


def test_random_operands_stay_within_the_fp32_fma_chain_bound():
    """(b): a reduced-precision path (a bf16 or tf32-like product, a half-precision accumulate) is orders of magnitude outside."""
    worst = {}
    for case in G.CASES:
        form, outs, probs = run(case, "random", LINEAR[case.kind])
        for i, (p, r) in enumerate(zip(probs, outs)):
            assert r["clean"], (case.id, i)
            for name, got, ref, mag, L in _linear_outputs(case, i, p, r, "random"):
                assert not np.isnan(got).any(), (case.id, i, name)
                bound = (L + 8) * EPS * mag
                ratio = float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())
                worst[form] = max(worst.get(form, 0.0), ratio)
                assert ratio <= 1.0, f"{case.id}[{i}] ({form}) {name}: error {ratio:.3f} x the bound"
    for f in _D().GEMM_F32_FORMS:
        print(f"random {f:11s} worst error / bound {worst[f]:.4f}")


def _activation_errors(case, variant, zkey="actZ", mask=None):
    """errors of the activation epilogues of a case: ({form: max |Y - gelu64(Z)| / mult}, {form: max gradient-factor error})"""
    eo, eg = 0.0, 0.0
    form, outs, probs = run(case, "exact", variant, zkey=zkey)
    for i, (p, r) in enumerate(zip(probs, outs)):
        S, lin, _, _ = reference(case, i, p, "exact")
        mult = mask(i, p) if mask else None
        if case.kind == "nt" and p["act"] == 1 and p["ksplit"] == 1:
            want = gelu64(lin)
            if mult is not None:
                assert ((r["Y"] == 0) | (mult != 0)).all(), (case.id, i, "a dropped element is not 0")
                want = want * mult.astype(np.float64)
            slack = 0.0 if mult is None else EPS * np.abs(want)          # the multiplication by 1/(1-p) rounds once more
            eo = max(eo, float((np.maximum(0.0, np.abs(r["Y"] - want) - slack) / (1.0 if mult is None else float(mult.max()))).max()))
        if case.kind == "nn" and p["actZ"] and p["nsplit"] == 1:
            z = operands(case, i, "exact")[zkey][:p["M"]]
            f = gelu_grad64(z)
            if mult is not None:
                assert ((r["out"] == (operands(case, i, "exact")["add"][:p["M"]] if p["add"] else 0)) | (mult != 0) | (S == 0)).all(), (case.id, i)
                f = f * mult.astype(np.float64)
            want = S * f + (operands(case, i, "exact")["add"][:p["M"]] if p["add"] else 0.0)
            # one fp32 rounding of the result is not the factor's error: 2^-23 |want| is taken off before dividing by |S|
            slack = 2 * EPS * np.abs(want) + (0.0 if mult is None else EPS * np.abs(S * f))
            err = np.maximum(0.0, np.abs(r["out"] - want) - slack) / np.maximum(np.abs(S), 1.0 / 16) / (1.0 if mult is None else float(mult.max()))
            eg = max(eg, float(err.max()))
    return form, eo, eg


def test_activation_epilogues_against_float64_gelu():
    """(c): the measured errors per form next to their bounds."""
    out, grad = {}, {}
    for case in G.CASES:
        if case.kind == "tn" or not any(p.get("act") == 1 or p.get("actZ") for p in case.probs):
            continue
        form, eo, eg = _activation_errors(case, {"drop": 0.0})
        out[form], grad[form] = max(out.get(form, 0.0), eo), max(grad.get(form, 0.0), eg)
    for f in _D().GEMM_F32_FORMS[:10]:
        kind, e, b = ("gelu   max |Y - gelu64(Z)|", out[f], BOUND_GELU) if f.startswith("nt") else ("gelu'  max factor error  ", grad[f], BOUND_GRAD)
        print(f"activation {f:8s} {kind} {e:.3e}   bound {b:.3e}")
    print(f"activation: measured gelu {max(out.values()):.3e} gelu' {max(grad.values()):.3e}; bounds {BOUND_GELU:.3e} / {BOUND_GRAD:.3e}")
    assert BOUND_GELU <= TOL_OUT and BOUND_GRAD <= TOL_GRAD
    assert max(v for f, v in out.items() if f.startswith("nt")) <= BOUND_GELU, out
    assert max(v for f, v in grad.items() if f.startswith("nn")) <= BOUND_GRAD, grad


_MASKS = {}


def _mirror(p, i, rows, cols, ld, step=STEP):
    key = (p["drop"], i, rows, cols, ld, step)
    if key not in _MASKS:
        _MASKS[key] = DM.multipliers(SEED, step, G.DROP_LAYER + i, p["drop"], rows, cols, ld)
    return _MASKS[key]


def test_dropout_masks_sit_at_the_documented_element_index():
    """(d): nt draws at m N + n, nn at m drop_ld + k; exact operands, so kept elements are fp32(exact) * 1/(1-p) to the bit."""
    agree = {}          # form -> [elements, wrong under the next step's masks, elements with a wrong-stride control, wrong under it]

    def tally(form, got, base, i, p, rows, cols, ld, wrong_ld):
        want = (base * _mirror(p, i, rows, cols, ld)).astype(np.float32)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), f"{form} problem {i}: {int(bad.sum())} of {bad.size} elements differ from the mirror's mask, first at {np.argwhere(bad)[0]}"
        assert (got[_mirror(p, i, rows, cols, ld) == 0] == 0).all()
        t = agree.setdefault(form, [0, 0, 0, 0])
        t[0] += got.size
        t[1] += int((_bits(got) != _bits(base * _mirror(p, i, rows, cols, ld, STEP + 1))).sum())
        if wrong_ld != ld and rows > 1:
            t[2] += got.size
            t[3] += int((_bits(got) != _bits(base * _mirror(p, i, rows, cols, wrong_ld))).sum())

    for case in G.CASES:
        if case.kind == "tn" or not any(p["drop"] > 0 for p in case.probs):
            continue
        if case.kind == "nt":
            form, outs, probs = run(case, "exact", {"act": 0})
            for i, (p, r) in enumerate(zip(probs, outs)):
                if p["drop"] > 0:
                    base = reference(case, i, p, "exact")[1].astype(np.float32)
                    tally(form, r["Y"], base, i, p, p["M"], p["N"], p["N"], p["ldy"])
                    if p["Z"]:
                        assert (_bits(r["Z"]) == _bits(base)).all(), (case.id, i, "Z is the pre-activation, before the mask")
        else:
            # gelu'(0) = 1/2 and gelu'(8) = 1 exactly in fp32 (erff(0) = 0, erff(5.66) = 1, 8 pdf(8) < 2^-24): S g is exact
            form, outs, probs = run(case, "exact", {"add": False}, zkey="flat")
            for i, (p, r) in enumerate(zip(probs, outs)):
                if p["drop"] > 0:
                    g = np.where(operands(case, i, "exact")["flat"][:p["M"]] == 8.0, 1.0, 0.5)
                    base = (reference(case, i, p, "exact")[0] * g).astype(np.float32)
                    tally(form, r["out"], base, i, p, p["M"], p["K"], p["drop_ld"], p["ldo"])
        # the case as it stands (GELU and mask together, add after the mask), within the activation bounds
        f2, eo, eg = _activation_errors(case, None, mask=lambda i, p: _mirror(p, i, p["M"], p["N"] if case.kind == "nt" else p["K"],
                                                                              p["N"] if case.kind == "nt" else p["drop_ld"]))
        print(f"dropout {case.id:24s} as it stands ({f2}): gelu error {eo:.3e}, gelu' factor error {eg:.3e}")
        assert f2 == form and eo <= BOUND_GELU and eg <= BOUND_GRAD, (case.id, eo, eg)
    for f in _D().GEMM_F32_FORMS[:10]:
        n, nxt, ns, ws = agree[f]
        print(f"dropout {f:8s} {n:7d} elements on the mirror's mask; next step's mask differs on {nxt / n:.3f}, "
              f"the output-stride index on {ws / max(ns, 1):.3f} of {ns}")
        assert nxt >= 0.25 * n and ns > 0 and ws >= 0.25 * ns, (f, agree[f])


def test_nn4_mask_is_the_same_at_aligned_and_unaligned_drop_ld():
    """nn_kernel<4> draws four multipliers with one Philox evaluation when drop_ld % 4 == 0 and element by element otherwise:
    one problem, the same operands, both strides, each on the mirror's mask (so the two agree wherever the indices do)."""
    case = G.BY_ID["nn4_group_k4100"]
    for ld in (4100, 4104, 4101, 4102, 4103):
        form, outs, probs = run(case, "exact", {"add": False, "drop_ld": ld}, zkey="flat")
        assert form == "nn<4>"
        for i, (p, r) in enumerate(zip(probs, outs)):
            if p["drop"] > 0:
                g = np.where(operands(case, i, "exact")["flat"][:p["M"]] == 8.0, 1.0, 0.5)
                base = (reference(case, i, p, "exact")[0] * g).astype(np.float32)
                assert (_bits(r["out"]) == _bits(base * _mirror(p, i, p["M"], p["K"], ld))).all(), (ld, i)
    # row 0 has the same indices at every stride: the vector path and the scalar path drew the same words
    a = run(case, "exact", {"add": False, "drop_ld": 4100}, zkey="flat")[1][0]["out"][0]
    b = run(case, "exact", {"add": False, "drop_ld": 4102}, zkey="flat")[1][0]["out"][0]
    assert (_bits(a) == _bits(b)).all()


def test_row_zero_does_not_depend_on_the_batch_it_is_computed_in():
    """(f): launch_nt's promise -- random operands, every nt case (so every nt form) and every nn case at 1, 33 and 65 rows."""
    seen = {}
    for case in G.CASES:
        if case.kind == "tn":
            continue
        rows = {}
        for M in (1, 33, 65):
            form, outs, probs = run(case, "random", {"M": M})
            seen.setdefault(case.id, []).append(form)
            for i, (p, r) in enumerate(zip(probs, outs)):
                assert r["clean"], (case.id, M, i)
                key = "Yparts" if "Yparts" in r else ("Y" if case.kind == "nt" else "out")
                row = r[key][..., 0, :]
                assert not np.isnan(row).any()
                rows.setdefault(i, []).append(row)
                if r.get("Z") is not None:
                    rows.setdefault((i, "Z"), []).append(r["Z"][0])
        for k, v in rows.items():
            assert (v[0].view(np.uint32) == v[1].view(np.uint32)).all() and (v[0].view(np.uint32) == v[2].view(np.uint32)).all(), (case.id, k, seen[case.id])
    for cid, f in seen.items():
        print(f"batch  {cid:24s} rows 1 / 33 / 65 on {f}: row 0 bit-equal")
    nt_forms = {f for cid, fs in seen.items() if G.BY_ID[cid].kind == "nt" for f in fs}
    assert nt_forms == set(_D().GEMM_F32_FORMS[:6]), nt_forms
