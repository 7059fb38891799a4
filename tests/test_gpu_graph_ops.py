"""The graph side (csrc/gcn.hip) and the temporal side (csrc/tcn.hip, csrc/temporal.hip) through the C ABI against the float64
references of tests/graph_ops_cases.py, case by case: exact families bit for bit, ufnd_node_features against its derived bound,
the composite entries within 3 x the float32 restatement's own distance from float64 on the same input.

Every call gets a workspace and outputs filled with NaN, and NaN beyond N / Dv / the slice width wherever an input has a row
stride: no NaN may come out (tests.frozen_ops_cases.worst_ratio is inf for one).  Every test prints its figures before it asserts;
tools/graph_ops_errors.py collects them into profiles/graph_ops_errors.txt.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import graph_ops_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _L():
    from ultrafnd_git_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _strided(a, extra):
    """(R, C) -> a device (R, C + extra) buffer, NaN beyond C."""
    a = np.asarray(a, dtype=np.float32)
    buf = np.full((a.shape[0], a.shape[1] + extra), np.nan, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return _dev(buf)


def _host(t):
    return t.detach().cpu().numpy()


def _state(step=G.DROP_STEP):
    from ultrafnd_git_amd.state import StepStateBuffer
    st = StepStateBuffer(torch.device(DEV), seed=G.DROP_SEED)
    st.set_u64("step", step)
    return st


@functools.lru_cache(maxsize=None)
def inp_ref(op, i):
    case = G.OPS[op].cases[i]
    inp = G.OPS[op].make(case)
    return inp, G.reference(op, case, inp)


def _flat_params(inp):
    L = _L()
    flat = _dev(np.concatenate([inp[k].ravel() for k in ("w1", "b1", "w2", "b2")]))
    p, off = L.GcnParams(), 0
    for k in ("w1", "b1", "w2", "b2"):
        setattr(p, k, flat.data_ptr() + 4 * off)
        off += inp[k].size
    return flat, p


# ---------------------------------------------------------------------------------------------------------------------
# runners: one call (or one forward + backward) through the C ABI, outputs as host arrays
def run_gnn(case, inp, ws=None):
    L = _L()
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    N, kind, F, hid, od, ldx, fam = case
    x, adj, dz = _dev(inp["x"]), _strided(inp["adj"], ldx), _dev(inp["d_z"])
    flat, p = _flat_params(inp)
    need = lib.ufnd_gnn_workspace_floats(N, F, hid, od)
    if ws is None:
        ws = _nan(need)
    assert ws.numel() >= need
    z, g = _nan(N, od), _nan(flat.numel())
    drop = G.DROP_P if fam == "dropout" else 0.0
    st = _state() if drop else None
    sp = st.ptr if st else None
    L.check(lib.ufnd_gnn_forward(x.data_ptr(), adj.data_ptr(), N + ldx, C.byref(p), z.data_ptr(), ws.data_ptr(), N, F, hid, od, drop, sp, s), "ufnd_gnn_forward")
    o1, o2, o3 = hid * F, hid * F + hid, hid * F + hid + od * hid
    gp = g.data_ptr()
    L.check(lib.ufnd_gnn_backward(x.data_ptr(), C.byref(p), gp, gp + 4 * o1, gp + 4 * o2, gp + 4 * o3, dz.data_ptr(), ws.data_ptr(), N, F, hid, od, drop, sp, s),
            "ufnd_gnn_backward")
    torch.cuda.synchronize()
    g = _host(g)
    return {"z": _host(z), "g_w1": g[:o1].reshape(hid, F), "g_b1": g[o1:o2], "g_w2": g[o2:o3].reshape(od, hid), "g_b2": g[o3:]}


def run_gcn_pretrain(case, inp, ws=None):
    L = _L()
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    N, kind, F, hid, od, ldx, variant = case
    x, adj = _dev(inp["x"]), _strided(inp["adj"], ldx)
    flat, p = _flat_params(inp)
    m, v, hw, hb = _dev(inp["m"]), _dev(inp["v"]), _dev(inp["head_w"]), _dev(inp["head_b"])
    need = lib.ufnd_gcn_workspace_floats(N, F, hid, od, 1)
    ws, z, loss = _nan(need) if ws is None else ws, _nan(N, od), _nan(1)
    assert ws.numel() >= need
    L.check(lib.ufnd_gcn_pretrain_step(x.data_ptr(), adj.data_ptr(), N + ldx, C.byref(p), m.data_ptr(), v.data_ptr(), hw.data_ptr(), hb.data_ptr(), z.data_ptr(),
                                       ws.data_ptr(), N, F, hid, od, 0.0, G.GCN_LR, inp["wd"], inp["step"], None, loss.data_ptr(), s), "ufnd_gcn_pretrain_step")
    torch.cuda.synchronize()
    return {"z": _host(z), "loss": _host(loss), "params": _host(flat), "exp_avg": _host(m), "exp_avg_sq": _host(v)}


def run_gcn_forward(case, inp):
    L = _L()
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    N, kind, F, hid, od, ldx, variant = case
    x, adj = _dev(inp["x"]), _strided(inp["adj"], ldx)
    flat, p = _flat_params(inp)
    ws, z = _nan(lib.ufnd_gcn_workspace_floats(N, F, hid, od, 0)), _nan(N, od)
    L.check(lib.ufnd_gcn_forward(x.data_ptr(), adj.data_ptr(), N + ldx, C.byref(p), z.data_ptr(), ws.data_ptr(), N, F, hid, od, 0.0, None, s), "ufnd_gcn_forward")
    torch.cuda.synchronize()
    return {"z": _host(z)}


def run_node_features(case, inp):
    L = _L()
    w, B = case
    bufs = [_strided(p, e) for p, e in zip(inp["parts"], G.NF_LD_EXTRA)]
    out = _nan(B, sum(w))
    args = []
    for b in bufs:
        args += [b.data_ptr(), b.shape[1]]
    L.check(L.lib().ufnd_node_features(*args, *w, B, out.data_ptr(), L.stream_ptr(torch.device(DEV))), "ufnd_node_features")
    torch.cuda.synchronize()
    return {"out": _host(out)}


def run_temporal_align(case, inp, w0=None):
    L = _L()
    lib = L.lib()
    D, Dv, B = case
    ld = lib.ufnd_temporal_weight_ld(D)
    assert ld % 4 == 0 and 4 * D + 1 <= ld < 4 * D + 5
    w0p = np.zeros((G.TA_HIDDEN, ld), dtype=np.float32)
    w0p[:, :4 * D + 1] = inp["w0"] if w0 is None else w0
    v = inp["v"].copy()
    if Dv > D:
        v[:, D:] = np.nan                                            # truncated columns are never read
    t, v, w0d, b0, w3, b3 = (_dev(a) for a in (inp["t"], v, w0p, inp["b0"], inp["w3"], inp["b3"]))
    ws, out = _nan(lib.ufnd_temporal_workspace_floats(B, D, G.TA_HIDDEN)), _nan(B, G.TA_OUT)
    L.check(lib.ufnd_temporal_align(t.data_ptr(), v.data_ptr(), w0d.data_ptr(), b0.data_ptr(), w3.data_ptr(), b3.data_ptr(), ws.data_ptr(), out.data_ptr(), B, D, Dv,
                                    G.TA_HIDDEN, G.TA_OUT, 0.0, None, L.stream_ptr(torch.device(DEV))), "ufnd_temporal_align")
    torch.cuda.synchronize()
    return {"out": _host(out)}


def run_tcn(case, inp, rows=None):
    """rows: a slice of the batch (clips run alone for the batch-invariance check)."""
    L = _L()
    lib = L.lib()
    td, vd, hid, k, layers, T, B, mode, edge = case
    text, vis = inp["text"], inp["vis"]
    if rows is not None:
        text, vis, B = text[rows], vis[rows], len(range(*rows.indices(B)))
    keep, arr, ch = [], (L.TcnLayer * layers)(), td + vd
    for i, ly in enumerate(inp["layers"]):
        ld = lib.ufnd_tcn_weight_ld(ch, k)
        w = np.zeros((hid, ld), dtype=np.float32)
        w[:, :k * ch] = ly["w"].reshape(hid, k * ch)                 # tap-major: w[h][j * ch + c]
        t = {n: _dev(a) for n, a in (("w", w), ("b", ly["b"]), ("gamma", ly["gamma"]), ("beta", ly["beta"]), ("running_mean", ly["rm"]), ("running_var", ly["rv"]))}
        keep.append(t)
        for n, d in t.items():
            setattr(arr[i], n, d.data_ptr())
        ch = hid
    tx, vx, hw, hb = _dev(text), _dev(vis), _dev(inp["head_w"]), _dev(inp["head_b"])
    ws, out = _nan(lib.ufnd_tcn_workspace_floats(B, T, td + vd, hid, k)), _nan(B, G.TCN_OUT)
    drop = G.DROP_P if mode == "dropout" else 0.0
    st = _state() if drop else None
    L.check(lib.ufnd_tcn_forward(tx.data_ptr(), td, vx.data_ptr(), vd, B, T, arr, layers, k, hid, hw.data_ptr(), hb.data_ptr(), G.TCN_OUT, int(mode != "eval"), drop,
                                 G.TCN_MOMENTUM, G.TCN_EPS, st.ptr if st else None, ws.data_ptr(), out.data_ptr(), L.stream_ptr(torch.device(DEV))), "ufnd_tcn_forward")
    torch.cuda.synchronize()
    got = {"out": _host(out)}
    for i, t in enumerate(keep):
        if mode != "eval":
            got[f"running_mean{i}"], got[f"running_var{i}"] = _host(t["running_mean"]), _host(t["running_var"])
        else:
            assert np.array_equal(_host(t["running_mean"]), inp["layers"][i]["rm"]) and np.array_equal(_host(t["running_var"]), inp["layers"][i]["rv"])
    return got


RUN = {"gnn": run_gnn, "gcn_pretrain": run_gcn_pretrain, "node_features": run_node_features, "temporal_align": run_temporal_align, "tcn": run_tcn}


def figures_of(op, i, got=None):
    case = G.OPS[op].cases[i]
    inp, refs = inp_ref(op, i)
    got = RUN[op](case, inp) if got is None else got
    return case, got, G.figures(op, case, got, refs)


def _hold(op, i, got=None, tag=""):
    case, got, fig = figures_of(op, i, got)
    for k, (err, bound, ratio) in fig.items():
        print(f"GRAPH_OPS_ERR {op}{tag} {G.case_id(case)} {k} gpu={err:.3e} bound={bound:.3e} ratio={ratio:.3g}")
    bad = {k: v for k, v in fig.items() if not v[2] <= 1.0}
    assert not bad, (op, case, bad)
    return got


def _ids(op):
    return [G.case_id(c) for c in G.OPS[op].cases]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(G.OPS["gnn"].cases)), ids=_ids("gnn"))
def test_gnn_forward_and_backward_against_float64(i):
    """Every graph kind at every N, ld_adj = N and N + 3; the exact family and ReLU-at-zero bit for bit; the dropout cases against the
    reference run with the mirror's masks (tag 10, element row * hid + col), forward and backward on the same key."""
    _hold("gnn", i)


def test_gnn_stale_pad_rows_in_a_reused_workspace():
    """N = 65, then N = 33 in the same workspace: the second call's pad rows lie where the first left its values."""
    cases = G.OPS["gnn"].cases
    big = next(i for i, c in enumerate(cases) if c[0] == 65 and c[3] == 96 and c[6] == "normal")
    small = next(i for i, c in enumerate(cases) if c[0] == 33 and c[3] == 96 and c[2] == cases[big][2] and c[6] == "normal")
    c = cases[big]
    ws = _nan(_L().lib().ufnd_gnn_workspace_floats(c[0], c[2], c[3], c[4]))
    _hold("gnn", big, run_gnn(c, inp_ref("gnn", big)[0], ws), tag=".shared_ws")
    _hold("gnn", small, run_gnn(cases[small], inp_ref("gnn", small)[0], ws), tag=".stale_ws")


@pytest.mark.parametrize("i", [i for i, c in enumerate(G.OPS["gnn"].cases) if c[6] == "dropout"])
def test_gnn_dropout_negative_controls(i):
    """The GPU's train-mode outputs are far from the reference run with the next step's masks, with a row stride of hid + 4, and with
    the GCN's tag: each puts at least a quarter of the elements outside the bound."""
    case = G.OPS["gnn"].cases[i]
    inp, refs = inp_ref("gnn", i)
    got = run_gnn(case, inp)
    for what, kw in (("next step", dict(step=G.DROP_STEP + 1)), ("row stride hid + 4", dict(ld=case[3] + 4)), ("the GCN's tag", dict(tag=9))):
        bad = G.OPS["gnn"].restate(case, inp, G.F64, None, G.gnn_muls(case, **kw))
        for k in ("z", "g_w1", "g_w2"):
            frac = G.outside_fraction(got[k], bad[k], refs[k][1])
            print(f"GRAPH_OPS_CONTROL gnn {G.case_id(case)} {what}: {k} outside the bound on {frac:.3f}")
            assert frac >= 0.25, (case, what, k, frac)


@functools.lru_cache(maxsize=None)
def _pretrain(i):
    case = G.OPS["gcn_pretrain"].cases[i]
    return run_gcn_pretrain(case, inp_ref("gcn_pretrain", i)[0])


@pytest.mark.parametrize("i", range(len(G.OPS["gcn_pretrain"].cases)), ids=_ids("gcn_pretrain"))
def test_gcn_pretrain_step_against_float64(i):
    """z, the parameters and both Adam moments after one step (the gradient is exp_avg / (1 - beta1) at step 1 without weight decay);
    steps 2 and 1000, L2 weight decay, and the saturated head, where every moment is exactly 0 and the parameters keep their bits."""
    got = _hold("gcn_pretrain", i, _pretrain(i))
    assert math.isfinite(float(got["loss"][0]))


def test_gcn_pretrain_stale_pad_rows_in_a_reused_workspace():
    cases = G.OPS["gcn_pretrain"].cases
    big = next(i for i, c in enumerate(cases) if c[0] == 65 and c[3] == 96)
    small = next(i for i, c in enumerate(cases) if c[0] == 33 and c[3] == 96 and c[2] == cases[big][2] and c[6] == "step1")
    c = cases[big]
    ws = _nan(_L().lib().ufnd_gcn_workspace_floats(c[0], c[2], c[3], c[4], 1))
    _hold("gcn_pretrain", big, run_gcn_pretrain(c, inp_ref("gcn_pretrain", big)[0], ws), tag=".shared_ws")
    _hold("gcn_pretrain", small, run_gcn_pretrain(cases[small], inp_ref("gcn_pretrain", small)[0], ws), tag=".stale_ws")


def test_gcn_pretrain_losses_over_the_table():
    n = len(G.OPS["gcn_pretrain"].cases)
    got = [float(_pretrain(i)["loss"][0]) for i in range(n)]
    ratio = G.loss_table_ratio(got, [inp_ref("gcn_pretrain", i)[1] for i in range(n)])
    print(f"GRAPH_OPS_ERR gcn_pretrain table loss ratio={ratio:.3g}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("i", [i for i, c in enumerate(G.OPS["gcn_pretrain"].cases) if c[6] == "step1"], ids=[G.case_id(c) for c in G.OPS["gcn_pretrain"].cases if c[6] == "step1"])
def test_gcn_forward_against_float64(i):
    case = G.OPS["gcn_pretrain"].cases[i]
    inp, refs = inp_ref("gcn_pretrain", i)
    got = run_gcn_forward(case, inp)
    err, bound, ratio = G.figures("gcn_pretrain", case, got, {"z": refs["z"]})["z"]
    print(f"GRAPH_OPS_ERR gcn_forward {G.case_id(case)} z gpu={err:.3e} bound={bound:.3e} ratio={ratio:.3g}")
    assert ratio <= 1.0, (case, ratio)
    assert np.array_equal(got["z"], _pretrain(i)["z"]), "the step's forward is the eval forward at p = 0, bit for bit"


@pytest.mark.parametrize("i", range(len(G.OPS["node_features"].cases)), ids=_ids("node_features"))
def test_node_features_against_the_derived_bound(i):
    got = _hold("node_features", i)
    if G.OPS["node_features"].cases[i][1] >= 4:
        assert not got["out"][1].any(), "a zero row gives exact zeros"


@pytest.mark.parametrize("i", range(len(G.OPS["temporal_align"].cases)), ids=_ids("temporal_align"))
def test_temporal_align_against_float64(i):
    """Eval mode.  On rows whose text or visual part is zero the cosine is exactly 0, so the weights of the cosine's column cannot
    reach the output: those rows keep their bits when that column of W0 is replaced (every other row changes)."""
    case = G.OPS["temporal_align"].cases[i]
    inp, _ = inp_ref("temporal_align", i)
    got = _hold("temporal_align", i)
    D = case[0]
    w0 = inp["w0"].copy()
    w0[:, 4 * D] = -3.0 * w0[:, 4 * D] + 0.5
    other = run_temporal_align(case, inp, w0)
    for r, kind in enumerate(G.ta_row_kinds(case[2])):
        same = np.array_equal(got["out"][r], other["out"][r])
        assert same == ("zero" in kind), (case, r, kind)


@pytest.mark.parametrize("i", range(len(G.OPS["tcn"].cases)), ids=_ids("tcn"))
def test_tcn_forward_against_float64(i):
    """Eval and train mode (the running statistics after the call included); the dropout cases against the reference run with the
    mirror's masks (tags 16 + layer, element m * hid + c; the six-layer case pins tag 21).  Eval: clip b alone gives the bits it
    gives in the batch -- no tap reaches into a neighbouring clip at any dilation."""
    case = G.OPS["tcn"].cases[i]
    got = _hold("tcn", i)
    if case[7] == "eval" and case[6] > 1:
        inp, _ = inp_ref("tcn", i)
        for b in range(case[6]):
            alone = run_tcn(case, inp, rows=slice(b, b + 1))["out"]
            assert np.array_equal(alone[0], got["out"][b]), (case, b)


@pytest.mark.parametrize("i", [i for i, c in enumerate(G.OPS["tcn"].cases) if c[7] == "dropout"])
def test_tcn_dropout_negative_controls(i):
    case = G.OPS["tcn"].cases[i]
    inp, refs = inp_ref("tcn", i)
    got = run_tcn(case, inp)
    for what, kw in (("next step", dict(step=G.DROP_STEP + 1)), ("row stride hid + 4", dict(ld=case[2] + 4)), ("next layer's tag", dict(shift=1))):
        bad = G.OPS["tcn"].restate(case, inp, G.F64, None, G.tcn_muls(case, **kw))
        frac = G.outside_fraction(got["out"], bad["out"], refs["out"][1])
        print(f"GRAPH_OPS_CONTROL tcn {G.case_id(case)} {what}: out outside the bound on {frac:.3f}")
        assert frac >= 0.25, (case, what, frac)


@pytest.mark.parametrize("N", G.ADJ_N)
def test_ocr_adjacencies_at_the_lds_window_and_at_a_jaccard_on_the_threshold(N):
    """Sets of exactly 2048 and 2049 phrases, N on both sides of the 256-thread column loop, and a pair whose Jaccard is exactly 1 / 3
    at thresh = 1 / 3: the unweighted form's + 1e-9 rejects it, the weighted form keeps it.  Bit for bit, ld = N + 3."""
    from ultrafnd_git_amd.gcn import sets_to_csr
    L = _L()
    lib, s = L.lib(), L.stream_ptr(torch.device(DEV))
    sets = G.adjacency_sets(N)
    offs, toks = sets_to_csr(sets)
    o, t = _dev(offs), _dev(toks)
    ref_a, ref_w = G.adjacency_refs(sets, G.ADJ_THRESH)
    assert ref_a[3, 4] == 0 and ref_w[3, 4] == np.float32(1 / 3)
    for name, fn, ref in (("ufnd_ocr_adjacency", lib.ufnd_ocr_adjacency, ref_a), ("ufnd_ocr_adjacency_weighted", lib.ufnd_ocr_adjacency_weighted, ref_w)):
        adj = _nan(N, N + 3)
        L.check(fn(o.data_ptr(), t.data_ptr(), N, G.ADJ_THRESH, adj.data_ptr(), N + 3, s), name)
        torch.cuda.synchronize()
        got = _host(adj)
        assert np.array_equal(got[:, :N], ref), name
        assert np.isnan(got[:, N:]).all(), name
