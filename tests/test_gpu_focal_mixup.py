"""GPU: the raw-data trainer's recipe -- ufnd_softmax_focal, ufnd_gather_mix_rows and the trainer paths that use them.

  * the criterion, every case of tests/focal_cases.py through the C ABI, against the float64 reference and its derived bounds
    (the buffers between sentinel pads, read-only inputs unchanged, of the state only `loss` written, the forward-only arm);
  * bit anchors: gamma = 0, alpha = 1 without labels_b IS ufnd_softmax_ce, bit for bit; mix = (1, 0) with any labels_b gives the
    values of labels_b = NULL;
  * tests/golden/recipe.npz (the reference's own FocalLoss / mixup_criterion / mixup_data) within the device bound plus the
    reference's own cancellation in 1 - exp(-ce);
  * the mixing gather, bit for bit against the torch CPU expression lam * x + (1 - lam) * x[index, :], alone = rerun, lam = 1 = the
    plain gather;
  * ForensicTrainer on a synthetic cache: three steps against the oracle composed of oracle.tier_a.forward_batch, the criterion in
    torch, autograd, clip_grads_ and AdamWState, with the same draws on both sides; captured graph = eager with a different
    (lam, permutation) every step; two runs leave the same bits; a forced one-rank exchange changes none; validation and test
    never mix.
Each test prints its worst figure; tools/focal_mixup_errors.py collects them into profiles/focal_mixup_errors.txt."""
import json
import socket
import sys

import numpy as np
import pytest
import torch

from tests import focal_cases as F
from tests.helpers import digest, load_npz
from tests.test_gpu_step_tail import Buf, State, _lib, _ok, _s, _same_bits, fresh

pytestmark = pytest.mark.gpu
DEV = "cuda"
OP = F.OPS["focal"]


# ---------------------------------------------------------------------------------------------------------------------
def focal_call(lg, ya, yb, mix, B, alpha, gamma, rows, d, st):
    lib = _lib().lib()
    p = lambda b: None if b is None else b.ptr
    _ok(lib.ufnd_softmax_focal(lg.ptr, ya.ptr, p(yb), p(mix), B, alpha, gamma, p(rows), p(d), st.ptr, _s()), "ufnd_softmax_focal")
    torch.cuda.synchronize()
    for b in (lg, ya, yb, mix):
        if b is not None:
            b.unchanged()
    return st.get(("loss",)).loss


def run_focal(logits, ya, yb, mix, alpha, gamma):
    """every output of one call, after the forward-only arm has produced the same loss"""
    B = ya.size
    lg, a = Buf(logits, 148 if B % 2 else 64), Buf(ya)
    b, m = (None, None) if yb is None else (Buf(yb), Buf(mix))
    rows, d = fresh(B), fresh(2 * B)
    loss = focal_call(lg, a, b, m, B, alpha, gamma, rows, d, State())
    loss2 = focal_call(lg, a, b, m, B, alpha, gamma, None, None, State(loss=-5.0))
    assert _same_bits([loss], [loss2]), ("state->loss differs without the outputs", loss, loss2)
    return dict(loss_rows=rows.read().copy(), loss=np.array([float(loss)]), d_logits=d.read().copy().reshape(B, 2))


def run_case(case, inp):
    return F.with_zero_rows(case, inp, run_focal(inp["logits"], inp["labels_a"], inp["labels_b"], inp["mix"], case[1][0], case[1][1]))


@pytest.mark.parametrize("B", F.FOCAL_B)
def test_criterion_against_float64(B):
    worst = (-1.0, None, None)
    for case in (c for c in OP.cases if c[0] == B):
        inp = OP.make(case)
        for k, r in F.check(case, inp, run_case(case, inp)).items():
            if r > worst[0]:
                worst = (r, case, k)
    print(f"focal B={B}: worst error / bound {worst[0]:.3g} at {worst[1]} ({worst[2]})")
    assert worst[0] <= 1.0, worst


def test_every_case_of_the_table_is_run():
    assert sorted({c[0] for c in OP.cases}) == sorted(F.FOCAL_B) and len(OP.cases) >= 9 * 18


def test_gamma_zero_is_the_cross_entropy_entry_bit_for_bit():
    from tests import step_tail_cases as S
    lib = _lib().lib()
    for B in (1, 65, 257, 1000):
        for kind in ("randn2", "one_of_each", "grid_shifted"):
            inp = S.OPS["cross_entropy"].make((B, "mixed", None, kind))
            lg, y, rows, d, st = Buf(inp["logits"]), Buf(inp["labels"]), fresh(B), fresh(2 * B), State()
            _ok(lib.ufnd_softmax_ce(lg.ptr, y.ptr, B, rows.ptr, d.ptr, st.ptr, _s()), "ufnd_softmax_ce")
            torch.cuda.synchronize()
            ce = dict(loss_rows=rows.read().copy(), loss=np.array([float(st.get(("loss",)).loss)]), d_logits=d.read().copy().reshape(B, 2))
            fo = run_focal(inp["logits"], inp["labels"], None, None, 1.0, 0.0)
            for k in ce:
                assert _same_bits(ce[k], fo[k]), (B, kind, k)


def test_mix_one_zero_gives_the_values_of_no_mixup():
    for i, case in enumerate(OP.cases):
        if case[0] not in (2, 65, 257) or case[4] is not None:
            continue
        inp = OP.make(case)
        plain = run_focal(inp["logits"], inp["labels_a"], None, None, *case[1])
        yb = np.random.default_rng(i).integers(0, 2, case[0]).astype(np.int64)
        mixed = run_focal(inp["logits"], inp["labels_a"], yb, F.mix_of(1.0), *case[1])
        for k in plain:
            assert np.array_equal(plain[k], mixed[k]), (case, k)      # as values: 1 x + 0 y = x (a zero may change its sign)


def test_reference_fixture():
    z = load_npz("recipe.npz")
    lg, ya, yb, m = z["focal/logits"], z["focal/labels_a"], z["focal/labels_b"], z["focal/moderate"]
    worst = {}
    for k, (alpha, gamma) in enumerate(z["focal/alpha_gamma"]):
        for mixed in (False, True):
            mix = F.mix_of(float(z["focal/lam"])) if mixed else None
            a = run_focal(lg, ya, yb if mixed else None, mix, float(alpha), float(gamma))
            b = run_focal(lg[m], ya[m], yb[m] if mixed else None, mix, float(alpha), float(gamma))
            for key, r in F.fixture_checks(z, k, a["loss_rows"], float(a["loss"][0]), b["d_logits"], mixed).items():
                worst[key] = max(worst.get(key, 0.0), r)
    print("device against the reference fixture, error / (device bound + reference error):", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (768, 512, 256, 128, 2)      # floats per row: the step's text / visual / temporal / audio (and gnn) / aux rows
SRC_ROWS = 41


def perms_of(B, rng):
    ident = np.arange(B)
    fixed = ident.copy()
    if B >= 3:
        fixed[:B // 2] = rng.permutation(B // 2)           # the upper half stays in place
    return {"identity": ident, "reversal": ident[::-1].copy(), "one_cycle": np.roll(ident, 1), "fixed_points": fixed}


def gather_mix(idx, perms, mixes, sources, groups, B):
    """one ufnd_gather_mix_rows launch over `sources` ([(array, kind)]) -> the destinations (labels: a pair), pads checked"""
    L = _lib()
    I, P, M = Buf(idx.astype(np.int64)), Buf(np.ascontiguousarray(perms, dtype=np.int64)), Buf(np.ascontiguousarray(mixes, dtype=np.float32))
    src = [Buf(a) for a, _ in sources]
    dst = [Buf(np.full((B,) + a.shape[1:], 77, dtype=a.dtype)) for a, _ in sources]
    dst_b = [Buf(np.full(B, 77, dtype=np.int64)) if kind else None for _, kind in sources]
    items = (L.MixItem * len(sources))()
    for it, (a, kind), s, d, db, g in zip(items, sources, src, dst, dst_b, groups):
        it.src, it.dst, it.dst_b = s.ptr, d.ptr, None if db is None else db.ptr
        it.row_bytes, it.src_rows, it.kind, it.group = a[0].size * a.itemsize, a.shape[0], kind, g
    _ok(L.lib().ufnd_gather_mix_rows(I.ptr, P.ptr, M.ptr, B, items, len(sources), len(mixes), _s()), "ufnd_gather_mix_rows")
    torch.cuda.synchronize()
    for b in [I, P, M] + src:
        b.unchanged()
    return [d.read().copy().reshape((B,) + a.shape[1:]) if db is None else (d.read().copy(), db.read().copy())
            for (a, _), d, db in zip(sources, dst, dst_b)]


def torch_mix(x, idx, perm, lam):
    """mixup_data's expression on the CPU, on the gathered rows"""
    xt = torch.from_numpy(x)[torch.from_numpy(idx)]
    return (lam * xt + (1 - lam) * xt[torch.from_numpy(perm), :]).numpy()


@pytest.mark.parametrize("B", [1, 3, 64, 257])
def test_gather_mix_equals_the_torch_expression_bit_for_bit(B):
    rng = np.random.default_rng(B)
    data = [(rng.normal(0, 1, (SRC_ROWS, w)) * 10.0 ** rng.integers(-3, 4, (SRC_ROWS, w))).astype(np.float32) for w in WIDTHS]
    labels = rng.integers(0, 2, SRC_ROWS).astype(np.int64) * 0x100000001 + np.arange(SRC_ROWS)      # (both halves of the 8 bytes carry something)
    sources = [(a, 0) for a in data] + [(labels, 1)]
    idx = rng.integers(0, SRC_ROWS, B)                       # with repeats (B = 64 and 257 exceed the 41 source rows)
    if B >= 3:
        idx[1] = idx[0]
    checked = 0
    for name, perm in perms_of(B, rng).items():
        for lam in (float(rng.beta(0.2, 0.2)), 0.5, 1.0, 0.0, 1e-9):
            out = gather_mix(idx, perm[None], F.mix_of(lam)[None], sources, [0] * len(sources), B)
            for a, got in zip(data, out):
                assert np.array_equal(got.view(np.uint32), torch_mix(a, idx, perm, lam).view(np.uint32)), (name, lam, a.shape)
            ya, yb = out[-1]
            assert np.array_equal(ya, labels[idx]) and np.array_equal(yb, labels[idx][perm]), (name, lam)
            if lam == 1.0:                                   # the plain gather's values, whatever the permutation
                for a, got in zip(data, out):
                    assert np.array_equal(got, a[idx]), (name, a.shape)
            checked += 1
    # alone = rerun = together: one item per launch against the seven-item launch, twice
    perm, lam = perms_of(B, rng)["one_cycle"], 0.3
    full = gather_mix(idx, perm[None], F.mix_of(lam)[None], sources, [0] * len(sources), B)
    again = gather_mix(idx, perm[None], F.mix_of(lam)[None], sources, [0] * len(sources), B)
    for k, (src, a, b) in enumerate(zip(sources, full, again)):
        alone = gather_mix(idx, perm[None], F.mix_of(lam)[None], [src], [0], B)[0]
        for x, y, zz in zip(*(v if isinstance(v, tuple) else (v,) for v in (a, b, alone))):
            assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.int64), y.view(np.uint32 if x.dtype == np.float32 else np.int64))
            assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.int64), zz.view(np.uint32 if x.dtype == np.float32 else np.int64))
    # four draws in one launch: text, audio, visual, temporal each with their own (lam, permutation); aux and labels follow draw 0
    ps = perms_of(B, rng)
    perms4 = np.stack([ps["reversal"], ps["one_cycle"], ps["fixed_points"], ps["identity"]])
    lams4 = [0.25, float(rng.beta(0.2, 0.2)), 1.0, 0.9]
    groups = [0, 2, 3, 1, 0, 0]                              # 768 text, 512 visual, 256 temporal, 128 audio, aux, labels
    out = gather_mix(idx, perms4, np.stack([F.mix_of(l) for l in lams4]), sources, groups, B)
    for a, got, g in zip(data, out, groups):
        assert np.array_equal(got.view(np.uint32), torch_mix(a, idx, perms4[g], lams4[g]).view(np.uint32)), (a.shape, g)
    assert np.array_equal(out[-1][0], labels[idx]) and np.array_equal(out[-1][1], labels[idx][perms4[0]])
    # indices outside the source and permutation entries outside the batch are clamped, as ufnd_gather_rows clamps
    bad_idx, bad_perm = idx.copy(), ps["reversal"].copy()
    bad_idx[0], bad_perm[-1] = SRC_ROWS + 5, -3
    if B >= 3:
        bad_idx[2], bad_perm[1] = -1, B + 7
    ok_idx, ok_perm = np.clip(bad_idx, 0, SRC_ROWS - 1), np.clip(bad_perm, 0, B - 1)
    got = gather_mix(bad_idx, bad_perm[None], F.mix_of(0.3)[None], sources[:2], [0, 0], B)
    for a, g in zip(data[:2], got):
        assert np.array_equal(g.view(np.uint32), torch_mix(a, ok_idx, ok_perm, 0.3).view(np.uint32))
    print(f"gather-mix B={B}: {checked} (permutation, lam) pairs x {len(sources)} tensors bit-equal to the torch expression")


def test_gather_mix_of_the_fixture_rows():
    z = load_npz("recipe.npz")
    x, lam, index = z["mixup/x"], float(z["mixup/lam"]), z["mixup/index"]
    got, (ya, yb) = gather_mix(np.arange(len(x)), index[None], F.mix_of(lam)[None], [(x, 0), (z["mixup/y"], 1)], [0, 0], len(x))
    assert np.array_equal(got.view(np.uint32), z["mixup/mixed"].view(np.uint32))
    assert np.array_equal(ya, z["mixup/y"]) and np.array_equal(yb, z["mixup/y_b"])


# ---------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, B, use_graph=True, n=96, **kw):
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    cfg = TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), batch_size=B, device=DEV, use_graph=use_graph, **kw)
    return ForensicTrainer(cfg, cache=synthetic_cache(n, seed=3))


def _draws(B, groups, steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(steps):
        lams = np.array([float(rng.beta(0.2, 0.2)) for _ in range(groups)])
        perms = np.stack([rng.permutation(B) for _ in range(groups)])
        if s == 1:      # an unmixed step between two mixed ones
            lams, perms = np.ones(groups), np.tile(np.arange(B), (groups, 1))
        out.append((lams, perms))
    return out


def _focal_torch(logits, ya, yb, lam, alpha, gamma):
    """the criterion in torch (float64 from the fp32 logits on): q is the other class's probability"""
    lp = torch.log_softmax(logits.double(), dim=-1)
    r = torch.arange(logits.shape[0])

    def fl(y):
        return (alpha * torch.exp(lp[r, 1 - y]) ** gamma * -lp[r, y]).sum()
    return ((lam * fl(ya) + (1 - lam) * fl(yb)) / logits.shape[0]).float()


def _digest_close(got, ref, rtol, atol, what):
    """tests/helpers.assert_digest_close, with the digest of the oracle's tensor in place of a stored one"""
    d, r = digest(got), digest(ref)
    scale = max(r["norm"] / max(1.0, np.sqrt(ref.numel())), 1e-12)
    assert abs(d["norm"] - r["norm"]) <= rtol * r["norm"] + atol, (what, "norm", d["norm"], r["norm"])
    for k in ("head", "strided"):
        err = np.abs(d[k] - r[k]).max()
        assert err <= rtol * max(np.abs(r[k]).max(), scale) + atol, (what, k, err)


@pytest.mark.parametrize("mode", ["shared", "per_modality"])
@pytest.mark.parametrize("B", [4, 32])
def test_trainer_steps_match_the_oracle(tmp_path, B, mode):
    """Three captured steps of focal + mixup on cached rows against forward_batch + the criterion in torch + autograd + clip_grads_ +
    AdamWState on the CPU, the same draws on both sides (the second step unmixed).  Tolerances: those of
    tests/test_gpu_tier_a.py::test_train_steps_match_reference -- its B = 32 set while the oracle's steps do not clip, its B = 2 set
    (a clip coefficient carries the norm's own fp32 error into every parameter) once one does."""
    from oracle import tier_a as O
    from ultrafnd_git_amd.data import IndexedBatch
    alpha, gamma, G = 0.25, 2.0, 4 if mode == "per_modality" else 1
    tr = _trainer(tmp_path, B, True, criterion="focal", focal_alpha=alpha, focal_gamma=gamma, mixup_alpha=0.2, mixup_prob=1.0, mixup_mode=mode)
    assert tr.head.fused_entries is False and tr.head.mix_groups == G
    fus, clf = O.seeded_params(4321)
    tr.fusion.load_state_dict(fus)
    tr.clf.load_state_dict(clf)
    tr.fusion.dropout = tr.clf.dropout = tr.clf.node_dropout = 0.0
    tr.head.step_bufs.clear()
    tr.fusion.train(); tr.clf.train()
    draws = _draws(B, G, 3, 100 + B)
    queue = list(draws)
    tr.head.draw_source = lambda n: queue.pop(0)
    ds = tr._dataset("train")
    rng = np.random.default_rng(B)
    opt = O.AdamWState()
    fus, clf = {k: v.clone() for k, v in fus.items()}, {k: v.clone() for k, v in clf.items()}
    clipped = False
    for step, (lams, perms) in enumerate(draws, 1):
        idx = torch.from_numpy(rng.integers(0, len(ds), B))
        out = tr.train_step(IndexedBatch(ds, idx.to(DEV)))
        loss, logits = float(out["loss"].cpu()), out["logits"].cpu()
        assert torch.equal(out["y"].cpu(), ds.y.cpu()[idx])                    # accuracy is counted against labels_a
        # the oracle: the mixed inputs by the torch expression, draw g for the tensors of group g
        grp = (0, 1, 2, 3) if G == 4 else (0, 0, 0, 0)
        mixd = lambda x, g: float(lams[g]) * x[idx] + (1 - float(lams[g])) * x[idx][torch.from_numpy(perms[g]), :]
        batch = {"text_features": mixd(ds.T.cpu(), grp[0]), "audio_features": mixd(ds.A.cpu(), grp[1]), "visual_features": mixd(ds.V.cpu(), grp[2]),
                 "temporal_features": mixd(ds.U.cpu(), grp[3]), "gnn_feat": mixd(ds.G.cpu(), 0), "aux": mixd(ds.AUX.cpu(), 0), "label": ds.y.cpu()[idx]}
        fl = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point) for k, v in fus.items()}
        cl = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("tau")) for k, v in clf.items()}
        ref = O.forward_batch(fl, cl, batch, train=False)
        ya = batch["label"]
        ref_loss = _focal_torch(ref["logits"], ya, ya[torch.from_numpy(perms[0])], float(np.float32(lams[0])), alpha, gamma)
        ref_loss.backward()
        ref_loss = ref_loss.detach()
        grads = {**{"fusion." + k: v.grad for k, v in fl.items()}, **{"clf." + k: v.grad for k, v in cl.items()}}
        raw = {k: g.clone() for k, g in grads.items() if g is not None}
        total = O.clip_grads_(grads, 5.0)
        clipped = clipped or total > 5.0
        opt.step({**{"fusion." + k: v for k, v in fus.items()}, **{"clf." + k: v for k, v in clf.items()}}, grads)
        lt, (rt, at) = (1e-3, (2e-4, 2e-6)) if clipped else (1e-4, (2e-5, 2e-7))
        err = (logits - ref["logits"].detach()).abs().max().item()
        print(f"B={B} {mode} step {step}: loss {loss:.6f} (oracle {float(ref_loss):.6f}) logits max-abs-err {err:.2e} norm {total:.4f} lam {lams}")
        assert abs(loss - float(ref_loss)) <= 5e-5 and err <= lt, (step, loss, float(ref_loss), err)
        mine = dict(list(("fusion." + k, p) for k, p in tr.fusion.named_parameters()) + list(("clf." + k, p) for k, p in tr.clf.named_parameters()))
        if step == 1:      # (the gradient arena of step 1, unclipped: the clip lives in the optimizer kernel)
            seen = 0
            for k, g in raw.items():
                if k in tr.arena.offsets and tr.arena.has_grad(k) and g.dim():
                    e = (tr.arena.grad_view(k).cpu() - g).abs().max().item()
                    assert e <= 2e-4 * max(1e-3, g.abs().max().item()), (k, e)
                    seen += 1
            assert seen >= 40, seen
        if step in (1, 3):
            for k, p in mine.items():
                if p.dim():
                    _digest_close(p.detach(), (fus if k.startswith("fusion.") else clf)[k.split(".", 1)[1]], rt, at, f"step{step} {k}")
    assert int(tr.optim.state.read().step) == 3 and not queue


def _run_steps(tmp_path, use_graph, steps, B=16, seed=42, draws=None, **kw):
    torch.manual_seed(5)
    tr = _trainer(tmp_path, B, use_graph, seed=seed, criterion="focal", mixup_alpha=0.2, **kw)
    if draws is not None:
        queue = list(draws)
        tr.head.draw_source = lambda n: queue.pop(0)
    tr.fusion.train(); tr.clf.train()                                             # dropout on
    it, outs = iter(tr.train_loader), []
    for _ in range(steps):
        out = tr.train_step(next(it))
        outs.append((out["logits"].clone(), out["loss"].clone()))
    torch.cuda.synchronize()
    return tr, outs


@pytest.mark.parametrize("mode", ["shared", "per_modality"])
def test_graph_replay_equals_eager_with_a_new_draw_every_step(tmp_path, mode):
    """what catches a lam (or a permutation) baked into the captured graph: four steps, four different draws, one of them unmixed"""
    G = 4 if mode == "per_modality" else 1
    draws = _draws(16, G, 4, 7)
    assert len({float(l[0]) for l, _ in draws}) == 4
    (ta, a), (tb, b) = (_run_steps(tmp_path, g, 4, draws=draws, mixup_prob=1.0, mixup_mode=mode) for g in (False, True))
    assert tb.head.head_graph and not ta.head.head_graph
    for (la, sa), (lb, sb) in zip(a, b):
        assert torch.equal(la, lb) and torch.equal(sa, sb)
    assert torch.equal(ta.arena.data, tb.arena.data)
    assert len({float(s) for _, s in a}) == 4


def test_two_runs_with_the_same_seed_leave_the_same_bits(tmp_path):
    (ta, a), (tb, b), (tc, c) = (_run_steps(tmp_path, True, 5, seed=s) for s in (42, 42, 43))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b)) and torch.equal(ta.arena.data, tb.arena.data)
    assert torch.equal(ta.head.bufs(16, True)["perm"], tb.head.bufs(16, True)["perm"])
    assert not torch.equal(ta.arena.data, tc.arena.data)                          # (another seed: other draws, other masks)


def test_validation_and_test_never_mix(tmp_path):
    """after two mixed train steps, the forward-only logits of every validation and test batch equal those of a trainer WITHOUT mixup
    that holds the same parameters, bit for bit; both report the focal loss"""
    tr, _ = _run_steps(tmp_path, True, 2, mixup_prob=1.0)
    torch.manual_seed(5)
    plain = _trainer(tmp_path, 16, True, criterion="focal")
    plain.arena.data.copy_(tr.arena.data)
    for t in (tr, plain):
        t.fusion.eval(); t.clf.eval()
    n = 0
    for split, la, lb in (("val", tr.val_loader, plain.val_loader), ("test", tr.test_loader, plain.test_loader)):
        for ba, bb in zip(la, lb):
            oa, ob = tr._forward_batch(ba, split), plain._forward_batch(bb, split)
            assert torch.equal(oa["logits"], ob["logits"]) and torch.equal(oa["y"], ob["y"])
            assert torch.equal(tr.optim.state.float_view("loss"), plain.optim.state.float_view("loss"))
            n += 1
    assert n >= 2
    # ... and that loss is the focal loss of the unmixed rows
    lg, y = oa["logits"].cpu(), oa["y"].cpu()
    want = float(_focal_torch(lg, y, y, 1.0, 1.0, 2.0))
    assert abs(float(tr.optim.state.float_view("loss").cpu()) - want) <= 1e-6 + 1e-5 * want


def test_forced_exchange_on_one_rank_changes_no_bit(launch_job, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", str(port),
           "tests/focal_mixup_dp_child.py", "--out", str(tmp_path)]
    r = launch_job(cmd, env={"HSA_ENABLE_IPC_MODE_LEGACY": "0"}, timeout=300)
    assert r["rc"] == 0, (r["rc"], r["out"][-3000:], r["err"][-6000:])
    res = json.loads([ln for ln in r["out"].splitlines() if ln.startswith("{")][-1])
    assert res["backend"] == "nccl" and res["steps"] == 3 and res["bit_identical"], res
