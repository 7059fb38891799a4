"""GPU: the RoBERTa emotion classifier and AffectiveForensics (ultrafnd_git_amd/affective.py) against tests/affective_ref.py.

  pack + embeddings   position ids exact against HF's rule, cu_seqlens / row_src equal to ufnd_text_pack's, embeddings at the fp32
                      bound, rows past the live count never written
  stages              embeddings, hidden_states[1..], logits and class probabilities against float64 HF, each criterion within
                      BOUND_FACTOR x the bf16 mirror's own error on that input: two-launch attention (L = 40), fused attention over
                      slot bins and over sample tiles (L = 128), one 6-layer pass
  exact properties    packed = padded, alone = in a batch, run = rerun, eager = captured graph, cls_tail on = off: bit comparisons
  head / arousal      ufnd_emotion_head and ufnd_audio_arousal against float64 at their derived bounds and against
                      tests/golden/affective.npz (the real reference's analyze); AffectiveForensics.analyze_batch end to end
Every test prints its figures before it asserts, prefixed AFFECTIVE_ERR (tools/affective_errors.py collects them)."""
import functools

import numpy as np
import pytest
import torch

from tests import affective_ref as R

DEV = "cuda"
gpu = pytest.mark.gpu


def _report(what, got, bounds):
    for k, v in got.items():
        print(f"AFFECTIVE_ERR {what} {k} err {v:.3e} bound {bounds[k]:.3e}")
    bad = {k: (v, bounds[k]) for k, v in got.items() if not v <= bounds[k]}
    assert not bad, (what, bad)


@functools.lru_cache(maxsize=None)
def _weights(layers):
    from ultrafnd_git_amd.affective import RobertaEmotionClassifier
    return R.case_weights(RobertaEmotionClassifier(num_hidden_layers=layers, vocab_size=R.VOCAB).state_dict())


def _encoder(layers, form="folded-bf16"):
    from ultrafnd_git_amd.affective import RobertaEmotionClassifier
    fold, residual = R.FORMS[form]
    enc = RobertaEmotionClassifier(num_hidden_layers=layers, vocab_size=R.VOCAB, fold_ln=fold, residual_dtype=residual)
    enc.load_state_dict(_weights(layers))
    return enc.to(DEV)


@functools.lru_cache(maxsize=None)
def _default_encoder(layers):
    return _encoder(layers)


def _dev(ids, mask):
    return ids.to(DEV), mask.to(DEV, torch.int32)


# ------------------------------------------------------------------ pack and embeddings
def _pack_case(B, L):
    lengths = [L, 0, max(1, L // 2), 1, L - 1 if L > 1 else 1][:B]
    holes = []
    if L >= 8:
        holes.append((0, L // 2))
        if B >= 3:
            holes.append((2, 1))
        if B >= 5 and L >= 128:      # (either side of the scan's 64-token chunk edge)
            holes += [(4, 63), (4, 64)]
    return R.make_batch(lengths, L, seed=100 * B + L, holes=holes), lengths


@gpu
@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 130])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_pack_and_embeddings(B, L):
    from ultrafnd_git_amd import _lib as Lb
    lib, s = Lb.lib(), Lb.stream_ptr(torch.device(DEV))
    (ids, mask), lengths = _pack_case(B, L)
    want_pos = R.position_ids(ids)
    from transformers.models.roberta import modeling_roberta as MR
    hf = getattr(MR, "create_position_ids_from_input_ids", None) or MR.RobertaEmbeddings.create_position_ids_from_input_ids
    assert torch.equal(want_pos, hf(ids, R.PAD))
    d_ids, d_mask = _dev(ids, mask)
    i32 = dict(dtype=torch.int32, device=DEV)
    M = B * L
    cu, row_src, pos, valid = torch.full((B + 1,), -7, **i32), torch.full((M,), -7, **i32), torch.full((M,), -7, **i32), torch.full((B,), -7, **i32)
    Lb.check(lib.ufnd_roberta_pack(d_ids.data_ptr(), d_mask.data_ptr(), B, L, R.PAD, cu.data_ptr(), row_src.data_ptr(), pos.data_ptr(), valid.data_ptr(), s),
             "ufnd_roberta_pack")
    cu0, row0 = torch.full((B + 1,), -7, **i32), torch.full((M,), -7, **i32)
    Lb.check(lib.ufnd_text_pack(d_mask.data_ptr(), B, L, cu0.data_ptr(), row0.data_ptr(), s), "ufnd_text_pack")
    pos1 = torch.full((M,), -7, **i32)
    Lb.check(lib.ufnd_roberta_pack(d_ids.data_ptr(), d_mask.data_ptr(), B, L, R.PAD, None, None, pos1.data_ptr(), None, s), "ufnd_roberta_pack")
    assert torch.equal(pos.cpu().view(B, L).long(), want_pos) and torch.equal(pos1, pos)
    assert torch.equal(cu, cu0) and torch.equal(row_src, row0)      # (row_src past the live count: both leave the prefill)
    assert cu.cpu().tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert valid.cpu().tolist() == [1 if n else 0 for n in lengths]
    live = int(cu[-1])

    sd = _weights(2)
    E = "roberta.embeddings."
    w = {k: sd[E + k].to(DEV).contiguous() for k in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                                                    "LayerNorm.weight", "LayerNorm.bias")}
    w64 = {k: v.double().cpu() for k, v in w.items()}
    x = w64["word_embeddings.weight"][ids] + w64["position_embeddings.weight"][want_pos] + w64["token_type_embeddings.weight"][0]
    ref = torch.nn.functional.layer_norm(x, (R.HIDDEN,), w64["LayerNorm.weight"], w64["LayerNorm.bias"], 1e-5).view(M, R.HIDDEN)
    bound = R.FP32_BOUNDS["embed"] * float(ref.abs().max())
    tabs = [t.data_ptr() for t in w.values()]
    tail = (L, R.HIDDEN, R.VOCAB, R.MAX_POS, R.PAD, 1e-5, s)
    xb, xf = torch.empty(M, R.HIDDEN, dtype=torch.bfloat16, device=DEV), torch.empty(M, R.HIDDEN, dtype=torch.float32, device=DEV)
    Lb.check(lib.ufnd_roberta_embed(d_ids.data_ptr(), pos.data_ptr(), *tabs, xb.data_ptr(), xf.data_ptr(), B, *tail), "ufnd_roberta_embed")
    lb = torch.full((M, R.HIDDEN), float("nan"), dtype=torch.bfloat16, device=DEV)
    lf = torch.full((M, R.HIDDEN), float("nan"), dtype=torch.float32, device=DEV)
    Lb.check(lib.ufnd_roberta_embed_live(d_ids.data_ptr(), pos.data_ptr(), row_src.data_ptr(), cu.data_ptr() + 4 * B, *tabs, lb.data_ptr(), lf.data_ptr(),
                                         M, *tail), "ufnd_roberta_embed_live")
    torch.cuda.synchronize()
    err = float((xf.double().cpu() - ref).abs().max())
    print(f"AFFECTIVE_ERR embed B{B}_L{L} max_abs err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert torch.equal(xb, xf.to(torch.bfloat16))
    rows = row0[:live].long()
    assert torch.equal(lf[:live], xf[rows]) and torch.equal(lb[:live], xb[rows])      # a packed row is its padded row, bit for bit
    assert torch.isnan(lf[live:]).all() and torch.isnan(lb[live:].float()).all()      # rows past cu[B] are never written


# ------------------------------------------------------------------ stages and logits
STAGE_CASES = {
    "L40-two-launch": dict(layers=2, L=40, lengths=(40, 17, 1, 33, 8), holes=((0, 20), (3, 2))),
    "L128-slot-bins": dict(layers=2, L=128, lengths=(128, 20, 64, 65, 3), holes=((0, 64), (3, 63))),
    "L128-sample-tiles": dict(layers=2, L=128, lengths=tuple(1 + (7 * b) % 24 for b in range(44)), holes=((3, 5),)),
    "L40-six-layers": dict(layers=6, L=40, lengths=(40, 9, 33, 24), holes=((2, 7),)),
}


@gpu
@pytest.mark.parametrize("case", list(STAGE_CASES))
def test_stages_against_float64(case):
    c = STAGE_CASES[case]
    layers, L, B = c["layers"], c["L"], len(c["lengths"])
    ids, mask = R.make_batch(c["lengths"], L, seed=7, holes=c["holes"])
    Lr = max(c["lengths"])      # the float64 passes run on the columns any sample keeps: masked keys change nothing
    sd = _weights(layers)
    ref = R.reference(R.hf_model(sd, layers), ids[:, :Lr], mask[:, :Lr])
    mir = R.mirror(sd, ids[:, :Lr], mask[:, :Lr], layers, form="folded-bf16")
    enc = _default_encoder(layers)
    assert enc.cls_tail and enc.fold_ln and enc.residual_dtype == "bf16"
    if case == "L128-sample-tiles":
        assert B * (enc.heads // 2) >= enc.text_tile_min_grid and "tiles" in enc._workbufs(B, L)
    if case == "L128-slot-bins":
        assert B * (enc.heads // 2) < enc.text_tile_min_grid
    d_ids, d_mask = _dev(ids, mask)
    emb = enc.embeddings(d_ids, d_mask)[:, :Lr].double().cpu()
    err = float((emb - ref["embed"]).abs().max())
    bound = R.FP32_BOUNDS["embed"] * float(ref["embed"].abs().max())
    print(f"AFFECTIVE_ERR stage {case} embed max_abs err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    for k in range(1, layers + 1):
        h = enc.last_hidden_state(d_ids, d_mask, n_layers=k)[:, :Lr].double().cpu()
        _report(f"stage {case} hidden{k}", R.criteria(h, ref["layers"][k - 1]), R.bounds_from_mirror(mir["layers"][k - 1], ref["layers"][k - 1]))
    logits = enc.logits(d_ids, d_mask).double().cpu()
    probs = enc.probs(d_ids, d_mask).double().cpu()
    assert enc.fold_ln      # the fold guard never switched the form under test
    _report(f"stage {case} logits", R.criteria(logits, ref["logits"]), R.bounds_from_mirror(mir["logits"], ref["logits"]))
    _report(f"stage {case} class_probs", R.criteria(probs, ref["class_probs"]), R.bounds_from_mirror(mir["class_probs"], ref["class_probs"]))


# ------------------------------------------------------------------ exact properties
EXACT_BATCHES = {"L40": ((40, 17, 0, 33, 1), 40, ((0, 20),)), "L128": ((128, 20, 0, 65, 3), 128, ((0, 64),))}


@gpu
@pytest.mark.parametrize("name", list(EXACT_BATCHES))
def test_packed_alone_and_rerun_are_bit_identical(name):
    lengths, L, holes = EXACT_BATCHES[name]
    ids, mask = _dev(*R.make_batch(lengths, L, seed=9, holes=holes))
    enc = _default_encoder(2)
    packed = enc.logits(ids, mask).clone()
    probs = enc.probs(ids, mask).clone()
    assert torch.isfinite(packed).all()
    assert torch.equal(enc.logits(ids, mask), packed)                               # run = rerun
    padded = enc.logits(ids, mask, packed=False).clone()
    assert torch.equal(padded, packed) and torch.equal(enc.probs(ids, mask, packed=False), probs)      # packed = padded (the all-pad sample too)
    for b in range(len(lengths)):                                                    # a sample alone = in the batch
        assert torch.equal(enc.logits(ids[b:b + 1], mask[b:b + 1])[0], packed[b]), b
    assert torch.equal(packed[2], enc.logits(torch.full_like(ids[:1], R.PAD), torch.zeros_like(mask[:1]))[0])      # no text: the head of zero features
    print(f"AFFECTIVE_ERR exact {name} packed=padded=alone=rerun bits equal err 0 bound 0")


@gpu
def test_eager_equals_a_captured_graph():
    """The call captured once and replayed with the ids / mask rewritten in between: each replay equals the eager call on what the
    buffers then hold (no host synchronisation, fixed launch geometry)."""
    enc = _encoder(2)
    lengths, L, holes = EXACT_BATCHES["L128"]
    ids, mask = _dev(*R.make_batch(lengths, L, seed=9, holes=holes))
    ids, mask = ids.clone(), mask.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc.logits(ids, mask)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc.logits(ids, mask)
    ref = _default_encoder(2)
    for seed, lens in ((21, (5, 128, 77, 0, 31)), (22, (64, 1, 2, 128, 100))):
        i2, m2 = _dev(*R.make_batch(lens, L, seed=seed))
        ids.copy_(i2)
        mask.copy_(m2)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = ref.logits(i2, m2)
        assert torch.isfinite(out).all() and torch.equal(out, want), seed
    del graph
    print("AFFECTIVE_ERR exact graph eager=replay bits equal err 0 bound 0")


def _tail_batch(B, L, seed):
    lengths = [1 + (5 * b + 3) % L for b in range(B)]
    if B >= 5:
        lengths[1] = 0      # a sample without rows
        lengths[B - 1] = L
    return R.make_batch(lengths, L, seed=seed)


@gpu
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("form", list(R.FORMS))
def test_cls_tail_equals_the_all_rows_pass(form, layers):
    enc = _encoder(layers, form)
    for B, L in ((1, 16), (5, 16), (129, 16), (257, 16), (44, 128)):
        ids, mask = _dev(*_tail_batch(B, L, seed=B))
        if L == 128:
            assert B * (enc.heads // 2) >= enc.text_tile_min_grid      # the packed pass goes through the sample tiles
        for packed in (True, False):
            enc.cls_tail = False
            want_l, want_p = enc.logits(ids, mask, packed=packed).clone(), enc.probs(ids, mask, packed=packed).clone()
            enc.cls_tail = True
            got_l, got_p = enc.logits(ids, mask, packed=packed).clone(), enc.probs(ids, mask, packed=packed).clone()
            assert ("st" in enc._workbufs(B, L)) == R.FORMS[form][0]      # (the form under test is the form that ran)
            assert torch.isfinite(want_l).all() and got_l.shape == (B, R.LABELS)
            assert torch.equal(got_l, want_l) and torch.equal(got_p, want_p), (B, L, packed)
    print(f"AFFECTIVE_ERR exact cls_tail {form} layers{layers} bits equal err 0 bound 0")


# ------------------------------------------------------------------ head, arousal, AffectiveForensics
def _head(x, wd, bd, wo, bo, group, valid=None, arousal=None):
    from ultrafnd_git_amd import _lib as Lb
    B, H = x.shape
    C = wo.shape[0]
    f = lambda t, dt=torch.float32: None if t is None else torch.as_tensor(t).to(DEV, dt).contiguous()
    x, wd, bd, wo, bo, arousal = (f(t) for t in (x, wd, bd, wo, bo, arousal))
    group, valid = f(group, torch.int32), f(valid, torch.int32)
    out = {k: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV) for k, shape in
           (("logits", (B, C)), ("class_probs", (B, C)), ("probs", (B, 3)), ("text_intensity", (B,)), ("intensity", (B,)), ("valence", (B,)))}
    ws = torch.empty(B, H, dtype=torch.float32, device=DEV)
    Lb.check(Lb.lib().ufnd_emotion_head(x.data_ptr(), wd.data_ptr(), bd.data_ptr(), wo.data_ptr(), bo.data_ptr(), group.data_ptr(), Lb.ptr(valid),
                                        Lb.ptr(arousal), ws.data_ptr(), *(out[k].data_ptr() for k in ("logits", "class_probs", "probs", "text_intensity",
                                                                                                      "intensity", "valence")),
                                        B, H, C, Lb.stream_ptr(torch.device(DEV))), "ufnd_emotion_head")
    torch.cuda.synchronize()
    return {k: v.double().cpu() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("C", [7, 32])
def test_emotion_head_against_float64(C):
    g = torch.Generator().manual_seed(40 + C)
    B, H = 5, 768
    x = torch.randn(B, H, generator=g)
    wd, bd = 0.04 * torch.randn(H, H, generator=g), 0.05 * torch.randn(H, generator=g)
    wo, bo = 0.15 * torch.randn(C, H, generator=g), 0.05 * torch.randn(C, generator=g)
    names = list(R.DEFAULT_LABELS) if C == 7 else [("fear rage", "joyful anger", "worry", "amused", "plain")[c % 5] + str(c) for c in range(C)]
    valid, arousal = [1, 1, 0, 1, 1], torch.rand(B, generator=g)
    ref = R.head_ref(x, wd, bd, wo, bo, names, valid, arousal)
    bounds = R.head_bounds(x, wd, bd, wo, bo, valid)
    got = _head(x, wd, bd, wo, bo, R.group_table(names), valid, arousal)
    _report(f"head C{C}", {k: float((got[k] - ref[k]).abs().max()) for k in bounds}, bounds)
    assert got["probs"][2].tolist() == [0.0, 0.0, 0.0] and float(got["text_intensity"][2]) == 0.5
    again = _head(x, wd, bd, wo, bo, R.group_table(names), valid, arousal)
    alone = _head(x[3:4], wd, bd, wo, bo, R.group_table(names), valid[3:4], arousal[3:4])
    for k in got:      # run = rerun, a sample alone = in the batch: bits
        assert torch.equal(got[k], again[k]) and torch.equal(got[k][3], alone[k][0]), k
    no_audio = _head(x, wd, bd, wo, bo, R.group_table(names), valid, None)
    assert float((no_audio["intensity"] - R.head_ref(x, wd, bd, wo, bo, names, valid, None)["intensity"]).abs().max()) <= bounds["intensity"]


def _fixture(golden_dir):
    z = np.load(golden_dir / "affective.npz")
    lens = z["clip_lengths"]
    ends = np.cumsum(np.maximum(lens, 0))
    clips = [None if n < 0 else torch.from_numpy(z["clips"][e - n:e]) for n, e in zip(lens, ends)]
    return z, [str(n) for n in z["labels"]], clips


def _golden_slack(z, clips):
    """What the float64 restatement may differ from the recorded reference by, whose softmax, group sums and mean(x^2) are float32
    (tests/test_affective_ref.py derives the terms)."""
    C = z["logits"].shape[1]
    rng = float((z["logits"].max(-1) - z["logits"].min(-1)).max())
    probs = 2 * ((rng + C + 5) * R.EPS32 + C * R.EPS32)
    ar = max(1.25 * float((c.double() ** 2).mean()) * (21 + np.log2(len(c))) * R.EPS32 for c in clips if c is not None)
    return {"probs": probs, "arousal": ar, "intensity": 0.6 * 0.625 * 2 * probs + 0.4 * ar, "valence": probs}


@gpu
def test_head_and_arousal_reproduce_the_reference(golden_dir):
    """The head entry on the fixture's logits: x = atanh(logits / 16) through an identity dense layer and out_proj = 16 I reproduces
    them up to a slack that is computed in float64 and added to the bound; the arousal entry on the fixture's clips."""
    from ultrafnd_git_amd.affective import audio_arousal
    z, names, clips = _fixture(golden_dir)
    N, C = z["logits"].shape
    H = 32
    lg = torch.from_numpy(z["logits"]).double()
    assert float(lg.abs().max()) < 15.0
    x = torch.zeros(N, H, dtype=torch.float64)
    x[:, :C] = torch.atanh(lg / 16.0)
    wo = torch.zeros(C, H)
    wo[:, :C] = 16.0 * torch.eye(C)
    wd, bd, bo = torch.eye(H), torch.zeros(H), torch.zeros(C)
    slack = float((R.head_ref(x.float(), wd, bd, wo, bo, names)["logits"] - lg).abs().max())
    with_audio = [i for i, c in enumerate(clips) if c is not None]
    T = max(len(clips[i]) for i in with_audio)
    waves = torch.zeros(len(with_audio), T)
    for r, i in enumerate(with_audio):
        waves[r, :len(clips[i])] = clips[i]
    ar_gpu = audio_arousal(waves.to(DEV), torch.tensor([len(clips[i]) for i in with_audio])).double().cpu()
    ar_bound = max(R.arousal_bound(clips[i]) for i in with_audio)
    arousal = torch.full((N,), 0.5, dtype=torch.float64)
    arousal[with_audio] = ar_gpu
    got = _head(x, wd, bd, wo, bo, R.group_table(names), z["text_valid"], arousal)
    got["arousal"] = arousal
    bounds = R.head_bounds(x.float(), wd, bd, wo, bo, z["text_valid"], logits_slack=slack, arousal_err=ar_bound)
    bounds["arousal"] = ar_bound
    extra = _golden_slack(z, clips)
    keys = ("probs", "arousal", "intensity", "valence")
    _report("golden", {k: float((got[k] - torch.from_numpy(z["out/" + k])).abs().max()) for k in keys}, {k: bounds[k] + extra[k] for k in keys})


@gpu
def test_audio_arousal_lengths():
    from ultrafnd_git_amd.affective import audio_arousal
    lengths = [0, 1, 63, 64, 65, 16000, 80001]
    g = torch.Generator().manual_seed(5)
    T = max(lengths)
    waves = 0.5 * torch.randn(len(lengths), T, generator=g) * torch.linspace(0.2, 1.5, len(lengths))[:, None]
    d = waves.to(DEV)
    got = audio_arousal(d, torch.tensor(lengths)).clone()
    for b, n in enumerate(lengths):
        ref, bound = R.arousal_ref(waves[b, :n]), R.arousal_bound(waves[b, :n])
        err = abs(float(got[b]) - ref)
        print(f"AFFECTIVE_ERR arousal T{n} max_abs err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (n, err, bound)
        alone = audio_arousal(d[b:b + 1, :max(n, 1)].contiguous(), torch.tensor([n]))      # a clip alone, its row exactly its length
        assert torch.equal(alone[0], got[b]), n
        if n:
            assert torch.equal(audio_arousal(d[b:b + 1, :n].contiguous())[0], got[b]), n          # lengths=None: T
    assert float(got[0]) == 0.5
    assert audio_arousal(torch.zeros(3, 0, device=DEV)).tolist() == [0.5, 0.5, 0.5]                # T = 0


@gpu
def test_analyze_batch_end_to_end(golden_dir):
    """ids -> the classifier -> the head with the group table, the text_valid flags and the arousal wired in: every output against
    the float64 chain applied to the pass's own logits (the encoder's precision is the stage tests' subject)."""
    from ultrafnd_git_amd.affective import AffectiveForensics
    _, names, clips = _fixture(golden_dir)
    enc = _default_encoder(2)
    af = AffectiveForensics(classifier=enc, id2label=dict(enumerate(names)), device=DEV)
    assert af.groups == [1, -1, 0, 2, -1, -1, -1]
    lengths = (40, 17, 0, 33, 1)
    ids, mask = _dev(*R.make_batch(lengths, 40, seed=31))
    use = [c for c in clips if c is not None][:5]
    T = max(len(c) for c in use)
    waves = torch.zeros(5, T)
    for r, c in enumerate(use):
        waves[r, :len(c)] = c
    lens = torch.tensor([len(c) for c in use])
    out = {k: v.double().cpu() for k, v in af.analyze_batch(ids, mask, waves.to(DEV), lens).items()}
    logits = enc.logits(ids, mask).double().cpu()
    valid = [1 if n else 0 for n in lengths]
    ar = [R.arousal_ref(c) for c in use]
    ref = R.post_ref(logits, names, valid, ar)
    ar_bound = max(R.arousal_bound(c) for c in use)
    bounds = dict(R.post_bounds(logits, 0.0, ar_bound), arousal=ar_bound)
    _report("analyze_batch", {k: float((out[k] - ref[k]).abs().max()) for k in bounds}, bounds)
    assert out["probs"][2].tolist() == [0.0, 0.0, 0.0] and float(out["text_intensity"][2]) == 0.5
    assert torch.equal(af.get_emotion_intensity(ids, mask, waves.to(DEV), lens).double().cpu(), out["intensity"])
    quiet = {k: v.double().cpu() for k, v in af.analyze_batch(ids, mask).items()}      # audio=None: arousal 0.5
    ref0 = R.post_ref(logits, names, valid, None)
    assert quiet["arousal"].tolist() == [0.5] * 5
    _report("analyze_batch no-audio", {k: float((quiet[k] - ref0[k]).abs().max()) for k in ("intensity", "valence")}, R.post_bounds(logits))
