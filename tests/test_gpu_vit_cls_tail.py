"""ClipVisualEncoder's class-token tail: past its attention the last layer runs over the N class-token rows only (cls_tail, on by
default for forward / image_embeds).  A row's arithmetic does not depend on the launch it is part of, so the features must equal
the all-rows pass bit for bit: in the three forms of the pass (folded bf16 stream, folded fp32 stream, unfolded), with one layer
(the last layer is also the first) and two, at frame counts around the fused attention's 5-samples-per-tile boundary and one row
past a 128- and a 256-row GEMM tile, with several frames per sample, eagerly and in a captured graph.  hidden_state keeps every
row.  The CPU part checks what the compact statistics buffers rely on: the GEMMs write the same number of row partials at N rows
as at the full row count."""
import functools

import pytest
import torch

DEV = "cuda"
gpu = pytest.mark.gpu
FORMS = {"folded-bf16": (True, "bf16"), "folded-fp32": (True, "fp32"), "unfolded": (False, "fp32")}
SHAPES = ((1, 1), (5, 1), (2, 3), (129, 1), (43, 3), (257, 1))      # (B, F): N = 1, 5, 6, 129, 129, 257 frames
NS = sorted({B * Fr for B, Fr in SHAPES})


def test_stat_parts_do_not_depend_on_the_row_count():
    """An even count, the same at N class-token rows as at the headline pass's 6,400 (and at N * 50) rows, for both GEMM widths that
    write a residual-stream row: the tail's statistics are the partials the all-rows launch would have written for those rows."""
    from ultrafnd_git_amd import _lib as L
    f = L.lib().ufnd_gemm_bf16_stat_parts
    for K in (768, 3072):
        want = f(6400, 768, K)
        assert want > 0 and want % 2 == 0
        for N in NS + [128, 256]:
            assert f(N, 768, K) == want == f(N * 50, 768, K), (N, K)


@functools.lru_cache(maxsize=None)
def _frames(B, Fr, seed=0):
    g = torch.Generator(device=DEV).manual_seed(7000 + 10 * B + Fr + seed)
    return torch.randn(B, Fr, 3, 224, 224, generator=g, device=DEV)


def _encoder(form, layers):
    from oracle import encoders_ref as E
    from ultrafnd_git_amd.encoders import ClipVisualEncoder
    fold, residual = FORMS[form]
    enc = ClipVisualEncoder(layers=layers, fold_ln=fold, residual_dtype=residual)
    enc.load_state_dict(E.seeded_weights(E.vit_shapes(layers=layers), 62))
    enc = enc.to(DEV)
    assert enc.cls_tail and enc.hidden == 768
    return enc


@gpu
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("form", list(FORMS))
def test_cls_tail_equals_the_all_rows_pass(form, layers):
    enc = _encoder(form, layers)
    for B, Fr in SHAPES:
        frames = _frames(B, Fr)
        flat = frames.view(B * Fr, 3, 224, 224)
        enc.cls_tail = False
        h0 = enc.hidden_state(frames).clone()
        want_f, want_e = enc(frames).clone(), enc.image_embeds(flat).clone()
        enc.cls_tail = True
        got_f, got_e = enc(frames).clone(), enc.image_embeds(flat).clone()
        h1 = enc.hidden_state(frames).clone()
        assert ("st0" in enc._workbufs(B, Fr)) == FORMS[form][0]      # (the form under test is the form that ran)
        assert got_f.shape == (B, enc.proj) and got_e.shape == (B * Fr, enc.proj)
        assert torch.isfinite(want_f).all() and torch.isfinite(want_e).all() and torch.isfinite(h0).all()
        assert torch.equal(got_f, want_f) and torch.equal(got_e, want_e), (B, Fr)
        assert torch.equal(h1, h0), (B, Fr)
    if FORMS[form][0]:
        assert 0.0 < enc.fold_ratio() < float("inf")      # the guard still sees the rows each launch folds


@gpu
def test_cls_tail_in_a_captured_graph():
    """The pass captured once and replayed with the frames rewritten in between: each replay equals the eager all-rows pass on the
    frames the buffer then holds."""
    enc = _encoder("folded-bf16", 2)
    B = 6
    frames = _frames(B, 1).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(frames)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc(frames)
    ref = _encoder("folded-bf16", 2)
    ref.cls_tail = False
    for seed in (1, 2):
        fr = _frames(B, 1, seed)
        frames.copy_(fr)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = ref(fr)
        assert torch.isfinite(out).all() and torch.equal(out, want), seed
    del graph
