"""CPU: host-side logic of the drop-in layer -- module structure and initialisation parity with the
reference, arena layout, config loading, scheduler, loaders, loud failure without a HIP device."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN


@pytest.fixture(scope="module")
def parity():
    return json.loads((GOLDEN / "init_parity.json").read_text())


def test_same_seed_gives_the_reference_initial_weights(parity):
    """state_dict keys, order, shapes AND values of freshly constructed modules equal the reference's under
    the same torch seed (parameters are created in the reference's order; tests/golden/init_parity.json)."""
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.fusion import CrossModalTransformer
    torch.manual_seed(123)
    fusion, clf = CrossModalTransformer(), DeepTruthClassifier()
    for mod, ref in ((fusion, parity["fusion"]), (clf, parity["clf"])):
        sd = mod.state_dict()
        assert list(sd.keys()) == list(ref.keys())
        for k, (shape, s, a) in ref.items():
            assert list(sd[k].shape) == shape, k
            assert abs(float(sd[k].double().sum()) - s) <= 1e-9 * max(1.0, a), k
            assert abs(float(sd[k].double().abs().sum()) - a) <= 1e-9 * max(1.0, a), k
    assert sum(p.numel() for p in fusion.parameters()) == 12_732_421
    assert sum(p.numel() for p in clf.parameters()) == 539_873


def test_simple_gcn_same_seed_init_and_rng_position(parity):
    """SimpleGCN mirror: the reference's initial weights under the same seed, and the global RNG is left where
    the reference leaves it (so that everything constructed afterwards also matches)."""
    from ultrafnd_git_amd.gcn import SimpleGCN, sets_to_csr
    torch.manual_seed(321)
    sd = SimpleGCN(in_dim=416, hid=256, out_dim=128, dropout=0.2).state_dict()
    assert float(torch.rand(1)) == parity["gcn_rng_after"]
    assert list(sd.keys()) == list(parity["gcn"].keys())
    for k, (shape, s_, a) in parity["gcn"].items():
        assert list(sd[k].shape) == shape and abs(float(sd[k].double().sum()) - s_) <= 1e-9 * max(1.0, a), k
    offs, toks = sets_to_csr([{"b", "a"}, set(), {"a", "c", "a"}])
    assert offs.tolist() == [0, 2, 2, 4] and len(set(toks[:2].tolist())) == 2 and sorted(toks[2:].tolist()) == toks[2:].tolist()
    assert len(set(toks.tolist())) == 3          # three distinct phrases, "a" shared


def test_train_config_mirrors_the_reference_dataclass(parity):
    from ultrafnd_git_amd.trainer import TrainConfig
    mine = [(f.name, repr(f.default) if f.default is not dataclasses.MISSING else None) for f in dataclasses.fields(TrainConfig)]
    ref = [tuple(x) for x in parity["train_config_fields"]]
    assert mine[:len(ref)] == ref                 # same fields, order and defaults; additions only at the end
    assert [n for n, _ in mine[len(ref):]] == ["device", "use_graph", "encode_inline", "label_smoothing", "class_weighting", "use_cosine",
                                               "min_lr_scale", "cu_split", "gnn_in_graph", "encoder_lookahead", "head_graph", "persistent_inputs",
                                               "grad_payload", "grad_exchange", "train_encoders", "fused_head"]


def test_arena_layout_keeps_stacked_groups_contiguous_and_aligned():
    from ultrafnd_git_amd.arena import rehome
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.fusion import _QKV_ORDER, CrossModalTransformer
    fusion, clf = CrossModalTransformer(), DeepTruthClassifier()
    arena = rehome([clf, fusion], ["clf.", "fusion."])
    H = fusion.hidden
    off = arena.offsets
    base = off["fusion.attn_tv.q.weight"][0]
    for i, (blk, p) in enumerate(_QKV_ORDER):
        assert off[f"fusion.{blk}.{p}.weight"][0] == base + i * H * H
        assert off[f"fusion.{blk}.{p}.bias"][0] == off["fusion.attn_tv.q.bias"][0] + i * H
    g0 = off["clf.node.trees.0.gates.0"][0]
    for t in range(6):
        for k in range(4):
            assert off[f"clf.node.trees.{t}.gates.{k}"][0] == g0 + (t * 4 + k) * H
            assert off[f"clf.node.trees.{t}.thresh.{k}"][0] == off["clf.node.trees.0.thresh.0"][0] + t * 4 + k
    for key in ("fusion.fuse_mlp.0.weight", "fusion.text_proj.weight", "clf.pre.0.weight", "fusion.attn_tv.q.weight"):
        assert off[key][0] % 64 == 0
    # no-grad tensors sit behind the gradient range; the range holds exactly the 12,745,949 trainable scalars
    nograd = [k for k in off if not arena.has_grad(k)]
    assert sorted(nograd) == sorted(["clf.temperature"] + [f"clf.node.trees.{t}.tau" for t in range(6)] +
                                    [f"fusion.semantic.{n}.0.{w}" for n in ("text_proj", "vision_proj") for w in ("weight", "bias")] +
                                    ["fusion.classifier.weight", "fusion.classifier.bias"])
    n_train = sum(int(np.prod(off[k][1])) if off[k][1] else 1 for k in off if arena.has_grad(k))
    assert n_train == 12_745_949 and arena.n_grad % 64 == 0 and arena.n_grad >= n_train
    # parameters really are views of the arena and load_state_dict writes through
    p = dict(fusion.named_parameters())["fuse_mlp.3.bias"]
    assert p.data_ptr() == arena.view("fusion.fuse_mlp.3.bias").data_ptr()
    sd = fusion.state_dict()
    sd["fuse_mlp.3.bias"] = torch.full_like(sd["fuse_mlp.3.bias"], 0.25)
    fusion.load_state_dict(sd)
    assert float(arena.view("fusion.fuse_mlp.3.bias").mean()) == 0.25


def test_config_manager_semantics(tmp_path):
    """src/utils/config_utils.py:34-71: missing file -> {}, non-dict YAML -> {}, defaults merged, cached."""
    from ultrafnd_git_amd.config_utils import ConfigManager, load_yaml
    cm = ConfigManager()
    assert cm.load_config(str(tmp_path / "nope.yaml")) == {}
    assert cm.load_config(str(tmp_path / "nope.yaml"), defaults={"a": 1}) == {"a": 1}
    (tmp_path / "l.yaml").write_text("- 1\n- 2\n")
    assert cm.load_config(str(tmp_path / "l.yaml")) == {}
    (tmp_path / "ok.yaml").write_text("hidden_dim: 256\ndropout: 0.2\n")
    assert cm.load_config(str(tmp_path / "ok.yaml"), defaults={"hidden_dim": 1, "x": 2}) == {"hidden_dim": 256, "x": 2, "dropout": 0.2}
    (tmp_path / "ok.yaml").write_text("hidden_dim: 999\n")
    assert cm.load_config(str(tmp_path / "ok.yaml"))["hidden_dim"] == 256           # cached per instance
    assert load_yaml("configs/model_configs/fusion.yaml")["hidden_dim"] == 512      # resolved against the repo root
    assert load_yaml("configs/model_configs/classifier.yaml")["node_trees"] == 6


def test_code_defaults_apply_when_yaml_is_missing():
    """cross_modal_transformer.py:87 / deep_truth_classifier.py:107: dropout 0.3 if the YAML is absent (0.1 with it)."""
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.fusion import CrossModalTransformer
    assert CrossModalTransformer("does/not/exist.yaml").dropout == 0.3
    assert CrossModalTransformer().dropout == 0.1
    assert DeepTruthClassifier("does/not/exist.yaml").dropout == 0.3 and DeepTruthClassifier().dropout == 0.1


def test_everything_refuses_to_run_without_a_hip_device(tmp_path):
    from ultrafnd_git_amd._lib import UltrafndHipError
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.encoders import BertTextEncoder, ClipVisualEncoder
    from ultrafnd_git_amd.temporal import TemporalSyncNet
    from ultrafnd_git_amd.trainer import ForensicTrainer, TrainConfig, synthetic_cache
    with pytest.raises(UltrafndHipError):
        DeepTruthClassifier()(torch.zeros(2, 512), torch.zeros(2, 2))
    with pytest.raises(UltrafndHipError):
        BertTextEncoder(layers=1, vocab_size=50)(torch.zeros(1, 8, dtype=torch.long), torch.ones(1, 8, dtype=torch.long))
    with pytest.raises(UltrafndHipError):
        ClipVisualEncoder(layers=1)(torch.zeros(1, 3, 224, 224))
    with pytest.raises(UltrafndHipError):
        TemporalSyncNet().align(np.zeros(768, np.float32), np.zeros(512, np.float32))
    with pytest.raises(UltrafndHipError):
        ForensicTrainer(TrainConfig(data_root="", ocr_phrase_pkl=None, out_dir=str(tmp_path), device="cpu"), cache=synthetic_cache(8))


def test_cached_dataset_and_loader_on_host_tensors():
    """CachedTensorDataset item schema (forensic_trainer.py:73-83) and DataLoader-equivalent batching."""
    from ultrafnd_git_amd.trainer import CachedTensorDataset, DeviceBatchLoader, synthetic_cache
    cache = synthetic_cache(23, seed=4)
    tr_idx = cache["split"][0]
    ds = CachedTensorDataset(cache, tr_idx)
    assert len(ds) == len(tr_idx) == 16
    item = ds[3]
    assert set(item) == {"text_features", "audio_features", "visual_features", "temporal_features", "aux", "label", "index"}
    assert item["index"] == 3 and item["text_features"].shape == (768,) and item["label"].dtype == torch.int64
    assert np.allclose(item["text_features"].numpy(), cache["text"][tr_idx[3]])
    sizes = [b["label"].shape[0] for b in DeviceBatchLoader(ds, 5, shuffle=False)]
    assert sizes == [5, 5, 5, 1]                                   # drop_last=False
    ld = DeviceBatchLoader(ds, 16, shuffle=True, seed=1)
    e1 = next(iter(ld))["index"].tolist()
    e2 = next(iter(ld))["index"].tolist()
    assert sorted(e1) == list(range(16)) and e1 != e2               # reshuffled every epoch
    b = next(iter(DeviceBatchLoader(ds, 4, shuffle=False)))
    assert torch.equal(b["index"], torch.arange(4)) and b["aux"].shape == (4, 2)


def test_step_lr_matches_torch():
    """StepLR(step_size=3, gamma=0.7) (forensic_trainer.py:177) vs torch's own scheduler."""
    from ultrafnd_git_amd.optim import StepLR

    class FakeOpt:
        param_groups = [{"lr": 2e-4, "initial_lr": 2e-4}]

        def set_lr(self, lr):
            self.param_groups[0]["lr"] = lr
    mine = StepLR(FakeOpt(), 3, 0.7)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=2e-4)
    ref = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.7)
    for _ in range(10):
        opt.step(); ref.step(); mine.step()
        assert abs(mine.get_last_lr()[0] - ref.get_last_lr()[0]) < 1e-15


def test_temporal_sequence_module_init_and_delay_estimators():
    """TemporalSyncNet(use_tcn=True): the reference's state_dict keys / order and initial weights under the same seed,
    with the global RNG left where the reference leaves it; delay_score / estimate_av_lag equal the reference's
    static methods on known inputs, ragged lengths and the < 4 samples case (tests/golden/temporal_seq.npz)."""
    from tests.helpers import load_npz
    from ultrafnd_git_amd.temporal import TemporalSyncNet
    g = load_npz("temporal_seq.npz")
    torch.manual_seed(654)
    net = TemporalSyncNet(in_dim=768, out_dim=256, use_tcn=True)
    assert float(torch.rand(1)) == float(g["init/rng_after"])
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["init/keys"]]
    for v, s_, a in zip(sd.values(), g["init/sums"], g["init/abs_sums"]):
        assert abs(float(v.double().sum()) - s_) <= 1e-9 * max(1.0, a) and abs(float(v.double().abs().sum()) - a) <= 1e-9 * max(1.0, a)
    assert not any(p.requires_grad for p in net.parameters())
    with pytest.raises(AssertionError):
        TemporalSyncNet()(torch.zeros(1, 4, 384), torch.zeros(1, 4, 384))          # use_tcn=False: the reference's assert
    for (a, v), want in zip(g["delay/args"], g["delay/out"]):
        assert TemporalSyncNet.delay_score(int(a), int(v)) == float(want)
    for i, want in enumerate(g["lag/out"]):
        sr, max_lag = g[f"lag/{i}/args"]
        got = TemporalSyncNet.estimate_av_lag(g[f"lag/{i}/a"], torch.from_numpy(g[f"lag/{i}/m"]), sr=float(sr), max_lag_s=float(max_lag))
        assert got == float(want), (i, got, want)


def test_head_step_sizes_aux_from_the_classifier_and_refuses_other_widths():
    """HeadStep reads clf.eff_aux (aux_dim with use_aux, else 0): a dataset whose aux rows are not aux_dim wide is refused at
    construction, naming the limit; without use_aux any width passes (the column is never read, deep_truth_classifier.py:142-146)."""
    from types import SimpleNamespace
    from ultrafnd_git_amd.head_step import HeadStep
    cfg = SimpleNamespace(use_graph=False, head_graph=False, label_smoothing=0.0, class_weighting=False, fused_head=True)
    for eff_aux, ok, bad in ((2, 2, 4), (4, 4, 2)):
        hs = HeadStep(cfg, torch.device("cpu"), None, SimpleNamespace(eff_aux=eff_aux, hidden=512), None, None)
        assert hs.aux_dim == eff_aux
        hs.check_aux_width(ok)
        with pytest.raises(ValueError, match=f"aux_dim: {eff_aux}"):
            hs.check_aux_width(bad)
    hs = HeadStep(cfg, torch.device("cpu"), None, SimpleNamespace(eff_aux=0, hidden=512), None, None)
    assert hs.aux_dim == 0
    hs.check_aux_width(2)
    hs.check_aux_width(4)


@pytest.mark.parametrize("use_aux,aux_dim", [(False, 2), (True, 2), (True, 4)])
def test_head_step_aux_buffer_and_pointer_follow_the_classifier(tmp_path, use_aux, aux_dim):
    """The step's aux buffer is (B, clf.eff_aux) and the head gets a null aux pointer without use_aux (both entry points refuse a
    non-null aux when aux_dim is 0).  Host side only: the workspace sizes come from the library's host functions."""
    from types import SimpleNamespace
    from ultrafnd_git_amd.classifier import DeepTruthClassifier
    from ultrafnd_git_amd.head_step import HeadStep
    cy = tmp_path / "classifier.yaml"
    cy.write_text(f"input_dim: 256\nhidden_dim: 256\nuse_aux: {str(use_aux).lower()}\naux_dim: {aux_dim}\nnode_trees: 3\nnode_depth: 6\n")
    clf = DeepTruthClassifier(str(cy))
    eff = aux_dim if use_aux else 0
    assert clf.eff_aux == eff and clf.dims().aux_dim == eff
    cfg = SimpleNamespace(use_graph=False, head_graph=False, label_smoothing=0.0, class_weighting=False, fused_head=True)
    hs = HeadStep(cfg, torch.device("cpu"), SimpleNamespace(dropout=0.1, gnn_dim=128, hidden=256), clf, None, None)
    b = hs.bufs(5, True)
    assert tuple(b["aux"].shape) == (5, eff)
    io = hs._io(b)
    assert (io.aux is None) == (eff == 0)
    aux = torch.rand(5, aux_dim)
    hs.stage_aux(b, aux)
    if eff:
        assert torch.equal(b["aux"], aux)


# ---- the encoders' layer tables (layer_keys) and the arena layout they feed (groups()): checkpoints depend on both
_BERT_REST = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
              "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
_VIT_REST = ["vision_model.embeddings.class_embedding", "vision_model.embeddings.patch_embedding.weight",
             "vision_model.embeddings.position_embedding.weight", "vision_model.pre_layrnorm.weight", "vision_model.pre_layrnorm.bias",
             "vision_model.post_layernorm.weight", "vision_model.post_layernorm.bias", "visual_projection.weight"]
_CLIP_TEXT_REST = ["text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight",
                   "text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias", "text_projection.weight"]
_W2V2_REST = ([f"feature_extractor.conv_layers.{i}.conv.weight" for i in range(7)] +
              ["feature_extractor.conv_layers.0.layer_norm.weight", "feature_extractor.conv_layers.0.layer_norm.bias",
               "feature_projection.layer_norm.weight", "feature_projection.layer_norm.bias", "feature_projection.projection.weight",
               "feature_projection.projection.bias", "encoder.pos_conv_embed.conv.bias",
               "encoder.pos_conv_embed.conv.parametrizations.weight.original0", "encoder.pos_conv_embed.conv.parametrizations.weight.original1",
               "encoder.layer_norm.weight", "encoder.layer_norm.bias", "proj.weight", "proj.bias"])
_LAYER_NAMES = ["qkv_w", "qkv_b", "o_w", "o_b", "g1", "b1n", "w1", "b1", "w2", "b2", "g2", "b2n"]


def _tiny_encoder(name):
    """(a 2-layer encoder, its keys outside the layers): only the one asked for is built."""
    if name == "bert":
        from ultrafnd_git_amd.encoders import BertTextEncoder
        return BertTextEncoder(layers=2, vocab_size=64, max_position=16), _BERT_REST
    if name == "vit":
        from ultrafnd_git_amd.encoders import ClipVisualEncoder
        return ClipVisualEncoder(layers=2), _VIT_REST
    if name == "clip_text":
        from ultrafnd_git_amd.semantic import ClipTextEncoder
        return ClipTextEncoder(vocab_size=64, num_hidden_layers=2), _CLIP_TEXT_REST
    from ultrafnd_git_amd.audio import Wav2Vec2AudioEncoder
    return Wav2Vec2AudioEncoder(layers=2, intermediate=256), _W2V2_REST


@pytest.mark.parametrize("name", ["bert", "vit", "clip_text", "w2v2"])
def test_layer_keys_and_the_non_layer_keys_are_exactly_the_state_dict(name):
    """layer_keys(i) over the layers plus the keys outside the layers: every state_dict key once, nothing else; the twelve names, each a
    list of keys (three for the stacked Q/K/V, one otherwise); memoised."""
    enc, rest = _tiny_encoder(name)
    keys = list(rest)
    for i in range(2):
        k = enc.layer_keys(i)
        assert list(k) == _LAYER_NAMES and enc.layer_keys(i) is k
        assert [len(k[n]) for n in _LAYER_NAMES] == [3, 3] + [1] * 10
        assert all(f".{i}." in key for n in _LAYER_NAMES for key in k[n])
        keys += [key for n in _LAYER_NAMES for key in k[n]]
    sd = enc.state_dict()
    assert len(keys) == len(set(keys)) and set(keys) == set(sd.keys())
    k = enc.layer_keys(1)
    H = enc.hidden
    assert [tuple(sd[x].shape) for x in k["qkv_w"] + k["o_w"]] == [(H, H)] * 4 and tuple(sd[k["w1"][0]].shape) == (enc.inter, H)
    assert tuple(sd[k["w2"][0]].shape) == (H, enc.inter) and tuple(sd[k["b1"][0]].shape) == (enc.inter,)
    assert all(tuple(sd[k[n][0]].shape) == (H,) for n in ("o_b", "g1", "b1n", "b2", "g2", "b2n"))


def test_backprop_groups_are_the_recorded_arena_order():
    """TextBackprop.groups() / VisualBackprop.groups() at 2 layers against the key lists recorded before the layer table moved into the
    encoders: the arena layout (order, and which tensors are adjacent) is what checkpoints and the stacked Q/K/V views depend on."""
    from ultrafnd_git_amd.encoder_train import TextBackprop, VisualBackprop

    def bert_layer(i):
        P = f"encoder.layer.{i}."
        return [[P + "output.LayerNorm.weight"], [P + "output.LayerNorm.bias"], [P + "output.dense.weight"], [P + "output.dense.bias"],
                [P + "intermediate.dense.weight"], [P + "intermediate.dense.bias"], [P + "attention.output.LayerNorm.weight"],
                [P + "attention.output.LayerNorm.bias"], [P + "attention.output.dense.weight"], [P + "attention.output.dense.bias"],
                [P + "attention.self.query.weight", P + "attention.self.key.weight", P + "attention.self.value.weight"],
                [P + "attention.self.query.bias", P + "attention.self.key.bias", P + "attention.self.value.bias"]]

    def vit_layer(i):
        P = f"vision_model.encoder.layers.{i}."
        return [[P + "mlp.fc2.weight"], [P + "mlp.fc2.bias"], [P + "mlp.fc1.weight"], [P + "mlp.fc1.bias"], [P + "layer_norm2.weight"],
                [P + "layer_norm2.bias"], [P + "self_attn.out_proj.weight"], [P + "self_attn.out_proj.bias"],
                [P + "self_attn.q_proj.weight", P + "self_attn.k_proj.weight", P + "self_attn.v_proj.weight"],
                [P + "self_attn.q_proj.bias", P + "self_attn.k_proj.bias", P + "self_attn.v_proj.bias"], [P + "layer_norm1.weight"],
                [P + "layer_norm1.bias"]]

    want_text = bert_layer(1) + bert_layer(0) + [["embeddings.LayerNorm.weight"], ["embeddings.LayerNorm.bias"],
                                                 ["embeddings.position_embeddings.weight"], ["embeddings.token_type_embeddings.weight"],
                                                 ["embeddings.word_embeddings.weight"]]
    want_vis = ([["visual_projection.weight"], ["vision_model.post_layernorm.weight"], ["vision_model.post_layernorm.bias"]] +
                vit_layer(1) + vit_layer(0) +
                [["vision_model.pre_layrnorm.weight"], ["vision_model.pre_layrnorm.bias"], ["vision_model.embeddings.position_embedding.weight"],
                 ["vision_model.embeddings.class_embedding"], ["vision_model.embeddings.patch_embedding.weight"]])
    for bp, enc, want in ((TextBackprop, _tiny_encoder("bert")[0], want_text), (VisualBackprop, _tiny_encoder("vit")[0], want_vis)):
        got = bp(enc).groups()
        assert [[k for k, _ in g] for g in got] == want
        sd = enc.state_dict()
        assert all(shape == tuple(sd[k].shape) for g in got for k, shape in g)
        lin = bp(enc).linears()
        assert lin["1.qkv"] == (enc.layer_keys(1)["qkv_w"], enc.layer_keys(1)["qkv_b"]) and lin["0.w2"] == (enc.layer_keys(0)["w2"], enc.layer_keys(0)["b2"])
