"""Cases, float64 references, float32 mirrors, bounds and mutants of the fusion head and the NODE classifier (csrc/tier_a.hip:
ufnd_fusion_forward / _backward / _input_grads, ufnd_classifier_forward / _backward, ufnd_softmax_ce).  Shared by
tests/test_head_cases.py (CPU: the conditions hold, a second float32 evaluation in the kernels' order of addition stays inside
every bound, every mutant leaves one by MUTANT_FACTOR, the table reaches every path) and tests/test_gpu_head_cases.py (GPU: every
case through the modules and the C ABI against float64).  The layout is that of tests/graph_ops_cases.py, whose BOUND_FACTOR,
MUTANT_FACTOR and HW_ULP are used here.

Reference and mirror.  oracle/tier_a.py runs in its parameters' dtype: the reference is fusion_forward, classifier_forward and
autograd in float64, the mirror the same in float32 on the same inputs.  Nothing is bounded by what a kernel produces.

Five checks per case (the keys of an evaluation are "<check>/<tensor>"):
  fwd    fusion forward: fused, the aux logits, the three forensic vectors.
  fbwd   fusion backward alone: seeded upstream gradients at `fused` and at the aux logits together; every parameter gradient
         (classifier.* included: the aux head receives one here) and the five input gradients.
  cfwd   classifier forward alone on the float64 reference's `fused` rounded to float32: logits, probs, the clamped temperature.
  cbwd   classifier backward alone from a seeded gradient at the logits: every parameter gradient and the gradient at `fused`.
  chain  fusion -> classifier -> cross-entropy: loss, logits, fused and every gradient (what the older head tests compare).

Bound.  For every compared vector max|gpu - ref64| <= BOUND_FACTOR (3) x the float32 oracle's own max|float32 - ref64| on that same
input, case by case.  All node.trees.*.thresh.* gradients of a check form one vector per case, so do the
evidence_proj.2.bias, bypass.bias and classifier.bias gradients; every other tensor is a vector of its own.  Only the loss, one
number per case, is judged over the table (`loss_table_ratio`, as graph_ops_cases judges the GCN pretrain loss).  No figure of
any other case, and none from a GPU, enters a bound.

The float32 oracle's error is a maximum over orders.  One float32 evaluation is one draw of the rounding errors.  Where a vector
has many elements with errors of their own, the maximum over them is a stable yardstick; where it has few (the forensic scalars
and logits at B = 1, the threshold gradients, whose elements all carry the error of one scalar per row; the gradients of the
outliers and saturated_trees families, which three rows or a few steep gates carry), a single draw can land anywhere below the
typical error, and then 3 x it excludes other float32 evaluations of the same formula that are every bit as good.  So the
yardstick of a vector is the largest error over N_ENS = 12 float32 evaluations of the oracle on that input, each in another
legitimate order: member 0 is the oracle as it stands; member m has the rows of the batch in a seeded order (the parameter
gradients then add their rows in that order) and every Linear summed over 2 to 5 chunks of its K; odd members also write the two
forensic cosines as dot / (norm x norm) and the trees' leaf probabilities leaf by leaf, as the kernels do, where the oracle
normalises first and doubles level by level -- the same functions, whose float32 errors differ most where a cosine sits on its
clamp or a gate's signed sum over the leaves cancels (`reordered`).  N_ENS comes
from the worst vector there is, one whose elements all share a single Gaussian error: another draw of that error exceeds 3 x the
largest of N draws with probability 0.21 at N = 1, 0.024 at 3, 8e-4 at 8, 1.3e-4 at 12 (simulated), and the table makes some 6,000
comparisons, a few hundred of them of such vectors.  With 3 orders the CPU suite's own second evaluation, below, left two
bounds (4.0 x at a gate vector of B = 257, 4.3 x at the tiny biases of the constant rows of B = 290 ablation); with 12 its
worst over the table is 0.65 of a bound.  The evaluation in the kernels' own orders (`ordered=True`) is NOT a member: the CPU suite holds it
to these bounds as the evidence that they admit a legitimate order they were not made from.  Nothing is excluded from any
comparison.

Input families (conditions in tests/test_head_cases.py):
  gaussian         O.seeded_batch.
  ablation         visual and temporal inputs exactly zero.
  aligned          visual_proj = 2 x text_proj's first 512 columns, temporal_proj = -1 x its first 256, text columns from 256 on
                   zero: v = 2t, u = -t; conflict < 1e-3, delay > 0.999.
  outliers         text rows 0, B // 2, B - 1 scaled 20 x (emotion > 0.99), row 1 scaled 1e-3 when B > 3 (emotion < 0.05).
  saturated_trees  every tau x 8, and two thresholds of every three moved by -+0.15: with tau x 8 alone the seeded gates'
                   sigmoids stay in [0.03, 1], and the family is there for some sigmoid < 1e-3 and some > 1 - 1e-3.

Hardware approximations (__expf in the softmaxes and ce_row, reciprocals) would be modelled in the mirror at their site with
HW_ULP, never by a wider factor; none is needed for the table below (profiles/head_errors.txt).
"""
from __future__ import annotations

import functools
import math
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import tier_a as O
from tests import dropout_mirror as D
from tests.graph_ops_cases import BOUND_FACTOR, HW_ULP, MUTANT_FACTOR  # noqa: F401

CHECKS = ("fwd", "fbwd", "cfwd", "cbwd", "chain")
FEATS = ("text_features", "audio_features", "visual_features", "temporal_features", "gnn_feat")
P_FUSION, P_CLF, P_NODE = 0.1, 0.1, 0.3           # fusion.yaml / classifier.yaml dropout, the trees' hard-coded 0.3
FUSION_KEY, CLF_KEY = (0x5EED0001, 1), (0x5EED0002, 1)      # (seed, step) of the train-mode cases: a fresh state after one forward
TOL_OUT, TOL_GRAD = 2e-5, 5e-4                    # the older head tests' criteria (tests/test_gpu_head_geometry.py), for the record


class Geometry(NamedTuple):
    hidden: int
    trees: int
    depth: int
    aux: int          # 0: use_aux false
    use_gnn: bool


GEOMS: "OrderedDict[str, Geometry]" = OrderedDict([
    ("G0", Geometry(512, 6, 4, 2, True)),         # the shipped geometry
    ("G1", Geometry(256, 16, 2, 4, True)),        # NI = 1, both tree caps (16 trees, trees x depth = 32), aux 4
    ("G2", Geometry(1024, 5, 6, 0, True)),        # NI = 4, the depth cap (64 leaves), no aux
    ("G3", Geometry(512, 1, 1, 2, False)),        # one stump, the 15-slot concat
])
FAMILIES = ("gaussian", "ablation", "aligned", "outliers", "saturated_trees")


class Case(NamedTuple):
    geom: str
    B: int
    family: str
    train: bool = False


def case_id(c: Case) -> str:
    return f"{c.geom}-B{c.B}-{c.family}" + ("-train" if c.train else "")


G0_SIZES = (1, 2, 63, 64, 65, 127, 128, 130, 256, 257, 290, 1000)


def _table() -> List[Case]:
    cases = [Case("G0", b, "gaussian") for b in G0_SIZES]
    cases += [Case("G0", b, f) for f in FAMILIES[1:] for b in (1, 65, 290)]
    # one family each on G1 .. G3, rotating; the order puts saturated_trees on several rows of many gates (G1 at 65, G2 at 130):
    # one row, or the one gate of G3, cannot reach both ends of a sigmoid
    rot = ("ablation", "saturated_trees", "aligned", "outliers")
    for g, sizes in (("G1", (1, 65, 290)), ("G2", (1, 65, 130)), ("G3", (1, 65, 290))):
        for b in sizes:
            cases.append(Case(g, b, rot[(len(cases) - 24) % 4]))
    cases += [Case("G0", 65, "gaussian", True), Case("G0", 290, "gaussian", True), Case("G1", 65, "gaussian", True)]
    return cases


CASES = _table()
# batch seeds moved off a draw that puts an element of |t - a| or |t - v| inside the mirror's forward error (the no-kink condition)
SEED_BUMP: Dict[str, int] = {
    "G0-B65-gaussian": 1, "G0-B127-gaussian": 1, "G0-B128-gaussian": 4, "G0-B256-gaussian": 3, "G0-B257-gaussian": 1,
    "G0-B290-gaussian": 5, "G0-B1000-gaussian": 45, "G0-B65-ablation": 1, "G0-B290-ablation": 5, "G0-B290-aligned": 1,
    "G0-B65-outliers": 1, "G0-B290-outliers": 5, "G0-B290-saturated_trees": 1, "G1-B290-aligned": 1,
    "G2-B130-saturated_trees": 4, "G3-B290-ablation": 2}


def slice_rule(B: int) -> Tuple[int, int]:
    """(slices, rows per slice) of the evidence-gate and NODE parameter reductions, as the issue states the rule; the CPU suite
    checks it against the library's workspace sizes (tests/test_head_cases.py)."""
    if B <= 64:
        return 1, B
    S = min(-(-B // 8), 32)
    return S, -(-B // S)


# ---------------------------------------------------------------------------------------------------------------------
# problems
class Problem(NamedTuple):
    case: Case
    fus: Dict[str, torch.Tensor]
    clf: Dict[str, torch.Tensor]
    batch: Dict[str, torch.Tensor]
    masks: Optional[Dict[str, torch.Tensor]]
    up: Dict[str, torch.Tensor]          # seeded upstream gradients: d_fused, d_aux (fbwd), d_logits (cbwd)


def problem(c: Case) -> Problem:
    g = GEOMS[c.geom]
    base = c._replace(train=False)                     # a train-mode case runs on the batch of its dropout-off twin
    idx = CASES.index(base) if base in CASES else len(CASES)
    fus, clf = O.seeded_params(77 + 10 * list(GEOMS).index(c.geom), use_gnn=g.use_gnn, hidden=g.hidden, trees=g.trees, depth=g.depth,
                               aux_dim=g.aux or 2, use_aux=g.aux > 0)
    batch = O.seeded_batch(1000 + 7 * idx + SEED_BUMP.get(case_id(base), 0), c.B, aux_dim=g.aux or 2)
    B = c.B
    if c.family == "ablation":
        batch["visual_features"].zero_()
        batch["temporal_features"].zero_()
    elif c.family == "aligned":
        tw, tb = fus["text_proj.weight"], fus["text_proj.bias"]
        fus["visual_proj.weight"], fus["visual_proj.bias"] = 2.0 * tw[:, :512].clone(), 2.0 * tb.clone()
        fus["temporal_proj.weight"], fus["temporal_proj.bias"] = -1.0 * tw[:, :256].clone(), -1.0 * tb.clone()
        batch["text_features"][:, 256:] = 0.0
        batch["visual_features"] = batch["text_features"][:, :512].clone()
        batch["temporal_features"] = batch["text_features"][:, :256].clone()
    elif c.family == "outliers":
        for r in {0, B // 2, B - 1}:
            batch["text_features"][r] *= 20.0
        if B > 3:
            batch["text_features"][1] *= 1e-3
    elif c.family == "saturated_trees":
        # tau x 8 alone leaves the seeded gates' sigmoids in [0.03, 1] (feat - thresh lies in [-0.04, 0.19]): the low end is not
        # reached.  So two gates of every three also have their threshold moved by -+ 0.15; the third stays where it was.
        for t in range(g.trees):
            clf[f"node.trees.{t}.tau"] = clf[f"node.trees.{t}.tau"] * 8.0
            for k in range(g.depth):
                clf[f"node.trees.{t}.thresh.{k}"] = clf[f"node.trees.{t}.thresh.{k}"] + (-0.15, 0.15, 0.0)[(t * g.depth + k) % 3]
    elif c.family != "gaussian":
        raise KeyError(c.family)
    gen = torch.Generator().manual_seed(5000 + idx)
    up = {"d_fused": torch.randn(B, g.hidden, generator=gen) / B, "d_aux": torch.randn(B, 2, generator=gen) / B,
          "d_logits": torch.randn(B, 2, generator=gen) / B}
    masks = D.head_masks(B, g.hidden, g.trees, P_FUSION, P_CLF, P_NODE, FUSION_KEY, CLF_KEY) if c.train else None
    return Problem(c, fus, clf, batch, masks, up)


# ---------------------------------------------------------------------------------------------------------------------
# evaluation: the oracle and autograd in `dt`
_EV = tuple(f"{b}.evidence_proj.{i}.{w}" for b in ("attn_tv", "attn_ta", "attn_vu") for i in (0, 2) for w in ("weight", "bias"))


def _node_keys(clf) -> List[str]:
    return [k for k in clf if (k.startswith("node.trees.") and not k.endswith(".tau")) or k.startswith("bypass.")]


def _leaves(src, keys, dt, override=None):
    src = {**src, **(override or {})}
    return {k: src[k].to(dt).clone().requires_grad_(k in keys) for k in src}


def _cos01_dot_over_norms(x1, x2):
    """cos01 of O.fusion_forward with the cosine as dot / (norm x norm), the kernels' form, instead of the dot of two normalised
    vectors: the same number, other roundings (at cos = 1 the one lands on the clamp where the other may sit an ulp below)."""
    n1, n2 = x1.norm(dim=-1, keepdim=True).clamp_min(1e-12), x2.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    c = (x1 * x2).sum(dim=-1, keepdim=True) / (n1 * n2)
    return 0.5 * (c.clamp(-1, 1) + 1.0)


def _classifier_leafwise(p, fused, aux, train=False, masks=None):
    """O.classifier_forward with every leaf's probability as the product of its own gate factors, the kernels' form, instead of
    the level-by-level doubling (leaf l takes s of gate k where bit k of l is set): the same function; autograd then forms a
    gate's gradient as the signed sum over the leaves that the kernels form."""
    trees, depth, aux_w = O.clf_geometry(p)
    dt = p["pre.0.weight"].dtype
    x = fused.to(dt)
    if aux is not None and aux_w > 0:
        x = torch.cat([x, aux.to(dt)], dim=-1)
    h = O._drop(O.F.gelu(O.F.linear(x, p["pre.0.weight"], p["pre.0.bias"])), 0.0, False, O._mask(masks, "pre0"))
    h = O._drop(O.F.gelu(O.F.linear(h, p["pre.3.weight"], p["pre.3.bias"])), 0.0, False, O._mask(masks, "pre3"))
    outs = []
    for t in range(trees):
        tau = p[f"node.trees.{t}.tau"]
        s = [torch.sigmoid(tau * ((h * torch.softmax(p[f"node.trees.{t}.gates.{k}"], dim=0)).sum(dim=-1, keepdim=True) - p[f"node.trees.{t}.thresh.{k}"]))
             for k in range(depth)]
        cols = []
        for leaf in range(1 << depth):
            prob = None
            for k in range(depth):
                f = s[k] if (leaf >> k) & 1 else 1.0 - s[k]
                prob = f if prob is None else prob * f
            cols.append(prob)
        tm = None if masks is None else masks["tree"][:, 2 * t:2 * t + 2]
        outs.append(O._drop(torch.cat(cols, dim=1) @ p[f"node.trees.{t}.leaf_logits"], 0.0, False, tm))
    logits = torch.stack(outs, 0).mean(0) + O.F.linear(h, p["bypass.weight"], p["bypass.bias"])
    T = torch.clamp(p["temperature"], min=0.5, max=5.0)
    return {"logits": logits, "probs": F.softmax(logits / T, dim=-1), "temperature": T, "h": h}


def _fusion_ordered(p, feats, masks, B, slice_leaves):
    """O.fusion_forward with the kernels' orders of addition: the evidence gates' parameters enter through one set of leaves per
    row slice (their gradients are then added slice by slice, ascending), and fuse_mlp.0 is eight K-chunks summed in order."""
    dt = p["text_proj.weight"].dtype
    t = F.linear(feats["text_features"], p["text_proj.weight"], p["text_proj.bias"])
    a = F.linear(feats["audio_features"], p["audio_proj.weight"], p["audio_proj.bias"])
    v = F.linear(feats["visual_features"], p["visual_proj.weight"], p["visual_proj.bias"])
    u = F.linear(feats["temporal_features"], p["temporal_proj.weight"], p["temporal_proj.bias"])
    with torch.no_grad():
        conflict = 1.0 - _cos01_dot_over_norms(t, v)
        emo = t.abs().mean(dim=-1, keepdim=True).tanh()
        delay = 1.0 - _cos01_dot_over_norms(t, u)
        z = torch.zeros_like(emo)
    S, R = slice_rule(B)
    evs = {"attn_tv": torch.cat([conflict, emo, z], -1), "attn_ta": torch.cat([emo, z, z], -1), "attn_vu": torch.cat([delay, z, z], -1)}
    xy = {"attn_tv": (t, v), "attn_ta": (t, a), "attn_vu": (v, u)}
    co = {}
    for blk in evs:
        rows = []
        for s in range(S):
            r0, r1 = s * R, min((s + 1) * R, B)
            if r0 >= r1:
                continue                               # an empty slice adds zeros
            ps = {**p, **slice_leaves[s]}
            rows.append(O._co_attention(ps, blk, xy[blk][0][r0:r1], xy[blk][1][r0:r1], evs[blk][r0:r1]))
        co[blk] = torch.cat(rows, 0)
    cat = [t, a, v, u, t + a, t * a, (t - a).abs(), t + v, t * v, (t - v).abs(), t + u, v + u, co["attn_tv"], co["attn_ta"], co["attn_vu"]]
    if "gnn_proj.weight" in p:
        cat.append(F.linear(feats["gnn_feat"], p["gnn_proj.weight"], p["gnn_proj.bias"]))
    fused_cat = torch.cat(cat, -1)
    K = fused_cat.shape[1]
    acc = None
    for ch in range(8):
        k0, k1 = ch * K // 8, (ch + 1) * K // 8
        part = fused_cat[:, k0:k1] @ p["fuse_mlp.0.weight"][:, k0:k1].t()
        acc = part if acc is None else acc + part
    h = O._drop(F.gelu(acc + p["fuse_mlp.0.bias"]), 0.0, False, O._mask(masks, "fuse0"))
    fused = O._drop(F.gelu(F.linear(h, p["fuse_mlp.3.weight"], p["fuse_mlp.3.bias"])), 0.0, False, O._mask(masks, "fuse3"))
    logits = F.linear(fused, p["classifier.weight"], p["classifier.bias"])
    return {"fused": fused, "logits": logits, "fused_cat": fused_cat,
            "forensic": {"emotion_intensity": emo.squeeze(-1), "semantic_conflict": conflict.squeeze(-1), "temporal_delay": delay.squeeze(-1)}}


def _clf_ordered(p, fused, aux, masks, B, slice_leaves):
    """The classifier row slice by row slice, leaf by leaf (_classifier_leafwise), the NODE and bypass parameters through one set of
    leaves per slice."""
    S, R = slice_rule(B)
    outs = []
    for s in range(S):
        r0, r1 = s * R, min((s + 1) * R, B)
        if r0 >= r1:
            continue
        ms = None if masks is None else {k: m[r0:r1] for k, m in masks.items()}
        outs.append(_classifier_leafwise({**p, **slice_leaves[s]}, fused[r0:r1], None if aux is None else aux[r0:r1],
                                         train=masks is not None, masks=ms))
    return {"logits": torch.cat([o["logits"] for o in outs], 0), "probs": torch.cat([o["probs"] for o in outs], 0),
            "temperature": outs[0]["temperature"], "h": torch.cat([o["h"] for o in outs], 0)}


def _sum_slices(slice_leaves, key, grads_of):
    """Gradients of the per-slice leaves added in ascending slice order, in the leaves' dtype."""
    tot = None
    for s in sorted(slice_leaves):
        gs = grads_of.get(id(slice_leaves[s][key]))
        if gs is None:
            continue
        tot = gs.clone() if tot is None else tot + gs
    return tot


def _grads(outputs, leaves: List[torch.Tensor], grad_outputs=None):
    gs = torch.autograd.grad(outputs, leaves, grad_outputs, retain_graph=True, allow_unused=True)
    return {id(x): g for x, g in zip(leaves, gs)}


def evaluate(pr: Problem, dt, fused_in: Optional[torch.Tensor] = None, *, ordered: bool = False, kernel_forms: bool = False,
             keep_rows: Optional[int] = None,
             fus_override=None, clf_override=None, batch_override=None) -> Dict[str, torch.Tensor]:
    """Every compared tensor of the five checks in `dt` ("<check>/<tensor>"), plus "_cat" (the concat) and "_h" (the trees' input)
    for the conditions.  `fused_in`: the classifier-alone input (None: this evaluation's own `fused`, rounded to float32).
    ordered: the kernels' orders of addition and forms (the second float32 evaluation).  kernel_forms: the oracle with the
    kernels' forms alone, the leaf-by-leaf trees and -- for the two forensic cosines only -- dot / (norm x norm).  keep_rows: parameter gradients formed from rows
    [0, keep_rows) only (the row-loss mutants).  *_override: replaced parameters / inputs (the other mutants)."""
    g = GEOMS[pr.case.geom]
    B, train, masks = pr.case.B, pr.case.train, pr.masks
    batch = {**pr.batch, **(batch_override or {})}
    fkeys = [k for k in pr.fus if not k.startswith("semantic.")]
    ckeys = [k for k in pr.clf if k != "temperature" and not k.endswith(".tau")]
    pf = _leaves(pr.fus, fkeys, dt, fus_override)
    pc = _leaves(pr.clf, ckeys, dt, clf_override)
    names = [n for n in FEATS if g.use_gnn or n != "gnn_feat"]
    x = {n: batch[n].to(dt).clone().requires_grad_(True) for n in names}
    aux = batch["aux"].to(dt) if g.aux else None
    y = batch["label"]
    up = {k: v.to(dt) for k, v in pr.up.items()}
    if keep_rows is not None:
        live = (torch.arange(B) < keep_rows).to(dt)[:, None]
        up = {k: v * live for k, v in up.items()}
    S, R = slice_rule(B)
    ev_sl = {s: {k: pf[k].detach().clone().requires_grad_(True) for k in _EV} for s in range(S)} if ordered else None
    nd_sl = {s: {k: pc[k].detach().clone().requires_grad_(True) for k in _node_keys(pc)} for s in range(S)} if ordered else None

    def fusion():
        if ordered:
            return _fusion_ordered(pf, x, masks, B, ev_sl)
        return O.fusion_forward(pf, x, train=train, masks=masks)

    def classifier(fused, sl):
        if ordered:
            return _clf_ordered(pc, fused, aux, masks, B, sl)
        if kernel_forms:
            return _classifier_leafwise(pc, fused, aux, train=train, masks=masks)
        return O.classifier_forward(pc, fused, aux, train=train, masks=masks)

    def param_grads(outputs, grad_outputs, params, keys, sl):
        leaves = [params[k] for k in keys] + ([t for s in sl for t in sl[s].values()] if sl else [])
        got = _grads(outputs, leaves, grad_outputs)
        res = {}
        for k in keys:
            res[k] = _sum_slices(sl, k, got) if sl and k in sl[0] else got[id(params[k])]
        return res

    out: Dict[str, torch.Tensor] = {}
    fo = fusion()
    out["fwd/fused"], out["fwd/aux_logits"] = fo["fused"].detach(), fo["logits"].detach()
    for k, v in fo["forensic"].items():
        out[f"fwd/{k}"] = v.detach()
    out["_cat"] = fo["fused_cat"].detach()
    if kernel_forms and not ordered:
        Hd = g.hidden
        t_, v_, u_ = (out["_cat"][:, i * Hd:(i + 1) * Hd] for i in (0, 2, 3))
        out["fwd/semantic_conflict"] = (1.0 - _cos01_dot_over_norms(t_, v_)).squeeze(-1)
        out["fwd/temporal_delay"] = (1.0 - _cos01_dot_over_norms(t_, u_)).squeeze(-1)
    # fbwd: supplied gradients at fused and at the aux logits together
    for k, gk in param_grads([fo["fused"], fo["logits"]], [up["d_fused"], up["d_aux"]], pf, fkeys, ev_sl).items():
        out[f"fbwd/{k}"] = gk
    full = [pr.up["d_fused"].to(dt), pr.up["d_aux"].to(dt)]
    gx = _grads([fo["fused"], fo["logits"]], [x[n] for n in names], full)
    for n in names:
        out[f"fbwd/d_{n}"] = gx[id(x[n])]
    # chain: fusion -> classifier -> cross-entropy
    nd_chain = {s: {k: v.detach().clone().requires_grad_(True) for k, v in d.items()} for s, d in nd_sl.items()} if ordered else None
    co = classifier(fo["fused"], nd_chain)
    rows = F.cross_entropy(co["logits"], y, reduction="none")
    loss = rows.sum() / B
    out["chain/loss"], out["chain/logits"], out["chain/fused"] = loss.detach().reshape(1), co["logits"].detach(), fo["fused"].detach()
    loss_p = loss if keep_rows is None else rows[:keep_rows].sum() / B
    for k, gk in param_grads([loss_p], None, pf, [k for k in fkeys if not k.startswith("classifier.")], ev_sl).items():
        out[f"chain/fusion.{k}"] = gk
    for k, gk in param_grads([loss_p], None, pc, ckeys, nd_chain).items():
        out[f"chain/clf.{k}"] = gk
    out["_h"] = co["h"].detach()
    # the classifier alone
    fin = (out["fwd/fused"].float() if fused_in is None else fused_in).to(dt).clone().requires_grad_(True)
    ca = classifier(fin, nd_sl)
    out["cfwd/logits"], out["cfwd/probs"], out["cfwd/temperature"] = ca["logits"].detach(), ca["probs"].detach(), ca["temperature"].detach().reshape(1)
    for k, gk in param_grads([ca["logits"]], [up["d_logits"]], pc, ckeys, nd_sl).items():
        out[f"cbwd/{k}"] = gk
    out["cbwd/d_fused"] = _grads([ca["logits"]], [fin], [pr.up["d_logits"].to(dt)])[id(fin)]
    missing = [k for k, v in out.items() if v is None]
    assert not missing, missing
    return out


class Refs(NamedTuple):
    problem: Problem
    ref: Dict[str, torch.Tensor]          # float64
    mir: Dict[str, torch.Tensor]          # float32: the oracle as it stands (member 0)
    fused_in: torch.Tensor                # the classifier-alone input: ref64 fused rounded to float32
    yard: Dict[str, float]                # pooled vector -> the float32 oracle's largest error over its N_ENS orders


N_ENS = 12               # float32 evaluations behind a case's yardstick (module docstring)


class _ChunkedF:
    """torch.nn.functional with every Linear summed over 2 to 5 chunks of its K, ascending or descending."""

    def __init__(self, m: int):
        self.m = m

    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, b=None):
        K, c = w.shape[1], min(2 + self.m % 4, w.shape[1])
        if c < 2:
            return F.linear(x, w, b)
        phi = 0.8 * (((self.m * 0.6180339887) % 1.0) - 0.5)              # the cuts move with m as well
        edges = [0, *sorted({min(K - 1, max(1, round(K * (j + phi) / c))) for j in range(1, c)}), K]
        parts = [x[..., k0:k1] @ w[:, k0:k1].t() for k0, k1 in zip(edges[:-1], edges[1:])]
        if self.m % 2:
            parts.reverse()
        acc = parts[0]
        for part in parts[1:]:
            acc = acc + part
        return acc if b is None else acc + b


_ROWWISE = ("fwd/", "fbwd/d_", "cfwd/logits", "cfwd/probs", "cbwd/d_fused", "chain/logits", "chain/fused", "_cat", "_h")


def reordered(pr: Problem, fused_in: torch.Tensor, m: int) -> Dict[str, torch.Tensor]:
    """The float32 oracle on `pr` in the m-th legitimate order: the rows of the batch (inputs, labels, masks, upstream
    gradients) in a seeded order, every Linear over chunks of K.  Row-indexed results come back in the case's own row order."""
    if m == 0:
        return evaluate(pr, torch.float32, fused_in)
    perm = torch.randperm(pr.case.B, generator=torch.Generator().manual_seed(9000 + m))
    inv = torch.argsort(perm)

    def rows(d):
        return None if d is None else {k: v[perm] for k, v in d.items()}
    q = pr._replace(batch=rows(pr.batch), masks=rows(pr.masks), up=rows(pr.up))
    saved, O.F = O.F, _ChunkedF(m)
    try:
        out = evaluate(q, torch.float32, fused_in[perm], kernel_forms=bool(m % 2))
    finally:
        O.F = saved
    return {k: (v[inv] if k.startswith(_ROWWISE) else v) for k, v in out.items()}


def _references(c: Case) -> Refs:
    pr = problem(c)
    ref = evaluate(pr, torch.float64)
    fused_in = ref["fwd/fused"].float()
    R = pooled(ref)
    mir, yard = None, {k: 0.0 for k in R}
    for m in range(N_ENS):
        out = reordered(pr, fused_in, m)
        mir = out if m == 0 else mir
        for k, v in pooled(out).items():
            yard[k] = max(yard[k], _err(v, R[k]))
    return Refs(pr, ref, mir, fused_in, yard)


references = functools.lru_cache(maxsize=2)(_references)


# ---------------------------------------------------------------------------------------------------------------------
# pooling, bounds, figures
_BIASES = ("evidence_proj.2.bias", "bypass.bias", "classifier.bias")
_GRAD_CHECKS = ("fbwd", "cbwd", "chain")


def _pool_of(chk: str, t: str) -> Optional[str]:
    """The pool a gradient joins (None: it stands alone)."""
    if chk not in _GRAD_CHECKS:
        return None
    if ".thresh." in t:
        return "thresh"
    if t.endswith(_BIASES):
        return "biases"
    return None


def pooled(out: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """{name: vector float64} of an evaluation: the compared vectors, the thresholds and the tiny biases of a check pooled as the
    module docstring says.  Keys starting with "_" are dropped."""
    res: Dict[str, torch.Tensor] = {}
    groups: Dict[Tuple[str, str], List[Tuple[str, torch.Tensor]]] = {}
    for name, v in out.items():
        if name.startswith("_"):
            continue
        chk, t = name.split("/", 1)
        v = v.detach().double().reshape(-1).cpu()
        pool = _pool_of(chk, t)
        if pool:
            groups.setdefault((chk, pool), []).append((t, v))
        else:
            res[name] = v
    for (chk, pool), members in sorted(groups.items()):
        res[f"{chk}/{pool}(all)"] = torch.cat([v for _, v in sorted(members, key=lambda e: e[0])])
    return res


def _err(got: torch.Tensor, ref: torch.Tensor) -> float:
    e = (got - ref).abs().max().item() if ref.numel() else 0.0
    return math.inf if e != e else e


LOSS = "chain/loss"


def figures(got: Dict[str, torch.Tensor], r: Refs, check: Optional[str] = None):
    """({vector: (error, bound, error / the float32 oracle's error)} of every compared vector of the case but the loss, and the
    loss's (error, float32 oracle's error), both relative to the loss, for `loss_table_ratio`; None under another `check`).
    error / oracle error may reach BOUND_FACTOR; it is inf where a NaN came out or where the oracle is exact and `got` is not."""
    G, R = pooled(got), pooled(r.ref)
    assert set(G) == set(R) == set(r.yard), sorted(set(G) ^ set(R))
    per_case, loss = {}, None
    for k in R:
        if check is not None and not k.startswith(check + "/"):
            continue
        assert G[k].shape == R[k].shape, (k, G[k].shape, R[k].shape)
        e, m = _err(G[k], R[k]), r.yard[k]
        if k == LOSS:
            loss = (e / abs(R[k].item()), m / abs(R[k].item()))
        else:
            per_case[k] = (e, BOUND_FACTOR * m, (e / m) if m > 0 else (0.0 if e == 0 else math.inf))
    return per_case, loss


def loss_table_ratio(entries) -> float:
    """entries: the loss's (relative error, float32 oracle's relative error) of every case.  max error / (BOUND_FACTOR x max
    oracle error): at most 1 to pass."""
    gmax = max(e for e, _ in entries)
    m = max(m for _, m in entries)
    if gmax == 0.0:
        return 0.0
    return math.inf if (m == 0.0 or not math.isfinite(gmax)) else gmax / (BOUND_FACTOR * m)


def worst(big) -> Tuple[float, Optional[str]]:
    """(worst error / bound, where): at most 1 to pass."""
    w, at = 0.0, None
    for k, (e, b, ratio) in big.items():
        x = ratio / BOUND_FACTOR
        if x >= w:
            w, at = x, k
    return w, at


def old_criteria(got: Dict[str, torch.Tensor], r: Refs) -> float:
    """The chain check on the older head tests' criteria (outputs 2e-5 max-abs, gradients 5e-4 of the tensor's scale, tensor by
    tensor): worst error / tolerance, at most 1 to pass them."""
    w = 0.0
    for k, ref in r.ref.items():
        if not k.startswith("chain/"):
            continue
        e = _err(got[k].double().reshape(-1), ref.reshape(-1))
        if k in ("chain/loss", "chain/logits", "chain/fused"):
            w = max(w, e / TOL_OUT)
        else:
            scale = max(ref.abs().max().item(), ref.norm().item() / max(1.0, ref.numel() ** 0.5), 1e-9)
            w = max(w, e / scale / TOL_GRAD)
    return w


# ---------------------------------------------------------------------------------------------------------------------
# conditions
def gate_sigmoids(pr: Problem, h: torch.Tensor) -> torch.Tensor:
    """The trees' gate sigmoids (B, trees x depth) at `h`, float64."""
    g = GEOMS[pr.case.geom]
    cols = []
    for t in range(g.trees):
        for k in range(g.depth):
            alpha = torch.softmax(pr.clf[f"node.trees.{t}.gates.{k}"].double(), 0)
            cols.append(torch.sigmoid(pr.clf[f"node.trees.{t}.tau"].double() * ((h.double() * alpha).sum(-1) - pr.clf[f"node.trees.{t}.thresh.{k}"].double())))
    return torch.stack(cols, 1)


def conditions(r: Refs) -> Dict[str, float]:
    """What a case must satisfy (tests/test_head_cases.py asserts it).  kink_margin: min over rows and elements of |t - a| and
    |t - v| in float64, over BOUND_FACTOR x the mirror's largest forward error in that row of that CAT slot; above 1 no sign of
    either difference can differ between float64 and anything inside the forward bound."""
    g = GEOMS[r.problem.case.geom]
    H = g.hidden
    margin = math.inf
    for slot in (6, 9):                                    # cat = [t a v u | t+a t*a |t-a| | t+v t*v |t-v| | ...]
        ref = r.ref["_cat"][:, slot * H:(slot + 1) * H]
        err = (r.mir["_cat"][:, slot * H:(slot + 1) * H].double() - ref).abs().max(dim=1, keepdim=True).values
        margin = min(margin, (ref / (BOUND_FACTOR * err.clamp_min(1e-300))).min().item())
    f = {k: r.ref[f"fwd/{k}"] for k in ("emotion_intensity", "semantic_conflict", "temporal_delay")}
    s = gate_sigmoids(r.problem, r.ref["_h"])
    return {"kink_margin": margin, "temperature": float(r.ref["cfwd/temperature"]),
            "conflict_max": f["semantic_conflict"].max().item(), "delay_min": f["temporal_delay"].min().item(),
            "emotion": f["emotion_intensity"], "sigmoid_min": s.min().item(), "sigmoid_max": s.max().item()}


# ---------------------------------------------------------------------------------------------------------------------
# mutants
def trunc10(w: torch.Tensor) -> torch.Tensor:
    """float32 with the 13 low mantissa bits cleared: 10 explicit bits, an xf32-style MFMA operand."""
    return (w.float().contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


_QKV = [f"{b}.{p}.weight" for b in ("attn_tv", "attn_ta", "attn_vu") for p in ("q", "k", "v")]
TF32_LINEARS: "OrderedDict[str, Tuple[str, List[str]]]" = OrderedDict(
    [(f"{n}_proj", ("fus", [f"{n}_proj.weight"])) for n in ("text", "audio", "visual", "temporal", "gnn")] +
    [("qkv", ("fus", _QKV)), ("fuse_mlp.0", ("fus", ["fuse_mlp.0.weight"])), ("fuse_mlp.3", ("fus", ["fuse_mlp.3.weight"])),
     ("pre.0", ("clf", ["pre.0.weight"])), ("pre.3", ("clf", ["pre.3.weight"])), ("bypass", ("clf", ["bypass.weight"]))])
MUTANTS = tuple(f"tf32_{n}" for n in TF32_LINEARS) + ("drop_last_row", "slices_capped_at_256_rows", "ablation_bias_only")


def mutant_cases(m: str) -> List[Case]:
    if m == "drop_last_row":
        return [Case("G0", b, "gaussian") for b in (65, 257, 290)]
    if m == "slices_capped_at_256_rows":
        return [Case("G0", b, "gaussian") for b in (257, 290, 1000)]
    if m == "ablation_bias_only":
        return [Case("G0", 65, "ablation")]
    return [Case("G0", 65, "gaussian")]


def run_mutant(m: str, r: Refs) -> Dict[str, torch.Tensor]:
    """The float32 mirror with the mutant's mistake."""
    pr, B = r.problem, r.problem.case.B
    if m.startswith("tf32_"):
        side, keys = TF32_LINEARS[m[5:]]
        ov = {k: trunc10((pr.fus if side == "fus" else pr.clf)[k]) for k in keys}
        return evaluate(pr, torch.float32, r.fused_in, **{("fus_override" if side == "fus" else "clf_override"): ov})
    if m in ("drop_last_row", "slices_capped_at_256_rows"):
        return evaluate(pr, torch.float32, r.fused_in, keep_rows=B - 1 if m == "drop_last_row" else 256)
    if m == "ablation_bias_only":
        return evaluate(pr, torch.float32, r.fused_in, batch_override={"text_features": torch.zeros_like(pr.batch["text_features"])})
    raise KeyError(m)
