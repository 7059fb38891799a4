"""CPU: the case table of tests/test_gpu_gemm_f32.py (tests/gemm_f32_cases.py) still reaches every one of the 20 kernel
instantiations of csrc/gemm_f32.hip and every edge it is there for.  The form of each case is read from the library's own
host-side validation + choice (ufnd_diag_gemm_f32_plan: no launch, no GPU), so a retuned threshold that moves the cases off a form
fails here and the cases have to be chosen again.  The launchers' argument checks are exercised on the same entry."""
import ctypes as C

import pytest

from tests import gemm_f32_cases as G


@pytest.fixture(scope="module")
def D():
    from tools import _diaglib
    _diaglib.diag()
    return _diaglib


def _forms(D):
    return {c.id: G.plan(D, c)[0] for c in G.CASES}


def _cdiv(a, b):
    return (a + b - 1) // b


def _up(a, b):
    return _cdiv(a, b) * b


def _nt_ranges(form, p):
    """[(k0, k1)] of the four waves of every K split, as the kernels cut them"""
    K, out = p["K"], []
    if form.startswith("nt16"):
        sub = _up(_cdiv(K, 4), 16)
        return [[(min(K, w * sub), min(K, min(K, w * sub) + sub)) for w in range(4)]]
    kblk = _up(_cdiv(K, p["ksplit"]), 32)
    for ks in range(p["ksplit"]):
        kb0, kb1 = ks * kblk, min(K, ks * kblk + kblk)
        out.append([(kb0 + w * kblk // 4, min(kb1, kb0 + (w + 1) * kblk // 4)) for w in range(4)])
    return out


def _nn_ranges(form, p):
    N = p["N"]
    if form == "nn16":
        sub = _up(_cdiv(N, 4), 16)
        return [[(min(N, w * sub), min(N, min(N, w * sub) + sub)) for w in range(4)]]
    nblk, out = _up(_cdiv(N, p["nsplit"]), 32), []
    for ns in range(p["nsplit"]):
        nb0, nb1 = ns * nblk, min(N, ns * nblk + nblk)
        out.append([(nb0 + w * nblk // 4, min(nb1, nb0 + (w + 1) * nblk // 4)) for w in range(4)])
    return out


def _geometry(form, c):
    """What is ragged in a launch, from the kernels' own cuts: per problem, every wave's contraction sub-range (nt, nn; for tn
    the four row ranges of the row-split forms, else the one chain and its last pass) and how far the last column strip is filled"""
    out = []
    for p in c.probs:
        if c.kind == "nt":
            out.append(tuple(map(tuple, _nt_ranges(form, p))))
        elif c.kind == "nn":
            strip = {"nn16": 16, "nn<4>": 128, "nn<2>": 64, "nn<1>": 32}[form]
            out.append((tuple(map(tuple, _nn_ranges(form, p))), p["K"] % strip))
        else:
            M = p["M"]
            per = _up(_cdiv(M, 4), 8)
            rows = tuple((w * per, min(M, (w + 1) * per)) for w in range(4)) if form.split(",")[1] == "1" else ((0, M),)
            out.append((rows, M % 32, p["K"] % 128, p["K"] % 64))
    return tuple(out)


def test_struct_mirrors_and_form_names_match_the_library(D):
    s = (C.c_int * 4)()
    D.diag().ufnd_diag_gemm_f32_sizes(s)
    assert list(s) == [C.sizeof(D.NtProb), C.sizeof(D.NnProb), C.sizeof(D.TnProb), len(D.GEMM_F32_FORMS)] and s[3] == 20


def test_every_instantiation_is_reached(D):
    forms = _forms(D)
    by = {}
    for c in G.CASES:
        print(f"{c.id:24s} -> {forms[c.id]:11s} grid {G.plan(D, c)[1]:4d}   {c.tail}")
        by.setdefault(forms[c.id], []).append(c)
    print({f: len(by.get(f, [])) for f in D.GEMM_F32_FORMS})
    assert set(by) == set(D.GEMM_F32_FORMS), set(D.GEMM_F32_FORMS) - set(by)
    for f, cs in by.items():
        assert f.split("<")[0].rstrip("16") == cs[0].kind
        if f not in G.SEG_FORMS:
            assert len({_geometry(f, c) for c in cs}) >= 2, f
    for c in G.CASES:
        assert 1 <= len(c.probs) <= G.MAX_PROB and all(G.exact_ok(c.kind, p) for p in c.probs), c.id


def test_nt_cases_cover_their_edges(D):
    forms = _forms(D)
    ps = [(forms[c.id], p) for c in G.CASES if c.kind == "nt" for p in c.probs]
    assert {1, 17, 33, 65} <= {p["M"] for _, p in ps}
    assert any(p["K"] % 8 and p["K"] % 16 for _, p in ps) and any(p["K"] < 8 for _, p in ps)
    for fam in ("nt16", "nt<"):       # both tile sizes: a ragged K tail, and a wave with an empty sub-range
        mine = [(f, p) for f, p in ps if f.startswith(fam)]
        assert any(p["K"] % (16 if fam == "nt16" else 8) for f, p in mine), fam
        assert any(k1 <= k0 for f, p in mine for split in _nt_ranges(f, p) for k0, k1 in split), fam
        assert any(all(k1 > k0 for k0, k1 in split) for f, p in mine for split in _nt_ranges(f, p)), fam    # and one with all four at work
    split = [(f, p) for f, p in ps if p["ksplit"] > 1]
    assert any(0 < r[-1][3][1] - r[-1][0][0] < r[0][3][1] - r[0][0][0] for f, p in split for r in [_nt_ranges(f, p)]), "no short last split"
    assert any(r[-1][0][0] >= p["K"] for f, p in split for r in [_nt_ranges(f, p)]), "no empty last split"
    assert any(p["ldx"] > p["K"] for _, p in ps) and any(p["ldw"] > p["K"] for _, p in ps)
    assert any(p["ldy"] > p["N"] for _, p in ps) and any(p["Z"] and p["ldz"] > p["N"] for _, p in ps)
    assert any(p["a8"] for _, p in ps) and any(p["ldw"] % 4 for _, p in ps)
    for key in ("bias", "Z", "act"):
        assert {bool(p[key]) for _, p in ps} == {False, True}, key
    # the in-kernel epilogue (bias, Z, GELU, mask) of every form: an unsplit case that draws a mask and one with Z and GELU
    for f in D.GEMM_F32_FORMS[:6]:
        mine = [p for g, p in ps if g == f and p["ksplit"] == 1]
        assert any(p["drop"] > 0 for p in mine) and any(p["act"] == 1 and p["Z"] for p in mine), f
        assert any(p["drop"] > 0 and p["ldy"] != p["N"] and p["M"] > 1 for p in mine), f     # the mask index is m N + n, not m ldy + n


def test_nn_cases_cover_their_edges(D):
    forms = _forms(D)
    ps = [(forms[c.id], p) for c in G.CASES if c.kind == "nn" for p in c.probs]
    for f, w in (("nn16", 16), ("nn<4>", 128), ("nn<2>", 64), ("nn<1>", 32)):
        assert any(p["K"] % w for g, p in ps if g == f), f                       # K ends inside a strip
    assert any(p["K"] % 4 == 2 for _, p in ps)
    assert any(sum(n1 <= n0 for n0, n1 in split) == 2 and split[0][1] > split[0][0] for f, p in ps if p["nsplit"] > 1
               for split in _nn_ranges(f, p)), "no split that feeds two waves only"
    assert any(p["nsplit"] > 1 and p["ldo"] > p["K"] for _, p in ps)
    assert {(p["actZ"], p["add"]) for _, p in ps if p["nsplit"] == 1} == {(False, False), (True, False), (False, True), (True, True)}
    d4 = [p for g, p in ps if g == "nn<4>" and p["drop"] > 0]
    assert any(p["drop_ld"] % 4 == 0 for p in d4) and any(p["drop_ld"] % 4 for p in d4)
    for f in ("nn16", "nn<4>", "nn<2>", "nn<1>"):     # every form draws a mask at a stride that is not the output's
        assert any(p["drop"] > 0 and p["drop_ld"] != p["ldo"] for g, p in ps if g == f), f
    assert any(p["a8"] for _, p in ps)


def test_tn_cases_cover_their_edges(D):
    forms = _forms(D)
    cs = [c for c in G.CASES if c.kind == "tn"]
    ps = [(forms[c.id], p) for c in cs for p in c.probs]
    assert {1, 7, 33, 128, 129, 135} <= {p["M"] for _, p in ps}
    assert {p["db"] for _, p in ps} == {False, True}
    vec = {"tn<4": 4, "tn<2": 2}
    assert any(p["K"] % (32 * v) for f, p in ps for k, v in vec.items() if f.startswith(k))
    # db comes from strip 0 alone: a launch of one strip and one of several, with db
    assert any(p["db"] and p["K"] <= 64 for _, p in ps) and any(p["db"] and p["K"] > 128 for _, p in ps)

    def widths(c):
        return {4 if (p["K"] % 4 == 0 and p["ldx"] % 4 == 0 and p["ldw"] % 4 == 0 and not p["a8"] and p["seg_x"] % 4 == 0) else 2 for p in c.probs}
    mixed = [c for c in cs if widths(c) == {2, 4}]
    assert any(max(p["M"] for p in c.probs) < 128 and forms[c.id] == "tn<-1,0,0>" for c in mixed)
    assert any(min(p["M"] for p in c.probs) >= 128 and forms[c.id] == "tn<2,1,0>" for c in mixed)
    for f in G.SEG_FORMS:
        mine = [p for g, p in ps if g == f]
        assert any(p["seg_rows"] % 4 and p["seg_dy"] > p["seg_rows"] * p["lddy"] and p["seg_x"] > p["seg_rows"] * p["ldx"] for p in mine), f


def test_group_limits(D):
    sizes = {k: {len(c.probs) for c in G.CASES if c.kind == k} for k in ("nt", "nn", "tn")}
    for k, s in sizes.items():
        assert (2 in s or 3 in s) and 16 in s, (k, s)
    assert any(len(c.probs) == 2 for c in G.CASES)
    for c in G.CASES:
        if len(c.probs) > 1:
            assert len({(p["M"], p["N"], p["K"]) for p in c.probs}) > 1, c.id
    for kind, cid in (("nt", "nt16_group16"), ("nn", "nn16_group16"), ("tn", "tnmix_group16")):
        probs = G.make_probs(D, G.BY_ID[cid])
        assert D.gemm_f32_plan(kind, probs)[0] == 0
        rc, _, _, err = D.gemm_f32_plan(kind, probs + probs[:1])
        assert rc == 1 and "17 problems" in err, (kind, err)
        assert D.gemm_f32_plan(kind, [])[0] == 1


def _refused(D, kind, case_id, needle, idx=0, **change):
    probs = G.make_probs(D, G.BY_ID[case_id])
    assert D.gemm_f32_plan(kind, probs)[0] == 0
    for k, v in change.items():
        setattr(probs[idx], k, v)
    rc, _, _, err = D.gemm_f32_plan(kind, probs)
    assert rc == 1 and needle in err, (kind, change, rc, err)


def test_every_argument_check_of_the_three_launchers_refuses(D):
    nt, nn, tn = "nt16_m33_k21", "nn16_group2", "tn4_m7_k132"
    for ch, needle in (({"X": None}, "null/empty"), ({"W": None}, "null/empty"), ({"Y": None}, "null/empty"), ({"M": 0}, "null/empty"),
                       ({"K": 0}, "null/empty"), ({"N": 48}, "multiple of 32"), ({"ldx": 26}, "X must be"), ({"X": 0x1008}, "X must be"),
                       ({"ldw": 23}, "W must be"), ({"W": 0x1004}, "W must be"), ({"ksplit": 0}, "ksplit"), ({"ksplit": 65}, "ksplit"),
                       ({"Y": 0x1008}, "Y alignment"), ({"ldy": 34}, "Y alignment"), ({"Z": 0x1008}, "Z alignment"), ({"ldz": 34}, "Z alignment"),
                       ({"bias": 0x1008}, "bias alignment"), ({"M": 1 << 27}, "too large")):
        _refused(D, "nt", nt, needle, **ch)
    for ch, needle in (({"dY": None}, "null/empty"), ({"W": None}, "null/empty"), ({"out": None}, "null/empty"), ({"M": 0}, "null/empty"),
                       ({"K": 0}, "null/empty"), ({"N": 16}, "multiple of 32"), ({"lddy": 66}, "dY alignment"), ({"dY": 0x1008}, "dY alignment"),
                       ({"K": 33}, "W alignment"), ({"ldw": 35}, "W alignment"), ({"W": 0x1004}, "W alignment"), ({"nsplit": 0}, "nsplit"),
                       ({"nsplit": 65}, "nsplit"), ({"M": 1 << 27}, "too large"), ({"actZ": None}, "without actZ")):
        _refused(D, "nn", nn, needle, **ch)
    _refused(D, "nn", nn, "without actZ", idx=1, drop_p=0.5)          # the second problem has no actZ
    _refused(D, "nn", nn, "drop_ld=32", drop_ld=32)                   # K = 34: two elements of a row would share an index
    _refused(D, "nn", nn, "drop_ld=", drop_ld=(1 << 31) // 17 + 1)     # M = 17: the last row's index leaves 31 bits
    probs = G.make_probs(D, G.BY_ID[nn])
    probs[0].drop_ld = (1 << 31) // 17
    probs[1].drop_ld = 0                                              # no mask drawn: drop_ld is not looked at
    assert D.gemm_f32_plan("nn", probs)[0] == 0
    for ch, needle in (({"dY": None}, "null/empty"), ({"X": None}, "null/empty"), ({"dW": None}, "null/empty"), ({"M": 0}, "null/empty"),
                       ({"K": 0}, "null/empty"), ({"N": 80}, "multiple of 32"), ({"K": 131}, "X/dW alignment"), ({"ldx": 137}, "X/dW alignment"),
                       ({"ldw": 141}, "X/dW alignment"), ({"X": 0x1004}, "X/dW alignment"), ({"dW": 0x1004}, "X/dW alignment"),
                       ({"seg_rows": -1}, "segments"), ({"seg_rows": 2, "seg_dy": 200, "seg_x": 300}, "segments"),
                       ({"seg_rows": 7, "seg_dy": 0, "seg_x": 1000}, "segments"), ({"seg_rows": 7, "seg_dy": 1000, "seg_x": 0}, "segments"),
                       ({"seg_rows": 7, "seg_dy": 1000, "seg_x": 1001}, "segment stride")):
        _refused(D, "tn", tn, needle, **ch)
    _refused(D, "tn", "tnmix_below128", "segmented and one-panel", idx=1, seg_rows=7, seg_dy=1000, seg_x=1000)
    _refused(D, "tn", "tnmixseg_m33", "segmented and one-panel", idx=1, seg_rows=0)
    f, g = C.c_int(), C.c_int()
    for kind, name in enumerate(("nt", "nn", "tn")):      # a null problem array has its own message
        assert D.diag().ufnd_diag_gemm_f32_plan(kind, None, 1, C.byref(f), C.byref(g)) == 1
        assert D.diag().ufnd_diag_last_error().decode() == f"{name}: null problem array"
    assert D.diag().ufnd_diag_gemm_f32_plan(3, None, 1, C.byref(f), C.byref(g)) == 1          # an unknown kind is the entry's own refusal
    assert b"kind 3" in D.diag().ufnd_diag_last_error()


def test_product_library_does_not_export_the_seam():
    import torch  # noqa: F401
    from ultrafnd_git_amd.build import build
    lib = C.CDLL(str(build()))
    for name in ("ufnd_diag_gemm_f32_nt", "ufnd_diag_gemm_f32_nn", "ufnd_diag_gemm_f32_tn", "ufnd_diag_gemm_f32_plan"):
        assert not hasattr(lib, name), name
