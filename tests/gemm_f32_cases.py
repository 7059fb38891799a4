"""Case table of the fp32 skinny-GEMM family (csrc/gemm_f32.hip), shared by tests/test_gemm_f32_cases.py (CPU: the table still
reaches every kernel form and edge, read from the library's own host-side choice) and tests/test_gpu_gemm_f32.py (GPU: every
case against float64).

A case is one launch: a kind ("nt", "nn", "tn") and one to sixteen problems.  A problem is a plain dict of the fields of
NtProb / NnProb / TnProb, with booleans where the structure has optional pointers (bias, Z, actZ, add, db) and `a8` for an
operand that is aligned to 8 bytes only (W of nt / nn, X and dW of tn).  Strides default to the tightest legal ones.

Shapes are the smallest that put a launch on the form it is there for: the launchers choose by tile counts (nt: summed
N / 32 <= 128 -> 16x16 tiles; nn: summed cdiv(K, 32) <= 128 -> 16x16 tiles, then block counts 64 / 256; tn: 128 rows), so the
epilogues of the 32x32 forms need N = 4128 (nt) or K > 4096 (nn) unless the launch is split."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple

MAX_PROB = 16
DROP_LAYER = 7          # any tag: the mirror is keyed with the same one


class Case(NamedTuple):
    id: str
    kind: str
    probs: List[Dict]
    tail: str = ""      # what is ragged in this case, in words (the CPU test compares the real wave ranges)


def _up(x, m):
    return (x + m - 1) // m * m


def nt(M, N, K, ksplit=1, *, ldx=None, ldw=None, ldy=None, ldz=None, bias=True, Z=False, act=0, drop=0.0, a8=False):
    return dict(M=M, N=N, K=K, ksplit=ksplit, ldx=ldx or _up(K, 4), ldw=ldw or _up(K, 4), ldy=ldy or N, ldz=ldz or N, bias=bias, Z=Z,
                act=act, drop=drop, a8=a8)


def nn(M, N, K, nsplit=1, *, lddy=None, ldw=None, ldo=None, ldz=None, ldadd=None, actZ=False, add=False, drop=0.0, drop_ld=None,
       a8=False):
    return dict(M=M, N=N, K=K, nsplit=nsplit, lddy=lddy or N, ldw=ldw or K, ldo=ldo or K, ldz=ldz or K, ldadd=ldadd or K, actZ=actZ,
                add=add, drop=drop, drop_ld=drop_ld or K, a8=a8)


def tn(M, N, K, *, lddy=None, ldx=None, ldw=None, db=True, seg_rows=0, seg_dy=0, seg_x=0, a8=False):
    lddy, ldx = lddy or N, ldx or K
    if seg_rows:
        seg_dy, seg_x = seg_dy or seg_rows * lddy, seg_x or seg_rows * ldx
    return dict(M=M, N=N, K=K, lddy=lddy, ldx=ldx, ldw=ldw or K, db=db, seg_rows=seg_rows, seg_dy=seg_dy, seg_x=seg_x, a8=a8)


P = 0.25        # dropout probability of the cases that draw a mask (keep multiplier 4/3: not a power of two)

CASES: List[Case] = [
    # ------------------------------------------------------------------ nt, 16x16 tiles (sub-range of a wave: K / 4 rounded up to 16)
    Case("nt16_m33_k21", "nt", [nt(33, 32, 21, ldx=24, ldw=24, ldy=36, ldz=40, Z=True, act=1)], "K=21: tail 5, waves 2 3 empty"),
    Case("nt16_m1_k5", "nt", [nt(1, 64, 5, bias=False, drop=P, ldy=68)], "K=5 < 8: wave 0 tail only"),
    Case("nt16_m17_k100", "nt", [nt(17, 32, 100, ldx=104, ldw=108, ldy=40, drop=P, act=1)], "K=100: wave 3 holds a tail of 4"),
    Case("nt16_m65_k256", "nt", [nt(65, 96, 256, Z=True)], "K=256: no tail, 64 per wave"),
    Case("nt16w2_m33_k21", "nt", [nt(33, 32, 21, ldx=24, ldw=22, Z=True, act=1)], "ldw=22: 8-B rows, K=21"),
    Case("nt16w2_m65_k70", "nt", [nt(65, 64, 70, a8=True, ldw=76, drop=P, ldy=72, act=1, Z=True)], "W 8-B aligned, K=70: waves of 32 32 6 0"),
    Case("nt16_group2", "nt", [nt(17, 32, 40, act=1, Z=True), nt(33, 64, 9, bias=False)], "two problems, K=40 and 9"),
    Case("nt16_group16", "nt", [nt(1 + 3 * i, 32 * (1 + i % 3), 7 + 5 * i, bias=bool(i % 2), act=i % 2, Z=(i % 4 == 0), drop=P if i % 3 == 0 else 0.0)
                                  for i in range(16)], "sixteen unequal problems"),
    # ------------------------------------------------------------------ nt, 32x32 tiles: split K (bare partial sums) ...
    Case("nt1_m33_k70_s2", "nt", [nt(33, 32, 70, 2, bias=False)], "ksplit 2: splits of 64 and 6"),
    Case("nt1_m17_k21_s3", "nt", [nt(17, 64, 21, 3, ldx=24, ldw=28, bias=False)], "ksplit 3, K=21: last two splits empty"),
    Case("nt1w2_m33_k70_s2", "nt", [nt(33, 32, 70, 2, a8=True, ldw=72, bias=False)], "ksplit 2, W 8-B aligned"),
    Case("nt1w2_m1_k13_s1", "nt", [nt(1, 4128, 13, ldw=14, ldx=16, act=1, Z=True, ldz=4132, drop=P)], "epilogue form, ldw=14, K=13"),
    Case("nt2_m65_k709_s22", "nt", [nt(65, 256, 709, 22, ldx=712, ldw=712, bias=False)], "ksplit 22 of 64: split 11 holds 5, 12.. empty"),
    Case("nt2w2_m65_k709_s22", "nt", [nt(65, 256, 709, 22, ldx=712, ldw=710, bias=False)], "ksplit 22, ldw=710"),
    # ... and the in-kernel epilogue (only launches wider than 128 tiles of 32 reach it unsplit)
    Case("nt1_m17_n4128_k21", "nt", [nt(17, 4128, 21, ldx=24, ldw=24, ldy=4132, ldz=4136, Z=True, act=1, drop=P)], "epilogue, K=21: wave 3 empty"),
    Case("nt1_m33_n4128_k44", "nt", [nt(33, 4128, 44, bias=False, drop=P)], "epilogue, K=44: waves 8 8 8 8 + tails"),
    Case("nt1w2_m17_n4128_k9", "nt", [nt(17, 4128, 9, ldx=12, ldw=10, ldy=4136, drop=P)], "epilogue, ldw=10, K=9: waves 2 3 empty"),
    Case("nt2_m65_n5504_k13", "nt", [nt(65, 5504, 13, ldx=16, ldw=16, Z=True, act=1, drop=P, ldy=5508)], "epilogue, two row tiles, K=13"),
    Case("nt2w2_m65_n5504_k38", "nt", [nt(65, 5504, 38, ldx=40, ldw=38, ldy=5512, drop=P, act=1, Z=True)], "epilogue, ldw=38, K=38"),
    # ------------------------------------------------------------------ nn, 16x16 tiles
    Case("nn16_m17_k18", "nn", [nn(17, 32, 18, ldo=20, actZ=True, drop=P, drop_ld=18, ldz=22)], "K=18: strip of 16 ends at 2"),
    Case("nn16_m33_k100", "nn", [nn(33, 96, 100, add=True, ldadd=104, lddy=100)], "K=100, N=96: waves of 32 32 32 0"),
    Case("nn16_group2", "nn", [nn(17, 64, 34, actZ=True, add=True, drop=P, drop_ld=34, ldo=40), nn(33, 32, 16)], "two problems"),
    Case("nn16_group16", "nn", [nn(1 + 2 * i, 32 * (1 + i % 2), 2 * (3 + i), actZ=bool(i % 2), add=(i % 3 == 0), drop=P if i % 2 else 0.0,
                                   drop_ld=2 * (3 + i) + (i % 4), ldo=2 * (3 + i) + 2 * (i % 3)) for i in range(16)], "sixteen unequal problems"),
    # ------------------------------------------------------------------ nn, strips of 32 VEC columns: split N (bare partials) ...
    Case("nn4_m33_k132_s64", "nn", [nn(33, 96, 132, 64, ldo=136)], "nsplit 64 of 32: splits 3.. empty; K=132 ends 4 into a strip; ldo > K"),
    Case("nn2_m33_k130_s64", "nn", [nn(33, 96, 130, 64)], "K=130: K % 4 == 2, ends 2 into a strip of 64"),
    Case("nn1_m33_k132_s2", "nn", [nn(33, 96, 132, 2, ldo=140)], "nsplit 2 of 64: split 1 feeds waves 0 1 only; ldo > K"),
    Case("nn1_m17_k36_s4", "nn", [nn(17, 64, 36, 4, a8=True, ldw=38)], "nsplit 4: splits 2 3 empty; K=36 ends 4 into a strip of 32"),
    # ... and the in-kernel epilogue (K > 4096 unsplit)
    Case("nn4_group_k4100", "nn", [nn(33, 32, 4100, actZ=True, drop=P, drop_ld=4100, ldo=4104),
                                   nn(33, 64, 4100, actZ=True, add=True, drop=P, drop_ld=4102, ldo=4100),
                                   nn(17, 32, 4100, add=True, ldadd=4104),
                                   nn(1, 32, 4100, actZ=True), nn(33, 32, 4100)], "K=4100 ends 4 into a strip of 128; drop_ld % 4 = 0 and 2"),
    Case("nn4_group_k4228", "nn", [nn(65, 32, 4228, actZ=True, drop=P, drop_ld=4231, ldz=4232), nn(65, 64, 4228, add=True),
                                   nn(33, 32, 4228, actZ=True, add=True)], "K=4228 = 33 strips + 4; drop_ld odd"),
    Case("nn2_group_k4098", "nn", [nn(33, 32, 4098, actZ=True, drop=P, drop_ld=4099, ldo=4100), nn(33, 64, 4098, add=True),
                                   nn(1, 32, 4098, actZ=True, add=True, drop=P)], "K=4098: K % 4 == 2, ends 2 into a strip of 64"),
    Case("nn2_group_w8", "nn", [nn(65, 32, 4100, a8=True, ldw=4102, actZ=True, drop=P, ldo=4104), nn(65, 32, 4104, add=True)],
         "W 8-B aligned; K=4100 ends 4 into a strip of 64"),
    Case("nn1_m33_k4100", "nn", [nn(33, 32, 4100, actZ=True, add=True, drop=P, drop_ld=4100, ldo=4102)], "K=4100 ends 4 into a strip of 32"),
    Case("nn1_m17_k4106", "nn", [nn(17, 64, 4106, actZ=True, drop=P, drop_ld=4107)], "K=4106 ends 10 into a strip of 32; two waves' N"),
    # ------------------------------------------------------------------ tn, one wave per tile (fewer than 128 rows)
    Case("tn4_m1_k8", "tn", [tn(1, 32, 8)], "M=1, one strip ending at 8"),
    Case("tn4_m7_k132", "tn", [tn(7, 64, 132, ldx=136, ldw=140, lddy=68)], "M=7, K=132 ends 4 into the second strip"),
    Case("tn4_m33_k128", "tn", [tn(33, 32, 128, db=False)], "M=33: second pass of one row; no db"),
    Case("tn2_m33_k34", "tn", [tn(33, 32, 34, ldx=34, ldw=36)], "K=34: K % 4 == 2, one strip of 64"),
    Case("tn2_m7_k70", "tn", [tn(7, 64, 70, a8=True, ldx=72, ldw=72, db=False)], "X and dW 8-B aligned, K=70 ends 6 into the second strip"),
    Case("tnmix_below128", "tn", [tn(33, 32, 132), tn(7, 64, 34, ldw=36), tn(127, 32, 8, a8=True)], "16-B, 8-B and 8-B-aligned problems, M < 128"),
    Case("tnmix_group16", "tn", [tn(1 + 7 * i, 32 * (1 + i % 2), 2 * (2 + 3 * i), db=bool(i % 3)) for i in range(16)], "sixteen unequal problems"),
    # ------------------------------------------------------------------ tn, batch rows split over four waves (128 rows and more)
    Case("tn4ms_m128_k8", "tn", [tn(128, 32, 8)], "M=128: quarters of 32"),
    Case("tn4ms_m129_k132", "tn", [tn(129, 64, 132, ldx=136, lddy=72)], "M=129: quarters of 40 40 40 9"),
    Case("tn4ms_m135_k256", "tn", [tn(135, 32, 256, db=False)], "M=135: last quarter 15; no db"),
    Case("tn2ms_m129_k34", "tn", [tn(129, 32, 34)], "K=34, M=129"),
    Case("tn2ms_mixed_above128", "tn", [tn(135, 32, 132), tn(128, 64, 38, ldw=40, db=False), tn(129, 32, 8, a8=True)], "16-B and 8-B problems, M >= 128"),
    # ------------------------------------------------------------------ tn, rows in segments
    Case("tn4seg_m33", "tn", [tn(33, 32, 132, seg_rows=3, seg_dy=3 * 32 + 16, seg_x=3 * 132 + 8)], "11 segments of 3 rows"),
    Case("tn2seg_m14", "tn", [tn(14, 64, 34, seg_rows=7, seg_dy=7 * 64 + 8, seg_x=7 * 34 + 6)], "2 segments of 7 rows, seg_x % 4 == 2"),
    Case("tnmixseg_m33", "tn", [tn(33, 32, 8, seg_rows=11, seg_dy=11 * 32 + 4, seg_x=11 * 8 + 4),
                                tn(21, 32, 38, seg_rows=7, seg_dy=7 * 32 + 4, seg_x=7 * 38 + 2, db=False)], "16-B and 8-B segmented problems"),
    Case("tn4msseg_m129", "tn", [tn(129, 32, 132, seg_rows=43, seg_dy=43 * 32 + 12, seg_x=43 * 132 + 4)], "3 segments of 43 rows, M=129"),
    Case("tn2msseg_m135", "tn", [tn(135, 32, 34, seg_rows=5, seg_dy=5 * 32 + 4, seg_x=5 * 34 + 2)], "27 segments of 5 rows, M=135"),
]

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def contraction(kind: str, p: Dict) -> int:
    return {"nt": p["K"], "nn": p["N"], "tn": p["M"]}[kind]


def exact_ok(kind: str, p: Dict) -> bool:
    """Operands that are multiples of 1/4 in [-2, 2]: products are multiples of 1/16 up to 4, so every partial sum of L of them
    plus a bias is a multiple of 1/16 below 4 L + 2 -- exact in fp32 while 16 (4 L + 2) < 2^24, whatever the order."""
    return 16 * (4 * contraction(kind, p) + 2) < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------
# ctypes problems.  `addr(name, index, floats)` returns the address of an operand; the CPU test passes made-up aligned
# addresses, the GPU test device buffers.  a8 operands sit 8 bytes past a 16-byte boundary in both.
def fake_addr(name: str, i: int, a8: bool) -> int:
    return 0x100000 * (1 + i) + 0x1000 * (1 + sum(map(ord, name)) % 50) + (8 if a8 else 0)


def make_probs(D, case: Case, addr=None, variant: Dict = None):
    """ctypes structures of a case (D = tools._diaglib).  addr(name, i) -> int address; variant overrides fields of every problem."""
    out = []
    for i, q in enumerate(case.probs):
        p = dict(q)
        if variant:
            p.update(variant)
        a8 = p["a8"]

        def A(name, is8=False, i=i):
            return addr(name, i) if addr else fake_addr(name, i, is8)
        if case.kind == "nt":
            s = D.NtProb(X=A("X"), W=A("W", a8), bias=A("bias") if p["bias"] else None, Y=A("Y"), Z=A("Z") if p["Z"] else None,
                         M=p["M"], N=p["N"], K=p["K"], ldx=p["ldx"], ldw=p["ldw"], ldy=p["ldy"], ldz=p["ldz"] if p["Z"] else 0, act=p["act"],
                         drop_p=p["drop"], drop_layer=DROP_LAYER + i, ksplit=p["ksplit"])
        elif case.kind == "nn":
            s = D.NnProb(dY=A("dY"), W=A("W", a8), out=A("out"), actZ=A("actZ") if p["actZ"] else None, add=A("add") if p["add"] else None,
                         M=p["M"], N=p["N"], K=p["K"], lddy=p["lddy"], ldw=p["ldw"], ldo=p["ldo"], ldz=p["ldz"], ldadd=p["ldadd"],
                         drop_p=p["drop"], drop_layer=DROP_LAYER + i, drop_ld=p["drop_ld"], nsplit=p["nsplit"])
        else:
            s = D.TnProb(dY=A("dY"), X=A("X", a8), dW=A("dW", a8), db=A("db") if p["db"] else None, M=p["M"], N=p["N"], K=p["K"],
                         lddy=p["lddy"], ldx=p["ldx"], ldw=p["ldw"], seg_rows=p["seg_rows"], seg_dy=p["seg_dy"], seg_x=p["seg_x"])
        out.append(s)
    return out


def plan(D, case: Case):
    rc, form, grid, err = D.gemm_f32_plan(case.kind, make_probs(D, case))
    assert rc == 0, (case.id, err)
    return form, grid


# forms that read rows by segment (each needs one case); every other form needs two cases with different tails
SEG_FORMS = ("tn<4,0,1>", "tn<2,0,1>", "tn<-1,0,1>", "tn<4,1,1>", "tn<2,1,1>")
