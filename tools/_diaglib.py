"""Loader of libultrafnd_hip_diag.so (csrc/diag/, built with -DUFND_DIAG): timing ablations, in-kernel stamps, every
experimental GEMM tile, the placement probe.  Tools only -- the product package never loads it."""
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: F401,E402  (its HIP runtime must be resident first)

from ultrafnd_git_amd import _lib as L  # noqa: E402
from ultrafnd_git_amd.build import DIAG_LIB, build_diag  # noqa: E402

_d = None

_FP = C.c_void_p


class NtProb(C.Structure):      # csrc/gemm_f32.hpp
    _fields_ = [("X", _FP), ("W", _FP), ("bias", _FP), ("Y", _FP), ("Z", _FP)] + \
               [(n, C.c_int) for n in ("M", "N", "K", "ldx", "ldw", "ldy", "ldz", "act")] + \
               [("drop_p", C.c_float), ("drop_layer", C.c_uint32), ("ksplit", C.c_int)]


class NnProb(C.Structure):
    _fields_ = [("dY", _FP), ("W", _FP), ("out", _FP), ("actZ", _FP), ("add", _FP)] + \
               [(n, C.c_int) for n in ("M", "N", "K", "lddy", "ldw", "ldo", "ldz", "ldadd")] + \
               [("drop_p", C.c_float), ("drop_layer", C.c_uint32), ("drop_ld", C.c_int), ("nsplit", C.c_int)]


class TnProb(C.Structure):
    _fields_ = [("dY", _FP), ("X", _FP), ("dW", _FP), ("db", _FP)] + \
               [(n, C.c_int) for n in ("M", "N", "K", "lddy", "ldx", "ldw", "seg_rows", "seg_dy", "seg_x")]


# enum GemmF32Form (csrc/gemm_f32.hpp), in its order
GEMM_F32_FORMS = ("nt16<4>", "nt16<2>", "nt<1,4>", "nt<1,2>", "nt<2,4>", "nt<2,2>", "nn16", "nn<4>", "nn<2>", "nn<1>",
                  "tn<4,0,0>", "tn<2,0,0>", "tn<-1,0,0>", "tn<4,1,0>", "tn<2,1,0>",
                  "tn<4,0,1>", "tn<2,0,1>", "tn<-1,0,1>", "tn<4,1,1>", "tn<2,1,1>")
GEMM_F32_KINDS = {"nt": (0, NtProb), "nn": (1, NnProb), "tn": (2, TnProb)}


def diag() -> C.CDLL:
    global _d
    if _d is None:
        if not DIAG_LIB.exists():
            build_diag()
        d = C.CDLL(str(DIAG_LIB))
        P, I = C.c_void_p, C.c_int
        d.ufnd_diag_last_error.restype = C.c_char_p
        d.ufnd_diag_gemm_bf16_ex.argtypes = [P] * 6 + [I] * 10 + [P]
        d.ufnd_diag_gemm_bf16_ex.restype = I
        d.ufnd_diag_gemm_bf16_stamps.argtypes = [P, P, P, I, I, I, I, P, C.POINTER(L.GemmLn), P, P, P, P]
        d.ufnd_diag_gemm_bf16_stamps.restype = I
        d.ufnd_diag_qkv_attention_stamps.argtypes = [P, P, P, P, P, I, I, C.POINTER(L.GemmLn), P, P]
        d.ufnd_diag_qkv_attention_stamps.restype = I
        d.ufnd_diag_qkv_attention_tiles_stamps.argtypes = [P, P, P, P, P, P, I, I, C.POINTER(L.GemmLn), P, P]
        d.ufnd_diag_qkv_attention_tiles_stamps.restype = I
        d.ufnd_diag_gemm_pp_stamps.argtypes = [P, P, P, I, I, I, P, C.POINTER(L.GemmLn), P, I, I, P]
        d.ufnd_diag_gemm_pp_stamps.restype = I
        d.ufnd_diag_where.argtypes = [P, I, C.c_uint64, P]
        d.ufnd_diag_where.restype = I
        IP = C.POINTER(I)
        d.ufnd_diag_gemm_f32_nt.argtypes = [C.POINTER(NtProb), I, P, IP, IP, P]
        d.ufnd_diag_gemm_f32_nn.argtypes = [C.POINTER(NnProb), I, P, IP, IP, P]
        d.ufnd_diag_gemm_f32_tn.argtypes = [C.POINTER(TnProb), I, IP, IP, P]
        d.ufnd_diag_gemm_f32_plan.argtypes = [I, P, I, IP, IP]
        for f in (d.ufnd_diag_gemm_f32_nt, d.ufnd_diag_gemm_f32_nn, d.ufnd_diag_gemm_f32_tn, d.ufnd_diag_gemm_f32_plan):
            f.restype = I
        d.ufnd_diag_gemm_bf16_plan.argtypes = [I] + [P] * 7 + [I] * 11 + [C.POINTER(L.GemmLn), IP]
        d.ufnd_diag_gemm_bf16_plan.restype = I
        d.ufnd_diag_gemm_pp_plan.argtypes = [P] * 6 + [I] * 9 + [C.POINTER(L.GemmLn), I, I, IP]
        d.ufnd_diag_gemm_pp_plan.restype = I
        d.ufnd_diag_gemm_f32_sizes.argtypes = [IP]
        d.ufnd_diag_gemm_f32_sizes.restype = None
        _d = d
    return _d


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {diag().ufnd_diag_last_error().decode()}")


def gemm_f32_plan(kind: str, probs) -> tuple:
    """Host-only validation + choice of a launch of the fp32 GEMM family: (rc, form name or None, grid, error text).  `probs` is
    a list of NtProb / NnProb / TnProb; their pointers are never dereferenced (no GPU needed)."""
    k, T = GEMM_F32_KINDS[kind]
    arr = (T * max(1, len(probs)))(*probs)
    form, grid = C.c_int(-1), C.c_int(0)
    rc = diag().ufnd_diag_gemm_f32_plan(k, C.cast(arr, C.c_void_p), len(probs), C.byref(form), C.byref(grid))
    if rc != 0:
        return rc, None, 0, diag().ufnd_diag_last_error().decode()
    return 0, GEMM_F32_FORMS[form.value], grid.value, ""


def gemm_f32_launch(kind: str, probs, state_ptr, stream) -> tuple:
    """Launch nt / nn / tn on `stream` (state_ptr: device ufnd_step_state or None; ignored by tn).  Returns (form name, grid)."""
    k, T = GEMM_F32_KINDS[kind]
    arr = (T * len(probs))(*probs)
    form, grid = C.c_int(-1), C.c_int(0)
    d = diag()
    if kind == "nt":
        rc = d.ufnd_diag_gemm_f32_nt(arr, len(probs), state_ptr, C.byref(form), C.byref(grid), stream)
    elif kind == "nn":
        rc = d.ufnd_diag_gemm_f32_nn(arr, len(probs), state_ptr, C.byref(form), C.byref(grid), stream)
    else:
        rc = d.ufnd_diag_gemm_f32_tn(arr, len(probs), C.byref(form), C.byref(grid), stream)
    check(rc, f"ufnd_diag_gemm_f32_{kind}")
    return GEMM_F32_FORMS[form.value], grid.value


GEMM_BF16_ENTRIES = {"tile": -1, "gemm": 0, "ex": 1, "ln": 2, "dgrad": 3}
GEMM_BF16_PLAN_FIELDS = ("tile", "m_tiles", "n_tiles", "xcd_cols", "stat_parts", "bm", "bn", "sta", "stb", "ln_aware", "prod", "bwd")


def gemm_bf16_plan(entry: str, *, A=0, W=0, bias=None, residual=None, aux=None, out_bf16=None, out_f32=None, M=0, N=0, K=0, lda=0,
                   ldw=0, ldr=0, ldaux=0, ldo=0, ldf=0, act=0, tile=-1, ln=None) -> tuple:
    """Host-only validation + tile choice + grid of one call of ufnd_gemm_bf16 ("gemm"), ufnd_gemm_bf16_ex ("ex"), ufnd_gemm_bf16_ln
    ("ln", ln: L.GemmLn) or ufnd_gemm_bf16_dgrad ("dgrad"); "tile": the table row of `tile`.  Addresses are integers that are never
    dereferenced (no GPU needed).  Returns (rc, dict of GEMM_BF16_PLAN_FIELDS or None, error text)."""
    out = (C.c_int * len(GEMM_BF16_PLAN_FIELDS))()
    rc = diag().ufnd_diag_gemm_bf16_plan(GEMM_BF16_ENTRIES[entry], A, W, bias, residual, aux, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldaux,
                                         ldo, ldf, act, tile, C.byref(ln) if ln is not None else None, out)
    if rc != 0:
        return rc, None, diag().ufnd_diag_last_error().decode()
    return 0, dict(zip(GEMM_BF16_PLAN_FIELDS, out)), ""


GEMM_PP_PLAN_FIELDS = ("mode", "act", "m_tiles", "n_tiles", "pp_rows", "G", "picked", "stat_parts")
GEMM_PP_MODES = ("plain", "fold", "rln", "res")      # pp::PLAIN, FOLD, RES_LN, RES (csrc/gemm_bf16_pp.hpp)


def gemm_pp_plan(*, A=0, W=0, bias=None, residual=None, out_bf16=None, out_f32=None, M=0, N=0, K=0, lda=0, ldw=0, ldr=0, ldo=0, ldf=0,
                 act=0, ln=None, tile=64, cus=256) -> tuple:
    """Host-only validation, mode, walk geometry and automatic choice of one call of the persistent bf16 GEMM (csrc/gemm_bf16_pp.hpp)
    for a device of `cus` compute units: the arguments of ufnd_gemm_bf16_ln (ln: L.GemmLn, whose tile_cfg is not read) or, with
    ln = None, of ufnd_gemm_bf16_ex; tile = 64 is a forced call, tile < 0 the automatic choice.  Addresses are integers that are never
    dereferenced (no GPU needed).  Returns (rc, dict of GEMM_PP_PLAN_FIELDS or None, error text)."""
    out = (C.c_int * len(GEMM_PP_PLAN_FIELDS))()
    rc = diag().ufnd_diag_gemm_pp_plan(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act,
                                       C.byref(ln) if ln is not None else None, tile, cus, out)
    if rc != 0:
        return rc, None, diag().ufnd_diag_last_error().decode()
    return 0, dict(zip(GEMM_PP_PLAN_FIELDS, out)), ""
