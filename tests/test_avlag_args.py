"""CPU: the A/V lag entries (csrc/av_lag.hip) and their Python layer (ultrafnd_git_amd/temporal.py, video.py) refuse bad calls by name
without touching a GPU; the workspace query returns 0 at the stated limits; both classes' host estimate_av_lag still return the
reference's seconds (tests/golden/avlag.npz)."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import avlag_ref as R

P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch
REPO = Path(__file__).resolve().parents[1]


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


def test_exported_constants_mirror_the_header_and_the_checker():
    from ultrafnd_git_amd import _lib as L
    text = (REPO / "include" / "ultrafnd_hip.h").read_text()
    assert int(re.search(r"#define UFND_AVLAG_SEGMENT (\d+)", text).group(1)) == L.AVLAG_SEGMENT == R.SEG == 2048
    assert int(re.search(r"#define UFND_AVLAG_LAG_BLOCK (\d+)", text).group(1)) == L.AVLAG_LAG_BLOCK == R.LAG_BLOCK == 1024
    assert int(re.search(r"#define UFND_AVLAG_MAX_B (\d+)", text).group(1)) == L.AVLAG_MAX_B == 65535
    assert re.search(r"#define UFND_AVLAG_MAX_N \(1 << 26\)", text) and L.AVLAG_MAX_N == 1 << 26
    assert re.search(r"#define UFND_AVLAG_MAX_LAG \(1 << 26\)", text) and L.AVLAG_MAX_LAG == 1 << 26
    assert int(re.search(r"#define UFND_AVLAG_MAX_PARTIAL_FLOATS (\d+)LL", text).group(1)) == L.AVLAG_MAX_PARTIAL_FLOATS == 1 << 31
    assert "size_t ufnd_av_lag_workspace_bytes(int B, int n_max, int max_lag);" in text and "int ufnd_av_lag(const float* a, int64_t a_row_stride" in text


def test_workspace_query_its_64_bit_size_and_the_refusal_limits():
    from ultrafnd_git_amd import _lib as L
    lib = _lib()
    r16 = lambda n: -(-n // 16) * 16
    for B, n, K in ((1, 1, 0), (1, 4, 8000), (32, 125, 12), (32, 4000, 2000), (32, 80000, 8000), (7, 2049, 511), (3, 1 << 26, 10), (65535, 16, 3)):
        nwp, S = -(-n // 8) * 8, -(-n // 2048)
        assert lib.ufnd_av_lag_workspace_bytes(B, n, K) == 2 * r16(B * nwp * 4) + r16(B * S * (2 * K + 1) * 4), (B, n, K)
    assert lib.ufnd_av_lag_workspace_bytes(16, 1 << 26, 2000) > 1 << 32       # a size_t, past 2^32
    # by name: B, n_max, max_lag < 0, max_lag above its limit
    for B, n, K in ((0, 100, 5), (-1, 100, 5), (L.AVLAG_MAX_B + 1, 100, 5), (1, 0, 5), (1, -3, 5), (1, L.AVLAG_MAX_N + 1, 5), (1, 100, -1),
                    (1, 100, L.AVLAG_MAX_LAG + 1)):
        assert lib.ufnd_av_lag_workspace_bytes(B, n, K) == 0, (B, n, K)
    assert lib.ufnd_av_lag_workspace_bytes(L.AVLAG_MAX_B, 100, 5) > 0 and lib.ufnd_av_lag_workspace_bytes(1, L.AVLAG_MAX_N, 5) > 0
    assert lib.ufnd_av_lag_workspace_bytes(1, 100, L.AVLAG_MAX_LAG) > 0
    # the product the partial buffer needs: B ceil(n_max / 2048) (2 max_lag + 1) <= 2^31 floats, met exactly and passed by one row
    B, n, K = 1 << 10, 2048 * 1024, 1023      # 2^10 * 2^10 * 2047 < 2^31
    assert lib.ufnd_av_lag_workspace_bytes(B, n, K) > 0
    assert lib.ufnd_av_lag_workspace_bytes(B, n, K + 1) == 0      # 2^20 * 2049 > 2^31
    assert lib.ufnd_av_lag_workspace_bytes(32, 80000, 8000) > 0 and lib.ufnd_av_lag_workspace_bytes(32, 8000000, 800000) == 0


def test_entry_refusals():
    from ultrafnd_git_amd import _lib as L
    lib = _lib()
    err = lib.ufnd_last_error

    def call(a=P, m=P, ws=P, outs=(P, None, None, None, None), sa=100, sm=100, B=2, na=100, nm=100, K=10):
        return lib.ufnd_av_lag(a, sa, m, sm, None, None, ws, outs[0], outs[1], outs[2], outs[3], outs[4], B, na, nm, K, None)

    for key in ("a", "m", "ws"):
        assert call(**{key: None}) == 1 and b"null" in err(), key
    assert call(outs=(None,) * 5) == 1 and b"no output" in err()
    assert call(B=0) == 1 and b"B=0" in err()
    assert call(B=65536) == 1 and b"B=65536" in err()
    assert call(na=0) == 1 and b"na_max=0" in err()
    assert call(nm=(1 << 26) + 1) == 1 and b"nm_max=67108865" in err()
    assert call(K=-1) == 1 and b"max_lag=-1" in err()
    assert call(K=(1 << 26) + 1) == 1 and b"max_lag=67108865" in err()
    assert call(B=1 << 10, na=2048 * 1024, nm=2048 * 1024 + 5, K=1024) == 1 and b"partials=2148532224" in err()
    assert call(sa=-1) == 1 and b"stride" in err()
    assert call(sm=-100) == 1 and b"stride" in err()
    assert call(ws=P + 8) == 1 and b"alignment" in err()
    assert call(a=P + 2) == 1 and b"alignment" in err()
    assert call(m=P + 1) == 1 and b"alignment" in err()


def test_python_refusals_by_name():
    from ultrafnd_git_amd import temporal
    from ultrafnd_git_amd._lib import UltrafndHipError
    from ultrafnd_git_amd.video import ChronosGuard
    a, m = torch.zeros(2, 100), torch.zeros(2, 100)
    for fn in (temporal.av_lag, temporal.TemporalSyncNet.estimate_av_lag_batch, ChronosGuard.estimate_av_lag_batch):
        with pytest.raises(UltrafndHipError, match="HIP device only"):      # a valid call on the CPU: there is no CPU path
            fn(a, m)
        with pytest.raises(UltrafndHipError, match="HIP device only"):
            fn(np.zeros((2, 100), np.float32), m)
        with pytest.raises(ValueError, match="sr=0.0"):
            fn(a, m, sr=0.0)
        with pytest.raises(ValueError, match="sr=-16000.0"):
            fn(a, m, sr=-16000.0)
        with pytest.raises(ValueError, match="max_lag_s=-0.5"):
            fn(a, m, max_lag_s=-0.5)
        with pytest.raises(ValueError, match="sr=nan"):
            fn(a, m, sr=float("nan"))
        with pytest.raises(ValueError, match="max_lag_s=inf"):
            fn(a, m, max_lag_s=float("inf"))
        with pytest.raises(ValueError, match="want='lag'"):
            fn(a, m, want=("lag",))
        with pytest.raises(ValueError, match="want is empty"):
            fn(a, m, want=())
    sig = inspect.signature(temporal.av_lag).parameters
    assert list(sig) == ["audio_env", "mouth_open", "len_a", "len_m", "sr", "fps", "max_lag_s", "want"]
    assert [sig[k].default for k in ("len_a", "len_m", "sr", "fps", "max_lag_s", "want")] == [None, None, 16000.0, 25.0, 0.5, ("lag_seconds",)]
    for cls in (temporal.TemporalSyncNet, ChronosGuard):
        assert isinstance(inspect.getattr_static(cls, "estimate_av_lag_batch"), staticmethod)
        assert list(inspect.signature(cls.estimate_av_lag_batch).parameters) == list(sig)


def test_both_host_estimate_av_lag_still_return_the_reference_s_seconds():
    """The host forms are untouched: NumPy in, a Python float out, no GPU -- and equal to the fixture minted from the reference."""
    from ultrafnd_git_amd.temporal import TemporalSyncNet
    from ultrafnd_git_amd.video import ChronosGuard
    cases = R.load_fixture(REPO / "tests" / "golden" / "avlag.npz")
    assert len(cases) >= 20
    for name, c in cases.items():
        for cls in (TemporalSyncNet, ChronosGuard):
            got = cls.estimate_av_lag(c["a"], c["m"], sr=c["sr"], fps=c["fps"], max_lag_s=c["max_lag_s"])
            assert isinstance(got, float) and got == c["seconds"], (name, cls.__name__, got, c["seconds"])
    got = TemporalSyncNet.estimate_av_lag(torch.from_numpy(cases["n257"]["a"]), cases["n257"]["m"])
    assert got == cases["n257"]["seconds"]
