"""CPU: the audio encoder's entries refuse bad calls by name without touching a GPU (beside tests/test_abi.py)."""
import pytest
import torch


def _lib():
    from ultrafnd_git_amd import _lib as L
    return L.lib()


P = 1 << 12      # an aligned, never dereferenced address: every refusal below happens before any launch


def test_conv1d_rows_argument_checks():
    lib = _lib()
    ok = dict(M=4, N=64, K=128, lda=64, ldw=128, ldo=64, ldf=0, act=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ufnd_conv1d_rows_bf16(P, P, None, P, None, a["M"], a["N"], a["K"], a["lda"], a["ldw"], a["ldo"], a["ldf"], a["act"], None)

    assert call(lda=12) == 1 and b"lda=12" in lib.ufnd_last_error()                   # lda % 8 != 0
    assert call(lda=0) == 1 and b"lda=0" in lib.ufnd_last_error()
    assert call(K=100) == 1 and b"K=100" in lib.ufnd_last_error()                     # K % 64 != 0
    assert call(N=96) == 1 and b"N=96" in lib.ufnd_last_error()                       # N % 64 != 0
    assert call(ldw=64) == 1 and b"ldw=64" in lib.ufnd_last_error()                   # the weight rows stay whole
    assert call(act=7) == 1 and b"act=7" in lib.ufnd_last_error()
    assert call(M=1 << 22, lda=1024) == 1 and b"2^31" in lib.ufnd_last_error()
    assert lib.ufnd_conv1d_rows_bf16(None, P, None, P, None, 4, 64, 128, 64, 128, 64, 0, 1, None) == 1 and b"null" in lib.ufnd_last_error()
    assert lib.ufnd_conv1d_rows_bf16(P + 2, P, None, P, None, 4, 64, 128, 64, 128, 64, 0, 1, None) == 1


def test_public_gemm_entries_still_require_whole_rows():
    lib = _lib()
    # lda < K is what ufnd_conv1d_rows_bf16 is for: ufnd_gemm_bf16 keeps refusing it
    assert lib.ufnd_gemm_bf16(P, P, None, None, P, None, 4, 64, 128, 64, 128, 0, 64, 0, 0, None) == 1
    assert b"strides" in lib.ufnd_last_error()


def test_audio_kernel_entries_refuse_short_clips_and_bad_slabs():
    lib = _lib()
    assert lib.ufnd_wave_normalize(P, P, P, P, 1, 399, None) == 1 and b"at least 400" in lib.ufnd_last_error()
    assert lib.ufnd_wave_normalize(P, None, P, P, 1, 400, None) == 1 and b"null" in lib.ufnd_last_error()
    assert lib.ufnd_w2v2_conv0(P, P, P, P, P, P, None, P, 1, 399, 64, 1e-5, None) == 1 and b"at least 400" in lib.ufnd_last_error()
    assert lib.ufnd_w2v2_conv0(P, P, P, P, P, P, None, P, 1, 16000, 3136, 1e-5, None) == 1 and b"S1=3136" in lib.ufnd_last_error()      # < 3,199 frames
    assert lib.ufnd_w2v2_conv0(P, P, P, P, P, P, None, P, 1, 16000, 3210, 1e-5, None) == 1 and b"S1=3210" in lib.ufnd_last_error()      # not a multiple of 64
    assert lib.ufnd_w2v2_pos_pack(P, P, P, 0, 4, None) == 1 and lib.ufnd_w2v2_pos_add(P, P, P, P, 1, 0, None) == 1
    assert lib.ufnd_masked_meanpool(P, P, P, 1, 4, 100, None) == 1 and b"H=100" in lib.ufnd_last_error()
    assert lib.ufnd_linear_f32(P, P, None, P, 1, 100, 768, None) == 1


def test_encoder_refuses_short_clips_and_foreign_geometries_by_name():
    from ultrafnd_git_amd.audio import MIN_SAMPLES, Wav2Vec2AudioEncoder
    assert MIN_SAMPLES == 400
    enc = Wav2Vec2AudioEncoder(layers=1)
    with pytest.raises(ValueError, match="at least 400 samples"):
        enc(torch.zeros(1, 399))
    with pytest.raises(ValueError, match="clip length 399"):
        enc(torch.zeros(2, 1000), [1000, 399])
    with pytest.raises(ValueError, match="n_max=1000"):
        enc(torch.zeros(1, 1000), [1001])
    with pytest.raises(ValueError, match="2 entries for 1 clips"):
        enc(torch.zeros(1, 1000), [1000, 1000])
    for kw, name in ((dict(hidden=1024, heads=16), "hidden=1024"), (dict(conv_kernel=(10, 3, 3, 3, 3, 3, 2)), "conv_kernel"),
                     (dict(feat_extract_norm="layer"), "feat_extract_norm='layer'"), (dict(do_stable_layer_norm=True), "do_stable_layer_norm=True"),
                     (dict(num_conv_pos_embedding_groups=8), "num_conv_pos_embedding_groups=8"), (dict(conv_bias=True), "conv_bias=True"),
                     (dict(hidden_act="relu"), "hidden_act='relu'")):
        with pytest.raises(ValueError, match=name):
            Wav2Vec2AudioEncoder(layers=1, **kw)
    # a valid call on the CPU is refused too: there is no CPU path
    from ultrafnd_git_amd._lib import UltrafndHipError
    with pytest.raises(UltrafndHipError, match="HIP device only"):
        enc(torch.zeros(1, 400))


def test_spectral_forensics_refuses_text_and_other_rates_by_name():
    from ultrafnd_git_amd.audio import SpectralForensics, Wav2Vec2AudioEncoder
    sf = SpectralForensics(dim=128, encoder=Wav2Vec2AudioEncoder(layers=1))
    with pytest.raises(TypeError, match="hash"):
        sf.extract("a title")
    with pytest.raises(ValueError, match="sr=8000"):
        sf.extract(torch.zeros(1000), sr=8000)
    with pytest.raises(ValueError, match="dim=64"):
        SpectralForensics(dim=64, encoder=Wav2Vec2AudioEncoder(layers=1))
