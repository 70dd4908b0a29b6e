"""The parts of the mel-spectrogram front end that need no GPU: the Slaney basis, the frame-count formula, the
fake kernel, the inference.py flag surface, the float64 test reference against the golden, and the no-device
error path."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import melspec_ref as R  # tests/melspec_ref.py
from m2s import _native as N
from m2s import melspec, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "melspec.npz")


# ---- Slaney basis ------------------------------------------------------------------------------------------
def test_mel_scale_closed_forms():
    for k in range(0, 16):
        assert abs(float(melspec.hz_to_mel(200.0 * k / 3.0)) - k) < 1e-12  # 200/3 Hz per mel below 1 kHz
    assert float(melspec.hz_to_mel(1000.0)) == 15.0
    assert abs(float(melspec.hz_to_mel(6400.0)) - 42.0) < 1e-12  # 27 mels per factor of 6.4 above
    f = np.array([0.0, 50.0, 999.0, 1000.0, 1001.0, 4000.0, 8000.0])
    np.testing.assert_allclose(melspec.mel_to_hz(melspec.hz_to_mel(f)), f, rtol=1e-12, atol=1e-9)


def test_slaney_basis_config_a():
    c = R.CONFIGS["A"]
    b = R.basis(c)
    assert b.shape == (64, 1025) and b.dtype == np.float32 and (b >= 0).all()
    nonempty = np.flatnonzero(b.sum(1) > 0)
    assert list(nonempty) == list(range(58))  # fmax 8000 > sr / 2: the top six filters lie above Nyquist
    peaks = b[:58].argmax(1)
    assert (np.diff(peaks) > 0).all()
    # unit area over Hz for every filter wide enough to be sampled well (>= 8 bins) and wholly below Nyquist
    df = (c["sr"] / 2.0) / 1024
    edges = melspec.mel_to_hz(np.linspace(0.0, float(melspec.hz_to_mel(8000.0)), 66))
    wide = [i for i in range(58) if (b[i] > 0).sum() >= 8 and edges[i + 2] <= c["sr"] / 2.0]
    assert len(wide) >= 20
    for i in wide:
        assert abs(b[i].astype(np.float64).sum() * df - 1.0) < 0.02, i


def test_slaney_basis_defaults():
    b = melspec.slaney_mel_basis(8000, 64, 8)  # fmax None: sr / 2
    assert b.shape == (8, 33) and (b.sum(1) > 0).all()
    assert np.array_equal(b, melspec.slaney_mel_basis(8000, 64, 8, 0.0, 4000.0))
    assert (np.diff(b.argmax(1)) > 0).all()


# ---- frame count -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,win", [(64, 16, 48), (256, 101, 200), (2048, 420, 2048), (64, 30, 64)])
def test_frame_count_matches_torch_stft(n_fft, hop, win):
    p = (n_fft - hop) // 2
    for pad in (0, 1):
        for L in sorted({1, p, p + 1, n_fft - 2 * p - 1, n_fft - 2 * p, n_fft - 1, n_fft, n_fft + 1, n_fft + hop - 1,
                         n_fft + hop, 3 * n_fft + 7}):
            if L < 1:
                continue
            T = R.n_frames(L, n_fft, hop, pad)
            y = torch.zeros(1, L)
            try:
                if pad:
                    y = torch.nn.functional.pad(y[:, None], (p, p), mode="reflect")[:, 0]
                want = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win),
                                  center=False, return_complex=True).shape[-1]
            except RuntimeError:
                want = 0  # torch refuses what the engine refuses: a reflect pad >= L, fewer than n_fft samples
            assert T == want, (pad, L)


# ---- fake kernel -------------------------------------------------------------------------------------------
def test_fake_kernel_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    o = ops.load()
    assert ops.ANALYSIS_OPS == ("mel_spectrogram",)
    assert str(o.mel_spectrogram.default._schema) == "m2s::mel_spectrogram(int handle, Tensor wav, int layout) -> Tensor"
    handle = 0x5EED0  # never dereferenced: fake kernels only shape their outputs
    ops.register_melspec(handle, 2048, 420, (2048 - 420) // 2, 64)
    try:
        with FakeTensorMode():
            wav = torch.empty(2, 5040)
            assert tuple(o.mel_spectrogram(handle, wav, 0).shape) == (2, 64, 12)
            assert tuple(o.mel_spectrogram(handle, wav, 1).shape) == (2, 12, 64)
            assert o.mel_spectrogram(handle, wav, 0).dtype == torch.float32
    finally:
        ops.unregister_melspec(handle)
    with pytest.raises(Exception):
        with FakeTensorMode():
            o.mel_spectrogram(handle, torch.empty(2, 5040), 0)  # an unknown handle


# ---- inference.py ------------------------------------------------------------------------------------------
def test_inference_flag_surface():
    spec = importlib.util.spec_from_file_location("m2s_inference_cli",
                                                  os.path.join(REPO, "mri-to-speech_amd", "inference.py"))
    inf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inf)
    a = inf.parse_args(["--checkpoint_file", "cp/g_1"])
    assert (a.input_wavs_dir, a.output_dir, a.checkpoint_file) == ("test_files", "generated_files", "cp/g_1")
    assert a.dtype is None and a.report is None  # additive flags
    a = inf.parse_args(["--input_wavs_dir", "i", "--output_dir", "o", "--checkpoint_file", "c", "--dtype", "fp32",
                        "--report", "r.json"])
    assert (a.input_wavs_dir, a.output_dir, a.dtype, a.report) == ("i", "o", "fp32", "r.json")
    with pytest.raises(SystemExit):
        inf.parse_args([])
    import meldataset
    assert meldataset.MAX_WAV_VALUE == 32768.0
    with pytest.raises(RuntimeError):  # fails loudly for CPU tensors, like every other plug-in module
        meldataset.mel_spectrogram(torch.zeros(1, 4096), 2048, 64, 11413, 420, 2048, 0, 8000)
    with pytest.raises(FileNotFoundError):
        meldataset.load_wav("/nonexistent/x.wav.wav")


def test_load_wav_round_trip(tmp_path):
    from scipy.io import wavfile
    import meldataset
    pcm = (np.arange(-50, 50) * 300).astype(np.int16)
    wavfile.write(str(tmp_path / "t.wav"), 11413, pcm)
    data, sr = meldataset.load_wav(str(tmp_path / "t.wav.wav"))  # the doubled suffix is repaired
    assert sr == 11413 and np.array_equal(data, pcm)


# ---- the test reference itself -----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C", "A"])
def test_float64_reference_matches_golden(cfg):
    """Ties tests/melspec_ref.py to the reference's own code: meldataset.mel_spectrogram on CPU (fp32)."""
    g, c = np.load(GOLD), R.CONFIGS[cfg]
    assert np.array_equal(g[f"{cfg}_basis"], R.basis(c))
    want = R.mel_f64(g[f"{cfg}_wav"], g[f"{cfg}_basis"], c["n_fft"], c["hop"], c["win"], pad=1, power=1, out=0)
    assert want.shape == g[f"{cfg}_mel"].shape
    assert R.error(g[f"{cfg}_mel"], want, 0) <= R.LN_BAR / 4
    assert os.path.getsize(GOLD) <= 360 * 1024


def test_signals_are_the_documented_ones():
    w = R.signals(3, 5040, 11413)
    assert w.dtype == np.float32 and np.abs(w).max() <= 1.0 and not w[2].any()
    assert 0.15 < w[0].std() < 0.25 and w[1].std() > 0.1


# ---- no device ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_create_without_a_device_fails_loudly():
    L = N.lib()
    cfg = N.MelspecCfg(64, 16, 48, 8, 1, 1, 0, 0.0)
    basis = melspec.slaney_mel_basis(8000, 64, 8)
    h = C.c_void_p()
    assert L.m2s_melspec_create(C.byref(cfg), basis.ctypes.data, 0, C.byref(h)) == 4  # M2S_E_NODEV
    assert not h.value
    with pytest.raises(N.M2SError):
        melspec.MelSpectrogram(64, 16, 48, basis)
