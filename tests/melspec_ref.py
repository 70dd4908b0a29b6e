"""Float64 reference, inputs and configs of the mel-spectrogram tests (no GPU, no product code path).

``mel_f64`` restates both conventions on float64 frames with numpy's ``rfft``:

* HiFi-GAN (meldataset.py:57-93): reflect pad by ``(n_fft - hop) // 2``, periodic Hann of ``win`` samples centred
  in the frame as ``torch.stft`` does, ``sqrt(re^2 + im^2 + 1e-9)``, mel, ``ln(max(., 1e-5))``
* acoustic target (preprocess_rtmri_data.py:37-43,121-147): pre-emphasis, no pad, power, mel,
  ``10 log10(max(., 1e-10))``, floor at the clip's maximum minus ``top_db``

``mel_torch_f32`` is the same formula as a user would write it with fp32 torch on the CPU (``torch.stft``): the
parity tests hold it to a quarter of their bar on every input, so an input is never what fails.
"""
from __future__ import annotations

import numpy as np
import torch

from m2s.melspec import slaney_mel_basis

LN_BAR = 5e-4                          # mel_log
DB_BAR = 5e-4 * 10.0 / np.log(10.0)    # the same in dB: 2.2e-3
REL_BAR = 5e-4                         # linear output, relative

# name -> engine config and the batch the tests run
CONFIGS = {
    "A": dict(n_fft=2048, hop=420, win=2048, n_mels=64, sr=11413, fmin=0, fmax=8000, B=2, L=5040),
    "B": dict(n_fft=64, hop=16, win=48, n_mels=8, sr=8000, fmin=0, fmax=None, B=3, L=325),
    "C": dict(n_fft=256, hop=101, win=200, n_mels=20, sr=8000, fmin=0, fmax=None, B=3, L=1237),
}


def basis(c) -> np.ndarray:
    return slaney_mel_basis(c["sr"], c["n_fft"], c["n_mels"], c["fmin"], c["fmax"])


def signals(B: int, L: int, sr: float, seed: int = 0) -> np.ndarray:
    """(B, L) float32 within |y| <= 1, cycling through: white noise at 0.2; a 19-harmonic tone stack at 110 Hz
    with amplitudes 0.3 / k over a 1e-2 noise floor; an exact-zero clip."""
    rng = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64) / float(sr)
    out = np.zeros((B, L), dtype=np.float64)
    for b in range(B):
        kind = b % 3
        if kind == 0:
            out[b] = 0.2 * rng.standard_normal(L)
        elif kind == 1:
            for k in range(1, 20):
                out[b] += (0.3 / k) * np.sin(2.0 * np.pi * 110.0 * k * t + 0.37 * k)
            out[b] += 1e-2 * rng.standard_normal(L)
    return np.clip(out, -1.0, 1.0).astype(np.float32)


def n_frames(L: int, n_fft: int, hop: int, pad: int) -> int:
    """Frames of an L-sample clip, 0 where the engine refuses it (pad: 0 none, 1 reflect)."""
    p = (n_fft - hop) // 2 if pad else 0
    if L < 1 or p >= L or L + 2 * p < n_fft:
        return 0
    return 1 + (L + 2 * p - n_fft) // hop


def window_f64(n_fft: int, win: int) -> np.ndarray:
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w


def mel_f64(wav, mel_basis, n_fft, hop, win, pad=1, power=1, out=0, preemph=0.0, top_db=None) -> np.ndarray:
    """(B, L) -> (B, n_mels, T) float64."""
    y = np.asarray(wav, dtype=np.float64)
    if preemph:
        y = np.concatenate([y[:, :1], y[:, 1:] - float(np.float32(preemph)) * y[:, :-1]], axis=1)
    if pad:
        p = (n_fft - hop) // 2
        y = np.pad(y, ((0, 0), (p, p)), mode="reflect")
    T = 1 + (y.shape[1] - n_fft) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    spec = np.fft.rfft(y[:, idx] * window_f64(n_fft, win), axis=-1)      # (B, T, bins)
    s = spec.real ** 2 + spec.imag ** 2
    if power == 1:
        s = np.sqrt(s + 1e-9)
    m = np.einsum("mk,btk->bmt", np.asarray(mel_basis, dtype=np.float64), s)
    if out == 0:
        m = np.log(np.maximum(m, 1e-5))
    elif out == 1:
        m = 10.0 * np.log10(np.maximum(m, 1e-10))
        if top_db is not None:
            m = np.maximum(m, m.max(axis=(1, 2), keepdims=True) - top_db)
    return m


def mel_torch_f32(wav, mel_basis, n_fft, hop, win, pad=1, power=1, out=0, preemph=0.0, top_db=None) -> np.ndarray:
    """The same in fp32 torch on the CPU: F.pad reflect + torch.stft + matmul + log."""
    y = torch.as_tensor(np.asarray(wav, dtype=np.float32))
    if preemph:
        y = torch.cat([y[:, :1], y[:, 1:] - float(preemph) * y[:, :-1]], dim=1)
    if pad:
        p = (n_fft - hop) // 2
        y = torch.nn.functional.pad(y[:, None], (p, p), mode="reflect")[:, 0]
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win), center=False,
                      normalized=False, onesided=True, return_complex=True)
    s = spec.real ** 2 + spec.imag ** 2
    if power == 1:
        s = torch.sqrt(s + 1e-9)
    m = torch.matmul(torch.as_tensor(np.asarray(mel_basis, dtype=np.float32)), s)
    if out == 0:
        m = torch.log(torch.clamp(m, min=1e-5))
    elif out == 1:
        m = 10.0 * torch.log10(torch.clamp(m, min=1e-10))
        if top_db is not None:
            m = torch.maximum(m, m.amax(dim=(1, 2), keepdim=True) - top_db)
    return m.numpy()


def error(got, want, out: int) -> float:
    """Worst error in the unit of the bar: absolute for ln and dB, relative element by element for linear (an
    element that is exactly zero on both sides counts as no error)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = np.abs(got - want)
    if out == 2:
        d = d / np.maximum(np.abs(want), 1e-300)
    return float(d.max())


def bar(out: int) -> float:
    return (LN_BAR, DB_BAR, REL_BAR)[out]
