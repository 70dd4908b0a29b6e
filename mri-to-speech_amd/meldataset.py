"""wav -> ln-mel on the MI355X: the part of meldataset.py that inference and validation import.

Contract kept from the reference (meldataset.py:11-24,57-93): ``MAX_WAV_VALUE``; ``load_wav(path)`` returning
``(data, sampling_rate)`` as scipy reads them, a doubled ``.wav.wav`` suffix repaired and a missing file
raising ``FileNotFoundError``; ``mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin,
fmax, center=False)`` taking (B, L) samples in [-1, 1] and returning the (B, num_mels, T) ln-mel: reflect pad
by ``int((n_fft - hop_size) / 2)``, periodic-Hann STFT without centring, ``sqrt(re^2 + im^2 + 1e-9)``, Slaney mel
basis, ``ln(clamp(., 1e-5))``.

How it runs: one ``m2s.melspec.MelSpectrogram`` engine per FULL config (every argument) and device, built on
first use and kept.  The reference keys its cached basis by ``fmax`` alone and its window by device alone, so a
second call with another ``n_fft``, ``num_mels`` or ``win_size`` silently reuses the first call's tables; here
every config gets its own.  ``center=True`` (which the reference's signature defaults to but its STFT call
ignores) is refused.  The training dataset class is not part of this module.  There is no CPU path.
"""
from __future__ import annotations

import os
import sys

import torch

_ROOT = os.path.dirname(os.path.abspath(__file__))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from m2s import melspec as _melspec  # noqa: E402

MAX_WAV_VALUE = 32768.0


def load_wav(full_path):
    """(samples as stored, sampling rate)."""
    from scipy.io.wavfile import read

    path = str(full_path)
    if path.endswith(".wav.wav"):
        path = path[:-4]
    if not os.path.exists(path):
        raise FileNotFoundError(f"File not found: {path}")
    sampling_rate, data = read(path)
    return data, sampling_rate


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    if center:
        raise NotImplementedError("mel_spectrogram: center=True is not implemented (the reference pads by "
                                  "(n_fft - hop_size) / 2 and runs its STFT with center=False whatever is passed)")
    if not isinstance(y, torch.Tensor) or y.device.type != "cuda":
        raise RuntimeError("mel_spectrogram runs on the MI355X (HIP) device only: move the samples there first; "
                           "there is no CPU path")
    eng = _melspec.hifigan_engine(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, y.device)
    return eng.forward(y, layout=0)
