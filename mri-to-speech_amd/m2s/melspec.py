"""Waveform -> mel spectrogram on the device (csrc/melspec.hip, ``torch.ops.m2s.mel_spectrogram``).

The opposite direction of the vocoder, in the two conventions the reference uses:

* ``MelSpectrogram.hifigan(h)``         - ``mel_spectrogram`` (meldataset.py:57-93): reflect pad by
  ``(n_fft - hop) // 2``, periodic-Hann STFT, ``sqrt(re^2 + im^2 + 1e-9)``, mel, ``ln(clamp(., 1e-5))``
* ``MelSpectrogram.acoustic_target()``  - ``compute_mel_db`` (mri2speech_code/preprocess_rtmri_data.py:121-147):
  pre-emphasis 0.97, no padding, power spectrum, mel, ``10 log10(max(., 1e-10))``, floor at ``max - top_db``
* ``mel_l1``                            - train.py:228-252's validation metric ``l1(mel(y), mel(G(mel)))``

The engine takes the mel basis from its caller; ``slaney_mel_basis`` is this project's own statement of
``librosa.filters.mel``'s defaults (Slaney scale, ``htk=False``, ``norm="slaney"``).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _native as N
from . import ops as _ops

PAD_NONE, PAD_REFLECT = 0, 1
OUT_LN, OUT_DB, OUT_LINEAR = 0, 1, 2

_F_SP = 200.0 / 3.0               # Hz per mel below the knee
_KNEE_HZ, _KNEE_MEL = 1000.0, 15.0
_LOGSTEP = math.log(6.4) / 27.0   # above the knee: 27 mels per factor of 6.4


def hz_to_mel(f):
    """Slaney's mel scale: linear (200/3 Hz per mel) below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _KNEE_HZ, _KNEE_MEL + np.log(np.maximum(f, _KNEE_HZ) / _KNEE_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _KNEE_MEL, _KNEE_HZ * np.exp(_LOGSTEP * (m - _KNEE_MEL)), _F_SP * m)


def slaney_mel_basis(sr, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None) -> np.ndarray:
    """(n_mels, n_fft // 2 + 1) float32 triangular filters: ``n_mels + 2`` points evenly spaced on the Slaney mel
    scale between ``fmin`` and ``fmax`` (None: ``sr / 2``), each triangle scaled to unit area over Hz
    (``2 / (f[i + 2] - f[i])``).  Computed in float64.  An ``fmax`` above Nyquist is allowed: the filters that lie
    wholly above ``sr / 2`` come out empty."""
    if fmax is None:
        fmax = float(sr) / 2.0
    bins = n_fft // 2 + 1
    fft_hz = np.linspace(0.0, float(sr) / 2.0, bins)
    edges = mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - fft_hz[None, :]
    up = -ramps[:-2] / width[:-1, None]
    down = ramps[2:] / width[1:, None]
    w = np.maximum(0.0, np.minimum(up, down))
    w *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return w.astype(np.float32)


class MelSpectrogram:
    """libm2s's mel-spectrogram engine on one device (include/m2s.h ``m2s_melspec_*``): the tables are built at
    construction, ``forward`` is one call on the current stream."""

    def __init__(self, n_fft: int, hop: int, win: int, mel_basis, pad: int = PAD_REFLECT, power: int = 1,
                 out: int = OUT_LN, preemph: float = 0.0, top_db: Optional[float] = None, out_layout: int = 0,
                 device=None):
        from .runtime import _device
        self.device = _device(device)
        basis = np.ascontiguousarray(np.asarray(mel_basis, dtype=np.float32))
        if basis.ndim != 2 or basis.shape[1] != n_fft // 2 + 1:
            raise N.M2SError(f"mel basis must be (n_mels, {n_fft // 2 + 1}), got {basis.shape}")
        self.n_fft, self.hop, self.win, self.n_mels = int(n_fft), int(hop), int(win), int(basis.shape[0])
        self.top_db, self.out_layout = top_db, int(out_layout)
        L = N.lib()
        self.ops = _ops.load()
        N.check(L.m2s_device_check(self.device.index))
        self._cfg = N.MelspecCfg(self.n_fft, self.hop, self.win, self.n_mels, int(pad), int(power), int(out),
                                 float(preemph))
        h = C.c_void_p()
        N.check(L.m2s_melspec_create(C.byref(self._cfg), basis.ctypes.data, self.device.index, C.byref(h)))
        self._h = h
        self._destroy = L.m2s_melspec_destroy  # bound now: module globals may be gone at exit
        self._unregister = _ops.unregister_melspec
        _ops.register_melspec(h.value, self.n_fft, self.hop, (self.n_fft - self.hop) // 2 if pad else 0, self.n_mels)

    def __del__(self):
        h, destroy = getattr(self, "_h", None), getattr(self, "_destroy", None)
        if h is not None and h.value and destroy is not None:
            self._unregister(h.value)
            destroy(h)
            self._h = None

    @classmethod
    def hifigan(cls, h, device=None) -> "MelSpectrogram":
        """The HiFi-GAN convention from a generator config (``n_fft``, ``num_mels``, ``sampling_rate``,
        ``hop_size``, ``win_size``, ``fmin``, ``fmax``): ln-mel, ``forward`` returns (B, num_mels, T)."""
        basis = slaney_mel_basis(h["sampling_rate"], int(h["n_fft"]), int(h["num_mels"]), h["fmin"], h["fmax"])
        return cls(int(h["n_fft"]), int(h["hop_size"]), int(h["win_size"]), basis, pad=PAD_REFLECT, power=1,
                   out=OUT_LN, device=device)

    @classmethod
    def acoustic_target(cls, sr=11413, n_mels=64, n_fft=2048, win=2048, hop=420, fmin=0, fmax=None, preemph=0.97,
                        top_db=80, device=None) -> "MelSpectrogram":
        """The acoustic model's training target (``mel_db``): ``forward`` returns (B, T, n_mels) in dB, floored at
        each clip's maximum minus ``top_db`` (None: no floor)."""
        basis = slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax)
        return cls(n_fft, hop, win, basis, pad=PAD_NONE, power=2, out=OUT_DB, preemph=preemph, top_db=top_db,
                   out_layout=1, device=device)

    @property
    def handle(self) -> int:
        """The m2s_melspec* as the int ``torch.ops.m2s.mel_spectrogram`` takes."""
        return int(self._h.value)

    def frames(self, L: int) -> int:
        """Frames of an L-sample clip; 0 where ``forward`` would refuse it."""
        return int(N.lib().m2s_melspec_frames(self._h, int(L)))

    def forward(self, wav: torch.Tensor, layout: Optional[int] = None) -> torch.Tensor:
        """wav (B, L), (B, 1, L) or (L,) fp32 in [-1, 1] -> (B, n_mels, T) [layout 0] or (B, T, n_mels) [layout 1];
        the default layout is the convention's (0 for ``hifigan``, 1 for ``acoustic_target``)."""
        from .runtime import _as_f32
        if wav.dim() == 3 and wav.shape[1] == 1:
            wav = wav[:, 0]
        if wav.dim() == 1:
            wav = wav[None]
        if wav.dim() != 2:
            raise N.M2SError(f"expected (B, L) samples, got {tuple(wav.shape)}")
        layout = self.out_layout if layout is None else int(layout)
        mel = self.ops.mel_spectrogram(self.handle, _as_f32(wav, self.device), layout)
        if self.top_db is not None:
            mel = torch.maximum(mel, mel.amax(dim=(1, 2), keepdim=True) - float(self.top_db))
        return mel

    __call__ = forward


_ENGINES: Dict[Tuple, MelSpectrogram] = {}


def hifigan_engine(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, device) -> MelSpectrogram:
    """One HiFi-GAN-convention engine per full config and device, kept for the life of the process."""
    from .runtime import _device
    dev = _device(device)
    key = (int(n_fft), int(num_mels), float(sampling_rate), int(hop_size), int(win_size), float(fmin),
           None if fmax is None else float(fmax), dev.index)
    eng = _ENGINES.get(key)
    if eng is None:
        eng = _ENGINES[key] = MelSpectrogram.hifigan(
            dict(n_fft=n_fft, num_mels=num_mels, sampling_rate=sampling_rate, hop_size=hop_size, win_size=win_size,
                 fmin=fmin, fmax=fmax), device=dev)
    return eng


def mel_l1(wav: torch.Tensor, mel_log: torch.Tensor, h, layout: int = 0) -> torch.Tensor:
    """train.py:228-252's ``mel_spec_error`` per clip: mean |mel(wav) - mel_log| over bins and frames, (B,).
    ``wav`` (B, L) or (B, 1, L) on the device; ``mel_log`` the ln-mel it was generated from, (B, num_mels, T)
    [layout 0] or (B, T, num_mels) [layout 1]; ``h`` the HiFi-GAN config."""
    if wav.device.type != "cuda":
        raise N.M2SError("mel_l1 runs on the HIP device; there is no CPU path")
    eng = hifigan_engine(h["n_fft"], h["num_mels"], h["sampling_rate"], h["hop_size"], h["win_size"], h["fmin"],
                         h["fmax"], wav.device)
    mel = eng.forward(wav, layout=layout)
    ref = mel_log.to(device=mel.device, dtype=torch.float32)
    if ref.shape != mel.shape:
        raise N.M2SError(f"mel of the waveform is {tuple(mel.shape)}, the given mel {tuple(ref.shape)}")
    return (mel - ref).abs().mean(dim=(1, 2))
