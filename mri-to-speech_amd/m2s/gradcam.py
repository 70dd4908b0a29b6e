"""Grad-CAM engine: every formant band and every target frame of one clip in one device pass.

What the reference's scripts/mri_gradcam_formant.py does per band with autograd (compute_gradcam :203-279 over
_forward_with_features :128-166 and _compute_cam_from_grads :169-200) is one ``torch.ops.m2s.gradcam`` call
here: one train-mode backbone forward, GAP, the BiLSTM with saved activations and the head; then
the K = n_bands * (1 + n_frames) targets' cotangents go through the backward through time together, and the
heat maps (channel weights, ReLU, bilinear resize, min-max) are made on the device.  ``feats.grad`` is constant
over a channel's positions (``pooled = feats.mean((2, 3))``), so the channel weights are ``dpooled / (h w)`` and
no gradient map is ever formed.

The band arithmetic (``mel_bin_frequencies``, ``parse_band_arguments``) follows :58-119: HTK mel scale,
n_mels + 2 points from fmin to fmax, the midpoints of neighbouring points as bin centres.

No CPU path: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import ops as _ops
from .autograd import CamEngine, _need_hip

DEFAULT_BANDS = {"F1": (300.0, 900.0), "F2": (900.0, 2500.0)}
REDUCTIONS = {"mean": 0, "sum": 1}


def mel_bin_frequencies(n_mels: int, sampling_rate: int, fmin: float, fmax: Optional[float]) -> np.ndarray:
    """Centre frequencies (Hz) between the n_mels + 2 HTK-mel points from fmin to fmax: n_mels + 1 values
    (65 for 64 mels).  fmax None or <= 0 means Nyquist."""
    if fmax is None or fmax <= 0:
        fmax = sampling_rate / 2
    lo, hi = (2595.0 * np.log10(1.0 + f / 700.0) for f in (float(fmin), float(fmax)))
    pts = np.linspace(lo, hi, n_mels + 2)
    return 700.0 * (10.0 ** ((0.5 * (pts[:-1] + pts[1:])) / 2595.0) - 1.0)


def parse_band_arguments(band_args: Optional[Sequence[str]], n_mels: int, sampling_rate: int, fmin: float,
                         fmax: Optional[float]) -> Dict[str, np.ndarray]:
    """``NAME:LOW-HIGH`` specs (Hz) -> {name: mel-bin indices whose centre lies in [LOW, HIGH]}; no specs = F1
    300-900 and F2 900-2500.  ValueError for a malformed spec, an empty band, and a band that selects centre
    index n_mels (there are n_mels + 1 centres but n_mels bins; the reference fails later, in index_select)."""
    bands = {}
    for spec in band_args or ():
        name, sep, rest = spec.partition(":")
        low_s, dash, high_s = rest.partition("-")
        if not sep or not dash:
            raise ValueError(f"invalid band specification {spec!r}: use NAME:LOW-HIGH")
        try:
            low, high = float(low_s), float(high_s)
        except ValueError:
            raise ValueError(f"band range must be numeric: {spec!r}") from None
        if high <= low:
            raise ValueError(f"band upper bound must exceed the lower bound: {spec!r}")
        bands[name.strip()] = (low, high)
    if not bands:
        bands = dict(DEFAULT_BANDS)
    freqs = mel_bin_frequencies(n_mels, sampling_rate, fmin, fmax)
    out = {}
    for name, (low, high) in bands.items():
        idx = np.flatnonzero((freqs >= low) & (freqs <= high))
        if idx.size == 0:
            raise ValueError(f"no mel bin centre lies inside {name} ({low}-{high} Hz); adjust the band or the mel settings")
        if idx[-1] >= n_mels:
            raise ValueError(f"band {name} ({low}-{high} Hz) reaches centre index {int(idx[-1])}, but the model has "
                             f"mel bins 0..{n_mels - 1}; lower the band's upper bound (centre {n_mels} is at "
                             f"{freqs[n_mels]:.0f} Hz)")
        out[name] = idx
    return out


class GradCam:
    """``GradCam(model_or_state_dict, device).run(frames, mean, std, bands, ...)``."""

    def __init__(self, model_or_state_dict, device=None):
        from .runtime import _device
        self.device = _device(device)
        self.module = model_or_state_dict if isinstance(model_or_state_dict, torch.nn.Module) else None
        sd = self.module.state_dict() if self.module is not None else model_or_state_dict
        L = N.lib()
        self.ops = _ops.load()
        N.check(L.m2s_device_check(self.device.index))
        sd = {k: v for k, v in sd.items() if k.startswith(("cnn.backbone.", "rnn.lstm.", "head."))}
        arr, keep = N.tensor_array(sd)
        h = C.c_void_p()
        N.check(L.m2s_gradcam_create(arr, len(arr), self.device.index, C.byref(h)))
        del keep
        self._h = h
        self._destroy = L.m2s_gradcam_destroy
        self.n_mels = L.m2s_gradcam_n_mels(h)
        self.chunk = L.m2s_gradcam_chunk()
        self.layers = _ops.cam_bn_layers()  # what CamEngine.update_running_stats walks
        if L.m2s_gradcam_bn_stats_floats(h) != _ops.CAM_BN_STATS:
            raise N.M2SError("libm2s BatchNorm layer table does not match the timm block table")

    def __del__(self):
        h, destroy = getattr(self, "_h", None), getattr(self, "_destroy", None)
        if h is not None and h.value and destroy is not None:
            destroy(h)
            self._h = None

    @property
    def handle(self) -> int:
        """The m2s_gradcam* as the int torch.ops.m2s.gradcam takes."""
        return int(self._h.value)

    def band_mask(self, bands: Mapping[str, Iterable[int]]) -> torch.Tensor:
        if not bands:
            raise ValueError("GradCam.run needs at least one band")
        mask = torch.zeros(len(bands), self.n_mels)
        for b, (name, idx) in enumerate(bands.items()):
            idx = [int(i) for i in idx]
            if not idx:
                raise ValueError(f"band {name!r} selects no mel bin")
            if min(idx) < 0 or max(idx) >= self.n_mels:
                raise IndexError(f"band {name!r} has a mel bin outside 0..{self.n_mels - 1}")
            mask[b, idx] = 1.0
        return mask

    def run(self, frames: torch.Tensor, mean, std, bands: Mapping[str, Iterable[int]], reduction: str = "mean",
            frame_indices: Sequence[int] = (), update_running_stats: bool = False, return_dpooled: bool = True):
        """frames (T,H,W) or (1,T,1,H,W) on the device; mean / std the scaler (arrays or tensors); bands
        {name: mel-bin indices}.  Returns {name: {"heatmaps" (T,H,W), "per_frame" {idx: (H,W)}, "pred_norm"
        (T,n_mels), "dpooled" (1 + F,T,208): row 0 the whole-clip target, row 1 + j target frame j; None with
        return_dpooled=False}}.  The module's BatchNorm buffers are left alone unless update_running_stats."""
        _need_hip(frames, "GradCam")
        if frames.dim() == 5:
            if frames.shape[0] != 1 or frames.shape[2] != 1:
                raise ValueError(f"GradCam takes one clip, (1,T,1,H,W); got {tuple(frames.shape)}")
            frames = frames[0, :, 0]
        if frames.dim() != 3:
            raise ValueError(f"GradCam frames must be (T,H,W) or (1,T,1,H,W); got {tuple(frames.shape)}")
        if reduction not in REDUCTIONS:
            raise ValueError(f"unknown reduction {reduction!r}; choose mean or sum")
        T, H, W = frames.shape
        fidx = [int(i) for i in frame_indices]
        for i in fidx:
            if not 0 <= i < T:
                raise IndexError(f"target frame {i} outside [0, {T})")
        mask = self.band_mask(bands)
        dev = frames.device
        mu, sd = (torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=torch.float32).to(dev)
                  for v in (mean, std))
        x = frames.to(torch.float32).contiguous()
        heat_seq, heat_frame, pred, dpooled, stats = self.ops.gradcam(self.handle, x, mu, sd, mask, fidx,
                                                                      REDUCTIONS[reduction], bool(return_dpooled))
        if update_running_stats:
            self._update_running_stats(stats, T, H, W)
        out = {}
        F = len(fidx)
        for b, name in enumerate(bands):
            out[name] = {"heatmaps": heat_seq[b], "per_frame": {i: heat_frame[b, j] for j, i in enumerate(fidx)},
                         "pred_norm": pred,
                         "dpooled": dpooled[b * (1 + F):(b + 1) * (1 + F)] if return_dpooled else None}
        self.last_stats = stats
        return out

    def _update_running_stats(self, stats, n, h, w):
        if self.module is None:
            raise N.M2SError("update_running_stats needs the module GradCam was built from")
        bns = {k: m for k, m in self.module.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
        bufs = {f"{k}.{b}": t for k, m in bns.items() for b, t in m.named_buffers()}
        momenta = {k: m.momentum for k, m in bns.items() if m.track_running_stats}
        if momenta:
            CamEngine.update_running_stats(self, bufs, stats, n, h, w, momenta)
