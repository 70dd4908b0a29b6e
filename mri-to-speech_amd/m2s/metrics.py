"""Validation metrics of the acoustic model on the device (csrc/metrics.hip, include/m2s.h "fused mel metrics").

What the reference computes when it judges a checkpoint, restated as one op:

* ``OTNLikeTrainer.validate()`` (mri2speech_code/train_mri_acoustic_model.py:349-384): the weighted ``MaskedMSEMAE``
  criterion (:57-167) and the band MAEs (:263-277), averaged over the batches;
* ``eval_mel.py``: its ``MaskedMSEMAE`` (:19-32), ``mcd_like`` (:39-82) and the loop that averages them (:104-155).

``torch.ops.m2s.mel_metrics`` takes one (B,T,M) batch of predictions and targets, treats every ``group`` consecutive
sequences as one batch of the reference, and adds the per-batch losses and the batch count to a device accumulator:
two launches, no host synchronisation.  ``MelMetrics`` owns the weights and the accumulator; ``compute()`` is the
one download.  There is no CPU path: a CPU tensor raises ``M2SError``.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import ops as _ops

SLOTS = N.METRICS_SLOTS
RAMP_STEPS = 120000          # MaskedMSEMAE(ramp_steps=...) default, :64
MAX_FRAMES = 128             # MaskedMSEMAE(max_frames=...) default, :64
FOCUS_WEIGHTS = (1.6, 1.45, 1.3, 1.2, 1.15, 1.1, 1.05, 1.02)  # :89
BAND_NAMES = ("f0", "f1", "f2", "high")  # band_ranges' keys, :98-103


def ramp_of_step(step: int, ramp_steps: int = RAMP_STEPS) -> float:
    """The criterion's ramp at a global training step (:117)."""
    return min(1.0, float(step) / float(ramp_steps)) if ramp_steps > 0 else 1.0


def train_weights(n_mels: int, T: int, ramp: float = 1.0):
    """``(freq_w (n_mels,), time_w (T,), (delta, accel, latest) coefficients, bands)`` of the reference's training
    criterion at ``ramp`` in [0, 1] (:64-103,117-121,162-164); float32 arrays computed as the reference computes
    them, ``bands`` a dict name -> (start, end) in the reference's order.

    The frequency ranges are applied in the reference's order, so where they overlap (n_mels < 64) the later range
    wins: at n_mels = 16 the ``high`` range (0, 16) overrides f0 and f1.  The reference builds the time weights for
    ``max_frames`` = 128 rows and raises beyond; here rows past 128 get weight 1.0 (an extension: the reference
    defines no value there)."""
    n, ramp = int(n_mels), float(ramp)
    if n < 1 or T < 1 or not 0.0 <= ramp <= 1.0:
        raise N.M2SError(f"train_weights: n_mels = {n_mels}, T = {T}, ramp = {ramp}")
    ranges = [((0, min(6, n)), 2.0), ((6, min(16, n)), 3.0), ((16, min(32, n)), 2.4), ((32, min(48, n)), 1.6),
              ((max(n - 16, 0), n), 1.8)]
    base = np.ones(n, np.float32)
    target = base.copy()
    for (start, end), w in ranges:
        if end > start:
            target[start:end] = w
    freq_w = np.float32(1.0 - ramp) * base + np.float32(ramp) * target
    tbase = np.ones(T, np.float32)
    ttarget = tbase.copy()
    for i, v in enumerate(FOCUS_WEIGHTS):
        if i < min(T, MAX_FRAMES):
            ttarget[i] = v
    time_w = np.float32(1.0 - ramp) * tbase + np.float32(ramp) * ttarget
    coeffs = (0.3 + 0.15 * ramp, 0.1 + 0.05 * ramp, 0.2 + 0.2 * ramp)
    bands = {"f0": ranges[0][0], "f1": ranges[1][0], "f2": ranges[2][0], "high": ranges[4][0]}
    return freq_w.astype(np.float32), time_w.astype(np.float32), coeffs, bands


def pair_index(lengths: Sequence[int], window: int, device=None) -> torch.Tensor:
    """(P, window) int64: the packed row of row s of pair p, pairs in clip order and windows ascending within a clip
    (the order of ``forward_pairs`` and of the reference's pass3_save_pairs)."""
    rows, off = [], 0
    for n in lengths:
        n = int(n)
        if n < window:
            raise N.M2SError(f"a clip of {n} rows is shorter than the window of {window}")
        rows.append(off + np.arange(n - window + 1)[:, None] + np.arange(window)[None, :])
        off += n
    idx = torch.from_numpy(np.concatenate(rows, 0).astype(np.int64)) if rows else torch.zeros((0, window), dtype=torch.long)
    return idx.to(device) if device is not None else idx


def mel_metrics(pred, target, mask, group, freq_w, time_w, coeffs, bands, mean, std, n_mfcc, acc):
    """``torch.ops.m2s.mel_metrics`` with the device check: (out (len(SLOTS),) fp32 of this call, per_seq (B,3));
    ``acc`` (len(SLOTS),) float64 is added to in place."""
    for name, t in (("pred", pred), ("target", target)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise N.M2SError(f"mel_metrics: {name} must be on the HIP device; there is no CPU path")
    return _ops.load().mel_metrics(pred, target, mask, int(group), freq_w, time_w, [float(c) for c in coeffs],
                                   [int(b) for b in bands], mean, std, int(n_mfcc), acc)


class MelMetrics:
    """The reference's validation numbers, accumulated on the device.

    ``mean`` / ``std`` (n_mels): the scaler, for the MCD-like (both None: skipped, as eval_mel.py without
    ``--stats_json``).  ``ramp``: the training criterion's ramp in [0, 1] (``ramp_of_step(global_step)``; 1.0 = a
    finished schedule).  ``update`` is stream-ordered and does not synchronise; ``compute`` downloads once."""

    def __init__(self, n_mels: int, mean=None, std=None, ramp: float = 1.0, n_mfcc: int = 13, device=None):
        from .runtime import _device
        self.device = _device(device)
        self.n_mels, self.ramp, self.n_mfcc = int(n_mels), float(ramp), int(n_mfcc)
        if (mean is None) != (std is None):
            raise N.M2SError("MelMetrics: mean and std go together")
        to = lambda v: torch.as_tensor(v, dtype=torch.float32).to(self.device).contiguous()
        self.mean, self.std = (None, None) if mean is None else (to(mean), to(std))
        _, _, self.coeffs, self.bands = train_weights(self.n_mels, 1, self.ramp)
        self._flat_bands = [int(v) for name in BAND_NAMES for v in self.bands[name]]
        self._weights: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.acc = torch.zeros(len(SLOTS), dtype=torch.float64, device=self.device)
        self.last: Optional[torch.Tensor] = None      # `out` of the last update
        self.per_seq: Optional[torch.Tensor] = None   # (B,3) of the last update

    def _w(self, T: int):
        if T not in self._weights:
            fw, tw, _, _ = train_weights(self.n_mels, T, self.ramp)
            self._weights[T] = (torch.from_numpy(fw).to(self.device), torch.from_numpy(tw).to(self.device))
        return self._weights[T]

    def update(self, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, group: int = 0):
        """pred / target (B,T,n_mels) standardised dB mels, mask (B,T) floats or None = ones.  Every ``group``
        consecutive sequences are one batch of the reference (0: the whole call is one batch)."""
        if pred.dim() != 3 or pred.shape != target.shape or pred.shape[2] != self.n_mels:
            raise N.M2SError(f"MelMetrics.update: pred {tuple(pred.shape)}, target {tuple(target.shape)}, "
                             f"n_mels {self.n_mels}")
        if pred.shape[0] == 0:
            return self
        fw, tw = self._w(int(pred.shape[1]))
        self.last, self.per_seq = mel_metrics(pred, target, mask, group, fw, tw, self.coeffs, self._flat_bands,
                                              self.mean, self.std, self.n_mfcc, self.acc)
        return self

    def reset(self):
        self.acc.zero_()
        self.last = self.per_seq = None
        return self

    def compute(self) -> dict:
        """One download.  ``loss, mse, mae, delta, accel, latest`` (the criterion's terms, averaged over the
        batches as validate() averages loss, mse, mae), ``band`` {f0, f1, f2, high} (bands that are empty at this
        n_mels are left out, as the reference leaves them out), ``eval`` {loss, mse, mae} (eval_mel.py) and
        ``mcd_like`` (None when no sequence gave a value), plus the counts ``batches`` and ``mcd_sequences``."""
        return result_dict(self.acc.cpu().numpy(), self.bands, self.n_mels)


def result_dict(acc, bands, n_mels: int) -> dict:
    """The accumulator's sums and counts -> the reference's averages (host arithmetic only)."""
    a = {k: float(v) for k, v in zip(SLOTS, acc)}
    n = a["groups"]
    if n <= 0:
        raise N.M2SError("MelMetrics.compute: nothing was accumulated")
    out = {k: a[k] / n for k in ("loss", "mse", "mae", "delta", "accel", "latest")}
    out["band"] = {name: a[f"band{i}"] / n for i, name in enumerate(BAND_NAMES)
                   if min(bands[name][1], n_mels) > bands[name][0]}
    out["eval"] = {k: a[f"eval_{k}"] / n for k in ("loss", "mse", "mae")}
    out["mcd_like"] = a["mcd_sum"] / a["mcd_count"] if a["mcd_count"] > 0 else None
    out["batches"], out["mcd_sequences"] = int(n), int(a["mcd_count"])
    return out
