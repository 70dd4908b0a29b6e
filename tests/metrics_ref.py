"""Float64 restatement of the validation metrics (include/m2s.h "fused mel metrics").

Written as the specification reads, one group at a time, in numpy float64 with ``scipy.fft.dct(type=2,
norm="ortho")`` for the MCD-like's DCT.  ``metrics(...)`` returns the dict of slot name -> SUM over the groups (what
one m2s_mel_metrics call writes to ``out``), plus ``per_seq`` (B,3).  tests/test_metrics_cpu.py holds it against the
reference's own classes through tests/golden/metrics_*.npz.
"""
import math

import numpy as np
from scipy.fft import dct

SLOTS = ("loss", "mse", "mae", "delta", "accel", "latest", "band0", "band1", "band2", "band3", "band4", "band5",
         "band6", "band7", "eval_loss", "eval_mse", "eval_mae", "groups", "mcd_sum", "mcd_count")


def train_criterion(pred, target, mask, freq_w, time_w, coeffs):
    """MaskedMSEMAE.forward of the trainer on one batch -> dict loss, mse, mae, delta, accel, latest."""
    B, T, M = pred.shape
    fw = np.asarray(freq_w, np.float64)[None, None, :]
    tw = np.asarray(time_w, np.float64)[None, :, None]
    mk = np.ones((B, T, 1)) if mask is None else np.asarray(mask, np.float64)[:, :, None]
    diff = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    w = fw * tw * mk
    den = max(w.sum(), 1e-6)
    out = {"mse": (diff ** 2 * w).sum() / den, "mae": (np.abs(diff) * w).sum() / den, "delta": 0.0, "accel": 0.0}
    if T > 1:
        d = diff[:, 1:] - diff[:, :-1]
        wd = fw * tw[:, 1:] * mk[:, 1:] * mk[:, :-1]  # the later row's time weight
        out["delta"] = (d ** 2 * wd).sum() / max(wd.sum(), 1e-6)
    if T > 2:
        a = diff[:, 2:] - 2 * diff[:, 1:-1] + diff[:, :-2]
        wa = fw * tw[:, 1:T - 1] * mk[:, 2:] * mk[:, 1:-1] * mk[:, :-2]  # the middle row's time weight
        out["accel"] = (a ** 2 * wa).sum() / max(wa.sum(), 1e-6)
    lw = np.broadcast_to(fw[:, 0], (B, M))  # unmasked, no time weight
    out["latest"] = (diff[:, -1] ** 2 * lw).sum() / max(lw.sum(), 1e-6)
    out["loss"] = out["mse"] + coeffs[0] * out["delta"] + coeffs[1] * out["accel"] + coeffs[2] * out["latest"]
    return out


def band_mae(pred, target, bands):
    """_compute_band_mae: list of (value or None where the clipped band is empty), in the order of ``bands``."""
    diff = np.abs(np.asarray(pred, np.float64) - np.asarray(target, np.float64))
    out = []
    for start, end in bands:
        end = min(end, diff.shape[-1])
        out.append(None if end <= start else diff[..., start:end].mean())
    return out


def eval_criterion(pred, target, mask):
    """eval_mel.py's MaskedMSEMAE on one batch."""
    B, T, _ = pred.shape
    mk = np.ones((B, T, 1)) if mask is None else np.asarray(mask, np.float64)[:, :, None]
    diff = (np.asarray(pred, np.float64) - np.asarray(target, np.float64)) * mk
    den = max(mk.sum(), 1.0)
    mse, mae = (diff ** 2).sum() / den, np.abs(diff).sum() / den
    return {"eval_loss": 0.8 * mse + 0.2 * mae, "eval_mse": mse, "eval_mae": mae}


def power_to_db_of_db(db):
    """librosa.power_to_db(librosa.db_to_power(db)) with ref = 1, amin = 1e-10, top_db = 80, over one array."""
    x = 10.0 * np.log10(np.maximum(1e-10, 10.0 ** (db / 10.0)))
    return np.maximum(x, x.max() - 80.0)


def mcd_like(pred_rows, target_rows, mean, std, n_mfcc=13):
    """eval_mel.mcd_like on the masked rows (n, M) of one sequence."""
    xs = [power_to_db_of_db(np.asarray(v, np.float64) * np.asarray(std, np.float64) + np.asarray(mean, np.float64))
          for v in (pred_rows, target_rows)]
    c = [dct(x, type=2, norm="ortho", axis=1)[:, :n_mfcc] for x in xs]
    return (10.0 / math.log(10.0)) * math.sqrt(2.0) * np.sqrt(((c[0] - c[1]) ** 2).sum(1)).mean()


def metrics(pred, target, mask, group, freq_w, time_w, coeffs, bands, mean=None, std=None, n_mfcc=13):
    B = pred.shape[0]
    group = B if group <= 0 or group >= B else group
    out = {k: 0.0 for k in SLOTS}
    per_seq = np.full((B, 3), np.nan)
    for b0 in range(0, B, group):
        sl = slice(b0, min(B, b0 + group))
        mk = None if mask is None else mask[sl]
        for k, v in train_criterion(pred[sl], target[sl], mk, freq_w, time_w, coeffs).items():
            out[k] += v
        for i, v in enumerate(band_mae(pred[sl], target[sl], bands)):
            if v is not None:
                out[f"band{i}"] += v
        for k, v in eval_criterion(pred[sl], target[sl], mk).items():
            out[k] += v
        out["groups"] += 1
    for b in range(B):
        mk = np.ones(pred.shape[1]) if mask is None else np.asarray(mask[b], np.float64)
        e = (np.asarray(pred[b], np.float64) - np.asarray(target[b], np.float64)) * mk[:, None]
        per_seq[b, 0], per_seq[b, 1] = (e ** 2).sum(), np.abs(e).sum()
        rows = mk != 0
        if mean is None or not rows.any():
            continue
        v = mcd_like(pred[b][rows], target[b][rows], mean, std, n_mfcc)
        if np.isfinite(v):
            per_seq[b, 2] = v
            out["mcd_sum"] += v
            out["mcd_count"] += 1
    return out, per_seq
