"""Numpy restatement of the masking experiment's device side (csrc/frames.hip masked variant, csrc/occlusion.hip;
DESIGN.md §30), independent of m2s/occlusion.py and in float64 where the device sums in float32.

* ``apply_mask``     the reference's application (scripts/mask_rtmri_video.py:96-98): every byte of every channel
                     becomes ``(uint8)clip((float32)byte * mask[y][x], 0, 255)``, truncated toward zero.  A single
                     float32 multiply, so this is exact on every host.
* ``masked_frames``  that on top of tests/frames_ref.py: (M, n, out_h, out_w) uint8 resized variants.
* ``scores``         per variant and band (plus an "all bins" column) the mean over t and the band's bins of
                     |mel[m + 1] - mel[0]|, and the same per frame, float64.
* ``occlusion_map``  the coverage-weighted mean score, c_m = max(1 - mask_m, 0), 0 where the coverage does not exceed
                     1e-6; ``normalize``: (v - min) / ((max - min) + 1e-6) per band, the Grad-CAM heat maps' rule.
"""
import numpy as np

import frames_ref as FR


def apply_mask(frames: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """uint8 (n,h,w) or (n,h,w,3), float32 (h,w) -> uint8 of the same shape."""
    assert frames.dtype == np.uint8 and mask.dtype == np.float32 and mask.shape == frames.shape[1:3]
    m = mask[None, :, :, None] if frames.ndim == 4 else mask[None]
    prod = frames.astype(np.float32) * m
    assert prod.dtype == np.float32
    return np.trunc(np.minimum(np.maximum(prod, np.float32(0)), np.float32(255))).astype(np.uint8)


def masked_frames(frames: np.ndarray, masks: np.ndarray, out_h: int, out_w: int, interp: int) -> np.ndarray:
    return np.stack([FR.frames_ref(apply_mask(frames, m), out_h, out_w, interp) for m in masks])


def band_columns(band_mask: np.ndarray, n_mels: int) -> np.ndarray:
    """(n_bands, n_mels) 0 / 1 -> (n_bands + 1, n_mels) bool with the all-bins row appended."""
    bm = np.asarray(band_mask, dtype=np.float64).reshape(-1, n_mels) != 0
    return np.concatenate([bm, np.ones((1, n_mels), bool)])


def scores(mel: np.ndarray, band_mask: np.ndarray):
    """mel (V,T,n_mels) -> (score (V-1,nb), per_frame (V-1,T,nb)) in float64."""
    mel = np.asarray(mel)
    V, T, n_mels = mel.shape
    d = np.abs(mel[1:].astype(np.float64) - mel[:1].astype(np.float64))  # (M,T,n_mels)
    cols = band_columns(band_mask, n_mels)
    per_frame = np.stack([d[:, :, c].mean(axis=2) if c.any() else np.zeros(d.shape[:2]) for c in cols], axis=2)
    score = np.stack([d[:, :, c].mean(axis=(1, 2)) if c.any() else np.zeros(d.shape[0]) for c in cols], axis=1)
    return score, per_frame


def occlusion_map(score: np.ndarray, masks: np.ndarray, normalize: bool = False) -> np.ndarray:
    """score (M,nb), masks (M,h,w) -> (nb,h,w) float64."""
    c = np.maximum(1.0 - np.asarray(masks, dtype=np.float64), 0.0)  # (M,h,w)
    den = c.sum(axis=0)
    num = np.einsum("mhw,mb->bhw", c, np.asarray(score, dtype=np.float64))
    out = np.where(den > 1e-6, num / np.where(den > 1e-6, den, 1.0), 0.0)
    if normalize:
        lo = out.min(axis=(1, 2), keepdims=True)
        hi = out.max(axis=(1, 2), keepdims=True)
        out = (out - lo) / ((hi - lo) + 1e-6)
    return out
