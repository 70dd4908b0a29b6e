"""Numpy restatement of the device frame front end's resize rule (csrc/frames.hip).

The rule is OpenCV's 8-bit two-tap fixed-point path: ``cv2.resize(..., INTER_LINEAR)``, and ``INTER_AREA`` where no
axis shrinks.  Per axis with source size ``s`` and destination size ``d``: ``inv = (double)d / s``, ``scale = 1.0 /
inv``, and for destination index ``i``

* LINEAR  ``f = (float)((i + 0.5) * scale - 0.5); i0 = floor(f); f = f - (float)i0``
* AREA    ``i0 = floor(i * scale); f = (float)((i + 1) - (i0 + 1) * inv); f = 0 if f <= 0 else f - floor(f)``
* ``w1 = rint(f * 2048)``, ``w0 = rint((1 - f) * 2048)`` in float32, half to even
* taps ``clamp(i0, 0, s - 1)`` and ``clamp(i0 + 1, 0, s - 1)``, the weights kept when a tap is clamped
* ``R[y][x] = S[y][x0] * a0 + S[y][x1] * a1`` (int32)
* ``out = (((b0 * (R[y0][x] >> 4)) >> 16) + ((b1 * (R[y1][x] >> 4)) >> 16) + 2) >> 2``

Everything below is integers, float32 and float64 basic operations, so it is exact on every host.  ``bilinear_f64``
is the plain half-pixel bilinear interpolation in float64 the fixed-point LINEAR rule approximates.
"""
import numpy as np

LINEAR, AREA = 0, 1
INTERPS = {"linear": LINEAR, "area": AREA}
COEF_ONE = 2048


def axis_coefficients(s: int, d: int, interp: int):
    """(t0, t1, w0, w1) int32 arrays of length d: the two clamped taps and their 11-bit weights."""
    if interp not in (LINEAR, AREA):
        raise ValueError(f"unknown interp {interp}")
    if d < s:
        raise ValueError("the two-tap rule covers no shrinking axis")
    inv = np.float64(d) / np.float64(s)
    scale = np.float64(1.0) / inv
    i = np.arange(d, dtype=np.float64)
    if interp == LINEAR:
        f = ((i + 0.5) * scale - 0.5).astype(np.float32)
        fl = np.floor(f)
        i0 = fl.astype(np.int64)
        f = f - fl  # float32
    else:
        i0 = np.floor(i * scale).astype(np.int64)
        f = ((i + 1.0) - (i0 + 1).astype(np.float64) * inv).astype(np.float32)
        f = np.where(f <= 0, np.float32(0), f - np.floor(f)).astype(np.float32)
    assert f.dtype == np.float32
    w1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int32)
    w0 = np.rint((np.float32(1) - f) * np.float32(COEF_ONE)).astype(np.int32)
    t0 = np.clip(i0, 0, s - 1).astype(np.int32)
    t1 = np.clip(i0 + 1, 0, s - 1).astype(np.int32)
    return t0, t1, w0, w1


def bgr_to_grey(frame: np.ndarray) -> np.ndarray:
    """cv2.COLOR_BGR2GRAY's 8-bit fixed point, as csrc/preprocess.hip restates it."""
    f = frame.astype(np.int64)
    return ((1868 * f[..., 0] + 9617 * f[..., 1] + 4899 * f[..., 2] + (1 << 13)) >> 14).astype(np.uint8)


def resize(grey: np.ndarray, out_h: int, out_w: int, interp: int) -> np.ndarray:
    """(h, w) uint8 -> (out_h, out_w) uint8 by the rule above."""
    if grey.dtype != np.uint8 or grey.ndim != 2:
        raise ValueError("expected one (h, w) uint8 frame")
    h, w = grey.shape
    y0, y1, b0, b1 = axis_coefficients(h, out_h, interp)
    x0, x1, a0, a1 = axis_coefficients(w, out_w, interp)
    S = grey.astype(np.int32)
    R = S[:, x0] * a0[None, :] + S[:, x1] * a1[None, :]  # (h, out_w) int32
    top = (b0[:, None] * (R[y0] >> 4)) >> 16
    bot = (b1[:, None] * (R[y1] >> 4)) >> 16
    out = (top + bot + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def frames_ref(frames: np.ndarray, out_h: int, out_w: int, interp: int) -> np.ndarray:
    """(n, h, w) grey or (n, h, w, 3) BGR uint8 -> (n, out_h, out_w) uint8: grey first, then the resize."""
    grey = bgr_to_grey(frames) if frames.ndim == 4 else frames
    return np.stack([resize(g, out_h, out_w, interp) for g in grey]) if len(grey) else \
        np.zeros((0, out_h, out_w), np.uint8)


def unit(resized: np.ndarray) -> np.ndarray:
    """The training convention's normalisation: float32 / 255 (correctly rounded)."""
    return resized.astype(np.float32) / np.float32(255)


def bilinear_f64(grey: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """Half-pixel-centre bilinear interpolation with replicated borders, float64, unrounded."""
    h, w = grey.shape
    S = grey.astype(np.float64)

    def axis(s, d):
        c = (np.arange(d, dtype=np.float64) + 0.5) * (s / d) - 0.5
        i0 = np.floor(c)
        f = c - i0
        return np.clip(i0, 0, s - 1).astype(np.int64), np.clip(i0 + 1, 0, s - 1).astype(np.int64), f

    y0, y1, fy = axis(h, out_h)
    x0, x1, fx = axis(w, out_w)
    R = S[:, x0] * (1 - fx)[None, :] + S[:, x1] * fx[None, :]
    return R[y0] * (1 - fy)[:, None] + R[y1] * fy[:, None]
