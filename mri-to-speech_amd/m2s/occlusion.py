"""The masking experiment (docs/rtmri_pipeline_notes.md step 5; scripts/mask_rtmri_video.py) on the device.

* ``build_mask`` / ``preset_mask`` / ``polygon_from_json`` / ``grid_masks``: soft articulator masks, built once per
  experiment on the host (a mask is at most 65536 floats).  They restate the reference's ``build_mask`` (:53-68): a
  float32 image of ones, a convex polygon filled with ``alpha``, a Gaussian blur, a clip to [alpha, 1].  The fill and
  the blur follow the rules of DESIGN.md §30; their parity with cv2.fillConvexPoly / cv2.GaussianBlur is
  unpinned.
* ``apply_mask_host``: the reference's application (:96-98) in numpy, for writing a masked stack to disk.
* ``reduce``: ``torch.ops.m2s.occlusion_reduce``, the variants' mels -> scores, per-frame scores and a coverage-weighted
  map, on the device (csrc/occlusion.hip).

The masked variants themselves are made by ``torch.ops.m2s.preprocess_frames_masked`` (``runtime.
preprocess_frames_masked``) and the whole experiment by ``runtime.Pipeline.occlusion``.
"""
from __future__ import annotations

import json
from typing import Dict, Iterable, Mapping, Optional, Sequence, Tuple

import numpy as np

# name -> polygon vertices (x, y) on a 256 x 256 frame: the regions the reference's --mask-type presets darken
PRESETS: Dict[str, Tuple[Tuple[float, float], ...]] = {
    "lip": ((8.0, 84.0), (43.0, 84.0), (45.0, 156.0), (8.0, 156.0)),
    "tongue": ((36.1, 102.7), (63.4, 90.9), (122.7, 111.5), (133.4, 172.2), (47.6, 155.0)),
}
PRESET_BASE = (256.0, 256.0)  # (width, height) the presets are drawn on

_FIXED_KERNELS = {
    1: (1.0,),
    3: (0.25, 0.5, 0.25),
    5: (0.0625, 0.25, 0.375, 0.25, 0.0625),
    7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125),
}


def odd_kernel(blur_kernel: int) -> int:
    """The kernel size the blur runs at: 0 / 1 = none, an even size is the next odd one."""
    k = int(blur_kernel)
    if k <= 1:
        return 1
    return k + 1 if k % 2 == 0 else k


def gaussian_kernel(k: int) -> np.ndarray:
    """The 1-D float32 Gaussian of odd size k for sigma = 0 (OpenCV's getGaussianKernel rule): fixed tables up to 7,
    else sigma = 0.3 ((k - 1) / 2 - 1) + 0.8 and exp(-x^2 / 2 sigma^2) in double, normalised to sum 1."""
    k = int(k)
    if k < 1 or k % 2 == 0:
        raise ValueError(f"Gaussian kernel size {k} must be odd and positive")
    if k in _FIXED_KERNELS:
        return np.asarray(_FIXED_KERNELS[k], dtype=np.float32)
    sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def _blur_axis(img: np.ndarray, kern: np.ndarray, axis: int) -> np.ndarray:
    r = len(kern) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(img, pad, mode="reflect")  # reflect-101: the border pixel is not repeated
    acc = np.zeros_like(img, dtype=np.float32)
    n = img.shape[axis]
    for i, c in enumerate(kern):
        acc += np.float32(c) * (p[:, i:i + n] if axis == 1 else p[i:i + n, :])
    return acc


def gaussian_blur(img: np.ndarray, blur_kernel: int) -> np.ndarray:
    """Separable Gaussian of ``odd_kernel(blur_kernel)`` taps along rows, then columns, border reflect-101, float32
    accumulation in tap order."""
    k = odd_kernel(blur_kernel)
    img = np.ascontiguousarray(img, dtype=np.float32)
    if k == 1:
        return img
    kern = gaussian_kernel(k)
    return _blur_axis(_blur_axis(img, kern, 1), kern, 0)


def _round_half_up(x: float) -> int:
    return int(np.floor(x + 0.5))


def check_polygon(points) -> np.ndarray:
    """(n, 2) float64 vertices of a convex polygon with n >= 3, or ValueError."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 3:
        raise ValueError("a mask polygon needs at least 3 vertices [[x, y], ...]")
    if not np.isfinite(pts).all():
        raise ValueError("mask polygon vertices must be finite")
    d = np.roll(pts, -1, axis=0) - pts
    cross = d[:, 0] * np.roll(d, -1, axis=0)[:, 1] - d[:, 1] * np.roll(d, -1, axis=0)[:, 0]
    if (cross > 0).any() and (cross < 0).any():
        raise ValueError("the mask polygon is concave; only convex polygons are filled")
    if not (cross != 0).any():
        raise ValueError("the mask polygon is degenerate (all vertices on one line)")
    return pts


def scale_polygon(points, shape: Tuple[int, int], base_size=PRESET_BASE) -> np.ndarray:
    """Vertices drawn on ``base_size`` = (width, height) -> integer vertices on a frame of ``shape`` = (h, w): scaled
    in float32 and rounded as ``np.round`` does, the reference's MaskPreset.scaled + build_mask."""
    h, w = int(shape[0]), int(shape[1])
    pts = np.array(points, dtype=np.float32)
    pts[:, 0] *= np.float32(w / float(base_size[0]))
    pts[:, 1] *= np.float32(h / float(base_size[1]))
    return np.round(pts).astype(np.int32)


def fill_convex(mask: np.ndarray, poly_int: np.ndarray, value: float) -> None:
    """Fill the convex polygon with integer vertices into ``mask`` in place, boundary included: for every row y from
    ymin to ymax the columns round-half-up(x_left(y)) .. round-half-up(x_right(y)), clipped to the image."""
    h, w = mask.shape
    pts = [(int(x), int(y)) for x, y in poly_int]
    ymin, ymax = min(p[1] for p in pts), max(p[1] for p in pts)
    for y in range(max(ymin, 0), min(ymax, h - 1) + 1):
        xs = []
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            if y0 == y1:
                if y == y0:
                    xs += [float(x0), float(x1)]
            elif min(y0, y1) <= y <= max(y0, y1):
                xs.append(x0 + (y - y0) * (x1 - x0) / float(y1 - y0))
        if not xs:
            continue
        lo, hi = max(_round_half_up(min(xs)), 0), min(_round_half_up(max(xs)), w - 1)
        if lo <= hi:
            mask[y, lo:hi + 1] = value


def build_mask(shape: Tuple[int, int], polygon, alpha: float = 0.1, blur_kernel: int = 11) -> np.ndarray:
    """(h, w) float32 soft mask: ones, ``polygon`` ((n, 2) vertices in frame pixels, rounded to integers) filled with
    ``alpha``, blurred with ``blur_kernel`` taps where that is > 1, clipped to [alpha, 1]."""
    h, w = int(shape[0]), int(shape[1])
    if h < 1 or w < 1:
        raise ValueError(f"bad mask shape {shape}")
    check_polygon(polygon)
    mask = np.ones((h, w), dtype=np.float32)
    fill_convex(mask, np.round(np.asarray(polygon, dtype=np.float32)).astype(np.int32), np.float32(alpha))
    if int(blur_kernel) > 1:
        mask = gaussian_blur(mask, blur_kernel)
    return np.clip(mask, np.float32(alpha), np.float32(1.0)).astype(np.float32)


def preset_mask(name: str, shape: Tuple[int, int], alpha: float = 0.1, blur_kernel: int = 11) -> np.ndarray:
    """The reference's ``--mask-type`` presets ("lip", "tongue") on a frame of ``shape`` = (h, w)."""
    if name not in PRESETS:
        raise ValueError(f"unknown mask preset {name!r}; one of {sorted(PRESETS)}")
    return build_mask(shape, scale_polygon(PRESETS[name], shape), alpha, blur_kernel)


def polygon_from_json(path_or_obj):
    """A custom polygon: ``[[x, y], ...]`` or ``{"points": [[x, y], ...], "base_size": [width, height]}`` (a path, a
    JSON string's parsed object, or the object itself) -> (vertices (n, 2) float64, base_size or None = frame
    pixels).  Fewer than 3 vertices or a concave polygon: ValueError."""
    obj = path_or_obj
    if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__"):
        with open(obj) as f:
            obj = json.load(f)
    base = None
    if isinstance(obj, Mapping):
        base = obj.get("base_size")
        obj = obj.get("points")
    pts = check_polygon(obj)
    if base is not None:
        base = (float(base[0]), float(base[1]))
        if not (base[0] > 0 and base[1] > 0):
            raise ValueError("base_size must be positive [width, height]")
    return pts, base


def custom_mask(path_or_obj, shape: Tuple[int, int], alpha: float = 0.1, blur_kernel: int = 11) -> np.ndarray:
    """``build_mask`` of a JSON polygon, scaled from its ``base_size`` where it names one."""
    pts, base = polygon_from_json(path_or_obj)
    poly = scale_polygon(pts, shape, base) if base is not None else pts
    return build_mask(shape, poly, alpha, blur_kernel)


def grid_positions(shape: Tuple[int, int], patch: int, stride: int):
    """Top-left corners (y, x) of the sweep's squares: every ``stride`` pixels from 0 while the corner is inside."""
    h, w = int(shape[0]), int(shape[1])
    if patch < 1 or stride < 1:
        raise ValueError("patch and stride must be positive")
    return [(y, x) for y in range(0, h, int(stride)) for x in range(0, w, int(stride))]


def grid_masks(shape: Tuple[int, int], patch: int, stride: int, alpha: float = 0.0, blur_kernel: int = 0) -> np.ndarray:
    """(G, h, w) float32: one soft square of ``patch`` pixels (cut at the border) per ``grid_positions`` corner, made
    as ``build_mask`` makes a polygon: fill with ``alpha``, blur, clip to [alpha, 1]."""
    h, w = int(shape[0]), int(shape[1])
    out = []
    for y, x in grid_positions(shape, patch, stride):
        m = np.ones((h, w), dtype=np.float32)
        m[y:y + int(patch), x:x + int(patch)] = np.float32(alpha)
        if int(blur_kernel) > 1:
            m = gaussian_blur(m, blur_kernel)
        out.append(np.clip(m, np.float32(alpha), np.float32(1.0)).astype(np.float32))
    return np.stack(out)


def apply_mask_host(frames: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """The reference's application on the host: uint8 (n,h,w) or (n,h,w,3) frames, (h,w) mask ->
    ``(frame.astype(float32) * mask).clip(0, 255).astype(uint8)``; the device front end gives the same bytes."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim not in (3, 4):
        raise ValueError("expected uint8 frames (n,h,w) or (n,h,w,3)")
    mask = np.asarray(mask, dtype=np.float32)
    if mask.shape != frames.shape[1:3]:
        raise ValueError(f"mask shape {mask.shape} != frame shape {frames.shape[1:3]}")
    m = mask[None, :, :, None] if frames.ndim == 4 else mask[None]
    return (frames.astype(np.float32) * m).clip(0.0, 255.0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- device reduction
def band_matrix(bands: Optional[Mapping[str, Iterable[int]]], n_mels: int):
    """{name: mel-bin indices} (``m2s.gradcam.parse_band_arguments``) -> ((n_bands, n_mels) 0 / 1 float32 tensor on the
    host, column names with "all" appended).  At most 8 bands."""
    import torch
    bands = dict(bands or {})
    if len(bands) > 8:
        raise ValueError("at most 8 bands")
    if "all" in bands:
        raise ValueError('the band name "all" is taken by the all-bins column')
    m = torch.zeros(len(bands), int(n_mels))
    for b, (name, idx) in enumerate(bands.items()):
        idx = [int(i) for i in idx]
        if not idx:
            raise ValueError(f"band {name!r} selects no mel bin")
        if min(idx) < 0 or max(idx) >= n_mels:
            raise IndexError(f"band {name!r} has a mel bin outside 0..{n_mels - 1}")
        m[b, idx] = 1.0
    return m, [*bands, "all"]


def reduce(mel, bands=None, masks=None, normalize: bool = False, per_frame: bool = True):
    """mel (V,T,n_mels) on the device, variant 0 the baseline -> dict: ``score`` (V-1,nb), ``per_frame`` (V-1,T,nb) or
    None, ``map`` (nb,h,w) or None (needs ``masks`` (V-1,h,w)), ``names`` (nb column names, the last "all").
    ``bands``: {name: bin indices}, a (n_bands,n_mels) 0 / 1 tensor, or None for the all-bins column alone.  One
    ``torch.ops.m2s.occlusion_reduce`` call: two launches, no host read, bit-identical on repetition."""
    import torch

    from . import _native as N
    from . import ops as _ops
    if not torch.is_tensor(mel) or mel.device.type != "cuda":
        raise N.M2SError("occlusion.reduce runs on the HIP device; there is no CPU path")
    if mel.dim() != 3:
        raise N.M2SError(f"expected mel (V,T,n_mels), got {tuple(mel.shape)}")
    if torch.is_tensor(bands):
        bm, names = bands, [f"band{i}" for i in range(bands.shape[0])] + ["all"]
    else:
        bm, names = band_matrix(bands, mel.shape[2])
    mk = None
    if masks is not None:
        mk = torch.as_tensor(masks, dtype=torch.float32).to(mel.device)
    score, pf, mp = _ops.load().occlusion_reduce(mel, bm.to(mel.device, torch.float32), mk, bool(normalize),
                                                 bool(per_frame))
    return {"score": score, "per_frame": pf if per_frame else None, "map": mp if mk is not None else None,
            "names": names}
