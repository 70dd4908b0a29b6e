"""Quantisation-faithful float64 restatements of the bf16 and e4m3 early-CNN kernels, with per-element budgets.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Plain torch / numpy on the CPU, written from this
repository's kernels (csrc/*.hip) and packers (csrc/pack.hpp, csrc/pack_acoustic.cpp).

Every block function takes the block's input exactly as the engine stores it (bf16 values, or the fp32 frames for
the stem) and returns ``(ref, budget)`` in float64 with the block's output shape (N, C, H, W):

  ref     the value the kernel holds in fp32 just before its final bf16 store, evaluated in float64 on the
          kernel's own quantised operands (rounded weights, rounded input, rounded intermediate map);
  budget  a bound on |stored output - ref| for an implementation that rounds where the kernel rounds.

The budget is a sum of named terms, each tied to one rounding point of the kernel (the docstrings list them with
file and line):

  output rounding   half a spacing of the bf16 grid at |ref| + (the terms below) (the spacing of the binade the
                    perturbed value can reach).  The stored value is the bf16 nearest to the device's fp32 value,
                    which lies within the terms below of ref, so half a spacing on top of them bounds every
                    element, whether or not ref sits near a rounding boundary; the budget is never widened to a
                    whole spacing.
  fp32 accumulation one fp32 ulp (2^-23, which covers round-to-nearest and truncation) of the running magnitude
                    per operation: (K + the epilogue's multiplies and adds) * 2^-23 * sum|w||x| per GEMM, plus
                    2^-23 times the bias and skip magnitudes for the adds they enter.
  split operands    stem_b0.hip only: its three-term bf16 split of the fp32 frame and weight is restated exactly
                    (hi = bf16(v), lo = bf16(v - hi); hi*hi + hi*lo + lo*hi), so it adds no term of its own.
  transcendentals   the fast SiLU x * v_rcp_f32(1 + v_exp_f32(-x log2 e)) (m2s_common.hpp:225-234, which states
                    the 1 ulp of v_exp_f32 and v_rcp_f32 the AMD ISA documents; the rounding of the exponent's
                    argument, of 1 + e and of the product add half an ulp each), times |SiLU|, and SiLU's slope
                    bound 1.1 on the error of its argument.
  intermediate flips  every element of an intermediate map whose pre-rounding value lies within its accumulated
                    error of a rounding boundary of its grid may be stored one grid step away: one spacing at that
                    value (plus the error itself where that exceeds the spacing, which happens only next to zero),
                    carried through the following GEMM as sum|w| * spacing over the flagged elements only.

There is no multiplier on the sum and no cap on the number of flagged elements.  ``arith="exact"`` turns every
rounding off (the budget is zero), which ties the restatement to oracle/effnet.py; ``impl="float32"`` evaluates
the same quantised operands with float32 convolutions and rounds as the kernel does (a correctly rounded
stand-in with another summation order), returning the stored output alone.  ``fault`` seeds one indexing or
operand mistake into the computation (tests/test_lowprec_cpu.py).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -23       # one fp32 ulp, relative
SILU_SLOPE = 1.1       # max |d/dx x sigmoid(x)| = 1.0998
E4M3_MAX = 448.0
# grid: explicit mantissa bits, smallest normal exponent, largest finite value (saturated to it) or None
GRIDS = {"bf16": (7, -126, None), "e4m3": (3, -6, E4M3_MAX)}
FAULTS = ("tap", "kswap", "chan", "toprow", "pad")
FAULT_SITES = {"tap": (2, 2), "kswap": (5, 9), "chan": (3, 4), "toprow": None, "pad": None}  # default sites


def _top_cols(kind, site, tile_w, width):
    """fault "toprow": the input columns whose top pad row is a copy of row 0: all, or those of tile column ``site``."""
    if kind != "toprow":
        return None
    return (0, width) if site is None else (site * tile_w, (site + 1) * tile_w)


def _fault(fault):
    """fault: None, a kind of FAULTS (at its default site) or (kind, site) -> (kind, site)."""
    if fault is None:
        return None, None
    kind, site = (fault, FAULT_SITES[fault]) if isinstance(fault, str) else fault
    assert kind in FAULTS, kind
    return kind, site
TAPS = {"stem_b0": 2, "blocks.1.0": 3, "blocks.1.1": 4, "blocks.1.2": 5, "blocks.2.0": 6, "blocks.2.1": 7,
        "blocks.2.2": 8}


# ------------------------------------------------------------------------------------------------ grids
def _exponent(a: torch.Tensor, emin: int) -> torch.Tensor:
    """floor(log2 a) clamped to emin (emin for a = 0), a >= 0 float64."""
    _, e = torch.frexp(a)  # a = m 2^e, m in [0.5, 1)
    e = torch.where(a > 0, e - 1, torch.full_like(e, emin))
    return torch.clamp(e, min=emin)


def _clamped(x: torch.Tensor, grid: str) -> torch.Tensor:
    top = GRIDS[grid][2]
    return x if top is None else torch.clamp(x, -top, top)  # sat_e4m3 (m2s_common.hpp:194), NaN kept


def spacing(x: torch.Tensor, grid: str) -> torch.Tensor:
    """The grid's spacing in the binade of |x| (subnormal spacing below the smallest normal)."""
    mant, emin, _ = GRIDS[grid]
    x = _clamped(x.double(), grid)
    return torch.ldexp(torch.ones_like(x), _exponent(x.abs(), emin) - mant)


def round_to(x: torch.Tensor, grid: str) -> torch.Tensor:
    """Round to nearest even onto the grid.  bf16: v_cvt_pk_bf16_f32 / f2bf_host (pack.hpp:35-41).  e4m3: finite
    values clamped to +-448 first, then RNE, as sat_e4m3 + v_cvt_pk_fp8_f32 (m2s_common.hpp:192-222) and e4m3_host
    (pack.hpp:68-76) do."""
    x = _clamped(x.double(), grid)
    sp = spacing(x, grid)
    return torch.round(x / sp) * sp  # x / sp is exact (a power of two); torch.round is half-to-even


def boundary_distance(x: torch.Tensor, grid: str) -> torch.Tensor:
    """Distance of x to the nearest rounding boundary (a midpoint of two neighbouring grid values)."""
    mant, emin, _ = GRIDS[grid]
    a = _clamped(x.double(), grid).abs()
    e = _exponent(a, emin)
    sp = torch.ldexp(torch.ones_like(a), e - mant)
    q = a / sp
    d = (q - torch.floor(q) - 0.5).abs() * sp
    # the midpoint just below the binade's first value belongs to the finer binade underneath
    lo = a - torch.ldexp(torch.ones_like(a), e) + sp / 4
    return torch.where(e > emin, torch.minimum(d, lo), d)


# ------------------------------------------------------------------------------------------------ weights
def _f32(sd, key) -> np.ndarray:
    v = sd[key]
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float32)


def fold_bn(sd, p: str) -> Tuple[np.ndarray, np.ndarray]:
    """fold_bn (pack_acoustic.cpp:45-59) in float32 and its operation order: 1.0f / sqrt(v + 1e-3f), * w,
    b - m * a."""
    w, b, m, v = (_f32(sd, p + s) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    invstd = np.float32(1.0) / np.sqrt(v + np.float32(1e-3))
    a = invstd * w
    return a, b - m * a


def stem_weights(sd, prefix: str = "cnn.backbone.") -> Dict[str, np.ndarray]:
    """pack_acoustic.cpp:204-213: the grey repeat folded (sum over the three input channels), then bn1's scale."""
    w = _f32(sd, prefix + "conv_stem.weight")
    a, b = fold_bn(sd, prefix + "bn1")
    return {"W": ((w[:, 0] + w[:, 1] + w[:, 2]) * a[:, None, None])[:, None], "b": b}


def cn_weights(sd, stage: int, idx: int, prefix: str = "cnn.backbone.") -> Dict[str, np.ndarray]:
    """ConvBnAct (pack_acoustic.cpp:222-238): conv weight times bn1's scale, bn1's bias."""
    q = f"{prefix}blocks.{stage}.{idx}."
    a, b = fold_bn(sd, q + "bn1")
    return {"W": _f32(sd, q + "conv.weight") * a[:, None, None, None], "b": b}


def er_weights(sd, stage: int, idx: int, prefix: str = "cnn.backbone.") -> Dict[str, np.ndarray]:
    """EdgeResidual (ErWeights, pack_acoustic.cpp:63-73): conv_exp (mid, cin, 3, 3) * bn1 scale, conv_pwl
    (cout, mid) * bn2 scale, both in float32, and the two folded biases."""
    q = f"{prefix}blocks.{stage}.{idx}."
    a1, b1 = fold_bn(sd, q + "bn1")
    a2, b2 = fold_bn(sd, q + "bn2")
    return {"W1": _f32(sd, q + "conv_exp.weight") * a1[:, None, None, None], "b1": b1,
            "W2": _f32(sd, q + "conv_pwl.weight")[:, :, 0, 0] * a2[:, None], "b2": b2}


def channel_scales(W: np.ndarray) -> np.ndarray:
    """channel_scales (pack.hpp:93-102): amax / 448 per output channel in float32, 1 for an all-zero row."""
    amax = np.abs(W.reshape(W.shape[0], -1)).max(axis=1).astype(np.float32)
    return np.where(amax > 0, amax / np.float32(E4M3_MAX), np.float32(1.0)).astype(np.float32)


def e4m3_weights(W: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
    """emit_e4m3 (pack.hpp:104): e4m3_host(w / s) with the float32 quotient; returns (values, scales) float64."""
    s = channel_scales(W)
    q = (W / s.reshape((-1,) + (1,) * (W.ndim - 1))).astype(np.float32)
    return round_to(torch.from_numpy(q), "e4m3"), torch.from_numpy(s).double()


def bf16_weights(W: np.ndarray) -> torch.Tensor:
    """emit16(Plane::bf16) = f2bf_host (pack.hpp:35-41, 108-113)."""
    return round_to(torch.from_numpy(np.ascontiguousarray(W, np.float32)), "bf16")


def saturated_state(state, factor: float = 4000.0, channels=(0, 63, 127), block: str = "blocks.1.1"):
    """A copy of a state dict in which bn1.weight of three mid channels of ``block`` is scaled by ``factor``, so
    that their e4m3 pre-activation passes 448 (silu_e4m3's clamp, m2s_common.hpp:234)."""
    out = {k: (v.clone() if isinstance(v, torch.Tensor) else np.array(v, copy=True)) for k, v in state.items()}
    w = out[f"cnn.backbone.{block}.bn1.weight"]
    for c in channels:
        w[c] = w[c] * factor
    return out


# ------------------------------------------------------------------------------------------------ arithmetic
def _silu(x, sat: bool):
    return (torch.clamp(x, max=E4M3_MAX) if sat else x) * torch.sigmoid(x)


def _silu_rel(x: torch.Tensor) -> torch.Tensor:
    """Relative error of silu / silu_e4m3 (m2s_common.hpp:229-234): the product x * -log2(e) rounds (2^-24 of the
    argument = |x| 2^-24 relative on e^-x), v_exp_f32 1 ulp; both enter through e / (1 + e) = 1 - sigmoid(x);
    1 + e rounds (2^-24), v_rcp_f32 1 ulp, the final product rounds (2^-24)."""
    return (x.abs() * 2.0 ** -24 + U32) * (1 - torch.sigmoid(x)) + 2.0 ** -24 + U32 + 2.0 ** -24


def same_pads(size: int, stride: int, lead: Optional[int] = None) -> Tuple[int, int]:
    """(leading, trailing) zero pad of a 3-tap axis: TF-SAME for stride 2 (same_pad, pack.hpp:266-274: leading =
    total / 2), 1 / 1 for stride 1; ``lead`` overrides the leading pad (the engine passes pad_t / pad_l)."""
    if stride == 1:
        return 1, 1
    out = -(-size // stride)
    total = max((out - 1) * stride + 3 - size, 0)
    lead = total // 2 if lead is None else lead
    return lead, total - lead


def _conv(x, W, stride, pads, rep_top=None):
    (t, b), (l, r) = pads
    xp = F.pad(x, (l, r, t, b))
    if rep_top is not None and t > 0:  # fault "toprow": the row above the image read as a copy of row 0
        c0, c1 = rep_top
        xp[:, :, :t, l + c0:l + min(c1, x.shape[3])] = x[:, :, :1, c0:c1]
    return F.conv2d(xp, W, None, stride)


class _Ctx:
    """How one evaluation runs: float64 restatement with budgets, or the float32 stand-in."""

    def __init__(self, arith: str, impl: str):
        assert arith in ("bf16", "e4m3", "exact") and impl in ("float64", "float32")
        self.exact = arith == "exact"
        self.f32 = impl == "float32"
        self.dt = torch.float32 if self.f32 else torch.float64
        self.budget = not (self.exact or self.f32)


def _gemm(cx: _Ctx, x, dx, Wq, scale, bias, *, stride=1, pads=((0, 0), (0, 0)), nops=1, prod_rel=0.0, bias_first=False,
          drop_tap=None, rep_top=None):
    """acc = conv(x, Wq); pre = acc * scale + bias.  Returns (pre, err): err bounds the fp32 evaluation's distance
    from pre: (K + nops) fp32 operations on a running magnitude of at most sum|w||x| (+ |bias|), prod_rel *
    sum|w||x| for inexact products, and the flips dx of the input carried through |Wq|."""
    K = Wq.shape[1] * Wq.shape[2] * Wq.shape[3]
    W = Wq.to(cx.dt)
    acc = _conv(x.to(cx.dt), W, stride, pads, rep_top)
    if drop_tap:  # fault "tap": tap (ky, kx) dropped on the last column of every tile of width tw
        tw, ky, kx = drop_tap
        Wt = torch.zeros_like(W)
        Wt[:, :, ky, kx] = W[:, :, ky, kx]
        col = (torch.arange(acc.shape[3]) % tw == tw - 1).to(cx.dt)
        acc = acc - _conv(x.to(cx.dt), Wt, stride, pads, rep_top) * col
    b = bias.to(cx.dt).view(1, -1, 1, 1)
    pre = acc + b if scale is None else acc * scale.to(cx.dt).view(1, -1, 1, 1) + b
    if not cx.budget:
        return pre, None
    sc = 1.0 if scale is None else scale.view(1, -1, 1, 1)
    ab = _conv(x.abs(), Wq.abs(), stride, pads) * sc
    # bias_first: the bias is the accumulator's initial value (stem_b0.hip:253), so it is part of every partial sum
    err = (prod_rel + (K + nops) * U32) * (ab + b.abs() if bias_first else ab) + (0.0 if bias_first else U32 * b.abs())
    if dx is not None:
        err = err + _conv(dx, Wq.abs(), stride, pads) * sc
    return pre, err


def _act_store(cx: _Ctx, pre, err, grid: Optional[str], sat=False):
    """SiLU, then the store onto ``grid``.  Returns (stored, flips, err_m): flips = the distance the device's stored
    value may lie from ours, per element (zero where the pre-rounding value is further from every rounding boundary
    than its accumulated error err_m)."""
    m = _silu(pre, sat)
    if cx.exact:
        return m, None, None
    if cx.f32:
        return round_to(m, grid).float(), None, None
    err_m = SILU_SLOPE * err + _silu_rel(pre) * m.abs()
    sp = spacing(m.abs() + err_m, grid)
    flagged = boundary_distance(m, grid) <= err_m
    flips = torch.where(flagged, torch.where(err_m < sp, sp, sp + err_m), torch.zeros_like(sp))
    return round_to(m, grid), flips, err_m


def _finish(cx: _Ctx, ref, err):
    """The final bf16 store (pack_bf16x2 / f2bf): half a spacing at the value the error can reach, plus the error."""
    if cx.f32:
        return round_to(ref, "bf16")
    if cx.exact:
        return ref, torch.zeros_like(ref)
    return ref, err + spacing(ref.abs() + err, "bf16") / 2


def stored(ref: torch.Tensor) -> torch.Tensor:
    """What a kernel that meets ``ref`` exactly stores: its bf16 rounding."""
    return round_to(ref, "bf16")


# ------------------------------------------------------------------------------------------------ blocks
def edge_residual(x, w, arith: str = "bf16", stride: int = 1, pad_t: Optional[int] = None, pad_l: Optional[int] = None,
                  impl: str = "float64", fault: Optional[str] = None, tile_w: int = 16, return_mid: bool = False):
    """EdgeResidual conv_exp 3x3 (stride) + bn1 + SiLU -> conv_pwl 1x1 + bn2 (+ shortcut at stride 1), x (N, cin, H, W)
    bf16 values, ``w`` from er_weights.  ``pad_t`` / ``pad_l``: the TF-SAME top / left pads the engine passes to the
    stride-2 kernel (default: same_pad's); the bottom / right take the rest.

    arith="bf16": er_fused.hip (blocks.1.1/.2), er2_fused.hip (blocks.2.1/.2), ers2_fused.hip (blocks.1.0, 2.0) and
    the unfused conv_gemm / conv_halo sequence (acoustic_cnn.cpp:163-176, M2S_ER_FUSED=0) round at the same points, so
    there is no switch between them:
      * x: bf16 as stored, not rounded again (er_fused.hip:132, ers2_fused.hip halo DMA);
      * weights: bf16 of the BatchNorm-folded float32 weight (pack.hpp:108-113 through frag_bf16 / frag_bf16_pwl /
        pack_conv, pack.hpp:197-200);
      * conv_exp: fp32 MFMA accumulation over K = 9 cin (er_fused.hip:137, er2_fused.hip, ers2_fused.hip; K-split
        partial sums added in fp32 in conv_gemm_ksum_kernel), + bn1 bias in fp32, fast SiLU in fp32, then the mid
        map rounded to bf16 (er_fused.hip:153-154, er2_fused.hip:182-183, ers2_fused.hip:154-155; unfused: the
        conv's bf16 store, conv_gemm.hip:658-669, 727-728, conv_halo.hip:192-194);
      * conv_pwl: fp32 accumulation over K = mid, + bn2 bias, + the bf16 shortcut in fp32 (er_fused.hip:166-169,
        er2_fused.hip:216, conv_gemm.hip:679-701; none at stride 2, ers2_fused.hip:169-170), one bf16 rounding of
        the output (pack_bf16x2).
    arith="e4m3": er8_fused.hip (blocks.1.1/.2) and er8w_fused.hip (blocks.2.1/.2):
      * x: e4m3 of the stored bf16 input, saturated (er8_fused.hip:206 e4m3x8, or the producer's y8 bytes
        e4m3x4_bf16, er8_fused.hip:308, er8w_fused.hip:328, ers2_fused.hip:172: the same bytes);
      * weights: e4m3 of W / s, s = amax / 448 per output channel (pack_acoustic.cpp:92-110, 132-151; pack.hpp:93-104);
      * conv_exp: fp32 accumulation of exact e4m3 products (unit E8M0 block scales, er8_fused.hip:254), then
        acc * s + bias in fp32 and min(x, 448) * sigmoid(x) (er8_fused.hip:276-277, er8w_fused.hip:296-297), the mid
        map rounded to e4m3 without a second clamp (e4m3x8_nosat, er8_fused.hip:279, er8w_fused.hip:299);
      * conv_pwl: fp32 accumulation over K = mid, o * s + bias + bf16 shortcut in fp32 (er8_fused.hip:300-303,
        er8w_fused.hip:321-324), one bf16 rounding of the output (er8_fused.hip:306, er8w_fused.hip:325).
    fault, a kind or (kind, site): "tap" (tap (ky, kx), default (2, 2), dropped on the last column of every ``tile_w``
    tile), "kswap" (mid channels (a, b), default (5, 9), exchanged in conv_pwl's K order), "chan" (output channel c
    takes channel d's conv_pwl scale (e4m3) or bn2 bias (bf16), default (3, 4)), "toprow" (the row above the image a
    copy of row 0: everywhere, or with site k under tile column k only), "pad" (stride 2: the pad at the top / left instead of TF-SAME's bottom / right)."""
    fault, site = _fault(fault)
    cx = _Ctx(arith, impl)
    x = torch.as_tensor(x).double()
    W1, W2 = w["W1"], w["W2"]
    b1, b2 = torch.from_numpy(w["b1"]).double(), torch.from_numpy(w["b2"]).double()
    s1 = s2 = None
    if arith == "e4m3":
        xq = round_to(x, "e4m3")
        W1q, s1 = e4m3_weights(W1)
        W2q, s2 = e4m3_weights(W2)
    elif arith == "bf16":
        xq, W1q, W2q = x, bf16_weights(W1), bf16_weights(W2)
    else:
        xq, W1q, W2q = x, torch.from_numpy(W1).double(), torch.from_numpy(W2).double()
    if fault == "kswap":
        W2q = W2q.clone()
        W2q[:, list(site)] = W2q[:, list(site)[::-1]]
    if fault == "chan":
        if s2 is not None:
            s2 = s2.clone()
            s2[site[0]] = s2[site[1]]
        else:
            b2 = b2.clone()
            b2[site[0]] = b2[site[1]]
    ph, pw = same_pads(x.shape[2], stride, pad_t), same_pads(x.shape[3], stride, pad_l)
    if fault == "pad":
        ph, pw = ph[::-1], pw[::-1]
    nmul = 1 if s1 is not None else 0  # the epilogue's scale multiply
    pre1, err1 = _gemm(cx, xq, None, W1q, s1, b1, stride=stride, pads=(ph, pw), nops=nmul + 1,
                       drop_tap=(tile_w,) + tuple(site) if fault == "tap" else None,
                       rep_top=_top_cols(fault, site, tile_w * stride, x.shape[3]))
    mid, flips, _ = _act_store(cx, pre1, err1, None if cx.exact else arith, sat=arith == "e4m3")
    skip = stride == 1 and W2.shape[0] == x.shape[1]
    pre2, err2 = _gemm(cx, mid, flips, W2q[:, :, None, None], s2, b2, nops=nmul + 1 + (1 if skip else 0))
    if skip:  # the shortcut is the stored bf16 input, not its e4m3 form
        pre2 = pre2 + x.to(cx.dt)
        if cx.budget:
            err2 = err2 + U32 * (b2.abs().view(1, -1, 1, 1) + x.abs())
    out = _finish(cx, pre2, err2)
    return (out, mid) if return_mid else out


def stem(frames, w, pad_t: Optional[int] = None, pad_l: Optional[int] = None, split: bool = False,
         arith: str = "bf16", impl: str = "float64", fault: Optional[str] = None):
    """conv_stem 3x3 / s2 (TF-SAME) + bn1 + SiLU on the fp32 frames (N, H, W), the grey repeat folded into fp32
    weights (stem_weights).  split=False: stem32_kernel (kernels.hip:68-102): fp32 FMAs from the bias, fast SiLU,
    bf16 store (:98).  split=True: phase 1 of stem_b0.hip (see stem_b0)."""
    cx = _Ctx(arith, impl)
    pre, err = _stem(cx, torch.as_tensor(frames).double()[:, None], w, pad_t, pad_l, split, fault)
    m = _silu(pre, False)
    return _finish(cx, m, SILU_SLOPE * err + _silu_rel(pre) * m.abs() if cx.budget else None)


def _split(v):
    """split4 (m2s_common.hpp:127-134): hi = bf16(v), lo = bf16(v - hi)."""
    hi = round_to(v, "bf16")
    return hi, round_to(v - hi, "bf16")


def _stem(cx, x, w, pad_t, pad_l, split, fault):
    ph, pw = same_pads(x.shape[2], 2, pad_t), same_pads(x.shape[3], 2, pad_l)
    if _fault(fault)[0] == "pad":
        ph, pw = ph[::-1], pw[::-1]
    W, b = torch.from_numpy(w["W"]).double(), torch.from_numpy(w["b"]).double()
    if not split or cx.exact:  # a0 += w * in per tap from the bias (kernels.hip:92-97): a multiply and an add, or one FMA
        return _gemm(cx, x, None, W, None, b, stride=2, pads=(ph, pw), nops=9, bias_first=True)
    # split: frame and weight as bf16 hi + lo (stem_b0.hip:188, 239), the product as the three exact bf16 MFMA terms
    # wl*xh + wh*xl + wh*xh (mma3, stem_b0.hip:71-75; lo*lo is not computed), accumulated in fp32 from the bias the
    # accumulator starts with (stem_b0.hip:253): one GEMM over K = 27 on the concatenated operands
    xh, xl = _split(x)
    wh, wl = _split(W)
    return _gemm(cx, torch.cat([xh, xh, xl], 1), None, torch.cat([wl, wh, wh], 1), None, b, stride=2, pads=(ph, pw),
                 nops=0, bias_first=True)


def conv_bn_act(x, w, arith: str = "bf16", impl: str = "float64", fault: Optional[str] = None, tile_w: int = 16):
    """ConvBnAct 3x3 / s1 + bn1 + SiLU (+ shortcut when cin == cout): blocks.0.0 / blocks.0.1 as the unfused bf16
    engine runs them (conv_halo.hip:192-207 / conv_gemm.hip:658-728): bf16 weights (pack.hpp:197-200), fp32
    accumulation over K = 9 cin, + bias, fast SiLU, + the bf16 shortcut, all in fp32, one bf16 store."""
    cx = _Ctx(arith, impl)
    x = torch.as_tensor(x).double()
    return _finish(cx, *_cba(cx, x, None, w, x if w["W"].shape[0] == x.shape[1] else None, None, fault, tile_w))


def _cba(cx, x, dx, w, skip, dskip, fault, tile_w):
    """SiLU(conv3x3(x) + b) (+ skip) before the store: (value, err)."""
    Wq = torch.from_numpy(w["W"]).double() if cx.exact else bf16_weights(w["W"])
    b = torch.from_numpy(w["b"]).double()
    fault, site = _fault(fault)
    if fault == "kswap":
        Wq = Wq.clone()
        Wq[:, list(site)] = Wq[:, list(site)[::-1]]
    if fault == "chan":
        b = b.clone()
        b[site[0]] = b[site[1]]
    pre, err = _gemm(cx, x, dx, Wq, None, b, pads=((1, 1), (1, 1)),
                     drop_tap=(tile_w,) + tuple(site) if fault == "tap" else None,
                     rep_top=_top_cols(fault, site, tile_w, x.shape[3]))
    m = _silu(pre, False)
    if cx.budget:
        err = SILU_SLOPE * err + _silu_rel(pre) * m.abs()
    if skip is not None:
        m = m + skip.to(cx.dt)
        if cx.budget:
            err = err + U32 * m.abs() + (dskip if dskip is not None else 0.0)
    return m, err


def stem_b0(frames, w_stem, w00, w01, pad_t: Optional[int] = None, pad_l: Optional[int] = None, arith: str = "bf16",
            impl: str = "float64", fault: Optional[str] = None, tile_w: int = 16):
    """conv_stem + blocks.0.0 + blocks.0.1 as stem_b0.hip (the bf16 engine's fused front, SP = 0) computes them,
    frames (N, H, W) fp32 -> (N, 16, OH, OW):
      * phase 1 (stem_b0.hip:237-263): the fp32 frame values and fp32 stem weights each split into bf16 hi + lo, three
        MFMA terms accumulated in fp32 from the bias; fast SiLU; S stored as bf16 (:260-261), exact zeros outside the
        image (:256);
      * phase 2 (:330, 365-371): blocks.0.0 on bf16 weights (pack.hpp:197-200) and S, fp32 accumulation over
        K = 288, + bias, fast SiLU, A stored as bf16, zeros outside the image (:364);
      * phase 3 (:416, 432-441): blocks.0.1 on bf16 weights and A, K = 144, + bias, fast SiLU, + the bf16 shortcut
        read back from A, one bf16 store.
    fault: "pad" on the stem's TF-SAME pad; "toprow", "tap", "kswap" and "chan" on blocks.0.1."""
    kind = _fault(fault)[0]
    cx = _Ctx(arith, impl)
    x = torch.as_tensor(frames).double()[:, None]
    preS, errS = _stem(cx, x, w_stem, pad_t, pad_l, True, "pad" if kind == "pad" else None)
    S, dS, _ = _act_store(cx, preS, errS, None if cx.exact else "bf16")
    Wq = torch.from_numpy(w00["W"]).double() if cx.exact else bf16_weights(w00["W"])
    preA, errA = _gemm(cx, S, dS, Wq, None, torch.from_numpy(w00["b"]).double(), pads=((1, 1), (1, 1)))
    A, dA, _ = _act_store(cx, preA, errA, None if cx.exact else "bf16")
    return _finish(cx, *_cba(cx, A, dA, w01, A, dA, fault if kind != "pad" else None, tile_w))
