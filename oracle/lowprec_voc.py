"""Quantisation-faithful float64 restatements of the bf16 and e4m3 vocoder kernels, stage by stage, with per-element
budgets.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Plain torch / numpy on the CPU, written from this repository's
kernels (csrc/conv_gemm.hip, mrf_fused.hip, gemm128.hip, kernels.hip), its executor (csrc/vocoder.cpp) and its packer
(csrc/pack_vocoder.cpp, pack.hpp), on the helpers and in the scheme of oracle/lowprec.py: every function takes its
input exactly as VocoderEngine.probe returned it (bf16 values, (B, C, L); conv_pre takes the fp32 mel) and returns
``(ref, budget)`` in float64 with the piece's output shape:

  ref     the value the kernel holds in fp32 just before its final store, evaluated in float64 on the kernel's own
          quantised operands (rounded weights, rounded operand images, rounded intermediate tensors);
  budget  a bound on |stored output - ref| for an implementation that rounds where the kernel rounds.

The budget is the same sum of named terms as oracle/lowprec.py's, with no multiplier and no cap on flagged elements:

  output rounding     half a bf16 spacing at |ref| + (the terms below); conv_post stores fp32 and has none.
  fp32 accumulation   (K + the epilogue's operations) * 2^-23 * sum|w||x| per GEMM, and 2^-23 of the bias, residual
                      and running-sum magnitudes for the adds they enter.
  intermediate flips  an element of a stored intermediate tensor (the bf16 tensors T1 / Hb / S, the LDS images A / T,
                      the e4m3 operands X8 / T8 / H8) whose pre-rounding value lies within its accumulated error of a
                      rounding boundary may be stored one grid step away: one spacing there (plus the error where that
                      exceeds the spacing), carried through the next GEMM as sum|w| * spacing over the flagged
                      elements only, through a residual or the running sum as it stands, through LeakyReLU with slope
                      <= 1 and through rb1_fused's recovered residual with its slope 10.
  tanh                conv_post only: tanhf's error taken as 2 ulp of its result (the device library's tanhf, not a
                      hand-written fast form: kernels.hip:277, 309), slope <= 1 on the error of its argument.

LeakyReLU itself is restated bit for bit where its operand is a stored tensor: the kernels form lrelu(x) = x * 0.1f in
fp32 from a bf16 x and round the product again (to bf16 or e4m3), and so does ``_lrelu_image`` in float32.

``arith="exact"`` turns every rounding off (budget zero), which ties the wiring (causal pads, dilations, the
transposed conv's phases, the running sum and its division) to oracle/hifigan.py tap by tap; ``impl="float32"``
evaluates the same quantised operands in float32 with another summation order and rounds as the kernel does, returning
the stored output alone; ``fault=(kind, site)`` seeds one mistake (FAULTS below; tests/test_lowprec_voc_cpu.py).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .lowprec import U32, _Ctx, _f32, bf16_weights, boundary_distance, e4m3_weights, round_to, spacing

SLOPE32 = float(np.float32(0.1))      # 0.1f as the kernels multiply by it
POST_SLOPE32 = float(np.float32(0.01))
TANH_ULPS = 2.0
FAULTS = ("hist", "leak", "tap", "dil", "kswap", "chan", "res10", "accum", "phase")
# MRF kinds: which kernel family the stage runs on, hence where it rounds
KINDS = ("pairs", "fused", "f8", "pairs8")
# rows of one tile of the family's kernel at C <= 64, and whether the tiles count the flat B * L rows or each clip's own
TILES = {"pairs": (256, True), "pairs8": (256, True), "fused": (256, False), "f8": (256, True)}


def tile_rows(kind: str, C: int) -> Tuple[int, bool]:
    """conv_gemm: BM = 128 rows at 128 outputs and more, 256 at 64 and fewer (launch_kind_xf, conv_gemm.hip:922-968);
    rb1_fused: TOUT = 256 rows of one clip (mrf_fused.hip:366-369); conv1d_f8: BM = 64 WM = 256 rows of
    gemm128_kernel<KIND_F8_C1D, 4, 1, NT> at C <= 128, 128 rows of <2, 2, 8> at C = 256 (gemm128.hip:475-482)."""
    rows, flat = TILES[kind]
    if (kind == "f8" and C == 256) or (kind in ("pairs", "pairs8") and C >= 128):
        rows = 128
    return rows, flat


# ------------------------------------------------------------------------------------------------ weights
def fold_wn(sd, p: str) -> np.ndarray:
    """fold_wn (pack_vocoder.cpp:15-34): the plain weight if present, else w = v * (g / (float)sqrt(sum v^2)) per
    slice of dim 0: the sum in double, the quotient and the product in float32."""
    if p + ".weight" in sd:
        return _f32(sd, p + ".weight")
    v = _f32(sd, p + ".weight_v")
    g = _f32(sd, p + ".weight_g").reshape(-1)
    acc = (v.astype(np.float64) ** 2).reshape(v.shape[0], -1).sum(axis=1)
    sc = g / np.sqrt(acc).astype(np.float32)
    return (v * sc.reshape((-1,) + (1,) * (v.ndim - 1))).astype(np.float32)


def voc_weights(sd, h) -> Dict:
    """The generator's folded float32 weights by piece: pre, ups[i], rbs[i][j] (c1 / c2 lists over the pairs; c2 is
    None for ResBlock2), post."""
    nk = len(h["resblock_kernel_sizes"])
    w = {"pre": {"W": _f32(sd, "conv_pre.weight"), "b": _f32(sd, "conv_pre.bias")}, "ups": [], "rbs": [],
         "post": {"W": fold_wn(sd, "conv_post"), "b": _f32(sd, "conv_post.bias")}, "nk": nk}
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        w["ups"].append({"W": fold_wn(sd, f"ups.{i}"), "b": _f32(sd, f"ups.{i}.bias"), "u": int(u), "k": int(k)})
        stage = []
        for j, (rk, rd) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}"
            conv = lambda q: (fold_wn(sd, q), _f32(sd, q + ".bias"))  # noqa: E731
            if str(h["resblock"]) == "1":
                c1 = [conv(f"{p}.convs1.{n}") for n in range(len(rd))]
                c2 = [conv(f"{p}.convs2.{n}") for n in range(len(rd))]
            else:
                c1, c2 = [conv(f"{p}.convs.{n}") for n in range(len(rd))], None
            stage.append({"k": int(rk), "dil": [int(d) for d in rd], "c1": c1, "c2": c2})
        w["rbs"].append(stage)
    return w


def _quant(cx: _Ctx, W: np.ndarray, e4m3: bool):
    """(values float64, per-output-channel scales or None): exact, bf16 (pack_conv / frag_bf16, pack.hpp:108-113,
    197-200) or e4m3 of W / s with s = amax / 448 per output channel (pack_gemm_f8 / channel_scales, pack.hpp:93-104)."""
    if cx.exact:
        return torch.from_numpy(W).double(), None
    if e4m3:
        return e4m3_weights(W)
    return bf16_weights(W), None


# ------------------------------------------------------------------------------------------------ arithmetic
def _shift(x: torch.Tensor, off: int, leak: bool = False) -> torch.Tensor:
    """y[b, :, t] = x[b, :, t + off], zeros outside the clip; leak: the rows outside come from the neighbouring clip
    (the flat (B L) row order the GEMM kernels index), zeros only outside the batch."""
    if off == 0:
        return x
    B, C, L = x.shape
    if leak:
        return _shift(x.permute(1, 0, 2).reshape(1, C, B * L), off).reshape(C, B, L).permute(1, 0, 2)
    y = torch.zeros_like(x)
    if abs(off) < L:
        if off < 0:
            y[:, :, -off:] = x[:, :, :L + off]
        else:
            y[:, :, :L - off] = x[:, :, off:]
    return y


def _rows(B: int, L: int, flat: bool) -> torch.Tensor:
    t = torch.arange(L).view(1, L).expand(B, L)
    return t + torch.arange(B).view(B, 1) * L if flat else t


def _acc(x, Ws: Sequence[torch.Tensor], offs: Sequence[int], leak: bool = False, masks=None) -> torch.Tensor:
    """sum_j Ws[j] (co, ci) applied to the rows t + offs[j]; masks[j] (B, L), if given, zeroes tap j's term per row."""
    out = None
    for j, (W, off) in enumerate(zip(Ws, offs)):
        y = torch.einsum("oc,bcl->bol", W, _shift(x, off, leak))
        if masks is not None and masks[j] is not None:
            y = y * masks[j].to(y.dtype).unsqueeze(1)
        out = y if out is None else out + y
    return out


def _gemm1(cx: _Ctx, x, dx, Ws, offs, scale, bias, nops: int, *, leak=False, masks=None):
    """pre = (sum_j Ws[j] x[t + offs[j]]) * scale + bias and the bound err on the fp32 evaluation's distance from it:
    (K + nops) fp32 operations on a running magnitude of at most sum|w||x|, 2^-23 of the bias, and the flips dx of the
    input carried through |W|."""
    Wd = [W.to(cx.dt) for W in Ws]
    acc = _acc(x.to(cx.dt), Wd, offs, leak, masks)
    b = bias.to(cx.dt).view(1, -1, 1)
    pre = acc + b if scale is None else acc * scale.to(cx.dt).view(1, -1, 1) + b
    if not cx.budget:
        return pre, None
    sc = 1.0 if scale is None else scale.view(1, -1, 1)
    Wa = [W.abs() for W in Ws]
    K = len(Ws) * Ws[0].shape[1]
    err = (K + nops) * U32 * _acc(x.abs(), Wa, offs) * sc + U32 * b.abs()
    if dx is not None:
        err = err + _acc(dx, Wa, offs) * sc
    return pre, err


def _store(cx: _Ctx, m, err, grid: str):
    """An intermediate store onto ``grid``: (stored, flips) as oracle/lowprec.py's _act_store without the SiLU."""
    if cx.exact:
        return m, None
    if cx.f32:
        return round_to(m, grid).float(), None
    if err is None:  # want_budget=False
        return round_to(m, grid), None
    sp = spacing(m.abs() + err, grid)
    flagged = boundary_distance(m, grid) <= err
    flips = torch.where(flagged, torch.where(err < sp, sp, sp + err), torch.zeros_like(sp))
    return round_to(m, grid), flips


def _finish(cx: _Ctx, ref, err):
    if cx.f32:
        return round_to(ref, "bf16")
    if cx.exact:
        return ref, torch.zeros_like(ref)
    if err is None:  # want_budget=False: the value alone
        return ref, None
    return ref, err + spacing(ref.abs() + err, "bf16") / 2


def _lrelu(cx: _Ctx, v, err, slope32: float = SLOPE32, slope: float = 0.1):
    """LeakyReLU of an fp32 value in the epilogue: v * 0.1f rounds once more (2^-24 relative; 2^-23 taken)."""
    if cx.exact:
        return torch.where(v > 0, v, v * slope), None
    m = torch.where(v > 0, v, v * torch.tensor(slope32, dtype=v.dtype))
    return m, (None if err is None else err + U32 * m.abs())


def _lrelu_image(cx: _Ctx, x, dx, grid: str, slope32: float = SLOPE32, slope: float = 0.1):
    """grid(lrelu(x)) of a STORED bf16 tensor, bit for bit: the float32 product x * 0.1f, rounded again onto ``grid``
    (lrelu_frag conv_gemm.hip:28-39; lrelu_pk mrf_fused.hip:62-66, 297-304; lrelu_e4m3_kernel kernels.hip:330-341).
    dx, the stored tensor's own flips, moves the image by at most dx plus one spacing of the image."""
    if cx.exact:
        return torch.where(x > 0, x, x * slope), None
    xf = x.float()
    a = round_to(torch.where(xf > 0, xf, xf * torch.tensor(slope32)), grid)
    a = a.float() if cx.f32 else a
    if dx is None or not cx.budget:
        return a, None
    return a, torch.where(dx > 0, dx + spacing(a.abs() + dx, grid), torch.zeros_like(dx))


def stored(ref: torch.Tensor) -> torch.Tensor:
    """What a kernel that meets ``ref`` exactly stores: its bf16 rounding."""
    return round_to(ref, "bf16")


def _fault(fault):
    if fault is None:
        return None, None
    kind, site = (fault, None) if isinstance(fault, str) else fault
    assert kind in FAULTS, kind
    return kind, site


def _t(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ------------------------------------------------------------------------------------------------ single GEMMs
def conv_pre(mel, w, arith: str = "bf16", impl: str = "float64", fault=None):
    """conv_pre (models.py:113-114: F.pad(x, (0, 6)), Conv1d(num_mels, C0, 7)), mel (B, num_mels, T) fp32 -> tap 0.
      * the mel rounds to bf16 on its way to the channel-last input (mel_to_nlc_kernel, kernels.hip:246-257, act_st);
      * weights: bf16 of the float32 weight, no weight norm (pack_vocoder.cpp:109-119; pack.hpp:197-200); the fp8
        engine packs conv_pre as bf16 too (io_dt, pack_vocoder.cpp:105-107);
      * conv_gemm_kernel<KIND_CONV1D>: fp32 accumulation over K = 7 num_mels, + bias, one bf16 store
        (conv_gemm.hip:639-640, 708-711; split K adds its partial sums in fp32, :730-737).
    fault: "leak" (the 6 rows past a clip's end read the next clip's first rows), "tap" ((tile, j): tap j dropped on
    the last row of every tile), "kswap" ((a, b): two mel bins exchanged in the K order), "chan" ((c, d): channel c
    takes channel d's bias)."""
    cx = _Ctx(arith, impl)
    kind, site = _fault(fault)
    x = torch.as_tensor(mel).double()
    x = x if cx.exact else round_to(x, "bf16")
    Wq, _ = _quant(cx, w["W"], False)
    b = _t(w["b"])
    Wq, b = _operand_faults(kind, site, Wq, b, None)[:2]
    B, _, L = x.shape
    masks = _tap_masks(kind, site, B, L, list(range(7)), 1)
    pre, err = _gemm1(cx, x, None, [Wq[:, :, j] for j in range(7)], list(range(7)), None, b, 1, leak=kind == "leak",
                      masks=masks)
    return _finish(cx, pre, err)


def upsampler(x, w, in_act: bool = False, arith: str = "bf16", impl: str = "float64", fault=None):
    """lrelu(0.1) -> ConvTranspose1d(k, u, padding (k - u) / 2) (models.py:116-117), tap 2i -> tap 2i + 1.
      * operand: bf16(lrelu(x)) formed from the stored bf16 x in the fragments (IN_LRELU, conv_gemm.hip:379-381,
        lrelu_frag :28-39); with ``in_act`` the producer stored lrelu(x) and x is taken as it is (vocoder.cpp:528-531);
      * weights: weight norm folded in float32 (pack_vocoder.cpp:15-34, 132), packed per output phase: tap t of phase
        ph is kernel index (ph + pad) % u + t u and reads input row q + (ph + pad) / u - t for output q u + ph
        (pack_vocoder.cpp:141-146; conv_gemm.hip KIND_CONVT), rounded to bf16 (pack.hpp:197-200);
      * conv_gemm_kernel<KIND_CONVT>: fp32 accumulation over K = ceil(k / u) C_in, + bias, one bf16 store
        (conv_gemm.hip:639-640, 708-711).
    fault: "phase" (at the last input row of every clip output phase r takes phase r + 1's taps), "leak" (rows outside
    a clip read the neighbouring clip), "kswap" ((a, b)), "chan" ((c, d): bias)."""
    cx = _Ctx(arith, impl)
    kind, site = _fault(fault)
    x = torch.as_tensor(x).double()
    a = x.to(cx.dt) if in_act else _lrelu_image(cx, x, None, "bf16")[0]
    u, k = w["u"], w["k"]
    pad, ntap = (k - u) // 2, -(-k // u)
    Wq, _ = _quant(cx, w["W"], False)  # (ci, co, k)
    b = _t(w["b"])
    if kind == "kswap":
        Wq = Wq.clone()
        Wq[list(site)] = Wq[list(site)[::-1]]
    if kind == "chan":
        b = b.clone()
        b[site[0]] = b[site[1]]
    B, _, L = x.shape
    zero = torch.zeros_like(Wq[:, :, 0].t())

    def taps(ph):
        js = [(ph + pad) % u + t * u for t in range(ntap)]
        return [Wq[:, :, j].t() if j < k else zero for j in js], [(ph + pad) // u - t for t in range(ntap)]

    pres, errs = [], []
    for ph in range(u):
        Ws, offs = taps(ph)
        pre, err = _gemm1(cx, a, None, Ws, offs, None, b, 1, leak=kind == "leak")
        if kind == "phase":
            pre = pre.clone()
            pre[:, :, L - 1] = _gemm1(cx, a, None, taps((ph + 1) % u)[0], offs, None, b, 1)[0][:, :, L - 1]
        pres.append(pre)
        errs.append(err)
    pre = torch.stack(pres, dim=3).reshape(B, -1, L * u)
    err = torch.stack(errs, dim=3).reshape(B, -1, L * u) if cx.budget else None
    return _finish(cx, pre, err)


def conv_post(x, w, arith: str = "bf16", impl: str = "float64", fault=None):
    """leaky_relu (slope 0.01) -> F.pad(x, (0, 6)) -> conv_post (Conv1d(C, 1, 7)) -> tanh (models.py:126-130), the last
    tap -> wav (B, 1, L) fp32.  conv_post_kernel / conv_post_tile_kernel (kernels.hip:259-310):
      * operand: the stored bf16 x, lrelu'd in fp32 as 0.01f * v (one fp32 rounding, restated in float32), not rounded
        to bf16;
      * weights: fp32, weight norm folded in float32 (pack_vocoder.cpp:205-211);
      * fp32 accumulation over K = 7 C, tap-major, + bias, tanhf, fp32 store: no output rounding term beyond tanhf's.
    fault: "leak", "tap" ((tile, j)), "kswap" ((a, b))."""
    cx = _Ctx(arith, impl)
    kind, site = _fault(fault)
    x = torch.as_tensor(x).double()
    if cx.exact:
        a = torch.where(x > 0, x, x * 0.01)
    else:
        xf = x.float()
        a = torch.where(xf > 0, xf, torch.tensor(POST_SLOPE32) * xf).to(cx.dt)
    W = _t(w["W"])
    b = _t(w["b"])
    W = _operand_faults(kind, site, W, b, None)[0]
    B, _, L = x.shape
    masks = _tap_masks(kind, site, B, L, list(range(7)), 1)
    pre, err = _gemm1(cx, a, None, [W[:, :, j] for j in range(7)], list(range(7)), None, b, 1, leak=kind == "leak",
                      masks=masks)
    y = torch.tanh(pre)
    if cx.f32:
        return y
    if cx.exact:
        return y, torch.zeros_like(y)
    return y, err + TANH_ULPS * U32 * y.abs()


# ------------------------------------------------------------------------------------------------ the MRF
def _operand_faults(kind, site, Wq, b, s):
    """kswap: input channels (a, b) exchanged in the K order; chan: output channel c takes d's scale (e4m3) or bias."""
    if kind == "kswap":
        Wq = Wq.clone()
        Wq[:, list(site)] = Wq[:, list(site)[::-1]]
    if kind == "chan":
        if s is not None:
            s = s.clone()
            s[site[0]] = s[site[1]]
        else:
            b = b.clone()
            b[site[0]] = b[site[1]]
    return Wq, b, s


def _tap_masks(kind, site, B, L, offs, flat_default):
    """hist, site (tile, which, flat): in tile ``which`` (None: every tile but the first) the rows read zeros instead
    of the rows before the tile's first; tap, site (tile, j[, flat]): tap j dropped on the last row of every tile."""
    if kind == "hist":
        tile, which, flat = site
        r = _rows(B, L, flat)
        start = (r // tile) * tile
        hit = (start > 0) & ((r // tile == which) if which is not None else torch.ones_like(r, dtype=torch.bool))
        return [~(hit & (r + off < start)) for off in offs]
    if kind == "tap":
        tile, j = site[0], site[1]
        flat = site[2] if len(site) > 2 else flat_default
        last = _rows(B, L, flat) % tile == tile - 1
        return [~last if n == j else None for n in range(len(offs))]
    return None


class _Conv:
    """One causal dilated resblock conv on its quantised weights: y[t] = sum_j w[j] x[t - (k - 1) d + j d]
    (get_padding(k, d) on both sides, the output cut to len(x): utils.py:33-34, models.py:43-47)."""

    def __init__(self, cx, Wb, k, e4m3):
        self.cx, self.k = cx, k
        self.Wq, self.s = _quant(cx, Wb[0], e4m3)
        self.b = _t(Wb[1])

    def __call__(self, x, dx, d, nops, fault=(None, None), flat=True):
        kind, site = fault
        Wq, b, s = _operand_faults(kind, site, self.Wq, self.b, self.s)
        k = self.k
        offs = [(j - (k - 1)) * d for j in range(k)]
        B, _, L = x.shape
        masks = _tap_masks(kind, site, B, L, offs, flat)
        return _gemm1(self.cx, x, dx, [Wq[:, :, j] for j in range(k)], offs, s, b, nops + (1 if s is not None else 0),
                      leak=kind == "leak", masks=masks)


def _add(cx, v, e, r, dr):
    """v + r in fp32: the add rounds (2^-23 of the sum) and r's own uncertainty dr enters as it stands."""
    out = v + r.to(cx.dt)
    if not cx.budget:
        return out, None
    return out, e + (dr if dr is not None else 0.0) + U32 * out.abs()


def _resblock(cx, kind, x, rb, fault, at_rb, flat):
    """One resblock up to the fp32 value its last conv holds before the MRF sum: (value, err)."""
    fk, site = fault
    k, dil, np_ = rb["k"], list(rb["dil"]), len(rb["dil"])
    e4 = kind in ("f8", "pairs8") and not cx.exact
    grid = "e4m3" if e4 else "bf16"
    one = rb["c2"] is None  # ResBlock2: x = c(lrelu(x)) + x
    conv_fault = lambda p, c: (fk, site) if (at_rb and fk in ("hist", "leak", "tap", "kswap", "chan") and  # noqa: E731
                                              (p, c) == (0, 0)) else (None, None)
    if at_rb and fk == "dil":
        dil[0] = dil[1 % np_] if np_ > 1 and dil[1 % np_] != dil[0] else dil[0] + 1
    xs, dxs = x.to(cx.dt), None            # the residual as stored (bf16), and its flips
    a, da = _lrelu_image(cx, x, None, grid)  # the c1 operand
    if kind == "pairs8" and not cx.exact:    # conv_gemm SP = 2: e4m3 of the bf16 image (fp8x8, conv_gemm.hip:102-120)
        a = round_to(_lrelu_image(cx, x, None, "bf16")[0], "e4m3")
        a = a.float() if cx.f32 else a
    v = e = None
    for p in range(np_):
        last = p == np_ - 1
        c1 = _Conv(cx, rb["c1"][p], k, e4)
        pre, err = c1(a, da, dil[p], 1, conv_fault(p, 0), flat)
        if not one:
            m, err = _lrelu(cx, pre, err)
            if kind == "pairs8" and not cx.exact:  # T1 is stored as bf16, c2's fragments round it to e4m3
                t, dt_ = _store(cx, m, err, "bf16")
                t8 = round_to(t, "e4m3")
                t8 = t8.float() if cx.f32 else t8
                dt_ = None if dt_ is None else torch.where(dt_ > 0, dt_ + spacing(t8.abs() + dt_, "e4m3"), dt_)
                t = t8
            else:
                t, dt_ = _store(cx, m, err, grid)
            pre, err = _Conv(cx, rb["c2"][p], k, e4)(t, dt_, 1, 2, conv_fault(p, 1), flat)
        if kind == "fused":
            # the residual recovered from the LDS image A = bf16(lrelu(x)): a > 0 ? a : 10 a (mrf_fused.hip:63, 189-201)
            r = a if (at_rb and fk == "res10") else torch.where(a > 0, a, a * 10.0)
            dr = None if da is None else 10.0 * da
            v, e = _add(cx, pre, err, r, dr)
            if not last:
                m, em = _lrelu(cx, v, e)
                a, da = _store(cx, m, em, "bf16")
        else:
            v, e = _add(cx, pre, err, xs, dxs)
            if not last:
                if kind == "f8":  # y = bf16(v) and y8 = e4m3(lrelu(v)), both from the fp32 v (gemm128.hip:366-377)
                    m, em = _lrelu(cx, v, e)
                    a, da = _store(cx, m, em, "e4m3")
                    xs, dxs = _store(cx, v, e, "bf16")
                else:
                    xs, dxs = _store(cx, v, e, "bf16")
                    a, da = _lrelu_image(cx, xs, dxs, "bf16")
                    if kind == "pairs8" and not cx.exact:
                        a8 = round_to(a, "e4m3")
                        a8 = a8.float() if cx.f32 else a8
                        da = None if da is None else torch.where(da > 0, da + spacing(a8.abs() + da, "e4m3"), da)
                        a = a8
    return v, e


def mrf(x, rbs: List[Dict], kind: str = "pairs", arith: str = "bf16", impl: str = "float64", fault=None, at: int = 0,
        want_budget: bool = True):
    """One stage's MRF, tap 2i + 1 -> tap 2i + 2: xs = sum_j resblock_j(x); x = xs / num_kernels (models.py:119-125).
    x (B, C, L) bf16 values as stored, ``rbs`` = voc_weights(...)["rbs"][i].  The sum runs in resblock order through the
    stored bf16 S: S = bf16(y_0); S = bf16(S + y_j); the last S = bf16((S + y) / num_kernels) (mrf_accum,
    vocoder.cpp:259-260; conv_gemm.hip:685-700; mrf_fused.hip:218-235; gemm128.hip:360-366): each is a rounding point.

    kind="pairs": run_conv pairs on conv_gemm_kernel (vocoder.cpp mrf_stage_resblocks, the bf16 engine's C = 256 / 128
      stages and every stage under M2S_MRF_FUSED=0; ResBlock2 runs one conv a pair):
      * c1's operand bf16(lrelu(x)) from the stored bf16 x in the fragments (IN_LRELU, conv_gemm.hip:379-381, 28-39);
      * bf16 weights (pack_vocoder.cpp:160-169; pack.hpp:197-200), fp32 accumulation over K = k C, + bias, lrelu in
        fp32, T1 stored as bf16 (conv_gemm.hip:639-660, 708-711);
      * c2 on T1 as stored, + bias + the stored bf16 x in fp32 (conv_gemm.hip:661-684), Hb stored as bf16: the next
        pair's residual and, lrelu'd to bf16 in the fragments again, its c1 operand;
    kind="fused": rb1_fused_kernel (mrf_fused.hip; bf16, C = 64 / 32): the LDS images A = bf16(lrelu(x)) (:297-304) and
      T = bf16(lrelu(c1 + b1)) (:202-215) are the rounding points, with exact zeros before the clip start (:204); c2
      adds the residual recovered from A as a > 0 ? a : 10 a (:63, 189-201), so a negative residual is 10 bf16(0.1 x),
      and stores A = bf16(lrelu(v)) for the next pair; the last pair's v goes to S (:216-243);
    kind="f8": mrf_stage_f8 (vocoder.cpp:385-421): X8 = e4m3(lrelu(x)), saturated (lrelu_e4m3_kernel,
      kernels.hip:330-341); weights e4m3(W / s), s = amax / 448 per output channel (pack_vocoder.cpp:170-177;
      pack.hpp:93-104); conv1d_f8 = gemm128_kernel<KIND_F8_C1D>: fp32 accumulation of exact e4m3 products,
      fma(acc, s, b) (gemm128.hip:356-358); c1 stores T8 = e4m3(lrelu(v)) only (:371-377); c2 adds the bf16 residual
      and stores both bf16(v) and e4m3(lrelu(v)) from the fp32 v (:357-377);
    kind="pairs8": the fp8 engine's run_conv pairs (M2S_MRF_FUSED=0 at C = 64 / 32): conv_gemm_kernel with SP = 2, the
      weights on the e4m3 grid with per-channel scales (pack.hpp:189-196), the bf16 operand images rounded to e4m3,
      saturated, in the fragments (fp8x8, conv_gemm.hip:102-120, 393), T1 / Hb / S stored as bf16.

    fault=(kind, site), seeded into resblock ``at``'s first c1 unless said otherwise: "hist" ((tile, which, flat)),
    "leak" (the first (k - 1) d rows of clip b > 0 read the previous clip's last rows), "tap" ((tile, j)), "dil" (the
    first pair's c1 runs with the next pair's dilation; d + 1 where there is none), "kswap" ((a, b)), "chan" ((c, d):
    bias, or scale on e4m3), "res10" (fused: every negative residual of the resblock taken as a instead of 10 a),
    "accum" (the middle resblock's share missing from S).  want_budget=False returns (ref, None), at a third of the
    work."""
    assert kind in KINDS, kind
    cx = _Ctx("exact" if arith == "exact" else ("e4m3" if kind in ("f8", "pairs8") else "bf16"), impl)
    cx.budget = cx.budget and want_budget
    fault = _fault(fault)
    x = torch.as_tensor(x).double()
    nk = len(rbs)
    flat = TILES[kind][1]
    S = dS = pre = e = None
    for j, rb in enumerate(rbs):
        v, ev = _resblock(cx, kind, x, rb, fault, j == at, flat)
        if fault[0] == "accum" and j == nk // 2 and 0 < j:
            v, ev = torch.zeros_like(v), (torch.zeros_like(ev) if ev is not None else None)
        if j == 0:
            pre, e = v, ev
        else:
            pre, e = _add(cx, v, ev, S, dS)
            if j == nk - 1:
                pre = pre / nk
                e = e / nk + U32 * pre.abs() if cx.budget else None
        if j < nk - 1:
            S, dS = _store(cx, pre, e, "bf16")
    return _finish(cx, pre, e)


# ------------------------------------------------------------------------------------------------ the generator
def generator(w: Dict, h, mel, kinds: Optional[Sequence[str]] = None, arith: str = "exact", start: int = -1,
              x=None, taps: Optional[list] = None, stop: Optional[int] = None):
    """The pieces chained, each fed what the previous one stores: mel -> wav (B, 1, T hop), or from tap ``start``
    (x = that tap's tensor) on.  arith="exact" restates oracle/hifigan.py; otherwise ``kinds[i]`` names stage i's MRF
    kernel family.  ``taps`` receives every tap computed (tap 0, then 2i + 1 and 2i + 2 per stage); ``stop``: return tap ``stop`` instead
    of running on to the waveform."""
    out = lambda rb: rb[0] if arith == "exact" else stored(rb[0])  # noqa: E731
    n_up = len(w["ups"])
    if start < 0:
        x = out(conv_pre(mel, w["pre"], arith=arith))
        if taps is not None:
            taps.append(x)
        start = 0
    for i in range(n_up):
        if stop is not None and stop <= max(start, 2 * i):
            return x
        if start <= 2 * i:
            x = out(upsampler(x, w["ups"][i], arith=arith))
            if taps is not None:
                taps.append(x)
        if stop is not None and stop <= 2 * i + 1:
            return x
        if start <= 2 * i + 1:
            x = out(mrf(x, w["rbs"][i], kind=kinds[i] if kinds else "pairs", arith=arith, want_budget=False))
            if taps is not None:
                taps.append(x)
    if stop is not None:
        return x
    return conv_post(x, w["post"], arith=arith)[0]
