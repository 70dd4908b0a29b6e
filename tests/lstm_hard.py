"""BiLSTM weights on which the recurrence matters, and a float64 reference that can be wrong on purpose
(DESIGN.md §34).

``synth.synth_acoustic_state`` draws every ``rnn.lstm.*`` tensor from uniform(+-1/sqrt(640)), PyTorch's untrained
initialisation: W_hh . h stays below 0.15, every forget gate averages 0.5 and |c| <= 0.46, so an error in the
recurrent path halves each step and a kernel that loses one of the three split product terms passes the suite's
1e-4.  ``hard_acoustic_state`` has what a trained LSTM has (orthogonal W_hh blocks at gain 1, forget bias +2, cell
states in the tens, saturating gates) and still contracts; ``saturating_acoustic_state`` adds units whose
pre-activations leave the range of exp and whose cell state integrates past the range of tanh's exp.

``bilstm_f64`` is the sum-merged BiLSTM as an explicit float64 loop (the wiring of
``oracle.acoustic.bilstm_summerge_loop``), dense or ragged.  Its ``mode`` selects the exact recurrence, an emulation
of what a correct kernel's arithmetic does (``split``, ``act32``), or one of the planted defects of ``MUTATIONS``.
The emulations and defects describe arithmetic; none of them is the code under test.

Helper module, not a conftest; imported by test_lstm_hard_cpu.py, test_gpu_lstm_hard.py and the gradcam tests.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from m2s import synth
from oracle import acoustic

H = 640
C_IN = 208
FORGET_BIAS = 2.0   # at +3 (or W_hh gain 1.5) the recurrence stops contracting over 1000 steps: fp32 alone drifts
W_HH_GAIN = 1.0     # 3e-5 .. 8e-5 from float64 and a correct split 1e-3; such weights measure chaos, not kernels
LOG2E = 1.4426950408889634

ARITHMETIC = ("exact", "split", "act32")
MUTATIONS = ("no_wlo", "no_hlo", "stale", "gate_swap", "rev_shift")
SPLIT_ONLY = ("no_wlo", "no_hlo")  # defects of the three-term product: they do not exist in the fp32 engine
STALE_EVERY, STALE_UNITS = 7, 32

# the suite's bars, as test_gpu_parity.py / test_gpu_windowed.py state them (atol on y; the head gets 5x)
BAR_SPLIT = 1e-4
BAR_WINDOW4 = 2e-5


def bar(engine: str, T: int, window: bool = False) -> float:
    """atol on y of an engine class ("fp32" or "split") at sequence length T; window: the window-4 kernels."""
    assert engine in ("fp32", "split")
    if window:
        return BAR_WINDOW4
    if engine == "split":
        return BAR_SPLIT
    return 2e-5 if T <= 64 else 1e-4


# ---------------------------------------------------------------------------------------------------- weights
def _orthogonal(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))  # the sign fix makes q Haar-distributed and independent of LAPACK's convention


def _hard_lstm(seed: int):
    rng = np.random.default_rng([seed, 0x15D])
    out = {}
    for sfx in ("", "_reverse"):
        out[f"rnn.lstm.weight_hh_l0{sfx}"] = W_HH_GAIN * np.concatenate([_orthogonal(rng, H) for _ in range(4)])
        out[f"rnn.lstm.weight_ih_l0{sfx}"] = rng.normal(0.0, 1.0 / math.sqrt(C_IN), size=(4 * H, C_IN))
        b = rng.normal(0.0, 0.5, size=4 * H)
        b[H:2 * H] += FORGET_BIAS
        out[f"rnn.lstm.bias_ih_l0{sfx}"] = b
    return {k: v.astype(np.float32) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _hard_cached(seed: int):
    st = synth.synth_acoustic_state(seed)
    st.update(_hard_lstm(seed))  # bias_hh and the head stay synth's
    return st


def hard_acoustic_state(seed: int = 0):
    """``synth.synth_acoustic_state(seed)`` with, per direction, W_hh = four independent random orthogonal 640 x 640
    blocks (QR of a normal matrix) at gain 1, W_ih ~ N(0, 1/sqrt(208)), bias_ih ~ N(0, 0.5) + 2 on the forget slice,
    all float32.  Deterministic in ``seed``; returns a fresh dict of fresh arrays."""
    return {k: np.array(v, copy=True) for k, v in _hard_cached(seed).items()}


# unit groups of the saturating state (the same in both directions); everything from SAT_FREE on is the hard state's
SAT_UP = slice(0, 32)        # i = f = 1, g = +1: c grows by one a step
SAT_DOWN = slice(32, 64)     # i = f = 1, g = -1: c falls by one a step
SAT_OPEN = slice(64, 80)     # every gate's bias +100: sigmoid = 1 and tanh = 1 through exp -> 0
SAT_SHUT = slice(80, 96)     # every gate's bias -100: sigmoid = 0 and tanh = -1 through exp -> inf
SAT_SWING_UP = slice(96, 112)     # W_ih rows x 20 (pre-activation std 10) around a bias of +75: 45 .. 105
SAT_SWING_DOWN = slice(112, 128)  # the same around -75
SAT_FREE = 128
SAT_BIAS, SAT_HUGE, SAT_SWING_BIAS, SAT_IH_SCALE = 20.0, 100.0, 75.0, 20.0


def saturating_acoustic_state(seed: int = 0):
    """The hard state with 128 units per direction driven out of exp's range: see the SAT_* groups.  The integrating
    units reach |c| = T (2c passes 88.7, where exp2 in tanh(c) overflows, after 45 steps); the reference's sigmoid
    and tanh give exactly 0, 1 and +-1 there, and the kernels must reach the same through exp2 -> inf and
    rcp(inf) = 0 without a NaN."""
    st = hard_acoustic_state(seed)
    for sfx in ("", "_reverse"):
        b = st[f"rnn.lstm.bias_ih_l0{sfx}"].reshape(4, H)
        w = st[f"rnn.lstm.weight_ih_l0{sfx}"].reshape(4, H, C_IN)
        for grp, g_sign in ((SAT_UP, 1.0), (SAT_DOWN, -1.0)):
            b[0, grp] = SAT_BIAS
            b[1, grp] = SAT_BIAS
            b[2, grp] = g_sign * SAT_BIAS
        b[:, SAT_OPEN] = SAT_HUGE
        b[:, SAT_SHUT] = -SAT_HUGE
        for grp, sign in ((SAT_SWING_UP, 1.0), (SAT_SWING_DOWN, -1.0)):
            b[:, grp] = sign * SAT_SWING_BIAS
            w[:, grp] *= SAT_IH_SCALE
    return st


# -------------------------------------------------------------------------------------------------- reference
def _t64(a):
    return torch.as_tensor(np.asarray(a)).to(torch.float64)


def _bf16(a):
    """float64 -> nearest bf16, back in float64 (through fp32: the kernels split fp32 values)."""
    return a.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _split(a):
    hi = _bf16(a)
    return hi, _bf16(a.to(torch.float32).to(torch.float64) - hi)


def _sig32(x):
    return 1.0 / (1.0 + torch.exp2(x * -LOG2E))


def _activate(g, c, mode, first):
    """(B, 4H) pre-activations and the cell state -> (gates (B, 4H), c', h'), in float64 or the kernels' fp32 form."""
    if mode == "act32":
        g, c = g.to(torch.float32), c.to(torch.float32)
        i, f, gg, o = g.chunk(4, dim=1)
        i, f, o = _sig32(i), _sig32(f), _sig32(o)
        gg = 2.0 * _sig32(2.0 * gg) - 1.0
        ig = i * gg            # two rounded products and a rounded sum: no fma (lstm_cell.hpp lstm_cell)
        c = ig if first else f * c + ig
        h = o * (2.0 * _sig32(2.0 * c) - 1.0)
        return torch.cat([i, f, gg, o], 1).double(), c.double(), h.double()
    i, f, gg, o = g.chunk(4, dim=1)
    i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    c = f * c + i * gg
    return torch.cat([i, f, gg, o], 1), c, o * torch.tanh(c)


def bilstm_f64(sd, x, lengths=None, mode: str = "exact", state: bool = False, prefix: str = "rnn.lstm."):
    """Sum-merged BiLSTM in float64.  ``x`` (B, T, 208); ``lengths`` (B ints <= T): clip b is x[b, :lengths[b]], its
    reverse direction starts at its own last frame, rows past its length come out zero (and are never read).

    mode: "exact"; "split" (W_hh and h each hi + lo, both halves rounded to bf16, product hi.hi + hi.lo + lo.hi);
    "act32" (gates through fp32 1 / (1 + exp2(-x log2 e)) and 2 sig(2x) - 1, cell update in fp32 without fma);
    or a defect: "no_wlo" / "no_hlo" (split without W_lo.h_hi / W_hi.h_lo), "stale" (at every 7th step the gate
    rows of units 0..31 read h from one step earlier), "gate_swap" (the f and g rows of W_hh exchanged),
    "rev_shift" (the reverse direction starts at the padded end T - 1 over zero input rows, not at len - 1).

    Returns y (B, T, 640) float64; with ``state`` also a dict of "h", "c" (2, B, T, 640), "gates" (2, B, T, 2560:
    i, f, g, o after their activations) and "pre" (the same before them)."""
    assert mode in ARITHMETIC + MUTATIONS, mode
    x = _t64(x)
    B, T, _ = x.shape
    lens = torch.as_tensor([T] * B if lengths is None else list(lengths), dtype=torch.long)
    assert lens.shape == (B,) and int(lens.min()) >= 1 and int(lens.max()) <= T
    valid_t = torch.arange(T)[None, :] < lens[:, None]
    x = x * valid_t[..., None]
    rows = torch.arange(B)
    split = mode in ("split",) + SPLIT_ONLY
    hs, cs, gs, ps = [], [], [], []
    for d, params in enumerate(acoustic.lstm_params(sd, prefix)):
        w_ih, w_hh, b_ih, b_hh = (_t64(p) for p in params)
        if mode == "gate_swap":
            w_hh = torch.cat([w_hh[:H], w_hh[2 * H:3 * H], w_hh[H:2 * H], w_hh[3 * H:]])
        w_hi, w_lo = _split(w_hh) if split else (w_hh, None)
        pre = x @ w_ih.t() + (b_ih + b_hh)
        h, c, h_old = x.new_zeros(B, H), x.new_zeros(B, H), x.new_zeros(B, H)
        hd, cd, gd, pd = x.new_zeros(B, T, H), x.new_zeros(B, T, H), x.new_zeros(B, T, 4 * H), x.new_zeros(B, T, 4 * H)
        for s in range(T):
            if d == 0:
                t, on = torch.full((B,), s), s < lens
            elif mode == "rev_shift":
                t, on = torch.full((B,), T - 1 - s), torch.ones(B, dtype=torch.bool)
            else:
                t, on = (lens - 1 - s).clamp(min=0), s < lens
            if split:
                h_hi, h_lo = _split(h)
                rec = h_hi @ w_hi.t()
                if mode != "no_hlo":
                    rec = rec + h_lo @ w_hi.t()
                if mode != "no_wlo":
                    rec = rec + h_hi @ w_lo.t()
            else:
                rec = h @ w_hi.t()
                if mode == "stale" and s >= 2 and s % STALE_EVERY == 0:
                    late = (h_old @ w_hi.t()).view(B, 4, H)
                    rec = rec.view(B, 4, H).clone()
                    rec[:, :, :STALE_UNITS] = late[:, :, :STALE_UNITS]
                    rec = rec.view(B, 4 * H)
            g_in = pre[rows, t] + rec
            gates, c_new, h_new = _activate(g_in, c, mode, s == 0)
            keep = on[:, None]
            h_old = torch.where(keep, h, h_old)
            h, c = torch.where(keep, h_new, h), torch.where(keep, c_new, c)
            sel = rows[on], t[on]
            hd[sel], cd[sel], gd[sel], pd[sel] = h_new[on], c_new[on], gates[on], g_in[on]
        hs.append(hd)
        cs.append(cd)
        gs.append(gd)
        ps.append(pd)
    y = (hs[0] + hs[1]) * valid_t[..., None]
    if state:
        return y, {"h": torch.stack(hs), "c": torch.stack(cs), "gates": torch.stack(gs), "pre": torch.stack(ps)}
    return y


def head_f64(sd, y):
    return acoustic.head({k: _t64(sd[k]) for k in ("head.weight", "head.bias")}, _t64(y))


def err(sd, x, mode, ref=None, lengths=None):
    """max |y(mode) - y(exact)| over the valid rows."""
    ref = bilstm_f64(sd, x, lengths) if ref is None else ref
    return float((bilstm_f64(sd, x, lengths, mode) - ref).abs().max())


# ------------------------------------------------------------------------------------- windows and pairs
def _run_windows(sd, wins, mode):
    """A list of (k, 208) windows (k may differ) -> the list of their (k, 640) float64 outputs, each window from
    zero state, all in one ragged call."""
    lens = [int(w.shape[0]) for w in wins]
    x = torch.zeros(len(wins), max(lens), C_IN, dtype=torch.float64)
    for b, w in enumerate(wins):
        x[b, :lens[b]] = _t64(w)
    y = bilstm_f64(sd, x, lens, mode)
    return [y[b, :n] for b, n in enumerate(lens)]


def windowed_f64(sd, clips, W, merge="latest", context=None, mode="exact"):
    """tests/windowed_ref.py's three definitions on ``bilstm_f64``: packed (y (R, 640), mel_norm (R, 64)) float64 of
    a list of (len_b, 208) clips, in clip order.  Under ``mean`` the head is applied per window and averaged, as
    there."""
    context = [0] * len(clips) if context is None else list(context)
    assert merge in ("latest", "mean") and (merge == "latest" or not any(context))
    ys, ms = [], []
    for xc, ctx in zip(clips, context):
        n = int(xc.shape[0])
        if merge == "latest":
            out = _run_windows(sd, [xc[max(0, t - W + 1):t + 1] for t in range(ctx, n)], mode)
            y = torch.stack([o[-1] for o in out])
            m = head_f64(sd, y)
        elif n <= W:
            (y,) = _run_windows(sd, [xc], mode)
            m = head_f64(sd, y)
        else:
            out = _run_windows(sd, [xc[w:w + W] for w in range(n - W + 1)], mode)
            acc_y = [[] for _ in range(n)]
            acc_m = [[] for _ in range(n)]
            for w, o in enumerate(out):
                mo = head_f64(sd, o)
                for s in range(W):
                    acc_y[w + s].append(o[s])
                    acc_m[w + s].append(mo[s])
            y = torch.stack([torch.stack(v).mean(0) for v in acc_y])
            m = torch.stack([torch.stack(v).mean(0) for v in acc_m])
        ys.append(y)
        ms.append(m)
    return torch.cat(ys), torch.cat(ms)


def pairs_f64(sd, clips, W, mode="exact"):
    """(y (P, W, 640), mel_norm (P, W, 64)) float64: every window of W consecutive rows of every clip, all rows
    kept, clips in order, windows ascending.  Every clip needs at least W rows."""
    assert all(int(c.shape[0]) >= W for c in clips)
    y = torch.stack(_run_windows(sd, [c[i:i + W] for c in clips for i in range(int(c.shape[0]) - W + 1)], mode))
    return y, head_f64(sd, y)


# ------------------------------------------------------------------------------------------------- inputs
# The weights of every hard test; fixed before any kernel ran on them.  Part of the tests' definition: over 1000 steps
# the emulated correct split's worst element at 17 sequences is 4.7e-5 .. 8.8e-5 for seeds 0-5 and 11 but 1.5e-4 for
# seed 7, over the split engines' bar.
SEED = 11
RAGGED_LENS, RAGGED_SEED = [40, 7, 1], 71
WINDOW_LENS, WINDOW_SEED = [1, 3, 4, 9], 72   # a one-frame clip, a partial window, exactly one window, six windows
WINDOW_CONTEXT = [0, 2, 3, 2]                  # history rows of the context case (latest only, < window and < len)


def feats(B: int, T: int, seed=None) -> torch.Tensor:
    """x ~ N(0, 0.5), (B, T, 208) fp32, as the suite's BiLSTM tests draw it."""
    rng = np.random.default_rng(1000 * B + T if seed is None else seed)
    return torch.from_numpy(rng.normal(0.0, 0.5, (B, T, C_IN)).astype(np.float32))


def clip_feats(lens, seed: int):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.normal(0.0, 0.5, (n, C_IN)).astype(np.float32)) for n in lens]


def torch_state(st):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}


@functools.lru_cache(maxsize=None)
def reference(kind: str, B: int, T: int):
    """(x fp32 (B, T, 208), y float64 numpy, mel_norm float64 numpy) of ``feats(B, T)`` under the "hard" or "sat"
    state of SEED.  Computed once per process, read-only."""
    st = torch_state(hard_acoustic_state(SEED) if kind == "hard" else saturating_acoustic_state(SEED))
    x = feats(B, T)
    y = bilstm_f64(st, x)
    out = (y.numpy(), head_f64(st, y).numpy())
    for a in out:
        a.flags.writeable = False
    return (x,) + out


# ----------------------------------------------------------------------------------- training-mode reference
TRAIN_SHAPES = [(1, 9), (3, 5), (1, 40)]
LSTM_NAMES = [f"rnn.lstm.{n}_l0{s}" for s in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def state_of(kind: str):
    """The "hard" or "sat" state of SEED as torch tensors."""
    return torch_state({"hard": hard_acoustic_state, "sat": saturating_acoustic_state}[kind](SEED))


def train_inputs(B: int, T: int):
    """(x (B, T, 208), cotangent of y (B, T, 640)) as test_bilstm_autograd_matches_torch draws them."""
    g = torch.Generator().manual_seed(B * 100 + T)
    return torch.randn(B, T, C_IN, generator=g), torch.randn(B, T, H, generator=g)


def lstm_autograd(sd, x, dy, dtype=torch.float64):
    """torch's nn.LSTM + sum merge on the CPU in ``dtype`` with autograd: {"y", "dx", and every nn.LSTM parameter's
    gradient by its name} for the cotangent(s) ``dy`` ((B, T, 640), or (K, B, T, 640): then "dx" is (K, B, T, 208)
    and the weight gradients are left out)."""
    lstm = torch.nn.LSTM(C_IN, H, 1, batch_first=True, bidirectional=True).to(dtype)
    lstm.load_state_dict({k[len("rnn.lstm."):]: v.to(dtype) for k, v in sd.items() if k.startswith("rnn.lstm.")})
    xr = x.to(dtype).clone().requires_grad_(True)
    y = lstm(xr)[0]
    y = y[..., :H] + y[..., H:]
    if dy.dim() == 4:
        dx = torch.stack([torch.autograd.grad(y, xr, d.to(dtype), retain_graph=True)[0] for d in dy])
        return {"y": y.detach(), "dx": dx}
    (y * dy.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": xr.grad, **{n: p.grad for n, p in lstm.named_parameters()}}


def rel(a, b) -> float:
    """max |a - b| relative to the largest element of b, in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
