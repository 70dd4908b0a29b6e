"""The yardstick of the fine-tuning engine (include/m2s.h "fine-tuning"): one optimisation step of the BiLSTM and the
mel head as torch computes it on the CPU, in float64 (``dtype=torch.float32`` for calibration).

``nn.LSTM`` + sum merge + the dropout mask of the numpy restatement of the mix (``m2s.finetune.dropout_keep``) +
``nn.Linear`` on gathered windows; the criterion as a differentiable restatement of tests/metrics_ref.py's
``train_criterion``; ``clip_grad_norm_``; ``torch.optim.AdamW``.  Nothing here touches the device or the library.
"""
import functools

import numpy as np
import torch

from m2s.finetune import KEYS, dropout_keep
from m2s.metrics import pair_index, train_weights

H, C_IN = 640, 208
LSTM_KEYS = KEYS[:8]


def criterion(pred, target, mask, freq_w, time_w, coeffs):
    """MaskedMSEMAE.forward of the trainer on one batch (B,T,M), differentiable: dict loss, mse, mae, delta, accel,
    latest (tests/metrics_ref.py train_criterion, term by term)."""
    B, T, M = pred.shape
    dt = pred.dtype
    fw = torch.as_tensor(np.asarray(freq_w), dtype=dt)[None, None, :]
    tw = torch.as_tensor(np.asarray(time_w), dtype=dt)[None, :, None]
    mk = torch.ones(B, T, 1, dtype=dt) if mask is None else torch.as_tensor(mask).to(dt)[:, :, None]
    diff = pred - target.to(dt)
    floor = torch.tensor(1e-6, dtype=dt)
    w = fw * tw * mk
    den = torch.maximum(w.sum(), floor)
    zero = torch.zeros((), dtype=dt)
    out = {"mse": (diff ** 2 * w).sum() / den, "mae": (diff.abs() * w).sum() / den, "delta": zero, "accel": zero}
    if T > 1:
        d = diff[:, 1:] - diff[:, :-1]
        wd = fw * tw[:, 1:] * mk[:, 1:] * mk[:, :-1]
        out["delta"] = (d ** 2 * wd).sum() / torch.maximum(wd.sum(), floor)
    if T > 2:
        a = diff[:, 2:] - 2 * diff[:, 1:-1] + diff[:, :-2]
        wa = fw * tw[:, 1:T - 1] * mk[:, 2:] * mk[:, 1:-1] * mk[:, :-2]
        out["accel"] = (a ** 2 * wa).sum() / torch.maximum(wa.sum(), floor)
    lw = fw[:, 0].expand(B, M)
    out["latest"] = (diff[:, -1] ** 2 * lw).sum() / torch.maximum(lw.sum(), floor)
    out["loss"] = out["mse"] + coeffs[0] * out["delta"] + coeffs[1] * out["accel"] + coeffs[2] * out["latest"]
    return out


class RefTuner:
    """The reference step.  ``sd``: the 10 tensors (numpy or torch) under the reference's key names."""

    def __init__(self, sd, n_mels=64, lr=1e-4, weight_decay=1e-4, grad_clip=1.0, dropout=0.5, seed=0, window=4,
                 dtype=torch.float64):
        self.dtype, self.n_mels, self.window = dtype, int(n_mels), int(window)
        self.grad_clip, self.dropout, self.seed = float(grad_clip), float(dropout), int(seed)
        self.lstm = torch.nn.LSTM(C_IN, H, 1, batch_first=True, bidirectional=True).to(dtype)
        self.head = torch.nn.Linear(H, n_mels).to(dtype)
        t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)  # noqa: E731
        self.lstm.load_state_dict({k[len("rnn.lstm."):]: t(sd[k]) for k in LSTM_KEYS})
        self.head.load_state_dict({"weight": t(sd["head.weight"]), "bias": t(sd["head.bias"])})
        self.opt = torch.optim.AdamW(self.params(), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
        self.steps = 0

    def named(self):
        d = {f"rnn.lstm.{k}": p for k, p in self.lstm.named_parameters()}
        d.update({"head.weight": self.head.weight, "head.bias": self.head.bias})
        return {k: d[k] for k in KEYS}

    def params(self):
        return list(self.named().values())

    def merged(self, feats, lengths):
        """Sum-merged BiLSTM rows (P, W, 640) of every window, eval mode."""
        idx = pair_index(lengths, self.window)
        y, _ = self.lstm(torch.as_tensor(feats).to(self.dtype)[idx])
        return y[..., :H] + y[..., H:]

    def predict(self, feats, lengths, train=False):
        y = self.merged(feats, lengths)
        if train and self.dropout > 0:
            keep = dropout_keep(tuple(y.shape), self.dropout, self.seed, self.steps + 1)
            y = y * torch.from_numpy(keep).to(self.dtype) / (1.0 - self.dropout)
        return self.head(y)

    def step(self, feats, target, mask, lengths, ramp=1.0):
        """One step; returns {loss, mse, mae, delta, accel, latest, grad_norm, clip_coef} as floats (before the
        update) and leaves the gradients before clipping in ``self.grads``."""
        idx = pair_index(lengths, self.window)
        fw, tw, coeffs, _ = train_weights(self.n_mels, self.window, ramp)
        self.opt.zero_grad(set_to_none=True)
        pred = self.predict(feats, lengths, train=True)
        tgt = torch.as_tensor(target).to(self.dtype)[idx]
        mk = None if mask is None else torch.as_tensor(mask).to(self.dtype)[idx]
        out = criterion(pred, tgt, mk, fw, tw, coeffs)
        out["loss"].backward()
        self.grads = {k: p.grad.detach().clone() for k, p in self.named().items()}
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in self.grads.values()))
        coef = 1.0
        if self.grad_clip > 0:
            total = torch.nn.utils.clip_grad_norm_(self.params(), self.grad_clip)
            coef = min(1.0, self.grad_clip / (float(total) + 1e-6))
        self.opt.step()
        self.steps += 1
        res = {k: float(v) for k, v in out.items()}
        res["grad_norm"], res["clip_coef"] = float(norm), coef
        return res

    def state(self):
        return {k: p.detach().clone() for k, p in self.named().items()}


def adamw_update(w, g, m, v, step, lr, weight_decay, coef):
    """One AdamW update in float64 numpy on given gradients: returns (w', m', v'); ``step`` counts from 1."""
    w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
    g = g * coef
    w = w * (1.0 - lr * weight_decay)
    m = 0.9 * m + 0.1 * g
    v = 0.999 * v + 0.001 * g * g
    bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
    return w - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + 1e-8), m, v


def inputs(lengths, n_mels, seed, masked="some"):
    """(feats (rows,208), target (rows,n_mels), mask (rows)) fp32 numpy.  masked: "some" = zeros, one 0.5 and the
    rows of one whole window set to 0; "all" = every row 0; "none" = None."""
    rng = np.random.default_rng(seed)
    rows = int(sum(lengths))
    feats = rng.normal(0.0, 0.5, (rows, C_IN)).astype(np.float32)
    target = rng.normal(0.0, 1.0, (rows, n_mels)).astype(np.float32)
    if masked == "none":
        return feats, target, None
    mask = np.ones(rows, np.float32)
    if masked == "all":
        mask[:] = 0.0
    else:
        mask[rng.integers(0, rows, max(1, rows // 8))] = 0.0
        mask[rows // 2] = 0.5
        mask[:min(rows, lengths[0])] = 0.0  # the first clip: at least its first window is fully masked
    return feats, target, mask


@functools.lru_cache(maxsize=None)
def state_of(kind, n_mels=64, seed=0):
    """The 10 tensors (fp32 numpy, read-only: cached) of the synth state or of tests/lstm_hard.py's hard LSTM with the synth head."""
    from m2s import synth
    st = synth.synth_acoustic_state(seed, n_mels=n_mels)
    if kind == "hard":
        import lstm_hard
        hard = lstm_hard.hard_acoustic_state(seed)
        st.update({k: hard[k] for k in LSTM_KEYS})
    else:
        assert kind == "synth", kind
    return {k: np.asarray(st[k], np.float32) for k in KEYS}
