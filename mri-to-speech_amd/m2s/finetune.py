"""Fine-tuning the BiLSTM and the mel head on the device, encoder frozen (csrc/finetune.cpp, include/m2s.h
"fine-tuning", DESIGN.md "Fine-tuning").

One ``HeadTuner.step`` is one batch of ``OTNLikeTrainer.train_epoch`` (mri2speech_code/train_mri_acoustic_model.py)
with a single micro-batch, restricted to ``rnn.lstm.*`` and ``head.*``: the train-mode windowed BiLSTM, sum merge,
dropout, the head, the ``MaskedMSEMAE`` criterion, exact gradients, ``clip_grad_norm_`` and ``torch.optim.AdamW``,
all in fp32 on cached encoder features (``AcousticEngine.effnet``).  A step downloads nothing; its eight slots come
back as a device tensor.  There is no CPU path.

The dropout mask is the project's own counter-based stream, restated here in numpy (``dropout_keep``): element ``e``
of the (P, window, 640) merged rows at optimiser step ``t`` (counted from 1) is kept iff
``mix(e, seed, t) >= floor(p * 2**32)``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _native as N
from . import ops as _ops
from .metrics import train_weights

KEYS = _ops.FINETUNE_KEYS
SLOTS = _ops.FINETUNE_SLOTS
HIDDEN = 640


def dropout_mix(index, seed: int, step: int) -> np.ndarray:
    """The 32-bit mix of (element index, seed, optimiser step) -> uint32, as ft_mix in csrc/lstm_window_train.hip."""
    e = np.asarray(index, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    lo, hi = e & m32, e >> np.uint64(32)
    x = (lo * np.uint64(0x9E3779B1) + hi * np.uint64(0x27D4EB2F) + np.uint64((int(seed) * 0x85EBCA77) & 0xFFFFFFFF)
         + np.uint64((int(step) * 0xC2B2AE3D) & 0xFFFFFFFF)) & m32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def dropout_keep(shape, p: float, seed: int, step: int) -> np.ndarray:
    """Boolean keep mask of a (P, window, 640) tensor at optimiser step ``step`` (from 1); p = 0 keeps everything."""
    n = int(np.prod(shape))
    thr = int(np.floor(float(p) * 4294967296.0))
    if thr == 0:
        return np.ones(shape, dtype=bool)
    return (dropout_mix(np.arange(n, dtype=np.uint64), seed, step) >= np.uint32(thr)).reshape(shape)


def merge_state_dict(frozen_sd: Dict, tuned: Dict) -> Dict[str, torch.Tensor]:
    """``frozen_sd`` with the 10 tuned tensors of ``tuned`` replaced (every one must be there, nothing else may be):
    the full checkpoint dict the reference's strict ``load_state_dict`` reads.  CPU tensors, copies."""
    if set(tuned) != set(KEYS):
        raise N.M2SError(f"merge_state_dict: expected exactly the keys {KEYS}")
    missing = [k for k in KEYS if k not in frozen_sd]
    if missing:
        raise N.M2SError(f"merge_state_dict: the frozen state dict lacks {missing}")
    out = {k: (v.detach().cpu().clone() if hasattr(v, "detach") else torch.from_numpy(np.array(v)))
           for k, v in frozen_sd.items()}
    for k in KEYS:
        v = tuned[k]
        v = v.detach().cpu().clone() if hasattr(v, "detach") else torch.from_numpy(np.array(v))
        if v.numel() != out[k].numel():
            raise N.M2SError(f"merge_state_dict: {k} has {v.numel()} elements, the checkpoint {out[k].numel()}")
        out[k] = v.reshape(out[k].shape).to(out[k].dtype)
    return out


class HeadTuner:
    """``HeadTuner(state_dict).step(feats, target, mask, lengths)``: see the module docstring.

    ``state_dict``: a full or partial reference checkpoint dict holding ``rnn.lstm.*`` and ``head.*``.  ``window`` is
    the pair length (ref_frames); ``grad_clip <= 0`` turns clipping off."""

    def __init__(self, state_dict: Dict, n_mels: int = 64, device=None, lr: float = 1e-4, weight_decay: float = 1e-4,
                 grad_clip: float = 1.0, dropout: float = 0.5, seed: int = 0, window: int = 4):
        from .runtime import _device
        self.device = _device(device)
        self.n_mels, self.window = int(n_mels), int(window)
        self.lr, self.weight_decay, self.grad_clip = float(lr), float(weight_decay), float(grad_clip)
        self.dropout, self.seed = float(dropout), int(seed)
        L = N.lib()
        self.ops = _ops.load()
        N.check(L.m2s_device_check(self.device.index))
        sd = {k: v for k, v in state_dict.items() if k in KEYS}
        arr, keep = N.tensor_array(sd)
        h = C.c_void_p()
        N.check(L.m2s_finetune_create(arr, len(arr), self.n_mels, self.device.index, C.byref(h)))
        del keep
        self._h = h
        self._destroy = L.m2s_finetune_destroy
        _ops._FINETUNE_MELS[int(h.value)] = self.n_mels
        self._like = torch.empty(1, device=self.device)
        self._ramp: Optional[float] = None
        self._push(1.0)

    def __del__(self):
        h, destroy = getattr(self, "_h", None), getattr(self, "_destroy", None)
        if h is not None and h.value and destroy is not None:
            _ops._FINETUNE_MELS.pop(int(h.value), None)
            destroy(h)
            self._h = None

    @property
    def handle(self) -> int:
        """The m2s_finetune* as the int the torch.ops.m2s.finetune_* ops take."""
        return int(self._h.value)

    def _push(self, ramp: float) -> None:
        """The hyper-parameters and the criterion's weights at ``ramp`` -> the device block, on the current stream."""
        fw, tw, coeffs, _ = train_weights(self.n_mels, self.window, ramp)
        hy = N.FinetuneHyper(self.lr, self.weight_decay, self.grad_clip, self.dropout, self.seed & 0xFFFFFFFF,
                             float(coeffs[0]), float(coeffs[1]), float(coeffs[2]))
        fw = np.ascontiguousarray(fw, np.float32)
        tw = np.ascontiguousarray(tw, np.float32)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            N.check(N.lib().m2s_finetune_set_hyper(self._h, C.byref(hy), fw.ctypes.data_as(C.POINTER(C.c_float)),
                                                   tw.ctypes.data_as(C.POINTER(C.c_float)), self.window,
                                                   C.c_void_p(stream)))
        self._ramp = float(ramp)

    def set_lr(self, lr: float) -> None:
        self.lr = float(lr)
        self._push(self._ramp if self._ramp is not None else 1.0)

    def set_hyper(self, **kw) -> None:
        """Any of lr, weight_decay, grad_clip, dropout, seed."""
        for k, v in kw.items():
            if k not in ("lr", "weight_decay", "grad_clip", "dropout", "seed"):
                raise N.M2SError(f"HeadTuner.set_hyper: unknown hyper-parameter {k!r}")
            setattr(self, k, int(v) if k == "seed" else float(v))
        self._push(self._ramp if self._ramp is not None else 1.0)

    def _args(self, feats, lengths):
        from .runtime import _packed
        if lengths is None and not isinstance(feats, (list, tuple)):
            lengths = [int(feats.shape[0])]
        return _packed(feats, lengths, self.device, 1)

    def step(self, feats, target, mask=None, lengths=None, ramp: float = 1.0) -> torch.Tensor:
        """One optimisation step on packed ``feats`` (rows,208), ``target`` (rows,n_mels), ``mask`` (rows) or None.
        Returns the device tensor of ``SLOTS`` (the losses before the update, the gradient norm, the clip factor);
        nothing is downloaded."""
        x, lengths = self._args(feats, lengths)
        if float(ramp) != self._ramp:
            self._push(float(ramp))
        if not isinstance(target, torch.Tensor) or target.device != self.device:
            raise N.M2SError("HeadTuner.step: target must be on the engine's device; there is no CPU path")
        return self.ops.finetune_step(self.handle, x, target, mask, lengths, self.window)

    def predict(self, feats, lengths=None, train: bool = False) -> torch.Tensor:
        """(P, window, n_mels) predictions of every pair; ``train``: with the dropout mask of the next step."""
        x, lengths = self._args(feats, lengths)
        return self.ops.finetune_forward(self.handle, x, lengths, self.window, bool(train))

    def evaluate(self, feats, target, mask, lengths, metrics):
        """Eval-mode predictions of every pair into ``metrics.update`` (m2s.metrics.MelMetrics); returns ``metrics``."""
        from .metrics import pair_index
        x, lengths = self._args(feats, lengths)
        pred = self.ops.finetune_forward(self.handle, x, lengths, self.window, False)
        idx = pair_index(lengths, self.window, self.device)
        mk = None if mask is None else mask.to(self.device, torch.float32)[idx]
        return metrics.update(pred, target.to(self.device, torch.float32)[idx], mk)

    def grads(self) -> Dict[str, torch.Tensor]:
        """The last step's gradients before clipping, under the reference's key names."""
        return dict(zip(KEYS, self.ops.finetune_grads(self.handle, self._like)))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The 10 tensors under the reference's key names (device tensors, copies)."""
        params, _, _, _ = self.ops.finetune_export(self.handle, self._like)
        return dict(zip(KEYS, params))

    def merged_state_dict(self, frozen_sd: Dict) -> Dict[str, torch.Tensor]:
        """``frozen_sd`` (the checkpoint the tuner started from) with the 10 tuned tensors replaced: the dict the
        reference's strict ``load_state_dict`` and this project's loaders read.  CPU tensors."""
        return merge_state_dict(frozen_sd, self.state_dict())

    def optimizer_state(self) -> Dict:
        """{"m": {key: tensor}, "v": {key: tensor}, "step": device int64 (1,)}; copies."""
        _, m, v, step = self.ops.finetune_export(self.handle, self._like)
        return {"m": dict(zip(KEYS, m)), "v": dict(zip(KEYS, v)), "step": step}

    def load_optimizer_state(self, state: Dict) -> None:
        m = [state["m"][k].to(self.device) for k in KEYS]
        v = [state["v"][k].to(self.device) for k in KEYS]
        step = torch.as_tensor(state["step"], dtype=torch.int64).reshape(1).to(self.device).contiguous()
        self.ops.finetune_import(self.handle, m, v, step)
