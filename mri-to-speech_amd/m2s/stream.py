"""Streaming acoustic inference over the windowed engine call (include/m2s.h "windowed inference").

The windowed model's prediction for frame t needs the window ending at t and nothing after it, so a stream only
has to remember the last ``window - 1`` FEATURE rows (the CNN's 208-wide output per frame).  ``push`` runs the CNN
on the new frames alone, prepends the remembered rows as ``context`` and gets back rows for exactly the pushed
frames.  No hidden state crosses a call: every chunking of a clip gives the rows of
``AcousticEngine.forward_windowed`` on the whole clip (merge "latest"), bit for bit.
"""
from __future__ import annotations

import torch


class AcousticStream:
    """``engine``: an ``m2s.runtime.AcousticEngine`` (anything with ``effnet(frames) -> (n, F)`` and
    ``bilstm_windowed(feats, lengths, window, merge, context) -> (y, mel_norm)``)."""

    def __init__(self, engine, window: int = 4):
        if not 1 <= int(window) <= 16:
            raise ValueError(f"window = {window} outside 1..16")
        self.engine, self.window = engine, int(window)
        self._tail = None  # the last <= window - 1 feature rows of the stream so far

    def reset(self) -> None:
        """Forget the stream: the next ``push`` starts a new clip."""
        self._tail = None

    @property
    def context(self) -> int:
        """Feature rows held between calls (0 .. window - 1)."""
        return 0 if self._tail is None else int(self._tail.shape[0])

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        """frames (n,[1,]H,W) fp32 in [0, 1] on the engine's device, n >= 1 -> mel_norm (n, n_mels) for exactly
        these frames."""
        if frames.dim() == 4:
            frames = frames[:, 0]
        if frames.dim() != 3 or frames.shape[0] < 1:
            raise ValueError(f"expected (n,[1,]H,W) frames with n >= 1, got {tuple(frames.shape)}")
        feats = self.engine.effnet(frames)
        ctx = self.context
        x = feats if ctx == 0 else torch.cat([self._tail, feats], dim=0)
        _, mel = self.engine.bilstm_windowed(x, [int(x.shape[0])], self.window, "latest", [ctx])
        keep = self.window - 1
        self._tail = x[max(0, int(x.shape[0]) - keep):].clone() if keep > 0 else None
        return mel
