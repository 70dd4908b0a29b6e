"""Streaming inference: frames in, mel rows and audio out while the clip is still arriving.

* ``AcousticStream``  frames -> the mel rows of exactly those frames (the windowed engine call); uint8 frames at the
                      scanner's size are resized and normalised on the device first (csrc/frames.hip)
* ``VocoderStream``   mel rows -> the audio of the rows that have become final (the chunk call)
* ``push_all``        several ``VocoderStream``s through one engine call
* ``SpeechStream``    the two chained through the mel glue: frames -> mel rows of the pushed frames + audio

Acoustic side (include/m2s.h "windowed inference").

The windowed model's prediction for frame t needs the window ending at t and nothing after it, so a stream only
has to remember the last ``window - 1`` FEATURE rows (the CNN's 208-wide output per frame).  ``push`` runs the CNN
on the new frames alone, prepends the remembered rows as ``context`` and gets back rows for exactly the pushed
frames.  No hidden state crosses a call: every chunking of a clip gives the rows of
``AcousticEngine.forward_windowed`` on the whole clip (merge "latest"), bit for bit.

Vocoder side (include/m2s.h "streaming vocoder").  Output frame o of the generator depends on mel rows
o - back .. o + ahead only (``VocoderEngine.reach``; (16, 7) for the shipped config).  A row is FINAL once its
``ahead`` successors are present, so a stream emits with a latency of ``ahead`` rows (7 x 420 / 11413 s = 258 ms
for the shipped config: a property of the model, not of the implementation) and remembers the last
``back + ahead`` mel rows.  Nothing else crosses a call, and the concatenation of everything a stream returns is the
whole clip's waveform for every chunking.
"""
from __future__ import annotations

import torch


class AcousticStream:
    """``engine``: an ``m2s.runtime.AcousticEngine`` (anything with ``effnet(frames) -> (n, F)`` and
    ``bilstm_windowed(feats, lengths, window, merge, context) -> (y, mel_norm)``)."""

    def __init__(self, engine, window: int = 4, size=(256, 256), interp: str = "linear", norm: str = "zscore"):
        if not 1 <= int(window) <= 16:
            raise ValueError(f"window = {window} outside 1..16")
        self.engine, self.window = engine, int(window)
        self.size, self.interp, self.norm = (int(size[0]), int(size[1])), interp, norm  # the uint8 front end
        self._tail = None  # the last <= window - 1 feature rows of the stream so far

    def reset(self) -> None:
        """Forget the stream: the next ``push`` starts a new clip."""
        self._tail = None

    @property
    def context(self) -> int:
        """Feature rows held between calls (0 .. window - 1)."""
        return 0 if self._tail is None else int(self._tail.shape[0])

    def push(self, frames: torch.Tensor, masks=None) -> torch.Tensor:
        """frames (n,[1,]H,W) fp32 in [0, 1] on the engine's device, n >= 1 -> mel_norm (n, n_mels) for exactly
        these frames.  uint8 frames, (n,h,w) grey or (n,h,w,3) BGR at the scanner's size, go through the device
        front end first (``runtime.preprocess_frames`` to the ``size`` (H, W) / ``interp`` / ``norm`` given at
        construction).  ``masks``: one (h,w) articulator mask (``m2s.occlusion``) applied to the uint8 frames on
        the way (``runtime.preprocess_frames_masked``): the stream of the host-masked frames, bit for bit."""
        if masks is not None:
            from .runtime import preprocess_frames_masked
            if frames.dtype != torch.uint8:
                raise ValueError("masks apply to uint8 frames at the scanner's size")
            mk = torch.as_tensor(masks, dtype=torch.float32)
            if mk.dim() == 3 and mk.shape[0] == 1:
                mk = mk[0]
            if mk.dim() != 2:
                raise ValueError(f"a stream takes one (h,w) mask, got {tuple(mk.shape)}")
            frames = preprocess_frames_masked(frames, mk, self.size, self.interp, self.norm)[0]
        elif frames.dtype == torch.uint8:
            from .runtime import preprocess_frames
            frames = preprocess_frames(frames, self.size, self.interp, self.norm)
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


class VocoderStream:
    """``engine``: an ``m2s.runtime.VocoderEngine`` (anything with ``reach -> (back, ahead)``, ``hop`` and
    ``forward_chunk(mel, lengths, context, hold) -> packed wav``)."""

    def __init__(self, engine):
        self.engine = engine
        self.back, self.ahead = (int(v) for v in engine.reach)
        self.hop = int(engine.hop)
        self.reset()

    def reset(self) -> None:
        """Forget the stream: the next ``push`` starts a new clip."""
        self._rows = None  # the last <= back + ahead mel rows: rows _seen - len(_rows) .. _seen - 1 of the clip
        self._seen = 0     # rows pushed so far
        self._done = 0     # rows whose audio has been returned

    @property
    def pending(self) -> int:
        """Rows pushed whose audio is still to come (0 .. ahead)."""
        return self._seen - self._done

    def _empty(self, like) -> torch.Tensor:
        return torch.empty(0, dtype=torch.float32, device=like.device)

    def _stage(self, mel_rows: torch.Tensor, last: bool = False):
        """The span the next call needs for this stream, (x, context, hold, k); k = rows it makes final."""
        if mel_rows is not None:
            if mel_rows.dim() != 2 or mel_rows.shape[0] < 1:
                raise ValueError(f"expected (n, num_mels) mel rows with n >= 1, got {tuple(mel_rows.shape)}")
            x = mel_rows if self._rows is None else torch.cat([self._rows, mel_rows], dim=0)
        else:
            x = self._rows
        seen = self._seen + (0 if mel_rows is None else int(mel_rows.shape[0]))
        final = seen if last else max(self._done, seen - self.ahead)
        first = seen - (0 if x is None else int(x.shape[0]))  # clip row of x[0]
        return x, self._done - first, seen - final, final - self._done

    def _commit(self, x: torch.Tensor, k: int, n_new: int) -> None:
        first = self._seen + n_new - int(x.shape[0])
        self._seen += n_new
        self._done += k
        keep_from = max(0, self._done - self.back)  # a later row reaches back to here at most
        self._rows = x[keep_from - first:].clone() if keep_from > first else x

    def push(self, mel_rows: torch.Tensor) -> torch.Tensor:
        """mel_rows (n, num_mels) ln-mel on the engine's device, n >= 1 -> the k * hop samples of the k rows that
        became final (empty while fewer than ahead + 1 rows exist)."""
        x, ctx, hold, k = self._stage(mel_rows)
        wav = self.engine.forward_chunk(x, [int(x.shape[0])], [ctx], [hold]) if k > 0 else self._empty(x)
        self._commit(x, k, int(mel_rows.shape[0]))
        return wav

    def flush(self) -> torch.Tensor:
        """The clip has ended: the audio of the remaining <= ahead rows, computed with the clip's true end; then
        ``reset``."""
        x, ctx, hold, k = self._stage(None, last=True)
        if k > 0:
            wav = self.engine.forward_chunk(x, [int(x.shape[0])], [ctx], [0])
        else:
            wav = torch.empty(0, dtype=torch.float32) if x is None else self._empty(x)
        self.reset()
        return wav


def push_all(streams, chunks):
    """``streams[i].push(chunks[i])`` for several ``VocoderStream``s of ONE engine through one ``forward_chunk``
    call; the streams may be at different phases.  Streams with nothing to emit yet are left out of the call.
    Returns the list of per-stream waveforms."""
    if len(streams) != len(chunks) or not streams:
        raise ValueError("one chunk per stream, at least one stream")
    engine = streams[0].engine
    if any(st.engine is not engine for st in streams):
        raise ValueError("push_all: the streams must share one engine")
    staged = [st._stage(c) for st, c in zip(streams, chunks)]
    live = [i for i, (_, _, _, k) in enumerate(staged) if k > 0]
    out = [st._empty(staged[i][0]) for i, st in enumerate(streams)]
    if live:
        wav = engine.forward_chunk([staged[i][0] for i in live], None, [staged[i][1] for i in live],
                                   [staged[i][2] for i in live])
        for i, w in zip(live, torch.split(wav, [staged[i][3] * streams[i].hop for i in live])):
            out[i] = w
    for st, c, (x, _, _, k) in zip(streams, chunks, staged):
        st._commit(x, k, int(c.shape[0]))
    return out


class SpeechStream:
    """frames -> mel rows and audio, all on the device: ``AcousticStream.push``, the mel glue, ``VocoderStream.push``.
    ``pipeline``: an ``m2s.runtime.Pipeline``.  The acoustic side is the windowed model (the whole-clip BiLSTM cannot
    stream), so a clip streamed in any chunking gives ``Pipeline.forward_windowed``'s mel rows bit for bit and its
    waveform to rounding."""

    def __init__(self, pipeline, window: int = 4, size=(256, 256), interp: str = "linear", norm: str = "zscore"):
        self.pipeline = pipeline
        self.acoustic = AcousticStream(pipeline.ac, window, size, interp, norm)
        self.vocoder = VocoderStream(pipeline.voc)

    def reset(self) -> None:
        self.acoustic.reset()
        self.vocoder.reset()

    def push(self, frames: torch.Tensor, masks=None):
        """frames (n,[1,]H,W) fp32, or uint8 (n,h,w[,3]) at the scanner's size (``AcousticStream.push``; ``masks``:
        one (h,w) articulator mask for uint8 frames) -> dict: mel_norm / mel_db / mel_log (n, n_mels) of the
        pushed frames, wav = the samples of the rows that became final (``VocoderStream.push``)."""
        from .runtime import mel_glue
        mn = self.acoustic.push(frames, masks)
        db, ln = mel_glue(mn, self.pipeline.mean, self.pipeline.std)
        return {"mel_norm": mn, "mel_db": db, "mel_log": ln, "wav": self.vocoder.push(ln)}

    def flush(self) -> torch.Tensor:
        """End of the clip: the remaining audio; both streams start anew."""
        wav = self.vocoder.flush()
        self.acoustic.reset()
        return wav
