"""Device-side engines over libm2s.

The packed models are created and destroyed through the C ABI (ctypes, ``_native``); every compute
call goes through the PyTorch-ROCm custom ops ``torch.ops.m2s.*`` (``ops``, csrc/torch_ops.cpp), which
allocate outputs and workspace with the torch caching allocator on the current HIP stream.

* ``AcousticEngine``  - packed CNN + BiLSTM + head (replaces OTNLikeCNNBiLSTM.forward,
                        mri2speech_code/mri_acoustic_model.py:116-136)
* ``VocoderEngine``   - packed HiFi-GAN generator (replaces Generator.forward, models.py:113-131)
* ``mel_glue``        - denormalize_mel + dB -> ln-power (run_mri_video_inference.py:160-163,227-233)
* ``Pipeline``        - frames -> mel_norm / mel_db / mel_log / wav in one call on one stream

The opposite direction, waveform -> mel, is ``m2s.melspec.MelSpectrogram``.

Every engine also has ``forward_ragged`` (and ``AcousticEngine.bilstm_ragged``): clips of different lengths in one
call, as a packed tensor of ``sum(lengths)`` rows plus ``lengths``, or as a list of per-clip tensors; outputs are
packed and ``split_packed`` returns the per-clip views.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _native as N
from . import ops as _ops
from .config import CNN_CHUNK


def _device(device) -> torch.device:
    if not torch.cuda.is_available():
        raise N.M2SError("m2s needs a HIP device (MI355X / gfx950); none is visible and there is no CPU fallback")
    d = torch.device(device if device is not None else "cuda")
    if d.type != "cuda":
        raise N.M2SError(f"m2s runs on HIP devices only, got {d}")
    return torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())


def _as_f32(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    if t.device != device:
        raise N.M2SError(f"input on {t.device}, engine on {device}")
    return t.to(torch.float32).contiguous()


def _packed(x, lengths, device: torch.device, row_ndim: int):
    """A ragged call's input as (packed fp32 tensor of sum(lengths) rows, lengths as a list of ints).  ``x`` is
    either that packed tensor already or a list / tuple of per-clip tensors (clip b: ``lengths[b]`` rows of
    ``row_ndim`` axes each; ``lengths`` may then be None), concatenated here."""
    if isinstance(x, (list, tuple)):
        if lengths is None:
            lengths = [int(t.shape[0]) for t in x]
        elif [int(t.shape[0]) for t in x] != [int(n) for n in lengths]:
            raise N.M2SError("lengths do not match the per-clip tensors")
        if not x:
            raise N.M2SError("ragged call without clips")
        x = torch.cat([_as_f32(t, device) for t in x], dim=0)
    if lengths is None:
        raise N.M2SError("a packed tensor needs its clip lengths")
    lengths = [int(n) for n in lengths]
    x = _as_f32(x, device)
    if x.dim() != 1 + row_ndim:
        raise N.M2SError(f"expected a packed tensor of {1 + row_ndim} axes, got {tuple(x.shape)}")
    return x, lengths


def split_packed(x: torch.Tensor, lengths, per_step: int = 1):
    """Per-clip views of a packed tensor: clip b owns ``lengths[b] * per_step`` consecutive entries of axis 0
    (``per_step`` = hop for a packed waveform)."""
    sizes = [int(n) * int(per_step) for n in lengths]
    if sum(sizes) != x.shape[0]:
        raise ValueError(f"packed tensor has {x.shape[0]} rows, lengths give {sum(sizes)}")
    return list(torch.split(x, sizes, dim=0))


class AcousticEngine:
    """libm2s's acoustic model on one device.  ``chunk``: frames per CNN pass (include/m2s.h
    m2s_acoustic_set_chunk); a pass may hold up to chunk + chunk // 16 frames when that saves a short tail
    pass, so size limits chosen through ``chunk`` have ~6 % of headroom to leave."""

    def __init__(self, state_dict: Dict, n_mels: int = 64, rnn_hidden: int = 640, dtype: str = "bf16x3",
                 device=None, chunk: int = CNN_CHUNK):
        self.device = _device(device)
        self.n_mels, self.rnn_hidden, self.dtype = n_mels, rnn_hidden, dtype
        if dtype not in N.DTYPES:
            raise N.M2SError(f"unknown dtype {dtype!r}; one of {sorted(N.DTYPES)}")
        L = N.lib()
        self.ops = _ops.load()
        N.check(L.m2s_device_check(self.device.index))
        arr, keep = N.tensor_array(state_dict)
        h = C.c_void_p()
        N.check(L.m2s_acoustic_create(arr, len(arr), n_mels, rnn_hidden, N.DTYPES[dtype], self.device.index,
                                      C.byref(h)))
        del keep
        self._h = h
        self._destroy = L.m2s_acoustic_destroy  # bound now: module globals may be gone at exit
        N.check(L.m2s_acoustic_set_chunk(self._h, int(chunk)))

    def __del__(self):
        h, destroy = getattr(self, "_h", None), getattr(self, "_destroy", None)
        if h is not None and h.value and destroy is not None:
            destroy(h)
            self._h = None

    @property
    def handle(self) -> int:
        """The m2s_acoustic* as the int the torch.ops.m2s ops take."""
        return int(self._h.value)

    def check(self):
        """Synchronise the device and raise M2SError if a launch of this engine failed asynchronously
        (a BiLSTM grid-barrier timeout: its outputs hold NaN; include/m2s.h m2s_acoustic_status)."""
        torch.cuda.synchronize(self.device)
        N.check(N.lib().m2s_acoustic_status(self._h))

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        """frames (B,T,1,H,W) or (B,T,H,W) fp32 -> normalised mel (B,T,n_mels) fp32."""
        if frames.dim() == 5:
            if frames.size(2) != 1:
                raise N.M2SError("expected a single grey channel")
            frames = frames[:, :, 0]
        if frames.dim() != 4:
            raise N.M2SError(f"expected (B,T,H,W) frames, got {tuple(frames.shape)}")
        return self.ops.acoustic_forward(self.handle, _as_f32(frames, self.device), self.n_mels)

    def effnet(self, frames: torch.Tensor) -> torch.Tensor:
        """frames (N,H,W) -> GAP features (N,208)."""
        return self.ops.effnet_forward(self.handle, _as_f32(frames, self.device))

    def probe(self, frames: torch.Tensor, n_blocks: int) -> torch.Tensor:
        """Feature map after ``n_blocks`` timm blocks (0 = stem), (N,C,OH,OW) fp32."""
        return self.ops.effnet_features(self.handle, _as_f32(frames, self.device), int(n_blocks))

    def bilstm(self, feats: torch.Tensor):
        """feats (B,T,208) -> (sum-merged BiLSTM output (B,T,H), head output (B,T,n_mels))."""
        return self.ops.bilstm_summerge(self.handle, _as_f32(feats, self.device), self.rnn_hidden, self.n_mels)

    def forward_ragged(self, frames, lengths=None) -> torch.Tensor:
        """Clips of different lengths in one call: packed frames (N,[1,]H,W), N = sum(lengths), or a list of
        per-clip (T_b,[1,]H,W) tensors -> packed normalised mel (N,n_mels); ``split_packed`` gives the clips."""
        if isinstance(frames, (list, tuple)):
            frames = [f[:, 0] if f.dim() == 4 else f for f in frames]
        elif frames.dim() == 4:
            frames = frames[:, 0]
        x, lengths = _packed(frames, lengths, self.device, 2)
        return self.ops.acoustic_forward_ragged(self.handle, x, lengths, self.n_mels)

    def bilstm_ragged(self, feats, lengths=None):
        """packed feats (N,208) or a list of (T_b,208) -> packed (BiLSTM output (N,H), head output (N,n_mels))."""
        x, lengths = _packed(feats, lengths, self.device, 1)
        return self.ops.bilstm_summerge_ragged(self.handle, x, lengths, self.rnn_hidden, self.n_mels)

    # ---- windowed inference (include/m2s.h "windowed inference"): the BiLSTM on sliding windows of `window` frames,
    # the distribution the checkpoint was trained on; additive, the whole-clip calls above stay the default
    @staticmethod
    def _window_args(x, lengths, window, merge, context):
        if merge not in _ops.WINDOW_MERGES:
            raise N.M2SError(f"unknown window merge {merge!r}; one of {sorted(_ops.WINDOW_MERGES)}")
        if lengths is None and not isinstance(x, (list, tuple)):
            lengths = [int(x.shape[0])]  # one clip
        context = [] if context is None else [int(c) for c in context]
        return lengths, int(window), _ops.WINDOW_MERGES[merge], context

    def bilstm_windowed(self, feats, lengths=None, window: int = 4, merge: str = "latest", context=None):
        """packed feats (N,208) (one clip if ``lengths`` is None) or a list of (T_b,208) -> packed (merged BiLSTM
        output (R,H), head output (R,n_mels)).  ``latest``: row t comes from the window ending at t (causal);
        ``mean``: the average over the full windows containing t.  ``context[b]`` (latest only, <= window - 1):
        leading rows of clip b that are history only, R = N - sum(context)."""
        lengths, window, merge, context = self._window_args(feats, lengths, window, merge, context)
        x, lengths = _packed(feats, lengths, self.device, 1)
        return self.ops.bilstm_windowed(self.handle, x, lengths, context, window, merge, self.rnn_hidden, self.n_mels)

    def forward_windowed(self, frames, lengths=None, window: int = 4, merge: str = "latest", context=None):
        """packed frames (N,[1,]H,W) (one clip if ``lengths`` is None) or a list of per-clip tensors -> packed
        normalised mel (R,n_mels) of the windowed model; the CNN runs once per frame."""
        if isinstance(frames, (list, tuple)):
            frames = [f[:, 0] if f.dim() == 4 else f for f in frames]
        elif frames.dim() == 4:
            frames = frames[:, 0]
        lengths, window, merge, context = self._window_args(frames, lengths, window, merge, context)
        x, lengths = _packed(frames, lengths, self.device, 2)
        return self.ops.acoustic_forward_windowed(self.handle, x, lengths, context, window, merge, self.n_mels)

    # ---- pair outputs (include/m2s.h "pair outputs"): the model on every training pair, i.e. every window of
    # `window` consecutive frames of a clip, stride 1, with all `window` rows of each kept: what a loss over the
    # reference's pairs_ref{window} needs.  The CNN still runs once per frame row.
    def bilstm_pairs(self, feats, lengths=None, window: int = 4):
        """packed feats (N,208) (one clip if ``lengths`` is None) or a list of (T_b,208) -> (merged BiLSTM output
        (P,window,H), head output (P,window,n_mels)), P = sum(T_b - window + 1): pairs in clip order, windows
        ascending within a clip.  Every clip must have at least ``window`` rows."""
        if lengths is None and not isinstance(feats, (list, tuple)):
            lengths = [int(feats.shape[0])]
        x, lengths = _packed(feats, lengths, self.device, 1)
        return self.ops.bilstm_pairs(self.handle, x, lengths, int(window), self.rnn_hidden, self.n_mels)

    def forward_pairs(self, frames, lengths=None, window: int = 4):
        """packed frames (N,[1,]H,W) (one clip if ``lengths`` is None) or a list of per-clip tensors -> normalised
        mel (P,window,n_mels) of every training pair."""
        if isinstance(frames, (list, tuple)):
            frames = [f[:, 0] if f.dim() == 4 else f for f in frames]
        elif frames.dim() == 4:
            frames = frames[:, 0]
        if lengths is None and not isinstance(frames, (list, tuple)):
            lengths = [int(frames.shape[0])]
        x, lengths = _packed(frames, lengths, self.device, 2)
        return self.ops.acoustic_forward_pairs(self.handle, x, lengths, int(window), self.n_mels)


class VocoderEngine:
    def __init__(self, state_dict: Dict, h, dtype: str = "bf16x3", device=None):
        self.device = _device(device)
        self.h, self.dtype = dict(h), dtype
        if dtype not in N.DTYPES:
            raise N.M2SError(f"unknown dtype {dtype!r}; one of {sorted(N.DTYPES)}")
        L = N.lib()
        self.ops = _ops.load()
        N.check(L.m2s_device_check(self.device.index))
        arr, keep = N.tensor_array(state_dict)
        self._hh = N.hifigan_h(h)
        v = C.c_void_p()
        N.check(L.m2s_vocoder_create(arr, len(arr), C.byref(self._hh), N.DTYPES[dtype], self.device.index,
                                     C.byref(v)))
        del keep
        self._h = v
        self._destroy = L.m2s_vocoder_destroy
        self.hop = 1
        for u in h["upsample_rates"]:
            self.hop *= int(u)

    def __del__(self):
        h, destroy = getattr(self, "_h", None), getattr(self, "_destroy", None)
        if h is not None and h.value and destroy is not None:
            destroy(h)
            self._h = None

    @property
    def handle(self) -> int:
        return int(self._h.value)

    def forward(self, mel: torch.Tensor, layout: int = 0) -> torch.Tensor:
        """mel (B,num_mels,T) [layout 0, as Generator.forward] or (B,T,num_mels) [layout 1] -> (B,1,T*hop)."""
        x = _as_f32(mel, self.device)
        if x.dim() != 3:
            raise N.M2SError(f"expected a 3-D mel, got {tuple(x.shape)}")
        C_ = x.shape[1] if layout == 0 else x.shape[2]
        if C_ != self.h["num_mels"]:
            raise N.M2SError(f"mel has {C_} bins, generator expects {self.h['num_mels']}")
        return self.ops.hifigan_forward(self.handle, x, int(layout), self.hop)

    def tap_shape(self, tap: int):
        """(channels, rows per mel frame) of ``probe``'s tap: 0 = conv_pre's output, 2i + 1 = stage i's upsampler
        output, 2i + 2 = stage i's MRF output."""
        if not 0 <= tap <= 2 * len(self.h["upsample_rates"]):
            raise N.M2SError(f"tap {tap} outside 0 .. {2 * len(self.h['upsample_rates'])}")
        c, scale = int(self.h["upsample_initial_channel"]), 1
        for u in self.h["upsample_rates"][: (tap + 1) // 2]:
            c, scale = c // 2, scale * int(u)
        return c, scale

    def probe(self, mel: torch.Tensor, tap: int, layout: int = 0):
        """The tensor the dense call stores at ``tap`` (see ``tap_shape``), exactly as stored: (B, C, L) fp32 (every
        value a bf16 value in a bf16 / fp8 engine), and whether the engine holds it as LeakyReLU(x) (slope 0.1; the
        split engine's batched stages), in which case it is returned as held."""
        x = _as_f32(mel, self.device)
        if x.dim() != 3:
            raise N.M2SError(f"expected a 3-D mel, got {tuple(x.shape)}")
        c, scale = self.tap_shape(int(tap))
        act = C.c_int(0)
        N.check(N.lib().m2s_vocoder_tap_info(self._h, int(tap), 1, None, None, C.byref(act)))
        return self.ops.hifigan_features(self.handle, x, int(layout), int(tap), c, scale), bool(act.value)

    def forward_ragged(self, mel, lengths=None) -> torch.Tensor:
        """Mels of different lengths in one call: packed (N,num_mels) ln-mel (time-major rows), or a list of
        per-clip (T_b,num_mels) tensors -> packed waveform (N*hop,); ``split_packed(wav, lengths, hop)``."""
        x, lengths = _packed(mel, lengths, self.device, 1)
        if x.shape[1] != self.h["num_mels"]:
            raise N.M2SError(f"mel has {x.shape[1]} bins, generator expects {self.h['num_mels']}")
        return self.ops.hifigan_forward_ragged(self.handle, x, lengths, self.hop)

    @property
    def reach(self):
        """(back, ahead): output frame o depends on mel rows o - back .. o + ahead (m2s_vocoder_reach; the same
        numbers as ``config.generator_reach(h)``)."""
        b, a = C.c_int(0), C.c_int(0)
        N.check(N.lib().m2s_vocoder_reach(self._h, C.byref(b), C.byref(a)))
        return int(b.value), int(a.value)

    def set_chunk_cone(self, on: bool) -> None:
        """Tests and timing: whether ``forward_chunk`` drops, between stages, the rows no emitted sample depends on.
        The results are the same either way."""
        N.check(N.lib().m2s_vocoder_set_chunk_cone(self._h, 1 if on else 0))

    def forward_chunk(self, mel, lengths=None, context=None, hold=None) -> torch.Tensor:
        """Spans of streams in one stateless call: packed (N,num_mels) ln-mel (one span if ``lengths`` is None) or a
        list of per-span (T_b,num_mels) tensors -> packed waveform of the rows ``context[b] .. T_b - hold[b] - 1`` of
        every span, ``(N - sum(context) - sum(hold)) * hop`` samples.  They are the whole clip's rows where the span
        brings ``context >= reach[0]`` rows of history (or starts the clip) and ``hold >= reach[1]`` rows of
        look-ahead (or ends it)."""
        if lengths is None and not isinstance(mel, (list, tuple)):
            lengths = [int(mel.shape[0])]
        x, lengths = _packed(mel, lengths, self.device, 1)
        if x.shape[1] != self.h["num_mels"]:
            raise N.M2SError(f"mel has {x.shape[1]} bins, generator expects {self.h['num_mels']}")
        context = [0] * len(lengths) if context is None else [int(c) for c in context]
        hold = [0] * len(lengths) if hold is None else [int(c) for c in hold]
        if len(context) != len(lengths) or len(hold) != len(lengths):
            raise N.M2SError("one context and one hold entry per span")
        return self.ops.hifigan_forward_chunk(self.handle, x, lengths, context, hold, self.hop)


def mel_glue(mel_norm: torch.Tensor, mean: torch.Tensor, std: torch.Tensor):
    """(rows..., n_mels) -> (mel_db, mel_log), same shape."""
    d = mel_norm.device
    return _ops.load().mel_glue(mel_norm.to(torch.float32).contiguous(), torch.as_tensor(mean).to(d),
                                torch.as_tensor(std).to(d))


def preprocess_frames(frames: torch.Tensor, size=None, interp: str = "linear", norm: str = "zscore") -> torch.Tensor:
    """Decoded uint8 frames on the device, (T,h,w) grey or (T,h,w,3) BGR -> (T,H,W) fp32 in [0, 1].

    ``size=None`` with the defaults: the frames already have the model's size and get _preprocess_frame's
    normalisation (run_mri_video_inference.py:34-54; ``torch.ops.m2s.preprocess_frames``).  Otherwise the frames
    are at the scanner's size and ``torch.ops.m2s.preprocess_frames_resize`` resizes them to ``size`` = (H, W)
    (default: their own size) on the device as ``cv2.resize`` would (``interp`` "linear" = INTER_LINEAR, "area" =
    INTER_AREA; no axis may shrink, at most 65536 pixels a frame) and normalises them (``norm`` "zscore" = per-frame
    z-score + min-max, "unit" = / 255).  ("linear", "zscore") is the reference's inference convention, ("area",
    "unit") its training convention (mri2speech_code/preprocess_rtmri_data.py:99-113)."""
    if frames.dtype != torch.uint8:
        raise N.M2SError(f"expected uint8 frames, got {frames.dtype}")
    if frames.device.type != "cuda":
        raise N.M2SError("preprocess_frames runs on the HIP device; move the decoded frames there first")
    if not (frames.dim() == 3 or (frames.dim() == 4 and frames.shape[-1] == 3)):
        raise N.M2SError(f"expected (T,H,W) or (T,H,W,3) frames, got {tuple(frames.shape)}")
    if interp not in _ops.FRAME_INTERPS:
        raise N.M2SError(f"interp {interp!r} is none of {sorted(_ops.FRAME_INTERPS)}")
    if norm not in _ops.FRAME_NORMS:
        raise N.M2SError(f"norm {norm!r} is none of {sorted(_ops.FRAME_NORMS)}")
    if size is None and interp == "linear" and norm == "zscore":
        return _ops.load().preprocess_frames(frames.contiguous())
    out_h, out_w = (int(frames.shape[1]), int(frames.shape[2])) if size is None else (int(size[0]), int(size[1]))
    return _ops.load().preprocess_frames_resize(frames.contiguous(), out_h, out_w, _ops.FRAME_INTERPS[interp],
                                                _ops.FRAME_NORMS[norm])


def preprocess_frames_masked(frames: torch.Tensor, masks, size=None, interp: str = "linear",
                             norm: str = "zscore") -> torch.Tensor:
    """``preprocess_frames`` for M masked variants of every frame in one launch: uint8 frames (T,h,w[,3]) on the
    device, ``masks`` (M,h,w) or one (h,w) mask (tensor or array, fp32) -> (M,T,H,W) fp32.  Variant m is the
    reference's application, ``(frame.astype(float32) * mask).clip(0, 255).astype(uint8)`` on every channel
    (scripts/mask_rtmri_video.py:96-98), followed by the front end of ``preprocess_frames(frames, size, interp,
    norm)`` (``size`` None = the frames' own size); an all-ones mask gives that call's output bit for bit."""
    if frames.dtype != torch.uint8:
        raise N.M2SError(f"expected uint8 frames, got {frames.dtype}")
    if frames.device.type != "cuda":
        raise N.M2SError("preprocess_frames_masked runs on the HIP device; move the decoded frames there first")
    if not (frames.dim() == 3 or (frames.dim() == 4 and frames.shape[-1] == 3)):
        raise N.M2SError(f"expected (T,H,W) or (T,H,W,3) frames, got {tuple(frames.shape)}")
    if interp not in _ops.FRAME_INTERPS:
        raise N.M2SError(f"interp {interp!r} is none of {sorted(_ops.FRAME_INTERPS)}")
    if norm not in _ops.FRAME_NORMS:
        raise N.M2SError(f"norm {norm!r} is none of {sorted(_ops.FRAME_NORMS)}")
    mk = torch.as_tensor(masks, dtype=torch.float32).to(frames.device)
    if mk.dim() == 2:
        mk = mk[None]
    if mk.dim() != 3 or mk.shape[0] < 1 or tuple(mk.shape[1:]) != tuple(frames.shape[1:3]):
        raise N.M2SError(f"expected masks (M,{frames.shape[1]},{frames.shape[2]}), got {tuple(mk.shape)}")
    out_h, out_w = (int(frames.shape[1]), int(frames.shape[2])) if size is None else (int(size[0]), int(size[1]))
    return _ops.load().preprocess_frames_masked(frames.contiguous(), mk.contiguous(), out_h, out_w,
                                                _ops.FRAME_INTERPS[interp], _ops.FRAME_NORMS[norm])


class Pipeline:
    """frames -> (mel_norm, mel_db, mel_log, wav) on one stream (run_mri_video_inference.py:218-242)."""

    def __init__(self, acoustic: AcousticEngine, vocoder: VocoderEngine, mean, std):
        if acoustic.device != vocoder.device:
            raise N.M2SError("acoustic model and vocoder must share a device")
        self.ac, self.voc, self.device = acoustic, vocoder, acoustic.device
        self.mean = torch.as_tensor(mean, dtype=torch.float32).to(self.device).contiguous()
        self.std = torch.as_tensor(std, dtype=torch.float32).to(self.device).contiguous()

    def forward(self, frames: torch.Tensor, out: Optional[Dict[str, torch.Tensor]] = None):
        """frames (B,T,[1,]H,W) -> dict mel_norm / mel_db / mel_log (B,T,n_mels), wav (B,T*hop)."""
        if frames.dim() == 5:
            frames = frames[:, :, 0]
        x = _as_f32(frames, self.device)
        mn, db, ln, wav = self.ac.ops.pipeline_forward(self.ac.handle, self.voc.handle, x, self.mean, self.std,
                                                       self.ac.n_mels, self.voc.hop)
        res = {"mel_norm": mn, "mel_db": db, "mel_log": ln, "wav": wav}
        if out is not None:  # caller-owned buffers (kept for API compatibility)
            for k, v in res.items():
                if k in out:
                    out[k].copy_(v)
            return out
        return res

    def roundtrip_error(self, out: Dict[str, torch.Tensor], h=None) -> torch.Tensor:
        """The HiFi-GAN validation metric (train.py:228-252) of a ``forward`` result: per clip, the mean
        |mel(out["wav"]) - out["mel_log"]|, with the mel taken on the device (m2s/melspec.py).  ``h``: the analysis
        config (n_fft, win_size, fmin, fmax, ...); default: the vocoder's own config over config.HIFIGAN_MEL."""
        from .config import HIFIGAN_MEL
        from .melspec import mel_l1
        cfg = {**HIFIGAN_MEL, **self.voc.h} if h is None else h
        return mel_l1(out["wav"], out["mel_log"], cfg, layout=1)

    def forward_ragged(self, frames, lengths=None):
        """Clips of different lengths in one call: packed frames (N,[1,]H,W) or a list of per-clip tensors ->
        dict of packed mel_norm / mel_db / mel_log (N,n_mels) and wav (N*hop,)."""
        if isinstance(frames, (list, tuple)):
            frames = [f[:, 0] if f.dim() == 4 else f for f in frames]
        elif frames.dim() == 4:
            frames = frames[:, 0]
        x, lengths = _packed(frames, lengths, self.device, 2)
        mn, db, ln, wav = self.ac.ops.pipeline_forward_ragged(self.ac.handle, self.voc.handle, x, lengths, self.mean,
                                                              self.std, self.ac.n_mels, self.voc.hop)
        return {"mel_norm": mn, "mel_db": db, "mel_log": ln, "wav": wav}

    def forward_windowed(self, frames, lengths=None, window: int = 4, merge: str = "latest"):
        """``forward_ragged`` with the windowed acoustic model (AcousticEngine.forward_windowed): the windowed
        acoustic call, the mel glue, then the ragged vocoder leg on its mel_log, all on the device."""
        if isinstance(frames, (list, tuple)):
            lengths = [int(f.shape[0]) for f in frames] if lengths is None else lengths
        elif lengths is None:
            lengths = [int(frames.shape[0])]
        mn = self.ac.forward_windowed(frames, lengths, window, merge)
        db, ln = mel_glue(mn, self.mean, self.std)
        wav = self.voc.forward_ragged(ln, lengths)
        return {"mel_norm": mn, "mel_db": db, "mel_log": ln, "wav": wav}

    def occlusion(self, frames_u8: torch.Tensor, masks, bands=None, size=None, interp: str = "linear",
                  norm: str = "zscore", windowed=None, wav_variants=(), chunk: int = 64, normalize: bool = False):
        """The masking experiment of one clip on the device (docs/rtmri_pipeline_notes.md step 5).

        ``frames_u8`` uint8 (T,h,w[,3]) on the device, ``masks`` (M,h,w) fp32 (``m2s.occlusion``), ``bands`` {name:
        mel-bin indices} (``m2s.gradcam.parse_band_arguments``) or None.  An all-ones mask is prepended as variant
        0, the masked front end makes the (1 + M, T) batch at ``size`` (None = the frames' size), ONE engine call
        runs it (whole-clip ``forward``; ``windowed`` = a window length for ``forward_windowed``, merge "latest"),
        the mel glue gives mel_db and ``occlusion_reduce`` the scores in dB.  Returns dict: ``score`` (M,nb),
        ``per_frame`` (M,T,nb), ``map`` (nb,h,w) (min-max scaled with ``normalize``), ``names`` (nb columns, the
        last "all"), ``mel_db`` / ``mel_norm`` (T,n_mels) of the baseline, ``wavs`` {v: (T*hop,)} for the variants
        ``wav_variants`` names (0 = baseline, m + 1 = masks[m]).  An engine call holds at most ``chunk`` variants,
        variant 0 included in every one, so each difference is taken inside one batch.  Nothing is read back to
        the host between the uint8 upload and the returned tensors."""
        from .occlusion import band_matrix
        if frames_u8.dim() not in (3, 4) or frames_u8.shape[0] < 1:
            raise N.M2SError(f"expected one clip of uint8 frames (T,h,w[,3]), got {tuple(frames_u8.shape)}")
        if frames_u8.device != self.device:
            raise N.M2SError(f"frames on {frames_u8.device}, pipeline on {self.device}")
        mk = torch.as_tensor(masks, dtype=torch.float32).to(self.device)
        if mk.dim() == 2:
            mk = mk[None]
        M, T = int(mk.shape[0]), int(frames_u8.shape[0])
        chunk = int(chunk)
        if M < 1 or chunk < 2:
            raise N.M2SError("occlusion needs at least one mask and a chunk of at least 2 variants")
        wav_variants = [int(v) for v in wav_variants]
        if any(not 0 <= v <= M for v in wav_variants):
            raise N.M2SError(f"wav_variants outside 0..{M}")
        bm, names = band_matrix(bands, self.ac.n_mels)
        bm = bm.to(self.device)
        ones = torch.ones_like(mk[:1])
        red = _ops.load().occlusion_reduce
        base, parts, wavs = None, [], {}
        for lo in range(0, M, chunk - 1):
            hi = min(M, lo + chunk - 1)
            x = preprocess_frames_masked(frames_u8, torch.cat([ones, mk[lo:hi]]), size, interp, norm)  # (1+Mc,T,H,W)
            B = int(x.shape[0])
            if windowed is None:
                mn = self.ac.forward(x)
            else:
                mn = self.ac.forward_windowed(x.reshape(B * T, *x.shape[2:]), [T] * B, int(windowed), "latest")
                mn = mn.view(B, T, -1)
            db, ln = mel_glue(mn, self.mean, self.std)
            if base is None:
                base = {"mel_db": db[0], "mel_norm": mn[0]}
            for v in wav_variants:
                row = 0 if v == 0 else v - lo
                if (v == 0 and lo == 0) or (v > 0 and lo < v <= hi):
                    wavs[v] = self.voc.forward(ln[row:row + 1], layout=1)[0, 0]
            parts.append((db, lo, hi))
        if len(parts) == 1:
            score, pf, mp = red(parts[0][0], bm, mk, bool(normalize), True)
        else:
            # |(a - b) - 0| = |a - b| exactly: the chunks' own differences against a zero baseline give the bits of
            # a per-chunk reduction, and the map sees every variant
            diff = torch.cat([torch.zeros_like(parts[0][0][:1])] + [db[1:] - db[:1] for db, _, _ in parts])
            score, pf, mp = red(diff, bm, mk, bool(normalize), True)
        return {"score": score, "per_frame": pf, "map": mp, "names": names, "wavs": wavs, **base}

    def forward_pairs(self, frames, lengths=None, window: int = 4):
        """The acoustic model on every training pair of the clips (AcousticEngine.forward_pairs): normalised mel
        (P,window,n_mels).  No vocoder leg: the pairs are what the validation losses are taken on."""
        return self.ac.forward_pairs(frames, lengths, window)

    def validate(self, frames, lengths, mel_db, mask=None, mean=None, std=None, window: int = 4, select=None,
                 group: int = 8, metrics=None):
        """The reference's validation numbers (OTNLikeTrainer.validate, eval_mel.py) of packed clips, on the device.

        ``frames`` packed (N,[1,]H,W) or a list of per-clip tensors, ``mel_db`` the packed (N,n_mels) dB mels of the
        same rows (what save_sample writes), ``mask`` packed (N,) floats or None = ones; ``mean`` / ``std`` the
        scaler (default: the pipeline's).  Runs ``forward_pairs``, standardises the target ``(mel_db - mean) / std``
        and cuts target and mask into the same (P,window,.) pairs, keeps the pairs ``select`` names (an index
        tensor into the P pairs, in the order the groups are to be formed), and updates ``metrics`` (a
        ``m2s.metrics.MelMetrics``; a new one if None) with groups of ``group`` pairs.  Every clip must have at least
        ``window`` rows.  No host synchronisation; returns the MelMetrics, whose ``compute()`` downloads."""
        from .metrics import MelMetrics, pair_index
        if isinstance(frames, (list, tuple)):
            lengths = [int(f.shape[0]) for f in frames] if lengths is None else lengths
        elif lengths is None:
            lengths = [int(frames.shape[0])]
        lengths = [int(n) for n in lengths]
        mean = self.mean if mean is None else torch.as_tensor(mean, dtype=torch.float32).to(self.device)
        std = self.std if std is None else torch.as_tensor(std, dtype=torch.float32).to(self.device)
        pred = self.ac.forward_pairs(frames, lengths, window)
        tgt = (_as_f32(mel_db, self.device) - mean) / std
        if tgt.shape[0] != sum(lengths):
            raise N.M2SError(f"mel_db has {tgt.shape[0]} rows, lengths give {sum(lengths)}")
        idx = pair_index(lengths, window, self.device)  # (P, window) packed row of every pair row
        if select is not None:
            sel = torch.as_tensor(select, dtype=torch.long).to(self.device)
            pred, idx = pred.index_select(0, sel), idx.index_select(0, sel)
        mk = None if mask is None else _as_f32(mask, self.device)[idx]
        if metrics is None:
            metrics = MelMetrics(self.ac.n_mels, mean, std, device=self.device)
        metrics.update(pred, tgt[idx], mk, group=group)
        return metrics
