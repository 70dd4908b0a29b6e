"""torch.ops.m2s.* - the PyTorch-ROCm custom ops of libm2s (csrc/torch_ops.cpp) and their fake kernels.

``load()`` loads ``libm2s_torch.so`` (built in-tree next to ``libm2s.so``, which it links) with
``torch.ops.load_library``; there is no fallback: a missing library raises ``M2SError``.  The ops
take the packed model as an opaque int handle (``AcousticEngine.handle`` / ``VocoderEngine.handle``)
and run on the current HIP stream.  The fake (meta) kernels below give every op its output shapes
for FakeTensor tracing / torch.compile / ``torch.library.opcheck``.

Reference interfaces: mri2speech_code/mri_acoustic_model.py:15-18,39-48,67-72,116-136 (acoustic model),
models.py:113-131 (Generator.forward), scripts/run_mri_video_inference.py:34-54,160-163,222-242.
"""
from __future__ import annotations

import os

import torch

from ._native import M2SError

TORCH_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libm2s_torch.so")
OPS = ("acoustic_forward", "effnet_forward", "effnet_features", "bilstm_summerge", "mel_glue", "hifigan_forward",
       "pipeline_forward", "preprocess_frames", "cam_backbone", "bilstm_train_forward", "bilstm_train_backward",
       "linear_forward", "linear_backward", "gap_forward", "gap_backward")
# ragged batches: clips of different lengths in one call, packed tensors of sum(lengths) rows (include/m2s.h)
RAGGED_OPS = ("bilstm_summerge_ragged", "acoustic_forward_ragged", "hifigan_forward_ragged", "pipeline_forward_ragged")
# windowed inference: the BiLSTM over sliding windows of `window` frames (packed like the ragged ops; merge 0 = latest,
# 1 = mean; `context` = leading history rows per clip that get no output row, [] = none)
WINDOWED_OPS = ("bilstm_windowed", "acoustic_forward_windowed")
WINDOW_MERGES = {"latest": 0, "mean": 1}
# validation: the model on every training pair (window of `window` frames, stride 1) of packed clips, P =
# sum(lengths[b] - window + 1) pairs, and the reference's validation numbers of a (B,T,M) batch in two launches
# (include/m2s.h "pair outputs", "fused mel metrics"; m2s/metrics.py)
PAIR_OPS = ("bilstm_pairs", "acoustic_forward_pairs")
METRIC_OPS = ("mel_metrics",)
# streaming vocoder: the generator on spans of a stream, emitting only the rows that are final (packed like the ragged
# ops; `context` / `hold` = leading / trailing rows per clip that are read but get no output)
STREAM_OPS = ("hifigan_forward_chunk",)
# the vocoder's stage tap (include/m2s.h m2s_vocoder_probe; VocoderEngine.probe): the tensor stored at `tap`
PROBE_OPS = ("hifigan_features",)
# analysis: waveform -> mel (m2s/melspec.py; handle = MelSpectrogram.handle)
ANALYSIS_OPS = ("mel_spectrogram",)
# frame front end: native-size uint8 frames -> resized, normalised fp32 frames (csrc/frames.hip); interp / norm are the
# values of m2s_frame_interp / m2s_frame_norm (include/m2s.h)
FRAME_OPS = ("preprocess_frames_resize",)
FRAME_INTERPS = {"linear": 0, "area": 1}
FRAME_NORMS = {"zscore": 0, "unit": 1}
# occlusion (m2s/occlusion.py; include/m2s.h "occlusion"): the frame front end for M masked variants of every frame, and
# the variants' mels -> per-band scores and a coverage-weighted map
OCCLUSION_OPS = ("preprocess_frames_masked", "occlusion_reduce")
# Grad-CAM engine (m2s/gradcam.py; handle = GradCam.handle): every band and target frame of a clip in one call, and
# its stages (include/m2s.h "Grad-CAM engine")
GRADCAM_OPS = ("gradcam", "gradcam_cotangents", "bilstm_train_backward_multi", "cam_heatmap")
# fine-tuning engine (m2s/finetune.py; handle = HeadTuner.handle): one optimisation step of the BiLSTM and mel head on
# cached encoder features, its forward alone, the last gradients, and the state out of / into the engine
FINETUNE_OPS = ("finetune_step", "finetune_forward", "finetune_grads", "finetune_export", "finetune_import")
FINETUNE_SLOTS = ("loss", "mse", "mae", "delta", "accel", "latest", "grad_norm", "clip_coef")
# the engine's 10 tensors in its order (include/m2s.h "fine-tuning"), under the reference's key names
FINETUNE_KEYS = tuple(f"rnn.lstm.{n}_l0{sfx}" for sfx in ("", "_reverse")
                      for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) + ("head.weight", "head.bias")

# timm tf_efficientnetv2_b2 (features_only): stride and output channels of the stem (index 0) and of
# the 29 blocks that follow (effnet_features' n_blocks = how many of them ran)
_FEAT_STRIDE = [2] + [1, 1] + [2, 1, 1] + [2, 1, 1] + [2, 1, 1, 1] + [1] * 6 + [2] + [1] * 9
_FEAT_CH = [32] + [16] * 2 + [32] * 3 + [56] * 3 + [104] * 4 + [120] * 6 + [208] * 10

def cam_bn_layers():
    """(state-dict prefix, channels, input reduction) of every BatchNorm in cam_backbone's statistics
    order: conv_stem's bn1, then per block bn1 / bn2 / bn3 (timm key names).  The reduction is the
    layer's spatial stride w.r.t. the frame (its map is ceil-halved that many times)."""
    from .config import EFFNET_STEM, effnet_blocks
    out = [("cnn.backbone.bn1", EFFNET_STEM, 2)]
    red = 2
    for b in effnet_blocks():
        q = f"cnn.backbone.blocks.{b['stage']}.{b['idx']}."
        r_in, red = red, red * b["stride"]
        layers = {"cn": [(b["cout"], red)], "er": [(b["mid"], red), (b["cout"], red)],
                  "ir": [(b["mid"], r_in), (b["mid"], red), (b["cout"], red)]}[b["type"]]
        out += [(f"{q}bn{i + 1}", c, r) for i, (c, r) in enumerate(layers)]
    return out


# floats of cam_backbone's BatchNorm statistics: [mean C | var C] per layer
CAM_BN_STATS = 2 * sum(c for _, c, _ in cam_bn_layers())

_loaded = False

# m2s_melspec* handle -> (n_fft, hop, reflect pad per side, n_mels): what mel_spectrogram's fake kernel needs to
# shape its output without touching the device; MelSpectrogram registers itself here
_MELSPEC_GEOMETRY = {}


def register_melspec(handle: int, n_fft: int, hop: int, pad: int, n_mels: int) -> None:
    _MELSPEC_GEOMETRY[int(handle)] = (int(n_fft), int(hop), int(pad), int(n_mels))


def unregister_melspec(handle: int) -> None:
    _MELSPEC_GEOMETRY.pop(int(handle), None)


def melspec_geometry(handle: int):
    try:
        return _MELSPEC_GEOMETRY[int(handle)]
    except KeyError:
        raise M2SError(f"mel_spectrogram: handle {handle:#x} was not created by m2s.melspec.MelSpectrogram") from None


# m2s_finetune* handle -> n_mels, for finetune_forward's fake kernel; HeadTuner registers itself here
_FINETUNE_MELS = {}


def target_mels(handle: int) -> int:
    try:
        return _FINETUNE_MELS[int(handle)]
    except KeyError:
        raise M2SError(f"finetune: handle {handle:#x} was not created by m2s.finetune.HeadTuner") from None


def load():
    """Load libm2s_torch.so once (registers torch.ops.m2s.*) and the fake kernels."""
    global _loaded
    if _loaded:
        return torch.ops.m2s
    if not os.path.exists(TORCH_LIB_PATH):
        raise M2SError(f"libm2s_torch.so not found at {TORCH_LIB_PATH}; build it with `make -C mri-to-speech_amd/csrc` "
                       "(there is no CPU fallback)")
    torch.ops.load_library(TORCH_LIB_PATH)
    _register_fakes()
    _loaded = True
    return torch.ops.m2s


def feature_shape(n: int, h: int, w: int, n_blocks: int):
    """(N, C, OH, OW) of effnet_features after `n_blocks` blocks (TF-SAME: out = ceil(in / stride))."""
    oh, ow = h, w
    for s in _FEAT_STRIDE[: n_blocks + 1]:
        oh, ow = (oh + s - 1) // s, (ow + s - 1) // s
    return n, _FEAT_CH[n_blocks], oh, ow


def _register_fakes():
    f = torch.library.register_fake

    @f("m2s::acoustic_forward")
    def _acoustic(handle, frames, n_mels):
        return frames.new_empty((frames.shape[0], frames.shape[1], n_mels), dtype=torch.float32)

    @f("m2s::effnet_forward")
    def _effnet(handle, frames):
        return frames.new_empty((frames.shape[0], 208), dtype=torch.float32)

    @f("m2s::effnet_features")
    def _features(handle, frames, n_blocks):
        return frames.new_empty(feature_shape(frames.shape[0], frames.shape[1], frames.shape[2], n_blocks),
                                dtype=torch.float32)

    @f("m2s::bilstm_summerge")
    def _bilstm(handle, feats, hidden, n_mels):
        b, t = feats.shape[0], feats.shape[1]
        return (feats.new_empty((b, t, hidden), dtype=torch.float32),
                feats.new_empty((b, t, n_mels), dtype=torch.float32))

    @f("m2s::mel_glue")
    def _glue(mel_norm, mean, std):
        return (torch.empty_like(mel_norm, dtype=torch.float32), torch.empty_like(mel_norm, dtype=torch.float32))

    @f("m2s::hifigan_forward")
    def _hifigan(handle, mel, layout, hop):
        t = mel.shape[2] if layout == 0 else mel.shape[1]
        return mel.new_empty((mel.shape[0], 1, t * hop), dtype=torch.float32)

    @f("m2s::hifigan_features")
    def _hifigan_features(handle, mel, layout, tap, channels, scale):
        t = mel.shape[2] if layout == 0 else mel.shape[1]
        return mel.new_empty((mel.shape[0], channels, t * scale), dtype=torch.float32)

    @f("m2s::pipeline_forward")
    def _pipeline(acoustic, vocoder, frames, mean, std, n_mels, hop):
        b, t = frames.shape[0], frames.shape[1]
        mel = [frames.new_empty((b, t, n_mels), dtype=torch.float32) for _ in range(3)]
        return mel[0], mel[1], mel[2], frames.new_empty((b, t * hop), dtype=torch.float32)

    @f("m2s::bilstm_summerge_ragged")
    def _bilstm_ragged(handle, feats, lengths, hidden, n_mels):
        n = feats.shape[0]
        return (feats.new_empty((n, hidden), dtype=torch.float32), feats.new_empty((n, n_mels), dtype=torch.float32))

    @f("m2s::acoustic_forward_ragged")
    def _acoustic_ragged(handle, frames, lengths, n_mels):
        return frames.new_empty((frames.shape[0], n_mels), dtype=torch.float32)

    @f("m2s::hifigan_forward_ragged")
    def _hifigan_ragged(handle, mel, lengths, hop):
        return mel.new_empty((mel.shape[0] * hop,), dtype=torch.float32)

    @f("m2s::pipeline_forward_ragged")
    def _pipeline_ragged(acoustic, vocoder, frames, lengths, mean, std, n_mels, hop):
        n = frames.shape[0]
        mel = [frames.new_empty((n, n_mels), dtype=torch.float32) for _ in range(3)]
        return mel[0], mel[1], mel[2], frames.new_empty((n * hop,), dtype=torch.float32)

    @f("m2s::bilstm_windowed")
    def _bilstm_windowed(handle, feats, lengths, context, window, merge, hidden, n_mels):
        r = feats.shape[0] - sum(context)
        return (feats.new_empty((r, hidden), dtype=torch.float32), feats.new_empty((r, n_mels), dtype=torch.float32))

    @f("m2s::acoustic_forward_windowed")
    def _acoustic_windowed(handle, frames, lengths, context, window, merge, n_mels):
        return frames.new_empty((frames.shape[0] - sum(context), n_mels), dtype=torch.float32)

    def _pairs(lengths, window):
        return sum(max(0, n - window + 1) for n in lengths)

    @f("m2s::bilstm_pairs")
    def _bilstm_pairs(handle, feats, lengths, window, hidden, n_mels):
        p = _pairs(lengths, window)
        return (feats.new_empty((p, window, hidden), dtype=torch.float32),
                feats.new_empty((p, window, n_mels), dtype=torch.float32))

    @f("m2s::acoustic_forward_pairs")
    def _acoustic_pairs(handle, frames, lengths, window, n_mels):
        return frames.new_empty((_pairs(lengths, window), window, n_mels), dtype=torch.float32)

    @f("m2s::mel_metrics")
    def _mel_metrics(pred, target, mask, group, freq_w, time_w, coeffs, bands, mean, std, n_mfcc, acc):
        return (pred.new_empty((acc.shape[0],), dtype=torch.float32),
                pred.new_empty((pred.shape[0], 3), dtype=torch.float32))

    @f("m2s::hifigan_forward_chunk")
    def _hifigan_chunk(handle, mel, lengths, context, hold, hop):
        return mel.new_empty(((mel.shape[0] - sum(context) - sum(hold)) * hop,), dtype=torch.float32)

    @f("m2s::mel_spectrogram")
    def _melspec(handle, wav, layout):
        n_fft, hop, pad, nm = melspec_geometry(handle)
        t = (wav.shape[1] + 2 * pad - n_fft) // hop + 1  # shape arithmetic only: stays symbolic under tracing
        shape = (wav.shape[0], nm, t) if layout == 0 else (wav.shape[0], t, nm)
        return wav.new_empty(shape, dtype=torch.float32)

    @f("m2s::preprocess_frames")
    def _pre(frames):
        return frames.new_empty(tuple(frames.shape[:3]), dtype=torch.float32)

    @f("m2s::preprocess_frames_resize")
    def _pre_resize(frames, out_h, out_w, interp, norm):
        return frames.new_empty((frames.shape[0], out_h, out_w), dtype=torch.float32)

    @f("m2s::preprocess_frames_masked")
    def _pre_masked(frames, masks, out_h, out_w, interp, norm):
        return frames.new_empty((masks.shape[0], frames.shape[0], out_h, out_w), dtype=torch.float32)

    @f("m2s::occlusion_reduce")
    def _occlusion(mel, band_mask, masks, normalize, want_per_frame):
        m, t, nb = mel.shape[0] - 1, mel.shape[1], band_mask.shape[0] + 1
        e = lambda *shape: mel.new_empty(shape, dtype=torch.float32)
        h, w = (masks.shape[1], masks.shape[2]) if masks is not None else (0, 0)
        return e(m, nb), e(m if want_per_frame else 0, t, nb), e(nb, h, w)

    @f("m2s::cam_backbone")
    def _cam(handle, frames):
        n, h, w = frames.shape
        maps = [frames.new_empty(feature_shape(n, h, w, k), dtype=torch.float32) for k in (2, 5, 8, 18, 28)]
        return (*maps, frames.new_empty((CAM_BN_STATS,), dtype=torch.float32))

    @f("m2s::bilstm_train_forward")
    def _lstm_fwd(x, weights):
        b, t, hd = x.shape[0], x.shape[1], weights[1].shape[1]
        return (x.new_empty((b, t, hd)), x.new_empty((2, b, t, 4 * hd)), x.new_empty((2, b, t, hd)),
                x.new_empty((2, b, t, hd)))

    @f("m2s::bilstm_train_backward")
    def _lstm_bwd(dy, x, weights, gates, cells, hid):
        return torch.empty_like(x), [torch.empty_like(weights[i]) for i in (0, 1, 2, 4, 5, 6)]

    @f("m2s::gradcam")
    def _gradcam(handle, frames, mean, std, band_mask, frame_idx, reduction, want_dpooled):
        t, h, w = frames.shape
        nb, nm, nf = band_mask.shape[0], band_mask.shape[1], len(frame_idx)
        e = lambda *shape: frames.new_empty(shape, dtype=torch.float32)
        return (e(nb, t, h, w), e(nb, nf, h, w), e(t, nm), e(nb * (1 + nf) if want_dpooled else 0, t, 208),
                e(CAM_BN_STATS))

    @f("m2s::gradcam_cotangents")
    def _gradcam_cot(pred_norm, mean, std, band_mask, frame_idx, reduction):
        return pred_norm.new_empty((band_mask.shape[0] * (1 + len(frame_idx)), *pred_norm.shape), dtype=torch.float32)

    @f("m2s::bilstm_train_backward_multi")
    def _lstm_bwd_multi(dy, weights, gates, cells):
        return dy.new_empty((dy.shape[0], dy.shape[1], weights[0].shape[1]), dtype=torch.float32)

    @f("m2s::cam_heatmap")
    def _heatmap(feats, weights, frame, H, W):
        return feats.new_empty((weights.shape[0], H, W), dtype=torch.float32)

    @f("m2s::linear_forward")
    def _lin(x, weight, bias):
        return x.new_empty((*x.shape[:-1], weight.shape[0]))

    @f("m2s::linear_backward")
    def _lin_bwd(dy, x, weight):
        return torch.empty_like(x), torch.empty_like(weight), weight.new_empty((weight.shape[0],))

    @f("m2s::finetune_step")
    def _ft_step(handle, feats, target, mask, lengths, window):
        return feats.new_empty((len(FINETUNE_SLOTS),), dtype=torch.float32)

    @f("m2s::finetune_forward")
    def _ft_forward(handle, feats, lengths, window, train):
        return feats.new_empty((_pairs(lengths, window), window, target_mels(handle)), dtype=torch.float32)

    def _ft_list(handle, like):
        nm = target_mels(handle)
        shapes = [(2560, 208), (2560, 640), (2560,), (2560,)] * 2 + [(nm, 640), (nm,)]
        return [like.new_empty(s, dtype=torch.float32) for s in shapes]

    @f("m2s::finetune_grads")
    def _ft_grads(handle, like):
        return _ft_list(handle, like)

    @f("m2s::finetune_export")
    def _ft_export(handle, like):
        return (_ft_list(handle, like), _ft_list(handle, like), _ft_list(handle, like),
                like.new_empty((1,), dtype=torch.int64))

    @f("m2s::finetune_import")
    def _ft_import(handle, m, v, step):
        return None

    @f("m2s::gap_forward")
    def _gap(x):
        return x.new_empty((x.shape[0], x.shape[1]))

    @f("m2s::gap_backward")
    def _gap_bwd(dy, h, w):
        return dy.new_empty((dy.shape[0], dy.shape[1], h, w))
