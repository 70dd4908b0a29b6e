"""ctypes binding of libm2s.so (C ABI: include/m2s.h).

The library is built in-tree (``make -C mri-to-speech_amd/csrc``) next to this file.  There
is no fallback: if the library is missing, or no gfx950 device is visible, every entry point
raises ``M2SError``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Tuple

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libm2s.so")

F32, BF16, BF16X3, FP8 = 0, 1, 2, 3
# "bf16x3": split fp32 (hi + lo bf16 pairs, three-term MFMA products), fp32 tolerance;
# "fp8": e4m3 MFMA operands with per-channel weight scales (configs[4]; include/m2s.h)
DTYPES = {"fp32": F32, "float32": F32, "f32": F32, "bf16": BF16, "bfloat16": BF16, "bf16x3": BF16X3,
          "fp8": FP8, "e4m3": FP8}
ELEM_F32, ELEM_I64 = 0, 1
ABI_VERSION = 6  # include/m2s.h M2S_ABI_VERSION
# enum m2s_metrics_slot (include/m2s.h): the slots of m2s_mel_metrics' `acc` / `out`, in order
METRICS_SLOTS = ("loss", "mse", "mae", "delta", "accel", "latest", "band0", "band1", "band2", "band3", "band4", "band5",
                 "band6", "band7", "eval_loss", "eval_mse", "eval_mae", "groups", "mcd_sum", "mcd_count")


class M2SError(RuntimeError):
    pass


class Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("elem", C.c_int), ("ndim", C.c_int),
                ("shape", C.c_int64 * 4)]


class HifiganH(C.Structure):
    _fields_ = [("resblock", C.c_int), ("num_mels", C.c_int), ("upsample_initial_channel", C.c_int),
                ("n_up", C.c_int), ("upsample_rates", C.c_int * 8), ("upsample_kernel_sizes", C.c_int * 8),
                ("n_kernels", C.c_int), ("resblock_kernel_sizes", C.c_int * 8), ("n_dilations", C.c_int * 8),
                ("resblock_dilation_sizes", (C.c_int * 8) * 8)]


class MelspecCfg(C.Structure):
    _fields_ = [("n_fft", C.c_int), ("hop", C.c_int), ("win", C.c_int), ("n_mels", C.c_int), ("pad", C.c_int),
                ("power", C.c_int), ("out", C.c_int), ("preemph", C.c_float)]


class FinetuneHyper(C.Structure):
    _fields_ = [("lr", C.c_float), ("weight_decay", C.c_float), ("max_norm", C.c_float), ("dropout", C.c_float),
                ("seed", C.c_uint), ("delta_coeff", C.c_float), ("accel_coeff", C.c_float), ("latest_coeff", C.c_float)]


class ProfStat(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


class ProfLaunch(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("stage", C.c_char * 24), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double), ("spill_bytes", C.c_double)]


_lib = None


def lib():
    """Load libm2s.so once; raise loudly if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise M2SError(f"libm2s.so not found at {LIB_PATH}; build it with `make -C mri-to-speech_amd/csrc` "
                       "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i, sz, fp = C.c_void_p, C.c_int, C.c_size_t, C.c_void_p
    sig = {
        "m2s_abi_version": (i, []),
        "m2s_last_error": (C.c_char_p, []),
        "m2s_device_check": (i, [i]),
        "m2s_acoustic_create": (i, [C.POINTER(Tensor), i, i, i, i, i, C.POINTER(vp)]),
        "m2s_acoustic_destroy": (None, [vp]),
        "m2s_acoustic_set_chunk": (i, [vp, i]),
        "m2s_acoustic_status": (i, [vp]),
        "m2s_acoustic_set_lstm_spin_limit": (i, [vp, C.c_uint]),
        "m2s_acoustic_set_ws_spin_limit": (i, [vp, C.c_uint]),
        "m2s_acoustic_workspace_bytes": (sz, [vp, i, i, i, i]),
        "m2s_acoustic_forward": (i, [vp, fp, i, i, i, i, fp, vp, sz, vp]),
        "m2s_effnet_forward": (i, [vp, fp, i, i, i, fp, vp, sz, vp]),
        "m2s_effnet_probe": (i, [vp, fp, i, i, i, i, fp, C.POINTER(i), C.POINTER(i), C.POINTER(i), vp, sz, vp]),
        "m2s_bilstm_summerge": (i, [vp, fp, i, i, fp, fp, vp, sz, vp]),
        "m2s_mel_glue": (i, [fp, i, i, fp, fp, fp, fp, vp]),
        "m2s_preprocess_frames": (i, [fp, i, i, i, i, fp, vp]),
        "m2s_preprocess_frames_resize": (i, [fp, i, i, i, i, i, i, i, i, fp, vp]),
        # occlusion: masks / mel / band_mask and every output are device pointers
        "m2s_preprocess_frames_masked": (i, [fp, i, i, i, i, fp, i, i, i, i, i, fp, vp]),
        "m2s_occlusion_reduce": (i, [fp, i, i, i, fp, i, fp, i, i, i, fp, fp, fp, vp]),
        "m2s_vocoder_create": (i, [C.POINTER(Tensor), i, C.POINTER(HifiganH), i, i, C.POINTER(vp)]),
        "m2s_vocoder_destroy": (None, [vp]),
        "m2s_vocoder_workspace_bytes": (sz, [vp, i, i]),
        "m2s_vocoder_forward": (i, [vp, fp, i, i, i, fp, vp, sz, vp]),
        "m2s_vocoder_probe": (i, [vp, fp, i, i, i, i, fp, C.POINTER(i), C.POINTER(i), C.POINTER(i), vp, sz, vp]),
        "m2s_vocoder_tap_info": (i, [vp, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "m2s_pipeline_workspace_bytes": (sz, [vp, vp, i, i, i, i]),
        "m2s_pipeline_forward": (i, [vp, vp, fp, i, i, i, i, fp, fp, fp, fp, fp, fp, vp, sz, vp]),
        # ragged batches: `lengths` is a host int array (C.POINTER(c_int)), rows = sum(lengths)
        "m2s_acoustic_ragged_workspace_bytes": (sz, [vp, C.POINTER(i), i, i, i]),
        "m2s_bilstm_summerge_ragged": (i, [vp, fp, C.POINTER(i), i, i, fp, fp, vp, sz, vp]),
        "m2s_acoustic_forward_ragged": (i, [vp, fp, C.POINTER(i), i, i, i, i, fp, vp, sz, vp]),
        "m2s_vocoder_ragged_workspace_bytes": (sz, [vp, C.POINTER(i), i]),
        "m2s_vocoder_forward_ragged": (i, [vp, fp, C.POINTER(i), i, i, fp, vp, sz, vp]),
        # streaming vocoder: `context` / `hold` are host int arrays like `lengths`
        "m2s_vocoder_reach": (i, [vp, C.POINTER(i), C.POINTER(i)]),
        "m2s_vocoder_set_chunk_cone": (i, [vp, i]),
        "m2s_vocoder_chunk_workspace_bytes": (sz, [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), i]),
        "m2s_vocoder_forward_chunk": (i, [vp, fp, C.POINTER(i), C.POINTER(i), C.POINTER(i), i, i, fp, vp, sz, vp]),
        "m2s_pipeline_ragged_workspace_bytes": (sz, [vp, vp, C.POINTER(i), i, i, i]),
        "m2s_pipeline_forward_ragged": (i, [vp, vp, fp, C.POINTER(i), i, i, i, i, fp, fp, fp, fp, fp, fp, vp, sz, vp]),
        # windowed inference: `context` is a host int array like `lengths`, or NULL
        "m2s_acoustic_windowed_workspace_bytes": (sz, [vp, C.POINTER(i), C.POINTER(i), i, i, i, i, i]),
        "m2s_bilstm_windowed": (i, [vp, fp, C.POINTER(i), C.POINTER(i), i, i, i, i, fp, fp, vp, sz, vp]),
        "m2s_acoustic_forward_windowed": (i, [vp, fp, C.POINTER(i), C.POINTER(i), i, i, i, i, i, i, fp, vp, sz, vp]),
        # pair outputs (every row of every training window) and the fused validation metrics; `bands` is a host array
        "m2s_acoustic_pairs_workspace_bytes": (sz, [vp, C.POINTER(i), i, i, i, i]),
        "m2s_bilstm_pairs": (i, [vp, fp, C.POINTER(i), i, i, i, fp, fp, vp, sz, vp]),
        "m2s_acoustic_forward_pairs": (i, [vp, fp, C.POINTER(i), i, i, i, i, i, fp, vp, sz, vp]),
        "m2s_mel_metrics_workspace_bytes": (sz, [i]),
        "m2s_mel_metrics": (i, [fp, fp, fp, i, i, i, i, fp, fp, C.c_float, C.c_float, C.c_float, C.POINTER(i), i, fp, fp,
                                i, fp, fp, fp, vp, sz, vp]),
        "m2s_cam_create": (i, [C.POINTER(Tensor), i, i, C.POINTER(vp)]),
        "m2s_cam_destroy": (None, [vp]),
        "m2s_cam_bn_layers": (i, [vp]),
        "m2s_cam_bn_channels": (i, [vp, i]),
        "m2s_cam_workspace_bytes": (sz, [vp, i, i, i]),
        "m2s_cam_backbone": (i, [vp, fp, i, i, i, vp, fp, vp, sz, vp]),
        "m2s_bilstm_train_workspace_bytes": (sz, [i, i, i, i]),
        "m2s_bilstm_train_forward": (i, [fp, i, i, i, i, vp, fp, fp, fp, fp, vp, sz, vp]),
        "m2s_bilstm_train_backward": (i, [fp, fp, i, i, i, i, vp, fp, fp, fp, fp, vp, vp, sz, vp]),
        # Grad-CAM engine: band_mask / frame_idx of m2s_gradcam_forward are host arrays, the stage calls take
        # device pointers throughout
        "m2s_gradcam_create": (i, [C.POINTER(Tensor), i, i, C.POINTER(vp)]),
        "m2s_gradcam_destroy": (None, [vp]),
        "m2s_gradcam_n_mels": (i, [vp]),
        "m2s_gradcam_bn_stats_floats": (i, [vp]),
        "m2s_gradcam_chunk": (i, []),
        "m2s_gradcam_workspace_bytes": (sz, [vp, i, i, i, i, i]),
        "m2s_gradcam_forward": (i, [vp, fp, i, i, i, fp, fp, C.POINTER(C.c_float), i, C.POINTER(i), i, i, fp, fp, fp,
                                    fp, fp, vp, sz, vp]),
        "m2s_gradcam_cotangents": (i, [fp, i, i, fp, fp, fp, i, vp, i, i, fp, vp]),
        "m2s_bilstm_train_backward_multi_workspace_bytes": (sz, [i, i, i, i]),
        "m2s_bilstm_train_backward_multi": (i, [fp, i, i, i, i, vp, fp, fp, fp, vp, sz, vp]),
        "m2s_cam_heatmap": (i, [fp, i, i, i, i, fp, vp, i, i, i, fp, vp]),
        "m2s_linear_forward": (i, [fp, i, i, i, fp, fp, fp, vp]),
        "m2s_linear_backward": (i, [fp, fp, i, i, i, fp, fp, fp, fp, vp]),
        "m2s_gap_forward": (i, [fp, C.c_int64, i, fp, vp]),
        "m2s_gap_backward": (i, [fp, C.c_int64, i, fp, vp]),
        "m2s_melspec_create": (i, [C.POINTER(MelspecCfg), fp, i, C.POINTER(vp)]),
        "m2s_melspec_destroy": (None, [vp]),
        "m2s_melspec_n_mels": (i, [vp]),
        "m2s_melspec_frames": (i, [vp, i]),
        "m2s_melspec_workspace_bytes": (sz, [vp, i, i]),
        "m2s_melspec_forward": (i, [vp, fp, i, i, fp, i, vp, sz, vp]),
        # fine-tuning engine: `lengths`, the hyper struct, freq_w and time_w are host memory; grads10 / params10 / m10 /
        # v10 are host arrays of 10 device pointers
        "m2s_finetune_create": (i, [C.POINTER(Tensor), i, i, i, C.POINTER(vp)]),
        "m2s_finetune_destroy": (None, [vp]),
        "m2s_finetune_n_mels": (i, [vp]),
        "m2s_finetune_set_hyper": (i, [vp, C.POINTER(FinetuneHyper), C.POINTER(C.c_float), C.POINTER(C.c_float), i, vp]),
        "m2s_finetune_workspace_bytes": (sz, [vp, C.POINTER(i), i, i]),
        "m2s_finetune_step": (i, [vp, fp, fp, fp, C.POINTER(i), i, i, i, fp, vp, sz, vp]),
        "m2s_finetune_forward": (i, [vp, fp, C.POINTER(i), i, i, i, i, fp, vp, sz, vp]),
        "m2s_finetune_grads": (i, [vp, C.POINTER(vp), vp]),
        "m2s_finetune_export": (i, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]),
        "m2s_finetune_import_moments": (i, [vp, C.POINTER(vp), C.POINTER(vp), vp, vp]),
        "m2s_prof_enable": (i, [i]),
        "m2s_prof_collect": (i, [C.POINTER(ProfStat), i, C.POINTER(i)]),
        "m2s_prof_launches": (i, [C.POINTER(ProfLaunch), i, C.POINTER(i)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.m2s_abi_version() != ABI_VERSION:
        raise M2SError("libm2s ABI version mismatch")
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().m2s_last_error().decode(errors="replace")
        raise M2SError(f"libm2s error {rc}: {msg}")


def exported_symbols() -> List[str]:
    return [n for n in ("m2s_abi_version", "m2s_last_error", "m2s_device_check", "m2s_acoustic_create",
                        "m2s_acoustic_destroy", "m2s_acoustic_set_chunk", "m2s_acoustic_status",
                        "m2s_acoustic_set_lstm_spin_limit", "m2s_acoustic_set_ws_spin_limit", "m2s_acoustic_workspace_bytes",
                        "m2s_acoustic_forward", "m2s_effnet_forward", "m2s_effnet_probe", "m2s_bilstm_summerge",
                        "m2s_mel_glue", "m2s_preprocess_frames", "m2s_preprocess_frames_resize", "m2s_preprocess_frames_masked",
                        "m2s_occlusion_reduce", "m2s_vocoder_create",
                        "m2s_vocoder_destroy",
                        "m2s_vocoder_workspace_bytes", "m2s_vocoder_forward", "m2s_vocoder_probe",
                        "m2s_vocoder_tap_info", "m2s_pipeline_workspace_bytes",
                        "m2s_pipeline_forward", "m2s_acoustic_ragged_workspace_bytes", "m2s_bilstm_summerge_ragged",
                        "m2s_acoustic_forward_ragged", "m2s_vocoder_ragged_workspace_bytes",
                        "m2s_vocoder_forward_ragged", "m2s_pipeline_ragged_workspace_bytes",
                        "m2s_pipeline_forward_ragged", "m2s_acoustic_windowed_workspace_bytes", "m2s_bilstm_windowed",
                        "m2s_acoustic_forward_windowed", "m2s_acoustic_pairs_workspace_bytes", "m2s_bilstm_pairs",
                        "m2s_acoustic_forward_pairs", "m2s_mel_metrics_workspace_bytes", "m2s_mel_metrics",
                        "m2s_vocoder_reach", "m2s_vocoder_set_chunk_cone",
                        "m2s_vocoder_chunk_workspace_bytes", "m2s_vocoder_forward_chunk", "m2s_cam_create",
                        "m2s_cam_destroy", "m2s_cam_bn_layers",
                        "m2s_cam_bn_channels", "m2s_cam_workspace_bytes", "m2s_cam_backbone",
                        "m2s_bilstm_train_workspace_bytes", "m2s_bilstm_train_forward", "m2s_bilstm_train_backward",
                        "m2s_gradcam_create", "m2s_gradcam_destroy", "m2s_gradcam_n_mels", "m2s_gradcam_bn_stats_floats",
                        "m2s_gradcam_chunk",
                        "m2s_gradcam_workspace_bytes", "m2s_gradcam_forward", "m2s_gradcam_cotangents",
                        "m2s_bilstm_train_backward_multi_workspace_bytes", "m2s_bilstm_train_backward_multi",
                        "m2s_cam_heatmap",
                        "m2s_linear_forward", "m2s_linear_backward", "m2s_gap_forward", "m2s_gap_backward",
                        "m2s_melspec_create", "m2s_melspec_destroy", "m2s_melspec_n_mels", "m2s_melspec_frames",
                        "m2s_melspec_workspace_bytes", "m2s_melspec_forward",
                        "m2s_finetune_create", "m2s_finetune_destroy", "m2s_finetune_n_mels", "m2s_finetune_set_hyper",
                        "m2s_finetune_workspace_bytes", "m2s_finetune_step", "m2s_finetune_forward", "m2s_finetune_grads",
                        "m2s_finetune_export", "m2s_finetune_import_moments",
                        "m2s_prof_enable", "m2s_prof_collect", "m2s_prof_launches")]


def tensor_array(state: Dict[str, "np.ndarray"]) -> Tuple[C.Array, list]:
    """Reference-format state dict (numpy / CPU torch) -> m2s_tensor[] plus the keep-alive list."""
    keep, items = [], []
    for k, v in state.items():
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if a.dtype == np.int64:
            elem = ELEM_I64
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            elem = ELEM_F32
        a = np.ascontiguousarray(a)
        if a.ndim > 4:
            raise M2SError(f"{k}: rank {a.ndim} > 4")
        name = k.encode()
        keep += [a, name]
        shape = (C.c_int64 * 4)(*(list(a.shape) + [0] * (4 - a.ndim)))
        items.append(Tensor(name, a.ctypes.data, elem, a.ndim, shape))
    arr = (Tensor * len(items))(*items)
    return arr, keep


def hifigan_h(h) -> HifiganH:
    s = HifiganH()
    rb = str(h["resblock"])
    if rb not in ("1", "2"):
        raise M2SError(f"unsupported resblock type {rb!r}")
    s.resblock = int(rb)
    s.num_mels = int(h["num_mels"])
    s.upsample_initial_channel = int(h["upsample_initial_channel"])
    ur, uk = list(h["upsample_rates"]), list(h["upsample_kernel_sizes"])
    rk, rd = list(h["resblock_kernel_sizes"]), list(h["resblock_dilation_sizes"])
    if len(ur) != len(uk) or len(rk) != len(rd) or not (1 <= len(ur) <= 8) or not (1 <= len(rk) <= 8):
        raise M2SError("inconsistent generator config")
    s.n_up = len(ur)
    for i, (u, k) in enumerate(zip(ur, uk)):
        s.upsample_rates[i], s.upsample_kernel_sizes[i] = int(u), int(k)
    s.n_kernels = len(rk)
    for j, (k, d) in enumerate(zip(rk, rd)):
        s.resblock_kernel_sizes[j] = int(k)
        s.n_dilations[j] = len(d)
        for q, dd in enumerate(d):
            s.resblock_dilation_sizes[j][q] = int(dd)
    return s


def prof_enable(on: bool) -> None:
    check(lib().m2s_prof_enable(1 if on else 0))


def prof_launches() -> List[dict]:
    """Every launch recorded since prof_enable(True), in launch order: name, stage, ms, flops, bytes
    (m2s_prof_launches); clears the record."""
    n = C.c_int(0)
    check(lib().m2s_prof_launches(None, 0, C.byref(n)))  # count only (records kept)
    cap = max(n.value, 1)
    buf = (ProfLaunch * cap)()
    check(lib().m2s_prof_launches(buf, cap, C.byref(n)))
    return [dict(name=buf[i].name.decode(), stage=buf[i].stage.decode(), ms=buf[i].ms, flops=buf[i].flops,
                 bytes=buf[i].bytes, spill_bytes=buf[i].spill_bytes) for i in range(min(n.value, cap))]


def aggregate(launches: List[dict], key: str = "name") -> List[dict]:
    """Per-kernel (key="name") or per-stage (key="stage") sums of prof_launches() records."""
    agg: Dict[str, dict] = {}
    for r in launches:
        a = agg.setdefault(r[key], dict(name=r[key], launches=0, ms=0.0, flops=0.0, bytes=0.0, spill_bytes=0.0))
        a["launches"] += 1
        for f in ("ms", "flops", "bytes", "spill_bytes"):
            a[f] += r.get(f, 0.0)
    return list(agg.values())


def prof_collect() -> List[dict]:
    """Per-kernel sums of the recorded launches (name, launches, ms, flops, bytes); clears the record."""
    return aggregate(prof_launches(), "name")
